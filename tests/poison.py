"""Adversarial memory contents for the library's own allocations.

Every buffer the package writes into is a ``torch.empty`` tensor from the
caching allocator: in a test it is driver-zeroed or holds the leftovers of an
identical earlier call, and other live tensors sit right behind it. Inside
``poisoned(pkg, fill)`` every ``torch.empty`` / ``torch.empty_like`` issued
from the package's modules (fused, network, train_ops, model) instead returns
a tensor placed in the middle of a larger uint8 backing tensor that is filled
entirely with the byte ``fill``: the buffer starts out as ``fill`` (a read
before write sees it) and has GUARD bytes of ``fill`` before and after it (a
write past either end changes them). ``guarded(t, fill)`` places a test input
the same way and remembers its bytes. ``check_guards()`` asserts that no guard
byte changed, ``check_inputs()`` that no read-only input did.

The fills: 0xFF is NaN as fp32 / fp64 / bf16 / fp16, 0xFFFFFFFF for a "largest
word wins" maximum and -1 as an integer; 0x4B is finite (fp32 1.33e7, fp64
1e55), so fmax, ReLU and comparisons do not swallow it the way they swallow a
NaN; 0x00 is the clean run.

Only the name ``torch`` in those modules' namespaces is replaced, by a proxy
that forwards everything but the two functions; ``torch`` itself is untouched.
"""
import contextlib
import math
import os
import sys

import torch

GUARD = 64 * 1024   # bytes of fill before and after every buffer
ALIGN = 256         # buffers start at this alignment (the library asks for 16), plus ``skew``
MODULES = ("fused", "network", "train_ops", "model")
FILLS = (0x00, 0xFF, 0x4B)

_RECORD = []


class Allocation:
    """One guarded buffer: ``tensor`` lives at ``backing[offset : offset + nbytes]``."""

    def __init__(self, order, kind, name, backing, offset, tensor, fill, site):
        self.order, self.kind, self.name = order, kind, name
        self.site = site        # (file name, line, function) of the call that allocated it
        self.backing, self.offset, self.tensor, self.fill = backing, offset, tensor, fill
        self.shape, self.dtype = tuple(tensor.shape), tensor.dtype
        self.nbytes = tensor.numel() * tensor.element_size()
        self.snapshot = None    # the bytes a read-only input went in with (CPU)

    def describe(self):
        what = f"{self.kind} #{self.order}" + (f" '{self.name}'" if self.name else "")
        return (f"{what}: shape {self.shape} dtype {self.dtype} nbytes {self.nbytes} "
                f"on {self.backing.device}, allocated at {self.site[0]}:{self.site[1]} "
                f"({self.site[2]})")

    def view_bytes(self):
        return self.backing[self.offset:self.offset + self.nbytes]

    def guards(self):
        return self.backing[:self.offset], self.backing[self.offset + self.nbytes:]


def _call_site():
    """The first frame outside this module: who asked for the buffer."""
    here = sys._getframe(0).f_code.co_filename
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename == here:
        f = f.f_back
    if f is None:
        return ("?", 0, "?")
    return (os.path.basename(f.f_code.co_filename), f.f_lineno, f.f_code.co_name)


def _alloc(shape, dtype, device, fill, kind, name=None, skew=0):
    """skew: bytes the buffer starts past its ALIGN boundary (a multiple of the
    element size below ALIGN), as a view into a flat bucket or a slice of a batch
    does; both guard bands keep at least GUARD bytes."""
    shape = tuple(int(s) for s in shape)
    item = torch.empty((), dtype=dtype).element_size()
    assert 0 <= skew < ALIGN and skew % item == 0, (skew, item)
    nbytes = math.prod(shape) * item
    backing = torch.full((nbytes + 2 * GUARD + 2 * ALIGN,), fill, dtype=torch.uint8,
                         device=device)
    offset = GUARD + (-(backing.data_ptr() + GUARD)) % ALIGN + skew
    strides, acc = [], 1
    for s in reversed(shape):
        strides.append(acc)
        acc *= max(s, 1)
    # (set_ on the storage, not a view of ``backing``: the tensor has a version
    # counter and an autograd identity of its own, like a fresh torch.empty)
    t = torch.empty(0, dtype=dtype, device=device).set_(
        backing.untyped_storage(), (backing.storage_offset() + offset) // item, shape,
        tuple(reversed(strides)))
    assert nbytes == 0 or (t.data_ptr() == backing.data_ptr() + offset
                           and t.data_ptr() % ALIGN == skew)
    a = Allocation(len(_RECORD), kind, name, backing, offset, t, fill, _call_site())
    _RECORD.append(a)
    return a


def _size_of(args, kwargs):
    """torch.empty's size: ints, one tuple / list / torch.Size, or size=..."""
    if "size" in kwargs:
        return tuple(kwargs.pop("size")), args
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(args[0]), ()
    return tuple(args), ()


class TorchProxy:
    """Stands in for the ``torch`` module in a package module's namespace."""

    def __init__(self, fill, device_type):
        self._fill, self._device_type = fill, device_type

    def __getattr__(self, name):
        return getattr(torch, name)

    def _ours(self, device, kwargs):
        if kwargs.get("pin_memory") or kwargs.get("layout", torch.strided) != torch.strided:
            return False
        device = torch.device(device) if device is not None else torch.empty(0).device
        return device.type == self._device_type

    def empty(self, *args, **kwargs):
        if not self._ours(kwargs.get("device"), kwargs) or "out" in kwargs:
            return torch.empty(*args, **kwargs)
        kw = dict(kwargs)
        size, rest = _size_of(args, kw)
        assert not rest and not (set(kw) - {"device", "dtype", "requires_grad", "pin_memory",
                                            "layout", "memory_format"}), (args, kwargs)
        dtype = kw.get("dtype") or torch.get_default_dtype()
        device = kw.get("device")
        t = _alloc(size, dtype, device if device is not None else "cpu", self._fill, "empty").tensor
        return t.requires_grad_(True) if kw.get("requires_grad") else t

    def empty_like(self, t, **kwargs):
        device = kwargs.get("device", t.device)
        if not self._ours(device, kwargs) or t.is_sparse:
            return torch.empty_like(t, **kwargs)
        # (dense and contiguous whatever t's strides: what the package's callers
        # get from empty_like of a contiguous tensor, and the dense tensor of that
        # shape for an expanded, stride-0 placeholder)
        return _alloc(t.shape, kwargs.get("dtype") or t.dtype, device, self._fill,
                      "empty_like").tensor


@contextlib.contextmanager
def poisoned(pkg, fill, device_type="cuda"):
    """Within the context the package's own torch.empty / torch.empty_like on
    ``device_type`` come back filled with ``fill`` and guard-banded; host
    allocations (pinned, or another device type) pass through. Starts a fresh
    record; the record stays readable after the context exits."""
    assert 0 <= fill <= 0xFF
    del _RECORD[:]
    proxy = TorchProxy(fill, device_type)
    mods = [getattr(pkg, m) for m in MODULES]
    for m in mods:
        assert m.torch is torch, f"{m.__name__} is already poisoned"
    try:
        for m in mods:
            m.torch = proxy
        yield proxy
    finally:
        for m in mods:
            m.torch = torch


def guarded(t, fill, device="cuda:0", name=None, readonly=True, skew=0):
    """A copy of the test input ``t`` on ``device`` inside a guarded backing
    filled with ``fill`` (same dtype and shape, contiguous). readonly: its bytes
    are remembered and ``check_inputs()`` requires them unchanged. skew: the
    copy starts that many bytes past a 256-byte boundary (``_alloc``)."""
    src = t.detach().contiguous()
    a = _alloc(src.shape, src.dtype, device, fill, "input", name, skew=skew)
    a.tensor.copy_(src)
    if readonly:
        a.snapshot = a.view_bytes().cpu().clone()
    return a.tensor


def empty(size, fill, dtype=torch.float32, device="cuda:0", name=None):
    """A guarded, ``fill``-filled buffer for an allocation the test itself makes
    on the library's behalf (e.g. a stgcn_fold_prep buffer)."""
    size = (size,) if isinstance(size, int) else tuple(size)
    return _alloc(size, dtype, device, fill, "empty", name).tensor


def allocations():
    """The record since the last ``poisoned`` began, in allocation order."""
    return list(_RECORD)


def _dirty(a):
    pre, post = a.guards()
    return torch.stack([(pre != a.fill).any(), (post != a.fill).any()])


def check_guards():
    """Every guard byte of every recorded backing still equals its fill."""
    if not _RECORD:
        return
    by_dev = {}
    for a in _RECORD:
        by_dev.setdefault(a.backing.device, []).append(_dirty(a))
    if not any(bool(torch.stack(v).any().item()) for v in by_dev.values()):
        return
    bad = []
    for a in _RECORD:
        for side, g in zip(("before", "after"), a.guards()):
            idx = (g != a.fill).nonzero().flatten()
            if idx.numel():
                first, last = int(idx[0]), int(idx[-1])
                where = (f"{a.offset - last} .. {a.offset - first} bytes before its start"
                         if side == "before" else
                         f"{first} .. {last} bytes past its end")
                bad.append(f"{a.describe()}: {idx.numel()} guard bytes overwritten, {where}")
    raise AssertionError("guard band overrun -- " + "; ".join(bad))


def check_inputs():
    """Every read-only guarded input is bit-identical to what went in."""
    bad = [a.describe() for a in _RECORD
           if a.snapshot is not None and not torch.equal(a.view_bytes().cpu(), a.snapshot)]
    assert not bad, "read-only input modified -- " + "; ".join(bad)


def resnapshot():
    """Re-reads the bytes of the read-only inputs (after a legitimate update,
    e.g. the optimizer's step on guarded parameters)."""
    for a in _RECORD:
        if a.snapshot is not None:
            a.snapshot = a.view_bytes().cpu().clone()
