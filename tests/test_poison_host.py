"""The poison helper (tests/poison.py) itself, on CPU tensors: what the GPU
module (test_gpu_poison.py) relies on when it reads a green check_guards()."""
import pytest
import torch

import poison


@pytest.fixture(params=[0xFF, 0x4B, 0x00])
def cpu_poison(pkg, request):
    with poison.poisoned(pkg, request.param, device_type="cpu") as proxy:
        yield pkg, proxy, request.param


def test_fresh_empty_shows_the_fill(cpu_poison):
    pkg, proxy, fill = cpu_poison
    assert pkg.fused.torch is proxy and pkg.train_ops.torch is proxy
    assert pkg.network.torch is proxy and pkg.model.torch is proxy
    a = pkg.fused.torch.empty(3, 5, dtype=torch.float32)
    b = pkg.fused.torch.empty((2, 7), device="cpu", dtype=torch.float64)
    c = pkg.train_ops.torch.empty((), dtype=torch.float32)
    d = pkg.network.torch.empty(size=(6,), dtype=torch.int64)
    e = pkg.fused.torch.empty(11, dtype=torch.uint8)
    z = pkg.fused.torch.empty(0, dtype=torch.float32)
    for t, shape in ((a, (3, 5)), (b, (2, 7)), (c, ()), (d, (6,)), (e, (11,)), (z, (0,))):
        assert tuple(t.shape) == shape and t.is_contiguous()
        assert t.data_ptr() % poison.ALIGN == 0
        assert (t.view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)
                ).eq(fill).all()
    if fill == 0xFF:
        assert a.isnan().all() and b.isnan().all() and (d == -1).all()
        assert (a.view(torch.int32) == -1).all()    # 0xFFFFFFFF: beats every amax word
    if fill == 0x4B:
        assert torch.isfinite(a).all() and (a > 1e7).all() and (b > 1e54).all()
    rec = poison.allocations()
    assert [r.order for r in rec] == list(range(6))
    assert all(r.site[0] == "test_poison_host.py" and r.site[1] > 0
               and r.site[2] == "test_fresh_empty_shows_the_fill" for r in rec)
    assert "allocated at test_poison_host.py:" in rec[0].describe()
    assert [r.nbytes for r in rec] == [60, 112, 4, 48, 11, 0]
    assert rec[1].dtype == torch.float64 and rec[1].shape == (2, 7)
    for r in rec:
        pre, post = r.guards()
        assert pre.numel() >= poison.GUARD and post.numel() >= poison.GUARD
    poison.check_guards()


def test_empty_like_of_expanded_placeholder_is_dense(cpu_poison):
    pkg, proxy, fill = cpu_poison
    ph = pkg.fused.torch.empty(1, dtype=torch.float32).expand(2, 3, 4, 5)
    assert ph.stride() == (0, 0, 0, 0)
    t = pkg.fused.torch.empty_like(ph)
    assert t.shape == ph.shape and t.stride() == (60, 20, 5, 1) and t.dtype == torch.float32
    assert t.view(torch.uint8).eq(fill).all()
    p = torch.nn.Parameter(torch.zeros(3, 2))
    u = pkg.fused.torch.empty_like(p)
    assert type(u) is torch.Tensor and u.shape == (3, 2) and not u.requires_grad
    assert poison.allocations()[-1].kind == "empty_like"
    # a tensor of its own, not a view of the backing: its own version counter
    v0, b0 = u._version, poison.allocations()[-1].backing._version
    u.add_(1)
    assert u._version == v0 + 1 and poison.allocations()[-1].backing._version == b0
    assert not u._is_view()


@pytest.mark.parametrize("where", ["after", "before", "after_far", "before_far"])
def test_write_outside_the_view_is_caught_and_named(cpu_poison, where):
    pkg, proxy, fill = cpu_poison
    pkg.fused.torch.empty(8, dtype=torch.float32)
    t = pkg.fused.torch.empty((5, 3), dtype=torch.float32)
    pkg.fused.torch.empty(8, dtype=torch.float32)
    a = poison.allocations()[1]
    assert a.tensor is t
    pos = {"after": a.offset + a.nbytes, "before": a.offset - 1,
           "after_far": a.offset + a.nbytes + poison.GUARD - 1,
           "before_far": a.offset - poison.GUARD}[where]
    a.backing[pos] = fill ^ 0x01
    with pytest.raises(AssertionError) as ei:
        poison.check_guards()
    msg = str(ei.value)
    assert "#1" in msg and "(5, 3)" in msg and "torch.float32" in msg and "nbytes 60" in msg
    assert "#0" not in msg and "#2" not in msg
    assert ("past its end" in msg) == where.startswith("after")
    a.backing[pos] = fill
    poison.check_guards()


def test_write_inside_the_view_passes(cpu_poison):
    pkg, proxy, fill = cpu_poison
    t = pkg.fused.torch.empty((5, 3), dtype=torch.float32)
    t.fill_(1.5)
    t.view(-1)[0] = -2.0
    t.view(-1)[-1] = 7.0
    poison.check_guards()
    a = poison.allocations()[0]
    assert a.view_bytes().view(torch.float32)[-1] == 7.0  # the record sees the same bytes


def test_guarded_inputs(cpu_poison):
    pkg, proxy, fill = cpu_poison
    src = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4).transpose(1, 2)
    lab = torch.tensor([3, 1, 4], dtype=torch.int64)
    g = poison.guarded(src, fill, device="cpu", name="x")
    gl = poison.guarded(lab, fill, device="cpu", name="labels")
    rs = poison.guarded(torch.ones(4), fill, device="cpu", name="running_mean", readonly=False)
    assert torch.equal(g, src) and g.is_contiguous() and g.data_ptr() % poison.ALIGN == 0
    assert torch.equal(gl, lab) and gl.dtype == torch.int64
    assert not g.requires_grad and g.requires_grad_(True).is_leaf
    poison.check_inputs()
    poison.check_guards()
    rs.mul_(0.9)             # in/out: exempt
    poison.check_inputs()
    with torch.no_grad():
        g[1, 2, 0] += 1.0
    with pytest.raises(AssertionError, match=r"'x'.*\(2, 4, 3\)"):
        poison.check_inputs()
    poison.resnapshot()
    poison.check_inputs()
    a = [r for r in poison.allocations() if r.name == "labels"][0]
    a.backing[a.offset + a.nbytes] = fill ^ 0x80
    with pytest.raises(AssertionError, match=r"input #1 'labels'.*past its end"):
        poison.check_guards()


def test_host_allocations_pass_through(pkg):
    """In the GPU module's mode (device_type "cuda") CPU and pinned allocations
    go to torch untouched and are not recorded."""
    with poison.poisoned(pkg, 0xFF) as proxy:
        t = pkg.train_ops.torch.empty(16, dtype=torch.uint8)
        u = pkg.train_ops.torch.empty((2, 2), device="cpu")
        v = pkg.fused.torch.empty_like(torch.zeros(3))
        assert t.shape == (16,) and u.shape == (2, 2) and v.shape == (3,)
        if torch.cuda.is_available():
            p = pkg.train_ops.torch.empty(16, dtype=torch.uint8, pin_memory=True)
            assert p.is_pinned() and p.device.type == "cpu" and p.shape == (16,)
        else:
            # no accelerator: torch refuses a pinned allocation, and the proxy's
            # call must end in that very refusal, raised from its hand-over to torch
            with pytest.raises(RuntimeError) as real:
                torch.empty(16, dtype=torch.uint8, pin_memory=True)
            with pytest.raises(RuntimeError) as ours:
                pkg.train_ops.torch.empty(16, dtype=torch.uint8, pin_memory=True)
            assert str(ours.value) == str(real.value)
            last = ours.traceback[-1]
            assert last.name == "empty" and str(last.path).endswith("poison.py")
            assert "return torch.empty(*args, **kwargs)" in str(last.statement)
        assert poison.allocations() == []
        # everything else is torch's own
        assert pkg.fused.torch.float32 is torch.float32
        assert pkg.fused.torch.zeros is torch.zeros and pkg.fused.torch.autograd is torch.autograd
    poison.check_guards()


def test_proxy_is_gone_after_the_context(pkg):
    with poison.poisoned(pkg, 0x4B, device_type="cpu"):
        assert pkg.fused.torch is not torch
        pkg.fused.torch.empty(4)
    for m in poison.MODULES:
        assert getattr(pkg, m).torch is torch
    with pytest.raises(RuntimeError, match="boom"):
        with poison.poisoned(pkg, 0x4B, device_type="cpu"):
            raise RuntimeError("boom")
    for m in poison.MODULES:
        assert getattr(pkg, m).torch is torch
    import torch as real
    assert real.empty is torch.empty and not isinstance(real, poison.TorchProxy)
    # the record outlives the context (read after the run), and a new context starts afresh
    with poison.poisoned(pkg, 0x00, device_type="cpu"):
        assert poison.allocations() == []


@pytest.mark.parametrize("skew", [0, 4, 8, 12])
def test_skewed_inputs_keep_their_guards(cpu_poison, skew):
    """guarded(..., skew=): the tensor starts ``skew`` bytes past a 256-byte
    boundary (what a view into a flat bucket or x[1:] of an odd-sized batch
    gives), is contiguous, survives the runners' ``.float().contiguous()``
    without a copy, and a write one element before its start or past its end
    still trips the guard check."""
    pkg, proxy, fill = cpu_poison
    src = torch.arange(30, dtype=torch.float32).reshape(2, 3, 5)
    g = poison.guarded(src, fill, device="cpu", name="x", skew=skew)
    assert g.data_ptr() % 16 == skew and g.data_ptr() % poison.ALIGN == skew
    assert g.is_contiguous() and torch.equal(g, src)
    same = g.float().contiguous()
    assert same.data_ptr() == g.data_ptr()
    assert same.untyped_storage().data_ptr() == g.untyped_storage().data_ptr()
    a = poison.allocations()[-1]
    assert a.tensor is g and a.offset % 16 == (skew - a.backing.data_ptr()) % 16
    pre, post = a.guards()
    assert pre.numel() >= poison.GUARD and post.numel() >= poison.GUARD
    assert torch.equal(a.view_bytes().view(torch.float32), src.reshape(-1))
    poison.check_guards()
    poison.check_inputs()
    for pos in (a.offset - 4, a.offset - 1, a.offset + a.nbytes, a.offset + a.nbytes + 3):
        a.backing[pos] = fill ^ 0x01
        with pytest.raises(AssertionError, match="guard band overrun"):
            poison.check_guards()
        a.backing[pos] = fill
        poison.check_guards()
    if skew % 8 == 0:   # int64 labels: multiples of 8 only
        lab = poison.guarded(torch.tensor([3, 1, 4]), fill, device="cpu", name="labels",
                             skew=skew)
        assert lab.dtype == torch.int64 and lab.data_ptr() % 16 == skew
        assert lab.contiguous().data_ptr() == lab.data_ptr()
    else:
        with pytest.raises(AssertionError):
            poison.guarded(torch.tensor([3, 1, 4]), fill, device="cpu", skew=skew)
    with pytest.raises(AssertionError):
        poison.guarded(src, fill, device="cpu", skew=skew + 2)
