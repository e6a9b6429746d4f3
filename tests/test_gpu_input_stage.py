"""The input stage on the GPU (stgcn_input_stage through data.stage_clips and
data.RaggedDeviceLoader): ragged clips -> loop padding, per-clip 2x2 transform,
fp32 cast, NCTV.

Expected values come from the host functions the reference-generated fixtures
pin (tests/test_data_pipeline.py): per clip ``pad_array_with_loops`` to T_out,
times the clip's own matrix in float64 by augment_data's arithmetic
(homogeneous [x, y, 0] rows ``.dot`` the 3x3 matrix), then the transpose.

Gates. Untransformed clips (and channels 2 ..): bit-equal to the host's fp32
cast. Transformed channels, a derived bound: one fp32 rounding of the result
plus the fp64 evaluation error of both sides (each two products and one sum,
|error| <= 2 * 2^-53 * (|x m0j| + |y m1j|) to first order, for the device and
for the reference):

    |dev - ref64| <= 2^-24 |ref64| + 2^-51 (|x m0j| + |y m1j|)
"""
import contextlib
import io
import random

import numpy as np
import pytest
import torch

import poison
from conftest import load_npz, rel_to_max

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = (1, 7, 13)   # single frame, wrap, truncation at T_out = 11
T_OUT = 11
# one general matrix (no zero entry, nothing a power of two) beside the reference's draws
GENERAL = np.array([[0.83, -1.7, 0.0], [2.9, 0.31, 0.0], [5.0, 5.0, 1.0]])


def _clips(seed, lengths, V, C_src, dtype, scale=40.0, shift=100.0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((t, V, C_src)) * scale + shift).astype(dtype) for t in lengths]


def _matrices(pkg, n, seed=0):
    """n matrices that move points: the reference's draws, and GENERAL first."""
    rng = np.random.RandomState(seed)
    out = [GENERAL]
    while len(out) < n:
        M = pkg.data.augmentation_matrix(rng)
        if not np.array_equal(M[:2, :2], np.eye(2)):
            out.append(M)
    return np.asarray(out)


def _expected(pkg, clip, T_out, M, C):
    """(cast (C, T_out, V) fp32: the host's plain cast; ref64 (2, T_out, V) and
    bound (2, T_out, V) of the transformed channels, None without M)."""
    padded = pkg.data.pad_array_with_loops(clip[None], T_out)[0][:T_out]
    with np.errstate(over="ignore"):
        cast = np.ascontiguousarray(padded[:, :, :C].astype(np.float32).transpose(2, 0, 1))
    if M is None:
        return cast, None, None
    wide = padded.astype(np.float64)
    t, v = wide.shape[:2]
    h = np.zeros((t, v, 3))
    h[:, :, :2] = wide[:, :, :2]
    ref = np.reshape(np.reshape(h, (t * v, 3)).dot(M), (t, v, 3))[:, :, :2]
    mag = np.abs(wide[:, :, 0:1] * M[0, :2]) + np.abs(wide[:, :, 1:2] * M[1, :2])
    bound = 2.0 ** -24 * np.abs(ref) + 2.0 ** -51 * mag
    return cast, ref.transpose(2, 0, 1), bound.transpose(2, 0, 1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check_clip(pkg, got, clip, T_out, M, C, what=""):
    """got (C, T_out, V) fp32 from the device against the gates above."""
    identity = M is None or np.array_equal(M, np.eye(M.shape[0]))
    cast, ref, bound = _expected(pkg, clip, T_out, None if identity else M, C)
    assert got.shape == cast.shape and got.dtype == np.float32, what
    if identity:
        assert np.array_equal(_bits(got), _bits(cast)), what
        return 0.0
    assert np.array_equal(_bits(got[2:]), _bits(cast[2:])), what
    diff = np.abs(got[:2].astype(np.float64) - ref)
    worst = float((diff / bound).max())
    assert np.all(diff <= bound), (what, worst)
    return worst


def _to_device(pkg, clips, T_out, C_src, dtype, transforms=None, place=None):
    """pack_clips -> (src, table) on the device, src with exactly the frames the
    batch needs. place(t, name): how a host tensor gets there."""
    place = place or (lambda t, name: t.to(DEV))
    items = [(c, np.array([0])) for c in clips]
    buf, table, _ = pkg.data.pack_clips(items, T_out, C_src, dtype, transforms=transforms)
    src = place(torch.from_numpy(buf), "src")
    tab = place(torch.from_numpy(table.view(np.uint8).copy()), "table")
    return src, tab, table


def _stage(pkg, clips, T_out, C, C_src, dtype, transforms=None):
    src, tab, _ = _to_device(pkg, clips, T_out, C_src, dtype, transforms)
    V = clips[0].shape[1]
    x = torch.empty(len(clips), C, T_out, V, device=DEV)
    status = torch.full((len(clips),), -7, dtype=torch.int32, device=DEV)
    pkg.data.stage_clips(src, tab, x, status)
    torch.cuda.synchronize()
    assert status.tolist() == [0] * len(clips)
    return x.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("C_src,C", [(2, 2), (3, 2), (3, 3)])
@pytest.mark.parametrize("V", [18, 25, 50])
def test_stage_matches_host_pipeline(pkg, V, C_src, C, dtype):
    clips = _clips(V * 10 + C_src + C, LENGTHS, V, C_src, dtype)
    got = _stage(pkg, clips, T_OUT, C, C_src, dtype)
    for n, clip in enumerate(clips):
        _check_clip(pkg, got[n], clip, T_OUT, None, C, f"plain clip {n}")
    Ms = _matrices(pkg, 3, seed=V)
    got = _stage(pkg, clips, T_OUT, C, C_src, dtype, transforms=Ms)
    worst = [_check_clip(pkg, got[n], clip, T_OUT, Ms[n], C, f"transformed clip {n}")
             for n, clip in enumerate(clips)]
    print("worst |dev - ref64| / bound per clip", worst)
    # mixed: an identity among transforms takes the cast path (flags = 0)
    mixed = np.asarray([Ms[0], np.eye(3), Ms[2]])
    got = _stage(pkg, clips, T_OUT, C, C_src, dtype, transforms=mixed)
    for n, clip in enumerate(clips):
        _check_clip(pkg, got[n], clip, T_OUT, mixed[n], C, f"mixed clip {n}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_stage_clip_spans_workgroups(pkg, dtype):
    """T_out = 64, V = 50: 3200 points per plane, 13 workgroups per clip."""
    clips = _clips(64, (5, 64, 90), 50, 3, dtype)
    Ms = _matrices(pkg, 3, seed=64)
    Ms[1] = np.eye(3)
    got = _stage(pkg, clips, 64, 3, 3, dtype, transforms=Ms)
    for n, clip in enumerate(clips):
        _check_clip(pkg, got[n], clip, 64, Ms[n], 3, f"clip {n}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_plain_cast_is_bit_exact_on_special_values(pkg, dtype):
    """The "no transform" path is the host's cast bit for bit: infinities, NaN,
    signed zero, values that overflow fp32 or land in its subnormals."""
    clips = _clips(3, LENGTHS, 25, 3, dtype)
    special = [np.inf, -np.inf, np.nan, -0.0, 3.0e38, 1e-40, -1e-45]
    if dtype == np.float64:
        special += [1e300, -1e300, 1e-50, 3.4028235677973366e38, 1.0 + 2.0 ** -24]
    for clip in clips:
        flat = clip.reshape(-1)
        with np.errstate(over="ignore"):
            flat[:len(special)] = np.asarray(special).astype(dtype)
    got = _stage(pkg, clips, T_OUT, 3, 3, dtype)
    for n, clip in enumerate(clips):
        cast, _, _ = _expected(pkg, clip, T_OUT, None, 3)
        assert np.array_equal(_bits(got[n]), _bits(cast)), n
    assert np.isnan(got).any() and np.isinf(got).any()


@pytest.mark.parametrize("seed", range(6))
def test_stage_matches_reference_augmentation(pkg, seed):
    """The reference's own augment_data outputs (data_pipeline.npz): seed s,
    M = augmentation_matrix(), applied by the kernel to augment_in."""
    gold = load_npz("data_pipeline.npz")
    seqs, want = gold["augment_in"], gold[f"augment_out_seed{seed}"]
    np.random.seed(seed)
    M = pkg.data.augmentation_matrix()
    clips = [np.ascontiguousarray(s) for s in seqs]
    T_out = max(c.shape[0] for c in clips)
    assert all(c.shape[0] == T_out for c in clips)   # (no padding in this fixture)
    got = _stage(pkg, clips, T_out, 2, 2, np.float64, transforms=np.tile(M, (len(clips), 1, 1)))
    for n, clip in enumerate(clips):
        ref = want[n].transpose(2, 0, 1)
        mag = np.abs(clip[:, :, 0:1] * M[0, :2]) + np.abs(clip[:, :, 1:2] * M[1, :2])
        bound = 2.0 ** -24 * np.abs(ref) + 2.0 ** -51 * mag.transpose(2, 0, 1)
        diff = np.abs(got[n].astype(np.float64) - ref)
        assert np.all(diff <= bound), (n, float((diff / np.maximum(bound, 1e-300)).max()))


def _clean(pkg, dtype, transforms):
    clips = _clips(7, LENGTHS, 25, 3, dtype)
    return clips, _stage(pkg, clips, T_OUT, 3, 3, dtype, transforms=transforms)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_stage_poisoned(pkg, dtype):
    """x and status start as the fill inside guard bands, src and the table are
    guarded inputs: no guard byte moves, no input changes, and every element of
    x and status is written (the result equals the clean run under every fill,
    and an unwritten element would keep a fill)."""
    Ms = _matrices(pkg, 3, seed=1)
    Ms[2] = np.eye(3)
    clips, clean = _clean(pkg, dtype, Ms)
    for fill in poison.FILLS:
        with poison.poisoned(pkg, fill):
            src, tab, _ = _to_device(
                pkg, clips, T_OUT, 3, dtype, Ms,
                place=lambda t, name: poison.guarded(t, fill, DEV, name=name))
            x = poison.empty((3, 3, T_OUT, 25), fill, device=DEV, name="x")
            status = poison.empty(3, fill, dtype=torch.int32, device=DEV, name="status")
            pkg.data.stage_clips(src, tab, x, status)
            torch.cuda.synchronize()
        poison.check_guards()
        poison.check_inputs()
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(clean)), f"fill {fill:#04x}"
        assert status.tolist() == [0, 0, 0], f"fill {fill:#04x}"


def test_src_at_its_natural_alignment(pkg):
    """fp32 src 4 bytes and fp64 src 8 bytes off a 16-byte boundary: the same
    results; x 4 bytes off is refused, naming x."""
    Ms = _matrices(pkg, 3, seed=2)
    for dtype, skew in ((np.float32, 4), (np.float64, 8)):
        clips, clean = _clean(pkg, dtype, Ms)
        with poison.poisoned(pkg, 0x4B):
            src, tab, _ = _to_device(
                pkg, clips, T_OUT, 3, dtype, Ms,
                place=lambda t, name: poison.guarded(t, 0x4B, DEV, name=name,
                                                     skew=skew if name == "src" else 0))
            assert src.data_ptr() % 16 == skew
            x = torch.empty(3, 3, T_OUT, 25, device=DEV)
            status = torch.empty(3, dtype=torch.int32, device=DEV)
            pkg.data.stage_clips(src, tab, x, status)
            torch.cuda.synchronize()
        poison.check_guards()
        poison.check_inputs()
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(clean)), dtype
        flat = torch.zeros(x.numel() + 8, device=DEV)
        off = next(o for o in range(8) if (flat.data_ptr() + 4 * o) % 16 == 4)
        x4 = flat[off:off + x.numel()].view(x.shape)
        assert x4.data_ptr() % 16 == 4 and x4.is_contiguous()
        with pytest.raises(RuntimeError, match="x: must be 16-byte aligned"):
            pkg.data.stage_clips(src, tab, x4, status)
        torch.cuda.synchronize()
        assert not flat.any()    # refused before any launch


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("bad", ["frames=0", "past the end", "first_frame=-1"])
def test_invalid_entries(pkg, bad, dtype):
    """A table entry outside [0, src_frames): that clip zeros, status 1, its
    neighbours right, no guard touched. src is a window of src_frames frames
    one frame inside a larger guarded allocation, so even a read the kernel
    must not make would stay in memory this test owns."""
    V, C_src, C, fill = 25, 3, 3, 0x4B
    Ms = _matrices(pkg, 3, seed=3)
    clips = _clips(11, LENGTHS, V, C_src, dtype)
    clean = _stage(pkg, clips, T_OUT, C, C_src, dtype, transforms=Ms)
    items = [(c, np.array([0])) for c in clips]
    buf, table, _ = pkg.data.pack_clips(items, T_OUT, C_src, dtype, transforms=Ms)
    F = buf.shape[0]
    if bad == "frames=0":
        table["frames"][1] = 0
    elif bad == "past the end":
        table["first_frame"][1], table["frames"][1] = F - 2, 5
    else:
        table["first_frame"][1], table["frames"][1] = -1, 3
    big = np.concatenate([np.full((3,) + buf.shape[1:], 1e6, dtype), buf,
                          np.full((8,) + buf.shape[1:], 1e6, dtype)])
    with poison.poisoned(pkg, fill):
        bigd = poison.guarded(torch.from_numpy(big), fill, DEV, name="src")
        src = bigd[3:3 + F]
        tab = poison.guarded(torch.from_numpy(table.view(np.uint8).copy()), fill, DEV,
                             name="table")
        x = poison.empty((3, C, T_OUT, V), fill, device=DEV, name="x")
        status = poison.empty(3, fill, dtype=torch.int32, device=DEV, name="status")
        pkg.data.stage_clips(src, tab, x, status)
        torch.cuda.synchronize()
    poison.check_guards()
    poison.check_inputs()
    got = x.cpu().numpy()
    assert status.tolist() == [0, 1, 0]
    assert not got[1].any() and not np.signbit(got[1]).any()
    assert np.array_equal(_bits(got[0]), _bits(clean[0]))
    assert np.array_equal(_bits(got[2]), _bits(clean[2]))


def test_stage_in_a_captured_graph(pkg):
    """stage_clips recorded once, replayed three times with the staging buffer
    and the table rewritten before each replay: every replay equals an eager
    launch on the same contents bit for bit (the table is read when the kernel
    runs, not when it is recorded)."""
    V, C_src, C, N = 25, 3, 3, 3
    cap = N * T_OUT
    src = torch.zeros(cap, V, C_src, device=DEV)
    tab = torch.zeros(N * 48, dtype=torch.uint8, device=DEV)
    x = torch.zeros(N, C, T_OUT, V, device=DEV)
    status = torch.zeros(N, dtype=torch.int32, device=DEV)

    def fill(i):
        lengths = [(1, 7, 13), (11, 2, 5), (4, 30, 1)][i]
        clips = _clips(20 + i, lengths, V, C_src, np.float32)
        Ms = _matrices(pkg, 3, seed=30 + i)
        Ms[i] = np.eye(3)
        buf, table, _ = pkg.data.pack_clips([(c, np.array([0])) for c in clips], T_OUT, C_src,
                                            np.float32, transforms=Ms)
        src[:buf.shape[0]].copy_(torch.from_numpy(buf))
        tab.copy_(torch.from_numpy(table.view(np.uint8).copy()))
        return clips, Ms

    fill(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # (one launch before the capture, as torch asks)
        pkg.data.stage_clips(src, tab, x, status)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pkg.data.stage_clips(src, tab, x, status)
    seen = []
    for i in (1, 2, 0):
        clips, Ms = fill(i)
        x.fill_(float("nan"))
        status.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        got = x.cpu().numpy().copy()
        assert status.tolist() == [0, 0, 0]
        x2 = torch.empty_like(x)
        st2 = torch.empty_like(status)
        pkg.data.stage_clips(src, tab, x2, st2)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(got), _bits(x2.cpu().numpy())), i
        for n, clip in enumerate(clips):
            _check_clip(pkg, got[n], clip, T_OUT, Ms[n], C, f"replay {i} clip {n}")
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


def _batches(V, C_src, dtype, scale=40.0, shift=100.0):
    out = []
    for b, lengths in enumerate(((9, 5, 12), (1, 14, 3), (6, 6, 2))):
        clips = _clips(40 + b, lengths, V, C_src, dtype, scale, shift)
        out.append([(c[None] if b == 1 else c, np.array([(b + i) % 6]))
                    for i, c in enumerate(clips)])
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_ragged_device_loader(pkg, dtype):
    """Three ragged batches, T_out = the batch maximum, per-clip matrices drawn
    by the loader under fixed seeds: each clip equals its expected value."""
    V, C_src, C = 25, 3, 2
    batches = _batches(V, C_src, dtype)
    random.seed(4)
    np.random.seed(4)
    want_tr = [pkg.data.clip_transforms(len(b)) for b in batches]
    assert any(not np.array_equal(t, np.eye(3)) for tr in want_tr for t in tr)
    assert any(np.array_equal(t, np.eye(3)) for tr in want_tr for t in tr)
    random.seed(4)
    np.random.seed(4)
    loader = pkg.data.RaggedDeviceLoader(
        batches, DEV, V, C, C_src, augment=True,
        src_dtype=torch.float32 if dtype == np.float32 else torch.float64)
    seen = 0
    for (x, y), items, tr in zip(loader, batches, want_tr):
        T_out = max(np.asarray(c).shape[-3] for c, _ in items)
        assert tuple(x.shape) == (3, C, T_out, V) and x.dtype == torch.float32
        assert x.is_contiguous() and y.dtype == torch.int64 and y.device == x.device
        assert y.tolist() == [int(lab[0]) for _, lab in items]
        got = x.cpu().numpy()
        for n, (clip, _) in enumerate(items):
            clip = clip[0] if clip.ndim == 4 else clip
            _check_clip(pkg, got[n], clip, T_out, tr[n], C, f"batch {seen} clip {n}")
        seen += 1
    assert seen == 3


def test_ragged_device_loader_static_outputs(pkg):
    """A fixed T_out with out= / labels_out=: the loader yields the caller's own
    tensors (what a GraphedStep captured), rewritten per batch; longer clips are
    cut to T_out."""
    V, C_src, C, T_out = 18, 2, 2, 8
    batches = _batches(V, C_src, np.float32)
    out = torch.full((3, C, T_out, V), float("nan"), device=DEV)
    labels_out = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    loader = pkg.data.RaggedDeviceLoader(batches, DEV, V, C, C_src, T_out=T_out, out=out,
                                         labels_out=labels_out)
    seen = 0
    for (x, y), items in zip(loader, batches):
        assert x.data_ptr() == out.data_ptr() and x is out
        assert y.data_ptr() == labels_out.data_ptr()
        assert y.tolist() == [int(lab[0]) for _, lab in items]
        got = x.cpu().numpy()
        for n, (clip, _) in enumerate(items):
            clip = clip[0] if clip.ndim == 4 else clip
            _check_clip(pkg, got[n], clip, T_out, None, C, f"batch {seen} clip {n}")
        seen += 1
    assert seen == 3
    with pytest.raises(ValueError, match="fixed T_out"):
        pkg.data.RaggedDeviceLoader(batches, DEV, V, C, C_src, out=out)


def test_ragged_device_loader_reports_invalid_entries_once(pkg, monkeypatch):
    """A table entry the kernel refuses (here: the packer is made to write
    frames = 0 for one clip of the second batch) does not stop the iteration:
    every batch is yielded, that clip as zeros, and the loader raises after the
    last one, naming the clip."""
    V, C_src, C = 25, 3, 3
    batches = _batches(V, C_src, np.float32)
    real, calls = pkg.data.pack_clips, []

    def broken(items, *a, **kw):
        buf, table, labels = real(items, *a, **kw)
        calls.append(len(calls))
        if len(calls) == 2:
            table["frames"][2] = 0
        return buf, table, labels

    monkeypatch.setattr(pkg.data, "pack_clips", broken)
    it = iter(pkg.data.RaggedDeviceLoader(batches, DEV, V, C, C_src))
    seen = []
    with pytest.raises(RuntimeError, match=r"invalid clip table entries.*\[5\]"):
        while True:
            try:
                x, _ = next(it)
            except StopIteration:
                break
            seen.append(x.cpu().numpy())
    assert len(seen) == 3
    assert not seen[1][2].any() and seen[1][0].any() and seen[1][1].any()
    assert all(s.any(axis=(1, 2, 3)).all() for s in (seen[0], seen[2]))


def test_loader_feeds_eval_step_like_the_old_route(pkg):
    """A cfg1-sized stack's eval_step on the loader's tensor against the same
    step on the old route's tensor (per-clip float64 transform on the host,
    loopy_pad_collate_fn, DeviceLoader). The inputs agree to the bound above
    (one fp32 rounding apart at most), so the logits are held to the stack
    gate of tests/test_gpu_stack.py for the fp32 GEMM modes: rel-to-max < 1e-4."""
    V, C = 18, 2
    gr = pkg.graph
    A = gr.get_normalized_adjacency_matrices(0, 1, graph=gr.graph_for(V))
    A = A / A.abs().sum(dim=(0, 2), keepdim=True)   # (eval mode: test_gpu_eval._stack)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = pkg.STGCNStack(C, 2, A, f32_gemm="f16x2").to(DEV).eval()
    batches = _batches(V, C, np.float64, scale=1.0, shift=0.0)
    random.seed(9)
    np.random.seed(9)
    trs = [pkg.data.clip_transforms(len(b)) for b in batches]
    old = []
    for items, tr in zip(batches, trs):
        moved = []
        for (clip, lab), M in zip(items, tr):
            clip = clip if clip.ndim == 4 else clip[None]
            t, v = clip.shape[1:3]
            h = np.zeros((t * v, 3))
            h[:, :2] = clip.reshape(t * v, 2)
            moved.append((h.dot(M)[:, :2].reshape(1, t, v, 2), lab))
        old.append(pkg.data.loopy_pad_collate_fn(moved))
    random.seed(9)
    np.random.seed(9)
    new = pkg.data.RaggedDeviceLoader(batches, DEV, V, C, C, src_dtype=torch.float64,
                                      augment=True)
    seen = 0
    for (xo, yo), (xn, yn) in zip(pkg.data.DeviceLoader(old, DEV), new):
        assert xo.shape == xn.shape and torch.equal(yo, yn)
        _, lo = model.eval_step(xo, yo)
        lo = lo.cpu().numpy().copy()
        _, ln = model.eval_step(xn, yn)
        err = rel_to_max(ln.cpu().numpy(), lo)
        print("input max |new - old|", float((xn - xo).abs().max()), "logits rel-to-max", err)
        assert np.isfinite(lo).all() and err < 1e-4, err
        seen += 1
    assert seen == 3
