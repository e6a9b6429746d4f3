"""Random moving in the input stage on the GPU (stgcn_input_stage_move through
data.stage_clips(moves=...) and data.RaggedDeviceLoader(move=True,
crop="random")).

Expected values: per clip ``pad_array_with_loops`` to T_out, the clip's own 2x2
matrix by the kernel's operations (two products and one sum in float64), then
``data.apply_moves_reference`` (numpy float64), then the transpose.

Gate of a moved element. Both sides evaluate the same fp64 operations; only the
device's sin / cos may differ from numpy's in the last bits, a relative 2^-52 or
so of c and sn that the products carry into the three terms of the sum. So, with
one fp32 rounding at the end,

    |dev - ref64| <= ulp32(ref64) + 2^-45 (|c x| + |sn y| + |tx|)

(likewise for y'), and because that slack only matters where the fp64 values
straddle an fp32 rounding boundary, at least 99 % of the moved elements must be
bit-equal to the reference rounded to fp32. The inputs are chosen without
cancellation (|x'| >= 2^-10 of the summed terms, asserted on the CPU), so the
reference itself is well inside the bound. The channels past the first two are
bit-equal to the host's cast, and an unmoved clip (nk = 0) is bit-equal to the
launch without moves (stgcn_input_stage), whose matrix product the compiler
contracts to one fused multiply-add: numpy cannot restate that bit for bit.
"""
import random

import numpy as np
import pytest
import torch

import poison

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 3
# positive entries: points in the first quadrant stay there (no cancellation)
MATRIX = np.array([[0.83, 0.41, 0.0], [0.29, 1.31, 0.0], [5.0, 5.0, 1.0]])


def _lengths(T_out):
    return (max(1, T_out - 3), T_out, T_out + 5)    # below, equal to, above T_out


def _clips(seed, lengths, V, C_src, dtype):
    """x, y in [1, 3), confidence in [0, 1)."""
    rng = np.random.default_rng(seed)
    out = []
    for t in lengths:
        c = rng.random((t, V, C_src))
        c[:, :, :2] = 1.0 + 2.0 * c[:, :, :2]
        out.append(c.astype(dtype))
    return out


def _moves(pkg, seed, nks, T_out):
    """One record per entry of nks (0, 2, 3 or 4 key frames), parameters from
    the published candidates' ranges but not on their grid."""
    rng = np.random.default_rng(seed)
    mv = np.zeros(len(nks), dtype=pkg.data.MOVE_DTYPE)
    for n, nk in enumerate(nks):
        if nk == 0:
            continue
        inner = np.sort(rng.choice(np.arange(1, T_out - 1), nk - 2, replace=False))
        mv["nk"][n] = nk
        # the last node at T_out (the loader's) or at T_out - 1 (the least allowed)
        mv["frame"][n, :nk] = np.r_[0, inner, T_out - (n % 2)]
        mv["angle"][n, :nk] = rng.uniform(-10, 10, nk) * np.pi / 180
        mv["scale"][n, :nk] = rng.uniform(0.9, 1.1, nk)
        mv["tx"][n, :nk] = rng.uniform(-0.2, 0.2, nk)
        mv["ty"][n, :nk] = rng.uniform(-0.2, 0.2, nk)
        assert pkg.data.move_is_valid(mv[n], T_out)
    return mv


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def _expected(pkg, clips, T_out, Ms, moves, C):
    """ref64 (N, C, T_out, V) float64 and bound (N, 2, T_out, V): the gate of the
    moved channels (a clip without a move is held to bit-equality instead)."""
    padded = np.stack([pkg.data.pad_array_with_loops(c[None], T_out)[0][:T_out]
                       for c in clips]).astype(np.float64)
    for n, M in enumerate(Ms):
        if M is not None:
            px, py = padded[n, :, :, 0].copy(), padded[n, :, :, 1].copy()
            padded[n, :, :, 0] = px * M[0, 0] + py * M[1, 0]
            padded[n, :, :, 1] = px * M[0, 1] + py * M[1, 1]
    ref = pkg.data.apply_moves_reference(padded, moves)
    c, sn, tx, ty = (q[:, :, None] for q in
                     pkg.data.move_frame_affine(moves, T_out).transpose(1, 0, 2))
    px, py = padded[..., 0], padded[..., 1]
    terms = np.stack([np.abs(c * px) + np.abs(sn * py) + np.abs(tx),
                      np.abs(sn * px) + np.abs(c * py) + np.abs(ty)], axis=1)
    ref = np.ascontiguousarray(ref[..., :C].transpose(0, 3, 1, 2))
    # no cancellation in the chosen inputs: the reference is well-conditioned
    assert np.all(np.abs(ref[:, :2]) >= 2.0 ** -10 * terms)
    return ref, _ulp32(ref[:, :2]) + 2.0 ** -45 * terms


def _check(got, ref, bound, moves, plain, what=""):
    """plain: the same clips and matrices through the launch without moves
    (needed where a clip has nk = 0)."""
    with np.errstate(over="ignore"):
        cast = ref.astype(np.float32)
    assert got.shape == ref.shape and got.dtype == np.float32, what
    assert np.array_equal(_bits(got[:, 2:]), _bits(cast[:, 2:])), what    # confidence
    moved = moves["nk"] != 0
    if not moved.all():
        assert np.array_equal(_bits(got[~moved]), _bits(plain[~moved])), what  # nk = 0: exact
    diff = np.abs(got[:, :2].astype(np.float64) - ref[:, :2])
    worst = float((diff[moved] / bound[moved]).max()) if moved.any() else 0.0
    equal = float((_bits(got[moved][:, :2]) == _bits(cast[moved][:, :2])).mean()) \
        if moved.any() else 1.0
    print(f"{what}: worst |dev - ref64| / bound {worst:.3f}, bit-equal {equal:.5f}")
    assert np.all(diff[moved] <= bound[moved]), (what, worst)
    assert equal >= 0.99, (what, equal)


def _to_device(pkg, clips, T_out, C_src, dtype, Ms, moves, place=None):
    place = place or (lambda t, name: t.to(DEV))
    tr = None if Ms is None else np.asarray([np.eye(3) if M is None else M for M in Ms])
    buf, table, _ = pkg.data.pack_clips([(c, np.array([0])) for c in clips], T_out, C_src, dtype,
                                        transforms=tr)
    src = place(torch.from_numpy(buf), "src")
    tab = place(torch.from_numpy(table.view(np.uint8).copy()), "table")
    mvd = None if moves is None else place(torch.from_numpy(moves.view(np.uint8).copy()),
                                           "moves")
    return src, tab, mvd


def _stage(pkg, clips, T_out, C, C_src, dtype, Ms, moves, want_status=None):
    src, tab, mvd = _to_device(pkg, clips, T_out, C_src, dtype, Ms, moves)
    x = torch.full((len(clips), C, T_out, clips[0].shape[1]), float("nan"), device=DEV)
    status = torch.full((len(clips),), -7, dtype=torch.int32, device=DEV)
    pkg.data.stage_clips(src, tab, x, status, moves=mvd)
    torch.cuda.synchronize()
    assert status.tolist() == (want_status or [0] * len(clips))
    return x.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("C_src,C", [(2, 2), (3, 3)])
@pytest.mark.parametrize("T_out", [7, 20])
@pytest.mark.parametrize("V", [18, 25])
def test_move_matches_reference(pkg, V, T_out, C_src, C, dtype):
    """T_out = 20: a clip spans 2 workgroups; (7, 25): planes of 175 points, only
    dword aligned. Every nk, with and without the clip's matrix."""
    clips = _clips(V + T_out + C_src, _lengths(T_out), V, C_src, dtype)
    for i, (nks, Ms) in enumerate((((2, 4, 0), (MATRIX, None, MATRIX)),
                                   ((4, 3, 2), (None, MATRIX, MATRIX)),
                                   ((0, 2, 4), (None, None, None)))):
        moves = _moves(pkg, 100 * i + V, nks, T_out)
        ref, bound = _expected(pkg, clips, T_out, Ms, moves, C)
        got = _stage(pkg, clips, T_out, C, C_src, dtype, Ms, moves)
        plain = _stage(pkg, clips, T_out, C, C_src, dtype, Ms, None)
        _check(got, ref, bound, moves, plain, f"nk {nks}")


def test_move_with_the_published_draws(pkg):
    """clip_moves' own records (key nodes at 0 and T_out, parameters on the
    published grid, zeros among them)."""
    V, T_out, C = 25, 20, 3
    clips = _clips(5, _lengths(T_out), V, C, np.float64)
    moves = pkg.data.clip_moves(N, T_out, rng=np.random.RandomState(2), coin=random.Random(2))
    ref, bound = _expected(pkg, clips, T_out, (None, MATRIX, None), moves, C)
    got = _stage(pkg, clips, T_out, C, C, np.float64, (None, MATRIX, None), moves)
    _check(got, ref, bound, moves, None, "clip_moves")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_no_move_has_the_plain_stage_bits(pkg, dtype):
    """nk = 0 everywhere, and moves = None: stgcn_input_stage's output bit for
    bit, infinities, NaN, signed zero and fp32 subnormals included, with the
    clip's matrix and without."""
    V, T_out, C = 25, 20, 3
    clips = _clips(9, _lengths(T_out), V, C, dtype)
    special = [np.inf, -np.inf, np.nan, -0.0, 3.0e38, 1e-40, -1e-45]
    if dtype == np.float64:
        special += [1e300, -1e300, 1e-50, 3.4028235677973366e38, 1.0 + 2.0 ** -24]
    for clip in clips:
        with np.errstate(over="ignore"):
            clip.reshape(-1)[:len(special)] = np.asarray(special).astype(dtype)
    Ms = (MATRIX, None, MATRIX)
    plain = _stage(pkg, clips, T_out, C, C, dtype, Ms, None)
    assert np.isnan(plain).any() and np.isinf(plain).any()
    none = np.zeros(N, dtype=pkg.data.MOVE_DTYPE)
    got = _stage(pkg, clips, T_out, C, C, dtype, Ms, none)
    assert np.array_equal(_bits(got), _bits(plain))
    # garbage behind nk = 0 is not looked at
    none["frame"], none["angle"], none["tx"] = -5, np.nan, np.inf
    got = _stage(pkg, clips, T_out, C, C, dtype, Ms, none)
    assert np.array_equal(_bits(got), _bits(plain))


BAD = {"nk=1": ("nk", None, 1), "nk=5": ("nk", None, 5), "nk=-2": ("nk", None, -2),
       "frame[0]=1": ("frame", 0, 1), "frames equal": ("frame", 1, 0),
       "frames fall": ("frame", 2, 1), "last frame short": ("frame", 3, 18),
       "angle nan": ("angle", 1, np.nan), "scale inf": ("scale", 0, np.inf),
       "tx -inf": ("tx", 3, -np.inf), "ty nan": ("ty", 2, np.nan)}


@pytest.mark.parametrize("bad", list(BAD))
def test_bad_records(pkg, bad):
    """Every kind of invalid record: its clip zeros, status bit 1, the
    neighbours as in the clean run, no guard touched. A defined result, not a
    fault: src is a window one frame inside a larger guarded allocation, as in
    test_gpu_input_stage.test_invalid_entries."""
    V, T_out, C, fill, dtype = 25, 20, 3, 0x4B, np.float32
    clips = _clips(11, _lengths(T_out), V, C, dtype)
    Ms = (MATRIX, MATRIX, None)
    moves = _moves(pkg, 7, (2, 4, 3), T_out)
    moves["frame"][1, :4] = [0, 6, 12, 19]
    clean = _stage(pkg, clips, T_out, C, C, dtype, Ms, moves)
    field, idx, value = BAD[bad]
    if idx is None:
        moves[field][1] = value
    else:
        moves[field][1, idx] = value
    assert not pkg.data.move_is_valid(moves[1], T_out)
    tr = np.asarray([np.eye(3) if M is None else M for M in Ms])
    buf, table, _ = pkg.data.pack_clips([(c, np.array([0])) for c in clips], T_out, C, dtype,
                                        transforms=tr)
    F = buf.shape[0]
    big = np.concatenate([np.full((3,) + buf.shape[1:], 1e6, dtype), buf,
                          np.full((8,) + buf.shape[1:], 1e6, dtype)])

    def run(table, want):
        with poison.poisoned(pkg, fill):
            src = poison.guarded(torch.from_numpy(big), fill, DEV, name="src")[3:3 + F]
            tab = poison.guarded(torch.from_numpy(table.view(np.uint8).copy()), fill, DEV,
                                 name="table")
            mvd = poison.guarded(torch.from_numpy(moves.view(np.uint8).copy()), fill, DEV,
                                 name="moves")
            x = poison.empty((N, C, T_out, V), fill, device=DEV, name="x")
            status = poison.empty(N, fill, dtype=torch.int32, device=DEV, name="status")
            pkg.data.stage_clips(src, tab, x, status, moves=mvd)
            torch.cuda.synchronize()
        poison.check_guards()
        poison.check_inputs()
        assert status.tolist() == want
        return x.cpu().numpy()

    got = run(table, [0, 2, 0])
    assert not got[1].any() and not np.signbit(got[1]).any()
    assert np.array_equal(_bits(got[0]), _bits(clean[0]))
    assert np.array_equal(_bits(got[2]), _bits(clean[2]))
    if bad == "nk=1":   # bit 0 keeps its meaning beside bit 1
        table["frames"][1] = 0
        table["first_frame"][2] = F - 2
        got = run(table, [0, 3, 1])
        assert not got[1].any() and not got[2].any()
        assert np.array_equal(_bits(got[0]), _bits(clean[0]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_move_poisoned(pkg, dtype):
    """x and status start as the fill inside guard bands; src and both tables
    are guarded inputs: no guard byte moves, no input changes, and every element
    of x and status is written (the result equals the clean run under every
    fill)."""
    V, T_out, C = 25, 7, 3
    clips = _clips(13, _lengths(T_out), V, C, dtype)
    Ms = (MATRIX, None, MATRIX)
    moves = _moves(pkg, 3, (4, 2, 0), T_out)
    clean = _stage(pkg, clips, T_out, C, C, dtype, Ms, moves)
    for fill in poison.FILLS:
        with poison.poisoned(pkg, fill):
            src, tab, mvd = _to_device(
                pkg, clips, T_out, C, dtype, Ms, moves,
                place=lambda t, name: poison.guarded(t, fill, DEV, name=name))
            x = poison.empty((N, C, T_out, V), fill, device=DEV, name="x")
            status = poison.empty(N, fill, dtype=torch.int32, device=DEV, name="status")
            pkg.data.stage_clips(src, tab, x, status, moves=mvd)
            torch.cuda.synchronize()
        poison.check_guards()
        poison.check_inputs()
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(clean)), f"fill {fill:#04x}"
        assert status.tolist() == [0, 0, 0], f"fill {fill:#04x}"


def test_move_in_a_captured_graph(pkg):
    """One captured launch; the staging buffer, the clip table and the move
    table are rewritten between two replays: each replay matches the reference
    of its own tables (the records are read when the kernel runs)."""
    V, T_out, C = 25, 20, 3
    src = torch.zeros(N * T_out, V, C, device=DEV)
    tab = torch.zeros(N * 48, dtype=torch.uint8, device=DEV)
    mvd = torch.zeros(N * 160, dtype=torch.uint8, device=DEV)
    x = torch.zeros(N, C, T_out, V, device=DEV)
    status = torch.zeros(N, dtype=torch.int32, device=DEV)

    def fill(i):
        lengths = [(20, 3, 31), (9, 25, 20)][i]
        clips = _clips(50 + i, lengths, V, C, np.float32)
        Ms = [(MATRIX, None, None), (None, MATRIX, MATRIX)][i]
        moves = _moves(pkg, 60 + i, [(2, 0, 4), (3, 4, 2)][i], T_out)
        tr = np.asarray([np.eye(3) if M is None else M for M in Ms])
        buf, table, _ = pkg.data.pack_clips([(c, np.array([0])) for c in clips], T_out, C,
                                            np.float32, transforms=tr)
        src[:buf.shape[0]].copy_(torch.from_numpy(buf))
        tab.copy_(torch.from_numpy(table.view(np.uint8).copy()))
        mvd.copy_(torch.from_numpy(moves.view(np.uint8).copy()))
        return _expected(pkg, clips, T_out, Ms, moves, C) + (moves,)

    fill(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # (one launch before the capture, as torch asks)
        pkg.data.stage_clips(src, tab, x, status, moves=mvd)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pkg.data.stage_clips(src, tab, x, status, moves=mvd)
    seen = []
    for i in (1, 0):
        ref, bound, moves = fill(i)
        x.fill_(float("nan"))
        status.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        got = x.cpu().numpy().copy()
        assert status.tolist() == [0, 0, 0]
        plain = torch.empty_like(x)
        pkg.data.stage_clips(src, tab, plain, torch.empty_like(status))
        _check(got, ref, bound, moves, plain.cpu().numpy(), f"replay of tables {i}")
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1])


def _batches(V, C_src, dtype, T_out):
    out = []
    for b, lengths in enumerate(((T_out + 9, 5, T_out), (1, T_out + 14, T_out + 3))):
        clips = _clips(40 + b, lengths, V, C_src, dtype)
        out.append([(c[None] if b == 1 else c, np.array([(b + i) % 6]))
                    for i, c in enumerate(clips)])
    return out


@pytest.mark.parametrize("static", [False, True], ids=["fresh", "out="])
def test_loader_move_and_random_crop(pkg, static):
    """RaggedDeviceLoader(augment, move, crop="random") over two batches under a
    seed equals stage_clips on the same draws (per batch: the matrices, the
    moves, the window starts), bit for bit; also into out= / labels_out=."""
    V, C_src, C, T_out = 25, 3, 2, 20
    batches = _batches(V, C_src, np.float64, T_out)
    random.seed(6)
    np.random.seed(6)
    want = []
    for items in batches:
        tr = pkg.data.clip_transforms(N)
        mv = pkg.data.clip_moves(N, T_out)
        buf, table, labels = pkg.data.pack_clips(items, T_out, C_src, np.float64, transforms=tr,
                                                 crop="random")
        x = torch.empty(N, C, T_out, V, device=DEV)
        status = torch.empty(N, dtype=torch.int32, device=DEV)
        pkg.data.stage_clips(torch.from_numpy(buf).to(DEV),
                             torch.from_numpy(table.view(np.uint8).copy()).to(DEV), x, status,
                             moves=torch.from_numpy(mv.view(np.uint8).copy()).to(DEV))
        assert status.tolist() == [0] * N and (mv["nk"] == 2).all()
        want.append((x.cpu().numpy(), labels.tolist(), table["frames"].tolist()))
    # the second batch's long clips were cut somewhere past their start
    assert want[0][2] == [T_out, 5, T_out] and want[1][2] == [1, T_out, T_out]
    random.seed(6)
    np.random.seed(6)
    kw = {}
    if static:
        kw = dict(out=torch.full((N, C, T_out, V), float("nan"), device=DEV),
                  labels_out=torch.full((N,), -1, dtype=torch.int64, device=DEV))
    loader = pkg.data.RaggedDeviceLoader(batches, DEV, V, C, C_src, T_out=T_out,
                                         src_dtype=torch.float64, augment=True, move=True,
                                         crop="random", **kw)
    seen = 0
    for (x, y), (wx, wy, _) in zip(loader, want):
        if static:
            assert x is kw["out"] and y is kw["labels_out"]
        assert y.tolist() == wy
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(wx)), seen
        seen += 1
    assert seen == 2
    # the move changes the input: the same draws without it differ
    random.seed(6)
    np.random.seed(6)
    x0, _ = next(iter(pkg.data.RaggedDeviceLoader(batches[:1], DEV, V, C, C_src, T_out=T_out,
                                                  src_dtype=torch.float64, augment=True)))
    assert not np.array_equal(x0.cpu().numpy(), want[0][0])


def test_loader_reports_invalid_move_records_once(pkg, monkeypatch):
    """A record the kernel refuses (clip_moves is made to write nk = 1 for one
    clip of the second batch) does not stop the iteration: that clip is zeros,
    and the loader raises after the last batch, naming the clip."""
    V, C_src, C, T_out = 25, 3, 3, 20
    batches = _batches(V, C_src, np.float32, T_out)
    real, calls = pkg.data.clip_moves, []

    def broken(*a, **kw):
        mv = real(*a, **kw)
        calls.append(len(calls))
        if len(calls) == 2:
            mv["nk"][1] = 1
        return mv

    monkeypatch.setattr(pkg.data, "clip_moves", broken)
    it = iter(pkg.data.RaggedDeviceLoader(batches, DEV, V, C, C_src, T_out=T_out, move=True))
    seen = []
    with pytest.raises(RuntimeError, match=r"invalid move records.*\[4\]"):
        while True:
            try:
                x, _ = next(it)
            except StopIteration:
                break
            seen.append(x.cpu().numpy())
    assert len(seen) == 2
    assert not seen[1][1].any() and seen[1][0].any() and seen[1][2].any()
    assert seen[0].any(axis=(1, 2, 3)).all()
