"""STGCN_FEATURE_INPUT_MOVE without a GPU: the feature bit, the exports and the
record's size, the argument checks of stgcn_input_stage_move, and the host half
(data.clip_moves, data.apply_moves_reference, pack_clips' random crop)."""
import ctypes
import random

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.hip_lib.load_library()


def _desc(pkg, **kw):
    base = dict(N=3, C=2, T_out=11, V=25, C_src=3, src_f64=0, src_frames=33)
    base.update(kw)
    return pkg.hip_lib.InputDesc(**base)


def test_feature_bit_exports_and_struct_size(pkg, lib):
    hl = pkg.hip_lib
    for name in ("stgcn_input_move_check", "stgcn_input_stage_move"):
        assert hasattr(lib, name), name
        assert name in hl.EXPORTED
    assert lib.stgcn_features() & 64 == hl.FEATURE_INPUT_MOVE == 64
    assert lib.stgcn_features() & 63 == 63  # (the earlier bits stay)
    assert lib.stgcn_abi_version() == hl.ABI_VERSION == 11
    assert ctypes.sizeof(hl.Move) == 160 and ctypes.sizeof(hl.Move) % 16 == 0
    assert ctypes.sizeof(hl.Clip) == 48     # (unchanged)
    dt = pkg.data.MOVE_DTYPE
    assert dt.itemsize == 160
    for name in ("nk", "frame", "angle", "scale", "tx", "ty"):
        assert dt.fields[name][1] == getattr(hl.Move, name).offset, name
    assert [dt.fields[n][1] for n in ("nk", "frame", "angle", "scale", "tx", "ty")] == \
        [0, 4, 24, 56, 88, 120]


def test_move_check_and_argument_checks_before_any_launch(pkg, lib):
    """Fake pointers, no GPU touched: every call stops at an argument check."""
    d = _desc(pkg)
    assert lib.stgcn_input_move_check(ctypes.byref(d)) == 0
    bad = _desc(pkg, C=1)
    assert lib.stgcn_input_move_check(ctypes.byref(bad)) == -1
    assert b"input: C " in lib.stgcn_last_error()
    assert lib.stgcn_input_move_check(None) == -1
    ok = ctypes.c_void_p(256)
    call = lambda **p: lib.stgcn_input_stage_move(  # noqa: E731
        ctypes.byref(d), p.get("src", ok), p.get("clips", ok), p.get("moves", ok),
        p.get("x", ok), p.get("status", ok), None)
    for name in ("src", "clips", "x", "status"):
        assert call(**{name: None}) == -1
        assert b"null" in lib.stgcn_last_error()
    assert call(moves=ctypes.c_void_p(260)) == -1
    assert b"moves: must be 8-byte aligned" in lib.stgcn_last_error()
    assert call(x=ctypes.c_void_p(260)) == -1
    assert b"x: must be 16-byte aligned" in lib.stgcn_last_error()
    assert call(clips=ctypes.c_void_p(260)) == -1
    assert b"clips: must be 8-byte aligned" in lib.stgcn_last_error()


@pytest.mark.parametrize("seed", range(3))
def test_clip_moves_draw_order(pkg, seed):
    """ST-GCN's random_move, clip by clip: random.choice of the segment count,
    then np.random.choice of the angles, the scales, the x and the y
    translations of the key nodes, in that order."""
    n, T_out = 7, 20
    random.seed(seed)
    np.random.seed(seed)
    got = pkg.data.clip_moves(n, T_out)
    random.seed(seed)
    np.random.seed(seed)
    for i in range(n):
        assert random.choice((1,)) == 1
        A = np.random.choice([-10., -5., 0., 5., 10.], 2)
        S = np.random.choice([0.9, 1.0, 1.1], 2)
        Tx = np.random.choice([-0.2, -0.1, 0.0, 0.1, 0.2], 2)
        Ty = np.random.choice([-0.2, -0.1, 0.0, 0.1, 0.2], 2)
        assert got["nk"][i] == 2 and got["frame"][i].tolist() == [0, T_out, 0, 0]
        assert np.array_equal(got["angle"][i], np.r_[A * np.pi / 180, 0, 0])
        assert np.array_equal(got["scale"][i], np.r_[S, 0, 0])
        assert np.array_equal(got["tx"][i], np.r_[Tx, 0, 0])
        assert np.array_equal(got["ty"][i], np.r_[Ty, 0, 0])
        assert pkg.data.move_is_valid(got[i], T_out)
    assert got.dtype == pkg.data.MOVE_DTYPE and got.shape == (n,)
    assert len(np.unique(got["angle"][:, :2])) > 1      # (the draws vary)


def test_clip_moves_candidates_and_segments(pkg):
    rng, coin = np.random.RandomState(3), random.Random(3)
    got = pkg.data.clip_moves(5, 20, rng=rng, coin=coin, angle_candidate=[90.0],
                              scale_candidate=[2.0], transform_candidate=[0.5],
                              move_time_candidate=[3])
    assert got["nk"].tolist() == [4] * 5
    assert got["frame"][0].tolist() == [0, 7, 13, 20]   # arange(0, 20, 20 / 3).round(), then 20
    assert np.all(got["angle"] == 90.0 * np.pi / 180) and np.all(got["scale"] == 2.0)
    assert np.all(got["tx"] == 0.5) and np.all(got["ty"] == 0.5)
    with pytest.raises(ValueError, match="2 to 4"):
        pkg.data.clip_moves(1, 20, move_time_candidate=[4])


def _x(seed, N=3, T=9, V=5, C=3):
    return np.random.default_rng(seed).standard_normal((N, T, V, C)) * 3 + 1


def test_reference_without_a_move_is_the_identity(pkg):
    x = _x(0)
    x[0, 0, 0] = [np.inf, np.nan, -0.0]
    moves = np.zeros(3, dtype=pkg.data.MOVE_DTYPE)
    got = pkg.data.apply_moves_reference(x, moves)
    assert got.dtype == np.float64
    assert np.array_equal(got.view(np.int64), x.view(np.int64))
    aff = pkg.data.move_frame_affine(moves, 9)
    assert np.array_equal(aff, np.tile(np.array([1.0, 0, 0, 0])[:, None], (3, 1, 9)))


def test_reference_with_constant_parameters_is_one_affine_map(pkg):
    x = _x(1)
    moves = np.zeros(3, dtype=pkg.data.MOVE_DTYPE)
    a, s, tx, ty = 0.3, 1.25, -0.75, 2.0
    for n, frames in enumerate(([0, 9], [0, 4, 8], [0, 2, 5, 30])):
        k = len(frames)
        moves["nk"][n] = k
        moves["frame"][n, :k] = frames
        moves["angle"][n, :k], moves["scale"][n, :k] = a, s
        moves["tx"][n, :k], moves["ty"][n, :k] = tx, ty
    got = pkg.data.apply_moves_reference(x, moves)
    c, sn = np.cos(a) * s, np.sin(a) * s
    assert np.array_equal(got[..., 0], (c * x[..., 0] - sn * x[..., 1]) + tx)
    assert np.array_equal(got[..., 1], (sn * x[..., 0] + c * x[..., 1]) + ty)
    assert np.array_equal(got[..., 2], x[..., 2])       # confidence passes through


def test_reference_interpolates_like_linspace(pkg):
    """Two segments: frame t of segment k has start + i * step with step =
    (p_{k+1} - p_k) / (f_{k+1} - f_k); the last frame belongs to the last one."""
    T = 9
    moves = np.zeros(1, dtype=pkg.data.MOVE_DTYPE)
    moves["nk"], moves["frame"][0, :3] = 3, [0, 3, 8]
    moves["angle"][0, :3], moves["scale"][0, :3] = [0.1, 0.4, -0.2], [1.0, 1.3, 0.7]
    moves["tx"][0, :3], moves["ty"][0, :3] = [0.0, 0.3, 0.1], [1.0, -1.0, 2.0]
    aff = pkg.data.move_frame_affine(moves, T)[0]
    for t in range(T):
        k = 0 if t < 3 else 1
        f0, f1 = moves["frame"][0, k], moves["frame"][0, k + 1]
        p = {q: moves[q][0, k] + float(t - f0) * ((moves[q][0, k + 1] - moves[q][0, k]) /
                                                   float(f1 - f0))
             for q in ("angle", "scale", "tx", "ty")}
        want = [np.cos(p["angle"]) * p["scale"], np.sin(p["angle"]) * p["scale"], p["tx"],
                p["ty"]]
        assert aff[:, t].tolist() == want, t
    # t = 8 is the end node, reached by start + i * step (to rounding, not exactly)
    assert abs(aff[2, 8] - 0.1) < 1e-15 and abs(aff[3, 8] - 2.0) < 1e-15


@pytest.mark.parametrize("what", ["nk=1", "nk=5", "frame0", "order", "short", "nan", "inf"])
def test_reference_refuses_what_the_kernel_refuses(pkg, what):
    T = 9
    mv = np.zeros(1, dtype=pkg.data.MOVE_DTYPE)
    mv["nk"], mv["frame"][0, :3], mv["scale"][0, :3] = 3, [0, 4, 8], 1.0
    assert pkg.data.move_is_valid(mv[0], T)
    if what == "nk=1":
        mv["nk"] = 1
    elif what == "nk=5":
        mv["nk"] = 5
    elif what == "frame0":
        mv["frame"][0, 0] = 1
    elif what == "order":
        mv["frame"][0, :3] = [0, 8, 8]
    elif what == "short":
        mv["frame"][0, :3] = [0, 4, 7]
    elif what == "nan":
        mv["tx"][0, 2] = np.nan
    else:
        mv["angle"][0, 0] = np.inf
    assert not pkg.data.move_is_valid(mv[0], T)
    with pytest.raises(ValueError, match="record 0 is invalid"):
        pkg.data.apply_moves_reference(_x(2, N=1), mv)
    mv["nk"] = 0                                        # nk = 0: nothing else is looked at
    assert pkg.data.move_is_valid(mv[0], T)


def _frame_items(lengths, V=4, C_src=2):
    """Clips whose every value is their frame index: a window shows its start."""
    return [(np.tile(np.arange(t, dtype=np.float64)[:, None, None], (1, V, C_src)),
             np.array([i])) for i, t in enumerate(lengths)]


@pytest.mark.parametrize("seed", range(3))
def test_random_crop_windows(pkg, seed):
    lengths, T_out = (30, 5, 12, 12, 13, 40), 12
    items = _frame_items(lengths)
    buf, table, labels = pkg.data.pack_clips(items, T_out, 2, np.float64, crop="random",
                                             coin=random.Random(seed))
    coin = random.Random(seed)
    want = [coin.randint(0, t - T_out) if t > T_out else 0 for t in lengths]
    assert table["frames"].tolist() == [min(t, T_out) for t in lengths]
    starts = []
    for first, f, t in zip(table["first_frame"], table["frames"], lengths):
        window = buf[first:first + f, 0, 0]
        assert np.array_equal(window, window[0] + np.arange(f))      # consecutive frames
        assert 0 <= window[0] and window[-1] <= t - 1               # inside the clip
        starts.append(int(window[0]))
    assert starts == want
    assert labels.tolist() == list(range(len(lengths)))
    # python's global generator by default
    random.seed(seed)
    buf2, _, _ = pkg.data.pack_clips(items, T_out, 2, np.float64, crop="random")
    random.seed(seed)
    want2 = [random.randint(0, t - T_out) if t > T_out else 0 for t in lengths]
    assert [int(buf2[f, 0, 0]) for f in table["first_frame"]] == want2
    with pytest.raises(ValueError, match="crop is"):
        pkg.data.pack_clips(items, T_out, 2, np.float64, crop="last")


def test_random_crop_over_seeds_reaches_both_ends(pkg):
    items = _frame_items((14,))
    seen = {int(pkg.data.pack_clips(items, 12, 2, np.float64, crop="random",
                                    coin=random.Random(s))[0][0, 0, 0]) for s in range(40)}
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pack_clips_default_is_unchanged(pkg, dtype):
    """Without the new argument, and with crop="first": the same bytes, and no
    draw from python's generator."""
    rng = np.random.default_rng(5)
    items = [((rng.standard_normal((t, 25, 3)) * 40 + 100).astype(dtype), np.array([i]))
             for i, t in enumerate((1, 7, 13, 11, 30))]
    tr = np.tile(np.eye(3), (5, 1, 1))
    tr[2] = [[0.5, 2.0, 0.0], [-3.0, 4.0, 0.0], [5.0, 5.0, 1.0]]
    random.seed(1)
    state = random.getstate()
    a = pkg.data.pack_clips(items, 11, 3, dtype, transforms=tr)
    b = pkg.data.pack_clips(items, 11, 3, dtype, transforms=tr, crop="first")
    assert random.getstate() == state
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes()
    first = a[1]["first_frame"]
    for (clip, _), f0, f in zip(items, first, a[1]["frames"]):
        assert a[0][f0:f0 + f].tobytes() == clip[:f].tobytes()      # the first frames
