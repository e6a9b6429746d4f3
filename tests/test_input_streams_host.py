"""STGCN_FEATURE_INPUT_STREAMS without a GPU: the feature bit, the exports and
the descriptor's size, stgcn_input_streams_check and the argument checks of
stgcn_input_stage_streams, graph.parents, the stream-name parser and
data.streams_reference against a hand-written loop."""
import ctypes

import numpy as np
import pytest

COCO18 = [1, 1, 1, 2, 3, 1, 5, 6, 2, 8, 9, 5, 11, 12, 0, 0, 14, 15]
BODY25 = [1, 1, 1, 2, 3, 1, 5, 6, 1, 8, 9, 10, 8, 12, 13, 0, 0, 15, 16, 14, 19, 14, 11, 22, 11]


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.hip_lib.load_library()


def _desc(pkg, streams=15, score_channel=-1, **kw):
    base = dict(N=3, C=3, T_out=11, V=25, C_src=3, src_f64=0, src_frames=33)
    base.update(kw)
    return pkg.hip_lib.StreamsDesc(pkg.hip_lib.InputDesc(**base), streams, score_channel)


def test_feature_bit_exports_and_struct_size(pkg, lib):
    hl = pkg.hip_lib
    for name in ("stgcn_input_streams_check", "stgcn_input_stage_streams"):
        assert hasattr(lib, name), name
        assert name in hl.EXPORTED
    assert lib.stgcn_features() & 256 == hl.FEATURE_INPUT_STREAMS == 256
    assert lib.stgcn_features() & 255 == 255  # (bits 0..7 stay)
    assert lib.stgcn_abi_version() == hl.ABI_VERSION == 11
    assert ctypes.sizeof(hl.StreamsDesc) == 40
    assert hl.StreamsDesc.streams.offset == 32 and hl.StreamsDesc.score_channel.offset == 36
    assert ctypes.sizeof(hl.InputDesc) == 32     # (unchanged)
    assert (hl.STREAM_JOINT, hl.STREAM_BONE, hl.STREAM_JOINT_MOTION,
            hl.STREAM_BONE_MOTION) == (1, 2, 4, 8)


@pytest.mark.parametrize("kw", [
    dict(), dict(streams=1), dict(streams=2), dict(streams=4), dict(streams=8), dict(streams=6),
    dict(score_channel=2), dict(C=4, C_src=4, score_channel=3), dict(C=2, C_src=2),
    dict(C=2), dict(src_f64=1), dict(V=256), dict(V=300, streams=5), dict(V=1, T_out=300),
    dict(N=128, T_out=300, V=50)])
def test_streams_check_accepts(pkg, lib, kw):
    assert lib.stgcn_input_streams_check(ctypes.byref(_desc(pkg, **kw))) == 0, \
        lib.stgcn_last_error()


@pytest.mark.parametrize("kw,code,msg", [
    (dict(streams=0), -1, b"mask"), (dict(streams=16), -1, b"mask"),
    (dict(streams=31), -1, b"mask"), (dict(streams=-1), -1, b"mask"),
    (dict(score_channel=1), -1, b"score_channel"), (dict(score_channel=0), -1, b"score_channel"),
    (dict(score_channel=3), -1, b"score_channel"), (dict(score_channel=-2), -1, b"score_channel"),
    (dict(C=2, score_channel=1), -1, b"score_channel"),      # in.C - 1, but below 2
    (dict(C=4, C_src=4, score_channel=2), -1, b"score_channel"),
    (dict(V=257, streams=2), -2, b"V <= 256"), (dict(V=300, streams=8), -2, b"V <= 256"),
    (dict(V=300, streams=15), -2, b"V <= 256"),
    # the input descriptor's own rules come first; its launch limit (N * ceil(T_out * V /
    # 256) < 2^31) is tighter than the streams check's own int64 size limit behind it
    (dict(N=2 ** 31 - 1, T_out=2 ** 31 - 1, V=1, src_frames=1), -2, b"too large for one launch"),
    (dict(C=1), -1, b"input: C "), (dict(N=0), -1, b"input: N"),
    (dict(T_out=2 ** 30, V=4), -2, b"T_out * V")])
def test_streams_check_refuses(pkg, lib, kw, code, msg):
    assert lib.stgcn_input_streams_check(ctypes.byref(_desc(pkg, **kw))) == code
    assert msg in lib.stgcn_last_error(), lib.stgcn_last_error()


def test_streams_check_takes_the_grid_limit_from_the_input_check(pkg, lib):
    """One more clip than the launch grid holds is the input check's refusal,
    not the size check's."""
    d = _desc(pkg, N=2 ** 31 - 1, T_out=300, V=25)
    assert lib.stgcn_input_streams_check(ctypes.byref(d)) == -2
    assert b"too large for one launch" in lib.stgcn_last_error()
    assert lib.stgcn_input_streams_check(None) == -1
    assert b"null descriptor" in lib.stgcn_last_error()


def test_argument_checks_before_any_launch(pkg, lib):
    """Fake pointers, no GPU touched: every call stops at an argument check."""
    ok = ctypes.c_void_p(256)
    names = ("src", "clips", "moves", "parents", "x", "status")

    def call(d, **p):
        return lib.stgcn_input_stage_streams(ctypes.byref(d), *[p.get(n, ok) for n in names], None)

    d = _desc(pkg)
    assert call(_desc(pkg, streams=0)) == -1 and b"mask" in lib.stgcn_last_error()
    for name in ("src", "clips", "x", "status"):
        assert call(d, **{name: None}) == -1
        assert b"null" in lib.stgcn_last_error(), name
    for bone in (2, 8, 15):
        assert call(_desc(pkg, streams=bone), parents=None) == -1
        assert b"null parents" in lib.stgcn_last_error()
    for name, bad, align in (("x", 260, 16), ("src", 258, 4), ("clips", 260, 8),
                             ("status", 258, 4), ("moves", 260, 8), ("parents", 258, 4)):
        assert call(d, **{name: ctypes.c_void_p(bad)}) == -1
        assert f"{name}: must be {align}-byte aligned".encode() in lib.stgcn_last_error()
    # without a bone bit the parents table is not looked at: null and misaligned
    # pass on to the next check (here the misaligned x)
    for par in (None, ctypes.c_void_p(258)):
        assert call(_desc(pkg, streams=5), parents=par, x=ctypes.c_void_p(260)) == -1
        assert b"x: must be 16-byte aligned" in lib.stgcn_last_error()
    # the joint stream alone is the existing launch, with its checks
    assert call(_desc(pkg, streams=1), parents=None, x=ctypes.c_void_p(260)) == -1
    assert b"x: must be 16-byte aligned" in lib.stgcn_last_error()


def test_parents_tables(pkg):
    gr = pkg.graph
    for graph, want, roots in ((gr.coco18(), COCO18, [1]), (gr.body25(), BODY25, [1]),
                               (gr.two_person_body25(), BODY25 + [p + 25 for p in BODY25],
                                [1, 26])):
        par = gr.parents(graph)
        assert par.dtype == np.int32 and par.shape == (graph.num_joints,)
        assert par.tolist() == want, graph.name
        assert np.array_equal(par, gr.parents(graph, roots=roots))
        for r in roots:
            assert par[r] == r
        assert [v for v in range(len(par)) if par[v] == v] == roots
        for v in range(len(par)):       # every chain ends at a root, inside V steps
            steps = 0
            while par[v] != v:
                assert v in graph.adj_list[par[v]]      # a bone is an edge
                v, steps = par[v], steps + 1
                assert steps < len(par)
            assert v in roots
    # another root gives another table
    par0 = gr.parents(gr.coco18(), roots=[0])
    assert par0[0] == 0 and par0[1] == 0 and par0[2] == 1


def test_parents_raises_for_unreachable_joints(pkg):
    gr = pkg.graph
    with pytest.raises(ValueError, match="cannot be reached"):
        gr.parents(gr.two_person_body25(), roots=[1])       # the second person
    adj = {0: [1], 1: [0], 2: []}
    with pytest.raises(ValueError, match=r"\[2\].*cannot be reached"):
        gr.parents(gr.SkeletonGraph("three", 3, adj, {}), roots=[0])
    with pytest.raises(ValueError, match="no default roots"):
        gr.parents(gr.SkeletonGraph("three", 3, adj, {}))
    with pytest.raises(ValueError, match="not joints"):
        gr.parents(gr.coco18(), roots=[18])


def test_stream_names(pkg):
    data = pkg.data
    assert data.STREAMS == {"j": 1, "b": 2, "jm": 4, "bm": 8}
    for name, bit in data.STREAMS.items():
        assert data.parse_streams(name) == bit
        assert data.parse_streams([name]) == bit
    assert data.parse_streams("j+b+jm+bm") == 15
    assert data.parse_streams("bm+j") == 9              # the order asked for does not matter
    assert data.parse_streams(("jm", "b")) == 6
    assert data.parse_streams(iter(["b", "b"])) == 2
    assert data.parse_streams(5) == 5
    assert [data.stream_count(m) for m in (1, 6, 15)] == [1, 2, 4]
    for bad in ("", "x", "j+", "j,b", "J", [], ["j", 2], 0, 16):
        with pytest.raises(ValueError, match="streams"):
            data.parse_streams(bad)


def _by_hand(j, par, mask, score):
    """The definitions, element by element, in float32."""
    N, C, T, V = j.shape
    half = np.float32(0.5)

    def op(b, a, c):
        return (b + a) * half if c == score else b - a

    def bone(n, c, t, v):
        return op(j[n, c, t, v], j[n, c, t, par[v]], c)

    planes = []
    for bit in (1, 2, 4, 8):
        if not mask & bit:
            continue
        out = np.zeros((N, C, T, V), dtype=np.float32)
        for n in range(N):
            for c in range(C):
                for t in range(T):
                    for v in range(V):
                        if bit == 1:
                            out[n, c, t, v] = j[n, c, t, v]
                        elif bit == 2:
                            out[n, c, t, v] = bone(n, c, t, v)
                        elif t == T - 1:
                            out[n, c, t, v] = 0.0
                        elif bit == 4:
                            out[n, c, t, v] = op(j[n, c, t + 1, v], j[n, c, t, v], c)
                        else:
                            out[n, c, t, v] = op(bone(n, c, t + 1, v), bone(n, c, t, v), c)
        planes.append(out)
    return np.concatenate(planes, axis=1)


@pytest.mark.parametrize("score", [None, 2])
@pytest.mark.parametrize("T", [4, 1])
def test_streams_reference_against_a_loop(pkg, T, score):
    rng = np.random.default_rng(T)
    j = (rng.standard_normal((2, 3, T, 5)) * 3 + 1).astype(np.float32)
    par = np.array([1, 1, 1, 2, 0], dtype=np.int32)
    for mask in (15, 1, 2, 4, 8, 10):
        got = pkg.data.streams_reference(j, par, mask, score_channel=score)
        want = _by_hand(j, par, mask, score)
        assert got.dtype == np.float32 and got.shape == (2, 3 * bin(mask).count("1"), T, 5)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), mask
    full = pkg.data.streams_reference(j, par, "j+b+jm+bm", score_channel=score)
    assert np.array_equal(full[:, :3], j)
    assert not full[:, 3:5, :, 1].any() and not np.signbit(full[:, 3:5, :, 1]).any()   # the root
    if score is None:
        assert not full[:, 5, :, 1].any()
    else:                                                # (the mean of a value with itself)
        assert np.array_equal(full[:, 5, :, 1], j[:, 2, :, 1])
    assert not full[:, 6:, T - 1].any()                  # the motion streams' last frame
    if T > 1:
        assert full[:, 6:9, :T - 1].all() and full[:, 9:, :T - 1, 2:].all()
    if score is not None:   # a mean of means stays a confidence
        lo, hi = j[:, 2].min(), j[:, 2].max()
        for s in (1, 2, 3):
            ch = full[:, 3 * s + 2, :T - 1 if s > 1 else T]
            assert ch.size == 0 or (lo <= ch.min() and ch.max() <= hi)


def test_streams_reference_refuses(pkg):
    j = np.zeros((1, 3, 2, 4), dtype=np.float32)
    par = np.zeros(4, dtype=np.int32)
    ref = pkg.data.streams_reference
    with pytest.raises(ValueError, match="float32"):
        ref(j.astype(np.float64), par, "b")
    with pytest.raises(ValueError, match="score_channel"):
        ref(j, par, "b", score_channel=1)
    with pytest.raises(ValueError, match="score_channel"):
        ref(j[:, :2], par, "b", score_channel=1)
    for bad in (np.array([0, 0, 0, 4]), np.array([0, -1, 0, 0]), np.zeros(3, dtype=np.int32)):
        with pytest.raises(ValueError, match="parents"):
            ref(j, bad, "j+bm")
    assert ref(j, None, "j+jm").shape == (1, 6, 2, 4)    # no bone stream: no table needed
