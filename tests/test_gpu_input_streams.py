"""The bone and motion input streams of the input stage on the GPU
(stgcn_input_stage_streams through data.stage_clips(streams=...) and
data.RaggedDeviceLoader(streams=...)).

Every comparison is for bit-equality on 100 % of the elements. The joint
channels J are the existing launches' (stgcn_input_stage / _move): without a
matrix and a move they are the host's own cast of the padded source, so
``data.streams_reference`` (numpy float32, one operation at a time) of that
array is an independent reference of all four streams; with matrices and moves
the joint channels are held to the existing launch on the same device buffers
(its own tests gate it against numpy) and the derived streams to
``streams_reference`` of that output. Finite inputs only: NaN payload bits are
not specified."""
import contextlib
import io
import random

import numpy as np
import pytest
import torch

import poison
from conftest import rel_to_max
from test_gpu_input_move import DEV, MATRIX, N, _batches, _bits, _clips, _lengths, _moves, \
    _to_device
from test_gpu_stack import capture_relu_masks, check_relu_ties, gate_stack_grads, \
    oracle_through_masks, snapshot_stack

pytestmark = pytest.mark.gpu
FULL = "j+b+jm+bm"


def _parents(pkg, V):
    if V == 1:
        return np.zeros(1, dtype=np.int32)
    return pkg.graph.parents(pkg.graph.graph_for(V))


def _launch(pkg, src, tab, mvd, C, T_out, streams, parents, score, want_status=None):
    """One launch on device buffers -> x as numpy; x and status start as NaN / -7."""
    V, n = src.shape[1], tab.numel() // 48
    S = 1 if streams is None else pkg.data.stream_count(pkg.data.parse_streams(streams))
    x = torch.full((n, S * C, T_out, V), float("nan"), device=DEV)
    status = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    par = None if parents is None else torch.from_numpy(np.asarray(parents, np.int32)).to(DEV)
    kw = {} if streams is None else dict(streams=streams, parents=par, score_channel=score)
    pkg.data.stage_clips(src, tab, x, status, moves=mvd, **kw)
    torch.cuda.synchronize()
    assert status.tolist() == (want_status or [0] * n)
    return x.cpu().numpy()


def _host_joints(pkg, clips, T_out, C):
    """J without a matrix and a move: the padded source, cast and transposed."""
    padded = np.stack([pkg.data.pad_array_with_loops(c[None], T_out)[0][:T_out] for c in clips])
    return np.ascontiguousarray(padded[..., :C].astype(np.float32).transpose(0, 3, 1, 2))


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    equal = float((_bits(got) == _bits(want)).mean())
    print(f"{what}: bit-equal {equal:.6f}")
    assert equal == 1.0, (what, equal)


CASES = [(C_src, C, score) for C_src, C in ((2, 2), (3, 3)) for score in (None, 2)
         if score is None or C == 3]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("C_src,C,score", CASES)
@pytest.mark.parametrize("T_out", [7, 20])
@pytest.mark.parametrize("V", [18, 25])
def test_streams_match_the_host_reference(pkg, V, T_out, C_src, C, score, dtype):
    """No matrix, no move: all four streams against numpy on the host's own
    padded array. T_out = 20 spans two workgroups per clip: frame t + 1 and the
    parent of a point then lie in another workgroup's chunk. The clip shorter
    than T_out wraps: its seam is a real difference."""
    clips = _clips(V + T_out + C_src, _lengths(T_out), V, C_src, dtype)
    par = _parents(pkg, V)
    want = pkg.data.streams_reference(_host_joints(pkg, clips, T_out, C), par, FULL,
                                      score_channel=score)
    src, tab, _ = _to_device(pkg, clips, T_out, C_src, dtype, None, None)
    got = _launch(pkg, src, tab, None, C, T_out, FULL, par, score)
    _same(got, want, "host reference")
    assert not got[:, 2 * C:, T_out - 1].any()          # the motion streams' last frame
    assert got[:, 2 * C:2 * C + 2, :T_out - 1].all()    # and the seam of the short clip


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("V,T_out,C_src,C,score", [(25, 20, 3, 3, 2), (18, 7, 3, 2, None),
                                                   (25, 7, 2, 2, None), (18, 20, 3, 3, None)])
def test_streams_with_matrices_and_moves(pkg, V, T_out, C_src, C, score, dtype):
    """Every nk, with and without the clip's matrix: the joint channels are the
    existing move launch's bits, the other streams their float32 restatement."""
    clips = _clips(V + T_out + C_src, _lengths(T_out), V, C_src, dtype)
    par = _parents(pkg, V)
    for i, (nks, Ms) in enumerate((((2, 4, 0), (MATRIX, None, MATRIX)),
                                   ((4, 3, 2), (None, MATRIX, MATRIX)),
                                   ((0, 0, 3), (None, MATRIX, None)))):
        moves = _moves(pkg, 100 * i + V, nks, T_out)
        src, tab, mvd = _to_device(pkg, clips, T_out, C_src, dtype, Ms, moves)
        joints = _launch(pkg, src, tab, mvd, C, T_out, None, None, None)
        got = _launch(pkg, src, tab, mvd, C, T_out, FULL, par, score)
        _same(got[:, :C], joints, f"nk {nks}: joints")
        _same(got, pkg.data.streams_reference(joints, par, FULL, score_channel=score),
              f"nk {nks}: streams")
        if i == 0:      # and without the move table: stgcn_input_stage's bits
            plain = _launch(pkg, src, tab, None, C, T_out, None, None, None)
            got = _launch(pkg, src, tab, None, C, T_out, FULL, par, score)
            _same(got, pkg.data.streams_reference(plain, par, FULL, score_channel=score),
                  "matrices only")


@pytest.mark.parametrize("streams,groups", [("j", [0]), ("b", [1]), ("jm", [2]), ("bm", [3]),
                                            ("jm+b", [1, 2]), (FULL, [0, 1, 2, 3]),
                                            (["bm", "j"], [0, 3])])
def test_masks_select_and_order_the_channels(pkg, streams, groups):
    V, T_out, C = 25, 20, 3
    clips = _clips(21, _lengths(T_out), V, C, np.float32)
    moves = _moves(pkg, 22, (3, 0, 2), T_out)
    par = _parents(pkg, V)
    src, tab, mvd = _to_device(pkg, clips, T_out, C, np.float32, (MATRIX, MATRIX, None), moves)
    joints = _launch(pkg, src, tab, mvd, C, T_out, None, None, None)
    full = pkg.data.streams_reference(joints, par, FULL, score_channel=2)
    want = np.concatenate([full[:, C * g:C * (g + 1)] for g in groups], axis=1)
    needs_table = any(g in (1, 3) for g in groups)
    got = _launch(pkg, src, tab, mvd, C, T_out, streams, par if needs_table else None, 2)
    _same(got, want, str(streams))
    if groups == [0]:       # "j" alone is the existing launch, with a move table and without
        _same(got, joints, "j alone")
        plain = _launch(pkg, src, tab, None, C, T_out, None, None, None)
        _same(_launch(pkg, src, tab, None, C, T_out, "j", None, None), plain, "j, no moves")


def test_stage_clips_validates_x_and_parents(pkg):
    V, T_out, C = 25, 7, 3
    clips = _clips(23, _lengths(T_out), V, C, np.float32)
    src, tab, _ = _to_device(pkg, clips, T_out, C, np.float32, None, None)
    status = torch.empty(N, dtype=torch.int32, device=DEV)
    par = torch.from_numpy(_parents(pkg, V)).to(DEV)
    x = torch.empty(N, 4 * C, T_out, V, device=DEV)
    stage = pkg.data.stage_clips
    with pytest.raises(ValueError, match="multiple of the 4 streams"):
        stage(src, tab, torch.empty(N, 4 * C + 1, T_out, V, device=DEV), status, streams=FULL,
              parents=par)
    for bad in (None, par.long(), par[:-1], par.cpu(), torch.cat([par, par])[::2]):
        with pytest.raises(ValueError, match=f"int32 tensor of {V} entries"):
            stage(src, tab, x, status, streams=FULL, parents=bad)
    # a table given without a bone stream is checked too, though not used
    xj = torch.empty(N, 2 * C, T_out, V, device=DEV)
    with pytest.raises(ValueError, match=f"int32 tensor of {V} entries"):
        stage(src, tab, xj, status, streams="j+jm", parents=par[:-1])
    stage(src, tab, xj, status, streams="j+jm", parents=par)
    with pytest.raises(ValueError, match=f"parents holds {V} entries"):
        pkg.data.RaggedDeviceLoader([], DEV, V, C, C, T_out=T_out, streams="j+jm",
                                    parents=np.zeros(V - 1, dtype=np.int32))
    with pytest.raises(ValueError, match="go with streams"):
        stage(src, tab, x[:, :C].contiguous(), status, parents=par)
    with pytest.raises(RuntimeError, match="score_channel"):      # the library's own check
        stage(src, tab, x, status, streams=FULL, parents=par, score_channel=1)


def test_edges(pkg):
    # T_out = 1: the motion streams are all zero, whatever the clip lengths
    V, C = 25, 3
    clips = _clips(31, (1, 4, 1), V, C, np.float64)
    par = _parents(pkg, V)
    src, tab, _ = _to_device(pkg, clips, 1, C, np.float64, (MATRIX, None, None), None)
    plain = _launch(pkg, src, tab, None, C, 1, None, None, None)
    got = _launch(pkg, src, tab, None, C, 1, FULL, par, None)
    _same(got, pkg.data.streams_reference(plain, par, FULL), "T_out = 1")
    assert not got[:, 2 * C:].any() and got[:, :C].all()
    # one-frame clips padded to T_out = 7: every frame is that frame, the
    # coordinates' motion is +0 and the score's mean is the score
    clips = _clips(32, (1, 7, 1), V, C, np.float32)
    moves = _moves(pkg, 33, (0, 2, 0), 7)
    src, tab, mvd = _to_device(pkg, clips, 7, C, np.float32, None, moves)
    joints = _launch(pkg, src, tab, mvd, C, 7, None, None, None)
    got = _launch(pkg, src, tab, mvd, C, 7, FULL, par, 2)
    _same(got, pkg.data.streams_reference(joints, par, FULL, score_channel=2), "one frame")
    assert not got[0, 2 * C:2 * C + 2].any() and not np.signbit(got[0, 2 * C:2 * C + 2]).any()
    assert np.array_equal(got[0, 2 * C + 2, :6], joints[0, 2, :6])
    # V = 50: two persons, two roots
    V = 50
    par = _parents(pkg, V)
    assert par[1] == 1 and par[26] == 26
    clips = _clips(34, _lengths(7), V, 2, np.float32)
    moves = _moves(pkg, 35, (4, 2, 3), 7)
    src, tab, mvd = _to_device(pkg, clips, 7, 2, np.float32, (None, MATRIX, None), moves)
    joints = _launch(pkg, src, tab, mvd, 2, 7, None, None, None)
    got = _launch(pkg, src, tab, mvd, 2, 7, FULL, par, None)
    _same(got, pkg.data.streams_reference(joints, par, FULL), "V = 50")
    assert not got[:, 2:4, :, [1, 26]].any() and got[:, 2:4, :, [0, 25, 27]].all()


def test_one_joint_fills_the_frame_table(pkg):
    """V = 1, T_out = 300, parents = [0], with a move: a workgroup's 256 points
    and their successors lie in 257 frames, the most the LDS frame table holds;
    the second workgroup starts at frame 256."""
    V, T_out, C = 1, 300, 2
    clips = _clips(41, (297, 300, 305), V, C, np.float64)
    moves = _moves(pkg, 42, (4, 2, 3), T_out)
    src, tab, mvd = _to_device(pkg, clips, T_out, C, np.float64, (MATRIX, None, None), moves)
    joints = _launch(pkg, src, tab, mvd, C, T_out, None, None, None)
    got = _launch(pkg, src, tab, mvd, C, T_out, FULL, [0], None)
    _same(got, pkg.data.streams_reference(joints, [0], FULL), "V = 1")
    assert not got[:, C:2 * C].any() and not got[:, 3 * C:].any()   # a root's bone is +0
    assert got[:, 2 * C:3 * C, :T_out - 1].all()


@pytest.mark.parametrize("entry", [-1, 25, 2 ** 31 - 1])
def test_bad_parents_zero_everything(pkg, entry):
    """An entry outside [0, V), also in the last slot: status 4 on every clip
    beside the unchanged bits 0 and 1, x all zeros; a good table keeps bits 0
    and 1 and the neighbours' values."""
    V, T_out, C = 25, 20, 3
    clips = _clips(51, _lengths(T_out), V, C, np.float32)
    moves = _moves(pkg, 52, (2, 4, 3), T_out)
    par = _parents(pkg, V)
    src, tab, mvd = _to_device(pkg, clips, T_out, C, np.float32, (MATRIX, None, None), moves)
    clean = _launch(pkg, src, tab, mvd, C, T_out, FULL, par, 2)
    bad = par.copy()
    bad[24 if entry == 25 else 7] = entry
    got = _launch(pkg, src, tab, mvd, C, T_out, FULL, bad, 2, want_status=[4, 4, 4])
    assert not got.any() and not np.signbit(got).any()
    got = _launch(pkg, src, tab, mvd, C, T_out, "jm+b", bad, 2, want_status=[4, 4, 4])
    assert not got.any()
    # without a bone stream the table is not read
    got = _launch(pkg, src, tab, mvd, C, T_out, "j+jm", None, 2)
    _same(got, np.concatenate([clean[:, :C], clean[:, 2 * C:3 * C]], axis=1), "no table")
    # a bad clip entry and a bad move record still give 1 and 2
    buf, table, _ = pkg.data.pack_clips([(c, np.array([0])) for c in clips], T_out, C,
                                        np.float32, transforms=np.asarray(
                                            [MATRIX, np.eye(3), np.eye(3)]))
    table["frames"][1] = 0
    moves["nk"][2] = 1
    tab2 = torch.from_numpy(table.view(np.uint8).copy()).to(DEV)
    mvd2 = torch.from_numpy(moves.view(np.uint8).copy()).to(DEV)
    got = _launch(pkg, src, tab2, mvd2, C, T_out, FULL, par, 2, want_status=[0, 1, 2])
    assert not got[1].any() and not got[2].any()
    _same(got[0], clean[0], "the valid neighbour")
    got = _launch(pkg, src, tab2, mvd2, C, T_out, FULL, bad, 2, want_status=[4, 5, 6])
    assert not got.any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_streams_poisoned(pkg, dtype):
    """x and status start as the fill inside guard bands; src, the tables and
    parents are guarded inputs: no guard byte moves, no input changes, and every
    element of x and status is written."""
    V, T_out, C = 25, 7, 3
    clips = _clips(13, _lengths(T_out), V, C, dtype)
    Ms = (MATRIX, None, MATRIX)
    moves = _moves(pkg, 3, (4, 2, 0), T_out)
    par = _parents(pkg, V)
    src, tab, mvd = _to_device(pkg, clips, T_out, C, dtype, Ms, moves)
    clean = _launch(pkg, src, tab, mvd, C, T_out, FULL, par, 2)
    for fill in poison.FILLS:
        with poison.poisoned(pkg, fill):
            src, tab, mvd = _to_device(
                pkg, clips, T_out, C, dtype, Ms, moves,
                place=lambda t, name: poison.guarded(t, fill, DEV, name=name))
            pard = poison.guarded(torch.from_numpy(par), fill, DEV, name="parents")
            x = poison.empty((N, 4 * C, T_out, V), fill, device=DEV, name="x")
            status = poison.empty(N, fill, dtype=torch.int32, device=DEV, name="status")
            pkg.data.stage_clips(src, tab, x, status, moves=mvd, streams=FULL, parents=pard,
                                 score_channel=2)
            torch.cuda.synchronize()
        poison.check_guards()
        poison.check_inputs()
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(clean)), f"fill {fill:#04x}"
        assert status.tolist() == [0, 0, 0], f"fill {fill:#04x}"


def test_streams_in_a_captured_graph(pkg):
    """One captured launch; src, both tables and parents are rewritten between
    two replays: each replay equals the eager launch on the same buffers."""
    V, T_out, C = 25, 20, 3
    src = torch.zeros(N * T_out, V, C, device=DEV)
    tab = torch.zeros(N * 48, dtype=torch.uint8, device=DEV)
    mvd = torch.zeros(N * 160, dtype=torch.uint8, device=DEV)
    pard = torch.zeros(V, dtype=torch.int32, device=DEV)
    x = torch.zeros(N, 4 * C, T_out, V, device=DEV)
    status = torch.zeros(N, dtype=torch.int32, device=DEV)
    tables = (_parents(pkg, V), pkg.graph.parents(pkg.graph.graph_for(V), roots=[0]))
    assert not np.array_equal(*tables)

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
        pard.copy_(torch.from_numpy(tables[i]))

    def launch(out, st):
        pkg.data.stage_clips(src, tab, out, st, moves=mvd, streams=FULL, parents=pard,
                             score_channel=2)

    fill(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # (one launch before the capture, as torch asks)
        launch(x, status)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(x, status)
    seen = []
    for i in (1, 0):
        fill(i)
        x.fill_(float("nan"))
        status.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        got = x.cpu().numpy().copy()
        assert status.tolist() == [0, 0, 0]
        eager = torch.full_like(x, float("nan"))
        launch(eager, torch.empty_like(status))
        _same(got, eager.cpu().numpy(), f"replay of tables {i}")
        joints = torch.empty(N, C, T_out, V, device=DEV)
        pkg.data.stage_clips(src, tab, joints, torch.empty_like(status), moves=mvd)
        _same(got, pkg.data.streams_reference(joints.cpu().numpy(), tables[i], FULL,
                                              score_channel=2), f"reference of tables {i}")
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1])


@pytest.mark.parametrize("static", [False, True], ids=["fresh", "out="])
def test_loader_streams(pkg, static):
    """RaggedDeviceLoader(streams="j+b+jm+bm", augment, move, crop="random") over
    two batches under a seed equals stage_clips on the same draws, bit for bit,
    with the graph's default parents; also into out= / labels_out=."""
    V, C_src, C, T_out = 25, 3, 2, 20
    batches = _batches(V, C_src, np.float64, T_out)
    par = torch.from_numpy(_parents(pkg, V)).to(DEV)
    random.seed(6)
    np.random.seed(6)
    want = []
    for items in batches:
        tr = pkg.data.clip_transforms(N)
        mv = pkg.data.clip_moves(N, T_out)
        buf, table, labels = pkg.data.pack_clips(items, T_out, C_src, np.float64, transforms=tr,
                                                 crop="random")
        x = torch.empty(N, 4 * C, T_out, V, device=DEV)
        status = torch.empty(N, dtype=torch.int32, device=DEV)
        pkg.data.stage_clips(torch.from_numpy(buf).to(DEV),
                             torch.from_numpy(table.view(np.uint8).copy()).to(DEV), x, status,
                             moves=torch.from_numpy(mv.view(np.uint8).copy()).to(DEV),
                             streams=FULL, parents=par)
        assert status.tolist() == [0] * N
        want.append((x.cpu().numpy(), labels.tolist()))
    random.seed(6)
    np.random.seed(6)
    kw = {}
    if static:
        kw = dict(out=torch.full((N, 4 * C, T_out, V), float("nan"), device=DEV),
                  labels_out=torch.full((N,), -1, dtype=torch.int64, device=DEV))
    loader = pkg.data.RaggedDeviceLoader(batches, DEV, V, C, C_src, T_out=T_out,
                                         src_dtype=torch.float64, augment=True, move=True,
                                         crop="random", streams=FULL, **kw)
    seen = 0
    for (x, y), (wx, wy) in zip(loader, want):
        if static:
            assert x is kw["out"] and y is kw["labels_out"]
        assert tuple(x.shape) == (N, 4 * C, T_out, V) and y.tolist() == wy
        _same(x.cpu().numpy(), wx, f"batch {seen}")
        seen += 1
    assert seen == 2
    # out= is validated against S * C channels
    with pytest.raises(ValueError, match=rf"\(N, {4 * C}, {T_out}, {V}\)"):
        pkg.data.RaggedDeviceLoader(batches, DEV, V, C, C_src, T_out=T_out, streams=FULL,
                                    out=torch.empty(N, C, T_out, V, device=DEV))


def test_loader_reports_an_invalid_parents_table_once(pkg):
    V, C_src, C, T_out = 25, 3, 3, 20
    batches = _batches(V, C_src, np.float32, T_out)
    bad = _parents(pkg, V)
    bad[3] = V
    it = iter(pkg.data.RaggedDeviceLoader(batches, DEV, V, C, C_src, T_out=T_out, streams="j+b",
                                          parents=bad))
    seen = []
    with pytest.raises(RuntimeError, match="invalid parents table"):
        while True:
            try:
                x, _ = next(it)
            except StopIteration:
                break
            seen.append(x.cpu().numpy())
    assert len(seen) == 2 and not seen[0].any() and not seen[1].any()


@pytest.mark.parametrize("f32_gemm,streams", [("mfma", "j"), ("f16x2", "j"), ("f16x2", "j+b")])
def test_stream_input_trains_the_stack(pkg, f32_gemm, streams):
    """End to end: the loader's input (C = 2, N = 2, T_out = 16, V = 18) through
    STGCNStack.forward_loss and backward, compared the way test_gpu_stack.py
    compares a stack step with the oracle: logits and loss against the fp64
    oracle differentiated through the run's ReLU masks, gradients per tensor at
    max(1e-4, 3x the fp32 oracle's own error).

    The two-stream input "j+b" (C_in = 4) runs on the benched f16x2 path only:
    on the exact-fp32 "mfma" path it missed this gate on two deep tensors
    (conv.8.spatialConv.A 2.96e-4 against 2.58e-4, conv.9.spatialConv.A 1.83e-4
    against 1.63e-4), so that path is held to the single stream (C_in = C); the
    figures at the other widths are in DESIGN.md, "Bone and motion streams"."""
    V, C, T_out, n, classes = 18, 2, 16, 2, 5
    S = streams.count("+") + 1
    clips = _clips(71, (11, 23), V, 3, np.float32)
    items = [(c, np.array([i + 1])) for i, c in enumerate(clips)]
    random.seed(7)
    np.random.seed(7)
    loader = pkg.data.RaggedDeviceLoader([items], DEV, V, C, 3, T_out=T_out, augment=True,
                                         move=True, streams=streams)
    (x, lab), = list(loader)
    assert tuple(x.shape) == (n, S * C, T_out, V)
    gr = pkg.graph
    A = gr.get_normalized_adjacency_matrices(0, 1, graph=gr.graph_for(V))
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = pkg.STGCNStack(S * C, classes, A, f32_gemm=f32_gemm)
    p0, b0 = snapshot_stack(model)
    model = model.cuda().train()
    masks, unhook = capture_relu_masks(model)
    loss, logits = model.forward_loss(x, lab)
    loss.backward()
    torch.cuda.synchronize()
    unhook()
    x_ntvc = x.detach().cpu().permute(0, 2, 3, 1).contiguous()
    l64, loss64, g64, pre64 = oracle_through_masks(p0, b0, x_ntvc, lab.cpu(), masks,
                                                   torch.float64)
    _, _, g32, _ = oracle_through_masks(p0, b0, x_ntvc, lab.cpu(), masks, torch.float32)
    err = rel_to_max(logits.detach().cpu().numpy(), l64.numpy())
    print(f"C_in = {S * C} {f32_gemm}: logits {err:.2e}, loss {loss.item() - loss64.item():.2e}")
    assert err < 1e-4
    assert abs(loss.item() - loss64.item()) < 1e-5
    check_relu_ties(pre64, masks)
    for k, v in model.named_parameters():
        if k.endswith("temporalConv.bias"):
            assert v.grad.abs().max().item() < 1e-5, k
    gate_stack_grads(model, g64, g32)
