"""STGCN_FEATURE_BWD_OVERLAP on the GPU: the folded block's backward with its
small kernels (k_fold_tq, k_bn_grads_out, k_fold_red64, k_fold_small_sd,
k_dA_reduce1 / 2, k_chain_coef) on the library's side stream beside the data- and
weight-gradient GEMMs, against the same step with every launch on the caller's
stream (stgcn_bwd_overlap(0)). The kernels, their launch parameters and the order
between any two that touch the same buffer are the same, so every comparison
here is torch.equal.

The stack is the smallest that reaches every moved kernel: blocks (3, 64, 1),
(64, 64, 1), (64, 128, 2) at V = 18, K = 1, N = 3, T = 20, training, f16x2,
chained with lazy links -- a stride-1 folded block with deferred dx, a stride-2
folded block with both data-gradient phases, and the unfolded first block, which
stays serial. (A folded block whose dx does not defer -- the serial BN1 tail
after the join -- is the stand-alone block of the capture child.)

The atomics fallback (a data-gradient launch without dA partial slots joins the
side stream first, capi.hip bwd_fold_temporal) is not reachable through the
public descriptor: the workspace the call insists on holds dA_part_cap slots,
counted at 64-row tiles, and the launches use 64- or 128-row tiles, so every
phase of a fused folded block fits. That branch is covered by review.
"""
import contextlib
import copy
import io
import os
import subprocess
import sys

import pytest
import torch

import poison
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCKS = [(3, 64, 1), (64, 64, 1), (64, 128, 2)]
N, T, V, CLASSES = 3, 20, 18, 10


@pytest.fixture
def lib(pkg):
    lib = pkg.hip_lib.lib()
    assert lib.stgcn_bwd_overlap(-1) == 1  # on by default
    yield lib
    lib.stgcn_bwd_overlap(1)


def _small_stack(pkg):
    """STGCNStack's training step (StackChain, FoldPrep, lazy links, fused head)
    over BLOCKS instead of the reference's ten layers."""
    gr = pkg.graph
    A = gr.get_normalized_adjacency_matrices(0, 1, graph=gr.graph_for(V))

    class SmallStack(pkg.STGCNStack):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.dropout_seed = "host"
            self.K, self.V, self.nr_classes = A.shape[0], A.shape[1], CLASSES
            self.Masks = [torch.ones(A.shape) for _ in BLOCKS]
            self.conv = torch.nn.Sequential(*[
                pkg.SpatialTemporalConv(ci, co, A, 9, s, 4, dropout_rate=0, f32_gemm="f16x2")
                for ci, co, s in BLOCKS]).float()
            self.fc_layer = torch.nn.Linear(BLOCKS[-1][1], CLASSES).float()

    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = SmallStack()
    return m.to(DEV).train()


@pytest.fixture(scope="module")
def case(pkg):
    """The model's initial state, the input, and the serial step's results
    (computed once, shared, never modified)."""
    lib = pkg.hip_lib.lib()
    model = _small_stack(pkg)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, 3, T, V, generator=g).to(DEV)
    labels = torch.randint(0, CLASSES, (N,), generator=g).to(DEV)
    prev = lib.stgcn_bwd_overlap(0)
    try:
        ref = _step(copy.deepcopy(model), x, labels)
    finally:
        lib.stgcn_bwd_overlap(prev)
    return model, x, labels, ref


def _step(model, x, labels):
    """forward_loss + backward: the loss and every parameter gradient."""
    model.zero_grad(set_to_none=True)
    loss, _ = model.forward_loss(x, labels)
    loss.backward()
    torch.cuda.synchronize()
    res = {"loss": loss.detach().clone()}
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        res["grad." + k] = p.grad.detach().clone()
    return res


def _assert_equal(got, ref, what):
    assert got.keys() == ref.keys()
    diff = [k for k in ref if not torch.equal(got[k], ref[k])]
    assert not diff, f"{what}: not bit-identical to the serial step: {diff}"


def test_stack_reaches_the_forked_and_the_serial_paths(pkg, case):
    """Blocks 1 and 2 take the fused folded backward (the forked path), block 0
    does not fold (serial); the gradients include spatialConv.A of each."""
    model, x, _, ref = case
    hl = pkg.hip_lib
    descs = pkg.fused.stack_descs(list(model.conv), tuple(x.shape))
    plans = [hl.block_plan(d) for d in descs]
    assert not plans[0] & hl.PLAN_FOLD
    for p in plans[1:]:
        assert p & hl.PLAN_FOLD and p & hl.PLAN_SP_BWD_FUSED and p & hl.PLAN_F16X2, hex(p)
    assert descs[2].stride == 2 and descs[2].T == T  # both data-gradient phases
    for i in range(len(BLOCKS)):
        assert f"grad.conv.{i}.spatialConv.A" in ref
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())


def test_overlapped_equals_serial(lib, case):
    model, x, labels, ref = case
    lib.stgcn_bwd_overlap(0)
    _assert_equal(_step(copy.deepcopy(model), x, labels), ref, "serial again")
    lib.stgcn_bwd_overlap(1)
    _assert_equal(_step(copy.deepcopy(model), x, labels), ref, "overlapped")


def test_overlapped_with_poisoned_buffers(pkg, lib, case):
    """Workspaces, saved tensors and gradient buffers start out as the fill: a
    kernel that runs ahead of its producer reads poison, and it shows in a
    gradient -- three runs, three fills."""
    model, x, labels, ref = case
    lib.stgcn_bwd_overlap(1)
    for fill in poison.FILLS:
        m = copy.deepcopy(model)
        with poison.poisoned(pkg, fill):
            got = _step(m, x, labels)
            poison.check_guards()
        assert poison.allocations(), "the poison reached no buffer"
        _assert_equal(got, ref, f"overlapped, fill {fill:#04x}")


def test_overlapped_on_a_non_default_stream(lib, case):
    model, x, labels, ref = case
    lib.stgcn_bwd_overlap(1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = _step(copy.deepcopy(model), x, labels)
    torch.cuda.current_stream().wait_stream(s)
    _assert_equal(got, ref, "overlapped on a non-default stream")


def test_graphed_overlapped_step_equals_eager_serial(pkg, lib, case):
    """GraphedStep(warmup=1) + 3 replays with the fork captured (two parallel
    branches per folded block) against 4 eager serial steps from the same start."""
    model, x, labels, _ = case

    def make():
        m = copy.deepcopy(model)
        opt = pkg.FusedAdam(list(m.parameters()), lr=1e-3, capturable=True)

        def step():
            opt.zero_grad(set_to_none=True)
            loss, logits = m.forward_loss(x, labels)
            loss.backward()
            opt.step()
            return loss, logits
        return m, step

    ma, step_a = make()
    mb, step_b = make()
    lib.stgcn_bwd_overlap(0)
    for _ in range(4):
        la, ga = step_a()
    torch.cuda.synchronize()
    lib.stgcn_bwd_overlap(1)
    graphed = pkg.GraphedStep(step_b, warmup=1)
    for _ in range(3):
        lb, gb = graphed()
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    for (ka, a), (kb, b) in zip(ma.state_dict().items(), mb.state_dict().items()):
        assert ka == kb
        assert torch.equal(a, b), ka


def test_capture_before_the_side_stream_exists_runs_serially():
    """A fresh process whose first library calls are a block's forward and
    backward under torch.cuda.graph: nothing is created during the capture, the
    call runs serially, and the replay equals the eager step that follows
    (tests/bwd_overlap_worker.py)."""
    cmd = [sys.executable, os.path.join(ROOT, "tests", "bwd_overlap_worker.py")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bwd_overlap_worker ok" in r.stdout, r.stdout[-3000:]
