"""The fresh process of tests/test_gpu_bwd_overlap.py: the FIRST launches of the
library are one folded block's forward and backward under torch.cuda.graph, so
the backward arrives under stream capture before the device's side stream
exists. It must create nothing during the capture and run serially; the capture
must end (no un-joined work) and replay. The replayed results then equal the
same step run eagerly afterwards, overlapped (the call that creates the side
stream; a stand-alone block, so its dx does not defer and the BN1 tail runs
serially after the join) and serial. Prints "bwd_overlap_worker ok".
"""
import contextlib
import copy
import io
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stgcn_loader import load  # noqa: E402


def results(blk, x):
    res = {"dx": x.grad.detach().clone()}
    for k, p in blk.named_parameters():
        res[k] = p.grad.detach().clone()
    return res


def eager(blk, x0, g):
    x = x0.clone().requires_grad_(True)
    y = blk(x)
    y.backward(g)
    torch.cuda.synchronize()
    return dict(results(blk, x), y=y.detach().clone())


def main():
    pkg = load()
    dev = torch.device("cuda:0")
    gr = pkg.graph
    A = gr.get_normalized_adjacency_matrices(0, 1, graph=gr.graph_for(18))
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        blk0 = pkg.SpatialTemporalConv(64, 64, A, 9, 1, 4, dropout_rate=0, f32_gemm="f16x2")
    blk0 = blk0.to(dev).train()
    gen = torch.Generator().manual_seed(5)
    x0 = torch.randn(3, 64, 20, 18, generator=gen).to(dev)
    g = torch.randn(3, 64, 20, 18, generator=gen).to(dev)
    lib = pkg.hip_lib.lib()
    assert lib.stgcn_bwd_overlap(-1) == 1  # on by default
    d =pkg.fused.make_desc(tuple(x0.shape), 64, 1, 1, 4, 1e-5, 0.1, True, f16x2=True)
    plan = pkg.hip_lib.block_plan(d)
    assert plan & pkg.hip_lib.PLAN_FOLD and plan & pkg.hip_lib.PLAN_SP_BWD_FUSED, hex(plan)

    blk = copy.deepcopy(blk0)
    x = x0.clone().requires_grad_(True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # the first library calls of this process
        y = blk(x)
        y.backward(g)
    graph.replay()
    torch.cuda.synchronize()
    captured = dict(results(blk, x), y=y.detach().clone())

    over = eager(copy.deepcopy(blk0), x0, g)   # creates the side stream, forks
    lib.stgcn_bwd_overlap(0)
    serial = eager(copy.deepcopy(blk0), x0, g)
    lib.stgcn_bwd_overlap(1)
    for name, got in (("captured", captured), ("overlapped", over)):
        bad = [k for k in serial if not torch.equal(got[k], serial[k])]
        assert not bad, f"{name} differs from the eager serial step: {bad}"
    assert all(bool(torch.isfinite(v).all()) for v in serial.values())
    print("bwd_overlap_worker ok")


if __name__ == "__main__":
    main()
