"""The non-finite rule on the CPU (tests/gates.py, tests/nonfinite_cases.py):

* the footprint functions against the fp64 oracle run on an indicator input,
  with BatchNorm as the identity and |W|, |A| weights (no cancellation: an
  output is positive exactly where the input element reaches it);
* the oracle alone satisfies rules (a), (b), (c) against itself -- its fp32 run
  against its fp64 run -- for every case of the GPU tests' items 1 and 2: the
  rules are attainable before any kernel is held to them."""
import numpy as np
import pytest
import torch

import gates
import nonfinite_cases as nc
from oracle import ref_cpu
from test_gpu_block import TOL, _random_case


def _positive_block(pkg, shape, residual, sparse_A):
    """Block parameters with BatchNorm as the identity (eval mode, mean 0,
    var 1 - eps), no biases and |W|, |A| weights, as fp64 tensors. sparse_A:
    the skeleton's own edges and self-loops only, asymmetric (the reference's
    normalised adjacency is dense: its footprints are the dense ones)."""
    arrays, _, _ = _random_case(pkg, *shape, residual=residual)
    p, b = ref_cpu.block_params_from_arrays(arrays, dtype=torch.float64, requires_grad=False)
    for k in p:
        if k.startswith("batch_n"):
            p[k] = torch.ones_like(p[k]) if k.endswith("weight") else torch.zeros_like(p[k])
        elif k.endswith("bias"):
            p[k] = torch.zeros_like(p[k])
        else:
            p[k] = p[k].abs()
    if sparse_A:
        V = shape[3]
        adj = pkg.graph.graph_for(V).adj_list
        keep = torch.eye(V, dtype=torch.bool)
        for v, ws in adj.items():
            for w in ws:
                keep[v, w] = not (v > w and (v + w) % 3 == 0)  # (some edges one way only)
        p["spatialConv.A"] = p["spatialConv.A"] * keep
    for k in b:
        if k.endswith("running_mean"):
            b[k] = torch.zeros_like(b[k])
        elif k.endswith("running_var"):
            b[k] = torch.full_like(b[k], 1.0 - 1e-5)
    return p, b


FOOT_SHAPES = [((64, 64, 1, 18, 1, 3, 20), False), ((64, 128, 2, 18, 1, 3, 21), False),
               ((64, 64, 1, 25, 3, 3, 20), False), ((5, 7, 1, 50, 3, 3, 9), False),
               ((64, 64, 1, 18, 1, 3, 20), True), ((64, 128, 2, 25, 3, 3, 21), True)]


@pytest.mark.parametrize("sparse_A", [True, False], ids=["sparseA", "denseA"])
@pytest.mark.parametrize("shape,residual", FOOT_SHAPES)
def test_footprints_match_the_oracle_on_an_indicator(pkg, shape, residual, sparse_A):
    C_in, C_out, stride, V, K, N, T = shape
    p, b = _positive_block(pkg, shape, residual, sparse_A)
    A = p["spatialConv.A"].numpy()
    assert (A != 0).all() == (not sparse_A)
    if sparse_A:  # (and not symmetric: a transposed footprint would show)
        assert not np.array_equal(A != 0, (A != 0).transpose(0, 2, 1))
    T_out = (T - 1) // stride + 1
    for c, t, v in nc.positions(pkg, V, T, C_in):
        x = torch.zeros(N, C_in, T, V, dtype=torch.float64)
        x[nc.CLIP, c, t, v] = 1.0
        with torch.no_grad():
            y = ref_cpu.block_forward(x, p, b, stride, residual=residual, training=False,
                                      dtype=torch.float64, return_pre_relu=True)
        sparse, dense = gates.fwd_footprint(A, stride, x.shape, C_out, (nc.CLIP, c, t, v),
                                            residual=residual)
        assert np.array_equal((y != 0).numpy(), sparse), (c, t, v)
        assert (y >= 0).all() and not (sparse & ~dense).any()
        assert (sparse != dense).any() == sparse_A
        assert dense[nc.CLIP].all(axis=(0, 2)).sum() == dense[nc.CLIP, 0, :, 0].sum() > 0
        assert not dense[[n for n in range(N) if n != nc.CLIP]].any()
    # the backward of a bad g: x = 1 keeps every ReLU of the positive block open
    edge, hub = nc.joints(pkg, V)
    for o, to, w in ((1, 0, edge), (C_out - 1, T_out // 2, hub), (0, T_out - 1, hub)):
        x = torch.ones(N, C_in, T, V, dtype=torch.float64, requires_grad=True)
        y = ref_cpu.block_forward(x, p, b, stride, residual=residual, training=False,
                                  dtype=torch.float64, return_pre_relu=True)
        g = torch.zeros_like(y)
        g[nc.CLIP, o, to, w] = 1.0
        y.backward(g)
        sparse, dense = gates.bwd_footprint(A, stride, x.shape, (nc.CLIP, o, to, w),
                                            residual=residual)
        assert np.array_equal((x.grad != 0).numpy(), sparse), (o, to, w)
        assert not (sparse & ~dense).any()


def _bad_x(case, val, pos):
    x = case[1].clone()
    x[(nc.CLIP,) + tuple(pos)] = val
    return x


@pytest.mark.parametrize("case", nc.fwd_cases(), ids=nc.case_id)
def test_oracle_meets_the_forward_rules_against_itself(pkg, case):
    shape, gemm, val, ipos = case
    C_in, C_out, stride, V, K, N, T = shape
    ec = nc.eval_case(pkg, shape)
    A = ec[3]["spatialConv.A"].numpy()
    pos = nc.positions(pkg, V, T, C_in)[ipos]
    x = _bad_x(ec, val, pos)
    want = nc.oracle_fwd(ec, x, torch.float64)
    got = nc.oracle_fwd(ec, x, torch.float32)
    clean = nc.clean_fwd(pkg, shape, torch.float64)
    sparse, dense = gates.fwd_footprint(A, stride, x.shape, C_out, (nc.CLIP,) + pos)
    assert not np.isfinite(want.numpy())[sparse].all(), "the bad element reaches the output"
    assert np.isfinite(want.numpy())[~dense].all()
    gates.check_rules("y", got, want, TOL, sparse, dense, clean=clean, clip=nc.CLIP)


@pytest.mark.parametrize("val", [nc.NAN, nc.PINF], ids=["nan", "inf"])
@pytest.mark.parametrize("where", ["active", "masked"])
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("shape", nc.BWD_SHAPES, ids=nc.case_id)
def test_oracle_meets_the_backward_rules_against_itself(pkg, shape, residual, where, val):
    C_in, C_out, stride, V, K, N, T = shape
    ec = nc.eval_case(pkg, shape, residual)
    A = ec[3]["spatialConv.A"].numpy()
    clean = nc.oracle_bwd(ec, ec[2], torch.float64)
    act, off = nc.pick_output_elements(nc.pre_relu(ec))
    pos = act if where == "active" else off
    g = ec[2].clone()
    g[pos] = val
    want = nc.oracle_bwd(ec, g, torch.float64)
    got = nc.oracle_bwd(ec, g, torch.float32, relu_mask=want["y"] > 0)
    if where == "masked":
        for k, w in want.items():
            assert torch.isfinite(w).all() and torch.equal(w, clean[k]), k
            gates.check_rules(k, got[k], w, 2 * TOL, whole=True)
        return
    sparse, dense = gates.bwd_footprint(A, stride, ec[1].shape, pos, residual=residual)
    assert not torch.isfinite(want["grad.x"]).all()
    assert np.isfinite(want["grad.x"].numpy())[~dense].all()
    gates.check_rules("grad.x", got["grad.x"], want["grad.x"], TOL, sparse, dense,
                      clean=clean["grad.x"], clip=nc.CLIP)
    for k, w in want.items():
        if k.startswith("grad.") and k != "grad.x":
            gates.check_rules(k, got[k], w, 2 * TOL, whole=True)

