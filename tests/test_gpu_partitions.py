"""GPU parity of the fused block over the adjacency partition counts K = 1..4
at V = 18, 25 and 50, against the fp64 oracle.

The library picks its spatial kernels by (V, K); the other GPU tests run
(18, 1), (25, 3) and (50, 3) (and K = 1 at V = 25 / 50 in a few places). Here A
is the reference's own adjacency for its other strategies (tests/golden/
adjacency.npz, key ``V<V>_s<strategy>_d<depth>``: distance s1 gives K = d + 1,
spatial s2 K = 3, symmetrical s3 K = d + 1, uni-labelling s0 K = 1), and for
K = 4 the distance strategy at depth 3 from the package's graph module. The
shapes are the smallest that still split the dispatch conditions (C * T a
multiple of 256 / 128 / 64 / none of them, element count a multiple of 4 or
not, K <= 3 or not).

Case -> kernels, read from the dispatch (kernels.hip launch_gather_fwd /
launch_bwd56 / launch_spatial_dx, kernels_fused.hip launch_sp_fwd_bf16, capi.hip
fused_sp / fused_spb):

  a  V18 K2 C*T=768   k_gather4<18> (K = 2), k_spatial_bwd5<18,128,2>;
                      bf16: k_sp_fwd_bf16<18,2>, kept bf16 G, H GEMM over
                      K*C_in = 128 rows, bwd5
  b  V18 K2 C*T=1344  k_gather3<18>, k_spatial_bwd5<18,64,2>
  c  V18 K3 stride 2  k_spatial_bwd5<18,64,3>; bf16: k_sp_fwd_bf16<18,3>
  d  V18 K3 (d = 2)   k_gather4<18> (K = 3), k_spatial_bwd5<18,128,3>
  e  V18 K3 C_in=3    2430 elements (not a multiple of 4): k_sum_nt,
                      k_spatial_bwd3<18>
  f  V25 K2 C*T=768   k_gather_mfma<25,2>, k_spatial_bwd5<25,128,2>;
                      bf16: k_sp_fwd_bf16<25,2>
  g  V25 K2 C*T=352   symmetrical; no bwd5 (C*T not a multiple of 64):
                      k_spatial_bwd3<25> at K = 2
  h  V25 K2 C*T=1344  k_gather_mfma refuses (not a multiple of 128):
                      k_gather3<25>, k_spatial_bwd5<25,64,2>
  i  V25 K2 C_in=3    3375 elements: the unaligned fallbacks at K = 2
  j  V25 K1 (d = 2)   two-hop uni-labelling; bf16: k_sp_fwd_bf16<25,1> with
                      k_spatial_bwd5<25,*,1>; split modes: the folded block
  k  V50 K2           k_gather_mfma<50,2>, k_spatial_bwd6<50,2,false>; bf16:
                      unfused gather + bf16 W' GEMM, k_spatial_bwd6<50,2,true>
  l  V50 K1           k_gather4<50> (K = 1), k_spatial_bwd6<50,1,*> at 64 channels
  m  V50 K2 C_in=3    first block at V = 50, K = 2
  n  V18 K4           K > 3: generic k_spatial_dx, k_gather4<18> with K = 4,
                      stacked W' / H GEMMs over K*C_in = 256 rows
  o  V25 K4           the same at V = 25 (both k_gather_mfma instances refuse)

launch_spatial_small runs in every case. The stacked W' weight gradient over
K * C_in rows is k_wgrad_sp in the fp32 and split runs of the unfolded cases
(all but j, which folds and has none), on split products in the split modes
(a, c, f, h, n); the bf16 runs with the fused forward (a, b, c, f, g, j) form
dW' from the kept bf16 G instead (k_wgrad_gemm_gk).

Gates, unchanged from test_gpu_block.py / test_gpu_bf16.py: fp32 modes
max(1e-5, 2 x the fp32 oracle's own error), bf16 max(2e-2, 3 x the bf16-operand
oracle's error) plus the fp32-path band. So that those floors cannot widen a
gate unnoticed, each test also caps them (reasoned from CPU measurements with
the oracle's own ReLU mask, 8 threads):

  fp32, non-residual  floor <= 1e-5 on every tensor (worst measured 4.1e-6,
                      case e grad.spatialConv.W.bias): no gate above 2e-5
  fp32, residual      only grad.spatialConv.W.bias above 1e-5 (measured
                      2.0e-5 / 4.2e-5 / 1.9e-4), and <= 1e-3: the margin is
                      for the thread-count-dependent fp32 summation order
  bf16, non-residual  floor <= 1e-2 on every tensor (worst measured 8.3e-3,
                      case i grad.batch_n.weight): no gate above 3e-2
  bf16, residual      the floor follows the GPU run's inner ReLU mask; the
                      measured worst floor and its tensor are recorded in
                      RES_BF16_FLOOR; that tensor's floor must stay within a
                      factor 2 of it either way, and no tensor's may pass 2x

Case m is left out of the bf16 runs: its bf16-operand reference error on y
alone is 1.1e-2, which would widen its gate to 3.4e-2.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import load_npz
from partition_cases import BF16, CASES, D3, MATRIX, NO_DX, RESIDUAL, SPLIT
from test_gpu_bf16 import _check_bf16
from test_gpu_block import _compare, _oracle, _random_case, _run_hip

pytestmark = pytest.mark.gpu

FP32_FLOOR_CAP = 1e-5
RES_BIAS_FLOOR_CAP = 1e-3
BF16_FLOOR_CAP = 1e-2
# worst bf16-operand oracle error over the tensors of the residual bf16 cases and
# the tensor that has it, through the GPU run's ReLU masks (MI355X, seed 0)
RES_BF16_FLOOR = {"a": ("grad.batch_n.weight", 4.6e-3), "k": ("grad.batch_n_2.weight", 5.8e-3),
                  "r": ("grad.batch_n.bias", 4.2e-3)}


@functools.lru_cache(maxsize=None)
def _golden_adjacency():
    return load_npz("adjacency.npz")


def adjacency(pkg, V, key):
    """The (K, V, V) adjacency of a case: the reference's own tensor by key, or
    the distance strategy at depth 3 (K = 4) from the package's graph module."""
    if key == D3:
        gr = pkg.graph
        return gr.get_normalized_adjacency_matrices(1, 3, graph=gr.graph_for(V))
    return torch.from_numpy(_golden_adjacency()[f"V{V}_{key}"])


def _case(pkg, cid, residual=False):
    C_in, C_out, stride, V, key, K, N, T = CASES[cid]
    A = adjacency(pkg, V, key)
    assert tuple(A.shape) == (K, V, V), (cid, tuple(A.shape))
    return _random_case(pkg, C_in, C_out, stride, V, K, N, T, residual=residual, A=A)


def _plan(pkg, cid, gemm, residual=False, need_dx=True):
    C_in, C_out, stride, V, _, K, N, T = CASES[cid]
    return pkg.hip_lib.block_plan(pkg.fused.make_desc(
        (N, C_in, T, V), C_out, K, stride, 4, 1e-5, 0.1, True, need_dx=int(need_dx),
        residual=residual, **pkg.fused._gemm_flags(gemm)))


def _cap_fp32_floor(floor, residual):
    """The fp32 oracle's own error stays small enough that no gate widens past
    2e-5 (residual: the spatial bias gradient alone, to 2e-3)."""
    bad = {}
    for k, f in floor.items():
        if not residual and k == "grad.temporalConv.bias":
            continue  # analytically 0: gated in absolute terms ("abs:" + k)
        if residual and k.startswith("abs:"):
            continue  # (a real gradient there: its relative error is capped)
        cap = RES_BIAS_FLOOR_CAP if residual and k == "grad.spatialConv.W.bias" else FP32_FLOOR_CAP
        if not f <= cap:
            bad[k] = (f, cap)
    assert not bad, f"fp32 oracle error above its cap: {bad}"


def _check_fp32(pkg, cid, gemm="fp32", residual=False, need_dx=True):
    arrays, x, g = _case(pkg, cid, residual)
    got = _run_hip(pkg, arrays, x, g, need_dx=need_dx, gemm=gemm)
    want, floor = _oracle(arrays, got)
    print(cid, gemm, "fp32-oracle floors",
          {k: float(np.format_float_scientific(v, 2)) for k, v in floor.items()})
    _cap_fp32_floor(floor, residual)
    if not need_dx:
        want.pop("grad.x")
    _compare(got, want, residual=residual, floor=floor)
    return arrays, x, g, got


def _check_bf16_case(pkg, cid, residual=False, need_dx=True):
    C_in, C_out, stride, V, key, K, N, T = CASES[cid]
    floor = {}
    errs = _check_bf16(pkg, (C_in, C_out, stride, V, K, N, T), residual=residual,
                       need_dx=need_dx, A=adjacency(pkg, V, key), floor_out=floor)
    fmt = lambda d: {k: float(np.format_float_scientific(v, 2)) for k, v in d.items()}  # noqa: E731
    print(cid, "bf16 errors", fmt(errs))
    print(cid, "bf16-operand oracle floors", fmt(floor))
    return floor


@pytest.mark.parametrize("cid", MATRIX)
def test_partition_block_fp32(pkg, cid):
    _check_fp32(pkg, cid)


@pytest.mark.parametrize("gemm", ["f32x3", "f16x2"])
@pytest.mark.parametrize("cid", SPLIT)
def test_partition_block_split(pkg, cid, gemm):
    """The fp32 split modes at K > 1: the block does not fold, the stacked
    spatial weight gradient (K * C_in rows) runs on split products and the
    temporal GEMMs on k_conv_x3 (V = 18 also k_wgrad_x3); case j (K = 1) folds,
    with the 2-way fp16 splits under f16x2. Wherever the plan names a split
    kernel its result differs from the exact fp32 MFMA run of the same inputs."""
    hl = pkg.hip_lib
    arrays, x, g, got = _check_fp32(pkg, cid, gemm=gemm)
    ref = _run_hip(pkg, arrays, x, g, gemm="fp32")
    C_in, C_out, stride, V, _, K, N, T = CASES[cid]
    plan = _plan(pkg, cid, gemm)
    assert plan & hl.PLAN_TCONV_SPLIT, plan
    if K == 1:
        assert plan & hl.PLAN_FOLD and not plan & hl.PLAN_WSP_SPLIT, plan
        assert bool(plan & hl.PLAN_F16X2) == (gemm == "f16x2"), plan
    else:
        assert not plan & hl.PLAN_FOLD and plan & hl.PLAN_WSP_SPLIT, plan
        assert not plan & hl.PLAN_F16X2, plan   # (the fp16 splits are K = 1 only)
        assert bool(plan & hl.PLAN_TWGRAD_SPLIT) == (V == 18), plan
    # stride 1: the forward runs k_conv_x3; stride 2: the data-gradient phases
    key = "y" if stride == 1 else "grad.x"
    assert not torch.equal(got[key], ref[key]), "the split temporal GEMMs did not run"
    if plan & hl.PLAN_WSP_SPLIT:
        k = "grad.spatialConv.W.weight"
        assert not torch.equal(got[k], ref[k]), "the split spatial weight gradient did not run"
    if plan & hl.PLAN_TWGRAD_SPLIT:
        k = "grad.temporalConv.weight"
        assert not torch.equal(got[k], ref[k]), "k_wgrad_x3 did not run"


@pytest.mark.parametrize("cid", BF16)
def test_partition_block_bf16(pkg, cid):
    floor = _check_bf16_case(pkg, cid)
    bad = {k: f for k, f in floor.items() if not f <= BF16_FLOOR_CAP}
    assert not bad, f"bf16-operand oracle error above {BF16_FLOOR_CAP}: {bad}"
    hl = pkg.hip_lib
    C_in, _, _, V, _, K, _, _ = CASES[cid]
    plan = _plan(pkg, cid, "bf16")
    # the fused forward at V = 18 / 25 with K <= 3 from 16 channels on; never the
    # fused backward (V = 25 / 50 with K = 3 only)
    assert bool(plan & hl.PLAN_SP_FWD_FUSED) == (V in (18, 25) and K <= 3 and C_in >= 16), plan
    assert not plan & hl.PLAN_SP_BWD_FUSED, plan


@pytest.mark.parametrize("cid", RESIDUAL)
def test_partition_residual_block_fp32(pkg, cid):
    """Residual blocks at K = 2: identity (a, k) and the strided projection (r)."""
    _check_fp32(pkg, cid, residual=True)


@pytest.mark.parametrize("gemm", ["fp32", "f32x3", "f16x2"])
def test_partition_block_stride2_v18_k2(pkg, gemm):
    """The 64 -> 128 stride-2 block at V = 18 with two partitions (the shape of
    the reference's K = 1 block fixture; the reference's own K = 2 fixture of
    this block has 64 output channels, block_b64x64s2_v18k2.npz), in every fp32
    GEMM mode: k_gather3<18> and k_spatial_bwd5<18,64,2> (C * T = 832)."""
    _check_fp32(pkg, "s", gemm=gemm)


@pytest.mark.parametrize("cid", RESIDUAL)
def test_partition_residual_block_bf16(pkg, cid):
    """Measured worst bf16-operand oracle floors, through the GPU run's ReLU
    masks: a 4.6e-3 (grad.batch_n.weight), k 5.8e-3 (grad.batch_n_2.weight),
    r 4.2e-3 (grad.batch_n.bias), the numbers RES_BF16_FLOOR asserts. All are
    below 2e-2 / 3, so the gate is the flat 2e-2. The recorded tensor's floor
    must stay within a factor 2 of its value in both directions (a floor that
    collapses means the reference no longer rounds its operands), and no
    tensor's floor may exceed twice the recorded worst."""
    floor = _check_bf16_case(pkg, cid, residual=True)
    worst = max(floor.values())
    print(cid, "worst residual bf16 floor", max(floor, key=floor.get), worst)
    assert worst <= 5e-2, "such a gate tests nothing: choose another seed"
    key, recorded = RES_BF16_FLOOR[cid]
    assert recorded / 2 <= floor[key] <= 2 * recorded, (key, floor[key], recorded)
    assert worst <= 2 * recorded, (max(floor, key=floor.get), worst, recorded)


@pytest.mark.parametrize("gemm", ["fp32", "bf16"])
@pytest.mark.parametrize("cid", NO_DX)
def test_partition_block_without_dx(pkg, cid, gemm):
    """need_dx = 0 (write_dx = 0 in bwd5 / bwd6): parameter gradients unchanged."""
    if gemm == "fp32":
        _check_fp32(pkg, cid, need_dx=False)
    else:
        floor = _check_bf16_case(pkg, cid, need_dx=False)
        assert max(floor.values()) <= BF16_FLOOR_CAP, floor


def test_partition_v50_k4_is_refused(pkg):
    """K * V * V = 10000 > 8192 (the generic spatial kernels keep A and dA in
    LDS): refused up front with STGCN_E_UNSUPPORTED, not run."""
    with pytest.raises(RuntimeError, match=r"failed \(-2\)"):
        pkg.hip_lib.block_plan(pkg.fused.make_desc((2, 64, 8, 50), 64, 4, 1, 4, 1e-5, 0.1, True))
