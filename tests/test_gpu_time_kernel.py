"""The measurement entry point stgcn_time_kernel (st-gcn_amd/csrc/capi.hip
plan_timed; bench.py --full and scripts/kbench*.py call it): one descriptor per
kernel path, every `which` 0..6.

For each: stgcn_time_kernel_bytes is 0 exactly where the call answers
STGCN_E_UNSUPPORTED; every other call succeeds, reports a finite positive
time, and the algorithmic FLOPs of the comment block above plan_timed
(SURVEY.md section 8d terms), restated here from the descriptor and the
stgcn_block_plan bits:

  tconv   = 2 * 9 * C_out * CZ * T_out * V * N,  CZ = C_in folded, else C_out
  gemm    = 2 * K * C_in * C_out * T * V * N     (W' G, or H = W'^T dZ)
  joint   = 2 * K * C_in * T * V^2 * N           (one contraction with A)
  which 0 : tconv (+ 2 * K * C_out * T_out * V^2 * N without G: the forward's
            joint contraction runs in this kernel's epilogue)
        1 : tconv (+ 2 joint where the data gradient carries the spatial backward)
        2 : tconv
        3 : gemm (+ joint in the fused bf16 spatial forward)
        4 : gemm + 2 joint (no gemm on the folded block: H is there already)
        5 : gemm;   6 : 2 joint;   V = 50 fused, 5 and 6: gemm + joint each
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

N, T = 2, 24
CASES = {
    # name: (C_in, C_out, V, K, stride, make_desc flags)
    "fp32_s2": (16, 32, 18, 1, 2, {}),
    "f32x3_fold_s1": (16, 32, 18, 1, 1, {"f32x3": True}),
    "f32x3_fold_s2": (16, 32, 18, 1, 2, {"f32x3": True}),
    "f16x2_s1": (16, 32, 18, 1, 1, {"f16x2": True}),
    "f16x2_nog_s1": (16, 32, 18, 1, 1, {"no_g": True}),
    "f16x2_first_block": (3, 16, 18, 1, 1, {"f16x2": True}),
    "f32x3_fold_v25": (16, 32, 25, 1, 1, {"f32x3": True}),
    "bf16_v25_k3": (16, 32, 25, 3, 1, {"bf16": True}),
    "bf16_v50_k3": (16, 32, 50, 3, 1, {"bf16": True}),
    # (C_in a multiple of 32, C_out >= 64: the fused backward pair k_sp50_dx / k_sp50_dA,
    # which 5 and 6 one of them each)
    "bf16_v50_k3_fused_bwd": (32, 64, 50, 3, 1, {"bf16": True}),
    "fp32_residual_proj_s2": (16, 32, 18, 1, 2, {"residual": True}),
}


def _want_flops(hl, d, plan, which):
    C, R, V, K, Tt, To, Nn = d.C_in, d.C_out, d.V, d.K, d.T, d.T_out, d.N
    fold = bool(plan & hl.PLAN_FOLD)
    fold_spb = fold and bool(plan & hl.PLAN_SP_BWD_FUSED)
    fused_spb = not fold and bool(plan & hl.PLAN_SP_BWD_FUSED)
    CZ = C if fold else R
    tconv = 2.0 * 9 * R * CZ * To * V * Nn
    gemm = 2.0 * K * C * R * Tt * V * Nn
    joint = 2.0 * K * C * Tt * V * V * Nn
    if which == 0:
        return tconv + (2.0 * K * R * To * V * V * Nn if plan & hl.PLAN_FOLD_NO_G else 0.0)
    if which == 1:
        return tconv + (2 * joint if fold_spb else 0.0)
    if which == 2:
        return tconv
    if which == 3:
        return gemm + (joint if plan & hl.PLAN_SP_FWD_FUSED else 0.0)
    if fused_spb and V == 50 and which >= 5:
        return gemm + joint
    return (gemm if which != 6 and not fold else 0.0) + (2 * joint if which != 5 else 0.0)


@pytest.mark.parametrize("name", list(CASES))
def test_time_kernel(pkg, name):
    hl = pkg.hip_lib
    lib = hl.lib()
    dev = torch.device("cuda", 0)
    ci, co, V, K, stride, flags = CASES[name]
    d = pkg.fused.make_desc((N, ci, T, V), co, K, stride, 4, 1e-5, 0.1, True, **flags)
    assert lib.stgcn_check_desc(ctypes.byref(d)) == 0
    plan = hl.block_plan(d)
    if name.startswith(("f32x3_fold", "f16x2_s1", "f16x2_nog")):
        assert plan & hl.PLAN_FOLD
    if name == "f16x2_nog_s1":
        assert plan & hl.PLAN_FOLD_NO_G
    if name == "f16x2_first_block":
        assert plan & hl.PLAN_F16X2 and not plan & hl.PLAN_FOLD
    if name.startswith("bf16"):
        assert plan & hl.PLAN_SP_FWD_FUSED
    if name == "bf16_v50_k3_fused_bwd":
        assert plan & hl.PLAN_SP_BWD_FUSED
    ran = 0
    for which in range(7):
        nbytes = lib.stgcn_time_kernel_bytes(ctypes.byref(d), which)
        scratch = torch.randn(nbytes // 4 + 1, device=dev)  # (as bench.py does)
        ms, fl = ctypes.c_float(float("nan")), ctypes.c_double(float("nan"))
        rc = lib.stgcn_time_kernel(ctypes.byref(d), which, hl.ptr(scratch), nbytes, 2,
                                   hl.stream_handle(dev), ctypes.byref(ms), ctypes.byref(fl))
        torch.cuda.synchronize(dev)
        print(f"{name} which {which}: bytes {nbytes} rc {rc} ms {ms.value} flops {fl.value}")
        assert (nbytes == 0) == (rc == hl.E_UNSUPPORTED), (which, nbytes, rc)
        if nbytes == 0:
            continue
        assert rc == 0, (which, lib.stgcn_last_error().decode(errors="replace"))
        assert math.isfinite(ms.value) and ms.value > 0, (which, ms.value)
        assert fl.value == _want_flops(hl, d, plan, which), (which, fl.value)
        ran += 1
    assert ran >= 3  # the three temporal GEMMs are timed on every path
