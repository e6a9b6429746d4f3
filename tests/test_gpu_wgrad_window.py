"""GPU parity of the temporal weight gradient's rolling Q window
(st-gcn_amd/csrc/kernels_x3.hip k_wgrad_x3): a split keeps G's frames in an LDS
ring across its run of work items (4 output frames each), stages only the
frames an item adds, and refills the ring at its first item and at every clip
start inside the run.

The small cases of test_gpu_f16x2.py / test_gpu_f32x3.py give every split one
item, or start every split on a clip, so they never roll the window. The cases
here are the smallest where, by plan_wgrad_x3 (S = min(ceil(256 / tiles),
N ceil(M / 4)) splits of per = ceil(items / S) items), a split runs several
items (so the ring turns through its phases), crosses a clip start inside its
run, and the splits start at every offset of a clip's item sequence modulo the
ring period (4 items at stride 1, 3 at stride 2):

  C_in C_out s  N   T   tiles   S  items per
   64   64   1  8  292    2    128  584   5   64-row tiles; 73 items per clip:
                                              clip starts inside splits;
                                              trailing empty splits
  128  128   1  4  150    4     64  152   3   128-row tiles; 38 items per
                                              clip; ragged last frame tile
  256  256   1  2   75   16     16   38   3   128-row tiles, two row tiles;
                                              19 items per clip
   64  128   2 16  149    2    128  304   3   stride 2, 128-row tiles (the
                                              double buffer the ring makes room for)
   32   64   2 32  150    1    256  608   3   stride 2, 64-row tiles, one
                                              partial channel tile

Each case runs in the modes f16x2 (2-way fp16 splits), f16x2_nog (the same with
BN1 applied while staging Q) and f32x3 (3-way bf16 splits), at the same fp32
gate against the fp64 oracle as test_gpu_f16x2.py; the folded modes also check
that the plan selected the fp16 splits and that the weight gradient differs
from the bf16-split one (the kernel ran).
"""
import pytest
import torch

from test_gpu_block import _compare, _oracle, _random_case, _run_hip

pytestmark = pytest.mark.gpu

CASES = [
    # C_in, C_out, stride, V, K, N, T
    (64, 64, 1, 18, 1, 8, 292),
    (128, 128, 1, 18, 1, 4, 150),
    (256, 256, 1, 18, 1, 2, 75),
    (64, 128, 2, 18, 1, 16, 149),
    (32, 64, 2, 18, 1, 32, 150),
]
MODES = ["f16x2", "f16x2_nog", "f32x3"]
WT = "grad.temporalConv.weight"

_inputs = {}    # case -> (arrays, x, g), read-only
_oracles = {}   # (case, ReLU mask) -> (want, floor): one fp64 oracle per case unless
                # a mode lands a tie on the other side
_bf16x3_wt = {}  # case -> the f32x3 mode's weight gradient


def _case_inputs(pkg, case):
    if case not in _inputs:
        _inputs[case] = _random_case(pkg, *case)
    return _inputs[case]


def _case_oracle(case, arrays, got):
    key = (case, (got["y"] > 0).numpy().tobytes())
    if key not in _oracles:
        _oracles[key] = _oracle(arrays, got)
    return _oracles[key]


def _wgrad_plan(case):
    """(tiles, splits, items, items per split, items per clip) of plan_wgrad_x3;
    128-row tiles on the fp16 splits where C_out is a multiple of 128"""
    C_in, C_out, stride, _, _, N, T = case
    M = (T - 1) // stride + 1
    out = {}
    for mode in MODES:
        rows = 128 if mode != "f32x3" and C_out % 128 == 0 else 64
        tiles = -(-C_out // rows) * -(-C_in // 32)
        per_clip = -(-M // 4)
        items = N * per_clip
        S = max(1, min(-(-256 // tiles), items))
        out[mode] = (tiles, S, items, -(-items // S), per_clip)
    return out


@pytest.mark.parametrize("case", CASES)
def test_cases_roll_the_window(case):
    """The shapes do what the table says: several items per split, a clip start
    strictly inside some split's run, and splits that start at every offset of
    a clip's items modulo the ring period (4 items at stride 1, 3 at stride 2)."""
    for mode, (tiles, S, items, per, per_clip) in _wgrad_plan(case).items():
        assert per >= 3, (mode, per)
        starts = [s * per for s in range(S) if s * per < items]
        inside = [s0 for s0 in starts
                  if any(it % per_clip == 0 for it in range(s0 + 1, min(items, s0 + per)))]
        assert inside, (mode, "no clip start inside a split")
        nph = 4 if case[2] == 1 else 3
        assert {(s0 % per_clip) % nph for s0 in starts} == set(range(nph)), mode


@pytest.mark.parametrize("gemm", MODES)
@pytest.mark.parametrize("case", CASES)
def test_wgrad_window_block(pkg, case, gemm):
    arrays, x, g = _case_inputs(pkg, case)
    got = _run_hip(pkg, arrays, x, g, gemm=gemm)
    want, floor = _case_oracle(case, arrays, got)
    _compare(got, want, floor=floor)
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
    C_in, C_out, stride = case[:3]
    hl = pkg.hip_lib
    plan = hl.block_plan(pkg.fused.make_desc(
        tuple(x.shape), C_out, 1, stride, 4, 1e-5, 0.1, True, **pkg.fused._gemm_flags(gemm)))
    assert plan & hl.PLAN_FOLD, plan
    if gemm == "f32x3":
        assert not plan & hl.PLAN_F16X2, plan
        _bf16x3_wt[case] = got[WT]
        ref = _run_hip(pkg, arrays, x, g, gemm="fp32")
        assert not torch.equal(got[WT], ref[WT]), "k_wgrad_x3 (bf16 splits) did not run"
    else:
        assert plan & hl.PLAN_F16X2, plan
        assert bool(plan & hl.PLAN_FOLD_NO_G) == (gemm == "f16x2_nog"), plan
        if case not in _bf16x3_wt:
            _bf16x3_wt[case] = _run_hip(pkg, arrays, x, g, gemm="f32x3")[WT]
        assert not torch.equal(got[WT], _bf16x3_wt[case]), "k_wgrad_x3 (fp16 splits) did not run"
