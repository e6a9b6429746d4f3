"""Cases and oracles of the non-finite tests (test_nonfinite_host.py on the
CPU, test_gpu_nonfinite.py on the GPU): one block in eval mode with one bad
element in x (forward) or in g (backward). Shapes are (C_in, C_out, stride, V,
K, N, T); the bad element is always in clip ``CLIP``. The rule they test is in
include/stgcn_hip.h (Conventions, "Non-finite values") and tests/gates.py."""
import functools

import numpy as np
import torch

from oracle import ref_cpu
from test_gpu_callers import _eval_case

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
CLIP = 1

FWD_SHAPES = [
    (64, 64, 1, 18, 1, 3, 20),
    (64, 128, 2, 18, 1, 3, 21),
    (64, 64, 1, 25, 3, 3, 20),
    (64, 64, 1, 50, 3, 3, 17),
    (5, 7, 1, 18, 1, 3, 9),
]
BWD_SHAPES = [(64, 64, 1, 18, 1, 3, 20), (64, 128, 2, 25, 3, 3, 21)]


def fwd_modes(V):
    return ("fp32", "f32x3", "f16x2") if V == 18 else ("fp32", "bf16")


def joints(pkg, V):
    """(edge joint, hub joint) of the skeleton graph for V joints: a joint with
    the fewest and one with the most neighbours. (The reference's normalised
    adjacency itself is dense -- its normalisation adds a small constant to
    every entry -- so A's support does not tell them apart.)"""
    adj = pkg.graph.graph_for(V).adj_list
    deg = [len(adj[v]) for v in range(V)]
    return int(np.argmin(deg)), int(np.argmax(deg))


def positions(pkg, V, T, C):
    """The six (c, t, v) of the bad element: t = 0, an interior frame and T - 1,
    each at the edge joint and at the hub joint; the channel moves along."""
    edge, hub = joints(pkg, V)
    tv = [(t, v) for t in (0, T // 2 + 1, T - 1) for v in (edge, hub)]
    return [((3 * i + 1) % C, t, v) for i, (t, v) in enumerate(tv)]


def fwd_cases():
    """(shape, gemm, bad value, position index): every shape sees every value
    and every position, every mode sees NaN and +Inf."""
    out = []
    for shape in FWD_SHAPES:
        modes = fwd_modes(shape[3])
        if len(modes) == 3:
            plan = [(0, NAN), (1, PINF), (2, NAN), (0, PINF), (1, NAN), (2, PINF),
                    (0, NINF), (2, NINF)]
        else:
            plan = [(0, NAN), (1, PINF), (0, NINF), (1, NAN), (0, PINF), (1, NINF)]
        out += [(shape, modes[m], val, i % 6) for i, (m, val) in enumerate(plan)]
    return out


def case_id(c):
    return "-".join("x".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in c)


@functools.lru_cache(maxsize=None)
def eval_case(pkg, shape, residual=False):
    """(arrays, x, g, params, buffers) of a block with non-trivial running
    statistics; shared between the tests and never written."""
    arrays, x, g = _eval_case(pkg, shape, residual)
    p, b = ref_cpu.block_params_from_arrays(arrays, dtype=torch.float32, requires_grad=False)
    return arrays, x, g, p, b


def oracle_fwd(case, x, dtype, gemm_bf16=False):
    """y of the block in eval mode, dense torch ops: IEEE propagation."""
    arrays, _, _, p, b = case
    pp = {k: v.to(dtype) for k, v in p.items()}
    bb = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in b.items()}
    with torch.no_grad():
        return ref_cpu.block_forward(x.to(dtype), pp, bb, int(arrays["meta"][2]),
                                     residual=bool(arrays["meta"][7]), training=False,
                                     dtype=dtype, gemm_bf16=gemm_bf16)


@functools.lru_cache(maxsize=None)
def clean_fwd(pkg, shape, dtype, gemm_bf16=False):
    case = eval_case(pkg, shape)
    return oracle_fwd(case, case[1], dtype, gemm_bf16)


def oracle_bwd(case, g, dtype, relu_mask=None, gemm_bf16=False):
    """(y, dx, parameter gradients) of the block in eval mode with gradients.
    The final ReLU's backward is a select, as the reference's (threshold
    backward): a bad g at a masked-off element reaches nothing. relu_mask: the
    mask to select with (default: the oracle's own y > 0)."""
    arrays, x, _, p, b = case
    pp = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in p.items()}
    bb = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in b.items()}
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    pre = ref_cpu.block_forward(xx, pp, bb, int(arrays["meta"][2]),
                                residual=bool(arrays["meta"][7]), training=False, dtype=dtype,
                                return_pre_relu=True, gemm_bf16=gemm_bf16)
    mask = (pre.detach() > 0) if relu_mask is None else relu_mask.bool()
    y = torch.where(mask, pre, torch.zeros((), dtype=dtype))
    y.backward(g.to(dtype))
    out = {"y": y.detach(), "grad.x": xx.grad}
    out.update({"grad." + k: v.grad for k, v in pp.items()})
    return out


def pre_relu(case):
    """The block's output before its final ReLU, eval mode, fp64."""
    arrays, x, _, p, b = case
    p64 = {k: v.double() for k, v in p.items()}
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in b.items()}
    with torch.no_grad():
        return ref_cpu.block_forward(x.double(), p64, b64, int(arrays["meta"][2]),
                                     residual=bool(arrays["meta"][7]), training=False,
                                     dtype=torch.float64, return_pre_relu=True)


def pick_output_elements(pre, clip=CLIP, margin=0.1):
    """(active, masked): positions (n, o, t', w) in clip ``clip`` whose pre-ReLU
    value is above ``margin`` / below -``margin`` (far from a ReLU tie), interior
    in time where there is one."""
    pre = pre[clip]
    tmid = pre.shape[1] // 2
    act = torch.nonzero(pre[:, tmid, :] > margin)[0]
    off = torch.nonzero(pre[:, tmid, :] < -margin)[-1]
    return (clip, int(act[0]), tmid, int(act[1])), (clip, int(off[0]), tmid, int(off[1]))
