"""GPU: a non-finite value is never turned into a finite wrong one
(include/stgcn_hip.h, Conventions, "Non-finite values").

The oracle is oracle/ref_cpu.py with torch's dense ops, i.e. IEEE propagation
as the reference has it. Per output element (tests/gates.py check_rules):
(a) where the oracle is non-finite inside the bad element's sparse footprint,
the result is non-finite (NaN and +-Inf interchangeable: the fp16 / bf16 splits
turn Inf into NaN); (b) where the oracle is finite, the result is within the
test's usual gate of it, or non-finite inside the dense footprint (a dense
0 * NaN is NaN, a kernel that skips zeros gives a finite value, ReLU(-Inf) = 0);
(c) in eval mode every element of every other clip is finite and within the
gate of a clean run's oracle, in every GEMM mode, f16x2 with an Inf input
included. In training mode one bad element makes the batch statistics
non-finite: rule (a) over the whole of every tensor.

Non-finite masks are compared first, then the finite remainder with the
existing gate; no array holding a NaN reaches conftest.rel_to_max.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

import gates
import nonfinite_cases as nc
import test_gpu_bf16 as tb
import test_gpu_eval as te
from conftest import rel_to_max
from oracle import ref_cpu
from test_gpu_block import DEV, TOL, _compare, _oracle, _random_case, _run_hip
from test_gpu_callers import _run_eval_backward
from test_gpu_stack import snapshot_stack

pytestmark = pytest.mark.gpu
NAN, PINF, NINF = nc.NAN, nc.PINF, nc.NINF


def _vid(v):
    return {"nan": "nan", "inf": "inf", "-inf": "ninf"}[str(v)]


# --- 1. block, eval mode, forward ---------------------------------------------

def _run_eval_fwd(pkg, ec, x, gemm):
    arrays, _, _, p, b = ec
    cu = {k: v.to(DEV) for k, v in p.items()}
    bu = {k: v.to(DEV).clone() for k, v in b.items() if "num_batches" not in k}
    with torch.no_grad():
        y = pkg.fused.StgcnBlockFn.apply(
            x.to(DEV), cu["spatialConv.A"], cu["spatialConv.W.weight"], cu["spatialConv.W.bias"],
            cu["temporalConv.weight"], cu["temporalConv.bias"], cu["batch_n.weight"],
            cu["batch_n.bias"], cu["batch_n_2.weight"], cu["batch_n_2.bias"],
            bu["batch_n.running_mean"], bu["batch_n.running_var"],
            bu["batch_n_2.running_mean"], bu["batch_n_2.running_var"],
            int(arrays["meta"][2]), 4, 1e-5, 0.1, False, None, 0.0, gemm)
    torch.cuda.synchronize()
    for k in bu:  # eval mode leaves the running statistics untouched
        assert torch.equal(bu[k].cpu(), b[k]), k
    return y.cpu()


def _fwd_gate(pkg, shape, gemm):
    """The usual gate of y in eval mode: 1e-5 in the fp32 modes
    (test_eval_mode_uses_running_stats), bf16 max(2e-2, 3x the bf16-operand
    oracle's own error on the clean input)."""
    if gemm != "bf16":
        return TOL
    floor = rel_to_max(nc.clean_fwd(pkg, shape, torch.float32, True).double().numpy(),
                       nc.clean_fwd(pkg, shape, torch.float64).numpy())
    return max(2e-2, 3 * floor)


@pytest.mark.parametrize("case", nc.fwd_cases(), ids=nc.case_id)
def test_block_eval_forward(pkg, case):
    shape, gemm, val, ipos = case
    C_in, C_out, stride, V, K, N, T = shape
    ec = nc.eval_case(pkg, shape)
    A = ec[3]["spatialConv.A"].numpy()
    pos = nc.positions(pkg, V, T, C_in)[ipos]
    x = ec[1].clone()
    x[(nc.CLIP,) + pos] = val
    got = _run_eval_fwd(pkg, ec, x, gemm)
    want = nc.oracle_fwd(ec, x, torch.float64)
    sparse, dense = gates.fwd_footprint(A, stride, x.shape, C_out, (nc.CLIP,) + pos)
    gates.check_rules("y", got, want, _fwd_gate(pkg, shape, gemm), sparse, dense,
                      clean=nc.clean_fwd(pkg, shape, torch.float64), clip=nc.CLIP)


# --- 2. block, eval mode with gradients ---------------------------------------

# (shape, residual, gemm): the fp32 route plain and residual at both shapes, and
# the other GEMM modes of test_block_eval_mode_backward where a shape takes them
# (f16: the folded f16x2 block, whose operand scales a bad dy must not collapse)
BWD_ROUTES = [(s, r, "fp32") for s in nc.BWD_SHAPES for r in (False, True)] + [
    (nc.BWD_SHAPES[0], False, "x3"), (nc.BWD_SHAPES[0], False, "f16"),
    (nc.BWD_SHAPES[1], False, "bf16")]


def _rid(r):
    return "-".join(["x".join(map(str, r[0])), "residual" if r[1] else "plain", r[2]])


@pytest.mark.parametrize("val", [NAN, PINF], ids=_vid)
@pytest.mark.parametrize("where", ["active", "masked"])
@pytest.mark.parametrize("route", BWD_ROUTES, ids=_rid)
def test_block_eval_backward(pkg, route, where, val):
    """A clean x and one bad element in g, where the output is active (y > 0)
    and where it is masked off (y == 0: the reference's ReLU backward is a
    select, so nothing is reached and every gradient is finite and at the gate)."""
    shape, residual, gemm = route
    C_in, C_out, stride, V, K, N, T = shape
    ec = nc.eval_case(pkg, shape, residual)
    arrays, x, g0 = ec[0], ec[1], ec[2]
    act, off = nc.pick_output_elements(nc.pre_relu(ec))
    pos = act if where == "active" else off
    g = g0.clone()
    g[pos] = val
    _, _, got, _, _ = _run_eval_backward(pkg, arrays, x, g, shape, residual, gemm)
    assert bool(got["y"][pos] > 0) == (where == "active")
    mask = got["y"] > 0
    want = nc.oracle_bwd(ec, g, torch.float64, relu_mask=mask)
    clean = nc.oracle_bwd(ec, g0, torch.float64, relu_mask=mask)
    if gemm == "bf16":  # max(2e-2, 3x the bf16-operand oracle's own error), on the clean g
        ref16 = nc.oracle_bwd(ec, g0, torch.float32, relu_mask=mask, gemm_bf16=True)
        gate = {k: max(2e-2, 3 * rel_to_max(ref16[k].double().numpy(), w.numpy()))
                for k, w in clean.items()}
    else:  # (_check_eval_backward)
        gate = {k: (TOL if k in ("y", "grad.x") else 2 * TOL) for k in want}
    if where == "masked":
        for k, w in want.items():
            assert torch.isfinite(got[k]).all(), k
            gates.check_rules(k, got[k], w, gate[k], whole=True)
        return
    sparse, dense = gates.bwd_footprint(ec[3]["spatialConv.A"].numpy(), stride, x.shape, pos,
                                        residual=residual)
    gates.check_rules("y", got["y"], want["y"], gate["y"], whole=True)
    gates.check_rules("grad.x", got["grad.x"], want["grad.x"], gate["grad.x"], sparse, dense,
                      clean=clean["grad.x"], clip=nc.CLIP)
    for k, w in want.items():  # every parameter gradient the oracle has non-finite
        if k.startswith("grad.") and k != "grad.x":
            assert not torch.isfinite(w).all(), k
            gates.check_rules(k, got[k], w, gate[k], whole=True)


# --- 3. block, training mode --------------------------------------------------

TRAIN_SHAPES = [(64, 64, 1, 18, 1, 2, 20), (64, 128, 2, 25, 3, 2, 21), (3, 64, 1, 18, 1, 2, 24)]
BAD = ["x-nan", "x-inf", "g-nan-active", "g-nan-masked"]


def _train_cases():
    """Every (shape, mode, plain / residual) sees all four bad inputs, need_dx on
    and off by turns; the fp32 mode sees both for every bad input."""
    out = []
    for shape in TRAIN_SHAPES:
        for m, gemm in enumerate(nc.fwd_modes(shape[3])):
            for residual in (False, True):
                for i, bad in enumerate(BAD):
                    # (the pairing turns with the mode and the block kind, so that every
                    # bad input meets need_dx on and off outside fp32 as well)
                    out.append((shape, gemm, residual, bad, (i + m + residual) % 2 == 0))
                    if gemm == "fp32":
                        out.append((shape, gemm, residual, bad, (i + m + residual) % 2 == 1))
    return out


def _tid(c):
    shape, gemm, residual, bad, need_dx = c
    return "-".join(["x".join(map(str, shape)), gemm, "res" if residual else "plain", bad,
                     "dx" if need_dx else "nodx"])


@pytest.mark.parametrize("case", _train_cases(), ids=_tid)
def test_block_training(pkg, case):
    shape, gemm, residual, bad, need_dx = case
    arrays, x, g = _random_case(pkg, *shape, residual=residual)
    arrays = dict(arrays)
    x, g = x.clone(), g.clone()
    pre = ref_cpu.block_pre_relu(arrays)
    act, off = nc.pick_output_elements(pre, clip=1)
    if bad.startswith("x"):
        x[1, 1 % shape[0], shape[6] // 2, 3] = NAN if bad == "x-nan" else PINF
    else:
        g[act if bad.endswith("active") else off] = NAN
    arrays["x"], arrays["g"] = x.numpy(), g.numpy()
    got = _run_hip(pkg, arrays, x, g, need_dx=need_dx, gemm=gemm)
    assert ("grad.x" in got) == need_dx
    if bad == "g-nan-masked":  # the select drops it: everything finite and at the gate
        for k, v in got.items():
            assert torch.isfinite(v).all(), k
        g[off] = 0.0  # (the oracle's mask multiplies: 0 * NaN; a select is g = 0 there)
        arrays["g"] = g.numpy()
        if gemm == "bf16":
            got["inner_mask"] = tb._run(pkg, arrays, x, g, True, need_dx)["inner_mask"]
            want, ref16 = tb._bf16_reference(arrays, got, need_dx)
            errs, floor = tb._errors(got, want, residual), tb._errors(ref16, want, residual)
            badk = {k: (e, floor[k]) for k, e in errs.items()
                    if not e < max(tb.TOL_BF16, tb.FLOOR_FACTOR * floor[k])}
            assert not badk, badk
        else:
            want, floor = _oracle(arrays, got)
            if not need_dx:
                want.pop("grad.x")
            _compare(got, want, residual=residual, floor=floor)
        return
    # rule (a) over the whole of each tensor against the fp32 oracle; what it
    # leaves finite (with a bad g: y, the running statistics and the rows of the
    # per-channel gradients other than the bad element's channel) at the usual
    # gate against the fp64 oracle, through the run's ReLU mask where y is finite
    mask = (got["y"] > 0) if bad.startswith("g") else None
    w32 = ref_cpu.block_step(arrays, dtype=torch.float32, relu_mask=mask)
    w64 = ref_cpu.block_step(arrays, dtype=torch.float64, relu_mask=mask)
    wfl = ref_cpu.block_step(arrays, dtype=torch.float32, relu_mask=mask, gemm_bf16=True) \
        if gemm == "bf16" else w32
    nonfinite = 0
    for k, v in got.items():
        w = w32[k].detach()
        lost = ~torch.isfinite(w) & torch.isfinite(v)
        assert not lost.any(), f"{k}: {int(lost.sum())} of {int((~torch.isfinite(w)).sum())} " \
                               "non-finite oracle elements came out finite"
        nonfinite += int((~torch.isfinite(w)).sum())
        if bad.startswith("g") and torch.isfinite(w).all():  # (y, the running statistics)
            assert torch.isfinite(v).all(), k
        if k in ("y", "grad.x", "after.batch_n_2.running_mean", "after.batch_n_2.running_var") \
                and bad.startswith("x"):
            assert not torch.isfinite(w).any(), (k, "the oracle is non-finite throughout")
        w6 = w64[k].detach().numpy()
        if k == "grad.temporalConv.bias" and not residual:  # (analytically 0)
            fin = torch.isfinite(v).numpy() & np.isfinite(w6)
            assert not fin.any() or np.abs(v.numpy()[fin]).max() < (1e-3 if gemm == "bf16" else 1e-5)
            continue
        floor = gates.finite_err(wfl[k].detach().numpy(), w6)
        lim = max(2e-2, 3 * floor) if gemm == "bf16" else max(TOL, 2 * floor)
        err = gates.finite_err(v.numpy(), w6)
        assert not gates.exceeds(err, lim), f"{k}: finite remainder {err:.2e} > {lim:.1e}"
    assert nonfinite > 0


# --- 4. stack -----------------------------------------------------------------

STACKS = {"v18-f16x2": (18, 1, dict(f32_gemm="f16x2")),
          "v25k3-bf16": (25, 3, dict(gemm_dtype=torch.bfloat16))}


@pytest.mark.parametrize("name", list(STACKS))
def test_stack_training_step(pkg, name):
    """One NaN in clip 2 of the input: forward_loss gives a non-finite loss, and
    every parameter gradient the oracle stack has non-finite is non-finite."""
    V, K, kw = STACKS[name]
    A = te._adjacency(pkg, V, K)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = pkg.STGCNStack(3, 10, A, **kw)
    p0, b0 = snapshot_stack(m)
    m = m.to(DEV).train()
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 3, 32, V, generator=gen)
    lab = torch.randint(0, 10, (4,), generator=gen)
    x[2, 1, 17, 5] = NAN
    loss, logits = m.forward_loss(x.to(DEV), lab.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    assert not np.isfinite(loss.item()), loss.item()
    p = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    b = {k: v.clone() for k, v in b0.items()}
    lg = ref_cpu.Stack(p, b).forward(x.permute(0, 2, 3, 1).contiguous(), dtype=torch.float32)
    ls = torch.nn.functional.cross_entropy(lg, lab)
    ls.backward()
    assert not np.isfinite(ls.item())
    checked = 0
    for k, v in m.named_parameters():
        if k.startswith("Masks.") or p[k].grad is None:
            continue
        w = p[k].grad
        lost = ~torch.isfinite(w) & torch.isfinite(v.grad.cpu())
        assert not lost.any(), f"{k}: {int(lost.sum())} of {int((~torch.isfinite(w)).sum())} " \
                               "non-finite oracle elements came out finite"
        checked += int((~torch.isfinite(w)).sum())
    assert checked > 0


def _split_rows(r_bad, r_clean, lab2):
    """Clips 0, 1 and 3 contribute the same to both confusion matrices: the
    matrices differ at most by clip 2's single entry, inside its label's row."""
    d = r_bad["confusion"].numpy().astype(np.int64) - r_clean["confusion"].numpy()
    rows = [i for i in range(d.shape[0]) if i != lab2]
    assert not d[rows].any(), d
    row = d[lab2]
    assert row.sum() == 0 and np.abs(row).sum() in (0, 2), row


@pytest.mark.parametrize("name", list(STACKS))
def test_stack_eval_step(pkg, name):
    """eval_step on a batch with one corrupt clip: the accumulated loss is
    non-finite, the confusion matrix still sums to the clip count, and what
    clips 0, 1 and 3 contribute equals that of the same call with clip 2
    replaced by a clean clip -- eagerly and through one captured graph replayed
    twice, the second time with the NaN."""
    to = pkg.train_ops
    V = te.CONFIGS[name][0]
    m, _, _ = te._stack(pkg, name)
    x, lab = te._inputs(4, 32, V)
    xb = x.clone()
    xb[2, 1, 17, 5] = NAN
    lab2 = int(lab[2])
    tol = 2e-2 if "bf16" in name else 1e-4

    def one(xin):
        mt = to.EvalMetrics(10, 3, device=DEV)
        _, logits = m.eval_step(xin, lab, mt)
        torch.cuda.synchronize()
        return mt.result(), logits.cpu().clone()

    r_clean, l_clean = one(x)
    r_bad, l_bad = one(xb)
    assert np.isfinite(r_clean["loss"]) and not np.isfinite(r_bad["loss"]), r_bad["loss"]
    assert int(r_bad["confusion"].sum()) == 4 == r_bad["clips"] and r_bad["batches"] == 1
    assert r_bad["invalid"] == 0
    _split_rows(r_bad, r_clean, lab2)
    others = [0, 1, 3]
    assert torch.isfinite(l_bad[others]).all() and not torch.isfinite(l_bad[2]).any()
    assert rel_to_max(l_bad[others].numpy(), l_clean[others].numpy()) < tol
    for key in ("correct", "topk_hits"):
        assert r_bad[key] - r_clean[key] in (-1, 0, 1), key

    xs = x.clone()
    mt = to.EvalMetrics(10, 3, device=DEV)
    step = to.GraphedStep(lambda: m.eval_step(xs, lab, mt), warmup=2)
    mt.reset()
    step()
    xs.copy_(xb)
    _, lg = step()
    torch.cuda.synchronize()
    r = mt.result()
    assert r["batches"] == 2 and r["clips"] == 8 and int(r["confusion"].sum()) == 8
    assert not np.isfinite(r["loss"])
    both = r_bad["confusion"].numpy().astype(np.int64) + r_clean["confusion"].numpy()
    assert np.array_equal(r["confusion"].numpy(), both)
    assert r["correct"] == r_bad["correct"] + r_clean["correct"]
    assert torch.equal(lg.cpu()[others], l_bad[others])


# --- 5. optimizer and clipping ------------------------------------------------

OPT_SIZES = (1, 257, 1000)


def _opt_inputs():
    g = torch.Generator().manual_seed(11)
    p0 = [torch.randn(n, generator=g) for n in OPT_SIZES]
    grads = [[torch.randn(n, generator=g) for n in OPT_SIZES] for _ in range(3)]
    return p0, grads


OPT_P0, OPT_GRADS = _opt_inputs()  # shared, never written


def _masks_then_values(name, got, want):
    """Non-finite masks equal, then the finite remainder at test_gpu_optim.py's
    tolerance (|d| <= 2e-6 |ref| + 1e-7 per element)."""
    got, want = got.double().cpu(), want.double()
    gm, wm = ~torch.isfinite(got), ~torch.isfinite(want)
    assert torch.equal(gm, wm), \
        f"{name}: non-finite at {gm.nonzero().flatten().tolist()[:8]} ({int(gm.sum())}), " \
        f"torch at {wm.nonzero().flatten().tolist()[:8]} ({int(wm.sum())})"
    d = (got - want).abs()[~wm]
    assert (d <= 2e-6 * want.abs()[~wm] + 1e-7).all(), (name, float(d.max()))


# (max_grad_norm needs capturable=True: FusedAdam refuses it otherwise, test_gpu_optim.py)
@pytest.mark.parametrize("capturable,clip", [(False, False), (True, False), (True, True)],
                         ids=["host-noclip", "capturable-noclip", "capturable-clip"])
@pytest.mark.parametrize("kind", ["adam", "adamw", "amsgrad"])
@pytest.mark.parametrize("val", [NAN, PINF], ids=_vid)
def test_optimizer_step(pkg, val, kind, capturable, clip):
    """A clean step, a step with one bad gradient element (element 100 of the
    257-element parameter), a clean step, against torch.optim.Adam / AdamW on
    the CPU in fp64, preceded by clip_grad_norm_ where max_grad_norm = 1 is given."""
    decoupled, amsgrad = kind == "adamw", kind == "amsgrad"
    wd = 0.01 if decoupled else 0.0
    ref = [p.clone().double().requires_grad_(True) for p in OPT_P0]
    opt_ref = (torch.optim.AdamW if decoupled else torch.optim.Adam)(
        ref, lr=1e-2, weight_decay=wd, amsgrad=amsgrad, foreach=False)
    dut = [p.clone().to(DEV).requires_grad_(True) for p in OPT_P0]
    opt = (pkg.FusedAdamW if decoupled else pkg.FusedAdam)(
        dut, lr=1e-2, weight_decay=wd, amsgrad=amsgrad, capturable=capturable,
        **({"max_grad_norm": 1.0} if clip else {}))
    for step, gs in enumerate(OPT_GRADS):
        gs = [t.clone() for t in gs]
        if step == 1:
            gs[1][100] = val
        for p, q, t in zip(ref, dut, gs):
            p.grad, q.grad = t.double(), t.to(DEV)
        if clip:
            norm = torch.nn.utils.clip_grad_norm_(ref, 1.0)
            coef = torch.clamp(1.0 / (norm + 1e-6), max=1.0)
        opt_ref.step()
        opt.step()
        torch.cuda.synchronize()
        if clip:  # stgcn_grad_norm's norm_out and coef_out: NaN in gives NaN out
            _masks_then_values(f"step {step} norm", opt.grad_norm.reshape(1), norm.reshape(1))
            _masks_then_values(f"step {step} coef", opt.clip_coef.reshape(1), coef.reshape(1))
            if step == 1:
                assert not np.isfinite(float(opt.grad_norm))
                assert np.isnan(float(opt.clip_coef)) == np.isnan(val)
    keys = ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if amsgrad else ())
    for i, (a, b) in enumerate(zip(dut, ref)):
        _masks_then_values(f"param {i}", a.detach(), b.detach())
        for key in keys:
            _masks_then_values(f"{key} {i}", opt.state[a][key], opt_ref.state[b][key])
    bad = [int((~torch.isfinite(a.detach())).sum()) for a in dut]
    if clip and np.isnan(val):  # a NaN norm: every element of every parameter
        assert bad == list(OPT_SIZES), bad
    else:  # only that element
        assert bad == [0, 1, 0], bad
