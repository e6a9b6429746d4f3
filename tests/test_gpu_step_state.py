"""STGCN_FEATURE_STEP_STATE on the GPU: per-step values read from device memory,
so a step captured in a HIP graph (train_ops.GraphedStep) replays the
reference's recipe -- dropout with a new mask per step, Adam under a
learning-rate schedule, gradient clipping.

1. the block with its dropout seeded from a device token: the mask is
   fused.dropout_mask(seed, shape, p, counter) and the gradients pass the oracle
   gates of the host-seeded block (tests/test_gpu_block.py; the bf16 case the
   bf16 gate of tests/test_gpu_bf16.py with the dropout mask folded into the
   oracle's ReLU mask); without a token the _dseed calls are the old calls;
2. a backward regenerates the mask of ITS forward, whatever ran in between;
3. replays of a captured dropout step draw new masks (the parent applied one
   frozen mask to every replay); a host seed refuses the capture;
4. the graphed dropout step equals the eager one;
5. a tensor lr written between steps equals the float lr of the same value;
6. clipping: the device norm, its reproducibility, the clipped step.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from test_gpu_block import DEV, _gate_dropout, _random_case
from test_gpu_bf16 import FLOOR_FACTOR, TIE_BF16, TOL_BF16, _errors

pytestmark = pytest.mark.gpu


def _token(c):
    return torch.tensor([c], dtype=torch.int64, device=DEV)


def _run_block(pkg, arrays, x, g, drop, gemm="fp32", dseed=None, host_seed=1234):
    """The fused block fwd + bwd with dropout; dseed = (salt, token tensor) seeds
    it from device memory, else the host seed torch.manual_seed(host_seed) gives."""
    torch.manual_seed(host_seed)
    p, b = ref_cpu.block_params_from_arrays(arrays, dtype=torch.float32, requires_grad=False)
    stride, residual = int(arrays["meta"][2]), bool(arrays["meta"][7])
    cu = {k: v.to(DEV).contiguous().requires_grad_(True) for k, v in p.items()}
    bu = {k: v.to(DEV) for k, v in b.items() if "num_batches" not in k}
    xd = x.to(DEV).float().contiguous().requires_grad_(True)
    common = (xd, cu["spatialConv.A"], cu["spatialConv.W.weight"], cu["spatialConv.W.bias"],
              cu["temporalConv.weight"], cu["temporalConv.bias"], cu["batch_n.weight"],
              cu["batch_n.bias"], cu["batch_n_2.weight"], cu["batch_n_2.bias"])
    running = (bu["batch_n.running_mean"], bu["batch_n.running_var"],
               bu["batch_n_2.running_mean"], bu["batch_n_2.running_var"])
    if residual:
        y = pkg.fused.StgcnResBlockFn.apply(
            *common, cu.get("apply_residual.weight"), cu.get("apply_residual.bias"), *running,
            stride, 4, 1e-5, 0.1, True, None, drop, gemm, dseed)
    else:
        y = pkg.fused.StgcnBlockFn.apply(*common, *running, stride, 4, 1e-5, 0.1, True,
                                         None, drop, gemm, dseed)
    y.backward(g.to(DEV).float())
    torch.cuda.synchronize()
    out = {"y": y.detach().cpu(), "grad.x": xd.grad.cpu()}
    for k, t in cu.items():
        out["grad." + k] = t.grad.cpu()
    for k, t in bu.items():
        out["after." + k] = t.cpu()
    return out


# C_in, C_out, stride, V, K, N, T, residual, p, gemm: the cases of
# test_block_dropout_matches_oracle that reach every dropout site (the output
# pass and the three ReLU + BN2 backward passes; the temporal conv's epilogues
# of the residual block; stride 2) and one bf16 V = 25, K = 3 block
BLOCK_CASES = [
    (64, 64, 1, 18, 1, 3, 40, False, 0.5, "fp32"),
    (64, 64, 1, 18, 1, 3, 40, True, 0.5, "fp32"),
    (64, 128, 2, 18, 1, 2, 37, False, 0.2, "fp32"),
    (64, 128, 2, 25, 3, 2, 33, False, 0.5, "bf16"),
]
SALT = 0x1234567887654321 >> 2


def _effective_seed(pkg, salt, c):
    return pkg.fused._mix64((salt + c * pkg.fused._PHI) & pkg.fused._M64)


def _gate_bf16_dropout(arrays, got, keep, drop):
    """tests/test_gpu_bf16.py's gate (_bf16_reference + _gate_bf16's oracle part)
    with the dropout mask in the oracle's ReLU mask, as _gate_dropout does."""
    y = got["y"]
    assert (y[~keep] == 0).all(), "dropped elements must be 0"
    pre = ref_cpu.block_pre_relu(arrays)
    relu = y > 0
    flips = keep & (relu != (pre > 0))
    if flips.any():
        assert pre[flips].abs().max().item() < TIE_BF16 * pre.abs().max().item()
    mask = (keep & relu).double() / (1 - drop)
    want = ref_cpu.block_step(arrays, dtype=torch.float64, relu_mask=mask)
    ref16 = ref_cpu.block_step(arrays, dtype=torch.float32, relu_mask=mask.float(),
                               gemm_bf16=True)
    errs, floor = _errors(got, want, False), _errors(ref16, want, False)
    print("bf16 dropout errs", errs)
    bad = {k: (e, floor[k]) for k, e in errs.items()
           if not e < max(TOL_BF16, FLOOR_FACTOR * floor[k])}
    assert not bad, f"bf16 dropout block vs fp64 oracle: {bad}"
    assert got["grad.temporalConv.bias"].abs().max().item() < 1e-3


@pytest.mark.parametrize("counter", [0, 5])
@pytest.mark.parametrize("case", BLOCK_CASES)
def test_block_device_seed_matches_oracle(pkg, case, counter):
    *shape, residual, drop, gemm = case
    C_in, C_out, stride, V, K, N, T = shape
    arrays, x, g = _random_case(pkg, C_in, C_out, stride, V, K, N, T, seed=5, residual=residual)
    got = _run_block(pkg, arrays, x, g, drop, gemm, dseed=(SALT, _token(counter)))
    keep = torch.from_numpy(pkg.fused.dropout_mask(SALT, tuple(got["y"].shape), drop, counter))
    y = got["y"]
    # the zero pattern: dropped elements are 0, and the kept ones are not all 0
    assert (y[~keep] == 0).all()
    assert (y[keep] != 0).double().mean().item() > 0.25
    # ... and it is this token's mask, not the by-value seed's or the next token's
    for other in (pkg.fused.dropout_mask(SALT, tuple(y.shape), drop),
                  pkg.fused.dropout_mask(SALT, tuple(y.shape), drop, counter + 1)):
        assert (y[~torch.from_numpy(other)] != 0).any()
    if gemm == "bf16":
        _gate_bf16_dropout(arrays, got, keep, drop)
    else:
        # the scaling and the gradients: test_block_dropout_matches_oracle's gate
        # with the effective seed (its _keep_mask is dropout_mask without counter)
        _gate_dropout(arrays, got, _effective_seed(pkg, SALT, counter), drop, residual)


class _OldCalls:
    """The library with the _dseed block calls routed to the calls without a
    seed pointer (which must be given none)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def stgcn_block_fwd_dseed(self, d, a, tok, ws, n, s):
        assert tok is None
        return self._lib.stgcn_block_fwd(d, a, ws, n, s)

    def stgcn_block_bwd_dseed(self, d, a, tok, ws, n, s):
        assert tok is None
        return self._lib.stgcn_block_bwd(d, a, ws, n, s)


@pytest.mark.parametrize("case", BLOCK_CASES[:3])
def test_null_seed_dev_is_the_old_call(pkg, case, monkeypatch):
    *shape, residual, drop, gemm = case
    C_in, C_out, stride, V, K, N, T = shape
    arrays, x, g = _random_case(pkg, C_in, C_out, stride, V, K, N, T, seed=5, residual=residual)
    new = _run_block(pkg, arrays, x, g, drop, gemm)
    monkeypatch.setattr(pkg.hip_lib, "_LIB", _OldCalls(pkg.hip_lib.lib()))
    old = _run_block(pkg, arrays, x, g, drop, gemm)
    assert (new["y"] == 0).double().mean().item() > drop - 0.05  # (dropout ran)
    for k in new:
        assert torch.equal(new[k], old[k]), k


def _block(pkg, V=18, drop=0.5, residual=False, salt=SALT):
    gr = pkg.graph
    A = gr.get_normalized_adjacency_matrices(0, 1, graph=gr.graph_for(V))
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        blk = pkg.SpatialTemporalConv(64, 64, A, 9, 1, 4, dropout_rate=drop, residual=residual)
    blk = blk.to(DEV).train()
    blk.drop_counter = pkg.fused.DropoutCounter(DEV)
    blk.drop_salt = salt
    return blk


@pytest.mark.parametrize("residual", [False, True])
def test_backward_uses_its_forwards_token(pkg, residual):
    """Forward A, forward B (advances the counter), backward A: A's gradients are
    those of a run without forward B (gradient accumulation keeps its masks)."""
    gen = torch.Generator().manual_seed(2)
    xa = torch.randn(3, 64, 20, 18, generator=gen).to(DEV)
    xb = torch.randn(3, 64, 20, 18, generator=gen).to(DEV)
    g = torch.randn(3, 64, 20, 18, generator=gen).to(DEV)

    def run(with_b):
        blk = _block(pkg, residual=residual)
        x = xa.clone().requires_grad_(True)
        ya = blk(x)
        if with_b:
            yb = blk(xb)
            assert not torch.equal(ya == 0, yb == 0)
        ya.backward(g)
        torch.cuda.synchronize()
        assert int(blk.drop_counter.counter.item()) == (2 if with_b else 1)
        return ya.detach(), x.grad, {k: p.grad for k, p in blk.named_parameters()}

    ya1, dx1, g1 = run(True)
    ya2, dx2, g2 = run(False)
    keep = torch.from_numpy(pkg.fused.dropout_mask(SALT, tuple(ya1.shape), 0.5, 1)).to(DEV)
    assert (ya1[~keep] == 0).all() and torch.equal(ya1, ya2)
    assert torch.equal(dx1, dx2)
    # (the backward dropped dx through mask 1: with mask 2 it would differ)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def _stack(pkg, V, K, bf16, drop, dropout_seed):
    gr = pkg.graph
    if K == 1:
        A = gr.get_normalized_adjacency_matrices(0, 1, graph=gr.graph_for(V))
    else:
        A = gr.get_normalized_adjacency_matrices(2, 1, distances=gr.synthetic_distances(V),
                                                 graph=gr.graph_for(V))
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = pkg.STGCNStack(3, 10, A, dropout_rate=drop,
                           gemm_dtype=torch.bfloat16 if bf16 else torch.float32,
                           f32_gemm="f16x2", dropout_seed=dropout_seed)
    return m.to(DEV).train()


def _step_fn(pkg, m, x, labels, lr):
    """(step, opt): one training step that also returns a copy of the first
    block's output (a forward hook's clone, so it outlives the step)."""
    opt = pkg.FusedAdam(list(m.parameters()), lr=lr, capturable=True)
    seen = {}
    m.conv[0].register_forward_hook(lambda mod, inp, out: seen.__setitem__(
        "y0", out.detach().clone()))

    def step():
        opt.zero_grad(set_to_none=True)
        loss, logits = m.forward_loss(x, labels)
        loss.backward()
        opt.step()
        return seen["y0"], loss, logits
    return step, opt


def _batch(V, N=4, T=32):
    g = torch.Generator().manual_seed(3)
    return (torch.randn(N, 3, T, V, generator=g).to(DEV),
            torch.randint(0, 10, (N,), generator=g).to(DEV))


STACKS = [(18, 1, False), (25, 3, True)]


@pytest.mark.parametrize("V,K,bf16", STACKS)
def test_replays_draw_new_masks(pkg, V, K, bf16):
    """lr = 0: the parameters stay put, so the first block's pre-dropout output is
    the same in every step and only the mask changes between replays."""
    x, labels = _batch(V)
    m = _stack(pkg, V, K, bf16, 0.5, "device")
    assert "drop_counter" not in m.state_dict()
    assert "drop_counter" in dict(m.named_buffers())
    step, _ = _step_fn(pkg, m, x, labels, lr=0.0)
    warm = 2
    graphed = pkg.GraphedStep(step, warmup=warm)
    ys = []
    for _ in range(3):
        ys.append(graphed()[0].clone())
    torch.cuda.synchronize()
    assert int(m.drop_counter.item()) == warm + 3  # (the capture itself runs nothing)
    salt = m.conv[0].drop_salt
    keeps = [torch.from_numpy(pkg.fused.dropout_mask(salt, tuple(ys[0].shape), 0.5, warm + 1 + k))
             .to(DEV) for k in range(3)]
    for k, (y, keep) in enumerate(zip(ys, keeps)):
        assert (y[~keep] == 0).all(), k
        assert (y[keep] != 0).double().mean().item() > 0.25, k
    for k in range(2):
        assert not torch.equal(ys[k] == 0, ys[k + 1] == 0), "the same zero pattern twice"
        both = keeps[k] & keeps[k + 1]
        assert torch.equal(ys[k][both], ys[k + 1][both])  # (same values under both masks)
        only = keeps[k] & ~keeps[k + 1]
        assert (ys[k][only] != 0).any()  # (replay k did not use replay k + 1's mask)


def test_host_seed_refuses_capture(pkg):
    x, labels = _batch(18)
    m = _stack(pkg, 18, 1, False, 0.5, "host")
    step, _ = _step_fn(pkg, m, x, labels, lr=0.0)
    with pytest.raises(RuntimeError, match='dropout_seed="device"'):
        pkg.GraphedStep(step, warmup=1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("V,K,bf16", STACKS)
def test_graphed_dropout_step_matches_eager(pkg, V, K, bf16):
    """Same init, same torch.manual_seed (so the same salts): 5 eager steps
    against 2 warm-up steps + 3 replays. Two runs of these dropout steps are
    bit-identical on the GPU (measured on an MI355X for both configurations: the
    fp64 BatchNorm sums of the unchained dropout path absorb the order of their
    atomics before they are rounded to fp32), so everything is compared with
    torch.equal: the masks, loss, logits, parameters and buffers."""
    x, labels = _batch(V)
    ma = _stack(pkg, V, K, bf16, 0.5, "device")
    mb = _stack(pkg, V, K, bf16, 0.5, "device")
    assert [b.drop_salt for b in ma.conv] == [b.drop_salt for b in mb.conv]
    step_a, _ = _step_fn(pkg, ma, x, labels, lr=1e-3)
    step_b, _ = _step_fn(pkg, mb, x, labels, lr=1e-3)
    for _ in range(5):
        ya, la, ga = step_a()
    graphed = pkg.GraphedStep(step_b, warmup=2)
    for _ in range(3):
        yb, lb, gb = graphed()
    torch.cuda.synchronize()
    assert int(ma.drop_counter.item()) == int(mb.drop_counter.item()) == 5
    keep = torch.from_numpy(pkg.fused.dropout_mask(ma.conv[0].drop_salt, tuple(ya.shape),
                                                   0.5, 5)).to(DEV)
    assert (ya[~keep] == 0).all() and (yb[~keep] == 0).all()
    assert torch.equal(ya, yb)
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    for (ka, a), (kb, b) in zip(ma.state_dict().items(), mb.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka


ADAM_SHAPES = [(64, 3, 9), (256,), (400, 256), (18, 18), (2049,)]


def _adam_inputs(steps=6, seed=7):
    g = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(s, generator=g) for s in ADAM_SHAPES]
    grads = [[torch.randn(s, generator=g) for s in ADAM_SHAPES] for _ in range(steps)]
    return p0, grads


def _same_state(oa, pa, ob, pb):
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[a][k], ob.state[b][k]), k


LRS = [1e-3, 3e-3, 7e-4, 1e-2, 1.234e-5, 0.5]


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_tensor_lr_matches_float_lr(pkg, wd):
    p0, grads = _adam_inputs()
    pa = [t.to(DEV).requires_grad_(True) for t in p0]
    pb = [t.to(DEV).requires_grad_(True) for t in p0]
    lr_t = torch.tensor(LRS[0], device=DEV)
    oa = pkg.FusedAdam(pa, lr=float(np.float32(LRS[0])), weight_decay=wd, capturable=True)
    ob = pkg.FusedAdam(pb, lr=lr_t, weight_decay=wd, capturable=True)
    for v, gs in zip(LRS, grads):
        oa.param_groups[0]["lr"] = float(np.float32(v))
        ob.param_groups[0]["lr"].fill_(v)
        for p, gg in zip(pa, gs):
            p.grad = gg.to(DEV)
        for p, gg in zip(pb, gs):
            p.grad = gg.to(DEV)
        oa.step()
        ob.step()
    torch.cuda.synchronize()
    assert ob.param_groups[0]["lr"] is lr_t
    assert float(ob.state[pb[0]]["step"]) == 6.0
    _same_state(oa, pa, ob, pb)


def test_tensor_lr_is_checked(pkg):
    p = [torch.randn(8, device=DEV).requires_grad_(True)]
    p[0].grad = torch.ones(8, device=DEV)
    for lr, cap in ((torch.tensor(1e-3), True), (torch.tensor([1e-3], device=DEV), True),
                    (torch.tensor(1e-3, device=DEV, dtype=torch.float64), True),
                    (torch.tensor(1e-3, device=DEV), False)):
        with pytest.raises(RuntimeError, match="tensor lr"):
            pkg.FusedAdam(p, lr=lr, capturable=cap).step()
    with pytest.raises(ValueError, match="capturable"):
        pkg.FusedAdam(p, lr=1e-3, max_grad_norm=1.0)


def test_tensor_lr_graphed_with_steplr(pkg):
    """A captured Adam step under torch's StepLR (which fill_s a tensor lr)
    against eager float-lr steps of the schedule's values."""
    p0, grads = _adam_inputs(steps=1)
    pa = [t.to(DEV).requires_grad_(True) for t in p0]
    pb = [t.to(DEV).requires_grad_(True) for t in p0]
    for p, q, gg in zip(pa, pb, grads[0]):
        p.grad, q.grad = gg.to(DEV), gg.to(DEV)
    lr_t = torch.tensor(1e-2, device=DEV)
    ob = pkg.FusedAdam(pb, lr=lr_t, capturable=True)
    sched = torch.optim.lr_scheduler.StepLR(ob, step_size=2, gamma=0.5)
    graphed = pkg.GraphedStep(ob.step, warmup=1)
    lrs = [float(lr_t)]  # (the warm-up step's)
    for _ in range(5):
        lrs.append(float(lr_t))
        graphed()
        sched.step()
    torch.cuda.synchronize()
    assert ob.param_groups[0]["lr"] is lr_t and len(set(lrs)) == 3  # (the schedule moved)
    assert float(ob.state[pb[0]]["step"]) == len(lrs)
    oa = pkg.FusedAdam(pa, lr=lrs[0], capturable=True)
    for v in lrs:  # (float(lr_t) is already a float32 value)
        oa.param_groups[0]["lr"] = v
        oa.step()
    torch.cuda.synchronize()
    _same_state(oa, pa, ob, pb)


def _np_norm(grads):
    return float(np.sqrt(sum((g.double().numpy() ** 2).sum() for g in grads)))


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_clipping(pkg, wd):
    """Float lrs are float32 values: the clipped step reads lr as a device
    float, the plain step as a double."""
    steps = 3
    p0, grads = _adam_inputs(steps=steps, seed=8)
    lr = float(np.float32(1e-3))
    norms = [_np_norm(gs) for gs in grads]
    max_norm = 0.25 * min(norms)  # below every step's norm

    def run(max_grad_norm, scale_by=None):
        ps = [t.to(DEV).requires_grad_(True) for t in p0]
        opt = pkg.FusedAdam(ps, lr=lr, weight_decay=wd, capturable=True,
                            max_grad_norm=max_grad_norm)
        seen = []
        for k, gs in enumerate(grads):
            for p, gg in zip(ps, gs):
                p.grad = gg.to(DEV)
                if scale_by is not None:
                    p.grad.mul_(scale_by[k][1])
            opt.step()
            if max_grad_norm is not None:
                seen.append((opt.grad_norm.clone(), opt.clip_coef.clone()))
                for p, gg in zip(ps, gs):  # p.grad is not rescaled
                    assert torch.equal(p.grad, gg.to(DEV))
        torch.cuda.synchronize()
        return ps, opt, seen

    pc, oc, seen = run(max_norm)
    for (n, c), want in zip(seen, norms):
        assert n.dtype == torch.float32 and abs(float(n) - want) <= 1e-6 * want
        assert float(c) < 1.0
        # min(1, max_norm / (norm + 1e-6)) in float: one division's rounding apart
        cw = float(np.float32(max_norm) / (np.float32(float(n)) + np.float32(1e-6)))
        assert abs(float(c) - cw) <= 2.0 ** -22 * cw
    # the same bits on a second run
    pc2, oc2, seen2 = run(max_norm)
    for (n, c), (n2, c2) in zip(seen, seen2):
        assert torch.equal(n, n2) and torch.equal(c, c2)
    _same_state(oc, pc, oc2, pc2)
    # the clipped step is the plain step on gradients scaled by clip_coef
    pp, op_, _ = run(None, scale_by=seen)
    _same_state(oc, pc, op_, pp)
    # a bound above the norm: coefficient exactly 1, the unclipped step
    pl, ol, seen_l = run(4.0 * max(norms))
    assert all(float(c) == 1.0 for _, c in seen_l)
    pu, ou, _ = run(None)
    _same_state(ol, pl, ou, pu)
    assert not torch.equal(pc[2].detach(), pu[2].detach())  # (clipping changed the step)


def test_clipping_two_groups_one_norm(pkg):
    p0, grads = _adam_inputs(steps=1, seed=9)
    ps = [t.to(DEV).requires_grad_(True) for t in p0]
    opt = pkg.FusedAdam([dict(params=ps[:2], lr=1e-3), dict(params=ps[2:], lr=3e-3)],
                        capturable=True, max_grad_norm=1.0)
    for p, gg in zip(ps, grads[0]):
        p.grad = gg.to(DEV)
    opt.step()
    want = _np_norm(grads[0])
    assert abs(float(opt.grad_norm) - want) <= 1e-6 * want


def test_clipping_graphed_matches_eager(pkg):
    steps = 4
    p0, grads = _adam_inputs(steps=1, seed=10)
    lr_a, lr_b = torch.tensor(1e-3, device=DEV), torch.tensor(1e-3, device=DEV)
    pa = [t.to(DEV).requires_grad_(True) for t in p0]
    pb = [t.to(DEV).requires_grad_(True) for t in p0]
    for p, q, gg in zip(pa, pb, grads[0]):
        p.grad, q.grad = gg.to(DEV), gg.to(DEV)
    max_norm = 0.5 * _np_norm(grads[0])
    oa = pkg.FusedAdam(pa, lr=lr_a, weight_decay=0.01, capturable=True, max_grad_norm=max_norm)
    ob = pkg.FusedAdam(pb, lr=lr_b, weight_decay=0.01, capturable=True, max_grad_norm=max_norm)

    gd = [gg.to(DEV) for gg in grads[0]]

    def regrad(ps):  # gradients that change with the parameters, formed on the device
        for p, gg in zip(ps, gd):
            p.grad.copy_(gg + 0.1 * p.detach())

    def step_b():
        regrad(pb)
        ob.step()

    for _ in range(steps):
        regrad(pa)
        oa.step()
    graphed = pkg.GraphedStep(step_b, warmup=1)
    for _ in range(steps - 1):
        graphed()
    torch.cuda.synchronize()
    assert torch.equal(oa.grad_norm, ob.grad_norm) and torch.equal(oa.clip_coef, ob.clip_coef)
    assert float(ob.clip_coef) < 1.0
    _same_state(oa, pa, ob, pb)
