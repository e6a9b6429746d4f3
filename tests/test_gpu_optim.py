"""STGCN_FEATURE_OPTIMIZERS on the GPU: FusedAdam with decoupled weight decay
(FusedAdamW) and AMSGrad.

One tensor set serves every case: numel 1, 2047, 2048, 2049 and 5000 (the edges
of the 2048-element chunks and a multi-chunk tail) and the shapes (64, 64, 9, 1),
(1, 18, 18) and (400, 256) -- eight tensors, so the kernel's search of the chunk
table has three levels. Five steps, with fresh gradient tensors every step
unless a test says otherwise, so the tables are rebuilt.

Gates. Against torch on the CPU: FusedAdam's own gate
(tests/test_gpu_train_ops.py), |d| <= 2e-6 |ref| + 1e-7 per element and states
< 1e-6 rel-to-max. Everything that compares two runs of this library compares
bits."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_to_max

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1,), (2047,), (2048,), (2049,), (5000,), (64, 64, 9, 1), (1, 18, 18), (400, 256)]
STEPS = 5
LRS = [0.05, 0.1, 7e-4, 1e-2, 1.234e-5]  # (one per step, for the tensor-lr tests)
AMS_KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def _inputs():
    g = torch.Generator().manual_seed(3)
    p0 = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(STEPS)]
    return p0, grads


P0, GRADS = _inputs()  # shared, never written


def _dev_params():
    return [p.clone().to(DEV).requires_grad_(True) for p in P0]


def _norm(gs):
    return float(np.sqrt(sum((g.double().numpy() ** 2).sum() for g in gs)))


def _adam_gate(opt, dut, opt_ref, ref, keys):
    for a, b in zip(dut, ref):
        d = (a.detach().cpu() - b.detach()).abs()
        assert (d <= 2e-6 * b.detach().abs() + 1e-7).all(), float(d.max())
    for a, b in zip(dut, ref):
        for key in keys:
            err = rel_to_max(opt.state[a][key].cpu().numpy(), opt_ref.state[b][key].numpy())
            assert err < 1e-6, (key, err)
        assert float(opt.state[a]["step"]) == float(opt_ref.state[b]["step"])


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("decoupled,wd,amsgrad", [(True, 0.01, False), (True, 0.1, False),
                                                  (False, 0.0, True), (True, 0.01, True)])
def test_adamw_and_amsgrad_match_torch(pkg, decoupled, wd, amsgrad, capturable):
    ref = [p.clone().requires_grad_(True) for p in P0]
    ref_cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt_ref = ref_cls(ref, lr=1e-2, weight_decay=wd, amsgrad=amsgrad, foreach=False)
    dut = _dev_params()
    cls = pkg.FusedAdamW if decoupled else pkg.FusedAdam
    opt = cls(dut, lr=1e-2, weight_decay=wd, amsgrad=amsgrad, capturable=capturable)
    for gs in GRADS:
        for p, q, g in zip(ref, dut, gs):
            p.grad, q.grad = g.clone(), g.to(DEV)
        opt_ref.step()
        opt.step()
    torch.cuda.synchronize()
    _adam_gate(opt, dut, opt_ref, ref, AMS_KEYS if amsgrad else AMS_KEYS[:2])
    if not amsgrad:
        assert "max_exp_avg_sq" not in opt.state[dut[0]]


def _legacy_adam(pkg, form, max_norm):
    """Five steps through the Adam-format entry points by raw ctypes calls:
    stgcn_adam_build_table over the eight tensors (fresh gradients, so a new
    table every step), then stgcn_adam_step ("host_step"), stgcn_adam_step_dev
    ("device_step") or stgcn_adam_step_dev2 with a device lr and the grad_coef of
    a raw stgcn_grad_norm call. Returns (params, exp_avg, exp_avg_sq, clip_coef)."""
    hl = pkg.hip_lib
    lib = hl.lib()
    dev = torch.device(DEV)
    ps = [p.clone().to(DEV) for p in P0]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    n = len(ps)
    step_dev = torch.zeros((), device=DEV)
    lr_dev = torch.zeros((), device=DEV)
    norm, coef = torch.zeros((), device=DEV), torch.ones((), device=DEV)
    nbytes = lib.stgcn_adam_table_bytes(n)
    for k, (v, gs) in enumerate(zip(LRS, GRADS)):
        grads = [g.to(DEV) for g in gs]
        arr = (hl.AdamTensor * n)(*[
            hl.AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), q.data_ptr(), p.numel())
            for p, g, m, q in zip(ps, grads, ms, vs)])
        host = torch.empty(nbytes, dtype=torch.uint8)
        chunks = ctypes.c_int64(0)
        hl.check(lib.stgcn_adam_build_table(arr, n, ctypes.c_void_p(host.data_ptr()), nbytes,
                                            ctypes.byref(chunks)))
        table = host.to(DEV)
        args = (hl.ptr(table), n, chunks.value)
        if form == "host_step":
            hl.check(lib.stgcn_adam_step(*args, 1e-2, 0.9, 0.999, 1e-8, 0.0, k + 1,
                                         hl.stream_handle(dev)))
        elif form == "device_step":
            hl.check(lib.stgcn_adam_step_dev(*args, 1e-2, 0.9, 0.999, 1e-8, 0.0,
                                             hl.ptr(step_dev), hl.stream_handle(dev)))
        else:
            lr_dev.fill_(v)
            partials = torch.empty(lib.stgcn_grad_norm_bytes(chunks.value) // 8, device=DEV,
                                   dtype=torch.float64)
            hl.check(lib.stgcn_grad_norm(*args, max_norm, hl.ptr(partials), hl.ptr(norm),
                                         hl.ptr(coef), hl.stream_handle(dev)))
            hl.check(lib.stgcn_adam_step_dev2(*args, hl.ptr(lr_dev), hl.ptr(coef), 0.9, 0.999,
                                              1e-8, 0.0, hl.ptr(step_dev),
                                              hl.stream_handle(dev)))
        torch.cuda.synchronize()  # (the table and the gradients live until the step has run)
    return ps, ms, vs, coef


@pytest.mark.parametrize("form", ["host_step", "device_step", "device_lr_and_clip"])
def test_new_route_without_its_options_is_todays_fused_adam(pkg, form):
    """FusedAdam() runs stgcn_opt_step's kernel with neither option in effect;
    stgcn_adam_step / _dev / _dev2, which nothing in Python launches, are called
    here directly (_legacy_adam). The same bits in all three launch forms."""
    max_norm = 0.5 * min(_norm(gs) for gs in GRADS)
    kw = {"host_step": dict(lr=1e-2),
          "device_step": dict(lr=1e-2, capturable=True),
          "device_lr_and_clip": dict(lr=torch.tensor(1e-2, device=DEV), capturable=True,
                                     max_grad_norm=max_norm)}[form]
    pa, ma, va, coef_a = _legacy_adam(pkg, form, max_norm)
    pb = _dev_params()
    ob = pkg.FusedAdam(pb, **kw)
    assert not ob.param_groups[0]["decoupled_weight_decay"] and not ob.param_groups[0]["amsgrad"]
    for v, gs in zip(LRS, GRADS):
        if form == "device_lr_and_clip":
            ob.param_groups[0]["lr"].fill_(v)
        for q, g in zip(pb, gs):
            q.grad = g.to(DEV)
        ob.step()
    torch.cuda.synchronize()
    if form == "device_lr_and_clip":
        assert torch.equal(coef_a, ob.clip_coef) and float(ob.clip_coef) < 1.0
    for a, m, v, b in zip(pa, ma, va, pb):
        assert torch.equal(a, b.detach())
        assert torch.equal(m, ob.state[b]["exp_avg"])
        assert torch.equal(v, ob.state[b]["exp_avg_sq"])


@pytest.mark.parametrize("decoupled", [False, True])
def test_amsgrad_tensor_lr_and_clipping_match_the_plain_step(pkg, decoupled):
    """A tensor lr equals a float lr of the same value, and the clipped step is
    the plain step on gradients pre-scaled by the recorded clip_coef, bit for
    bit (the design of test_gpu_step_state.py::test_clipping)."""
    cls = pkg.FusedAdamW if decoupled else pkg.FusedAdam
    max_norm = 0.25 * min(_norm(gs) for gs in GRADS)  # below every step's norm

    def run(lr_tensor, max_grad_norm=None, prescale=None):
        ps = _dev_params()
        lr = torch.tensor(LRS[0], device=DEV) if lr_tensor else float(np.float32(LRS[0]))
        opt = cls(ps, lr=lr, weight_decay=0.01, amsgrad=True, capturable=True,
                  max_grad_norm=max_grad_norm)
        coefs = []
        for k, (v, gs) in enumerate(zip(LRS, GRADS)):
            if lr_tensor:
                opt.param_groups[0]["lr"].fill_(v)
            else:
                opt.param_groups[0]["lr"] = float(np.float32(v))
            for p, g in zip(ps, gs):
                p.grad = g.to(DEV)
                if prescale is not None:
                    p.grad.mul_(prescale[k])
            opt.step()
            if max_grad_norm is not None:
                coefs.append(opt.clip_coef.clone())
                for p, g in zip(ps, gs):  # p.grad is not rescaled
                    assert torch.equal(p.grad, g.to(DEV))
        torch.cuda.synchronize()
        return ps, opt, coefs

    def same(a, b):
        for p, q in zip(a[0], b[0]):
            assert torch.equal(p.detach(), q.detach())
            for k in AMS_KEYS:
                assert torch.equal(a[1].state[p][k], b[1].state[q][k]), k

    plain = run(False)
    same(plain, run(True))
    clipped = run(True, max_grad_norm=max_norm)
    assert all(float(c) < 1.0 for c in clipped[2])
    same(clipped, run(True, prescale=clipped[2]))
    assert not torch.equal(clipped[0][4].detach(), plain[0][4].detach())
    loose = run(True, max_grad_norm=4.0 * max(_norm(gs) for gs in GRADS))
    assert all(float(c) == 1.0 for c in loose[2])
    same(loose, plain)


def _moved(sd, dev):
    sd = dict(sd)
    sd["state"] = {k: {kk: (vv.to(dev) if kk != "step" else vv.clone()) for kk, vv in v.items()}
                   for k, v in sd["state"].items()}
    return sd


@pytest.mark.parametrize("direction", ["torch_to_fused", "fused_to_torch"])
def test_amsgrad_state_dicts_interchange(pkg, direction):
    g = torch.Generator().manual_seed(4)
    w = torch.randn(32, 16, generator=g)
    g1, g2 = torch.randn(32, 16, generator=g), torch.randn(32, 16, generator=g)
    ref = [w.clone().requires_grad_(True)]
    dut = [w.clone().to(DEV).requires_grad_(True)]
    opt_ref = torch.optim.Adam(ref, lr=1e-3, amsgrad=True, foreach=False)
    opt = pkg.FusedAdam(dut, lr=1e-3, amsgrad=True)
    first, second = (opt, opt_ref) if direction == "fused_to_torch" else (opt_ref, opt)
    src, dst = (dut, ref) if direction == "fused_to_torch" else (ref, dut)
    src[0].grad = g1.to(src[0].device)
    first.step()
    second.load_state_dict(_moved(first.state_dict(), dst[0].device))
    with torch.no_grad():
        dst[0].copy_(src[0].detach().to(dst[0].device))
    ref[0].grad, dut[0].grad = g2.clone(), g2.to(DEV)
    opt_ref.step()
    opt.step()
    torch.cuda.synchronize()
    assert not np.allclose(dut[0].detach().cpu().numpy(), w.numpy(), rtol=1e-3, atol=0)
    assert np.allclose(dut[0].detach().cpu().numpy(), ref[0].detach().numpy(), rtol=2e-6,
                       atol=1e-8)
    assert np.allclose(opt.state[dut[0]]["max_exp_avg_sq"].cpu().numpy(),
                       opt_ref.state[ref[0]]["max_exp_avg_sq"].numpy(), rtol=2e-6, atol=1e-12)


def _placed(t, off):
    """A copy of t on the GPU that starts ``off`` floats past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 4, device=DEV)
    assert flat.data_ptr() % 16 == 0
    v = flat[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return v


def test_offset_placement_gives_the_same_bits(pkg):
    """Parameters, gradients and state 4, 8 and 12 bytes off a 16-byte boundary
    (views into flat buckets are placed like that) against aligned ones."""
    def make(ps):
        return pkg.FusedAdamW(ps, lr=1e-2, weight_decay=0.01, amsgrad=True)

    pa = _dev_params()
    oa = make(pa)
    pb = [_placed(p, 1 + i % 3).requires_grad_(True) for i, p in enumerate(P0)]
    ob = make(pb)
    for i, p in enumerate(pb):
        ob.state[p] = {"step": torch.tensor(0.0)}
        for j, k in enumerate(AMS_KEYS):
            ob.state[p][k] = _placed(torch.zeros(p.shape), 1 + (i + j + 2) % 3)
    for gs in GRADS:
        for i, (p, q, g) in enumerate(zip(pa, pb, gs)):
            p.grad, q.grad = g.to(DEV), _placed(g, 1 + (i + 1) % 3)
        oa.step()
        ob.step()
    torch.cuda.synchronize()
    for a, b in zip(pa, pb):
        assert b.data_ptr() % 16 != 0
        assert torch.equal(a.detach(), b.detach())
        for k in AMS_KEYS:
            assert ob.state[b][k].data_ptr() % 16 != 0
            assert torch.equal(oa.state[a][k], ob.state[b][k]), k


@pytest.mark.parametrize("decoupled", [False, True])
def test_graphed_step_on_plain_tensors(pkg, decoupled):
    """Static gradient tensors; 2 eager steps, a capture, 3 replays with the lr
    written by fill_ and new gradients copied in between them, against 5 eager
    steps."""
    max_norm = 0.5 * min(_norm(gs) for gs in GRADS)
    cls = pkg.FusedAdamW if decoupled else pkg.FusedAdam
    pa, pb = _dev_params(), _dev_params()
    lr_a, lr_b = torch.tensor(LRS[0], device=DEV), torch.tensor(LRS[0], device=DEV)
    oa = cls(pa, lr=lr_a, amsgrad=True, capturable=True, max_grad_norm=max_norm)
    ob = cls(pb, lr=lr_b, amsgrad=True, capturable=True, max_grad_norm=max_norm)
    for ps in (pa, pb):
        for p in ps:
            p.grad = torch.zeros_like(p)

    def load(ps, lr, k):
        lr.fill_(LRS[k])
        for p, g in zip(ps, GRADS[k]):
            p.grad.copy_(g.to(DEV))

    for k in range(STEPS):
        load(pa, lr_a, k)
        oa.step()
    for k in range(2):
        load(pb, lr_b, k)
        ob.step()
    graphed = pkg.GraphedStep(ob.step, warmup=0)
    for k in range(2, STEPS):
        load(pb, lr_b, k)
        graphed()
    torch.cuda.synchronize()
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
        for k in AMS_KEYS:
            assert torch.equal(oa.state[a][k], ob.state[b][k]), k
    assert torch.equal(oa.clip_coef, ob.clip_coef) and float(ob.clip_coef) < 1.0
    assert float(ob.state[pb[0]]["step"]) == float(STEPS)


def test_capture_without_an_eager_step_raises(pkg):
    ps = _dev_params()
    for p, g in zip(ps, GRADS[0]):
        p.grad = g.to(DEV)
    opt = pkg.FusedAdam(ps, lr=1e-2, amsgrad=True, capturable=True)
    with pytest.raises(RuntimeError, match="eager step"):
        pkg.GraphedStep(opt.step, warmup=0)
    torch.cuda.synchronize()


def test_graphed_adamw_amsgrad_step_on_the_stack(pkg):
    """test_gpu_graph.py::test_graphed_step_matches_eager's stack (N = 4, T = 32,
    V = 18, K = 1, f16x2) under FusedAdamW(amsgrad=True): five eager steps equal
    2 warm-up steps + 3 replays in loss, logits, every state_dict entry and the
    optimizer's state."""
    N, T, V = 4, 32, 18
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, 3, T, V, generator=g).to(DEV)
    labels = torch.randint(0, 10, (N,), generator=g).to(DEV)
    gr = pkg.graph
    A = gr.get_normalized_adjacency_matrices(0, 1, graph=gr.graph_for(V))

    def make():
        torch.manual_seed(0)
        m = pkg.STGCNStack(3, 10, A, gemm_dtype=torch.float32, f32_gemm="f16x2").to(DEV)
        opt = pkg.FusedAdamW(list(m.parameters()), lr=1e-3, amsgrad=True, capturable=True)

        def step():
            opt.zero_grad(set_to_none=True)
            loss, logits = m.forward_loss(x, labels)
            loss.backward()
            opt.step()
            return loss, logits
        return m, opt, step

    ma, oa, step_a = make()
    mb, ob, step_b = make()
    w0 = next(iter(ma.parameters())).detach().clone()
    for _ in range(5):
        la, ga = step_a()
    graphed = pkg.GraphedStep(step_b, warmup=2)
    for _ in range(3):
        lb, gb = graphed()
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    for (ka, a), (kb, b) in zip(ma.state_dict().items(), mb.state_dict().items()):
        assert ka == kb
        assert torch.equal(a, b), ka
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    assert sorted(sa) == sorted(sb) and len(sa) > 0
    for k in sa:
        for key in AMS_KEYS:
            assert torch.equal(sa[k][key], sb[k][key]), (k, key)
    assert not torch.equal(next(iter(ma.parameters())).detach(), w0)  # (it trained)
