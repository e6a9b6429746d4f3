"""STGCN_FEATURE_HEAD_LOSS on the GPU: the evaluation head with
F.cross_entropy's ``weight=`` / ``label_smoothing=`` / ignored labels
(stgcn_head_eval_loss / _u, train_ops.head_eval, STGCNStack.eval_step) against
F.cross_entropy on the CPU in fp64 over F.linear(avg_pool2d(...)), with the
gates of test_gpu_train_ops.py::test_head_matches_torch (loss 1e-5 relative,
logits 1e-5 rel-to-max); the default options against stgcn_head_eval bit for
bit; D == 0; the metrics block; a HIP graph; poisoned, guard-banded buffers."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import poison
import test_gpu_eval as ev
from conftest import rel_to_max

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# one active lane (2 classes), classes crossing the 256-thread stride by one, L = 1,
# L no multiple of 64
GRID = [(5, 32, 1, 18, 2), (3, 64, 4, 50, 7), (4, 64, 3, 25, 257), (8, 256, 5, 18, 400)]
_CASES = {}


def _case(shape):
    """The inputs of a grid shape, formed once and left unchanged: U, BN2
    parameters, y = ReLU(BN2(U)), W, b, a weight vector in [0.2, 1.2] with one
    class at 0, labels (clip 0 the zero-weight class; one or two ignored), and
    the fp64 logits of F.linear(avg_pool2d(y))."""
    if shape not in _CASES:
        N, C, T, V, classes = shape
        g = torch.Generator().manual_seed(sum(shape))
        U = torch.randn(N, C, T, V, generator=g)
        stats2 = torch.cat([torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5])
        g2, b2 = torch.randn(C, generator=g), torch.randn(C, generator=g)
        W = torch.randn(classes, C, generator=g) * 0.3
        b = torch.randn(classes, generator=g) * 0.3
        w = torch.rand(classes, generator=g) + 0.2
        zero = int(torch.randint(0, classes, (1,), generator=g))
        w[zero] = 0.0
        lab = torch.randint(0, classes, (N,), generator=g)
        lab[lab == zero] = (zero + 1) % classes
        lab[0] = zero
        lab[1] = -100
        if N >= 4:
            lab[3] = classes
        y = ev._y_of(U, stats2, g2, b2).contiguous()
        pooled = F.avg_pool2d(y.double(), (T, V)).view(N, C)
        logits64 = F.linear(pooled, W.double(), b.double())
        _CASES[shape] = dict(U=U, stats2=stats2, g2=g2, b2=b2, y=y, W=W, b=b, w=w, lab=lab,
                             logits64=logits64, zero=zero)
    return _CASES[shape]


def _torch_loss(logits64, lab, classes, w, eps, reduction="mean"):
    tgt = torch.where((lab >= 0) & (lab < classes), lab, torch.full_like(lab, -100))
    return F.cross_entropy(logits64, tgt, weight=None if w is None else w.double(),
                           label_smoothing=eps, ignore_index=-100, reduction=reduction)


def _dev(c, *names):
    return [c[n].to(DEV) for n in names]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("shape", GRID)
def test_parity_grid(pkg, shape, eps, weighted):
    N, C, T, V, classes = shape
    c = _case(shape)
    U, stats2, g2, b2, y, W, b, lab = _dev(c, "U", "stats2", "g2", "b2", "y", "W", "b", "lab")
    w = c["w"] if weighted else None
    want = _torch_loss(c["logits64"], c["lab"], classes, w, eps)
    wantv = _torch_loss(c["logits64"], c["lab"], classes, w, eps, "none")
    assert torch.isfinite(want) and want.item() > 0
    wd = None if w is None else w.to(DEV)
    loss, logits, pred, lossv = pkg.train_ops.head_eval(y, W, b, lab, weight=wd,
                                                        label_smoothing=eps)
    lu, lgu, pu, lvu = pkg.train_ops.head_eval(None, W, b, lab, from_u=(U, stats2, g2, b2),
                                               weight=wd, label_smoothing=eps)
    ignored = (c["lab"] < 0) | (c["lab"] >= classes)
    assert ignored.sum() == (2 if N >= 4 else 1)
    # (the U form pools ReLU(BN2(U)) with the block's own fused arithmetic, which
    # torch's y above need not match to the bit: each form against the reference)
    for form, (ls, lg, pr, lv) in (("y", (loss, logits, pred, lossv)), ("U", (lu, lgu, pu, lvu))):
        err = abs(ls.item() - want.item()) / abs(want.item())
        rl, rv = rel_to_max(lg.cpu(), c["logits64"]), rel_to_max(lv.cpu(), wantv)
        print(f"{form}: loss {ls.item():.8g} want {want.item():.8g} rel {err:.2e}; "
              f"logits {rl:.2e}; lossv {rv:.2e}")
        assert err <= 1e-5
        assert rl < 1e-5
        assert rv < 1e-5  # (per clip: the same kind of quantity under the same measure)
        assert not lv.cpu()[ignored].any()
        assert torch.equal(pr.cpu().long(), lg.cpu().argmax(1))  # (no ties in random logits)


def _raw(pkg, c, lab, flags, eps, w=None, metrics=None, topk=1, from_u=False):
    """stgcn_head_eval_loss / _u itself: (loss, logits, pred, lossv, denom)."""
    hl = pkg.hip_lib
    y, W, b = _dev(c, "y", "W", "b")
    N, C = y.shape[0], y.shape[1]
    classes = W.shape[0]
    d = hl.LossDesc(N, C, y[0, 0].numel(), classes, topk, flags, eps)
    pooled = torch.empty(N, C, device=DEV)
    logits = torch.empty(N, classes, device=DEV)
    lossv, loss, denom = (torch.empty(N, device=DEV), torch.empty((), device=DEV),
                          torch.empty((), device=DEV))
    pred = torch.empty(N, device=DEV, dtype=torch.int32)
    tail = (W, b, w, lab, pooled, logits, lossv, denom, loss, pred,
            None if metrics is None else metrics.buf)
    if from_u:
        hl.check(hl.lib().stgcn_head_eval_loss_u(ctypes.byref(d), *[hl.ptr(t) for t in (
            *_dev(c, "U", "stats2", "g2", "b2"), *tail)], hl.stream_handle(y.device)))
    else:
        hl.check(hl.lib().stgcn_head_eval_loss(ctypes.byref(d), *[hl.ptr(t) for t in (
            y, *tail)], hl.stream_handle(y.device)))
    return loss, logits, pred, lossv, denom


def _raw_eval(pkg, c, lab, metrics=None, topk=1, from_u=False):
    """stgcn_head_eval / _u itself (nothing in Python calls them: head_eval goes
    through stgcn_head_eval_loss): (loss, logits, pred, lossv)."""
    hl = pkg.hip_lib
    y, W, b = _dev(c, "y", "W", "b")
    N, C = y.shape[0], y.shape[1]
    classes = W.shape[0]
    d = hl.EvalDesc(N, C, y[0, 0].numel(), classes, topk)
    pooled = torch.empty(N, C, device=DEV)
    logits = torch.empty(N, classes, device=DEV)
    lossv, loss = torch.empty(N, device=DEV), torch.empty((), device=DEV)
    pred = torch.empty(N, device=DEV, dtype=torch.int32)
    tail = (W, b, lab, pooled, logits, lossv, loss, pred,
            None if metrics is None else metrics.buf)
    if from_u:
        hl.check(hl.lib().stgcn_head_eval_u(ctypes.byref(d), *[hl.ptr(t) for t in (
            *_dev(c, "U", "stats2", "g2", "b2"), *tail)], hl.stream_handle(y.device)))
    else:
        hl.check(hl.lib().stgcn_head_eval(ctypes.byref(d), *[hl.ptr(t) for t in (
            y, *tail)], hl.stream_handle(y.device)))
    return loss, logits, pred, lossv


def test_one_clip(pkg):
    """N = 1, one valid clip with a weight: D = w[y], so the loss is the clip's
    unweighted one."""
    shape = (3, 64, 4, 50, 7)
    c = {k: (v[:1] if k in ("U", "y", "lab", "logits64") else v) for k, v in _case(shape).items()}
    lab = torch.tensor([(c["zero"] + 2) % 7])
    want = _torch_loss(c["logits64"], lab, 7, c["w"], 0.0)
    assert torch.isfinite(want)
    loss, logits, pred, lossv, denom = _raw(pkg, c, lab.to(DEV), 1, 0.0, c["w"].to(DEV))
    assert denom.item() == c["w"][lab[0]].item()
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item()), (loss.item(), want.item())
    plain, _, _, _ = pkg.train_ops.head_eval(c["y"].to(DEV), c["W"].to(DEV), c["b"].to(DEV),
                                             lab.to(DEV))
    assert abs(loss.item() - plain.item()) <= 2e-7 * abs(plain.item())  # (w[y] nll / w[y])


@pytest.mark.parametrize("shape", [(8, 256, 5, 18, 400), (3, 64, 4, 50, 7)])
@pytest.mark.parametrize("ignored", [False, True])
@pytest.mark.parametrize("from_u", [False, True])
def test_default_options_have_the_eval_heads_bits(pkg, shape, ignored, from_u):
    """eps = 0 and no weight through the new entry point: loss, logits, lossv,
    pred and the metrics block of stgcn_head_eval, bit for bit; D is the number
    of valid clips."""
    to = pkg.train_ops
    c = _case(shape)
    classes = shape[4]
    g = torch.Generator().manual_seed(3)
    lab = c["lab"] if ignored else torch.randint(0, classes, (shape[0],), generator=g)
    lab = lab.to(DEV)
    y, W, b = _dev(c, "y", "W", "b")
    m0, m1 = to.EvalMetrics(classes, 3, device=DEV), to.EvalMetrics(classes, 3, device=DEV)
    fu = tuple(_dev(c, "U", "stats2", "g2", "b2")) if from_u else None
    y = None if from_u else y
    loss0, logits0, pred0, lossv0 = _raw_eval(pkg, c, lab, metrics=m0, topk=3, from_u=from_u)
    loss, logits, pred, lossv, denom = _raw(pkg, c, lab, 0, 0.0, metrics=m1, topk=3,
                                            from_u=from_u)
    assert torch.equal(loss, loss0) and torch.equal(logits, logits0)
    assert torch.equal(lossv, lossv0) and torch.equal(pred, pred0)
    assert torch.equal(m0.buf, m1.buf)
    assert denom.item() == int(((lab >= 0) & (lab < classes)).sum())
    # the Python route, with its defaults left out and spelled out
    for kw in ({}, dict(weight=None, label_smoothing=0.0)):
        loss2, logits2, pred2, lossv2 = to.head_eval(y, W, b, lab, from_u=fu, **kw)
        assert torch.equal(loss2, loss0) and torch.equal(logits2, logits0)
        assert torch.equal(lossv2, lossv0) and torch.equal(pred2, pred0)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_zero_denominator(pkg, eps):
    """Every label ignored, and every label of a zero-weight class: loss exactly 0
    (torch: NaN), D = 0, and the metrics block counts the clips all the same."""
    to = pkg.train_ops
    shape = (4, 64, 3, 25, 257)
    c = _case(shape)
    y, W, b = _dev(c, "y", "W", "b")
    w = c["w"].to(DEV)
    for lab in (torch.tensor([-100, 257, -1, 2 ** 40]), torch.full((4,), c["zero"])):
        m = to.EvalMetrics(257, 1, device=DEV)
        loss, logits, pred, lossv, denom = _raw(pkg, c, lab.to(DEV), 1, eps, w, metrics=m)
        assert loss.item() == 0.0 and denom.item() == 0.0
        assert torch.isfinite(lossv).all()
        r = m.result()
        valid = int(((lab >= 0) & (lab < 257)).sum())
        assert (r["batches"], r["clips"], r["invalid"]) == (1, valid, 4 - valid)
        assert r["val_loss"] == 0.0
        if not valid:
            assert not lossv.any()
        loss2, _, _, _ = to.head_eval(y, W, b, lab.to(DEV), weight=w, label_smoothing=eps)
        assert loss2.item() == 0.0


def _accumulate(pkg, place, metrics_buf=None):
    """Three batches (4, 4 and 3 clips; ties in the second batch's weights, an
    ignored label in the third) with class weights, eps = 0.1 and topk = 3 into
    one metrics block, checked against a host recount from the returned logits
    and per-clip losses. place(t, name): tensor to the device."""
    to = pkg.train_ops
    classes, topk, eps = 10, 3, 0.1
    m = to.EvalMetrics(classes, topk, device=DEV, buf=metrics_buf)
    w_host = torch.rand(classes, generator=torch.Generator().manual_seed(9)) + 0.2
    w_host[7] = 0.0
    w = place(w_host, "weight")
    want = np.zeros(5, dtype=np.int64)
    conf = np.zeros((classes, classes), dtype=np.int64)
    s_loss = s_bloss = s_bacc = 0.0
    out = []
    for i, n in enumerate((4, 4, 3)):
        U, stats2, g2, b2, W, b, lab = ev._head_inputs(n, 48, 54, classes, 20 + i, ties=(i == 1))
        if i == 2:
            lab[1] = classes
        U, stats2, g2, b2, W, b, labd = [place(t, k) for t, k in zip(
            (U, stats2, g2, b2, W, b, lab), ("U", "stats2", "g2", "b2", "W", "b", "labels"))]
        if i == 0:
            y = place(ev._y_of(U, stats2, g2, b2).contiguous(), "y")
            loss, logits, pred, lossv = to.head_eval(y, W, b, labd, metrics=m, weight=w,
                                                     label_smoothing=eps)
        else:
            loss, logits, pred, lossv = to.head_eval(None, W, b, labd, metrics=m,
                                                     from_u=(U, stats2, g2, b2), weight=w,
                                                     label_smoothing=eps)
        lg, lv = logits.cpu().numpy(), lossv.cpu().numpy().astype(np.float64)
        p, (valid, invalid, correct, hits, cm) = ev._np_rules(lg, lab.numpy(), topk)
        assert np.array_equal(pred.cpu().numpy(), p)
        ok = (lab.numpy() >= 0) & (lab.numpy() < classes)
        D = w_host.double().numpy()[lab.numpy()[ok]].sum()
        ref = _torch_loss(torch.from_numpy(lg).double(), lab, classes, w_host, eps).item()
        assert abs(loss.item() - ref) <= 1e-5 * abs(ref), (i, loss.item(), ref)
        assert abs(loss.item() - lv[ok].sum() / D) <= 6e-8 * abs(ref)  # (one float rounding)
        want += np.array([1, valid, correct, hits, invalid])
        conf += cm
        s_loss += lv[ok].sum()
        s_bloss += lv[ok].sum() / D
        s_bacc += correct / valid
        out += [loss, logits, pred, lossv]
    r = m.result()
    got = (r["batches"], r["clips"], r["correct"], r["topk_hits"], r["invalid"])
    assert got == tuple(int(v) for v in want), (got, want)
    assert np.array_equal(r["confusion"].numpy(), conf)
    for key, val in (("loss", s_loss / want[1]), ("val_loss", s_bloss / 3),
                     ("val_acc", s_bacc / 3)):
        assert abs(r[key] - val) <= 1e-12 * abs(val), (key, r[key], val)
    return [t.clone() for t in out] + [m.buf.clone()]


def test_metrics_with_options(pkg):
    _accumulate(pkg, lambda t, name: t.to(DEV))


def test_poisoned(pkg):
    """The same with every output, the metrics block and pred in poisoned,
    guard-banded memory and the inputs (the weight vector too) guarded and
    unchanged: bit-identical to the clean run under each fill."""
    clean = _accumulate(pkg, lambda t, name: t.to(DEV))
    nbytes = pkg.hip_lib.lib().stgcn_eval_metrics_bytes(10)
    for fill in poison.FILLS:
        with poison.poisoned(pkg, fill):
            buf = poison.empty(nbytes, fill, dtype=torch.uint8, device=DEV, name="metrics")
            got = _accumulate(pkg, lambda t, name: poison.guarded(t, fill, DEV, name=name), buf)
            torch.cuda.synchronize()
        poison.check_guards()
        poison.check_inputs()
        for a, b in zip(got, clean):
            assert torch.equal(a, b), f"fill {fill:#04x}"


@pytest.mark.parametrize("name", ["v18-f16x2", "v18-residual", "v25k3-bf16"])
def test_eval_step_with_options(pkg, name):
    """eval_step(weight=, label_smoothing=) in the stack, from U ("head") and
    from a written y (residual): the logits are the default call's bits, the
    loss is F.cross_entropy's of those logits in fp64, and the default call is
    unchanged by spelling the defaults out."""
    m, _, _ = ev._stack(pkg, name)
    x, lab = ev._inputs(5, 20, ev.CONFIGS[name][0])
    lab[2] = -100
    loss0, logits0 = m.eval_step(x, lab)
    loss0, logits0 = loss0.clone(), logits0.clone()
    loss1, logits1 = m.eval_step(x, lab, weight=None, label_smoothing=0.0)
    assert torch.equal(loss1, loss0) and torch.equal(logits1, logits0)
    w = torch.rand(10, generator=torch.Generator().manual_seed(4)) + 0.2
    w[int(lab[0])] = 0.0
    loss, logits = m.eval_step(x, lab, weight=w.to(DEV), label_smoothing=0.1)
    assert m.last_eval_plan[-1] == ("written" if name == "v18-residual" else "head")
    assert torch.equal(logits, logits0)
    want = _torch_loss(logits.cpu().double(), lab.cpu(), 10, w, 0.1).item()
    assert np.isfinite(want)
    assert abs(loss.item() - want) <= 1e-5 * abs(want), (loss.item(), want)
    assert loss.item() != loss0.item()


def test_eval_step_graph_with_options(pkg):
    """The step with weight, smoothing and a metrics block captured in a HIP
    graph; labels rewritten in the static buffer between three replays (ignored
    ones among them): losses and the metrics block equal the eager calls' bits."""
    to = pkg.train_ops
    m, _, _ = ev._stack(pkg, "v18-f16x2")
    x, lab = ev._inputs(4, 20, 18)
    w = (torch.rand(10, generator=torch.Generator().manual_seed(6)) + 0.2).to(DEV)
    labels = [lab.clone(), torch.tensor([1, -100, 3, 10], device=DEV),
              torch.tensor([-1, -1, 12, -100], device=DEV)]
    eager = to.EvalMetrics(10, 3, device=DEV)
    want = [m.eval_step(x, l, eager, weight=w, label_smoothing=0.1)[0].clone() for l in labels]
    static = lab.clone()
    metrics = to.EvalMetrics(10, 3, device=DEV)
    step = to.GraphedStep(lambda: m.eval_step(x, static, metrics, weight=w, label_smoothing=0.1),
                          warmup=2)
    metrics.reset()
    for l, wl in zip(labels, want):
        static.copy_(l)
        loss, _ = step()
        assert torch.equal(loss, wl)
    torch.cuda.synchronize()
    assert want[2].item() == 0.0
    assert torch.equal(metrics.buf.cpu(), eager.buf.cpu())


def test_weight_on_the_host_is_refused(pkg):
    c = _case((3, 64, 4, 50, 7))
    y, W, b, lab = _dev(c, "y", "W", "b", "lab")
    with pytest.raises(RuntimeError, match="weight: expected a contiguous float32 GPU tensor"):
        pkg.train_ops.head_eval(y, W, b, lab, weight=c["w"])
    with pytest.raises(ValueError, match="weight: expected 7 elements"):
        pkg.train_ops.head_eval(y, W, b, lab, weight=torch.ones(8, device=DEV))
    with pytest.raises(ValueError, match="label_smoothing"):
        pkg.train_ops.head_eval(y, W, b, lab, label_smoothing=1.5)
