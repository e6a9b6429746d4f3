"""The evaluation step on the GPU: the scoring head (stgcn_head_eval / _u and
the metrics block) against the training head and a numpy restatement of its
rules, and ``STGCNStack.eval_step`` (eval chaining through U, nothing kept for
a backward) against the existing eval route and the fp64 oracle, eagerly, in a
HIP graph and on poisoned, guard-banded buffers."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import poison
from conftest import rel_to_max
from oracle import ref_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# --- the head ----------------------------------------------------------------------

def _np_rules(logits, labels, topk):
    """The head's rules restated: pred, and (valid, invalid, correct, hits, confusion)."""
    logits, labels = np.asarray(logits), np.asarray(labels)
    N, K = logits.shape
    pred = np.array([int(np.flatnonzero(r == r.max())[0]) for r in logits], dtype=np.int64)
    conf = np.zeros((K, K), dtype=np.int64)
    valid = invalid = correct = hits = 0
    idx = np.arange(K)
    for n in range(N):
        y = int(labels[n])
        if not 0 <= y < K:
            invalid += 1
            continue
        valid += 1
        correct += int(pred[n] == y)
        r = logits[n]
        hits += int(((r > r[y]) | ((r == r[y]) & (idx < y))).sum() < topk)
        conf[y, pred[n]] += 1
    return pred, (valid, invalid, correct, hits, conf)


def _head_inputs(N, C, L, classes, seed, ties=False):
    g = torch.Generator().manual_seed(seed)
    T = 2 if L % 2 == 0 else 5
    U = torch.randn(N, C, T, L // T, generator=g)
    stats2 = torch.cat([torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5])
    g2, b2 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    g2[::7] = 0.0
    W = torch.randn(classes, C, generator=g) * 0.1
    b = torch.randn(classes, generator=g) * 0.1
    if ties:  # classes 3, 5, 7 and 1, 2: bit-equal logits; the triple is the maximum
        for grp, lift in (((3, 5, 7), 50.0), ((1, 2), 0.0)):
            w0, b0 = W[grp[0]].clone(), float(b[grp[0]]) + lift
            for j in grp:
                W[j], b[j] = w0, b0
    lab = torch.randint(0, classes, (N,), generator=g)
    return U, stats2, g2, b2, W, b, lab


def _y_of(U, stats2, g2, b2):
    """y = ReLU(BN2(U)) with the output pass's arithmetic (k_bn_relu_fwd)."""
    C = U.shape[1]
    sh = (1, C, 1, 1)
    a = (stats2[C:] * g2).view(sh)
    return torch.clamp_min((U - stats2[:C].view(sh)) * a + b2.view(sh), 0.0)


def _train_head(pkg, src, W, b, lab, from_u=None):
    """stgcn_head_fwd / _u through the library: (logits, lossv, loss)."""
    hl = pkg.hip_lib
    lib = hl.lib()
    N, C = src.shape[0], src.shape[1]
    L, classes = src[0, 0].numel(), W.shape[0]
    d = hl.HeadDesc(N, C, L, classes)
    pooled = torch.empty(N, C, device=DEV)
    logits = torch.empty(N, classes, device=DEV)
    lossv = torch.empty(N, device=DEV)
    loss = torch.empty((), device=DEV)
    if from_u is None:
        hl.check(lib.stgcn_head_fwd(ctypes.byref(d), *[hl.ptr(t) for t in (
            src, W, b, lab, pooled, logits, lossv, loss)], hl.stream_handle(src.device)))
    else:
        hl.check(lib.stgcn_head_fwd_u(ctypes.byref(d), *[hl.ptr(t) for t in (
            src, *from_u, W, b, lab, pooled, logits, lossv, loss)],
            hl.stream_handle(src.device)))
    return logits, lossv, loss


def _check_rules(pkg, metrics, batches, topk):
    """The metrics block against the rules over ``batches`` of (logits, lossv,
    labels, pred) the head returned; integers exact, sums within 1e-12."""
    classes = metrics.classes
    want = np.zeros(5, dtype=np.int64)
    conf = np.zeros((classes, classes), dtype=np.int64)
    s_loss = s_bloss = s_bacc = 0.0
    for logits, lossv, lab, pred in batches:
        lg, lv, lb = logits.cpu().numpy(), lossv.cpu().numpy().astype(np.float64), lab.cpu().numpy()
        p, (valid, invalid, correct, hits, c) = _np_rules(lg, lb, topk)
        assert np.array_equal(pred.cpu().numpy(), p)
        ok = (lb >= 0) & (lb < classes)
        assert np.all(lv[~ok] == 0.0)
        want += np.array([1, valid, correct, hits, invalid])
        conf += c
        s_loss += lv[ok].sum()
        if valid:
            s_bloss += lv[ok].sum() / valid
            s_bacc += correct / valid
    r = metrics.result()
    got = (r["batches"], r["clips"], r["correct"], r["topk_hits"], r["invalid"])
    assert got == tuple(int(v) for v in want), (got, want)
    assert np.array_equal(r["confusion"].numpy(), conf)
    clips, nb = int(want[1]), int(want[0])
    for key, val in (("loss", s_loss / max(clips, 1)), ("val_loss", s_bloss / nb),
                     ("val_acc", s_bacc / nb)):
        assert abs(r[key] - val) <= 1e-12 * abs(val), (key, r[key], val)
    assert r["acc"] == want[2] / max(clips, 1) and r["topk_acc"] == want[3] / max(clips, 1)
    return r


@pytest.mark.parametrize("classes", [2, 10, 65, 400])
@pytest.mark.parametrize("N,C,L", [(n, c, l) for n in (1, 5) for c in (48, 256)
                                   for l in (54, 125)])
def test_head_eval_matches_training_head(pkg, N, C, L, classes):
    """logits, lossv and loss bit-identical to stgcn_head_fwd / _fwd_u and to
    StgcnHeadFn, in the y form and the U form; pred and the counts by the rules."""
    to = pkg.train_ops
    U, stats2, g2, b2, W, b, lab = (t.to(DEV) for t in _head_inputs(
        N, C, L, classes, seed=N * 1000 + C + L + classes))
    y = _y_of(U, stats2, g2, b2).contiguous()
    for topk in sorted({1, min(5, classes)}):
        for from_u in (None, (U, stats2, g2, b2)):
            m = to.EvalMetrics(classes, topk, device=DEV)
            loss, logits, pred, lossv = to.head_eval(None if from_u else y, W, b, lab,
                                                     metrics=m, from_u=from_u)
            rl, rv, rloss = _train_head(pkg, U if from_u else y, W, b, lab,
                                        from_u and from_u[1:])
            assert torch.equal(logits, rl) and torch.equal(lossv, rv) and torch.equal(loss, rloss)
            with torch.no_grad():
                ph = torch.empty(1, device=DEV).expand(U.shape)
                floss, flogits = to.StgcnHeadFn.apply(ph if from_u else y, W, b, lab, from_u)
            assert torch.equal(logits, flogits) and torch.equal(loss, floss)
            _check_rules(pkg, m, [(logits, lossv, lab, pred)], topk)


@pytest.mark.parametrize("label", [3, 5, 7, 1, 2, 0])
def test_head_eval_ties(pkg, label):
    """Three bit-equal maximal logits (classes 3, 5, 7) and two bit-equal ones
    (1, 2), the label on the first, middle and last of them: the prediction is
    the lowest index, and an equal logit ranks before the label only from a
    lower index."""
    to = pkg.train_ops
    classes, N = 10, 4
    U, stats2, g2, b2, W, b, _ = (t.to(DEV) for t in _head_inputs(N, 48, 54, classes, 7, True))
    y = _y_of(U, stats2, g2, b2).contiguous()
    lab = torch.full((N,), label, device=DEV, dtype=torch.int64)
    for topk in (1, 2, 3, 5):
        m = to.EvalMetrics(classes, topk, device=DEV)
        loss, logits, pred, lossv = to.head_eval(y, W, b, lab, metrics=m)
        lg = logits.cpu().numpy()
        assert np.all(lg[:, 3] == lg[:, 5]) and np.all(lg[:, 5] == lg[:, 7])
        assert np.all(lg[:, 1] == lg[:, 2]) and np.all(lg.argmax(1) == 3)
        assert pred.tolist() == [3] * N
        r = _check_rules(pkg, m, [(logits, lossv, lab, pred)], topk)
        if label in (3, 5, 7):  # rank 0, 1, 2 among the tied maxima
            assert r["topk_hits"] == (N if (3, 5, 7).index(label) < topk else 0)
            assert r["correct"] == (N if label == 3 else 0)


def test_head_eval_invalid_labels(pkg):
    to = pkg.train_ops
    classes, N = 10, 5
    U, stats2, g2, b2, W, b, _ = (t.to(DEV) for t in _head_inputs(N, 48, 125, classes, 11))
    y = _y_of(U, stats2, g2, b2).contiguous()
    lab = torch.tensor([-1, 3, classes, 2 ** 40, 1], device=DEV)
    m = to.EvalMetrics(classes, 5, device=DEV)
    loss, logits, pred, lossv = to.head_eval(y, W, b, lab, metrics=m)
    r = _check_rules(pkg, m, [(logits, lossv, lab, pred)], 5)
    assert (r["clips"], r["invalid"]) == (2, 3)
    tgt = torch.tensor([-100, 3, -100, -100, 1])
    want = F.cross_entropy(logits.cpu().double(), tgt, ignore_index=-100).item()
    assert abs(loss.item() - want) <= 1e-6 * abs(want), (loss.item(), want)
    # the valid clips' logits and losses are those of the training head
    rl, rv, _ = _train_head(pkg, y, W, b, lab.clamp(0, classes - 1))
    assert torch.equal(logits, rl) and torch.equal(lossv[[1, 4]], rv[[1, 4]])
    bad = torch.tensor([-1, classes, 2 ** 40, -2 ** 40, classes + 1], device=DEV)
    loss, logits, pred, lossv = to.head_eval(y, W, b, bad, metrics=m)
    assert loss.item() == 0.0 and not lossv.any()
    r = m.result()
    assert (r["batches"], r["clips"], r["invalid"]) == (2, 2, 8)
    assert int(r["confusion"].sum()) == 2


def _accumulate(pkg, place, metrics_buf=None):
    """Three batches of 4, 4 and 3 clips (ties in the weights, one invalid label)
    into one metrics block; then a reset. place(t, name): tensor to the device."""
    to = pkg.train_ops
    classes, topk = 10, 3
    m = to.EvalMetrics(classes, topk, device=DEV, buf=metrics_buf)
    batches = []
    for i, n in enumerate((4, 4, 3)):
        U, stats2, g2, b2, W, b, lab = _head_inputs(n, 48, 54, classes, 20 + i, ties=(i == 1))
        if i == 2:
            lab[1] = classes
        args = [place(t, k) for t, k in zip((U, stats2, g2, b2, W, b, lab),
                                            ("U", "stats2", "g2", "b2", "W", "b", "labels"))]
        U, stats2, g2, b2, W, b, lab = args
        if i == 0:
            y = place(_y_of(U, stats2, g2, b2).contiguous(), "y")
            loss, logits, pred, lossv = to.head_eval(y, W, b, lab, metrics=m)
        else:
            loss, logits, pred, lossv = to.head_eval(None, W, b, lab, metrics=m,
                                                     from_u=(U, stats2, g2, b2))
        batches.append((logits, lossv, lab, pred))
    r = _check_rules(pkg, m, batches, topk)
    assert (r["batches"], r["clips"], r["invalid"]) == (3, 10, 1)
    assert r["val_loss"] != r["loss"]
    out = [t.clone() for bt in batches for t in bt]
    m.reset()
    assert not m.buf.cpu().any()
    return out


def test_head_eval_accumulates(pkg):
    _accumulate(pkg, lambda t, name: t.to(DEV))


def test_head_eval_poisoned(pkg):
    """The same under every fill: the metrics block (reset by the library, not
    assumed zero), pred and the outputs in poisoned, guard-banded memory, the
    inputs guarded and unchanged; bit-identical to the clean run."""
    clean = _accumulate(pkg, lambda t, name: t.to(DEV))
    nbytes = pkg.hip_lib.lib().stgcn_eval_metrics_bytes(10)
    for fill in poison.FILLS:
        with poison.poisoned(pkg, fill):
            buf = poison.empty(nbytes, fill, dtype=torch.uint8, device=DEV, name="metrics")
            got = _accumulate(pkg, lambda t, name: poison.guarded(t, fill, DEV, name=name), buf)
            torch.cuda.synchronize()
        poison.check_guards()
        poison.check_inputs()
        assert any(a.dtype == torch.int32 and a.site[0] == "train_ops.py"
                   for a in poison.allocations()), "pred was not placed in poisoned memory"
        for a, b in zip(got, clean):
            assert torch.equal(a, b), f"fill {fill:#04x}"


# --- the stack ---------------------------------------------------------------------

CONFIGS = {
    "v18-f16x2": (18, 1, dict(f32_gemm="f16x2")),
    "v18-bf16x3": (18, 1, dict(f32_gemm="bf16x3")),
    "v18-mfma": (18, 1, dict(f32_gemm="mfma")),
    "v18-f16x2-nog": (18, 1, dict(f32_gemm="f16x2-nog")),
    "v25k3-bf16": (25, 3, dict(gemm_dtype=torch.bfloat16)),
    "v50k3-bf16": (50, 3, dict(gemm_dtype=torch.bfloat16)),
    "v25k1-f16x2": (25, 1, dict(f32_gemm="f16x2")),
    "v18-residual": (18, 1, dict(residual=True)),
    "v18-dropout": (18, 1, dict(dropout_rate=0.5, f32_gemm="f16x2")),
}
ALL_LAZY = ("v18-f16x2", "v18-bf16x3", "v25k3-bf16", "v50k3-bf16", "v18-dropout")
_STACKS = {}


def _adjacency(pkg, V, K):
    gr = pkg.graph
    if K == 1:  # unilabeling
        return gr.get_normalized_adjacency_matrices(0, 1, graph=gr.graph_for(V))
    return gr.get_normalized_adjacency_matrices(2, 1, distances=gr.synthetic_distances(V),
                                                graph=gr.graph_for(V))


def _stack(pkg, name):
    """The config's stack on DEV in eval mode (shared by the tests: an eval step
    changes nothing in it), its running statistics and BN affines random, one
    g2 = 0 channel per block; with its CPU state_dict and adjacency."""
    if name not in _STACKS:
        V, K, kw = CONFIGS[name]
        # The reference's normalisation leaves entries of 2e4 .. 5e4 in A (its
        # alpha = 0.001), which BatchNorm's batch statistics absorb in training;
        # with the random running statistics set below nothing does, every block
        # gains 1e5 and fp32 (the fp32 oracle included) overflows at block 6.
        # Each joint's weights are scaled to sum to 1 so that all ten blocks
        # compute on values of order 1.
        A = _adjacency(pkg, V, K)
        assert A.shape[0] == K
        A = A / A.abs().sum(dim=(0, 2), keepdim=True)
        torch.manual_seed(sum(map(ord, name)))
        with contextlib.redirect_stdout(io.StringIO()):
            m = pkg.STGCNStack(3, 10, A, **kw)
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for blk in m.conv:
                for bn in (blk.batch_n, blk.batch_n_2):
                    bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=g))
                    bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=g) + 0.5)
                    bn.weight.copy_(torch.randn(bn.weight.shape, generator=g))
                    bn.bias.copy_(torch.randn(bn.bias.shape, generator=g))
                blk.batch_n_2.weight[1] = 0.0
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        _STACKS[name] = (m.to(DEV).eval(), state, A)
    return _STACKS[name]


def _inputs(N, T, V, seed=1):
    x = torch.randn(N, 3, T, V, generator=torch.Generator().manual_seed(seed)).to(DEV)
    lab = torch.randint(0, 10, (N,), generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
    return x, lab


def _plan_by_bits(pkg, m, x):
    """last_eval_plan as block_plan of each consumer's eval descriptor says."""
    blocks = list(m.conv)
    descs = pkg.fused.stack_descs(blocks, tuple(x.shape), training=False)
    out = []
    for i, blk in enumerate(blocks[:-1]):
        bit = pkg.hip_lib.block_plan(descs[i + 1]) & pkg.hip_lib.PLAN_X_FROM_U_EVAL
        out.append("lazy" if bit and not blk.residual else "written")
    return out + ["written" if blocks[-1].residual else "head"]


def _reference(m, x, lab, pkg):
    """The existing eval route: forward_nctv's logits, the training head on the
    blocks' written output (the tensor forward_nctv pools), and the bound on the
    distance between two fp32 heads on that tensor (``_head_bound``)."""
    with torch.no_grad():
        ref_logits = m.forward_nctv(x)
        y = m.conv(x)
        W, b = m.fc_layer.weight, m.fc_layer.bias
        hloss, hlogits = pkg.train_ops.StgcnHeadFn.apply(y, W, b, lab)
        bound = _head_bound(y, W, b)
    return ref_logits, hloss, hlogits, bound


def _head_bound(y, W, b):
    """Per logit, how far two correct fp32 evaluations of the head on the same y
    may lie apart. forward_nctv's head is torch's (mean over L = T V, then
    Linear: library reductions), the scoring head is stgcn_head_fwd's (a
    wave-strided sum, then an fma chain): the same sums in another order. Each
    is a sum of L terms followed by one of C + 1 terms, so each lies within
    gamma = (L + C + 2) u, u = 2^-24, of the exact value relative to
    sum_c |pooled_c W_jc| + |b_j| (the standard bound of a recursive fp32 sum);
    two of them within twice that."""
    L, C = y[0, 0].numel(), y.shape[1]
    pooled = y.double().flatten(2).mean(dim=2).abs()
    mag = pooled @ W.double().abs().t() + b.double().abs()
    return 2.0 * (L + C + 2) * 2.0 ** -24 * mag


def _cases():
    for name, (V, _, _) in CONFIGS.items():
        for N in (1, 3):
            for T in (8, 20, 21):
                if V == 50 and (N != 1 or T == 21):
                    continue
                yield pytest.param(name, N, T, id=f"{name}-N{N}-T{T}")


@pytest.mark.parametrize("name,N,T", list(_cases()))
def test_eval_step_matches_eval_forward(pkg, name, N, T):
    """eval_step against the existing eval route (every block alone, its y
    written). The blocks and the head are held bit for bit: logits and loss are
    torch.equal to StgcnHeadFn on ``conv(x)``, the tensor forward_nctv pools.
    forward_nctv's own logits cannot be held that way together with the head's
    bit-identity to stgcn_head_fwd: its head is torch's mean + Linear, and the
    two heads on one and the same y already differ on the parent commit (each
    2e-7 .. 4e-7 rel-to-max from an fp64 head on that y; measured over these
    cases 1.5e-7 .. 7.4e-7 apart, at most 0.0031 of the bound). They are held
    to ``_head_bound``, the distance two fp32 summation orders of that head can
    have."""
    m, state, _ = _stack(pkg, name)
    V = CONFIGS[name][0]
    x, lab = _inputs(N, T, V)
    ref_logits, hloss, hlogits, bound = _reference(m, x, lab, pkg)
    loss, logits = m.eval_step(x, lab)
    torch.cuda.synchronize()
    # bit for bit the training head on the output the existing route's blocks wrote
    assert torch.equal(logits, hlogits) and torch.equal(loss, hloss)
    # ... and forward_nctv's own logits up to the two heads' summation order
    diff = (logits.double() - ref_logits.double()).abs().detach()
    print("eval_step vs forward_nctv: worst diff / bound", float((diff / bound).max()),
          "rel-to-max", float(diff.max() / ref_logits.abs().max()))
    assert bool((diff <= bound).all()), float((diff / bound).max())
    plan = m.last_eval_plan
    assert len(plan) == 10 and plan == _plan_by_bits(pkg, m, x), plan
    if name in ALL_LAZY and T in (8, 20):
        assert plan == ["lazy"] * 9 + ["head"], plan
    if name == "v18-f16x2" and T == 21:
        assert "lazy" in plan[:9] and "written" in plan[:9], plan
    if name in ("v18-mfma", "v18-f16x2-nog"):
        assert plan == ["written"] * 9 + ["head"], plan
    if name == "v18-residual":
        assert plan == ["written"] * 10, plan
    # nothing in the module moved, nothing wants a gradient
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), state[k]), k
    assert all(p.grad is None for p in m.parameters())
    assert not loss.requires_grad and not logits.requires_grad


@pytest.mark.parametrize("name", ["v18-f16x2", "v25k3-bf16"])
def test_eval_step_oracle(pkg, name):
    """The logits at the stack gates of test_gpu_stack.py against the fp64
    oracle in eval mode on the module's own state_dict: fp32-type path
    rel-to-max <= max(1e-4, 3 e32), bf16 path <= max(2e-2, 4 e_bf16)."""
    m, state, _ = _stack(pkg, name)
    V = CONFIGS[name][0]
    x, lab = _inputs(3, 20, V)
    _, logits = m.eval_step(x, lab)
    xr = x.cpu().permute(0, 2, 3, 1).contiguous()

    def oracle(dtype, bf16):
        p = {k: v.to(dtype) for k, v in state.items() if "running" not in k
             and "num_batches" not in k}
        b = {k: (v.to(dtype) if v.is_floating_point() else v.clone())
             for k, v in state.items() if "running" in k or "num_batches" in k}
        with torch.no_grad():
            return ref_cpu.Stack(p, b).forward(xr, training=False, dtype=dtype, gemm_bf16=bf16)

    l64 = oracle(torch.float64, False).numpy()
    err = rel_to_max(logits.cpu().numpy(), l64)
    if name == "v25k3-bf16":
        floor = rel_to_max(oracle(torch.float32, True).numpy(), l64)
        print("bf16 logits err", err, "reference bf16 floor", floor)
        assert err <= max(2e-2, 4 * floor), (err, floor)
    else:
        floor = rel_to_max(oracle(torch.float32, False).numpy(), l64)
        print("fp32 logits err", err, "fp32 oracle floor", floor)
        assert err <= max(1e-4, 3 * floor), (err, floor)


def test_eval_step_refuses_training_mode(pkg):
    m, _, _ = _stack(pkg, "v18-f16x2")
    x, lab = _inputs(1, 8, 18)
    m.train()
    try:
        with pytest.raises(RuntimeError, match="training"):
            m.eval_step(x, lab)
        with pytest.raises(RuntimeError, match="training"):
            m.compute_conf_mat([])
    finally:
        m.eval()


def test_eval_step_forward_hook(pkg):
    """A forward hook on block 4 keeps its input and output written (links 3 -> 4
    and 4 -> 5), fires with the written output, and the logits do not move."""
    m, _, _ = _stack(pkg, "v18-f16x2")
    x, lab = _inputs(3, 20, 18)
    _, clean = m.eval_step(x, lab)
    clean = clean.clone()
    seen = {}
    with torch.no_grad():
        y4 = m.conv[:5](x)
    h = m.conv[4].register_forward_hook(lambda mod, i, o: seen.__setitem__("y4", o.clone()))
    try:
        _, logits = m.eval_step(x, lab)
        plan = list(m.last_eval_plan)
    finally:
        h.remove()
    assert plan == ["lazy"] * 3 + ["written"] * 2 + ["lazy"] * 4 + ["head"], plan
    assert torch.equal(logits, clean)
    assert torch.equal(seen["y4"], y4)
    m.eval_step(x, lab)
    assert m.last_eval_plan == ["lazy"] * 9 + ["head"]


@pytest.mark.parametrize("name", ["v18-f16x2", "v25k3-bf16"])
def test_eval_step_graph(pkg, name):
    """eval_step captured in a HIP graph: logits and loss of a replay equal the
    eager call's, and three replays fill the metrics block bit for bit as three
    eager calls do."""
    to = pkg.train_ops
    m, _, _ = _stack(pkg, name)
    x, lab = _inputs(3, 20, CONFIGS[name][0])
    eager = to.EvalMetrics(10, 3, device=DEV)
    for _ in range(3):
        loss0, logits0 = m.eval_step(x, lab, eager)
    loss0, logits0 = loss0.clone(), logits0.clone()
    want = eager.buf.cpu()
    metrics = to.EvalMetrics(10, 3, device=DEV)
    step = to.GraphedStep(lambda: m.eval_step(x, lab, metrics), warmup=2)
    metrics.reset()
    for _ in range(3):
        loss, logits = step()
    torch.cuda.synchronize()
    assert torch.equal(logits, logits0) and torch.equal(loss, loss0)
    assert torch.equal(metrics.buf.cpu(), want)
    assert metrics.result()["batches"] == 3 and metrics.result()["clips"] == 9


@pytest.mark.parametrize("name", ["v18-f16x2", "v25k3-bf16"])
def test_eval_step_poisoned(pkg, name):
    """Every buffer of the step (ping-pong U / y, Z, workspace, stats, fold-prep,
    head outputs) starts as the fill and is guard-banded, the input guarded: a
    read of an unwritten y, or a write past a shared buffer, would show."""
    m, _, _ = _stack(pkg, name)
    x, lab = _inputs(3, 20, CONFIGS[name][0])
    _, clean = m.eval_step(x, lab)
    clean = clean.clone()
    for fill in poison.FILLS:
        m._fold_prep_eval = None  # (its buffers anew, inside the poisoned region)
        with poison.poisoned(pkg, fill):
            xg = poison.guarded(x, fill, DEV, name="x")
            lg = poison.guarded(lab, fill, DEV, name="labels")
            loss, logits = m.eval_step(xg, lg)
            torch.cuda.synchronize()
        poison.check_guards()
        poison.check_inputs()
        sites = {a.site[2] for a in poison.allocations() if a.kind != "input"}
        assert "eval_forward" in sites and "head_eval" in sites, sites
        assert torch.isfinite(loss).all()
        assert torch.equal(logits, clean), f"fill {fill:#04x}"
    m._fold_prep_eval = None


def test_compute_conf_mat_and_accuracy(pkg):
    """compute_conf_mat over three (x NTVC, y) batches equals the reference's
    Python loop (lightning_model.py:123-133) on forward's arg-max;
    compute_accuracy is the reference's host float."""
    m, _, _ = _stack(pkg, "v18-f16x2")
    batches = []
    for i, n in enumerate((3, 3, 2)):
        x, lab = _inputs(n, 20, 18, seed=30 + i)
        batches.append((x.permute(0, 2, 3, 1).contiguous().cpu(), lab.cpu()))
    conf = m.compute_conf_mat(batches)
    want = torch.zeros(10, 10, dtype=torch.int64)
    acc = []
    with torch.no_grad():
        for x, y in batches:
            out = m(x.to(DEV))
            pred = torch.argmax(out, dim=1).cpu()
            for i, j in zip(y, pred):
                want[i, j] += 1
            acc.append(m.compute_accuracy(out, y.to(DEV)))
            assert acc[-1] == (pred == y).sum().item() / len(pred)
    assert conf.dtype == torch.int64 and torch.equal(conf, want)
    assert isinstance(acc[0], float)
