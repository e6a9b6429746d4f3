"""GPU: tensors that do not start on a 16-byte boundary.

Every buffer the other GPU modules hand to the library starts on a 256-byte
boundary (the caching allocator's blocks, tests/poison.py's ALIGN), yet torch
makes contiguous tensors that do not: ``x[1:]`` of a batch with an odd T * V,
a view into a flat gradient bucket after the 1875-float NTU adjacency (12 mod
16). The contract (include/stgcn_hip.h, Conventions; DESIGN.md "Pointer
alignment"): the block, fold-prep and bf16 SpatialConv calls take 16-byte
aligned pointers (the running statistics, updated in place, 4-byte) and refuse
anything else by name before a launch -- ``fused._f32c`` hands them an aligned
copy of such an input; the fp32 SpatialConv on its own reads its inputs in
place and routes a misaligned x / output gradient to its narrower kernels; the
head and Adam kernels access single elements and take any naturally aligned
pointer.

Here the value tests' own runners place their inputs through the ``to_dev``
hook (as test_gpu_poison.py does) into guarded, 0xFF-filled memory at a skew of
4 / 8 / 12 bytes, under four placements: x alone, the output gradient alone,
every parameter and running statistic (rotating 4 / 8 / 12 by name), and all
of them. Per placement: the value test's gate, unchanged; every returned float
finite; no guard byte changed; no read-only input changed; and -- where the
library read an aligned copy -- every result bit-identical to the aligned run
of the same case (the adjacency gradient, summed by fp32 atomics in some paths, to
the run-to-run bound of test_gpu_f16x2.test_fold_prep_matches_own_operands).
The hook asserts each tensor it returns has ``data_ptr() % 16 == skew``.

Shapes: the smallest that meet the shape halves of the pointer-gated fast
paths (N C T V % 4 == 0, C_in T % 256 == 0, T V % 4 == 0), so that alignment
alone decides; no new tolerance.
"""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

import poison
from conftest import load_npz, rel_to_max
from oracle import ref_cpu
from test_gpu_bf16 import _bf16_reference, _gate_bf16
from test_gpu_bf16 import _run as _run_bf16
from test_gpu_block import DEV, TOL, _compare, _gate_dropout, _oracle, _random_case, _run_hip, \
    _run_hip_dropout
from test_gpu_callers import _check_eval_backward, _spatial_oracle, _spatial_run
from test_gpu_partitions import adjacency
from test_gpu_poison import _all_finite, _Memo
from test_gpu_stack import _bf16_stack_oracle, _bf16_stack_setup, _bf16_stack_vs_oracle

pytestmark = pytest.mark.gpu

FILL = 0xFF   # NaN as any float: a wide read that strays into a guard band shows
PLACEMENTS = ("x", "g", "params", "all")


class Skewed:
    """The runners' ``to_dev`` hook: inputs into guarded memory, ``skew`` bytes
    past a 256-byte boundary according to the placement. Names as the runners
    give them: "x", "g" (the output gradient), "labels", else a parameter or a
    running statistic, which rotate 4 / 8 / 12 in order of first appearance
    (int64 tensors: 8). ``seen`` records what was placed."""

    def __init__(self, placement):
        assert placement in PLACEMENTS + ("none",)
        self.placement, self.order, self.seen = placement, {}, []

    def skew_of(self, t, name):
        pl = self.placement
        if name in ("x", "g"):
            return 4 if pl in (name, "all") else 0
        if name == "labels":
            return 8 if pl in ("x", "all") else 0
        if pl not in ("params", "all"):
            return 0
        if t.element_size() == 8:
            return 8
        return (4, 8, 12)[self.order.setdefault(name, len(self.order)) % 3]

    def __call__(self, t, name):
        skew = self.skew_of(t, name)
        inout = "running_" in name or "num_batches" in name
        out = poison.guarded(t, FILL, DEV, name=name, readonly=not inout, skew=skew)
        assert out.data_ptr() % 16 == skew and out.is_contiguous(), (name, skew)
        self.seen.append((name, skew))
        return out

    def empty(self, size, device, dtype):
        return poison.empty(size, FILL, dtype=dtype, device=device, name="prep")

    def assert_skewed(self, *names):
        """The placement really reached the library: each named input (or, for
        "params", every parameter / statistic) was placed off a boundary."""
        got = dict(self.seen)
        for n in names:
            assert got.get(n, 0) != 0, (n, self.seen)
        if self.placement in ("params", "all"):
            par = [(n, s) for n, s in self.seen if n not in ("x", "g", "labels")]
            assert par and all(s != 0 for _, s in par), self.seen
            assert {s for _, s in par if s != 8} <= {4, 12} and len({s for _, s in par}) > 1


def _same(got, base, what):
    """Bit-identical to the aligned run; the adjacency gradient within the
    fp32 atomic-order bound (test_fold_prep_matches_own_operands)."""
    assert set(got) == set(base), (what, sorted(set(got) ^ set(base)))
    for k, b in base.items():
        g = got[k]
        if b is None or g is None:
            assert b is None and g is None, (what, k)
        elif k == "grad.spatialConv.A" or k == "grad.A":
            torch.testing.assert_close(g, b, rtol=1e-5, atol=1e-6 * float(b.abs().max()),
                                       msg=lambda m: f"{what}: {k}: {m}")
        else:
            assert torch.equal(g, b), f"{what}: {k} differs from the aligned run"


def _placed(pkg, run, gate, needs=("x", "g"), same=_same):
    """run(hook) -> result dict under the aligned placement, then the four
    skewed ones: guards, inputs, finiteness, ``gate`` and equality with the
    aligned run, each."""
    base = None
    for pl in ("none",) + PLACEMENTS:
        hook = Skewed(pl)
        try:
            with poison.poisoned(pkg, FILL):
                got = run(hook)
                torch.cuda.synchronize()
            poison.check_guards()
            poison.check_inputs()
            hook.assert_skewed(*[n for n in needs if pl in (n, "all")])
            _all_finite(got)
            if gate is not None:
                gate(got)
            if base is None:
                base = got
            elif same is not None:
                same(got, base, pl)
        except AssertionError as e:
            raise AssertionError(f"placement {pl!r}: {e}") from e
    return base


# --- blocks: (C_in, C_out, stride, V, K, N, T) ---------------------------------

def _check_block(pkg, case, gemm, residual=False, need_dx=True, prep=False):
    arrays, x, g = _random_case(pkg, *case, residual=residual)
    oracle = _Memo(lambda got: _oracle(arrays, got), lambda got: (got["y"] > 0,))

    def gate(got):
        want, floor = oracle(got)
        want = {k: v for k, v in want.items() if need_dx or k != "grad.x"}
        _compare(got, want, residual=residual, floor=floor)

    _placed(pkg, lambda hook: _run_hip(pkg, arrays, x, g, need_dx=need_dx, gemm=gemm, prep=prep,
                                       to_dev=hook),
            gate)


SPLIT = [(c, m, p) for c in [(64, 64, 1, 18, 1, 2, 16), (64, 128, 2, 18, 1, 2, 16)]
         for m, preps in (("fp32", (False,)), ("f32x3", (False, True)), ("f16x2", (False, True)),
                          ("f16x2_nog", (False, True))) for p in preps]


@pytest.mark.parametrize("case,gemm,prep", SPLIT,
                         ids=["-".join(map(str, c)) + f"-{m}" + ("-prep" if p else "")
                              for c, m, p in SPLIT])
def test_misaligned_v18_block(pkg, case, gemm, prep):
    """(fp32 does not fold: no stgcn_fold_prep buffer to take)"""
    _check_block(pkg, case, gemm, prep=prep)


@pytest.mark.parametrize("need_dx", [True, False])
@pytest.mark.parametrize("gemm", ["fp32", "f16x2"])
def test_misaligned_first_block(pkg, gemm, need_dx):
    """C_in = 3 with C_in * T = 768: the k_gather4 shape condition holds."""
    _check_block(pkg, (3, 64, 1, 18, 1, 2, 256), gemm, need_dx=need_dx)


def test_misaligned_folded_v25(pkg):
    _check_block(pkg, (64, 64, 1, 25, 1, 2, 16), "f16x2")


@pytest.mark.parametrize("case", [(64, 64, 1, 25, 2, 2, 16), (64, 64, 1, 25, 3, 2, 16),
                                  (64, 64, 1, 50, 3, 2, 8)], ids=lambda c: "-".join(map(str, c)))
def test_misaligned_partitioned_fp32(pkg, case):
    """K > 1: the MFMA gather and k_spatial_bwd5 (V = 25) / _bwd6 (V = 50)."""
    C_in, C_out, stride, V, K, N, T = case
    A = None
    if K == 2:   # (the reference's distance partitioning at depth 1, as test_gpu_partitions)
        A = adjacency(pkg, V, "s1_d1")
        assert tuple(A.shape) == (2, V, V)
    arrays, x, g = _random_case(pkg, *case, A=A)
    oracle = _Memo(lambda got: _oracle(arrays, got), lambda got: (got["y"] > 0,))

    def gate(got):
        want, floor = oracle(got)
        _compare(got, want, floor=floor)

    _placed(pkg, lambda hook: _run_hip(pkg, arrays, x, g, to_dev=hook), gate)


def _check_bf16(pkg, case, residual=False):
    arrays, x, g = _random_case(pkg, *case, residual=residual)
    oracle = _Memo(lambda got: _bf16_reference(arrays, got, True),
                   lambda got: (got["y"] > 0, got["inner_mask"]))
    f32 = _run_bf16(pkg, arrays, x, g, bf16=False)   # (aligned, once: the band check's other side)

    def gate(got):
        want, ref16 = oracle(got)
        _gate_bf16(got, want, ref16, f32, residual)

    _placed(pkg, lambda hook: _run_bf16(pkg, arrays, x, g, bf16=True, to_dev=hook), gate)


@pytest.mark.parametrize("case", [(64, 64, 1, 25, 3, 2, 16), (64, 128, 2, 25, 3, 2, 16),
                                  (64, 64, 1, 50, 3, 2, 8), (256, 256, 1, 50, 3, 2, 8)],
                         ids=lambda c: "-".join(map(str, c)))
def test_misaligned_bf16_block(pkg, case):
    """The fused SpatialConv forward / backward (fixed Z / kept-G layouts, 16-byte
    DMA from the tensor base): served by the wrapper's aligned copy."""
    _check_bf16(pkg, case)


@pytest.mark.parametrize("case,gemm", [((64, 64, 1, 18, 1, 2, 16), "fp32"),
                                       ((64, 128, 2, 25, 3, 2, 16), "bf16"),
                                       ((64, 64, 1, 50, 3, 2, 8), "bf16")],
                         ids=["identity-fp32", "projection-bf16", "identity-bf16-v50"])
def test_misaligned_residual_block(pkg, case, gemm):
    if gemm == "bf16":
        _check_bf16(pkg, case, residual=True)
    else:
        _check_block(pkg, case, gemm, residual=True)


@pytest.mark.parametrize("residual", [False, True])
def test_misaligned_dropout_block(pkg, residual):
    """Gated as test_gpu_block.test_block_dropout_matches_oracle (p = 0.5)."""
    case, drop = (64, 64, 1, 18, 1, 2, 16), 0.5
    arrays, x, g = _random_case(pkg, *case, seed=5, residual=residual)
    seeds = []

    def run(hook):
        got, seed = _run_hip_dropout(pkg, arrays, x, g, drop, to_dev=hook)
        seeds.append(seed)
        return got

    _placed(pkg, run, lambda got: _gate_dropout(arrays, got, seeds[-1], drop, residual))
    assert len(set(seeds)) == 1


@pytest.mark.parametrize("case,residual", [((64, 64, 1, 18, 1, 2, 16), False),
                                           ((64, 128, 2, 18, 1, 2, 16), True)])
def test_misaligned_eval_mode_backward(pkg, case, residual):
    """test_gpu_callers._check_eval_backward (its gate included) per placement;
    the running statistics are read in place at 4 / 8 / 12 and stay untouched."""
    _placed(pkg, lambda hook: _check_eval_backward(pkg, case, residual, "fp32", to_dev=hook) or {},
            None, same=None)


# --- SpatialConv on its own ------------------------------------------------------

@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("fixture", ["spatialconv_s64x64_v18k2.npz", "spatialconv_s64x64_v25k3.npz",
                                     "spatialconv_s64x128_v50k3.npz"])
def test_misaligned_spatialconv(pkg, fixture, bf16):
    """Gated as test_gpu_callers.test_spatialconv_standalone_matches_reference
    (fp32) and test_spatialconv_standalone_bf16. fp32: the library reads the
    skewed tensors in place -- a misaligned x takes k_gather3 in place of the
    MFMA gather / k_gather4 and k_spatial_bwd3 in place of k_spatial_bwd5 / 6, a
    misaligned output gradient k_sum_nt, the 4-byte staging of k_wgrad_sp and
    of the H GEMM -- so only the gate applies; bf16: aligned copies, bit for bit."""
    ref = load_npz(fixture)
    want = _spatial_oracle(ref, torch.float64)
    near = _spatial_oracle(ref, torch.float32, gemm_bf16=bf16)

    def gate(got):
        for k, w in want.items():
            err = rel_to_max(got[k].double().numpy(), w.double().numpy())
            floor = rel_to_max(near[k].double().numpy(), w.double().numpy())
            if bf16:
                assert err < max(2e-2, 3 * floor), (k, err, floor)
            else:
                assert err < max(TOL, 2 * floor), (k, err, floor)
                assert rel_to_max(got[k].double().numpy(), ref[k]) < 5e-5, k

    _placed(pkg, lambda hook: _spatial_run(pkg, ref, bf16=bf16, to_dev=hook), gate,
            same=_same if bf16 else None)


# --- head ------------------------------------------------------------------------

HEAD_SHAPES = [(4, 64, 4, 18, 10), (3, 64, 5, 25, 7)]   # L = 72, 125


def _head_inputs(N, C, T, V, classes):
    g = torch.Generator().manual_seed(N * 31 + classes)
    y = torch.relu(torch.randn(N, C, T, V, generator=g))
    W = torch.randn(classes, C, generator=g) * 0.1
    b = torch.randn(classes, generator=g) * 0.1
    lab = torch.randint(0, classes, (N,), generator=g)
    return y, W, b, lab


def _head_place(skewed):
    def place(t, name):
        skew = 0 if not skewed else (8 if t.dtype == torch.int64 else 4)
        out = poison.guarded(t, FILL, DEV, name=name, skew=skew)
        assert out.data_ptr() % 16 == skew
        return out
    return place


@pytest.mark.parametrize("N,C,T,V,classes", HEAD_SHAPES)
def test_misaligned_head_matches_torch(pkg, N, C, T, V, classes):
    """StgcnHeadFn with y, W, bias at skew 4 and the labels at skew 8, read in
    place (scalar kernels), against the fp64 torch head at
    test_gpu_train_ops.test_head_matches_torch's 1e-5, and bit for bit against
    the aligned run."""
    y, W, b, lab = _head_inputs(N, C, T, V, classes)
    y64, W64, b64 = (t.double().requires_grad_(True) for t in (y, W, b))
    logits64 = F.linear(F.avg_pool2d(y64, (T, V)).view(N, C), W64, b64)
    loss64 = F.cross_entropy(logits64, lab)
    loss64.backward()
    runs = []
    for skewed in (False, True):
        place = _head_place(skewed)
        with poison.poisoned(pkg, FILL):
            yd, Wd, bd = (place(t, n).requires_grad_(True) for t, n in ((y, "y"), (W, "W"),
                                                                         (b, "bias")))
            loss, logits = pkg.train_ops.StgcnHeadFn.apply(yd, Wd, bd, place(lab, "labels"))
            loss.backward()
            torch.cuda.synchronize()
        poison.check_guards()
        poison.check_inputs()
        got = {"loss": loss.detach().cpu(), "logits": logits.detach().cpu(), "dy": yd.grad.cpu(),
               "dW": Wd.grad.cpu(), "db": bd.grad.cpu()}
        _all_finite(got)
        assert abs(got["loss"].item() - loss64.item()) <= 1e-5 * abs(loss64.item())
        assert rel_to_max(got["logits"].numpy(), logits64.detach().numpy()) < 1e-5
        for k, want in (("dy", y64.grad), ("dW", W64.grad), ("db", b64.grad)):
            assert rel_to_max(got[k].numpy(), want.numpy()) < 1e-5, k
        runs.append(got)
    for k, v in runs[0].items():
        assert torch.equal(v, runs[1][k]), k


@pytest.mark.parametrize("N,C,T,V,classes", HEAD_SHAPES)
def test_misaligned_head_u_and_eval_forms(pkg, N, C, T, V, classes):
    """The from-U training head and stgcn_head_eval / _u with the same
    placements (U, stats2, g2, b2 at skew 4 too): bit-identical to their aligned
    runs, metrics block included."""
    y, W, b, lab = _head_inputs(N, C, T, V, classes)
    g = torch.Generator().manual_seed(7)
    U = torch.randn(N, C, T, V, generator=g)
    stats2 = torch.cat([0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)])
    g2, b2 = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    runs = []
    for skewed in (False, True):
        place = _head_place(skewed)
        with poison.poisoned(pkg, FILL):
            Wd, bd, labd = place(W, "W"), place(b, "bias"), place(lab, "labels")
            from_u = tuple(place(t, n) for t, n in ((U, "U"), (stats2, "stats2"), (g2, "g2"),
                                                    (b2, "b2")))
            ph = torch.empty(1, device=DEV).expand(N, C, T, V)
            loss_u, logits_u = pkg.train_ops.StgcnHeadFn.apply(ph, Wd, bd, labd, from_u)
            got = {"u.loss": loss_u, "u.logits": logits_u}
            for form, kw in (("eval", dict(y=place(y, "y"))), ("eval_u", dict(y=None,
                                                                              from_u=from_u))):
                m = pkg.train_ops.EvalMetrics(classes, topk=2, device=DEV)
                loss, logits, pred, lossv = pkg.train_ops.head_eval(kw.pop("y"), Wd, bd, labd,
                                                                    metrics=m, **kw)
                got.update({f"{form}.loss": loss, f"{form}.logits": logits, f"{form}.pred": pred,
                            f"{form}.lossv": lossv, f"{form}.metrics": m.buf})
            torch.cuda.synchronize()
            got = {k: v.detach().cpu() for k, v in got.items()}
        poison.check_guards()
        poison.check_inputs()
        _all_finite(got)
        runs.append(got)
    for k, v in runs[0].items():
        assert torch.equal(v, runs[1][k]), k
    # (and the eval head equals the training head on valid labels: stgcn_hip.h)
    assert torch.equal(runs[1]["eval_u.logits"], runs[1]["u.logits"])
    assert torch.equal(runs[1]["eval_u.loss"], runs[1]["u.loss"])


# --- Adam --------------------------------------------------------------------------

ADAM_SHAPES = [(3, 25, 25), (64, 64, 9, 1), (64,), (5000,)]   # 1875 floats first


def _bucket_views(flat):
    """Views of ``flat`` laid out back to back as dp.GradAllReduce lays a bucket out."""
    out, off = [], 0
    for s in ADAM_SHAPES:
        n = 1
        for d in s:
            n *= d
        out.append(flat[off:off + n].view(s))
        off += n
    assert off == flat.numel()
    return out


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_misaligned_adam_matches_torch_adam(pkg, wd, capturable):
    """Parameters, gradients and both moments as views into flat buffers: after
    the 1875-float adjacency every view starts at 12 mod 16. Five steps, both
    step forms, against torch.optim.Adam at test_gpu_train_ops's tolerances."""
    g = torch.Generator().manual_seed(3)
    total = sum(torch.Size(s).numel() for s in ADAM_SHAPES)
    p0 = torch.randn(total, generator=g)
    grads = [torch.randn(total, generator=g) for _ in range(5)]
    ref = [v.clone().requires_grad_(True) for v in _bucket_views(p0)]
    opt_ref = torch.optim.Adam(ref, lr=1e-2, weight_decay=wd, foreach=False)
    with poison.poisoned(pkg, FILL):
        flats = {n: poison.guarded(t, FILL, DEV, name=n, readonly=False)
                 for n, t in (("param", p0), ("grad", grads[0]), ("exp_avg", torch.zeros(total)),
                              ("exp_avg_sq", torch.zeros(total)))}
        views = {n: _bucket_views(f) for n, f in flats.items()}
        for n, vs in views.items():
            assert [v.data_ptr() % 16 for v in vs] == [0, 12, 12, 12], n
            assert all(v.is_contiguous() for v in vs)
        dut = [v.requires_grad_(True) for v in views["param"]]
        opt = pkg.FusedAdam(dut, lr=1e-2, weight_decay=wd, capturable=capturable)
        for i, p in enumerate(dut):
            p.grad = views["grad"][i]
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": views["exp_avg"][i],
                            "exp_avg_sq": views["exp_avg_sq"][i]}
        for k in range(5):
            flats["grad"].copy_(grads[k])      # (the views stay: the table is built once)
            for p, gv in zip(ref, _bucket_views(grads[k])):
                p.grad = gv.clone()
            opt_ref.step()
            opt.step()
        torch.cuda.synchronize()
        for i, p in enumerate(dut):   # the step ran on the views, in place
            assert opt.state[p]["exp_avg"].data_ptr() == views["exp_avg"][i].data_ptr()
            assert p.data_ptr() == views["param"][i].data_ptr()
    poison.check_guards()
    for a, b in zip(dut, ref):
        d = (a.detach().cpu() - b.detach()).abs()
        assert torch.isfinite(a).all()
        assert (d <= 2e-6 * b.detach().abs() + 1e-7).all(), float(d.max())
        for key in ("exp_avg", "exp_avg_sq"):
            err = rel_to_max(opt.state[a][key].cpu().numpy(), opt_ref.state[b][key].numpy())
            assert err < 1e-6, (key, err)
        assert float(opt.state[a]["step"]) == opt_ref.state[b]["step"].item() == 5


# --- stacks ------------------------------------------------------------------------

@pytest.fixture
def three_blocks(pkg, monkeypatch):
    """The stack and its oracle cut to three of their blocks: the first (3 -> 64),
    the first strided one (64 -> 128) and the one that reaches the head's 256
    channels (128 -> 256, stride 2)."""
    layers = [pkg.model.LAYERS[i] for i in (0, 4, 7)]
    assert layers == [(64, 1), (128, 2), (256, 2)] == [ref_cpu.LAYERS[i] for i in (0, 4, 7)]
    monkeypatch.setattr(pkg.model, "LAYERS", layers)
    monkeypatch.setattr(ref_cpu, "LAYERS", layers)


def _stack_step(pkg, model, x, lab, skewed, after_backward=None, bucket=False):
    """forward_loss + backward + one FusedAdam step with x at skew 4 and the
    labels at skew 8 (``skewed``); bucket: the gradients accumulate into
    dp.GradAllReduce's flat bucket views (world size 1, no collective)."""
    res = {}
    with poison.poisoned(pkg, FILL):
        model = model.to(DEV).train()
        opt = pkg.FusedAdam(model.parameters(), lr=1e-3)
        xd = poison.guarded(x, FILL, DEV, name="x", skew=4 if skewed else 0)
        labd = poison.guarded(lab, FILL, DEV, name="labels", skew=8 if skewed else 0)
        assert xd.data_ptr() % 16 == (4 if skewed else 0)
        assert labd.data_ptr() % 16 == (8 if skewed else 0)
        sync = contextlib.nullcontext()
        if bucket:
            dp = pkg.dp.GradAllReduce(model, world_size=1)
            dp.zero_grad()
            sync = dp.no_sync()
        with sync:
            loss, logits = model.forward_loss(xd, labd)
            loss.backward()
        torch.cuda.synchronize()
        poison.check_inputs()
        if bucket:   # every gradient is a view into a flat bucket; most start off a boundary
            ptrs = [p.grad.data_ptr() % 16 for p in model.parameters()]
            assert all(p.grad._is_view() for p in model.parameters())
            assert sum(1 for q in ptrs if q) > len(ptrs) // 2, ptrs
        if after_backward is not None:
            after_backward(model, loss, logits)
        res["loss"], res["logits"] = loss.detach().cpu(), logits.detach().cpu()
        for k, v in model.named_parameters():
            res["grad." + k] = v.grad.cpu().clone()
        opt.step()
        torch.cuda.synchronize()
        for k, v in list(model.named_parameters()) + list(model.named_buffers()):
            res["end." + k] = v.detach().cpu()
    poison.check_guards()
    _all_finite(res)
    return res


def _v18_stack(pkg, classes=60):
    gr = pkg.graph
    A = gr.get_normalized_adjacency_matrices(0, 1, graph=gr.graph_for(18))
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        return pkg.STGCNStack(3, classes, A, f32_gemm="f16x2")


def test_misaligned_stack_f16x2_bitwise(pkg, three_blocks):
    """A 3-block V = 18 f16x2 stack (lazy links, x from U, deferred dx, the head
    from U): bit-reproducible (test_gpu_poison.test_poisoned_stack_fp32_split_
    bitwise), so the skewed step equals the aligned one in every tensor."""
    x = torch.randn(2, 3, 16, 18, generator=torch.Generator().manual_seed(4))
    lab = torch.randint(0, 60, (2,), generator=torch.Generator().manual_seed(14))
    runs = [_stack_step(pkg, _v18_stack(pkg), x, lab, skewed) for skewed in (False, True)]
    assert len(list(_v18_stack(pkg).conv)) == 3 and "end.fc_layer.weight" in runs[0]
    diff = [k for k, v in runs[0].items() if not torch.equal(v, runs[1][k])]
    assert not diff, f"not bit-identical to the aligned run: {diff}"


def test_misaligned_stack_bf16(pkg, three_blocks):
    """A 3-block V = 25, K = 3 bf16 stack at the single-seed bound of
    test_gpu_stack.test_stack_bf16_multi_seed / test_poisoned_stack_bf16:
    max(2e-2, 4x the bf16-operand reference's error) per tensor."""
    seed, N, T, V = 0, 2, 16, 25
    A, model0, x, lab, params0 = _bf16_stack_setup(pkg, V, seed, N, T)
    assert len(list(model0.conv)) == 3
    oracles = _bf16_stack_oracle(A, params0, x, lab, seed)
    state0 = {k: v.clone() for k, v in model0.state_dict().items()}

    def gate(model, loss, logits):
        errs, floor = _bf16_stack_vs_oracle(model, loss, logits, oracles)
        bad = [f"{k}: {e:.2e} (ref bf16 {floor[k]:.2e})" for k, e in errs.items()
               if not e <= max(2e-2, 4 * floor[k])]
        assert not bad, "; ".join(bad)

    for skewed in (False, True):
        _, model, _, _, _ = _bf16_stack_setup(pkg, V, seed, N, T)
        model.load_state_dict(state0)
        _stack_step(pkg, model, x.permute(0, 3, 1, 2).contiguous(), lab, skewed,
                    after_backward=gate)


def test_bucket_view_gradients_bitwise(pkg, three_blocks):
    """The data-parallel layout at world size 1: every gradient a view into
    GradAllReduce's flat bucket (FusedAdam reads them in place) against plain
    .grad tensors: loss, logits, gradients, parameters and buffers after the
    step, bit for bit."""
    x = torch.randn(2, 3, 16, 18, generator=torch.Generator().manual_seed(4))
    lab = torch.randint(0, 61, (2,), generator=torch.Generator().manual_seed(14))
    # (61 classes: the head's bias, the first view of the bucket, is an odd number
    # of floats, so every view behind it starts at 4 mod 16 -- what the 1875-float
    # NTU adjacency does to a V = 25 stack, on the stack that is bit-reproducible)
    plain = _stack_step(pkg, _v18_stack(pkg, 61), x, lab, skewed=False)
    views = _stack_step(pkg, _v18_stack(pkg, 61), x, lab, skewed=False, bucket=True)
    diff = [k for k, v in plain.items() if not torch.equal(v, views[k])]
    assert not diff, f"bucket-view gradients: not bit-identical: {diff}"
