"""GPU: buffer discipline of the HIP library under adversarial memory contents.

The value tests run on memory that is driver-zeroed or holds the leftovers of
an identical earlier call, with other tensors packed right behind every buffer.
Here every buffer the package allocates (tests/poison.py: outputs, saved Z / U /
stats, kept G, y_stats, dx_coef, prev_sums, every gradient, both workspaces) and
every test input sits in the middle of a guarded backing filled with one byte,
and each case runs under three fills: 0x00 (clean), 0xFF (NaN as any float,
0xFFFFFFFF for a "largest word wins" maximum, -1 as an integer) and 0x4B (finite:
fp32 1.33e7, fp64 1e55 -- not swallowed by fmax / ReLU / comparisons). Per fill:

* the run passes the project's existing gate for that path, unchanged (the
  runners and gates are the value tests' own, with the inputs placed through
  their ``to_dev`` hook): a read before write of a partial slot, accumulator or
  workspace word, or a masked read past an end (0 * NaN), shows there;
* every floating-point tensor the run returns is finite (the fp32 gate's
  ``err > lim`` is False for a NaN, so it alone would let one through);
* no guard byte changed (a partial tile written past y, dx, a gradient or a
  workspace), before or after any buffer;
* every read-only input (x, parameters, g, labels) is bit-identical to what
  went in (the running statistics are in/out and exempt);
* the allocation record holds a buffer of exactly stgcn_fwd_workspace_bytes
  asked for by the Function's forward and one of exactly
  stgcn_bwd_workspace_bytes asked for by its backward (the record keeps each
  buffer's call site): the poison reached the workspaces.

Which comparison applies: block, dropout, eval-mode and SpatialConv cases the
oracle gate of their value test (fp32 atomics remain in some adjacency-gradient
paths, test_gpu_f16x2.test_fold_prep_matches_own_operands); the fp32-split V = 18
training stacks bitwise against the clean run (loss, logits, every gradient,
buffer and parameter after FusedAdam, two steps: the paths
test_gpu_stack.test_stack_lazy_links_bit_identical holds bit-reproducible); the
bf16 stacks the single-seed oracle bound of test_stack_bf16_multi_seed.
"""
import contextlib
import ctypes
import io
import os
import re

import pytest
import torch

import poison
from conftest import ROOT, load_npz, rel_to_max
from test_gpu_bf16 import _bf16_reference, _gate_bf16
from test_gpu_bf16 import _run as _run_bf16
from test_gpu_block import DEV, TOL, _compare, _gate_dropout, _oracle, _random_case, _run_hip, \
    _run_hip_dropout
from test_gpu_callers import _check_eval_backward, _spatial_fixtures, _spatial_oracle, \
    _spatial_run
from test_gpu_stack import _bf16_stack_oracle, _bf16_stack_setup, _bf16_stack_vs_oracle

pytestmark = pytest.mark.gpu


class Place:
    """The runners' ``to_dev`` hook: inputs into guarded memory (read-only but
    for the running statistics), the fold-prep buffer poisoned like the rest."""

    def __init__(self, fill):
        self.fill = fill

    def __call__(self, t, name):
        inout = "running_" in name or "num_batches" in name
        return poison.guarded(t, self.fill, DEV, name=name, readonly=not inout)

    def empty(self, size, device, dtype):
        return poison.empty(size, self.fill, dtype=dtype, device=device, name="prep")


@contextlib.contextmanager
def _fill_named(fill):
    try:
        yield
    except AssertionError as e:
        raise AssertionError(f"fill {fill:#04x}: {e}") from e


def _has_buffer(nbytes, func, what):
    """The record holds a uint8 buffer of exactly ``nbytes`` that fused.py's
    ``func`` (forward / backward of the autograd Functions: the only uint8
    buffers those allocate themselves are the workspaces) asked for."""
    sizes = [a.nbytes for a in poison.allocations()
             if a.kind != "input" and a.dtype == torch.uint8
             and a.site[0] == "fused.py" and a.site[2] == func]
    assert nbytes in sizes, (f"no poisoned {what} of {nbytes} bytes allocated by fused.py "
                             f"{func} (its uint8 buffers: {sizes})")


def _all_finite(res):
    """Every floating-point tensor anywhere in a result (dicts / tuples of
    tensors) is finite: the value gates' ``err > lim`` is False for a NaN."""
    bad = []

    def walk(o, path):
        if torch.is_tensor(o):
            if o.is_floating_point() and not torch.isfinite(o).all():
                bad.append(f"{path} ({int((~torch.isfinite(o)).sum())} of {o.numel()})")
        elif isinstance(o, dict):
            for k, v in o.items():
                walk(v, f"{path}.{k}" if path else str(k))
        elif isinstance(o, (tuple, list)):
            for i, v in enumerate(o):
                walk(v, f"{path}[{i}]")

    walk(res, "")
    assert not bad, f"not finite: {bad}"


def _under_fills(pkg, run, gate, desc=None, bwd_desc=None, workspaces=None):
    """run(place) -> result, under each fill; gate(result) is the value test's
    own gate. workspaces: (fwd bytes, bwd bytes) where no block descriptor
    gives them. Returns {fill: result}."""
    lib = pkg.hip_lib.lib()
    if desc is not None:
        workspaces = (lib.stgcn_fwd_workspace_bytes(ctypes.byref(desc)),
                      lib.stgcn_bwd_workspace_bytes(ctypes.byref(bwd_desc or desc)))
    out = {}
    for fill in poison.FILLS:
        with _fill_named(fill):
            with poison.poisoned(pkg, fill):
                got = run(Place(fill))
                torch.cuda.synchronize()
            poison.check_guards()
            poison.check_inputs()
            _has_buffer(workspaces[0], "forward", "forward workspace")
            _has_buffer(workspaces[1], "backward", "backward workspace")
            if got is not None:
                _all_finite(got)
                gate(got)
            out[fill] = got
    return out


def _desc(pkg, case, gemm, residual=False, need_dx=True, training=True):
    C_in, C_out, stride, V, K, N, T = case
    return pkg.fused.make_desc((N, C_in, T, V), C_out, K, stride, 4, 1e-5, 0.1, training,
                               need_dx=need_dx, residual=residual,
                               **pkg.fused._gemm_flags(gemm))


class _Memo:
    """The oracle of a case, computed once and shared by the fills: it depends
    on the run only through the run's ReLU masks."""

    def __init__(self, fn, masks):
        self.fn, self.masks, self.key, self.val = fn, masks, None, None

    def __call__(self, got):
        key = self.masks(got)
        if self.key is None or not all(
                (a is None and b is None) or torch.equal(a, b) for a, b in zip(key, self.key)):
            self.key, self.val = key, self.fn(got)
        return self.val


# --- block cases: (C_in, C_out, stride, V, K, N, T), the smallest shapes at which
# each kernel still has its partial tiles --------------------------------------

FP32_CASES = [
    # case, residual, need_dx
    ((64, 64, 1, 18, 1, 2, 21), False, True),
    ((64, 128, 2, 18, 1, 2, 37), False, True),     # stride 2, odd T
    ((5, 7, 1, 18, 1, 2, 9), False, True),         # odd channel counts
    ((64, 64, 2, 18, 1, 1, 1), False, True),       # T = 1
    ((64, 64, 1, 25, 3, 2, 19), False, True),
    ((3, 64, 1, 50, 3, 2, 11), False, True),       # V = 50 ragged frame tiles
    ((64, 128, 2, 18, 1, 2, 37), True, True),
    ((64, 64, 1, 25, 3, 2, 17), True, True),
    ((5, 7, 2, 18, 1, 2, 9), True, True),
    ((3, 64, 1, 18, 1, 2, 30), False, False),
]
SPLIT_MODES = ["f32x3", "f16x2", "f16x2_nog"]
SPLIT_CASES = [
    # case, need_dx, prep (the stgcn_fold_prep buffer)
    (case, True, prep)
    for case in [(64, 64, 1, 18, 1, 2, 21), (64, 128, 2, 18, 1, 2, 37),
                 (256, 256, 1, 18, 1, 2, 19), (64, 64, 1, 25, 1, 2, 19)]
    for prep in (False, True)
] + [((3, 64, 1, 18, 1, 2, 45), need_dx, False) for need_dx in (True, False)]  # unfolded
BF16_CASES = [
    # case, residual, need_dx
    ((64, 64, 1, 25, 3, 2, 29), False, True),
    ((64, 64, 1, 25, 3, 2, 29), False, False),
    ((64, 128, 2, 25, 3, 2, 33), False, True),
    ((32, 96, 1, 25, 3, 2, 42), False, True),
    ((64, 64, 1, 25, 3, 4, 2), False, True),
    ((64, 64, 1, 50, 3, 2, 17), False, True),
    ((96, 96, 1, 50, 3, 2, 13), False, True),
    ((24, 40, 1, 50, 3, 2, 11), False, True),
    ((64, 128, 2, 50, 3, 2, 23), False, True),
    ((256, 256, 1, 50, 3, 2, 7), False, True),
    ((64, 64, 1, 50, 3, 2, 16), True, True),
    ((64, 128, 2, 18, 1, 2, 37), True, True),
]


def _ids(cases):
    return ["-".join(str(p) for p in c[0]) + "".join(f"-{x}" for x in c[1:]) for c in cases]


def _check_block(pkg, case, gemm, residual=False, need_dx=True, prep=False):
    arrays, x, g = _random_case(pkg, *case, residual=residual)
    oracle = _Memo(lambda got: _oracle(arrays, got), lambda got: (got["y"] > 0,))

    def gate(got):
        want, floor = oracle(got)
        want = {k: v for k, v in want.items() if need_dx or k != "grad.x"}
        _compare(got, want, residual=residual, floor=floor)

    return _under_fills(
        pkg, lambda place: _run_hip(pkg, arrays, x, g, need_dx=need_dx, gemm=gemm, prep=prep,
                                    to_dev=place),
        gate, _desc(pkg, case, gemm, residual), _desc(pkg, case, gemm, residual, need_dx))


@pytest.mark.parametrize("case,residual,need_dx", FP32_CASES, ids=_ids(FP32_CASES))
def test_poisoned_fp32_block(pkg, case, residual, need_dx):
    _check_block(pkg, case, "fp32", residual, need_dx)


@pytest.mark.parametrize("gemm", SPLIT_MODES)
@pytest.mark.parametrize("case,need_dx,prep", SPLIT_CASES, ids=_ids(SPLIT_CASES))
def test_poisoned_split_block(pkg, case, need_dx, prep, gemm):
    _check_block(pkg, case, gemm, need_dx=need_dx, prep=prep)


@pytest.mark.parametrize("case,residual,need_dx", BF16_CASES, ids=_ids(BF16_CASES))
def test_poisoned_bf16_block(pkg, case, residual, need_dx):
    """test_gpu_bf16._check_bf16 per fill: the bf16 run and the fp32 run of its
    band check both on poisoned memory."""
    arrays, x, g = _random_case(pkg, *case, residual=residual)
    oracle = _Memo(lambda got: _bf16_reference(arrays, got, need_dx),
                   lambda got: (got["y"] > 0, got["inner_mask"]))

    def run(place):
        return (_run_bf16(pkg, arrays, x, g, bf16=True, need_dx=need_dx, to_dev=place),
                _run_bf16(pkg, arrays, x, g, bf16=False, need_dx=need_dx, to_dev=place))

    def gate(res):
        got, f32 = res
        want, ref16 = oracle(got)
        _gate_bf16(got, want, ref16, f32, residual)

    _under_fills(pkg, run, gate, _desc(pkg, case, "bf16", residual),
                 _desc(pkg, case, "bf16", residual, need_dx))


def test_block_cases_cover_every_plan(pkg):
    """Every STGCN_PLAN_* bit of include/stgcn_hip.h is selected by at least one
    block case above: a new kernel plan cannot arrive without a poison case."""
    with open(os.path.join(ROOT, "include", "stgcn_hip.h")) as f:
        bits = {n: int(v) for n, v in re.findall(r"#define\s+(STGCN_PLAN_\w+)\s+(\d+)", f.read())}
    assert len(bits) >= 10 and bits["STGCN_PLAN_X_FROM_U"] == pkg.hip_lib.PLAN_X_FROM_U
    descs = [_desc(pkg, c, "fp32", r, dx) for c, r, dx in FP32_CASES]
    descs += [_desc(pkg, c, m, False, dx) for c, dx, _ in SPLIT_CASES for m in SPLIT_MODES]
    descs += [_desc(pkg, c, "bf16", r, dx) for c, r, dx in BF16_CASES]
    union = 0
    for d in descs:
        union |= pkg.hip_lib.block_plan(d)
    missing = [n for n, v in bits.items() if not union & v]
    assert not missing, f"no poison block case selects {missing} (union {union:#x})"


@pytest.mark.parametrize("residual", [False, True])
def test_poisoned_dropout_block(pkg, residual):
    """Gated as test_gpu_block.test_block_dropout_matches_oracle."""
    case, drop = (64, 64, 1, 18, 1, 3, 40), 0.5
    arrays, x, g = _random_case(pkg, *case, seed=5, residual=residual)
    _under_fills(pkg, lambda place: _run_hip_dropout(pkg, arrays, x, g, drop, to_dev=place),
                 lambda res: _gate_dropout(arrays, res[0], res[1], drop, residual),
                 _desc(pkg, case, "fp32", residual))


@pytest.mark.parametrize("case,residual", [((64, 64, 1, 18, 1, 3, 40), False),
                                           ((64, 128, 2, 18, 1, 2, 37), True)])
def test_poisoned_eval_mode_backward(pkg, case, residual):
    """test_gpu_callers.test_block_eval_mode_backward (gate included) per fill."""
    _under_fills(pkg, lambda place: _check_eval_backward(pkg, case, residual, "fp32",
                                                         to_dev=place),
                 None, _desc(pkg, case, "fp32", residual, training=False))


# --- SpatialConv on its own (stgcn_spatial_fwd / _bwd) ----------------------------

@pytest.mark.parametrize("x_grad", [True, False])
@pytest.mark.parametrize("fixture,bf16", [(f, False) for f in _spatial_fixtures()] + [
    ("spatialconv_s64x64_v25k3.npz", True), ("spatialconv_s64x128_v50k3.npz", True)])
def test_poisoned_spatialconv(pkg, fixture, bf16, x_grad):
    """Gated as test_gpu_callers.test_spatialconv_standalone_matches_reference
    (fp32) and test_spatialconv_standalone_bf16."""
    ref = load_npz(fixture)
    want = _spatial_oracle(ref, torch.float64)
    near = _spatial_oracle(ref, torch.float32, gemm_bf16=bf16)
    if not x_grad:
        want.pop("grad.x")

    def gate(got):
        for k, w in want.items():
            err = rel_to_max(got[k].double().numpy(), w.double().numpy())
            floor = rel_to_max(near[k].double().numpy(), w.double().numpy())
            if bf16:
                assert err < max(2e-2, 3 * floor), (k, err, floor)
            else:
                assert err < max(TOL, 2 * floor), (k, err, floor)
                assert rel_to_max(got[k].double().numpy(), ref[k]) < 5e-5, k

    hl = pkg.hip_lib
    C_in, C_out = int(ref["meta"][0]), int(ref["meta"][1])
    N, _, T, V = ref["x"].shape
    d = hl.SpatialDesc(N, C_in, C_out, T, V, ref["param.A"].shape[0], hl.F_BF16 if bf16 else 0)
    ws = tuple(hl.lib().stgcn_spatial_workspace_bytes(ctypes.byref(d), w) for w in (0, 1))
    res = _under_fills(pkg, lambda place: _spatial_run(pkg, ref, bf16=bf16, to_dev=place,
                                                       x_grad=x_grad), gate, workspaces=ws)
    if bf16:
        with poison.poisoned(pkg, 0x00):
            f32 = _spatial_run(pkg, ref, to_dev=Place(0x00), x_grad=x_grad)
        assert not torch.equal(res[0x00]["y"], f32["y"]), "bf16 kernels did not run"


# --- stack cases: two full training steps (forward_loss, backward, FusedAdam), the
# persistent FoldPrep buffers and the Adam state reused, the rest poisoned again ---

def _stack_steps(pkg, model, xs, labs, fill, after_backward=None):
    """xs: NCTV inputs, one per step. Returns {name: CPU tensor} of every step's
    loss, logits and gradients, and the parameters and buffers at the end."""
    res = {}
    with poison.poisoned(pkg, fill):
        place = Place(fill)
        model = model.to(DEV).train()
        for k, v in list(model.named_parameters()) + list(model.named_buffers()):
            v.data = place(v.data.cpu(), k)
        opt = pkg.FusedAdam(model.parameters(), lr=1e-3)
        for step, (x, lab) in enumerate(zip(xs, labs)):
            loss, logits = model.forward_loss(place(x, "x"), place(lab, "labels"))
            opt.zero_grad()
            loss.backward()
            torch.cuda.synchronize()
            poison.check_inputs()   # x, the labels and the parameters, before Adam moves them
            if after_backward is not None:
                after_backward(step, model, loss, logits)
            res[f"{step}.loss"], res[f"{step}.logits"] = loss.detach().cpu(), logits.detach().cpu()
            for k, v in model.named_parameters():
                res[f"{step}.grad.{k}"] = v.grad.cpu()
            opt.step()
            torch.cuda.synchronize()
            poison.check_guards()
            poison.resnapshot()
        for k, v in list(model.named_parameters()) + list(model.named_buffers()):
            res["end." + k] = v.detach().cpu()
    poison.check_guards()
    lib = pkg.hip_lib.lib()   # the poison reached every block's workspaces
    for i, d in enumerate(pkg.fused.stack_descs(list(model.conv), tuple(xs[0].shape))):
        _has_buffer(lib.stgcn_fwd_workspace_bytes(ctypes.byref(d)), "forward",
                    f"forward workspace {i}")
        d.need_dx = int(i > 0)  # (the stack input needs no gradient)
        _has_buffer(lib.stgcn_bwd_workspace_bytes(ctypes.byref(d)), "backward",
                    f"backward workspace {i}")
    return res


@pytest.mark.parametrize("f32_gemm", ["f16x2", "bf16x3", "f16x2-nog"])
def test_poisoned_stack_fp32_split_bitwise(pkg, f32_gemm):
    """STGCNStack at V = 18: lazy links, x from U, deferred dx, y_stats, the head
    from U, dy_nc and the forward without its workspace memset. These paths are
    bit-reproducible (test_stack_lazy_links_bit_identical; the head and Adam use
    no atomics), so under both poisons everything equals the clean run."""
    gr = pkg.graph
    A = gr.get_normalized_adjacency_matrices(0, 1, graph=gr.graph_for(18))
    xs = [torch.randn(2, 3, 40, 18, generator=torch.Generator().manual_seed(4 + s))
          for s in range(2)]
    labs = [torch.randint(0, 400, (2,), generator=torch.Generator().manual_seed(14 + s))
            for s in range(2)]
    runs = {}
    for fill in poison.FILLS:
        torch.manual_seed(3)
        with contextlib.redirect_stdout(io.StringIO()):
            model = pkg.STGCNStack(3, 400, A, f32_gemm=f32_gemm)
        with _fill_named(fill):
            runs[fill] = _stack_steps(pkg, model, xs, labs, fill)
            _all_finite(runs[fill])
    clean = runs[0x00]
    assert any(k.startswith("1.grad.") for k in clean) and "end.fc_layer.weight" in clean
    for fill in poison.FILLS[1:]:
        diff = [k for k, v in clean.items() if not torch.equal(v, runs[fill][k])]
        assert not diff, f"fill {fill:#04x}: not bit-identical to the clean run: {diff}"


@pytest.mark.parametrize("V", [25, 50])
def test_poisoned_stack_bf16(pkg, V):
    """bf16 stacks (K = 3): the first step of every fill within the single-seed
    bound of test_stack_bf16_multi_seed, max(2e-2, 4x the bf16-operand reference's
    error) per tensor; both steps finite."""
    seed, N, T = 0, 2, 40
    A, model0, x, lab, params0 = _bf16_stack_setup(pkg, V, seed, N, T)
    oracles = _bf16_stack_oracle(A, params0, x, lab, seed)
    state0 = {k: v.clone() for k, v in model0.state_dict().items()}
    xs = [x.permute(0, 3, 1, 2).contiguous(),
          torch.randn(N, 3, T, V, generator=torch.Generator().manual_seed(seed + 7))]
    labs = [lab, lab.flip(0)]

    def gate(step, model, loss, logits):
        if step != 0:
            return
        errs, floor = _bf16_stack_vs_oracle(model, loss, logits, oracles)
        bad = [f"{k}: {e:.2e} (ref bf16 {floor[k]:.2e})" for k, e in errs.items()
               if not e <= max(2e-2, 4 * floor[k])]
        assert not bad, "; ".join(bad)

    for fill in poison.FILLS:
        _, model, _, _, _ = _bf16_stack_setup(pkg, V, seed, N, T)
        model.load_state_dict(state0)
        with _fill_named(fill):
            _all_finite(_stack_steps(pkg, model, xs, labs, fill, after_backward=gate))
