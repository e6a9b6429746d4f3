"""The parity gates fail on non-finite errors (CPU; tests/gates.py).

`err > lim` is false for a NaN error, and conftest.rel_to_max returns NaN as
soon as either side holds one, so a gate written that way passed an all-NaN
gradient. The gates of test_gpu_block / _stack / _callers go through
gates.exceeds; here each is handed hand-made tensors with a NaN in them."""
import math

import numpy as np
import pytest
import torch

import test_gpu_block
import test_gpu_callers
import test_gpu_stack
from gates import exceeds, worst_of

NAN, INF = float("nan"), float("inf")


def test_exceeds_rejects_nonfinite_and_accepts_the_limit():
    assert exceeds(NAN, 1e-5) and exceeds(INF, 1e-5) and exceeds(2e-5, 1e-5)
    assert exceeds(0.0, NAN) and exceeds(NAN, NAN) and exceeds(NAN, INF)
    assert not exceeds(1e-5, 1e-5) and not exceeds(0.0, 1e-5) and not exceeds(1e30, INF)
    assert exceeds(np.float64(NAN), 1e-5) and not exceeds(np.float32(0.5), np.float32(0.5))
    assert math.isnan(NAN) and not (NAN > 1e-5)  # (the form the gates had)


# the three situations: one NaN in `got`, a whole tensor of `got` NaN, a NaN in `want` only
def _spoil(how, got, want):
    got, want = got.clone(), want.clone()
    if how == "one":
        got.view(-1)[1] = NAN
    elif how == "all":
        got[...] = NAN
    else:
        want.view(-1)[1] = NAN
    return got, want


HOW = ["one", "all", "want"]


def _block_dicts():
    y = torch.tensor([[0.0, 1.0, 2.0], [3.0, 0.5, 0.25]])
    return {k: y.clone() * s for k, s in (("y", 1.0), ("grad.x", 2.0),
                                           ("grad.temporalConv.bias", 1e-7))}


@pytest.mark.parametrize("key", ["y", "grad.x", "grad.temporalConv.bias"])
@pytest.mark.parametrize("how", HOW)
def test_block_compare_raises(how, key):
    got, want = _block_dicts(), _block_dicts()
    test_gpu_block._compare(got, want)  # (equal tensors pass)
    floor = {k: 0.0 for k in want}
    floor["abs:grad.temporalConv.bias"] = 0.0
    test_gpu_block._compare(got, want, floor=floor)
    got[key], want[key] = _spoil(how, got[key], want[key])
    with pytest.raises(AssertionError):
        test_gpu_block._compare(got, want)
    with pytest.raises(AssertionError):
        test_gpu_block._compare(got, want, floor=floor)


class _P:
    """A named parameter as the stack gates read it: .grad only."""

    def __init__(self, grad):
        self.grad = grad


class _Model:
    def __init__(self, grads):
        self._g = grads

    def named_parameters(self):
        return [(k, _P(v)) for k, v in self._g.items()]


def _grads():
    g = torch.Generator().manual_seed(0)
    return {"conv.0.spatialConv.A": torch.randn(1, 3, 3, generator=g),
            "conv.0.batch_n.weight": torch.randn(4, generator=g),
            "fc_layer.weight": torch.randn(2, 4, generator=g)}


@pytest.mark.parametrize("key", list(_grads()))
@pytest.mark.parametrize("how", HOW)
def test_stack_gate_raises(how, key):
    got, want = _grads(), _grads()
    test_gpu_stack.gate_stack_grads(_Model(got), want, want)
    got[key], want[key] = _spoil(how, got[key], want[key])
    with pytest.raises(AssertionError):
        test_gpu_stack.gate_stack_grads(_Model(got), want, _grads())


@pytest.mark.parametrize("key", list(_grads()))
@pytest.mark.parametrize("how", HOW)
def test_callers_gates_raise(how, key):
    got, want = _grads(), _grads()
    test_gpu_callers._gate_chain_pairs(_Model(got).named_parameters(),
                                       _Model(want).named_parameters())
    ref = {}
    for k, v in want.items():
        ref["pidx." + k] = np.arange(v.numel())
        ref["gval." + k] = v.reshape(-1).numpy().copy()
    test_gpu_callers._gate_sampled_grads(_Model(got).named_parameters(), ref)
    got[key], want[key] = _spoil(how, got[key], want[key])
    ref["gval." + key] = want[key].reshape(-1).numpy().copy()
    with pytest.raises(AssertionError):
        test_gpu_callers._gate_chain_pairs(_Model(got).named_parameters(),
                                           _Model(want).named_parameters())
    with pytest.raises(AssertionError):
        test_gpu_callers._gate_sampled_grads(_Model(got).named_parameters(), ref)


def test_worst_of_keeps_a_nan_wherever_it_stands():
    """The data-parallel tests (dp_gpu_worker.py, test_dp_gloo.py) reduce their
    per-tensor errors with worst_of and assert `worst < tol`."""
    assert worst_of([]) == 0.0 and worst_of([0.5, 2.0, 1.0]) == 2.0
    for errs in ([NAN, 1.0], [1.0, NAN], [0.0, 1.0, NAN, 2.0], (e for e in (1.0, NAN))):
        w = worst_of(errs)
        assert math.isnan(w) and not w < 1e-6
    assert worst_of([1.0, INF]) == INF
    assert max(0.0, NAN) == 0.0 and max([1.0, NAN]) == 1.0  # (the forms the tests had)


def test_dp_gloo_gradient_gate_sees_a_nan():
    """test_dp_gloo's worker with one NaN planted in a reduced gradient reports
    a NaN error, which `assert worst < 1e-5` rejects."""
    import test_dp_gloo
    errs = []
    a, b = torch.ones(4), torch.ones(4)
    for got in (a, torch.tensor([1.0, NAN, 1.0, 1.0])):
        denom = max(b.abs().max().item(), 1e-12)
        errs.append((got - b).abs().max().item() / denom)
    assert test_dp_gloo.worst_of is worst_of and math.isnan(worst_of(errs))
    with pytest.raises(AssertionError):
        assert worst_of(errs) < 1e-5
