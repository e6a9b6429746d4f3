"""Gate helpers shared by the parity tests.

``exceeds`` is the one comparison every "collect the bad tensors" gate uses:
``err > lim`` is false for a NaN error, so a kernel that returned an all-NaN
gradient passed such a gate; ``not (err <= lim)`` is true for it.

The rest states the non-finite rule of include/stgcn_hip.h (Conventions,
"Non-finite values") for one block: which output elements one bad input
element reaches (its footprint), and the three checks (a), (b), (c) of a HIP
result against the oracle's IEEE propagation. Index convention of the
adjacency as in oracle/ref_cpu.py: out[n, c, t, v] = sum_kw A[k, v, w] Y[n, k, c, t, w],
so input joint ``w`` reaches the output joints ``v`` with A[k, v, w] != 0.
"""
import numpy as np

PAD = 4  # temporal kernel 9: an input frame t reaches output frames |t' * stride - t| <= 4


def exceeds(err, lim):
    """Does this error exceed this limit? A NaN (or +Inf) error, or a NaN
    limit, counts as exceeding; an error equal to the limit does not."""
    return not (err <= lim)


def worst_of(errs):
    """The largest of some errors, NaN as soon as one of them is NaN. Python's
    max() keeps its first argument against a NaN (max(0.0, nan) is 0.0) and
    drops a NaN in any later position, so `worst = max(worst, e)` followed by
    `assert worst < tol` passed an all-NaN gradient."""
    errs = [float(e) for e in errs]
    if any(e != e for e in errs):
        return float("nan")
    return max(errs, default=0.0)


def _frames_out(t, stride, T_out):
    tt = np.arange(T_out)
    return np.abs(tt * stride - t) <= PAD


def _frames_in(t_out, stride, T):
    tt = np.arange(T)
    return np.abs(t_out * stride - tt) <= PAD


def _as_A(A):
    return np.asarray(A, dtype=np.float64)


def fwd_footprint(A, stride, xshape, C_out, pos, residual=False):
    """(sparse, dense) boolean masks over y (N, C_out, T_out, V) of the output
    elements that x[pos] = x[n, c, t, v] reaches in the block's forward.
    sparse: clip n, every channel, frames |t' * stride - t| <= 4, joints v'
    with A[k, v', v] != 0 for some k (and, in a residual block, the element the
    skip path carries x[pos] to). dense: the same frames at every joint -- what
    dense arithmetic reaches when 0 * NaN counts."""
    A = _as_A(A)
    N, _, T, V = xshape
    n, _, t, v = pos
    T_out = (T - 1) // stride + 1
    fr = _frames_out(t, stride, T_out)
    jo = (A[:, :, v] != 0).any(axis=0)
    skip = np.zeros((T_out, V), bool)
    if residual and t % stride == 0:  # (the skip path: frame t / stride, joint v)
        skip[t // stride, v] = True
    sparse = np.zeros((N, C_out, T_out, V), bool)
    dense = np.zeros_like(sparse)
    sparse[n] = (fr[:, None] & jo[None, :]) | skip
    dense[n] = fr[:, None]
    return sparse, dense


def bwd_footprint(A, stride, xshape, pos, residual=False):
    """(sparse, dense) masks over dx (N, C_in, T, V) of the elements that a bad
    g[pos] = g[n, o, t', w] reaches in the eval-mode backward: the transposed
    set of ``fwd_footprint`` (joints v with A[k, w, v] != 0)."""
    A = _as_A(A)
    N, C_in, T, V = xshape
    n, _, to, w = pos
    fr = _frames_in(to, stride, T)
    jo = (A[:, w, :] != 0).any(axis=0)
    skip = np.zeros((T, V), bool)
    if residual and to * stride < T:
        skip[to * stride, w] = True
    sparse = np.zeros((N, C_in, T, V), bool)
    dense = np.zeros_like(sparse)
    sparse[n] = (fr[:, None] & jo[None, :]) | skip
    dense[n] = fr[:, None]
    return sparse, dense


def finite_err(got, want, where=None):
    """max |got - want| / max |want| over the elements of ``where`` (default:
    all) at which both are finite -- conftest.rel_to_max restricted to them, so
    no NaN reaches it. The scale is max |want| over want's finite elements."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    fw = np.isfinite(want)
    both = fw & np.isfinite(got)
    if where is not None:
        both &= where
    if not both.any():
        return 0.0
    denom = max(np.abs(want[fw]).max(), 1e-30)
    return float(np.abs(got[both] - want[both]).max() / denom)


def check_rules(name, got, want, lim, sparse=None, dense=None, clean=None, clip=None,
                whole=False, nonfinite_ok=False):
    """Rules (a), (b), (c) on one tensor; raises AssertionError naming the rule.

    got / want: the HIP result and the oracle's (IEEE propagation) for the
    input with the bad element. lim: the test's usual rel-to-max gate.
    sparse / dense: the bad element's footprints over this tensor.
    whole: training mode -- rule (a) over the whole tensor, wherever ``want``
    is non-finite. clean / clip: rule (c), the oracle of the clean input and
    the index of the clip that holds the bad element (eval mode).
    nonfinite_ok: the narrowed rule (c) -- other clips finite and at the gate,
    or non-finite."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    gf, wf = np.isfinite(got), np.isfinite(want)
    # (a) a non-finite oracle value the sparse arithmetic reaches stays non-finite
    must = ~wf if whole else (~wf & sparse if sparse is not None else np.zeros_like(wf))
    lost = must & gf
    assert not lost.any(), \
        f"{name}: rule (a): {int(lost.sum())} of {int(must.sum())} non-finite oracle elements " \
        f"came out finite, first at {tuple(np.argwhere(lost)[0])} = {got[lost][0]!r}"
    # (b) where the oracle is finite: at the gate, or non-finite inside the dense footprint
    stray = wf & ~gf
    if dense is not None:
        stray &= ~dense
    elif whole and not wf.all():
        stray &= False  # (no footprint to hold it to; a wholly finite oracle stays strict)
    if clip is not None and nonfinite_ok:
        stray &= False
    assert not stray.any(), \
        f"{name}: rule (b): {int(stray.sum())} non-finite elements outside the dense footprint, " \
        f"first at {tuple(np.argwhere(stray)[0])}"
    err = finite_err(got, want)
    assert not exceeds(err, lim), f"{name}: rule (b): finite remainder {err:.2e} > {lim:.1e}"
    # (c) every other clip as if the bad element were not there
    if clip is not None:
        clean = np.asarray(clean, np.float64)
        others = np.ones(got.shape[0], bool)
        others[clip] = False
        if not nonfinite_ok:
            assert gf[others].all(), \
                f"{name}: rule (c): {int((~gf[others]).sum())} non-finite elements in other clips"
        where = np.zeros(got.shape, bool)
        where[others] = True
        err = finite_err(got, clean, where)
        assert not exceeds(err, lim), f"{name}: rule (c): other clips {err:.2e} > {lim:.1e}"
