"""The C-ABI library builds, loads and exports every symbol include/stgcn_hip.h
declares; descriptor validation and workspace sizing work without a GPU."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "stgcn_hip.h")


def _header_functions():
    text = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:int|size_t|const char\s*\*)\s*\*?\s*(stgcn_\w+)\s*\(",
                                 text, flags=re.M)))


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.hip_lib.load_library()


def test_header_declares_entry_points(pkg):
    assert _header_functions() == sorted(pkg.hip_lib.EXPORTED)


def test_library_exports_every_header_symbol(pkg, lib):
    for name in _header_functions():
        assert hasattr(lib, name), name
    assert lib.stgcn_abi_version() == pkg.hip_lib.ABI_VERSION == 11


def _desc(pkg, **kw):
    base = dict(N=128, C_in=64, C_out=64, T=300, T_out=300, V=18, K=1, gamma=9, stride=1,
                pad=4, eps=1e-5, momentum=0.1, training=1, need_dx=1, flags=0)
    base.update(kw)
    return pkg.hip_lib.Desc(**base)


def test_check_desc_accepts_north_star_shapes(pkg, lib):
    for kw in (dict(), dict(C_in=3), dict(C_in=64, C_out=128, stride=2, T_out=150),
               dict(V=25, K=3), dict(V=50, K=3, C_in=256, C_out=256, T=75, T_out=75),
               dict(flags=1), dict(flags=1, C_in=64, C_out=128, stride=2, T_out=150),
               dict(flags=1, V=25, K=3, C_in=3),
               # STGCN_F_BF16 (cfg3 / cfg5 shapes, residual + bf16)
               dict(flags=2, V=25, K=3), dict(flags=2, V=50, K=3, C_in=128, C_out=256, stride=2,
                                               T_out=150), dict(flags=3, V=18),
               # STGCN_F_F32X3 (fp32 via bf16 splits), plain and residual; + STGCN_F_F16X2
               dict(flags=4), dict(flags=5, V=25, K=3), dict(flags=12),
               # + STGCN_F_NO_G (ABI 7)
               dict(flags=28)):
        d = _desc(pkg, **kw)
        assert lib.stgcn_check_desc(ctypes.byref(d)) == 0, kw
        assert lib.stgcn_fwd_workspace_bytes(ctypes.byref(d)) > 0
        assert lib.stgcn_bwd_workspace_bytes(ctypes.byref(d)) > 0


@pytest.mark.parametrize("kw,code", [
    (dict(flags=32), -2), (dict(flags=16), -1), (dict(flags=20), -1), (dict(flags=8), -1), (dict(flags=10), -1), (dict(flags=6), -1), (dict(gamma=7, pad=3, T_out=300), -2), (dict(stride=3, T_out=100), -2),
    (dict(T_out=299), -1), (dict(N=0), -1), (dict(V=300), -2)])
def test_check_desc_rejects(pkg, lib, kw, code):
    d = _desc(pkg, **kw)
    assert lib.stgcn_check_desc(ctypes.byref(d)) == code
    assert lib.stgcn_last_error()
    assert lib.stgcn_fwd_workspace_bytes(ctypes.byref(d)) == 0


@pytest.mark.parametrize("flags", [0, 2, 4, 12])
def test_check_desc_partition_counts(pkg, lib, flags):
    """K = 1..4 at V = 18 / 25 / 50 (the descriptors of test_gpu_partitions.py's
    matrix, every GEMM mode): accepted, with workspaces and a plan; V = 50 with
    K = 4 has K * V * V = 10000 > 8192 and is refused as unsupported."""
    from partition_cases import CASES, MATRIX
    for cid in MATRIX:
        C_in, C_out, stride, V, _, K, N, T = CASES[cid]
        d = _desc(pkg, N=N, C_in=C_in, C_out=C_out, T=T, T_out=(T - 1) // stride + 1, V=V, K=K,
                  stride=stride, flags=flags)
        assert lib.stgcn_check_desc(ctypes.byref(d)) == 0, (cid, lib.stgcn_last_error())
        assert lib.stgcn_fwd_workspace_bytes(ctypes.byref(d)) > 0, cid
        assert lib.stgcn_bwd_workspace_bytes(ctypes.byref(d)) > 0, cid
        pkg.hip_lib.block_plan(d)
    d = _desc(pkg, N=2, T=8, T_out=8, V=50, K=4, flags=flags)
    assert lib.stgcn_check_desc(ctypes.byref(d)) == -2
    assert b"K*V*V" in lib.stgcn_last_error()
    assert lib.stgcn_fwd_workspace_bytes(ctypes.byref(d)) == 0
    with pytest.raises(RuntimeError, match=r"failed \(-2\)"):
        pkg.hip_lib.block_plan(d)


def test_null_arguments_fail_without_touching_gpu(pkg, lib):
    d = _desc(pkg)
    args = pkg.hip_lib.FwdArgs()
    assert lib.stgcn_block_fwd(ctypes.byref(d), ctypes.byref(args), None, 0, None) == -1
    assert b"null" in lib.stgcn_last_error()


def test_residual_null_projection_fails(pkg, lib):
    """A projection residual block (C_in != C_out) needs Wr / br / Za."""
    d = _desc(pkg, flags=1, C_in=32)
    args = pkg.hip_lib.FwdArgs(*([ctypes.c_void_p(256)] * 18))  # dummy non-null core args
    assert lib.stgcn_block_fwd(ctypes.byref(d), ctypes.byref(args), None, 0, None) == -1
    assert b"residual" in lib.stgcn_last_error()


def test_cpu_tensors_fail_loudly(pkg):
    """No CPU fallback on the product path."""
    import torch
    A = torch.ones(1, 18, 18)
    blk = pkg.SpatialTemporalConv(3, 64, A, 9, 1, 4, dropout_rate=0)
    with pytest.raises(RuntimeError):
        blk(torch.randn(2, 3, 20, 18))


def test_spatial_desc_workspace_and_rejects(pkg, lib):
    """ABI 4 SpatialConv entry points: workspace queries for the reference's
    graphs; unknown flags / bad shapes rejected without touching the GPU."""
    SD = pkg.hip_lib.SpatialDesc
    for kw in (dict(V=18, K=1, C_in=3), dict(V=25, K=3), dict(V=50, K=3, flags=2)):
        base = dict(N=8, C_in=64, C_out=64, T=300, V=18, K=1, flags=0)
        base.update(kw)
        d = SD(**base)
        assert lib.stgcn_spatial_workspace_bytes(ctypes.byref(d), 0) > 0, kw
        assert lib.stgcn_spatial_workspace_bytes(ctypes.byref(d), 1) > 0, kw
    for kw in (dict(flags=1), dict(flags=4), dict(N=0), dict(V=300)):
        base = dict(N=8, C_in=64, C_out=64, T=300, V=18, K=1, flags=0)
        base.update(kw)
        d = SD(**base)
        assert lib.stgcn_spatial_workspace_bytes(ctypes.byref(d), 0) == 0, kw
    d = SD(N=8, C_in=64, C_out=64, T=30, V=18, K=1, flags=0)
    assert lib.stgcn_spatial_fwd(ctypes.byref(d), None, None, None, None, None, None, 0,
                                 None) == -1
    assert b"null" in lib.stgcn_last_error()


def test_block_plan_pins_the_paths(pkg, lib):
    """ABI 6 stgcn_block_plan (host logic, no GPU): the fp32 split path folds W'
    into the temporal conv on the cfg2 non-residual blocks with C_in >= 16
    (STGCN_PLAN_FOLD) and keeps the unfolded spatial dW' on split products where
    it does not fold (residual blocks); the bf16 path fuses both SpatialConv
    halves at V = 25, K = 3; the exact fp32-MFMA path selects none of these."""
    hl = pkg.hip_lib
    plan = lambda **kw: hl.block_plan(_desc(pkg, **kw))  # noqa: E731
    p = plan(flags=4)  # cfg2 L1-type block (64 -> 64)
    assert p & hl.PLAN_FOLD and p & hl.PLAN_TCONV_SPLIT and p & hl.PLAN_TWGRAD_SPLIT, p
    assert p & hl.PLAN_SP_BWD_FUSED, p  # the SpatialConv backward in the data gradient
    assert plan(flags=4, C_in=128, C_out=256, stride=2, T=150, T_out=75) & hl.PLAN_FOLD
    assert not plan(flags=4, C_in=3) & hl.PLAN_FOLD          # C_in < 16
    p = plan(flags=5)                                        # residual: never folded
    assert not p & hl.PLAN_FOLD and p & hl.PLAN_WSP_SPLIT, p
    assert not plan(flags=4, V=25, K=3) & hl.PLAN_FOLD       # K = 3
    # the reference's default graph (V = 25, unilabeling K = 1) folds too, with the
    # unfused SpatialConv backward (the fused epilogue is V = 18 only)
    p = plan(flags=12, V=25, K=1)
    assert p & hl.PLAN_FOLD and p & hl.PLAN_F16X2 and not p & hl.PLAN_SP_BWD_FUSED, p
    assert not p & hl.PLAN_X_FROM_U, p
    assert not plan(flags=12, V=50, K=1) & hl.PLAN_FOLD      # (no V = 50 split instances)
    p = plan(flags=2, V=25, K=3)
    assert p & hl.PLAN_SP_FWD_FUSED and p & hl.PLAN_SP_BWD_FUSED and not p & hl.PLAN_FOLD, p
    assert plan() == 0
    # STGCN_F_F16X2 (with F32X3): the folded GEMMs on fp16 splits; unfolded blocks unchanged
    p = plan(flags=12)
    assert p & hl.PLAN_FOLD and p & hl.PLAN_F16X2, p
    # the unfolded first block (C_in = 3): forward and weight gradient on fp16 splits
    p = plan(flags=12, C_in=3)
    assert p & hl.PLAN_F16X2 and not p & hl.PLAN_FOLD, p
    assert not plan(flags=13) & hl.PLAN_F16X2
    d = _desc(pkg, N=0)
    out = ctypes.c_uint32(7)
    assert lib.stgcn_block_plan(ctypes.byref(d), ctypes.byref(out)) == -1


def test_fold_prep_sizes(pkg, lib):
    """ABI 7 stgcn_fold_prep_bytes: a buffer for the folded split-path blocks
    (K = 1, V = 18, fp32 via splits), none for blocks that do not fold (first
    block C_in = 3, K = 3, residual, bf16, exact fp32 MFMA)."""
    fl = pkg.hip_lib
    folded = [dict(C_in=64, flags=12), dict(C_in=64, C_out=128, stride=2, T_out=150, flags=12),
              dict(C_in=64, flags=4), dict(C_in=64, flags=28), dict(C_in=64, V=25, flags=12)]
    for kw in folded:
        assert lib.stgcn_fold_prep_bytes(ctypes.byref(_desc(pkg, **kw))) > 0, kw
    for kw in (dict(C_in=3, flags=12), dict(V=25, K=3, flags=4), dict(C_in=64, flags=13),
               dict(C_in=64, flags=2), dict(C_in=64, flags=0)):
        assert lib.stgcn_fold_prep_bytes(ctypes.byref(_desc(pkg, **kw))) == 0, kw
    # no blocks: nothing to do, no GPU touched
    assert lib.stgcn_fold_prep(0, None, None, None, None) == 0



def test_x_from_u_plan_and_argument_checks(pkg, lib):
    """ABI 8 (host logic, no GPU): STGCN_PLAN_X_FROM_U on the folded training
    blocks that form G (cfg2 f16x2 / split paths) and, round 6, on the bf16
    blocks whose fused spatial forward stages x (cfg3 / cfg5: V = 25, 50 with
    K = 3); not in eval, not without G (STGCN_F_NO_G), not on residual blocks,
    not where the block neither folds nor runs the bf16 fused forward. A forward
    with prev_U on a block without the plan, and a backward with x null outside
    it, fail before any launch."""
    hl = pkg.hip_lib
    plan = lambda **kw: hl.block_plan(_desc(pkg, **kw))  # noqa: E731
    for kw in (dict(flags=12), dict(flags=4), dict(flags=12, C_in=128, C_out=256, stride=2,
                                                  T=150, T_out=75),
               dict(flags=2, V=25, K=3), dict(flags=2, V=50, K=3)):
        assert plan(**kw) & hl.PLAN_X_FROM_U, kw
    for kw in (dict(flags=12, training=0), dict(flags=28), dict(flags=12, C_in=3),
               dict(flags=13), dict(flags=3, V=25, K=3), dict(flags=2, V=25, K=3, training=0),
               dict(flags=0)):
        assert not plan(**kw) & hl.PLAN_X_FROM_U, kw
    one = ctypes.c_void_p(256)
    d = _desc(pkg, flags=0)  # exact fp32 MFMA: no X_FROM_U
    a = hl.FwdArgs(*([one] * 18))
    a.prev_U = a.prev_stats = a.prev_g2 = a.prev_b2 = one
    a.x_stats = one
    assert lib.stgcn_block_fwd(ctypes.byref(d), ctypes.byref(a), None, 0, None) == -1
    assert b"prev_U" in lib.stgcn_last_error()
    b = hl.BwdArgs(*([one] * 23))
    b.x = None
    b.G = one
    assert lib.stgcn_block_bwd(ctypes.byref(d), ctypes.byref(b), None, 0, None) == -1
    assert b"x null" in lib.stgcn_last_error()


def test_head_link_decision(pkg):
    """ABI 9: the last block's output is left to the fused head only for a
    non-residual block without dropout and without forward hooks."""
    import contextlib
    import io
    gr = pkg.graph
    A = gr.get_normalized_adjacency_matrices(0, 1, graph=gr.graph_for(18))
    with contextlib.redirect_stdout(io.StringIO()):
        m = pkg.STGCNStack(3, 10, A)
        mr = pkg.STGCNStack(3, 10, A, residual=True)
        md = pkg.STGCNStack(3, 10, A, dropout_rate=0.5)
    assert pkg.fused.head_link_ok(m.conv[-1])
    assert not pkg.fused.head_link_ok(mr.conv[-1])
    assert not pkg.fused.head_link_ok(md.conv[-1])
    h = m.conv[-1].register_forward_hook(lambda *a: None)
    assert not pkg.fused.head_link_ok(m.conv[-1])
    h.remove()
    assert pkg.fused.head_link_ok(m.conv[-1])


# ---------------------------------------------------------------------------
# The alignment contract (include/stgcn_hip.h, Conventions): with fake pointer
# values, no GPU touched -- every call below stops at an argument check.
# ---------------------------------------------------------------------------
_FWD_PTRS = ("x", "A", "W", "bW", "Wt", "bWt", "g1", "b1", "g2", "b2", "rm1", "rv1", "rm2",
             "rv2", "y", "Z", "U", "stats", "Wr", "br", "Za", "G", "x_stats", "y_stats", "prep",
             "prev_U", "prev_stats", "prev_g2", "prev_b2")
_BWD_PTRS = ("dy", "x", "Z", "U", "stats", "A", "W", "bW", "Wt", "g1", "b1", "g2", "b2", "dx",
             "dA", "dW", "dbW", "dWt", "dbWt", "dg1", "db1", "dg2", "db2", "Wr", "Za", "y", "dWr",
             "dbr", "G", "dy_sums", "prev_g2", "prev_b2", "prev_sums", "prev_U", "prev_stats",
             "x_stats", "dx_coef", "dy_coef", "prep", "dy_nc")
_NATURAL = ("rm1", "rv1", "rm2", "rv2", "prev_stats")      # fp32, taken at 4 bytes
_FP64 = ("x_stats", "y_stats", "dy_sums", "prev_sums")     # fp64 blocks: 16 all the same
_OK = 256


def _named(lib, name, align):
    return f"{name}: must be {align}-byte aligned".encode() in lib.stgcn_last_error()


def _block_call(pkg, lib, which, ws=None, **ptrs):
    """stgcn_block_fwd / _bwd of a folded f16x2 block (every optional argument
    applies to it) with every pointer argument a 256-aligned fake but ``ptrs``;
    no workspace bytes, so a call that passes the argument checks stops at
    "workspace too small"."""
    hl = pkg.hip_lib
    d = _desc(pkg, flags=12)
    a = hl.FwdArgs() if which == "fwd" else hl.BwdArgs()
    for n in (_FWD_PTRS if which == "fwd" else _BWD_PTRS):
        setattr(a, n, ptrs.get(n, _OK))
    if which == "bwd":
        a.dx_deferred = _OK     # (a host int: no alignment asked)
    fn = lib.stgcn_block_fwd if which == "fwd" else lib.stgcn_block_bwd
    return fn(ctypes.byref(d), ctypes.byref(a), ws, 0, None)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_block_pointer_alignment_is_checked_by_name(pkg, lib, which):
    assert _block_call(pkg, lib, which) == -1
    assert b"workspace too small" in lib.stgcn_last_error()
    assert _block_call(pkg, lib, which, ws=_OK) == -1
    assert b"workspace too small" in lib.stgcn_last_error()
    for off in (4, 8, 12):
        assert _block_call(pkg, lib, which, ws=_OK + off) == -1
        assert _named(lib, "workspace", 16), lib.stgcn_last_error()
    for name in (_FWD_PTRS if which == "fwd" else _BWD_PTRS):
        if name in _NATURAL:
            for off in (4, 8, 12):   # natural alignment: accepted
                assert _block_call(pkg, lib, which, **{name: _OK + off}) == -1
                assert b"workspace too small" in lib.stgcn_last_error(), (name, off)
            assert _block_call(pkg, lib, which, **{name: _OK + 2}) == -1
            assert _named(lib, name, 4), (name, lib.stgcn_last_error())
            continue
        for off in (4, 8) if name in _FP64 else (4,):
            assert _block_call(pkg, lib, which, **{name: _OK + off}) == -1
            if name == "prev_U" and which == "fwd":   # (its own, older message)
                assert b"16-byte aligned prev_U" in lib.stgcn_last_error()
            else:
                assert _named(lib, name, 16), (name, off, lib.stgcn_last_error())


def test_ignored_block_pointers_are_not_checked(pkg, lib):
    """dx without need_dx and U of a residual block are ignored, misaligned or not."""
    hl = pkg.hip_lib
    d = _desc(pkg, need_dx=0)
    b = hl.BwdArgs(*([_OK] * 23))
    b.dx = _OK + 4
    assert lib.stgcn_block_bwd(ctypes.byref(d), ctypes.byref(b), None, 0, None) == -1
    assert b"workspace too small" in lib.stgcn_last_error()
    d = _desc(pkg, flags=1)
    a = hl.FwdArgs(*([_OK] * 21))
    a.U = _OK + 4
    assert lib.stgcn_block_fwd(ctypes.byref(d), ctypes.byref(a), None, 0, None) == -1
    assert b"workspace too small" in lib.stgcn_last_error()


def test_spatial_pointer_alignment_is_checked_by_name(pkg, lib):
    """SpatialConv on its own: outputs and the workspace at 16 bytes; the inputs at
    16 under STGCN_F_BF16, at their natural 4 on the fp32 path (which routes a
    misaligned x / dout to its narrower kernels)."""
    fwd, bwd = ("x", "A", "W", "bW", "out"), ("dout", "x", "A", "W", "bW", "dx", "dA", "dW", "dbW")
    inputs = ("x", "A", "W", "bW", "dout")
    for flags in (0, 2):
        d = pkg.hip_lib.SpatialDesc(N=8, C_in=64, C_out=64, T=30, V=25, K=3, flags=flags)
        for names, fn in ((fwd, lib.stgcn_spatial_fwd), (bwd, lib.stgcn_spatial_bwd)):
            assert fn(ctypes.byref(d), *([_OK] * len(names)), None, 0, None) == -1
            assert b"workspace too small" in lib.stgcn_last_error()
            assert fn(ctypes.byref(d), *([_OK] * len(names)), _OK + 4, 0, None) == -1
            assert _named(lib, "workspace", 16), lib.stgcn_last_error()
            for i, name in enumerate(names):
                vals = [_OK] * len(names)
                vals[i] = _OK + 4
                assert fn(ctypes.byref(d), *vals, None, 0, None) == -1
                if name in inputs and flags == 0:
                    assert b"workspace too small" in lib.stgcn_last_error(), name
                    vals[i] = _OK + 2
                    assert fn(ctypes.byref(d), *vals, None, 0, None) == -1
                    assert _named(lib, name, 4), (name, lib.stgcn_last_error())
                else:
                    assert _named(lib, name, 16), (name, flags, lib.stgcn_last_error())


def test_fold_prep_pointer_alignment_is_checked_by_name(pkg, lib):
    hl = pkg.hip_lib
    d = _desc(pkg, flags=12)
    names = ("A", "W", "bW", "Wt", "bWt")
    for bad in names + ("prep",):
        w = hl.FoldWeights(*[(_OK + 4 if n == bad else _OK) for n in names])
        prep = (ctypes.c_void_p * 1)(_OK + 4 if bad == "prep" else _OK)
        assert lib.stgcn_fold_prep(1, ctypes.byref(d), ctypes.byref(w), prep, None) == -1
        assert _named(lib, bad, 16), (bad, lib.stgcn_last_error())


def test_head_and_adam_take_natural_alignment(pkg, lib):
    """The head and Adam kernels access one element at a time: fp32 tensors are
    taken at 4 bytes (a view into a flat gradient bucket), int64 labels, the
    metrics block and the Adam table at 8. A head that is too large for its LDS
    is refused (-2) after the alignment checks: that is how an accepted fake
    call ends here without a launch."""
    hl = pkg.hip_lib
    big = hl.HeadDesc(4, 64, 54, 20000)
    ebig = hl.EvalDesc(4, 64, 54, 20000, 1)
    calls = [  # (function, descriptor, argument names)
        (lib.stgcn_head_fwd, big, ("y", "W", "bias", "labels", "pooled", "logits", "lossv",
                                   "loss")),
        (lib.stgcn_head_fwd_u, big, ("U", "stats2", "g2", "b2", "W", "bias", "labels", "pooled",
                                     "logits", "lossv", "loss")),
        (lib.stgcn_head_eval, ebig, ("y / U", "W", "bias", "labels", "pooled", "logits", "lossv",
                                     "loss", "pred", "metrics")),
        (lib.stgcn_head_eval_u, ebig, ("y / U", "stats2", "g2", "b2", "W", "bias", "labels",
                                       "pooled", "logits", "lossv", "loss", "pred", "metrics")),
    ]
    for fn, d, names in calls:
        for i, name in enumerate(names):
            wide = name in ("labels", "metrics")
            vals = [_OK + (8 if n in ("labels", "metrics") else 4) for n in names]
            if name == "metrics":
                # (checked after the LDS limit's -2 would hit: take a head that fits,
                # and let the call stop at the misaligned block itself)
                d2 = hl.EvalDesc(4, 64, 54, 10, 1)
                vals[i] = _OK + 4
                assert fn(ctypes.byref(d2), *vals, None) == -1
                assert _named(lib, name, 8), (name, lib.stgcn_last_error())
                continue
            assert fn(ctypes.byref(d), *vals, None) == -2, (name, lib.stgcn_last_error())
            assert b"too large" in lib.stgcn_last_error()
            vals[i] = _OK + (4 if wide else 2)
            assert fn(ctypes.byref(d), *vals, None) == -1
            assert _named(lib, name, 8 if wide else 4), (name, lib.stgcn_last_error())
    small = hl.HeadDesc(4, 64, 54, 10)
    for fn, names in ((lib.stgcn_head_bwd, ("pooled", "logits", "W", "labels", "dloss", "dlogits",
                                            "dpooled", "dy", "dW", "dbias")),
                      (lib.stgcn_head_bwd_nc, ("pooled", "logits", "W", "labels", "dloss",
                                               "dlogits", "dpooled", "dy_nc", "dW", "dbias"))):
        for i, name in enumerate(names):
            vals = [_OK] * len(names)
            vals[i] = _OK + (4 if name == "labels" else 2)
            assert fn(ctypes.byref(small), *vals, None) == -1
            assert _named(lib, name, 8 if name == "labels" else 4), (name, lib.stgcn_last_error())
    assert lib.stgcn_eval_metrics_reset(_OK + 4, 10, None) == -1
    assert _named(lib, "metrics", 8)
    # Adam: the table at 8 bytes, its tensors at 4 (views into a flat bucket pass)
    f64 = [ctypes.c_double(v) for v in (1e-3, 0.9, 0.999, 1e-8, 0.0)]
    assert lib.stgcn_adam_step(_OK + 4, 1, 1, *f64, 1, None) == -1
    assert _named(lib, "dev_table", 8)
    assert lib.stgcn_adam_step_dev(_OK + 4, 1, 1, *f64, _OK, None) == -1
    assert _named(lib, "dev_table", 8)
    assert lib.stgcn_adam_step_dev(_OK, 1, 1, *f64, _OK + 2, None) == -1
    assert _named(lib, "step", 4)
    nbytes = lib.stgcn_adam_table_bytes(2)
    host = (ctypes.c_char * nbytes)()
    chunks = ctypes.c_int64(0)
    ok = (hl.AdamTensor * 2)(hl.AdamTensor(_OK + 12, _OK + 4, _OK + 8, _OK, 1875),
                             hl.AdamTensor(_OK + 4, _OK + 12, _OK + 4, _OK + 8, 5000))
    assert lib.stgcn_adam_build_table(ok, 2, host, nbytes, ctypes.byref(chunks)) == 0
    assert chunks.value == 1 + 3
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        t = hl.AdamTensor(_OK, _OK, _OK, _OK, 64)
        setattr(t, field, _OK + 2)
        bad = (hl.AdamTensor * 2)(ok[0], t)
        assert lib.stgcn_adam_build_table(bad, 2, host, nbytes, ctypes.byref(chunks)) == -1
        assert b"tensor 1" in lib.stgcn_last_error() and b"4-byte aligned" in lib.stgcn_last_error()
