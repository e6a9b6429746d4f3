"""The evaluation step's host side (no GPU): the feature mask, the metrics
block's size, argument checks of stgcn_head_eval, the STGCN_PLAN_X_FROM_U_EVAL
plan table and the decoding of a metrics block."""
import ctypes
import struct

import pytest
import torch


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.hip_lib.load_library()


def _desc(pkg, **kw):
    # (the defaults of test_capi._desc)
    base = dict(N=128, C_in=64, C_out=64, T=300, T_out=300, V=18, K=1, gamma=9, stride=1,
                pad=4, eps=1e-5, momentum=0.1, training=1, need_dx=1, flags=0)
    base.update(kw)
    return pkg.hip_lib.Desc(**base)


def test_features_and_abi(pkg, lib):
    hl = pkg.hip_lib
    assert lib.stgcn_features() & hl.FEATURE_EVAL_CHAIN == hl.FEATURE_EVAL_CHAIN == 1
    assert lib.stgcn_features() & hl.FEATURE_EVAL_HEAD == hl.FEATURE_EVAL_HEAD == 2
    assert lib.stgcn_abi_version() == hl.ABI_VERSION == 11


def test_metrics_bytes(lib):
    assert lib.stgcn_eval_metrics_bytes(10) == 64 + 800
    assert lib.stgcn_eval_metrics_bytes(400) == 64 + 8 * 400 * 400
    assert lib.stgcn_eval_metrics_bytes(0) == 0
    assert lib.stgcn_eval_metrics_bytes(-3) == 0
    assert lib.stgcn_eval_metrics_reset(None, 10, None) == -1


def test_head_eval_rejects_without_touching_gpu(pkg, lib):
    hl = pkg.hip_lib
    one = ctypes.c_void_p(256)
    d = hl.EvalDesc(4, 64, 54, 10, 1)
    assert lib.stgcn_head_eval(ctypes.byref(d), *([None] * 10), None) == -1
    assert b"null" in lib.stgcn_last_error()
    assert lib.stgcn_head_eval_u(ctypes.byref(d), *([None] * 13), None) == -1
    assert b"null" in lib.stgcn_last_error()
    # the U form with its BN2 arguments missing
    assert lib.stgcn_head_eval_u(ctypes.byref(d), one, None, None, None, *([one] * 8), None,
                                 None) == -1
    assert b"null" in lib.stgcn_last_error()
    assert lib.stgcn_head_eval(None, *([one] * 9), None, None) == -1
    for topk in (0, 11, -1):
        d = hl.EvalDesc(4, 64, 54, 10, topk)
        assert lib.stgcn_head_eval(ctypes.byref(d), *([one] * 9), None, None) == -1, topk
        assert b"topk" in lib.stgcn_last_error()
        assert lib.stgcn_head_eval_u(ctypes.byref(d), *([one] * 12), None, None) == -1, topk
        assert b"topk" in lib.stgcn_last_error()


def test_eval_plan_table(pkg):
    hl = pkg.hip_lib
    plan = lambda **kw: hl.block_plan(_desc(pkg, **kw))  # noqa: E731
    for kw in (dict(flags=12), dict(flags=4),
               dict(flags=12, C_in=128, C_out=256, stride=2, T=150, T_out=75),
               dict(flags=2, V=25, K=3), dict(flags=2, V=50, K=3)):
        assert plan(training=0, **kw) & hl.PLAN_X_FROM_U_EVAL, kw
        assert not plan(training=1, **kw) & hl.PLAN_X_FROM_U_EVAL, kw
        # PLAN_X_FROM_U itself is the training bit
        assert not plan(training=0, **kw) & hl.PLAN_X_FROM_U, kw
    for kw in (dict(flags=0), dict(flags=13), dict(flags=28), dict(flags=12, C_in=3),
               dict(flags=12, T=21, T_out=21)):   # 64 * 21 is not a multiple of 256
        assert not plan(training=0, **kw) & hl.PLAN_X_FROM_U_EVAL, kw
        assert not plan(training=1, **kw) & hl.PLAN_X_FROM_U_EVAL, kw
        assert not plan(training=0, **kw) & hl.PLAN_X_FROM_U, kw
    # no backward condition: the default graph (V = 25, K = 1) chains in eval only
    assert plan(training=0, flags=12, V=25, K=1) & hl.PLAN_X_FROM_U_EVAL
    assert not plan(training=1, flags=12, V=25, K=1) & hl.PLAN_X_FROM_U


def test_eval_prev_u_needs_the_plan(pkg, lib):
    """An eval forward with prev_U on a block without the plan bit, and one with
    y null but y_stats given, fail before any launch."""
    hl = pkg.hip_lib
    one = ctypes.c_void_p(256)
    d = _desc(pkg, flags=0, training=0)
    a = hl.FwdArgs(*([one] * 18))
    a.x = None
    a.prev_U = a.prev_stats = a.prev_g2 = a.prev_b2 = one
    assert lib.stgcn_block_fwd(ctypes.byref(d), ctypes.byref(a), None, 0, None) == -1
    assert b"prev_U" in lib.stgcn_last_error()
    d = _desc(pkg, flags=12, training=0)
    a = hl.FwdArgs(*([one] * 18))
    a.y = None
    a.y_stats = one
    assert lib.stgcn_block_fwd(ctypes.byref(d), ctypes.byref(a), None, 0, None) == -1
    assert b"null" in lib.stgcn_last_error()
    # with the bit, prev_U without x_stats passes the argument checks (it stops
    # at the missing workspace); a residual block still needs y
    a = hl.FwdArgs(*([one] * 18))
    a.x = a.y = None
    a.prev_U = a.prev_stats = a.prev_g2 = a.prev_b2 = one
    assert lib.stgcn_block_fwd(ctypes.byref(d), ctypes.byref(a), None, 0, None) == -1
    assert b"workspace" in lib.stgcn_last_error()
    d = _desc(pkg, flags=13, training=0)
    a = hl.FwdArgs(*([one] * 21))
    a.y = None
    assert lib.stgcn_block_fwd(ctypes.byref(d), ctypes.byref(a), None, 0, None) == -1
    assert b"null" in lib.stgcn_last_error()


def test_decode_eval_metrics(pkg):
    """3 classes, two batches of 4 and 3 clips, one invalid label in the second."""
    classes = 3
    # batch 1: labels 0 1 2 2, preds 0 1 2 0; losses .5 .25 1. 2.  (3 correct)
    # batch 2: labels 1 -1 0, preds 2 . 0; losses 3. (ignored) .5  (1 of 2 correct)
    l1, l2 = [0.5, 0.25, 1.0, 2.0], [3.0, 0.5]
    conf = [[0] * 3 for _ in range(3)]
    for y, p in ((0, 0), (1, 1), (2, 2), (2, 0), (1, 2), (0, 0)):
        conf[y][p] += 1
    topk_hits = 5
    words = struct.pack("<5q3d", 2, 6, 4, topk_hits, 1, sum(l1) + sum(l2),
                        sum(l1) / 4 + sum(l2) / 2, 3 / 4 + 1 / 2)
    raw = words + struct.pack("<9q", *[c for row in conf for c in row])
    buf = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    r = pkg.train_ops.decode_eval_metrics(buf, classes)
    assert (r["batches"], r["clips"], r["invalid"], r["correct"], r["topk_hits"]) == (2, 6, 1, 4, 5)
    assert r["loss"] == (sum(l1) + sum(l2)) / 6
    assert r["acc"] == 4 / 6 and r["topk_acc"] == 5 / 6
    assert r["val_loss"] == (sum(l1) / 4 + sum(l2) / 2) / 2
    assert r["val_acc"] == (3 / 4 + 1 / 2) / 2
    assert r["val_loss"] != r["loss"] and r["val_acc"] != r["acc"]
    assert r["confusion"].dtype == torch.int64 and r["confusion"].tolist() == conf
    # an empty block decodes to zeros, not to a division by zero
    z = pkg.train_ops.decode_eval_metrics(torch.zeros(64 + 72, dtype=torch.uint8), classes)
    assert z["loss"] == z["val_acc"] == 0.0 and not z["confusion"].any()
    with pytest.raises(ValueError):
        pkg.train_ops.decode_eval_metrics(buf[:-8], classes)
