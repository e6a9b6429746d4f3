"""STGCN_FEATURE_OPTIMIZERS without a GPU: the feature bit and the exports, every
refusal of the stgcn_opt_* calls by its message, the table's chunk prefix sums,
and the constructor checks of FusedAdam / FusedAdamW."""
import ctypes

import numpy as np
import pytest
import torch

NEW = ("stgcn_opt_check", "stgcn_opt_table_bytes", "stgcn_opt_build_table", "stgcn_opt_step")
OK = 256


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.hip_lib.load_library()


def _adam(pkg, **kw):
    base = dict(algo=pkg.hip_lib.OPT_ADAM, flags=0, lr=1e-3, beta1=0.9, beta2=0.999,
                eps=1e-8, weight_decay=0.0, step=1)
    base.update(kw)
    return pkg.hip_lib.OptDesc(**base)


def test_exports_feature_bit_and_abi(pkg, lib):
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in pkg.hip_lib.EXPORTED
    assert lib.stgcn_features() & 16 == pkg.hip_lib.FEATURE_OPTIMIZERS == 16
    assert lib.stgcn_features() & 15 == 15  # (the earlier bits stay)
    assert lib.stgcn_abi_version() == pkg.hip_lib.ABI_VERSION == 11
    assert ctypes.sizeof(pkg.hip_lib.OptTensor) == 56
    assert ctypes.sizeof(pkg.hip_lib.OptDesc) == 8 + 5 * 8 + 8 + 3 * ctypes.sizeof(ctypes.c_void_p)
    assert lib.stgcn_opt_table_bytes(3) == 3 * 56 + 4 * 8
    assert lib.stgcn_opt_table_bytes(0) == 0


def test_check_accepts(pkg, lib):
    hl = pkg.hip_lib
    for d in (_adam(pkg), _adam(pkg, flags=hl.OPT_AMSGRAD | hl.OPT_DECOUPLED_WD, weight_decay=0.1),
              _adam(pkg, lr=-1.0, lr_dev=OK + 4),  # (lr ignored with lr_dev)
              _adam(pkg, step=0, step_dev=OK + 12, lr_dev=OK, grad_coef=OK + 4)):
        assert lib.stgcn_opt_check(ctypes.byref(d)) == 0, lib.stgcn_last_error()


def test_check_refuses_by_name(pkg, lib):
    cases = [
        (_adam(pkg, algo=0), b"unknown algo"),
        (_adam(pkg, algo=2), b"unknown algo"),
        (_adam(pkg, algo=-1), b"unknown algo"),
        (_adam(pkg, flags=1), b"unknown flags"),
        (_adam(pkg, flags=8), b"unknown flags"),
        (_adam(pkg, lr=-1e-3), b"lr must"),
        (_adam(pkg, weight_decay=-0.01), b"weight_decay must"),
        (_adam(pkg, beta1=1.0), b"beta1"),
        (_adam(pkg, beta2=-0.1), b"beta2"),
        (_adam(pkg, eps=-1e-8), b"eps must"),
        (_adam(pkg, step=0), b"step must"),
        (_adam(pkg, lr_dev=OK + 2), b"lr_dev: must be 4-byte aligned"),
        (_adam(pkg, grad_coef=OK + 1), b"grad_coef: must be 4-byte aligned"),
        (_adam(pkg, step_dev=OK + 2), b"step_dev: must be 4-byte aligned"),
    ]
    for d, msg in cases:
        assert lib.stgcn_opt_check(ctypes.byref(d)) == -1, msg
        assert msg in lib.stgcn_last_error(), (msg, lib.stgcn_last_error())
    assert lib.stgcn_opt_check(None) == -1
    assert b"null descriptor" in lib.stgcn_last_error()
    # the step call checks its descriptor before anything else, without a launch
    for d, msg in cases[:5]:
        assert lib.stgcn_opt_step(ctypes.byref(d), OK, 1, 1, None) == -1
        assert msg in lib.stgcn_last_error()


def _build(pkg, lib, d, tensors):
    hl = pkg.hip_lib
    n = len(tensors)
    nbytes = lib.stgcn_opt_table_bytes(n)
    host = (ctypes.c_char * nbytes)()
    chunks = ctypes.c_int64(-1)
    arr = (hl.OptTensor * n)(*tensors)
    rc = lib.stgcn_opt_build_table(None if d is None else ctypes.byref(d), arr, n, host, nbytes,
                                   ctypes.byref(chunks))
    return rc, chunks.value, bytes(host)


def test_table_chunk_prefix_sums(pkg, lib):
    """numel 1, 2047, 2048, 2049, 5000: chunks of 2048 elements start at 0, 1, 2,
    3, 5 and there are 8 (the tensors placed off 16-byte alignment: accepted)."""
    hl = pkg.hip_lib
    numels = (1, 2047, 2048, 2049, 5000)
    tensors = [hl.OptTensor(OK + 4, OK + 8, OK + 12, OK + 4, None, n, 0, 0) for n in numels]
    rc, chunks, host = _build(pkg, lib, _adam(pkg), tensors)
    assert rc == 0, lib.stgcn_last_error()
    assert chunks == 8
    cs = np.frombuffer(host, dtype=np.int64, offset=len(numels) * 56)
    assert cs.tolist() == [0, 1, 2, 3, 5, 8]
    ent = np.frombuffer(host, dtype=np.int64, count=len(numels) * 7).reshape(-1, 7)
    assert ent[:, 5].tolist() == list(numels)
    assert ent[:, 0].tolist() == [OK + 4] * 5 and ent[:, 2].tolist() == [OK + 12] * 5
    assert ent[:, 4].tolist() == [0] * 5 and ent[:, 6].tolist() == [0] * 5


def test_table_refuses_by_name(pkg, lib):
    hl = pkg.hip_lib
    T = hl.OptTensor
    good = T(OK, OK, OK, OK, OK, 64, 0, 0)
    plain, ams = _adam(pkg), _adam(pkg, flags=hl.OPT_AMSGRAD)
    cases = [
        (plain, T(OK, OK, OK, None, None, 64, 0, 0), b"state slot s1"),
        (plain, T(OK, OK, None, OK, None, 64, 0, 0), b"state slot s0"),
        (ams, T(OK, OK, OK, OK, None, 64, 0, 0), b"state slot s2"),
        (plain, T(OK, OK, OK, OK, None, 0, 0, 0), b"numel <= 0"),
        (plain, T(OK, OK, OK, OK, None, -5, 0, 0), b"numel <= 0"),
        (plain, T(None, OK, OK, OK, None, 64, 0, 0), b"param or grad is null"),
        (plain, T(OK, None, OK, OK, None, 64, 0, 0), b"param or grad is null"),
        (plain, T(OK, OK, OK, OK, None, 64, 1, 0), b"unknown tensor flags"),
    ]
    for field in ("param", "grad", "s0", "s1", "s2"):
        t = T(OK, OK, OK, OK, OK, 64, 0, 0)
        setattr(t, field, OK + 2)
        cases.append((ams, t, b"4-byte aligned"))
    for d, bad, msg in cases:
        rc, _, _ = _build(pkg, lib, d, [good, bad])
        assert rc == -1, msg
        assert b"tensor 1" in lib.stgcn_last_error() and msg in lib.stgcn_last_error(), \
            (msg, lib.stgcn_last_error())
    # without AMSGrad the third slot is not asked for
    assert _build(pkg, lib, plain, [T(OK, OK, OK, OK, None, 64, 0, 0)])[0] == 0
    # a refused or missing descriptor refuses the build
    assert _build(pkg, lib, _adam(pkg, algo=7), [good])[0] == -1
    assert b"unknown algo" in lib.stgcn_last_error()
    assert _build(pkg, lib, None, [good])[0] == -1
    assert b"null descriptor" in lib.stgcn_last_error()
    # too small a buffer, no tensors
    arr = (T * 1)(good)
    chunks = ctypes.c_int64(0)
    host = (ctypes.c_char * 64)()
    assert lib.stgcn_opt_build_table(ctypes.byref(plain), arr, 1, host, 63,
                                     ctypes.byref(chunks)) == -1
    assert b"too small" in lib.stgcn_last_error()
    assert lib.stgcn_opt_build_table(ctypes.byref(plain), arr, 0, host, 64,
                                     ctypes.byref(chunks)) == -1
    assert b"no tensors" in lib.stgcn_last_error()


def test_step_refuses_bad_tables(pkg, lib):
    d = _adam(pkg)
    assert lib.stgcn_opt_step(ctypes.byref(d), OK + 4, 1, 1, None) == -1
    assert b"dev_table: must be 8-byte aligned" in lib.stgcn_last_error()
    for args in ((None, 1, 1), (OK, 0, 1), (OK, 1, 0), (OK, 1, 2 ** 31)):
        assert lib.stgcn_opt_step(ctypes.byref(d), *args, None) == -1
        assert b"bad table" in lib.stgcn_last_error()


def test_constructor_checks(pkg):
    p = [torch.zeros(4, requires_grad=True)]
    with pytest.raises(ValueError, match="positive"):
        pkg.FusedAdam(p, capturable=True, max_grad_norm=0.0)
    with pytest.raises(ValueError, match="positive"):
        pkg.FusedAdamW(p, capturable=True, max_grad_norm=-1.0)
    with pytest.raises(ValueError, match="capturable"):
        pkg.FusedAdamW(p, max_grad_norm=1.0)
    # the AMSGrad / AdamW switches are torch.optim.Adam's group keys
    a = pkg.FusedAdam(p, amsgrad=True)
    assert a.param_groups[0]["amsgrad"] is True
    assert a.param_groups[0]["decoupled_weight_decay"] is False
    d = pkg.FusedAdam(p)
    assert d.param_groups[0]["amsgrad"] is False
    assert d.param_groups[0]["decoupled_weight_decay"] is False
    w = pkg.FusedAdamW(p)
    assert w.param_groups[0]["decoupled_weight_decay"] is True
    assert w.param_groups[0]["weight_decay"] == 1e-2 and w.param_groups[0]["amsgrad"] is False
