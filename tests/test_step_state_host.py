"""STGCN_FEATURE_STEP_STATE without a GPU: the new entry points exist, their
argument checks name what they refuse before any launch, and the host
restatement of the dropout mask (fused.dropout_mask) has the statistics the
device-seed derivation needs: seed' = mix64(seed + c * PHI) decorrelates
consecutive step tokens, which a plain seed + c * PHI would not."""
import ctypes

import numpy as np
import pytest

NEW = ("stgcn_block_fwd_dseed", "stgcn_block_bwd_dseed", "stgcn_seed_next",
       "stgcn_adam_step_dev2", "stgcn_grad_norm")
SEEDS = (0, 1, 12345, 2 ** 61 + 7)
NEL, P = 4096, 0.5
# 6 sigma of the mean of 4096 fair coin flips: 6 * 0.5 / sqrt(4096)
BOUND = 0.047


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.hip_lib.load_library()


def _desc(pkg, **kw):
    base = dict(N=2, C_in=64, C_out=64, T=40, T_out=40, V=18, K=1, gamma=9, stride=1,
                pad=4, eps=1e-5, momentum=0.1, training=1, need_dx=1, flags=0)
    base.update(kw)
    return pkg.hip_lib.Desc(**base)


def test_exports_feature_bit_and_abi(pkg, lib):
    for name in NEW + ("stgcn_grad_norm_bytes",):
        assert hasattr(lib, name), name
        assert name in pkg.hip_lib.EXPORTED
    assert lib.stgcn_features() & 4 == pkg.hip_lib.FEATURE_STEP_STATE == 4
    assert lib.stgcn_features() & 3 == 3  # (the earlier bits stay)
    assert lib.stgcn_abi_version() == pkg.hip_lib.ABI_VERSION == 11
    assert lib.stgcn_grad_norm_bytes(5) == 40
    assert lib.stgcn_grad_norm_bytes(0) == 0


def test_args_struct_sizes_unchanged(pkg):
    """ABI 11 pins the argument blocks: the device seed is a call argument."""
    vp = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(pkg.hip_lib.FwdArgs) == 24 * vp + 16 + 5 * vp
    assert ctypes.sizeof(pkg.hip_lib.BwdArgs) == 33 * vp + 16 + 8 * vp


def test_seed_next_refuses_null_and_misaligned(lib):
    ok = ctypes.c_void_p(256)
    assert lib.stgcn_seed_next(None, ok, None) == -1
    assert b"counter" in lib.stgcn_last_error()
    assert lib.stgcn_seed_next(ok, None, None) == -1
    assert b"token" in lib.stgcn_last_error()
    assert lib.stgcn_seed_next(ctypes.c_void_p(260), ok, None) == -1
    assert b"counter" in lib.stgcn_last_error() and b"8-byte" in lib.stgcn_last_error()
    assert lib.stgcn_seed_next(ok, ctypes.c_void_p(260), None) == -1
    assert b"token" in lib.stgcn_last_error() and b"8-byte" in lib.stgcn_last_error()


def test_block_dseed_refuses_misaligned_seed_dev(pkg, lib):
    d = _desc(pkg)
    fa = pkg.hip_lib.FwdArgs(*([ctypes.c_void_p(256)] * 18))
    ba = pkg.hip_lib.BwdArgs(*([ctypes.c_void_p(256)] * 23))
    for off in (4, 2, 1):
        bad = ctypes.c_void_p(256 + off)
        assert lib.stgcn_block_fwd_dseed(ctypes.byref(d), ctypes.byref(fa), bad, None, 0,
                                         None) == -1
        assert b"seed_dev" in lib.stgcn_last_error()
        assert lib.stgcn_block_bwd_dseed(ctypes.byref(d), ctypes.byref(ba), bad, None, 0,
                                         None) == -1
        assert b"seed_dev" in lib.stgcn_last_error()
    # an aligned seed_dev passes that check: the call then stops at its workspace
    good = ctypes.c_void_p(264)
    assert lib.stgcn_block_fwd_dseed(ctypes.byref(d), ctypes.byref(fa), good, None, 0, None) == -1
    assert b"seed_dev" not in lib.stgcn_last_error()
    # null arguments are refused as by the calls without a seed
    empty = pkg.hip_lib.FwdArgs()
    assert lib.stgcn_block_fwd_dseed(ctypes.byref(d), ctypes.byref(empty), None, None, 0,
                                     None) == -1
    assert b"null" in lib.stgcn_last_error()


def test_adam_dev2_and_grad_norm_refuse_bad_arguments(lib):
    ok = ctypes.c_void_p(256)
    hp = (0.9, 0.999, 1e-8, 0.0)
    assert lib.stgcn_adam_step_dev2(ok, 1, 1, None, None, *hp, ok, None) == -1
    assert b"lr_dev" in lib.stgcn_last_error()
    assert lib.stgcn_adam_step_dev2(ok, 1, 1, ctypes.c_void_p(258), None, *hp, ok, None) == -1
    assert b"lr_dev" in lib.stgcn_last_error()
    assert lib.stgcn_adam_step_dev2(ok, 1, 1, ok, ctypes.c_void_p(258), *hp, ok, None) == -1
    assert b"grad_coef" in lib.stgcn_last_error()
    assert lib.stgcn_adam_step_dev2(ok, 1, 1, ok, None, *hp, None, None) == -1
    assert b"step" in lib.stgcn_last_error()
    assert lib.stgcn_grad_norm(ok, 1, 1, 1.0, None, ok, ok, None) == -1
    assert b"partials" in lib.stgcn_last_error()
    assert lib.stgcn_grad_norm(ok, 1, 1, 1.0, ok, None, ok, None) == -1
    assert b"norm_out" in lib.stgcn_last_error()
    assert lib.stgcn_grad_norm(ok, 1, 1, 1.0, ok, ok, None, None) == -1
    assert b"coef_out" in lib.stgcn_last_error()
    assert lib.stgcn_grad_norm(ok, 1, 1, 0.0, ok, ok, ok, None) == -1
    assert b"max_norm" in lib.stgcn_last_error()
    assert lib.stgcn_grad_norm(ok, 1, 1, 1.0, ctypes.c_void_p(260), ok, ok, None) == -1
    assert b"partials" in lib.stgcn_last_error()


def _keep_mask(seed, shape, p):
    """tests/test_gpu_block.py's statement of the mask with a by-value seed."""
    e = np.arange(int(np.prod(shape)), dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + e * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    thresh = min(int(p * 2.0 ** 32), 2 ** 32 - 1)
    return ((z >> np.uint64(32)) >= np.uint64(thresh)).reshape(shape)


@pytest.mark.parametrize("p", [0.5, 0.2, 0.9])
def test_mask_without_counter_is_the_by_value_formula(pkg, p):
    for seed in SEEDS + (2 ** 62 - 1,):
        got = pkg.fused.dropout_mask(seed, (3, 5, 7, 18), p)
        assert got.dtype == np.bool_ and got.shape == (3, 5, 7, 18)
        assert np.array_equal(got, _keep_mask(seed, (3, 5, 7, 18), p))


def test_counter_enters_through_mix64(pkg):
    """seed' = mix64(seed + c * PHI): the mask with a counter is the by-value mask
    of seed' (computed here in plain Python integers)."""
    M = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    for seed in SEEDS:
        for c in (0, 1, 5, 2 ** 40):
            eff = mix((seed + c * 0x9E3779B97F4A7C15) & M)
            assert np.array_equal(pkg.fused.dropout_mask(seed, (NEL,), P, counter=c),
                                  _keep_mask(eff, (NEL,), P))
    # (counter 0 is not "no counter": the hash still applies)
    assert not np.array_equal(pkg.fused.dropout_mask(7, (NEL,), P, counter=0),
                              pkg.fused.dropout_mask(7, (NEL,), P))


def test_counter_mask_statistics(pkg):
    rates, agree, shifted = [], [], []
    for seed in SEEDS:
        masks = [pkg.fused.dropout_mask(seed, (NEL,), P, counter=c) for c in range(4)]
        rates += [m.mean() for m in masks]
        for a, b in zip(masks, masks[1:]):
            agree.append((a == b).mean())
            shifted.append((b[:-1] == a[1:]).mean())
    print("keep rates", min(rates), max(rates), "agreement", min(agree), max(agree),
          "shifted agreement", min(shifted), max(shifted))
    assert all(abs(r - 0.5) < BOUND for r in rates), rates
    assert all(abs(a - 0.5) < BOUND for a in agree), agree
    assert all(s < 0.5 + BOUND for s in shifted), shifted


def test_plain_counter_sum_would_shift_the_mask():
    """Why the hash is there: with seed + c * PHI, step c + 1's mask is step c's
    shifted by one element."""
    for seed in SEEDS:
        with np.errstate(over="ignore"):
            a = _keep_mask(np.uint64(seed), (NEL,), P)
            b = _keep_mask(np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15), (NEL,), P)
        assert np.array_equal(b[:-1], a[1:])


def test_stack_device_seed_keeps_the_state_dict(pkg):
    """dropout_seed="device": same parameters and state_dict keys as "host" under
    the same torch.manual_seed; the counter is a non-persistent buffer; one salt
    per block, reproduced by the seed."""
    import contextlib
    import io

    import torch
    A = torch.ones(1, 18, 18) / 18

    def make(mode, seed=3):
        torch.manual_seed(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            return pkg.STGCNStack(3, 10, A, dropout_rate=0.5, dropout_seed=mode)

    host, dev, dev2, dev3 = make("host"), make("device"), make("device"), make("device", 4)
    assert list(host.state_dict()) == list(dev.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(host.state_dict().values(),
                                                 dev.state_dict().values()))
    assert "drop_counter" in dict(dev.named_buffers()) and dev.drop_counter.dtype == torch.int64
    assert "drop_counter" not in dict(host.named_buffers())
    salts = [b.drop_salt for b in dev.conv]
    assert len(set(salts)) == 10 and all(0 <= s < 2 ** 62 for s in salts)
    assert salts == [b.drop_salt for b in dev2.conv]
    assert salts != [b.drop_salt for b in dev3.conv]
    assert all(b.drop_salt is None for b in host.conv)
    with pytest.raises(ValueError, match="dropout_seed"):
        pkg.STGCNStack(3, 10, A, dropout_seed="gpu")
