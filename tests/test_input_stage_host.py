"""STGCN_FEATURE_INPUT_STAGE without a GPU: the feature bit, the two structs,
stgcn_input_check's verdicts and messages, and the host half of the stage
(data.pack_clips, data.clip_transforms)."""
import ctypes
import random

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.hip_lib.load_library()


def _desc(pkg, **kw):
    base = dict(N=3, C=2, T_out=11, V=25, C_src=3, src_f64=0, src_frames=33)
    base.update(kw)
    return pkg.hip_lib.InputDesc(**base)


def test_feature_bit_exports_and_abi(pkg, lib):
    for name in ("stgcn_input_check", "stgcn_input_stage"):
        assert hasattr(lib, name), name
        assert name in pkg.hip_lib.EXPORTED
    assert lib.stgcn_features() & 8 == pkg.hip_lib.FEATURE_INPUT_STAGE == 8
    assert lib.stgcn_features() & 7 == 7  # (bits 1, 2 and 4 stay)
    assert lib.stgcn_abi_version() == pkg.hip_lib.ABI_VERSION == 11


def test_struct_sizes(pkg):
    hl = pkg.hip_lib
    assert ctypes.sizeof(hl.InputDesc) == 32
    assert ctypes.sizeof(hl.Clip) == 48
    dt = pkg.data.CLIP_DTYPE
    assert dt.itemsize == 48
    for name in ("first_frame", "frames", "flags", "m"):
        assert dt.fields[name][1] == getattr(hl.Clip, name).offset, name


@pytest.mark.parametrize("shape", [(3, 2, 11, 25, 3), (128, 3, 300, 18, 3), (8, 2, 300, 50, 2)])
@pytest.mark.parametrize("f64", [0, 1])
def test_input_check_accepts(pkg, lib, shape, f64):
    N, C, T_out, V, C_src = shape
    d = _desc(pkg, N=N, C=C, T_out=T_out, V=V, C_src=C_src, src_f64=f64, src_frames=N * T_out)
    assert lib.stgcn_input_check(ctypes.byref(d)) == 0, lib.stgcn_last_error()


@pytest.mark.parametrize("kw,field", [
    (dict(C=3, C_src=2), b"C_src"), (dict(C=1), b"C "), (dict(C=0), b"C "),
    (dict(C_src=5), b"C_src"), (dict(C=5, C_src=5), b"C_src"),
    (dict(N=0), b"N "), (dict(N=-1), b"N "), (dict(T_out=0), b"T_out"), (dict(T_out=-3), b"T_out"),
    (dict(V=0), b"V "), (dict(V=-25), b"V "), (dict(src_frames=0), b"src_frames"),
    (dict(src_frames=-1), b"src_frames"), (dict(src_f64=2), b"src_f64"),
    (dict(src_f64=-1), b"src_f64")])
def test_input_check_rejects_naming_the_field(pkg, lib, kw, field):
    d = _desc(pkg, **kw)
    assert lib.stgcn_input_check(ctypes.byref(d)) == -1, kw
    msg = lib.stgcn_last_error()
    assert msg.startswith(b"input: ") and field in msg, (kw, msg)


def test_input_stage_checks_arguments_before_any_launch(pkg, lib):
    """Fake pointers, no GPU touched: every call stops at an argument check."""
    ok = ctypes.c_void_p(256)
    d = _desc(pkg)
    call = lambda **p: lib.stgcn_input_stage(  # noqa: E731
        ctypes.byref(d), p.get("src", ok), p.get("clips", ok), p.get("x", ok),
        p.get("status", ok), None)
    for name in ("src", "clips", "x", "status"):
        assert call(**{name: None}) == -1
        assert b"null" in lib.stgcn_last_error()
    for off in (4, 8, 12):
        assert call(x=ctypes.c_void_p(256 + off)) == -1
        assert b"x: must be 16-byte aligned" in lib.stgcn_last_error()
    assert call(src=ctypes.c_void_p(258)) == -1
    assert b"src: must be 4-byte aligned" in lib.stgcn_last_error()
    assert call(clips=ctypes.c_void_p(260)) == -1
    assert b"clips: must be 8-byte aligned" in lib.stgcn_last_error()
    assert call(status=ctypes.c_void_p(258)) == -1
    assert b"status: must be 4-byte aligned" in lib.stgcn_last_error()
    d = _desc(pkg, src_f64=1)
    assert call(src=ctypes.c_void_p(260)) == -1
    assert b"src: must be 8-byte aligned" in lib.stgcn_last_error()
    d = _desc(pkg, C=1)
    assert call() == -1 and b"input: C " in lib.stgcn_last_error()


def _items(rng, lengths, V, C_src, dtype=np.float64, lead=False):
    out = []
    for i, t in enumerate(lengths):
        clip = (rng.standard_normal((t, V, C_src)) * 40 + 100).astype(dtype)
        out.append((clip[None] if lead else clip, np.array([i % 6])))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("lead", [False, True])
def test_pack_clips_layout(pkg, dtype, lead):
    rng = np.random.default_rng(0)
    lengths, T_out, V, C_src = (1, 7, 13, 11), 11, 25, 3
    items = _items(rng, lengths, V, C_src, dtype, lead)
    buf, table, labels = pkg.data.pack_clips(items, T_out, C_src, dtype)
    kept = [min(t, T_out) for t in lengths]
    assert buf.dtype == dtype and buf.shape == (sum(kept), V, C_src)
    assert table.dtype == pkg.data.CLIP_DTYPE and table.shape == (4,)
    assert table["frames"].tolist() == kept                       # 13 truncated to 11
    assert table["first_frame"].tolist() == [0, 1, 8, 19]         # contiguous, item order
    for (clip, _), first, f in zip(items, table["first_frame"], table["frames"]):
        clip = clip[0] if lead else clip
        assert np.array_equal(buf[first:first + f], clip[:f])
    assert not table["flags"].any()
    assert np.array_equal(table["m"], np.tile([1.0, 0.0, 0.0, 1.0], (4, 1)))
    assert labels.dtype == np.int64 and labels.tolist() == [0, 1, 2, 3]


def test_pack_clips_transforms_and_out(pkg):
    rng = np.random.default_rng(1)
    items = _items(rng, (5, 3, 9), 18, 2)
    tr = np.tile(np.eye(3), (3, 1, 1))
    tr[1] = [[0.5, 2.0, 0.0], [-3.0, 4.0, 0.0], [5.0, 5.0, 1.0]]
    out = np.full(3 * 6 * 18 * 2 + 7, -1.0)
    buf, table, _ = pkg.data.pack_clips(items, 6, 2, np.float64, out=out, transforms=tr)
    assert table["flags"].tolist() == [0, 1, 0]       # identities: the plain cast
    assert table["m"][1].tolist() == [0.5, 2.0, -3.0, 4.0]
    assert table["frames"].tolist() == [5, 3, 6]
    assert np.shares_memory(buf, out) and buf.shape == (14, 18, 2)
    assert np.array_equal(out[:buf.size], buf.reshape(-1)) and np.all(out[buf.size:] == -1.0)
    # (N, 2, 2) matrices; a pinned-style torch tensor as out
    import torch
    tout = torch.empty(3 * 6 * 18 * 2, dtype=torch.float32)
    buf, table, _ = pkg.data.pack_clips([(c.astype(np.float32), y) for c, y in items], 6, 2,
                                        torch.float32, out=tout, transforms=tr[:, :2, :2])
    assert table["flags"].tolist() == [0, 1, 0] and np.shares_memory(buf, tout.numpy())
    with pytest.raises(ValueError, match="out holds"):
        pkg.data.pack_clips(items, 6, 2, np.float64, out=np.empty(10))
    with pytest.raises(ValueError, match="float32 or float64"):
        pkg.data.pack_clips(items, 6, 2, np.int32)
    with pytest.raises(ValueError, match="a clip is"):
        pkg.data.pack_clips(items, 6, 3, np.float64)


@pytest.mark.parametrize("seed", range(4))
def test_clip_transforms_draw_order(pkg, seed):
    """Coin, then the matrix, clip by clip: KTHDataset.__getitem__'s
    random.randint(0, 1) followed by augment_data's draws from np.random."""
    n = 9
    random.seed(seed)
    np.random.seed(seed)
    got = pkg.data.clip_transforms(n)
    random.seed(seed)
    np.random.seed(seed)
    want = []
    for _ in range(n):
        want.append(pkg.data.augmentation_matrix() if random.randint(0, 1) else np.eye(3))
    assert got.dtype == np.float64 and got.shape == (n, 3, 3)
    assert np.array_equal(got, np.asarray(want))


def test_clip_transforms_without_augmentation_draws_nothing(pkg):
    random.seed(5)
    np.random.seed(5)
    s_py, s_np = random.getstate(), np.random.get_state()
    got = pkg.data.clip_transforms(6, augment=False)
    assert np.array_equal(got, np.tile(np.eye(3), (6, 1, 1)))
    assert random.getstate() == s_py
    after = np.random.get_state()
    assert after[0] == s_np[0] and np.array_equal(after[1], s_np[1]) and after[2:] == s_np[2:]
