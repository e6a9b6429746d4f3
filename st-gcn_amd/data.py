"""Host input pipeline for real skeleton data.

Mirrors of the reference's host-side data functions, bit-compatible with them
(checked against fixtures produced by the reference itself,
tests/golden/data_pipeline.npz):

  * ``pad_array_with_loops`` / ``loopy_pad_collate_fn``  src/data/util.py:12-47
  * ``augment_data``       src/data/augmentation.py:8-69 (same draws from
                           ``np.random``, in the same order)
  * ``load_clip``          the per-clip part of KTHDataset.__getitem__,
                           src/data/datasets.py:144-160 (.npy (T, 25, 3):
                           x, y, OpenPose confidence; the confidence dropped)
  * ``calculate_distances`` src/data/calculate_distances.py:7-48 (mean joint
                           distance to the per-frame centre of gravity: the
                           input of the spatial-configuration partitioning,
                           ``graph.get_normalized_adjacency_matrices(2, ...)``)

and what the reference leaves to Lightning: ``DeviceLoader`` turns collated
(N, T, V, C) float64 batches into the NCTV fp32 device layout the fused blocks
consume (the permute of lightning_model.py:101, done on the GPU), staging
through pinned host memory with the copy of batch i+1 in flight on a side
stream while batch i trains. Variable T is fine: the HIP blocks take any T.

Beside it, the same pipeline with the per-element work on the GPU
(``pack_clips`` / ``clip_transforms`` / ``stage_clips`` /
``RaggedDeviceLoader``): the host copies each ragged clip once into pinned
memory, one HIP kernel (csrc/input_stage.hip) loop-pads, applies a transform
drawn PER CLIP as the reference's dataset does (datasets.py:154), casts and
transposes to NCTV, into a tensor the caller may own (a GraphedStep's input).
On top of it ST-GCN's training augmentation, which the reference leaves as a
TODO (augmentation.py:48): ``clip_moves`` / ``apply_moves_reference`` ("random
moving": per-frame interpolated rotation, scale and translation, applied by
the same kernel) and ``pack_clips(crop="random")`` ("random choose"); and the
input views of the ST-GCN descendants, bone, joint motion and bone motion
beside the joints (``STREAMS`` / ``streams_reference`` / ``stage_clips(streams=)``
/ ``RaggedDeviceLoader(streams=)``), formed by that launch after the augmentation.
"""
import ctypes
import os
import random

import numpy as np
import torch

from . import graph, hip_lib


def pad_array_with_loops(x, target_len):
    """(N, T, V, C) -> (N, target_len, V, C) by repeating the clip from its
    start (np.pad 'wrap'); unchanged when already long enough
    (src/data/util.py:12-30)."""
    if x.shape[1] >= target_len:
        return x
    return np.pad(x, [(0, 0), (0, target_len - x.shape[1]), (0, 0), (0, 0)], mode="wrap")


def loopy_pad_collate_fn(batch):
    """[(x (1, T_i, V, C), label (1,)), ...] -> (xx (N, T*, V, C), labels (N,))
    with T* = max T_i, every clip loop-padded (src/data/util.py:33-47)."""
    max_len = max(x.shape[1] for x, _ in batch)
    xx = torch.cat([torch.from_numpy(pad_array_with_loops(x, max_len)) for x, _ in batch])
    labels = torch.cat([torch.from_numpy(np.asarray(y)) for _, y in batch])
    return xx, labels


_ROTATIONS = [15, -15, 5, -5, 10, -10]
_TRANSLATIONS = [[5, 5], [0, 5], [5, 0]]
_SCALES = [1.05, 1.1, 0.95]
_TRANSFORMS = ["rotation", "translation", "scaling", "flip"]


def augmentation_matrix(rng=np.random):
    """The random homogeneous 3x3 transform of augment_data
    (src/data/augmentation.py:15-45): two draws (with replacement) from
    {rotation, translation, scaling, flip}, then one parameter draw per chosen
    kind, composed in that fixed order. Consumes ``rng`` exactly as the
    reference consumes ``np.random``."""
    chosen = rng.choice(_TRANSFORMS, 2)
    T = np.eye(3)
    if "rotation" in chosen:
        theta = np.radians(rng.choice(_ROTATIONS))
        c, s = np.cos(theta), np.sin(theta)
        T = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]]).dot(T)
    if "translation" in chosen:
        tx, ty = _TRANSLATIONS[rng.choice(range(3))]
        T = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]]).dot(T)
    if "scaling" in chosen:
        f = rng.choice(_SCALES)
        T = np.array([[f, 0, 0], [0, f, 0], [0, 0, 1]]).dot(T)
    if "flip" in chosen:
        T = np.array([[-1, 0, 0], [0, 1, 0], [0, 0, 1]]).dot(T)
    return T


def augment_data(sequences, rng=np.random):
    """Apply one random transform to every (T, 25, 2) sequence of
    ``sequences`` (src/data/augmentation.py:8-69): homogeneous coordinates
    [x, y, 0] (the reference fills the third coordinate with 0, not 1, so
    translations do not move the points — kept as is) times the matrix from
    the right."""
    T = augmentation_matrix(rng)
    out = []
    for seq in sequences:
        n, v, d = seq.shape
        if v != 25:
            raise ValueError("augment_data: the reference's transform is for 25 joints")
        h = np.zeros((n, v, d + 1))
        h[:, :, :2] = np.copy(seq)
        h = np.reshape(h, (n * v, d + 1)).dot(T)
        out.append(np.reshape(h, (n, v, d + 1))[:, :, :2])
    return np.asarray(out)


def load_clip(path):
    """One clip of the KTH numpy format: (T, 25, 3) [x, y, confidence] ->
    (T, 25, 2) joint coordinates (datasets.py:144-160 with
    use_confidence_scores=False, the only supported mode there)."""
    seq = np.load(path, allow_pickle=False)
    return seq[:, :, :-1]


def _joint_distances(clip, V, acc, cnt):
    for t in range(clip.shape[0]):
        x, y = clip[t, :, 0], clip[t, :, 1]
        gx, gy = np.average(x), np.average(y)
        acc += np.sqrt((gx - clip[t, :V, 0]) ** 2 + (gy - clip[t, :V, 1]) ** 2)
        cnt += 1


def joint_distances(clips, V=25):
    """Mean distance of every joint to the per-frame centre of gravity over
    all frames of ``clips`` (iterable of (T, V, >=2) arrays), accumulated in
    the reference's order (clip by clip, frame by frame)."""
    acc, cnt = np.zeros(V), np.zeros(V)
    for c in clips:
        _joint_distances(c, V, acc, cnt)
    return acc / cnt


def calculate_distances(V=25, dataset_dir="../datasets/KTH_Action_Dataset",
                        output_file="../datasets/KTH_Action_Dataset/dist/distances.npy"):
    """File-level mirror of src/data/calculate_distances.py:7-48: every .npy
    clip of ``dataset_dir`` (os.listdir order, as the reference) -> saved
    (V,) distances; also returned."""
    files = [f for f in os.listdir(dataset_dir) if f.endswith(".npy") and f != output_file]
    d = joint_distances((np.load(os.path.join(dataset_dir, f), allow_pickle=False)
                         for f in files), V)
    np.save(output_file, d)
    return d


class DeviceLoader:
    """Iterate (x_nctv fp32 on ``device``, labels int64 on ``device``) from an
    iterable of collated (x (N, T, V, C), labels (N,)) CPU batches. Each batch
    is converted to fp32 into pinned memory, copied with non_blocking=True on
    a side stream one batch ahead, and permuted NTVC -> NCTV on the device
    (lightning_model.py:101)."""

    def __init__(self, batches, device):
        self.batches = batches
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(self.device)

    def _stage(self, item):
        x, y = item
        xh = torch.as_tensor(x).to(torch.float32).pin_memory()
        yh = torch.as_tensor(y).to(torch.int64).pin_memory()
        with torch.cuda.stream(self.stream):
            xd = xh.to(self.device, non_blocking=True)
            yd = yh.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return xd, yd, ev

    def __iter__(self):
        it = iter(self.batches)
        nxt = None
        try:
            nxt = self._stage(next(it))
        except StopIteration:
            return
        while nxt is not None:
            xd, yd, ev = nxt
            try:
                nxt = self._stage(next(it))
            except StopIteration:
                nxt = None
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            xd.record_stream(cur)
            yd.record_stream(cur)
            yield xd.permute(0, 3, 1, 2).contiguous(), yd


# ---------------------------------------------------------------------------
# The input stage on the device (stgcn_input_stage, hip_lib.FEATURE_INPUT_STAGE):
# the host only copies each clip's frames into pinned memory; the loop padding,
# the per-clip augmentation, the fp32 cast and the transpose to NCTV are one
# kernel (csrc/input_stage.hip).
# ---------------------------------------------------------------------------

# stgcn_clip_t (include/stgcn_hip.h), 48 bytes
CLIP_DTYPE = np.dtype([("first_frame", "<i8"), ("frames", "<i4"), ("flags", "<i4"),
                       ("m", "<f8", (4,))])
assert CLIP_DTYPE.itemsize == ctypes.sizeof(hip_lib.Clip) == 48


def clip_transforms(n, augment=True, rng=np.random, coin=random):
    """(n, 3, 3) float64: the transform of each of n clips as the reference's
    dataset draws it per item (KTHDataset.__getitem__, datasets.py:154): a coin
    ``coin.randint(0, 1)``, and on 1 one ``augmentation_matrix(rng)``; the
    identity on 0. Clip by clip, so ``coin`` and ``rng`` are consumed in the
    reference's order. augment=False: identities, nothing drawn."""
    out = np.tile(np.eye(3), (n, 1, 1))
    if augment:
        for i in range(n):
            if coin.randint(0, 1):
                out[i] = augmentation_matrix(rng)
    return out


# stgcn_move_t (include/stgcn_hip.h), 160 bytes: the "random moving" of ST-GCN's
# training recipe (feeder/tools.py random_move), one record per clip
MOVE_DTYPE = np.dtype({"names": ["nk", "frame", "angle", "scale", "tx", "ty"],
                       "formats": ["<i4", ("<i4", (4,))] + [("<f8", (4,))] * 4,
                       "offsets": [0, 4, 24, 56, 88, 120], "itemsize": 160})
assert MOVE_DTYPE.itemsize == ctypes.sizeof(hip_lib.Move) == 160
MOVE_ANGLES = (-10.0, -5.0, 0.0, 5.0, 10.0)   # degrees
MOVE_SCALES = (0.9, 1.0, 1.1)
MOVE_SHIFTS = (-0.2, -0.1, 0.0, 0.1, 0.2)


def clip_moves(n, T_out, rng=np.random, coin=random, angle_candidate=MOVE_ANGLES,
               scale_candidate=MOVE_SCALES, transform_candidate=MOVE_SHIFTS,
               move_time_candidate=(1,)):
    """(n,) MOVE_DTYPE: one random move per clip, drawn as ST-GCN's random_move
    draws it, clip by clip: ``coin.choice(move_time_candidate)`` segments with
    key nodes at ``arange(0, T_out, T_out / move_time).round()`` and at T_out
    (frames 0 and T_out by default), then ``rng.choice`` of one angle (degrees;
    stored in radians, ``* np.pi / 180``), one scale, one x and one y translation
    per node, in that order. At most 3 segments (4 nodes)."""
    out = np.zeros(n, dtype=MOVE_DTYPE)
    for i in range(n):
        move_time = coin.choice(move_time_candidate)
        node = np.append(np.arange(0, T_out, T_out * 1.0 / move_time).round().astype(int), T_out)
        k = len(node)
        if not 2 <= k <= 4 or np.any(np.diff(node) <= 0):
            raise ValueError(f"clip_moves: {move_time} segments over {T_out} frames give the "
                             f"nodes {node.tolist()}: 2 to 4 strictly increasing frames needed")
        out["nk"][i] = k
        out["frame"][i, :k] = node
        out["angle"][i, :k] = rng.choice(angle_candidate, k) * np.pi / 180
        out["scale"][i, :k] = rng.choice(scale_candidate, k)
        out["tx"][i, :k] = rng.choice(transform_candidate, k)
        out["ty"][i, :k] = rng.choice(transform_candidate, k)
    return out


def move_is_valid(mv, T_out):
    """What the kernel accepts of one MOVE_DTYPE record: nk = 0, or 2..4 nodes
    with frame[0] = 0, strictly increasing frames, the last at T_out - 1 or
    later, and finite parameters."""
    nk = int(mv["nk"])
    if nk == 0:
        return True
    if not 2 <= nk <= 4:
        return False
    f = mv["frame"][:nk].astype(np.int64)
    return bool(f[0] == 0 and np.all(np.diff(f) > 0) and f[-1] >= T_out - 1 and
                all(np.isfinite(mv[p][:nk]).all() for p in ("angle", "scale", "tx", "ty")))


def move_frame_affine(moves, T_out):
    """(N, 4, T_out) float64 [c, sn, tx, ty] of every frame, by the kernel's
    arithmetic: frame t in segment k (frame[k] <= t < frame[k + 1], the last
    frame in the last segment), every parameter p(t) = p_k + (t - f_k) *
    ((p_{k+1} - p_k) / (f_{k+1} - f_k)) (np.linspace's start + i * step), then
    c = cos(a) * s, sn = sin(a) * s. nk = 0 gives [1, 0, 0, 0]."""
    out = np.zeros((len(moves), 4, T_out))
    out[:, 0] = 1.0
    t = np.arange(T_out)
    for n, mv in enumerate(moves):
        nk = int(mv["nk"])
        if nk == 0:
            continue
        if not move_is_valid(mv, T_out):
            raise ValueError(f"move_frame_affine: record {n} is invalid for {T_out} frames")
        f = mv["frame"][:nk].astype(np.int64)
        k = np.clip(np.searchsorted(f, t, side="right") - 1, 0, nk - 2)
        i, span = (t - f[k]).astype(np.float64), (f[k + 1] - f[k]).astype(np.float64)
        a, s, tx, ty = (mv[p][k] + i * ((mv[p][k + 1] - mv[p][k]) / span)
                        for p in ("angle", "scale", "tx", "ty"))
        out[n] = np.cos(a) * s, np.sin(a) * s, tx, ty
    return out


def apply_moves_reference(x_ntvc, moves):
    """The move kernel's arithmetic in numpy float64 (the CPU yardstick of
    stgcn_input_stage_move): x_ntvc (N, T, V, C >= 2) -> float64 of that shape
    with x' = (c x - sn y) + tx, y' = (sn x + c y) + ty per frame
    (``move_frame_affine``), every operation rounded on its own; further channels
    and the clips with nk = 0 unchanged."""
    out = np.array(x_ntvc, dtype=np.float64)
    aff = move_frame_affine(moves, out.shape[1])
    for n, mv in enumerate(moves):
        if int(mv["nk"]) == 0:
            continue
        c, sn, tx, ty = (q[:, None] for q in aff[n])
        px, py = out[n, :, :, 0].copy(), out[n, :, :, 1].copy()
        out[n, :, :, 0] = (c * px - sn * py) + tx
        out[n, :, :, 1] = (sn * px + c * py) + ty
    return out


# STGCN_STREAM_* (include/stgcn_hip.h): the input views of the ST-GCN descendants
# (2s-AGCN, ST-GCN++, PYSKL), by the names their recipes use. Whatever the order
# they are asked for in, the channel groups of x come in bit order.
STREAMS = {"j": hip_lib.STREAM_JOINT, "b": hip_lib.STREAM_BONE,
           "jm": hip_lib.STREAM_JOINT_MOTION, "bm": hip_lib.STREAM_BONE_MOTION}
_BONE_STREAMS = hip_lib.STREAM_BONE | hip_lib.STREAM_BONE_MOTION


def parse_streams(streams):
    """The STGCN_STREAM_* mask of "j", "b", "jm", "bm", a "+"-joined combination
    ("j+b+jm+bm") or an iterable of those names; a mask passes through."""
    if isinstance(streams, (int, np.integer)) and not isinstance(streams, bool):
        if not 1 <= streams <= 15:
            raise ValueError(f"streams: the mask {streams} is not a non-empty subset of 1 | 2 | "
                             "4 | 8")
        return int(streams)
    names = streams.split("+") if isinstance(streams, str) else list(streams)
    mask = 0
    for name in names:
        if not isinstance(name, str) or name.strip() not in STREAMS:
            raise ValueError(f"streams: {name!r} is not one of {', '.join(STREAMS)}")
        mask |= STREAMS[name.strip()]
    if not mask:
        raise ValueError("streams: at least one of " + ", ".join(STREAMS))
    return mask


def stream_count(mask):
    """S: the number of streams of a mask (x has S * C channels)."""
    return bin(mask).count("1")


def streams_reference(j_nctv, parents, streams, score_channel=None):
    """The stream kernel's arithmetic in numpy float32 (the CPU yardstick of
    stgcn_input_stage_streams): the joint array J (N, C, T, V) float32 -> (N,
    S * C, T, V) float32, the selected streams in bit order. With p = parents[v]:
    bone B = J[.., v] - J[.., p]; joint motion J[t + 1] - J[t] and bone motion
    B[t + 1] - B[t], 0 in the last frame; on ``score_channel`` (a confidence)
    the mean (a + b) * 0.5 instead of each difference, the last frame of the
    motion streams 0 there too. Every operation is one float32 operation."""
    j = np.asarray(j_nctv)
    if j.dtype != np.float32 or j.ndim != 4:
        raise ValueError("streams_reference: J is an (N, C, T, V) float32 array")
    mask = parse_streams(streams)
    C, V = j.shape[1], j.shape[3]
    if score_channel is not None and not (score_channel == C - 1 and score_channel >= 2):
        raise ValueError(f"streams_reference: score_channel is None or C - 1 = {C - 1} (>= 2)")
    half = np.float32(0.5)

    def op(b, a):
        out = b - a
        if score_channel is not None:
            out[:, score_channel] = (b[:, score_channel] + a[:, score_channel]) * half
        return out

    def motion(a):
        out = np.zeros_like(a)
        out[:, :, :-1] = op(a[:, :, 1:], a[:, :, :-1])
        return out

    bone = None
    if mask & _BONE_STREAMS:
        par = np.asarray(parents)
        if par.shape != (V,) or ((par < 0) | (par >= V)).any():
            raise ValueError(f"streams_reference: parents holds {V} joints of [0, {V})")
        bone = op(j, j[:, :, :, par])
    parts = [(hip_lib.STREAM_JOINT, lambda: j), (hip_lib.STREAM_BONE, lambda: bone),
             (hip_lib.STREAM_JOINT_MOTION, lambda: motion(j)),
             (hip_lib.STREAM_BONE_MOTION, lambda: motion(bone))]
    return np.concatenate([f() for bit, f in parts if mask & bit], axis=1)


def _np_dtype(dtype):
    if isinstance(dtype, torch.dtype):
        dtype = {torch.float32: np.float32, torch.float64: np.float64}.get(dtype, dtype)
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"pack_clips: the source is float32 or float64, not {dtype}")
    return dtype


def pack_clips(items, T_out, C_src, dtype, out=None, transforms=None, crop="first",
               coin=random):
    """items: [(clip (T_i, V, C_src) or (1, T_i, V, C_src), label), ...] ->
    (staging (frames, V, C_src) of ``dtype``, table (N,) CLIP_DTYPE, labels (N,)
    int64). The first min(T_i, T_out) frames of every clip lie back to back in
    item order (the kernel repeats a short clip from its start, so nothing is
    padded here); table[i] says where clip i lies. transforms: (N, 3, 3) or
    (N, 2, 2) matrices (``clip_transforms``); an identity, or None, gives
    flags = 0 (the kernel's plain cast). out: a float array or CPU tensor of
    ``dtype`` to pack into (pinned memory, for an asynchronous copy) with room
    for the frames: N * T_out frames always suffice. Without it a new array.
    crop="random": a clip with T_i > T_out gives the T_out frames from
    ``coin.randint(0, T_i - T_out)`` on (ST-GCN's "random choose"), drawn clip by
    clip in item order; nothing is drawn for a clip that fits."""
    dtype = _np_dtype(dtype)
    if crop not in ("first", "random"):
        raise ValueError(f"pack_clips: crop is 'first' or 'random', not {crop!r}")
    clips = []
    for x, _ in items:
        x = np.asarray(x)
        if x.ndim == 4 and x.shape[0] == 1:
            x = x[0]
        if x.ndim != 3 or x.shape[2] != C_src or x.shape[0] < 1:
            raise ValueError(f"pack_clips: a clip is (T >= 1, V, {C_src}), got {x.shape}")
        clips.append(x)
    N = len(clips)
    if N == 0 or T_out < 1:
        raise ValueError("pack_clips: needs at least one clip and T_out >= 1")
    V = clips[0].shape[1]
    if any(c.shape[1] != V for c in clips):
        raise ValueError("pack_clips: the clips differ in their joint count")
    frames = [min(c.shape[0], T_out) for c in clips]
    total = sum(frames)
    if out is None:
        buf = np.empty((total, V, C_src), dtype=dtype)
    else:
        flat = out.numpy() if isinstance(out, torch.Tensor) else out
        if flat.dtype != dtype or not flat.flags["C_CONTIGUOUS"]:
            raise ValueError(f"pack_clips: out must be a contiguous {dtype} array")
        flat = flat.reshape(-1)
        if flat.size < total * V * C_src:
            raise ValueError(f"pack_clips: out holds {flat.size} elements, the batch needs "
                             f"{total * V * C_src}")
        buf = flat[:total * V * C_src].reshape(total, V, C_src)
    table = np.zeros(N, dtype=CLIP_DTYPE)
    table["m"] = (1.0, 0.0, 0.0, 1.0)
    first = 0
    for i, (c, f) in enumerate(zip(clips, frames)):
        start = coin.randint(0, c.shape[0] - f) if crop == "random" and c.shape[0] > f else 0
        buf[first:first + f] = c[start:start + f]
        table["first_frame"][i], table["frames"][i] = first, f
        first += f
    if transforms is not None:
        transforms = np.asarray(transforms, dtype=np.float64)
        if transforms.shape not in ((N, 3, 3), (N, 2, 2)):
            raise ValueError(f"pack_clips: transforms is (N, 3, 3) or (N, 2, 2), "
                             f"got {transforms.shape}")
        eye = np.eye(transforms.shape[1])
        for i, T in enumerate(transforms):
            if not np.array_equal(T, eye):
                table["flags"][i] = hip_lib.CLIP_APPLY
                table["m"][i] = T[:2, :2].reshape(4)
    labels = np.concatenate([np.asarray(y).reshape(-1) for _, y in items]).astype(np.int64)
    return buf, table, labels


def stage_clips(src, table, x, status, moves=None, streams=None, parents=None,
                score_channel=None):
    """One stgcn_input_stage launch on the current stream: src (frames, V,
    C_src) fp32 / fp64 on the device (its first dimension is the capacity the
    kernel checks the table against), table the device copy of a CLIP_DTYPE
    table (any dtype, N * 48 bytes), x (N, C, T_out, V) fp32 written in full,
    status (N,) int32 written in full: 1 where the clip's entry was invalid
    (that clip is zeros). The table is read when the kernel runs: inside a
    captured graph, rewrite src and the table between replays. Returns x.
    moves: the device copy of a MOVE_DTYPE table (any dtype, N * 160 bytes, read
    when the kernel runs like the clip table): the launch is
    stgcn_input_stage_move, which applies each clip's move after its matrix; an
    invalid record adds 2 to status[n] and zeros the clip.
    streams (``parse_streams``): the launch is stgcn_input_stage_streams and x is
    (N, S * C, T_out, V), the S selected streams of C channels each in bit order
    (joint, bone, joint motion, bone motion; ``streams_reference``). parents: a
    contiguous int32 tensor of V entries on x's GPU (``graph.parents``), needed
    with "b" or "bm" and read when the kernel runs; an entry outside [0, V) adds
    4 to every status[n] and zeros x. score_channel: None, or C - 1 >= 2, the
    confidence channel, averaged where the coordinates are subtracted."""
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous():
        raise ValueError("stage_clips: x is a contiguous (N, C, T_out, V) float32 tensor")
    N, C, T_out, V = x.shape
    mask = None
    if streams is None:
        if parents is not None or score_channel is not None:
            raise ValueError("stage_clips: parents and score_channel go with streams")
    else:
        mask = parse_streams(streams)
        S = stream_count(mask)
        if C % S:
            raise ValueError(f"stage_clips: x has {C} channels, not a multiple of the {S} "
                             "streams")
        C //= S
        # (a table is needed with a bone stream; one given without is checked all the
        # same and not passed on)
        if (parents is None and mask & _BONE_STREAMS) or (parents is not None and (
                parents.dtype != torch.int32 or parents.dim() != 1 or
                parents.numel() != V or not parents.is_contiguous() or
                parents.device != x.device)):
            raise ValueError(f"stage_clips: parents is a contiguous int32 tensor of {V} "
                             "entries on x's GPU")
    if src.dtype not in (torch.float32, torch.float64) or src.dim() != 3 or \
            not src.is_contiguous() or src.shape[1] != V:
        raise ValueError(f"stage_clips: src is a contiguous (frames, {V}, C_src) float32 or "
                         f"float64 tensor, got {tuple(src.shape)} {src.dtype}")
    if not table.is_contiguous() or table.numel() * table.element_size() < N * CLIP_DTYPE.itemsize:
        raise ValueError(f"stage_clips: the table needs {N * CLIP_DTYPE.itemsize} bytes")
    if status.dtype != torch.int32 or not status.is_contiguous() or status.numel() < N:
        raise ValueError(f"stage_clips: status is a contiguous int32 tensor of {N} elements")
    if not (src.device == table.device == x.device == status.device) or not x.is_cuda:
        raise ValueError("stage_clips: src, table, x and status live on one GPU")
    d = hip_lib.InputDesc(N, C, T_out, V, src.shape[2], int(src.dtype == torch.float64),
                          src.shape[0])
    if moves is None and mask is None:
        hip_lib.check(hip_lib.lib().stgcn_input_stage(
            ctypes.byref(d), hip_lib.ptr(src), hip_lib.ptr(table), hip_lib.ptr(x),
            hip_lib.ptr(status), hip_lib.stream_handle(x.device)))
        return x
    if moves is not None and (
            not moves.is_contiguous() or moves.device != x.device or
            moves.numel() * moves.element_size() < N * MOVE_DTYPE.itemsize):
        raise ValueError(f"stage_clips: moves needs {N * MOVE_DTYPE.itemsize} contiguous bytes "
                         "on x's GPU")
    if mask is not None:
        sd = hip_lib.StreamsDesc(d, mask, -1 if score_channel is None else int(score_channel))
        hip_lib.check(hip_lib.lib().stgcn_input_stage_streams(
            ctypes.byref(sd), hip_lib.ptr(src), hip_lib.ptr(table), hip_lib.ptr(moves),
            hip_lib.ptr(parents if mask & _BONE_STREAMS else None), hip_lib.ptr(x),
            hip_lib.ptr(status), hip_lib.stream_handle(x.device)))
        return x
    hip_lib.check(hip_lib.lib().stgcn_input_stage_move(
        ctypes.byref(d), hip_lib.ptr(src), hip_lib.ptr(table), hip_lib.ptr(moves), hip_lib.ptr(x),
        hip_lib.ptr(status), hip_lib.stream_handle(x.device)))
    return x


class _Slot:
    """One staging slot of RaggedDeviceLoader: pinned host and device buffers
    for the packed frames and the table, and the two events that order its
    reuse (``copied``: its H2D copies are done; ``free``: the stage kernel that
    read it is done)."""

    def __init__(self):
        self.host = self.dev = self.host_table = self.dev_table = None
        self.copied = self.free = None


class RaggedDeviceLoader:
    """Iterate (x (N, C, T_out, V) fp32 on ``device``, labels int64 on
    ``device``) from an iterable of batches of items [(clip (T_i, V, C_src),
    label), ...]. Per batch the host packs the clips into pinned memory
    (``pack_clips``) and the device pads, augments, casts and transposes
    (``stage_clips``). Two staging slots: the copies of batch i + 1 run on a
    side stream while batch i is consumed; the stage kernel waits for its
    slot's copies, and a slot's next copies wait for the kernel that read it.

    T_out=None: the longest clip of each batch (loopy_pad_collate_fn); a fixed
    T_out also truncates longer clips to their first T_out frames. augment:
    per-clip transforms by ``clip_transforms`` (np.random and random, in batch
    order). out / labels_out (with a fixed T_out): static tensors every batch is
    written into and that are yielded themselves, e.g. the inputs a GraphedStep
    captured; each batch then has out.shape[0] clips. An invalid table entry
    (there is none unless the packing is broken) raises once, after the last
    batch, from one host read.

    move=True: one random move per clip (``clip_moves`` over the batch's T_out,
    python's random and np.random) applied by the kernel after the clip's
    matrix (stgcn_input_stage_move); the records travel behind the clip table
    in the slot's table staging, under the same events. crop="random": a clip
    longer than T_out gives a random window instead of its first T_out frames
    (``pack_clips``). Per batch the draws are: the matrices, the moves, the
    window starts. An invalid move record is reported like an invalid table
    entry, once, after the last batch.

    streams (``parse_streams``, e.g. "j+b+jm+bm"): x has S * C channels, the S
    selected streams of the augmented and moved clip in bit order, from the same
    one launch (stgcn_input_stage_streams); out= is then (N, S * C, T_out, V).
    parents (V entries; default ``graph.parents(graph.graph_for(V))``) is
    uploaded once, on the side stream; score_channel as in ``stage_clips``. A
    parents table the kernel refuses is reported once, after the last batch."""

    def __init__(self, batches_of_items, device, V, C, C_src, T_out=None,
                 src_dtype=torch.float32, augment=False, out=None, labels_out=None,
                 move=False, crop="first", streams=None, parents=None, score_channel=None):
        self.batches, self.device = batches_of_items, torch.device(device)
        if streams is None and (parents is not None or score_channel is not None):
            raise ValueError("RaggedDeviceLoader: parents and score_channel go with streams")
        self.streams = None if streams is None else parse_streams(streams)
        self.score_channel = score_channel
        S = 1 if streams is None else stream_count(self.streams)
        if crop not in ("first", "random"):
            raise ValueError(f"RaggedDeviceLoader: crop is 'first' or 'random', not {crop!r}")
        self.move, self.crop = bool(move), crop
        self.V, self.C, self.C_src, self.T_out = V, C, C_src, T_out
        self.src_dtype, self.augment = src_dtype, augment
        self.np_dtype = _np_dtype(src_dtype)
        self.out, self.labels_out = out, labels_out
        if (out is not None or labels_out is not None) and T_out is None:
            raise ValueError("RaggedDeviceLoader: out / labels_out need a fixed T_out")
        if out is not None and (tuple(out.shape[1:]) != (S * C, T_out, V) or
                                out.dtype != torch.float32 or not out.is_contiguous()):
            raise ValueError(f"RaggedDeviceLoader: out is a contiguous (N, {S * C}, {T_out}, {V}) "
                             "float32 tensor")
        d = hip_lib.InputDesc(1, C, T_out or 1, V, C_src, int(src_dtype == torch.float64), 1)
        lib = hip_lib.load_library()
        if self.streams is not None:
            sd = hip_lib.StreamsDesc(d, self.streams,
                                     -1 if score_channel is None else int(score_channel))
            rc = lib.stgcn_input_streams_check(ctypes.byref(sd))
        else:
            check = lib.stgcn_input_move_check if self.move else lib.stgcn_input_check
            rc = check(ctypes.byref(d))
        if rc != 0:
            raise ValueError("RaggedDeviceLoader: " +
                             lib.stgcn_last_error().decode(errors="replace"))
        self.stream = torch.cuda.Stream(self.device)
        self.slots = (_Slot(), _Slot())
        self.parents = self.parents_host = self.parents_copied = None
        if parents is not None and np.shape(parents) != (V,):
            raise ValueError(f"RaggedDeviceLoader: parents holds {V} entries, got "
                             f"{np.shape(parents)}")
        if self.streams is not None and self.streams & _BONE_STREAMS:
            if parents is None:
                parents = graph.parents(graph.graph_for(V))
            par = np.ascontiguousarray(parents, dtype=np.int32)
            # uploaded once, on the side stream like the slots' buffers; the first
            # stage kernel of every iteration waits for the copy
            self.parents_host = torch.from_numpy(par).pin_memory()
            with torch.cuda.stream(self.stream):
                self.parents = self.parents_host.to(self.device, non_blocking=True)
                self.parents_copied = torch.cuda.Event()
                self.parents_copied.record(self.stream)

    def _stage(self, items, slot):
        """Packs ``items`` into the slot and starts its copies on the side stream."""
        N = len(items)
        T_out = self.T_out or max(np.asarray(x).shape[-3] for x, _ in items)
        need = N * T_out * self.V * self.C_src
        if slot.copied is not None:
            slot.copied.synchronize()  # (the pinned buffers: their last copy has left)
        # The device buffers come from the SIDE stream's pool (as DeviceLoader's do):
        # their first use is the copy below on that stream, and a block of the
        # consumer's stream could still be in use by its queued kernels. The stage
        # kernel's use on the consumer's stream is recorded in __iter__.
        if slot.host is None or slot.host.numel() < need:
            slot.host = torch.empty(need, dtype=self.src_dtype).pin_memory()
            with torch.cuda.stream(self.stream):
                slot.dev = torch.empty(need, dtype=self.src_dtype, device=self.device)
        nc = N * CLIP_DTYPE.itemsize   # (a multiple of 16: the records behind it are aligned)
        nb = nc + (N * MOVE_DTYPE.itemsize if self.move else 0)
        if slot.host_table is None or slot.host_table.numel() < nb:
            slot.host_table = torch.empty(nb, dtype=torch.uint8).pin_memory()
            with torch.cuda.stream(self.stream):
                slot.dev_table = torch.empty(nb, dtype=torch.uint8, device=self.device)
        tr = clip_transforms(N, True) if self.augment else None
        mv = clip_moves(N, T_out) if self.move else None
        buf, table, labels = pack_clips(items, T_out, self.C_src, self.np_dtype, out=slot.host,
                                        transforms=tr, crop=self.crop)
        if buf.shape[1] != self.V:
            raise ValueError(f"RaggedDeviceLoader: clips of {buf.shape[1]} joints, V = {self.V}")
        slot.host_table.numpy()[:nc] = table.view(np.uint8)
        if mv is not None:
            slot.host_table.numpy()[nc:nb] = mv.view(np.uint8)
        yh = torch.from_numpy(labels).pin_memory()
        with torch.cuda.stream(self.stream):
            if slot.free is not None:
                self.stream.wait_event(slot.free)
            slot.dev[:buf.size].copy_(slot.host[:buf.size], non_blocking=True)
            slot.dev_table[:nb].copy_(slot.host_table[:nb], non_blocking=True)
            yd = yh.to(self.device, non_blocking=True)
            slot.copied = torch.cuda.Event()
            slot.copied.record(self.stream)
        return slot, N, T_out, yd

    def __iter__(self):
        it = iter(self.batches)
        try:
            nxt = self._stage(next(it), self.slots[0])
        except StopIteration:
            return
        statuses, i = [], 0
        while nxt is not None:
            slot, N, T_out, yd = nxt
            i += 1
            try:
                nxt = self._stage(next(it), self.slots[i % 2])
            except StopIteration:
                nxt = None
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(slot.copied)
            yd.record_stream(cur)
            slot.dev.record_stream(cur)
            slot.dev_table.record_stream(cur)
            if self.out is not None:
                if self.out.shape[0] != N:
                    raise ValueError(f"RaggedDeviceLoader: a batch of {N} clips for out of "
                                     f"{self.out.shape[0]}")
                x = self.out
            else:
                S = 1 if self.streams is None else stream_count(self.streams)
                x = torch.empty((N, S * self.C, T_out, self.V), dtype=torch.float32,
                                device=self.device)
            if self.parents is not None:
                cur.wait_event(self.parents_copied)
                self.parents.record_stream(cur)
            status = torch.empty(N, dtype=torch.int32, device=self.device)
            cap = slot.dev.numel() // (self.V * self.C_src)
            src = slot.dev[:cap * self.V * self.C_src].view(cap, self.V, self.C_src)
            nc = N * CLIP_DTYPE.itemsize
            stage_clips(src, slot.dev_table, x, status,
                        moves=slot.dev_table[nc:nc + N * MOVE_DTYPE.itemsize] if self.move
                        else None, streams=self.streams, parents=self.parents,
                        score_channel=self.score_channel)
            slot.free = torch.cuda.Event()
            slot.free.record(cur)
            statuses.append(status)
            if self.labels_out is not None:
                self.labels_out.copy_(yd)
                yd = self.labels_out
            yield x, yd
        flags = torch.cat(statuses).cpu()  # (the one host read)
        if (flags & 4).any():
            raise RuntimeError("RaggedDeviceLoader: invalid parents table (an entry outside "
                               f"[0, {self.V})): every clip was staged as zeros")
        for bit, what in ((1, "clip table entries"), (2, "move records")):
            bad = (flags & bit).nonzero().flatten().tolist()
            if bad:
                raise RuntimeError(f"RaggedDeviceLoader: invalid {what} (flat clip "
                                   f"indices {bad[:8]}{' ...' if len(bad) > 8 else ''}): those "
                                   "clips were staged as zeros")
