"""What the bone and motion streams cost in the input stage: the one stream
launch against the existing launch followed by the derivation in torch, on the
same clips, in one run.

One process, the batches of scripts/input_stage_bench.py (N = 128 ragged
synthetic clips of the bench.py config, T_i uniform in [T/2, T], (T_i, V, 2)
float64), timed windows alternating between the legs, the median of --windows
windows per leg:

  (a) kernel+torch  stgcn_input_stage_move, then the four streams in torch: a
                    gather of the parents, two subtractions, two shifted-slice
                    subtractions into zeroed tensors, one cat (8 launches)
  (b) streams       stgcn_input_stage_streams with the full mask (1 launch)
  (c) kernel        stgcn_input_stage_move alone: the floor of (a)
  loader (a)        RaggedDeviceLoader(move=True), the torch derivation per batch
  loader (b)        RaggedDeviceLoader(move=True, streams="j+b+jm+bm")

Each kernel leg is --kernel-iters repetitions between two device events. Before
timing, (a) and (b) are compared once: the same bits. The script holds no
training step, no model and no captured graph. Writes
profiles/input_streams_<config>.json (also printed as one JSON line):
microseconds per repetition and window spread per kernel leg, clips/s and window
spread per loader leg, launches per batch, the algorithmic bytes, the (a) / (b)
ratios and whether (b) is faster by more than both legs' window spread, and the
GPU clock state under load.

    python scripts/input_streams_bench.py --config cfg3
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from input_stage_bench import make_batches  # noqa: E402
from stgcn_loader import load  # noqa: E402

FULL = "j+b+jm+bm"
TORCH_LAUNCHES = 7   # index_select, sub, 2 x (zeros_like, sub into the slice), cat


def torch_streams(j, par):
    """The four streams of j (N, C, T, V) the way a user of the staged x forms
    them today (no score channel)."""
    b = j - j.index_select(3, par)
    jm, bm = torch.zeros_like(j), torch.zeros_like(j)
    torch.sub(j[:, :, 1:], j[:, :, :-1], out=jm[:, :, :-1])
    torch.sub(b[:, :, 1:], b[:, :, :-1], out=bm[:, :, :-1])
    return torch.cat((j, b, jm, bm), 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", choices=["cfg2", "cfg3"], default="cfg2")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--batches", type=int, default=6, help="batches per pass")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per leg")
    ap.add_argument("--window-seconds", type=float, default=0.6,
                    help="each loader leg repeats its pass until a window lasts about this long")
    ap.add_argument("--kernel-iters", type=int, default=200, help="repetitions per kernel window")
    ap.add_argument("--out", default=None, help="default profiles/input_streams_<config>.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("input_streams_bench needs a ROCm GPU; there is no CPU path")
    pkg = load()
    data = pkg.data
    dev = torch.device("cuda", 0)
    C = C_src = 2
    S = 4
    cfg = bench.CONFIGS[args.config]
    N, T, V = args.batch, cfg["T"], cfg["V"]
    batches = make_batches(args.batches, N, T, V, C_src, cfg["classes"])
    par = torch.from_numpy(pkg.graph.parents(pkg.graph.graph_for(V))).to(dev)
    par64 = par.long()
    bench.progress(f"{args.batches} batches of {N} ragged clips made")

    def loader(streams):
        def run(passes=1):
            last = None
            for _ in range(passes):
                for x, _ in data.RaggedDeviceLoader(
                        batches, dev, V, C, C_src, T_out=T, src_dtype=torch.float64,
                        augment=True, move=True, crop="random", streams=streams):
                    last = x if streams else torch_streams(x, par64)
            return last
        return run

    # the kernels alone: one staging buffer, clip table and move table for all legs
    tr = data.clip_transforms(N, True)
    buf, table, _ = data.pack_clips(batches[0], T, C_src, np.float64, transforms=tr)
    src = torch.from_numpy(buf).to(dev)
    tab = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    mvd = torch.from_numpy(data.clip_moves(N, T).view(np.uint8).copy()).to(dev)
    xj = torch.empty(N, C, T, V, device=dev)
    xs = torch.empty(N, S * C, T, V, device=dev)
    status = torch.empty(N, dtype=torch.int32, device=dev)

    def leg_a():
        return torch_streams(data.stage_clips(src, tab, xj, status, moves=mvd), par64)

    def leg_b():
        return data.stage_clips(src, tab, xs, status, moves=mvd, streams=FULL, parents=par)

    def leg_c():
        return data.stage_clips(src, tab, xj, status, moves=mvd)

    if not torch.equal(leg_a().view(torch.int32), leg_b().view(torch.int32)):
        raise SystemExit("the stream launch and the torch derivation differ")

    def kernel(fn):
        def run(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if status.any().item():
                raise SystemExit("the stage kernel flagged a clip")
            return e0.elapsed_time(e1) * 1e3 / iters     # us per repetition
        return run

    loaders = {"loader (a)": loader(None), "loader (b)": loader(FULL)}
    kernels = {"(a) kernel+torch": kernel(leg_a), "(b) streams": kernel(leg_b),
               "(c) kernel": kernel(leg_c)}
    passes = {}
    for name, fn in loaders.items():
        out = fn()                  # (untimed: pinned pools)
        torch.cuda.synchronize()
        if not torch.isfinite(out).all().item():
            raise SystemExit(f"leg {name}: not finite")
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        passes[name] = max(1, math.ceil(args.window_seconds / (time.perf_counter() - t0)))
        bench.progress(f"leg {name} warmed up, {passes[name]} passes per window")
    for fn in kernels.values():
        fn(10)
    times = {k: [] for k in (*loaders, *kernels)}
    smi, state = None, None
    for w in range(args.windows):
        for name, fn in loaders.items():
            torch.cuda.synchronize()
            if w == args.windows // 2 and name == "loader (b)":
                smi = bench.gpu_state_start()   # (read-only sample while the leg runs)
            t0 = time.perf_counter()
            fn(passes[name])
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / passes[name])
            if smi is not None and state is None:
                state = bench.gpu_state_read(smi)
                smi = None
        for name, fn in kernels.items():
            times[name].append(fn(args.kernel_iters))
        bench.progress(f"window {w + 1}/{args.windows}")

    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    clips = N * args.batches
    nbytes = {"(a) kernel+torch": None,
              "(b) streams": N * T * V * (C_src * 8 + 4 * S * C),
              "(c) kernel": N * T * V * (C_src * 8 + 4 * C)}
    legs = {}
    for k in loaders:
        legs[k] = {"clips_per_s": round(clips / med[k], 1),
                   "window_clips_per_s": [round(clips / t, 1) for t in times[k]],
                   "window_spread": round(spread[k], 3)}
    for k in kernels:
        legs[k] = {"us": round(med[k], 3), "window_us": [round(t, 3) for t in times[k]],
                   "window_spread": round(spread[k], 3)}
        if nbytes[k]:
            legs[k]["algorithmic_bytes"] = nbytes[k]
            legs[k]["GBps"] = round(nbytes[k] / (med[k] * 1e-6) / 1e9, 1)

    def faster(a, b):   # b beats a by more than the window spread both legs show
        return bool(med[b] * (1 + spread[b]) < med[a] * (1 - spread[a]))

    out = {"bench": "input_streams", "config": args.config, "N": N, "T": T, "V": V, "C": C,
           "C_src": C_src, "streams": FULL, "src_dtype": "float64",
           "batches_per_pass": args.batches, "passes_per_window": passes,
           "windows": args.windows, "kernel_repetitions_per_window": args.kernel_iters,
           "launches_per_batch": {"a": 1 + TORCH_LAUNCHES, "b": 1},
           "legs": legs,
           "kernel_a_over_b_time": round(med["(a) kernel+torch"] / med["(b) streams"], 3),
           "kernel_b_over_c_time": round(med["(b) streams"] / med["(c) kernel"], 3),
           "loader_a_over_b_time": round(med["loader (a)"] / med["loader (b)"], 3),
           "kernel_b_faster_beyond_spread": faster("(a) kernel+torch", "(b) streams"),
           "loader_b_faster_beyond_spread": faster("loader (a)", "loader (b)"),
           "gpu_state_under_load": state,
           "gpu": torch.cuda.get_device_name(0)}
    path = args.out or os.path.join(ROOT, "profiles", f"input_streams_{args.config}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
