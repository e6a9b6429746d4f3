"""What "random moving" costs in the input stage: the move launch and loader
against the plain ones, on the same clips, in one run.

One process, the batches of scripts/input_stage_bench.py (N = 128 ragged
synthetic clips of the bench.py config, T_i uniform in [T/2, T], (T_i, V, 2)
float64), timed windows alternating between the legs, the median of --windows
windows per leg:

  loader        RaggedDeviceLoader, per-clip matrices        (stgcn_input_stage)
  loader+move   ... with move=True, crop="random"            (stgcn_input_stage_move)
  kernel        stgcn_input_stage alone, --kernel-iters launches between two events
  kernel+move   stgcn_input_stage_move alone on the same staging buffer and clip
                table, with clip_moves' records

The script holds no training step and no captured graph: loaders and launches
only. Writes profiles/input_move_<config>.json (also printed as one JSON line):
clips/s and window spread per loader leg, microseconds per launch and window
spread per kernel leg, the move / plain ratios and whether each is inside the
plain leg's own window spread, and the GPU clock state under load.

    python scripts/input_move_bench.py --config cfg3
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", choices=["cfg2", "cfg3"], default="cfg2")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--batches", type=int, default=6, help="batches per pass")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per leg")
    ap.add_argument("--window-seconds", type=float, default=0.6,
                    help="each loader leg repeats its pass until a window lasts about this long")
    ap.add_argument("--kernel-iters", type=int, default=200, help="launches per kernel window")
    ap.add_argument("--out", default=None, help="default profiles/input_move_<config>.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("input_move_bench needs a ROCm GPU; there is no CPU path")
    pkg = load()
    data = pkg.data
    dev = torch.device("cuda", 0)
    C = C_src = 2
    cfg = bench.CONFIGS[args.config]
    N, T, V = args.batch, cfg["T"], cfg["V"]
    batches = make_batches(args.batches, N, T, V, C_src, cfg["classes"])
    bench.progress(f"{args.batches} batches of {N} ragged clips made")

    def loader(move):
        def run(passes=1):
            last = None
            for _ in range(passes):
                for x, _ in data.RaggedDeviceLoader(
                        batches, dev, V, C, C_src, T_out=T, src_dtype=torch.float64,
                        augment=True, move=move, crop="random" if move else "first"):
                    last = x
            return last
        return run

    # the kernels alone: one staging buffer and clip table for both launches
    tr = data.clip_transforms(N, True)
    buf, table, _ = data.pack_clips(batches[0], T, C_src, np.float64, transforms=tr)
    src = torch.from_numpy(buf).to(dev)
    tab = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    mvd = torch.from_numpy(data.clip_moves(N, T).view(np.uint8).copy()).to(dev)
    x = torch.empty(N, C, T, V, device=dev)
    status = torch.empty(N, dtype=torch.int32, device=dev)

    def kernel(moves):
        def run(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                data.stage_clips(src, tab, x, status, moves=moves)
            e1.record()
            torch.cuda.synchronize()
            if status.any().item():
                raise SystemExit("the stage kernel flagged a clip")
            return e0.elapsed_time(e1) * 1e3 / iters     # us per launch
        return run

    loaders = {"loader": loader(False), "loader+move": loader(True)}
    kernels = {"kernel": kernel(None), "kernel+move": kernel(mvd)}
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
            if w == args.windows // 2 and name == "loader+move":
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
    nbytes = N * T * V * (C_src * 8 + 4 * C)
    legs = {}
    for k in loaders:
        legs[k] = {"clips_per_s": round(clips / med[k], 1),
                   "window_clips_per_s": [round(clips / t, 1) for t in times[k]],
                   "window_spread": round(spread[k], 3)}
    for k in kernels:
        legs[k] = {"us_per_launch": round(med[k], 3),
                   "window_us_per_launch": [round(t, 3) for t in times[k]],
                   "window_spread": round(spread[k], 3),
                   "GBps": round(nbytes / (med[k] * 1e-6) / 1e9, 1)}
    out = {"bench": "input_move", "config": args.config, "N": N, "T": T, "V": V, "C": C,
           "C_src": C_src, "src_dtype": "float64", "batches_per_pass": args.batches,
           "passes_per_window": passes, "windows": args.windows,
           "kernel_launches_per_window": args.kernel_iters, "algorithmic_bytes": nbytes,
           "legs": legs,
           "loader_move_over_plain_time": round(med["loader+move"] / med["loader"], 3),
           "kernel_move_over_plain_time": round(med["kernel+move"] / med["kernel"], 3),
           "loader_move_within_plain_spread": bool(
               med["loader+move"] <= med["loader"] * (1 + spread["loader"])),
           "kernel_move_within_plain_spread": bool(
               med["kernel+move"] <= med["kernel"] * (1 + spread["kernel"])),
           "gpu_state_under_load": state,
           "gpu": torch.cuda.get_device_name(0)}
    path = args.out or os.path.join(ROOT, "profiles", f"input_move_{args.config}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
