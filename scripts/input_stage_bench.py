"""Input pipeline throughput: the host route against the device input stage.

One process, batches of N = 128 ragged synthetic clips of the bench.py config
(T_i uniform in [T/2, T], one clip per batch at T so every batch pads to T and
the eval step sees one shape; (T_i, V, 2) float64, as np.load gives a clip),
timed windows alternating between the legs (so clock state and neighbours hit
them alike). A pass is one iteration over --batches batches; a window repeats
the leg's pass until it lasts about --window-seconds (times are per pass):

  a        loopy_pad_collate_fn -> augment_data (float64, one matrix per batch)
           -> DeviceLoader (fp32 cast, pinned copy, permute on the device)
  b        RaggedDeviceLoader with per-clip augmentation (pack_clips into pinned
           memory, stgcn_input_stage on the device)
  a+eval   route a feeding STGCNStack.eval_step
  b+eval   route b feeding STGCNStack.eval_step

augment_data takes 25 joints only; at another V route a applies the same
arithmetic (one augmentation_matrix per batch, homogeneous rows .dot the
matrix) without that check. Writes profiles/input_stage_<config>.json (also
printed as one JSON line): clips/s per leg (median window, and every window),
b / a, the window-to-window spread, the stage kernel's time per batch between
two hipEvents with its algorithmic bytes and share of the HBM peak, and the GPU
clock state under load.

    python scripts/input_stage_bench.py --config cfg3
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from stgcn_loader import load  # noqa: E402


def make_batches(nbatches, N, T, V, C_src, classes, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nbatches):
        lengths = rng.integers(T // 2, T + 1, size=N)
        lengths[0] = T
        out.append([(rng.standard_normal((1, int(t), V, C_src)), np.array([int(lab)]))
                    for t, lab in zip(lengths, rng.integers(0, classes, size=N))])
    return out


def augment_batch(data, x):
    """augment_data on a collated (N, T, V, 2) float64 batch; its arithmetic
    without the 25-joint check at another V."""
    if x.shape[2] == 25:
        return data.augment_data(x)
    M = data.augmentation_matrix()
    n, t, v, d = x.shape
    h = np.zeros((n * t * v, d + 1))
    h[:, :2] = x.reshape(n * t * v, d)
    return h.dot(M)[:, :2].reshape(n, t, v, d)


def calibrate(model, x):
    """running_mean / running_var <- the statistics of x's activations (eval_bench.py)."""
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for bn in bns:
        bn.momentum = 1.0
    model.train()
    with torch.no_grad():
        model.forward_nctv(x)
    for bn in bns:
        bn.momentum = 0.1
    model.eval()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", choices=["cfg2", "cfg3"], default="cfg2")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--batches", type=int, default=6, help="batches per pass")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per leg")
    ap.add_argument("--window-seconds", type=float, default=0.6,
                    help="each leg repeats its pass until a window lasts about this long")
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="default profiles/input_stage_<config>.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("input_stage_bench needs a ROCm GPU; there is no CPU path")
    pkg = load()
    data = pkg.data
    dev = torch.device("cuda", 0)
    C = C_src = 2   # x, y: what augment_data yields
    cfg = dict(bench.CONFIGS[args.config], N=args.batch, C=C, f32_gemm="f16x2")
    N, T, V = cfg["N"], cfg["T"], cfg["V"]
    batches = make_batches(args.batches, N, T, V, C_src, cfg["classes"])
    bench.progress(f"{args.batches} batches of {N} ragged clips made")
    model = bench.build_model(pkg, cfg, dev)
    gen = torch.Generator(device="cpu").manual_seed(1)
    calibrate(model, torch.randn(N, C, T, V, generator=gen).to(dev))
    metrics = pkg.EvalMetrics(cfg["classes"], device=dev)

    def route_a():
        def collated():
            for items in batches:
                x, y = data.loopy_pad_collate_fn(items)
                yield torch.from_numpy(augment_batch(data, x.numpy())), y
        return data.DeviceLoader(collated(), dev)

    def route_b():
        return data.RaggedDeviceLoader(batches, dev, V, C, C_src, src_dtype=torch.float64,
                                       augment=True)

    def alone(route):
        def run(passes=1):
            last = None
            for _ in range(passes):
                for x, y in route():
                    last = x
            return last
        return run

    def with_eval(route):
        def run(passes=1):
            loss = None
            for _ in range(passes):
                for x, y in route():
                    loss, _ = model.eval_step(x, y, metrics)
            return loss
        return run

    legs = {"a": alone(route_a), "b": alone(route_b),
            "a+eval": with_eval(route_a), "b+eval": with_eval(route_b)}
    passes = {}
    for name, fn in legs.items():
        out = fn()                  # (untimed: pinned pools, workspaces)
        torch.cuda.synchronize()
        if not torch.isfinite(out).all().item():
            raise SystemExit(f"leg {name}: not finite")
        t0 = time.perf_counter()    # one pass timed, to size the leg's windows
        fn()
        torch.cuda.synchronize()
        passes[name] = max(1, math.ceil(args.window_seconds / (time.perf_counter() - t0)))
        bench.progress(f"leg {name} warmed up, {passes[name]} passes per window")
    times = {k: [] for k in legs}
    smi, state = None, None
    for w in range(args.windows):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            if w == args.windows // 2 and name == "b+eval":
                smi = bench.gpu_state_start()   # (read-only sample while the leg runs)
            t0 = time.perf_counter()
            fn(passes[name])
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / passes[name])
            if smi is not None and state is None:
                state = bench.gpu_state_read(smi)
                smi = None
        bench.progress(f"window {w + 1}/{args.windows}")

    # the stage kernel alone, between two events on the launch stream
    tr = data.clip_transforms(N, True)
    buf, table, _ = data.pack_clips(batches[0], T, C_src, np.float64, transforms=tr)
    src = torch.from_numpy(buf).to(dev)
    tab = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    x = torch.empty(N, C, T, V, device=dev)
    status = torch.empty(N, dtype=torch.int32, device=dev)
    for _ in range(5):
        data.stage_clips(src, tab, x, status)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.kernel_iters):
        data.stage_clips(src, tab, x, status)
    e1.record()
    torch.cuda.synchronize()
    kernel_ms = e0.elapsed_time(e1) / args.kernel_iters
    if status.any().item():
        raise SystemExit("the stage kernel flagged a clip")
    nbytes = N * T * V * (C_src * 8 + 4 * C)

    clips = N * args.batches
    rate = {k: clips / statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in times.items()}
    out = {"bench": "input_stage", "config": args.config, "N": N, "T": T, "V": V, "C": C,
           "C_src": C_src, "src_dtype": "float64", "gemm": "bf16" if cfg["bf16"] else "f16x2",
           "batches_per_pass": args.batches, "passes_per_window": passes,
           "windows": args.windows,
           "legs": {k: {"clips_per_s": round(rate[k], 1),
                        "window_clips_per_s": [round(clips / t, 1) for t in times[k]],
                        "window_spread": round(spread[k], 3)} for k in legs},
           "leg_names": {"a": "loopy_pad_collate_fn -> augment_data -> DeviceLoader",
                         "b": "RaggedDeviceLoader, per-clip augmentation",
                         "a+eval": "route a feeding eval_step",
                         "b+eval": "route b feeding eval_step"},
           "b_over_a": round(rate["b"] / rate["a"], 3),
           "b_eval_over_a_eval": round(rate["b+eval"] / rate["a+eval"], 3),
           "b_not_slower_within_spread": bool(
               rate["b"] >= rate["a"] * (1 - max(spread["a"], spread["b"])) and
               rate["b+eval"] >= rate["a+eval"] * (1 - max(spread["a+eval"], spread["b+eval"]))),
           "stage_kernel": {"ms_per_batch": round(kernel_ms, 4), "algorithmic_bytes": nbytes,
                            "GBps": round(nbytes / (kernel_ms * 1e-3) / 1e9, 1),
                            "share_of_hbm_peak": round(
                                nbytes / (kernel_ms * 1e-3) / 1e9 / bench.HBM_PEAK_GBS, 4),
                            "launches_timed": args.kernel_iters},
           "gpu_state_under_load": state,
           "gpu": torch.cuda.get_device_name(0)}
    path = args.out or os.path.join(ROOT, "profiles", f"input_stage_{args.config}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
