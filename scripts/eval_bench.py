"""Evaluation-step throughput: today's eval route against STGCNStack.eval_step.

One process, N = 128 clips of the bench.py config, timed windows alternating
between the legs (so clock state and neighbours hit them alike):

  A        eval() + no_grad: forward_nctv, F.cross_entropy, argmax and a torch
           bincount confusion matrix kept on the device (no host read per step:
           kinder to this leg than the reference's .item() per batch)
  B        eval_step + EvalMetrics (blocks chained through U, nothing kept for a
           backward, the scoring head with device-side metrics)
  B-graph  the same step in a HIP graph (train_ops.GraphedStep); with --graph

The running statistics are first set to the statistics of the bench batch (one
training-mode forward with momentum 1), so eval-mode activations have the scale
they have in training. Prints one JSON line: clips/s (median window), kernel
launches per step (torch profiler, a run of its own) and peak allocated bytes
per leg, and B / A.

    python scripts/eval_bench.py --config cfg2 --graph
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402
from stgcn_loader import load  # noqa: E402


def calibrate(model, x):
    """running_mean / running_var <- the statistics of x's activations."""
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for bn in bns:
        bn.momentum = 1.0
    model.train()
    with torch.no_grad():
        model.forward_nctv(x)
    for bn in bns:
        bn.momentum = 0.1
    model.eval()


def count_launches(fn):
    """Device kernels of one call of fn (after it ran once)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
            and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    if n == 0:
        raise RuntimeError("the profiler recorded no device kernel")
    return n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", choices=["cfg2", "cfg3", "cfg5"], default="cfg2")
    ap.add_argument("--graph", action="store_true", help="add the HIP-graph leg of eval_step")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20, help="steps per timed window")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per leg")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-launch-count", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a ROCm GPU; there is no CPU path")
    pkg = load()
    dev = torch.device("cuda", 0)
    cfg = dict(bench.CONFIGS[args.config], N=args.batch, f32_gemm="f16x2")
    model = bench.build_model(pkg, cfg, dev)
    gen = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(cfg["N"], cfg["C"], cfg["T"], cfg["V"], generator=gen).to(dev)
    labels = torch.randint(0, cfg["classes"], (cfg["N"],), generator=gen).to(dev)
    calibrate(model, x)
    classes = cfg["classes"]
    conf = torch.zeros(classes * classes, dtype=torch.int64, device=dev)
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    metrics = pkg.EvalMetrics(classes, device=dev)

    @torch.no_grad()
    def leg_a():
        logits = model.forward_nctv(x)
        loss = F.cross_entropy(logits, labels)
        pred = torch.argmax(logits, dim=1)
        sums[0] += loss
        sums[1] += (pred == labels).sum() / len(pred)
        conf.add_(torch.bincount(labels * classes + pred, minlength=classes * classes))
        return loss, logits

    def leg_b():
        return model.eval_step(x, labels, metrics)

    legs = {"A": leg_a, "B": leg_b}
    peak, launches = {}, {}
    for name, fn in list(legs.items()):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated(dev) - base
    if args.graph:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        legs["B-graph"] = pkg.GraphedStep(leg_b, warmup=2)
        for _ in range(args.warmup):
            legs["B-graph"]()
        torch.cuda.synchronize()
        peak["B-graph"] = torch.cuda.max_memory_allocated(dev) - base
    # the two routes agree before anything is timed
    la, lb = leg_a()[1], leg_b()[1]
    agree = float((la - lb).abs().max() / la.abs().max())
    if not agree < 1e-5:
        raise SystemExit(f"eval_step and forward_nctv disagree: rel-to-max {agree}")
    times = {name: [] for name in legs}
    for _ in range(args.windows):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    launch_note = None
    if not args.no_launch_count:
        try:
            for name, fn in legs.items():
                launches[name] = count_launches(fn)
        except Exception as e:  # (the timings stand; the count is reported as not measured)
            launches, launch_note = {}, f"not measured: {type(e).__name__}: {e}"
    rate = {k: cfg["N"] * args.steps / statistics.median(v) for k, v in times.items()}
    out = {"bench": "eval_step", "config": args.config, "N": cfg["N"], "T": cfg["T"],
           "V": cfg["V"], "K": cfg["K"], "classes": classes,
           "gemm": "bf16" if cfg["bf16"] else cfg["f32_gemm"],
           "steps_per_window": args.steps, "windows": args.windows,
           "eval_plan": model.last_eval_plan, "logits_rel_to_max_A_vs_B": agree,
           "legs": {k: {"clips_per_s": round(rate[k], 1),
                        "window_clips_per_s": [round(cfg["N"] * args.steps / t, 1)
                                               for t in times[k]],
                        "launches_per_step": launches.get(k),
                        "peak_allocated_bytes": peak[k]} for k in legs},
           "B_over_A": round(rate["B"] / rate["A"], 3),
           "gpu": torch.cuda.get_device_name(0)}
    if launch_note:
        out["launches_per_step"] = launch_note
    if args.graph:
        out["B_graph_over_A"] = round(rate["B-graph"] / rate["A"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
