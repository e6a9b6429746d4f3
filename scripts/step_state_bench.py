"""Training-step throughput with per-step values in device memory.

One process, N = 128 clips of the bench.py config, timed windows alternating
between the legs (so clock state and neighbours hit them alike):

  a  the eager dropout-0.5 step with host seeds (before dropout_seed="device"
     the only correct dropout route: a capture would freeze the mask)
  b  the same stack with dropout_seed="device" in a HIP graph (GraphedStep)
  c  the graphed no-dropout step, float lr (bench.py's N = 1 step mode)
  d  the same with a tensor lr and max_grad_norm = 1.0 (stgcn_adam_step_dev2
     behind stgcn_grad_norm)

Writes profiles/step_state_<config>.json (also printed as one JSON line):
clips/s per leg (median window), kernel launches per step (torch profiler, a
run of its own), the GPU clock state under load, and b / a, d / c.

    python scripts/step_state_bench.py --config cfg2
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from stgcn_loader import load  # noqa: E402


def count_launches(fn):
    """Device kernels of one call of fn (after it ran once): the profiler's
    device-side events, host activity recorded too (a backward runs on the
    autograd thread, a replay is one host call)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    for _ in range(3):  # (a trace now and then comes back without its device events)
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        n = sum(1 for e in dev
                if "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        if n:
            return n
    raise RuntimeError(f"the profiler recorded no device kernel ({len(prof.events())} events)")


def build(pkg, cfg, dev, drop, dropout_seed):
    A = bench.adjacency(pkg, cfg)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = pkg.STGCNStack(cfg["C"], cfg["classes"], A, dropout_rate=drop,
                           gemm_dtype=torch.bfloat16 if cfg["bf16"] else torch.float32,
                           f32_gemm="f16x2", dropout_seed=dropout_seed)
    return m.to(dev).train()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", choices=["cfg2", "cfg3"], default="cfg2")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per leg")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None, help="default profiles/step_state_<config>.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("step_state_bench needs a ROCm GPU; there is no CPU path")
    pkg = load()
    dev = torch.device("cuda", 0)
    cfg = dict(bench.CONFIGS[args.config], N=args.batch)
    gen = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(cfg["N"], cfg["C"], cfg["T"], cfg["V"], generator=gen).to(dev)
    labels = torch.randint(0, cfg["classes"], (cfg["N"],), generator=gen).to(dev)

    def make(drop, dropout_seed, **adam):
        m = build(pkg, cfg, dev, drop, dropout_seed)
        opt = pkg.FusedAdam(list(m.parameters()), capturable=True, **adam)

        def step():
            opt.zero_grad(set_to_none=True)
            loss, logits = m.forward_loss(x, labels)
            loss.backward()
            opt.step()
            return loss
        return m, step

    legs, models = {}, {}
    bench.progress("leg a: eager dropout step, host seeds")
    models["a"], legs["a"] = make(0.5, "host", lr=1e-3)
    for _ in range(args.warmup):
        legs["a"]()
    bench.progress("leg b: graphed dropout step, device seeds")
    models["b"], step_b = make(0.5, "device", lr=1e-3)
    legs["b"] = pkg.GraphedStep(step_b, warmup=args.warmup)
    bench.progress("leg c: graphed step, float lr")
    models["c"], step_c = make(0, "host", lr=1e-3)
    legs["c"] = pkg.GraphedStep(step_c, warmup=args.warmup)
    bench.progress("leg d: graphed step, tensor lr + max_grad_norm")
    models["d"], step_d = make(0, "host", lr=torch.tensor(1e-3, device=dev), max_grad_norm=1.0)
    legs["d"] = pkg.GraphedStep(step_d, warmup=args.warmup)
    for fn in legs.values():  # (one untimed pass: the first window after the captures is cold)
        for _ in range(2):
            fn()
    torch.cuda.synchronize()

    times = {k: [] for k in legs}
    smi, state = None, None
    for w in range(args.windows):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            if w == args.windows // 2 and name == "c":
                smi = bench.gpu_state_start()  # (read-only sample while leg c runs)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            if smi is not None and state is None:
                state = bench.gpu_state_read(smi)
                smi = None
            if not torch.isfinite(loss).item():
                raise SystemExit(f"leg {name}: the loss is not finite")
        bench.progress(f"window {w + 1}/{args.windows}")
    counter = int(models["b"].drop_counter.item())
    launches, note = {}, None
    if not args.no_launch_count:
        try:
            for name, fn in legs.items():
                launches[name] = count_launches(fn)
        except Exception as e:  # (the timings stand; the count is reported as not measured)
            launches, note = {}, f"not measured: {type(e).__name__}: {e}"
    rate = {k: cfg["N"] * args.steps / statistics.median(v) for k, v in times.items()}
    out = {"bench": "step_state", "config": args.config, "N": cfg["N"], "T": cfg["T"],
           "V": cfg["V"], "K": cfg["K"], "classes": cfg["classes"],
           "gemm": "bf16" if cfg["bf16"] else "f16x2",
           "steps_per_window": args.steps, "windows": args.windows,
           "legs": {k: {"clips_per_s": round(rate[k], 1),
                        "window_clips_per_s": [round(cfg["N"] * args.steps / t, 1)
                                               for t in times[k]],
                        "launches_per_step": launches.get(k)} for k in legs},
           "leg_names": {"a": "eager, dropout 0.5, host seeds",
                         "b": "graphed, dropout 0.5, device seeds",
                         "c": "graphed, no dropout, float lr",
                         "d": "graphed, no dropout, tensor lr + max_grad_norm=1.0"},
           "b_over_a": round(rate["b"] / rate["a"], 3),
           "d_over_c": round(rate["d"] / rate["c"], 3),
           "dropout_steps_counted_on_device": counter,
           "gpu_state_under_load": state,
           "gpu": torch.cuda.get_device_name(0)}
    if note:
        out["launches_per_step"] = note
    path = args.out or os.path.join(ROOT, "profiles", f"step_state_{args.config}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
