"""One rank of the multi-rank HIP data-parallel check (tests/test_dp_gpu.py).

Launched by torch.distributed.run with WORLD_SIZE ranks that all share the one
GPU of the box (cuda:0) over the gloo backend (RCCL refuses two ranks on one
device; the 8-GPU RCCL run is the driver's). Each rank runs the benched step
on its own shard: STGCNStack (the benched f16x2 fp32 path: stgcn_fold_prep,
unwritten block outputs, the head pooling from U; StackChain, fused head) +
dp.GradAllReduce (bucket-view gradients) + FusedAdam. Rank 0 then recomputes,
in the same process and without any collective, the per-shard HIP gradients
of every rank on a fresh copy of the initial model, and checks
  * the all-reduced gradients == the mean of the per-shard gradients,
  * every rank ends the step with bit-identical parameters,
  * the parameters == one FusedAdam step on the mean gradients.
Writes a JSON verdict to $DP_OUT (rank 0).
"""
import contextlib
import io
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stgcn_loader import load  # noqa: E402
from gates import worst_of  # noqa: E402  (tests/, this script's directory)


def build(pkg, A):
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = pkg.STGCNStack(3, 60, A, f32_gemm="f16x2")
    return m.cuda().train()


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    pkg = load()
    gr = pkg.graph
    A = gr.get_normalized_adjacency_matrices(0, 1, graph=gr.graph_for(18))
    N, T = 4, 64
    gen = torch.Generator().manual_seed(77)
    xs = torch.randn(world, N, 3, T, 18, generator=gen)
    ys = torch.randint(0, 60, (world, N), generator=gen)

    model = build(pkg, A)
    p_init = [p.detach().clone() for p in model.parameters()]
    opt = pkg.FusedAdam(list(model.parameters()), lr=1e-3)
    dp = pkg.dp.GradAllReduce(model, world, bucket_bytes=1 << 20, trace=True)
    dp.zero_grad()
    loss, _ = model.forward_loss(xs[rank].cuda(), ys[rank].cuda())
    loss.backward()
    dp.synchronize()
    # overlap: the first bucket's all-reduce is issued before block 0 (whose
    # backward runs last) has produced any gradient
    names0 = [k for k, _ in model.named_parameters()]
    blk0 = {i for i, k in enumerate(names0) if k.startswith("conv.0.")}
    tr = dp.last_trace
    first_launch = next(j for j, (k, _) in enumerate(tr) if k == "launch")
    first_blk0 = next(j for j, (k, i) in enumerate(tr) if k == "grad" and i in blk0)
    launches_before_blk0 = sum(1 for k, _ in tr[:first_blk0] if k == "launch")
    views = all(p.grad is dp._view[p] for p in model.parameters())
    grads = [p.grad.detach().clone() for p in model.parameters()]
    opt.step()
    torch.cuda.synchronize()
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()
    gathered = [torch.empty_like(flat) for _ in range(world)]
    dist.all_gather(gathered, flat)
    if rank == 0:
        # per-shard HIP gradients, sequentially in this process (no collective)
        def shard_grads(r):
            m = build(pkg, A)
            with torch.no_grad():
                for p, q in zip(m.parameters(), p_init):
                    p.copy_(q)
            ls, _ = m.forward_loss(xs[r].cuda(), ys[r].cuda())
            ls.backward()
            return [p.grad.detach().clone() for p in m.parameters()]

        per = [shard_grads(r) for r in range(world)]
        # (every gradient, dA included, is run-to-run deterministic: dA is summed
        # from per-workgroup partials in a fixed order, launch_dA_reduce; a
        # re-run of shard 0 must reproduce it bit for bit)
        rerun0 = shard_grads(0)
        rerun_exact = all(torch.equal(a, b) for a, b in zip(per[0], rerun0))
        errs = []
        for i, g in enumerate(grads):
            want = sum(pg[i] for pg in per) / world
            errs.append(((g - want).abs().max() / want.abs().max().clamp_min(1e-30)).item())
        worst = worst_of(errs)  # (NaN when a gradient holds one: tests/gates.py)
        # one FusedAdam step on the mean gradients from the same initial params
        m = build(pkg, A)
        with torch.no_grad():
            for p, q in zip(m.parameters(), p_init):
                p.copy_(q)
        for i, p in enumerate(m.parameters()):
            p.grad = sum(pg[i] for pg in per) / world
        pkg.FusedAdam(list(m.parameters()), lr=1e-3).step()
        torch.cuda.synchronize()
        want_flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu()
        step_err = ((flat - want_flat).abs().max() / want_flat.abs().max()).item()
        same = all(torch.equal(gathered[0], g) for g in gathered[1:])
        out = {"world": world, "grad_err": worst, "rerun_exact": rerun_exact,
               "ranks_identical": same, "step_err": step_err,
               "bucket_views": views, "buckets": len(dp.buckets), "loss": loss.item(),
               "first_launch_pos": first_launch, "first_block0_grad_pos": first_blk0,
               "launches_before_block0": launches_before_blk0, "trace_len": len(tr)}
        with open(os.environ["DP_OUT"], "w") as f:
            json.dump(out, f)
        print(json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
