"""What activation checkpointing costs and saves: forward + backward of one micro-batch of the flagship model (ego-b, N = M = 2048, the
benchmark's micro-batch) with `act_checkpoint` off and on, in one process on the same device, back to back.  With the flag every block
but the last of either stack is run a second time in front of its backward (without its last residual GEMM); embeddings, logits and
the cross-entropy are not - the expected time ratio is below 4/3.  The flag keeps one fp32 [rows, D] tensor per layer instead of the
layer's whole buffer set.

    python tools/act_checkpoint_cost.py [--micro-batch 64] [--iters 5] [--repeats 3]

Prints one JSON line: per setting the median milliseconds per forward + backward (of `--repeats` timed runs of `--iters` steps, after
a warm-up), `Engine.workspace_bytes()` and torch's peak allocated bytes; the time ratio, and whether the two losses and gradients agree
bit for bit."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egom2p_amd import synth  # noqa: E402
from egom2p_amd.config import MODEL_CFGS  # noqa: E402
from egom2p_amd.engine import Engine  # noqa: E402


def measure(cfg, mb, mbs, iters, repeats, flag, warmup=2):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    eng = Engine(cfg, "cuda:0", max_batch=mb, n_enc=2048, n_dec=2048, act_checkpoint=flag)
    eng.init_random(seed=0)
    names = [m.name for m in cfg.mods]

    def step(i):
        eng.forward(mbs[i % len(mbs)], dec_order=names, loss_grad=1.0, training=True)
        eng.backward(1.0)

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for i in range(iters):
            step(i)
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]) / iters)
    # one step from clean gradients for the comparison of the two settings
    eng.zero_grad()
    step(0)
    torch.cuda.synchronize()
    res = {"fwd_bwd_ms": round(statistics.median(times), 2), "fwd_bwd_ms_runs": [round(t, 2) for t in times],
           "workspace_bytes": eng.workspace_bytes(), "peak_allocated_bytes": int(torch.cuda.max_memory_allocated()),
           "allocated_before_bytes": int(base), "loss": float(eng.loss_out[0].item())}
    return res, eng.loss_out.clone(), eng.G.to("cpu")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="egom2p_base_12e_12d_swiglu_nobias")
    ap.add_argument("--micro-batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    cfg = MODEL_CFGS[args.model]
    mb = args.micro_batch
    mbs = [synth.make_clip_batch_device(cfg, mb, synth.CANONICAL_BUDGETS, seed=100, sample_offset=i * mb, device="cuda:0") for i in range(2)]
    off, loss0, g0 = measure(cfg, mb, mbs, args.iters, args.repeats, False)
    on, loss1, g1 = measure(cfg, mb, mbs, args.iters, args.repeats, True)
    print(json.dumps({"model": args.model, "micro_batch": mb, "off": off, "on": on,
                      "time_ratio": round(on["fwd_bwd_ms"] / off["fwd_bwd_ms"], 4),
                      "peak_ratio": round(on["peak_allocated_bytes"] / off["peak_allocated_bytes"], 4),
                      "bit_identical": bool(torch.equal(loss0, loss1) and torch.equal(g0, g1))}))


if __name__ == "__main__":
    main()
