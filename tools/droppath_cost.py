"""What stochastic depth costs: forward + backward of one micro-batch of the flagship model (ego-b, N = M = 2048, the benchmark's
micro-batch) with drop-path rates 0 and `--rate` (encoder and decoder, per-stack linspace: 55 active sites at 12 + 12 layers), on the
same device, back to back.  A site that drops paths writes its branch as bf16 and adds it in a pass of its own (ego_droppath_resid)
instead of inside the GEMM epilogue, and scales the branch's upstream gradient once (ego_droppath_scale): extra HBM traffic, no FLOPs.

    python tools/droppath_cost.py [--micro-batch 64] [--rate 0.1] [--iters 5]

Prints one JSON line: milliseconds per forward + backward at either rate, their ratio, and the time of the three kernels alone."""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egom2p_amd import ops, synth  # noqa: E402
from egom2p_amd.config import MODEL_CFGS  # noqa: E402
from egom2p_amd.engine import Engine  # noqa: E402


def time_fwd_bwd(cfg, mb, mbs, iters, warmup=2):
    eng = Engine(cfg, "cuda:0", max_batch=mb, n_enc=2048, n_dec=2048)
    eng.init_random(seed=0)
    names = [m.name for m in cfg.mods]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(warmup + iters):
        if i == warmup:
            ev[0].record()
        eng.forward(mbs[i % len(mbs)], dec_order=names, loss_grad=1.0, training=True)
        eng.backward(1.0)
    ev[1].record()
    torch.cuda.synchronize()
    loss = float(eng.loss_out[0].item())
    n_sites = len(eng.dp_sites)
    return ev[0].elapsed_time(ev[1]) / iters, loss, n_sites


def time_kernels(rows, D, rps, B, kp, iters=20):
    """the residual add and the gradient scale alone at the model's row count: ms per launch and achieved GB/s (every sample kept)"""
    R = torch.randn(rows, D, device="cuda")
    br = torch.randn(rows, D, device="cuda").bfloat16()
    out, dst = torch.empty_like(R), torch.empty_like(br)
    keep = torch.ones(B, dtype=torch.uint8, device="cuda")
    res = {}
    for name, fn, nbytes in (("resid", lambda: ops.droppath_resid(R, br, out, keep, rows, rps, D, kp), 10.0),
                             ("scale", lambda: ops.droppath_scale(br, dst, keep, rows, rps, D, kp), 4.0)):
        fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(iters):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / iters
        res[name] = {"ms": round(ms, 4), "gbs": round(rows * D * nbytes / ms / 1e6, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="egom2p_base_12e_12d_swiglu_nobias")
    ap.add_argument("--micro-batch", type=int, default=64)
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    cfg = MODEL_CFGS[args.model]
    mb = args.micro_batch
    mbs = [synth.make_clip_batch_device(cfg, mb, synth.CANONICAL_BUDGETS, seed=100, sample_offset=i * mb, device="cuda:0") for i in range(2)]
    ms0, loss0, n0 = time_fwd_bwd(cfg, mb, mbs, args.iters)
    torch.cuda.empty_cache()
    ms1, loss1, n1 = time_fwd_bwd(dataclasses.replace(cfg, drop_path_rate_encoder=args.rate, drop_path_rate_decoder=args.rate), mb, mbs, args.iters)
    torch.cuda.empty_cache()
    kern = time_kernels(mb * 2048, cfg.dim, 2048, mb, 1.0 - args.rate)
    print(json.dumps({"model": args.model, "micro_batch": mb, "rate": args.rate, "active_sites": n1, "fwd_bwd_ms_rate0": round(ms0, 2),
                      "fwd_bwd_ms_rate": round(ms1, 2), "ratio": round(ms1 / ms0, 4), "extra_ms": round(ms1 - ms0, 2),
                      "loss_rate0": loss0, "loss_rate": loss1, "kernels": kern}))
    assert n0 == 0


if __name__ == "__main__":
    main()
