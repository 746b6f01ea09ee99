"""`ego_adamw_step` against its gated twin at the ego-b flat size (`engine.P.numel()`), for `rocprofv3 --kernel-trace --stats`
with the program after `--`:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 tools/adamw_gate_bench.py
    python3 tools/adamw_gate_bench.py --summarize <dir> [out.txt]

One process, three phases of 5 warm-up + 20 measured launches each over the same buffers:
  plain        ops.adamw_step                       (adamw_kernel)
  twin         ops.adamw_gate + ops.adamw_step_gated, gate open      (adamw_gate_kernel + adamw_gated_kernel)
  gated_zero   the same with the gate shut and zero_grad: writes nothing but the cleared gradients
The statistics file merges the two phases of adamw_gated_kernel; --summarize splits them by dispatch order from the per-dispatch
trace and states the bar: the twin's mean against the plain kernel's own min-max spread over its 20 launches in that run.
"""
from __future__ import annotations

import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, RUNS = 5, 20


def run():
    import torch
    from egom2p_amd import ops
    from egom2p_amd.config import MODEL_CFGS
    from egom2p_amd.engine import Engine
    eng = Engine(MODEL_CFGS["egom2p_base_12e_12d_swiglu_nobias"], "cuda:0", max_batch=1, n_enc=64, n_dec=64)
    n = eng.P.numel()
    p, g = eng.P, eng.G
    p.normal_(); g.normal_()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    sq = torch.zeros(1, device=p.device, dtype=torch.float64)
    gate = torch.zeros(ops.GATE_WORDS, device=p.device, dtype=torch.int32)
    ops.grad_sqnorm(g, sq)
    torch.cuda.synchronize()
    for k in range(WARM + RUNS):
        ops.adamw_step(p, g, m, v, 1e-4, 0.05, k + 1, max_norm=1.0, sqnorm=sq, zero_grad=False)
    torch.cuda.synchronize()
    for k in range(WARM + RUNS):
        ops.adamw_gate(sq, gate, skip_norm=0.0, skip_nonfinite=True)
        ops.adamw_step_gated(p, g, m, v, 1e-4, 0.05, k + 1, gate, max_norm=1.0, sqnorm=sq, zero_grad=False)
    torch.cuda.synchronize()
    for k in range(WARM + RUNS):
        ops.adamw_gate(sq, gate, skip_norm=1e-9, skip_nonfinite=True)
        ops.adamw_step_gated(p, g, m, v, 1e-4, 0.05, k + 1, gate, max_norm=1.0, sqnorm=sq, zero_grad=True)
        g.normal_()
    torch.cuda.synchronize()
    print(f"adamw_gate_bench: n = {n} floats, gate block {gate.tolist()}", flush=True)


def summarize(d, out=None):
    path = next(iter(sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))), None)
    if path is None:
        raise SystemExit(f"no *kernel_trace.csv under {d}")
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = {"adamw_kernel": [], "adamw_gated_kernel": [], "adamw_gate_kernel": []}
    for r in rows:
        for k in dur:
            if k in r["Kernel_Name"]:                              # (no name is a substring of another)
                dur[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    per = WARM + RUNS
    assert len(dur["adamw_kernel"]) == per and len(dur["adamw_gated_kernel"]) == 2 * per and len(dur["adamw_gate_kernel"]) == 2 * per, \
        {k: len(x) for k, x in dur.items()}
    plain = dur["adamw_kernel"][WARM:]
    twin = dur["adamw_gated_kernel"][WARM:per]
    gz = dur["adamw_gated_kernel"][per + WARM:]
    gt = dur["adamw_gate_kernel"][WARM:per] + dur["adamw_gate_kernel"][per + WARM:]
    mean = lambda x: sum(x) / len(x)
    lines = [f"microseconds per launch, {RUNS} launches after {WARM} warm-up (rocprofv3 --kernel-trace)",
             f"plain  adamw_kernel                 mean {mean(plain):9.1f}  min {min(plain):9.1f}  max {max(plain):9.1f}",
             f"twin   adamw_gated_kernel (open)    mean {mean(twin):9.1f}  min {min(twin):9.1f}  max {max(twin):9.1f}",
             f"gated  adamw_gated_kernel (shut, zero_grad) mean {mean(gz):9.1f}  min {min(gz):9.1f}  max {max(gz):9.1f}",
             f"gate   adamw_gate_kernel            mean {mean(gt):9.2f}  min {min(gt):9.2f}  max {max(gt):9.2f}",
             f"bar: twin mean no higher than the plain kernel's max (its min-max spread): {mean(twin) <= max(plain)}; a gated-path call adds the gate launch "
             f"(twin mean - plain mean = {mean(twin) - mean(plain):+.1f} us, {100.0 * (mean(twin) / mean(plain) - 1.0):+.2f} %)"]
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        run()
