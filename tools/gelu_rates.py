"""Launches of the GELU family's row kernels beside their bias-free siblings at ego-b shapes (rows = 64 x 2048, F = 3072 for the gate
kernels, D = 768 for LayerNorm), for a `rocprofv3 --kernel-trace --stats -- python tools/gelu_rates.py` run: the per-kernel averages
of its stats table are the per-launch times.  The siblings move the same bytes per output element up to the
gate's second input: swiglu forward reads 4 B and writes 2 B per h element (GELU: 2 + 2), backward 6 + 4 (GELU: 4 + 2)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egom2p_amd import ops  # noqa: E402

DEV, BF16 = "cuda", torch.bfloat16
rows, F, D, reps = 64 * 2048, 3072, 768, 10
u = torch.randn(rows, F, device=DEV).to(BF16)
ab = torch.randn(rows, 2 * F, device=DEV).to(BF16)
dh = torch.randn(rows, F, device=DEV).to(BF16)
h, du, dab = torch.empty_like(u), torch.empty_like(u), torch.empty_like(ab)
x = torch.randn(rows, D, device=DEV)
w, b = torch.rand(D, device=DEV) + 0.5, torch.randn(D, device=DEV)
y, dy = torch.empty(rows, D, device=DEV, dtype=BF16), torch.randn(rows, D, device=DEV).to(BF16)
mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
dx, dxb = torch.empty(rows, D, device=DEV), torch.empty(rows, D, device=DEV, dtype=BF16)
dw, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
for _ in range(reps):
    ops.gelu_fwd(u, h, rows, F)
    ops.gelu_bwd(u, dh, du, rows, F)
    ops.swiglu_fwd(ab, h, rows, F)
    ops.swiglu_bwd(ab, dh, dab, rows, F)
    ops.layernorm_fwd(x, w, y, mean, rstd)
    ops.layernorm_bwd(dy, x, mean, rstd, w, dx, dw, dx_in=dx, dx_bf16=dxb)
    ops.layernorm_fwd(x, w, y, mean, rstd, b=b)
    ops.layernorm_bwd(dy, x, mean, rstd, w, dx, dw, dx_in=dx, dx_bf16=dxb, db=db)
torch.cuda.synchronize()
print("done")
