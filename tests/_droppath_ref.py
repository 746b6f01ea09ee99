"""Host restatements for the drop-path tests: the draw in Python integers (splitmix64, the generator of egom2p_amd/synth.py and
csrc/common.h), the per-layer rates by the reference's rule (egom2p_model.py:137-154), and the row kernels' arithmetic in torch."""
import struct

import torch

M64 = (1 << 64) - 1


def splitmix(key: int, i: int) -> int:
    x = (i * 0x9E3779B97F4A7C15 + key) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def f32(v: float) -> float:
    """the fp32 nearest to the double v, as a double"""
    return struct.unpack("f", struct.pack("f", v))[0]


def threshold(keep_prob: float) -> int:
    """floor(fp32(keep_prob) * 2^24): exact (a power-of-two scale of a 24-bit significand)"""
    return int(f32(keep_prob) * 16777216.0)


def draw(keep_probs, B: int, seed: int, counter: int):
    """keep[s][b] of ego_droppath_draw: top 24 bits of splitmix(splitmix(splitmix(seed, counter), s), b) < floor(keep_prob[s] * 2^24)"""
    base = splitmix(seed & M64, counter & M64)
    return [[1 if (splitmix(splitmix(base, s), b) >> 40) < threshold(kp) else 0 for b in range(B)] for s, kp in enumerate(keep_probs)]


def rates(r_enc: float, r_dec: float, Le: int, Ld: int, shared: bool):
    """the reference's per-layer rates: fp32 `.item()` values of its linspaces"""
    if shared:
        return ([v.item() for v in torch.linspace(0, r_enc, Le + Ld)][:Le], [v.item() for v in torch.linspace(0, r_dec, Le + Ld)][Le:])
    return [v.item() for v in torch.linspace(0, r_enc, Le)], [v.item() for v in torch.linspace(0, r_dec, Ld)]


def keep_prob(rate: float) -> float:
    """fp32(1 - rate.item()): what the reference's bf16 `x.div(keep_prob)` divides by (the scalar enters the fp32 op math)"""
    return f32(1.0 - rate)


def site_table(r_enc, r_dec):
    """(site name, keep_prob) of every site with a non-zero rate, in forward order"""
    out = []
    for kind, rs, subs in (("encoder", r_enc, ("attn", "mlp")), ("decoder", r_dec, ("self_attn", "cross_attn", "mlp"))):
        for i, r in enumerate(rs):
            if r > 0:
                out += [(f"{kind}.{i}.{s}", keep_prob(r)) for s in subs]
    return out


def scaled(branch: torch.Tensor, keep_rows: torch.Tensor, kp: float) -> torch.Tensor:
    """bf16 [rows, width]: keep ? bf16(float(branch) / kp) : 0 (dropped rows are not read: they may hold NaN)"""
    kpt = torch.tensor(kp, dtype=torch.float32, device=branch.device)
    return torch.where(keep_rows[:, None], (branch.float() / kpt).bfloat16(), torch.zeros((), dtype=torch.bfloat16, device=branch.device))


def resid(R: torch.Tensor, branch: torch.Tensor, keep_rows: torch.Tensor, kp: float) -> torch.Tensor:
    return R + scaled(branch, keep_rows, kp).float()
