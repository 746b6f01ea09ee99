"""fp64 restatement of the per-head LayerNorm of the QK-norm family (NormAttention / NormCrossAttention, egom2p_utils.py:247-332: a
bias-free LayerNorm over every head's 64 values, one [64] weight shared by the heads) and of its backward, for the kernel tests.

The operand is a strided view [B, n, H, 64] of a 1-D buffer: element 0 of (b, r, h) at off + b * bs + r * rs + h * 64."""
import torch

HD = 64


def head_view(buf, off, bs, rs, B, n, H):
    """[B, n, H, 64] view of the 1-D tensor `buf` (any dtype) addressed like an attention operand"""
    return buf.as_strided((B, n, H, HD), (bs, rs, HD, 1), off)


def headnorm_fwd(x, w, eps=1e-6):
    """x [..., 64] -> (y, mean, rstd) in fp64"""
    x, w = x.double(), w.double()
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    return (x - mean) * rstd * w, mean[..., 0], rstd[..., 0]


def headnorm_bwd(dy, x, w, eps=1e-6):
    """(dx [..., 64], dw [64]) in fp64: dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy w; dw = sum over slices of dy xhat"""
    dy, x, w = dy.double(), x.double(), w.double()
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xh = (x - mean) * rstd
    g = dy * w
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).reshape(-1, HD).sum(0)
