"""ego_headnorm_fwd / ego_headnorm_bwd - the per-head LayerNorm of q and k of the QK-norm family - against the fp64 restatement in
tests/_qknorm_ref.py, on operands addressed inside [rows, 3A] / [rows, 2A] buffers: values, saved statistics, untouched surroundings
(sentinels, bit for bit), special rows, accumulation, run-to-run reproducibility, refusals.

Tolerances are those tests/test_kernels_gpu.py::test_layernorm holds ego_layernorm_fwd / _bwd to against fp32 torch (the reference here
is fp64, which only removes reference error):
  y (bf16)    rel l2 < 4e-3    tests/test_kernels_gpu.py:620
  mean, rstd  rel l2 < 1e-5    tests/test_kernels_gpu.py:752 (test_layernorm_on_padded_rows)
  dx (bf16)   rel l2 < 4e-3    tests/test_kernels_gpu.py:631 (the bf16 copy of dx; tests/test_gelu_kernels_gpu.py:260 the same)
  dw          rel l2 < 1e-4    tests/test_kernels_gpu.py:632 (tests/test_gelu_kernels_gpu.py:261 the same)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _qknorm_ref as QR  # noqa: E402
from egom2p_amd import _lib as L  # noqa: E402
from egom2p_amd import ops  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
Y_TOL, STAT_TOL, DX_TOL, DW_TOL = 4e-3, 1e-5, 4e-3, 1e-4
BF16_MAX = float(torch.finfo(BF16).max)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _sentinel(n, gen):
    """n bf16 elements of seeded random BITS (NaN patterns included): compared through their int16 image"""
    return torch.randint(-32768, 32767, (n,), generator=gen, dtype=torch.int16).to(DEV).view(BF16)


def _bits(t):
    return t.view(torch.int16)


def _ptr(t, off):
    return t.data_ptr() + 2 * off


def _weight(gen):
    return (1.0 + 0.1 * torch.randn(64, generator=gen)).to(DEV)


def _outside(total, off, bs, rs, B, n, H):
    m = torch.ones(total, dtype=torch.bool, device=DEV)
    QR.head_view(m, off, bs, rs, B, n, H).fill_(False)
    return m


# (B, n, H, source: (elements, offset, sample stride, row stride), destination: the same)
A3, A6 = 3 * 64, 6 * 64
LAYOUTS = {
    "q slot of [rows, 3A]": (2, 70, 3, (140 * 3 * A3, 0, 70 * 3 * A3, 3 * A3), (140 * 3 * A3, 0, 70 * 3 * A3, 3 * A3)),
    "k slot of [rows, 3A] -> k half of [rows, 2A]": (2, 70, 3, (140 * 3 * A3, A3, 70 * 3 * A3, 3 * A3), (140 * 2 * A3, A3, 70 * 2 * A3, 2 * A3)),
    "one slice": (1, 1, 1, (64, 0, 64, 64), (64, 0, 64, 64)),
    "5 framing rows between samples": (3, 129, 6, (3 * 134 * 3 * A6 + 8, 8, 134 * 3 * A6, 3 * A6), (3 * 134 * 3 * A6 + 8, 8 + A6, 134 * 3 * A6, 3 * A6)),
    "k of a cross-attention kv [ctx rows, 2A] -> [ctx rows, A]": (2, 33, 6, (66 * 2 * A6, 0, 33 * 2 * A6, 2 * A6), (66 * A6, 0, 33 * A6, A6)),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_forward_against_fp64_and_leaves_everything_else_untouched(name):
    B, n, H, (ns, so, sbs, srs), (nd, do, dbs, drs) = LAYOUTS[name]
    gen = torch.Generator().manual_seed(len(name))
    src = torch.randn(ns, generator=gen).to(DEV).to(BF16)
    xv = QR.head_view(src, so, sbs, srs, B, n, H)
    special = B * n * H >= 3
    if special:
        xv[0, 0, 0] = 3.0                                                                    # constant: variance 0
        xv[B - 1, n // 2, H - 1] = (100.0 + 0.1 * torch.randn(64, generator=gen)).to(DEV).to(BF16)     # mean 100, std 0.1: cancellation
        sign = torch.where(torch.rand(64, generator=gen) < 0.5, -1.0, 1.0)
        xv[B - 1, n - 1, 0] = (sign * BF16_MAX).to(DEV).to(BF16)                             # bf16's largest magnitude, both signs
    src0 = src.clone()
    dst = _sentinel(nd, gen)
    dst0 = dst.clone()
    w = _weight(gen)
    S = B * n * H
    mean, rstd = torch.full((S + 16,), 7.0, device=DEV), torch.full((S + 16,), 7.0, device=DEV)
    ops.headnorm_fwd([(_ptr(src, so), sbs, srs, _ptr(dst, do), dbs, drs, w, mean, rstd)], B, n, H, eps=1e-6)
    torch.cuda.synchronize()
    y_ref, m_ref, r_ref = QR.headnorm_fwd(xv.cpu(), w.cpu())
    y = QR.head_view(dst, do, dbs, drs, B, n, H)
    assert bool(torch.isfinite(y.float()).all())
    err = dict(y=_rel(y, y_ref), mean=_rel(mean[:S].view(B, n, H), m_ref), rstd=_rel(rstd[:S].view(B, n, H), r_ref))
    print(name, err)
    assert err["y"] < Y_TOL and err["mean"] < STAT_TOL and err["rstd"] < STAT_TOL
    # bit for bit untouched: the whole source (raw q / k, the v slot, framing rows), the destination outside the slices, the statistics'
    # tails
    assert torch.equal(_bits(src), _bits(src0))
    out = _outside(nd, do, dbs, drs, B, n, H)
    assert torch.equal(_bits(dst)[out], _bits(dst0)[out])
    assert bool((mean[S:] == 7.0).all()) and bool((rstd[S:] == 7.0).all())
    if special:
        for what, idx in (("constant", (0, 0, 0)), ("mean 100, std 0.1", (B - 1, n // 2, H - 1)), ("bf16 max", (B - 1, n - 1, 0))):
            got, ref = y[idx].float().cpu().double(), y_ref[idx]
            s = (idx[0] * n + idx[1]) * H + idx[2]
            e = dict(y=_rel(got, ref), mean=abs(mean[s].item() - m_ref[idx].item()) / max(abs(m_ref[idx].item()), 1e-30),
                     rstd=abs(rstd[s].double().item() - r_ref[idx].item()) / r_ref[idx].item())
            print(name, what, e)
            assert bool(torch.isfinite(got).all()), what
            if what == "constant":
                assert not bool(got.any()) and mean[s].item() == 3.0          # x - mean is exactly 0: the output is 0, not 0 x inf
            else:
                assert e["y"] < Y_TOL, (what, e)
            assert e["mean"] < STAT_TOL and e["rstd"] < STAT_TOL, (what, e)


def _bwd_case(rows, H, two, seed):
    """q and k of a [rows, 3A] qkv buffer and their gradients in a [rows, 3A] gradient buffer (the v slots: sentinels)"""
    gen = torch.Generator().manual_seed(seed)
    A = H * 64
    x = torch.randn(rows * 3 * A, generator=gen).to(DEV).to(BF16)
    dy = torch.randn(rows * 3 * A, generator=gen).to(DEV).to(BF16)
    QR.head_view(dy, 2 * A, rows * 3 * A, 3 * A, 1, rows, H).copy_(QR.head_view(_sentinel(rows * 3 * A, gen), 2 * A, rows * 3 * A, 3 * A, 1, rows, H))
    ws = [_weight(gen) for _ in range(2)]
    S = rows * H
    st = torch.empty(4, S, device=DEV)
    nrm = torch.empty(rows * 2 * A, device=DEV, dtype=BF16)
    slots = (0, A) if two else (A,)
    fwd = [(_ptr(x, o), rows * 3 * A, 3 * A, _ptr(nrm, j * A), rows * 2 * A, 2 * A, ws[j], st[2 * j], st[2 * j + 1]) for j, o in enumerate(slots)]
    ops.headnorm_fwd(fwd, 1, rows, H)
    return A, x, dy, ws, st, slots


def _run_bwd(rows, H, A, x, dy, ws, st, slots, dws):
    g = dy.clone()
    sites = [(_ptr(x, o), rows * 3 * A, 3 * A, _ptr(g, o), rows * 3 * A, 3 * A, ws[j], st[2 * j], st[2 * j + 1], dws[j]) for j, o in enumerate(slots)]
    ops.headnorm_bwd(sites, 1, rows, H)
    torch.cuda.synchronize()
    return g


# 256 slices per workgroup and partial weight-gradient row: H = 2 -> 2, 254, 258 and 2000 slices (one slice pair; just under one
# workgroup; two slices into the second; eight workgroups, the last one partial); 70 rows of 3 heads: slices that straddle rows
@pytest.mark.parametrize("rows,H,two", [(1, 2, True), (127, 2, True), (129, 2, False), (1000, 2, True), (70, 3, False)])
def test_backward_against_fp64_accumulates_and_reproduces(rows, H, two):
    A, x, dy, ws, st, slots = _bwd_case(rows, H, two, seed=rows)
    dws = [torch.full((64,), 0.25, device=DEV) for _ in slots]
    g = _run_bwd(rows, H, A, x, dy, ws, st, slots, dws)
    touched = torch.zeros(rows * 3 * A, dtype=torch.bool, device=DEV)
    for j, o in enumerate(slots):
        view = lambda t: QR.head_view(t, o, rows * 3 * A, 3 * A, 1, rows, H)      # noqa: E731
        dx_ref, dw_ref = QR.headnorm_bwd(view(dy).cpu(), view(x).cpu(), ws[j].cpu())
        e = dict(dx=_rel(view(g), dx_ref), dw=_rel(dws[j] - 0.25, dw_ref))       # dw accumulates onto its non-zero start
        print(rows, H, "operand", j, e)
        assert e["dx"] < DX_TOL and e["dw"] < DW_TOL, e
        # element-wise: every dx within one bf16 rounding of the fp64 value (half an ulp: at most 2^-8 of the slice's largest |dx| for
        # its largest element, less for the others) plus the fp32 arithmetic in front of the rounding (a few 2^-24 per operation over
        # ~10 operations and two 64-term sums: 2^-14 is a generous cap, 64 times finer than the rounding)
        lim = dx_ref.abs().amax(-1, keepdim=True) * (2.0 ** -8 + 2.0 ** -14) + 1e-30
        assert bool(((view(g).float().cpu().double() - dx_ref).abs() <= lim).all())
        view(touched).fill_(True)
    # the v slot (and, with one operand, the other slot) of the gradient buffer is bit for bit what it was
    assert torch.equal(_bits(g)[~touched], _bits(dy)[~touched])
    # a second run from the same inputs: bitwise equal dx and dw
    dws2 = [torch.full((64,), 0.25, device=DEV) for _ in slots]
    g2 = _run_bwd(rows, H, A, x, dy, ws, st, slots, dws2)
    assert torch.equal(_bits(g), _bits(g2))
    for a, b in zip(dws, dws2):
        assert torch.equal(a, b)


def test_two_operand_launch_equals_two_single_launches():
    rows, H = 300, 2
    A, x, dy, ws, st, slots = _bwd_case(rows, H, True, seed=9)
    dws = [torch.zeros(64, device=DEV) for _ in slots]
    g = _run_bwd(rows, H, A, x, dy, ws, st, slots, dws)
    g1 = dy.clone()
    for j, o in enumerate(slots):
        dw1 = torch.zeros(64, device=DEV)
        ops.headnorm_bwd([(_ptr(x, o), rows * 3 * A, 3 * A, _ptr(g1, o), rows * 3 * A, 3 * A, ws[j], st[2 * j], st[2 * j + 1], dw1)], 1, rows, H)
        assert torch.equal(dw1, dws[j])
    assert torch.equal(_bits(g), _bits(g1))


def test_refusals():
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(8 * 256, generator=gen).to(DEV).to(BF16)
    y = torch.zeros_like(x)
    w, mean, rstd, dw = _weight(gen), torch.zeros(64, device=DEV), torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    y0 = y.clone()
    for hd in (32, 96, 128):                              # only heads of 64
        with pytest.raises(L.EgoHipError, match="bad arguments"):
            ops.headnorm_fwd([(_ptr(x, 0), 8 * 128, 128, _ptr(y, 0), 8 * 128, 128, w, mean, rstd)], 1, 8, 2, hd=hd)
        with pytest.raises(L.EgoHipError, match="bad arguments"):
            ops.headnorm_bwd([(_ptr(x, 0), 8 * 128, 128, _ptr(y, 0), 8 * 128, 128, w, mean, rstd, dw)], 1, 8, 2, hd=hd)
    for bad in ((_ptr(x, 4), 8 * 128, 128), (_ptr(x, 0), 8 * 128, 132), (_ptr(x, 0), 8 * 128, 64)):      # alignment; rows narrower than H heads
        with pytest.raises(L.EgoHipError, match="bad arguments"):
            ops.headnorm_fwd([bad + (_ptr(y, 0), 8 * 128, 128, w, mean, rstd)], 1, 8, 2)
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and not bool(dw.any())
