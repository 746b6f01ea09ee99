"""Kernels of the GELU / biased family (the `*_gelu` registrations, egom2p_model.py:881-978) on the GPU: ego_gelu_fwd / ego_gelu_bwd,
the EGO_EPI_BIAS_BF16 epilogue of ego_gemm_nt_bf16, ego_layernorm_bias_fwd / _bwd and ego_bias_grad beyond 2048 columns.

Where a result is a deterministic rounding of exact arithmetic (the GEMM epilogue and the column sums on small integers) the check
is torch.equal against fp64.  GELU is compared with fp64 under a bound built from the number format (half a bf16 ulp) plus the excess
torch's own CPU bf16 kernel shows over that bound, doubled - see `_gelu_allowance`.  The LayerNorm tolerances are the ones
tests/test_kernels_gpu.py states for the bias-free kernel."""
import math

import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

import _gemm_exact as X  # noqa: E402
import test_gemm_exact_gpu as TG  # noqa: E402
from egom2p_amd import _lib as L  # noqa: E402
from egom2p_amd import ops  # noqa: E402

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


# ---------------------------------------------------------------------------------------------------------------- GELU
def _all_finite_bf16():
    """every finite bf16 bit pattern once, in bit order (65,280 = 8 x 8160 values), on the CPU"""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[((bits >> 7) & 0xFF) != 0xFF]
    assert bits.numel() == 65280
    return bits.to(torch.int16).view(BF16)


def _ulp_bf16(g):
    """spacing of bf16 around the fp64 value g (8 significant bits; 2^-133 in the subnormal range)"""
    e = torch.floor(torch.log2(g.abs().clamp_min(2.0 ** -140))).clamp_min(-126.0)
    return torch.exp2(e - 7.0)


def _gelu64(u):
    x = u.double()
    return 0.5 * x * torch.special.erfc(-x * math.sqrt(0.5))          # x Phi(x) without the cancellation of 1 + erf in the tail


def _dgelu64(u):
    x = u.double()
    return 0.5 * torch.special.erfc(-x * math.sqrt(0.5)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _excess(h, want):
    """how far |h - want| goes beyond half a bf16 ulp of the fp64 value (0 for a correctly rounded result)"""
    return ((h.double() - want).abs() - 0.5 * _ulp_bf16(want)).clamp_min(0.0)


def _gelu_allowance(cpu_result, want):
    """A = twice the largest excess of torch's own CPU bf16 kernel over the half-ulp bound: both kernels form 1 + erf in fp32, which
    cancels in the negative tail, through two fp32 erf implementations of unknown relative quality - hence the factor two."""
    exc = _excess(cpu_result, want)
    # (torch's CPU kernels multiply by (1 + erf) before the 0.5 and overflow to inf from 2^127 up: no yardstick there - the kernel
    #  under test is still held to the bound at those values, where x * 1 is exact)
    return 2.0 * float(exc[torch.isfinite(cpu_result.float())].max())


@pytest.fixture(scope="module")
def gelu_case():
    u = _all_finite_bf16()
    want = _gelu64(u)
    cpu_bf16 = Fn.gelu(u)                                   # torch's own bf16 kernel
    cpu_f32 = Fn.gelu(u.float()).to(BF16)                   # fp32 math, rounded once
    return dict(u=u, ud=u.to(DEV), want=want, A=_gelu_allowance(cpu_bf16, want), cpu_f32=cpu_f32)


@pytest.mark.parametrize("shape", [(1, 65280), (255, 256)])
def test_gelu_forward_over_every_finite_bf16(gelu_case, shape):
    c = gelu_case
    rows, F = shape
    u = c["ud"].reshape(rows, F).contiguous()
    h = torch.full((rows, F), 7.0, device=DEV, dtype=BF16)
    ops.gelu_fwd(u, h, rows, F)
    torch.cuda.synchronize()
    hc = h.reshape(-1).cpu()
    exc = _excess(hc, c["want"])
    n_cpu_off = int((_excess(Fn.gelu(c["u"]), c["want"]) > 0).sum())
    print(f"gelu fwd {shape}: allowance A = {c['A']:.3e} (CPU bf16 kernel beyond half an ulp in {n_cpu_off} values), kernel's largest excess "
          f"{float(exc.max()):.3e}, values beyond half an ulp {int((exc > 0).sum())}")
    assert torch.isfinite(hc.float()).all()
    assert float(exc.max()) <= c["A"], (float(exc.max()), c["A"], int(exc.argmax()))
    # |u| <= 3: the bits of fp32 GELU rounded once.  Two fp32 evaluations can only round differently where the exact value sits
    # within their errors of a bf16 rounding boundary (the midpoint of two neighbouring bf16 values).  The CPU's fp32 result against
    # fp64 measures that error: eps(u) = its largest absolute error over the 129 bf16 values around u (one binade of neighbours, so
    # that a value the CPU happens to hit exactly still gets its neighbourhood's error).  A value is at risk when the fp64 result
    # lies within 2 eps(u) of a boundary - one eps per implementation; the share at risk is the allowance, never more than 1 %.
    near = c["u"].float().abs() <= 3.0
    err = (Fn.gelu(c["u"].float()).double() - c["want"]).abs()
    eps = Fn.max_pool1d(err[None, None], 129, stride=1, padding=64)[0, 0]
    ulp = _ulp_bf16(c["want"])
    dist = (((c["want"].abs() / ulp) % 1.0) - 0.5).abs() * ulp
    at_risk = near & (dist <= 2.0 * eps)
    allowed = min(float(at_risk.sum()) / float(near.sum()), 0.01)
    differ = hc.view(torch.int16) != c["cpu_f32"].view(torch.int16)
    share = float((differ & near).sum()) / float(near.sum())
    print(f"gelu fwd {shape}: |u| <= 3: {int(near.sum())} values, {int((differ & near).sum())} differ from CPU fp32 GELU (share {share:.5f}; "
          f"at risk {int(at_risk.sum())}, allowed share {allowed:.5f})")
    assert share <= allowed, (share, allowed)


def test_gelu_forward_special_values():
    vals = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 3.3895313892515355e38, -3.3895313892515355e38],
                        dtype=F32).to(BF16)
    u = torch.zeros(1, 8, dtype=BF16)
    u[0, :7] = vals
    u.view(torch.int16)[0, 7] = 0x7FC1                      # a NaN with a payload
    h = torch.empty(1, 8, device=DEV, dtype=BF16)
    ops.gelu_fwd(u.to(DEV), h, 1, 8)
    h = h.cpu().float()[0]
    assert h[0] == 0 and h[1] == 0
    assert h[2] == float("inf")
    assert h[3] == 0                                        # -0 or 0
    assert torch.isnan(h[4]) and torch.isnan(h[7])
    assert h[5] == vals[5].float() and h[6] == 0            # the largest finite values: x and -0


@pytest.mark.parametrize("seeded", [False, True])
def test_gelu_backward_over_every_finite_bf16(gelu_case, seeded):
    c = gelu_case
    n = c["u"].numel()
    if seeded:
        g = torch.Generator().manual_seed(1234)
        dh = torch.randn(n, generator=g).to(BF16)
    else:
        dh = torch.ones(n, dtype=BF16)
    want = dh.double() * _dgelu64(c["u"])
    uc = c["u"].clone().requires_grad_(True)
    Fn.gelu(uc).backward(dh)                                # torch's own bf16 backward kernel
    A = _gelu_allowance(uc.grad, want)
    du = torch.full((255, 256), 7.0, device=DEV, dtype=BF16)
    ops.gelu_bwd(c["ud"].reshape(255, 256).contiguous(), dh.to(DEV).reshape(255, 256).contiguous(), du, 255, 256)
    duc = du.reshape(-1).cpu()
    exc = _excess(duc, want)
    print(f"gelu bwd seeded={seeded}: allowance A = {A:.3e}, kernel's largest excess {float(exc.max()):.3e}, beyond half an ulp "
          f"{int((exc > 0).sum())} values")
    assert torch.isfinite(duc.float()).all()
    assert float(exc.max()) <= A, (float(exc.max()), A, int(exc.argmax()))


def test_gelu_ragged_rows_and_pitches():
    """rows = 3, F = 8 x 37 in rows of a larger pitch: the grid-stride loop's tail, and nothing outside [rows, F) is written"""
    rows, F, ld = 3, 8 * 37, 8 * 37 + 24
    g = torch.Generator().manual_seed(7)
    u = (torch.randn(rows, F, generator=g) * 2).to(BF16).to(DEV)
    dh = torch.randn(rows, F, generator=g).to(BF16).to(DEV)
    h0, du0 = torch.empty(rows, F, device=DEV, dtype=BF16), torch.empty(rows, F, device=DEV, dtype=BF16)
    ops.gelu_fwd(u, h0, rows, F)
    ops.gelu_bwd(u, dh, du0, rows, F)
    up, dhp = X.pitched(u, ld, float("nan")), X.pitched(dh, ld + 8, float("nan"))
    hbuf = torch.full((rows + 1, ld), TG.SENT, device=DEV, dtype=BF16)
    dbuf = torch.full((rows + 1, ld + 16), TG.SENT, device=DEV, dtype=BF16)
    ops.gelu_fwd(up, hbuf[:, :F], rows, F)
    ops.gelu_bwd(up, dhp, dbuf[:, :F], rows, F)
    torch.cuda.synchronize()
    exp_h = torch.full_like(hbuf, TG.SENT); exp_h[:rows, :F] = h0
    exp_d = torch.full_like(dbuf, TG.SENT); exp_d[:rows, :F] = du0
    assert torch.equal(hbuf.view(torch.int16), exp_h.view(torch.int16))
    assert torch.equal(dbuf.view(torch.int16), exp_d.view(torch.int16))
    assert _rel(h0.float(), _gelu64(u.cpu()).to(DEV)) < 4e-3
    assert _rel(du0.float(), (dh.cpu().double() * _dgelu64(u.cpu())).to(DEV)) < 4e-3
    with pytest.raises(L.EgoHipError):
        ops.gelu_fwd(u[:, :F - 4], h0, rows, F - 4)                     # F % 8


# ---------------------------------------------------------------------------------------------------------------- EGO_EPI_BIAS_BF16
def _want_bias_bf16(p):
    """bf16(acc + bias): the sum is an integer below 2^24, exact in fp32, and rounded once"""
    return (p.acc.double() + p.bias.double()[None, :]).float().to(BF16)


@pytest.mark.parametrize("M,N,K,branch", [
    (1707, 768, 128, "narrow, 84 tiles <= 100: 64 x 64 tiles"),
    (2181, 768, 128, "narrow, 108 tiles in 101..520: 128 x 64 tiles"),
    (1707, 2304, 128, "wide bf16, 252 tiles <= 330: 128 x 64 tiles"),
    (8320, 1024, 128, "520 tiles of 128, 132 of 256: 256 x 256 tiles"),
    (11141, 768, 64, "narrow, 528 tiles > 520 and K < 128: the persistent 128 x 128 kernel"),
    (257, 328, 192, "ragged last row tile, N = 8 x 41"),
])
def test_bias_bf16_epilogue_exact(M, N, K, branch):
    p = TG.nt_problem(M, N, K)
    want = _want_bias_bf16(p)
    with TG.family("default"):
        exp = TG.sentinel(M + 2, N + 8, BF16)
        exp[:M, :N] = want
        buf = TG.sentinel(M + 2, N + 8, BF16)
        ops.gemm_nt(p.A, p.B, buf[:, :N], M, N, K, L.EPI_BIAS_BF16, bias=p.bias)
        TG.assert_exact(buf, exp, p.acc, what=f"EPI_BIAS_BF16 ({branch}) M={M} N={N} K={K}")
        # a NULL bias is refused and nothing is written
        buf2 = TG.sentinel(M + 2, N + 8, BF16)
        with pytest.raises(L.EgoHipError):
            ops.gemm_nt(p.A, p.B, buf2[:, :N], M, N, K, L.EPI_BIAS_BF16, bias=None)
        torch.cuda.synchronize()
        assert torch.equal(buf2, TG.sentinel(M + 2, N + 8, BF16))
        # epilogue 3 (and the plain bf16 one) on the same operands: their old results
        TG.run_nt(p, M, epis=(L.EPI_BF16, L.EPI_BIAS_RESID), tag="beside EPI_BIAS_BF16")


@pytest.mark.parametrize("fam", ["t128", "t64", "t128x64", "t128x128", "nt256"])
def test_bias_bf16_epilogue_every_family(fam):
    """the same epilogue forced onto every NT tile family, on a shape with ragged row and column tiles"""
    M, N, K = 300, 1152, 320
    p = TG.nt_problem(M, N, K)
    exp = TG.sentinel(M + 2, N + 8, BF16)
    exp[:M, :N] = _want_bias_bf16(p)
    buf = TG.sentinel(M + 2, N + 8, BF16)
    with TG.family(fam):
        ops.gemm_nt(p.A, p.B, buf[:, :N], M, N, K, L.EPI_BIAS_BF16, bias=p.bias)
    TG.assert_exact(buf, exp, p.acc, what=f"EPI_BIAS_BF16 {fam}")


# ---------------------------------------------------------------------------------------------------------------- biased LayerNorm
@pytest.mark.parametrize("rows,D,ld", [(300, 384, 384), (77, 1020, 1024), (1, 768, 768)])
def test_layernorm_with_bias(rows, D, ld):
    """ego_layernorm_bias_fwd / _bwd against fp32 torch: y, dx, dw, db; out_row with a dropped row, dx_in accumulation, pad
    columns written as zeros, two runs bit for bit.  Tolerances: tests/test_kernels_gpu.py test_layernorm / _on_padded_rows
    (4e-3 for bf16 outputs, 1e-4 for dx on padded rows and 1e-5 otherwise, 1e-4 for dw - and db, a plainer sum, the same)."""
    g = torch.Generator(device=DEV).manual_seed(100 + rows)
    x = torch.zeros(rows, ld, device=DEV); x[:, :D] = torch.randn(rows, D, device=DEV, generator=g) * 2 + 0.3
    w = torch.zeros(ld, device=DEV); w[:D] = torch.rand(D, device=DEV, generator=g) + 0.5
    b = torch.zeros(ld, device=DEV); b[:D] = torch.randn(D, device=DEV, generator=g) * 0.5
    perm = torch.randperm(rows, device=DEV, generator=g).int()
    if rows > 3:
        perm[3] = -1
    keep = perm >= 0
    xr, wr, br = x[:, :D].clone().requires_grad_(True), w[:D].clone().requires_grad_(True), b[:D].clone().requires_grad_(True)
    ref = Fn.layer_norm(xr, (D,), wr, br, 1e-6)
    dy = torch.zeros(rows, ld, device=DEV); dy[:, :D] = torch.randn(rows, D, device=DEV, generator=g)
    dy = dy.to(BF16)                                              # stored in the permuted row order
    dy_rows = torch.zeros(rows, D, device=DEV)
    dy_rows[keep] = dy[perm[keep].long(), :D].float()
    ref.backward(dy_rows)
    dx_in = torch.zeros(rows, ld, device=DEV); dx_in[:, :D] = torch.randn(rows, D, device=DEV, generator=g)
    outs = []
    for _ in range(2):
        y = torch.full((rows, ld), 9.0, device=DEV, dtype=BF16)
        mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
        ops.layernorm_fwd(x, w, y, mean, rstd, out_row=perm, eps=1e-6, width=D, b=b)
        dx = torch.full((rows, ld), 9.0, device=DEV)
        dxb = torch.full((rows, ld), 9.0, device=DEV, dtype=BF16)
        dw, db = torch.zeros(ld, device=DEV), torch.zeros(ld, device=DEV)
        ops.layernorm_bwd(dy, x, mean, rstd, w, dx, dw, dx_in=dx_in, dx_bf16=dxb, dy_row=perm, width=D, db=db)
        outs.append((y, mean, rstd, dx, dxb, dw, db))
    torch.cuda.synchronize()
    y, mean, rstd, dx, dxb, dw, db = outs[0]
    rows_out = perm[keep].long()
    e = dict(y=_rel(y[rows_out, :D].float(), ref[keep]), mean=_rel(mean, xr.mean(-1)), dx=_rel(dx[:, :D], xr.grad + dx_in[:, :D]),
             dxb=_rel(dxb[:, :D].float(), xr.grad + dx_in[:, :D]), dw=_rel(dw[:D], wr.grad), db=_rel(db[:D], br.grad))
    print(f"biased LayerNorm rows={rows} D={D} ld={ld}:", {k: f"{v:.2e}" for k, v in e.items()})
    assert e["y"] < 4e-3 and e["mean"] < 1e-5
    assert e["dx"] < (1e-4 if ld != D else 1e-5) and e["dxb"] < 4e-3
    assert e["dw"] < 1e-4 and e["db"] < 1e-4
    if ld != D:                                                   # pad columns: zeros in y, dx and both parameter gradients
        assert not bool(y[rows_out, D:].any()) and not bool(dx[:, D:].any()) and not bool(dxb[:, D:].any())
        assert not bool(dw[D:].any()) and not bool(db[D:].any())
    if rows > 3:                                                  # the dropped row: nothing written for it (row 3 has no output row)
        written = torch.zeros(rows, dtype=torch.bool, device=DEV); written[rows_out] = True
        assert bool((y[~written].float() == 9.0).all())
    # accumulation: db adds to what is there, like dw
    dw2, db2 = torch.full((ld,), 2.0, device=DEV), torch.full((ld,), 3.0, device=DEV)
    ops.layernorm_bwd(dy, x, mean, rstd, w, torch.empty_like(dx), dw2, dx_in=None, dy_row=perm, width=D, db=db2)
    assert torch.equal(dw2[:D], 2.0 + dw[:D]) and torch.equal(db2[:D], 3.0 + db[:D])
    for a, c in zip(outs[0], outs[1]):
        assert torch.equal(a.view(torch.int16) if a.dtype == BF16 else a, c.view(torch.int16) if c.dtype == BF16 else c)
    # the bias-free entry on the same input: same statistics, and y moves by exactly the bias path
    y0 = torch.zeros(rows, ld, device=DEV, dtype=BF16)
    m0, r0 = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    ops.layernorm_fwd(x, w, y0, m0, r0, out_row=perm, eps=1e-6, width=D)
    assert torch.equal(m0, mean) and torch.equal(r0, rstd)
    assert not torch.equal(y0[rows_out, :D], y[rows_out, :D])


# ---------------------------------------------------------------------------------------------------------------- ego_bias_grad
@pytest.mark.parametrize("D", [2304, 3072, 8192, 768])
def test_bias_grad_wide_exact(D):
    """column sums of integer-valued bf16 (|g| <= 4, 300 rows: every partial sum an integer far below 2^24) are exact in any order"""
    rows = 300
    g = X.ints((rows, D), X.OPERAND_LO, X.OPERAND_HI, BF16, seed=D, device=DEV)
    db = torch.full((D,), 5.0, device=DEV)
    ops.bias_grad(g, rows, D, db)
    want = (5.0 + g.double().sum(0)).float()
    assert torch.equal(db, want), (D, int((db != want).sum()))


def test_bias_grad_narrow_path_keeps_its_bits():
    """D = 768 on non-integer data against the kernel's own summation order restated in torch (fp32 adds only): a workgroup owns 256
    rows, 256 / (D / 8) = 2 row groups sum every second row in order, the groups are added in order, then the workgroups."""
    rows, D = 600, 768
    gen = torch.Generator(device=DEV).manual_seed(9)
    g = torch.randn(rows, D, device=DEV, generator=gen).to(BF16)
    db = torch.zeros(D, device=DEV)
    ops.bias_grad(g, rows, D, db)
    gf = g.float()
    total = torch.zeros(D, device=DEV)
    for r0 in range(0, rows, 256):
        r1 = min(rows, r0 + 256)
        s = torch.zeros(D, device=DEV)
        for rg in range(2):
            acc = torch.zeros(D, device=DEV)
            for r in range(r0 + rg, r1, 2):
                acc = acc + gf[r]
            s = s + acc
        total = total + s
    want = torch.zeros(D, device=DEV) + total
    assert torch.equal(db, want), int((db != want).sum())
    assert _rel(db, g.double().sum(0)) < 1e-5
