"""Exact-arithmetic conformance of every GEMM kernel family in egom2p_amd/csrc/gemm.hip.

Operands are integers in [-4, 4]; R, bias and the preloaded C0 / C1 are integers in [-64, 64]; the contraction is at most 2048
long.  Every partial sum is then an integer below 2^24, the fp32 accumulator of ANY summation order equals the fp64 product, and
every epilogue is one or two deterministic roundings of it (tests/test_gemm_exact_cpu.py proves this of the reference on the
host).  The reference is `A.double() @ B.double().t()` through torch followed by the same roundings in torch
(tests/_gemm_exact.py); the comparison is torch.equal over the WHOLE output buffer - sentinel rows and pad columns included - and
every family is held to the reference directly, never to another family.  All operands and outputs have padded pitches; the pad
columns of the operands hold NaN.

What reaches which kernel instantiation:

  test_nt_128_families[t128]             gemm_nt_kernel                      (kernel_mode 0, small_tiles 0)
  test_nt_128_families[t64]              gemm_ntl_kernel<64, 64, 4>          (kernel_mode 0, small_tiles 1 << 30)
  test_nt_128_families[t128x64]          gemm_ntl_kernel<128, 64, 3>         (kernel_mode 0, tune(2, 1))
  test_nt_128_families[t128x128]         gemm_ntl_kernel<128, 128, 3>        (kernel_mode 0, tune(2, 2))
  test_nt_t128_persistent_second_tile    gemm_nt_kernel, 544 tiles on 512 workgroups
  test_nt256_one_tile_per_workgroup      gemm_nt256_kernel<0> (bf16), <1> (fp32 / residual / bias + residual)
  test_nt256_several_tiles_per_workgroup the same two, 289 tiles on 256 workgroups
  test_nt256_column_strips               gemm_nt256_kernel<0, false, true> (bf16, 33 column tiles), <1> row-major at that width
  test_nt_default_dispatch               the launcher's by-shape rule: <64,64,4>, <128,64,3>, nt256<0>, gemm_nt_kernel
  test_nt_device_row_ranges              every NT family above with m_range
  test_swiglu_fwd_fused                  gemm_nt256_kernel<3>
  test_swiglu_bwd_fused                  gemm_nt256_kernel<2>
  test_fp8_epilogues                     gemm_nt256_kernel<0, true>, <1, true>
  test_fp8_swiglu_fwd_fused              gemm_nt256_kernel<3, true>
  test_quant_fp8_rows_exact              quant_fp8_rows_kernel (rowops.hip), the producer of the fp8 operands
  test_tn* [tn128]                       gemm_tn_kernel (+ tn_reduce_kernel when splits > 1)
  test_tn* [tn256]                       gemm_tn256_kernel (+ tn_reduce_kernel when splits > 1)
  test_refusals_*                        the launchers' argument checks (nothing is launched)
  test_zz_dispatch_state_is_default      the process-wide selector state after this file
"""
import contextlib
import functools
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from egom2p_amd import _lib as L  # noqa: E402
from egom2p_amd import ops  # noqa: E402

import _gemm_exact as X  # noqa: E402
from _gemm_exact import ints, pitched  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
SENT = 1.3359375            # exact in bf16 and fp32; no integer, and no multiple of 2^-6 (the finest unit of an fp8 result here)
LO, HI, ALO, AHI = X.OPERAND_LO, X.OPERAND_HI, X.ADDEND_LO, X.ADDEND_HI
ALL_EPIS = (L.EPI_BF16, L.EPI_F32, L.EPI_RESID, L.EPI_BIAS_RESID)
EPI_NAME = {L.EPI_BF16: "EPI_BF16", L.EPI_F32: "EPI_F32", L.EPI_RESID: "EPI_RESID", L.EPI_BIAS_RESID: "EPI_BIAS_RESID"}
NT128_FAMILIES = ("t128", "t64", "t128x64", "t128x128")


# ---------------------------------------------------------------------------------------------------------------- helpers
@contextlib.contextmanager
def family(name):
    """Select a kernel family; the product's dispatch state is restored on exit whatever happens inside."""
    old = ops.gemm_small_tiles(-1)
    try:
        if name == "t128":
            ops.gemm_small_tiles(0); ops.gemm_tune(2, 0); ops.gemm_kernel_mode(0, 1)
        elif name == "t64":
            ops.gemm_small_tiles(1 << 30); ops.gemm_tune(2, 0); ops.gemm_kernel_mode(0, 1)
        elif name == "t128x64":
            ops.gemm_tune(2, 1); ops.gemm_kernel_mode(0, 1)
        elif name == "t128x128":
            ops.gemm_tune(2, 2); ops.gemm_kernel_mode(0, 1)
        elif name == "nt256":
            ops.gemm_kernel_mode(2, 1)
        elif name == "tn128":
            ops.gemm_kernel_mode(1, 0)
        elif name == "tn256":
            ops.gemm_kernel_mode(1, 2)
        else:
            assert name == "default", name
        yield
    finally:
        ops.gemm_small_tiles(old)
        ops.gemm_tune(2, 0)
        ops.gemm_tune(3, 0)
        ops.gemm_kernel_mode(1, 1)


def assert_exact(got, want, acc=None, tiles=(64, 128, 256), what=""):
    """torch.equal over the whole buffer; on mismatch say how many elements differ, where the first one is, what both sides and
    the reference accumulator hold there and which tile of each tile size it belongs to."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = got != want                                   # NaN compares unequal to everything
    n = int(bad.sum())
    r, c = divmod(int(bad.flatten().nonzero()[0]), got.shape[-1])
    rows_bad = bad.any(1).nonzero().flatten()
    cols_bad = bad.any(0).nonzero().flatten()
    a = "outside the product (sentinel row or pad column)"
    if acc is not None and r < acc.shape[0] and c < acc.shape[1]:
        a = repr(acc[r, c].item())
    where = ", ".join(f"{t}-tile ({r // t}, {c // t}) at +({r % t}, {c % t})" for t in tiles)
    pytest.fail(f"{what}: {n} of {bad.numel()} elements differ; first at (row {r}, col {c}): got {got[r, c].item()!r}, "
                f"want {want[r, c].item()!r}, reference accumulator {a}; {where}; differing rows {int(rows_bad[0])}..{int(rows_bad[-1])}, "
                f"cols {int(cols_bad[0])}..{int(cols_bad[-1])}", pytrace=False)


def sentinel(rows, cols, dtype):
    return torch.full((rows, cols), SENT, device=DEV, dtype=dtype)


def dev_ints(shape, lo, hi, dtype, seed):
    return ints(shape, lo, hi, dtype, seed=seed, device=DEV)


def exact_product(a, b_t):
    """fp64 product of two integer-valued matrices, returned as fp32 (exact: integers below 2^24)"""
    acc = a.double() @ b_t.double()
    assert float(acc.abs().max()) <= X.ACC_MAX if acc.numel() else True
    return acc.float()


# ---------------------------------------------------------------------------------------------------------------- NT
@functools.lru_cache(maxsize=2)
def nt_problem(rows, N, K):
    """operands with padded pitches (lda = K + 64, ldb = K + 8, ldr = N + 4; pad columns NaN), the exact accumulator and the
    four expected epilogue results - computed once per shape, shared by the families, never modified"""
    assert K <= X.K_MAX
    A = pitched(dev_ints((rows, K), LO, HI, BF16, 1), K + 64, NAN)
    B = pitched(dev_ints((N, K), LO, HI, BF16, 2), K + 8, NAN)
    acc = exact_product(A, B.t())
    R = dev_ints((rows, N), ALO, AHI, F32, 3)
    bias = dev_ints((N,), ALO, AHI, F32, 4)
    want = [f(acc, R, bias) for f in X.EPILOGUES]
    return SimpleNamespace(rows=rows, N=N, K=K, A=A, B=B, acc=acc, R=R, Rp=pitched(R, N + 4, NAN), bias=bias, want=want)


def run_nt(p, M, epis=ALL_EPIS, span=None, tag=""):
    """every epilogue in `epis` into a sentinel-filled [rows + 2, N + pad] buffer, residual epilogues also in place (C is R)"""
    rows, N, K = p.rows, p.N, p.K
    r0, r1 = (0, M) if span is None else (span[0], span[0] + min(span[1], M))
    assert r1 <= rows
    rng = None if span is None else torch.tensor(list(span), device=DEV, dtype=torch.int32)
    for epi in epis:
        what = f"{tag} M={M} N={N} K={K} {EPI_NAME[epi]}" + ("" if span is None else f" m_range={list(span)}")
        dtype, pad = (BF16, 8) if epi == L.EPI_BF16 else (F32, 4)
        resid = epi in (L.EPI_RESID, L.EPI_BIAS_RESID)
        bias = p.bias if epi == L.EPI_BIAS_RESID else None
        exp = sentinel(rows + 2, N + pad, dtype)
        exp[r0:r1, :N] = p.want[epi][r0:r1]
        buf = sentinel(rows + 2, N + pad, dtype)
        ops.gemm_nt(p.A, p.B, buf[:, :N], M, N, K, epi, R=p.Rp if resid else None, bias=bias, m_range=rng)
        assert_exact(buf, exp, p.acc, what=what)
        if resid:                                           # in place on the residual stream, like the engine
            buf = sentinel(rows + 2, N + pad, dtype)
            buf[:rows, :N] = p.R
            exp = buf.clone()
            exp[r0:r1, :N] = p.want[epi][r0:r1]
            C = buf[:, :N]
            ops.gemm_nt(p.A, p.B, C, M, N, K, epi, R=C, bias=bias, m_range=rng)
            assert_exact(buf, exp, p.acc, what=what + " in place")


# K-steps 1, 1, 2, 3, 4, 5, 7, 32: below, at and past each ring depth (2, 3, 4); rows / columns one short of, one past and far
# from a tile edge; N a multiple of 8 but not of 64
NT128_SHAPES = [(1, 8, 64), (65, 72, 64), (127, 136, 128), (129, 200, 192), (300, 256, 256), (257, 328, 320), (66, 1000, 448),
                (130, 64, 2048)]


@pytest.mark.parametrize("M,N,K,fam", [(*s, f) for s in NT128_SHAPES for f in NT128_FAMILIES])
def test_nt_128_families(M, N, K, fam):
    p = nt_problem(M, N, K)
    with family(fam):
        run_nt(p, M, tag=fam)


@pytest.mark.parametrize("M,N,K", [(128 * 33 + 3, 2048, 64), (128 * 33 + 3, 2048, 192)])
def test_nt_t128_persistent_second_tile(M, N, K):
    """34 x 16 = 544 tiles on the persistent kernel's 512 workgroups: some take a second tile, with one and three K-steps"""
    p = nt_problem(M, N, K)
    with family("t128"):
        run_nt(p, M, tag="t128")


@pytest.mark.parametrize("M,N,K", [(1, 128, 128), (255, 128, 128), (257, 384, 192), (300, 1152, 320), (513, 640, 2048)])
def test_nt256_one_tile_per_workgroup(M, N, K):
    """half-empty last column tiles, K-tile counts 2, 3, 5 and 32"""
    p = nt_problem(M, N, K)
    with family("nt256"):
        run_nt(p, M, tag="nt256")


@pytest.mark.parametrize("K", [128, 192, 320])
def test_nt256_several_tiles_per_workgroup(K):
    """17 x 17 = 289 tiles on 256 workgroups: a tile count that is no multiple of 8 (XCD remap), even and odd K-tile counts
    across the tile seam"""
    M, N = 256 * 16 + 7, 4352
    p = nt_problem(M, N, K)
    with family("nt256"):
        run_nt(p, M, tag="nt256")


@pytest.mark.parametrize("M,N,K", [(2050, 8320, 128), (300, 8320, 192)])
def test_nt256_column_strips(M, N, K):
    """33 column tiles: the bf16 epilogue takes the column-strip walk (5 strips of both widths, 297 and 66 tiles); the fp32
    epilogue runs row-major at the same width"""
    p = nt_problem(M, N, K)
    with family("nt256"):
        run_nt(p, M, epis=(L.EPI_BF16, L.EPI_F32), tag="nt256 strips")


@pytest.mark.parametrize("M,N,K,epis,branch", [
    (1707, 768, 128, (L.EPI_BF16, L.EPI_RESID), "narrow, 84 tiles <= 100: 64 x 64 tiles"),
    (2181, 768, 128, (L.EPI_BF16, L.EPI_RESID), "narrow, 108 tiles in 101..520: 128 x 64 tiles"),
    (1707, 2304, 128, (L.EPI_BF16,), "wide bf16, 252 tiles <= 330: 128 x 64 tiles"),
    (8320, 1024, 128, (L.EPI_BF16,), "520 tiles of 128, 132 of 256: 1.85 ceil(132 / 256) <= ceil(520 / 512): 256 x 256 tiles"),
    (11141, 768, 64, (L.EPI_RESID,), "narrow, 528 tiles > 520 and K < 128: the persistent 128 x 128 kernel"),
])
def test_nt_default_dispatch(M, N, K, epis, branch):
    """One shape per branch of the by-shape rule in ego_gemm_nt_bf16's comment, nothing forced.  A test cannot see which kernel
    ran; the exact result is the check."""
    p = nt_problem(M, N, K)
    with family("default"):
        run_nt(p, M, epis=epis, tag="default (" + branch + ")")


@pytest.mark.parametrize("fam", NT128_FAMILIES + ("nt256", "default"))
def test_nt_device_row_ranges(fam):
    """m_range = {offset, count} on the device, the host M only an upper bound: an interior range, an empty one (nothing is
    written) and one longer than the host M (rows [off, off + M) are written); every other row keeps the sentinel"""
    rows, M, N, K = 400, 300, (384 if fam == "nt256" else 200), 192
    p = nt_problem(rows, N, K)
    with family(fam):
        for span in ((37, 150), (50, 0), (64, 10000)):
            run_nt(p, M, span=span, tag=fam)


# ---------------------------------------------------------------------------------------------------------------- fused SwiGLU
@pytest.mark.parametrize("M,F,K", [(257, 128, 128), (300, 384, 192), (256 * 9 + 5, 3712, 128)])      # the last: 10 x 29 = 290 tiles
def test_swiglu_fwd_fused(M, F, K):
    Xa = pitched(dev_ints((M, K), LO, HI, BF16, 21), K + 64, NAN)
    W13 = pitched(dev_ints((2 * F, K), LO, HI, BF16, 22), K + 8, NAN)
    acc = exact_product(Xa, W13.t())
    ab_ref = X.epi_bf16(acc)
    h_ref = torch.empty(M, F, device=DEV, dtype=BF16)
    ops.swiglu_fwd(ab_ref, h_ref, M, F)                      # the gate of the REFERENCE ab, not of a GEMM call
    exp_ab, exp_h = sentinel(M + 2, 2 * F + 8, BF16), sentinel(M + 2, F + 8, BF16)
    exp_ab[:M, :2 * F] = ab_ref
    exp_h[:M, :F] = h_ref
    ab, h = sentinel(M + 2, 2 * F + 8, BF16), sentinel(M + 2, F + 8, BF16)
    ops.gemm_nt_swiglu_fwd(Xa, W13, ab[:, :2 * F], h[:, :F], M, F, K)
    assert_exact(ab, exp_ab, acc, tiles=(128, 256), what=f"swiglu fwd ab M={M} F={F} K={K}")
    assert_exact(h, exp_h, tiles=(128, 256), what=f"swiglu fwd h M={M} F={F} K={K}")


@pytest.mark.parametrize("M,F,K", [(257, 256, 128), (300, 512, 192), (256 * 9 + 5, 7424, 128)])      # the last: 10 x 29 = 290 tiles
def test_swiglu_bwd_fused(M, F, K):
    dY = pitched(dev_ints((M, K), LO, HI, BF16, 31), K + 64, NAN)
    W2t = pitched(dev_ints((F, K), LO, HI, BF16, 32), K + 8, NAN)
    acc = exact_product(dY, W2t.t())
    dh_ref = X.epi_bf16(acc)
    g = torch.Generator(device=DEV).manual_seed(33)
    ab_dense = (torch.randn(M, 2 * F, device=DEV, generator=g) * 2).to(BF16)          # ordinary values: only the GEMM is integer
    ref = torch.empty(M, 2 * F, device=DEV, dtype=BF16)
    ops.swiglu_bwd(ab_dense, dh_ref, ref, M, F)
    ab = sentinel(M + 2, 2 * F + 8, BF16)
    ab[:M, :2 * F] = ab_dense
    ab_before = ab.clone()
    exp = sentinel(M + 2, 2 * F + 8, BF16)
    exp[:M, :2 * F] = ref
    dab = sentinel(M + 2, 2 * F + 8, BF16)
    ops.gemm_nt_swiglu_bwd(dY, W2t, ab[:, :2 * F], dab[:, :2 * F], M, F, K)
    assert_exact(dab, exp, tiles=(256,), what=f"swiglu bwd dab M={M} F={F} K={K}")
    assert_exact(ab, ab_before, what="swiglu bwd: the saved ab is an input")


# ---------------------------------------------------------------------------------------------------------------- fp8
def e4m3(t):
    """e4m3 encodings (uint8) of a tensor of values e4m3 represents exactly"""
    q = t.float().cpu().to(torch.float8_e4m3fn)
    assert torch.equal(q.float(), t.float().cpu()), "not exactly representable in e4m3"
    return q.view(torch.uint8).to(t.device)


def fp8_operands(M, N, K, seed):
    """A8 [M, K] / B8 [N, K] as e4m3 bytes of integers in [-4, 4] (lda = K + 64, ldb = K + 16, pad bytes 0x7f = NaN), power-of-two
    row scales 2^-3 .. 2^3 and the exact scaled product sa[m] sb[n] acc[m, n] as fp32"""
    assert K <= X.K_MAX
    Ai, Bi = dev_ints((M, K), LO, HI, F32, seed), dev_ints((N, K), LO, HI, F32, seed + 1)
    A8, B8 = pitched(e4m3(Ai), K + 64, 0x7F), pitched(e4m3(Bi), K + 16, 0x7F)
    sa = torch.exp2(dev_ints((M,), -3, 3, F32, seed + 2))
    sb = torch.exp2(dev_ints((N,), -3, 3, F32, seed + 3))
    acc = (Ai.double() @ Bi.double().t()) * sa.double()[:, None] * sb.double()[None, :]
    assert torch.equal(acc.float().double(), acc)
    return A8, B8, sa, sb, acc.float()


FP8_SHAPES = [(1, 128, 256), (257, 384, 384), (300, 1152, 2048), (256 * 16 + 7, 4352, 256)]


@pytest.mark.parametrize("M,N,K", FP8_SHAPES)
def test_fp8_epilogues(M, N, K):
    A8, B8, sa, sb, acc = fp8_operands(M, N, K, 41)
    R = dev_ints((M, N), ALO, AHI, F32, 45)
    Rp = pitched(R, N + 4, NAN)
    bias = dev_ints((N,), ALO, AHI, F32, 46)
    s64 = acc.double() + bias.double()
    assert torch.equal(s64.float().double(), s64)            # acc + bias is exact in fp32 for these scales too
    for epi in ALL_EPIS:
        dtype, pad = (BF16, 8) if epi == L.EPI_BF16 else (F32, 4)
        resid = epi in (L.EPI_RESID, L.EPI_BIAS_RESID)
        exp = sentinel(M + 2, N + pad, dtype)
        exp[:M, :N] = X.EPILOGUES[epi](acc, R, bias)
        buf = sentinel(M + 2, N + pad, dtype)
        ops.gemm_nt_fp8(A8, sa, B8, sb, buf[:, :N], M, N, K, epi, R=Rp if resid else None,
                        bias=bias if epi == L.EPI_BIAS_RESID else None)
        assert_exact(buf, exp, acc, tiles=(256,), what=f"fp8 M={M} N={N} K={K} {EPI_NAME[epi]}")


@pytest.mark.parametrize("M,F,K", FP8_SHAPES)
def test_fp8_swiglu_fwd_fused(M, F, K):
    X8, W8, sx, sw, acc = fp8_operands(M, 2 * F, K, 51)
    ab_ref = X.epi_bf16(acc)
    h_ref = torch.empty(M, F, device=DEV, dtype=BF16)
    ops.swiglu_fwd(ab_ref, h_ref, M, F)
    exp_ab, exp_h = sentinel(M + 2, 2 * F + 8, BF16), sentinel(M + 2, F + 8, BF16)
    exp_ab[:M, :2 * F] = ab_ref
    exp_h[:M, :F] = h_ref
    ab, h = sentinel(M + 2, 2 * F + 8, BF16), sentinel(M + 2, F + 8, BF16)
    ops.gemm_nt_swiglu_fwd_fp8(X8, sx, W8, sw, ab[:, :2 * F], h[:, :F], M, F, K)
    assert_exact(ab, exp_ab, acc, tiles=(128, 256), what=f"fp8 swiglu fwd ab M={M} F={F} K={K}")
    assert_exact(h, exp_h, tiles=(128, 256), what=f"fp8 swiglu fwd h M={M} F={F} K={K}")


def test_quant_fp8_rows_exact():
    """rows holding only +-448 * 2^e and other multiples n * 2^e with n an integer e4m3 represents: amax / 448 = 2^e exactly, so
    the quantiser must return exactly the encodings of n and scale = 2^e"""
    K = 640                                                  # two passes of a wave over the row
    reps = [n for n in range(0, 449) if float(torch.tensor(float(n)).to(torch.float8_e4m3fn).float()) == n]
    assert len(reps) == 55 and 448 in reps and 17 not in reps       # 0..16, then steps of 2, 4, 8, 16, 32 up to 448
    exps = list(range(-8, 9))
    g = torch.Generator().manual_seed(61)
    n = torch.tensor(reps, dtype=torch.float32)[torch.randint(0, len(reps), (len(exps), K), generator=g)]
    n = n * (torch.randint(0, 2, n.shape, generator=g) * 2 - 1).float()
    n = torch.where(n == 0, torch.zeros_like(n), n)         # no negative zeros
    n[:, 3], n[:, K - 1] = 448.0, -448.0
    n[0::2, 3] = -448.0                                      # rows whose amax comes from the negative side only
    n[0::2, K - 1] = 0.0
    scale_ref = torch.exp2(torch.tensor(exps, dtype=torch.float32))
    Xb = (n * scale_ref[:, None]).to(BF16)
    assert torch.equal(Xb.float(), n * scale_ref[:, None])   # exact in bf16 (4 significant bits)
    Xp = pitched(Xb.to(DEV), K + 8, NAN)
    Q = torch.full((len(exps) + 1, K + 16), 0x55, device=DEV, dtype=torch.uint8)
    scale = sentinel(1, len(exps) + 1, F32)[0]
    ops.quant_fp8_rows(Xp, Q[:, :K], scale, rows=len(exps), K=K)
    expQ = torch.full_like(Q, 0x55)
    expQ[:len(exps), :K] = e4m3(n.to(DEV))
    exp_scale = sentinel(1, len(exps) + 1, F32)[0]
    exp_scale[:len(exps)] = scale_ref.to(DEV)
    assert_exact(scale[None], exp_scale[None], what="quant_fp8_rows scale")
    assert_exact(Q, expQ, what="quant_fp8_rows encodings")


# ---------------------------------------------------------------------------------------------------------------- TN
@functools.lru_cache(maxsize=2)
def tn_problem(rows, Ni, Nj):
    P, Q = dev_ints((rows, Ni), LO, HI, BF16, 71), dev_ints((rows, Nj), LO, HI, BF16, 72)
    return P, Q, dev_ints((Ni, Nj), ALO, AHI, F32, 73)


def run_tn(fam, M, Ni, Nj, splits, rows=None, span=None, routing=None):
    """C += P^T Q into sentinel-framed buffers (ldp = Ni + 8, ldq = Nj + 64, ldc = Nj + 4), the split-K slab poisoned with NaN;
    rows of P / Q outside the contraction range hold NaN.  routing = (split_row, rows0, rows1)."""
    rows = M if rows is None else rows
    assert M <= X.K_MAX
    Pd, Qd, Cinit = tn_problem(rows, Ni, Nj)
    r0, r1 = (0, M) if span is None else (span[0], span[0] + min(span[1], M))
    assert r1 <= rows
    prod = exact_product(Pd[r0:r1].t(), Qd[r0:r1])
    Pn, Qn = Pd.clone(), Qd.clone()
    Pn[:r0], Pn[r1:], Qn[:r0], Qn[r1:] = NAN, NAN, NAN, NAN      # zero fill is required beyond the range: clamping is not enough
    P, Q = pitched(Pn, Ni + 8, NAN), pitched(Qn, Nj + 64, NAN)
    full = Cinit + prod
    split_row, rows0, rows1 = (Ni, Ni, 0) if routing is None else routing
    bufs, exps = [], []
    for first, n in ((0, rows0), (split_row, rows1)):
        b = sentinel(n + 2, Nj + 4, F32)
        b[:n, :Nj] = Cinit[first:first + n]
        e = b.clone()
        e[:n, :Nj] = full[first:first + n]
        bufs.append(b); exps.append(e)
    slab = torch.full((splits, Ni, Nj), NAN, device=DEV) if splits > 1 else None
    rng = None if span is None else torch.tensor(list(span), device=DEV, dtype=torch.int32)
    with family(fam):
        ops.gemm_tn(P, Q, bufs[0][:, :Nj], Ni, Nj, M, C1=None if routing is None else bufs[1][:, :Nj], split_row=split_row,
                    rows0=rows0, rows1=rows1, m_range=rng, splits=splits, slab=slab)
    what = f"{fam} M={M} Ni={Ni} Nj={Nj} splits={splits}" + ("" if span is None else f" m_range={list(span)}")
    assert_exact(bufs[0], exps[0], prod, tiles=(128, 256), what=what + " C0")
    if routing is not None:
        assert_exact(bufs[1], exps[1], prod[split_row:], tiles=(128, 256), what=what + f" C1 (output rows from {split_row})")


# contraction rows below, at and one past a 64-row step (the ragged ones together with split-K); half-empty 256 tiles both ways
TN_SHAPES = [(1, 128, 128), (63, 128, 256), (64, 256, 128), (65, 384, 640), (461, 384, 256), (2048, 128, 128)]


@pytest.mark.parametrize("M,Ni,Nj,splits,fam", [(*s, k, f) for s in TN_SHAPES for k in (1, 2, 3, 8) for f in ("tn128", "tn256")])
def test_tn(M, Ni, Nj, splits, fam):
    """split counts include ones that leave some splits without any step; the slab starts as NaN"""
    run_tn(fam, M, Ni, Nj, splits)


@pytest.mark.parametrize("fam", ["tn128", "tn256"])
@pytest.mark.parametrize("splits", [1, 3])
def test_tn_row_routing(fam, splits):
    """output rows [0, 128) -> C0 (first 100 valid, 100..127 dropped), rows >= 128 -> C1 (first 200 valid)"""
    run_tn(fam, 461, 384, 256, splits, routing=(128, 100, 200))


@pytest.mark.parametrize("fam", ["tn128", "tn256"])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("span", [(70, 300), (5, 0), (100, 5000)], ids=["interior", "empty", "longer_than_M"])
def test_tn_device_row_ranges(fam, splits, span):
    """rows outside [off, off + min(count, M)) hold NaN and must not reach the result"""
    run_tn(fam, 461, 384, 256, splits, rows=600, span=span)


# ---------------------------------------------------------------------------------------------------------------- refusals
def refused(call, *outs):
    with pytest.raises(L.EgoHipError):
        call()
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == SENT).all()), "a refused call wrote to its output"


def test_refusals_nt():
    M, N, K = 64, 64, 128
    A, B = dev_ints((M, K + 8), LO, HI, BF16, 81), dev_ints((N, K + 8), LO, HI, BF16, 82)
    R, bias = dev_ints((M, N), ALO, AHI, F32, 83), dev_ints((N,), ALO, AHI, F32, 84)
    Cb, Cf = sentinel(M, N + 8, BF16), sentinel(M, N + 8, F32)
    nt = ops.gemm_nt
    refused(lambda: nt(A, B, Cb, M, N, 96, L.EPI_BF16), Cb)                                   # K % 64
    refused(lambda: nt(A, B, Cb, M, 60, K, L.EPI_BF16), Cb)                                   # N % 8
    refused(lambda: nt(A, B, Cb, M, N, K, L.EPI_BF16, lda=K + 4), Cb)                         # lda % 8
    refused(lambda: nt(A, B, Cb, M, N, K, L.EPI_BF16, ldb=K + 4), Cb)                         # ldb % 8
    refused(lambda: nt(A, B, Cb, M, N, K, L.EPI_BF16, ldc=N + 4), Cb)                         # bf16 output, ldc % 8
    refused(lambda: nt(A, B, Cf, M, N, K, L.EPI_F32, ldc=N + 2), Cf)                          # ldc % 4
    refused(lambda: nt(A, B, Cf, M, N, K, L.EPI_RESID), Cf)                                   # residual epilogue without R
    refused(lambda: nt(A, B, Cf, M, N, K, L.EPI_BIAS_RESID, bias=bias), Cf)
    refused(lambda: nt(A, B, Cf, M, N, K, L.EPI_BIAS_RESID, R=R), Cf)                         # ... without bias
    refused(lambda: nt(A, B, Cf, M, N, K, 4), Cf)                                             # unknown epilogue


def test_refusals_fused_swiglu():
    M, K = 64, 128
    Xa, W = dev_ints((M, K), LO, HI, BF16, 85), dev_ints((512, K), LO, HI, BF16, 86)
    ab, h, dab = sentinel(M, 512, BF16), sentinel(M, 256, BF16), sentinel(M, 512, BF16)
    refused(lambda: ops.gemm_nt_swiglu_fwd(Xa, W, ab, h, M, 64, K), ab, h)                   # F % 128
    refused(lambda: ops.gemm_nt_swiglu_fwd(Xa, W, ab, h, M, 192, K), ab, h)
    refused(lambda: ops.gemm_nt_swiglu_fwd(Xa, W, ab, h, M, 256, 64), ab, h)                 # K < 128
    refused(lambda: ops.gemm_nt_swiglu_fwd(Xa, W, ab, h, M, 256, 96), ab, h)                 # K % 64
    src = sentinel(M, 512, BF16)
    refused(lambda: ops.gemm_nt_swiglu_bwd(Xa, W, src, dab, M, 128, K), dab)                 # F % 256
    refused(lambda: ops.gemm_nt_swiglu_bwd(Xa, W, src, dab, M, 256, 64), dab)                # K < 128


def test_refusals_fp8():
    M, N, K = 64, 128, 256
    A8, B8 = e4m3(dev_ints((M, 512), LO, HI, F32, 87)), e4m3(dev_ints((256, 512), LO, HI, F32, 88))
    sa, sb = torch.ones(M, device=DEV), torch.ones(256, device=DEV)
    Cb, Cf = sentinel(M, 256, BF16), sentinel(M, 256, F32)
    f8 = ops.gemm_nt_fp8
    refused(lambda: f8(A8, sa, B8, sb, Cb, M, N, 128, L.EPI_BF16), Cb)                        # K < 256
    refused(lambda: f8(A8, sa, B8, sb, Cb, M, N, 320, L.EPI_BF16), Cb)                        # K % 128
    refused(lambda: f8(A8, sa, B8, sb, Cb, M, 192, K, L.EPI_BF16), Cb)                        # N % 128
    refused(lambda: f8(A8, None, B8, sb, Cb, M, N, K, L.EPI_BF16), Cb)                        # missing scales
    refused(lambda: f8(A8, sa, B8, None, Cb, M, N, K, L.EPI_BF16), Cb)
    refused(lambda: f8(A8, sa, B8, sb, Cf, M, N, K, L.EPI_RESID), Cf)                         # residual epilogue without R
    ab, h = sentinel(M, 256, BF16), sentinel(M, 128, BF16)
    refused(lambda: ops.gemm_nt_swiglu_fwd_fp8(A8, sa, B8, sb, ab, h, M, 128, 128), ab, h)   # K < 256
    refused(lambda: ops.gemm_nt_swiglu_fwd_fp8(A8, sa, B8, sb, ab, h, M, 64, K), ab, h)      # F % 128
    refused(lambda: ops.gemm_nt_swiglu_fwd_fp8(A8, None, B8, sb, ab, h, M, 128, K), ab, h)   # missing scales


def test_refusals_tn():
    M = 64
    P, Q = dev_ints((M, 256), LO, HI, BF16, 89), dev_ints((M, 256), LO, HI, BF16, 90)
    C = sentinel(256, 256, F32)
    refused(lambda: ops.gemm_tn(P, Q, C, 192, 128, M), C)                                     # Ni % 128
    refused(lambda: ops.gemm_tn(P, Q, C, 128, 192, M), C)                                     # Nj % 128
    refused(lambda: ops.gemm_tn(P, Q, C, 128, 128, M, splits=2), C)                           # splits > 1 without a slab
    refused(lambda: ops.gemm_tn(P, Q, C, 128, 128, M, ldp=252), C)                            # ldp % 8
    refused(lambda: ops.gemm_tn(P, Q, C, 128, 128, M, ldc=254), C)                            # ldc % 4


# ---------------------------------------------------------------------------------------------------------------- state
def test_zz_dispatch_state_is_default():
    """the family selector is process-wide: after this file it must be what the product runs with"""
    assert ops.gemm_small_tiles(-1) == 400
    assert ops.gemm_tune(1, -1) == 0 and ops.gemm_tune(2, -1) == 0 and ops.gemm_tune(3, -1) == 0
