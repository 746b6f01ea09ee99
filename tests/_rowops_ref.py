"""Shared pieces of the row / loss kernel conformance tests (tests/test_rowops_exact_gpu.py, tests/test_rowops_exact_cpu.py):
input builders, fp64 references, envelope models and fp32 CPU restatements of the kernels of egom2p_amd/csrc/rowops.hip.
Nothing in this module needs a GPU.

How a result is judged
----------------------
* Exact cases: the inputs are built so that every intermediate is exact in fp32 in ANY order (integers below 2^24, powers of two,
  exp(-200) = 0); the expected bits are written down and compared with ==.  tests/test_rowops_exact_cpu.py proves the exactness.
* Numeric cases: `need` = the smallest error BEFORE the documented roundings that explains the result.  For an fp32 output that is
  |got - ref64|; for a bf16 output it is the distance from ref64 to the set of reals that round to the bf16 value stored
  (`bf16_preimage`), so the bf16 store costs nothing and hides nothing; SwiGLU's inner round_bf16(silu(a)) is undone the same way
  (`swiglu_need`).  `need` is divided by a per-element `unit` - eps32 times the magnitudes that enter the fp32 formula, stated by
  each family's model below - which gives a deviation in "fp32 roundings".
* The slack is measured, not guessed: the same formula is evaluated in plain fp32 torch on the CPU over the test's own inputs, and
  its worst deviation in the same units is the constant CPU_DEV[family] below (tests/test_rowops_exact_cpu.py asserts that the
  constants still cover the CPU run).  The GPU may deviate FACTOR = 4 times as much: another summation order, and the hardware's
  approximate exp / log / rsqrt that a CPU run cannot show.
* Floors: where the fp32 FORMAT (not the arithmetic) loses a value - a sigmoid or softmax term below the smallest normal fp32,
  2^-126, which hardware may flush to zero - an absolute floor stated with the family is taken off `need` first.
"""
import zlib

import numpy as np
import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS32 = 2.0 ** -24                      # half an fp32 ulp of 1: one rounding
FLT_MIN = 2.0 ** -126                   # the smallest normal fp32
FACTOR = 4.0                            # GPU allowance over the CPU-measured deviation (see above)

# bit patterns of the frames: inputs NaN (a stray read poisons the result), outputs patterns no result can be (signalling NaNs
# with a payload: the kernels produce the canonical quiet NaN at most; 0xFF is e4m3's negative NaN, the converter saturates instead)
NAN_BF16, NAN_F32 = 0x7FC0, 0x7FC00000
SENT_BF16, SENT_F32, SENT_U8 = 0x7FA5, 0x7FA55AA5, 0xFF

# Worst deviation of the plain fp32 CPU evaluation from ref64 over the GPU test's own inputs, in the units of each family's model
# (measured by tests/test_rowops_exact_cpu.py::test_cpu_fp32_fits_the_recorded_deviation, which prints them; x86-64, torch CPU
# kernels), rounded up after adding 5 %: another torch build or SIMD width sums in another order and moves the CPU figure a
# little.  The GPU envelope of a family is FACTOR x this value.
CPU_DEV = {
    "ce_lse": 0.49,      # measured 0.4649, + 5 %; envelope = 4 x 0.49 = 1.96
    "ce_nll": 0.52,      # measured 0.4904, + 5 %; envelope = 4 x 0.52 = 2.08
    "ce_grad": 1.78,     # measured 1.6877, + 5 %; envelope = 4 x 1.78 = 7.12
    "ln_mean": 3.07,     # measured 2.9181, + 5 %; envelope = 4 x 3.07 = 12.28
    "ln_rstd": 2.20,     # measured 2.0951, + 5 %; envelope = 4 x 2.20 = 8.80
    "ln_y": 3.07,        # measured 2.9156, + 5 %; envelope = 4 x 3.07 = 12.28
    "ln_dx": 3.68,       # measured 3.4953, + 5 %; envelope = 4 x 3.68 = 14.72
    "ln_dw": 3.07,       # measured 2.9156, + 5 %; envelope = 4 x 3.07 = 12.28
    "swiglu_fwd": 2.95,  # measured 2.8023, + 5 %; envelope = 4 x 2.95 = 11.80
    "swiglu_da": 3.90,   # measured 3.7125, + 5 %; envelope = 4 x 3.90 = 15.60
    "swiglu_db": 3.04,   # measured 2.8926, + 5 %; envelope = 4 x 3.04 = 12.16
}


def envelope(family):
    return FACTOR * CPU_DEV[family]


def gen(*key):
    """a CPU generator seeded by the key: the same call gives the same numbers in every test and on every run"""
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def ibits(t):
    """the tensor's bits as integers of the same width"""
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def sbits(v, width):
    """an unsigned bit pattern as the signed integer torch stores"""
    return v - (1 << (8 * width)) if width > 1 and v >= 1 << (8 * width - 1) else v


def framed(rows, ld, dtype, bits, pre=2, post=2, device="cpu"):
    """a [pre + rows + post, ld] buffer filled with the bit pattern, and its [rows, ld] middle"""
    buf = torch.empty((pre + rows + post, ld), dtype=dtype, device=device)
    ibits(buf).fill_(sbits(bits, buf.element_size()))
    return buf, buf[pre:pre + rows]


def frame_intact(buf, bits, owned):
    """(frame untouched, every owned element written) for a boolean mask `owned` of buf's shape"""
    is_sent = ibits(buf) == sbits(bits, buf.element_size())
    return bool(is_sent[~owned].all()), not bool(is_sent[owned].any())


# ---------------------------------------------------------------------------------------------------------------- bf16
def all_finite_bf16():
    """every finite bf16 bit pattern once, in bit order (65,280 values)"""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[((bits >> 7) & 0xFF) != 0xFF]
    return bits.to(torch.int16).view(BF16)


def _mag_value(mag):
    """fp64 value of a non-negative bf16 magnitude pattern; 0x7F80 (inf) counts as 2^128, the end of the finite range's last cell"""
    v = mag.clamp(0, 0x7F7F).to(torch.int16).view(BF16).double()
    return torch.where(mag >= 0x7F80, torch.full_like(v, 2.0 ** 128), v)


def bf16_preimage(t):
    """[lo, hi] in fp64: the reals that round (to nearest) to the bf16 values t (finite or infinite); ties count as inside"""
    bits = ibits(t).to(torch.int32) & 0xFFFF
    mag, neg = bits & 0x7FFF, (bits >> 15) == 1
    v = _mag_value(mag)
    up = 0.5 * (v + _mag_value(mag + 1))
    up = torch.where(mag >= 0x7F80, torch.full_like(up, float("inf")), up)          # +-inf: everything beyond the last finite cell
    dn = torch.where(mag == 0, -0.5 * _mag_value(torch.ones_like(mag)), 0.5 * (v + _mag_value((mag - 1).clamp_min(0))))
    lo, hi = torch.where(neg, -up, dn), torch.where(neg, -dn, up)
    zero = mag == 0
    lo = torch.where(zero, -up, lo)
    hi = torch.where(zero, up, hi)
    return lo, hi


def need_bf16(got, ref64):
    """smallest |error| before the bf16 store that explains the stored value (an infinity is explained by a reference beyond the
    last finite cell; a NaN by nothing: inf)"""
    lo, hi = bf16_preimage(got)
    d = torch.maximum(torch.maximum(lo - ref64, ref64 - hi), torch.zeros_like(ref64))
    return torch.where(torch.isnan(got.float()), torch.full_like(d, float("inf")), d)


def deviation(need, unit, floor=0.0):
    """worst need in units, after the format floor"""
    return float(((need - floor).clamp_min(0.0) / unit).max())


# ---------------------------------------------------------------------------------------------------------------- cross-entropy
CE_VS = (8, 2040, 2048, 2056, 6144, 8184, 8200, 64000, 65536, 65544)
CE_FILL = -200.0                        # exp(-200) = 0 in fp32 (2^-288.5 is far below the smallest subnormal)


def ce_spike_positions(V):
    """the spike columns of the issue: 0..15, both sides of every multiple of 2048 and of 8192 below V, the last 16, 32 seeded"""
    pos = set(range(min(16, V))) | set(range(max(0, V - 16), V))
    for step in (2048, 8192):
        for m in range(step, V, step):
            pos |= {m - 1, m}
    pos |= set(torch.randint(0, V, (32,), generator=gen("ce spikes", V)).tolist())
    return sorted(pos)


def ce_spike_rows(V):
    """(spike column, target) per row: target = the spike, its two neighbours, 0 and V - 1; padded to a power of two of rows by
    starting over (n must be a power of two for the coefficient to be exact)"""
    rows = []
    for j in ce_spike_positions(V):
        for t in dict.fromkeys((j, j - 1, j + 1, 0, V - 1)):
            if 0 <= t < V:
                rows.append((j, t))
    n = 1 << (len(rows) - 1).bit_length()
    rows = (rows * (n // len(rows) + 1))[:n]
    j, t = torch.tensor(rows, dtype=torch.int64).t()
    return j.contiguous(), t.contiguous()


def ce_spike_logits(j, V, ld, pre, post, device="cpu"):
    """[pre + n + post, ld] bf16: NaN frame rows and pad columns, -200 inside, 0 at each row's spike"""
    n = j.numel()
    buf, mid = framed(n, ld, BF16, NAN_BF16, pre, post, device)
    mid[:, :V] = CE_FILL
    mid[torch.arange(n, device=device), j.to(device)] = 0.0
    return buf


def ce_spike_expected(j, t, V, ld, pre, post, coef, device="cpu"):
    """the bits every CE kernel must leave: lse = 0, nll = 0 or 200, d logits = (onehot(j) - onehot(t)) coef in bf16 (coef a
    power of two), frame NaN as before"""
    n = j.numel()
    buf, mid = framed(n, ld, BF16, NAN_BF16, pre, post, device)
    mid[:, :V] = 0.0
    ar = torch.arange(n, device=device)
    jd, td = j.to(device), t.to(device)
    ne = jd != td
    mid[ar[ne], jd[ne]] = coef
    mid[ar[ne], td[ne]] = -coef
    nll = ne.to(F32) * -CE_FILL
    return buf, torch.zeros(n, dtype=F32, device=device), nll


def ce_emul(x, tgt, coef, drop_chunk=None, onehot_xor=0, order="pairwise"):
    """fp32 CPU restatement of ce_fwd + ce_bwd on rows x [n, V] (fp32 holding bf16 values): lse, nll, the gradient before its bf16 store.
    drop_chunk: the 16-byte chunk (8 columns) a planted seam error leaves out of the sum; onehot_xor: the planted `tgt ^ 1`.
    order: how the V terms are summed (the exactness proofs run three)."""
    x = x.float()
    n, V = x.shape
    keep = torch.ones(V, dtype=torch.bool)
    if drop_chunk is not None:
        keep[drop_chunk * 8:drop_chunk * 8 + 8] = False
    xs = x[:, keep]
    mx = xs.max(-1).values
    e = torch.exp(xs - mx[:, None])
    if order == "pairwise":
        tot = e.sum(-1)
    elif order == "reverse":
        tot = e.flip(-1).cumsum(-1)[:, -1]
    else:                               # "strided": 256 threads, each its own chunks, then the threads in order
        pad = (-e.shape[1]) % 2048
        ep = torch.cat([e, torch.zeros(n, pad)], 1).reshape(n, -1, 256, 8)
        tot = ep.sum(3).cumsum(1)[:, -1].cumsum(1)[:, -1]
    lse = mx + torch.log(tot)
    nll = lse - x[torch.arange(n), tgt]
    p = torch.exp(x - lse[:, None])
    p[torch.arange(n), tgt ^ onehot_xor] -= 1.0
    return lse, nll, p * torch.tensor(coef, dtype=F32)


def ce_numeric_logits(V, sigma, shift, rows=6):
    """bf16(sigma randn + shift); the last row's maximum sits in its last 16-byte chunk"""
    x = (torch.randn(rows, V, generator=gen("ce numeric", V, sigma, shift)) * sigma + shift).to(BF16)
    x[rows - 1, V - 3] = (x[rows - 1].float().max() + 2.0).to(BF16)
    tgt = torch.randint(0, V, (rows,), generator=gen("ce targets", V, sigma, shift))
    tgt[0], tgt[1], tgt[rows - 1] = 0, V - 1, V - 3
    return x, tgt


def ce_model64(x, tgt, coef):
    """fp64 reference and units.  lse = mx + log(sum exp(x - mx)): the result is rounded at the magnitude of lse and of mx, and log's
    argument carries the roundings of the sum; nll = lse - x[t] adds one rounding at its own size; p = exp(x - lse) has the
    relative error of its exponent's absolute error: that of lse plus the rounding of x - lse.  Terms of the softmax below the
    smallest normal fp32 may be flushed: floor |coef| 2^-126 on the gradient."""
    xd = x.double()
    n = xd.shape[0]
    lse = torch.logsumexp(xd, -1)
    nll = lse - xd[torch.arange(n), tgt]
    p = torch.exp(xd - lse[:, None])
    oh = torch.zeros_like(p)
    oh[torch.arange(n), tgt] = 1.0
    grad = (p - oh) * coef
    u_lse = EPS32 * (lse.abs() + xd.max(-1).values.abs() + 1.0)
    u_nll = u_lse + EPS32 * nll.abs()
    u_grad = abs(coef) * EPS32 * (p * (xd.abs() + lse.abs()[:, None] + 1.0) + (p - oh).abs())
    return dict(lse=lse, nll=nll, grad=grad, u_lse=u_lse, u_nll=u_nll, u_grad=u_grad, floor_grad=abs(coef) * FLT_MIN)


# ---------------------------------------------------------------------------------------------------------------- loss_finalize
LF_NS = (0, 1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4099, 12289, 16389, 65536)


def lf_layout():
    """every offset residue mod 4 with every n: 56 disjoint ranges in one NaN-filled buffer, integer nll in 0..7 inside.
    Returns (nll fp32 [total], ranges [(off, n)], exact integer sums)."""
    ranges, off = [], 5
    for res in range(4):
        for n in LF_NS:
            off += (res - off) % 4
            ranges.append((off, n))
            off += n + 3                                     # a NaN gap behind every range
    nll = torch.full((off + 8,), float("nan"), dtype=F32)
    sums = []
    for i, (o, n) in enumerate(ranges):
        v = torch.randint(0, 8, (n,), generator=gen("lf", i))
        if n:                                                # the two end rows are never 0: dropping or doubling one always shows
            v[0], v[-1] = v[0] % 7 + 1, v[-1] % 7 + 1
        nll[o:o + n] = v.float()
        sums.append(int(v.sum()))
    return nll, ranges, sums


def lf_emul(nll, off, n, head_delta=0, tail_delta=0, order="kernel"):
    """fp32 restatement of loss_finalize_kernel's sum over nll[off, off + n): scalar head to the first 16-byte boundary, float4
    body, scalar tail.  head_delta / tail_delta = -1 / +1: the planted error drops / doubles the first head row or the last tail
    row (the first / last row of the range where there is no head / tail)."""
    p = nll[off:off + n].float()
    w = torch.ones(n)
    if n and head_delta:
        w[0] += head_delta
    if n and tail_delta:
        w[n - 1] += tail_delta
    p = p * w
    if order == "reverse":
        p = p.flip(0)
    if order == "kernel":
        head = min(n, (4 - (off & 3)) & 3)
        n4 = (n - head) // 4
        s = p[:head].sum() + p[head:head + 4 * n4].reshape(-1, 4).sum(1).sum() + p[head + 4 * n4:].sum()
    elif order == "sequential":
        s = p.cumsum(0)[-1] if n else torch.tensor(0.0)
    else:
        s = p.sum()
    return float(s) / np.float32(n) if n else np.float32(0.0)


def lf_mean(total, n):
    return np.float32(total) / np.float32(n) if n else np.float32(0.0)


def ulps32(a, b):
    """distance in fp32 ulps of b (numpy fp32 scalars / arrays)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
LN_SHAPES = [(4, 4), (8, 8), (252, 252), (256, 256), (260, 260), (768, 768), (772, 772), (1024, 1024), (1028, 1028), (1536, 1536),
             (1540, 1540), (2048, 2048),
             (1, 4), (3, 4), (126, 128), (770, 772), (1020, 1024), (2046, 2048),      # TAIL: D % 4 != 0
             (128, 1024)]                                                            # a narrow width in a wide pitch
LN_ROWS = (1, 3, 4, 5, 31, 32, 33)
LN_DISTS = ((2.0, 0.3), (1.0, 1000.0), (1e-3, 0.0))
LN_EPS = 1e-6


def ln_pad4(D):
    return (D + 3) // 4 * 4


def ln_inputs(rows, D, ld, s, m):
    """x [rows, ld] fp32 = randn s + m in [0, D); the entry point's contract makes the pad columns of x zero - they are, up to the
    end of D's last 16-byte chunk, and NaN behind it (whole pad chunks must not be read).  w [ld]: in [0.5, 1.5), zero pad."""
    g = gen("ln", rows, D, ld, s, m)
    x = torch.full((rows, ld), float("nan"))
    x[:, :ln_pad4(D)] = 0.0
    x[:, :D] = torch.randn(rows, D, generator=g) * s + m
    w = torch.zeros(ld)
    w[:D] = torch.rand(D, generator=g) + 0.5
    dy = torch.full((rows, ld), float("nan"))
    dy[:, :ln_pad4(D)] = 0.0
    dy[:, :D] = torch.randn(rows, D, generator=g)
    return x, w, dy.to(BF16)


def ln_multi_inputs(rows, D, ld, n_layers):
    """one x (randn 2 + 0.3) and per layer a weight and an upstream gradient, for the multi-layer kernels"""
    x, _, _ = ln_inputs(rows, D, ld, 2.0, 0.3)
    ws, dys = [], []
    for l in range(n_layers):
        _, w, dy = ln_inputs(rows, D, ld, 2.0, 0.3 + l)
        ws.append(w)
        dys.append(dy)
    return x, ws, dys


def ln_perm(rows):
    """an out_row / dy_row map with one -1 entry (rows >= 3), else None"""
    if rows < 3 or rows in (4, 32):
        return None
    p = torch.randperm(rows, generator=gen("ln perm", rows)).int()
    p[1] = -1
    return p


def ln_fwd64(x, w, D, mean_over=None):
    """fp64 reference and units of the forward.  mean / var over D (mean_over = ld: the planted error).
    Units: the mean's sum rounds at the size of the |x| it adds; rstd is relative; y = (x - mean) rstd w inherits the error of the
    fp32 MEAN, eps32 |mean|, as an absolute error of x - mean: the cancellation term |mean| rstd |w| beside |xhat w|."""
    xd, wd = x[:, :D].double(), w[:D].double()
    n = D if mean_over is None else mean_over
    mean = xd.sum(-1) / n
    var = ((xd - mean[:, None]) ** 2).sum(-1) / n
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    xh = (xd - mean[:, None]) * rstd[:, None]
    y = xh * wd
    canc = (mean.abs() * rstd)[:, None]
    return dict(mean=mean, rstd=rstd, xh=xh, y=y, u_mean=EPS32 * xd.abs().mean(-1).clamp_min(FLT_MIN),
                u_rstd=EPS32 * rstd * (1.0 + canc[:, 0]), u_y=EPS32 * wd.abs() * (xh.abs() + canc + 1.0))


def ln_fwd32(x, w, D):
    """the forward's formula in plain fp32 torch"""
    xf, wf = x[:, :D].float(), w[:D].float()
    mean = xf.sum(-1) / D
    d = xf - mean[:, None]
    rstd = torch.rsqrt((d * d).sum(-1) / D + torch.tensor(LN_EPS, dtype=F32))
    return mean, rstd, d * rstd[:, None] * wf


def ln_bwd64(dy, x, w, D, dx_in=None):
    """fp64 autograd of LayerNorm on dy [rows, D] (row order of x; zero rows where there is no gradient) and its units.
    dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy w: every term carries the forward's cancellation (1 + |mean| rstd) through
    xhat and rstd, at the size of the row's largest |g| (the two row means are sums of D such terms)."""
    xr = x[:, :D].double().requires_grad_(True)
    wr = w[:D].double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xr, (D,), wr, None, LN_EPS)
    y.backward(dy.double())
    f = ln_fwd64(x, w, D)
    g = (dy.double() * w[:D].double()).abs()
    canc = 1.0 + (f["mean"].abs() * f["rstd"])[:, None]
    u_dx = EPS32 * f["rstd"][:, None] * g.max(-1, keepdim=True).values.clamp_min(FLT_MIN) * (1.0 + f["xh"].abs()) * canc
    dx = xr.grad if dx_in is None else xr.grad + dx_in[:, :D].double()
    if dx_in is not None:
        u_dx = u_dx + EPS32 * dx.abs()
    u_dw = EPS32 * (dy.double().abs() * (f["xh"].abs() + canc)).sum(0).clamp_min(FLT_MIN)      # (xhat's error is absolute, like y's)
    return dict(dx=dx, dw=wr.grad, u_dx=u_dx, u_dw=u_dw)


def ln_bwd32(dy, x, w, D, dx_in=None):
    """the backward's formula in plain fp32 torch (statistics from ln_fwd32, like the kernel takes them from the forward)"""
    mean, rstd, _ = ln_fwd32(x, w, D)
    xh = (x[:, :D].float() - mean[:, None]) * rstd[:, None]
    d = dy.float()
    g = d * w[:D].float()
    c1, c2 = g.sum(-1, keepdim=True) / D, (g * xh).sum(-1, keepdim=True) / D
    dx = rstd[:, None] * (g - c1 - xh * c2)
    if dx_in is not None:
        dx = dx + dx_in[:, :D].float()
    return dx, (d * xh).sum(0)


def ln_exact_inputs(rows, D, L=1):
    """integers: x in [-4, 4], dy in [-4, 4] per layer, w in [1, 3]; with mean = 0 and rstd = 1 handed to the backward xhat = x, and
    dw = sum_rows dy x is an integer of at most 16 rows <= 2^24 in any order"""
    assert 16 * rows < 2 ** 24
    g = gen("ln exact", rows, D, L)
    x = torch.randint(-4, 5, (rows, D), generator=g).float()
    dys = [torch.randint(-4, 5, (rows, D), generator=g).to(BF16) for _ in range(L)]
    ws = [torch.randint(1, 4, (D,), generator=g).float() for _ in range(L)]
    dw0 = [torch.randint(-64, 65, (D,), generator=g).float() for _ in range(L)]
    return x, dys, ws, dw0


def colsum_emul(parts, chunk=64, lose=None, order="kernel"):
    """fp32 restatement of colsum_launch: levels of `chunk` rows summed in order.  lose = (level, row): the planted error skips
    that partial row at that level."""
    level = 0
    parts = parts.float()
    while True:
        n = parts.shape[0]
        if lose is not None and lose[0] == level:
            keep = torch.ones(n, dtype=torch.bool)
            keep[lose[1]] = False
            parts = parts * keep[:, None]
        if n <= chunk:
            break
        nc = (n + chunk - 1) // chunk
        mid = torch.zeros(nc, parts.shape[1])
        for b in range(nc):
            blk = parts[b * chunk:(b + 1) * chunk]
            mid[b] = blk.sum(0) if order == "pairwise" else (blk.flip(0) if order == "reverse" else blk).cumsum(0)[-1]
        parts, level = mid, level + 1
    return parts.sum(0) if order == "pairwise" else (parts.flip(0) if order == "reverse" else parts).cumsum(0)[-1]


def e4m3_rows(y):
    """host model of the row quantiser on bf16 rows y: scale = amax / 448 (1 for a zero row), q = e4m3(y / scale), in fp32"""
    yf = y.float()
    amax = yf.abs().max(-1).values
    sc = torch.where(amax > 0, amax * torch.tensor(1.0 / 448.0, dtype=F32), torch.ones_like(amax))
    q = (yf * (1.0 / sc)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, sc


# ---------------------------------------------------------------------------------------------------------------- SwiGLU
SWIGLU_BS = (1.0, -1.5, 2.0 ** -20, 2.0 ** 20, 0.0)
# sigmoid(a) = 1 / (1 + exp(-a)) drops below the smallest normal fp32 at a = -87.34 and exp(-a) leaves fp32 at a = -88.73: from there
# the formula (or the hardware's flush of subnormals) may return 0 where silu(a) = a sigmoid(a) is still up to 89 x 2^-126 in size
SILU_FLOOR = 89.0 * FLT_MIN


def silu64(a):
    ad = a.double()
    return ad * torch.sigmoid(ad)


def silu32(a):
    """the kernel's formula in plain fp32 torch"""
    af = a.float()
    return af * (1.0 / (1.0 + torch.exp(-af)))


def swiglu_want(a, b, inner=True):
    """bf16(bf16(silu64(a)) b) - inner = False: the planted error without the inner rounding"""
    s = silu64(a)
    s = s.to(BF16).double() if inner else s
    return (s * b.double()).to(BF16)


def _bf16_step(t, k):
    """the bf16 value k places from t in value order (t finite)"""
    b = ibits(t).to(torch.int32) & 0xFFFF
    o = torch.where(b >= 0x8000, 0x7FFF - (b & 0x7FFF), b + 0x8000) + k          # monotone in value; -0 = 0x7FFF, +0 = 0x8000
    o = o.clamp(0x7FFF - 0x7F7F, 0x8000 + 0x7F7F)
    b2 = torch.where(o >= 0x8000, o - 0x8000, 0x8000 | (0x7FFF - o))
    return torch.where(b2 >= 0x8000, b2 - 0x10000, b2).to(torch.int16).view(BF16)


def swiglu_need(h, a, b):
    """smallest |error| of silu(a) BEFORE its bf16 rounding that explains h = bf16(bf16(silu) b): over the bf16 values t within two
    places of bf16(silu64(a)) whose product with b rounds to h, the distance from silu64(a) to the reals rounding to t.  inf where
    no such t exists - a result that is not `bf16(some bf16 value near silu(a)) x b)` at all."""
    s = silu64(a)
    t0 = s.to(BF16)
    best = torch.where((t0.float() * b.float()).to(BF16).float() == h.float(), torch.zeros_like(s), torch.full_like(s, float("inf")))
    todo = (best != 0).nonzero().flatten()                   # (the correctly rounded t explains most elements at no cost)
    if todo.numel():
        st, ht, bt, part = s[todo], h[todo].float(), b[todo].float(), best[todo]
        for k in (-1, 1, -2, 2):
            t = _bf16_step(t0[todo], k)
            ok = (t.float() * bt).to(BF16).float() == ht
            part = torch.where(ok, torch.minimum(part, need_bf16(t, st)), part)
        # a silu flushed to zero (see SILU_FLOOR): t = 0 with the sign of silu(a), at the cost of |silu(a)| beyond zero's cell
        z = torch.where(torch.signbit(st), -torch.zeros_like(st), torch.zeros_like(st)).to(BF16)
        ok = (z.float() * bt).to(BF16).float() == ht
        part = torch.where(ok, torch.minimum(part, need_bf16(z, st)), part)
        best[todo] = part
    return best, EPS32 * s.abs().clamp_min(FLT_MIN)


def swiglu_bwd64(a, b, dh):
    """fp64 da = dh b s (1 + a (1 - s)), db = dh a s and their units: the derivative's two terms s and a s (1 - s) cancel near
    a = -1.28, so da's unit is built from their magnitudes, not from their sum.  Floors: s below 2^-126 may be flushed."""
    ad, bd, gd = a.double(), b.double(), dh.double()
    s = torch.sigmoid(ad)
    one_m = torch.sigmoid(-ad)                               # 1 - s without cancellation
    da = gd * bd * s * (1.0 + ad * one_m)
    db = gd * ad * s
    u_da = EPS32 * ((gd * bd).abs() * s * (1.0 + ad.abs() * one_m + ad.abs())).clamp_min(FLT_MIN)
    u_db = EPS32 * db.abs().clamp_min(FLT_MIN)
    fl = FLT_MIN * (1.0 + ad.abs())
    return dict(da=da, db=db, u_da=u_da, u_db=u_db, floor_da=(gd * bd).abs() * fl + FLT_MIN, floor_db=gd.abs() * fl + FLT_MIN)


def swiglu_bwd32(a, b, dh):
    """the kernel's formula in plain fp32 torch"""
    af, bf, gf = a.float(), b.float(), dh.float()
    s = 1.0 / (1.0 + torch.exp(-af))
    return gf * bf * s * (1.0 + af * (1.0 - s)), gf * af * s


def swiglu_sweep_inputs():
    """a = every finite bf16 value (65,280 = 255 rows of 256), b and dh seeded"""
    a = all_finite_bf16()
    g = gen("swiglu sweep")
    b = (torch.randn(a.numel(), generator=g) * 1.5).to(BF16)
    dh = torch.randn(a.numel(), generator=g).to(BF16)
    return a, b, dh


def swiglu_shape_inputs(rows, F):
    """ab [rows, 2F] bf16, seeded: a = 4 randn, b = 1.5 randn"""
    g = gen("swiglu shape", rows, F)
    a = (torch.randn(rows, F, generator=g) * 4.0).to(BF16)
    b = (torch.randn(rows, F, generator=g) * 1.5).to(BF16)
    return torch.cat([a, b], 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------- casts
def cast_inputs(n):
    """fp32 bit patterns: seeded random bits (NaN patterns replaced by bf16 ties), then planted ties both ways, subnormals, infinities"""
    bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=gen("cast", n), dtype=torch.int64).to(torch.int32)
    is_nan = ((bits >> 23) & 0xFF == 0xFF) & ((bits & 0x7FFFFF) != 0)
    bits = torch.where(is_nan, (bits & 0x3FFF0000) | 0x8000, bits)
    special = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00000001, 0x00008000, 0x00018000, 0x807FFFFF, 0x00400000,
                            0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x7F7F8000, 0x00808000], dtype=torch.int64)
    k = min(n, special.numel())
    bits[:k] = torch.where(special[:k] >= 2 ** 31, special[:k] - 2 ** 32, special[:k]).to(torch.int32)
    if n > 16:
        bits[n - k:] = bits[:k]                              # the same values at the very end (the grid-stride loop's last trip)
    return bits.view(F32)


CAST_W_CASES = [(1, 1), (31, 33), (32, 32), (341, 128), (65, 1030)]
