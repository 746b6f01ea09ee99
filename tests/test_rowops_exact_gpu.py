"""Conformance tests of the oldest row and loss kernels of egom2p_amd/csrc/rowops.hip on the GPU: cross-entropy (ce_fwd, ce_bwd,
ce_fwd_bwd), loss_weights / loss_finalize, the bias-free LayerNorm (single and multi-layer, with its e4m3 side output and the ordered
column sums behind dw), SwiGLU and the two casts.

Every buffer a kernel touches sits in a frame: rows before and after, pad columns behind the width wherever the entry point takes a
pitch.  Input frames hold NaN bits, output frames a bit pattern no result can be; after every call the frame must be untouched and
every owned element written.  Exact cases are compared bit for bit; numeric cases per element / per row on the host in fp64, as a
deviation in fp32 roundings held to FACTOR x the deviation the plain fp32 CPU evaluation shows (tests/_rowops_ref.py; the CPU half,
tests/test_rowops_exact_cpu.py, proves what this file relies on)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _rowops_ref as R  # noqa: E402
from conftest import bar  # noqa: E402
from egom2p_amd import _lib as L  # noqa: E402
from egom2p_amd import ops  # noqa: E402

DEV = "cuda"
BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32


def sent1(n, dtype, bits, lo=0, hi=0):
    """1-D buffer of the bit pattern with `lo` / `hi` frame elements round its [n] middle: (buffer, middle)"""
    buf = torch.empty(lo + n + hi, dtype=dtype, device=DEV)
    R.ibits(buf).fill_(R.sbits(bits, buf.element_size()))
    return buf, buf[lo:lo + n]


def check_frame(buf, bits, owned, what):
    intact, written = R.frame_intact(buf, bits, owned)
    assert intact, f"{what}: written outside the owned region"
    assert written, f"{what}: an owned element was not written"


def owned_rows(buf, r0, n, width=None):
    m = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    if buf.dim() == 1:
        m[r0:r0 + n] = True
    else:
        m[r0:r0 + n, :buf.shape[1] if width is None else width] = True
    return m


def eq_bits(a, b):
    return torch.equal(R.ibits(a), R.ibits(b))


def first_diff(a, b):
    bad = (R.ibits(a) != R.ibits(b)).nonzero()
    return f"{bad.shape[0]} elements differ, first at {bad[0].tolist()}: got {a[tuple(bad[0])].item()!r}, want {b[tuple(bad[0])].item()!r}"


# ================================================================================================================ cross-entropy
def _ce_coef(pad, n):
    """(gscale, n_mods, loss_w or None, coef): the 1 / n_mods path on ld = V, the loss_w path on ld = V + 8; all powers of two"""
    if pad == 0:
        return 8.0, 4, None, 8.0 * 0.25 / n
    return 0.25, 3, 0.5, 0.25 * 0.5 / n


def _ce_run(base, ld, V, targets, rng, max_rows, gscale, n_mods, lw, one_pass):
    total = base.shape[0]
    lg = base.clone()
    lse_b, _ = sent1(total, F32, R.SENT_F32)
    nll_b, _ = sent1(total, F32, R.SENT_F32)
    gs = torch.tensor([gscale], device=DEV)
    lwt = None if lw is None else torch.tensor([lw], device=DEV)
    if one_pass:
        ops.ce_fwd_bwd(lg, ld, V, targets, rng, max_rows, lse_b, nll_b, gs, n_mods, lwt)
    else:
        ops.ce_fwd(lg, ld, V, targets, rng, max_rows, lse_b, nll_b)
        ops.ce_bwd(lg, ld, V, targets, rng, max_rows, lse_b, gs, n_mods, lwt)
    torch.cuda.synchronize()
    return lg, lse_b, nll_b


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("V", R.CE_VS)
def test_ce_spike_rows_exact(V, pad):
    """a row of -200 with one 0: lse = 0, nll = 0 or 200 and d logits = (onehot(spike) - onehot(target)) coef, bit for bit, at every
    seam of the kernels' loops; odd row offset, more workgroups than rows, NaN frame (pad column included) neither read nor changed;
    the one-pass kernel bit for bit the two-call form"""
    ld, pre, post = V + pad, 3, 2
    j, t = R.ce_spike_rows(V)
    n = j.numel()
    gscale, n_mods, lw, coef = _ce_coef(pad, n)
    base = R.ce_spike_logits(j, V, ld, pre, post, DEV)
    exp_g, exp_lse, exp_nll = R.ce_spike_expected(j, t, V, ld, pre, post, coef, DEV)
    targets = torch.full((pre + n + post,), V - 1, dtype=I32, device=DEV)
    targets[pre:pre + n] = t.to(DEV)
    rng = torch.tensor([pre, n], dtype=I32, device=DEV)
    results = []
    for one_pass in (False, True):
        if one_pass and V > 65536:
            assert not ops.ce_fusable(V)
            with pytest.raises(L.EgoHipError):
                _ce_run(base, ld, V, targets, rng, n + 5, gscale, n_mods, lw, True)
            continue
        assert ops.ce_fusable(V) == (V <= 65536)
        lg, lse_b, nll_b = _ce_run(base, ld, V, targets, rng, n + 5, gscale, n_mods, lw, one_pass)
        what = f"V={V} ld={ld} {'one-pass' if one_pass else 'two-call'}"
        assert eq_bits(lg, exp_g), f"{what} d logits: {first_diff(lg, exp_g)}"
        check_frame(lse_b, R.SENT_F32, owned_rows(lse_b, pre, n), what + " lse")
        check_frame(nll_b, R.SENT_F32, owned_rows(nll_b, pre, n), what + " nll")
        assert eq_bits(lse_b[pre:pre + n], exp_lse), f"{what} lse: {first_diff(lse_b[pre:pre + n], exp_lse)}"
        assert eq_bits(nll_b[pre:pre + n], exp_nll), f"{what} nll: {first_diff(nll_b[pre:pre + n], exp_nll)}"
        results.append((lg, lse_b, nll_b))
    if len(results) == 2:
        for a, b in zip(*results):
            assert eq_bits(a, b)
    # range cases on the same rows: n = 1 at an even offset (coef x n, still a power of two), and n = 0
    for one_pass in ((False, True) if V <= 65536 else (False,)):
        r1 = pre + 1
        lg, lse_b, nll_b = _ce_run(base, ld, V, targets, torch.tensor([r1, 1], dtype=I32, device=DEV), 4, gscale, n_mods, lw, one_pass)
        want = base.clone()
        want[r1, :V] = (exp_g[r1, :V].float() * n).to(BF16)
        assert eq_bits(lg, want), f"V={V} n=1: {first_diff(lg, want)}"
        check_frame(lse_b, R.SENT_F32, owned_rows(lse_b, r1, 1), "n=1 lse")
        check_frame(nll_b, R.SENT_F32, owned_rows(nll_b, r1, 1), "n=1 nll")
        assert float(lse_b[r1]) == 0.0 and float(nll_b[r1]) == float(exp_nll[1])
        lg, lse_b, nll_b = _ce_run(base, ld, V, targets, torch.tensor([pre, 0], dtype=I32, device=DEV), 4, gscale, n_mods, lw, one_pass)
        assert eq_bits(lg, base)
        assert R.frame_intact(lse_b, R.SENT_F32, owned_rows(lse_b, 0, 0))[0] and R.frame_intact(nll_b, R.SENT_F32, owned_rows(nll_b, 0, 0))[0]


def test_ce_refusals():
    """V = 12 is refused by every entry (16-byte chunks), a pitch that is no multiple of 8 and n_mods = 0 too; the one-pass form
    refuses 65544 (a row must fit one workgroup's registers) - and nothing is written"""
    V = 16
    lg_b, lg = R.framed(2, V, BF16, R.SENT_BF16, device=DEV)
    tg = torch.zeros(6, dtype=I32, device=DEV)
    rng = torch.tensor([2, 2], dtype=I32, device=DEV)
    lse_b, _ = sent1(6, F32, R.SENT_F32)
    nll_b, _ = sent1(6, F32, R.SENT_F32)
    gs = torch.ones(1, device=DEV)
    for bad_V, bad_ld, nm in ((12, 16, 2), (16, 12, 2), (16, 16, 0)):
        if nm:
            with pytest.raises(L.EgoHipError):
                ops.ce_fwd(lg_b, bad_ld, bad_V, tg, rng, 2, lse_b, nll_b)
        with pytest.raises(L.EgoHipError):
            ops.ce_bwd(lg_b, bad_ld, bad_V, tg, rng, 2, lse_b, gs, nm)
        with pytest.raises(L.EgoHipError):
            ops.ce_fwd_bwd(lg_b, bad_ld, bad_V, tg, rng, 2, lse_b, nll_b, gs, nm)
    assert not ops.ce_fusable(12) and not ops.ce_fusable(65544) and ops.ce_fusable(65536)
    with pytest.raises(L.EgoHipError):
        ops.ce_fwd_bwd(lg_b, 65544, 65544, tg, rng, 2, lse_b, nll_b, gs, 2)
    torch.cuda.synchronize()
    for b, bits in ((lg_b, R.SENT_BF16), (lse_b, R.SENT_F32), (nll_b, R.SENT_F32)):
        assert R.frame_intact(b, bits, torch.zeros(b.shape, dtype=torch.bool, device=DEV))[0]


@pytest.mark.parametrize("V", [2056, 64000])
def test_ce_numeric_rows(V):
    """bf16(sigma randn + shift) logits, one row's maximum in the last chunk: lse and nll per row, d logits per element against fp64
    inside the envelope, with the loss_w and the 1 / n_mods coefficient; ld = V + 8 with a NaN pad column"""
    worst = dict(lse=0.0, nll=0.0, grad=0.0)
    pre, post, ld = 1, 2, V + 8
    for sigma in (2.0, 8.0):
        for shift in (0.0, 100.0, -100.0):
            x, tgt = R.ce_numeric_logits(V, sigma, shift)
            n = x.shape[0]
            base, mid = R.framed(n, ld, BF16, R.NAN_BF16, pre, post, DEV)
            mid[:, :V] = x.to(DEV)
            targets = torch.zeros(pre + n + post, dtype=I32, device=DEV)
            targets[pre:pre + n] = tgt.to(DEV)
            rng = torch.tensor([pre, n], dtype=I32, device=DEV)
            for gscale, n_mods, lw in ((1024.0, 4, None), (1024.0, 3, 0.625)):
                coef = float(np.float32(gscale) * np.float32(lw if lw is not None else np.float32(1.0) / np.float32(n_mods)) / np.float32(n))
                m = R.ce_model64(x, tgt, coef)
                got = {}
                for one_pass in (False, True):
                    lg, lse_b, nll_b = _ce_run(base, ld, V, targets, rng, n + 3, gscale, n_mods, lw, one_pass)
                    owned = owned_rows(lg, pre, n, V)
                    assert bool((R.ibits(lg)[~owned] == R.sbits(R.NAN_BF16, 2)).all()), "NaN frame of the logits changed"
                    check_frame(lse_b, R.SENT_F32, owned_rows(lse_b, pre, n), "lse")
                    check_frame(nll_b, R.SENT_F32, owned_rows(nll_b, pre, n), "nll")
                    got[one_pass] = (lg, lse_b, nll_b)
                for a, b in zip(got[False], got[True]):
                    assert eq_bits(a, b), "one-pass CE differs from the two-call form"
                lg, lse_b, nll_b = got[True]
                lse, nll, g = lse_b[pre:pre + n].cpu().double(), nll_b[pre:pre + n].cpu().double(), lg[pre:pre + n, :V].cpu()
                d = dict(lse=R.deviation((lse - m["lse"]).abs(), m["u_lse"]), nll=R.deviation((nll - m["nll"]).abs(), m["u_nll"]),
                         grad=R.deviation(R.need_bf16(g, m["grad"]), m["u_grad"], m["floor_grad"]))
                print(f"CE V={V} sigma={sigma} shift={shift} lw={lw}: deviation", {k: round(v, 3) for k, v in d.items()})
                for k in d:
                    worst[k] = max(worst[k], d[k])
    for k in worst:
        bar(f"rowops_ce_{k}_V{V}", worst[k], hard=R.envelope("ce_" + k))


# ================================================================================================================ loss_finalize
def _lf_call(nll_d, ranges, lw=None, ms=None, err=None):
    nm = len(ranges)
    rt = torch.tensor([v for r in ranges for v in r], dtype=I32, device=DEV)
    out_b, out = sent1(1 + nm, F32, R.SENT_F32, 2, 2)
    ops.loss_finalize(nll_d, rt, nm, out, err=err, loss_w=lw, mod_scale=ms)
    torch.cuda.synchronize()
    check_frame(out_b, R.SENT_F32, owned_rows(out_b, 2, 1 + nm), f"loss_finalize out, {nm} modalities")
    return out.cpu().numpy()


def test_loss_finalize_exact_ranges():
    """integer nll in 0..7 inside 56 ranges (every offset residue mod 4 x every n), NaN everywhere else: each per-modality mean within
    1 ulp of float32(sum) / float32(n) - a dropped or doubled row moves it by at least 1 / n of a unit - in calls of 1, 2 and 8
    modalities; out[0] within 1 ulp of the fp32 mean of the reported means; the lw / ms path; the err flag"""
    nll, ranges, sums = R.lf_layout()
    nll_d = nll.to(DEV)
    want = [R.lf_mean(s, n) for s, (_, n) in zip(sums, ranges)]
    order = torch.randperm(len(ranges), generator=R.gen("lf order")).tolist()      # mix residues and sizes within a call
    calls = [order[i:i + 8] for i in range(0, 56, 8)] + [order[i:i + 2] for i in range(0, 56, 2)] + [[i] for i in range(56)]
    for idx in calls:
        out = _lf_call(nll_d, [ranges[i] for i in idx])
        for k, i in enumerate(idx):
            assert R.ulps32(out[1 + k], want[i]) <= 1.0, (ranges[i], out[1 + k], want[i], "in a call of", len(idx))
        tot = np.float32(0.0)
        for k in range(len(idx)):
            tot = np.float32(tot + out[1 + k])
        assert R.ulps32(out[0], tot / np.float32(len(idx))) <= 1.0, (idx, out[0], tot)
    # lw / ms: out[1 + m] = ms[m] mean[m] (one rounding), out[0] = sum lw[m] mean[m]: a mean within 1 ulp, a product and an add per
    # modality at half an ulp each -> (2 n_mods + 2) half-ulps of the sum of the terms' magnitudes
    idx = order[:8]
    g = R.gen("lf lw")
    lw, ms = torch.rand(8, generator=g) + 0.25, torch.rand(8, generator=g) + 0.5
    out = _lf_call(nll_d, [ranges[i] for i in idx], lw=lw.to(DEV), ms=ms.to(DEV))
    means = np.array([want[i] for i in idx], np.float64)
    for k in range(8):
        assert R.ulps32(out[1 + k], np.float32(ms[k].item() * means[k])) <= 2.0, (k, out[1 + k])
    ref0 = float((lw.double().numpy() * means).sum())
    assert abs(float(out[0]) - ref0) <= (2 * 8 + 2) * R.EPS32 * float((lw.double().numpy() * means).sum()), (out[0], ref0)
    # a set err flag: every output NaN, the flag cleared, the next call clean
    err = torch.ones(1, dtype=I32, device=DEV)
    out = _lf_call(nll_d, [ranges[i] for i in idx], err=err)
    assert np.isnan(out).all() and int(err.item()) == 0
    out = _lf_call(nll_d, [ranges[i] for i in idx], err=err)
    assert all(R.ulps32(out[1 + k], want[i]) <= 1.0 for k, i in enumerate(idx)) and np.isfinite(out[0]) and int(err.item()) == 0
    # n = 0 gives 0
    out = _lf_call(nll_d, [(7, 0), (2, 0)])
    assert (out == 0).all()
    for nm in (0, 9):
        with pytest.raises(L.EgoHipError):
            ops.loss_finalize(nll_d, torch.zeros(18, dtype=I32, device=DEV), nm, torch.zeros(10, device=DEV))


def test_loss_weights():
    """mode 1: ms = ln 256 / ln V, lw = ms / n_mods; mode 2: lw = rows V / sum rows V, ms = 1; against fp64 within 4 fp32 ulp (the
    fp32 logarithm and its constant, one division, one more for lw: at most half an ulp each from correctly rounded operations, one
    or two for logf); all-empty ranges in mode 2 give NaN; bad modes, vocab < 2 and 0 / 9 modalities are refused"""
    vocab = [2, 256, 64000, 65536, 1024, 8200, 3, 100000]
    rows = [0, 1, 7, 4099, 65536, 12, 300, 5]
    for nm in (1, 2, 8):
        rt = torch.tensor([v for m in range(nm) for v in (11 * m + 1, rows[m])], dtype=I32, device=DEV)
        for mode in (1, 2):
            if mode == 2 and nm == 1:
                rt[1] = 9
            lw_b, lw = sent1(nm, F32, R.SENT_F32, 2, 2)
            ms_b, ms = sent1(nm, F32, R.SENT_F32, 2, 2)
            ops.loss_weights(rt, vocab[:nm], mode, lw, ms)
            torch.cuda.synchronize()
            check_frame(lw_b, R.SENT_F32, owned_rows(lw_b, 2, nm), "loss_w")
            check_frame(ms_b, R.SENT_F32, owned_rows(ms_b, 2, nm), "mod_scale")
            r = rt.cpu().double()[1::2]
            v = torch.tensor(vocab[:nm], dtype=F64)
            if mode == 1:
                ms_ref = np.log(256.0) / torch.log(v).numpy()
                lw_ref = ms_ref / nm
            else:
                ms_ref = np.ones(nm)
                lw_ref = (r * v / (r * v).sum()).numpy()
            assert (R.ulps32(ms.cpu().numpy(), ms_ref.astype(np.float32)) <= 4.0).all(), (mode, nm, ms.cpu(), ms_ref)
            nz = lw_ref != 0
            assert (R.ulps32(lw.cpu().numpy()[nz], lw_ref.astype(np.float32)[nz]) <= 4.0).all(), (mode, nm, lw.cpu(), lw_ref)
            assert (lw.cpu().numpy()[~nz] == 0).all()
    empty = torch.tensor([3, 0, 9, 0], dtype=I32, device=DEV)
    lw, ms = torch.zeros(2, device=DEV), torch.zeros(2, device=DEV)
    ops.loss_weights(empty, [256, 1024], 2, lw, ms)
    assert bool(torch.isnan(lw).all()) and bool((ms == 1).all())
    for bad in (dict(mode=0), dict(mode=3), dict(vocab=[256, 1]), dict(vocab=[]), dict(vocab=[4] * 9)):
        with pytest.raises(L.EgoHipError):
            ops.loss_weights(torch.zeros(18, dtype=I32, device=DEV), bad.get("vocab", [256, 1024]), bad.get("mode", 1),
                             torch.zeros(9, device=DEV), torch.zeros(9, device=DEV))


# ================================================================================================================ LayerNorm
def _ln_device_inputs(x, w, dy, perm):
    rows, ld = x.shape
    xb, xm = R.framed(rows, ld, F32, R.NAN_F32, device=DEV)
    xm.copy_(x)
    dyb, dym = R.framed(rows, ld, BF16, R.NAN_BF16, device=DEV)       # stored in the permuted row order; a row nobody maps to stays NaN
    if perm is None:
        dym.copy_(dy)
    else:
        keep = perm >= 0
        dym[perm[keep].long().to(DEV)] = dy[keep].to(DEV)
    return xm, w.to(DEV), dym, None if perm is None else perm.to(DEV)


def _ln_forward(xm, wd, permd, D, q8=False):
    rows, ld = xm.shape
    yb, ym = R.framed(rows, ld, BF16, R.SENT_BF16, device=DEV)
    mb, mean = sent1(rows, F32, R.SENT_F32, 3, 3)
    rb, rstd = sent1(rows, F32, R.SENT_F32, 3, 3)
    qb = qm = sb = qs = None
    if q8:
        qb, qm = R.framed(rows, ld, torch.uint8, R.SENT_U8, device=DEV)
        sb, qs = sent1(rows, F32, R.SENT_F32, 3, 3)
    ops.layernorm_fwd(xm, wd, ym, mean, rstd, out_row=permd, eps=R.LN_EPS, width=D, q8=qm, qscale=qs)
    torch.cuda.synchronize()
    check_frame(mb, R.SENT_F32, owned_rows(mb, 3, rows), "mean")
    check_frame(rb, R.SENT_F32, owned_rows(rb, 3, rows), "rstd")
    written = torch.ones(rows, dtype=torch.bool, device=DEV)
    if permd is not None:
        written[:] = False
        written[permd[permd >= 0].long()] = True
    own = torch.zeros(yb.shape, dtype=torch.bool, device=DEV)
    own[2:2 + rows][written] = True
    check_frame(yb, R.SENT_BF16, own, "y")
    if q8:
        own = torch.zeros(qb.shape, dtype=torch.bool, device=DEV)
        own[2:2 + rows][written] = True
        check_frame(qb, R.SENT_U8, own, "q8")
        own = torch.zeros(sb.shape, dtype=torch.bool, device=DEV)
        own[3:3 + rows][written] = True
        check_frame(sb, R.SENT_F32, own, "qscale")
    return ym, mean, rstd, qm, qs, written


def _ln_backward(dym, permd, xm, mean, rstd, wd, D, dx_in=None, dw0=None):
    rows, ld = xm.shape
    dxb_, dx = R.framed(rows, ld, F32, R.SENT_F32, device=DEV)
    dhb_, dxh = R.framed(rows, ld, BF16, R.SENT_BF16, device=DEV)
    dwb, dw = sent1(ld, F32, R.SENT_F32, 4, 4)
    dw.zero_()
    if dw0 is not None:
        dw[:D] = dw0.to(DEV)
    ops.layernorm_bwd(dym, xm, mean, rstd, wd, dx, dw, dx_in=dx_in, dx_bf16=dxh, dy_row=permd, width=D)
    torch.cuda.synchronize()
    check_frame(dxb_, R.SENT_F32, owned_rows(dxb_, 2, rows), "dx")
    check_frame(dhb_, R.SENT_BF16, owned_rows(dhb_, 2, rows), "dx bf16")
    check_frame(dwb, R.SENT_F32, owned_rows(dwb, 4, ld), "dw")
    assert not bool(dw[D:].any()), "dw pad columns"
    return dx, dxh, dw


@pytest.mark.parametrize("D,ld", R.LN_SHAPES)
def test_layernorm_numeric_per_element(D, ld):
    """forward (mean, rstd per row; y per element; pad columns exactly zero; out_row with a -1 entry) and backward (dx fp32 and bf16
    per element with and without dx_in, dw per column, dy_row with a -1 entry) against fp64, over rows 1..33 and three input
    distributions, one of them with a mean 1000 standard deviations from zero"""
    worst = dict(mean=0.0, rstd=0.0, y=0.0, dx=0.0, dw=0.0)
    for rows in R.LN_ROWS:
        for s, m in R.LN_DISTS:
            x, w, dy = R.ln_inputs(rows, D, ld, s, m)
            perm = R.ln_perm(rows)
            xm, wd, dym, permd = _ln_device_inputs(x, w, dy, perm)
            ym, mean, rstd, _, _, written = _ln_forward(xm, wd, permd, D)
            f = R.ln_fwd64(x, w, D)
            src = torch.arange(rows) if perm is None else perm.long()
            keep = src >= 0
            y = ym.cpu()
            assert not bool(R.ibits(y[src[keep], D:]).any()), "y pad columns are not +0"
            d = dict(mean=R.deviation((mean.cpu().double() - f["mean"]).abs(), f["u_mean"]),
                     rstd=R.deviation((rstd.cpu().double() - f["rstd"]).abs(), f["u_rstd"]),
                     y=R.deviation(R.need_bf16(y[src[keep], :D], f["y"][keep]), f["u_y"][keep]))
            dy_eff = dy[:, :D].float() * keep[:, None]
            for with_in in (False, True):
                dx_in = None
                if with_in:
                    _, dx_in = R.framed(rows, ld, F32, R.NAN_F32, device=DEV)
                    dx_in[:, :R.ln_pad4(D)] = 0.0
                    dx_in[:, :D] = torch.randn(rows, D, generator=R.gen("dx_in", rows, D)).to(DEV)
                b = R.ln_bwd64(dy_eff, x, w, D, None if dx_in is None else dx_in.cpu())
                dx, dxh, dw = _ln_backward(dym, permd, xm, mean, rstd, wd, D, dx_in=dx_in)
                assert not bool(R.ibits(dx[:, D:]).any()) and not bool(R.ibits(dxh[:, D:]).any()), "dx pad columns are not +0"
                d["dx"] = max(d.get("dx", 0.0), R.deviation((dx[:, :D].cpu().double() - b["dx"]).abs(), b["u_dx"]),
                              R.deviation(R.need_bf16(dxh[:, :D].cpu(), b["dx"]), b["u_dx"]))
                d["dw"] = max(d.get("dw", 0.0), R.deviation((dw[:D].cpu().double() - b["dw"]).abs(), b["u_dw"]))
            for k in worst:
                worst[k] = max(worst[k], d[k])
    print(f"LayerNorm D={D} ld={ld}: worst deviation", {k: round(v, 3) for k, v in worst.items()})
    for k in worst:
        bar(f"rowops_ln_{k}", worst[k], hard=R.envelope("ln_" + k))


def test_layernorm_refusals():
    x = torch.zeros(4, 2052, device=DEV)
    w = torch.ones(2052, device=DEV)
    y_b, y = R.framed(4, 2052, BF16, R.SENT_BF16, device=DEV)
    mean, rstd = torch.zeros(4, device=DEV), torch.zeros(4, device=DEV)
    dx, dw = torch.zeros(4, 2052, device=DEV), torch.zeros(2052, device=DEV)
    with pytest.raises(L.EgoHipError):
        ops.layernorm_fwd(x, w, y, mean, rstd)                                   # ld = 2052 > 2048
    with pytest.raises(L.EgoHipError):
        ops.layernorm_bwd(y, x, mean, rstd, w, dx, dw)
    with pytest.raises(L.EgoHipError):
        ops.layernorm_fwd_multi(x, [w], [y], mean, rstd)
    with pytest.raises(L.EgoHipError):
        ops.layernorm_bwd_multi([y], x, mean, rstd, [w], dx, [dw])
    with pytest.raises(L.EgoHipError):
        ops.layernorm_bwd_multi([y[:, :1540]], x[:, :1540].contiguous(), mean, rstd, [w], dx, [dw])      # the fused backward stops at 1536
    x6 = torch.zeros(4, 126, device=DEV)
    with pytest.raises(L.EgoHipError):
        ops.layernorm_fwd(x6, w, y, mean, rstd)                                  # ld % 4
    n_max = 32           # LN_MULTI_MAX of rowops.hip (= COLSUM_MAX_DST of common.h, not exported): keep in step with that constant
    xs = torch.zeros(4, 128, device=DEV)
    ys = [torch.zeros(4, 128, device=DEV, dtype=BF16) for _ in range(n_max + 1)]
    ws = [torch.ones(128, device=DEV) for _ in range(n_max + 1)]
    with pytest.raises(L.EgoHipError):
        ops.layernorm_fwd_multi(xs, ws, ys, mean, rstd)
    with pytest.raises(L.EgoHipError):
        ops.layernorm_bwd_multi(ys, xs, mean, rstd, ws, torch.zeros(4, 128, device=DEV), [torch.zeros(128, device=DEV) for _ in ws])
    # the e4m3 side output needs ld == D
    xq = torch.zeros(4, 256, device=DEV)
    q8, qs = torch.zeros(4, 256, device=DEV, dtype=torch.uint8), torch.zeros(4, device=DEV)
    with pytest.raises(L.EgoHipError):
        ops.layernorm_fwd(xq, w, y, mean, rstd, width=252, q8=q8, qscale=qs)
    torch.cuda.synchronize()
    assert R.frame_intact(y_b, R.SENT_BF16, torch.zeros(y_b.shape, dtype=torch.bool, device=DEV))[0]


@pytest.mark.parametrize("rows,L_", [(33, 0), (2080, 0), (2080, 1), (2080, 12), (2080, 32)])
def test_layernorm_backward_dw_exact(rows, L_):
    """mean = 0, rstd = 1 handed to the backward with integer x and dy: dw = start + sum_rows dy x is an integer below 2^24 and must
    come out bit for bit - 2080 rows are 65 partial rows of the single-layer kernel and 260 of the multi-layer one, past
    colsum_kernel's 64-row chunk (its second level); L_ = 0: the single-layer entry, else the multi-layer one with L_ layers"""
    D = 128
    x, dys, ws, dw0 = R.ln_exact_inputs(rows, D, max(L_, 1))
    xd = x.to(DEV)
    mean, rstd = torch.zeros(rows, device=DEV), torch.ones(rows, device=DEV)
    dx = torch.empty(rows, D, device=DEV)
    want = [(dw0[l].double() + (dys[l].double() * x.double()).sum(0)).float() for l in range(len(dys))]
    bufs = [sent1(D, F32, R.SENT_F32, 4, 4) for _ in dys]
    for (b, dw), s in zip(bufs, dw0):
        dw.copy_(s)
    if L_ == 0:
        ops.layernorm_bwd(dys[0].to(DEV), xd, mean, rstd, ws[0].to(DEV), dx, bufs[0][1])
    else:
        ops.layernorm_bwd_multi([d.to(DEV) for d in dys], xd, mean, rstd, [w.to(DEV) for w in ws], dx, [dw for _, dw in bufs])
    torch.cuda.synchronize()
    for l, (b, dw) in enumerate(bufs):
        check_frame(b, R.SENT_F32, owned_rows(b, 4, D), f"dw of layer {l}")
        assert eq_bits(dw.cpu(), want[l]), f"rows={rows} layers={L_} layer {l}: {first_diff(dw.cpu(), want[l])}"


@pytest.mark.parametrize("D,ld", R.LN_SHAPES)
def test_layernorm_multi_is_the_chained_single(D, ld):
    """ego_layernorm_fwd_multi / _bwd_multi against the chained single-layer calls on the new widths and every row count: y, mean,
    rstd, dx and its bf16 copy bit for bit (with and without dx_in); each layer's dw per column against fp64 inside the envelope
    (its partial rows are cut by the fused kernel's own workgroups, so it is not the chained calls' bits), pad columns of dw
    untouched zeros, frames intact; the fused backward stops at a pitch of 1536"""
    Lyr = 3
    worst_dw = 0.0
    for rows in R.LN_ROWS:
        x, ws_c, dys_c = R.ln_multi_inputs(rows, D, ld, Lyr)
        _, xm = R.framed(rows, ld, F32, R.NAN_F32, device=DEV)
        xm.copy_(x)
        ws, dys = [w.to(DEV) for w in ws_c], [d.to(DEV) for d in dys_c]
        ys1 = [R.framed(rows, ld, BF16, R.SENT_BF16, device=DEV) for _ in range(Lyr)]
        ys2 = [R.framed(rows, ld, BF16, R.SENT_BF16, device=DEV) for _ in range(Lyr)]
        m1, r1, m2, r2 = (torch.empty(rows, device=DEV) for _ in range(4))
        for l in range(Lyr):
            ops.layernorm_fwd(xm, ws[l], ys1[l][1], m1, r1, width=D)
        ops.layernorm_fwd_multi(xm, ws, [y for _, y in ys2], m2, r2, width=D)
        torch.cuda.synchronize()
        assert eq_bits(m1, m2) and eq_bits(r1, r2)
        for l in range(Lyr):
            assert eq_bits(ys1[l][0], ys2[l][0]), (rows, l)                      # frames included
            check_frame(ys2[l][0], R.SENT_BF16, owned_rows(ys2[l][0], 2, rows), "y of the fused forward")
        if ld > 1536:
            with pytest.raises(L.EgoHipError):
                ops.layernorm_bwd_multi(dys, xm, m2, r2, ws, torch.empty(rows, ld, device=DEV), [torch.zeros(ld, device=DEV) for _ in ws])
            continue
        refs = [R.ln_bwd64(dys_c[l][:, :D].float(), x, ws_c[l], D) for l in range(Lyr)]
        for with_in in (False, True):
            base = None
            if with_in:
                base = torch.zeros(rows, ld, device=DEV)
                base[:, :D] = torch.randn(rows, D, generator=R.gen("multi base", rows, D)).to(DEV)
            dx1, dxh1 = torch.empty(rows, ld, device=DEV), torch.empty(rows, ld, device=DEV, dtype=BF16)
            for k, l in enumerate(reversed(range(Lyr))):
                ops.layernorm_bwd(dys[l], xm, m1, r1, ws[l], dx1, torch.zeros(ld, device=DEV), dx_in=None if k == 0 else dx1, dx_bf16=dxh1, width=D)
            if with_in:                                                          # the fused kernel adds dx_in last: so does the chain
                dx1 = dx1 + base
                dxh1 = dx1.to(BF16)
            d2b, dx2 = R.framed(rows, ld, F32, R.SENT_F32, device=DEV)
            h2b, dxh2 = R.framed(rows, ld, BF16, R.SENT_BF16, device=DEV)
            dws = [sent1(ld, F32, R.SENT_F32, 4, 4) for _ in range(Lyr)]
            for _, dw in dws:
                dw.zero_()
            ops.layernorm_bwd_multi(dys, xm, m2, r2, ws, dx2, [dw for _, dw in dws], dx_in=base, dx_bf16=dxh2, width=D)
            torch.cuda.synchronize()
            check_frame(d2b, R.SENT_F32, owned_rows(d2b, 2, rows), "dx of the fused backward")
            check_frame(h2b, R.SENT_BF16, owned_rows(h2b, 2, rows), "bf16 dx of the fused backward")
            assert eq_bits(dx1, dx2), f"rows={rows} dx_in={with_in}: {first_diff(dx2, dx1)}"
            assert eq_bits(dxh1, dxh2)
            for l, (dwb, dw) in enumerate(dws):
                check_frame(dwb, R.SENT_F32, owned_rows(dwb, 4, ld), f"dw of layer {l} of the fused backward")
                assert not bool(R.ibits(dw[D:]).any()), f"rows={rows} layer {l}: dw pad columns"
                dev = R.deviation((dw[:D].cpu().double() - refs[l]["dw"]).abs(), refs[l]["u_dw"])
                assert dev <= R.envelope("ln_dw"), (rows, l, with_in, dev, int((dw[:D].cpu().double() - refs[l]["dw"]).abs().argmax()))
                worst_dw = max(worst_dw, dev)
    if ld <= 1536:
        print(f"fused LayerNorm backward D={D} ld={ld}: worst dw deviation {worst_dw:.3f}")
        bar("rowops_ln_multi_dw", worst_dw, hard=R.envelope("ln_dw"))


@pytest.mark.parametrize("D", [256, 768, 1024])
def test_layernorm_e4m3_side_output(D):
    """q8 / qscale of the forward: bit for bit what ops.quant_fp8_rows makes of the y the same call wrote, and what the host e4m3 model
    makes of it; with and without out_row (a -1 row's qscale slot and q8 row stay untouched); an all-zero row has scale 1"""
    for rows in (5, 9):
        for use_perm in (False, True):
            x, w, dy = R.ln_inputs(rows, D, D, 2.0, 0.3)
            x[2] = 0.0                                                           # y = 0: scale 1
            perm = R.ln_perm(rows) if use_perm else None
            xm, wd, _, permd = _ln_device_inputs(x, w, dy, perm)
            ym, mean, rstd, q8, qs, written = _ln_forward(xm, wd, permd, D, q8=True)
            yw = ym[written].contiguous()
            Q = torch.empty(yw.shape, dtype=torch.uint8, device=DEV)
            sc = torch.empty(yw.shape[0], device=DEV)
            ops.quant_fp8_rows(yw, Q, sc)
            torch.cuda.synchronize()
            assert torch.equal(q8[written], Q) and eq_bits(qs[written], sc)
            hq, hs = R.e4m3_rows(yw.cpu())
            assert torch.equal(q8[written].cpu(), hq), int((q8[written].cpu() != hq).sum())
            assert eq_bits(qs[written].cpu(), hs)
            zero_row = 2 if perm is None else int(perm[2])
            if zero_row >= 0:
                assert float(qs[zero_row]) == 1.0 and not bool((q8[zero_row] & 0x7F).any())


# ================================================================================================================ SwiGLU
def _swiglu_fwd_dev(ab, rows, F):
    abb, abm = R.framed(rows, 2 * F, BF16, R.NAN_BF16, device=DEV)
    abm.copy_(ab)
    hb, h = R.framed(rows, F, BF16, R.SENT_BF16, device=DEV)
    ops.swiglu_fwd(abm, h, rows, F)
    torch.cuda.synchronize()
    check_frame(hb, R.SENT_BF16, owned_rows(hb, 2, rows), f"swiglu h rows={rows} F={F}")
    return h.cpu(), abm


def _swiglu_bwd_dev(abm, dh, rows, F):
    gb, gm = R.framed(rows, F, BF16, R.NAN_BF16, device=DEV)
    gm.copy_(dh)
    db_, dab = R.framed(rows, 2 * F, BF16, R.SENT_BF16, device=DEV)
    ops.swiglu_bwd(abm, gm, dab, rows, F)
    torch.cuda.synchronize()
    check_frame(db_, R.SENT_BF16, owned_rows(db_, 2, rows), f"swiglu dab rows={rows} F={F}")
    return dab.cpu()


# The recorded forward deviation is 0: every h is explained by the correctly rounded bf16(silu(a)).  That is what was measured, not
# the contract - a result as good as plain fp32 on the CPU is no regression, so the baseline check allows that much on top (the
# envelope, FACTOR times it, stays the hard bound).
SWIGLU_FWD_MARGIN = R.CPU_DEV["swiglu_fwd"]


def _swiglu_dev(h, a, b):
    need, unit = R.swiglu_need(h, a, b)
    return R.deviation(need, unit, R.SILU_FLOOR)


@pytest.mark.parametrize("b", R.SWIGLU_BS)
def test_swiglu_forward_over_every_finite_bf16(b):
    """a = every finite bf16 value, b fixed: h must be bf16(t b) for a bf16 t that is a rounding of silu(a) up to the envelope (where
    the inner rounding sits on a boundary that is one bf16 place of h)"""
    a = R.all_finite_bf16().reshape(255, 256)
    bt = torch.full_like(a, b)
    h, _ = _swiglu_fwd_dev(torch.cat([a, bt], 1), 255, 256)
    dev = _swiglu_dev(h.reshape(-1), a.reshape(-1), bt.reshape(-1))
    same = float((h.float() == R.swiglu_want(a, bt).float()).float().mean())
    print(f"swiglu fwd b={b}: deviation {dev:.3f}, share equal to the fp64 double rounding {same:.5f}")
    bar("rowops_swiglu_fwd", dev, hard=R.envelope("swiglu_fwd"), abs_margin=SWIGLU_FWD_MARGIN)


def test_swiglu_forward_special_values():
    """what the kernel returns beside what fp64 silu returns: +-0 -> +-0; +inf -> +inf; -inf -> NaN in both (-inf x 0; the limit is -0);
    NaN -> NaN; the largest finite value is itself, the most negative one gives -0 (fp64: -0 as well, silu underflows)"""
    vals = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 3.3895313892515355e38, -3.3895313892515355e38, -89.0]
    a = torch.tensor(vals, dtype=F32).to(BF16).reshape(1, 8)
    b = torch.ones(1, 8, dtype=BF16)
    h, _ = _swiglu_fwd_dev(torch.cat([a, b], 1), 1, 8)
    h = h[0].float()
    s64 = R.silu64(a[0])
    assert h[0] == 0 and not torch.signbit(h[0]) and s64[0] == 0
    assert h[1] == 0 and torch.signbit(h[1]) and s64[1] == 0 and torch.signbit(s64[1])
    assert h[2] == float("inf") and s64[2] == float("inf")
    assert torch.isnan(h[3]) and torch.isnan(s64[3])
    assert torch.isnan(h[4]) and torch.isnan(s64[4])
    assert h[5] == a[0, 5].float() and s64[5] == a[0, 5].double()
    assert h[6] == 0 and torch.signbit(h[6]) and s64[6] == 0
    assert abs(float(h[7]) - float(s64[7])) <= R.SILU_FLOOR and float(s64[7]) < 0       # sigmoid(-89) is below fp32's normal range


def test_swiglu_backward_over_every_finite_bf16():
    """the same sweep of a with seeded b and dh: da and db per element, with an absolute term in da's unit (the derivative's two
    terms cancel near a = -1.28)"""
    a, b, dh = R.swiglu_sweep_inputs()
    _, abm = _swiglu_fwd_dev(torch.cat([a.reshape(255, 256), b.reshape(255, 256)], 1), 255, 256)
    dab = _swiglu_bwd_dev(abm, dh.reshape(255, 256), 255, 256)
    m = R.swiglu_bwd64(a, b, dh)
    dda = R.deviation(R.need_bf16(dab[:, :256].reshape(-1), m["da"]), m["u_da"], m["floor_da"])
    ddb = R.deviation(R.need_bf16(dab[:, 256:].reshape(-1), m["db"]), m["u_db"], m["floor_db"])
    print(f"swiglu bwd: deviation da {dda:.3f}, db {ddb:.3f}")
    bar("rowops_swiglu_da", dda, hard=R.envelope("swiglu_da"))
    bar("rowops_swiglu_db", ddb, hard=R.envelope("swiglu_db"))


@pytest.mark.parametrize("rows,F", [(3, 8), (5, 264), (4100, 2056)])
def test_swiglu_shapes(rows, F):
    """F = 8, F = 8 x 33, and 4100 x 2056 = 1,053,700 chunks: more than the 4096 x 256 threads of the capped grid, so the grid-stride
    loops take a second trip; every element checked, forward and backward"""
    ab = R.swiglu_shape_inputs(rows, F)
    dh = torch.randn(rows, F, generator=R.gen("swiglu dh", rows, F)).to(BF16)
    h, abm = _swiglu_fwd_dev(ab, rows, F)
    a, b = ab[:, :F].reshape(-1), ab[:, F:].reshape(-1)
    dev = _swiglu_dev(h.reshape(-1), a, b)
    dab = _swiglu_bwd_dev(abm, dh, rows, F)
    m = R.swiglu_bwd64(a, b, dh.reshape(-1))
    dda = R.deviation(R.need_bf16(dab[:, :F].reshape(-1), m["da"]), m["u_da"], m["floor_da"])
    ddb = R.deviation(R.need_bf16(dab[:, F:].reshape(-1), m["db"]), m["u_db"], m["floor_db"])
    print(f"swiglu rows={rows} F={F}: deviation fwd {dev:.3f}, da {dda:.3f}, db {ddb:.3f}")
    bar("rowops_swiglu_fwd", dev, hard=R.envelope("swiglu_fwd"), abs_margin=SWIGLU_FWD_MARGIN)
    bar("rowops_swiglu_da", dda, hard=R.envelope("swiglu_da"))
    bar("rowops_swiglu_db", ddb, hard=R.envelope("swiglu_db"))


def test_swiglu_refusals():
    ab = torch.zeros(2, 24, device=DEV, dtype=BF16)
    hb, h = R.framed(2, 12, BF16, R.SENT_BF16, device=DEV)
    db_, dab = R.framed(2, 24, BF16, R.SENT_BF16, device=DEV)
    with pytest.raises(L.EgoHipError):
        ops.swiglu_fwd(ab, h, 2, 12)
    with pytest.raises(L.EgoHipError):
        ops.swiglu_bwd(ab, h, dab, 2, 12)
    torch.cuda.synchronize()
    assert R.frame_intact(hb, R.SENT_BF16, torch.zeros(hb.shape, dtype=torch.bool, device=DEV))[0]
    assert R.frame_intact(db_, R.SENT_BF16, torch.zeros(db_.shape, dtype=torch.bool, device=DEV))[0]


# ================================================================================================================ casts
@pytest.mark.parametrize("n", [4, 4 * 1048576 + 4 * 4097])
def test_cast_f32_bf16_bits(n):
    """bit equality with torch's round-to-nearest-even, ties, fp32 subnormals and infinities included; the larger n is more than
    4096 x 256 float4 chunks: the grid-stride loop's second trip"""
    src = R.cast_inputs(n)
    sb, sm = sent1(n, F32, R.NAN_F32, 4, 4)
    sm.copy_(src)
    db_, dm = sent1(n, BF16, R.SENT_BF16, 8, 8)
    ops.cast_f32_bf16(sm, dm)
    torch.cuda.synchronize()
    check_frame(db_, R.SENT_BF16, owned_rows(db_, 8, n), "cast_f32_bf16")
    want = src.to(BF16)
    assert eq_bits(dm.cpu(), want), first_diff(dm.cpu(), want)
    with pytest.raises(L.EgoHipError):
        ops.cast_f32_bf16(torch.zeros(8, device=DEV)[:6], torch.zeros(8, device=DEV, dtype=BF16)[:6])       # n % 4


@pytest.mark.parametrize("rows,cols", R.CAST_W_CASES)
def test_cast_weight_bits(rows, cols):
    """W -> bf16 W (rows padded with zeros to rows_dst) and W^T, with ld_src > cols (NaN pad), destination pitches wider than needed,
    rows_dst > rows; Wb only, Wt only and both: bit equality, frames untouched"""
    W = torch.randn(rows, cols, generator=R.gen("cast w", rows, cols))
    W.view(torch.int32)[0, 0] = 0x3F808000                                       # a tie
    wb_, wm = R.framed(rows, cols + 3, F32, R.NAN_F32, device=DEV)
    wm[:, :cols] = W.to(DEV)
    src = wm[:, :cols]
    Wb16 = W.to(BF16)
    for rows_dst, ld_w, ld_t in ((rows, cols, rows), (rows + 7, cols + 5, rows + 7 + 3)):
        for use_b, use_t in ((True, False), (False, True), (True, True)):
            bb, bm = R.framed(rows_dst, ld_w, BF16, R.SENT_BF16, device=DEV)
            tb, tm = R.framed(cols, ld_t, BF16, R.SENT_BF16, device=DEV)
            ops.cast_weight(src, Wb=bm if use_b else None, Wt=tm if use_t else None, rows_dst=rows_dst, ld_w=ld_w, ld_t=ld_t)
            torch.cuda.synchronize()
            eb, em = R.framed(rows_dst, ld_w, BF16, R.SENT_BF16)
            et, etm = R.framed(cols, ld_t, BF16, R.SENT_BF16)
            if use_b:
                em[:, :cols] = 0.0
                em[:rows, :cols] = Wb16
            if use_t:
                etm[:, :rows_dst] = 0.0
                etm[:, :rows] = Wb16.t()
            what = f"rows_dst={rows_dst} ld_w={ld_w} ld_t={ld_t} Wb={use_b} Wt={use_t}"
            assert eq_bits(bb.cpu(), eb), f"Wb {what}: {first_diff(bb.cpu(), eb)}"
            assert eq_bits(tb.cpu(), et), f"Wt {what}: {first_diff(tb.cpu(), et)}"
    with pytest.raises(L.EgoHipError):
        ops.cast_weight(src, Wb=torch.zeros(rows, cols, device=DEV, dtype=BF16), rows_dst=rows - 1)
