"""What tests/test_rowops_exact_gpu.py relies on, proven on the host (no GPU):
  * every "exact" input really is exact: evaluated in fp32 under several summation orders, the bits are the same and are the ones the
    GPU test expects;
  * every envelope admits the plain fp32 CPU evaluation of its family on the GPU test's own inputs - this run is where the constants
    CPU_DEV of tests/_rowops_ref.py come from;
  * the checks have teeth: a CPU emulation of each kernel with one planted error (a 16-byte chunk dropped at a loop seam, the one-hot
    on the other half of the packed pair, a head or tail row dropped or doubled, the mean over the pitch, a partial row lost at the
    second colsum level, no inner bf16 rounding) is rejected by the very check the GPU result goes through."""
import numpy as np
import pytest
import torch

import _rowops_ref as R

BF16, F32 = torch.bfloat16, torch.float32


# ---------------------------------------------------------------------------------------------------------------- exactness
def _spike_sample(V, k=12):
    """a few of the GPU test's spike rows (vocabulary-sized rows are kept to a handful on the CPU), the loop seams first"""
    j, t = R.ce_spike_rows(V)
    want = [i for i in range(j.numel()) if int(j[i]) % 2048 in (0, 2047) or int(j[i]) >= V - 2][:k - 4] + [0, 1, 2, 3]
    idx = torch.tensor(sorted(set(want)))
    return j[idx], t[idx], j.numel()


@pytest.mark.parametrize("V", [8, 2056, 64000, 65544])
def test_ce_spike_rows_are_exact_in_any_order(V):
    j, t, n_all = _spike_sample(V)
    coef = 8.0 * 0.25 / n_all
    x = R.ce_spike_logits(j, V, V, 0, 0)[:, :V].float()
    exp_g, exp_lse, exp_nll = R.ce_spike_expected(j, t, V, V, 0, 0, coef)
    assert float(torch.exp(torch.tensor(R.CE_FILL, dtype=F32))) == 0.0
    for order in ("pairwise", "reverse", "strided"):
        lse, nll, g = R.ce_emul(x, t, coef, order=order)
        assert torch.equal(R.ibits(lse), R.ibits(exp_lse)), order
        assert torch.equal(R.ibits(nll), R.ibits(exp_nll)), order
        assert torch.equal(R.ibits(g.to(BF16)), R.ibits(exp_g)), order
        assert torch.equal(g.to(BF16).float(), g), "the gradient is not exact in bf16"


def test_ce_spike_positions_cover_the_seams():
    """vc = V / 8 chunks: ce_fwd_kernel's unrolled loop ends and its remainder loop begins at a multiple of 1024 chunks (8192
    columns), each of its four loads and ce_fwd_bwd_kernel's register chunks at multiples of 256 chunks (2048 columns)"""
    assert [V // 8 for V in R.CE_VS] == [1, 255, 256, 257, 768, 1023, 1025, 8000, 8192, 8193]
    for V in R.CE_VS:
        pos = set(R.ce_spike_positions(V))
        assert set(range(min(16, V))) <= pos and set(range(max(0, V - 16), V)) <= pos
        for m in list(range(2048, V, 2048)) + list(range(8192, V, 8192)):
            assert m - 1 in pos and m in pos
        j, t = R.ce_spike_rows(V)
        n = j.numel()
        assert n & (n - 1) == 0 and n >= len(pos)
        for jj in (0, V - 1, min(5, V - 2)):                             # every target kind appears with a spike
            tt = set(t[j == jj].tolist())
            assert {jj, 0, V - 1} <= tt and (jj + 1 in tt or jj + 1 >= V) and (jj - 1 in tt or jj == 0)


def test_loss_finalize_ranges_are_exact_in_any_order():
    nll, ranges, sums = R.lf_layout()
    assert sorted({o % 4 for o, _ in ranges}) == [0, 1, 2, 3] and len(ranges) == 4 * len(R.LF_NS)
    assert bool(torch.isnan(nll).sum() == nll.numel() - sum(n for _, n in ranges))
    for (o, n), s in zip(ranges, sums):
        assert s < 2 ** 24
        want = R.lf_mean(s, n)
        for order in ("kernel", "sequential", "pairwise", "reverse"):
            assert np.float32(R.lf_emul(nll, o, n, order=order)) == want, (o, n, order)


@pytest.mark.parametrize("rows,L_", [(33, 1), (2080, 1), (2080, 12), (2080, 32)])
def test_layernorm_exact_dw_in_any_order(rows, L_):
    x, dys, ws, dw0 = R.ln_exact_inputs(rows, 128, L_)
    for l in (0, L_ - 1):
        prod = dys[l].float() * x
        want = dw0[l].double() + prod.double().sum(0)
        assert float(want.abs().max()) < 2 ** 24
        for per in (32, 8):                                  # rows per workgroup of the single-layer / the fused backward
            pad = (-rows) % per
            parts = torch.cat([prod, torch.zeros(pad, 128)]).reshape(-1, per, 128)
            for order in ("kernel", "pairwise", "reverse"):
                p = parts.sum(1) if order == "pairwise" else (parts.flip(1) if order == "reverse" else parts).cumsum(1)[:, -1]
                got = dw0[l] + R.colsum_emul(p, order=order)
                assert torch.equal(got.double(), want), (rows, L_, l, per, order)
    assert (2080 + 31) // 32 == 65 and (2080 + 7) // 8 == 260          # past colsum_kernel's 64-row chunk: a second level


# ---------------------------------------------------------------------------------------------------------------- CPU deviation
def _ce_cpu_dev():
    d = dict(ce_lse=0.0, ce_nll=0.0, ce_grad=0.0)
    for V in (2056, 64000):
        for sigma in (2.0, 8.0):
            for shift in (0.0, 100.0, -100.0):
                x, tgt = R.ce_numeric_logits(V, sigma, shift)
                n = x.shape[0]
                for gscale, k in ((1024.0, 0.25), (1024.0, 0.625)):
                    coef = float(np.float32(gscale) * np.float32(k) / np.float32(n))
                    m = R.ce_model64(x, tgt, coef)
                    lse, nll, g = R.ce_emul(x.float(), tgt, coef)
                    d["ce_lse"] = max(d["ce_lse"], R.deviation((lse.double() - m["lse"]).abs(), m["u_lse"]))
                    d["ce_nll"] = max(d["ce_nll"], R.deviation((nll.double() - m["nll"]).abs(), m["u_nll"]))
                    d["ce_grad"] = max(d["ce_grad"], R.deviation((g.double() - m["grad"]).abs(), m["u_grad"], m["floor_grad"]))
    return d


def _ln_cpu_dev():
    d = dict(ln_mean=0.0, ln_rstd=0.0, ln_y=0.0, ln_dx=0.0, ln_dw=0.0)
    for D, ld in R.LN_SHAPES:
        for rows in R.LN_ROWS:
            for s, m in R.LN_DISTS:
                x, w, dy = R.ln_inputs(rows, D, ld, s, m)
                f = R.ln_fwd64(x, w, D)
                mean, rstd, y = R.ln_fwd32(x, w, D)
                d["ln_mean"] = max(d["ln_mean"], R.deviation((mean.double() - f["mean"]).abs(), f["u_mean"]))
                d["ln_rstd"] = max(d["ln_rstd"], R.deviation((rstd.double() - f["rstd"]).abs(), f["u_rstd"]))
                d["ln_y"] = max(d["ln_y"], R.deviation((y.double() - f["y"]).abs(), f["u_y"]))
                perm = R.ln_perm(rows)
                keep = torch.ones(rows, dtype=torch.bool) if perm is None else perm >= 0
                dy_eff = dy[:, :D].float() * keep[:, None]
                for with_in in (False, True):
                    dx_in = torch.randn(rows, D, generator=R.gen("dx_in", rows, D)) if with_in else None
                    b = R.ln_bwd64(dy_eff, x, w, D, dx_in)
                    dx, dw = R.ln_bwd32(dy_eff, x, w, D, dx_in)
                    d["ln_dx"] = max(d["ln_dx"], R.deviation((dx.double() - b["dx"]).abs(), b["u_dx"]))
                    d["ln_dw"] = max(d["ln_dw"], R.deviation((dw.double() - b["dw"]).abs(), b["u_dw"]))
        if ld <= 1536:                                       # the fused backward's own inputs (tests' three layers): dw per layer
            for rows in R.LN_ROWS:
                x, ws, dys = R.ln_multi_inputs(rows, D, ld, 3)
                for w, dy in zip(ws, dys):
                    b = R.ln_bwd64(dy[:, :D].float(), x, w, D)
                    _, dw = R.ln_bwd32(dy[:, :D].float(), x, w, D)
                    d["ln_dw"] = max(d["ln_dw"], R.deviation((dw.double() - b["dw"]).abs(), b["u_dw"]))
    return d


def _swiglu_cpu_dev():
    a, b, dh = R.swiglu_sweep_inputs()
    s64 = R.silu64(a)
    d = dict(swiglu_fwd=R.deviation((R.silu32(a).double() - s64).abs(), R.EPS32 * s64.abs().clamp_min(R.FLT_MIN), R.SILU_FLOOR),
             swiglu_da=0.0, swiglu_db=0.0)
    cases = [(a, b, dh)]
    for rows, F in ((3, 8), (5, 264), (4100, 2056)):
        ab = R.swiglu_shape_inputs(rows, F)
        g = torch.randn(rows, F, generator=R.gen("swiglu dh", rows, F)).to(BF16)
        cases.append((ab[:, :F].reshape(-1), ab[:, F:].reshape(-1), g.reshape(-1)))
    for a_, b_, g_ in cases:
        s = R.silu64(a_)
        d["swiglu_fwd"] = max(d["swiglu_fwd"], R.deviation((R.silu32(a_).double() - s).abs(), R.EPS32 * s.abs().clamp_min(R.FLT_MIN), R.SILU_FLOOR))
        m = R.swiglu_bwd64(a_, b_, g_)
        da, db = R.swiglu_bwd32(a_, b_, g_)
        d["swiglu_da"] = max(d["swiglu_da"], R.deviation((da.double() - m["da"]).abs(), m["u_da"], m["floor_da"]))
        d["swiglu_db"] = max(d["swiglu_db"], R.deviation((db.double() - m["db"]).abs(), m["u_db"], m["floor_db"]))
    return d


@pytest.mark.parametrize("family", ["ce", "ln", "swiglu"])
def test_cpu_fp32_fits_the_recorded_deviation(family):
    """the plain fp32 CPU evaluation on the GPU test's own inputs lies inside every envelope: its deviation is at most the recorded
    CPU_DEV (the envelope is FACTOR times that), and the record is not stale (at most 1.5 times what this run measures)"""
    d = dict(ce=_ce_cpu_dev, ln=_ln_cpu_dev, swiglu=_swiglu_cpu_dev)[family]()
    print("measured CPU deviation:", {k: round(v, 4) for k, v in d.items()})
    for k, v in d.items():
        assert 0.0 < v <= R.CPU_DEV[k], (k, v, R.CPU_DEV[k])
        assert R.CPU_DEV[k] <= 1.5 * v, (k, "stale record", v, R.CPU_DEV[k])
        assert R.envelope(k) == 4.0 * R.CPU_DEV[k]


def test_bf16_preimage_is_the_rounding_cell():
    """need_bf16 is 0 exactly for the values that round to the stored one, and grows with the distance beyond the cell"""
    t = R.all_finite_bf16()
    lo, hi = R.bf16_preimage(t)
    inside = 0.5 * (lo + hi)
    assert torch.equal(inside.to(BF16).float()[t.float() != 0], t.float()[t.float() != 0])
    assert bool((R.need_bf16(t, t.double()) == 0).all())
    nxt = R._bf16_step(t, 1)
    moved = nxt.float() != t.float()
    assert bool((R.need_bf16(t, nxt.double())[moved] > 0).all())
    assert bool((hi - lo > 0).all())


# ---------------------------------------------------------------------------------------------------------------- planted errors
def _seam_chunks(V):
    vc = V // 8
    return sorted({c for c in (0, 255, 256, 1023, 1024, (vc - 1) // 1024 * 1024 - 1, (vc - 1) // 1024 * 1024, vc - 1) if 0 <= c < vc})


@pytest.mark.parametrize("V", [2056, 64000])
def test_planted_ce_dropped_chunk_is_rejected(V):
    """a 16-byte chunk left out at a loop seam: the spike row whose spike sits in it no longer has lse = 0, and on the numeric rows lse
    leaves the envelope"""
    pos = R.ce_spike_positions(V)
    xn, tn = R.ce_numeric_logits(V, 2.0, 0.0)
    m = R.ce_model64(xn, tn, 1.0)
    for c in _seam_chunks(V):
        inside = [p for p in pos if p // 8 == c]
        assert inside, (V, c, "no spike in this chunk")
        j = torch.tensor(inside[:1])
        x = R.ce_spike_logits(j, V, V, 0, 0).float()
        lse, nll, g = R.ce_emul(x, j, 0.25, drop_chunk=c)
        assert float(lse[0]) != 0.0 and float(nll[0]) != 0.0
        lse, nll, g = R.ce_emul(xn.float(), tn, 1.0, drop_chunk=c)
        dev = R.deviation((lse.double() - m["lse"]).abs(), m["u_lse"])
        assert dev > R.envelope("ce_lse"), (V, c, dev)


def test_planted_ce_onehot_on_the_other_half_is_rejected():
    V = 2056
    j, t, n_all = _spike_sample(V)
    x = R.ce_spike_logits(j, V, V, 0, 0).float()
    exp_g, _, _ = R.ce_spike_expected(j, t, V, V, 0, 0, 0.25)
    _, _, g = R.ce_emul(x, t, 0.25, onehot_xor=1)
    differs = (R.ibits(g.to(BF16)) != R.ibits(exp_g)).any(1)
    assert bool(differs.all())                               # every row, whichever half of the pair the target is
    xn, tn = R.ce_numeric_logits(V, 2.0, 0.0)
    m = R.ce_model64(xn, tn, 1.0)
    _, _, g = R.ce_emul(xn.float(), tn, 1.0, onehot_xor=1)
    assert R.deviation(R.need_bf16(g.to(BF16), m["grad"]), m["u_grad"], m["floor_grad"]) > R.envelope("ce_grad")


def test_planted_loss_finalize_row_errors_are_rejected():
    nll, ranges, sums = R.lf_layout()
    seen = set()
    for (o, n), s in zip(ranges, sums):
        if n == 0:
            continue
        want = R.lf_mean(s, n)
        for hd, td in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            got = np.float32(R.lf_emul(nll, o, n, head_delta=hd, tail_delta=td))
            assert R.ulps32(got, want) > 1.0, (o, n, hd, td, got, want)
        seen.add((o % 4, n >= 1024))
    assert len(seen) == 8                                    # every residue with small and with large n


def test_planted_layernorm_mean_over_the_pitch_is_rejected():
    for D, ld in ((128, 1024), (126, 128), (770, 772)):
        x, w, _ = R.ln_inputs(5, D, ld, 2.0, 0.3)
        f = R.ln_fwd64(x, w, D)
        bad = R.ln_fwd64(x, w, D, mean_over=ld)
        assert R.deviation((bad["mean"] - f["mean"]).abs(), f["u_mean"]) > R.envelope("ln_mean")
        assert R.deviation(R.need_bf16(bad["y"].to(BF16), f["y"]), f["u_y"]) > R.envelope("ln_y")


def test_planted_colsum_lost_partial_row_is_rejected():
    x, dys, ws, dw0 = R.ln_exact_inputs(2080, 128, 1)
    parts = (dys[0].float() * x).reshape(65, 32, 128).sum(1)
    want = R.colsum_emul(parts)
    assert torch.equal(want.double(), (dys[0].double() * x.double()).sum(0))
    for lose in ((1, 0), (1, 1), (0, 64)):                   # a row of the second level (the 65th partial row alone is its row 1)
        assert not torch.equal(R.colsum_emul(parts, lose=lose), want), lose


def test_planted_swiglu_without_the_inner_rounding_is_rejected():
    a = R.all_finite_bf16()
    for bv in (-1.5, 1.0):
        b = torch.full_like(a, bv)
        need, unit = R.swiglu_need(R.swiglu_want(a, b), a, b)
        assert R.deviation(need, unit, R.SILU_FLOOR) == 0.0  # the fp64 double rounding itself costs nothing
        need, unit = R.swiglu_need(R.swiglu_want(a, b, inner=False), a, b)
        dev = R.deviation(need, unit, R.SILU_FLOOR)
        assert dev > R.envelope("swiglu_fwd") or bv == 1.0, (bv, dev)     # b = 1: bf16(bf16(s)) = bf16(s), nothing to see
