"""Host-side proofs behind tests/test_attention_exact_gpu.py: the integer recoveries hold for every size the GPU test uses,
ref64 / model64 agree with a naive dense fp64 implementation, and model64 sits inside its own envelope on every input."""
import math

import numpy as np
import pytest
import torch

import _attn_exact as X


def _f32(x):
    return np.float32(x)


def _bf16(x):
    """bf16 RNE of an fp32 numpy array, as fp64"""
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


EXACT = [c for c in X.cases() if c.exact]
PERTURB = (-2.0 ** -22, 0.0, 2.0 ** -22)


def test_case_list_covers_the_issue_shapes():
    geo = [c for c in X.cases() if c.group == "geometry"]
    assert 30 <= len(geo) <= 40
    assert {c.dims[2] for c in geo} >= {1, 31, 32, 33, 127, 128, 129, 257}
    assert {c.dims[3] for c in geo} >= {1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 321}
    for c in X.cases():
        B, H, Nq, Nk, d = c.dims
        assert B <= 3 and H <= 3 and Nq <= 700 and Nk <= 700
        assert (c.ks >= 0).all() and (c.ke >= 0).all()
        for t in (c.q, c.k, c.v, c.do):                           # the inputs are bf16 values
            assert torch.equal(X.bf16r(t), t)


def test_forward_recovery_for_every_size_used():
    """O = bf16(S * (1 / n)) with the reciprocal off by up to 2^-22 relative: round(O * n) == S, for every n an exact case has and
    every S up to the largest count any case has (<= S_FWD_MAX); and n == round(2^lse2) from a log2 that is 1 ulp off."""
    ns, smax = set(), 0
    for c in EXACT:
        t = X.exact_counts(c)
        ns |= set(t["n"].flatten().tolist())
        smax = max(smax, int(t["fwd"].max()))
    assert 1 <= min(ns) and max(ns) <= 4096 and smax <= X.S_FWD_MAX
    S = np.arange(smax + 1, dtype=np.float64)
    for n in sorted(ns):
        for e in PERTURB:
            inv = _f32(_f32(1.0) / _f32(n)) * _f32(1.0 + e)
            o = _bf16(_f32(S) * inv)
            assert np.array_equal(np.rint(o * n), S), (n, e)
        lg = _f32(math.log2(n))
        for cand in (np.nextafter(lg, _f32(-1)), lg, np.nextafter(lg, _f32(99))):
            assert round(2.0 ** float(cand)) == n, n


def test_backward_recovery_for_every_size_used():
    """dV = bf16(S * bf16(1 / n)) - exactly those two roundings (p = 1 / n also off by 2^-22 before its rounding): round(dV * n)
    == S for every n of a case whose rows all share n and every S such a case has; S * (2^-9 + 2^-8) < 0.25 as the sizes were
    chosen, and the general bound the GPU test uses on mixed-n masks (two bf16 roundings) cannot hide a missing query."""
    seen = 0
    for c in EXACT:
        t = X.exact_counts(c)
        smax = int(t["bwd"].max())
        assert smax <= X.S_BWD_MAX and smax * (2.0 ** -9 + 2.0 ** -8) < 0.25, (c.name, smax)
        # one query more or less changes dv by at least 1 / n_max, the bound allows 2 * U_BF16 * dv <= 2 * U_BF16 * smax / n_min
        if t["n_uniform"]:
            n = int(t["n"].flatten()[0])
            S = np.arange(smax + 1, dtype=np.float64)
            for e in PERTURB:
                p = _bf16(_f32(1.0 / n) * _f32(1.0 + e))
                dv = _bf16(_f32(S * p))
                assert np.array_equal(np.rint(dv * n), S), (c.name, n, e)
            seen += 1
    assert seen >= 8


def test_exact_inputs_are_exact_in_the_model():
    """on an exact case the rounding model has nothing to round but the outputs: O = bf16(S / n), dK = 0, lse = ln n"""
    for c in EXACT[::5]:
        ref, mod = X.reference(c.name)
        t = X.exact_counts(c)
        n = t["n"][:, None, :, None].double()
        assert torch.equal(torch.round(mod["o"][..., :64] * n), t["fwd"][:, None].expand_as(mod["o"][..., :64]))
        assert torch.equal(mod["dk"], torch.zeros_like(mod["dk"])) and torch.equal(ref["dk"], torch.zeros_like(ref["dk"]))
        assert torch.allclose(ref["lse"], torch.log(t["n"].double())[:, None].expand_as(ref["lse"]), rtol=0, atol=1e-12)
        assert torch.allclose(ref["dv"][..., :64], t["dv"][:, None].expand_as(ref["dv"][..., :64]), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("name", ["geo-33x193-ragged-iso", "geo-32x64-sample_edge", "rand-33x65-edges", "geo-128x129-beyond",
                                  "dyn-late_jump-33x257-full", "rand-129x63-sample"])
def test_ref64_agrees_with_a_naive_dense_implementation(name):
    c = X.get(name)
    ref, mod = X.reference(name)
    nv = X.naive(c.q, c.k, c.v, c.do, c.ks, c.ke, c.scale)
    for key in ("o", "lse", "delta", "dq", "dk", "dv"):
        assert torch.allclose(ref[key], nv[key], rtol=1e-10, atol=1e-10 * float(nv[key].abs().max() + 1)), key
    # model64 is the same operation up to its roundings: a few bf16 roundings of operands and outputs
    for key in ("o", "dq", "dk", "dv"):
        err = (mod[key] - nv[key]).norm() / nv[key].norm().clamp_min(1e-30)
        assert err < 2e-2, (key, float(err))


def test_pow2_scale_makes_the_prescale_exact():
    s = X.pow2_scale(0.125)
    assert np.float32(s) * X.LOG2E_F32 == np.float32(0.125)
    c = X.get("dyn-ascend-129x321-partial")
    assert torch.equal(X.bf16r(c.k * 0.125), c.k * 0.125) and torch.equal(X.bf16r(c.q * 0.125), c.q * 0.125)
    # the exp2-domain scores are the targets (bf16-rounded through K): they ascend by ~10 per key tile
    s2 = 0.125 * 64 * c.k[0, 0, :, X.SCORE_COL]
    assert 9 < float(s2[64] - s2[0]) < 11 and float(s2.max()) > 45


@pytest.mark.parametrize("name", X.case_names())
def test_model_sits_inside_its_envelope_and_no_row_is_empty(name):
    c = X.get(name)
    ref, mod = X.reference(name)
    for key in ("o", "dq", "dk", "dv"):
        assert torch.isfinite(ref[key]).all() and torch.isfinite(mod[key]).all()
        err, env = X.row_rms(mod[key] - ref[key]), X.envelope(mod[key], ref[key], 1.0)
        assert (err <= env).all(), key
        # an empty envelope only where the reference row is exactly zero (there the kernel must give exact zeros)
        assert ((env > 0) | (X.row_rms(ref[key]) == 0)).all(), key
        if not c.exact:
            # and on the float inputs that happens only by construction: zero dO rows (dQ), keys no query attends
            zero = X.row_rms(ref[key]) == 0
            if key == "o":
                assert not zero.any()
            if key == "dq":
                _, flat = X.intervals(c.ks, c.ke, c.dims[2], c.dims[3])
                by_design = (c.do.abs().sum(-1) == 0) | flat[:, None]
                assert not (zero & ~by_design).any()
    assert torch.isfinite(ref["lse"]).all() and torch.isfinite(mod["lse"]).all() and torch.isfinite(mod["delta"]).all()


@pytest.mark.parametrize("name", ["rand-129x193-ragged", "rand-33x65-edges", "dyn-halves-129x321-partial", "hd68p96r-129x193-random"])
def test_model_on_its_own_forward_outputs_is_the_model(name):
    """model64(fwd=...) only replaces the backward's operands: fed the model's own O, O_lo and lse2 it changes nothing"""
    c = X.get(name)
    _, mod = X.reference(name)
    again = X.model64(c.q, c.k, c.v, c.do, c.ks, c.ke, c.scale, c.o_lo, fwd=dict(o=mod["o"], olo=mod["olo"], lse2=mod["lse"] / X.LN2))
    for key in ("dq", "dk", "dv"):
        assert (X.row_rms(again[key] - mod[key]) <= 2.0 ** -9 * X.row_rms(mod[key])).all(), key
    assert torch.allclose(again["delta"], mod["delta"], rtol=0, atol=1e-12)
