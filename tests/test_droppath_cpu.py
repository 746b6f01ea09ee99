"""Host side of stochastic depth (no GPU): the per-layer rates by the reference's rule, the site table, and the integer restatement
of the device draw (tests/_droppath_ref.py) that the GPU tests compare ego_droppath_draw with bit for bit."""
import math

import pytest
import torch

import _droppath_ref as R
from egom2p_amd.config import MODEL_CFGS, ModelCfg
from egom2p_amd.engine import drop_path_rates

SEED = 20260         # the frequency test's fixed seed (its kept count sits well inside the bound: see the test)


@pytest.mark.parametrize("Le,Ld", [(2, 2), (12, 12), (6, 6)])
@pytest.mark.parametrize("shared", [False, True])
def test_rates_follow_the_reference_linspaces(Le, Ld, shared):
    """egom2p_model.py:137-154: fp32 linspace `.item()` values, per stack or one ramp over both stacks cut at the encoder depth"""
    cfg = ModelCfg("t", 384, Le, Ld, 6, drop_path_rate_encoder=0.1, drop_path_rate_decoder=0.3, shared_drop_path=shared)
    enc, dec = drop_path_rates(cfg)
    if shared:
        want_e = [v.item() for v in torch.linspace(0, 0.1, Le + Ld)][:Le]
        want_d = [v.item() for v in torch.linspace(0, 0.3, Le + Ld)][Le:]
        assert dec[0] > 0                                         # the decoder's ramp does not restart at 0
    else:
        want_e = [v.item() for v in torch.linspace(0, 0.1, Le)]
        want_d = [v.item() for v in torch.linspace(0, 0.3, Ld)]
        assert dec[0] == 0.0
    assert enc == want_e and dec == want_d and (enc, dec) == R.rates(0.1, 0.3, Le, Ld, shared)
    assert enc[0] == 0.0 and len(enc) == Le and len(dec) == Ld
    assert all(isinstance(v, float) and R.f32(v) == v for v in enc + dec)          # fp32 values, not the double ramp


def test_fixture_config_rates_and_sites():
    enc, dec = drop_path_rates(MODEL_CFGS["ego_384_2e_2d_droppath"])
    assert enc == [0.0, R.f32(0.1)] and dec == [pytest.approx(0.2, abs=1e-7), pytest.approx(0.3, abs=1e-7)]
    sites = R.site_table(enc, dec)
    assert [n for n, _ in sites] == ["encoder.1.attn", "encoder.1.mlp", "decoder.0.self_attn", "decoder.0.cross_attn", "decoder.0.mlp",
                                     "decoder.1.self_attn", "decoder.1.cross_attn", "decoder.1.mlp"]
    assert len({kp for _, kp in sites}) == 3 and all(R.f32(kp) == kp and 0 < kp < 1 for _, kp in sites)
    assert drop_path_rates(MODEL_CFGS["ego_b_2e_2d"]) == ([0.0, 0.0], [0.0, 0.0])


def test_splitmix_is_the_generator_of_synth():
    """one generator in the project: the restatement equals egom2p_amd.synth's vectorised splitmix64"""
    from egom2p_amd import synth
    key = int(synth._key("w", 3))
    assert [int(v) for v in synth._hash_u64("w", 5, 3, start=7)] == [R.splitmix(key, 7 + i) for i in range(5)]


def test_draw_restatement_frequency_and_independence():
    """4096 samples x 8 sites at keep_prob 0.7: the kept count within 5 sigma of n p (binomial), every site within 5 sigma of its own
    mean too; sample b's decision does not depend on the batch size; the next counter and the next seed give other tables."""
    n_sites, B, p = 8, 4096, R.f32(0.7)
    tab = R.draw([p] * n_sites, B, SEED, 0)
    n = n_sites * B
    kept = sum(map(sum, tab))
    print(f"kept {kept} of {n}: {(kept - n * p) / math.sqrt(n * p * (1 - p)):+.2f} sigma")
    assert abs(kept - n * p) <= 5 * math.sqrt(n * p * (1 - p))
    for row in tab:
        assert abs(sum(row) - B * p) <= 5 * math.sqrt(B * p * (1 - p))
    assert R.draw([p] * n_sites, 3, SEED, 0) == [row[:3] for row in tab]
    assert R.draw([p] * n_sites, 64, SEED, 1) != [row[:64] for row in tab]
    assert R.draw([p] * n_sites, 64, SEED + 1, 0) != [row[:64] for row in tab]
    assert tab[0][:64] != tab[1][:64]                             # sites draw independently
    # the threshold is integer-exact: keep_prob 1 keeps everything, a keep_prob below 2^-24 nothing
    assert R.threshold(1.0) == 1 << 24 and all(map(all, R.draw([1.0], 256, SEED, 0))) and not any(R.draw([1e-9], 256, SEED, 0)[0])
    assert R.threshold(p) == int(math.floor(p * 2 ** 24)) == 11744051
