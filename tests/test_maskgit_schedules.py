"""`build_chained_generation_schedules` for the MaskGIT token schedules (cosine / linear) and the `linear` /
`onex:{min_t}:{power}` temperature schedules against the reference's own output (tests/golden/maskgit_schedules.npz, made by
tools/make_goldens_maskgit.py from egom2p/models/generate.py:197-320 and egom2p/utils/generation.py)."""
import ast
import os

import numpy as np
import pytest

from egom2p_amd.generate import build_chained_generation_schedules

PATH = os.path.join(os.path.dirname(__file__), "golden", "maskgit_schedules.npz")
CASES = ["cos_5120x8", "cos_30x3", "lin_5120x8", "lin_30x7", "cos_5120x8_tlinear", "cos_5120x8_onex", "cos_30x3_onex",
         "lin_5120x8_onex", "roar_5120x3_onex", "chain_roar_maskgit"]


def _gold():
    assert os.path.exists(PATH), "tests/golden/maskgit_schedules.npz is missing (tools/make_goldens_maskgit.py)"
    return np.load(PATH, allow_pickle=False)


def test_fixture_holds_every_case():
    g = _gold()
    assert sorted(k[:-5] for k in g.files if k.endswith(".args")) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_schedule_equals_the_reference(name):
    g = _gold()
    kw = ast.literal_eval(str(g[name + ".args"]))
    sch = build_chained_generation_schedules(**kw)
    tokens = np.array([s["num_tokens"] for s in sch], dtype=np.int64)
    temps = np.array([s["temperature"] for s in sch], dtype=np.float64)
    assert tokens.shape == g[name + ".tokens"].shape and np.array_equal(tokens, g[name + ".tokens"])        # integers: exact
    assert np.abs(temps - g[name + ".temps"]).max() <= 1e-12
    # the rest of a step's record: scheme, guidance, growing conditioning (:303-318)
    n = len(kw["target_domains"])
    steps_of = [sum(1 for s in sch if s["target_domain"] == t) for t in kw["target_domains"]]
    assert sum(steps_of) == len(sch)
    i = 0
    for k in range(n):
        for s in sch[i:i + steps_of[k]]:
            assert s["scheme"] == kw["autoregression_schemes"][k] and s["cfg_scale"] == kw["cfg_scales"][k]
            assert s["cfg_cond_domains"] == kw["cond_domains"] + kw["target_domains"][:k]
            assert isinstance(s["num_tokens"], int) and isinstance(s["temperature"], float)
        i += steps_of[k]
    assert tokens.sum() == sum(kw["tokens_per_target"])


def _build(**over):
    kw = dict(cond_domains=["tok_rgb"], target_domains=["tok_depth"], tokens_per_target=[5120], autoregression_schemes=["maskgit"],
              decoding_steps=[4], token_decoding_schedules=["cosine"], temps=[1.0], temp_schedules=["constant"], cfg_scales=[2.0],
              cfg_schedules=["constant"])
    kw.update(over)
    return build_chained_generation_schedules(**kw)


def test_illegal_names_raise_value_error_with_the_reference_messages():
    with pytest.raises(ValueError, match="Illegal MaskGIT token schedule sqrt"):
        _build(token_decoding_schedules=["sqrt"])
    with pytest.raises(ValueError, match="Illegal temperature schedule exp"):
        _build(temp_schedules=["exp"])
    with pytest.raises(ValueError, match="Illegal guidance schedule ramp"):
        _build(cfg_schedules=["ramp"])
    with pytest.raises(ValueError, match="Illegal decoding scheme beam"):
        _build(autoregression_schemes=["beam"])
    # what the reference itself does not implement stays a NotImplementedError (:298)
    with pytest.raises(NotImplementedError):
        _build(cfg_schedules=["cosine"])
    assert len(_build()) == 4
