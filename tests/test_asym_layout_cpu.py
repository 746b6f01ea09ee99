"""Host-side checks of the asymmetric-model work: the flat parameter layout (a symmetric, shared-embedding model keeps the layout it
always had - tests/golden/layout_symmetric.json is a snapshot of the commit before the encoder / decoder modality sets existed,
written by tools/snapshot_layout.py), the parameter names of asymmetric / unshared models, and the masking host logic."""
import json
import os
from dataclasses import replace

import pytest

from egom2p_amd.config import MODEL_CFGS, ModelCfg
from egom2p_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAP = json.load(open(os.path.join(ROOT, "tests", "golden", "layout_symmetric.json")))

BASE = ModelCfg("asym", 384, 2, 2, 6, modalities=("tok_rgb", "tok_depth", "tok_cam"))
ASYM = replace(BASE, encoder_modalities=("tok_rgb", "tok_cam"), decoder_modalities=("tok_depth", "tok_cam"))
UNSHARED = replace(BASE, share_modality_embeddings=False)


def _engine(cfg):
    return Engine(cfg, device="cpu", max_batch=1, n_enc=8, n_dec=8)      # (parameters and workspaces only: no kernel runs)


@pytest.mark.parametrize("name", sorted(SNAP))
def test_symmetric_shared_layout_is_the_snapshot(name):
    """offsets, buckets, optimiser runs, layout tag and state-dict keys of a symmetric shared model, built through the spec code that
    now knows two modality sets - also when the two sets are spelled out - equal the snapshot: optimiser checkpoints stay loadable."""
    cfg = MODEL_CFGS[name]
    for c in (cfg, replace(cfg, encoder_modalities=cfg.modalities, decoder_modalities=cfg.modalities)):
        eng, s = _engine(c), SNAP[name]
        assert {k: [int(o), int(n), list(sh)] for k, (o, n, sh) in eng.offsets.items()} == s["offsets"]
        assert list(eng.offsets) == list(s["offsets"])
        assert [[n, int(a), int(b)] for n, a, b in eng.buckets] == s["buckets"]
        assert [[int(a), int(b), bool(nd)] for a, b, nd in eng.opt_runs] == s["opt_runs"]
        assert list(eng.layout_tag()) == s["layout_tag"]
        assert sorted(eng.never_grad) == s["never_grad"]
        assert list(eng.state_dict().keys()) == s["state_dict_keys"]
        assert not eng.dec_own_mod_emb


def _body_names(cfg):
    out = ["mask_token", "decoder_proj_context.weight", "decoder_proj_context.bias", "encoder_norm.weight", "decoder_norm.weight"]
    for i in range(cfg.encoder_depth):
        out += [f"encoder.{i}.{s}" for s in ("norm1.weight", "norm2.weight", "attn.qkv.weight", "attn.proj.weight",
                                             "mlp.fc1.weight", "mlp.fc2.weight", "mlp.fc3.weight")]
    for i in range(cfg.decoder_depth):
        out += [f"decoder.{i}.{s}" for s in ("norm1.weight", "norm2.weight", "query_norm.weight", "context_norm.weight",
                                             "self_attn.qkv.weight", "self_attn.proj.weight", "cross_attn.q.weight",
                                             "cross_attn.kv.weight", "cross_attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight",
                                             "mlp.fc3.weight")]
    return out


def test_asymmetric_parameter_names():
    """encoder {rgb, cam}, decoder {depth, cam}: encoder tables / mod_emb for the encoder modalities only, decoder tables for the decoder
    modalities only, a mod_emb of its own for the decoder-only depth, cam's decoder mod_emb the alias of the encoder's (no storage)."""
    eng = _engine(ASYM)
    want = set(_body_names(ASYM)) | {f"encoder_embeddings.{m}.{k}" for m in ("tok_rgb", "tok_cam") for k in ("token_emb.weight", "mod_emb")} | \
        {f"decoder_embeddings.{m}.token_emb.weight" for m in ("tok_depth", "tok_cam")} | {"decoder_embeddings.tok_depth.mod_emb"}
    assert set(eng.p) == want
    sd = eng.state_dict()
    assert sd["decoder_embeddings.tok_cam.mod_emb"].data_ptr() == sd["encoder_embeddings.tok_cam.mod_emb"].data_ptr()
    assert sd["decoder_embeddings.tok_depth.mod_emb"].data_ptr() == eng.p["decoder_embeddings.tok_depth.mod_emb"].data_ptr()
    assert not any(k.startswith(("encoder_embeddings.tok_depth", "decoder_embeddings.tok_rgb")) for k in sd)
    assert set(eng.pos) == {"tok_rgb", "tok_depth", "tok_cam"}            # a positional table per modality in either set
    # the new tensor: decayed (the mask token's run), in the "head" bucket, and the buckets still tile the flat buffer
    o = eng.offsets["decoder_embeddings.tok_depth.mod_emb"][0]
    assert any(a <= o < b and not nd for a, b, nd in eng.opt_runs)
    assert any(n == "head" and a <= o < b for n, a, b in eng.buckets)
    assert [b for _, _, b in eng.buckets[:-1]] == [a for _, a, _ in eng.buckets[1:]] and eng.buckets[-1][2] == eng.n_flat
    assert {n for n, _, _ in eng.buckets} >= {"enc_table.tok_rgb", "enc_table.tok_cam", "dec_table.tok_depth", "dec_table.tok_cam"}
    assert not {"enc_table.tok_depth", "dec_table.tok_rgb"} & {n for n, _, _ in eng.buckets}
    # keys of the side the model has no embedding on are reported, not aliased
    extra = eng.load_state_dict({"decoder_embeddings.tok_rgb.mod_emb": sd["encoder_embeddings.tok_rgb.mod_emb"],
                                 "encoder_embeddings.tok_depth.mod_emb": sd["decoder_embeddings.tok_depth.mod_emb"]})
    assert sorted(extra) == ["decoder_embeddings.tok_rgb.mod_emb", "encoder_embeddings.tok_depth.mod_emb"]


def test_unshared_parameter_names_and_untied_asymmetric_head():
    eng = _engine(UNSHARED)
    mods = ("tok_rgb", "tok_depth", "tok_cam")
    assert eng.dec_own_mod_emb == set(mods)
    assert {f"decoder_embeddings.{m}.mod_emb" for m in mods} <= set(eng.p)
    sd = eng.state_dict()
    for m in mods:
        assert sd[f"decoder_embeddings.{m}.mod_emb"].data_ptr() != sd[f"encoder_embeddings.{m}.mod_emb"].data_ptr()
    eng = _engine(replace(ASYM, share_embedding=False))
    assert eng.never_grad == {f"decoder_embeddings.{m}.token_emb.weight" for m in ("tok_depth", "tok_cam")}
    assert {f"decoder_embeddings.{m}.to_logits.weight" for m in ("tok_depth", "tok_cam")} <= set(eng.p)
    assert "decoder_embeddings.tok_rgb.to_logits.weight" not in eng.p


def test_modality_sets_must_come_from_the_models_modalities():
    with pytest.raises(ValueError):
        _engine(replace(BASE, encoder_modalities=("tok_gaze",)))
    with pytest.raises(ValueError):
        _engine(replace(BASE, decoder_modalities=()))
    assert all(c.encoder_modalities is None and c.decoder_modalities is None and c.share_modality_embeddings and c.decoder_sep_mask
               for c in MODEL_CFGS.values())                                  # the registered configurations are what they were


def test_masking_host_logic():
    """alpha 0 is floored at 1e-9 (the rule of egom2p/data/masking.py:159-165) and `sampling_mod_info` gives the union of the domains
    with alpha 0 outside the side's own, in_domains first (hand-stated expectations; the comparison with the reference's own
    setup_sampling_mod_info and UnifiedMasking is test_masking_info_and_zero_budgets_are_the_references below)."""
    from egom2p_amd.masking import ALPHA_EPS, UnifiedMasking, nosep_decoder_intervals, sampling_mod_info
    from egom2p_amd.model import MODALITY_INFO
    from egom2p_amd.synth import MOD4_MIXTURE_ALPHAS
    assert ALPHA_EPS == 1e-9
    info = sampling_mod_info(["tok_rgb", "tok_depth", "tok_cam"], ["tok_depth", "tok_cam"], MODALITY_INFO, [1.0], [0.5])
    assert set(info) == {"tok_rgb", "tok_depth", "tok_cam"}
    assert {m: (i["input_alphas"], i["target_alphas"]) for m, i in info.items()} == {
        "tok_rgb": ([1.0], [0.0]), "tok_depth": ([1.0], [0.5]), "tok_cam": ([1.0], [0.5])}
    assert info["tok_rgb"]["max_tokens"] == 5120 and "input_alphas" not in MODALITY_INFO["tok_rgb"]       # a copy
    info = sampling_mod_info(["tok_rgb"], ["tok_depth"], MODALITY_INFO)
    assert list(info) == ["tok_rgb", "tok_depth"]
    assert info["tok_rgb"]["target_alphas"] == [0.0] * 4 and info["tok_depth"]["input_alphas"] == [0.0] * 4
    um = UnifiedMasking(info, None, 64, 64, device="cpu")
    assert um.in_alphas == [[a, 1e-9] for a in MOD4_MIXTURE_ALPHAS] and um.tgt_alphas == [[1e-9, a] for a in MOD4_MIXTURE_ALPHAS]
    # in_domains == out_domains: the masking sees what it always saw
    same = sampling_mod_info(["tok_rgb", "tok_cam"], ["tok_rgb", "tok_cam"], MODALITY_INFO)
    um2, um3 = UnifiedMasking(same, None, 64, 64, device="cpu"), UnifiedMasking({m: MODALITY_INFO[m] for m in same}, None, 64, 64, device="cpu")
    assert (um2.names, um2.in_alphas, um2.tgt_alphas) == (um3.names, um3.in_alphas, um3.tgt_alphas)
    # the no-separation interval rule on the host: the cumsum staircase / the causal triangle, pads see the valid keys
    ks, ke = nosep_decoder_intervals([[5, 5, 7, 7, -1]], [[2, 0, 2, 0, 9]])
    assert ks.tolist() == [[0] * 5] and ke.tolist() == [[2, 2, 4, 4, 4]]
    assert nosep_decoder_intervals([[5, 5, 7, 7, -1]], [[2, 0, 2, 0, 9]], causal=True)[1].tolist() == [[1, 2, 3, 4, 4]]


@pytest.mark.parametrize("case", ["b2_asym", "b2_nosep", "b2_unshared"])
def test_parameter_names_are_the_reference_models(case):
    """the fixtures' meta holds the REAL reference model's named_parameters() and state_dict() names (tools/make_goldens_asym.py):
    the engine owns exactly those parameters (tied / shared names folded onto their storage) and writes exactly those keys"""
    import importlib.util
    from conftest import load_golden
    spec = importlib.util.spec_from_file_location("make_goldens_asym_names", os.path.join(ROOT, "tools", "make_goldens_asym.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    _, meta = load_golden(case)
    eng = _engine(tool.CFGS[case])
    assert {eng._canon_key(n) for n in meta["param_names"]} == set(eng.p)
    assert set(meta["state_keys"]) == set(eng.state_dict())
    own = {n for n in meta["param_names"] if n.startswith("decoder_embeddings") and n.endswith("mod_emb")}
    assert own == {f"decoder_embeddings.{m}.mod_emb" for m in eng.dec_own_mod_emb}


def test_masking_info_and_zero_budgets_are_the_references():
    """tests/golden/zero_alpha_budgets.npz (tools/make_goldens_zero_alpha.py) holds what the REAL reference made of in_domains
    tok_rgb-tok_cam / out_domains tok_depth-tok_cam: the modality_info of its setup_sampling_mod_info (pretrain_utils.py:30-83) and 4096
    budget draws of its UnifiedMasking (masking.py:181-234).  `sampling_mod_info` gives every name the same alphas (the reference sorts
    the names, ours keeps in_domains first: the order is not compared), and the reference's sampler - alpha floored at 1e-9 - gives the
    zero-alpha side of a modality a budget of 0 in every draw, which is what tests/test_asym_gpu.py asserts of the device sampler."""
    import ast
    import numpy as np
    from egom2p_amd.masking import UnifiedMasking, sampling_mod_info
    from egom2p_amd.model import MODALITY_INFO
    g = np.load(os.path.join(ROOT, "tests", "golden", "zero_alpha_budgets.npz"), allow_pickle=False)
    meta = ast.literal_eval(str(g["meta"]))
    names = [str(n) for n in g["names"]]
    assert names == sorted(names) and set(names) == {"tok_rgb", "tok_depth", "tok_cam"}
    ours = sampling_mod_info(meta["in_domains"].split("-"), meta["out_domains"].split("-"), MODALITY_INFO,
                             [float(meta["input_alphas"])], [float(meta["target_alphas"])])
    assert set(ours) == set(names)
    for j, n in enumerate(names):
        assert ours[n]["input_alphas"] == g["input_alphas"][j].tolist(), n
        assert ours[n]["target_alphas"] == g["target_alphas"][j].tolist(), n
        assert ours[n]["max_tokens"] == int(g["max_tokens"][j])
    # what our masking hands the kernel: the reference's clamp
    um = UnifiedMasking(ours, None, meta["n_in"], meta["n_tgt"], device="cpu")
    for j, n in enumerate(names):
        k = um.names.index(n)
        assert um.in_alphas[0][k] == max(float(g["input_alphas"][j, 0]), 1e-9) and um.tgt_alphas[0][k] == max(float(g["target_alphas"][j, 0]), 1e-9)
    # the reference's draws: zero budget on the zero-alpha side in every one of them, the rest takes the tokens
    k_in, k_tg = g["k_in"].astype(np.int64), g["k_tgt"].astype(np.int64)
    assert k_in.shape == (3, meta["draws"]) and meta["draws"] == 4096
    d, r, c = names.index("tok_depth"), names.index("tok_rgb"), names.index("tok_cam")
    assert (k_in[d] == 0).all() and (k_tg[r] == 0).all()
    assert k_in[r].max() > 200 and k_in[c].max() > 0 and k_tg[d].max() > 200 and k_tg[c].max() > 0
    assert (k_in[c] <= 30).all() and (k_in[c] + k_tg[c] <= 30).all() and (k_in.sum(0) <= meta["n_in"]).all() and (k_tg.sum(0) <= meta["n_tgt"]).all()
