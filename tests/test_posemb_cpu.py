"""Host-side checks of the learned positional tables (`sincos_pos_emb=False`): the C-ABI symbols, the configuration defaults, the entry
script's switch, and the flat layout - a learned table is a parameter BEHIND everything a model with fixed tables holds."""
import os
import re
from dataclasses import replace

import torch

from egom2p_amd import _lib as L
from egom2p_amd.config import MODEL_CFGS, ModelCfg
from egom2p_amd.engine import Engine
from egom2p_amd.optim import is_no_decay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = MODEL_CFGS["ego_tiny_2e_2d"]
LEARNED = replace(TINY, learned_pos_emb_encoder=("tok_cam",), learned_pos_emb_decoder=("tok_cam", "tok_gaze"))


def _engine(cfg):
    return Engine(cfg, device="cpu", max_batch=1, n_enc=8, n_dec=8)      # (parameters and workspaces only: no kernel runs)


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "egom2p_hip.h")).read()
    for name in ("ego_posemb_grad", "ego_posemb_grad_work_ints"):
        assert name in L.EXPORTS and re.search(r"^\s*(?:int|long)\s+%s\s*\(" % name, hdr, flags=re.M)
    assert len(L.EXPORTS) == 78 and L.ABI_VERSION == 12
    lib = L.load()
    assert lib.ego_posemb_grad_work_ints(4, 2, (L.i32 * L.MAX_MODS)(30, 5120)) == 4 * 5150
    from egom2p_amd import ops
    assert callable(ops.posemb_grad) and callable(ops.posemb_grad_work_ints)


def test_model_cfg_defaults_mean_none():
    c = ModelCfg("x", 128, 1, 1, 2)
    assert c.learned_pos_emb_encoder == () and c.learned_pos_emb_decoder == ()
    assert all(v.learned_pos_emb_encoder == () and v.learned_pos_emb_decoder == () for v in MODEL_CFGS.values())


def test_entry_script_switch_parses():
    import importlib.util
    spec = importlib.util.spec_from_file_location("run_training_posemb", os.path.join(ROOT, "run_training_egom2p.py"))
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    assert rt.get_args([]).learned_pos_emb == "none"
    for v in ("none", "encoder", "decoder", "both"):
        assert rt.get_args(["--learned_pos_emb", v]).learned_pos_emb == v
    try:
        rt.get_args(["--learned_pos_emb", "all"])
        raise AssertionError("an unknown choice was accepted")
    except SystemExit:
        pass


def test_learned_tables_lie_behind_the_fixed_layout():
    base, eng = _engine(TINY), _engine(LEARNED)
    keys = ["encoder_embeddings.tok_cam.pos_emb", "decoder_embeddings.tok_cam.pos_emb", "decoder_embeddings.tok_gaze.pos_emb"]
    assert list(eng.offsets)[:len(base.offsets)] == list(base.offsets) and list(eng.offsets)[len(base.offsets):] == keys
    assert all(eng.offsets[k] == v for k, v in base.offsets.items())
    assert eng.n_flat_body == base.n_flat and eng.n_flat == base.n_flat + 3 * 30 * 128 and base.n_flat_body == base.n_flat
    assert eng.buckets[:-1] == base.buckets and eng.buckets[-1] == ("pos_emb", base.n_flat, eng.n_flat)
    assert eng.layout_tag() != base.layout_tag()
    assert eng.num_params() == base.num_params() + 3 * 30 * 128
    for k in keys:
        o, n, shape = eng.offsets[k]
        assert shape == (30, 128) and not is_no_decay(k)
        assert any(a <= o and o + n <= b and not nd for a, b, nd in eng.opt_runs)           # in a decayed run
        assert not eng._is_buffer_key(k)
        p, g = eng.param_views(k)
        assert tuple(p.shape) == tuple(g.shape) == (1, 30, 128) and p.data_ptr() == eng.P[o:].data_ptr() and g.data_ptr() == eng.G[o:].data_ptr()
    assert eng._is_buffer_key("encoder_embeddings.tok_gaze.pos_emb") and base._is_buffer_key("encoder_embeddings.tok_cam.pos_emb")
    # the side's lookup: the parameter where there is one, the fixed table elsewhere
    assert eng.pos_enc["tok_cam"].data_ptr() == eng.p[keys[0]].data_ptr() and eng.pos_enc["tok_gaze"] is eng.pos["tok_gaze"]
    assert eng.pos_dec["tok_cam"].data_ptr() == eng.p[keys[1]].data_ptr() and eng.pos_dec["tok_gaze"].data_ptr() == eng.p[keys[2]].data_ptr()
    assert list(eng.state_dict().keys()) == list(base.state_dict().keys())


def test_state_dict_carries_a_learned_table_as_a_parameter():
    base, eng = _engine(TINY), _engine(LEARNED)
    base.init_random(3)
    eng.init_random(3)
    body = base.n_flat
    assert torch.equal(eng.P[:body], base.P[:body])                      # the tables draw behind everything else
    k = "decoder_embeddings.tok_gaze.pos_emb"
    t = eng.state_dict()[k]
    assert tuple(t.shape) == (1, 30, 128) and abs(float(t.std()) - 0.02) < 4e-3
    assert not torch.equal(t, eng.state_dict()["decoder_embeddings.tok_cam.pos_emb"])
    # a sin-cos state loads into the learned model (the fixed table is the starting value), a learned one into a learned model,
    # and a learned one into the sin-cos model, which keeps its fixed tables
    assert eng.load_state_dict(base.state_dict()) == []
    assert torch.equal(eng.state_dict()[k], base.state_dict()[k]) and torch.equal(eng.p[k], base.pos["tok_gaze"])
    other = _engine(LEARNED)
    eng.p[k].add_(1.0)
    assert other.load_state_dict(eng.state_dict()) == [] and torch.equal(other.P, eng.P)
    fixed = base.state_dict()[k].clone()
    assert base.load_state_dict(eng.state_dict()) == [] and torch.equal(base.state_dict()[k], fixed)


def test_padded_storage_keeps_the_reference_shape():
    cfg = replace(MODEL_CFGS["ego_L_1020_2e_2d"], modalities=("tok_cam", "tok_gaze"), learned_pos_emb_encoder=("tok_gaze",))
    eng = _engine(cfg)
    k = "encoder_embeddings.tok_gaze.pos_emb"
    assert eng.offsets[k][2] == (30, 1024)
    p, g = eng.param_views(k)
    assert tuple(p.shape) == (1, 30, 1020) and p.stride() == (30 * 1024, 1024, 1)
    eng.init_random(0)
    assert float(eng.p[k][:, 1020:].abs().max()) == 0.0 and tuple(eng.state_dict()[k].shape) == (1, 30, 1020)
