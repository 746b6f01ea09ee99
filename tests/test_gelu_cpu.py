"""CPU-side checks of the GELU / biased family: the registry, the configuration defaults and the fixtures (no kernel is launched)."""
import dataclasses

import numpy as np
import pytest

from conftest import load_golden
from egom2p_amd.config import MODEL_CFGS, ModelCfg
from egom2p_amd.model import create_model, list_models

GELU_NAMES = ["egom2p_tiny_6e_6d_gelu", "egom2p_small_8e_8d_gelu", "egom2p_base_12e_12d_gelu", "egom2p_large_24e_24d_gelu",
              "egom2p_xlarge_24e_24d_gelu"]
QKNORM_NAMES = ["egom2p_base_12e_12d_swiglu_qknorm_nobias", "egom2p_large_24e_24d_swiglu_qknorm_nobias",
                "egom2p_xlarge_24e_24d_swiglu_qknorm_nobias"]


def test_registry_lists_the_gelu_names_and_keeps_the_qknorm_stubs():
    names = list_models()
    assert len(names) == 14
    for n in GELU_NAMES + QKNORM_NAMES:
        assert n in names
    for n in QKNORM_NAMES:                      # still stubs: they raise before they look at their arguments
        with pytest.raises(NotImplementedError, match="qk-norm"):
            create_model(n)
    # the base name keeps its stub (tests/test_model_api_gpu.py::test_registry_and_scope_errors pins that it raises); its message
    # names the call that builds the same model
    with pytest.raises(NotImplementedError, match="egom2p_tiny_6e_6d_gelu with dim=768"):
        create_model("egom2p_base_12e_12d_gelu")


def test_model_cfg_defaults_are_the_bias_free_swiglu_family():
    d = {f.name: f.default for f in dataclasses.fields(ModelCfg)}
    assert (d["mlp"], d["qkv_bias"], d["proj_bias"], d["mlp_bias"], d["norm_bias"]) == ("swiglu", False, False, False, False)
    base = MODEL_CFGS["egom2p_base_12e_12d_swiglu_nobias"]
    assert base.mlp == "swiglu" and base.mlp_hidden == 2048 and not (base.qkv_bias or base.proj_bias or base.mlp_bias or base.norm_bias)
    g = MODEL_CFGS["ego_384_2e_2d_gelu"]
    assert g.mlp == "gelu" and g.mlp_hidden == 4 * 384 and g.qkv_bias and g.proj_bias and g.mlp_bias and g.norm_bias
    assert dataclasses.replace(base, mlp="gelu").mlp_hidden == 3072


def test_fixtures_load_and_record_nonzero_bias_gradients():
    g, meta = load_golden("b2_gelu")
    assert meta["cfg"] == "ego_384_2e_2d_gelu" and (meta["batch"], meta["n_enc"], meta["n_dec"]) == (2, 256, 320)
    names = [str(n) for n in g["grad_names"]]
    sq = dict(zip(names, g["grad_sqnorm_all"]))
    biases = [n for n in names if n.endswith(".bias")]
    assert len(biases) == 37 and not any("fc3" in n for n in names)
    for n in ("encoder.0.attn.qkv.bias", "decoder.1.norm2.bias", "decoder.0.cross_attn.kv.bias", "decoder.1.mlp.fc1.bias", "decoder_norm.bias"):
        assert n in sq
    for n in biases:
        assert sq[n] > 0.0, n
    assert g["dec_pad"].any() and np.isfinite(float(g["loss"]))
    gg, gmeta = load_golden("gen_rgb2depth_gelu")
    assert gmeta["cfg"] == "ego_gen_384_2e_2d_gelu" and int(gg["n_steps"]) == 3 and gg["final_tokens"].shape == (1, 5120)
    assert float(gg["s0.cfg"][2]) == 2.0
