"""Host side of activation checkpointing (no GPU): the configuration field and the training script's flag."""
import dataclasses
import importlib.util
import os

import pytest

from egom2p_amd.config import MODEL_CFGS, ModelCfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_field_default_and_round_trip():
    cfg = ModelCfg("t", 384, 2, 2, 6)
    assert cfg.use_act_checkpoint is False
    assert all(c.use_act_checkpoint is False for c in MODEL_CFGS.values())          # no registered configuration turns it on
    on = dataclasses.replace(cfg, use_act_checkpoint=True)
    assert on.use_act_checkpoint is True and on != cfg
    assert ModelCfg(**dataclasses.asdict(on)) == on
    assert dataclasses.replace(on, use_act_checkpoint=False) == cfg
    # it describes no shape: everything the parameter layout is computed from is unchanged
    assert (on.head_dim, on.mlp_hidden, on.total_positions) == (cfg.head_dim, cfg.mlp_hidden, cfg.total_positions)


@pytest.fixture(scope="module")
def script():
    spec = importlib.util.spec_from_file_location("run_training_egom2p_amd_ck_cpu", os.path.join(ROOT, "run_training_egom2p.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_training_script_flag(script):
    assert script.get_args([]).act_checkpoint is False
    assert script.get_args(["--act_checkpoint"]).act_checkpoint is True


def test_training_script_yaml_key(script, tmp_path):
    path = tmp_path / "m.yaml"
    path.write_text("model: egom2p_tiny_6e_6d_swiglu_nobias\nact_checkpoint: true\nbatch_size: 2\n")
    args = script.get_args(["--config", str(path)])
    assert args.act_checkpoint is True and args.batch_size == 2 and args.model == "egom2p_tiny_6e_6d_swiglu_nobias"
    path.write_text("model: egom2p_tiny_6e_6d_swiglu_nobias\n")
    assert script.get_args(["--config", str(path)]).act_checkpoint is False


def test_get_model_hands_the_keyword_over(script, monkeypatch):
    seen = []
    monkeypatch.setattr(script, "create_model", lambda name, **kw: seen.append(kw) or kw)
    script.get_model(script.get_args(["--in_domains", "tok_cam-tok_gaze", "--out_domains", "tok_cam-tok_gaze"]))
    script.get_model(script.get_args(["--in_domains", "tok_cam-tok_gaze", "--out_domains", "tok_cam-tok_gaze", "--act_checkpoint"]))
    assert "use_act_checkpoint" not in seen[0] and seen[1]["use_act_checkpoint"] is True
