"""Layer-wise lr decay through `create_optimizer(args, model, get_num_layer, get_layer_scale)` -> `FusedAdamW` on its segmented path
(one ops.adamw_step_seg launch per step), on `ego_tiny_2e_2d` and the synthetic clip of tests/golden/tiny.npz: beside it runs ONE
torch.optim.AdamW built from the reference's own groups (tests/golden/param_groups.json) over clones of the parameters, fed the
engine's own gradients.  Bars: the parameters agree to rel_l2 < 2e-6 per tensor (tests/test_step_gate_optim_gpu.py, the same setup
on the two-group path) and the updates to tests/test_engine_gpu.py's AdamW bars (element distance <= 2.2 lr, rel_l2 < 0.6)."""
import importlib.util
import json
import os
import random
import re
import types
from functools import partial

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

from conftest import GOLDEN_DIR, load_golden, rel_l2  # noqa: E402
from egom2p_amd import synth  # noqa: E402
from egom2p_amd.config import MODEL_CFGS  # noqa: E402
from egom2p_amd.model import MODALITY_INFO, EgoM2P, LayerNorm  # noqa: E402
from egom2p_amd.optim import (FusedAdamW, LayerDecayValueAssigner, create_optimizer, get_num_layer_for_fm,  # noqa: E402
                              layer_decay_values)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(GOLDEN_DIR, "param_groups.json")))["swiglu_nobias"]["variants"]
LR = 1e-2


def _tiny_model():
    mods = ["tok_cam", "tok_gaze"]
    enc = {m: MODALITY_INFO[m]["encoder_embedding"]() for m in mods}
    dec = {m: MODALITY_INFO[m]["decoder_embedding"]() for m in mods}
    return EgoM2P(enc, dec, {m: MODALITY_INFO[m] for m in mods}, dim=128, encoder_depth=2, decoder_depth=2, num_heads=2,
                  mlp_ratio=4, qkv_bias=False, proj_bias=False, mlp_bias=False,
                  norm_layer=partial(LayerNorm, eps=1e-6, bias=False), act_layer=nn.SiLU, gated_mlp=True)


def _args(variant="ld"):
    a = GOLD[variant]["args"]
    return types.SimpleNamespace(opt="adamw", lr=LR, weight_decay=0.05, opt_betas=(0.9, 0.95), opt_eps=1e-8,
                                 decoder_decay=a["decoder_decay"], no_lr_scale_list=a["no_lr_scale_list"])


def _layer_optimizer(model, variant="ld"):
    return create_optimizer(_args(variant), model, get_num_layer=partial(get_num_layer_for_fm, num_enc_layers=2, num_dec_layers=2),
                            get_layer_scale=LayerDecayValueAssigner(layer_decay_values(GOLD[variant]["args"]["layer_decay"], 4)).get_scale)


class Setup:
    def __init__(self, variant="ld"):
        g, meta = load_golden("tiny")
        cfg = MODEL_CFGS[meta["cfg"]]
        self.meta = meta
        md = synth.make_clip_batch(cfg, meta["batch"], meta["budgets"], meta["seed"])
        self.mdg = {k: {kk: vv.cuda() for kk, vv in v.items()} for k, v in md.items()}
        self.model = _tiny_model()
        self.model.load_state_dict(synth.build_state_dict(cfg, meta["seed"]))
        self.opt = _layer_optimizer(self.model, variant)
        assert self.opt.segmented
        for grp in self.opt.param_groups:                            # the training loop's part (run_training_egom2p.py:707-713)
            grp["lr"] = LR * grp["lr_scale"]
        self.named = dict(self.model.named_parameters())
        self.ref = {n: p.detach().clone().requires_grad_(True) for n, p in self.named.items()}
        fix = GOLD[variant]["params"]
        assert set(fix) == set(self.named)
        groups = {}
        for n, (gname, scale, wd) in fix.items():                    # the FIXTURE's groups: what the reference would hand torch
            groups.setdefault(gname, {"params": [], "weight_decay": wd, "lr": LR * scale})["params"].append(self.ref[n])
        self.scale = {n: v[1] for n, v in fix.items()}
        self.topt = torch.optim.AdamW(list(groups.values()), lr=LR, betas=(0.9, 0.95), eps=1e-8)

    def backward(self, step):
        random.seed(self.meta["py_seed"] + step)
        loss, _ = self.model(self.mdg, self.meta["n_enc"], self.meta["n_dec"])
        loss.backward()

    def feed(self):
        live = [n for n, p in self.named.items() if p.requires_grad]
        for n in self.named:
            self.ref[n].grad = self.named[n].grad.detach().clone() if n in live else None
        self.ref_before = {n: r.detach().clone() for n, r in self.ref.items()}
        return live

    def compare(self, tag, before):
        """`before`: the engine's parameters in front of the step (each side's update is measured from its own start)"""
        for n, p in self.named.items():
            got, want, p0, r0 = (x.detach().float().cpu().numpy() for x in (p, self.ref[n], before[n], self.ref_before[n]))
            assert rel_l2(got, want) < 2e-6, (tag, n, rel_l2(got, want))
            ug, uw = got - p0, want - r0
            assert abs(ug - uw).max() <= 2.2 * LR * self.scale[n], (tag, n)
            if abs(uw).max() > 0:
                assert rel_l2(ug, uw) < 0.6, (tag, n)


@pytest.mark.parametrize("variant", ["ld", "ld_dd"])
def test_layer_decay_with_clipping_against_torch(variant):
    s = Setup(variant)
    assert len(s.opt.param_groups) == (11 if variant == "ld" else 13)
    first = {}
    for step in range(3):
        s.backward(step)
        live = s.feed()
        before = {n: p.detach().clone() for n, p in s.named.items()}
        tnorm = torch.nn.utils.clip_grad_norm_([s.ref[n] for n in live], 1.0)
        s.topt.step()
        norm = s.opt.step(clip_grad=1.0)
        assert abs(norm.item() - tnorm.item()) < 1e-5 * tnorm.item()
        s.compare(step, before)
        assert float(s.model.engine.G.abs().max().item()) == 0.0
        if step == 0:
            first = {n: (s.named[n].detach() - before[n]).abs().median().item() for n in ("encoder.0.norm1.weight", "decoder.1.norm1.weight")}
    assert len(s.opt._launches) == 1                                 # eleven (thirteen) groups, one launch per step
    # Adam's first step moves an element by lr_eff * sign(g) (no weight decay on a norm weight): encoder block 0 is layer 1 of 5
    # (scale 0.75 ** 4), decoder block 1 layer 4 (0.75) - the two tensors provably took different effective learning rates
    lo, hi = first["encoder.0.norm1.weight"], first["decoder.1.norm1.weight"]
    assert abs(lo / (LR * 0.75 ** 4) - 1.0) < 0.02 and abs(hi / (LR * 0.75) - 1.0) < 0.02, (lo, hi)
    if variant == "ld_dd":                                           # a no_lr_scale_list name keeps scale 1 in its layer
        g = next(g for g in s.opt.param_groups if g["name"] == "layer_1_decay_no_lr_scale")
        assert g["lr_scale"] == 1.0 and g["param_names"] == ["encoder.0.attn.qkv.weight"]
        assert {g["weight_decay"] for g in s.opt.param_groups if "decoder_decay" in g["name"]} == {0.01}


def test_frozen_phase_restarts_step_counts_on_the_segmented_path():
    s = Setup()
    key = s.model.engine._canon_key
    shared = None
    for step in range(3):
        if step == 0:
            s.model.freeze_shared_params()
        elif step == 1:
            s.model.unfreeze_all()
        s.backward(step)
        live = s.feed()
        if step == 0:
            shared = [n for n in s.named if n not in live]
            assert shared and live
        before = {n: p.detach().clone() for n, p in s.named.items()}
        tnorm = torch.nn.utils.clip_grad_norm_([s.ref[n] for n in live], 1.0)
        s.topt.step()
        norm = s.opt.step(clip_grad=1.0)
        assert abs(norm.item() - tnorm.item()) < 1e-5 * tnorm.item()  # (the frozen tensors' gradients are left out of the norm)
        s.compare(step, before)
        assert float(s.model.engine.G.abs().max().item()) == 0.0     # frozen ranges cleared in the same launch
        if step == 0:
            assert any(f for *_, f in s.opt.segments())
            for n in shared:
                assert torch.equal(s.named[n].detach(), before[n]), n
    late = next(x for x in shared if x.endswith("attn.qkv.weight"))
    early = next(x for x in s.named if x not in shared and s.named[x].numel() > 4)
    assert s.topt.state[s.ref[late]]["step"].item() == 2 == s.opt.t - s.opt.skipped[key(late)]
    assert s.topt.state[s.ref[early]]["step"].item() == 3 == s.opt.t - s.opt.skipped.get(key(early), 0)
    assert any(sk == 1 for _, _, _, sk, fro in s.opt.segments() if not fro) and len(s.opt._launches) == 1


def test_skip_grad_gates_one_call():
    s = Setup()
    for step in range(3):
        thr = 1e-9 if step == 1 else 1e9
        s.backward(step)
        live = s.feed()
        before = {n: p.detach().clone() for n, p in s.named.items()}
        tnorm = torch.norm(torch.stack([torch.norm(s.ref[n].grad.detach(), 2.0) for n in live]), 2.0)
        if not tnorm >= thr:
            s.topt.step()
        norm = s.opt.step(clip_grad=None, skip_grad=thr)
        assert abs(norm.item() - tnorm.item()) < 1e-5 * tnorm.item()
        s.compare(step, before)
        if step == 1:
            for n in s.named:
                assert torch.equal(s.named[n].detach(), before[n]), n
        assert float(s.model.engine.G.abs().max().item()) == 0.0
    st = s.opt.state_dict()
    assert st["t"] == 2 and st["gated_total"] == 1
    assert all(int(s.topt.state[s.ref[n]]["step"].item()) == 2 for n in s.named)


def test_state_dict_round_trip_and_group_name_check():
    s = Setup()
    for step in range(2):
        s.backward(step)
        s.opt.step(clip_grad=1.0)
    st = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in s.opt.state_dict().items()}
    assert [g["name"] for g in st["param_groups"]] == [g["name"] for g in s.opt.param_groups]
    assert all("params" not in g and "param_names" not in g for g in st["param_groups"])
    opt2 = _layer_optimizer(s.model)
    opt2.load_state_dict(st)
    eng = s.model.engine
    s.backward(2)
    P0, G0 = eng.P.clone(), eng.G.clone()
    s.opt.step(clip_grad=1.0)
    Pa, ma, va = eng.P.clone(), s.opt.m.clone(), s.opt.v.clone()
    eng.P.copy_(P0); eng.G.copy_(G0)
    opt2.step(clip_grad=1.0)
    assert not torch.equal(Pa, P0)
    assert torch.equal(eng.P, Pa) and torch.equal(opt2.m, ma) and torch.equal(opt2.v, va)
    # a state saved under other groups does not load: the two-group optimiser, and a layer-decay one with decoder_decay groups
    for other in (create_optimizer(_args(), s.model), _layer_optimizer(s.model, "ld_dd")):
        with pytest.raises(RuntimeError, match="parameter groups"):
            other.load_state_dict(st)
    with pytest.raises(RuntimeError, match="parameter groups"):
        opt2.load_state_dict(create_optimizer(_args(), s.model).state_dict())


def test_default_grouping_is_bitwise_the_old_optimiser():
    s = Setup()
    eng = s.model.engine
    old = FusedAdamW(eng, lr=LR, weight_decay=0.05, betas=(0.9, 0.95), eps=1e-8, named_parameters=s.model.named_parameters())
    new = create_optimizer(_args(), s.model, get_num_layer=None, get_layer_scale=None, filter_bias_and_bn=True, skip_list=None)
    assert not new.segmented and [g["name"] for g in new.param_groups] == ["decay", "no_decay"]
    for step in range(2):
        s.backward(step)
        P0, G0 = eng.P.clone(), eng.G.clone()
        old.step(clip_grad=1.0)
        Pa = eng.P.clone()
        eng.P.copy_(P0); eng.G.copy_(G0)
        new.step(clip_grad=1.0)
        assert not torch.equal(Pa, P0)
        assert torch.equal(eng.P, Pa) and torch.equal(new.m, old.m) and torch.equal(new.v, old.v), step


def test_training_script_layer_decay_and_finetune(tmp_path, capsys):
    """`run_training_egom2p.py --layer_decay 0.75 --finetune <checkpoint of a 1-step run>`: the weights are taken over (minus
    `.pos_emb`), the missing / unexpected keys are printed, the groups train at lr * lr_scale, and the run finishes."""
    spec = importlib.util.spec_from_file_location("run_training_egom2p_ld", os.path.join(ROOT, "run_training_egom2p.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    common = ["--model", "egom2p_tiny_6e_6d_swiglu_nobias", "--in_domains", "tok_cam-tok_gaze", "--out_domains", "tok_cam-tok_gaze",
              "--num_input_tokens", "32", "--num_target_tokens", "32", "--batch_size", "4", "--epochs", "1", "--epoch_size", "12",
              "--blr", "1e-3", "--print_freq", "1", "--seed", "3"]
    env_keys = {k: os.environ.pop(k) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK") if k in os.environ}
    seen = {}
    real = R.train_one_epoch

    def spy(model, loader, optimizer, *rest):
        seen["start"] = {k: v.detach().clone() for k, v in model.module.state_dict().items()}
        seen["opt"] = optimizer
        return real(model, loader, optimizer, *rest)

    try:
        R.main(R.get_args(common + ["--max_steps", "1", "--output_dir", str(tmp_path)]))
        capsys.readouterr()
        ck = os.path.join(str(tmp_path), "checkpoint-0.pth")
        assert os.path.exists(ck)
        R.train_one_epoch = spy
        R.main(R.get_args(common + ["--max_steps", "2", "--seed", "4", "--layer_decay", "0.75", "--finetune", ck]))
    finally:
        R.train_one_epoch = real
        os.environ.update(env_keys)
    out = capsys.readouterr().out
    line = next(ln for ln in out.splitlines() if ln.startswith("finetune "))
    assert "missing keys [" in line and "unexpected keys []" in line and ".pos_emb" in line       # the dropped tables, nothing else
    saved = torch.load(ck, map_location="cpu", weights_only=True)["model"]
    for k, v in seen["start"].items():
        if ".pos_emb" not in k:
            assert torch.equal(v.cpu(), saved[k]), k                 # training started from the checkpoint's weights
    opt = seen["opt"]
    assert opt.segmented and opt.t == 2 and len(opt.param_groups) == 2 * 14 - 1      # 14 layer ids x 2 classes; layer 0 (the encoder embeddings) holds no norm
    lr = 1e-3 * 4 / 256
    logged = [ln for ln in out.splitlines() if " group_lrs " in ln]
    assert len(logged) == 2
    lrs = dict(re.findall(r"(layer_\d+_\w+)=([0-9.e+-]+)", logged[0].split(" group_lrs ")[1]))
    assert len(lrs) == len(opt.param_groups)
    for name, val in lrs.items():                                    # constant schedule: lr * 0.75 ** (13 - layer)
        layer = int(name.split("_")[1])
        assert abs(float(val) / (lr * 0.75 ** (13 - layer)) - 1.0) < 2e-3, (name, val)
    assert '"epoch": 0' in out
