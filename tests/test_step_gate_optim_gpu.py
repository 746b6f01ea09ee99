"""The step gate through `FusedAdamW.step(skip_grad=..., skip_nonfinite=...)` and `run_training_egom2p.py --skip_grad`:
per-tensor step counts stay torch's (a gated call counts for nobody) through freeze -> skip -> unfreeze, without a host
sync per step (the device counts the gated calls, the host folds them in where it syncs anyway)."""
import importlib.util
import os
import random
import re
import types
from functools import partial

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

from conftest import load_golden, rel_l2  # noqa: E402
from egom2p_amd import synth  # noqa: E402
from egom2p_amd.config import MODEL_CFGS  # noqa: E402
from egom2p_amd.model import MODALITY_INFO, EgoM2P, LayerNorm  # noqa: E402
from egom2p_amd.optim import create_optimizer  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny_model():
    mods = ["tok_cam", "tok_gaze"]
    enc = {m: MODALITY_INFO[m]["encoder_embedding"]() for m in mods}
    dec = {m: MODALITY_INFO[m]["decoder_embedding"]() for m in mods}
    return EgoM2P(enc, dec, {m: MODALITY_INFO[m] for m in mods}, dim=128, encoder_depth=2, decoder_depth=2, num_heads=2,
                  mlp_ratio=4, qkv_bias=False, proj_bias=False, mlp_bias=False,
                  norm_layer=partial(LayerNorm, eps=1e-6, bias=False), act_layer=nn.SiLU, gated_mlp=True)


def test_freeze_skip_unfreeze_keeps_torch_step_counts():
    """Seven calls against ONE torch.optim.AdamW that sees requires_grad flip (as in
    test_unfrozen_tensors_start_their_adamw_step_count_at_one): shared blocks frozen for calls 0-2, calls 1 and 4 skipped by a
    threshold below any norm.  The torch side restates native_scaler.py:36-39: no optimizer.step() when norm >= skip_grad."""
    g, meta = load_golden("tiny")
    cfg = MODEL_CFGS[meta["cfg"]]
    sd = synth.build_state_dict(cfg, meta["seed"])
    md = synth.make_clip_batch(cfg, meta["batch"], meta["budgets"], meta["seed"])
    mdg = {k: {kk: vv.cuda() for kk, vv in v.items()} for k, v in md.items()}
    model = _tiny_model()
    model.load_state_dict(sd)
    args = types.SimpleNamespace(opt="adamw", lr=1e-2, weight_decay=0.05, opt_betas=(0.9, 0.95), opt_eps=1e-8)
    opt = create_optimizer(args, model)
    named = dict(model.named_parameters())
    ref = {n: p.detach().clone().requires_grad_(True) for n, p in named.items()}
    nd = lambda n: ("norm." in n or ".norm" in n or n.endswith(".bias"))
    topt = torch.optim.AdamW([{"params": [ref[n] for n in named if not nd(n)], "weight_decay": 0.05},
                              {"params": [ref[n] for n in named if nd(n)], "weight_decay": 0.0}], lr=1e-2, betas=(0.9, 0.95), eps=1e-8)
    start = {n: p.detach().clone() for n, p in named.items()}
    shared = None

    def backward(step):
        random.seed(meta["py_seed"] + step)
        loss, _ = model(mdg, meta["n_enc"], meta["n_dec"])
        loss.backward()

    for step in range(7):
        if step == 0:
            model.freeze_shared_params()
        elif step == 3:
            model.unfreeze_all()
        live = [n for n, p in named.items() if p.requires_grad]
        if step == 0:
            shared = [n for n in named if n not in live]
            assert shared and live
        thr = 1e-9 if step in (1, 4) else 1e9
        backward(step)
        for n in named:
            ref[n].grad = named[n].grad.detach().clone() if n in live else None
        tnorm = torch.norm(torch.stack([torch.norm(ref[n].grad.detach(), 2.0) for n in live]), 2.0)      # get_grad_norm_
        before = {n: named[n].detach().clone() for n in named}
        if not tnorm >= thr:
            topt.step()
        norm = opt.step(clip_grad=None, skip_grad=thr)
        assert isinstance(norm, torch.Tensor) and norm.is_cuda
        assert abs(norm.item() - tnorm.item()) < 1e-5 * tnorm.item(), (step, norm.item(), tnorm.item())
        for n in named:
            assert rel_l2(named[n].detach().float().cpu().numpy(), ref[n].detach().float().cpu().numpy()) < 2e-6, (step, n)
            if step in (1, 4):
                assert torch.equal(named[n].detach(), before[n]), (step, n)
        if step < 3:
            for n in shared:
                assert torch.equal(named[n].detach(), start[n]), (step, n)
        assert float(model.engine.G.abs().max().item()) == 0.0
    st = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in opt.state_dict().items()}       # folds
    key = model.engine._canon_key
    late = next(x for x in shared if x.endswith("attn.qkv.weight"))
    early = next(x for x in named if x not in shared and named[x].numel() > 4)
    assert topt.state[ref[late]]["step"].item() == 3 == opt.t - opt.skipped[key(late)]
    assert topt.state[ref[early]]["step"].item() == 5 == opt.t - opt.skipped.get(key(early), 0)
    assert st["t"] == 5 and st["gated_total"] == 2 and opt.gated_total() == 2
    # round trip: a second optimiser restored from the state takes the same next step, bit for bit
    opt2 = create_optimizer(args, model)
    opt2.load_state_dict(st)
    assert opt2.t == opt.t and opt2.skipped == opt.skipped and opt2.gated_total() == 2
    eng = model.engine
    backward(7)
    P0, G0 = eng.P.clone(), eng.G.clone()
    opt.step(skip_grad=1e9)
    Pa, ma, va = eng.P.clone(), opt.m.clone(), opt.v.clone()
    eng.P.copy_(P0); eng.G.copy_(G0)
    opt2.step(skip_grad=1e9)
    assert not torch.equal(Pa, P0)
    assert torch.equal(eng.P, Pa) and torch.equal(opt2.m, ma) and torch.equal(opt2.v, va)


def test_training_script_skip_grad(tmp_path, capsys):
    """`run_training_egom2p.py --skip_grad` (reference :104, :737) on synthetic clips, tiny model: a threshold below any norm
    leaves the weights at their start values and the log line counts the gated steps; a threshold above any norm trains as the
    run without the flag does (the gated pass forms its bias corrections on the device: held to the 1e-6 of the kernel test)."""
    spec = importlib.util.spec_from_file_location("run_training_egom2p_gate", os.path.join(ROOT, "run_training_egom2p.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    common = ["--model", "egom2p_tiny_6e_6d_swiglu_nobias", "--in_domains", "tok_cam-tok_gaze", "--out_domains", "tok_cam-tok_gaze",
              "--num_input_tokens", "32", "--num_target_tokens", "32", "--batch_size", "4", "--epochs", "1", "--epoch_size", "12",
              "--blr", "1e-3", "--print_freq", "1", "--seed", "3", "--max_steps", "3"]
    snaps = []
    real = R.train_one_epoch

    def spy(model, loader, optimizer, scaler, args, epoch, *rest):
        first = {k: v.detach().clone() for k, v in model.module.state_dict().items()}
        r = real(model, loader, optimizer, scaler, args, epoch, *rest)
        snaps.append((first, {k: v.detach().clone() for k, v in model.module.state_dict().items()}, optimizer.gated_total()))
        return r

    env_keys = {k: os.environ.pop(k) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK") if k in os.environ}
    R.train_one_epoch = spy
    outs = []
    try:
        for extra in (["--skip_grad", "1e-9"], ["--skip_grad", "1e9"], []):
            R.main(R.get_args(common + extra))
            outs.append(capsys.readouterr().out)
    finally:
        R.train_one_epoch = real
        os.environ.update(env_keys)
    (a0, a1, na), (b0, b1, nb), (c0, c1, nc) = snaps
    for k in a0:
        assert torch.equal(a0[k], a1[k]), k                              # every step gated: nothing moved
    assert na == 3 and nb == 0 and nc == 0
    counts = [int(x) for x in re.findall(r"gated_steps (\d+)", outs[0])]
    assert counts == [1, 2, 3], outs[0]
    assert [int(x) for x in re.findall(r"gated_steps (\d+)", outs[1])] == [0, 0, 0] and "gated_steps" not in outs[2]
    moved, worst = 0, 0.0
    for k in b0:
        assert torch.equal(b0[k], c0[k]), k
        moved += int(not torch.equal(c0[k], c1[k]))
        worst = max(worst, float((b1[k].float() - c1[k].float()).abs().max()))
        assert rel_l2(b1[k].float().cpu().numpy(), c1[k].float().cpu().numpy()) < 1e-6, k
    print(f"largest element difference --skip_grad 1e9 vs no flag after 3 steps: {worst:.3e}")
    assert moved > 0
