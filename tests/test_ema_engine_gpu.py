"""The model EMA through the engine (egom2p_amd/ema.py; ModelEmaV2, egom2p/utils/timm/model_ema.py:84-149): the recursion
against a host restatement, `applied()` (an in-place exchange of the flat buffer: views and captured graphs stay valid), the
step gate, padded storage, checkpoints of the training script and `--use-ema` of the generation scripts.

Smallest shapes: ego_tiny_2e_2d (dim 128, 2 + 2 layers, tok_cam + tok_gaze: 30 + 30 positions, so N = M = 64 keeps 30 rows per
side), batch 2, a few steps per test.  decay = 0.5 makes the host recursion exact in fp32 (both products exact, one rounding),
so averages are compared bit for bit."""
import importlib.util
import os
import random
import types
from functools import partial

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

from egom2p_amd import synth  # noqa: E402
from egom2p_amd.config import MODEL_CFGS  # noqa: E402
from egom2p_amd.ema import ModelEma  # noqa: E402
from egom2p_amd.engine import Engine  # noqa: E402
from egom2p_amd.generate import (GenerationSampler, build_chained_generation_schedules, init_empty_target_modality,  # noqa: E402
                                 init_full_input_modality)
from egom2p_amd.model import MODALITY_INFO, EgoM2P, LayerNorm  # noqa: E402
from egom2p_amd.optim import NativeScalerWithGradNormCount, create_optimizer  # noqa: E402
from egom2p_amd.trainer import TrainStep  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CFG = MODEL_CFGS["ego_tiny_2e_2d"]
BUD = {"tok_cam": (15, 15), "tok_gaze": (15, 15)}
N = M = 64
ARGS = types.SimpleNamespace(opt="adamw", lr=1e-2, weight_decay=0.05, opt_betas=(0.9, 0.95), opt_eps=1e-8)


def _script():
    spec = importlib.util.spec_from_file_location("run_training_egom2p_ema", os.path.join(ROOT, "run_training_egom2p.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    return R


def _model(seed=1, **kw):
    mods = ["tok_cam", "tok_gaze"]
    enc = {m: MODALITY_INFO[m]["encoder_embedding"]() for m in mods}
    dec = {m: MODALITY_INFO[m]["decoder_embedding"]() for m in mods}
    args = dict(dim=128, encoder_depth=2, decoder_depth=2, num_heads=2, mlp_ratio=4, qkv_bias=False, proj_bias=False,
                mlp_bias=False, norm_layer=partial(LayerNorm, eps=1e-6, bias=False), act_layer=nn.SiLU, gated_mlp=True)
    args.update(kw)
    model = EgoM2P(enc, dec, {m: MODALITY_INFO[m] for m in mods}, **args)
    if seed is not None:
        model.load_state_dict(synth.build_state_dict(CFG, seed))
    return model


_BATCHES = {}


def _batch(step):
    if step not in _BATCHES:
        md = synth.make_clip_batch(CFG, 2, BUD, seed=40 + step)
        _BATCHES[step] = {k: {kk: vv.to(DEV) for kk, vv in v.items()} for k, v in md.items()}
    return _BATCHES[step]


def _train(model, opt, scaler, step, ema=None, **kw):
    """one step of run_training_egom2p.train_one_epoch: forward, scaler (backward + optimiser), the average"""
    model.train()
    random.seed(1000 + step)                                 # the decoder-modality shuffle of this step
    loss, _ = model(_batch(step), N, M)
    scaler(loss, opt, parameters=model.parameters(), update_grad=True, **(kw or dict(clip_grad=1.0)))
    if ema is not None:
        ema.update()
    return loss.detach().clone()


def _eval_loss(model, step=99):
    model.eval()
    random.seed(7)
    with torch.no_grad():
        loss, _ = model(_batch(step), N, M)
    model.train()
    return loss.detach().clone()


def _host(sd):
    from egom2p_amd.ema import host_copy
    return host_copy(sd)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert tuple(a[k].shape) == tuple(b[k].shape) and torch.equal(a[k].cpu(), b[k].cpu()), k


def test_recursion_is_the_host_formula_bit_for_bit():
    eng = Engine(CFG, DEV, max_batch=2, n_enc=30, n_dec=30)
    eng.init_random(3)
    ema = ModelEma(eng, decay=0.5)
    step = TrainStep(eng, lr=1e-2, weight_decay=0.05, clip_grad=1.0, ema=ema)
    want = _host(eng.state_dict())                              # the average starts as a copy of the weights
    _same(ema.state_dict()["state_dict_ema"], want)
    for s in range(4):
        step([_batch(s)])
        p = _host(eng.state_dict())
        assert any(not torch.equal(p[k], want[k]) for k in p)   # the weights moved away from the average
        want = {k: 0.5 * want[k] + 0.5 * p[k] for k in want}    # fp32 on the host: exact products, one rounding
        got = ema.state_dict()
        _same(got["state_dict_ema"], want)
        assert all(not v.is_cuda for v in got["state_dict_ema"].values())
        assert got["num_updates"] == s + 1 and got["decay"] == 0.5 and got["warmup"] is False
    assert set(want) == set(eng.state_dict())


def test_applied_exchanges_in_place_and_leaves_training_untouched():
    a, b = _model(), _model()
    oa, ob = create_optimizer(ARGS, a), create_optimizer(ARGS, b)
    sa, sb = NativeScalerWithGradNormCount(), NativeScalerWithGradNormCount()
    ema = ModelEma(a, decay=0.5)
    for s in range(2):
        la, lb = _train(a, oa, sa, s, ema), _train(b, ob, sb, s)
        assert torch.equal(la, lb)                              # the twin never sees an average
    eng = a.engine
    before, avg, ptr = eng.P.clone(), ema.ema.clone(), eng.P.data_ptr()
    assert not torch.equal(before, avg)
    with ema.applied():
        assert eng.params_swapped and eng.P.data_ptr() == ptr
        assert torch.equal(eng.P, avg) and torch.equal(ema.ema, before)
        inside = _eval_loss(a)
        with pytest.raises(RuntimeError):
            oa.step(clip_grad=1.0)                              # a step here would train the average
        with pytest.raises(RuntimeError):
            with ema.applied():
                pass
        with pytest.raises(RuntimeError):
            ema.update()
        assert eng.params_swapped                               # the refused nesting did not undo the exchange
    assert not eng.params_swapped and eng.weights_dirty
    assert torch.equal(eng.P, before) and torch.equal(ema.ema, avg)
    fresh = _model(seed=None)
    fresh.load_state_dict(ema.state_dict()["state_dict_ema"])
    assert torch.equal(_eval_loss(fresh), inside)
    assert not torch.equal(_eval_loss(a), inside)               # outside again: the trained weights
    la, lb = _train(a, oa, sa, 2, ema), _train(b, ob, sb, 2)
    assert torch.equal(la, lb) and torch.equal(a.engine.P, b.engine.P)


def test_average_moves_when_the_step_gate_passes_every_step_by():
    model = _model()
    opt, scaler = create_optimizer(ARGS, model), NativeScalerWithGradNormCount()
    ema = ModelEma(model, decay=0.5)
    eng = model.engine
    p0 = eng.P.clone()
    ema.ema.copy_(p0 * 1.5)                                     # a perturbed start (the storage pads stay 0)
    e0 = ema.ema.clone()
    for s in range(2):
        _train(model, opt, scaler, s, ema, skip_grad=1e-9)      # below any norm: every call is gated
        assert torch.equal(eng.P, p0)
        e0 = (0.5 * e0.double() + 0.5 * p0.double()).float()    # exact sum, one rounding
        assert torch.equal(ema.ema, e0)
    assert opt.gated_total() == 2 and ema.num_updates == 2
    assert not torch.equal(ema.ema, p0)


def test_padded_storage_keeps_its_pads_at_zero():
    model = _model(seed=None, dim=1020, num_heads=15, encoder_depth=1, decoder_depth=1)
    eng = model.engine
    assert eng.padded
    opt, scaler = create_optimizer(ARGS, model), NativeScalerWithGradNormCount()
    ema = ModelEma(model, decay=0.5)
    start = ema.ema.clone()
    for s in range(3):
        _train(model, opt, scaler, s, ema)
    assert not torch.equal(ema.ema, start)
    for buf in (ema.ema, eng.P):
        rest = buf.clone()
        for n, (o, cnt, shape) in eng.offsets.items():
            eng._logical(n, rest[o:o + cnt].view(shape)).zero_()
        assert not bool(rest.any())
    sd, own = ema.state_dict()["state_dict_ema"], model.state_dict()
    assert set(sd) == set(own) and all(tuple(sd[k].shape) == tuple(own[k].shape) for k in sd)


def _run(steps, R, tmp_path=None, save_after=None):
    """`steps` training steps with a warmed-up average; save_after: through a checkpoint file after that many steps"""
    model = _model()
    opt, scaler = create_optimizer(ARGS, model), NativeScalerWithGradNormCount()
    ema = ModelEma(model, decay=0.9, warmup=True)
    for s in range(steps):
        if save_after is not None and s == save_after:
            path = str(tmp_path / "checkpoint-0.pth")
            torch.save(R.checkpoint_dict(model, opt, 0, ARGS, ema), path)
            ck = torch.load(path, map_location="cpu", weights_only=True)
            assert set(ck["state_dict_ema"]) == set(ck["model"]) and set(ck["ema"]) == {"decay", "warmup", "num_updates"}
            model = _model(seed=5)                              # a fresh model, optimiser and average (other weights, other settings)
            opt, scaler = create_optimizer(ARGS, model), NativeScalerWithGradNormCount()
            ema = ModelEma(model, decay=0.5)
            assert R.load_checkpoint(ck, model, opt, ema) == 1
        _train(model, opt, scaler, s, ema)
    return model, ema


def test_resume_continues_the_average_bit_for_bit(tmp_path, capsys):
    R = _script()
    m4, e4 = _run(4, R)
    m22, e22 = _run(4, R, tmp_path, save_after=2)
    assert "Loaded state_dict_ema" in capsys.readouterr().out
    assert e22.num_updates == e4.num_updates == 4 and e22.decay == 0.9 and e22.warmup is True
    assert torch.equal(m22.engine.P, m4.engine.P) and torch.equal(e22.ema, e4.ema)
    _same(e22.state_dict()["state_dict_ema"], e4.state_dict()["state_dict_ema"])
    assert not torch.equal(e4.ema, m4.engine.P)


def test_checkpoint_without_the_key_starts_from_the_loaded_weights(capsys):
    R = _script()
    src = _model()
    ck = {"model": _host(src.state_dict()), "epoch": 3}
    model = _model(seed=5)
    ema = ModelEma(model, decay=0.5)
    assert not torch.equal(ema.ema, src.engine.P)
    assert R.load_checkpoint(ck, model, None, ema) == 4
    assert "Failed to find state_dict_ema, starting from loaded model weights" in capsys.readouterr().out
    assert torch.equal(model.engine.P, src.engine.P) and torch.equal(ema.ema, src.engine.P) and ema.num_updates == 0


GEN = dict(encoder_depth=2, decoder_depth=2)      # the registered tiny variant (dim 384: the video modalities need dim % 6 == 0) at 2 + 2 layers


def test_generation_scripts_use_ema(tmp_path):
    """`eval_model_rgb2cam.py --use-ema` (egom2p_amd/eval_generation.py) reads `state_dict_ema`: its tokens are those of a run
    whose checkpoint holds the averaged weights as `model` (the checkpoint's own `model` differs in every trained tensor; the
    refusal of a checkpoint without the key is in tests/test_ema_cpu.py)."""
    from egom2p_amd import eval_generation as E
    from egom2p_amd.model import create_model
    name = "egom2p_tiny_6e_6d_swiglu_nobias"
    mods = ["tok_rgb", "tok_depth", "tok_cam", "tok_gaze"]
    torch.manual_seed(11)
    model = create_model(name, encoder_embeddings={m: MODALITY_INFO[m]["encoder_embedding"]() for m in mods},
                         decoder_embeddings={m: MODALITY_INFO[m]["decoder_embedding"]() for m in mods}, modality_info=MODALITY_INFO, **GEN)
    ema = ModelEma(model, decay=0.5)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(12)
    with torch.no_grad():                                       # stands in for training: the weights leave the average behind
        for key in model.engine.p:                              # (the tensors' own elements: storage pads stay 0)
            v = model.engine._view_for_key(key)
            v.add_(torch.randn(v.shape, device=DEV, generator=gen) * 0.05)
    model.engine.weights_dirty = True
    ema.update()
    avg, own = ema.state_dict()["state_dict_ema"], _host(model.state_dict())
    assert not torch.equal(avg["encoder.0.attn.qkv.weight"], own["encoder.0.attn.qkv.weight"])
    both, plain = str(tmp_path / "both.pth"), str(tmp_path / "avg_as_model.pth")
    torch.save({"model": own, "state_dict_ema": avg}, both)
    torch.save({"model": avg}, plain)
    del model, ema
    common = ["--model", name, "--batch", "1"]

    def tokens(extra):
        try:
            out = E.main("rgb2cam", common + extra, **GEN)
        finally:
            torch.set_grad_enabled(True)                        # (the script switches autograd off for its process)
        return out["tok_cam"]["tensor"].clone()

    try:
        assert torch.equal(tokens(["--ckpt", both, "--use-ema"]), tokens(["--ckpt", plain]))
    finally:
        os.remove(both), os.remove(plain)


def test_captured_graphs_survive_the_exchange():
    cfg = MODEL_CFGS["ego_gen_384_2e_2d"]
    eng = Engine(cfg, DEV, max_batch=1, n_enc=64, n_dec=64)
    eng.init_random(3)
    ema = ModelEma(eng, decay=0.5)
    eng.load_state_dict(synth.build_state_dict(cfg, 5))         # other weights: the average sits between the two
    ema.update()
    sample = {"tok_rgb": {"tensor": synth.randint("ema.rgb", (1, 5, 32, 32), 64000, seed=2).to(DEV)}}
    sample = init_empty_target_modality(sample, MODALITY_INFO, "tok_depth", 1, 5120, DEV)
    sample = init_full_input_modality(sample, MODALITY_INFO, "tok_rgb", DEV)
    sch = build_chained_generation_schedules(["tok_rgb"], ["tok_depth"], [5120], ["roar"], [3], ["linear"], [0.01], ["constant"],
                                             [2.0], ["constant"], cfg_grow_conditioning=True)
    sampler = GenerationSampler(eng)

    def tokens():
        return sampler.generate_graphed(sample, sch, top_p=0.8, seed=7)["tok_depth"]["tensor"].clone()

    first = tokens()                                            # captures
    n_graphs = len(eng._graphs)
    with ema.applied():
        averaged = tokens()                                     # the same graph over the exchanged weights
    assert not torch.equal(averaged, first)
    assert torch.equal(tokens(), first) and len(eng._graphs) == n_graphs
    other = Engine(cfg, DEV, max_batch=1, n_enc=64, n_dec=64)
    other.load_state_dict(ema.state_dict()["state_dict_ema"])
    got = GenerationSampler(other, use_graphs=False).generate(sample, sch, top_p=0.8, seed=7)["tok_depth"]["tensor"]
    assert torch.equal(got, averaged)
