"""Learned positional tables (`sincos_pos_emb=False`) through the model, the engine, the optimiser, checkpoints and generation.

The gradient of a learned table is held to what the existing engine parity tests hold `mod_emb` to - relative L2 against the oracle's
`bf16_bwd` autograd, hard tolerance max(1e-2, 2.5 x the tensor's own bf16 sensitivity) (tests/test_engine_bf16_oracle_gpu.py) - with the
`mod_emb` gradients of the same run measured alongside (a sum over the same rows); the measured values are recorded in
tests/golden/parity_bars_posemb.json and held to recorded + 30 % (the tests/_asym_bars.py pattern)."""
import json
import os
import random
from dataclasses import replace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN_DIR, bar, rel_l2  # noqa: E402
from egom2p_amd import synth  # noqa: E402
from egom2p_amd.config import MODEL_CFGS  # noqa: E402
from egom2p_amd.engine import Engine  # noqa: E402
from egom2p_amd.generate import (GenerationSampler, build_chained_generation_schedules, init_empty_target_modality,  # noqa: E402
                                 init_full_input_modality)
from egom2p_amd.model import (MODALITY_INFO, GazeCamTokenDecoderEmbedding, GazeCamTokenEncoderEmbedding,  # noqa: E402
                              VideoTokenDecoderEmbedding, VideoTokenEncoderEmbedding, create_model)
from egom2p_amd.optim import FusedAdamW  # noqa: E402
from oracle import egom2p_oracle as O  # noqa: E402

DEV = "cuda:0"
GRAD_TOL, SENS_FACTOR, LOSS_TOL = 1e-2, 2.5, 3e-4          # tests/test_engine_bf16_oracle_gpu.py
_PATH = os.path.join(GOLDEN_DIR, "parity_bars_posemb.json")
_BASE = json.load(open(_PATH)) if os.path.exists(_PATH) else {}


def held(name, value, hard, rel_margin=0.30):
    value = bar(name, value, hard=hard, rel_margin=rel_margin)
    if not os.environ.get("EGOM2P_RECORD_BARS"):
        assert name in _BASE, (name, "has no recorded baseline in parity_bars_posemb.json")
        assert value <= _BASE[name] * (1.0 + rel_margin), (name, value, "recorded baseline", _BASE[name])
    return value


def _learned(cfg, enc=None, dec=None):
    return replace(cfg, learned_pos_emb_encoder=tuple(cfg.modalities if enc is None else enc),
                   learned_pos_emb_decoder=tuple(cfg.modalities if dec is None else dec))


def _pos_keys(cfg):
    return ([f"encoder_embeddings.{m}.pos_emb" for m in cfg.learned_pos_emb_encoder] +
            [f"decoder_embeddings.{m}.pos_emb" for m in cfg.learned_pos_emb_decoder])


def _state(cfg, seed):
    """the synthetic state with random (not sin-cos) tables, one per side and modality"""
    sd = synth.build_state_dict(cfg, seed)
    for k in _pos_keys(cfg):
        sd[k] = synth.normal(k, tuple(sd[k].shape), 0.02, seed)
    return sd


def _cuda(md):
    return {k: {kk: vv.cuda() for kk, vv in v.items()} for k, v in md.items()}


def _oracle_grads(cfg, sd, md, N, M, order, keys):
    """gradients of `keys` + every mod_emb under the oracle's three modes -> (bf16 loss, {name: bf16_bwd grad}, {name: sensitivity})"""
    torch.set_num_threads(16)
    out = {}
    for mode in ("bf16", "fp32", "bf16_bwd"):
        leaf = O.make_leaf_state(sd)
        for k in keys:
            leaf[k] = sd[k].clone().requires_grad_(True)
        loss, _ = O.forward(leaf, cfg, md, N, M, dec_order=order, mode=mode)
        loss.backward()
        names = list(keys) + [k for k in leaf if k.startswith("encoder_embeddings") and k.endswith("mod_emb")]
        out[mode] = (float(loss.detach()), {k: leaf[k].grad.numpy() for k in names})
    sens = {k: float(np.hypot(rel_l2(out["bf16"][1][k], out["fp32"][1][k]), rel_l2(out["bf16_bwd"][1][k], out["bf16"][1][k])))
            for k in out["bf16"][1]}
    return out["bf16"][0], out["bf16_bwd"][1], sens


def _parity(case, cfg, B, N, M, budgets, order):
    sd = _state(cfg, seed=11)
    md = synth.make_clip_batch(cfg, B, budgets, seed=11)
    keys = _pos_keys(cfg)
    eng = Engine(cfg, DEV, max_batch=B, n_enc=N, n_dec=M)
    assert eng.load_state_dict(sd) == []
    loss, _ = eng.forward(_cuda(md), dec_order=order)
    eng.zero_grad()
    eng.backward(1.0)
    torch.cuda.synchronize()
    assert int(eng.cd["err"].item()) == 0
    ref_loss, ref, sens = _oracle_grads(cfg, sd, md, N, M, order, keys)
    assert abs(loss.item() - ref_loss) < LOSS_TOL * abs(ref_loss), (loss.item(), ref_loss)
    errs = {"pos_emb": (0.0, 0.0), "mod_emb": (0.0, 0.0)}
    for k, r in ref.items():
        got = eng.grad_of(k).float().cpu().numpy().reshape(r.shape)
        e, tol = rel_l2(got, r), max(GRAD_TOL, SENS_FACTOR * sens[k])
        print(f"{case} {k}: rel_l2 {e:.3e} (tolerance {tol:.3e}, sensitivity {sens[k]:.3e})")
        kind = "pos_emb" if k.endswith("pos_emb") else "mod_emb"
        if e / tol >= errs[kind][0] / max(errs[kind][1], 1e-30):
            errs[kind] = (e, tol)
        if kind == "pos_emb":
            # positions no kept row holds: exactly zero, in the engine and in the oracle
            zero = np.abs(r).reshape(-1, r.shape[-1]).max(axis=1) == 0.0
            assert float(np.abs(got.reshape(-1, r.shape[-1])[zero]).max(initial=0.0)) == 0.0, k
    for kind, (e, tol) in errs.items():
        held(f"posemb.{case}.{kind}_grad", e, hard=tol)
    return eng, ref


def test_parity_with_the_oracle_sequence_modalities():
    cfg = _learned(MODEL_CFGS["ego_tiny_2e_2d"])
    _parity("tiny", cfg, 4, 24, 24, {"tok_cam": (12, 12), "tok_gaze": (12, 12)}, ["tok_gaze", "tok_cam"])


def test_parity_with_the_oracle_video_modality():
    """one learned video table per side (5120 positions): most positions receive no row - gradient exactly 0"""
    cfg = _learned(MODEL_CFGS["ego_gen_384_2e_2d"], enc=("tok_rgb",), dec=("tok_depth",))
    _, ref = _parity("video", cfg, 2, 256, 256, {"tok_rgb": (192, 64), "tok_depth": (64, 192)}, ["tok_depth", "tok_rgb"])
    for k, r in ref.items():
        if k.endswith("pos_emb"):
            rows = int((np.abs(r[0]).max(axis=1) > 0).sum())
            assert 0 < rows <= 2 * 192 and r.shape == (1, 5120, 384)


def _model(enc_learned=(), dec_learned=(), mods=("tok_cam", "tok_gaze"), **kw):
    enc = {m: MODALITY_INFO[m]["encoder_embedding"](sincos_pos_emb=m not in enc_learned) for m in mods}
    dec = {m: MODALITY_INFO[m]["decoder_embedding"](sincos_pos_emb=m not in dec_learned) for m in mods}
    args = dict(dim=128, num_heads=2, encoder_depth=2, decoder_depth=2)
    args.update(kw)
    return create_model("egom2p_tiny_6e_6d_swiglu_nobias", encoder_embeddings=enc, decoder_embeddings=dec,
                        modality_info={m: MODALITY_INFO[m] for m in mods}, **args)


def test_construction():
    for cls in (VideoTokenEncoderEmbedding, VideoTokenDecoderEmbedding, GazeCamTokenEncoderEmbedding, GazeCamTokenDecoderEmbedding):
        assert cls(vocab_size=256, sincos_pos_emb=False).sincos_pos_emb is False and cls(vocab_size=256).sincos_pos_emb is True
    base = _model()
    m = _model(enc_learned=("tok_cam",), dec_learned=("tok_gaze",))
    params, buffers = dict(m.named_parameters()), dict(m.named_buffers())
    for k in ("encoder_embeddings.tok_cam.pos_emb", "decoder_embeddings.tok_gaze.pos_emb"):
        assert tuple(params[k].shape) == (1, 30, 128) and params[k].requires_grad and tuple(params[k].grad.shape) == (1, 30, 128)
        assert abs(float(params[k].detach().std()) - 0.02) < 4e-3            # the register tokens' tolerance (test_model_api_gpu)
    for k in ("encoder_embeddings.tok_gaze.pos_emb", "decoder_embeddings.tok_cam.pos_emb"):
        assert k in buffers and k not in params
        assert torch.equal(buffers[k], dict(base.named_buffers())[k])
    assert m.cfg.learned_pos_emb_encoder == ("tok_cam",) and m.cfg.learned_pos_emb_decoder == ("tok_gaze",)
    assert m.engine.num_params() == base.engine.num_params() + 2 * 30 * 128
    assert sum(p.numel() for p in m.parameters()) == m.engine.num_params()
    # every flag at its default: the model of before
    same = _model(enc_learned=(), dec_learned=())
    assert same.engine.offsets == base.engine.offsets and same.engine.layout_tag() == base.engine.layout_tag()
    assert list(same.state_dict()) == list(base.state_dict()) == list(m.state_dict())
    assert not any(k.endswith("pos_emb") for k in dict(base.named_parameters()))
    # the video classes: a (1, 5120, dim) parameter per side
    v = _model(enc_learned=("tok_rgb",), dec_learned=("tok_rgb",), mods=("tok_rgb",), encoder_depth=1, decoder_depth=1, dim=384, num_heads=6)
    assert tuple(dict(v.named_parameters())["decoder_embeddings.tok_rgb.pos_emb"].shape) == (1, 5120, 384)
    assert dict(v.named_parameters())["decoder_embeddings.tok_rgb.pos_emb"].data_ptr() != \
        dict(v.named_parameters())["encoder_embeddings.tok_rgb.pos_emb"].data_ptr()


def test_optimiser_moves_decays_and_leaves_frozen_tables():
    torch.manual_seed(0)
    random.seed(0)
    m = _model(enc_learned=("tok_cam", "tok_gaze"), dec_learned=("tok_gaze",))
    lr, wd = 1e-2, 0.1
    opt = FusedAdamW(m.engine, lr=lr, weight_decay=wd, named_parameters=m.named_parameters())
    params = dict(m.named_parameters())
    frozen = params["encoder_embeddings.tok_gaze.pos_emb"]
    frozen.requires_grad_(False)
    md = synth.make_clip_batch(MODEL_CFGS["ego_tiny_2e_2d"], 2, {"tok_cam": (6, 6), "tok_gaze": (6, 6)}, seed=4)
    loss, _ = m(_cuda(md), 12, 12)
    loss.backward()
    keys = ("encoder_embeddings.tok_cam.pos_emb", "decoder_embeddings.tok_gaze.pos_emb")
    before = {k: (params[k].grad.clone(), params[k].detach().clone()) for k in keys}
    f0 = frozen.detach().clone()
    opt.step(zero_grad=False)
    torch.cuda.synchronize()
    assert torch.equal(frozen.detach(), f0)                                  # requires_grad_(False): bit-identical
    for k in keys:
        (g, p0), p1 = before[k], params[k].detach()
        hit = g[0].abs().amax(dim=1) > 0
        assert hit.any() and (~hit).any(), k
        # no gradient: m = v = 0, the update is the decoupled weight decay alone; with a gradient: the first AdamW step, ~ lr * sign(g)
        decayed = p0[0] * (1.0 - lr * wd)
        assert torch.allclose(p1[0][~hit], decayed[~hit], rtol=1e-6, atol=0.0) and not torch.equal(p1[0][~hit], p0[0][~hit])
        moved = (p1[0][hit] - decayed[hit]).abs()
        assert float(moved[g[0][hit].abs() > 1e-6].min()) > 0.5 * lr         # (|g| >> eps = 1e-8: the step is lr to within eps / |g|)


def _fb(eng, md, order, gscale=1.0, zero=True):
    loss, _ = eng.forward(md, dec_order=order)
    if zero:
        eng.zero_grad()
    eng.backward(gscale)
    torch.cuda.synchronize()
    return loss.clone(), eng.G.clone()


def test_reproducible_and_accumulating():
    cfg = _learned(MODEL_CFGS["ego_tiny_2e_2d"])
    eng = Engine(cfg, DEV, max_batch=4, n_enc=24, n_dec=24)
    eng.load_state_dict(_state(cfg, 5))
    order = ["tok_cam", "tok_gaze"]
    bud = {"tok_cam": (12, 12), "tok_gaze": (12, 12)}
    md1 = _cuda(synth.make_clip_batch(cfg, 4, bud, seed=5))
    md2 = _cuda(synth.make_clip_batch(cfg, 4, bud, seed=6))
    _, g1 = _fb(eng, md1, order, 0.5)
    _, g1b = _fb(eng, md1, order, 0.5)
    assert torch.equal(g1, g1b)                                              # two identical steps: bit-identical G
    _, g2 = _fb(eng, md2, order, 0.5)
    _fb(eng, md1, order, 0.5)
    _, acc = _fb(eng, md2, order, 0.5, zero=False)                           # accum_iter = 2
    for k in _pos_keys(cfg):
        o, n, _ = eng.offsets[k]
        a, s = acc[o:o + n], g1[o:o + n] + g2[o:o + n]
        assert float(g1[o:o + n].abs().max()) > 0 and float(g2[o:o + n].abs().max()) > 0
        # the kernel adds one micro-batch's sum onto what G holds: one fp32 rounding per element
        assert bool(((a - s).abs() <= 2.0 ** -23 * s.abs()).all()), k


def test_register_tokens_rows_and_context_gradient_reach_the_table():
    """with register tokens a sample's encoder rows are R + N and carry slot -2 rows; the table's gradient is the per-position sum
    of the input gradient and of the context gradient (`emb` is added back onto the projected context), summed here in fp64"""
    cfg = _learned(replace(MODEL_CFGS["ego_tiny_2e_2d"], num_register_tokens=4), dec=())
    eng = Engine(cfg, DEV, max_batch=3, n_enc=20, n_dec=20)
    eng.init_random(2)
    md = _cuda(synth.make_clip_batch(cfg, 3, {"tok_cam": (10, 10), "tok_gaze": (10, 10)}, seed=2))
    _fb(eng, md, ["tok_cam", "tok_gaze"])
    rows = 3 * eng.Ne
    slot, local = eng.ce["slot"].view(-1)[:rows].long(), eng.ce["local"].view(-1)[:rows].long()
    assert int((slot == -2).sum()) == 12
    term = eng.dxe[:rows].double() + eng.dctx[:rows].double()
    for i, m in enumerate(cfg.enc_mods):
        sel = slot == i
        ref = torch.zeros(30, eng.D, dtype=torch.float64, device=DEV).index_add_(0, local[sel], term[sel])
        mag = torch.zeros_like(ref).index_add_(0, local[sel], eng.dxe[:rows][sel].double().abs() + eng.dctx[:rows][sel].double().abs())
        got = eng.g[f"encoder_embeddings.{m.name}.pos_emb"].double()
        assert float(ref.abs().max()) > 0 and bool(((got - ref).abs() <= 4 * 2.0 ** -24 * mag).all()), m.name


def test_width_not_a_multiple_of_four():
    """the registered ego-XL geometry: dim 2046 in rows of 2048 - the table's gradient over all 2046 columns, pad columns zero"""
    cfg = _learned(replace(MODEL_CFGS["ego_XL_2046_1e_1d"], modalities=("tok_cam", "tok_gaze")), dec=("tok_gaze",))
    eng = Engine(cfg, DEV, max_batch=3, n_enc=20, n_dec=20)
    eng.init_random(6)
    assert (eng.Dl, eng.D) == (2046, 2048)
    md = _cuda(synth.make_clip_batch(cfg, 3, {"tok_cam": (10, 10), "tok_gaze": (10, 10)}, seed=6))
    _fb(eng, md, ["tok_cam", "tok_gaze"])
    assert int(eng.cd["err"].item()) == 0
    for side, c, dx, d2, mods, n in (("encoder", eng.ce, eng.dxe, eng.dctx, cfg.enc_mods, eng.Ne), ("decoder", eng.cd, eng.dres, None, eng.dmods, eng.M)):
        rows = 3 * n
        slot, local = c["slot"].view(-1)[:rows].long(), c["local"].view(-1)[:rows].long()
        term = dx[:rows].double() + (d2[:rows].double() if d2 is not None else 0.0)
        mag = dx[:rows].double().abs() + (d2[:rows].double().abs() if d2 is not None else 0.0)
        for i, m in enumerate(mods):
            k = f"{side}_embeddings.{m.name}.pos_emb"
            if k not in eng.g:
                continue
            sel = slot == i
            ref = torch.zeros(30, eng.D, dtype=torch.float64, device=DEV).index_add_(0, local[sel], term[sel])
            bound = 4 * 2.0 ** -24 * torch.zeros_like(ref).index_add_(0, local[sel], mag[sel])
            got = eng.g[k].double()
            assert float(ref[:, 2044:2046].abs().max()) > 0 and bool(((got - ref)[:, :2046].abs() <= bound[:, :2046]).all()), k
            assert float(got[:, 2046:].abs().max()) == 0.0, k
    assert "decoder_embeddings.tok_cam.pos_emb" not in eng.g and float(eng.g["decoder_embeddings.tok_gaze.pos_emb"].abs().max()) > 0


def test_broken_contract_turns_the_next_loss_into_nan():
    """rows that hold one position twice (what ego_compact never writes): the kernel raises the compaction's error word, and the next
    forward's loss is NaN - the run stops instead of training on a gradient with a row left out"""
    cfg = _learned(MODEL_CFGS["ego_tiny_2e_2d"])
    eng = Engine(cfg, DEV, max_batch=2, n_enc=24, n_dec=24)
    eng.init_random(1)
    md = _cuda(synth.make_clip_batch(cfg, 2, {"tok_cam": (12, 12), "tok_gaze": (12, 12)}, seed=1))
    order = ["tok_cam", "tok_gaze"]
    loss, _ = eng.forward(md, dec_order=order)
    assert torch.isfinite(loss)
    r = (eng.ce["slot"].view(-1)[:24] == 0).nonzero()[:2, 0]
    eng.ce["local"].view(-1)[r[1]] = eng.ce["local"].view(-1)[r[0]]
    eng.zero_grad()
    eng.backward(1.0)
    torch.cuda.synchronize()
    assert int(eng.cd["err"].item()) == 2
    loss, _ = eng.forward(md, dec_order=order)
    assert torch.isnan(loss) and int(eng.cd["err"].item()) == 0
    loss, _ = eng.forward(md, dec_order=order)
    assert torch.isfinite(loss)


def test_checkpoints_across_models():
    tiny = MODEL_CFGS["ego_tiny_2e_2d"]
    cfg = _learned(tiny)
    order = ["tok_gaze", "tok_cam"]
    md = _cuda(synth.make_clip_batch(tiny, 2, {"tok_cam": (12, 12), "tok_gaze": (12, 12)}, seed=8))
    fixed = Engine(tiny, DEV, max_batch=2, n_enc=24, n_dec=24)
    fixed.init_random(8)
    learned = Engine(cfg, DEV, max_batch=2, n_enc=24, n_dec=24)
    learned.init_random(9)
    # a sin-cos checkpoint into the learned model: the fixed tables are the starting values, the forward is the sin-cos model's
    assert learned.load_state_dict(fixed.state_dict()) == []
    for k in _pos_keys(cfg):
        assert torch.equal(learned.state_dict()[k], fixed.state_dict()[k])
    l0, _ = fixed.forward(md, dec_order=order)
    l1, _ = learned.forward(md, dec_order=order)
    assert torch.equal(l0, l1)
    # a learned checkpoint into a learned model, through the module surface (strict)
    a = _model(enc_learned=("tok_cam", "tok_gaze"), dec_learned=("tok_cam", "tok_gaze"))
    b = _model(enc_learned=("tok_cam", "tok_gaze"), dec_learned=("tok_cam", "tok_gaze"))
    assert not torch.equal(a.engine.P, b.engine.P)
    res = b.load_state_dict({k: v.clone() for k, v in a.state_dict().items()})
    assert not res.missing_keys and not res.unexpected_keys and torch.equal(a.engine.P, b.engine.P)
    # the optimiser state of the sin-cos run continues in the learned model: the tables start with zero moments at step 1
    of, ol = FusedAdamW(fixed), FusedAdamW(learned)
    of.m.fill_(0.25); of.v.fill_(0.5); of.t = 7
    ol.load_state_dict(of.state_dict())
    body = fixed.n_flat
    assert ol.t == 7 and torch.equal(ol.m[:body], of.m) and float(ol.m[body:].abs().max()) == 0.0 and float(ol.v[body:].abs().max()) == 0.0
    assert all(ol.skipped[k] == 7 for k in _pos_keys(cfg))
    # ... and the runs the next step walks say so (this optimiser has no named parameters): every table in a run that sat 7 steps out
    runs = ol._active_runs()
    for k in _pos_keys(cfg):
        o, n, _ = learned.offsets[k]
        assert any(lo <= o and o + n <= hi and sk == 7 for lo, hi, _, sk in runs), k
    assert all(sk == 0 for lo, hi, _, sk in runs if hi <= body) and runs[0][0] == 0


def test_generation_reads_the_learned_decoder_table():
    cfg = _learned(MODEL_CFGS["ego_gen_384_2e_2d"], enc=(), dec=("tok_rgb", "tok_depth"))
    eng = Engine(cfg, DEV, max_batch=1, n_enc=64, n_dec=64)
    eng.init_random(3)
    sample = {"tok_rgb": {"tensor": synth.randint("pg.rgb", (1, 5, 32, 32), 64000, seed=1).to(DEV)}}
    sample = init_empty_target_modality(sample, MODALITY_INFO, "tok_depth", 1, 5120, DEV)
    sample = init_full_input_modality(sample, MODALITY_INFO, "tok_rgb", DEV)
    sch = build_chained_generation_schedules(["tok_rgb"], ["tok_depth"], [5120], ["roar"], [3], ["linear"], [0.01], ["constant"],
                                             [2.0], ["constant"], cfg_grow_conditioning=True)
    a = GenerationSampler(eng, use_graphs=False).generate(sample, sch, top_p=0.8, seed=3)["tok_depth"]["tensor"].clone()
    b = GenerationSampler(eng, use_graphs=True).generate(sample, sch, top_p=0.8, seed=3)["tok_depth"]["tensor"].clone()
    assert torch.equal(a, b)
    # the same weights under the sin-cos table: other tokens - the generation path reads the learned table
    eng.drop_graphs()
    eng.p["decoder_embeddings.tok_depth.pos_emb"].copy_(eng.pos["tok_depth"])
    c = GenerationSampler(eng, use_graphs=False).generate(sample, sch, top_p=0.8, seed=3)["tok_depth"]["tensor"]
    assert not torch.equal(a, c)


def test_activation_checkpointing_composes():
    cfg = _learned(MODEL_CFGS["ego_tiny_2e_2d"])
    sd = _state(cfg, 12)
    md = _cuda(synth.make_clip_batch(cfg, 4, {"tok_cam": (12, 12), "tok_gaze": (12, 12)}, seed=12))
    out = []
    for ck in (False, True):
        eng = Engine(cfg, DEV, max_batch=4, n_enc=24, n_dec=24, act_checkpoint=ck)
        eng.load_state_dict(sd)
        out.append(_fb(eng, md, ["tok_cam", "tok_gaze"]))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    o, n, _ = eng.offsets["encoder_embeddings.tok_cam.pos_emb"]
    assert float(out[0][1][o:o + n].abs().max()) > 0
