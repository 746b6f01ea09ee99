"""The QK-norm family (`qk_norm=True`: NormAttention / NormCrossAttention, egom2p_utils.py:247-332; the `*_swiglu_qknorm_nobias`
registrations, egom2p_model.py:1122-1196) through the module surface on the GPU: construct through the constructor keyword, forward /
backward against a fixture made from the real reference (tools/make_goldens_qknorm.py: tests/golden/b2_qknorm.npz), the head-norm
weights applied, differentiated, stepped without weight decay and round-tripped, generation against tests/golden/
gen_rgb2depth_qknorm.npz, and what is refused.

Tolerances of the fixture replay are those `b2_causal` and `b2_gelu` are held to at this width and depth: `ACT_TOL` / `GRAD_TOL` /
`LOSS_RTOL` of tests/test_engine_gpu.py.  Every measured error is also held to its recorded value in
tests/golden/parity_bars_qknorm.json by the `_bar` rule of tests/test_gelu_engine_gpu.py, on a file of this family's own."""
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_engine_gpu as TE  # noqa: E402
import test_generate_gpu as TGEN  # noqa: E402
from conftest import GOLDEN_DIR, load_golden, rel_l2  # noqa: E402
from egom2p_amd import synth  # noqa: E402
from egom2p_amd.config import MODEL_CFGS  # noqa: E402
from egom2p_amd.engine import Engine  # noqa: E402
from egom2p_amd.generate import (GenerationSampler, build_chained_generation_schedules, init_empty_target_modality,  # noqa: E402
                                 init_full_input_modality)
from egom2p_amd.model import MODALITY_INFO, create_model  # noqa: E402
from egom2p_amd.optim import FusedAdamW, is_no_decay  # noqa: E402

DEV = "cuda"
BASE_NAME = "egom2p_tiny_6e_6d_swiglu_nobias"
MODS = ["tok_rgb", "tok_depth", "tok_cam", "tok_gaze"]
SITES = ([f"encoder.{i}.attn" for i in range(2)] + [f"decoder.{i}.{s}" for i in range(2) for s in ("self_attn", "cross_attn")])
HEAD_NORMS = [f"{s}.{n}_norm.weight" for s in SITES for n in ("q", "k")]
_CACHE = {}
BARS_PATH = os.path.join(GOLDEN_DIR, "parity_bars_qknorm.json")


def _bar(name, value, hard, rel_margin=0.30):
    """tests/test_gelu_engine_gpu.py's `_bar` on this family's own file: value <= the stated tolerance and <= the recorded value x 1.30.
    EGOM2P_RECORD_BARS=<file>: append {"name", "value"} lines instead of checking the recorded value."""
    value = float(value)
    rec = os.environ.get("EGOM2P_RECORD_BARS")
    if rec:
        with open(rec, "a") as f:
            f.write(json.dumps({"name": name, "value": value}) + "\n")
    assert value <= hard, (name, value, "stated tolerance", hard)
    if "bars" not in _CACHE:
        _CACHE["bars"] = json.load(open(BARS_PATH)) if os.path.exists(BARS_PATH) else {}
    base = _CACHE["bars"].get(name)
    if base is not None and not rec:
        assert value <= float(base) * (1.0 + rel_margin), (name, value, "recorded", base)
    return value


def _model(**kw):
    """the registered tiny variant at the fixtures' depth (dim 384, 6 heads, 2 + 2 layers); qk_norm through the constructor keyword"""
    enc = {m: MODALITY_INFO[m]["encoder_embedding"]() for m in MODS}
    dec = {m: MODALITY_INFO[m]["decoder_embedding"]() for m in MODS}
    args = dict(encoder_depth=2, decoder_depth=2)
    args.update(kw)
    return create_model(BASE_NAME, encoder_embeddings=enc, decoder_embeddings=dec, modality_info=MODALITY_INFO, **args)


def _case():
    if "case" not in _CACHE:
        g, meta = load_golden("b2_qknorm")
        cfg = MODEL_CFGS[meta["cfg"]]
        sd = synth.build_state_dict(cfg, meta["seed"])
        md = synth.make_clip_batch(cfg, meta["batch"], meta["budgets"], meta["seed"])
        _CACHE["case"] = (g, meta, cfg, sd, {k: {kk: vv.cuda() for kk, vv in v.items()} for k, v in md.items()})
    return _CACHE["case"]


def _qk_model():
    if "model" not in _CACHE:
        g, meta, cfg, sd, md = _case()
        model = _model(qk_norm=True)
        assert set(model.state_dict().keys()) == set(sd.keys())
        model.load_state_dict(sd)
        _CACHE["model"] = model
    return _CACHE["model"]


def _run(model, md, meta, backward=False):
    random.seed(meta["py_seed"])
    model.engine.weights_dirty = True
    if backward:
        model.engine.zero_grad()
        loss, _ = model(md, meta["n_enc"], meta["n_dec"])
        loss.backward()
        return float(loss.item())
    with torch.no_grad():
        return float(model(md, meta["n_enc"], meta["n_dec"])[0].item())


# ---------------------------------------------------------------------------------------------- construction
def test_qk_norm_constructs_through_the_constructor_keyword():
    """(raises NotImplementedError before the QK-norm family existed)"""
    model = _model(qk_norm=True)
    assert model.cfg.qk_norm and model.engine.qk_norm
    named = dict(model.named_parameters())
    for k in HEAD_NORMS:
        assert k in named and tuple(named[k].shape) == (64,) and bool((named[k] == 1.0).all()), k      # init: weight 1
        assert k[:-len("weight")] + "bias" in dict(model.named_buffers())                               # the bias-free LayerNorm's zero buffer
    # its key set is the reference's (the synthetic state dict is built under the reference's names and loads strictly there)
    sd = synth.build_state_dict(MODEL_CFGS["ego_384_2e_2d_qknorm"], 1, posemb=True)
    assert set(model.state_dict().keys()) == set(sd.keys())
    assert all(tuple(model.state_dict()[k].shape) == tuple(v.shape) for k, v in sd.items())
    # the same call without the keyword: the old key set, parameter count and physical layout
    plain = _model()
    assert not plain.cfg.qk_norm
    assert set(plain.state_dict().keys()) == set(synth.build_state_dict(MODEL_CFGS["ego_384_2e_2d_causal"], 1).keys())
    n_qk = sum(p.numel() for p in model.parameters())
    n_plain = sum(p.numel() for p in plain.parameters())
    assert n_qk - n_plain == 12 * 64 and model.engine.num_params() - plain.engine.num_params() == 12 * 64
    ref = Engine(MODEL_CFGS["ego_384_2e_2d_causal"], "cuda:0", max_batch=1, n_enc=1, n_dec=1)      # (the mask flag owns no storage)
    assert plain.engine.layout_tag() == ref.layout_tag() and plain.engine.offsets == ref.offsets
    assert model.engine.layout_tag() != plain.engine.layout_tag()
    assert model.engine.n_flat - plain.engine.n_flat == 12 * 64
    # flags are independent, as in the reference constructor: qk_norm beside linear biases
    m2 = _model(qk_norm=True, qkv_bias=True, proj_bias=True, encoder_depth=1, decoder_depth=1)
    n2 = dict(m2.named_parameters())
    assert "encoder.0.attn.qkv.bias" in n2 and "decoder.0.cross_attn.k_norm.weight" in n2


# ---------------------------------------------------------------------------------------------- b2_qknorm replay
def _dec_tap_err(g, key, t, valid):
    t = t.float().cpu()
    e1 = rel_l2(t[:, :6, :24].numpy(), g[f"tap_head.{key}"])
    e2 = rel_l2(t.double().norm(dim=-1).numpy()[valid], g[f"tap_rownorm.{key}"][valid])
    return max(e1, e2)


def test_qk_norm_model_matches_the_reference_fixture():
    model = _qk_model()
    g, meta, cfg, sd, md = _case()
    eng = model.engine
    B, N, M, D = meta["batch"], meta["n_enc"], meta["n_dec"], cfg.dim
    random.seed(meta["py_seed"])
    eng.weights_dirty = True
    eng.zero_grad()
    loss, mod_loss = model(md, N, M, loss_type="mod")
    torch.cuda.synchronize()
    # held exactly: ids, masks, decoder order
    assert [m.name for m in eng.dmods] == [str(x) for x in g["dec_order"]]
    assert np.array_equal(eng.ce["ids_keep"][:B].cpu().numpy(), g["enc_ids_keep"])
    assert np.array_equal(eng.cd["ids_keep"][:B].cpu().numpy(), g["dec_ids_keep"])
    assert np.array_equal(eng.ce["pad"][:B].cpu().numpy().astype(bool), g["enc_pad"])
    assert np.array_equal(eng.cd["pad"][:B].cpu().numpy().astype(bool), g["dec_pad"])
    assert np.array_equal(eng.ce["mod_mask"][:B].cpu().numpy(), g["enc_mod_mask"])
    assert np.array_equal(eng.cd["mod_mask"][:B].cpu().numpy(), g["dec_mod_mask"])
    assert np.array_equal(eng.cd["tok"][:B].cpu().numpy(), g["target_ids"])
    assert eng.cd["err"].item() == 0
    valid = ~g["dec_pad"]
    blocked = np.unpackbits(g["dec_attn_mask_packed"], axis=-1)[:, :, :M].astype(bool)
    ks, ke = eng.cd["ks"][:B].cpu().numpy(), eng.cd["ke"][:B].cpu().numpy()
    j = np.arange(M)[None, None, :]
    assert np.array_equal(((j >= ks[:, :, None]) & (j < ke[:, :, None]))[valid], ~blocked[valid])
    # taps, by slices and row norms
    RN, RM = B * N, B * M
    act = lambda t, rows, n: t[:rows].view(B, n, D)      # noqa: E731
    assert TE._tap(g, "enc_x0", act(eng.enc[0]["x"], RN, N)) < 1e-6
    _bar("b2_qknorm.enc_block0", TE._tap(g, "enc_block0", act(eng.enc[1]["x"], RN, N)), TE.ACT_TOL)
    _bar("b2_qknorm.enc_out", TE._tap(g, "enc_out", act(eng.xe, RN, N)), TE.ACT_TOL)
    _bar("b2_qknorm.context", TE._tap(g, "context", act(eng.ctx, RN, N)), TE.ACT_TOL)
    assert _dec_tap_err(g, "dec_y0", act(eng.dec[0]["x"], RM, M), valid) < 1e-6
    _bar("b2_qknorm.dec_block0", _dec_tap_err(g, "dec_block0", act(eng.dec[1]["x"], RM, M), valid), TE.ACT_TOL)
    vt = torch.from_numpy(valid).cuda()
    perm = eng.perm[:RM].view(B, M)[vt].long()
    _bar("b2_qknorm.dec_out", rel_l2(eng.yn[perm][:, :D].float().norm(dim=-1).cpu().numpy(), g["tap_rownorm.dec_out"][valid]), TE.ACT_TOL)
    # loss
    ref_loss = float(g["loss"])
    print(f"b2_qknorm: loss {loss.item():.6f} (reference {ref_loss:.6f})")
    _bar("b2_qknorm.loss", abs(loss.item() - ref_loss) / abs(ref_loss), TE.LOSS_RTOL)
    for n in MODS:
        r = float(g[f"mod_loss.{n}"])
        assert abs(mod_loss[n].item() - r) < TE.LOSS_RTOL * max(abs(r), 1.0), (n, mod_loss[n].item(), r)
    # gradients: one norm per tensor, the 12 head-norm weights included
    loss.backward()
    torch.cuda.synchronize()
    names = [str(x) for x in g["grad_names"]]
    assert sorted(n for n in names if "q_norm" in n or "k_norm" in n) == sorted(HEAD_NORMS)
    worst, worst_hn = ("", 0.0), ("", 0.0)
    for n, ref_sq in zip(names, g["grad_sqnorm_all"]):
        got_sq = eng.grad_of(n).double().pow(2).sum().item()
        if ref_sq < 0:
            assert got_sq == 0.0, n
            continue
        err = abs(got_sq ** 0.5 - ref_sq ** 0.5) / max(ref_sq ** 0.5, 1e-12)
        print(f"b2_qknorm grad {n}: {err:.3e}") if n in HEAD_NORMS else None
        assert err < TE.GRAD_TOL, (n, err)
        worst = max(worst, (n, err), key=lambda x: x[1])
        if n in HEAD_NORMS:
            assert got_sq > 0.0, n
            worst_hn = max(worst_hn, (n, err), key=lambda x: x[1])
    print(f"b2_qknorm: worst gradient norm error {worst}, among the head norms {worst_hn}")
    _bar("b2_qknorm.grad_norm_worst", worst[1], TE.GRAD_TOL)
    _bar("b2_qknorm.grad_norm_worst_head_norm", worst_hn[1], TE.GRAD_TOL)
    coef = min(1.0, 1.0 / (float(g["clip_total_norm"]) + 1e-6))
    for key in g.files:
        if key.startswith("grad_head."):
            gr = eng.grad_of(key[10:]) * coef
            e = rel_l2(gr.reshape(-1, gr.shape[-1])[:4, :32].float().cpu().numpy(), g[key])
            assert e < 2 * TE.GRAD_TOL, (key, e)


# ---------------------------------------------------------------------------------------------- the norm is applied
def test_head_norm_is_applied_and_its_weights_matter():
    model = _qk_model()
    g, meta, cfg, sd, md = _case()
    named = dict(model.named_parameters())
    try:
        l0 = _run(model, md, meta, backward=True)
        for k in HEAD_NORMS:
            assert bool(named[k].grad.any()), k
        # a weight that is loaded but not applied leaves the loss where it was
        for k in ("encoder.1.attn.k_norm.weight", "decoder.0.cross_attn.q_norm.weight", "decoder.1.self_attn.q_norm.weight"):
            with torch.no_grad():
                named[k].mul_(1.5)
            l1 = _run(model, md, meta)
            with torch.no_grad():
                named[k].copy_(sd[k].to(DEV))
            # (every kernel on the path is deterministic: an unapplied weight would give the same loss bit for bit)
            assert l1 != l0, (k, l0, l1)
        # all head-norm weights 1: still not the model without the norm (the norm itself is not skipped)
        with torch.no_grad():
            for k in HEAD_NORMS:
                named[k].fill_(1.0)
        l_ones = _run(model, md, meta)
        plain = _model()
        plain.load_state_dict({k: v for k, v in sd.items() if "q_norm" not in k and "k_norm" not in k})
        l_plain = _run(plain, md, meta)
        print(f"loss: qk_norm {l0:.6f}, head-norm weights 1 {l_ones:.6f}, qk_norm=False {l_plain:.6f}")
        # a norm that is skipped would run the flag-free model's launches on the same weights: the same loss bit for bit
        assert l_ones != l_plain
        # and the normalised q / k the attention launches read are normalised: every head slice has mean 0 and variance 1 to bf16's
        # rounding (2^-9 relative per element: 1e-2 on a mean of 64 values of size ~1 and 2e-2 on their variance are loose by 10x)
        eng, A = model.engine, model.engine.A
        # (the rows of sample 0, which has no padding rows: an all-zero padding row stays zero)
        for buf, rows, pitch, off in ((eng.enc[0]["qkn"], meta["n_enc"], 3 * A, 0), (eng.enc[1]["qkn"], meta["n_enc"], 3 * A, A),
                                      (eng.dec[1]["xqn"], meta["n_dec"], A, 0), (eng.dec[0]["xkn"], meta["n_enc"], 2 * A, 0)):
            v = buf[:rows].view(rows, pitch)[:, off:off + A].float().view(rows, A // 64, 64)
            assert float(v.mean(-1).abs().max()) < 1e-2 and float((v.var(-1, unbiased=False) - 1.0).abs().max()) < 2e-2
    finally:
        model.load_state_dict(sd)


def test_backward_is_bitwise_reproducible():
    model = _qk_model()
    g, meta, cfg, sd, md = _case()
    eng = model.engine
    random.seed(meta["py_seed"])
    eng.zero_grad()
    loss, _ = model(md, meta["n_enc"], meta["n_dec"])
    logits = {v: t.clone() for v, t in eng.logits.items()}      # (the cross-entropy backward turns the logits into d logits in place)
    eng.backward(1.0)
    G1 = eng.G.clone()
    eng.zero_grad()
    # a second backward pass of the SAME forward: the saved activations are still there, the logits are put back
    for v, t in logits.items():
        eng.logits[v].copy_(t)
    eng._have_fwd = True
    eng.backward(1.0)
    torch.cuda.synchronize()
    assert torch.equal(G1, eng.G) and bool(G1.any())


# ---------------------------------------------------------------------------------------------- step and state round trip
def test_fused_adamw_moves_the_head_norm_weights_without_decay_and_state_round_trips():
    model = _qk_model()
    g, meta, cfg, sd, md = _case()
    eng = model.engine
    model.load_state_dict(sd)
    named = dict(model.named_parameters())
    nd_ranges = [(lo, hi) for lo, hi, nd in eng.opt_runs if nd]
    for k in HEAD_NORMS:                       # the reference's rule matches "norm." (optim_factory.py:113)
        o, n, _ = eng.offsets[k]
        assert is_no_decay(k) and any(lo <= o and o + n <= hi for lo, hi in nd_ranges), k
    for name, (o, n, _) in eng.offsets.items():
        if not is_no_decay(name):
            assert not any(lo <= o < hi for lo, hi in nd_ranges), name
    opt = FusedAdamW(eng, lr=1e-3, weight_decay=0.05, named_parameters=model.named_parameters())
    ref = {n: p.detach().clone().requires_grad_(True) for n, p in named.items()}
    topt = torch.optim.AdamW([{"params": [ref[n] for n in ref if not is_no_decay(n)], "weight_decay": 0.05},
                              {"params": [ref[n] for n in ref if is_no_decay(n)], "weight_decay": 0.0}], lr=1e-3, betas=(0.9, 0.95), eps=1e-8)
    try:
        for step in range(2):
            random.seed(meta["py_seed"] + step)
            eng.zero_grad()
            loss, _ = model(md, meta["n_enc"], meta["n_dec"])
            loss.backward()
            for n in ref:
                ref[n].grad = named[n].grad.detach().clone()
            topt.step()
            opt.step()
            worst = max((rel_l2(named[n].detach().float().cpu().numpy(), ref[n].detach().float().cpu().numpy()), n) for n in ref)
            assert worst[0] < 1e-6, (step, worst)
        for k in HEAD_NORMS:
            assert not torch.equal(named[k].detach().cpu(), sd[k]), k
        # the optimiser state round-trips: a fresh optimiser over a fresh model takes it and steps to the same bits
        osd = opt.state_dict()
        out = {k: v.detach().clone() for k, v in model.state_dict().items()}
        fresh = _model(qk_norm=True)
        fresh.load_state_dict(out)
        assert torch.equal(fresh.engine.P, eng.P)
        fopt = FusedAdamW(fresh.engine, lr=1e-3, weight_decay=0.05, named_parameters=fresh.named_parameters())
        fopt.load_state_dict(osd)
        for m_, o_ in ((model, opt), (fresh, fopt)):
            random.seed(meta["py_seed"] + 7)
            m_.engine.zero_grad()
            loss, _ = m_(md, meta["n_enc"], meta["n_dec"])
            loss.backward()
            o_.step()
        assert torch.equal(fresh.engine.P, eng.P)
        # ... and a checkpoint of the flag-free layout is refused by the layout tag, not by a bare copy
        popt = FusedAdamW(_model().engine, lr=1e-3, weight_decay=0.05)
        with pytest.raises(RuntimeError, match="storage layout"):
            popt.load_state_dict(osd)
    finally:
        model.load_state_dict(sd)


# ---------------------------------------------------------------------------------------------- generation
def test_generation_matches_the_reference_fixture():
    """tests/test_generate_gpu.py's replay of a reference `GenerationSampler` run, token for token under teacher forcing, with its
    bars on the logits and its near-tie rule, on the qk-norm fixture"""
    TGEN.test_roar_cfg_generation_matches_reference("gen_rgb2depth_qknorm")


def test_graphed_generation_equals_eager():
    cfg = MODEL_CFGS["ego_gen_384_2e_2d_qknorm"]
    eng = Engine(cfg, "cuda:0", max_batch=1, n_enc=64, n_dec=64)
    eng.load_state_dict(synth.build_state_dict(cfg, 4))             # (head-norm weights off 1)
    sample = {"tok_rgb": {"tensor": synth.randint("gg.rgb", (1, 5, 32, 32), 64000, seed=1).to(DEV)}}
    sample = init_empty_target_modality(sample, MODALITY_INFO, "tok_depth", 1, 5120, DEV)
    sample = init_full_input_modality(sample, MODALITY_INFO, "tok_rgb", DEV)
    sch = build_chained_generation_schedules(["tok_rgb"], ["tok_depth"], [5120], ["roar"], [3], ["linear"], [0.01], ["constant"],
                                             [2.0], ["constant"], cfg_grow_conditioning=True)
    a = GenerationSampler(eng, use_graphs=False).generate(sample, sch, top_p=0.8, seed=3)["tok_depth"]["tensor"]
    b = GenerationSampler(eng, use_graphs=True).generate(sample, sch, top_p=0.8, seed=3)["tok_depth"]["tensor"]
    assert torch.equal(a, b)
    c = GenerationSampler(eng).generate_graphed(sample, sch, top_p=0.8, seed=3)["tok_depth"]["tensor"]
    assert torch.equal(a, c)


# ---------------------------------------------------------------------------------------------- refusals
def test_what_is_refused_with_qk_norm():
    from functools import partial
    from torch import nn
    with pytest.raises(NotImplementedError, match="qk_norm"):
        _model(qk_norm=True, dim=1020, num_heads=15, encoder_depth=1, decoder_depth=1)          # padded geometry
    with pytest.raises(NotImplementedError, match="qk_norm"):
        _model(qk_norm=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), encoder_depth=1, decoder_depth=1)      # norm_bias=True
    cfg = MODEL_CFGS["ego_384_2e_2d_qknorm"]
    for kw in (dict(fp8_forward=True), dict(fp8_forward=True, fp8_backward=True)):
        with pytest.raises(NotImplementedError, match="qk_norm"):
            Engine(cfg, "cuda:0", max_batch=1, n_enc=64, n_dec=64, **kw)
