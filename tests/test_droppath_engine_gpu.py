"""Stochastic depth (`drop_path_rate_encoder`, `drop_path_rate_decoder`, `shared_drop_path`: egom2p_model.py:96-98, 137-161; `DropPath`,
egom2p_utils.py:89-112, applied at :356-359, 387-391) through the module surface on the GPU: construction and the site table, forward /
backward against a fixture made from the real reference with hand-chosen keep tables (tools/make_goldens_droppath.py:
tests/golden/b2_droppath.npz), the exact identities of dropped branches, mode switching, the device draw inside the training loop,
and the combinations with the QK-norm and the GELU / biased families.

Tolerances of the fixture replay: `ACT_TOL` / `GRAD_TOL` / `LOSS_RTOL` of tests/test_engine_gpu.py.  Every measured error is also held to
its recorded value in tests/golden/parity_bars_droppath.json by the `_bar` rule of tests/test_gelu_engine_gpu.py."""
import dataclasses
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _droppath_ref as R  # noqa: E402
import test_engine_gpu as TE  # noqa: E402
from conftest import GOLDEN_DIR, load_golden, rel_l2  # noqa: E402
from egom2p_amd import ops, synth  # noqa: E402
from egom2p_amd.config import MODEL_CFGS  # noqa: E402
from egom2p_amd.engine import Engine  # noqa: E402
from egom2p_amd.generate import (GenerationSampler, build_chained_generation_schedules, init_empty_target_modality,  # noqa: E402
                                 init_full_input_modality)
from egom2p_amd.model import MODALITY_INFO, create_model  # noqa: E402

DEV = "cuda"
BASE_NAME = "egom2p_tiny_6e_6d_swiglu_nobias"
GELU_NAME = "egom2p_tiny_6e_6d_gelu"
MODS = ["tok_rgb", "tok_depth", "tok_cam", "tok_gaze"]
ENC_SUBS, DEC_SUBS = ("attn", "mlp"), ("self_attn", "cross_attn", "mlp")
_CACHE = {}
BARS_PATH = os.path.join(GOLDEN_DIR, "parity_bars_droppath.json")


def _bar(name, value, hard, rel_margin=0.30):
    """tests/test_gelu_engine_gpu.py's `_bar` on this feature's own file: value <= the stated tolerance and <= the recorded value x 1.30.
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


def _model(name=BASE_NAME, **kw):
    """the registered tiny variant at the fixtures' depth (dim 384, 6 heads, 2 + 2 layers); drop path through the constructor keywords"""
    enc = {m: MODALITY_INFO[m]["encoder_embedding"]() for m in MODS}
    dec = {m: MODALITY_INFO[m]["decoder_embedding"]() for m in MODS}
    args = dict(encoder_depth=2, decoder_depth=2)
    args.update(kw)
    return create_model(name, encoder_embeddings=enc, decoder_embeddings=dec, modality_info=MODALITY_INFO, **args)


def _case():
    if "case" not in _CACHE:
        g, meta = load_golden("b2_droppath")
        cfg = MODEL_CFGS[meta["cfg"]]
        sd = synth.build_state_dict(cfg, meta["seed"])
        md = synth.make_clip_batch(cfg, meta["batch"], meta["budgets"], meta["seed"])
        _CACHE["case"] = (g, meta, cfg, sd, {k: {kk: vv.cuda() for kk, vv in v.items()} for k, v in md.items()})
    return _CACHE["case"]


def _dp_model():
    """the fixture's model: rates 0.3 / 0.3 under shared_drop_path (per layer 0, 0.1 | 0.2, 0.3), the fixture's weights"""
    if "model" not in _CACHE:
        g, meta, cfg, sd, md = _case()
        model = _model(drop_path_rate_encoder=0.3, drop_path_rate_decoder=0.3, shared_drop_path=True)
        model.load_state_dict(sd)
        _CACHE["model"] = model
    return _CACHE["model"]


def _plain_model():
    if "plain" not in _CACHE:
        g, meta, cfg, sd, md = _case()
        model = _model()
        model.load_state_dict(sd)
        _CACHE["plain"] = model
    return _CACHE["plain"]


def _one_clip(cfg, seed=5):
    """one unpadded clip at N = 256, M = 320 (sample 0 of the fixture's budgets)"""
    budgets = {"tok_rgb": [(140, 200)], "tok_depth": [(100, 90)], "tok_cam": [(10, 20)], "tok_gaze": [(6, 10)]}
    md = synth.make_clip_batch(cfg, 1, budgets, seed)
    return {k: {kk: vv.cuda() for kk, vv in v.items()} for k, v in md.items()}


# ---------------------------------------------------------------------------------------------- 1. construction
def test_drop_path_constructs_and_owns_no_parameters():
    """(raised NotImplementedError "drop path" before the feature existed)"""
    model = _model(drop_path_rate_encoder=0.1)
    eng = model.engine
    assert model.cfg.drop_path_rate_encoder == 0.1 and model.cfg.drop_path_rate_decoder == 0.0 and not model.cfg.shared_drop_path
    # default rule: linspace(0, 0.1, 2) = [0, 0.1] for the encoder, the decoder at 0
    assert eng.dp_sites == R.site_table(*R.rates(0.1, 0.0, 2, 2, False)) == [("encoder.1.attn", R.keep_prob(R.f32(0.1))),
                                                                             ("encoder.1.mlp", R.keep_prob(R.f32(0.1)))]
    # shared rule: one ramp over 2 + 2 layers
    shared = _dp_model().engine
    want = R.site_table(*R.rates(0.3, 0.3, 2, 2, True))
    assert shared.dp_sites == want and len(want) == 8 and len({kp for _, kp in want}) == 3
    assert [n for n, _ in want] == [f"encoder.1.{s}" for s in ENC_SUBS] + [f"decoder.{i}.{s}" for i in range(2) for s in DEC_SUBS]
    g, meta = load_golden("b2_droppath")
    assert [r for r in meta["rates_encoder"] + meta["rates_decoder"]] == [repr(r) for r in sum(R.rates(0.3, 0.3, 2, 2, True), [])]
    # no parameters, no storage: key set, parameter count, flat layout of the model without drop path
    plain = _model()
    assert not plain.engine.dp_sites and not hasattr(plain.engine, "dp_keep") and not hasattr(plain.engine, "dp_branch")
    for m in (model, _dp_model()):
        assert set(m.state_dict().keys()) == set(plain.state_dict().keys())
        assert sum(p.numel() for p in m.parameters()) == sum(p.numel() for p in plain.parameters())
        assert m.engine.num_params() == plain.engine.num_params()
        assert m.engine.layout_tag() == plain.engine.layout_tag() and m.engine.offsets == plain.engine.offsets
    # every registered family takes the keywords
    m2 = _model(GELU_NAME, drop_path_rate_decoder=0.2, encoder_depth=1, decoder_depth=2)
    assert [n for n, _ in m2.engine.dp_sites] == [f"decoder.1.{s}" for s in DEC_SUBS]
    with pytest.raises(ValueError):
        _model(drop_path_rate_encoder=1.0)


# ---------------------------------------------------------------------------------------------- 2. b2_droppath replay
def _dec_tap_err(g, key, t, valid):
    t = t.float().cpu()
    e1 = rel_l2(t[:, :6, :24].numpy(), g[f"tap_head.{key}"])
    e2 = rel_l2(t.double().norm(dim=-1).numpy()[valid], g[f"tap_rownorm.{key}"][valid])
    return max(e1, e2)


def test_drop_path_model_matches_the_reference_fixture():
    model = _dp_model()
    g, meta, cfg, sd, md = _case()
    eng = model.engine
    B, N, M, D = meta["batch"], meta["n_enc"], meta["n_dec"], cfg.dim
    model.train()
    random.seed(meta["py_seed"])
    eng.weights_dirty = True
    eng.zero_grad()
    eng.inject_drop_path(torch.from_numpy(g["keep.encoder"]), torch.from_numpy(g["keep.decoder"]))
    loss, mod_loss = model(md, N, M, loss_type="mod")
    torch.cuda.synchronize()
    # the injected tables are the ones used (rate-0 entries ignored: encoder layer 0 has no site)
    tab = eng.drop_path_table().cpu().numpy().astype(bool)
    want = np.concatenate([g["keep.encoder"][1], g["keep.decoder"][0], g["keep.decoder"][1]])
    assert np.array_equal(tab, want) and all(r.any() and not r.all() for r in tab)
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
    # taps, by slices and row norms
    RN, RM = B * N, B * M
    act = lambda t, rows, n: t[:rows].view(B, n, D)      # noqa: E731
    assert TE._tap(g, "enc_x0", act(eng.enc[0]["x"], RN, N)) < 1e-6
    _bar("b2_droppath.enc_block0", TE._tap(g, "enc_block0", act(eng.enc[1]["x"], RN, N)), TE.ACT_TOL)
    _bar("b2_droppath.enc_out", TE._tap(g, "enc_out", act(eng.xe, RN, N)), TE.ACT_TOL)
    _bar("b2_droppath.context", TE._tap(g, "context", act(eng.ctx, RN, N)), TE.ACT_TOL)
    assert _dec_tap_err(g, "dec_y0", act(eng.dec[0]["x"], RM, M), valid) < 1e-6
    _bar("b2_droppath.dec_block0", _dec_tap_err(g, "dec_block0", act(eng.dec[1]["x"], RM, M), valid), TE.ACT_TOL)
    vt = torch.from_numpy(valid).cuda()
    perm = eng.perm[:RM].view(B, M)[vt].long()
    _bar("b2_droppath.dec_out", rel_l2(eng.yn[perm][:, :D].float().norm(dim=-1).cpu().numpy(), g["tap_rownorm.dec_out"][valid]), TE.ACT_TOL)
    # loss
    ref_loss = float(g["loss"])
    print(f"b2_droppath: loss {loss.item():.6f} (reference {ref_loss:.6f})")
    _bar("b2_droppath.loss", abs(loss.item() - ref_loss) / abs(ref_loss), TE.LOSS_RTOL)
    for n in MODS:
        r = float(g[f"mod_loss.{n}"])
        assert abs(mod_loss[n].item() - r) < TE.LOSS_RTOL * max(abs(r), 1.0), (n, mod_loss[n].item(), r)
    # gradients: one norm per tensor
    loss.backward()
    torch.cuda.synchronize()
    names = [str(x) for x in g["grad_names"]]
    worst = ("", 0.0)
    for n, ref_sq in zip(names, g["grad_sqnorm_all"]):
        got_sq = eng.grad_of(n).double().pow(2).sum().item()
        if ref_sq < 0:
            assert got_sq == 0.0, n
            continue
        err = abs(got_sq ** 0.5 - ref_sq ** 0.5) / max(ref_sq ** 0.5, 1e-12)
        print(f"b2_droppath grad {n}: {err:.3e}")
        assert err < TE.GRAD_TOL, (n, err)
        worst = max(worst, (n, err), key=lambda x: x[1])
    print(f"b2_droppath: worst gradient norm error {worst}")
    _bar("b2_droppath.grad_norm_worst", worst[1], TE.GRAD_TOL)
    coef = min(1.0, 1.0 / (float(g["clip_total_norm"]) + 1e-6))
    for key in g.files:
        if key.startswith("grad_head."):
            gr = eng.grad_of(key[10:]) * coef
            e = rel_l2(gr.reshape(-1, gr.shape[-1])[:4, :32].float().cpu().numpy(), g[key])
            assert e < 2 * TE.GRAD_TOL, (key, e)
    # dropped-branch identity on the same forward: sample 1 is dropped at both encoder-layer-1 sites, so its encoder output rows are
    # the encoder_norm of its own block-0 output, bit for bit (R + 0 leaves R's value)
    assert not g["keep.encoder"][1, :, 1].any()
    x1 = eng.enc[1]["x"][N:2 * N].clone()
    y = torch.empty(N, eng.D, device=DEV, dtype=torch.bfloat16)
    st = torch.empty(2, N, device=DEV)
    ops.layernorm_fwd(x1, eng.p["encoder_norm.weight"], y, st[0], st[1], eps=cfg.eps, width=eng.Dl)
    assert torch.equal(eng.xe[N:2 * N].view(torch.int16), y.view(torch.int16))
    assert torch.equal(eng.x_enc_out[N:2 * N] + 0.0, x1 + 0.0)
    # ... and a sample kept at both sites is not (the branch is there)
    assert g["keep.encoder"][1, :, 0].all() and not torch.equal(eng.x_enc_out[:N], eng.enc[1]["x"][:N])


# ---------------------------------------------------------------------------------------------- 3. all sites dropped
def _all_dropped_grads(model, cfg):
    """forward + backward of one clip with every active site dropped (non-shared rates on 2 + 2 layers: the sites of layer 1 of either
    stack): {name: gradient} and the loss"""
    eng = model.engine
    assert sorted({n.rsplit(".", 1)[0] for n, _ in eng.dp_sites}) == ["decoder.1", "encoder.1"]
    md = _one_clip(cfg)
    model.train()
    random.seed(3)
    eng.zero_grad()
    eng.inject_drop_path(torch.zeros(2, 2, 1, dtype=torch.bool), torch.zeros(2, 3, 1, dtype=torch.bool))
    loss, _ = model(md, 256, 320)
    loss.backward()
    torch.cuda.synchronize()
    assert not bool(eng.drop_path_table().any())
    return float(loss.item()), {n: p.grad for n, p in model.named_parameters()}


def _check_all_dropped(loss, grads):
    assert np.isfinite(loss)
    dead = [n for n in grads if n.startswith(("encoder.1.", "decoder.1."))]
    live = [n for n in grads if n.startswith(("encoder.0.", "decoder.0.", "encoder_embeddings.", "encoder_norm.", "decoder_norm.",
                                               "decoder_proj_context."))]
    assert dead and live
    for n in dead:                        # a dropped branch's upstream gradient is exactly 0, and everything inside is linear in it
        assert not bool(grads[n].any()), n
    for n in live:
        assert bool(grads[n].any()) and bool(torch.isfinite(grads[n]).all()), n


def test_all_sites_dropped_gives_exactly_zero_gradients_inside_the_branches():
    g, meta, cfg, sd, md = _case()
    model = _model(drop_path_rate_encoder=0.2, drop_path_rate_decoder=0.4)
    model.load_state_dict(sd)
    loss, grads = _all_dropped_grads(model, cfg)
    _check_all_dropped(loss, grads)
    # the dropped layers are identities of the residual stream
    eng = model.engine
    assert torch.equal(eng.x_enc_out[:256] + 0.0, eng.enc[1]["x"][:256] + 0.0) and torch.equal(eng.y_out[:320] + 0.0, eng.dec[1]["x"][:320] + 0.0)


# ---------------------------------------------------------------------------------------------- 4. mode switching
def _loss(model, md, meta, grad):
    random.seed(meta["py_seed"])
    model.engine.weights_dirty = True
    if grad:
        return float(model(md, meta["n_enc"], meta["n_dec"])[0].item())
    with torch.no_grad():
        return float(model(md, meta["n_enc"], meta["n_dec"])[0].item())


def test_drop_path_is_inactive_outside_training():
    model, plain = _dp_model(), _plain_model()
    g, meta, cfg, sd, md = _case()
    try:
        plain.train()
        ref = _loss(plain, md, meta, grad=True)
        model.eval()
        assert _loss(model, md, meta, grad=True) == ref          # eval mode, grad mode on
        assert _loss(model, md, meta, grad=False) == ref
        model.train()
        assert _loss(model, md, meta, grad=False) == ref         # train mode under no_grad: no backward can follow, nothing dropped
        for m in (model, plain):
            random.seed(meta["py_seed"])
            m._lg = m(md, meta["n_enc"], meta["n_dec"], return_logits=True)
        for k in MODS:
            assert torch.equal(model._lg[k], plain._lg[k]), k
        # training with every sample kept is NOT the model without drop path: the branches are divided by keep_prob
        model.engine.inject_drop_path(torch.ones(2, 2, 4, dtype=torch.bool), torch.ones(2, 3, 4, dtype=torch.bool))
        kept = _loss(model, md, meta, grad=True)
        assert bool(model.engine.drop_path_table().all()) and kept != ref
        # a direct engine caller keeps today's behaviour by default
        random.seed(meta["py_seed"])
        order = [str(x) for x in g["dec_order"]]
        l_eng = float(model.engine.forward(md, dec_order=order)[0].item())
        assert l_eng == ref and model.engine.drop_path_table() is None
    finally:
        model.train()
        del model._lg, plain._lg


def test_generation_ignores_drop_path():
    cfg = MODEL_CFGS["ego_gen_384_2e_2d"]
    cfg_dp = dataclasses.replace(cfg, drop_path_rate_encoder=0.3, drop_path_rate_decoder=0.3, shared_drop_path=True)
    sd = synth.build_state_dict(cfg, 4)
    sample = {"tok_rgb": {"tensor": synth.randint("gg.rgb", (1, 5, 32, 32), 64000, seed=1).to(DEV)}}
    sample = init_empty_target_modality(sample, MODALITY_INFO, "tok_depth", 1, 5120, DEV)
    sample = init_full_input_modality(sample, MODALITY_INFO, "tok_rgb", DEV)
    sch = build_chained_generation_schedules(["tok_rgb"], ["tok_depth"], [5120], ["roar"], [3], ["linear"], [0.01], ["constant"],
                                             [2.0], ["constant"], cfg_grow_conditioning=True)
    out = []
    for c in (cfg, cfg_dp):
        eng = Engine(c, "cuda:0", max_batch=1, n_enc=64, n_dec=64)
        eng.load_state_dict(sd)
        assert bool(eng.dp_sites) == (c is cfg_dp)
        out.append(GenerationSampler(eng, use_graphs=False).generate(sample, sch, top_p=0.8, seed=3)["tok_depth"]["tensor"])
    assert torch.equal(out[0], out[1])


# ---------------------------------------------------------------------------------------------- 5. the device draw in the loop
def test_device_draws_are_reproducible_and_match_the_host_restatement():
    model = _dp_model()
    g, meta, cfg, sd, md = _case()
    eng = model.engine
    kps = [kp for _, kp in eng.dp_sites]
    B = meta["batch"]
    model.train()

    def step():
        random.seed(meta["py_seed"])
        eng.zero_grad()
        loss, _ = model(md, meta["n_enc"], meta["n_dec"])
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), eng.G.clone(), eng.drop_path_table().cpu().tolist(), eng.dp_last

    eng.set_drop_path_seed(77, counter=3)
    l1, G1, t1, used1 = step()
    l_next, G_next, t_next, used_next = step()                # the counter advanced: micro-batches of one step differ
    eng.set_drop_path_seed(77, counter=3)
    l2, G2, t2, used2 = step()
    assert used1 == used2 == (77, 3) and used_next == (77, 4)
    assert t1 == t2 == R.draw(kps, B, 77, 3) and t_next == R.draw(kps, B, 77, 4) and t_next != t1
    assert torch.equal(l1, l2) and torch.equal(G1, G2) and bool(G1.any()) and bool(torch.isfinite(G1).all())
    assert not torch.equal(G1, G_next)
    # ranks seed with seed + rank: another stream
    eng.set_drop_path_seed(78, counter=3)
    assert step()[2] == R.draw(kps, B, 78, 3) != t1
    # a smaller batch draws the same decisions for the samples it has
    md2 = {k: {kk: vv[:2].contiguous() for kk, vv in v.items()} for k, v in md.items()}
    eng.set_drop_path_seed(77, counter=3)
    random.seed(meta["py_seed"])
    model(md2, meta["n_enc"], meta["n_dec"])
    assert eng.drop_path_table().cpu().tolist() == [row[:2] for row in t1]


# ---------------------------------------------------------------------------------------------- 6. combinations
def test_drop_path_with_qk_norm():
    cfg = MODEL_CFGS["ego_384_2e_2d_qknorm"]
    model = _model(qk_norm=True, drop_path_rate_encoder=0.2, drop_path_rate_decoder=0.4)
    model.load_state_dict(synth.build_state_dict(cfg, 6))
    loss, grads = _all_dropped_grads(model, cfg)
    _check_all_dropped(loss, grads)
    assert any("q_norm" in n for n in grads if n.startswith("decoder.1.")) and bool(grads["decoder.0.cross_attn.k_norm.weight"].any())
    # and a drawn forward + backward is finite
    model.engine.set_drop_path_seed(1)
    model.engine.zero_grad()
    l, _ = model(_one_clip(cfg), 256, 320)
    l.backward()
    assert np.isfinite(l.item()) and bool(torch.isfinite(model.engine.G).all())


def test_drop_path_with_the_gelu_biased_family():
    """the branch's bias is scaled (and dropped) with the branch: `drop_path(proj(x) + bias)`"""
    cfg = MODEL_CFGS["ego_384_2e_2d_gelu"]
    model = _model(GELU_NAME, drop_path_rate_encoder=0.2, drop_path_rate_decoder=0.4)
    model.load_state_dict(synth.build_state_dict(cfg, 6))                  # (non-zero biases)
    loss, grads = _all_dropped_grads(model, cfg)
    _check_all_dropped(loss, grads)
    for n in ("encoder.1.attn.proj.bias", "encoder.1.mlp.fc2.bias", "decoder.1.cross_attn.proj.bias", "decoder.1.norm1.bias"):
        assert n in grads and not bool(grads[n].any()), n                   # a dropped branch's bias gets no gradient either
    eng = model.engine
    # with the bias outside the drop the stream would move by bf16(bias) at a dropped site: it does not move at all
    assert torch.equal(eng.x_enc_out[:256] + 0.0, eng.enc[1]["x"][:256] + 0.0)
    # every sample kept: the bias is divided by keep_prob with the branch - not the plain model's x + proj + bias
    md = _one_clip(cfg)
    plain = _model(GELU_NAME)
    plain.load_state_dict(synth.build_state_dict(cfg, 6))
    random.seed(3)
    ref = float(plain(md, 256, 320)[0].item())
    eng.inject_drop_path(None, None)
    random.seed(3)
    kept = float(model(md, 256, 320)[0].item())
    assert np.isfinite(kept) and kept != ref


@pytest.mark.parametrize("variant", ["fp8_forward", "padded_1020", "register_tokens", "causal", "modality_subset"])
def test_drop_path_on_the_other_variants(variant):
    """the same code path under the fp8 forward (its NT GEMM has the bf16-out epilogue the dropped sites need: its dgrad uses it), on
    padded storage (dim 1020 in rows of 1024), with register tokens (rows per sample = registers + kept tokens), under the causal
    decoder mask and on a batch holding a subset of the modalities: all sites dropped -> exact zero gradients inside the branches; a
    drawn step is finite"""
    base = {"fp8_forward": "ego_384_2e_2d_droppath", "padded_1020": "ego_L_1020_2e_2d", "register_tokens": "ego_b_2e_2d_reg4",
            "causal": "ego_384_2e_2d_causal", "modality_subset": "ego_384_2e_2d_droppath"}[variant]
    cfg = dataclasses.replace(MODEL_CFGS[base], shared_drop_path=False, drop_path_rate_encoder=0.2, drop_path_rate_decoder=0.4)
    eng = Engine(cfg, "cuda:0", max_batch=1, n_enc=256, n_dec=320, fp8_forward=variant == "fp8_forward")
    eng.load_state_dict(synth.build_state_dict(cfg, 6))
    md = _one_clip(cfg)
    if variant == "modality_subset":
        md = {k: v for k, v in md.items() if k in ("tok_rgb", "tok_cam")}
    order = [m for m in MODS if m in md]
    eng.zero_grad()
    eng.inject_drop_path(torch.zeros(2, 2, 1, dtype=torch.bool), torch.zeros(2, 3, 1, dtype=torch.bool))
    loss, _ = eng.forward(md, dec_order=order, training=True)
    eng.backward(1.0)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item())
    for n in eng.p:
        gsum = eng.g[n].abs().sum().item()
        if n.startswith(("encoder.1.", "decoder.1.")):
            assert gsum == 0.0, n
        elif n.startswith(("encoder.0.", "decoder.0.", "encoder_norm", "decoder_norm", "decoder_proj_context")):
            assert gsum > 0.0 and np.isfinite(gsum), n
    if eng.padded:                         # pad columns of the residual stream stay zero behind a dropped and behind a kept site
        assert not bool(eng.x_enc_out[:, eng.Dl:].any()) and not bool(eng.y_out[:, eng.Dl:].any())
    eng.set_drop_path_seed(2)
    eng.zero_grad()
    loss, _ = eng.forward(md, dec_order=order, training=True)
    eng.backward(1.0)
    assert np.isfinite(loss.item()) and bool(torch.isfinite(eng.G).all())
    if eng.padded:
        assert not bool(eng.x_enc_out[:, eng.Dl:].any()) and not bool(eng.y_out[:, eng.Dl:].any())
