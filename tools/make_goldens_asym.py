"""Fixtures of the asymmetric / no-separation / unshared variants, from the REAL reference model.

    python tools/make_goldens_asym.py [--only b2_asym,b2_nosep,b2_unshared]

Runs where the reference checkout is (EGOM2P_REFERENCE, see oracle/make_goldens.py, whose loader this tool uses) and follows that
file's recipe: seeded weights and clips from `egom2p_amd.synth` (the fixtures hold no weights), the body of EgoM2P.forward
(egom2p_model.py:706-734) stage by stage with the integer outputs recorded in full, the dense decoder mask bit-packed, float taps as
slices + row norms, one squared norm per gradient tensor.  dim 384, 6 heads, 2 + 2 layers, modalities rgb / depth / cam, B = 2,
N = 192, M = 200 (padding rows on both sides):

  b2_asym      encoder {rgb, cam}, decoder {depth, cam}: depth's decoder mod_emb is a parameter of its own
  b2_nosep     decoder_sep_mask=False with three decoder modalities: the cumsum staircase runs across the modalities
  b2_unshared  share_modality_embeddings=False; the decoder mod_emb are drawn apart from the encoder's (`dec_mod_emb` below)

`meta["param_names"]` is the reference model's named_parameters() name list, `meta["state_keys"]` its state_dict() key list.
"""
from __future__ import annotations

import argparse
import os
import random
import sys
from dataclasses import replace
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egom2p_amd import synth                      # noqa: E402
from egom2p_amd.config import ModelCfg            # noqa: E402

BASE = ModelCfg("asym_base", 384, 2, 2, 6, modalities=("tok_rgb", "tok_depth", "tok_cam"))
CFGS = {
    "b2_asym": replace(BASE, encoder_modalities=("tok_rgb", "tok_cam"), decoder_modalities=("tok_depth", "tok_cam")),
    "b2_nosep": replace(BASE, decoder_sep_mask=False),
    "b2_unshared": replace(BASE, share_modality_embeddings=False),
}
BUDGETS = {"tok_rgb": [(80, 70), (60, 50)], "tok_depth": [(50, 90), (70, 60)], "tok_cam": [(12, 10), (15, 8)]}
B, N_ENC, N_DEC, SEED = 2, 192, 200, 4
PY_SEED = {"b2_asym": 41, "b2_nosep": 42, "b2_unshared": 43}
TAPS = ("enc_x0", "enc_out", "context", "dec_y0", "dec_out")


def dec_mod_emb(name: str, dim: int) -> torch.Tensor:
    """the decoder's own mod_emb of an unshared model (tests draw the same)"""
    return synth.normal(f"decoder_embeddings.{name}.mod_emb.own", (1, 1, dim), 0.02, SEED)


def state_dict_for(cfg) -> dict:
    sd = synth.build_state_dict(cfg, SEED)
    if not cfg.share_modality_embeddings:
        for m in cfg.dec_mods:
            sd[f"decoder_embeddings.{m.name}.mod_emb"] = dec_mod_emb(m.name, cfg.dim)
    return sd


def build_reference_model(cfg, enc, dec, model):
    info, e_emb, d_emb = {}, {}, {}
    for m in cfg.mods:
        info[m.name] = {"vocab_size": m.vocab_size, "max_tokens": m.max_tokens, "type": m.type, "id": m.id}
    for m in cfg.enc_mods:
        e_emb[m.name] = (enc.VideoTokenEncoderEmbedding(vocab_size=m.vocab_size, patch_size=(4, 8, 8), image_size=256) if m.kind == "video"
                         else enc.GazeCamTokenEncoderEmbedding(vocab_size=m.vocab_size))
    for m in cfg.dec_mods:
        d_emb[m.name] = (dec.VideoTokenDecoderEmbedding(vocab_size=m.vocab_size, patch_size=(4, 8, 8), image_size=256, share_embedding=True)
                         if m.kind == "video" else dec.GazeCamTokenDecoderEmbedding(vocab_size=m.vocab_size, share_embedding=True))
    return model.EgoM2P(
        encoder_embeddings=e_emb, decoder_embeddings=d_emb, modality_info=info, dim=cfg.dim, encoder_depth=cfg.encoder_depth,
        decoder_depth=cfg.decoder_depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, qkv_bias=False, proj_bias=False, mlp_bias=False,
        norm_layer=partial(model.LayerNorm, eps=1e-6, bias=False), act_layer=torch.nn.SiLU, gated_mlp=True,
        decoder_sep_mask=cfg.decoder_sep_mask, share_modality_embeddings=cfg.share_modality_embeddings)


def run_case(case, out_dir, enc, dec, model):
    cfg = CFGS[case]
    torch.manual_seed(0)
    net = build_reference_model(cfg, enc, dec, model)
    sd = state_dict_for(cfg)
    keys = list(net.state_dict().keys())
    net.load_state_dict({k: sd[k] for k in keys}, strict=True)
    net.train()
    mod_dict = synth.make_clip_batch(cfg, B, BUDGETS, SEED)

    def fresh():
        return {k: {kk: vv.clone() for kk, vv in v.items()} for k, v in mod_dict.items()}

    gold = {}
    random.seed(PY_SEED[case])
    md = fresh()
    enc_md = {mod: net.encoder_embeddings[mod](d) for mod, d in md.items() if mod in net.encoder_embeddings}
    captured, real_argsort = [], torch.argsort

    def spy(*a, **k):
        r = real_argsort(*a, **k)
        captured.append(r)
        return r

    torch.argsort = spy
    try:
        enc_tok, enc_emb, enc_mask, enc_mod = net.forward_mask_encoder(enc_md, N_ENC)
        dec_md = {mod: net.decoder_embeddings[mod].forward_embed(d) for mod, d in md.items() if mod in net.decoder_embeddings}
        st = random.getstate()
        order = [mod for mod, _ in random.sample(list(dec_md.items()), len(dec_md))]       # the draw of cat_decoder_tensors (:312)
        random.setstate(st)
        dec_tok, dec_emb, dec_mask, tgt_ids, dec_attn, dec_mod = net.forward_mask_decoder(dec_md, N_DEC)
    finally:
        torch.argsort = real_argsort
    gold["dec_order"] = np.array(order)
    gold["enc_ids_keep"] = captured[0][:, :N_ENC].numpy()
    gold["dec_ids_keep"] = captured[1][:, :N_DEC].numpy()
    gold["enc_pad"], gold["enc_mod_mask"] = enc_mask[:, 0].numpy(), enc_mod.numpy()
    gold["dec_pad"], gold["dec_mod_mask"] = dec_mask[:, 0].numpy(), dec_mod.numpy()
    gold["target_ids"] = tgt_ids.numpy()
    gold["dec_attn_mask_packed"] = np.packbits(dec_attn.numpy(), axis=-1)

    x = enc_tok + enc_emb
    taps = {"enc_x0": x}
    for blk in net.encoder:
        x = blk(x, mask=enc_mask)
    x = net.encoder_norm(x)
    taps["enc_out"] = x
    ctx = net.decoder_proj_context(x) + enc_emb
    taps["context"] = ctx
    y = dec_tok + dec_emb
    taps["dec_y0"] = y
    for blk in net.decoder:
        y = blk(y, ctx, sa_mask=dec_attn, xa_mask=enc_mask)
    y = net.decoder_norm(y)
    taps["dec_out"] = y
    loss_staged, _ = net.forward_loss(y, tgt_ids, dec_md, dec_mod, "mod")

    random.seed(PY_SEED[case])
    loss, mod_loss = net(fresh(), N_ENC, N_DEC, "mod")
    assert torch.equal(loss, loss_staged), (loss, loss_staged)
    gold["loss"] = np.array(loss.item(), dtype=np.float64)
    for mod, v in mod_loss.items():
        gold[f"mod_loss.{mod}"] = np.array(v.item(), dtype=np.float64)
    for k in TAPS:
        v = taps[k].detach()
        gold[f"tap_head.{k}"] = v[:, :6, :24].numpy().copy()
        gold[f"tap_rownorm.{k}"] = v.double().norm(dim=-1).numpy().astype(np.float32)

    net.zero_grad()
    loss.backward()
    named = dict(net.named_parameters())
    gold["grad_names"] = np.array(list(named.keys()))
    gold["grad_sqnorm_all"] = np.array([named[n].grad.double().pow(2).sum().item() if named[n].grad is not None else -1.0 for n in named])
    gold["grad_total_norm"] = np.array(sum(v for v in gold["grad_sqnorm_all"] if v > 0) ** 0.5)
    for n in named:
        if n.endswith("mod_emb") and named[n].grad is not None:
            gold[f"grad.{n}"] = named[n].grad.numpy().copy()
    meta = dict(case=case, batch=B, n_enc=N_ENC, n_dec=N_DEC, seed=SEED, py_seed=PY_SEED[case], budgets=repr(BUDGETS),
                param_names=list(named.keys()), state_keys=keys)
    gold["meta"] = np.array(repr(meta))
    path = os.path.join(out_dir, f"{case}.npz")
    np.savez_compressed(path, **gold)
    print(f"[goldens] {case}: loss={loss.item():.6f} order={order} -> {path} ({os.path.getsize(path) / 1e3:.0f} KB)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    from oracle import make_goldens as MG
    enc, dec, model = MG.load_reference()
    torch.set_num_threads(8)
    for case in CFGS:
        if not args.only or case in args.only.split(","):
            run_case(case, args.out, enc, dec, model)


if __name__ == "__main__":
    main()
