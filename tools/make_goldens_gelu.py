"""Fixtures of the GELU / biased family (the `*_gelu` registrations, egom2p_model.py:881-978), from the REAL reference model.

    python tools/make_goldens_gelu.py [--only b2_gelu|gen_rgb2depth_gelu]

Runs where the reference checkout is (EGOM2P_REFERENCE, see oracle/make_goldens.py).  The reference model is built with the
registrations' own arguments - `qkv_bias` / `proj_bias` / `mlp_bias` True, the plain Mlp under nn.GELU, `nn.LayerNorm` with its
bias - and takes its weights and clips from `egom2p_amd.synth` (seeded: every linear bias and every LayerNorm bias is drawn
NON-zero, so a bias that is loaded but not applied shows), so the fixtures hold no weights.

  b2_gelu             `oracle.make_goldens.run_case`: dim 384, 6 heads, 2 + 2 layers, B = 2, N = 256, M = 320, the budgets of b2_causal
                      (a ragged second sample with 97 padding rows, a one-row group) - integer outputs in full, float taps as slices +
                      row norms, one squared norm per gradient tensor (biases and LayerNorm biases included).
  gen_rgb2depth_gelu  `oracle/make_goldens_generate.py` (its `gen_rgb2depth` task: rgb -> depth, ROAR, 3 steps, CFG 2.0, T 0.01, top-p
                      0.8) run on the same small model with the biased GELU arguments.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from oracle import make_goldens as MG             # noqa: E402
from egom2p_amd.config import MODEL_CFGS          # noqa: E402

CFG = "ego_384_2e_2d_gelu"
GEN_CFG = "ego_gen_384_2e_2d_gelu"
# (tools/make_goldens_variants.py: b2_causal's budgets)
BUDGETS = {"tok_rgb": [(140, 200), (100, 150)], "tok_depth": [(100, 90), (80, 60)],
           "tok_cam": [(10, 20), (8, 1)], "tok_gaze": [(6, 10), (0, 12)]}


def build_reference_model(cfg, enc, dec, model):
    """oracle.make_goldens.build_reference_model with the configuration's MLP kind, bias flags and LayerNorm"""
    info, e_emb, d_emb = {}, {}, {}
    for m in cfg.mods:
        info[m.name] = {"vocab_size": m.vocab_size, "max_tokens": m.max_tokens, "type": m.type, "id": m.id}
        if m.kind == "video":
            e_emb[m.name] = enc.VideoTokenEncoderEmbedding(vocab_size=m.vocab_size, patch_size=(4, 8, 8), image_size=256)
            d_emb[m.name] = dec.VideoTokenDecoderEmbedding(vocab_size=m.vocab_size, patch_size=(4, 8, 8), image_size=256,
                                                           share_embedding=cfg.share_embedding)
        else:
            e_emb[m.name] = enc.GazeCamTokenEncoderEmbedding(vocab_size=m.vocab_size)
            d_emb[m.name] = dec.GazeCamTokenDecoderEmbedding(vocab_size=m.vocab_size, share_embedding=cfg.share_embedding)
    gelu = cfg.mlp == "gelu"
    norm = partial(torch.nn.LayerNorm, eps=1e-6) if cfg.norm_bias else partial(model.LayerNorm, eps=1e-6, bias=False)
    return model.EgoM2P(
        encoder_embeddings=e_emb, decoder_embeddings=d_emb, modality_info=info,
        dim=cfg.dim, encoder_depth=cfg.encoder_depth, decoder_depth=cfg.decoder_depth,
        num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, qkv_bias=cfg.qkv_bias, proj_bias=cfg.proj_bias, mlp_bias=cfg.mlp_bias,
        norm_layer=norm, act_layer=torch.nn.GELU if gelu else torch.nn.SiLU, gated_mlp=not gelu,
        num_register_tokens=cfg.num_register_tokens, decoder_causal_mask=cfg.decoder_causal_mask)


def make_b2(out_dir):
    enc, dec, model = MG.load_reference()
    torch.set_num_threads(8)
    MG.run_case("b2_gelu", cfg_name=CFG, batch=2, n_enc=256, n_dec=320, budgets=BUDGETS, seed=41, full_float=False,
                py_seed=33, out_dir=out_dir, enc=enc, dec=dec, model=model)


def make_gen(out_dir):
    """oracle/make_goldens_generate.py's `gen_rgb2depth` task, its small model swapped for the biased GELU configuration of the same
    shape; the tool writes beside its ROOT, which points at a scratch directory here (the existing fixture is not touched)."""
    import make_goldens_generate as MGG
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "tests", "golden"))
        MGG.MG.build_reference_model = build_reference_model      # (its own import of oracle/make_goldens.py)
        saved = (MGG.ROOT, MGG.MODEL_CFGS, sys.argv)
        MGG.ROOT, MGG.MODEL_CFGS, sys.argv = tmp, {**MODEL_CFGS, "ego_gen_384_2e_2d": MODEL_CFGS[GEN_CFG]}, [sys.argv[0], "gen_rgb2depth"]
        try:
            MGG.main()
        finally:
            MGG.ROOT, MGG.MODEL_CFGS, sys.argv = saved
            torch.set_grad_enabled(True)
        with np.load(os.path.join(tmp, "tests", "golden", "gen_rgb2depth.npz"), allow_pickle=False) as z:
            gold = {k: z[k] for k in z.files}
    meta = eval(str(gold["meta"]))
    meta["cfg"] = GEN_CFG
    gold["meta"] = np.array(repr(meta))
    path = os.path.join(out_dir, "gen_rgb2depth_gelu.npz")
    np.savez_compressed(path, **gold)
    print(f"[goldens] -> {path} ({os.path.getsize(path) / 1e6:.2f} MB)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    MG.build_reference_model = build_reference_model
    only = args.only.split(",") if args.only else ("b2_gelu", "gen_rgb2depth_gelu")
    if "b2_gelu" in only:
        make_b2(args.out)
    if "gen_rgb2depth_gelu" in only:
        make_gen(args.out)


if __name__ == "__main__":
    main()
