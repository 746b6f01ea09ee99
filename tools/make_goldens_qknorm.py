"""Fixtures of the QK-norm family (the `*_swiglu_qknorm_nobias` registrations, egom2p_model.py:1122-1196), from the REAL reference model.

    python tools/make_goldens_qknorm.py [--only b2_qknorm|gen_rgb2depth_qknorm]

Runs where the reference checkout is (EGOM2P_REFERENCE, see oracle/make_goldens.py).  The reference model is built with the
registrations' own arguments plus `qk_norm=cfg.qk_norm` - NormAttention / NormCrossAttention (egom2p_utils.py:247-332) with a bias-free
LayerNorm(head_dim, eps 1e-6) on q and k - and takes its weights and clips from `egom2p_amd.synth` (seeded: every head-norm weight is
drawn around 1 with std 0.1, so a weight that is loaded but not applied shows), so the fixtures hold no weights.

  b2_qknorm             `oracle.make_goldens.run_case`: dim 384, 6 heads, 2 + 2 layers, B = 2, N = 256, M = 320, the budgets of b2_causal /
                        b2_gelu (a ragged second sample with 97 padding rows, a one-row group) - integer outputs in full, float taps as
                        slices + row norms, one squared norm per gradient tensor (the 12 head-norm weights included).
  gen_rgb2depth_qknorm  `oracle/make_goldens_generate.py` (its `gen_rgb2depth` task: rgb -> depth, ROAR, 3 steps, CFG 2.0, T 0.01, top-p
                        0.8) run on the same small two-modality model with qk_norm.
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

CFG = "ego_384_2e_2d_qknorm"
GEN_CFG = "ego_gen_384_2e_2d_qknorm"
# (tools/make_goldens_variants.py: b2_causal's budgets)
BUDGETS = {"tok_rgb": [(140, 200), (100, 150)], "tok_depth": [(100, 90), (80, 60)],
           "tok_cam": [(10, 20), (8, 1)], "tok_gaze": [(6, 10), (0, 12)]}


def build_reference_model(cfg, enc, dec, model):
    """oracle.make_goldens.build_reference_model with the configuration's qk_norm"""
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
    return model.EgoM2P(
        encoder_embeddings=e_emb, decoder_embeddings=d_emb, modality_info=info,
        dim=cfg.dim, encoder_depth=cfg.encoder_depth, decoder_depth=cfg.decoder_depth,
        num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, qkv_bias=False, proj_bias=False, mlp_bias=False,
        norm_layer=partial(model.LayerNorm, eps=1e-6, bias=False), act_layer=torch.nn.SiLU, gated_mlp=True,
        qk_norm=cfg.qk_norm, num_register_tokens=cfg.num_register_tokens, decoder_causal_mask=cfg.decoder_causal_mask)


def make_b2(out_dir):
    enc, dec, model = MG.load_reference()
    torch.set_num_threads(8)
    MG.run_case("b2_qknorm", cfg_name=CFG, batch=2, n_enc=256, n_dec=320, budgets=BUDGETS, seed=43, full_float=False,
                py_seed=35, out_dir=out_dir, enc=enc, dec=dec, model=model)


def make_gen(out_dir):
    """oracle/make_goldens_generate.py's `gen_rgb2depth` task, its small model swapped for the qk-norm configuration of the same
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
    path = os.path.join(out_dir, "gen_rgb2depth_qknorm.npz")
    np.savez_compressed(path, **gold)
    print(f"[goldens] -> {path} ({os.path.getsize(path) / 1e6:.2f} MB)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    MG.build_reference_model = build_reference_model
    only = args.only.split(",") if args.only else ("b2_qknorm", "gen_rgb2depth_qknorm")
    if "b2_qknorm" in only:
        make_b2(args.out)
    if "gen_rgb2depth_qknorm" in only:
        make_gen(args.out)


if __name__ == "__main__":
    main()
