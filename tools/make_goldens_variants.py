"""Fixtures of the causal decoder variant and of a modality-subset batch, from the REAL reference model.

    python tools/make_goldens_variants.py [--only b2_causal|b2_subset]

Runs where the reference checkout is (EGOM2P_REFERENCE, see oracle/make_goldens.py, whose loader and `run_case` this tool
uses: the fixtures have the layout of the other `b2*` cases - integer outputs in full, the dense decoder mask bit-packed,
float taps as slices + row norms, one squared norm per gradient tensor).  Weights and clips come from `egom2p_amd.synth`
(seeded), so the fixtures hold no weights.

  b2_causal  dim 384, 6 heads, 2 + 2 layers, `decoder_causal_mask=True` (the registered variant's flag, egom2p_model.py:1029-1051),
             B = 2, N = 256, M = 320.  Sample 0 is fully valid with targets rgb 200 / depth 90 / cam 20 / gaze 10 (the rgb group
             spans two 128-row query tiles and four 64-key tiles whatever the shuffled order); sample 1 has 223 targets (97
             padding rows) and a one-row group (cam), and 188 of 256 encoder rows.
  b2_subset  the same model, weights and clips with only tok_rgb and tok_cam in the batch (egom2p_model.py:706-714): 150 / 108
             valid encoder rows, 220 / 151 valid decoder rows.
"""
from __future__ import annotations

import argparse
import os
import sys
from functools import partial

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_goldens as MG             # noqa: E402

CFG = "ego_384_2e_2d_causal"
BUDGETS = {"tok_rgb": [(140, 200), (100, 150)], "tok_depth": [(100, 90), (80, 60)],
           "tok_cam": [(10, 20), (8, 1)], "tok_gaze": [(6, 10), (0, 12)]}
CASES = {
    "b2_causal": dict(present=None, py_seed=31),
    "b2_subset": dict(present=("tok_rgb", "tok_cam"), py_seed=32),
}


def build_reference_model(cfg, enc, dec, model):
    """oracle.make_goldens.build_reference_model + the configuration's decoder_causal_mask"""
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
        num_register_tokens=cfg.num_register_tokens, decoder_causal_mask=cfg.decoder_causal_mask)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    enc, dec, model = MG.load_reference()
    torch.set_num_threads(8)
    MG.build_reference_model = build_reference_model
    real_batch = MG.synth.make_clip_batch
    for case, kw in CASES.items():
        if args.only and case not in args.only.split(","):
            continue

        def batch(*a, _present=kw["present"], **k):
            md = real_batch(*a, **k)
            return md if _present is None else {n: v for n, v in md.items() if n in _present}

        MG.synth.make_clip_batch = batch
        try:
            MG.run_case(case, cfg_name=CFG, batch=2, n_enc=256, n_dec=320, budgets=BUDGETS, seed=21, full_float=False,
                        py_seed=kw["py_seed"], out_dir=args.out, enc=enc, dec=dec, model=model)
        finally:
            MG.synth.make_clip_batch = real_batch


if __name__ == "__main__":
    main()
