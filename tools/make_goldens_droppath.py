"""Fixture of stochastic depth (`drop_path_rate_encoder`, `drop_path_rate_decoder`, `shared_drop_path`: egom2p_model.py:96-98, 137-161),
from the REAL reference model.

    python tools/make_goldens_droppath.py

Runs where the reference checkout is (EGOM2P_REFERENCE, see oracle/make_goldens.py).  The reference model is built with the SwiGLU
registrations' arguments plus drop_path_rate_encoder = drop_path_rate_decoder = 0.3 under shared_drop_path=True at dim 384, 6 heads,
2 + 2 layers: per-layer rates 0, 0.1 | 0.2, 0.3 (fp32 linspace values) - encoder layer 0 holds nn.Identity, the other three layers give
8 active sites at three keep probabilities.

`oracle.make_goldens.run_case` runs the model twice (staged, then end to end) and asserts equal losses, and torch's Philox stream is
not what the engine draws from: the loaded reference module's `DropPath.forward` is replaced, IN THIS TOOL ONLY, by one that performs
the reference's own arithmetic (`x.div(keep_prob) * random_tensor`, egom2p_utils.py:95-99) with `random_tensor` read from a fixed
table.  The table is chosen by hand: every active site has a kept and a dropped sample, sample 1 (the padded one) is dropped at both
encoder-layer-1 sites, sample 2 is dropped at decoder.0.cross_attn and kept at the two sites around it.

  b2_droppath   B = 4, N = 256, M = 320: samples 0 / 1 carry b2_causal's budgets (the second with 97 padding rows and a one-row group),
                samples 2 / 3 two more (the last padded on both sides, no camera input); run_case's format plus `keep.encoder` [2, 2, 4],
                `keep.decoder` [2, 3, 4] and the exact per-layer rates in `meta`.  Weights and clips come from `egom2p_amd.synth`: data only.
"""
from __future__ import annotations

import argparse
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from oracle import make_goldens as MG             # noqa: E402
from egom2p_amd.config import MODEL_CFGS          # noqa: E402

CFG = "ego_384_2e_2d_droppath"
BUDGETS = {"tok_rgb": [(140, 200), (100, 150), (120, 160), (90, 100)], "tok_depth": [(100, 90), (80, 60), (110, 130), (130, 170)],
           "tok_cam": [(10, 20), (8, 1), (14, 16), (0, 25)], "tok_gaze": [(6, 10), (0, 12), (12, 14), (20, 5)]}
T, F = True, False
# [layer, site, sample]; encoder sites (attn, mlp), decoder sites (self_attn, cross_attn, mlp).  Encoder layer 0 has rate 0: ignored.
KEEP_ENC = [[[T, T, T, T], [T, T, T, T]],
            [[T, F, T, F], [T, F, F, T]]]
KEEP_DEC = [[[F, T, T, T], [T, T, F, T], [T, T, T, F]],
            [[T, F, T, T], [F, T, T, F], [T, T, F, T]]]


def table_forward(self, x):
    """DropPath.forward with the reference's arithmetic (egom2p_utils.py:93-100) and `random_tensor` from the module's table: a block
    calls its one DropPath module once per residual site, in site order"""
    if self.drop_prob == 0. or not self.training:
        return x
    keep_prob = 1 - self.drop_prob
    shape = (x.shape[0],) + (1,) * (x.ndim - 1)
    row = self.keep_rows[self.calls % len(self.keep_rows)]
    self.calls += 1
    random_tensor = row.to(x.dtype).view(shape)
    return x.div(keep_prob) * random_tensor


def build_reference_model(cfg, enc, dec, model):
    """oracle.make_goldens.build_reference_model with the configuration's drop-path keywords, every DropPath carrying its keep rows"""
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
    net = model.EgoM2P(
        encoder_embeddings=e_emb, decoder_embeddings=d_emb, modality_info=info,
        dim=cfg.dim, encoder_depth=cfg.encoder_depth, decoder_depth=cfg.decoder_depth,
        num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, qkv_bias=False, proj_bias=False, mlp_bias=False,
        norm_layer=partial(model.LayerNorm, eps=1e-6, bias=False), act_layer=torch.nn.SiLU, gated_mlp=True,
        drop_path_rate_encoder=cfg.drop_path_rate_encoder, drop_path_rate_decoder=cfg.drop_path_rate_decoder,
        shared_drop_path=cfg.shared_drop_path)
    utils = sys.modules["egom2p.models.egom2p_utils"]
    utils.DropPath.forward = table_forward
    for blocks, keep in ((net.encoder, KEEP_ENC), (net.decoder, KEEP_DEC)):
        for blk, rows in zip(blocks, keep):
            if isinstance(blk.drop_path, utils.DropPath):
                blk.drop_path.keep_rows, blk.drop_path.calls = torch.tensor(rows), 0
    build_reference_model.rates = ([float(getattr(b.drop_path, "drop_prob", 0.0)) for b in net.encoder],
                                   [float(getattr(b.drop_path, "drop_prob", 0.0)) for b in net.decoder])
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    MG.build_reference_model = build_reference_model
    enc, dec, model = MG.load_reference()
    torch.set_num_threads(8)
    MG.run_case("b2_droppath", cfg_name=CFG, batch=4, n_enc=256, n_dec=320, budgets=BUDGETS, seed=47, full_float=False,
                py_seed=37, out_dir=args.out, enc=enc, dec=dec, model=model)
    path = os.path.join(args.out, "b2_droppath.npz")
    with np.load(path, allow_pickle=False) as z:
        gold = {k: z[k] for k in z.files}
    r_enc, r_dec = build_reference_model.rates
    assert MODEL_CFGS[CFG].shared_drop_path and r_enc[0] == 0.0 and all(r > 0 for r in r_enc[1:] + r_dec)
    meta = eval(str(gold["meta"]))
    meta.update(drop_path_rate_encoder=MODEL_CFGS[CFG].drop_path_rate_encoder, drop_path_rate_decoder=MODEL_CFGS[CFG].drop_path_rate_decoder,
                shared_drop_path=True, rates_encoder=[repr(r) for r in r_enc], rates_decoder=[repr(r) for r in r_dec])
    gold["meta"] = np.array(repr(meta))
    gold["keep.encoder"], gold["keep.decoder"] = np.array(KEEP_ENC, dtype=np.bool_), np.array(KEEP_DEC, dtype=np.bool_)
    np.savez_compressed(path, **gold)
    print(f"[goldens] b2_droppath: rates {r_enc} | {r_dec} -> {path} ({os.path.getsize(path) / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
