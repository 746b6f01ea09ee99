"""Fixture of the parameter groups of layer-wise lr decay, from the REAL reference: its `get_parameter_groups` and
`get_num_layer_for_fm` (egom2p/utils/optim_factory.py:62-154) run on its own model (egom2p_model.py) at the tiny geometry the tests
use (dim 128, 2 + 2 layers, 2 heads, tok_cam + tok_gaze).

    python tools/make_goldens_param_groups.py [--out tests/golden/param_groups.json]

Runs on the CPU where the reference checkout is (EGOM2P_REFERENCE, see oracle/make_goldens.py).  Names and numbers only:

  {configuration: {"model": the constructor switches that differ from the swiglu / nobias family,
                   "frozen": names set requires_grad=False before the groups are built,
                   "variants": {variant: {"args": {layer_decay, decoder_decay, no_lr_scale_list},
                                          "params": {parameter name: [group name, lr_scale, weight_decay]}}}}}

Configurations: swiglu_nobias, gelu (the biased GELU family), qknorm, registers (4 register tokens), unshared_mod_emb
(share_modality_embeddings=False) and frozen (swiglu_nobias after freeze_encoder(): the frozen tensors are in no group).
Variants: `ld` (layer_decay 0.75) and `ld_dd` (the same with decoder_decay 0.01 and two names in no_lr_scale_list).
The layer scales are layer_decay ** (L + 1 - i), i = 0 .. L + 1, L = 4; weight_decay 0.05.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
from functools import partial

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from oracle import make_goldens as MG             # noqa: E402

MODS = ("tok_cam", "tok_gaze")
DIM, ENC, DEC, HEADS = 128, 2, 2, 2
WEIGHT_DECAY, LAYER_DECAY, DECODER_DECAY = 0.05, 0.75, 0.01
NO_LR_SCALE = "encoder.0.attn.qkv.weight-decoder_norm.weight"
CONFIGS = {
    "swiglu_nobias": {},
    "gelu": {"gelu": True},
    "qknorm": {"qk_norm": True},
    "registers": {"num_register_tokens": 4},
    "unshared_mod_emb": {"share_modality_embeddings": False},
    "frozen": {"freeze": "encoder"},
}
VARIANTS = {
    "ld": {"layer_decay": LAYER_DECAY, "decoder_decay": None, "no_lr_scale_list": ""},
    "ld_dd": {"layer_decay": LAYER_DECAY, "decoder_decay": DECODER_DECAY, "no_lr_scale_list": NO_LR_SCALE},
}


def reference_model(enc, dec, model, gelu=False, qk_norm=False, num_register_tokens=0, share_modality_embeddings=True, **_):
    from egom2p_amd.config import MODALITIES
    info, e_emb, d_emb = {}, {}, {}
    for name in MODS:
        m = MODALITIES[name]
        info[name] = {"vocab_size": m.vocab_size, "max_tokens": m.max_tokens, "type": m.type, "id": m.id}
        e_emb[name] = enc.GazeCamTokenEncoderEmbedding(vocab_size=m.vocab_size)
        d_emb[name] = dec.GazeCamTokenDecoderEmbedding(vocab_size=m.vocab_size, share_embedding=True)
    norm = partial(torch.nn.LayerNorm, eps=1e-6) if gelu else partial(model.LayerNorm, eps=1e-6, bias=False)
    return model.EgoM2P(encoder_embeddings=e_emb, decoder_embeddings=d_emb, modality_info=info, dim=DIM, encoder_depth=ENC,
                        decoder_depth=DEC, num_heads=HEADS, mlp_ratio=4.0, qkv_bias=gelu, proj_bias=gelu, mlp_bias=gelu,
                        norm_layer=norm, act_layer=torch.nn.GELU if gelu else torch.nn.SiLU, gated_mlp=not gelu, qk_norm=qk_norm,
                        num_register_tokens=num_register_tokens, share_modality_embeddings=share_modality_embeddings)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "param_groups.json"))
    args = ap.parse_args()
    enc, dec, model = MG.load_reference()
    spec = importlib.util.spec_from_file_location("egom2p.utils.optim_factory", os.path.join(MG.REF, "egom2p/utils/optim_factory.py"))
    OF = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(OF)
    out = {}
    for cname, switches in CONFIGS.items():
        net = reference_model(enc, dec, model, **switches)
        if switches.get("freeze") == "encoder":
            net.freeze_encoder()
        frozen = [n for n, p in net.named_parameters() if not p.requires_grad]
        entry = {"model": {k: v for k, v in switches.items() if k != "freeze"}, "frozen": frozen, "variants": {}}
        for vname, v in VARIANTS.items():
            scales = [v["layer_decay"] ** (ENC + DEC + 1 - i) for i in range(ENC + DEC + 2)]
            layer_fn = partial(OF.get_num_layer_for_fm, num_enc_layers=ENC, num_dec_layers=DEC)
            # the group names and the tensors' names live in a local of the reference's function (`parameter_group_names`, the
            # dict its commented-out print would show): read it from the frame when the function returns
            caught = {}

            def on_return(frame, event, arg, _caught=caught):
                if event == "return" and frame.f_code.co_name == "get_parameter_groups":
                    _caught["names"] = frame.f_locals["parameter_group_names"]

            sys.setprofile(on_return)
            try:
                groups = OF.get_parameter_groups(net, WEIGHT_DECAY, (), layer_fn, OF.LayerDecayValueAssigner(scales).get_scale,
                                                 v["decoder_decay"], (), v["no_lr_scale_list"].split("-"))
            finally:
                sys.setprofile(None)
            assert len(groups) == len(caught["names"])
            params = {}
            for (gname, g), ret in zip(caught["names"].items(), groups):
                assert len(g["params"]) == len(ret["params"]) and g["lr_scale"] == ret["lr_scale"] and g["weight_decay"] == ret["weight_decay"]
                for n in g["params"]:
                    params[n] = [gname, float(g["lr_scale"]), float(g["weight_decay"])]
            entry["variants"][vname] = {"args": v, "params": params}
        out[cname] = entry
        print(f"[goldens] {cname}: {len(frozen)} frozen, " +
              ", ".join(f"{k}: {len(e['params'])} tensors in {len({p[0] for p in e['params'].values()})} groups" for k, e in entry["variants"].items()))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"[goldens] -> {args.out} ({os.path.getsize(args.out) / 1e3:.1f} KB)")


if __name__ == "__main__":
    main()
