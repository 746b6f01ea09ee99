"""Golden draws of the REAL reference's token-budget sampler for a dataset whose input and output modalities differ.

    python tools/make_goldens_zero_alpha.py [--draws 4096]

Runs where the reference checkout is (EGOM2P_REFERENCE; the loader of oracle/make_goldens_masking.py brings in the reference's
`egom2p/data/masking.py`, and `egom2p/data/pretrain_utils.py` is loaded the same way with its dataset imports stubbed: only
`setup_sampling_mod_info`, :30-83, is called).  The dataset: in_domains tok_rgb-tok_cam, out_domains tok_depth-tok_cam, input_alphas 1.0,
target_alphas 0.5, 256 input and 256 target tokens.  The reference's own `setup_sampling_mod_info` builds the masking modality_info
(alpha 0 for depth as input and for rgb as target), its own `UnifiedMasking` floors the alphas at 1e-9 (masking.py:159-165) and draws:

    tests/golden/zero_alpha_budgets.npz
        names                      the modality_info keys in the reference's order (sorted union)
        input_alphas, target_alphas [n_mods, n_mix] as setup_sampling_mod_info set them
        k_in, k_tgt                [n_mods, draws] int16: input_token_budget / target_token_budget of every draw

The fixture is data (names, alphas and integers drawn by the reference); nothing of the reference's text is stored.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egom2p_amd.config import MODALITIES           # noqa: E402
from oracle import make_goldens_masking as MM      # noqa: E402

IN_DOMAINS, OUT_DOMAINS = "tok_rgb-tok_cam", "tok_depth-tok_cam"
N_IN = N_TGT = 256


def load_reference_pretrain_utils():
    """egom2p/data/pretrain_utils.py by path; the modules it imports for its dataloaders are empty stand-ins"""
    for name, attrs in (("egom2p.data.image_augmenter", ("CenterCropImageAugmenter", "EmptyAugmenter", "PreTokenizedImageAugmenter",
                                                         "RandomCropImageAugmenter")),
                        ("egom2p.data.unified_datasets", ("build_pretraining_dataset", "build_huggingface_pretraining_dataloader",
                                                          "build_wds_pretraining_dataloader")),
                        ("egom2p.data.modality_transforms", ("CaptionTransform",)),
                        ("egom2p.data.modality_info", ("MODALITY_TRANSFORMS",))):
        mod = sys.modules.get(name) or types.ModuleType(name)
        for a in attrs:
            if not hasattr(mod, a):
                setattr(mod, a, None)
        sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("egom2p.data.pretrain_utils", os.path.join(MM.REF, "egom2p/data/pretrain_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "zero_alpha_budgets.npz"))
    args = ap.parse_args()
    M = MM.load_reference_masking()
    PU = load_reference_pretrain_utils()
    base = {n: {"type": MODALITIES[n].type, "min_tokens": 0, "max_tokens": MODALITIES[n].max_tokens}
            for n in ("tok_rgb", "tok_depth", "tok_cam", "tok_gaze")}
    info, weights = PU.setup_sampling_mod_info(dict(in_domains=IN_DOMAINS, out_domains=OUT_DOMAINS, input_alphas="1.0", target_alphas="0.5"), base)
    assert weights is None
    names = list(info)
    torch.manual_seed(7)
    um = M.UnifiedMasking(info, MM._NoTokenizer(), N_IN, N_TGT)
    k_in = np.zeros((len(names), args.draws), np.int16)
    k_tg = np.zeros((len(names), args.draws), np.int16)
    for i in range(args.draws):
        bi = um.input_token_budget(N_IN, 0)
        k_in[:, i], k_tg[:, i] = bi, um.target_token_budget(bi, N_TGT, 0)
    gold = {"names": np.array(names), "max_tokens": np.array([info[n]["max_tokens"] for n in names]),
            "input_alphas": np.array([info[n]["input_alphas"] for n in names], np.float64),
            "target_alphas": np.array([info[n]["target_alphas"] for n in names], np.float64), "k_in": k_in, "k_tgt": k_tg,
            "meta": np.array(repr(dict(what="reference setup_sampling_mod_info + UnifiedMasking budget draws", in_domains=IN_DOMAINS,
                                       out_domains=OUT_DOMAINS, input_alphas="1.0", target_alphas="0.5", n_in=N_IN, n_tgt=N_TGT,
                                       draws=args.draws)))}
    np.savez_compressed(args.out, **gold)
    print(names, "k_in max", k_in.max(1), "k_tgt max", k_tg.max(1), f"-> {args.out} ({os.path.getsize(args.out) / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
