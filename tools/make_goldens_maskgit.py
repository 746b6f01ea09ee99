"""Golden vectors for MaskGIT + CFG generation from the REAL reference `GenerationSampler` (egom2p/models/generate.py):
`forward_enc_dec_maskgit_batched` (:630-650), `select_tokens_batched(..., return_all_samples=True)` (:393-402) and
`sample_tokens_batched` (:373-382), plus `build_chained_generation_schedules` (:197-320) for the schedule fixture.

The reference's files are loaded by path through the helpers of oracle/make_goldens.py (as oracle/make_goldens_generate.py
does); weights come from the counter-based generator with the FLAT head (no synth.peak_logit_table: a peaked head saturates
every sampled probability to exactly 1.0f and turns the selection into a tie).  Temperature 1.0, top-p 0.8, CFG 2.0, three
cosine steps.  Before each step's sampling `torch.manual_seed(1000 + step)` is called - once for `select_tokens_batched` and
once more for `sample_tokens_batched`, so that the tokens and the probabilities belong together (asserted).

The generator ASSERTS that the K-th and the (K+1)-th largest probability differ in every step and batch row: otherwise the
reference's selected set would be torch.topk's arbitrary choice among equal values.  If it trips, change `gen_seed` of the
task; the smallest gap seen is recorded in `meta`.

    python tools/make_goldens_maskgit.py [maskgit_rgb2cam | maskgit_rgb2depth | maskgit_schedules]     (no argument: all three)

Writes data only, to tests/golden/.
"""
from __future__ import annotations

import copy
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from egom2p_amd import synth                      # noqa: E402
from egom2p_amd.config import MODEL_CFGS          # noqa: E402
import make_goldens as MG                         # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

# name: (cfg, weight seed, cond, target, batch, target tokens already known, generation seed)
TASKS = {
    # all 30 cam tokens open; the second clip is the first one rolled by one frame; step 0's unconditional pass has an empty context
    "maskgit_rgb2cam": ("ego_b_2e_2d", 31, "tok_rgb", "tok_cam", 2, 0, 0),
    # the first three depth frames (3072 tokens) are known (the rgb ids stand in), the last two (2048 tokens) are open: the
    # reference's fp32 sort over [rows, 64000] stays small, and step 0's unconditional pass already has a context
    "maskgit_rgb2depth": ("ego_gen_384_2e_2d", 32, "tok_rgb", "tok_depth", 1, 3072, 0),
}
N_STEPS, TEMP, TOP_P, TOP_K, CFG_SCALE = 3, 1.0, 0.8, 0.0, 2.0

# name: keyword arguments of build_chained_generation_schedules
SCHEDULE_CASES = {
    "cos_5120x8": dict(tokens_per_target=[5120], autoregression_schemes=["maskgit"], decoding_steps=[8], token_decoding_schedules=["cosine"],
                       temps=[1.0], temp_schedules=["constant"]),
    "cos_30x3": dict(tokens_per_target=[30], autoregression_schemes=["maskgit"], decoding_steps=[3], token_decoding_schedules=["cosine"],
                     temps=[1.0], temp_schedules=["constant"]),
    "lin_5120x8": dict(tokens_per_target=[5120], autoregression_schemes=["maskgit"], decoding_steps=[8], token_decoding_schedules=["linear"],
                       temps=[0.7], temp_schedules=["constant"]),
    "lin_30x7": dict(tokens_per_target=[30], autoregression_schemes=["maskgit"], decoding_steps=[7], token_decoding_schedules=["linear"],
                     temps=[1.0], temp_schedules=["linear"]),
    "cos_5120x8_tlinear": dict(tokens_per_target=[5120], autoregression_schemes=["maskgit"], decoding_steps=[8],
                               token_decoding_schedules=["cosine"], temps=[1.5], temp_schedules=["linear"]),
    "cos_5120x8_onex": dict(tokens_per_target=[5120], autoregression_schemes=["maskgit"], decoding_steps=[8],
                            token_decoding_schedules=["cosine"], temps=[1.0], temp_schedules=["onex:0.05:0.5"]),
    "cos_30x3_onex": dict(tokens_per_target=[30], autoregression_schemes=["maskgit"], decoding_steps=[3], token_decoding_schedules=["cosine"],
                          temps=[2.0], temp_schedules=["onex:0.05:0.5"]),
    "lin_5120x8_onex": dict(tokens_per_target=[5120], autoregression_schemes=["maskgit"], decoding_steps=[8],
                            token_decoding_schedules=["linear"], temps=[1.0], temp_schedules=["onex:0.05:0.5"]),
    "roar_5120x3_onex": dict(tokens_per_target=[5120], autoregression_schemes=["roar"], decoding_steps=[3], token_decoding_schedules=["linear"],
                             temps=[1.0], temp_schedules=["onex:0.05:0.5"]),
    "chain_roar_maskgit": dict(tokens_per_target=[5120, 30], autoregression_schemes=["roar", "maskgit"], decoding_steps=[3, 4],
                               token_decoding_schedules=["linear", "cosine"], temps=[0.01, 1.0], temp_schedules=["constant", "onex:0.05:0.5"]),
}


def load_generate():
    enc, dec, model = MG.load_reference()

    def _load(modname, relpath):
        spec = importlib.util.spec_from_file_location(modname, os.path.join(MG.REF, relpath))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[modname] = mod
        spec.loader.exec_module(mod)
        return mod

    _load("egom2p.utils.generation", "egom2p/utils/generation.py")
    sys.modules.setdefault("egom2p.utils.tokenizer", type(sys)("egom2p.utils.tokenizer"))
    tt = _load("egom2p.utils.tokenizer.text_tokenizer", "egom2p/utils/tokenizer/text_tokenizer.py")
    sys.modules["egom2p.utils"].get_sentinel_to_id_mapping = tt.get_sentinel_to_id_mapping
    sys.modules["egom2p.utils"].merge_span_masking = tt.merge_span_masking
    G = _load("egom2p.models.generate", "egom2p/models/generate.py")
    return enc, dec, model, G


def make_schedules(G):
    gold = {}
    for name, kw in SCHEDULE_CASES.items():
        n = len(kw["tokens_per_target"])
        full = dict(cond_domains=["tok_rgb"], target_domains=["tok_depth", "tok_cam"][:n], cfg_scales=[2.0] * n,
                    cfg_schedules=["constant"] * n, cfg_grow_conditioning=True, **kw)
        sch = G.build_chained_generation_schedules(**full)
        gold[f"{name}.tokens"] = np.array([s["num_tokens"] for s in sch], dtype=np.int64)
        gold[f"{name}.temps"] = np.array([s["temperature"] for s in sch], dtype=np.float64)
        gold[f"{name}.args"] = np.array(repr(full))
    path = os.path.join(GOLDEN, "maskgit_schedules.npz")
    np.savez_compressed(path, **gold)
    print(f"[goldens] -> {path} ({os.path.getsize(path) / 1e3:.1f} KB)")


def make_task(which, enc, dec, model, G):
    cfg_name, seed, cond, target_mod, B, n_known, gseed = TASKS[which]
    cfg = MODEL_CFGS[cfg_name]
    net = MG.build_reference_model(cfg, enc, dec, model)
    net.load_state_dict(synth.build_state_dict(cfg, seed), strict=True)          # flat head on purpose (module docstring)
    net.eval()
    sampler = G.GenerationSampler(net)
    info = net.modality_info
    n_target = info[target_mod]["max_tokens"]

    rgb = np.load(os.path.join(MG.REF, "example_data", "rgb2cam_egoexo.npz"))
    ids1 = np.asarray(rgb[rgb.files[0]]).astype(np.int64).reshape(1, 5, 32, 32)
    ids = np.concatenate([np.roll(ids1, b, axis=1) for b in range(B)], 0)        # clip b: the frames rolled by b
    sample = {cond: {"tensor": torch.from_numpy(ids), "input_mask": torch.zeros(B, 5120, dtype=torch.bool),
                     "target_mask": torch.ones(B, 5120, dtype=torch.bool)}}
    sample = G.init_empty_target_modality(sample, info, target_mod, B, n_target, "cpu")
    sample = G.init_full_input_modality(sample, info, cond, "cpu")
    if n_known:
        d = sample[target_mod]
        d["tensor"][:, :n_known] = torch.from_numpy(ids.reshape(B, -1)[:, :n_known])
        d["input_mask"][:, :n_known] = False
        d["target_mask"][:, :n_known] = True
    n_open = n_target - n_known
    schedule = G.build_chained_generation_schedules(
        cond_domains=[cond], target_domains=[target_mod], tokens_per_target=[n_open], autoregression_schemes=["maskgit"],
        decoding_steps=[N_STEPS], token_decoding_schedules=["cosine"], temps=[TEMP], temp_schedules=["constant"],
        cfg_scales=[CFG_SCALE], cfg_schedules=["constant"], cfg_grow_conditioning=True)

    gold = {"rgb_ids": ids.astype(np.int32), "n_steps": np.array(len(schedule)),
            # (the known target tokens are rgb_ids[:, :known]: not stored twice; per-step tensors hold the open part [:, known:])
            "init.input_mask": sample[target_mod]["input_mask"].numpy(), "init.target_mask": sample[target_mod]["target_mask"].numpy()}
    min_gap = float("inf")
    mod_dict = copy.deepcopy(sample)
    for step, sinfo in enumerate(schedule):
        target, num_select, temp, cfg_scale = sinfo["target_domain"], int(sinfo["num_tokens"]), sinfo["temperature"], sinfo["cfg_scale"]
        seed_i = gseed + step
        logits_cond, _ = sampler.forward_enc_dec_maskgit_batched(mod_dict, target, seed=seed_i)
        unc = copy.deepcopy(mod_dict)
        for m in sinfo["cfg_cond_domains"]:
            unc = G.empty_img_modality(unc, m)
        logits_uncond, mod_pos = sampler.forward_enc_dec_maskgit_batched(unc, target, seed=seed_i)
        mixed = logits_uncond + (logits_cond - logits_uncond) * cfg_scale
        torch.manual_seed(1000 + step)
        top_samples, top_indices, all_samples = sampler.select_tokens_batched(mixed.clone(), num_select, temperature=temp, top_k=TOP_K,
                                                                              top_p=TOP_P, return_all_samples=True)
        torch.manual_seed(1000 + step)
        samples, probs = sampler.sample_tokens_batched(mixed.clone(), temp, top_k=TOP_K, top_p=TOP_P)
        assert torch.equal(samples, all_samples), "the two seeded calls drew different tokens"
        M = probs.shape[1]
        srt = torch.sort(probs, dim=-1, descending=True).values
        if num_select < M:
            gap = (srt[:, num_select - 1] - srt[:, num_select])
            assert bool((gap > 0).all()), f"step {step}: the K-th and (K+1)-th largest probability tie - change gen_seed of {which}"
            min_gap = min(min_gap, float(gap.min()))
        assert torch.equal(torch.sort(top_indices, -1).values, torch.sort(torch.topk(probs, num_select, dim=-1)[1], -1).values)
        for nm, lg in (("cond", logits_cond), ("uncond", logits_uncond)):
            lg2 = lg.float()
            gold[f"s{step}.{nm}.head"] = lg2[:, :6, :48].numpy().copy()
            gold[f"s{step}.{nm}.argmax"] = lg2.argmax(-1).numpy().astype(np.int32)
            gold[f"s{step}.{nm}.max"] = lg2.max(-1).values.numpy()
            gold[f"s{step}.{nm}.lse"] = torch.logsumexp(lg2, -1).numpy()
            gold[f"s{step}.{nm}.rownorm"] = lg2.norm(dim=-1).numpy()
        gold[f"s{step}.mod_pos"] = mod_pos.numpy().astype(np.int32)
        gold[f"s{step}.samples"] = samples.numpy().astype(np.int32)
        gold[f"s{step}.probs"] = probs.numpy().astype(np.float32)
        gold[f"s{step}.top_indices"] = top_indices.numpy().astype(np.int32)
        gold[f"s{step}.cfg"] = np.array([num_select, temp, cfg_scale])
        gold[f"s{step}.n_enc"] = np.array([int((~mod_dict[m]["input_mask"][0]).sum()) for m in (cond, target_mod)])
        top_pos = torch.gather(mod_pos, -1, top_indices)                              # the reference's update (:697-703)
        d = mod_dict[target]
        d["tensor"] = torch.scatter(d["tensor"], -1, top_pos, top_samples)
        d["input_mask"] = torch.scatter(d["input_mask"], -1, top_pos, torch.zeros_like(top_samples, dtype=torch.bool))
        d["target_mask"] = torch.scatter(d["target_mask"], -1, top_pos, torch.ones_like(top_samples, dtype=torch.bool))
        assert torch.equal(d["tensor"][:, :n_known], sample[target_mod]["tensor"][:, :n_known])
        gold[f"s{step}.tensor"] = d["tensor"][:, n_known:].numpy().astype(np.int32)
        gold[f"s{step}.input_mask"] = d["input_mask"].numpy()
        gold[f"s{step}.target_mask"] = d["target_mask"].numpy()
        print(f"[goldens] {which} step {step}: rows {M}, select {num_select}, enc tokens {gold[f's{step}.n_enc'].tolist()}", flush=True)
    assert bool(mod_dict[target_mod]["target_mask"].all())
    gold["final_tokens"] = mod_dict[target_mod]["tensor"].numpy().astype(np.int32)
    gold["schedule_tokens"] = np.array([s["num_tokens"] for s in schedule])
    gold["meta"] = np.array(repr(dict(cfg=cfg_name, seed=seed, top_p=TOP_P, temperature=TEMP, cfg_scale=CFG_SCALE, gen_seed=gseed, peaked=False,
                                      cond=cond, target=target_mod, tokens=n_target, known=n_known, batch=B, steps=N_STEPS,
                                      min_gap=min_gap)))
    path = os.path.join(GOLDEN, f"{which}.npz")
    np.savez_compressed(path, **gold)
    print(f"[goldens] -> {path} ({os.path.getsize(path) / 1e3:.1f} KB), smallest K / K+1 probability gap {min_gap:.3e}")


def main():
    which = sys.argv[1:] or ["maskgit_schedules", "maskgit_rgb2cam", "maskgit_rgb2depth"]
    torch.set_num_threads(8)
    torch.set_grad_enabled(False)
    enc, dec, model, G = load_generate()
    for w in which:
        if w == "maskgit_schedules":
            make_schedules(G)
        else:
            make_task(w, enc, dec, model, G)


if __name__ == "__main__":
    main()
