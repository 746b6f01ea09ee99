"""The optimiser step of ego-b: the two-group `FusedAdamW` (one `ego_adamw_step` launch per run of equal weight-decay class) against
the same optimiser with layer-wise lr decay (`create_optimizer(..., get_num_layer, get_layer_scale)`: one `ego_adamw_step_seg` launch
over a segment table).  Same model, same bytes.

    python3 tools/adamw_seg_bench.py [--rounds 6] [--steps 30] [--out result.json]

Device events around whole `step()` calls; in every round the three contestants - the two-group optimiser, a SECOND two-group
optimiser (the spread of the baseline against itself) and the segmented one - run `--steps` steps each, alternating, in an order that
rotates from round to round.  Two kinds of step: `clip` (grad_sqnorm + AdamW, the training recipe) and `plain` (AdamW launches only:
its bytes / time is the kernels' bandwidth, 28 B per parameter).  Prints one JSON line: the median step time per contestant and
kind, the baseline-against-itself spread (largest |A1 - A2| of a round's medians, relative), the launch counts per step and the
segment count, and the acceptance `segmented <= two-group * (1 + spread)`.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import types
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODEL = "egom2p_base_12e_12d_swiglu_nobias"
MODS = ("tok_rgb", "tok_depth", "tok_cam", "tok_gaze")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layer_decay", type=float, default=0.75)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from egom2p_amd import ops
    from egom2p_amd.model import MODALITY_INFO, create_model
    from egom2p_amd.optim import FusedAdamW, LayerDecayValueAssigner, create_optimizer, get_num_layer_for_fm, layer_decay_values
    model = create_model(MODEL, encoder_embeddings={m: MODALITY_INFO[m]["encoder_embedding"]() for m in MODS},
                         decoder_embeddings={m: MODALITY_INFO[m]["decoder_embedding"]() for m in MODS}, modality_info=MODALITY_INFO)
    eng = model.engine
    args = types.SimpleNamespace(opt="adamw", lr=1e-4, weight_decay=0.05, opt_betas=(0.9, 0.95), opt_eps=1e-8)
    enc_l, dec_l = model.get_num_layers_encoder(), model.get_num_layers_decoder()
    two = [FusedAdamW(eng, lr=1e-4, weight_decay=0.05, named_parameters=model.named_parameters()) for _ in range(2)]
    seg = create_optimizer(args, model, get_num_layer=partial(get_num_layer_for_fm, num_enc_layers=enc_l, num_dec_layers=dec_l),
                           get_layer_scale=LayerDecayValueAssigner(layer_decay_values(a.layer_decay, enc_l + dec_l)).get_scale)
    who = {"two_group": two[0], "two_group_again": two[1], "segmented": seg}
    kinds = {"clip": 1.0, "plain": None}

    # launches per step, counted at the ops boundary
    counts = {}
    for name, opt in who.items():
        for kind, clip in kinds.items():
            n = {}
            saved = {f: getattr(ops, f) for f in ("adamw_step", "adamw_step_seg", "grad_sqnorm")}
            for f, fn in saved.items():
                def counted(*x, _f=f, _fn=fn, **k):
                    n[_f] = n.get(_f, 0) + 1
                    return _fn(*x, **k)
                setattr(ops, f, counted)
            try:
                opt.step(clip_grad=clip)
            finally:
                for f, fn in saved.items():
                    setattr(ops, f, fn)
            counts[f"{name}.{kind}"] = n
    torch.cuda.synchronize()

    def run(opt, clip, steps):
        ts = []
        for _ in range(steps):
            eng.G.normal_()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            opt.step(clip_grad=clip)
            e.record()
            ts.append((s, e))
        torch.cuda.synchronize()
        return [s.elapsed_time(e) * 1e3 for s, e in ts]             # microseconds

    for opt in who.values():
        for clip in kinds.values():
            run(opt, clip, a.warmup)
    names = list(who)
    med = {f"{n}.{k}": [] for n in names for k in kinds}
    for r in range(a.rounds):
        order = names[r % 3:] + names[:r % 3]
        for kind, clip in kinds.items():
            for n in order:
                med[f"{n}.{kind}"].append(statistics.median(run(who[n], clip, a.steps)))
    out = {"model": MODEL, "params": eng.num_params(), "n_flat": eng.n_flat, "rounds": a.rounds, "steps": a.steps,
           "groups": len(seg.param_groups), "segments": sum(len(t) for t, _ in seg._launches), "seg_launches": len(seg._launches),
           "two_group_runs": len(two[0]._runs), "launches_per_step": counts}
    for kind in kinds:
        a1, a2, b = (med[f"{n}.{kind}"] for n in names)
        spread = max(abs(x - y) / min(x, y) for x, y in zip(a1, a2))
        m1, m2, mb = statistics.median(a1), statistics.median(a2), statistics.median(b)
        out[kind] = {"two_group_us": m1, "two_group_again_us": m2, "segmented_us": mb, "per_round_us": {n: med[f"{n}.{kind}"] for n in names},
                     "baseline_spread": spread, "segmented_over_two_group": mb / m1, "accepted": mb <= m1 * (1.0 + spread)}
    nbytes = 28.0 * eng.n_flat
    out["plain"]["two_group_GBps"] = nbytes / out["plain"]["two_group_us"] / 1e3
    out["plain"]["segmented_GBps"] = nbytes / out["plain"]["segmented_us"] / 1e3
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
