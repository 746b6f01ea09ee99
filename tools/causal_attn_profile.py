"""Decoder self-attention of one ego-b micro-batch (B = 8, 12 heads of 64, M = 2048 decoder rows at the canonical target split),
forward + backward, under the standard block-diagonal mask or under the causal variant's mask - for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o <name> -- python tools/causal_attn_profile.py causal|standard

The intervals come from the compaction of a synthetic batch (ego_compact / ego_compact_causal), the launches are the engine's
(ego_attn_fwd_d64_seg / ego_attn_bwd_d64_seg with the compaction's row groups and seg_bad flags); q / k / v are random bf16.
Results: DESIGN.md section 4i, profiles/causal_attn_*_kernel_stats.csv."""
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from egom2p_amd import ops, synth                      # noqa: E402
from egom2p_amd.config import MODEL_CFGS               # noqa: E402


def main():
    causal = sys.argv[1] == "causal"
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    dev, B, H, M = "cuda", 8, 12, 2048
    A = H * 64
    cfg = MODEL_CFGS["ego_b_2e_2d"]
    md = synth.make_clip_batch(cfg, B, None, seed=3)
    mods = cfg.mods

    def e(*s, dt=torch.int32):
        return torch.zeros(*s, device=dev, dtype=dt)
    cd = dict(ids_keep=e(B, M, dt=torch.int64), pad=e(B, M, dt=torch.uint8), mod_mask=e(B, M, dt=torch.int16), slot=e(B, M), local=e(B, M),
              tok=e(B, M), ks=e(B, M), ke=e(B, M), n_valid=e(B), seg=e(B, len(mods), 2), err=e(1), seg_bad=e(B))
    ops.compact([md[m.name]["target_mask"].to(dev) for m in mods], [md[m.name]["tensor"].reshape(B, -1).contiguous().to(dev) for m in mods],
                [md[m.name]["decoder_attention_mask"].to(dev) for m in mods], [m.max_tokens for m in mods], [m.id for m in mods], M, True,
                cd, B, causal=causal)
    torch.manual_seed(0)
    qkv = torch.randn(B * M, 3 * A, device=dev).to(torch.bfloat16)
    do = torch.randn(B * M, A, device=dev).to(torch.bfloat16)
    o, dqkv = torch.empty(B * M, A, device=dev, dtype=torch.bfloat16), torch.empty(B * M, 3 * A, device=dev, dtype=torch.bfloat16)
    lse, delta = torch.empty(B, H, M, device=dev), torch.empty(B, H, M, device=dev)
    p, g, rs = qkv.data_ptr(), dqkv.data_ptr(), 3 * A
    for _ in range(iters):
        ops.attn_fwd(p, M * rs, rs, p + 2 * A, M * rs, rs, p + 4 * A, M * rs, rs, o.data_ptr(), M * A, A, lse, cd["ks"], cd["ke"], M, 1,
                     B, H, M, M, 0.125, seg=cd["seg"], seg_bad=cd["seg_bad"])
        ops.attn_bwd(p, M * rs, rs, p + 2 * A, M * rs, rs, p + 4 * A, M * rs, rs, o.data_ptr(), M * A, A, do.data_ptr(), M * A, A, lse, delta,
                     g, M * rs, rs, g + 2 * A, M * rs, rs, g + 4 * A, M * rs, rs, cd["ks"], cd["ke"], M, 1, B, H, M, M, 0.125,
                     seg=cd["seg"], seg_bad=cd["seg_bad"])
    torch.cuda.synchronize()
    print("causal" if causal else "standard", "seg_bad", cd["seg_bad"].tolist(), "err", cd["err"].item(),
          "finite", bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(dqkv.float()).all()))


if __name__ == "__main__":
    main()
