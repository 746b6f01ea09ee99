"""EgoM2P training/inference engine for one MI355X: owns the flat fp32 parameter / gradient buffers,
the bf16 weight copies, the activation workspaces, and issues the HIP kernels of one forward and one
hand-ordered backward pass (no autograd graph, no tracing compiler).

Dataflow = `EgoM2P.forward` of the reference (egom2p/models/egom2p_model.py:683-734) with the
autocast(bf16) numerics of `run_training_egom2p.py:725`: GEMM-class ops in bf16 with fp32 MFMA
accumulation, LayerNorm / softmax / cross-entropy / residual stream in fp32.

Layout decisions (MI355X-first, 288 GB HBM):
  * every parameter lives in ONE flat fp32 buffer in forward order; gradients in a twin buffer, so
    gradients become final from the tail backwards and per-layer slices are the all-reduce buckets;
  * every activation needed by the backward is kept (1.7 GB per clip at ego-b): no recompute - unless `act_checkpoint` is set:
    then a layer keeps only its fp32 input, every block runs in one buffer set per stack and the backward runs a block's
    forward again in front of the block's backward;
  * decoder rows are written modality-grouped by the final LayerNorm so the per-modality logits / CE
    run on contiguous row ranges whose (offset, count) stay on the device (no host sync anywhere);
  * MLP hidden size is padded to a multiple of 128 in the masters themselves (pad entries are exactly
    zero and stay zero), so every GEMM dimension is tile-aligned.
"""
from __future__ import annotations

import math
import os
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib as L
from . import ops
from .config import ModelCfg, Modality
from .posemb import build_pos_emb

BF16 = torch.bfloat16
F32 = torch.float32
I32 = torch.int32


_WARM_STREAMS: Dict[int, "torch.cuda.Stream"] = {}


def _warmup_stream(dev: torch.device) -> "torch.cuda.Stream":
    """The side stream graph captures warm up on: one per device and process (a stream is a hardware queue)."""
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _WARM_STREAMS:
        _WARM_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _WARM_STREAMS[key]


def head_layout(H: int, HD: int, min_pad: int = 0) -> Tuple[int, int]:
    """(elements between two stored heads, heads in storage) for H heads of dimension HD.

    Heads of 64 are stored as they are (the throughput attention kernels); A = H * 64 is the N / K extent of the qkv / proj
    GEMMs and the pitch of the [rows, A] buffers, which the kernels are validated for in multiples of 128 only: an odd head
    count (dim 960 = 15 x 64) is refused.  Other head dimensions are zero-padded to 96 or 128 (ego_attn_*_hd kernels) and, where
    that makes A a multiple of 128 with narrower rows, an all-zero PHANTOM head is appended: the registered ego-L (15 heads of
    68) is 16 x 96 = 1536 wide - the phantom head's q = k = v = 0 give a uniform softmax over zero values, output and every
    gradient through it exactly 0 - where 15 x 128 = 1920 cost 25 % more attention and qkv / proj GEMM work.
    min_pad (EGOM2P_HEAD_PAD) = 128 keeps the round-3 layout."""
    if HD == 64:
        if (H * 64) % 128:
            raise L.EgoHipError(f"heads of 64 need an even head count (heads={H}: A = {H * 64} is not a multiple of 128)")
        return 64, H
    fits = sorted((next(n for n in range(H, H + 9) if (n * h) % 128 == 0) * h, h) for h in (96, 128) if h >= HD and h >= min_pad)
    if not fits:
        raise L.EgoHipError(f"no storage layout for {H} heads of {HD}")
    return fits[0][1], fits[0][0] // fits[0][1]


def drop_path_rates(cfg: ModelCfg) -> Tuple[List[float], List[float]]:
    """Per-layer drop rates (encoder, decoder) by the reference's rule (egom2p_model.py:137-154): the fp32 `.item()` values of
    torch.linspace(0, rate, depth) per stack or, with shared_drop_path, of ONE linspace over encoder + decoder layers cut at the
    encoder depth.  A layer at rate 0 (always the first of a linspace from 0) holds nn.Identity there: it neither scales nor draws."""
    Le, Ld = cfg.encoder_depth, cfg.decoder_depth
    re_, rd = float(cfg.drop_path_rate_encoder), float(cfg.drop_path_rate_decoder)
    if cfg.shared_drop_path:
        return ([v.item() for v in torch.linspace(0, re_, Le + Ld)][:Le], [v.item() for v in torch.linspace(0, rd, Le + Ld)][Le:])
    return [v.item() for v in torch.linspace(0, re_, Le)], [v.item() for v in torch.linspace(0, rd, Ld)]


def _pad128(n: int) -> int:
    return (n + 127) // 128 * 128


class _Rows(NamedTuple):
    """One operand of an attention launch (q, k, v or a gradient of one): bf16 rows inside tensor `t`, the first one `off`
    elements in, `rs` elements apart; a sample's rows follow the previous sample's."""
    t: torch.Tensor
    off: int
    rs: int

    def args(self, n):        # the kernels' operand triple: address, elements between two samples of n rows, between two rows
        return self.t.data_ptr() + 2 * self.off, n * self.rs, self.rs


# The key interval [ks, ke) a query row may attend to, as the kernels take it: (ks, ke, stride per sample, stride per row).
def _keys_per_sample(zero_b, n_valid):
    """one interval [0, n_valid) per SAMPLE (key padding): the uniform form lets the attention kernels walk one (batch, head) pair
    per XCD (L2-resident K / V)"""
    return zero_b, n_valid, 1, 0


def _keys_per_row(ks, ke, M):
    """one interval per query ROW of M-row samples (the decoder's block-diagonal / causal self-attention mask)"""
    return ks, ke, M, 1


class _Lin:
    """One linear layer: master view [out, in] (possibly padded), bf16 W [out, in] and W^T [in, out]; with the fp8
    forward enabled also W as OCP e4m3 bytes with one fp32 scale per output channel."""
    __slots__ = ("name", "w", "g", "wb", "wt", "out_f", "in_f", "w8", "s8", "wt8", "st8", "b", "gb")

    def __init__(self, name, w, g, dev, fp8=False, fp8_bwd=False, b=None, gb=None):
        self.name, self.w, self.g = name, w, g
        self.b, self.gb = b, gb          # fp32 bias [out] and its gradient (the biased family), else None
        self.out_f, self.in_f = w.shape
        self.wb = torch.zeros(self.out_f, self.in_f, device=dev, dtype=BF16)
        self.wt = torch.zeros(self.in_f, self.out_f, device=dev, dtype=BF16)
        ok8 = fp8 and self.in_f % 128 == 0 and self.in_f >= 256 and self.out_f % 128 == 0
        self.w8 = torch.zeros(self.out_f, self.in_f, device=dev, dtype=torch.uint8) if ok8 else None
        self.s8 = torch.ones(self.out_f, device=dev, dtype=F32) if ok8 else None
        # fp8 dgrad (dX = dY W): W^T [in, out] as e4m3 with one scale per input channel - the contraction runs over `out`
        okb = fp8_bwd and self.out_f % 128 == 0 and self.out_f >= 256 and self.in_f % 128 == 0
        self.wt8 = torch.zeros(self.in_f, self.out_f, device=dev, dtype=torch.uint8) if okb else None
        self.st8 = torch.ones(self.in_f, device=dev, dtype=F32) if okb else None


class Engine:
    pair_stream = None        # the benchmark reads and restores this around its per-kernel leg; it is always None

    def __init__(self, cfg: ModelCfg, device="cuda:0", max_batch: int = 1, n_enc: int = 2048, n_dec: int = 2048,
                 attn_o_residual: str = "cross", fp8_forward: bool = False, fp8_backward: bool = False, act_checkpoint: bool = False):
        """act_checkpoint (or `cfg.use_act_checkpoint`): activation checkpointing per block - every layer saves its fp32 input only, the
        blocks of a stack run in ONE shared buffer set, and `backward` rebuilds a block from its saved input (the forward's own launches
        on the shared set) right before the block's backward.  Same bits as the plain engine, one more pass over the blocks per step.
        attn_o_residual: which attention sites also keep the bf16 rounding residual of their output so that the
        backward's delta = rowsum(dO o O) is formed from O to ~16 bits ("cross": the cross-attention sites - where, with
        near-uniform attention over ~2000 context keys, the plain flash-style delta put 3.5 % error on the query-path
        gradients; "all"; "none").  Costs one more bf16 [rows, D] write + read per site (~0.5 % of a step for "cross")."""
        L.load()  # fail loudly if the HIP library is missing
        # fp8_forward (BASELINE config 5, "bf16 + fp8 MFMA GEMMs"): the forward linears (qkv / q / kv / proj / fc1||fc3 / fc2 /
        # context projection) run on e4m3 operands - activations quantised per row right before the GEMM, weights per
        # output channel once per optimiser step - with fp32 accumulation; the backward and the logits stay bf16.
        self.fp8_forward = bool(fp8_forward)
        # fp8_backward (round 5): the dgrad GEMMs dX = dY W on e4m3 operands too - dY quantised per row (the
        # contraction runs over the output channels, so a per-row scale of dY and a per-input-channel scale of W^T factor out
        # exactly like the forward's scales); e4m3 rather than e5m2 because the per-ROW scale already takes the gradient's
        # row-to-row dynamic range out and the 3-bit mantissa is then the limit.  Weight gradients stay bf16: their contraction
        # runs over the rows, where per-row scales do not factor out.  Measured gain / kill criterion: DESIGN section 4f.
        self.fp8_backward = bool(fp8_backward)
        if attn_o_residual not in ("cross", "all", "none"):
            raise ValueError("attn_o_residual must be 'cross', 'all' or 'none'")
        self.attn_o_residual = attn_o_residual
        self.act_checkpoint = bool(act_checkpoint) or bool(cfg.use_act_checkpoint)     # (P, G and the layout tag do not depend on it)
        # Storage geometry.  D = the row pitch of every [rows, dim] activation and of every weight's model-dim axis: cfg.dim
        # rounded up to 128 (GEMM K steps / tiles) with zero pad columns - equal to cfg.dim for ego-b and the 1152-wide
        # ego-L; the REGISTERED ego-L (egom2p_model.py:1080-1092: dim 1020, 15 heads of 68) lives in rows of 1024.  Heads
        # are stored HDP elements apart (64 -> 64: the throughput attention kernels; otherwise zero-padded to 96 or 128 for
        # the ego_attn_*_hd kernels), A = H * HDP is the width of the q / k / v / attention-output rows.  Pad columns and
        # pad weight rows are zero and stay zero: their gradients are exact zeros (zero operands), and AdamW maps (0, 0) to 0.
        self.cfg = cfg
        self.dev = torch.device(device)
        self.Dl, self.D, self.H = cfg.dim, _pad128(cfg.dim), cfg.num_heads
        self.HD = cfg.head_dim
        self.HDP, self.Hs = head_layout(cfg.num_heads, cfg.head_dim, int(os.environ.get("EGOM2P_HEAD_PAD", "0")))
        self.A = self.Hs * self.HDP
        self.padded = self.D != self.Dl or self.HDP != self.HD or self.Hs != self.H
        if self.padded and (fp8_forward or fp8_backward):
            raise L.EgoHipError("the fp8 GEMMs are built for the unpadded shapes (dim % 128 == 0, head_dim 64)")
        self.F, self.Fp = cfg.mlp_hidden, _pad128(cfg.mlp_hidden)
        # the GELU / biased family (egom2p_model.py:881-978): plain Mlp under an erf GELU (one [F, D] fc1, no fc3), a bias on qkv / q /
        # kv, on proj and on fc1 / fc2, nn.LayerNorm with its bias - each its own flag of the configuration
        if cfg.mlp not in ("swiglu", "gelu"):
            raise ValueError(f"ModelCfg.mlp must be 'swiglu' or 'gelu', not {cfg.mlp!r}")
        self.gelu = cfg.mlp == "gelu"
        self.norm_bias = bool(cfg.norm_bias)
        self.lin_bias = dict(qkv=bool(cfg.qkv_bias), proj=bool(cfg.proj_bias), mlp=bool(cfg.mlp_bias))
        family = self.gelu or self.norm_bias or any(self.lin_bias.values())
        if family and (fp8_forward or fp8_backward):
            raise NotImplementedError("the fp8 GEMMs carry no bias epilogue and the fp8 forward no GELU / biased LayerNorm: the GELU / "
                                      "biased family (mlp='gelu', qkv_bias, proj_bias, mlp_bias, norm_bias) runs in bf16 only")
        if family and self.padded:
            raise NotImplementedError("the GELU / biased family is built for unpadded storage (dim % 128 == 0, heads of 64)")
        if cfg.mlp_bias and not self.gelu:
            raise NotImplementedError("mlp_bias with the gated MLP (a bias on the fused fc1||fc3 launch) is not built: mlp_bias needs mlp='gelu'")
        # the QK-norm family (egom2p_model.py:1122-1196; NormAttention / NormCrossAttention, egom2p_utils.py:247-332): a bias-free
        # LayerNorm over every head's 64 q and k values, one [64] weight per site and operand (ego_headnorm_fwd / _bwd)
        self.qk_norm = bool(cfg.qk_norm)
        if self.qk_norm and (self.padded or self.HD != 64):
            raise NotImplementedError("qk_norm is built for unpadded storage (dim % 128 == 0, heads of 64): the head-norm kernels take heads of 64")
        if self.qk_norm and (fp8_forward or fp8_backward):
            raise NotImplementedError("qk_norm with the fp8 GEMMs (fp8_forward / fp8_backward) is not built: the QK-norm family runs in bf16 only")
        if self.qk_norm and self.norm_bias:
            raise NotImplementedError("qk_norm with norm_bias=True (the reference then gives the head norms a bias) is not built")
        self.Fab = self.Fp if self.gelu else 2 * self.Fp        # width of the saved MLP pre-activation rows: u, or a || b
        # stochastic depth (egom2p_utils.py:89-112, 356-359, 387-391): the residual sites with a non-zero rate, in forward order - (site
        # name, keep_prob as the fp32 the reference's bf16 `x.div(keep_prob)` divides by).  No site: nothing below allocates or launches.
        r_enc, r_dec = drop_path_rates(cfg)
        for r in r_enc + r_dec:
            if not 0.0 <= r < 1.0:
                raise ValueError(f"drop path rates must lie in [0, 1), not {r}")
        self.dp_sites: List[Tuple[str, float]] = []
        for kind, rates, subs in (("encoder", r_enc, ("attn", "mlp")), ("decoder", r_dec, ("self_attn", "cross_attn", "mlp"))):
            for i, r in enumerate(rates):
                if r > 0.0:
                    kp = torch.tensor(1.0 - r, dtype=torch.float64).to(F32).item()
                    self.dp_sites += [(f"{kind}.{i}.{sub}", kp) for sub in subs]
        self._dp_ix = {name: (j, kp) for j, (name, kp) in enumerate(self.dp_sites)}
        self._dp_live = False                 # the forward in flight / being differentiated drops paths
        self._dp_seed, self._dp_counter, self._dp_inject = 0, 0, None
        self.dp_last = None                   # (seed, forward counter) the last training forward drew with; None: injected tables
        # asymmetric models (run_training_egom2p.py:354-389): enc_mods own an encoder embedding, dec_mods a decoder embedding; mods =
        # the ones in either set, in configuration order (slots, positional tables, workspace sizes).  A symmetric model: all three equal.
        self.enc_mods: List[Modality] = cfg.enc_mods
        self.dec_mods: List[Modality] = cfg.dec_mods
        if not self.enc_mods or not self.dec_mods:
            raise ValueError("a model needs at least one encoder and one decoder modality")
        either = {m.name for m in self.enc_mods} | {m.name for m in self.dec_mods}
        self.mods: List[Modality] = [m for m in cfg.mods if m.name in either]
        self.n_mods = len(self.mods)
        # decoder modalities whose mod_emb is a parameter of its own: the decoder-only ones and, with share_modality_embeddings=False,
        # all of them; the others alias the encoder's (share_modality_embeddings(), egom2p_model.py:179-183: the intersection)
        enc_names = {m.name for m in self.enc_mods}
        self.dec_own_mod_emb = {m.name for m in self.dec_mods if not cfg.share_modality_embeddings or m.name not in enc_names}
        self.sep_mask = bool(cfg.decoder_sep_mask)
        # learned positional tables (sincos_pos_emb=False): per side, the modalities whose pos_emb is a parameter in P / G
        for side, names, have in (("encoder", cfg.learned_pos_emb_encoder, self.enc_mods), ("decoder", cfg.learned_pos_emb_decoder, self.dec_mods)):
            unknown = [n for n in names if n not in {m.name for m in have}]
            if unknown:
                raise ValueError(f"learned_pos_emb_{side}: {unknown} not among the {side} modalities")
        self.learned_enc, self.learned_dec = set(cfg.learned_pos_emb_encoder), set(cfg.learned_pos_emb_decoder)
        self.N, self.M, self.Bmax = n_enc, n_dec, max_batch
        # register tokens (egom2p_model.py:170-171, 381-387): R learned rows in front of every sample's N kept encoder tokens - the
        # encoder, the context and the cross-attention keys have Ne = R + N rows per sample; the compaction keeps N
        self.R = int(cfg.num_register_tokens)
        self.Ne = self.N + self.R
        self.scale = cfg.head_dim ** -0.5
        self._build_params()
        self.q8, self.qs, self._q_of = None, None, None      # fp8 GEMMs: e4m3 copy + row scales of the current GEMM input, and whose it is
        self._alloc_workspaces()
        self.weights_dirty = True
        self.params_swapped = False                     # inside ModelEma.applied(): P holds the averaged weights (ema.py)
        self._have_fwd = False
        self.fmods, self.femods = self.dec_mods, self.enc_mods      # the decoder / encoder modalities of the last forward (a mod_dict may hold a subset)
        self._ce_done, self._ce_grad = set(), None      # modalities whose CE backward ran inside the forward (loss_grad)
        self._loss_mode = 0                             # ops.LOSS_MODES of the last forward
        self._canon_dev = {}                            # decoder order -> its modality indices on the device
        self.touched = None                             # track_touched_table_rows
        self.max_graphs = 16                  # captured generation passes kept alive at once (LRU)
        self._iw, self._infer_key = None, None
        # decoder self-attention launched by row groups (one interval per workgroup); 0: per-row interval launches (round 3)
        self.attn_groups = os.environ.get("EGOM2P_ATTN_GROUPS", "1") != "0"
        self.attn_split = os.environ.get("EGOM2P_ATTN_SPLIT", "1") != "0"       # generation path: split keys on under-filled grids
        self.cfg_pair = os.environ.get("EGOM2P_CFG_PAIR", "1") != "0"           # guided step: cond + uncond share one decoder pass
        # every decoder layer's context_norm normalises the SAME context tensor: one fused launch forward (x and its statistics
        # read once, one output per layer) and one backward (x once, one write of the context gradient) instead of one per layer
        # (the multi-layer launches have no biased twin: with norm_bias every layer's context_norm is its own launch)
        self.ctx_ln_fused = (os.environ.get("EGOM2P_CTX_LN_FUSED", "1") != "0" and not self.fp8_forward and self.D <= 1536
                             and 0 < cfg.decoder_depth <= 32 and not self.norm_bias)

    def layout_tag(self) -> Tuple[int, ...]:
        """What the PHYSICAL flat buffers (P, G and the optimiser's m / v) depend on beyond the model: saved with optimiser
        checkpoints and checked on load (a resume under another EGOM2P_HEAD_PAD must not die in a bare copy_)."""
        return (2, int(self.n_flat), int(self.D), int(self.Hs), int(self.HDP), int(self.Fp))    # 2: context_norm weights in one group (round 5)

    def _ring_next(self):
        self._ring_i = (self._ring_i + 1) % len(self.ring_b)
        return self.ring_b[self._ring_i]

    def _ln_bwd(self, dy, x, wname, st, dx_out, **kw):
        """The backward of `_ln(x, wname, y, st)` (kw: dx_in, dx_bf16; dw and, with norm_bias, db are accumulated)"""
        ops.layernorm_bwd(dy, x, st[0], st[1], self.p[wname], dx_out, self.g[wname], width=self.Dl,
                          db=self.g.get(wname[:-len("weight")] + "bias"), **kw)

    # ------------------------------------------------------------------------------------ parameters
    def _build_params(self):
        D, A, Fp, cfg = self.D, self.A, self.Fp, self.cfg
        spec: List[Tuple[str, Tuple[int, ...]]] = []
        groups: List[Tuple[str, int, int]] = []      # (group name, lo, hi) = all-reduce buckets, forward order

        def add(name, shape):
            spec.append((name, tuple(shape)))

        def norm(name):           # a LayerNorm's weight and, with norm_bias, its bias (nn.LayerNorm's names)
            add(f"{name}.weight", (D,))
            if self.norm_bias:
                add(f"{name}.bias", (D,))

        def layer(prefix, kind):
            # (a decoder layer's context_norm weight lives in the "ctx_norms" group in front of the decoder layers: with the fused
            #  context LayerNorm backward its gradient is only final after the LAST decoder layer's backward, and it must not
            #  hold the layer's 14 MB gradient bucket back from the data-parallel exchange until then - ADVICE r4)
            norms = ["norm1", "norm2"] if kind == "enc" else ["norm1", "query_norm", "norm2"]
            for n in norms:
                norm(f"{prefix}.{n}")
            if self.qk_norm:      # the head norms' weights (reference names), in the layer's no-decay run and its own bucket
                for site in (("attn",) if kind == "enc" else ("self_attn", "cross_attn")):
                    add(f"{prefix}.{site}.q_norm.weight", (self.HD,))
                    add(f"{prefix}.{site}.k_norm.weight", (self.HD,))
            # the linears' biases (reference names) sit behind the norms: one no-decay run per layer, in the layer's own bucket
            lins = ([("attn.qkv", 3 * A, "qkv"), ("attn.proj", D, "proj")] if kind == "enc" else
                    [("self_attn.qkv", 3 * A, "qkv"), ("self_attn.proj", D, "proj"), ("cross_attn.q", A, "qkv"),
                     ("cross_attn.kv", 2 * A, "qkv"), ("cross_attn.proj", D, "proj")]) + [("mlp.fc1", Fp, "mlp"), ("mlp.fc2", D, "mlp")]
            for sub, n, flag in lins:
                if self.lin_bias[flag]:
                    add(f"{prefix}.{sub}.bias", (n,))
            if kind == "enc":
                add(f"{prefix}.attn.qkv.weight", (3 * A, D))
                add(f"{prefix}.attn.proj.weight", (D, A))
            else:
                add(f"{prefix}.self_attn.qkv.weight", (3 * A, D))
                add(f"{prefix}.self_attn.proj.weight", (D, A))
                add(f"{prefix}.cross_attn.q.weight", (A, D))
                add(f"{prefix}.cross_attn.kv.weight", (2 * A, D))
                add(f"{prefix}.cross_attn.proj.weight", (D, A))
            add(f"{prefix}.mlp.fc1.weight", (Fp, D))      # fc1 | fc3 adjacent: one fused [2Fp, D] GEMM operand
            if not self.gelu:                             # (the plain Mlp has no fc3: egom2p_utils.py:136-151)
                add(f"{prefix}.mlp.fc3.weight", (Fp, D))
            add(f"{prefix}.mlp.fc2.weight", (D, Fp))

        marks = []
        for m in self.enc_mods:
            marks.append((f"enc_table.{m.name}", len(spec)))
            add(f"encoder_embeddings.{m.name}.token_emb.weight", (m.vocab_size, D))
        marks.append(("mod_emb", len(spec)))
        for m in self.enc_mods:
            add(f"encoder_embeddings.{m.name}.mod_emb", (D,))
        if cfg.num_register_tokens:
            add("register_tokens", (cfg.num_register_tokens, D))       # reference shape (1, R, dim); decayed like mod_emb / mask_token
        for i in range(cfg.encoder_depth):
            marks.append((f"encoder.{i}", len(spec)))
            layer(f"encoder.{i}", "enc")
        marks.append(("bridge", len(spec)))
        norm("encoder_norm")
        add("decoder_proj_context.bias", (D,))
        add("decoder_proj_context.weight", (D, D))
        if cfg.decoder_depth:
            marks.append(("ctx_norms", len(spec)))
            for i in range(cfg.decoder_depth):
                norm(f"decoder.{i}.context_norm")
        for i in range(cfg.decoder_depth):
            marks.append((f"decoder.{i}", len(spec)))
            layer(f"decoder.{i}", "dec")
        marks.append(("head", len(spec)))
        norm("decoder_norm")
        add("mask_token", (D,))
        # a decoder modality's own mod_emb (decoder-only modalities; all of them when unshared) sits beside the mask token: decayed
        # like it, final with it (the decoder embedding backward), in the "head" bucket.  A symmetric shared model has none.
        for m in self.dec_mods:
            if m.name in self.dec_own_mod_emb:
                add(f"decoder_embeddings.{m.name}.mod_emb", (D,))
        for m in self.dec_mods:
            marks.append((f"dec_table.{m.name}", len(spec)))
            add(f"decoder_embeddings.{m.name}.token_emb.weight", (m.vocab_size, D))
        if not cfg.share_embedding:
            for m in self.dec_mods:
                marks.append((f"to_logits.{m.name}", len(spec)))
                add(f"decoder_embeddings.{m.name}.to_logits.weight", (m.vocab_size, D))
        # learned positional tables behind everything else (a model without one keeps its layout): reference shape (1, n_pos, dim),
        # decayed like mod_emb (no_weight_decay() is empty); one bucket, final with the encoder embedding backward
        if self.learned_enc or self.learned_dec:
            marks.append(("pos_emb", len(spec)))
            for m in self.enc_mods:
                if m.name in self.learned_enc:
                    add(f"encoder_embeddings.{m.name}.pos_emb", (m.max_tokens, D))
            for m in self.dec_mods:
                if m.name in self.learned_dec:
                    add(f"decoder_embeddings.{m.name}.pos_emb", (m.max_tokens, D))

        offs, total = {}, 0
        for name, shape in spec:
            n = math.prod(shape)
            offs[name] = (total, n, shape)
            total += (n + 3) // 4 * 4
        self.n_flat = total
        # where the learned positional tables start: what lies in front is the flat layout of the same model with fixed tables
        self.n_flat_body = min([o for k, (o, _, _) in offs.items() if k.endswith("pos_emb")], default=total)
        self.P = torch.zeros(total, device=self.dev, dtype=F32)
        self.G = torch.zeros(total, device=self.dev, dtype=F32)
        self.p: Dict[str, torch.Tensor] = {}
        self.g: Dict[str, torch.Tensor] = {}
        self.offsets = offs
        for name, (o, n, shape) in offs.items():
            self.p[name] = self.P[o:o + n].view(shape)
            self.g[name] = self.G[o:o + n].view(shape)
        starts = [offs[spec[i][0]][0] for _, i in marks] + [total]
        self.buckets = [(marks[i][0], starts[i], starts[i + 1]) for i in range(len(marks))]
        # optimiser runs: contiguous ranges of equal weight-decay class (no_decay: norm weights and biases)
        # tensors no kernel ever writes a gradient for: with an untied head the decoder token tables are never read (the
        # decoder rows are the mask token, egom2p_model.py:328), the reference leaves their .grad None and AdamW skips them
        self.never_grad = set() if cfg.share_embedding else {f"decoder_embeddings.{m.name}.token_emb.weight" for m in self.dec_mods}
        runs: List[List] = []
        for name, shape in spec:
            if name in self.never_grad:
                continue
            o, n, _ = offs[name]
            nd = ("norm." in name or ".norm" in name or name.endswith(".bias"))
            n4 = (n + 3) // 4 * 4
            if runs and runs[-1][2] == nd and runs[-1][1] == o:
                runs[-1][1] = o + n4
            else:
                runs.append([o, o + n4, nd])
        self.opt_runs = [(a, b, nd) for a, b, nd in runs]
        # fixed positional tables (buffers)
        self.pos = {}
        for m in self.mods:
            pe = torch.zeros(m.max_tokens, D, device=self.dev, dtype=F32)
            pe[:, :self.Dl] = build_pos_emb(m, self.Dl)[0].to(self.dev)
            self.pos[m.name] = pe
        # the table a side's embedding reads: the fixed one, or the side's own parameter
        self.pos_enc = {m.name: self.p.get(f"encoder_embeddings.{m.name}.pos_emb", self.pos[m.name]) for m in self.enc_mods}
        self.pos_dec = {m.name: self.p.get(f"decoder_embeddings.{m.name}.pos_emb", self.pos[m.name]) for m in self.dec_mods}

        # linear layers: bf16 copies
        self.lin: Dict[str, _Lin] = {}

        def lin(name):
            body = "token_emb" not in name and "to_logits" not in name
            # a layer linear's own bias (the biased family); decoder_proj_context's bias is handed over by its call sites, as ever
            bk = name[:-len("weight")] + "bias" if name.startswith(("encoder.", "decoder.")) else None
            self.lin[name] = _Lin(name, self.p[name], self.g[name], self.dev, fp8=self.fp8_forward and body, fp8_bwd=self.fp8_backward and body,
                                  b=self.p.get(bk), gb=self.g.get(bk))

        for i in range(cfg.encoder_depth):
            for s in ("attn.qkv", "attn.proj", "mlp.fc2"):
                lin(f"encoder.{i}.{s}.weight")
            lin(f"encoder.{i}.mlp.fc1.weight") if self.gelu else self._fuse13(f"encoder.{i}")
        for i in range(cfg.decoder_depth):
            for s in ("self_attn.qkv", "self_attn.proj", "cross_attn.q", "cross_attn.kv", "cross_attn.proj", "mlp.fc2"):
                lin(f"decoder.{i}.{s}.weight")
            lin(f"decoder.{i}.mlp.fc1.weight") if self.gelu else self._fuse13(f"decoder.{i}")
        lin("decoder_proj_context.weight")
        self.logit_key = {m.name: (f"decoder_embeddings.{m.name}.token_emb.weight" if cfg.share_embedding
                                   else f"decoder_embeddings.{m.name}.to_logits.weight") for m in self.dec_mods}
        # the mod_emb a decoder row of modality m adds: its own parameter, or the encoder's
        self.dec_mod_emb_key = {m.name: (f"decoder_embeddings.{m.name}.mod_emb" if m.name in self.dec_own_mod_emb
                                         else f"encoder_embeddings.{m.name}.mod_emb") for m in self.dec_mods}
        for key in self.logit_key.values():
            lin(key)

    def _fuse13(self, prefix):
        """fc1 and fc3 are adjacent in the flat buffer: expose them as one [2Fp, D] linear."""
        o1 = self.offsets[f"{prefix}.mlp.fc1.weight"][0]
        n = 2 * self.Fp * self.D
        w = self.P[o1:o1 + n].view(2 * self.Fp, self.D)
        g = self.G[o1:o1 + n].view(2 * self.Fp, self.D)
        self.lin[f"{prefix}.mlp.fc13"] = _Lin(f"{prefix}.mlp.fc13", w, g, self.dev, fp8=self.fp8_forward, fp8_bwd=self.fp8_backward)

    # reference key layout <-> engine storage ----------------------------------------------------
    def _is_buffer_key(self, key: str) -> bool:
        """reference keys without storage here: fixed pos tables are rebuilt (a learned one is a parameter), LN bias is a zero buffer
        (a parameter with norm_bias)"""
        return (key.endswith("pos_emb") and key not in self.p) or (not self.norm_bias and key.endswith(".bias") and "norm" in key)

    def _view_for_key(self, key: str) -> Optional[torch.Tensor]:
        if self._is_buffer_key(key):
            return None
        key = self._canon_key(key)
        return self._logical(key, self.p[key])

    def _logical(self, key: str, t: torch.Tensor) -> torch.Tensor:
        """The part of a storage tensor (parameter or gradient) that is the reference's tensor `key`: a view without the
        zero padding.  Unpadded configurations: the tensor itself (fc1 / fc3 / fc2: without the F -> Fp pad).  Padded ones:
        the model-dim axes cut to cfg.dim and the head axis split so that every head loses its pad columns - a strided view
        of as many elements as the reference tensor, in its element order (`.reshape(reference shape)` gives the tensor)."""
        F, Dl, H, Hs, HD, HDP = self.F, self.Dl, self.H, self.Hs, self.HD, self.HDP
        if key.endswith("mlp.fc1.weight") or key.endswith("mlp.fc3.weight"):
            return t[:F, :Dl]
        if key.endswith("mlp.fc2.weight"):
            return t[:Dl, :F]
        if not self.padded:
            return t
        if t.dim() == 1:
            return t[:Dl]
        if key.endswith("qkv.weight"):
            return t.view(3, Hs, HDP, self.D)[:, :H, :HD, :Dl]
        if key.endswith("cross_attn.kv.weight"):
            return t.view(2, Hs, HDP, self.D)[:, :H, :HD, :Dl]
        if key.endswith("cross_attn.q.weight"):
            return t.view(Hs, HDP, self.D)[:H, :HD, :Dl]
        if key.endswith("proj.weight"):                       # attn.proj / self_attn.proj / cross_attn.proj: [D, A]
            return t.view(self.D, Hs, HDP)[:Dl, :H, :HD]
        if key == "decoder_proj_context.weight":
            return t[:Dl, :Dl]
        return t[:, :Dl]                                      # token tables, to_logits: [V, D]

    def _ref_shape(self, key: str) -> Tuple[int, ...]:
        """shape of the reference's tensor `key`"""
        v = self._view_for_key(key)
        if v.dim() == 4:
            return (v.shape[0] * v.shape[1] * v.shape[2], v.shape[3])
        if v.dim() == 3 and key.endswith("cross_attn.q.weight"):
            return (v.shape[0] * v.shape[1], v.shape[2])
        if v.dim() == 3:
            return (v.shape[0], v.shape[1] * v.shape[2])
        return tuple(v.shape)

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> List[str]:
        """Copies every known entry into the flat buffer; returns the keys this engine has no storage for (the module's
        `load_state_dict` reports them as unexpected / raises under strict=True)."""
        unexpected = []
        for key, val in sd.items():
            if self._is_buffer_key(key):
                continue
            side = key.split(".")
            foreign = ((side[0] == "decoder_embeddings" and side[1] not in self.logit_key) or
                       (side[0] == "encoder_embeddings" and f"encoder_embeddings.{side[1]}.mod_emb" not in self.p))
            if foreign or self._canon_key(key) not in self.p:           # (an embedding of the side this model has none on: no alias)
                unexpected.append(key)
                continue
            v = self._view_for_key(key)
            v.copy_(val.to(self.dev, F32).reshape(v.shape))        # (padded layouts: v is a strided view without the pads)
        self.weights_dirty = True
        return unexpected

    def state_dict(self) -> Dict[str, torch.Tensor]:
        out = {}
        cfg, D = self.cfg, self.Dl

        def ref(name):           # the reference's tensor: a view of the storage, or (padded layouts) a copy without the pads
            return self._view_for_key(name).reshape(self._ref_shape(name))

        enc_names, dec_names = {m.name for m in self.enc_mods}, {m.name for m in self.dec_mods}
        for m in self.mods:
            e, d = f"encoder_embeddings.{m.name}", f"decoder_embeddings.{m.name}"
            if m.name in enc_names:
                out[f"{e}.mod_emb"] = ref(f"{e}.mod_emb").view(1, 1, D)
                out[f"{e}.token_emb.weight"] = ref(f"{e}.token_emb.weight")
                out[f"{e}.pos_emb"] = ref(f"{e}.pos_emb")[None] if m.name in self.learned_enc else self.pos[m.name][None, :, :D]
            if m.name in dec_names:
                own = m.name in self.dec_own_mod_emb
                out[f"{d}.mod_emb"] = ref(f"{d}.mod_emb").view(1, 1, D) if own else out[f"{e}.mod_emb"]
                out[f"{d}.token_emb.weight"] = ref(f"{d}.token_emb.weight")
                out[f"{d}.to_logits.weight"] = ref(self.logit_key[m.name])
                out[f"{d}.pos_emb"] = ref(f"{d}.pos_emb")[None] if m.name in self.learned_dec else self.pos[m.name][None, :, :D]
        zeros = torch.zeros(D, device=self.dev)
        for name in self.p:
            if name.startswith(("encoder.", "decoder.", "encoder_norm", "decoder_norm", "decoder_proj_context")):
                out[name] = ref(name)
                if not self.norm_bias and (name.endswith("norm.weight") or ".norm" in name or "norm1" in name or "norm2" in name):
                    out[name[:-len("weight")] + "bias"] = zeros if out[name].numel() == D else torch.zeros_like(out[name])   # (head norms: [64])
        out["mask_token"] = ref("mask_token").view(1, 1, D)
        if self.R:
            out["register_tokens"] = ref("register_tokens").view(1, self.R, D)
        return out

    def _canon_key(self, key: str) -> str:
        """reference state-dict key -> engine storage key (shared mod_emb, tied to_logits)."""
        if key.startswith("decoder_embeddings") and key.endswith("mod_emb") and key.split(".")[1] not in self.dec_own_mod_emb:
            key = key.replace("decoder_embeddings", "encoder_embeddings")
        if key.endswith("to_logits.weight") and self.cfg.share_embedding:
            key = key.replace("to_logits.weight", "token_emb.weight")
        return key

    def param_views(self, key: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """(parameter, gradient) of the reference's tensor `key` as VIEWS of the flat buffers - what the nn.Module wrapper
        registers as nn.Parameter / .grad.  They have the reference's shape (mod_emb / mask_token: (1, 1, dim)) except, on a
        padded layout, the attention weights: there a head's rows are not contiguous with the next head's, so the views keep
        the head axis ((3, H, hd, dim) for qkv, (2, H, hd, dim) for kv, (H, hd, dim) for q, (dim, H, hd) for proj); element
        order = the reference's (`.reshape(reference shape)` gives its tensor)."""
        ck = self._canon_key(key)
        out = []
        for store in (self.p, self.g):
            v = self._logical(ck, store[ck])
            if v.dim() <= 2:
                shape = ((1, 1, self.Dl) if (ck.endswith("mod_emb") or ck == "mask_token") else
                         (1, self.R, self.Dl) if ck == "register_tokens" else
                         (1,) + self._ref_shape(ck) if ck.endswith("pos_emb") else self._ref_shape(ck))
                v = v.view(shape)
            out.append(v)
        return out[0], out[1]

    def grad_of(self, key: str) -> torch.Tensor:
        key = self._canon_key(key)
        return self._logical(key, self.g[key]).reshape(self._ref_shape(key))

    @torch.no_grad()
    def init_random(self, seed: int = 0):
        """Random init in the reference's distributions (egom2p_model.py:185-222), drawn on the device:
        xavier-uniform linears (qkv / kv as 3 / 2 matrices), N(0, 0.02) encoder tables / mod_emb / mask_token,
        LayerNorm weight 1.  The `to_logits` operand - the tied decoder table when `share_embedding` is set
        (decoder_embeddings.py:447-449: token_emb and to_logits are one tensor and the Linear is initialised last) -
        is xavier-uniform on its [V, D] shape."""
        gen = torch.Generator(device=self.dev)
        gen.manual_seed(seed)
        self.P.zero_()
        logit_keys = set(self.logit_key.values())
        for name in self.p:
            v = self._view_for_key(name)
            if name in logit_keys:
                a = math.sqrt(6.0 / (v.shape[0] + v.shape[1]))
                v.copy_((torch.rand(v.shape, device=self.dev, generator=gen) * 2 - 1) * a)
            elif name.endswith("token_emb.weight") or name.endswith("mod_emb") or name in ("mask_token", "register_tokens"):
                v.copy_(torch.randn(v.shape, device=self.dev, generator=gen) * 0.02)
            elif name.endswith("pos_emb"):
                pass                                      # (drawn below, behind every other draw: the stream of the others does not move)
            elif name.endswith(".bias"):
                v.zero_()                                 # (the biased family's own biases: drawn below, from their own generator)
            elif name.endswith("norm.weight") or ".norm" in name:
                v.fill_(1.0)
            else:
                fo, fi = self._ref_shape(name)
                if "qkv" in name: fo //= 3
                elif "kv" in name: fo //= 2
                a = math.sqrt(6.0 / (fo + fi))
                v.copy_((torch.rand(v.shape, device=self.dev, generator=gen) * 2 - 1) * a)
        # the biases of the biased family: NON-zero (the reference's init zeroes them - EgoM2P.init_weights does that - but a zero
        # bias hides a dead bias path from every test that starts here), from a generator of their own after all draws above, so
        # that the stream the other tensors see does not depend on the flags
        bgen = torch.Generator(device=self.dev)
        bgen.manual_seed(seed + 0x5EED)
        for name in self.p:
            if name.endswith(".bias") and name != "decoder_proj_context.bias":
                v = self._view_for_key(name)
                v.copy_(torch.randn(v.shape, device=self.dev, generator=bgen) * 0.05)
        # learned positional tables: N(0, 0.02) (encoder_embeddings.py:168-169), from a generator of their own
        pgen = torch.Generator(device=self.dev)
        pgen.manual_seed(seed + 0x905E)
        for name in self.p:
            if name.endswith("pos_emb"):
                v = self._view_for_key(name)
                v.copy_(torch.randn(v.shape, device=self.dev, generator=pgen) * 0.02)
        self.weights_dirty = True

    def param_names(self) -> List[str]:
        return list(self.p.keys())

    def num_params(self) -> int:
        n = 0
        for name, t in self.p.items():
            v = self._view_for_key(name)
            n += v.numel()
        return n

    def refresh_weights(self):
        """fp32 masters -> bf16 W and W^T copies (once per optimiser step; autocast re-casts per forward)."""
        for name, l in self.lin.items():
            ops.cast_weight(l.w, l.wb, l.wt)
            if l.w8 is not None:
                ops.quant_fp8_rows(l.wb, l.w8, l.s8)
            if l.wt8 is not None:
                ops.quant_fp8_rows(l.wt, l.wt8, l.st8)
        self.weights_dirty = False

    # ------------------------------------------------------------------------------------ workspaces
    def _compact_out(self, B, n_keep, train=False):
        """the buffers one ops.compact call fills for B samples of n_keep kept rows (seg_bad: the training decoder's row groups)"""
        i32 = dict(device=self.dev, dtype=I32)
        out = {k: torch.empty(B, n_keep, device=self.dev, dtype=dt) for k, dt in (
            ("ids_keep", torch.int64), ("pad", torch.uint8), ("mod_mask", torch.int16), ("slot", I32), ("local", I32), ("tok", I32),
            ("ks", I32), ("ke", I32))}
        out.update(n_valid=torch.zeros(B, **i32), seg=torch.empty(B, self.n_mods, 2, **i32), err=torch.zeros(1, **i32))
        if train:
            out["seg_bad"] = torch.zeros(B, **i32)
        return out

    def _hn_bufs(self, e, self_rows=0, q_rows=0, k_rows=0):
        """qk_norm: the normalised q / k of a layer's sites and their statistics - qkn [rows, 3A] = (q^ | k^ | unused) of self-attention
        with hst [(q mean, q rstd, k mean, k rstd), rows * H]; cross-attention: xqn [decoder rows, A], xkn [context rows, 2A] = (k^ |
        unused), hstq / hstk [(mean, rstd), rows * H].  The raw q / k stay in qkv / q / kv: the backward normalises from them.
        k^ keeps the pitch of the raw buffer because the attention kernels take K and V at ONE row stride (their LDS-DMA shares the
        lane offsets of the two slices: `check` in attention.hip); the slot beside it is address space only - never written or read."""
        if not self.qk_norm:
            return {}
        A, H = self.A, self.Hs
        out = dict(qkn=e(self_rows, 3 * A), hst=e(4, self_rows * H, dt=F32))
        if q_rows or k_rows:
            out.update(xqn=e(q_rows, A), hstq=e(2, q_rows * H, dt=F32), xkn=e(k_rows, 2 * A), hstk=e(2, k_rows * H, dt=F32))
        return out

    def _alloc_workspaces(self):
        B, N, M, D, A, Fp, H = self.Bmax, self.Ne, self.M, self.D, self.A, self.Fp, self.Hs      # N: encoder rows per sample (registers included)
        dev, cfg = self.dev, self.cfg
        RN, RM = B * N, B * M

        def e(*shape, dt=BF16):
            return torch.empty(*shape, device=dev, dtype=dt)

        self.ce, self.cd = self._compact_out(B, N, train=True), self._compact_out(B, M, train=True)
        self.zero_b = torch.zeros(B, device=dev, dtype=I32)
        self.emb_e = e(RN, D, dt=F32)
        self.perm = e(RM, dt=I32)
        self.tgt_perm = torch.zeros(RM, device=dev, dtype=I32)
        self.ranges = torch.zeros(self.n_mods, 2, device=dev, dtype=I32)
        self.perm_base = e(B, self.n_mods, dt=I32)
        self.canon = e(self.n_mods, dt=I32)

        def enc_layer():
            return dict(x=e(RN, D, dt=F32), xm=e(RN, D, dt=F32), ln1=e(RN, D), qkv=e(RN, 3 * A), ao=e(RN, A),
                        ao_lo=e(RN, A) if self.attn_o_residual == "all" else None,
                        lse=e(B, H, N, dt=F32), st1=e(2, RN, dt=F32), ln2=e(RN, D), ab=e(RN, self.Fab), h=e(RN, Fp),
                        st2=e(2, RN, dt=F32), **self._hn_bufs(e, self_rows=RN))

        def dec_layer():
            return dict(x=e(RM, D, dt=F32), x1=e(RM, D, dt=F32), x2=e(RM, D, dt=F32), ln1=e(RM, D), qkv=e(RM, 3 * A),
                        ao=e(RM, A), ao_lo=e(RM, A) if self.attn_o_residual == "all" else None, lse=e(B, H, M, dt=F32),
                        st1=e(2, RM, dt=F32), qn=e(RM, D), q=e(RM, A),
                        stq=e(2, RM, dt=F32), cn=e(RN, D), kv=e(RN, 2 * A), stc=e(2, RN, dt=F32), xo=e(RM, A),
                        xo_lo=e(RM, A) if self.attn_o_residual != "none" else None,
                        lse_x=e(B, H, M, dt=F32), ln2=e(RM, D), ab=e(RM, self.Fab), h=e(RM, Fp), st2=e(2, RM, dt=F32),
                        **self._hn_bufs(e, self_rows=RM, q_rows=RM, k_rows=RN))

        if self.act_checkpoint:
            # a layer keeps its input; everything else a block writes lives once per stack (enc_sh / dec_sh: a layer's buffers without
            # `x`) and is rebuilt from that input before the block's backward.  enc[i] / dec[i] stay the dictionaries the forward and
            # the backward index: the layer's own x beside the stack's shared buffers.
            self.enc_sh = {k: v for k, v in enc_layer().items() if k != "x"} if cfg.encoder_depth else {}
            self.dec_sh = {k: v for k, v in dec_layer().items() if k != "x"} if cfg.decoder_depth else {}
            self.enc = [dict(self.enc_sh, x=e(RN, D, dt=F32)) for _ in range(cfg.encoder_depth)]
            self.dec = [dict(self.dec_sh, x=e(RM, D, dt=F32)) for _ in range(cfg.decoder_depth)]
        else:
            self.enc_sh = self.dec_sh = None
            self.enc = [enc_layer() for _ in range(cfg.encoder_depth)]
            self.dec = [dec_layer() for _ in range(cfg.decoder_depth)]
        self.x_enc_out = e(RN, D, dt=F32)          # residual stream after the last encoder block
        self.st_en = e(2, RN, dt=F32)
        self.xe = e(RN, D)                         # encoder_norm output (bf16)
        self.ctx = e(RN, D, dt=F32)
        self.y_out = e(RM, D, dt=F32)
        self.st_dn = e(2, RM, dt=F32)
        self.yn = torch.zeros(RM, D, device=dev, dtype=BF16)     # decoder_norm output, modality-grouped rows
        vs = sorted({m.vocab_size for m in self.mods})
        self.logits = {v: e(RM, v) for v in vs}
        self.lse_ce = e(RM, dt=F32)
        self.nll = torch.zeros(RM, device=dev, dtype=F32)
        self.loss_out = torch.zeros(1 + self.n_mods, device=dev, dtype=F32)
        self.loss_w = torch.zeros(self.n_mods, device=dev, dtype=F32)      # loss_type 'weighted_mod' / 'token': per-modality weights
        self.loss_ms = torch.ones(self.n_mods, device=dev, dtype=F32)
        # backward temporaries
        R = max(RN, RM)
        self.dres = e(RM, D, dt=F32)               # decoder residual-stream gradient
        self.dres_b = e(RM, D)
        self.ring_b = [e(R, D) for _ in range(4)]   # rotating bf16 copies of the residual-stream gradient (wgrad operands)
        self._ring_i = 0
        self.t_d3 = e(R, D)
        self.dctx = e(RN, D, dt=F32)
        self.dctx_b = e(RN, D)
        self.st_ctx = e(2, RN, dt=F32)              # statistics of the context rows (one LayerNorm input for all decoder layers)
        self.dcn = None                             # per-layer gradients of the context_norm outputs (fused backward): allocated on first use
        self.dxe = e(RN, D, dt=F32)                # encoder residual-stream gradient
        self.dxe_b = e(RN, D)
        self.t_d = e(R, D)                         # generic [rows, D] bf16 temp
        self.t_d2 = e(R, D)
        # [rows, A] temps (gradients of attention outputs / queries): the same memory as t_d / t_d2 when A == D
        self.t_a, self.t_a2 = (self.t_d, self.t_d2) if A == D else (e(R, A), e(R, A))
        self.t_3d = e(R, 3 * A)
        self.t_2d = e(RN, 2 * A)
        self.t_f = e(R, Fp)
        self.t_2f = e(R, self.Fab)
        self.dyn = torch.zeros(RM, D, device=dev, dtype=BF16)
        self.delta = e(B, H, max(N, M), dt=F32)
        self.slab = e(64 * 1024 * 1024 // 4, dt=F32)   # 64 MiB of split-K partials (256 workgroups x 256 KiB)
        if self.fp8_forward or self.fp8_backward:      # e4m3 copy + row scales of the current GEMM input
            self.q8 = e(R, max(D, 3 * A, 2 * Fp), dt=torch.uint8)
            self.qs = e(R, dt=F32)
        self.gscale = torch.ones(1, device=dev, dtype=F32)
        if self.dp_sites:
            self.dp_kp = torch.tensor([kp for _, kp in self.dp_sites], dtype=F32).to(dev)
            self.dp_keep = torch.ones(len(self.dp_sites) * B, device=dev, dtype=torch.uint8)     # [n_sites, B of the forward] decisions
            self.dp_branch = e(R, D)          # a site's branch: the bf16 its last linear leaves in front of ego_droppath_resid
            self.dp_g = e(R, D)               # a site's scaled upstream gradient (ego_droppath_scale of the residual gradient)

    _BWD_TEMPS = ("dres", "dres_b", "ring_b", "t_d3", "dctx", "dctx_b", "dcn", "dxe", "dxe_b", "t_d", "t_d2", "t_a", "t_a2", "t_3d", "t_2d",
                  "t_f", "t_2f", "dyn", "delta", "slab", "dp_g")
    _FWD_OTHER = ("ce", "cd", "zero_b", "emb_e", "perm", "tgt_perm", "ranges", "perm_base", "canon", "x_enc_out", "st_en", "xe", "ctx", "y_out",
                  "st_dn", "yn", "logits", "lse_ce", "nll", "loss_out", "loss_w", "loss_ms", "st_ctx", "q8", "qs", "gscale", "dp_kp", "dp_keep",
                  "dp_branch")

    def workspace_bytes(self) -> Dict[str, int]:
        """Bytes of the training workspaces (`_alloc_workspaces`; `dcn` once the first backward made it), numel * element_size summed per
        class, every buffer once: `saved` - what the layers keep for the backward, per layer (under act_checkpoint their fp32 inputs);
        `shared` - the one block buffer set per stack of act_checkpoint (0 without); `other` - compaction, embeddings, context,
        logits, loss; `backward` - the backward's temporaries; `total`."""
        seen = set()

        def size(o):
            if isinstance(o, torch.Tensor):
                if o.data_ptr() in seen:
                    return 0
                seen.add(o.data_ptr())
                return o.numel() * o.element_size()
            if isinstance(o, dict):
                return sum(size(v) for v in o.values())
            if isinstance(o, (list, tuple)):
                return sum(size(v) for v in o)
            return 0

        out = dict(shared=size(self.enc_sh) + size(self.dec_sh))          # (first: a layer's dictionary names the shared buffers too)
        out["saved"] = size(self.enc) + size(self.dec)
        out["other"] = sum(size(getattr(self, k, None)) for k in self._FWD_OTHER)
        out["backward"] = sum(size(getattr(self, k, None)) for k in self._BWD_TEMPS)
        out["total"] = sum(out.values())
        return out

    # ------------------------------------------------------------------------------------ stochastic depth
    def set_drop_path_seed(self, seed: int, counter: int = 0):
        """The stream the drop-path decisions are drawn from: training forward number `counter` of stream `seed` draws, on the device,
        keep(site s, sample b) = top 24 bits of splitmix(splitmix(splitmix(seed, counter), s), b) < floor(keep_prob[s] * 2^24), and the
        counter advances by one per training forward (micro-batches of one step differ).  Ranks use seed + rank; a resumed run sets
        the counter to its loader-step position."""
        self._dp_seed, self._dp_counter = int(seed), int(counter)

    def inject_drop_path(self, encoder=None, decoder=None):
        """TEST HOOK: the keep tables of the NEXT training forward (and of its backward) instead of a draw - encoder bool [Le, 2, B]
        (attn, mlp), decoder bool [Ld, 3, B] (self_attn, cross_attn, mlp), True = the sample keeps the branch; a missing table keeps
        everything.  Entries of sites with rate 0 are ignored (those sites hold no drop path).  The forward counter does not advance."""
        self._dp_inject = (encoder, decoder)

    def drop_path_table(self) -> Optional[torch.Tensor]:
        """The decisions the last training forward used: uint8 [n_sites, B] in `dp_sites` order (a copy); None without one"""
        if not self.dp_sites or not self._dp_live:
            return None
        return self.dp_keep[:len(self.dp_sites) * self.B].view(len(self.dp_sites), self.B).clone()

    def _dp_begin(self, training: bool, B: int):
        """The decisions of the forward that starts: one ego_droppath_draw launch for all sites, or the injected tables"""
        self._dp_live = bool(training and self.dp_sites)
        inject, self._dp_inject = self._dp_inject, None
        if not self._dp_live:
            return
        n = len(self.dp_sites)
        if inject is not None:
            tab = torch.ones(n, B, dtype=torch.uint8)
            for kind, t, subs in (("encoder", inject[0], ("attn", "mlp")), ("decoder", inject[1], ("self_attn", "cross_attn", "mlp"))):
                if t is None:
                    continue
                t = torch.as_tensor(t).cpu()
                depth = self.cfg.encoder_depth if kind == "encoder" else self.cfg.decoder_depth
                if tuple(t.shape) != (depth, len(subs), B):
                    raise ValueError(f"inject_drop_path: the {kind} table must be [{depth}, {len(subs)}, {B}], not {tuple(t.shape)}")
                for i in range(depth):
                    for j, sub in enumerate(subs):
                        if f"{kind}.{i}.{sub}" in self._dp_ix:
                            tab[self._dp_ix[f"{kind}.{i}.{sub}"][0]] = t[i, j].to(torch.uint8)
            self.dp_keep[:n * B].copy_(tab.view(-1))
            self.dp_last = None
        else:
            ops.droppath_draw(self.dp_kp, self._dp_seed, self._dp_counter, self.dp_keep, B)
            self.dp_last = (self._dp_seed, self._dp_counter)
            self._dp_counter += 1

    def _dp(self, site: Optional[str]):
        """(the site's decisions [B], keep_prob) when the forward in flight / being differentiated drops paths at `site`, else None"""
        if site is None or not self._dp_live or site not in self._dp_ix:
            return None
        j, kp = self._dp_ix[site]
        return self.dp_keep[j * self.B:(j + 1) * self.B], kp

    def _resid_lin(self, name, A, x, out, rows, dp=None):
        """out = x + linear(A) over `rows` rows: the residual add at the end of a branch.  dp = (site, rows per sample) in the training
        forward: at a site that drops paths the linear leaves bf16 (its bias included: the reference scales the biased branch) and
        ego_droppath_resid adds the kept samples' branch / keep_prob"""
        d = self._dp(dp[0]) if dp is not None else None
        if d is None:
            self._lin_fwd(name, A, out, rows, L.EPI_RESID, R=x)
            return
        self._lin_fwd(name, A, self.dp_branch, rows)
        ops.droppath_resid(x, self.dp_branch, out, d[0], rows, dp[1], self.Dl, d[1])

    def _dp_grad(self, dres_b, rows, dp):
        """the upstream gradient of the branch at site dp = (site, rows per sample): the bf16 residual gradient itself or, where the
        forward dropped paths, ego_droppath_scale of it (everything inside the branch is linear in it: this is the whole backward)"""
        d = self._dp(dp[0]) if dp is not None else None
        if d is None:
            return dres_b
        ops.droppath_scale(dres_b, self.dp_g, d[0], rows, dp[1], self.Dl, d[1])
        return self.dp_g

    # ------------------------------------------------------------------------------------ small helpers
    def _ln(self, x, wname, y, st, out_row=None, q8=True):
        """LayerNorm forward (out_row: rows written permuted - decoder_norm); with the fp8 forward on, the row also leaves as
        e4m3 (+ scale) for the GEMM that follows (no separate quantisation pass for the LayerNorm-fed linears; q8=False: the
        consumer is no such linear)."""
        rows = x.shape[0]
        if q8 and self.fp8_forward and out_row is None and self.D % 128 == 0 and self.D >= 256:
            q = self._qbuf(rows, self.D)
            ops.layernorm_fwd(x, self.p[wname], y, st[0], st[1], eps=self.cfg.eps, q8=q, qscale=self.qs)
            self._q_of = (y.data_ptr(), rows, self.D)
        else:                         # (b: nn.LayerNorm's bias, a parameter with norm_bias only - never beside the fp8 forward)
            ops.layernorm_fwd(x, self.p[wname], y, st[0], st[1], out_row=out_row, eps=self.cfg.eps, width=self.Dl,
                              b=self.p.get(wname[:-len("weight")] + "bias"))

    def _qbuf(self, rows, K):
        if self.q8 is None or self.q8.shape[0] < rows or self.q8.shape[1] < K:
            self.q8 = torch.empty(rows, max(self.D, 3 * self.A, 2 * self.Fp), device=self.dev, dtype=torch.uint8)
            self.qs = torch.empty(rows, device=self.dev, dtype=F32)
        self._q_of = None
        return self.q8[:, :K]

    def _quant(self, A, rows, K):
        """e4m3 copy of the first `rows` rows of A (row scales in self.qs); the buffers are reused by the next GEMM input"""
        if self._q_of == (A.data_ptr(), rows, K):      # the LayerNorm that made A already left its e4m3 copy
            self._q_of = None
            return self.q8[:, :K]
        q = self._qbuf(rows, K)
        ops.quant_fp8_rows(A, q, self.qs, rows=rows, K=K)
        return q

    def _lin_fwd(self, name, A, C, rows, epi=L.EPI_BF16, R=None, bias=None):
        l = self.lin[name]
        if l.b is not None:
            # the linear's own bias: bf16(acc + bias) - qkv / q / kv / fc1 - or, in front of the residual add, proj / fc2
            epi, bias = {L.EPI_BF16: L.EPI_BIAS_BF16, L.EPI_RESID: L.EPI_BIAS_RESID}[epi], l.b
        if l.w8 is not None and rows > 0:
            q = self._quant(A, rows, l.in_f)
            ops.gemm_nt_fp8(q, self.qs, l.w8, l.s8, C, rows, l.out_f, l.in_f, epi, R=R, bias=bias)
            return
        ops.gemm_nt(A, l.wb, C, rows, l.out_f, l.in_f, epi, R=R, bias=bias, lda=A.shape[-1], ldb=l.in_f, ldc=C.shape[-1],
                    ldr=None if R is None else R.shape[-1])

    def _mlp_gate_fwd(self, pre, xn, ab, h, rows):
        """ab = fc1||fc3(xn), h = silu(a) * b - one launch where the shape allows it; the plain Mlp: ab = u = fc1(xn) (+ bias), the
        bf16 pre-activation the backward reads, h = gelu(u)"""
        if self.gelu:
            self._lin_fwd(f"{pre}.mlp.fc1.weight", xn, ab, rows)
            ops.gelu_fwd(ab, h, rows, self.Fp)
            return
        l = self.lin[f"{pre}.mlp.fc13"]
        if l.w8 is not None and rows > 0:
            q = self._quant(xn, rows, l.in_f)
            ops.gemm_nt_swiglu_fwd_fp8(q, self.qs, l.w8, l.s8, ab, h, rows, self.Fp, l.in_f)
            return
        if ops.swiglu_fwd_fusable(self.Fp, l.in_f) and rows >= self.SWIGLU_FWD_FUSED_ROWS:
            ops.gemm_nt_swiglu_fwd(xn, l.wb, ab, h, rows, self.Fp, l.in_f, ldx=xn.shape[-1], ldw=l.in_f)
        else:
            self._lin_fwd(f"{pre}.mlp.fc13", xn, ab, rows)
            ops.swiglu_fwd(ab, h, rows, self.Fp)

    def _lin_bwd(self, name, dY, X, dX, rows):
        """dX(bf16) = dY @ W ; dW += dY^T @ X ; with a bias of its own db += column sums of the bf16 dY."""
        l = self.lin[name]
        if l.gb is not None:
            ops.bias_grad(dY, rows, l.out_f, l.gb)
        if dX is not None and l.wt8 is not None and rows > 0:
            q = self._quant(dY, rows, l.out_f)               # e4m3 rows of dY + per-row scales (one pass over dY)
            ops.gemm_nt_fp8(q, self.qs, l.wt8, l.st8, dX, rows, l.in_f, l.out_f, L.EPI_BF16)
        elif dX is not None:
            ops.gemm_nt(dY, l.wt, dX, rows, l.in_f, l.out_f, L.EPI_BF16, lda=dY.shape[-1], ldb=l.out_f, ldc=dX.shape[-1])
        self._wgrad(l.g, dY, X, l.out_f, l.in_f, rows, ldp=dY.shape[-1], ldq=X.shape[-1])

    def _wgrad(self, G, dY, X, Ni, Nj, rows, ldp, ldq, m_range=None):
        """G[Ni,Nj] += dY^T X"""
        splits = ops.tn_splits(Ni, Nj, rows, self.slab.numel(), ranged=m_range is not None, ldp=ldp, ldq=ldq)
        ops.gemm_tn(dY, X, G, Ni, Nj, rows, m_range=m_range, splits=splits, slab=self.slab if splits > 1 else None,
                    ldp=ldp, ldq=ldq, ldc=Nj)

    def _qkv_packed(self, t, r0=0):
        """(q, k, v) of a [rows, 3A] qkv buffer (or its gradient), from row r0 on"""
        A = self.A
        return _Rows(t, r0 * 3 * A, 3 * A), _Rows(t, r0 * 3 * A + A, 3 * A), _Rows(t, r0 * 3 * A + 2 * A, 3 * A)

    def _q_kv(self, q_t, kv_t, r0=0, c0=0):
        """(q, k, v) of cross-attention: q [rows, A] from row r0 on against kv [context rows, 2A] from context row c0 on"""
        A = self.A
        return _Rows(q_t, r0 * A, A), _Rows(kv_t, c0 * 2 * A, 2 * A), _Rows(kv_t, c0 * 2 * A + A, 2 * A)

    # ---- qk_norm: q and k of an attention launch come from the normalised buffers, v from the raw one
    def _qkv_site(self, w, r0=0):
        """(q, k, v) of a self-attention site over the buffers w (a layer's, or a generation workspace), from row r0 on"""
        q, k, v = self._qkv_packed(w["qkv"], r0)
        if not self.qk_norm:
            return q, k, v
        A = self.A
        return _Rows(w["qkn"], r0 * 3 * A, 3 * A), _Rows(w["qkn"], r0 * 3 * A + A, 3 * A), v

    def _q_kv_site(self, w, kv_t, r0=0, c0=0):
        """(q, k, v) of a cross-attention site: q rows from r0 on against the context rows from c0 on (kv_t: the raw [context rows, 2A])"""
        q, k, v = self._q_kv(w["q"], kv_t, r0, c0)
        if not self.qk_norm:
            return q, k, v
        return _Rows(w["xqn"], r0 * self.A, self.A), _Rows(w["xkn"], c0 * 2 * self.A, 2 * self.A), v

    def _hn_self(self, pre, name, w, rows, grad=None):
        """q_norm / k_norm of a self-attention site over `rows` contiguous rows, one launch: qkv -> qkn (+ statistics); grad = the
        packed [rows, 3A] gradient: the backward, d q^ / d k^ -> d q / d k in place in its q and k slots, the weight gradients accumulated"""
        A, H = self.A, self.Hs
        q, k, _ = self._qkv_packed(w["qkv"])
        sites = []
        for j, (src, nm) in enumerate(((q, "q_norm"), (k, "k_norm"))):
            dst = _Rows(w["qkn"] if grad is None else grad, j * A, 3 * A)
            wn = f"{pre}.{name}.{nm}.weight"
            sites.append((*src.args(rows), *dst.args(rows), self.p[wn], w["hst"][2 * j], w["hst"][2 * j + 1]) + (() if grad is None else (self.g[wn],)))
        if grad is None:
            ops.headnorm_fwd(sites, 1, rows, H, eps=self.cfg.eps)
        else:
            ops.headnorm_bwd(sites, 1, rows, H)

    def _hn_one(self, wname, src, dst, st, rows, bwd=False):
        """one operand's head norm over `rows` contiguous rows (cross-attention: q and k have different row counts); bwd: dst holds the
        gradient, rewritten in place"""
        site = (*src.args(rows), *dst.args(rows), self.p[wname], st[0], st[1])
        if bwd:
            ops.headnorm_bwd([site + (self.g[wname],)], 1, rows, self.Hs)
        else:
            ops.headnorm_fwd([site], 1, rows, self.Hs, eps=self.cfg.eps)

    def _attn(self, qkv, o_t, lse, mask, B, Nq, Nk, o_lo=None, seg=None, seg_bad=None):
        """qkv: (q, k, v) `_Rows`; o_t [B * Nq, A] (o_lo: its bf16 rounding residual); mask: `_keys_per_sample` / `_keys_per_row`"""
        q, k, v = qkv
        ops.attn_fwd(*q.args(Nq), *k.args(Nk), *v.args(Nk), *_Rows(o_t, 0, self.A).args(Nq), lse, *mask,
                     B, self.Hs, Nq, Nk, self.scale, o_lo=None if o_lo is None else o_lo.data_ptr(), hd_pad=self.HDP,
                     seg=seg, seg_bad=seg_bad, hd=self.HD)

    # generation path: under-filled attention grids (1707 decoder rows x 12 heads = 168 workgroups on 256 CUs, each walking every
    # key tile serially: 26 - 47 us per launch) get their keys cut into runs (ego_attn_fwd_d64_split) until ~640 workgroups exist
    SPLIT_TARGET_WGS = 640
    # fc1||fc3 + gate in one launch from this many rows on: at 3414 rows - the paired decoder passes of a guided generation step - 29 us
    # against 35 for GEMM + gate pass; at 1707 rows the two launches win, 22 against 27: profiles/r05_gen_gemm_sweep_after.log
    SWIGLU_FWD_FUSED_ROWS = 3000
    SWIGLU_BWD_FUSED_ROWS = 4096        # fc2 dgrad + gate backward in one launch (_mlp_bwd) from this many rows on

    def _kv_splits(self, B, Nq, Nk):
        """Key runs per query tile of a generation-path attention launch (ego_attn_fwd_d64_split), from the measured table
        profiles/r05_gen_attn_split_sweep_before.log (one sample, 12 heads; us per launch unsplit / best split):
          168 workgroups (1707 queries): 1707 keys 28 / - (unsplit wins), 3414 keys 47 / 38 (3 runs), 8534 keys 105 / 67 (3 runs);
          324 (3414 x 3414): 66 / 62 (2 runs);  480, 648 (5120, 6827 rows): unsplit wins (99, 173 us: one full round of 768 slots);
          804 (8534 rows: 36 workgroups more than the 768 slots of one round): 299 / 275 (3 runs even out the tail).
        Round 4 split whenever fewer than 640 workgroups existed (1707 x 1707: 32 us against 28 unsplit)."""
        base = B * self.Hs * ((Nq + 127) // 128)
        if self.HDP != 64 or base <= 0 or not self.attn_split or Nk < 2048:
            return 1
        slots = 768                                           # three 4-wave workgroups per CU
        if base <= 200:
            s = 3
        elif base <= 400:
            s = 2
        elif slots < base <= slots + slots // 2:              # a short second round: cut every tile's keys so the rounds even out
            s = 3
        else:
            s = 1
        return max(1, min(s, ((Nk + 63) // 64) // 4))         # at least four 64-key tiles per run

    def _attn_infer(self, w, qkv, o_t, mask, B, Nq, Nk):
        """`_attn` of the generation passes: no LSE consumer, split keys when the grid is small"""
        sp = self._kv_splits(B, Nq, Nk)
        ws = w.get("att_ws")
        if sp > 1 and ws is not None and ws.numel() < ops.attn_fwd_split_floats(B, self.Hs, Nq, sp) and not torch.cuda.is_current_stream_capturing():
            ws = w["att_ws"] = torch.empty(ops.attn_fwd_split_floats(B, self.Hs, Nq, sp) + 4096, device=self.dev, dtype=F32)
        if sp > 1 and ws is not None and ws.numel() >= ops.attn_fwd_split_floats(B, self.Hs, Nq, sp):
            q, k, v = qkv
            ops.attn_fwd_split(*q.args(Nq), *k.args(Nk), *v.args(Nk), *_Rows(o_t, 0, self.A).args(Nq), w["lse"], *mask,
                               B, self.Hs, Nq, Nk, self.scale, sp, ws)
        else:
            self._attn(qkv, o_t, w["lse"], mask, B, Nq, Nk)

    def _dec_groups(self):
        """Row groups of the decoder's block-diagonal self-attention mask for the attention kernels (head dim 64): the
        compaction's (start, count) per modality slot + its per-sample "not the contract's mask" flags.  With them every
        attention workgroup sees one interval; EGOM2P_ATTN_GROUPS=0 keeps the per-row launches."""
        if self.HDP != 64 or not self.attn_groups or not self.sep_mask:      # (no separation: a row's keys are no modality segment)
            return {}
        # (the compaction packs (start, count) per PRESENT modality slot: [B, len(present), 2] at the front of the buffer.  A causal
        #  decoder goes through the same launch: ego_compact_causal raises seg_bad for every sample whose groups are not single rows,
        #  which sends it down the kernels' per-row interval class - forward, dQ and dK / dV)
        n = len(self.fmods)
        return dict(seg=self.cd["seg"].view(-1)[:self.B * n * 2].view(self.B, n, 2), seg_bad=self.cd["seg_bad"][:self.B])

    def _attn_bwd(self, qkv, o_t, do_t, lse, dqkv, mask, B, Nq, Nk, o_lo=None, seg=None, seg_bad=None):
        """the backward of `_attn(qkv, o_t, lse, mask, ...)`: do_t laid out like o_t, dqkv = (dq, dk, dv) laid out like qkv"""
        (q, k, v), (dq, dk, dv) = qkv, dqkv
        ops.attn_bwd(*q.args(Nq), *k.args(Nk), *v.args(Nk), *_Rows(o_t, 0, self.A).args(Nq), *_Rows(do_t, 0, self.A).args(Nq),
                     lse, self.delta, *dq.args(Nq), *dk.args(Nk), *dv.args(Nk), *mask, B, self.Hs, Nq, Nk, self.scale,
                     o_lo=None if o_lo is None else o_lo.data_ptr(), hd_pad=self.HDP, seg=seg, seg_bad=seg_bad, hd=self.HD)

    # ---- the two sub-layers every block has (Block.forward egom2p_utils.py:356-359, DecoderBlock.forward :387-391): the training
    # forward hands in each layer's saved buffers, the generation passes their shared ones
    def _attn_sublayer(self, pre, name, x, out, rows, ln, st, qkv, ao, attn, w=None, dp=None):
        """out = x + proj(attention(qkv(norm1(x)))) over `rows` rows; attn(): the site's attention launch(es), qkv -> ao
        (w: the buffers holding qkv - with qk_norm also qkn / hst, filled here: attn() then reads `_qkv_site(w)`; dp: the training
        forward's rows per sample - the site may drop paths, `_resid_lin`)"""
        self._ln(x[:rows], f"{pre}.norm1.weight", ln, st)
        self._lin_fwd(f"{pre}.{name}.qkv.weight", ln, qkv, rows)
        if self.qk_norm:
            self._hn_self(pre, name, w, rows)
        attn()
        self._resid_lin(f"{pre}.{name}.proj.weight", ao, x, out, rows, dp=None if dp is None else (f"{pre}.{name}", dp))

    def _mlp_sublayer(self, pre, x, out, rows, ln, st, ab, h, dp=None):
        """out = x + fc2(act(fc1(norm2(x)))) over `rows` rows"""
        self._ln(x[:rows], f"{pre}.norm2.weight", ln, st)
        self._mlp_gate_fwd(pre, ln, ab, h, rows)
        if out is None:           # a rebuild for the backward: the block's output is the next layer's saved input already
            return
        self._resid_lin(f"{pre}.mlp.fc2.weight", h, x, out, rows, dp=None if dp is None else (f"{pre}.mlp", dp))

    # ---- one block of the training forward over the buffers w (the layer's own or, under act_checkpoint, its x + the stack's shared
    # set).  out = the next layer's x; None: the backward's rebuild of the block from w["x"] - the same launches on the same operands
    # (masks, drop-path table and fp8 side buffers of the forward being differentiated) without the last residual GEMM, whose only
    # product is `out`.  A rebuild writes w's shared buffers, dp_branch and q8 / qs: nothing the backward holds live.
    def _enc_block(self, i, w, out):
        pre, B, N = f"encoder.{i}", self.B, self.Ne
        RN = B * N
        enc_keys = _keys_per_sample(self.zero_b, self.ce["n_valid"])        # the encoder rows as keys: self- and cross-attention
        # (key-padding mask: the per-row copies ce["ks"/"ke"] hold the same numbers as the per-sample interval)
        self._attn_sublayer(pre, "attn", w["x"], w["xm"], RN, w["ln1"], w["st1"], w["qkv"], w["ao"],
                            lambda: self._attn(self._qkv_site(w), w["ao"], w["lse"], enc_keys, B, N, N, o_lo=w["ao_lo"]), w=w, dp=N)
        self._mlp_sublayer(pre, w["xm"], out, RN, w["ln2"], w["st2"], w["ab"], w["h"], dp=N)

    def _dec_block(self, i, w, out, dec_keys, groups):
        pre, B, N, M, cfg = f"decoder.{i}", self.B, self.Ne, self.M, self.cfg
        RN, RM = B * N, B * M
        enc_keys = _keys_per_sample(self.zero_b, self.ce["n_valid"])
        self._attn_sublayer(pre, "self_attn", w["x"], w["x1"], RM, w["ln1"], w["st1"], w["qkv"], w["ao"],
                            lambda: self._attn(self._qkv_site(w), w["ao"], w["lse"], dec_keys, B, M, M, o_lo=w["ao_lo"], **groups), w=w, dp=M)
        self._ln(w["x1"][:RM], f"{pre}.query_norm.weight", w["qn"], w["stq"])
        self._lin_fwd(f"{pre}.cross_attn.q.weight", w["qn"], w["q"], RM)
        if not self.ctx_ln_fused:
            self._ln(self.ctx[:RN], f"{pre}.context_norm.weight", w["cn"], w["stc"])
        elif self.act_checkpoint:
            # the fused context LayerNorm would keep every layer's cn alive: under act_checkpoint the same kernel writes this layer's
            # alone (row-local: the bits of the all-layer launch).  The forward leaves the statistics where the fused backward reads
            # them - every layer writes the same values - a rebuild in the shared set
            st = self.st_ctx if out is not None else w["stc"]
            ops.layernorm_fwd_multi(self.ctx[:RN], [self.p[f"{pre}.context_norm.weight"]], [w["cn"]], st[0], st[1], eps=cfg.eps, width=self.Dl)
        self._lin_fwd(f"{pre}.cross_attn.kv.weight", w["cn"], w["kv"], RN)
        if self.qk_norm:
            self._hn_one(f"{pre}.cross_attn.q_norm.weight", _Rows(w["q"], 0, self.A), _Rows(w["xqn"], 0, self.A), w["hstq"], RM)
            self._hn_one(f"{pre}.cross_attn.k_norm.weight", _Rows(w["kv"], 0, 2 * self.A), _Rows(w["xkn"], 0, 2 * self.A), w["hstk"], RN)
        self._attn(self._q_kv_site(w, w["kv"]), w["xo"], w["lse_x"], enc_keys, B, M, N, o_lo=w["xo_lo"])
        self._resid_lin(f"{pre}.cross_attn.proj.weight", w["xo"], w["x1"], w["x2"], RM, dp=(f"{pre}.cross_attn", M))
        self._mlp_sublayer(pre, w["x2"], out, RM, w["ln2"], w["st2"], w["ab"], w["h"], dp=M)

    # ------------------------------------------------------------------------------------ forward
    def forward(self, mod_dict: Dict[str, Dict[str, torch.Tensor]], dec_order: Optional[Sequence[str]] = None,
                need_loss: bool = True, group_rows: bool = True, loss_grad=None, loss_type: str = "mod", training: bool = False):
        """Forward of one micro-batch (tensors already on the device).  Returns (loss, {mod: loss}) as
        views of a device buffer: reading them is the only host sync.
        loss_grad (float or 1-element device tensor, optional): the upstream d loss the following `backward` will be
        called with.  A training step knows it when the loss is formed, and the cross-entropy then runs forward and
        backward in ONE pass over the logits (`ego_ce_fwd_bwd`: bitwise the two-call result, the 16.5 GB of logits of a
        64-clip micro-batch are read once instead of twice); `backward` must then be given the same value.
        loss_type: 'mod' (forward_mod_loss, egom2p_model.py:614-644), 'weighted_mod' (:583-612) or 'token' (:646-681); the two
        others weight the modalities' mean cross-entropies by device-side weights (`ego_loss_weights`), forward and backward.
        training: a training-mode forward (`model.training and torch.is_grad_enabled()`): the sites of a model with drop path draw
        their per-sample decisions and the following `backward` differentiates that forward; False (default): no path is dropped."""
        if loss_type not in ops.LOSS_MODES:
            raise ValueError("Invalid loss type")                  # the reference's message (egom2p_model.py:579)
        self._loss_mode = ops.LOSS_MODES[loss_type]
        if self.weights_dirty:
            self.refresh_weights()
        cfg, D, N, M = self.cfg, self.D, self.Ne, self.M      # N: encoder rows per sample (registers included)
        # the modalities of this micro-batch: the configured ones present in mod_dict, in configuration order (the reference takes
        # whatever is there, egom2p_model.py:706-714); slots, loss rows and the loss mean run over these
        unknown = [k for k in mod_dict if k not in {m.name for m in self.mods}]
        if unknown:
            raise KeyError(f"not a configured modality: {unknown}")
        # the encoder takes the entries that are encoder modalities, the decoder (and the loss) those that are decoder modalities
        # (egom2p_model.py:706-714: each side walks the mod_dict keys it has an embedding for); a symmetric model: one list
        emods = [m for m in self.enc_mods if m.name in mod_dict]
        mods = [m for m in self.dec_mods if m.name in mod_dict]
        if not emods or not mods:
            raise ValueError("mod_dict holds no modality" if not (emods or mods) else
                             "mod_dict holds no encoder modality" if not emods else "mod_dict holds no decoder modality")
        self.fmods, self.femods, n_mods = mods, emods, len(mods)
        B = mod_dict[mods[0].name]["input_mask"].shape[0]
        if B > self.Bmax:
            raise L.EgoHipError(f"batch {B} exceeds the engine's workspace batch {self.Bmax}")
        self.B = B
        self._dp_begin(training, B)
        RN, RM = B * N, B * M
        byname = {m.name: m for m in mods}
        dmods = [byname[n] for n in (dec_order or [m.name for m in mods])]      # (dec_order names decoder modalities of the batch)
        self.dmods = dmods

        def flat_ids(m):
            t = mod_dict[m.name]["tensor"]
            return t.reshape(B, -1).contiguous()

        # ---- compaction + embeddings (egom2p_model.py:706-718, 723)
        ce, cd = self.ce, self.cd
        ops.compact([mod_dict[m.name]["input_mask"] for m in emods], [flat_ids(m) for m in emods], None,
                    [m.max_tokens for m in emods], [m.id for m in emods], self.N, False, ce, B, n_reg=self.R)
        ops.compact([mod_dict[m.name]["target_mask"] for m in dmods], [flat_ids(m) for m in dmods],
                    [mod_dict[m.name]["decoder_attention_mask"] for m in dmods],
                    [m.max_tokens for m in dmods], [m.id for m in dmods], M, True, cd, B, causal=bool(cfg.decoder_causal_mask),
                    sep=self.sep_mask)
        x0 = self.enc[0]["x"] if cfg.encoder_depth else self.x_enc_out
        ops.embed_fwd([self.p[f"encoder_embeddings.{m.name}.token_emb.weight"] for m in emods],
                      [self.pos_enc[m.name] for m in emods], [self.p[f"encoder_embeddings.{m.name}.mod_emb"] for m in emods],
                      None, ce["slot"], ce["local"], ce["tok"], x0, self.emb_e, RN, D, reg=self.p["register_tokens"] if self.R else None)
        y0 = self.dec[0]["x"] if cfg.decoder_depth else self.y_out
        ops.embed_fwd(None, [self.pos_dec[m.name] for m in dmods], [self.p[self.dec_mod_emb_key[m.name]] for m in dmods],
                      self.p["mask_token"], cd["slot"], cd["local"], cd["tok"], y0, None, RM, D)
        ckey = tuple(m.name for m in dmods)
        if ckey not in self._canon_dev:              # one small H2D copy per decoder order, ever (never inside a graph capture)
            self._canon_dev[ckey] = torch.tensor([mods.index(m) for m in dmods], dtype=I32).to(self.dev)
        self.canon[:n_mods].copy_(self._canon_dev[ckey])
        ops.loss_perm(cd["seg"], self.canon, cd["slot"], cd["tok"], B, M, n_mods, self.perm, self.tgt_perm,
                      self.ranges, self.perm_base)

        # ---- encoder (egom2p_model.py:496-499)
        for i, w in enumerate(self.enc):
            self._enc_block(i, w, self.enc[i + 1]["x"] if i + 1 < cfg.encoder_depth else self.x_enc_out)
        self._ln(self.x_enc_out[:RN], "encoder_norm.weight", self.xe, self.st_en)
        # context = decoder_proj_context(x) + encoder_emb   (egom2p_model.py:722)
        self._lin_fwd("decoder_proj_context.weight", self.xe, self.ctx, RN, L.EPI_BIAS_RESID, R=self.emb_e,
                      bias=self.p["decoder_proj_context.bias"])

        # ---- decoder (egom2p_model.py:520-523)
        dec_keys, groups = _keys_per_row(cd["ks"], cd["ke"], M), self._dec_groups()
        if self.ctx_ln_fused and not self.act_checkpoint:
            ops.layernorm_fwd_multi(self.ctx[:RN], [self.p[f"decoder.{i}.context_norm.weight"] for i in range(cfg.decoder_depth)],
                                    [w["cn"] for w in self.dec], self.st_ctx[0], self.st_ctx[1], eps=cfg.eps, width=self.Dl)
        for i, w in enumerate(self.dec):
            self._dec_block(i, w, self.dec[i + 1]["x"] if i + 1 < cfg.decoder_depth else self.y_out, dec_keys, groups)
        # decoder_norm, rows written modality-grouped (the row order of y[decoder_mod_mask == id], :633)
        self._ln(self.y_out[:RM], "decoder_norm.weight", self.yn, self.st_dn, out_row=self.perm if group_rows else None, q8=False)
        self._have_fwd = True
        if not need_loss:
            return None

        # ---- per-modality logits + CE (forward_mod_loss, egom2p_model.py:614-644)
        self._ce_done, self._ce_grad = set(), loss_grad
        if loss_grad is not None:
            self._set_gscale(loss_grad)
        lw = ms = None
        if self._loss_mode:
            lw, ms = self.loss_w, self.loss_ms
            ops.loss_weights(self.ranges, [m.vocab_size for m in mods], self._loss_mode, lw, ms)
        for c, m in enumerate(mods):
            l = self.lin[self.logit_key[m.name]]
            ub = min(RM, B * m.max_tokens)
            lg = self.logits[m.vocab_size]
            ops.gemm_nt(self.yn, l.wb, lg, ub, m.vocab_size, D, L.EPI_BF16, m_range=self.ranges[c], lda=D, ldb=D, ldc=m.vocab_size)
            if loss_grad is not None and ops.ce_fusable(m.vocab_size):
                ops.ce_fwd_bwd(lg, m.vocab_size, m.vocab_size, self.tgt_perm, self.ranges[c], ub, self.lse_ce, self.nll, self.gscale,
                               n_mods, loss_w=None if lw is None else lw[c:c + 1])
                self._ce_done.add(c)
            else:
                ops.ce_fwd(lg, m.vocab_size, m.vocab_size, self.tgt_perm, self.ranges[c], ub, self.lse_ce, self.nll)
        # a decoder_attention_mask that is not one interval per row (compaction flag) turns the loss into NaN
        ops.loss_finalize(self.nll, self.ranges, n_mods, self.loss_out, err=cd["err"], loss_w=lw, mod_scale=ms)
        return self.loss_out[0], {m.name: self.loss_out[1 + c] for c, m in enumerate(mods)}

    # ------------------------------------------------------------------------------------ backward
    def _mlp_bwd(self, pre, w, dres, dres_b, rows, xin, rps):
        """residual-stream gradient through x + fc2(swiglu(fc13(LN2(x)))); xin = LN2 input (saved); rps: rows per sample."""
        Fp = self.Fp
        dres_b = self._dp_grad(dres_b, rows, (f"{pre}.mlp", rps))
        dh, dab, dln = self.t_f, self.t_2f, self.t_d
        l2 = self.lin[f"{pre}.mlp.fc2.weight"]
        if self.gelu:
            # plain Mlp: dh = dY W2, du = dh * gelu'(u) on the stored bf16 pre-activation, then fc1 (their bias gradients: _lin_bwd)
            self._lin_bwd(f"{pre}.mlp.fc2.weight", dres_b, w["h"], dh, rows)
            ops.gelu_bwd(w["ab"], dh, dab, rows, Fp)
        elif ops.swiglu_bwd_fusable(Fp, l2.out_f) and rows >= self.SWIGLU_BWD_FUSED_ROWS:
            # fc2 dgrad and the gate backward in one launch (dh never reaches HBM), then the fc2 wgrad
            ops.gemm_nt_swiglu_bwd(dres_b, l2.wt, w["ab"], dab, rows, Fp, l2.out_f, ldy=dres_b.shape[-1], ldw=l2.out_f)
            self._wgrad(l2.g, dres_b, w["h"], l2.out_f, l2.in_f, rows, ldp=dres_b.shape[-1], ldq=w["h"].shape[-1])
        else:
            self._lin_bwd(f"{pre}.mlp.fc2.weight", dres_b, w["h"], dh, rows)
            ops.swiglu_bwd(w["ab"], dh, dab, rows, Fp)
        self._lin_bwd(f"{pre}.mlp.fc1.weight" if self.gelu else f"{pre}.mlp.fc13", dab, w["ln2"], dln, rows)
        nb = self._ring_next()
        self._ln_bwd(dln, xin[:rows], f"{pre}.norm2.weight", w["st2"], dres, dx_in=dres, dx_bf16=nb)
        return nb

    def _self_attn_bwd(self, pre, attn_name, w, dres, dres_b, rows, Nq, mask, groups=None):
        dao, dqkv, dln = self.t_a, self.t_3d, self.t_d2
        dres_b = self._dp_grad(dres_b, rows, (f"{pre}.{attn_name}", Nq))
        self._lin_bwd(f"{pre}.{attn_name}.proj.weight", dres_b, w["ao"], dao, rows)
        self._attn_bwd(self._qkv_site(w), w["ao"], dao, w["lse"], self._qkv_packed(dqkv), mask, self.B, Nq, Nq,
                       o_lo=w["ao_lo"], **(groups or {}))
        if self.qk_norm:          # d q^ / d k^ -> d q / d k in place (v's slot is not touched), q_norm / k_norm weight gradients
            self._hn_self(pre, attn_name, w, rows, grad=dqkv)
        self._lin_bwd(f"{pre}.{attn_name}.qkv.weight", dqkv, w["ln1"], dln, rows)
        nb = self._ring_next()
        self._ln_bwd(dln, w["x"][:rows], f"{pre}.norm1.weight", w["st1"], dres, dx_in=dres, dx_bf16=nb)
        return nb

    def _set_gscale(self, gscale):
        if isinstance(gscale, torch.Tensor):
            self.gscale.copy_(gscale.reshape(1).to(F32))
        else:
            self.gscale.fill_(float(gscale))

    def backward(self, gscale=1.0, bucket_done: Optional[Callable[[str, int, int], None]] = None):
        """Backward of the last forward; gradients are ACCUMULATED into the flat grad buffer scaled by
        `gscale` (float or 1-element device tensor: the upstream d loss).  `bucket_done(name, lo, hi)` is
        called (in launch order) as soon as every kernel writing G[lo:hi] has been enqueued."""
        assert self._have_fwd, "backward() needs a forward()"
        cfg, D, N, M, B = self.cfg, self.D, self.Ne, self.M, self.B       # N: encoder rows per sample (registers included)
        RN, RM = B * N, B * M
        mods, emods, ce, cd = self.fmods, self.femods, self.ce, self.cd     # the decoder / encoder modalities of the forward (absent ones: no kernel writes their gradients)
        if self._ce_done:
            # the forward already turned the logits into d logits with the upstream gradient it was promised
            same = (gscale is self._ce_grad) or (not isinstance(gscale, torch.Tensor) and not isinstance(self._ce_grad, torch.Tensor)
                                                 and float(gscale) == float(self._ce_grad))
            if not same:
                raise L.EgoHipError("backward(gscale) differs from the loss_grad the forward was given")
        else:
            self._set_gscale(gscale)
        bmap = {n: (lo, hi) for n, lo, hi in self.buckets}
        enc_keys = _keys_per_sample(self.zero_b, ce["n_valid"])             # the encoder rows as keys: self- and cross-attention

        def done(name):
            if bucket_done is not None:
                lo, hi = bmap[name]
                bucket_done(name, lo, hi)

        # ---- loss head: d logits in place, d yn, d table (tied to_logits/token_emb)
        for c, m in enumerate(mods):
            l = self.lin[self.logit_key[m.name]]
            ub = min(RM, B * m.max_tokens)
            V = m.vocab_size
            lg = self.logits[V]
            if c not in self._ce_done:
                ops.ce_bwd(lg, V, V, self.tgt_perm, self.ranges[c], ub, self.lse_ce, self.gscale, len(mods),
                           loss_w=self.loss_w[c:c + 1] if self._loss_mode else None)
            ops.gemm_nt(lg, l.wt, self.dyn, ub, D, V, L.EPI_BF16, m_range=self.ranges[c], lda=V, ldb=V, ldc=D)
            self._wgrad(l.g, lg, self.yn, V, D, ub, ldp=V, ldq=D, m_range=self.ranges[c])
        for m in reversed(self.dec_mods):                      # (every bucket is handed over, an absent modality's with zeros)
            done(f"dec_table.{m.name}" if cfg.share_embedding else f"to_logits.{m.name}")
        dres, dres_b = self.dres, self._ring_next()
        ops.layernorm_bwd(self.dyn, self.y_out[:RM], self.st_dn[0], self.st_dn[1], self.p["decoder_norm.weight"], dres,
                          self.g["decoder_norm.weight"], dx_in=None, dx_bf16=dres_b, dy_row=self.perm, width=self.Dl,
                          db=self.g.get("decoder_norm.bias"))

        # ---- decoder layers
        first_ctx = True
        fused = self.ctx_ln_fused
        dec_keys, groups = _keys_per_row(cd["ks"], cd["ke"], M), self._dec_groups()
        if fused and self.dcn is None:
            self.dcn = [torch.empty(self.Bmax * N, D, device=self.dev, dtype=BF16) for _ in range(cfg.decoder_depth)]
        for i in reversed(range(cfg.decoder_depth)):
            w, pre = self.dec[i], f"decoder.{i}"
            if self.act_checkpoint and i + 1 < cfg.decoder_depth:      # (the forward left the stack's last block in the shared set)
                self._dec_block(i, w, None, dec_keys, groups)
            dres_b = self._mlp_bwd(pre, w, dres, dres_b, RM, w["x2"], M)
            # cross attention
            dxo, dq, dkv, dln = self.t_a, self.t_a2, self.t_2d, self.t_d
            self._lin_bwd(f"{pre}.cross_attn.proj.weight", self._dp_grad(dres_b, RM, (f"{pre}.cross_attn", M)), w["xo"], dxo, RM)
            self._attn_bwd(self._q_kv_site(w, w["kv"]), w["xo"], dxo, w["lse_x"], self._q_kv(dq, dkv), enc_keys, B, M, N, o_lo=w["xo_lo"])
            if self.qk_norm:
                self._hn_one(f"{pre}.cross_attn.q_norm.weight", _Rows(w["q"], 0, self.A), _Rows(dq, 0, self.A), w["hstq"], RM, bwd=True)
                self._hn_one(f"{pre}.cross_attn.k_norm.weight", _Rows(w["kv"], 0, 2 * self.A), _Rows(dkv, 0, 2 * self.A), w["hstk"], RN, bwd=True)
            self._lin_bwd(f"{pre}.cross_attn.q.weight", dq, w["qn"], dln, RM)
            nb = self._ring_next()
            self._ln_bwd(dln, w["x1"][:RM], f"{pre}.query_norm.weight", w["stq"], dres, dx_in=dres, dx_bf16=nb)
            dres_b = nb
            dcn = self.dcn[i] if fused else self.t_d3    # t_d3 and not t_d2: kept so that buffer use and results stay what they were
            self._lin_bwd(f"{pre}.cross_attn.kv.weight", dkv, w["cn"], dcn, RN)
            if not fused:
                self._ln_bwd(dcn, self.ctx[:RN], f"{pre}.context_norm.weight", w["stc"], self.dctx, dx_in=None if first_ctx else self.dctx)
            first_ctx = False
            dres_b = self._self_attn_bwd(pre, "self_attn", w, dres, dres_b, RM, M, dec_keys, groups=groups)
            done(pre)                 # (the layer's context_norm weight is not in this bucket: "ctx_norms")
        if cfg.decoder_depth == 0:
            self.dctx[:RN].zero_()
        elif fused:
            # all layers' context_norm backward in one launch: the context and its statistics are read once, the context gradient
            # is written once (fp32 + the bf16 copy the context projection's backward reads) - summed in the chained launches'
            # order, bit for bit their result; the layers' own gradient buckets went out layer by layer, only the small
            # "ctx_norms" bucket (one weight vector per layer) is completed here
            Ld = cfg.decoder_depth
            ops.layernorm_bwd_multi([self.dcn[i][:RN] for i in range(Ld)], self.ctx[:RN], self.st_ctx[0], self.st_ctx[1],
                                    [self.p[f"decoder.{i}.context_norm.weight"] for i in range(Ld)], self.dctx[:RN],
                                    [self.g[f"decoder.{i}.context_norm.weight"] for i in range(Ld)], dx_bf16=self.dctx_b[:RN], width=self.Dl)
        if cfg.decoder_depth:
            done("ctx_norms")
        # decoder input embeddings: mask token + (pos + mod_emb)
        dmods = self.dmods
        ops.embed_bwd(None, [self.g[self.dec_mod_emb_key[m.name]] for m in dmods], self.g["mask_token"],
                      dres, None, cd["slot"], cd["tok"], RM, D)
        self._pos_grad("decoder", dmods, dres, None, cd, RM, M, B)
        done("head")

        # ---- context projection + encoder_norm
        if not (fused and cfg.decoder_depth > 0):
            ops.cast_f32_bf16(self.dctx[:RN], self.dctx_b)
        ops.bias_grad(self.dctx_b, RN, D, self.g["decoder_proj_context.bias"])
        dxe_n = self.t_d
        self._lin_bwd("decoder_proj_context.weight", self.dctx_b, self.xe, dxe_n, RN)
        dxe, dxe_b = self.dxe, self._ring_next()
        self._ln_bwd(dxe_n, self.x_enc_out[:RN], "encoder_norm.weight", self.st_en, dxe, dx_in=None, dx_bf16=dxe_b)
        done("bridge")

        # ---- encoder layers
        for i in reversed(range(cfg.encoder_depth)):
            w, pre = self.enc[i], f"encoder.{i}"
            if self.act_checkpoint and i + 1 < cfg.encoder_depth:
                self._enc_block(i, w, None)
            dxe_b = self._mlp_bwd(pre, w, dxe, dxe_b, RN, w["xm"], N)
            dxe_b = self._self_attn_bwd(pre, "attn", w, dxe, dxe_b, RN, N, enc_keys)
            done(pre)
        # encoder input embeddings: token rows, mod_emb (emb is used twice: x = tok + emb and context += emb)
        ops.embed_bwd([self.g[f"encoder_embeddings.{m.name}.token_emb.weight"] for m in emods],
                      [self.g[f"encoder_embeddings.{m.name}.mod_emb"] for m in emods], None, dxe, self.dctx,
                      ce["slot"], ce["tok"], RN, D,
                      touched=None if self.touched is None else [self.touched[self.enc_mods.index(m)] for m in emods])
        self._pos_grad("encoder", emods, dxe, self.dctx, ce, RN, N, B)
        if self.R:        # d register_tokens = the encoder input gradient of the register rows, summed over the batch (emb is 0 there)
            ops.reg_grad(dxe, B, N, self.R, D, self.g["register_tokens"])
        done("mod_emb")
        for m in reversed(self.enc_mods):
            done(f"enc_table.{m.name}")
        if self.learned_enc or self.learned_dec:
            done("pos_emb")           # (behind every other parameter in the flat buffer, final last: a bucket of its own)
        self._have_fwd = False
        self._ce_done = set()

    def _pos_grad(self, side, mods, dx, d2, c, rows, rows_per_sample, B):
        """Gradient of the learned positional tables of one side (mods: the side's modalities in slot order): the rows' dx (and, on the
        encoder side, the gradient d2 of the `emb` added back onto the projected context, egom2p_model.py:722) summed per position
        over the batch, accumulated into G.  A side without a learned table among `mods` launches nothing.
        Rows that break the kernel's contract (one position twice in a sample, a position outside its table - ego_compact writes neither)
        raise the DECODER compaction's error word, for either side: nothing clears it until the next forward's `loss_finalize`, which
        then returns NaN losses and clears it - the stop the reference's non-finite-loss exit gives a wrong attention mask."""
        learned = self.learned_enc if side == "encoder" else self.learned_dec
        if not any(m.name in learned for m in mods):
            return
        ops.posemb_grad([self.g[f"{side}_embeddings.{m.name}.pos_emb"] if m.name in learned else m.max_tokens for m in mods],
                        dx, d2, c["slot"], c["local"], rows, rows_per_sample, B, self.Dl, self.cd["err"], accumulate=True, ld=self.D)

    def zero_grad(self):
        self.G.zero_()

    def track_touched_table_rows(self, on: bool = True):
        """Let the embedding backward flag every encoder-table row that receives a gradient (uint8 [V] per table,
        accumulated over micro-batches, consumed and cleared by dp.SparseTableExchange).  Returns
        [(gradient view [V, D], flags)] for the encoder tables, in modality order."""
        if not on:
            self.touched = None
            return []
        self.touched = [torch.zeros(m.vocab_size, device=self.dev, dtype=torch.uint8) for m in self.enc_mods]
        return [(self.g[f"encoder_embeddings.{m.name}.token_emb.weight"], self.touched[i]) for i, m in enumerate(self.enc_mods)]

    def resize_workspaces(self, max_batch: int, n_enc: int, n_dec: int):
        """Re-allocate the activation workspaces for another (batch, N, M); parameters are untouched."""
        self.Bmax, self.N, self.M = max_batch, n_enc, n_dec
        self.Ne = self.N + self.R
        self._alloc_workspaces()
        self._have_fwd = False
        self.drop_graphs()

    def drop_graphs(self):
        """Forget every captured generation graph (and the workspace it owns).  A hipGraph bakes device addresses in: it
        is only valid while the buffers it was captured against are alive, so anything that re-allocates engine memory
        calls this.  (Round 1 hit exactly that: a graph captured against a shared inference workspace replayed after a
        larger pass had re-allocated it -> GPU memory access fault; since then each graph owns its workspace.)"""
        self.__dict__.pop("_graphs", None)
        self._iw, self._infer_key = None, None

    # ------------------------------------------------------------------------------------ generation (config 4)
    def _alloc_infer(self, B: int, Nmax: int, Mmax: int, fresh: bool = False, groups: int = 1):
        """One set of buffers (nothing is saved for a backward) for encoder-decoder passes of the ROAR / CFG
        generation path, sized for up to Nmax encoder rows and Mmax decoder rows per sample.  groups = 2: the conditional
        and the unconditional pass of one guided step share ONE decoder pass (`infer_logits_cfg`) - decoder buffers hold
        2 B samples, context buffers the two contexts one after the other."""
        G = int(groups)
        key = (G, B, Nmax, Mmax)
        if not fresh and self._infer_key is not None and self._infer_key[0] >= G and all(a >= b for a, b in zip(self._infer_key[1:], key[1:])):
            return self._iw
        D, A, Fp, H, dev = self.D, self.A, self.Fp, self.Hs, self.dev
        RE, RD, RC = G * B * Nmax, G * B * Mmax, G * B * Nmax     # encoder rows (all groups, back to back), decoder rows, context rows
        R = max(RE, RD)

        def e(*shape, dt=BF16):
            return torch.empty(*shape, device=dev, dtype=dt)

        w = dict(
            groups=G, sides=[self._compact_out(B, Nmax) for _ in range(G)],
            xa=e(RE, D, dt=F32), xb=e(RE, D, dt=F32), emb=e(RE, D, dt=F32), ctx=e(RC, D, dt=F32),
            ya=e(RD, D, dt=F32), yb=e(RD, D, dt=F32),
            ln=e(max(R, RC), D), qkv=e(R, 3 * A), ao=e(R, A), ab=e(R, self.Fab), h=e(R, Fp), q=e(RD, A), cn=e(RC, D),
            kv=e(RC, 2 * A), st=e(2, max(R, RC), dt=F32), lse=e(G * B, H, max(Nmax, Mmax), dt=F32),
            zero_b=torch.zeros(G * B, device=dev, dtype=I32), full_m=torch.zeros(G * B, device=dev, dtype=I32),
            dslot=torch.zeros(RD, device=dev, dtype=I32), dtok=torch.zeros(RD, device=dev, dtype=I32),
        )
        w["side"] = w["sides"][0]
        w.update(self._hn_bufs(e, self_rows=R, q_rows=RD, k_rows=RC))      # qk_norm: normalised q / k of the pass's sites
        # every decoder layer's context_norm output from one pass over the context (ego_layernorm_fwd_multi)
        w["cns"] = [e(RC, D) for _ in range(self.cfg.decoder_depth)] if self.ctx_ln_fused else None
        # scratch of the split-key attention launches: splits x B x H x ceil(Nq / 128) <= SPLIT_TARGET_WGS bounds it
        # (sized for the largest split launch this workspace can see: an encoder group's self-attention, the decoder's self-attention
        #  over all groups, one group's cross-attention - whatever _kv_splits would split; shorter passes through the same buffers
        #  split less or not at all)
        need = 0
        if self.HDP == 64 and self.attn_split:
            for b_, nq, nk in ((B, Nmax, Nmax), (G * B, Mmax, Mmax), (B, Mmax, Nmax)):
                for nq_ in {nq, max(1, nq // 2), max(1, nq // 4)}:          # (the split rule is not monotonic in the row count)
                    sp_ = max(self._kv_splits(b_, nq_, nk), self._kv_splits(b_, nq_, max(1, nk // 2)))
                    if sp_ > 1:
                        need = max(need, int(ops.attn_fwd_split_floats(b_, H, nq_, sp_)))
        w["att_ws"] = e(need + 4096, dt=F32) if (self.HDP == 64 and self.attn_split) else None
        if not fresh:
            self._iw, self._infer_key = w, key
        return w

    def _infer_context(self, w, parts, B: int):
        """Encoder half of a generation pass: compaction of the unmasked inputs, embeddings, encoder blocks,
        decoder_proj_context (+ embeddings) -> w["ctx"] fp32 (forward_mask_encoder_generation + encoder,
        egom2p/models/generate.py:747-757).  parts = [(side, enc_inputs, N, first row)]: one entry per group of B samples
        (the conditional and the unconditional inputs of a guided step); the groups' rows lie back to back, every row-wise
        launch (LayerNorm, GEMMs, gate) covers all of them - the unconditional pass's 1707 / 3414 rows alone leave most CUs
        idle - compaction, embedding and self-attention run per group (own row counts)."""
        cfg, D = self.cfg, self.D
        parts = [p for p in parts if p[2] > 0]
        R = sum(B * n for _, _, n, _ in parts)
        x, xn = w["xa"], w["xb"]
        for side, enc_inputs, N, r0 in parts:          # N = rows per sample, the engine's register tokens included
            foreign = [k for k in enc_inputs if k not in {m.name for m in self.enc_mods}]
            if foreign:
                raise KeyError(f"an encoder pass takes encoder modalities only (generate.py:749-751): {foreign}")
            mods = [m for m in self.enc_mods if m.name in enc_inputs]
            ops.compact([enc_inputs[m.name][1].contiguous() for m in mods], [enc_inputs[m.name][0].reshape(B, -1).contiguous() for m in mods],
                        None, [m.max_tokens for m in mods], [m.id for m in mods], N - self.R, False, side, B, n_reg=self.R)
            ops.embed_fwd([self.p[f"encoder_embeddings.{m.name}.token_emb.weight"] for m in mods], [self.pos_enc[m.name] for m in mods],
                          [self.p[f"encoder_embeddings.{m.name}.mod_emb"] for m in mods], None, side["slot"], side["local"], side["tok"],
                          x[r0:], w["emb"][r0:], B * N, D, reg=self.p["register_tokens"] if self.R else None)

        def enc_attn():
            for side, _, N, r0 in parts:
                self._attn_infer(w, self._qkv_site(w, r0), w["ao"][r0:], _keys_per_sample(w["zero_b"], side["n_valid"]), B, N, N)

        for i in range(cfg.encoder_depth):
            pre = f"encoder.{i}"
            self._attn_sublayer(pre, "attn", x, xn, R, w["ln"], w["st"], w["qkv"], w["ao"], enc_attn, w=w)
            self._mlp_sublayer(pre, xn, x, R, w["ln"], w["st"], w["ab"], w["h"])
        self._ln(x[:R], "encoder_norm.weight", w["ln"], w["st"])
        self._lin_fwd("decoder_proj_context.weight", w["ln"], w["ctx"], R, L.EPI_BIAS_RESID, R=w["emb"],
                      bias=self.p["decoder_proj_context.bias"])

    def _infer_decode(self, w, parts, target: str, dec_pos: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
        """Decoder half of a generation pass over len(parts) groups of B samples that decode the SAME positions against
        different contexts (parts[g] = (side, N_g, first context row); groups with an empty context last).  Everything
        but the cross-attention itself is one launch for all groups.  Returns bf16 logits [groups * B * M, V]."""
        cfg, D = self.cfg, self.D
        tm = {m.name: m for m in self.dec_mods}[target]          # (KeyError: the target must be a decoder modality)
        B, M = dec_pos.shape
        G = len(parts)
        RM, RD = B * M, G * B * M
        RC = sum(B * n for _, n, _ in parts)
        n_ctx = sum(1 for _, n, _ in parts if n > 0)
        if any(n > 0 for _, n, _ in parts[n_ctx:]):
            raise ValueError("groups with an empty context come last")
        RQ = n_ctx * RM                                     # decoder rows that have a context to attend to
        # decoder rows: mask token + positional + modality embedding of the selected target positions (:481-516)
        y, yn = w["ya"], w["yb"]
        local = dec_pos.to(self.dev, I32)
        local = (local.unsqueeze(0).expand(G, B, M) if G > 1 else local).contiguous()
        ops.embed_fwd(None, [self.pos_dec[tm.name]], [self.p[self.dec_mod_emb_key[tm.name]]], self.p["mask_token"],
                      w["dslot"], local, w["dtok"], y, None, RD, D)
        w["full_m"].fill_(M)
        all_keys = _keys_per_sample(w["zero_b"], w["full_m"])       # decoder self-attention is unmasked (sa_mask=None)
        fused = self.ctx_ln_fused and w.get("cns") is not None and RC > 0
        if fused:
            ops.layernorm_fwd_multi(w["ctx"][:RC], [self.p[f"decoder.{i}.context_norm.weight"] for i in range(cfg.decoder_depth)],
                                    w["cns"], w["st"][0], w["st"][1], eps=cfg.eps, width=self.Dl)
        for i in range(cfg.decoder_depth):
            pre = f"decoder.{i}"
            self._attn_sublayer(pre, "self_attn", y, yn, RD, w["ln"], w["st"], w["qkv"], w["ao"],
                                lambda: self._attn_infer(w, self._qkv_site(w), w["ao"], all_keys, G * B, M, M), w=w)
            proj_b = self.lin[f"{pre}.cross_attn.proj.weight"].b is not None
            if RQ > 0:
                self._ln(yn[:RQ], f"{pre}.query_norm.weight", w["ln"], w["st"])
                self._lin_fwd(f"{pre}.cross_attn.q.weight", w["ln"], w["q"], RQ)
                cn = w["cns"][i] if fused else w["cn"]
                if not fused:
                    self._ln(w["ctx"][:RC], f"{pre}.context_norm.weight", cn, w["st"])
                self._lin_fwd(f"{pre}.cross_attn.kv.weight", cn, w["kv"], RC)
                if self.qk_norm:
                    self._hn_one(f"{pre}.cross_attn.q_norm.weight", _Rows(w["q"], 0, self.A), _Rows(w["xqn"], 0, self.A), w["hstq"], RQ)
                    self._hn_one(f"{pre}.cross_attn.k_norm.weight", _Rows(w["kv"], 0, 2 * self.A), _Rows(w["xkn"], 0, 2 * self.A), w["hstk"], RC)
                for g in range(n_ctx):                          # the two halves of a guided step attend different contexts
                    side, n, c0 = parts[g]
                    self._attn_infer(w, self._q_kv_site(w, w["kv"], g * RM, c0), w["ao"][g * RM:], _keys_per_sample(w["zero_b"], side["n_valid"]),
                                     B, M, n)
                rows_p = RQ
                if RQ < RD and proj_b:
                    w["ao"][RQ:RD].zero_()                     # groups without a context: proj(0) = its bias (below)
                    rows_p = RD
                self._lin_fwd(f"{pre}.cross_attn.proj.weight", w["ao"], y, rows_p, L.EPI_RESID, R=yn)
                if rows_p < RD:
                    y[RQ:RD].copy_(yn[RQ:RD])
            elif proj_b:
                # empty context, proj with a bias: attn @ v over an empty axis = 0, so the block adds proj(0) = bf16(bias) to every row
                w["ao"][:RD].zero_()
                self._lin_fwd(f"{pre}.cross_attn.proj.weight", w["ao"], y, RD, L.EPI_RESID, R=yn)
            else:
                # empty context: softmax over zero keys contributes nothing (attn @ v over an empty axis = 0) and the
                # bias-free proj keeps it 0, so the cross-attention residual is the identity
                y, yn = yn, y
            self._mlp_sublayer(pre, y, yn, RD, w["ln"], w["st"], w["ab"], w["h"])
            y, yn = yn, y
        self._ln(y[:RD], "decoder_norm.weight", w["ln"], w["st"])
        l = self.lin[self.logit_key[tm.name]]
        logits = out if out is not None else torch.empty(RD, tm.vocab_size, device=self.dev, dtype=BF16)
        ops.gemm_nt(w["ln"], l.wb, logits, RD, tm.vocab_size, D, L.EPI_BF16, lda=D, ldb=D, ldc=tm.vocab_size)
        return logits

    @torch.no_grad()
    def infer_logits(self, enc_inputs: Dict[str, Tuple[torch.Tensor, torch.Tensor]], n_enc: int, target: str,
                     dec_pos: torch.Tensor, out: Optional[torch.Tensor] = None, ws: Optional[dict] = None) -> torch.Tensor:
        """One encoder-decoder pass of `forward_enc_dec_roar_batched` (egom2p/models/generate.py:747-766).

        enc_inputs: modality -> (ids int64 [B, n], input_mask bool [B, n]); n_enc = rows kept per sample (the
        reference takes the max unmasked count over the batch, :413-415; 0 = unconditional pass with an empty
        context).  dec_pos: int [B, M] positions of the decoded target tokens inside `target` (their order is the
        ROAR order; decoder self-attention is unmasked, sa_mask=None at :761).  Returns bf16 logits [B, M, V]."""
        if self.weights_dirty:
            self.refresh_weights()
        B, M = dec_pos.shape
        N = int(n_enc) + self.R                  # register tokens ride in front of the kept inputs: the context is never empty then
        w = ws if ws is not None else self._alloc_infer(B, max(N, 1), M)
        side = w["sides"][0]
        if N > 0:
            self._infer_context(w, [(side, enc_inputs, N, 0)], B)
        logits = self._infer_decode(w, [(side, N, 0)], target, dec_pos, out)
        return logits.view(B, M, -1)

    @torch.no_grad()
    def infer_logits_cfg(self, enc_cond, n_cond: int, enc_uncond, n_uncond: int, target: str, dec_pos: torch.Tensor,
                         out: Optional[torch.Tensor] = None, ws: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The conditional and the unconditional pass of one classifier-free-guidance step (generate.py:881-905 runs
        forward_enc_dec_roar_batched twice) as ONE pass: the encoder runs the two input sets as two groups of rows back to
        back (row-wise launches cover both, self-attention per group); both passes decode the same positions from the same
        mask-token rows, only the cross-attention context differs - the decoder runs 2 B samples per launch (the launches
        of this path are latency-bound: twice the rows cost the same time) and cross-attends per half.
        Returns (logits_cond, logits_uncond), each bf16 [B, M, V]."""
        if self.weights_dirty:
            self.refresh_weights()
        B, M = dec_pos.shape
        Nc, Nu = int(n_cond), int(n_uncond)
        if Nc <= 0:
            raise ValueError("the conditional pass of a guided step has a context")
        Nc, Nu = Nc + self.R, Nu + self.R        # register tokens ride in front of the kept inputs of either pass
        w = ws if ws is not None else self._alloc_infer(B, max(Nc, Nu, 1), M, groups=2)
        if w["groups"] < 2:
            raise ValueError("workspace allocated for single passes (groups=1)")
        sc, su = w["sides"]
        self._infer_context(w, [(sc, enc_cond, Nc, 0), (su, enc_uncond, Nu, B * Nc)], B)
        logits = self._infer_decode(w, [(sc, Nc, 0), (su, Nu, B * Nc)], target, dec_pos, out)
        V = logits.shape[-1]
        return logits[:B * M].view(B, M, V), logits[B * M:2 * B * M].view(B, M, V)

    def _graphed(self, key, make_state, run):
        """Capture-once / replay cache of the generation passes: `make_state()` builds the static buffers (a captured
        graph bakes in device addresses: it owns its workspace for as long as it lives), `run(st)` issues the launches.
        A graph reads the bf16 weight copies in place: they are refreshed here, before a capture and before every replay."""
        if self.weights_dirty:
            self.refresh_weights()
        graphs = self.__dict__.setdefault("_graphs", {})
        g = graphs.pop(key, None)
        if g is None:
            # every graph owns a workspace of ~30 KB per row: bound the cache (a ROAR schedule needs 2 x steps shapes;
            # the least recently used graph and its buffers are released first)
            while len(graphs) >= self.max_graphs:
                graphs.pop(next(iter(graphs)))
            st = make_state()
            side = _warmup_stream(self.dev)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                           # warm-up (lazy inits happen here, not in the capture)
                run(st)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                run(st)
            g = (graph, st)
        graphs[key] = g                                            # most recently used last
        return g

    def _replay(self, key, sets, dec_pos, V, alloc, run):
        """The graphed generation passes: static copies of the input sets (modality -> (ids, mask)) and of dec_pos, a captured
        `run(ws, static sets, static dec_pos, out)` over them (`_graphed`, keyed by key(modality names)), then copy-in and replay.
        Returns the static bf16 logits [len(sets) * B * M, V]: valid until the next replay of the same graph."""
        B, M = dec_pos.shape
        names = tuple(m.name for m in self.enc_mods if m.name in sets[0])

        def make_state():
            return {"ws": alloc(),
                    "ids": [{n: e[n][0].reshape(B, -1).to(self.dev, torch.int64).clone() for n in names} for e in sets],
                    "mask": [{n: e[n][1].reshape(B, -1).to(self.dev, torch.bool).clone() for n in names} for e in sets],
                    "pos": dec_pos.to(self.dev, I32).clone(),
                    "out": torch.empty(len(sets) * B * M, V, device=self.dev, dtype=BF16)}

        graph, st = self._graphed(key(names), make_state,
                                  lambda st: run(st["ws"], [{n: (i[n], m[n]) for n in names} for i, m in zip(st["ids"], st["mask"])],
                                                 st["pos"], st["out"]))
        for k, e in enumerate(sets):
            for n in names:
                st["ids"][k][n].copy_(e[n][0].reshape(B, -1))
                st["mask"][k][n].copy_(e[n][1].reshape(B, -1))
        st["pos"].copy_(dec_pos)
        graph.replay()
        return st["out"]

    def infer_logits_graphed(self, enc_inputs, n_enc: int, target: str, dec_pos: torch.Tensor) -> torch.Tensor:
        """`infer_logits` replayed from a captured hipGraph (BASELINE config 4: "hipGraph-captured decode").
        One graph per pass shape (batch, modalities, N, M, target): inputs are copied into static buffers, the
        ~300 kernel launches of a pass are replayed with one host call, the logits land in a static buffer
        that stays valid until the next replay of the same graph."""
        B, M = dec_pos.shape
        V = {m.name: m for m in self.dec_mods}[target].vocab_size
        out = self._replay(lambda names: (B, names, int(n_enc), M, target), [enc_inputs], dec_pos, V,
                           lambda: self._alloc_infer(B, max(int(n_enc) + self.R, 1), M, fresh=True),
                           lambda ws, sets, pos, out: self.infer_logits(sets[0], n_enc, target, pos, out=out, ws=ws))
        return out.view(B, M, V)

    def infer_logits_cfg_graphed(self, enc_cond, n_cond: int, enc_uncond, n_uncond: int, target: str, dec_pos: torch.Tensor):
        """`infer_logits_cfg` (both passes of a guided step, one decoder pass) replayed from a captured hipGraph"""
        B, M = dec_pos.shape
        V = {m.name: m for m in self.dec_mods}[target].vocab_size
        out = self._replay(lambda names: ("cfg", B, names, int(n_cond), int(n_uncond), M, target), [enc_cond, enc_uncond], dec_pos, V,
                           lambda: self._alloc_infer(B, max(int(n_cond), int(n_uncond), 1) + self.R, M, fresh=True, groups=2),
                           lambda ws, sets, pos, out: self.infer_logits_cfg(sets[0], n_cond, sets[1], n_uncond, target, pos, out=out, ws=ws))
        return out[:B * M].view(B, M, V), out[B * M:].view(B, M, V)

    @torch.no_grad()
    def forward_logits(self, mod_dict, dec_order=None) -> Dict[str, torch.Tensor]:
        """`return_logits=True` path of EgoM2P.forward (egom2p_model.py:727-729, 546-547): logits of every
        decoder row for every modality, (B, M, V) bf16."""
        self.forward(mod_dict, dec_order=dec_order, need_loss=False, group_rows=False)
        if int(self.cd["err"].item()):              # inference API: the caller reads the logits on the host anyway
            self.cd["err"].zero_()
            raise L.EgoHipError("decoder_attention_mask is not one key interval per row (egom2p_model.py:446-481 would "
                                "produce a mask this engine cannot express)")
        B, M, D = self.B, self.M, self.D
        out = {}
        for m in self.fmods:                      # (the modalities of the call: forward_logits walks decoder_mod_dict, :544)
            l = self.lin[self.logit_key[m.name]]
            lg = torch.empty(B * M, m.vocab_size, device=self.dev, dtype=BF16)
            ops.gemm_nt(self.yn, l.wb, lg, B * M, m.vocab_size, D, L.EPI_BF16, lda=D, ldb=D, ldc=m.vocab_size)
            out[m.name] = lg.view(B, M, m.vocab_size)
        self._have_fwd = False
        return out
