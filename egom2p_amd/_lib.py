"""ctypes binding of libegom2p_hip.so (the C-ABI declared in include/egom2p_hip.h).

The product path fails loudly when the HIP library is missing: there is no CPU or eager fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EGOM2P_HIP_LIB", os.path.join(_HERE, "libegom2p_hip.so"))   # override: kernel experiments
MAX_MODS = 8

ABI_VERSION = 12         # == EGO_ABI_VERSION of include/egom2p_hip.h (tests/test_cabi_exports.py holds the two together)
EPI_BF16, EPI_F32, EPI_RESID, EPI_BIAS_RESID, EPI_BIAS_BF16 = 0, 1, 2, 3, 4

vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_long, C.c_float


class CompactDesc(C.Structure):
    _fields_ = [
        ("n_mods", i32), ("n_keep", i32), ("is_decoder", i32),
        ("mask", vp * MAX_MODS), ("ids", vp * MAX_MODS), ("dam", vp * MAX_MODS),
        ("n_pos", i32 * MAX_MODS), ("mod_id", i32 * MAX_MODS),
        ("ids_keep", vp), ("pad", vp), ("mod_mask", vp), ("slot", vp), ("local", vp), ("tok", vp),
        ("ks", vp), ("ke", vp), ("n_valid", vp), ("seg", vp), ("err", vp), ("seg_bad", vp), ("n_reg", i32),
    ]


MAX_MIX = 8


class BudgetDesc(C.Structure):
    _fields_ = [
        ("n_mods", i32), ("n_mix", i32),
        ("in_alpha", (f32 * MAX_MODS) * MAX_MIX), ("tgt_alpha", (f32 * MAX_MODS) * MAX_MIX), ("mix_weight", f32 * MAX_MIX),
        ("max_tokens", i32 * MAX_MODS), ("min_tokens", i32 * MAX_MODS), ("not_seq", i32 * MAX_MODS),
        ("n_in_lo", i32), ("n_in_hi", i32), ("n_tgt_lo", i32), ("n_tgt_hi", i32), ("max_tries", i32),
    ]


class EmbedDesc(C.Structure):
    _fields_ = [
        ("table", vp * MAX_MODS), ("pos", vp * MAX_MODS), ("mod", vp * MAX_MODS), ("base_vec", vp),
        ("slot", vp), ("local", vp), ("tok", vp), ("x", vp), ("emb", vp), ("rows", i64), ("D", i32), ("reg", vp),
    ]


class EmbedBwdDesc(C.Structure):
    _fields_ = [
        ("dtable", vp * MAX_MODS), ("dmod", vp * MAX_MODS), ("dbase", vp), ("dx", vp), ("d2", vp),
        ("slot", vp), ("tok", vp), ("rows", i64), ("D", i32), ("n_mods", i32), ("touched", vp * MAX_MODS),
        ("work", vp), ("work_floats", i64), ("vocab", i32 * MAX_MODS),
    ]


class PosembGradDesc(C.Structure):
    _fields_ = [
        ("dx", vp), ("d2", vp), ("slot", vp), ("local", vp), ("rows", i64), ("rows_per_sample", i32), ("B", i32), ("D", i32),
        ("ld", i64), ("n_mods", i32), ("n_pos", i32 * MAX_MODS), ("dpos", vp * MAX_MODS), ("accumulate", i32),
        ("work", vp), ("work_ints", i64), ("err", vp),
    ]


class HeadNormOp(C.Structure):
    _fields_ = [("x", vp), ("x_bs", i64), ("x_rs", i64), ("y", vp), ("y_bs", i64), ("y_rs", i64),
                ("w", vp), ("mean", vp), ("rstd", vp), ("dw", vp)]


ADAMW_MAX_GROUPS, ADAMW_CHUNK, SEG_FROZEN = 128, 4096, 1     # EGO_ADAMW_MAX_GROUPS, EGO_ADAMW_CHUNK, EGO_SEG_FROZEN


class AdamwSeg(C.Structure):
    _fields_ = [("lo", i64), ("hi", i64), ("group", i32), ("flags", i32)]


class AdamwHp(C.Structure):
    _fields_ = [("lr", f32 * ADAMW_MAX_GROUPS), ("wd", f32 * ADAMW_MAX_GROUPS), ("bc1", f32 * ADAMW_MAX_GROUPS),
                ("bc2_sqrt", f32 * ADAMW_MAX_GROUPS), ("step", i32 * ADAMW_MAX_GROUPS), ("n_groups", i32)]


_SIGS = {
    "ego_abi_version": [],
    "ego_gemm_kernel_mode": [i32, i32],
    "ego_gemm_small_tiles": [i32],
    "ego_gemm_tune": [i32, i32],
    "ego_attn_tune": [i32, i32],
    "ego_compact": [C.POINTER(CompactDesc), i32, vp],
    "ego_compact_causal": [C.POINTER(CompactDesc), i32, vp],
    "ego_compact_nosep": [C.POINTER(CompactDesc), i32, i32, vp],
    "ego_embed_fwd": [C.POINTER(EmbedDesc), vp],
    "ego_embed_bwd_work_floats": [i64, i32, i32],
    "ego_embed_bwd": [C.POINTER(EmbedBwdDesc), vp],
    "ego_reg_grad": [vp, i32, i64, i32, i32, vp, vp],
    "ego_posemb_grad_work_ints": [i32, i32, C.POINTER(i32)],
    "ego_posemb_grad": [C.POINTER(PosembGradDesc), vp],
    "ego_rows_compact": [vp, i32, i32, vp, vp, vp],
    "ego_rows_gather": [vp, vp, vp, i32, i32, vp, vp],
    "ego_rows_scatter": [vp, vp, vp, i32, i32, vp, i32, vp],
    "ego_loss_perm": [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp],
    "ego_layernorm_fwd": [vp, vp, vp, vp, vp, vp, i32, i32, i64, f32, vp, i64, vp, vp],
    "ego_layernorm_bwd_work_floats": [i32, i32],
    "ego_layernorm_bwd": [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i64, vp],
    "ego_layernorm_bias_fwd": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i64, f32, vp],
    "ego_layernorm_bias_bwd_work_floats": [i32, i32],
    "ego_layernorm_bias_bwd": [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i64, vp],
    "ego_layernorm_fwd_multi": [vp, i32, vp, vp, vp, vp, i32, i32, i64, f32, vp],
    "ego_layernorm_bwd_multi_work_floats": [i32, i32, i32],
    "ego_layernorm_bwd_multi": [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i64, vp],
    "ego_headnorm_fwd": [C.POINTER(HeadNormOp), i32, i32, i32, i32, i32, f32, vp],
    "ego_headnorm_bwd_work_floats": [i32, i32, i32, i32],
    "ego_headnorm_bwd": [C.POINTER(HeadNormOp), i32, i32, i32, i32, i32, vp, i64, vp],
    "ego_droppath_draw": [vp, i32, i32, C.c_uint64, C.c_uint64, vp, vp],
    "ego_droppath_resid": [vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, i32, f32, vp],
    "ego_droppath_scale": [vp, i64, vp, i64, vp, i64, i32, i32, i32, f32, vp],
    "ego_gemm_nt_bf16": [vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, i32, i32, i32, i32, vp],
    "ego_gemm_tn_bf16": [vp, i64, vp, i64, vp, vp, i64, i32, i32, i32, vp, i32, i32, i32, i32, vp, vp],
    "ego_quant_fp8_rows": [vp, i64, i64, i32, vp, i64, vp, vp],
    "ego_gemm_nt_fp8": [vp, i64, vp, vp, i64, vp, vp, i64, vp, i64, vp, i32, i32, i32, i32, vp],
    "ego_gemm_nt_swiglu_fwd_fp8": [vp, i64, vp, vp, i64, vp, vp, i64, vp, i64, i32, i32, i32, vp],
    "ego_gemm_tn_plan": [i32, i32, i32, i64, i64, i64, i32],
    "ego_attn_fwd_d64": [vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, i64, i64,
                         i32, i32, i32, i32, f32, vp],
    "ego_attn_bwd_d64": [vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, vp, i64, i64, vp, vp,
                         vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, vp, i64, i64, i32, i32, i32, i32, f32, vp],
    "ego_attn_fwd_d64_seg": [vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, i64, i64, vp, i32, vp,
                             i32, i32, i32, i32, f32, vp],
    "ego_attn_bwd_d64_seg": [vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, vp, i64, i64, vp, vp,
                             vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, vp, i64, i64, vp, i32, vp, i32, i32, i32, i32, f32, vp],
    "ego_attn_fwd_split_floats": [i32, i32, i32, i32],
    "ego_attn_fwd_d64_split": [vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, vp, vp, i64, i64,
                               i32, i32, i32, i32, f32, i32, vp, i64, vp],
    "ego_attn_fwd_hd": [vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, i64, i64,
                        i32, i32, i32, i32, i32, f32, vp],
    "ego_attn_bwd_hd": [vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, vp, i64, i64, vp, vp,
                        vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, vp, i64, i64, i32, i32, i32, i32, i32, f32, vp],
    "ego_budget_dirichlet": [C.POINTER(BudgetDesc), vp, i32, vp, vp, vp],
    "ego_clip_synth": [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp],
    "ego_swiglu_fwd": [vp, vp, i64, i32, vp],
    "ego_swiglu_bwd": [vp, vp, vp, i64, i32, vp],
    "ego_gelu_fwd": [vp, vp, i64, i32, i64, i64, vp],
    "ego_gelu_bwd": [vp, vp, vp, i64, i32, i64, i64, i64, vp],
    "ego_gemm_nt_swiglu_bwd": [vp, i64, vp, i64, vp, vp, i64, i32, i32, i32, vp],
    "ego_gemm_nt_swiglu_fwd": [vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, i32, vp],
    "ego_ce_fwd": [vp, i64, i32, vp, vp, i32, vp, vp, vp],
    "ego_ce_bwd": [vp, i64, i32, vp, vp, i32, vp, vp, i32, vp, vp],
    "ego_ce_fwd_bwd": [vp, i64, i32, vp, vp, i32, vp, vp, vp, i32, vp, vp],
    "ego_loss_weights": [vp, C.POINTER(i32), i32, i32, vp, vp, vp],
    "ego_loss_finalize": [vp, vp, i32, vp, vp, vp, vp, vp],
    "ego_cast_weight": [vp, i32, i32, i64, vp, i64, vp, i64, i32, vp],
    "ego_cast_f32_bf16": [vp, vp, i64, vp],
    "ego_bias_grad_work_floats": [i64, i32],
    "ego_bias_grad": [vp, i64, i32, vp, vp, i64, vp],
    "ego_grad_sqnorm": [vp, i64, vp, vp, vp],
    "ego_adamw_step": [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i32, f32, f32, vp, i32, vp],
    "ego_adamw_gate": [vp, f32, f32, i32, vp, vp],
    "ego_adamw_step_gated": [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i32, f32, f32, vp, i32, vp, vp],
    "ego_ema_update": [vp, vp, i64, f32, f32, vp],
    "ego_swap_f32": [vp, vp, i64, vp],
    "ego_sample_cfg_topp": [vp, vp, i64, i32, f32, f32, i32, f32, vp, vp, vp, i32, vp],
    "ego_maskgit_positions": [vp, i32, i32, i32, vp, vp],
    "ego_maskgit_select": [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp],
    "ego_dp_unique_id": [vp],
    "ego_dp_comm_create": [vp, i32, i32, C.POINTER(vp)],
    "ego_dp_comm_destroy": [vp],
    "ego_dp_allreduce_begin": [vp, vp, i64, i32, vp, vp],
    "ego_dp_wait": [vp, vp, vp],
}

EXPORTS = tuple(_SIGS)

# the extension entries of include/egom2p_hip_optim.h (same library; tests/test_param_groups_cpu.py holds header and table together)
_SIGS_OPTIM = {
    "ego_adamw_step_seg": [vp, vp, vp, vp, i64, C.POINTER(AdamwSeg), vp, i32, vp, C.POINTER(AdamwHp), f32, f32, f32, f32, f32, vp, i32,
                           vp, vp],
}
EXPORTS_OPTIM = tuple(_SIGS_OPTIM)

# include/egom2p_hip_optim_kinds.h: Adam / SGD / Nesterov on the segmented launch (tests/test_optim_kinds_cpu.py holds header and table)
OPT_ADAM, OPT_SGD, OPT_NESTEROV = 1, 2, 3                  # EGO_OPT_ADAM, EGO_OPT_SGD, EGO_OPT_NESTEROV
_SIGS_OPTIM_KINDS = {
    "ego_optim_step_seg": _SIGS_OPTIM["ego_adamw_step_seg"][:-1] + [i32, f32, vp],
}
EXPORTS_OPTIM_KINDS = tuple(_SIGS_OPTIM_KINDS)
_lib = None


class EgoHipError(RuntimeError):
    pass


def load():
    """Load the HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EgoHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C egom2p_amd/csrc`). There is no CPU fallback for the product path.")
        # PyTorch-ROCm bundles its own libamdhip64; it must be in the process BEFORE our library is
        # dlopen'ed so both share one HIP runtime (streams and device pointers are per-runtime).
        import torch
        hip_rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(hip_rt):
            C.CDLL(hip_rt, mode=C.RTLD_GLOBAL)
        lib = C.CDLL(LIB_PATH)
        for name, args in {**_SIGS, **_SIGS_OPTIM, **_SIGS_OPTIM_KINDS}.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = i64 if name.endswith(("_work_floats", "_split_floats", "_work_ints")) else i32
        if lib.ego_abi_version() != ABI_VERSION:
            raise EgoHipError(f"libegom2p_hip.so ABI version {lib.ego_abi_version()} != binding {ABI_VERSION}: rebuild (make -C egom2p_amd/csrc)")
        # kernel experiments: EGO_GEMM_NT256 / EGO_GEMM_TN256 = 0 | 1 | 2 pick the GEMM tile family (the library itself
        # reads no environment; this is the same call tests make through ops.gemm_kernel_mode)
        if "EGO_GEMM_NT256" in os.environ or "EGO_GEMM_TN256" in os.environ:
            lib.ego_gemm_kernel_mode(int(os.environ.get("EGO_GEMM_NT256", "1")), int(os.environ.get("EGO_GEMM_TN256", "1")))
        if "EGO_GEMM_SMALL_TILES" in os.environ:
            lib.ego_gemm_small_tiles(int(os.environ["EGO_GEMM_SMALL_TILES"]))
        _lib = lib
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        raise EgoHipError(f"{what} failed: {'bad arguments' if rc == 1 else 'kernel launch failed'} (rc={rc})")

