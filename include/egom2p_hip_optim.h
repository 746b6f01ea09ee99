/* Extension entries of libegom2p_hip.so: the optimiser entry points added after the core header's entry list was settled.
 *
 * Same library, same conventions and the same ABI version as egom2p_hip.h (which includes this file): plain C functions over raw
 * device pointers and a hipStream_t, 0 on success, EGO_ERR_ARG / EGO_ERR_LAUNCH otherwise, no allocation, no synchronisation,
 * capturable.  The entries live in a header of their own because the core header's entry list is pinned by the suite
 * (tests/test_posemb_cpu.py holds it at 78 names); egom2p_amd/_lib.py binds them from a table of their own (EXPORTS_OPTIM) and
 * tests/test_param_groups_cpu.py holds this header, that table and the library's dynamic symbols together.  Nothing declared in
 * egom2p_hip.h changed, so EGO_ABI_VERSION stays 12 (new entries alone do not call for a bump). */
#ifndef EGOM2P_HIP_OPTIM_H
#define EGOM2P_HIP_OPTIM_H

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Parameter-group AdamW: the groups get_parameter_groups builds - one per (layer id, weight-decay class), each with its lr_scale
 * (egom2p/utils/optim_factory.py:97-154, 226; the loop multiplies lr by it, run_training_egom2p.py:707-713) - stepped in ONE launch
 * over the flat buffers p, g, m, v of n floats.
 * segs: n_segs segments [lo, hi) of the buffers, ascending and disjoint, lo and hi multiples of 4, 0 <= lo < hi <= n; `group`
 * indexes the hyper-parameter block.  flags & EGO_SEG_FROZEN: p, m, v are not touched, g is zeroed (when zero_grad).  Elements in
 * no segment are neither read nor written.  The table is static between steps: `segs` is its DEVICE copy, `segs_host` the same
 * table in host memory (the argument checks and the grid are formed from it; it is not kept past the call), `chunks` the device
 * array of n_segs longs that holds each segment's first chunk - chunks[0] = 0, chunks[s + 1] = chunks[s] + ceil((hi - lo) /
 * EGO_ADAMW_CHUNK) - so that no chunk of work crosses a segment.
 * hp: HOST struct, copied into the kernel arguments at launch (no device upload, capturable; the caller may rewrite it as soon as
 * the call returns).  Slots [0, n_groups) hold lr, wd and the step count of each (group, step offset) combination; the entry fills
 * bc1 / bc2_sqrt itself.  gate == NULL: the bias corrections are formed on the host in double, as ego_adamw_step forms them.
 * gate != NULL: ego_adamw_step_gated's semantics - gate[0] != 0 writes nothing but the zeroed gradients, otherwise a slot's step
 * count is step - gate[1], floored at 1, and the corrections are formed on the device.
 * The per-element arithmetic is ego_adamw_step's.  Grid capped at 4096 workgroups, 64-bit element indices, no atomics.
 * EGO_ERR_ARG (nothing is launched): a pointer that is not 16-byte aligned, n_segs < 0, n_groups outside [0, EGO_ADAMW_MAX_GROUPS],
 * a segment out of order / outside [0, n) / not a multiple of 4, a group outside [0, n_groups), step < 1 in the slot of a segment
 * that is not frozen.  More than EGO_ADAMW_MAX_GROUPS combinations: several calls over disjoint segment sets. */
#define EGO_ADAMW_MAX_GROUPS 128
#define EGO_ADAMW_CHUNK 4096
#define EGO_SEG_FROZEN 1
typedef struct { long lo, hi; int group; int flags; } ego_adamw_seg;
typedef struct {
    float lr[EGO_ADAMW_MAX_GROUPS], wd[EGO_ADAMW_MAX_GROUPS], bc1[EGO_ADAMW_MAX_GROUPS], bc2_sqrt[EGO_ADAMW_MAX_GROUPS];
    int step[EGO_ADAMW_MAX_GROUPS];
    int n_groups;
} ego_adamw_hp;
int ego_adamw_step_seg(float* p, float* g, float* m, float* v, long n, const ego_adamw_seg* segs_host, const ego_adamw_seg* segs,
                       int n_segs, const long* chunks, const ego_adamw_hp* hp, float beta1, float beta2, float eps, float gscale,
                       float max_norm, const double* sqnorm, int zero_grad, const int* gate, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
