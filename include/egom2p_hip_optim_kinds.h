/* Extension entries of libegom2p_hip.so, second sheet: the optimisers other than AdamW on the segmented flat-buffer launch.
 *
 * Same library, same conventions and the same ABI version as egom2p_hip.h (which includes this file behind egom2p_hip_optim.h):
 * plain C functions over raw device pointers and a hipStream_t, 0 on success, EGO_ERR_ARG / EGO_ERR_LAUNCH otherwise, no
 * allocation, no synchronisation, capturable.  The entry lives in a header of its own because the suite pins the entry lists of
 * the two headers before it (tests/test_posemb_cpu.py: 78 names in the core header; tests/test_param_groups_cpu.py:
 * egom2p_hip_optim.h holds ego_adamw_step_seg alone); egom2p_amd/_lib.py binds it from a table of its own (EXPORTS_OPTIM_KINDS)
 * and tests/test_optim_kinds_cpu.py holds this header, that table and the library's dynamic symbols together.  Nothing declared
 * before changed, so EGO_ABI_VERSION stays 12. */
#ifndef EGOM2P_HIP_OPTIM_KINDS_H
#define EGOM2P_HIP_OPTIM_KINDS_H

#include <hip/hip_runtime_api.h>

#include "egom2p_hip_optim.h"       /* ego_adamw_seg, ego_adamw_hp, EGO_SEG_FROZEN, EGO_ADAMW_CHUNK, EGO_ADAMW_MAX_GROUPS */

#ifdef __cplusplus
extern "C" {
#endif

/* The remaining choices of the reference's `--opt` (create_optimizer, egom2p/utils/optim_factory.py:217-224):
 *   sgd / nesterov -> optim.SGD(momentum=args.momentum, nesterov=True)     EGO_OPT_NESTEROV
 *   momentum       -> optim.SGD(momentum=args.momentum, nesterov=False)    EGO_OPT_SGD
 *   adam           -> optim.Adam (weight decay coupled into the gradient)  EGO_OPT_ADAM
 * stepped over ego_adamw_step_seg's frame: the same segment table (host and device copy), chunk prefix array and host-side
 * hyper-parameter block, the same gscale / max_norm / sqnorm clip coefficient `coef`, zero_grad, gate and EGO_SEG_FROZEN; every
 * argument up to `gate` means what it means there.  Elements in no segment are neither read nor written.
 * Per element, fp32, with ge = g * coef and lr / wd of the segment's slot:
 *   EGO_OPT_ADAM      d = ge + wd p;  m = b1 m + (1 - b1) d;  v = b2 v + (1 - b2) d d;  p -= (lr / bc1) (m / (sqrtf(v) / bc2_sqrt + eps))
 *                     (torch.optim.Adam, amsgrad=False).  bc1 / bc2_sqrt are formed as ego_adamw_step_seg forms them: on the host
 *                     in double from the slot's step without a gate, on the device from step - gate[1], floored at 1, with one.
 *   EGO_OPT_SGD       d = ge + wd p;  m = momentum m + d;  p -= lr m               (torch.optim.SGD, dampening 0; torch's first
 *                     step sets the buffer to d, which is this recurrence from a zero buffer)
 *   EGO_OPT_NESTEROV  d and m as EGO_OPT_SGD;  p -= lr (d + momentum m)
 * The two SGD kinds keep ONE state buffer, `m` (the momentum buffer); they take v == NULL and never read or write v, ignore
 * beta1 / beta2 / eps and the slots' step counts (step < 1 is no error for them).  `momentum` is one value per call, as in the
 * reference (it is not part of the per-group block); EGO_OPT_ADAM ignores it.
 * Grid capped at 4096 workgroups, 16-byte accesses, 64-bit element indices, no atomics: bitwise reproducible.
 * EGO_ERR_ARG (nothing is launched): whatever ego_adamw_step_seg refuses (v and the step counts only for EGO_OPT_ADAM), a kind
 * that is none of the three, v == NULL with EGO_OPT_ADAM, momentum negative or not finite with an SGD kind. */
#define EGO_OPT_ADAM 1
#define EGO_OPT_SGD 2
#define EGO_OPT_NESTEROV 3
int ego_optim_step_seg(float* p, float* g, float* m, float* v, long n, const ego_adamw_seg* segs_host, const ego_adamw_seg* segs,
                       int n_segs, const long* chunks, const ego_adamw_hp* hp, float beta1, float beta2, float eps, float gscale,
                       float max_norm, const double* sqnorm, int zero_grad, const int* gate, int kind, float momentum,
                       hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
