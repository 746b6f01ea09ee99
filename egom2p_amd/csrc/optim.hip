// Optimiser-side kernels over the flat fp32 parameter / gradient / moment buffers (gfx950, HBM-bound):
// global gradient sum of squares, and AdamW with the clip coefficient and the data-parallel 1/world
// factor folded in (no separate unscale / clip / zero_grad passes).
//
// Replaces: torch.nn.utils.clip_grad_norm_ (egom2p/utils/native_scaler.py:33) and torch.optim.AdamW
// created at egom2p/utils/optim_factory.py:226 (betas 0.9/0.95, eps 1e-8, decoupled weight decay).
#include "common.h"
#include "egom2p_hip.h"
#include <math.h>

namespace {

__global__ __launch_bounds__(256) void sqnorm_kernel(const float* __restrict__ g, long n4, long n, double* __restrict__ out,
                                                     double* __restrict__ part) {
    __shared__ float red[4];
    float s = 0.f;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 v = *(const f32x4*)(g + i * 4);
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long i = n4 * 4; i < n; ++i) s += g[i] * g[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t = (double)(red[0] + red[1] + red[2] + red[3]);
        if (part) part[blockIdx.x] = t;        // summed in block order by sqnorm_finish_kernel: bitwise reproducible
        else atomicAdd(out, t);
    }
}

__global__ __launch_bounds__(64) void sqnorm_finish_kernel(const double* __restrict__ part, int nparts, double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < nparts; ++i) s += part[i];
    *out += s;
}

// p, g, m, v: flat fp32 of length n.  sqnorm: device double, sum of squares of the RAW grads.
// effective grad = g * gscale * clip,  clip = min(1, max_norm / (sqrt(sqnorm) * gscale + 1e-6)) (max_norm <= 0: no clip)
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long n, float lr, float wd, float b1, float b2,
                                                    float eps, float bc1, float bc2_sqrt, float gscale, float max_norm,
                                                    const double* __restrict__ sqnorm, int zero_grad) {
    float coef = gscale;
    if (max_norm > 0.f && sqnorm) {
        const float total = (float)sqrt(*sqnorm) * gscale;
        coef *= fminf(1.f, max_norm / (total + 1e-6f));
    }
    const float step = lr / bc1, decay = 1.f - lr * wd;
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 pp = *(f32x4*)(p + i * 4), gg = *(f32x4*)(g + i * 4), mm = *(f32x4*)(m + i * 4), vv = *(f32x4*)(v + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ge = gg[e] * coef;
            pp[e] *= decay;
            mm[e] = b1 * mm[e] + (1.f - b1) * ge;
            vv[e] = b2 * vv[e] + (1.f - b2) * ge * ge;
            pp[e] -= step * (mm[e] / (sqrtf(vv[e]) / bc2_sqrt + eps));
        }
        *(f32x4*)(p + i * 4) = pp; *(f32x4*)(m + i * 4) = mm; *(f32x4*)(v + i * 4) = vv;
        if (zero_grad) *(f32x4*)(g + i * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (long i = n4 * 4; i < n; ++i) {
            const float ge = g[i] * coef;
            float pe = p[i] * decay;
            const float me = b1 * m[i] + (1.f - b1) * ge, ve = b2 * v[i] + (1.f - b2) * ge * ge;
            pe -= step * (me / (sqrtf(ve) / bc2_sqrt + eps));
            p[i] = pe; m[i] = me; v[i] = ve;
            if (zero_grad) g[i] = 0.f;
        }
    }
}

}  // namespace

extern "C" int ego_abi_version(void) { return EGO_ABI_VERSION; }

extern "C" int ego_grad_sqnorm(const float* g, long n, double* out, double* work, hipStream_t stream) {
    if (n <= 0) return EGO_OK;
    if (((uintptr_t)g) % 16) return EGO_ERR_ARG;
    const long n4 = n / 4;
    int blocks = (int)((n4 + 255) / 256 < EGO_SQNORM_WORK ? (n4 + 255) / 256 : EGO_SQNORM_WORK);
    if (blocks < 1) blocks = 1;
    EGO_LAUNCH(sqnorm_kernel, dim3(blocks), dim3(256), 0, stream, g, n4, n, out, work);
    LAUNCH_CHECK();
    if (work) {
        EGO_LAUNCH(sqnorm_finish_kernel, dim3(1), dim3(64), 0, stream, (const double*)work, blocks, out);
        LAUNCH_CHECK();
    }
    return EGO_OK;
}

extern "C" int ego_adamw_step(float* p, float* g, float* m, float* v, long n, float lr, float wd, float beta1, float beta2,
                              float eps, int step, float gscale, float max_norm, const double* sqnorm, int zero_grad,
                              hipStream_t stream) {
    if (n <= 0) return EGO_OK;
    if (step < 1 || ((uintptr_t)p) % 16 || ((uintptr_t)g) % 16 || ((uintptr_t)m) % 16 || ((uintptr_t)v) % 16) return EGO_ERR_ARG;
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    const long n4 = n / 4;
    const int blocks = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
    EGO_LAUNCH(adamw_kernel, dim3(blocks < 1 ? 1 : blocks), dim3(256), 0, stream, p, g, m, v, n, lr, wd, beta1, beta2, eps,
                       bc1, bc2s, gscale, max_norm, sqnorm, zero_grad);
    LAUNCH_CHECK();
    return EGO_OK;
}

// ---- step gate: skip_grad of the reference loop and the opt-in non-finite guard, decided on the device ----------------------
//
// Replaces: the `elif skip_grad is not None` branch of NativeScalerWithGradNormCount.__call__ (egom2p/utils/native_scaler.py:34-40:
// `if norm >= skip_grad: return norm` in front of optimizer.step()).  The reference reads the norm on the host; here the gate
// kernel leaves the decision in device memory and the gated AdamW pass reads it, so a step costs no host sync.
namespace {

// gate: EGO_GATE_WORDS int32 - [0] this call is gated, [1] gated calls since the host last folded them into its step counts,
// [2] gated calls in total.  One thread, plain loads and stores: no atomics, capturable.
__global__ __launch_bounds__(64) void adamw_gate_kernel(const double* __restrict__ sqnorm, float gscale, float skip_norm,
                                                        int skip_nonfinite, int* __restrict__ gate) {
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(*sqnorm) * gscale;              // as adamw_kernel forms it
    // a NaN norm compares false, as `norm >= skip_grad` does in the reference: only the guard stops it
    const int gated = ((skip_norm > 0.f && norm >= skip_norm) || (skip_nonfinite && !isfinite(norm))) ? 1 : 0;
    gate[0] = gated;
    gate[1] += gated;
    gate[2] += gated;
}

// adamw_kernel's twin (same math, vector width, grid, tail).  gate[0] != 0: p, m, v are not written (g is still zeroed when asked).
// Otherwise the step count is step - gate[1]: the host counts every call, the device knows how many of them were gated.  The two
// bias corrections are therefore formed here, once per thread in front of the loop (uniform values: no LDS, no barrier).
__global__ __launch_bounds__(256) void adamw_gated_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, long n, float lr, float wd, float b1, float b2,
                                                          float eps, int step_arg, float gscale, float max_norm,
                                                          const double* __restrict__ sqnorm, int zero_grad,
                                                          const int* __restrict__ gate) {
    const long n4 = n >> 2;
    if (gate[0]) {
        if (!zero_grad) return;
        for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
            *(f32x4*)(g + i * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (long i = n4 * 4; i < n; ++i) g[i] = 0.f;
        return;
    }
    int t = step_arg - gate[1];
    if (t < 1) t = 1;
    const float bc1 = (float)(1.0 - pow((double)b1, (double)t));
    const float bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, (double)t));
    float coef = gscale;
    if (max_norm > 0.f && sqnorm) {
        const float total = (float)sqrt(*sqnorm) * gscale;
        coef *= fminf(1.f, max_norm / (total + 1e-6f));
    }
    const float step = lr / bc1, decay = 1.f - lr * wd;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 pp = *(f32x4*)(p + i * 4), gg = *(f32x4*)(g + i * 4), mm = *(f32x4*)(m + i * 4), vv = *(f32x4*)(v + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ge = gg[e] * coef;
            pp[e] *= decay;
            mm[e] = b1 * mm[e] + (1.f - b1) * ge;
            vv[e] = b2 * vv[e] + (1.f - b2) * ge * ge;
            pp[e] -= step * (mm[e] / (sqrtf(vv[e]) / bc2_sqrt + eps));
        }
        *(f32x4*)(p + i * 4) = pp; *(f32x4*)(m + i * 4) = mm; *(f32x4*)(v + i * 4) = vv;
        if (zero_grad) *(f32x4*)(g + i * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (long i = n4 * 4; i < n; ++i) {
            const float ge = g[i] * coef;
            float pe = p[i] * decay;
            const float me = b1 * m[i] + (1.f - b1) * ge, ve = b2 * v[i] + (1.f - b2) * ge * ge;
            pe -= step * (me / (sqrtf(ve) / bc2_sqrt + eps));
            p[i] = pe; m[i] = me; v[i] = ve;
            if (zero_grad) g[i] = 0.f;
        }
    }
}

}  // namespace

extern "C" int ego_adamw_gate(const double* sqnorm, float gscale, float skip_norm, int skip_nonfinite, int* gate,
                              hipStream_t stream) {
    if (!sqnorm || !gate || ((uintptr_t)sqnorm) % 8 || ((uintptr_t)gate) % 4) return EGO_ERR_ARG;
    EGO_LAUNCH(adamw_gate_kernel, dim3(1), dim3(64), 0, stream, sqnorm, gscale, skip_norm, skip_nonfinite, gate);
    LAUNCH_CHECK();
    return EGO_OK;
}

extern "C" int ego_adamw_step_gated(float* p, float* g, float* m, float* v, long n, float lr, float wd, float beta1, float beta2,
                                    float eps, int step, float gscale, float max_norm, const double* sqnorm, int zero_grad,
                                    const int* gate, hipStream_t stream) {
    if (n <= 0) return EGO_OK;
    if (step < 1 || !gate || ((uintptr_t)gate) % 4 || ((uintptr_t)p) % 16 || ((uintptr_t)g) % 16 || ((uintptr_t)m) % 16 ||
        ((uintptr_t)v) % 16)
        return EGO_ERR_ARG;
    const long n4 = n / 4;
    const int blocks = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
    EGO_LAUNCH(adamw_gated_kernel, dim3(blocks < 1 ? 1 : blocks), dim3(256), 0, stream, p, g, m, v, n, lr, wd, beta1, beta2, eps,
                       step, gscale, max_norm, sqnorm, zero_grad, gate);
    LAUNCH_CHECK();
    return EGO_OK;
}

// ---- parameter-group AdamW: every (layer, weight-decay class) group of a layer-wise lr decay in ONE launch ---------------------
//
// Replaces: the per-group loop of torch.optim.AdamW over the groups get_parameter_groups builds (egom2p/utils/optim_factory.py:97-154,
// 226), each at lr * lr_scale (run_training_egom2p.py:707-713).  The flat buffers are cut into segments (contiguous runs of one
// group, one step offset, frozen or not); work is dealt in chunks of EGO_ADAMW_CHUNK floats that never cross a segment, and a
// workgroup finds its chunk's segment by binary search on the segments' first-chunk prefix array.
namespace {

constexpr int SEG_CHUNK = EGO_ADAMW_CHUNK;          // 256 threads x f32x4 x 4
static_assert(SEG_CHUNK == 256 * 4 * 4, "a chunk is four f32x4 per thread of a 256-thread workgroup");

// the per-element expression is adamw_kernel's, term for term, with the three multiply-adds the compiler fuses THERE written as
// fmaf here (decay, the two moments, the parameter update) and contraction switched off for the rest: left to itself the compiler
// fuses the four unrolled copies of this loop differently from adamw_kernel's one, and the two paths would differ in the last bit.
// Everything a workgroup decides (segment, group, frozen, gated) is uniform over it: the table loads are read-only and indexed by
// blockIdx / loop counters alone.
__global__ __launch_bounds__(256) void adamw_seg_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, long n, const ego_adamw_seg* __restrict__ segs,
                                                        int n_segs, const long* __restrict__ chunks, long n_chunks,
                                                        const ego_adamw_hp hp, float b1, float b2, float eps, float gscale,
                                                        float max_norm, const double* __restrict__ sqnorm, int zero_grad,
                                                        const int* __restrict__ gate) {
#pragma clang fp contract(off)
    __shared__ float s_bc1[EGO_ADAMW_MAX_GROUPS], s_bc2[EGO_ADAMW_MAX_GROUPS];
    const int gated = gate ? gate[0] : 0;
    if (gated && !zero_grad) return;
    if (!gated && threadIdx.x < EGO_ADAMW_MAX_GROUPS) {
        const int k = threadIdx.x;
        float bc1 = hp.bc1[k], bc2 = hp.bc2_sqrt[k];
        if (gate && k < hp.n_groups) {             // adamw_gated_kernel's count and corrections, once per group and workgroup
            int t = hp.step[k] - gate[1];
            if (t < 1) t = 1;
            bc1 = (float)(1.0 - pow((double)b1, (double)t));
            bc2 = (float)sqrt(1.0 - pow((double)b2, (double)t));
        }
        s_bc1[k] = bc1;
        s_bc2[k] = bc2;
    }
    __syncthreads();
    float coef = gscale;
    if (max_norm > 0.f && sqnorm) {
        coef *= fminf(1.f, max_norm / fmaf((float)sqrt(*sqnorm), gscale, 1e-6f));       // (total + 1e-6f, fused as adamw_kernel's is)
    }
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        int a = 0, b = n_segs - 1;                  // the last segment whose first chunk is <= c
        while (a < b) {
            const int mid = (a + b + 1) >> 1;
            if (chunks[mid] <= c) a = mid; else b = mid - 1;
        }
        const ego_adamw_seg sg = segs[a];
        const long lo = sg.lo + (c - chunks[a]) * SEG_CHUNK;
        const long hi = lo + SEG_CHUNK < sg.hi ? lo + SEG_CHUNK : sg.hi;
        const int grp = __builtin_amdgcn_readfirstlane(sg.group);
        // (a table that does not fit the buffers or the block is the caller's error - the entry point checks its host copy -
        //  but nothing outside [0, n) or the block is touched even then)
        if (sg.lo < 0 || sg.hi > n || lo < sg.lo || (unsigned)grp >= (unsigned)EGO_ADAMW_MAX_GROUPS) continue;
        if (gated || (sg.flags & EGO_SEG_FROZEN)) {
            if (zero_grad)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const long i = lo + ((long)k * 256 + threadIdx.x) * 4;
                    if (i < hi) *(f32x4*)(g + i) = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            continue;
        }
        const float lr = hp.lr[grp], wd = hp.wd[grp], bc1 = s_bc1[grp], bc2_sqrt = s_bc2[grp];
        const float step = lr / bc1, decay = fmaf(-lr, wd, 1.f);
        f32x4 pp[4], gg[4], mm[4], vv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long i = lo + ((long)k * 256 + threadIdx.x) * 4;
            if (i < hi) { pp[k] = *(f32x4*)(p + i); gg[k] = *(f32x4*)(g + i); mm[k] = *(f32x4*)(m + i); vv[k] = *(f32x4*)(v + i); }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long i = lo + ((long)k * 256 + threadIdx.x) * 4;
            if (i >= hi) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ge = gg[k][e] * coef;
                mm[k][e] = fmaf(b1, mm[k][e], (1.f - b1) * ge);
                vv[k][e] = fmaf(b2, vv[k][e], (1.f - b2) * ge * ge);
                pp[k][e] = fmaf(decay, pp[k][e], -(step * (mm[k][e] / (sqrtf(vv[k][e]) / bc2_sqrt + eps))));
            }
            *(f32x4*)(p + i) = pp[k]; *(f32x4*)(m + i) = mm[k]; *(f32x4*)(v + i) = vv[k];
            if (zero_grad) *(f32x4*)(g + i) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

}  // namespace

extern "C" int ego_adamw_step_seg(float* p, float* g, float* m, float* v, long n, const ego_adamw_seg* segs_host,
                                  const ego_adamw_seg* segs, int n_segs, const long* chunks, const ego_adamw_hp* hp, float beta1,
                                  float beta2, float eps, float gscale, float max_norm, const double* sqnorm, int zero_grad,
                                  const int* gate, hipStream_t stream) {
    if (n_segs < 0 || n < 0 || !hp || hp->n_groups < 0 || hp->n_groups > EGO_ADAMW_MAX_GROUPS) return EGO_ERR_ARG;
    if (((uintptr_t)p) % 16 || ((uintptr_t)g) % 16 || ((uintptr_t)m) % 16 || ((uintptr_t)v) % 16 || ((uintptr_t)gate) % 4 ||
        ((uintptr_t)sqnorm) % 8)
        return EGO_ERR_ARG;
    if (n_segs == 0) return EGO_OK;
    if (!p || !g || !m || !v || !segs_host || !segs || !chunks || ((uintptr_t)segs) % 8 || ((uintptr_t)chunks) % 8) return EGO_ERR_ARG;
    long n_chunks = 0, prev = 0;
    for (int s = 0; s < n_segs; ++s) {
        const ego_adamw_seg& sg = segs_host[s];
        if (sg.lo < prev || sg.hi <= sg.lo || sg.hi > n || (sg.lo & 3) || (sg.hi & 3)) return EGO_ERR_ARG;
        if (sg.group < 0 || sg.group >= hp->n_groups) return EGO_ERR_ARG;
        if (!(sg.flags & EGO_SEG_FROZEN) && hp->step[sg.group] < 1) return EGO_ERR_ARG;
        prev = sg.hi;
        n_chunks += (sg.hi - sg.lo + SEG_CHUNK - 1) / SEG_CHUNK;
    }
    ego_adamw_hp h = *hp;                           // passed by value: the launch owns its copy, the caller may rewrite its block
    if (!gate)
        for (int k = 0; k < h.n_groups; ++k) {      // as ego_adamw_step forms them
            const int t = h.step[k] < 1 ? 1 : h.step[k];
            h.bc1[k] = (float)(1.0 - pow((double)beta1, (double)t));
            h.bc2_sqrt[k] = (float)sqrt(1.0 - pow((double)beta2, (double)t));
        }
    const int blocks = (int)(n_chunks < 4096 ? n_chunks : 4096);
    EGO_LAUNCH(adamw_seg_kernel, dim3(blocks), dim3(256), 0, stream, p, g, m, v, n, segs, n_segs, chunks, n_chunks, h, beta1,
                       beta2, eps, gscale, max_norm, sqnorm, zero_grad, gate);
    LAUNCH_CHECK();
    return EGO_OK;
}

// ---- Adam, SGD with momentum and Nesterov on the segmented launch ---------------------------------------------------------------
//
// Replaces: optim.SGD(momentum, nesterov=True / False) and optim.Adam of create_optimizer (egom2p/utils/optim_factory.py:217-224),
// looped over the groups of :97-154.  adamw_seg_kernel's frame - chunks that never cross a segment, the segment found by binary
// search, everything a workgroup decides uniform over it - with the optimiser kind a template parameter: the SGD kinds carry
// no `v` traffic (20 B per element with zero_grad against 28) and no bias-correction prologue.
namespace {

template <int KIND>
__global__ __launch_bounds__(256) void optim_seg_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, long n, const ego_adamw_seg* __restrict__ segs,
                                                        int n_segs, const long* __restrict__ chunks, long n_chunks,
                                                        const ego_adamw_hp hp, float b1, float b2, float eps, float momentum,
                                                        float gscale, float max_norm, const double* __restrict__ sqnorm,
                                                        int zero_grad, const int* __restrict__ gate) {
    // every multiply-add is written out as fmaf and contraction is off for the rest (as in adamw_seg_kernel): the rounding points
    // are the ones stated here, whatever the unrolling
#pragma clang fp contract(off)
    constexpr bool ADAM = KIND == EGO_OPT_ADAM;
    __shared__ float s_bc1[ADAM ? EGO_ADAMW_MAX_GROUPS : 1], s_bc2[ADAM ? EGO_ADAMW_MAX_GROUPS : 1];
    const int gated = gate ? gate[0] : 0;
    if (gated && !zero_grad) return;
    if (ADAM) {
        if (!gated && threadIdx.x < EGO_ADAMW_MAX_GROUPS) {
            const int k = threadIdx.x;
            float bc1 = hp.bc1[k], bc2 = hp.bc2_sqrt[k];
            if (gate && k < hp.n_groups) {         // adamw_seg_kernel's count and corrections
                int t = hp.step[k] - gate[1];
                if (t < 1) t = 1;
                bc1 = (float)(1.0 - pow((double)b1, (double)t));
                bc2 = (float)sqrt(1.0 - pow((double)b2, (double)t));
            }
            s_bc1[k] = bc1;
            s_bc2[k] = bc2;
        }
        __syncthreads();
    }
    float coef = gscale;
    if (max_norm > 0.f && sqnorm) {
        coef *= fminf(1.f, max_norm / fmaf((float)sqrt(*sqnorm), gscale, 1e-6f));       // adamw_seg_kernel's coef
    }
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        int a = 0, b = n_segs - 1;                  // the last segment whose first chunk is <= c
        while (a < b) {
            const int mid = (a + b + 1) >> 1;
            if (chunks[mid] <= c) a = mid; else b = mid - 1;
        }
        const ego_adamw_seg sg = segs[a];
        const long lo = sg.lo + (c - chunks[a]) * SEG_CHUNK;
        const long hi = lo + SEG_CHUNK < sg.hi ? lo + SEG_CHUNK : sg.hi;
        const int grp = __builtin_amdgcn_readfirstlane(sg.group);
        // (as in adamw_seg_kernel: a table that does not fit is refused by the entry point from its host copy, and nothing outside
        //  [0, n) or the block is touched even if the device copy disagrees with it)
        if (sg.lo < 0 || sg.hi > n || lo < sg.lo || (unsigned)grp >= (unsigned)EGO_ADAMW_MAX_GROUPS) continue;
        if (gated || (sg.flags & EGO_SEG_FROZEN)) {
            if (zero_grad)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const long i = lo + ((long)k * 256 + threadIdx.x) * 4;
                    if (i < hi) *(f32x4*)(g + i) = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            continue;
        }
        const float lr = hp.lr[grp], wd = hp.wd[grp];
        float step = lr, bc2_sqrt = 1.f;
        if (ADAM) {
            step = lr / s_bc1[grp];
            bc2_sqrt = s_bc2[grp];
        }
        f32x4 pp[4], gg[4], mm[4], vv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long i = lo + ((long)k * 256 + threadIdx.x) * 4;
            if (i < hi) {
                pp[k] = *(f32x4*)(p + i); gg[k] = *(f32x4*)(g + i); mm[k] = *(f32x4*)(m + i);
                if (ADAM) vv[k] = *(f32x4*)(v + i);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long i = lo + ((long)k * 256 + threadIdx.x) * 4;
            if (i >= hi) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = fmaf(wd, pp[k][e], gg[k][e] * coef);
                if (ADAM) {
                    mm[k][e] = fmaf(b1, mm[k][e], (1.f - b1) * d);
                    vv[k][e] = fmaf(b2, vv[k][e], (1.f - b2) * d * d);
                    pp[k][e] = fmaf(-step, mm[k][e] / (sqrtf(vv[k][e]) / bc2_sqrt + eps), pp[k][e]);
                } else {
                    mm[k][e] = fmaf(momentum, mm[k][e], d);
                    const float u = KIND == EGO_OPT_NESTEROV ? fmaf(momentum, mm[k][e], d) : mm[k][e];
                    pp[k][e] = fmaf(-lr, u, pp[k][e]);
                }
            }
            *(f32x4*)(p + i) = pp[k]; *(f32x4*)(m + i) = mm[k];
            if (ADAM) *(f32x4*)(v + i) = vv[k];
            if (zero_grad) *(f32x4*)(g + i) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

}  // namespace

extern "C" int ego_optim_step_seg(float* p, float* g, float* m, float* v, long n, const ego_adamw_seg* segs_host,
                                  const ego_adamw_seg* segs, int n_segs, const long* chunks, const ego_adamw_hp* hp, float beta1,
                                  float beta2, float eps, float gscale, float max_norm, const double* sqnorm, int zero_grad,
                                  const int* gate, int kind, float momentum, hipStream_t stream) {
    if (kind != EGO_OPT_ADAM && kind != EGO_OPT_SGD && kind != EGO_OPT_NESTEROV) return EGO_ERR_ARG;
    const bool adam = kind == EGO_OPT_ADAM;
    if (!adam && !(momentum >= 0.f && momentum <= 3.0e38f)) return EGO_ERR_ARG;             // (NaN and inf fail the comparisons)
    if (n_segs < 0 || n < 0 || !hp || hp->n_groups < 0 || hp->n_groups > EGO_ADAMW_MAX_GROUPS) return EGO_ERR_ARG;
    if (((uintptr_t)p) % 16 || ((uintptr_t)g) % 16 || ((uintptr_t)m) % 16 || (adam && (!v || ((uintptr_t)v) % 16)) ||
        ((uintptr_t)gate) % 4 || ((uintptr_t)sqnorm) % 8)
        return EGO_ERR_ARG;
    if (n_segs == 0) return EGO_OK;
    if (!p || !g || !m || !segs_host || !segs || !chunks || ((uintptr_t)segs) % 8 || ((uintptr_t)chunks) % 8) return EGO_ERR_ARG;
    long n_chunks = 0, prev = 0;
    for (int s = 0; s < n_segs; ++s) {
        const ego_adamw_seg& sg = segs_host[s];
        if (sg.lo < prev || sg.hi <= sg.lo || sg.hi > n || (sg.lo & 3) || (sg.hi & 3)) return EGO_ERR_ARG;
        if (sg.group < 0 || sg.group >= hp->n_groups) return EGO_ERR_ARG;
        if (adam && !(sg.flags & EGO_SEG_FROZEN) && hp->step[sg.group] < 1) return EGO_ERR_ARG;
        prev = sg.hi;
        n_chunks += (sg.hi - sg.lo + SEG_CHUNK - 1) / SEG_CHUNK;
    }
    ego_adamw_hp h = *hp;                           // passed by value, as in ego_adamw_step_seg
    if (adam && !gate)
        for (int k = 0; k < h.n_groups; ++k) {      // as ego_adamw_step forms them
            const int t = h.step[k] < 1 ? 1 : h.step[k];
            h.bc1[k] = (float)(1.0 - pow((double)beta1, (double)t));
            h.bc2_sqrt[k] = (float)sqrt(1.0 - pow((double)beta2, (double)t));
        }
    const int blocks = (int)(n_chunks < 4096 ? n_chunks : 4096);
    if (adam) {
        EGO_LAUNCH(optim_seg_kernel<EGO_OPT_ADAM>, dim3(blocks), dim3(256), 0, stream, p, g, m, v, n, segs, n_segs, chunks, n_chunks,
                   h, beta1, beta2, eps, momentum, gscale, max_norm, sqnorm, zero_grad, gate);
    } else if (kind == EGO_OPT_SGD) {
        EGO_LAUNCH(optim_seg_kernel<EGO_OPT_SGD>, dim3(blocks), dim3(256), 0, stream, p, g, m, (float*)nullptr, n, segs, n_segs,
                   chunks, n_chunks, h, beta1, beta2, eps, momentum, gscale, max_norm, sqnorm, zero_grad, gate);
    } else {
        EGO_LAUNCH(optim_seg_kernel<EGO_OPT_NESTEROV>, dim3(blocks), dim3(256), 0, stream, p, g, m, (float*)nullptr, n, segs, n_segs,
                   chunks, n_chunks, h, beta1, beta2, eps, momentum, gscale, max_norm, sqnorm, zero_grad, gate);
    }
    LAUNCH_CHECK();
    return EGO_OK;
}

// ---- model EMA: a moving average of the flat parameter buffer, and the in-place exchange that applies it ---------------------
//
// Replaces: ModelEmaV2.update (egom2p/utils/timm/model_ema.py:128-132: `ema_v.copy_(decay * ema_v + (1 - decay) * model_v)` per
// state-dict tensor) by one pass over the flat buffer, and the deepcopy'd module of :111 by exchanging the contents of the two
// buffers (parameter views and captured graphs keep their addresses).  Both are HBM-bound streams: 12 and 16 B per element.
namespace {

// one fma: the same expression in the vector body and in the tail, whatever the compiler would contract
__device__ __forceinline__ float ema_one(float e, float p, float d, float omd) { return fmaf(d, e, omd * p); }

__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, float d,
                                                         float omd) {
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 ee = *(f32x4*)(ema + i * 4);
        const f32x4 pp = *(const f32x4*)(p + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) ee[e] = ema_one(ee[e], pp[e], d, omd);
        *(f32x4*)(ema + i * 4) = ee;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long i = n4 * 4; i < n; ++i) ema[i] = ema_one(ema[i], p[i], d, omd);
}

// bit patterns, not values: 32-bit integer loads and stores, no arithmetic (NaN payloads, -0.0 and denormals survive)
__global__ __launch_bounds__(256) void swap_u32_kernel(unsigned* __restrict__ a, unsigned* __restrict__ b, long n) {
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const u32x4 va = *(const u32x4*)(a + i * 4), vb = *(const u32x4*)(b + i * 4);
        *(u32x4*)(a + i * 4) = vb;
        *(u32x4*)(b + i * 4) = va;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long i = n4 * 4; i < n; ++i) {
            const unsigned t = a[i];
            a[i] = b[i];
            b[i] = t;
        }
}

// two ranges of n floats each: both given, 16-byte aligned, disjoint
bool flat_pair_ok(const void* a, const void* b, long n) {
    if (!a || !b || ((uintptr_t)a) % 16 || ((uintptr_t)b) % 16) return false;
    const uintptr_t lo = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)a : (uintptr_t)b;
    const uintptr_t hi = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)b : (uintptr_t)a;
    return hi - lo >= (uintptr_t)n * sizeof(float);
}

int flat_blocks(long n) {       // the grid adamw_kernel takes: capped, the kernels stride over the rest with 64-bit indices
    const long n4 = n / 4;
    const int blocks = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
    return blocks < 1 ? 1 : blocks;
}

}  // namespace

extern "C" int ego_ema_update(float* ema, const float* p, long n, float decay, float one_minus_decay, hipStream_t stream) {
    if (n < 0 || !(decay >= 0.f && decay <= 1.f) || !(one_minus_decay >= 0.f && one_minus_decay <= 1.f)) return EGO_ERR_ARG;
    if (n == 0) return EGO_OK;
    if (!flat_pair_ok(ema, p, n)) return EGO_ERR_ARG;
    EGO_LAUNCH(ema_update_kernel, dim3(flat_blocks(n)), dim3(256), 0, stream, ema, p, n, decay, one_minus_decay);
    LAUNCH_CHECK();
    return EGO_OK;
}

extern "C" int ego_swap_f32(float* a, float* b, long n, hipStream_t stream) {
    if (n < 0) return EGO_ERR_ARG;
    if (n == 0) return EGO_OK;
    if (!flat_pair_ok(a, b, n)) return EGO_ERR_ARG;
    EGO_LAUNCH(swap_u32_kernel, dim3(flat_blocks(n)), dim3(256), 0, stream, (unsigned*)a, (unsigned*)b, n);
    LAUNCH_CHECK();
    return EGO_OK;
}
