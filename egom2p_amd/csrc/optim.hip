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
