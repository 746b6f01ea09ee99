// Stochastic depth (drop path) of the reference's residual blocks (egom2p_utils.py:89-112 `drop_path` / `DropPath`, applied at
// :356-359 and :387-391): per residual site and SAMPLE one Bernoulli(keep_prob) decision; a kept sample's branch is divided by
// keep_prob, a dropped sample's branch does not reach the residual stream.  Three HBM-bound row kernels:
//   draw   the decisions of all sites of one forward, from the counter-based generator of mask.hip (splitmix64): a pure function of
//          (seed, forward counter, site, sample) - reproducible, independent of the batch size, no host sync;
//   resid  out(f32) = R(f32) + (keep ? bf16(float(branch) / keep_prob) : 0): the residual add of a training forward behind a branch
//          whose last linear left bf16 (`x.div(keep_prob) * random_tensor` under autocast: a bf16 result);
//   scale  dst(bf16) = keep ? bf16(float(src) / keep_prob) : 0: the branch's upstream gradient, at the entry of its backward.
// `/` is the correctly rounded fp32 divide (hipcc's default for HIP: v_div_scale / v_div_fmas / v_div_fixup, no reciprocal
// multiply; the build passes no fast-math flag), so the results are bit for bit torch's `branch.float() / keep_prob`.
#include "common.h"
#include "egom2p_hip.h"

namespace {

constexpr int DP_ROWS = 16;         // whole rows per workgroup and pass: one decision lookup per row, dropped rows skip the branch read

__global__ void droppath_draw_kernel(const float* __restrict__ keep_prob, int n_sites, int B, uint64_t seed, uint64_t counter,
                                     unsigned char* __restrict__ keep) {
    const long total = (long)n_sites * B;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int s = (int)(idx / B), b = (int)(idx % B);
        const uint64_t key = splitmix(splitmix(seed, counter), (uint64_t)s);
        // top 24 bits against floor(keep_prob * 2^24): the product is exact in fp32 (a power of two), so the host restates it in integers
        const unsigned thr = (unsigned)floorf(keep_prob[s] * 16777216.0f);
        keep[idx] = (unsigned)(splitmix(key, (uint64_t)b) >> 40) < thr ? 1 : 0;
    }
}

// bf16(float(v) / kp) of the two halves of a packed pair
__device__ __forceinline__ unsigned div_pair(unsigned v, float kp) {
    return pack_bf16x2(bf16_to_f32(v & 0xffff) / kp, bf16_to_f32(v >> 16) / kp);
}

// 8 columns (16 B of bf16, 2 x 16 B of fp32) per thread and step; columns [width, wc * 8) - the pad of a row whose logical width is no
// multiple of 8 - leave as zeros.  R and out may be the same buffer: every thread reads its chunk of R before it writes it.
__global__ __launch_bounds__(256) void droppath_resid_kernel(const float* R, long ld_r, const bf16_t* __restrict__ branch, long ld_b,
                                                             float* out, long ld_o, const unsigned char* __restrict__ keep,
                                                             long rows, int rps, int width, float kp) {
    const int wc = (width + 7) >> 3;
    const long groups = (rows + DP_ROWS - 1) / DP_ROWS;
    for (long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long r0 = g * DP_ROWS;
        const int nr = (int)(rows - r0 < DP_ROWS ? rows - r0 : DP_ROWS);
        for (int i = threadIdx.x; i < nr * wc; i += blockDim.x) {
            const long r = r0 + i / wc;
            const int c = (i % wc) * 8;
            f32x4 a = *(const f32x4*)(R + r * ld_r + c), b = *(const f32x4*)(R + r * ld_r + c + 4);
            u32x4 v = {0u, 0u, 0u, 0u};                     // a dropped sample adds +0 like the reference's branch * 0 (-0 + 0 = +0)
            if (keep[r / rps]) {
                const u32x4 t = *(const u32x4*)(branch + r * ld_b + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = div_pair(t[e], kp);
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                a[2 * e] += bf16_to_f32(v[e] & 0xffff); a[2 * e + 1] += bf16_to_f32(v[e] >> 16);
                b[2 * e] += bf16_to_f32(v[e + 2] & 0xffff); b[2 * e + 1] += bf16_to_f32(v[e + 2] >> 16);
            }
            if (c + 8 > width) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { if (c + e >= width) a[e] = 0.f; if (c + 4 + e >= width) b[e] = 0.f; }
            }
            *(f32x4*)(out + r * ld_o + c) = a;
            *(f32x4*)(out + r * ld_o + c + 4) = b;
        }
    }
}

__global__ __launch_bounds__(256) void droppath_scale_kernel(const bf16_t* __restrict__ src, long ld_s, bf16_t* __restrict__ dst, long ld_d,
                                                             const unsigned char* __restrict__ keep, long rows, int rps, int width, float kp) {
    const int wc = (width + 7) >> 3;
    const long groups = (rows + DP_ROWS - 1) / DP_ROWS;
    for (long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long r0 = g * DP_ROWS;
        const int nr = (int)(rows - r0 < DP_ROWS ? rows - r0 : DP_ROWS);
        for (int i = threadIdx.x; i < nr * wc; i += blockDim.x) {
            const long r = r0 + i / wc;
            const int c = (i % wc) * 8;
            u32x4 o = {0u, 0u, 0u, 0u};
            if (keep[r / rps]) {
                const u32x4 v = *(const u32x4*)(src + r * ld_s + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = div_pair(v[e], kp);
                if (c + 8 > width) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (c + 2 * e >= width) o[e] = 0u;
                        else if (c + 2 * e + 1 >= width) o[e] &= 0xffffu;
                    }
                }
            }
            *(u32x4*)(dst + r * ld_d + c) = o;
        }
    }
}

inline bool rows_ok(const void* a, const void* b, const void* keep, long rows, int rps, int n_samples, int width, float kp, long ld_a, long ld_b) {
    const long wpad = ((long)width + 7) / 8 * 8;
    return a && b && keep && rows >= 0 && rps > 0 && n_samples > 0 && rows <= (long)n_samples * rps && width > 0 && kp > 0.f && kp <= 1.f &&
           ld_a >= wpad && ld_b >= wpad && ld_a % 8 == 0 && ld_b % 8 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0;
}

inline int grid_rows(long rows) {
    const long g = (rows + DP_ROWS - 1) / DP_ROWS;
    return (int)(g < 4096 ? g : 4096);
}

}  // namespace

extern "C" int ego_droppath_draw(const float* keep_prob, int n_sites, int B, unsigned long long seed, unsigned long long counter,
                                 void* keep, hipStream_t stream) {
    if (n_sites <= 0 || B <= 0) return EGO_OK;
    if (!keep_prob || !keep) return EGO_ERR_ARG;
    const long total = (long)n_sites * B;
    EGO_LAUNCH(droppath_draw_kernel, dim3((unsigned)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024)), dim3(256), 0, stream,
               keep_prob, n_sites, B, (uint64_t)seed, (uint64_t)counter, (unsigned char*)keep);
    LAUNCH_CHECK();
    return EGO_OK;
}

extern "C" int ego_droppath_resid(const float* R, long ld_r, const void* branch, long ld_b, float* out, long ld_o, const void* keep,
                                  long rows, int rows_per_sample, int n_samples, int width, float keep_prob, hipStream_t stream) {
    if (!rows_ok(R, branch, keep, rows, rows_per_sample, n_samples, width, keep_prob, ld_r, ld_b) || !out || ((uintptr_t)out & 15) ||
        ld_o < ((long)width + 7) / 8 * 8 || ld_o % 8)
        return EGO_ERR_ARG;
    if (rows == 0) return EGO_OK;
    EGO_LAUNCH(droppath_resid_kernel, dim3(grid_rows(rows)), dim3(256), 0, stream, R, ld_r, (const bf16_t*)branch, ld_b, out, ld_o,
               (const unsigned char*)keep, rows, rows_per_sample, width, keep_prob);
    LAUNCH_CHECK();
    return EGO_OK;
}

extern "C" int ego_droppath_scale(const void* src, long ld_s, void* dst, long ld_d, const void* keep, long rows, int rows_per_sample,
                                  int n_samples, int width, float keep_prob, hipStream_t stream) {
    if (!rows_ok(src, dst, keep, rows, rows_per_sample, n_samples, width, keep_prob, ld_s, ld_d)) return EGO_ERR_ARG;
    if (rows == 0) return EGO_OK;
    EGO_LAUNCH(droppath_scale_kernel, dim3(grid_rows(rows)), dim3(256), 0, stream, (const bf16_t*)src, ld_s, (bf16_t*)dst, ld_d,
               (const unsigned char*)keep, rows, rows_per_sample, width, keep_prob);
    LAUNCH_CHECK();
    return EGO_OK;
}
