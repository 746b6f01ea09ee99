// MaskGIT parallel decoding: the device work around the sampler (gfx950).
//
// Replaces, per schedule step of the reference's GenerationSampler (egom2p/models/generate.py):
//   * ego_maskgit_positions - the decoder row order of forward_mask_decoder_maskgit (:463-467):
//     `argsort(target_mask + arange(T) * 1e-6)[:, :M]` = the open positions (mask false) ascending, then the closed ones
//     ascending.  One workgroup per batch row; a block prefix scan of the open flags gives every position its rank - no sort.
//   * ego_maskgit_select - select_tokens_batched's `torch.topk(sampled_probs, num_select)` (:393-402) and the three scatters of
//     maskgit_step_batched / guided_maskgit_step_batched (:660-663, :697-703).  One 1024-thread workgroup per batch row, the
//     row's M <= 8192 probabilities in registers (8 per lane, lane t owns decoder rows 8t .. 8t+7).  The K-th largest
//     probability is found WITHOUT sorting by a 31-step binary search on the bit pattern of p (p >= 0: the integer order of the
//     bits is the order of the values - the search sample_kernel runs for the nucleus cut); every row strictly above it is
//     taken, the remainder is filled from the rows EQUAL to it in ascending decoder-row order (block prefix scan).  That tie
//     rule is this engine's: torch.topk leaves the order of equal values unspecified, and at temperature 0 every probability
//     is 1.  No atomics, plain stores, one writer per element: results are bitwise reproducible.
#include "common.h"
#include "egom2p_hip.h"

namespace {

constexpr int MG_THREADS = 1024;
constexpr int MG_WAVES = MG_THREADS / 64;
constexpr int MG_PER = 8;                          // probabilities per lane
constexpr int MG_MAX_M = MG_THREADS * MG_PER;      // 8192

// block-wide sum of an int over 1024 threads; result broadcast to all threads
__device__ __forceinline__ int mg_block_sum(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int i = 0; i < MG_WAVES; ++i) t += red[i];
    return t;
}

// block-wide EXCLUSIVE prefix sum of an int over 1024 threads (thread order); `total` = sum over the block
__device__ __forceinline__ int mg_block_excl(int v, int* red, int& total) {
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if ((threadIdx.x & 63) >= o) incl += t;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = incl;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < MG_WAVES; ++i) {
        if (i < (int)(threadIdx.x >> 6)) base += red[i];
        total += red[i];
    }
    return base + incl - v;
}

__global__ __launch_bounds__(MG_THREADS) void maskgit_positions_kernel(const unsigned char* __restrict__ mask, int T, int M,
                                                                       long* __restrict__ out) {
    __shared__ int red[MG_WAVES];
    const int tid = threadIdx.x;
    const unsigned char* m = mask + (long)blockIdx.x * T;
    long* o = out + (long)blockIdx.x * M;
    // open positions of the row
    int mine = 0;
    for (int i = tid; i < T; i += MG_THREADS) mine += m[i] ? 0 : 1;
    const int n_open = mg_block_sum(mine, red);
    // rank of position i: open -> number of open positions before it; closed -> n_open + number of closed positions before it
    int base = 0;                                   // open positions in the chunks before this one
    for (int c0 = 0; c0 < T; c0 += MG_THREADS) {
        const int i = c0 + tid;
        const int open = (i < T && !m[i]) ? 1 : 0;
        int chunk;
        const int before = base + mg_block_excl(open, red, chunk);
        if (i < T) {
            const int dst = open ? before : n_open + (i - before);
            if (dst < M) o[dst] = i;
        }
        base += chunk;
    }
}

__global__ __launch_bounds__(MG_THREADS) void maskgit_select_kernel(const int* __restrict__ tokens, const float* __restrict__ probs,
                                                                    const long* __restrict__ positions, int M, int T, int K,
                                                                    long* __restrict__ tensor, unsigned char* __restrict__ input_mask,
                                                                    unsigned char* __restrict__ target_mask, long* __restrict__ out_idx) {
    __shared__ int red[MG_WAVES];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const int r0 = tid * MG_PER;
    const int nv = min(max(M - r0, 0), MG_PER);     // decoder rows this lane owns
    unsigned key[MG_PER];
#pragma unroll
    for (int e = 0; e < MG_PER; ++e) {
        const unsigned u = (e < nv) ? __float_as_uint(probs[b * M + r0 + e]) : 0u;
        key[e] = (u & 0x80000000u) ? 0u : u;        // p >= 0; a negative value (never a probability) ranks with 0
    }
    // the K-th largest: the largest pattern `lo` with count{key >= lo} >= K (1 <= K <= M: lo = 0 always qualifies)
    unsigned lo = 0u, hi = 0x7fffffffu;
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1) + ((hi - lo) & 1u);       // upper middle: the loop ends at the LARGEST such pattern
        int c = 0;
#pragma unroll
        for (int e = 0; e < MG_PER; ++e) c += (e < nv && key[e] >= mid) ? 1 : 0;
        if (mg_block_sum(c, red) >= K) lo = mid; else hi = mid - 1u;
    }
    const unsigned kth = lo;
    int above = 0, equal = 0;
#pragma unroll
    for (int e = 0; e < MG_PER; ++e) {
        above += (e < nv && key[e] > kth) ? 1 : 0;
        equal += (e < nv && key[e] == kth) ? 1 : 0;
    }
    const int n_above = mg_block_sum(above, red);   // < K by the choice of kth
    const int need = K - n_above;                   // rows equal to the K-th value that are taken: the first `need` in row order
    int n_equal;
    int eq_before = mg_block_excl(equal, red, n_equal);
    unsigned take = 0u;                             // bit e: row r0 + e is committed
    int n_take = 0;
#pragma unroll
    for (int e = 0; e < MG_PER; ++e) {
        if (e < nv) {
            bool t = key[e] > kth;
            if (key[e] == kth) { t = eq_before < need; ++eq_before; }
            if (t) { take |= 1u << e; ++n_take; }
        }
    }
    int total;
    int slot = mg_block_excl(n_take, red, total);   // total == K
#pragma unroll
    for (int e = 0; e < MG_PER; ++e) {
        if (take & (1u << e)) {
            const int r = r0 + e;
            const long pos = positions[b * M + r];
            if (pos >= 0 && pos < T) {
                tensor[b * T + pos] = tokens[b * M + r];
                input_mask[b * T + pos] = 0;
                target_mask[b * T + pos] = 1;
            }
            if (out_idx && slot < K) out_idx[b * K + slot] = r;
            ++slot;
        }
    }
}

}  // namespace

extern "C" int ego_maskgit_positions(const void* target_mask, int B, int T, int M, long* out_pos, hipStream_t stream) {
    if (B < 0 || T < 0 || M < 0 || M > T) return EGO_ERR_ARG;
    if (B == 0 || M == 0) return EGO_OK;
    if (!target_mask || !out_pos) return EGO_ERR_ARG;
    EGO_LAUNCH(maskgit_positions_kernel, dim3(B), dim3(MG_THREADS), 0, stream, (const unsigned char*)target_mask, T, M, out_pos);
    LAUNCH_CHECK();
    return EGO_OK;
}

extern "C" int ego_maskgit_select(const int* tokens, const float* probs, const long* positions, int B, int M, int T, int num_select,
                                  long* tensor, void* input_mask, void* target_mask, long* out_idx, hipStream_t stream) {
    if (B < 0 || M < 0 || T < 0 || num_select < 0 || M > MG_MAX_M) return EGO_ERR_ARG;
    const int K = num_select < M ? num_select : M;
    if (B == 0 || K == 0) return EGO_OK;
    if (!tokens || !probs || !positions || !tensor || !input_mask || !target_mask) return EGO_ERR_ARG;
    EGO_LAUNCH(maskgit_select_kernel, dim3(B), dim3(MG_THREADS), 0, stream, tokens, probs, positions, M, T, K, tensor,
               (unsigned char*)input_mask, (unsigned char*)target_mask, out_idx);
    LAUNCH_CHECK();
    return EGO_OK;
}
