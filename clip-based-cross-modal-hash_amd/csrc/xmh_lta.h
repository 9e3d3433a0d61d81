// MITH LocalizedTokenAggregation (models/MITH/hash/hash.py:109-169) + positional encoding (:41-65): the body of the kernel, shared by
// the eval path (k_lta_aggregate of xmh_encode.hip, which keeps nothing) and the training forward (xmh_mith_grad.hip), which also
// stores the attention A [B, K, L] that its backward multiplies by.  One statement of the selection and the softmax, so the two
// cannot drift apart; every output of the eval kernel is computed exactly as before.
//   sim = S (+ -inf on masked tokens); sim = sim > 0 ? sim : -inf                                   (:142-153)
//   per token keep the concepts >= its top_k-th largest score (ties kept), others -inf                (:114-124)
//   softmax over the TOKEN axis per (sample, concept); a concept with no token gives NaN -> 0         (:159-160)
//   M[b,k,:] = sum_l A[b,k,l] X[b,l,:]   (+ pe[k,:], the sin/cos table already divided by sqrt(D))    (:164-168, :63)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xmh {

// grid (B, ceil(D / 64)), 256 threads; sm: (L (K + 1) + L) floats of LDS.  S [B, L, K] concept scores (tanh outputs), X [B, L, D] raw
// CLIP tokens.  kStoreA: the blocks of column 0 write A [B, K, L] (exact zeros where a token is not kept).
template <bool kStoreA>
__device__ __forceinline__ void lta_aggregate_block(float* sm, const float* __restrict__ S, const float* __restrict__ X,
                                                    const uint8_t* __restrict__ mask, const float* __restrict__ pe, float* __restrict__ M,
                                                    float* __restrict__ A, int L, int K, int D, int topk) {
    // every block rebuilds the [L][K] attention of its sample (cheap, all 256 threads) and aggregates 64 feature columns -- one
    // block per sample left 60 % of the CUs idle and ran 0.46 ms
    const int b = blockIdx.x;
    const int ld = K + 1;
    float* thr_s = sm + L * ld;
    for (int e = threadIdx.x; e < L * K; e += 256) {
        const int l = e / K, k = e % K;
        float v = S[((int64_t)b * L + l) * K + k];
        if (mask && mask[(int64_t)b * L + l]) v = -INFINITY;
        sm[l * ld + k] = v > 0.0f ? v : -INFINITY;
    }
    for (int l = threadIdx.x; l < L; l += 256) thr_s[l] = -INFINITY;
    __syncthreads();
    // per-token top-k threshold: the value v with #(> v) < topk <= #(>= v); one (token, candidate) pair per thread step.
    // Several candidates of a row can qualify only if they are equal, so the racing stores write the same value.
    for (int e = threadIdx.x; e < L * K; e += 256) {
        const int l = e / K, i = e % K;
        const float* row = sm + l * ld;
        const float v = row[i];
        int gt = 0, ge = 0;
        for (int j = 0; j < K; ++j) {
            gt += row[j] > v;
            ge += row[j] >= v;
        }
        if (gt < topk && topk <= ge) thr_s[l] = v;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < L * K; e += 256) {
        const int l = e / K, i = e % K;
        if (!(sm[l * ld + i] >= thr_s[l])) sm[l * ld + i] = -INFINITY;
    }
    __syncthreads();
    // softmax over tokens per concept
    for (int k = threadIdx.x; k < K; k += 256) {
        float mx = -INFINITY;
        for (int l = 0; l < L; ++l) mx = fmaxf(mx, sm[l * ld + k]);
        if (mx == -INFINITY) {
            for (int l = 0; l < L; ++l) sm[l * ld + k] = 0.0f;                       // NaN -> 0 in the reference
        } else {
            float sum = 0.0f;
            for (int l = 0; l < L; ++l) {
                const float p = expf(sm[l * ld + k] - mx);
                sm[l * ld + k] = p;
                sum += p;
            }
            for (int l = 0; l < L; ++l) sm[l * ld + k] = sm[l * ld + k] / sum;
        }
    }
    __syncthreads();
    if (kStoreA) {
        if (blockIdx.y == 0)
            for (int e = threadIdx.x; e < L * K; e += 256) {
                const int k = e / L, l = e % L;
                A[((int64_t)b * K + k) * L + l] = sm[l * ld + k];
            }
    }
    // aggregate 64 feature columns: thread = (column, quarter of the concepts), 16 concepts at a time in registers
    const int d = blockIdx.y * 64 + (threadIdx.x & 63);
    const int kq = threadIdx.x >> 6;                                 // 0..3
    if (d >= D) return;
    for (int k0 = kq * 16; k0 < K; k0 += 64) {
        float acc[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc[u] = 0.0f;
        for (int l = 0; l < L; ++l) {
            const float x = X[((int64_t)b * L + l) * D + d];
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (k0 + u < K) acc[u] = fmaf(sm[l * ld + k0 + u], x, acc[u]);
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (k0 + u < K) M[((int64_t)b * K + k0 + u) * D + d] = acc[u] + (pe ? pe[(int64_t)(k0 + u) * D + d] : 0.0f);
    }
}

// LDS bytes of the body above
inline size_t lta_lds_bytes(int L, int K) { return ((size_t)L * (K + 1) + L) * sizeof(float); }
constexpr size_t kLtaMaxLds = 160 * 1024;

}  // namespace xmh
