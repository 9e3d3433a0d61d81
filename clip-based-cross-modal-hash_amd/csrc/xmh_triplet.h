// The label-weighted triplet term over a [B, B] distance table (reference models/DIMCH/loss/triplet_loss.py:16-88), as the objectives of
// DIMCH (xmh_dimch.hip) and UMoED (xmh_umoed.hip) both take it: the anchor row's weights, its sum of positive triplets with their
// count, and d / d D of the row.  Blocks of kThreads threads, one anchor row per block; every sum has one fixed order.  Each of the
// two files gets its own copy of these inline functions; the kernels around them (where the distances come from, where the results
// go) stay with the files.
#pragma once
#include "xmh_device.h"

namespace xmh {
namespace trip {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxB = 512;

__device__ __forceinline__ float clamp0(float v) { return v < 0.0f ? 0.0f : v; }                       // torch.clamp(v, 0): NaN stays

// Anchor row `row`: label overlaps c[p], sim[p] = c > 0, weights w[p] = (2^c - 1) / Z, Z = sum_j (2^{c_(j)} - 1) / log2(j + 2) over the row
// sorted descending (the rank of p: columns with a larger count, then equal ones to its left).  All in LDS [B].  Ends with a barrier.
__device__ __forceinline__ void weights(const uint32_t* __restrict__ lab, int Lw, int B, int row, int* cs, float* wsh, float* sim, double* dsh) {
    for (int p = threadIdx.x; p < B; p += kThreads) {
        int c = 0;
        for (int l = 0; l < Lw; ++l) c += __popc(lab[(int64_t)row * Lw + l] & lab[(int64_t)p * Lw + l]);
        cs[p] = c;
    }
    __syncthreads();
    double z = 0.0;
    for (int p = threadIdx.x; p < B; p += kThreads) {
        const int c = cs[p];
        int rank = 0;
        for (int q = 0; q < B; ++q) rank += (cs[q] > c) || (cs[q] == c && q < p);
        z += ((double)ldexpf(1.0f, c) - 1.0) / log2((double)(rank + 2));
    }
    const float Z = (float)xmh::block_sum<kWaves>(z, dsh);
    for (int p = threadIdx.x; p < B; p += kThreads) {
        wsh[p] = (ldexpf(1.0f, cs[p]) - 1.0f) / Z;               // Z = 0 (a row without a label): 0 / 0 = NaN, as in the reference
        sim[p] = cs[p] > 0 ? 1.0f : 0.0f;
    }
    __syncthreads();
}

// the anchor's sum of positive triplets and their count over the distance row ds [B] (LDS); both valid on every thread
__device__ __forceinline__ void row_terms(const float* wsh, const float* sim, const float* ds, int B, float mg, double* dsh, double* sum_out,
                                          double* cnt_out) {
    double sum = 0.0, cnt = 0.0;
    for (int p = threadIdx.x; p < B; p += kThreads) {
        const float wp = wsh[p], sp = sim[p], dp = ds[p];
        for (int n = 0; n < B; ++n) {
            const float v = ((wp - wsh[n]) * (sp * (1.0f - sim[n]))) * ((dp - ds[n]) + mg);
            sum += (double)clamp0(v);
            cnt += v > 1e-16f ? 1.0 : 0.0;
        }
    }
    *sum_out = xmh::block_sum<kWaves>(sum, dsh);
    *cnt_out = xmh::block_sum<kWaves>(cnt, dsh);
}

// d (the anchor's sum) / d ds[p]: column p's own triplets (a, p, *) and those in which it is the negative (a, *, p)
__device__ __forceinline__ float col_grad(const float* wsh, const float* sim, const float* ds, int B, float mg, int p) {
    const float wp = wsh[p], sp = sim[p], dp = ds[p];
    double acc = 0.0;
    for (int n = 0; n < B; ++n) {
        const float c1 = (wp - wsh[n]) * (sp * (1.0f - sim[n]));          // p the positive, n the negative
        const float v1 = c1 * ((dp - ds[n]) + mg);
        acc += (double)(c1 * (v1 >= 0.0f ? 1.0f : 0.0f));
        const float c2 = (wsh[n] - wp) * (sim[n] * (1.0f - sp));          // n the positive, p the negative
        const float v2 = c2 * ((ds[n] - dp) + mg);
        acc -= (double)(c2 * (v2 >= 0.0f ? 1.0f : 0.0f));
    }
    return (float)acc;
}

// sum of v [n] in double, the threads' strided partials through block_sum; valid on every thread
__device__ __forceinline__ double ordered_sum(const double* v, int n, double* dsh) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads) s += v[i];
    return xmh::block_sum<kWaves>(s, dsh);
}

}  // namespace trip
}  // namespace xmh
