// Row primitives of the objectives that L2-normalise their rows as F.normalize does (xmh_hyp, xmh_dnph; xmh_dimch and xmh_umoed take
// inv_norm): the clamped reciprocal norm, the norm of a row by one wave, the backward of the normalisation, and the label-bit test
// of rows packed by xmh_pack_labels.  Each including file gets its own copy of these inline functions; block sizes and the eps come
// from the caller.
#pragma once
#include <stdint.h>

#include "xmh_device.h"

namespace xmh {

// 1 / max(n, eps) as clamp_min forms it: a NaN norm stays NaN (fmaxf would drop it)
__device__ __forceinline__ float inv_norm(float n, float eps) { return 1.0f / (n < eps ? eps : n); }

__device__ __forceinline__ bool has_label(const uint32_t* lab, int Lw, int row, int c) {
    return (lab[(int64_t)row * Lw + (c >> 5)] >> (c & 31)) & 1u;
}

// |v| of a row the wave can read, every lane in the same order (lane, lane + 64, ...) wherever it is called
__device__ __forceinline__ float wave_norm(const float* v, int K) {
    const int lane = threadIdx.x & 63;
    float s = 0.0f;
    for (int k = lane; k < K; k += 64) s = fmaf(v[k], v[k], s);
    return sqrtf(wave_sum(s));
}

// dv of F.normalize for one row v (in LDS) of norm nv, with du in the thread's column slots (column threadIdx.x + r kThreads in
// slot r), written / accumulated times g.  kExtra: plus ex * extra[k], a gradient that reaches v directly, when extra is not null.
// sh: kThreads / 64 floats.
template <int kThreads, int kSlots, bool kExtra = false>
__device__ __forceinline__ void normalize_backward_store(const float* v, float nv, float eps, const float (&du)[kSlots], int K, float g,
                                                         float* __restrict__ out, int accumulate, float* sh, const float* extra = nullptr,
                                                         float ex = 0.0f) {
    const float iv = inv_norm(nv, eps);
    float vd = 0.0f;
#pragma unroll
    for (int r = 0; r < kSlots; ++r) {
        const int k = threadIdx.x + r * kThreads;
        if (k < K) vd = fmaf(v[k], du[r], vd);
    }
    vd = block_sum<kThreads / 64>(vd, sh);
    const float s = nv < eps ? 0.0f : vd * iv;                   // u . du; a clamped row passes du / eps only, a NaN norm stays NaN
#pragma unroll
    for (int r = 0; r < kSlots; ++r) {
        const int k = threadIdx.x + r * kThreads;
        if (k < K) {
            float d = (du[r] - v[k] * iv * s) * iv;
            if (kExtra && extra) d += ex * extra[k];
            d *= g;
            out[k] = accumulate ? out[k] + d : d;
        }
    }
}

}  // namespace xmh
