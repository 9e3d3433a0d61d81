// Device helpers shared by the training kernels (xmh_hyp, xmh_dnph, xmh_dimch, xmh_umoed, xmh_twdh, xmh_mith_loss, xmh_head_grad,
// xmh_block_grad, xmh_optim), xmh_encode, xmh_forward and xmh_dense, and the workspace carver of the host entry points: wave and block reductions (sum,
// maximum, log-sum-exp), the column kernels' group_sum.  xmh_rows.h (row normalisation) and xmh_triplet.h (the triplet term) build
// on it.  The scan, top-k and GEMM kernels keep their own hand-scheduled idioms; xmh_loss.hip keeps its block_sum, whose result
// lives on thread 0 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace xmh {

__host__ __device__ inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Carve-out of a caller-owned buffer in 256-byte aligned pieces.  The same walk sizes the buffer (base == nullptr: every take
// returns null) and hands out the pieces, so the two cannot disagree; `used` is the byte total so far.
struct Arena {
    char* base;
    size_t used = 0;
    __host__ __device__ explicit Arena(void* p) : base(static_cast<char*>(p)) {}
    template <typename T>
    __host__ __device__ T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used = align256(used + count * sizeof(T));
        return p;
    }
};

// Wave reductions by xor butterfly, 32 down to 1: every lane ends with the same bits (each step combines the same two values, in
// either order), and the order is fixed, which is what the bit-reproducibility promises of the callers rest on.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float, double or int");
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// Block sum in a fixed order (wave butterflies, then the kWaves waves in index order); valid on every thread.  sh: kWaves elements.
template <int kWaves, typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = sh[0];
    for (int w = 1; w < kWaves; ++w) s += sh[w];
    __syncthreads();
    return s;
}

// Block maximum, valid on every thread.  fmaxf drops a NaN; every caller sums exp(v - max) afterwards, where it comes back.
template <int kWaves>
__device__ __forceinline__ float block_max(float v, float* sh) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = sh[0];
    for (int w = 1; w < kWaves; ++w) m = fmaxf(m, sh[w]);
    __syncthreads();
    return m;
}

// sum_i exp(v[i] - max) over n values the block can read and the maximum in *mx; valid on every thread.  fsh, dsh: kWaves elements.
template <int kWaves>
__device__ __forceinline__ double block_exp_sum(const float* v, int n, float* fsh, double* dsh, float* mx) {
    float m = -INFINITY;
    for (int i = threadIdx.x; i < n; i += kWaves * 64) m = fmaxf(m, v[i]);
    m = block_max<kWaves>(m, fsh);
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kWaves * 64) s += (double)expf(v[i] - m);
    *mx = m;
    return block_sum<kWaves>(s, dsh);
}

// log sum_i exp(v[i]), the maximum subtracted; valid on every thread
template <int kWaves>
__device__ __forceinline__ float block_lse(const float* v, int n, float* fsh, double* dsh) {
    float m;
    const double s = block_exp_sum<kWaves>(v, n, fsh, dsh, &m);
    return m + logf((float)s);
}

// Column kernels (kCols adjacent columns x kGroups interleaved row groups per block): fixed-order sum of the row groups' partials of
// one column; valid on every thread of the column
template <int kGroups, int kCols>
__device__ __forceinline__ double group_sum(double v, double (&sh)[kGroups][kCols], int col, int grp) {
    sh[grp][col] = v;
    __syncthreads();
    double s = sh[0][col];
    for (int g = 1; g < kGroups; ++g) s += sh[g][col];
    __syncthreads();
    return s;
}

}  // namespace xmh
