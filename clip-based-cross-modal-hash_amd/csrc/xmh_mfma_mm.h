// The exact-fp32 product tile on v_mfma_f32_32x32x2_f32 that k_mfma_mm (xmh_grad_kernels.hip: every backward's NN / TN product, split reduction)
// and k_umoed_bmm (xmh_umoed_head.h: the batched soft-MoE products, forward and backward) wrap.  A block of kThreads threads owns 64 x 64 outputs C[i][j] = sum_k A(i, k)
// B(j, k), one 32 x 32 MFMA tile per wave.  A wrapper is address set-up (make_operand), one call of tile_product, its epilogue (for_each_output).
#pragma once
#include <hip/hip_runtime.h>

namespace xmh::mm {

constexpr int kThreads = 256, kTile = 64, kBK = 32, kLd = kTile + 1;
typedef float f32x16 __attribute__((ext_vector_type(16)));

// (row, k) of a 64 x 32 slab that a thread loads in its r-th of 8 turns.  KU: k is the operand's unit-stride index, so the lanes of a load walk k
template <bool KU>
__device__ __forceinline__ int slab_row(int r) { return KU ? (int)(threadIdx.x >> 5) + 8 * r : (int)(threadIdx.x & 63); }
template <bool KU>
__device__ __forceinline__ int slab_k(int r) { return KU ? (int)(threadIdx.x & 31) : (int)(threadIdx.x >> 6) + 4 * r; }

// An operand as the thread sees it: (row of turn r, k) is p[row[r] + k sk], zero where !ok[r] or k >= ke; make_operand: off(i) = offset of row i
struct Operand {
    const float* p;
    int64_t sk, row[8];
    bool ok[8];
    __device__ float load(int r, int k, int ke) const { return ok[r] && k < ke ? p[row[r] + (int64_t)k * sk] : 0.0f; }
};
template <bool KU, typename RowOffset>
__device__ __forceinline__ Operand make_operand(const float* p, int64_t sk, int r0, int rows, RowOffset&& off) {
    Operand o = {p, sk, {}, {}};
#pragma unroll
    for (int r = 0; r < 8; ++r) o.ok[r] = r0 + slab_row<KU>(r) < rows, o.row[r] = off(r0 + slab_row<KU>(r));
    return o;
}

// The wave's 16 accumulators of sum_{k in [kb, ke)} A(i, k) B(j, k): an exact fmaf chain over the kBK indices of a slab, the slabs added in index
// order.  LDS holds the slab k-major ([k][i], rows padded by one float): lane (l & 31, l >> 5) of the MFMA reads As[2 s + (l >> 5)][l & 31], 32
// consecutive floats per half wave.  slab(As) runs once per slab between its two barriers; As[k - k0][i - i0] = A(i, k), zero past ke and the rows.
template <bool AK, bool BK, typename Slab>
__device__ __forceinline__ f32x16 tile_product(const Operand& a, const Operand& b, int kb, int ke, Slab&& slab) {
    __shared__ float As[kBK][kLd], Bs[kBK][kLd];
    float ra[8], rb[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int r = 0; r < 8; ++r) ra[r] = a.load(r, k0 + slab_k<AK>(r), ke), rb[r] = b.load(r, k0 + slab_k<BK>(r), ke);
    };
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 31, fh = lane >> 5, wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    f32x16 tot = {};
    fetch(kb);
    for (int k0 = kb; k0 < ke; k0 += kBK) {
#pragma unroll
        for (int r = 0; r < 8; ++r) As[slab_k<AK>(r)][slab_row<AK>(r)] = ra[r], Bs[slab_k<BK>(r)][slab_row<BK>(r)] = rb[r];
        __syncthreads();
        if (k0 + kBK < ke) fetch(k0 + kBK);      // the next slab's loads fly over this slab's MFMAs
        f32x16 acc = {};
#pragma unroll
        for (int s = 0; s < kBK / 2; ++s)        // zero padding past ke: fmaf(0, 0, p) == p
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * s + fh][wi + fr], Bs[2 * s + fh][wj + fr], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) tot[e] += acc[e];       // two-level sum, as k_mm: a 32-term chain per slab, the slabs in order
        slab(As);
        __syncthreads();
    }
    return tot;
}

// the output column of this lane in the tile at (i0, j0), and its 16 rows: out(i, j, tot[e]) for every accumulator inside I x J
__device__ __forceinline__ int out_col(int j0) { return j0 + (int)((threadIdx.x >> 6) & 1) * 32 + (int)(threadIdx.x & 31); }
template <typename Out>
__device__ __forceinline__ void for_each_output(const f32x16& tot, int i0, int j0, int I, int J, Out&& out) {
    const int fh = (threadIdx.x >> 5) & 1, wi = (int)(threadIdx.x >> 7) * 32, j = out_col(j0);
    if (j >= J) return;
#pragma unroll
    for (int e = 0; e < 16; ++e)
        if (const int i = i0 + wi + (e & 3) + 8 * (e >> 2) + 4 * fh; i < I) out(i, j, tot[e]);
}

}  // namespace xmh::mm
