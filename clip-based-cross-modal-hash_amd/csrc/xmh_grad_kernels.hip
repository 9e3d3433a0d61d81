// The kernels behind xmh_grad_kernels.h, one copy for the three gradient files, with the launchers the header declares: the exact-fp32 product
// k_mfma_mm (the tile core of xmh_mfma_mm.h, a split reduction over grid z, QuickGELU' and the TN bias row sums), the bias column sums, LayerNorm.
#include "xmh_grad_kernels.h"
#include "xmh_mfma_mm.h"

namespace {

using namespace xmh::grad;
using xmh::group_sum, xmh::wave_sum, xmh::mm::kBK, xmh::mm::kTile;
static_assert(kThreads == xmh::mm::kThreads, "the tile core's block");
constexpr int kTilesWanted = 512, kCols = 32, kGroups = kThreads / kCols;

// d/dx [x sigmoid(1.702 x)] = s (1 + 1.702 x (1 - s))
__device__ __forceinline__ float quickgelu_grad(float x) {
    const float s = 1.0f / (1.0f + expf(-1.702f * x));
    return s * fmaf(1.702f * x, 1.0f - s, 1.0f);
}

struct MmArgs {
    const float* A;           // A(i, k) = A[i * sai + k * sak]
    int64_t sai, sak;
    const float* B;           // B(j, k) = B[j * sbj + k * sbk]
    int64_t sbj, sbk;
    int I, J, Kd;
    int kchunk;               // reduction indices per blockIdx.z (a multiple of kBK); gridDim.z chunks
    float* C;                 // [I, J] row-major
    int accumulate;           // C += instead of C = (one chunk; with several, k_reduce_parts applies it)
    float* part;              // gridDim.z > 1: [gridDim.z][I * J]
    const float* gelu_pre;    // [I, J] or NULL: the result is multiplied by QuickGELU'(gelu_pre)
    float* rowsum;            // SUM: [I], sum_k A(i, k) in double, k in index order (the bias gradient of a TN product)
    double* rowsum_part;      // gridDim.z > 1: [gridDim.z][I]
};

// AK / BK: k is the unit-stride index of that operand.  Grid (J tiles, I tiles, reduction chunks).
template <bool AK, bool BK, bool SUM>
__global__ __launch_bounds__(kThreads) void k_mfma_mm(MmArgs g) {
    namespace mm = xmh::mm;
    const int tid = threadIdx.x, i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    const int kb = blockIdx.z * g.kchunk, ke = kb + g.kchunk < g.Kd ? kb + g.kchunk : g.Kd;
    const mm::Operand a = mm::make_operand<AK>(g.A, g.sak, i0, g.I, [&](int i) { return (int64_t)i * g.sai; });
    const mm::Operand b = mm::make_operand<BK>(g.B, g.sbk, j0, g.J, [&](int j) { return (int64_t)j * g.sbj; });
    double rs = 0.0;
    const bool sums = SUM && blockIdx.x == 0 && tid < kTile;
    const mm::f32x16 tot = mm::tile_product<AK, BK>(a, b, kb, ke, [&](const float(&As)[kBK][mm::kLd]) {
        if (sums) {
#pragma unroll 8
            for (int k = 0; k < kBK; ++k) rs += (double)As[k][tid];
        }
    });
    const bool split = gridDim.z > 1;
    float* const part = g.part + (int64_t)blockIdx.z * g.I * g.J;
    mm::for_each_output(tot, i0, j0, g.I, g.J, [&](int i, int j, float v) {
        const int64_t at = (int64_t)i * g.J + j;
        if (!split && g.gelu_pre) v *= quickgelu_grad(g.gelu_pre[at]);
        if (split) part[at] = v;
        else g.C[at] = g.accumulate ? g.C[at] + v : v;
    });
    if (const int i = i0 + tid; sums && i < g.I) {
        if (split) g.rowsum_part[(int64_t)blockIdx.z * g.I + i] = rs;
        else g.rowsum[i] = g.accumulate ? g.rowsum[i] + (float)rs : (float)rs;
    }
}

// out[e] (+)= sum over the chunks, in index order; bias likewise from its double partials (bout may be NULL)
__global__ __launch_bounds__(kThreads) void k_reduce_parts(const float* __restrict__ part, int splits, int64_t n, float* out, int accumulate,
                                                           const double* __restrict__ bpart, int nb, float* bout) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e < n) {
        float s = part[e];
        for (int z = 1; z < splits; ++z) s += part[(int64_t)z * n + e];
        out[e] = accumulate ? out[e] + s : s;
    }
    if (bout && e < nb) {
        double s = bpart[e];
        for (int z = 1; z < splits; ++z) s += bpart[(int64_t)z * nb + e];
        bout[e] = accumulate ? bout[e] + (float)s : (float)s;
    }
}

// bias gradient alone (its weight is frozen): column sums of dy [M, N] in double, in the very order of the TN kernel's rowsum -- the
// rows of chunk blockIdx.y one after the other, the chunks added by k_reduce_parts -- so freezing a weight does not move a bit of
// its bias gradient
__global__ __launch_bounds__(kThreads) void k_col_sum(const float* __restrict__ dy, int64_t M, int N, int chunk, float* db, double* bpart,
                                                      int accumulate) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= N) return;
    const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = r0 + chunk < M ? r0 + chunk : M;
    double a = 0.0;
    for (int64_t r = r0; r < r1; ++r) a += (double)dy[r * N + e];
    if (gridDim.y > 1) bpart[(int64_t)blockIdx.y * N + e] = a;
    else db[e] = accumulate ? db[e] + (float)a : (float)a;
}

// LayerNorm backward over one row (one wave): the row statistics are recomputed in double from the saved input x (the record keeps
// no statistics), h = dn gamma, dres += rstd (h - mean(h) - xhat mean(h xhat)) -- the residual gradient is added in the same pass.
// stats (or NULL): [M][2] doubles, mean and rstd, for the column kernel.  dn == NULL: statistics only.
__global__ __launch_bounds__(kThreads) void k_ln_bwd_rows(const float* __restrict__ x, const float* __restrict__ dn,
                                                          const float* __restrict__ gamma, float* dres, double* stats, int64_t M, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + row * D;
    double a = 0.0;
    for (int e = lane; e < D; e += 64) a += (double)xr[e];
    const double mean = wave_sum(a) / (double)D;
    a = 0.0;
    for (int e = lane; e < D; e += 64) {
        const double d = (double)xr[e] - mean;
        a += d * d;
    }
    const double rstd = 1.0 / sqrt(wave_sum(a) / (double)D + (double)kLnEps);
    if (stats && lane == 0) {
        stats[2 * row] = mean;
        stats[2 * row + 1] = rstd;
    }
    if (!dn) return;
    const float* dr = dn + row * D;
    double sh = 0.0, sc = 0.0;
    for (int e = lane; e < D; e += 64) {
        const double h = (double)dr[e] * (double)gamma[e];
        sh += h;
        sc += h * (((double)xr[e] - mean) * rstd);
    }
    const double mh = wave_sum(sh) / (double)D, mc = wave_sum(sc) / (double)D;
    float* out = dres + row * D;
    for (int e = lane; e < D; e += 64) {
        const double h = (double)dr[e] * (double)gamma[e], xh = ((double)xr[e] - mean) * rstd;
        out[e] += (float)(rstd * (h - mh - xh * mc));
    }
}

// dgamma[e] = sum_rows dn xhat, dbeta[e] = sum_rows dn: double partials of row chunk blockIdx.y (rows of a chunk in 8 interleaved
// groups, the groups added in index order) -> part [chunks][2][D].  stats == NULL: dbeta alone.
__global__ __launch_bounds__(kThreads) void k_ln_bwd_cols(const float* __restrict__ dn, const float* __restrict__ x,
                                                          const double* __restrict__ stats, int64_t M, int D, int64_t rows_per_chunk,
                                                          double* part) {
    __shared__ double sh[kGroups][kCols];
    const int col = threadIdx.x % kCols, grp = threadIdx.x / kCols, e = blockIdx.x * kCols + col;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk, r1 = r0 + rows_per_chunk < M ? r0 + rows_per_chunk : M;
    double a = 0.0, c = 0.0;
    if (e < D)
        for (int64_t r = r0 + grp; r < r1; r += kGroups) {
            const double d = (double)dn[r * D + e];
            c += d;
            if (stats) a += d * (((double)x[r * D + e] - stats[2 * r]) * stats[2 * r + 1]);
        }
    const double sg = group_sum(a, sh, col, grp), sb = group_sum(c, sh, col, grp);
    if (e < D && grp == 0) {
        part[((int64_t)blockIdx.y * 2) * D + e] = sg;
        part[((int64_t)blockIdx.y * 2 + 1) * D + e] = sb;
    }
}

__global__ __launch_bounds__(kThreads) void k_ln_cols_reduce(const double* __restrict__ part, int chunks, int D, float* dgamma, float* dbeta,
                                                             int accumulate) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= D) return;
    double sg = 0.0, sb = 0.0;
    for (int c = 0; c < chunks; ++c) {
        sg += part[((int64_t)c * 2) * D + e];
        sb += part[((int64_t)c * 2 + 1) * D + e];
    }
    if (dgamma) dgamma[e] = accumulate ? dgamma[e] + (float)sg : (float)sg;
    if (dbeta) dbeta[e] = accumulate ? dbeta[e] + (float)sb : (float)sb;
}

}  // namespace

namespace xmh::grad {

void tn_split(int64_t M, int N, int K, int* splits, int* chunk) {
    const int64_t tiles = xmh::ceil_div(N, kTile) * xmh::ceil_div(K, kTile);
    int64_t s = xmh::ceil_div(kTilesWanted, tiles);
    const int64_t most = xmh::ceil_div(M, 2 * kBK);
    if (s > most) s = most;
    if (s > kMaxSplits) s = kMaxSplits;
    if (s < 1) s = 1;
    const int64_t c = xmh::ceil_div(xmh::ceil_div(M, s), kBK) * kBK;
    *chunk = (int)c;
    *splits = (int)xmh::ceil_div(M, c);
}

void launch_nn(hipStream_t st, const float* dy, const float* w, int64_t M, int N, int K, float* dx, const float* gelu_pre) {
    MmArgs g = {};
    g.A = dy; g.sai = N; g.sak = 1;
    g.B = w; g.sbj = 1; g.sbk = K;
    g.I = (int)M; g.J = K; g.Kd = N; g.kchunk = (int)(xmh::ceil_div(N, kBK) * kBK);
    g.C = dx;
    g.gelu_pre = gelu_pre;
    hipLaunchKernelGGL((k_mfma_mm<true, false, false>), dim3((K + kTile - 1) / kTile, (unsigned)((M + kTile - 1) / kTile), 1), dim3(kThreads), 0, st, g);
}

void weight_grads(hipStream_t st, const GradScratch& wk, const float* dy, const float* x, int64_t M, int N, int K, float* dw, float* db, int accumulate) {
    int splits, chunk;
    tn_split(M, N, K, &splits, &chunk);
    if (!dw) {
        if (!db) return;
        hipLaunchKernelGGL(k_col_sum, dim3((N + kThreads - 1) / kThreads, splits), dim3(kThreads), 0, st, dy, M, N, chunk, db, wk.bpart, accumulate);
        if (splits > 1)
            hipLaunchKernelGGL(k_reduce_parts, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, st, nullptr, splits, (int64_t)0, nullptr,
                               accumulate, wk.bpart, N, db);
        return;
    }
    MmArgs g = {};
    g.A = dy; g.sai = 1; g.sak = N;
    g.B = x; g.sbj = 1; g.sbk = K;
    g.I = N; g.J = K; g.Kd = (int)M; g.kchunk = chunk;
    g.C = dw;
    g.accumulate = accumulate;
    g.part = wk.part;
    g.rowsum = db;
    g.rowsum_part = wk.bpart;
    const dim3 grid((K + kTile - 1) / kTile, (N + kTile - 1) / kTile, splits);
    if (db) hipLaunchKernelGGL((k_mfma_mm<false, false, true>), grid, dim3(kThreads), 0, st, g);
    else hipLaunchKernelGGL((k_mfma_mm<false, false, false>), grid, dim3(kThreads), 0, st, g);
    if (splits > 1) {
        const int64_t n = (int64_t)N * K;
        hipLaunchKernelGGL(k_reduce_parts, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, wk.part, splits, n, dw, accumulate,
                           wk.bpart, N, db);
    }
}

void ln_bwd(hipStream_t st, const GradScratch& wk, const float* x, const float* dn, const float* gamma, float* dres, bool need_dx, float* dgamma,
            float* dbeta, int64_t M, int D, int accumulate) {
    if (need_dx || dgamma)
        hipLaunchKernelGGL(k_ln_bwd_rows, dim3((unsigned)((M + 3) / 4)), dim3(kThreads), 0, st, x, need_dx ? dn : nullptr, gamma, dres,
                           dgamma ? wk.stats : nullptr, M, D);
    if (dgamma || dbeta) {
        int64_t chunks = xmh::ceil_div(M, 64);
        if (chunks > kLnChunks) chunks = kLnChunks;
        const int64_t rows = xmh::ceil_div(M, chunks);
        chunks = xmh::ceil_div(M, rows);
        hipLaunchKernelGGL(k_ln_bwd_cols, dim3((D + kCols - 1) / kCols, (unsigned)chunks), dim3(kThreads), 0, st, dn, x,
                           dgamma ? wk.stats : nullptr, M, D, rows, wk.lnpart);
        hipLaunchKernelGGL(k_ln_cols_reduce, dim3((D + kThreads - 1) / kThreads), dim3(kThreads), 0, st, wk.lnpart, (int)chunks, D, dgamma, dbeta,
                           accumulate);
    }
}

}  // namespace xmh::grad
