// Kernels and launch helpers that both gradient files use (xmh_block_grad.hip: the block stack; xmh_tower_grad.hip: the towers' front and
// back ends): the exact-fp32 product kernel on v_mfma_f32_32x32x2_f32 with its split reduction, the bias column sums, the LayerNorm
// backward.  Every reduction here runs in one fixed order (no float atomics), so two calls on equal inputs agree to the bit; nothing
// synchronises with the host or allocates.  Included by exactly those two files, each of which gets its own copy of the kernels.
#pragma once
#include "xmh_common.h"
#include "xmh_device.h"

namespace {

constexpr int kThreads = 256;
constexpr float kLnEps = 1e-5f;                  // nn.LayerNorm default, as in the forward
constexpr int kTile = 64, kBK = 32, kLd = kTile + 1;
constexpr int kMaxSplits = 16, kTilesWanted = 512;
constexpr int kCols = 32, kGroups = kThreads / kCols;
constexpr int kLnChunks = 64;                    // row chunks of the LayerNorm column sums
constexpr int64_t kMaxRows = 1ll << 21;

typedef float f32x16 __attribute__((ext_vector_type(16)));

using xmh::group_sum;
using xmh::wave_sum;

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

// AK / BK: k is the unit-stride index of that operand (decides which index the lanes of a load walk).  64 x 64 outputs per block,
// one 32 x 32 MFMA tile per wave; LDS holds the slab k-major ([k][i], rows padded by one float) so that lane (l & 31, l >> 5) of
// the MFMA reads As[2 s + (l >> 5)][l & 31]: 32 consecutive floats per half wave.
template <bool AK, bool BK, bool SUM>
__global__ __launch_bounds__(kThreads) void k_mfma_mm(MmArgs g) {
    __shared__ float As[kBK][kLd];
    __shared__ float Bs[kBK][kLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    const int kb = blockIdx.z * g.kchunk;
    const int ke = kb + g.kchunk < g.Kd ? kb + g.kchunk : g.Kd;
    float ra[8], rb[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int ai = AK ? (tid >> 5) + 8 * r : (tid & 63), ak = AK ? (tid & 31) : (tid >> 6) + 4 * r;
            const int bj = BK ? (tid >> 5) + 8 * r : (tid & 63), bk = BK ? (tid & 31) : (tid >> 6) + 4 * r;
            ra[r] = (i0 + ai < g.I && k0 + ak < ke) ? g.A[(int64_t)(i0 + ai) * g.sai + (int64_t)(k0 + ak) * g.sak] : 0.0f;
            rb[r] = (j0 + bj < g.J && k0 + bk < ke) ? g.B[(int64_t)(j0 + bj) * g.sbj + (int64_t)(k0 + bk) * g.sbk] : 0.0f;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int ai = AK ? (tid >> 5) + 8 * r : (tid & 63), ak = AK ? (tid & 31) : (tid >> 6) + 4 * r;
            const int bj = BK ? (tid >> 5) + 8 * r : (tid & 63), bk = BK ? (tid & 31) : (tid >> 6) + 4 * r;
            As[ak][ai] = ra[r];
            Bs[bk][bj] = rb[r];
        }
    };
    const int fr = lane & 31, fh = lane >> 5;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    f32x16 tot;
#pragma unroll
    for (int e = 0; e < 16; ++e) tot[e] = 0.0f;
    double rs = 0.0;
    const bool sums = SUM && blockIdx.x == 0 && tid < kTile;
    fetch(kb);
    for (int k0 = kb; k0 < ke; k0 += kBK) {
        stash();
        __syncthreads();
        if (k0 + kBK < ke) fetch(k0 + kBK);      // the next slab's loads fly over this slab's MFMAs
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll
        for (int s = 0; s < kBK / 2; ++s)        // zero padding past ke: fmaf(0, 0, p) == p
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * s + fh][wi + fr], Bs[2 * s + fh][wj + fr], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) tot[e] += acc[e];       // two-level sum, as k_mm: a 32-term chain per slab, the slabs in order
        if (SUM) {
            if (sums) {
#pragma unroll 8
                for (int k = 0; k < kBK; ++k) rs += (double)As[k][tid];
            }
        }
        __syncthreads();
    }
    const int j = j0 + wj + fr;
    const bool split = gridDim.z > 1;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int i = i0 + wi + (e & 3) + 8 * (e >> 2) + 4 * fh;
        if (i >= g.I || j >= g.J) continue;
        const int64_t at = (int64_t)i * g.J + j;
        float v = tot[e];
        if (split) {
            g.part[(int64_t)blockIdx.z * g.I * g.J + at] = v;
        } else {
            if (g.gelu_pre) v *= quickgelu_grad(g.gelu_pre[at]);
            g.C[at] = g.accumulate ? g.C[at] + v : v;
        }
    }
    if (SUM) {
        if (sums && i0 + tid < g.I) {
            const int i = i0 + tid;
            if (split) g.rowsum_part[(int64_t)blockIdx.z * g.I + i] = rs;
            else g.rowsum[i] = g.accumulate ? g.rowsum[i] + (float)rs : (float)rs;
        }
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

// how many chunks the token reduction of dW [N, K] = dY^T X is cut into, and their length (a multiple of kBK)
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

// what weight_grads and ln_bwd need beside their operands
struct GradScratch {
    double* stats;    // [M][2]   LayerNorm row statistics
    double* lnpart;   // [kLnChunks][2][D]
    float* part;      // partials of a split TN product
    double* bpart;    // [kMaxSplits][N] bias partials
};

// a product dW [N, K] = dY^T X over M rows that weight_grads will be asked for
struct TnShape {
    int64_t M;
    int N, K;
};

// GradScratch's four buffers from a workspace: `rows` LayerNorm rows of width D, bias gradients up to `bias_width` wide, and the
// partials of the largest split product among `tn` (one with no rows or no columns is never launched)
template <size_t n>
void take_scratch(xmh::Arena& ar, int64_t rows, int D, int bias_width, const TnShape (&tn)[n], GradScratch* gs) {
    gs->stats = ar.take<double>((size_t)rows * 2);
    gs->lnpart = ar.take<double>((size_t)kLnChunks * 2 * D);
    size_t most = 0;
    for (const TnShape& s : tn) {
        if (s.M <= 0 || s.K <= 0) continue;
        int splits, chunk;
        tn_split(s.M, s.N, s.K, &splits, &chunk);
        if (splits > 1 && (size_t)splits * s.N * s.K > most) most = (size_t)splits * s.N * s.K;
    }
    gs->part = ar.take<float>(most);
    gs->bpart = ar.take<double>((size_t)kMaxSplits * bias_width);
}

// is any gradient of this block asked for
bool block_asked(const xmh_clip_block_grads& g) {
    return g.ln1_w || g.ln1_b || g.qkv_w || g.qkv_b || g.out_w || g.out_b || g.ln2_w || g.ln2_b || g.fc_w || g.fc_b || g.proj_w || g.proj_b;
}

// the shapes the size functions of both files answer for (the towers add their own bound on the width) ...
bool stack_limits_ok(int64_t B, int L, int width) { return B > 0 && L > 0 && width > 0 && width % 4 == 0 && L <= 128 && B * L <= kMaxRows; }

// ... and what the entry points say beyond them, after their own check of the width
int check_stack_limits(const char* who, int64_t B, int L, int width, int heads) {
    if (width / heads != 64) return xmh::fail(XMH_ENOTSUP, "%s: head dim %d (only 64, CLIP's width/heads)", who, width / heads);
    if (L > 128) return xmh::fail(XMH_ENOTSUP, "%s: L=%d > 128", who, L);
    if (B * L > kMaxRows) return xmh::fail(XMH_ENOTSUP, "%s: %lld x %d tokens (at most 2^21)", who, (long long)B, L);
    return XMH_OK;
}

// dx [M, K] = dy [M, N] w [N, K] (. QuickGELU'(gelu_pre))
void launch_nn(hipStream_t st, const float* dy, const float* w, int64_t M, int N, int K, float* dx, const float* gelu_pre) {
    MmArgs g = {};
    g.A = dy; g.sai = N; g.sak = 1;
    g.B = w; g.sbj = 1; g.sbk = K;
    g.I = (int)M; g.J = K; g.Kd = N; g.kchunk = (int)(xmh::ceil_div(N, kBK) * kBK);
    g.C = dx;
    g.gelu_pre = gelu_pre;
    hipLaunchKernelGGL((k_mfma_mm<true, false, false>), dim3((K + kTile - 1) / kTile, (unsigned)((M + kTile - 1) / kTile), 1), dim3(kThreads), 0, st, g);
}

// dw [N, K] = dy [M, N]^T x [M, K] and, when db is not NULL, db [N] = column sums of dy from the same pass; either may be NULL
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

// LayerNorm backward: dres += LN'(dn; x) when need_dx, dgamma / dbeta when asked for
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

}  // namespace
