// Backward of a stack of CLIP ResidualAttentionBlocks (models/CLIP/model.py:167-211) from the per-layer record that
// xmh_clip_blocks_forward_saved keeps.  Exact fp32 products throughout: a train step changes the weights every step, so
// the fp16 operand planes of the inference path would be re-made per step.
//
//   block, top down (dy = gradient of the block's output, [M, D], updated in place; M = B L, D = width):
//     c_proj   k_mfma_mm<TN> dW = dy^T fc_act, db = colsum dy          k_mfma_mm<NN> dfc_pre = (dy W) . QuickGELU'(fc_pre)   (epilogue)
//     c_fc     k_mfma_mm<TN> dW = dfc_pre^T ln2, db                    k_mfma_mm<NN> dln2 = dfc_pre W
//     ln_2     k_ln_bwd_rows dy += LN'(dln2; x_mid)  (= dx_mid)        k_ln_bwd_cols + k_ln_cols_reduce  dgamma, dbeta
//     out_proj k_mfma_mm<TN> dW = dy^T attn, db                        k_mfma_mm<NN> dattn = dy W
//     attn     k_attn_bwd   dqkv from the saved qkv (S and P recomputed per query tile)
//     in_proj  k_mfma_mm<TN> dW = dqkv^T ln1, db                       k_mfma_mm<NN> dln1 = dqkv W
//     ln_1     k_ln_bwd_rows dy += LN'(dln1; x_in)   (= dx)            k_ln_bwd_cols + k_ln_cols_reduce
//   A TN product whose 64 x 64 tiles would not fill the chip splits its reduction (the tokens) over blockIdx.z; the partials go to
//   the workspace and k_reduce_parts adds them in index order.
//
// One product kernel, C[i][j] = sum_k A(i, k) B(j, k) over strided views (as k_mm of xmh_head_grad.hip), on v_mfma_f32_32x32x2_f32:
// an exact fmaf chain per 32 consecutive k, the 32-blocks added in index order.  Every reduction here runs in one fixed order (no
// float atomics), so two calls on equal inputs agree to the bit; no host synchronisation, no allocation.
#include "xmh_clip_record.h"
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

// Attention backward of one (batch, head) per block.  K and V of the head stay in LDS (rows padded to 65 floats, key rows up to
// LP = 4 NJ zero-filled); the queries go by in tiles of 32 rows: S = (q / sqrt(dh)) K^T + mask and P = softmax(S) are recomputed as
// the forward computes them, dP = dO V^T, dS = P (dP - rowsum(dP P)), dQ = dS K / sqrt(dh) goes straight out, and dV += P^T dO,
// dK += dS^T (q / sqrt(dh)) accumulate in registers -- thread (c, jg) owns column c of key rows jg, jg + 4, ... -- over the tiles in
// index order: no atomics, one fixed order.  A whole-head-resident plan (Q, K, V, dO and a 128 x 128 P) would need 192 KB of LDS.
constexpr int kDh = 64, kTq = 32, kKp = kDh + 1;

template <int NJ>
__global__ __launch_bounds__(kThreads) void k_attn_bwd(const float* __restrict__ qkv, const float* __restrict__ dO, float* __restrict__ dqkv,
                                                       int L, int H, int causal, const uint8_t* __restrict__ kpm) {
    constexpr int LP = 4 * NJ, PP = LP + 1, NS = NJ / 2;
    extern __shared__ __attribute__((aligned(16))) float sm_attn[];
    float* sK = sm_attn;                         // [LP][kKp]
    float* sV = sK + LP * kKp;                   // [LP][kKp]
    float* sQ = sV + LP * kKp;                   // [kTq][kKp], scaled
    float* sG = sQ + kTq * kKp;                  // [kTq][kKp], dO
    float* sP = sG + kTq * kKp;                  // [kTq][PP]
    float* sS = sP + kTq * PP;                   // [kTq][PP], dS
    const int tid = threadIdx.x;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int D = H * kDh;
    const float scale = rsqrtf((float)kDh);
    const float* base = qkv + (int64_t)b * L * 3 * D + h * kDh;
    const float* gbase = dO + (int64_t)b * L * D + h * kDh;
    float* obase = dqkv + (int64_t)b * L * 3 * D + h * kDh;
    for (int e = tid; e < LP * (kDh / 4); e += kThreads) {
        const int j = e / (kDh / 4), c = (e % (kDh / 4)) * 4;
        float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
        if (j < L) {
            kv = *reinterpret_cast<const float4*>(base + (int64_t)j * 3 * D + D + c);
            vv = *reinterpret_cast<const float4*>(base + (int64_t)j * 3 * D + 2 * D + c);
        }
        float* pk = sK + j * kKp + c;
        float* pv = sV + j * kKp + c;
        pk[0] = kv.x; pk[1] = kv.y; pk[2] = kv.z; pk[3] = kv.w;
        pv[0] = vv.x; pv[1] = vv.y; pv[2] = vv.z; pv[3] = vv.w;
    }
    float accK[NJ], accV[NJ];
#pragma unroll
    for (int t = 0; t < NJ; ++t) accK[t] = accV[t] = 0.0f;
    const int r = tid >> 3, sub = tid & 7;       // score phase and dQ: query row of the tile, 8 threads per row
    const int oc = tid & 63, jg = tid >> 6;      // dK / dV phase
    for (int i0 = 0; i0 < L; i0 += kTq) {
        __syncthreads();                         // the previous tile's reads are done (first pass: K and V are in place)
        for (int e = tid; e < kTq * (kDh / 4); e += kThreads) {
            const int rr = e / (kDh / 4), c = (e % (kDh / 4)) * 4;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f), gg = q;
            if (i0 + rr < L) {
                q = *reinterpret_cast<const float4*>(base + (int64_t)(i0 + rr) * 3 * D + c);
                gg = *reinterpret_cast<const float4*>(gbase + (int64_t)(i0 + rr) * D + c);
            }
            float* pq = sQ + rr * kKp + c;
            float* pg = sG + rr * kKp + c;
            pq[0] = q.x * scale; pq[1] = q.y * scale; pq[2] = q.z * scale; pq[3] = q.w * scale;      // PyTorch scales q before QK^T
            pg[0] = gg.x; pg[1] = gg.y; pg[2] = gg.z; pg[3] = gg.w;
        }
        __syncthreads();
        const int i = i0 + r;
        float s[NS], dp[NS];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const int j = sub + 8 * t;
            float a0 = 0.0f, a1 = 0.0f;
            const float* q = sQ + r * kKp;
            const float* gq = sG + r * kKp;
            const float* kj = sK + j * kKp;
            const float* vj = sV + j * kKp;
#pragma unroll 8
            for (int c = 0; c < kDh; ++c) {
                a0 = fmaf(q[c], kj[c], a0);
                a1 = fmaf(gq[c], vj[c], a1);
            }
            const bool dead = j >= L || (causal && j > i) || (kpm && kpm[(int64_t)b * L + j]);
            s[t] = dead ? -INFINITY : a0;
            dp[t] = a1;
            mx = fmaxf(mx, s[t]);
        }
#pragma unroll
        for (int off = 4; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        float sum = 0.0f;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            s[t] = expf(s[t] - mx);
            sum += s[t];
        }
#pragma unroll
        for (int off = 4; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        const float inv = i < L ? 1.0f / sum : 0.0f;         // rows past L contribute nothing to dK / dV
        float dot = 0.0f;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            s[t] *= inv;
            dot = fmaf(s[t], dp[t], dot);
        }
#pragma unroll
        for (int off = 4; off > 0; off >>= 1) dot += __shfl_xor(dot, off);
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const int j = sub + 8 * t;
            sP[r * PP + j] = s[t];
            sS[r * PP + j] = s[t] * (dp[t] - dot);
        }
        __syncthreads();
        {                                        // dQ[i][c] = scale sum_j dS[i][j] K[j][c], c = sub + 8 u
            float dq[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) dq[u] = 0.0f;
            for (int j = 0; j < L; ++j) {
                const float ds = sS[r * PP + j];
                const float* kj = sK + j * kKp + sub;
#pragma unroll
                for (int u = 0; u < 8; ++u) dq[u] = fmaf(ds, kj[8 * u], dq[u]);
            }
            if (i < L) {
#pragma unroll
                for (int u = 0; u < 8; ++u) obase[(int64_t)i * 3 * D + sub + 8 * u] = dq[u] * scale;
            }
        }
        for (int ii = 0; ii < kTq; ++ii) {       // rows past L hold P = dS = 0
            const float go = sG[ii * kKp + oc], q = sQ[ii * kKp + oc];
            const float* pr = sP + ii * PP + jg;
            const float* sr = sS + ii * PP + jg;
#pragma unroll
            for (int t = 0; t < NJ; ++t) {
                accV[t] = fmaf(pr[4 * t], go, accV[t]);
                accK[t] = fmaf(sr[4 * t], q, accK[t]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NJ; ++t) {
        const int j = jg + 4 * t;
        if (j < L) {
            obase[(int64_t)j * 3 * D + D + oc] = accK[t];
            obase[(int64_t)j * 3 * D + 2 * D + oc] = accV[t];
        }
    }
}

template <int NJ>
int launch_attn_bwd(hipStream_t st, const float* qkv, const float* dO, float* dqkv, int64_t B, int L, int H, int causal, const uint8_t* kpm) {
    constexpr int LP = 4 * NJ;
    const size_t lds = ((size_t)2 * LP * kKp + (size_t)2 * kTq * kKp + (size_t)2 * kTq * (LP + 1)) * sizeof(float);
    auto kern = k_attn_bwd<NJ>;
    if (lds > 64 * 1024)
        if (const int rl = xmh::raise_dynamic_lds(reinterpret_cast<const void*>(kern), lds, "xmh_clip_blocks_backward")) return rl;
    hipLaunchKernelGGL(kern, dim3((unsigned)(B * H)), dim3(kThreads), lds, st, qkv, dO, dqkv, L, H, causal, kpm);
    return XMH_OK;
}

int attn_bwd(hipStream_t st, const float* qkv, const float* dO, float* dqkv, int64_t B, int L, int H, int causal, const uint8_t* kpm) {
    if (L <= 32) return launch_attn_bwd<8>(st, qkv, dO, dqkv, B, L, H, causal, kpm);
    if (L <= 64) return launch_attn_bwd<16>(st, qkv, dO, dqkv, B, L, H, causal, kpm);
    return launch_attn_bwd<32>(st, qkv, dO, dqkv, B, L, H, causal, kpm);
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

struct Work {
    float* t1;        // [M, D]   dln2, dattn, dln1
    float* t4;        // [M, 4D]  dfc_pre; dqkv [M, 3D] once dfc_pre is dead
    double* stats;    // [M][2]   LayerNorm row statistics
    double* lnpart;   // [kLnChunks][2][D]
    float* part;      // partials of a split TN product
    double* bpart;    // [kMaxSplits][4D] bias partials
};

size_t work_layout(int64_t M, int D, void* base, Work* w) {
    xmh::Arena ar(base);
    Work v;
    v.t1 = ar.take<float>((size_t)M * D);
    v.t4 = ar.take<float>((size_t)M * D * 4);
    v.stats = ar.take<double>((size_t)M * 2);
    v.lnpart = ar.take<double>((size_t)kLnChunks * 2 * D);
    size_t most = 0;
    const int shapes[4][2] = {{D, 4 * D}, {4 * D, D}, {D, D}, {3 * D, D}};
    for (const auto& s : shapes) {
        int splits, chunk;
        tn_split(M, s[0], s[1], &splits, &chunk);
        if (splits > 1 && (size_t)splits * s[0] * s[1] > most) most = (size_t)splits * s[0] * s[1];
    }
    v.part = ar.take<float>(most);
    v.bpart = ar.take<double>((size_t)kMaxSplits * 4 * D);
    if (w) *w = v;
    return ar.used;
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
void weight_grads(hipStream_t st, const Work& wk, const float* dy, const float* x, int64_t M, int N, int K, float* dw, float* db, int accumulate) {
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
void ln_bwd(hipStream_t st, const Work& wk, const float* x, const float* dn, const float* gamma, float* dres, bool need_dx, float* dgamma,
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

bool any_grad(const xmh_clip_block_grads& g) {
    return g.ln1_w || g.ln1_b || g.qkv_w || g.qkv_b || g.out_w || g.out_b || g.ln2_w || g.ln2_b || g.fc_w || g.fc_b || g.proj_w || g.proj_b;
}

bool limits_ok(int64_t B, int L, int width) { return B > 0 && L > 0 && width > 0 && width % 4 == 0 && L <= 128 && B * L <= kMaxRows; }

}  // namespace

extern "C" size_t xmh_clip_blocks_backward_ws_bytes(int64_t B, int L, int width) {
    if (!limits_ok(B, L, width)) return 0;
    return work_layout(B * L, width, nullptr, nullptr);
}

extern "C" int xmh_clip_blocks_backward(const xmh_clip_block* blocks, int layers, int width, int heads, int64_t B, int L, int causal,
                                        const uint8_t* key_padding_mask, const float* saved, size_t saved_bytes, float* dy, int need_dx,
                                        const xmh_clip_block_grads* grads, int accumulate, void* workspace, size_t workspace_bytes,
                                        xmh_stream_t stream) {
    XMH_RANGE("xmh_clip_blocks_backward");
    const char* who = "xmh_clip_blocks_backward";
    if (B == 0 || layers == 0) return XMH_OK;
    if (B < 0 || L <= 0 || layers < 0 || width <= 0 || heads <= 0 || width % heads) return xmh::fail(-22, "%s: bad arguments", who);
    if (!blocks || !grads) return xmh::fail(-22, "%s: null blocks / grads", who);
    if (!dy) return xmh::fail(-22, "%s: null dy", who);
    if (!saved) return xmh::fail(-22, "%s: null saved buffer", who);
    if (!workspace) return xmh::fail(-22, "%s: null workspace", who);
    if (width % 4) return xmh::fail(XMH_ENOTSUP, "%s: width %d is not a multiple of 4", who, width);
    if (width / heads != kDh) return xmh::fail(XMH_ENOTSUP, "%s: head dim %d (only 64, CLIP's width/heads)", who, width / heads);
    if (L > 128) return xmh::fail(XMH_ENOTSUP, "%s: L=%d > 128", who, L);
    if (B * L > kMaxRows) return xmh::fail(XMH_ENOTSUP, "%s: %lld x %d tokens (at most 2^21)", who, (long long)B, L);
    const int64_t M = B * L;
    const int D = width;
    const size_t need = xmh::saved_record_bytes(layers, M, D);
    if (saved_bytes < need) return xmh::fail(-12, "%s: saved buffer of %zu bytes, %zu needed", who, saved_bytes, need);
    Work wk;
    const size_t ws_need = work_layout(M, D, workspace, &wk);
    if (workspace_bytes < ws_need) return xmh::fail(-12, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, ws_need);

    // the walk stops at the lowest layer anything is asked of: below it nothing is read, neither its record nor its weights
    int lowest = 0;
    if (!need_dx) {
        while (lowest < layers && !any_grad(grads[lowest])) ++lowest;
        if (lowest == layers) return XMH_OK;
    }
    for (int i = lowest; i < layers; ++i) {
        const xmh_clip_block& b = blocks[i];
        if (!xmh::block_fits(b, D)) return xmh::fail(-22, "%s: block %d has layer shapes that do not fit width %d", who, i, D);
        if (!b.qkv.w_f32 || !b.out.w_f32 || !b.fc.w_f32 || !b.proj.w_f32 || !b.ln1_w || !b.ln2_w)
            return xmh::fail(-22, "%s: block %d lacks fp32 weights", who, i);
    }
    hipStream_t st = xmh::as_stream(stream);
    for (int i = layers - 1; i >= lowest; --i) {
        const xmh_clip_block& b = blocks[i];
        const xmh_clip_block_grads& g = grads[i];
        const xmh::SavedRecord<const float> r = xmh::saved_record(saved, i, M, D);
        // what has to exist for what is asked for: each stage is needed by everything upstream of it
        const bool need_in = i > lowest || need_dx;
        const bool need_dln1 = g.ln1_w || g.ln1_b || need_in;
        const bool need_dqkv = g.qkv_w || g.qkv_b || need_dln1;
        const bool need_dxmid = g.out_w || g.out_b || need_dqkv;
        const bool need_dln2 = g.ln2_w || g.ln2_b || need_dxmid;
        const bool need_dfc = g.fc_w || g.fc_b || need_dln2;
        weight_grads(st, wk, dy, r.fc_act, M, D, 4 * D, g.proj_w, g.proj_b, accumulate);
        if (!need_dfc) continue;
        launch_nn(st, dy, b.proj.w_f32, M, D, 4 * D, wk.t4, r.fc_pre);                         // dfc_pre
        weight_grads(st, wk, wk.t4, r.ln2, M, 4 * D, D, g.fc_w, g.fc_b, accumulate);
        if (!need_dln2) continue;
        launch_nn(st, wk.t4, b.fc.w_f32, M, 4 * D, D, wk.t1, nullptr);                         // dln2
        ln_bwd(st, wk, r.x_mid, wk.t1, b.ln2_w, dy, need_dxmid, g.ln2_w, g.ln2_b, M, D, accumulate);    // dy = dx_mid
        if (!need_dxmid) continue;
        weight_grads(st, wk, dy, r.attn, M, D, D, g.out_w, g.out_b, accumulate);
        if (!need_dqkv) continue;
        launch_nn(st, dy, b.out.w_f32, M, D, D, wk.t1, nullptr);                               // dattn
        if (int rc = attn_bwd(st, r.qkv, wk.t1, wk.t4, B, L, heads, causal, key_padding_mask)) return rc;      // dqkv [M, 3D]
        weight_grads(st, wk, wk.t4, r.ln1, M, 3 * D, D, g.qkv_w, g.qkv_b, accumulate);
        if (!need_dln1) continue;
        launch_nn(st, wk.t4, b.qkv.w_f32, M, 3 * D, D, wk.t1, nullptr);                        // dln1
        ln_bwd(st, wk, r.x_in, wk.t1, b.ln1_w, dy, need_in, g.ln1_w, g.ln1_b, M, D, accumulate);  // dy = dx
    }
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}
