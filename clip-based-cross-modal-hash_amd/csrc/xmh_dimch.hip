// Objective of DIMCH (reference models/DIMCH/DIMCH.py:152-234 chamfer_similarity_loss, distance/distance.py, loss/triplet_loss.py:16-88)
// and its gradient with respect to the two token-embedding tensors and the two codes.
//
//   N = B M.  x, y = F.normalize (eps 1e-12) of the rows of e_img, e_txt viewed as [N, K]; G = u v^T over a pair of sets (an M x M tile).
//   s(u, v)[i][j]   smooth_chamfer / chamfer / max / avg of the tile (set i of u, set j of v), see include/xmh.h
//   D_i2t = clamp(1 - s(x, y), 0), D_t2i = clamp(1 - s(y, x), 0); Dh = clamp(1 - cos(h_img, h_txt), 0) and its transpose
//   T(D, m)         the label-weighted triplet mean of triplet_loss.py (sum of positive triplets over their count + 1e-16)
//   MMD             mean exp(-gamma |x_a - x_b|) - 2 mean exp(-gamma |x_a - y_b|) + mean exp(-gamma |y_a - y_b|) over all N x N pairs
//   U(u)            sum_{a < b} exp(-20 |u_a - u_b|^2) / (M (M - 1) / 2) over all N rows (0 for M = 1)
//   loss = (T_i2t + T_t2i) / 2 triplet_alpha + mmd_alpha MMD + unif_alpha (U(x) + U(y)) + (Th_i2t + Th_t2i) / 2 hash_triplet_alpha
//          + (Q_img + Q_txt) / 2 quan_alpha
//
//   xmh_dimch_loss       4 launches
//     k_dimch_prep       a wave per row: norms, normalised token rows xn / yn, nn = the k-ordered fmaf chain of xn_k^2; norms of the codes
//     k_dimch_tiles      block (family, i, j), family = x.y, x.x, y.y: one M x M Gram tile (k-ordered fmaf chain per entry).  An x.y tile
//                        gives s(x, y)[i][j], s(y, x)[j][i] and its share of the MMD cross term; an x.x / y.y tile its shares of MMD and U.
//                        B further blocks: row a of cos(h_img, h_txt) and the quantisation sums of code row a.
//     k_dimch_triplet    block a: anchor row a of the four triplet terms (weights, sum, count) and row a of the tile partials
//     k_dimch_finalize   one block: ordered sums over the B rows -> out12
//   xmh_dimch_loss_grad  6 launches
//     k_dimch_prep, k_dimch_tiles, k_dimch_triplet as above (the call stands alone: nothing is kept from the forward)
//     k_dimch_triplet_grad  block a: d loss / d D of anchor row a of the four terms, gathered per column (a thread owns a column p:
//                        its own triplets (a, p, *) and those in which it is the negative (a, *, p)), through the clamps -> d / d s, d / d cos
//     k_dimch_owner      block (side, i, part): owns the M rows of set i of x (of y) and loops over its part of the B sets of the other
//                        side and the B sets of its own side: recomputes the tile, forms d loss / d G there, adds (d / d G) v into its
//                        rows' registers; its share goes to the workspace.  The loop is cut into P = 1 .. 4 parts (by B alone) so that
//                        a small batch still fills the device.  2B further blocks: the gradient of one code row each.
//     k_dimch_rows       a wave per token row: the parts' shares added in order, then the backward of the normalisation
//
// No host synchronisation, no allocation, no float atomics: every sum has one fixed order, so two calls on the same inputs agree to
// the bit.  The tiles use plain fp32 FMA in k order at every shape; no MFMA tile routine is built.  An fp32 MFMA accumulates along k as
// well, so one is EXPECTED to leave G's bits alone, but that is not measured, and it would have to hold for the scalar nn chain of
// k_dimch_prep too, which the q = 0 identity below depends on.  Squared distances come from the Gram entry, q = (nn_a + nn_b) - 2 G_ab: nn is formed by the same chain as G, so two rows with
// the same bits give q = 0 exactly (torch.cdist's zero, whose gradient is 0), the diagonal of x.x included.  Where q < 0.25 the
// cancellation would leave too few digits (U lives on exactly those pairs): there q is recomputed as sum_k (u_k - v_k)^2.
// Workspace O(N K + B^2): two normalised copies, and [B, B] tables.  Non-finite values pass through: clamps are written as
// (v < 0 ? 0 : v), which keeps a NaN where fmaxf would drop it; a row without a label has Z = 0 and weights 0 / 0 = NaN, as in the reference.
#include <math.h>

#include "xmh_common.h"
#include "xmh_rows.h"
#include "xmh_triplet.h"

namespace {

namespace trip = xmh::trip;                                     // the triplet term, shared with xmh_umoed.hip
constexpr int kThreads = trip::kThreads, kWaves = trip::kWaves;
constexpr int kMaxB = trip::kMaxB, kMaxM = 64, kMaxK = 256, kMaxC = 127;
constexpr int kT = 64;                 // tile edge: the largest set
constexpr int kKC = 32;                // k columns staged at a time
constexpr int kLd = kT + 1;            // row stride of the staged operands and of the G tile
constexpr int kLdW = kT + 4;           // row stride of the transposed d / d G tile (float4 reads)
constexpr float kEps = 1e-12f;         // F.normalize's eps
constexpr float kCosEps = 1e-8f;       // F.cosine_similarity's eps
constexpr float kNear = 0.25f;         // below this squared distance q is recomputed from differences
constexpr float kUnifT = 20.0f;        // batchwise_uniformity_loss's t

struct Ws {
    float* xn;       // [2][N][K] normalised token rows (x, then y)
    float* nrm;      // [2N] norms of the raw token rows
    float* nn;       // [2N] chain sum of squares of the normalised rows
    float* hn;       // [2B] norms of the code rows
    float* S[2];     // s(x, y)[i][j] and s(y, x)[j][i], both [B][B] by their own first index
    float* Ch;       // [B][B] cos(h_img[a], h_txt[p])
    float* gD[4];    // d loss / d s(x, y), d / d s(y, x), d / d Ch of Th_i2t by [a][p], d / d Ch^T of Th_t2i by [a][p]
    double* part;    // [3][B][B] sum of exp(-gamma d) of a tile, per family
    double* upart;   // [2][B][B] sum of exp(-20 d^2) over a != b of a tile (x.x, y.y)
    double* rowpart; // [B][8] row sums of part and upart
    double* qpart;   // [2B] quantisation sum of a code row
    double* tsum;    // [4][B] per anchor: sum of positive triplets
    double* tcnt;    // [4][B] per anchor: their count
    float* pd;       // [P][2N][K] backward: the gradient at the normalised rows, per part of the owner's loop
    float* pr;       // [P][2N] backward: the coefficient of the row itself, per part
};

// parts the owner's loop over the 2B tiles of a set is split into: enough blocks to fill the device at small B, one at the largest
__host__ __device__ inline int parts_of(int64_t B) {
    const int p = (int)(1024 / (2 * B));
    return p < 1 ? 1 : (p > 4 ? 4 : p);
}

__host__ __device__ inline size_t ws_layout(int64_t B, int M, int K, void* base, Ws* v) {
    xmh::Arena ar(base);
    const size_t N = (size_t)B * M, BB = (size_t)B * B;
    Ws w;
    w.xn = ar.take<float>(2 * N * K);
    w.nrm = ar.take<float>(2 * N);
    w.nn = ar.take<float>(2 * N);
    w.hn = ar.take<float>(2 * (size_t)B);
    w.S[0] = ar.take<float>(BB);
    w.S[1] = ar.take<float>(BB);
    w.Ch = ar.take<float>(BB);
    for (int t = 0; t < 4; ++t) w.gD[t] = ar.take<float>(BB);
    w.part = ar.take<double>(3 * BB);
    w.upart = ar.take<double>(2 * BB);
    w.rowpart = ar.take<double>((size_t)B * 8);
    w.qpart = ar.take<double>(2 * (size_t)B);
    w.tsum = ar.take<double>(4 * (size_t)B);
    w.tcnt = ar.take<double>(4 * (size_t)B);
    w.pd = ar.take<float>((size_t)parts_of(B) * 2 * N * K);
    w.pr = ar.take<float>((size_t)parts_of(B) * 2 * N);
    if (v) *v = w;
    return ar.used;
}

struct Args {
    const float* e[2];        // e_img, e_txt [B, M, K]
    const float* h[2];        // h_img, h_txt [B, Kh]
    const uint32_t* lab;      // [B][Lw]
    int B, M, K, Kh, Lw, N;
    xmh_dimch_consts c;
};

struct Grads {
    float* e[2];
    float* h[2];
};

using xmh::wave_sum;

using xmh::inv_norm;
using trip::clamp0;                                                                                    // torch.clamp(v, 0): NaN stays

// ---- preparation -----------------------------------------------------------------------------------------------------------------------
// One wave per row.  Rows [0, 2N): token rows (x, then y).  Rows [2N, 2N + 2B): code rows, their norm only.
__global__ __launch_bounds__(kThreads) void k_dimch_prep(Args a, Ws w) {
    __shared__ float un[kWaves][kMaxK];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kWaves + wave;
    const int64_t R = 2 * (int64_t)a.N + 2 * a.B;
    const bool token = row < 2 * (int64_t)a.N;
    if (row < R && !token) {
        const int64_t r = row - 2 * (int64_t)a.N;
        const int m = r >= a.B;
        const float* src = a.h[m] + (r - (int64_t)m * a.B) * a.Kh;
        float s = 0.0f;
        for (int k = lane; k < a.Kh; k += 64) s = fmaf(src[k], src[k], s);
        s = sqrtf(wave_sum(s));
        if (lane == 0) w.hn[r] = s;
    }
    float nv = 0.0f;
    if (token) {
        const int side = row >= a.N;
        const float* src = a.e[side] + (row - (int64_t)side * a.N) * a.K;
        float s = 0.0f;
        for (int k = lane; k < a.K; k += 64) s = fmaf(src[k], src[k], s);
        nv = sqrtf(wave_sum(s));
        const float iv = inv_norm(nv, kEps);
        float* dst = w.xn + row * a.K;
        for (int k = lane; k < a.K; k += 64) {
            const float u = __fmul_rn(src[k], iv);
            un[wave][k] = u;
            dst[k] = u;
        }
    }
    __syncthreads();
    if (token && lane == 0) {
        float s = 0.0f;                                          // the chain a diagonal Gram entry runs through
        for (int k = 0; k < a.K; ++k) s = fmaf(un[wave][k], un[wave][k], s);
        w.nn[row] = s;
        w.nrm[row] = nv;
    }
}

// ---- the Gram tile ---------------------------------------------------------------------------------------------------------------------
// acc[p][q] = sum_k U[u0 + r][k] V[v0 + c][k], r = ty + 16 p, c = tx + 16 q, k ascending, one fmaf per k (0 for r, c >= M).
// us, vs: [kKC][kLd] each.  Begins and ends with a barrier around every staged chunk.
__device__ __forceinline__ void gram_tile(const float* __restrict__ U, int64_t u0, const float* __restrict__ V, int64_t v0, int M, int K, float* us,
                                          float* vs, float (&acc)[4][4]) {
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += kKC) {
        for (int idx = threadIdx.x; idx < kT * kKC; idx += kThreads) {
            const int r = idx / kKC, k = idx % kKC;
            const bool ok = r < M && k0 + k < K;
            us[k * kLd + r] = ok ? U[(u0 + r) * K + k0 + k] : 0.0f;
            vs[k * kLd + r] = ok ? V[(v0 + r) * K + k0 + k] : 0.0f;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < kKC; ++k) {
            float ua[4], vb[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) ua[p] = us[k * kLd + ty + 16 * p], vb[p] = vs[k * kLd + tx + 16 * p];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = fmaf(ua[p], vb[q], acc[p][q]);
        }
        __syncthreads();
    }
}

// squared distance of two normalised rows from their Gram entry; see the header comment
__device__ __forceinline__ float dist2(float nu, float nv, float g, const float* __restrict__ ur, const float* __restrict__ vr, int K) {
    float q = (nu + nv) - 2.0f * g;
    if (q < kNear && q != 0.0f) {
        q = 0.0f;
        for (int k = 0; k < K; ++k) {
            const float d = ur[k] - vr[k];
            q = fmaf(d, d, q);
        }
    }
    return q;
}

// Row and column statistics of the G tile in gs ([kT][kLd], M x M valid) into st ([4][kT]) and ai (chamfer / max: rows by wave 0, columns by 1):
//   smooth_chamfer: st[0] / st[1] = log sum exp of (tau sigma G) / (tau G) along the row, st[2] / st[3] along the column (all threads)
//   chamfer / max:  st[0] / st[2] = the maximum along the row / column, ai[0] / ai[1] = where it is first reached
// No barrier inside.
__device__ __forceinline__ void tile_stats(const float* gs, int M, int mode, float ts, float t1, float* st, int* ai) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (mode == XMH_DIMCH_SMOOTH_CHAMFER) {
        // two threads per line (64 rows, then 64 columns), 32 entries each; the halves meet by one shuffle, in the same order everywhere
        const int line = threadIdx.x >> 1, half = threadIdx.x & 1, col = line >= kT, l = line - col * kT;
        const int sr = col ? 1 : kLd, sc = col ? kLd : 1;
        const float* src = gs + l * sr;
        const int e0 = half * 32, e1 = min(M, e0 + 32);
        float m = -INFINITY;
        for (int e = e0; e < e1; ++e) m = fmaxf(m, src[e * sc]);
        m = fmaxf(m, __shfl_xor(m, 1));
        float s0 = 0.0f, s1 = 0.0f;
        const bool same = ts == t1;                              // sigma = 1: one sum serves both
        for (int e = e0; e < e1; ++e) {
            const float g = src[e * sc] - m;                     // a NaN entry: fmaxf dropped it, it comes back here
            s0 += expf(ts * g);
            if (!same) s1 += expf(t1 * g);
        }
        s0 += __shfl_xor(s0, 1);
        s1 = same ? s0 : s1 + __shfl_xor(s1, 1);
        if (half == 0 && l < M) {
            st[(2 * col) * kT + l] = ts * m + logf(s0);
            st[(2 * col + 1) * kT + l] = t1 * m + logf(s1);
        }
        return;
    }
    if (wave > 1 || lane >= M || mode == XMH_DIMCH_AVG) return;
    const int sr = wave == 0 ? kLd : 1, sc = wave == 0 ? 1 : kLd;         // element e of line `lane`: gs[lane * sr + e * sc]
    const float* line = gs + lane * sr;
    float m = line[0];
    int am = 0;
    for (int e = 1; e < M; ++e) {
        const float g = line[e * sc];
        if (g > m) m = g, am = e;
    }
    st[(2 * wave) * kT + lane] = m;
    ai[wave * kT + lane] = am;
}

__device__ __forceinline__ float sigmoidf(float v) { return 1.0f / (1.0f + expf(-v)); }

// ---- forward tiles ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_dimch_tiles(Args a, Ws w) {
    __shared__ float us[kKC * kLd], vs[kKC * kLd], gs[kT * kLd], st[4 * kT];
    __shared__ int ai[2 * kT];
    __shared__ double dsh[kWaves];
    __shared__ float fsh[8];
    const int B = a.B, M = a.M, K = a.K, N = a.N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if ((int64_t)blockIdx.x >= 3 * (int64_t)B * B) {
        // row r of the cosine table and the quantisation sums of code row r of both modalities
        const int r = (int)((int64_t)blockIdx.x - 3 * (int64_t)B * B);
        const float* hi = a.h[0] + (int64_t)r * a.Kh;
        const float ia = inv_norm(w.hn[r], kCosEps);
        for (int p = wave; p < B; p += kWaves) {
            const float* ht = a.h[1] + (int64_t)p * a.Kh;
            float d = 0.0f;
            for (int k = lane; k < a.Kh; k += 64) d = fmaf(hi[k], ht[k], d);
            d = wave_sum(d);
            if (lane == 0) w.Ch[(int64_t)r * B + p] = d * ia * inv_norm(w.hn[B + p], kCosEps);
        }
        for (int m = 0; m < 2; ++m) {
            double q = 0.0;
            for (int k = threadIdx.x; k < a.Kh; k += kThreads) {
                const float h = a.h[m][(int64_t)r * a.Kh + k];
                float d;
                if (a.c.hash_func == XMH_DIMCH_TANH) d = h - (h > 0.0f ? 1.0f : (h < 0.0f ? -1.0f : h));      // sign(0) = 0, a NaN stays
                else d = 2.0f * h - 1.0f;
                q += (double)(d * d);
            }
            q = xmh::block_sum<kWaves>(q, dsh);
            if (threadIdx.x == 0) w.qpart[m * B + r] = q;
        }
        return;
    }
    const int fam = (int)(blockIdx.x / ((unsigned)B * B)), ij = (int)(blockIdx.x % ((unsigned)B * B)), i = ij / B, j = ij % B;
    const int su = fam == 2 ? 1 : 0, sv = fam == 1 ? 0 : 1;                 // x.y, x.x, y.y
    const float* U = w.xn + (int64_t)su * N * K;
    const float* V = w.xn + (int64_t)sv * N * K;
    const float* nu = w.nn + (int64_t)su * N + (int64_t)i * M;
    const float* nv = w.nn + (int64_t)sv * N + (int64_t)j * M;
    float acc[4][4];
    gram_tile(U, (int64_t)i * M, V, (int64_t)j * M, M, K, us, vs, acc);
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const bool diag = fam != 0 && i == j;
    double mm = 0.0, uu = 0.0, av = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = ty + 16 * p, c = tx + 16 * q;
            if (r < M && c < M) {
                const float g = acc[p][q];
                const float q2 = dist2(nu[r], nv[c], g, U + ((int64_t)i * M + r) * K, V + ((int64_t)j * M + c) * K, K);
                mm += (double)expf(-a.c.mmd_gamma * sqrtf(q2));
                if (fam != 0 && !(diag && r == c)) uu += (double)expf(-kUnifT * q2);
                if (fam == 0) {
                    gs[r * kLd + c] = g;
                    if (a.c.mode == XMH_DIMCH_AVG) av += (double)sigmoidf(g);
                }
            }
        }
    mm = xmh::block_sum<kWaves>(mm, dsh);
    if (fam != 0) {
        uu = xmh::block_sum<kWaves>(uu, dsh);
        if (threadIdx.x == 0) {
            w.part[(int64_t)fam * B * B + ij] = mm;
            w.upart[(int64_t)(fam - 1) * B * B + ij] = uu;
        }
        return;
    }
    if (threadIdx.x == 0) w.part[ij] = mm;
    float sA, sB;                                                // s(x, y)[i][j], s(y, x)[j][i]
    if (a.c.mode == XMH_DIMCH_AVG) {
        av = xmh::block_sum<kWaves>(av, dsh);
        sA = sB = (float)(av / ((double)M * M));
    } else {
        const float t1 = a.c.temperature, ts = a.c.temperature * a.c.temperature_txt_scale;
        __syncthreads();
        tile_stats(gs, M, a.c.mode, ts, t1, st, ai);
        __syncthreads();
        if (wave < 2) {
            const bool in = lane < M;
            const float v0 = in ? st[(2 * wave) * kT + lane] : 0.0f;
            if (a.c.mode == XMH_DIMCH_MAX) {
                const float mx = xmh::wave_max(in ? v0 : -INFINITY);
                if (lane == 0) fsh[2 * wave] = mx;
            } else {
                const float v1 = (in && a.c.mode == XMH_DIMCH_SMOOTH_CHAMFER) ? st[(2 * wave + 1) * kT + lane] : 0.0f;
                const float s0 = wave_sum(v0), s1 = wave_sum(v1);
                if (lane == 0) fsh[2 * wave] = s0, fsh[2 * wave + 1] = s1;
            }
        }
        __syncthreads();
        const float fM = (float)M, den = a.c.denominator;
        if (a.c.mode == XMH_DIMCH_SMOOTH_CHAMFER) {              // fsh: rows by tau sigma, rows by tau, columns by tau sigma, columns by tau
            sA = (fsh[0] / (fM * ts) + fsh[3] / (fM * t1)) / den;
            sB = (fsh[2] / (fM * ts) + fsh[1] / (fM * t1)) / den;
        } else if (a.c.mode == XMH_DIMCH_CHAMFER) {
            sA = sB = (fsh[0] / fM + fsh[2] / fM) / den;
        } else {
            sA = sB = fsh[0];
        }
    }
    if (threadIdx.x == 0) {
        w.S[0][(int64_t)i * B + j] = sA;
        w.S[1][(int64_t)j * B + i] = sB;
    }
}

// ---- the triplet terms -----------------------------------------------------------------------------------------------------------------
// Anchor row a: label overlaps c[p], sim[p] = c > 0, weights w[p] = (2^c - 1) / Z, Z = sum_j (2^{c_(j)} - 1) / log2(j + 2) over the row
// sorted descending (the rank of p: columns with a larger count, then equal ones to its left).  All in LDS [B].  Ends with a barrier.
__device__ __forceinline__ void triplet_weights(const Args& a, int row, int* cs, float* wsh, float* sim, double* dsh) {
    trip::weights(a.lab, a.Lw, a.B, row, cs, wsh, sim, dsh);     // xmh_triplet.h
}

// the distance row of anchor `row` of term t into ds [B]; ends with a barrier
__device__ __forceinline__ void triplet_distances(const Args& a, const Ws& w, int row, int t, float* ds) {
    const int B = a.B;
    for (int p = threadIdx.x; p < B; p += kThreads) {
        const float s = t < 2 ? w.S[t][(int64_t)row * B + p] : (t == 2 ? w.Ch[(int64_t)row * B + p] : w.Ch[(int64_t)p * B + row]);
        ds[p] = clamp0(1.0f - s);
    }
    __syncthreads();
}

__device__ __forceinline__ float term_margin(const Args& a, int t) { return t < 2 ? a.c.token_triplet_margin : a.c.triplet_margin; }

__global__ __launch_bounds__(kThreads) void k_dimch_triplet(Args a, Ws w) {
    __shared__ int cs[kMaxB];
    __shared__ float wsh[kMaxB], sim[kMaxB], ds[kMaxB];
    __shared__ double dsh[kWaves];
    const int B = a.B, row = blockIdx.x;
    for (int f = 0; f < 5; ++f) {                                // row sums of the tile partials
        const double* src = (f < 3 ? w.part + (int64_t)f * B * B : w.upart + (int64_t)(f - 3) * B * B) + (int64_t)row * B;
        double s = 0.0;
        for (int j = threadIdx.x; j < B; j += kThreads) s += src[j];
        s = xmh::block_sum<kWaves>(s, dsh);
        if (threadIdx.x == 0) w.rowpart[(int64_t)row * 8 + f] = s;
    }
    triplet_weights(a, row, cs, wsh, sim, dsh);
    for (int t = 0; t < 4; ++t) {
        triplet_distances(a, w, row, t, ds);
        const float mg = term_margin(a, t);
        double sum, cnt;
        trip::row_terms(wsh, sim, ds, B, mg, dsh, &sum, &cnt);
        if (threadIdx.x == 0) w.tsum[t * B + row] = sum, w.tcnt[t * B + row] = cnt;
        __syncthreads();
    }
}

using trip::ordered_sum;

__global__ __launch_bounds__(kThreads) void k_dimch_finalize(Args a, Ws w, double* __restrict__ out12) {
    __shared__ double dsh[kWaves];
    const int B = a.B;
    double T[4], P[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, Q[2];
    for (int t = 0; t < 4; ++t) {
        const double s = ordered_sum(w.tsum + t * B, B, dsh), c = ordered_sum(w.tcnt + t * B, B, dsh);
        T[t] = s / (c + 1e-16);
    }
    for (int r = threadIdx.x; r < B; r += kThreads)
        for (int f = 0; f < 5; ++f) P[f] += w.rowpart[(int64_t)r * 8 + f];
    for (int f = 0; f < 5; ++f) P[f] = xmh::block_sum<kWaves>(P[f], dsh);
    for (int m = 0; m < 2; ++m) Q[m] = ordered_sum(w.qpart + m * B, B, dsh);
    if (threadIdx.x == 0) {
        const double NN = (double)a.N * a.N, pairs = 0.5 * a.M * (a.M - 1), cnt = (double)B * a.Kh;
        const double mmd = (P[1] - 2.0 * P[0] + P[2]) / NN;
        const double uni = a.M > 1 ? (0.5 * P[3] + 0.5 * P[4]) / pairs : 0.0;
        const double qi = a.c.hash_func == XMH_DIMCH_TANH ? Q[0] / cnt : 1.0 - Q[0] / cnt;
        const double qt = a.c.hash_func == XMH_DIMCH_TANH ? Q[1] / cnt : 1.0 - Q[1] / cnt;
        out12[0] = (T[0] + T[1]) / 2 * a.c.triplet_alpha + a.c.mmd_alpha * mmd + a.c.unif_alpha * uni +
                   (T[2] + T[3]) / 2 * a.c.hash_triplet_alpha + (qi + qt) / 2 * a.c.quan_alpha;
        out12[1] = T[0], out12[2] = T[1], out12[3] = mmd, out12[4] = uni, out12[5] = T[2], out12[6] = T[3], out12[7] = qi, out12[8] = qt;
        out12[9] = out12[10] = out12[11] = 0.0;
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// Anchor row a of the four terms: gD[t][a][p] = d loss / d (the similarity behind D_t[a][p]), upstream included.
__global__ __launch_bounds__(kThreads) void k_dimch_triplet_grad(Args a, Ws w, const float* __restrict__ up) {
    __shared__ int cs[kMaxB];
    __shared__ float wsh[kMaxB], sim[kMaxB], ds[kMaxB];
    __shared__ double dsh[kWaves];
    const int B = a.B, row = blockIdx.x;
    const float g = up ? up[0] : 1.0f;
    triplet_weights(a, row, cs, wsh, sim, dsh);
    for (int t = 0; t < 4; ++t) {
        const double total = ordered_sum(w.tcnt + t * B, B, dsh);
        const float scale = g * 0.5f * (t < 2 ? a.c.triplet_alpha : a.c.hash_triplet_alpha) / (float)(total + 1e-16);
        triplet_distances(a, w, row, t, ds);
        const float mg = term_margin(a, t);
        for (int p = threadIdx.x; p < B; p += kThreads) {
            const float s = t < 2 ? w.S[t][(int64_t)row * B + p] : (t == 2 ? w.Ch[(int64_t)row * B + p] : w.Ch[(int64_t)p * B + row]);
            const float gd = trip::col_grad(wsh, sim, ds, B, mg, p) * scale;
            w.gD[t][(int64_t)row * B + p] = -gd * ((1.0f - s) >= 0.0f ? 1.0f : 0.0f);       // clamp(1 - s, 0) backward
        }
        __syncthreads();
    }
}

// kKS: 64-column slots of K a thread holds (K <= 64 kKS)
template <int kKS>
__global__ __launch_bounds__(kThreads) void k_dimch_owner(Args a, Ws w, const float* __restrict__ up, Grads gr, int accumulate, int P) {
    __shared__ float stage[2 * kKC * kLd], gs[kT * kLd], st[4 * kT];          // stage: the Gram operands, then 64 x 64 of V
    __shared__ __attribute__((aligned(16))) float wt[kT * kLdW];       // wt[c][r] = d loss / d G[r][c]
    float* const us = stage;
    float* const vs = stage + kKC * kLd;
    static_assert(2 * kKC * kLd >= kT * 64, "the staging buffer holds 64 columns of a set");
    __shared__ int ai[2 * kT];
    __shared__ int best[2];
    const int B = a.B, M = a.M, K = a.K, N = a.N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float g = up ? up[0] : 1.0f;

    if ((int)blockIdx.x >= 2 * B * P) {
        // gradient of code row r of modality m: through both cosine tables and the quantisation term
        const int rr = blockIdx.x - 2 * B * P, m = rr >= B, r = rr - m * B, k = threadIdx.x;
        if (!gr.h[m] || k >= a.Kh) return;
        const float* own = a.h[m] + (int64_t)r * a.Kh;
        const float no = w.hn[m * B + r], io = inv_norm(no, kCosEps);
        const float hk = own[k];
        double acc = 0.0;
        for (int p = 0; p < B; ++p) {
            const int64_t at = m == 0 ? (int64_t)r * B + p : (int64_t)p * B + r, ta = m == 0 ? (int64_t)p * B + r : (int64_t)r * B + p;
            const float cf = w.gD[2][at] + w.gD[3][ta];
            const float cosv = w.Ch[at];
            const float other = a.h[1 - m][(int64_t)p * a.Kh + k] * inv_norm(w.hn[(1 - m) * B + p], kCosEps);
            const float self = no < kCosEps ? 0.0f : cosv * hk * io;
            acc += (double)(cf * ((other - self) * io));
        }
        const float cnt = (float)B * (float)a.Kh;
        float qd;
        if (a.c.hash_func == XMH_DIMCH_TANH) qd = 2.0f * (hk - (hk > 0.0f ? 1.0f : (hk < 0.0f ? -1.0f : hk))) / cnt;
        else qd = -4.0f * (2.0f * hk - 1.0f) / cnt;
        const float d = (float)acc + g * 0.5f * a.c.quan_alpha * qd;
        float* out = gr.h[m] + (int64_t)r * a.Kh;
        out[k] = accumulate ? out[k] + d : d;
        return;
    }

    const int part = blockIdx.x % P, side = (blockIdx.x / P) / B, i = (blockIdx.x / P) % B;
    if (!gr.e[side]) return;
    const float* U = w.xn + (int64_t)side * N * K;
    const float* nu = w.nn + (int64_t)side * N + (int64_t)i * M;
    const float NN = (float)N * (float)N;
    const float cu = M > 1 ? g * 2.0f * a.c.unif_alpha / (0.5f * (float)M * (float)(M - 1)) : 0.0f;
    const float t1 = a.c.temperature, ts = a.c.temperature * a.c.temperature_txt_scale;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    float out[16][kKS];
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int s = 0; s < kKS; ++s) out[r][s] = 0.0f;
    float racc = 0.0f;                                           // thread t < kT: the coefficient of its own row u_t (sum of the distance terms)

    // tiles [0, B): set j of the other side (x.y); tiles [B, 2B): set j of its own side (x.x or y.y).  Part `part` takes its share in order.
    const int t_lo = (int)((int64_t)2 * B * part / P), t_hi = (int)((int64_t)2 * B * (part + 1) / P);
    for (int t = t_lo; t < t_hi; ++t) {
        const int fam = t >= B, j = t - fam * B;
        const int sv = fam == 0 ? 1 - side : side;
        const float* V = w.xn + (int64_t)sv * N * K;
        const float cm = (fam == 0 ? -4.0f : 4.0f) * g * a.c.mmd_alpha / NN;
        const float* nv = w.nn + (int64_t)sv * N + (int64_t)j * M;
        float acc[4][4];
        gram_tile(U, (int64_t)i * M, V, (int64_t)j * M, M, K, us, vs, acc);
        const bool diag = fam == 1 && i == j;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = ty + 16 * p, c = tx + 16 * q;
                float e = 0.0f;
                if (r < M && c < M) {
                    const float q2 = dist2(nu[r], nv[c], acc[p][q], U + ((int64_t)i * M + r) * K, V + ((int64_t)j * M + c) * K, K);
                    const float sq = sqrtf(q2);
                    // d exp(-gamma sqrt(q)) / dq, 0 at q = 0 as torch.cdist's backward; a NaN stays
                    e = q2 == 0.0f ? 0.0f : cm * (-a.c.mmd_gamma * expf(-a.c.mmd_gamma * sq) / (2.0f * sq));
                    if (fam == 1 && !(diag && r == c)) e += cu * (-kUnifT * expf(-kUnifT * q2));
                }
                wt[c * kLdW + r] = -e;                       // d q / d u_r = 2 (u_r - v_c): e (u_r - v_c) is folded as -e on v_c, +e on u_r
                if (fam == 0) gs[r * kLd + c] = acc[p][q];
            }
        __syncthreads();
        if (threadIdx.x < kT) {
            float s = 0.0f;
            for (int c = 0; c < M; ++c) s += wt[c * kLdW + threadIdx.x];
            racc -= s;
        }
        if (fam == 0) {
            const float A = side == 0 ? w.gD[0][(int64_t)i * B + j] : w.gD[1][(int64_t)i * B + j];       // d / d s(own, other)[i][j]
            const float Bc = side == 0 ? w.gD[1][(int64_t)j * B + i] : w.gD[0][(int64_t)j * B + i];      // d / d s(other, own)[j][i]
            tile_stats(gs, M, a.c.mode, ts, t1, st, ai);
            __syncthreads();
            if (a.c.mode == XMH_DIMCH_MAX && wave == 0) {    // the first maximum in row-major order
                const float mine = lane < M ? st[lane] : -INFINITY;
                const float mx = xmh::wave_max(mine);
                const unsigned long long hit = __ballot(lane < M && mine == mx);
                if (lane == 0) {
                    const int r0 = hit ? __ffsll((long long)hit) - 1 : 0;
                    best[0] = r0, best[1] = ai[r0];
                }
            }
            if (a.c.mode == XMH_DIMCH_MAX) __syncthreads();
            const float fM = (float)M;
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = ty + 16 * p, c = tx + 16 * q;
                    if (r < M && c < M) {
                        const float gv = gs[r * kLd + c];
                        float d;
                        if (a.c.mode == XMH_DIMCH_SMOOTH_CHAMFER) {
                            const float prs = expf(ts * gv - st[r]), pcs = expf(ts * gv - st[2 * kT + c]);
                            const float pr1 = ts == t1 ? prs : expf(t1 * gv - st[kT + r]);
                            const float pc1 = ts == t1 ? pcs : expf(t1 * gv - st[3 * kT + c]);
                            d = (A * (prs + pc1) + Bc * (pcs + pr1)) / (a.c.denominator * fM);
                        } else if (a.c.mode == XMH_DIMCH_CHAMFER) {
                            d = (A + Bc) * ((ai[r] == c ? 1.0f : 0.0f) + (ai[kT + c] == r ? 1.0f : 0.0f)) / (a.c.denominator * fM);
                        } else if (a.c.mode == XMH_DIMCH_MAX) {
                            d = (r == best[0] && c == best[1]) ? A + Bc : 0.0f;
                        } else {
                            const float sg = sigmoidf(gv);
                            d = (A + Bc) * (sg * (1.0f - sg)) / (fM * fM);
                        }
                        wt[c * kLdW + r] += d;
                    }
                }
        }
        __syncthreads();
        // out[rows wave * 16 ..][k] += sum_c wt[c][row] V[j M + c][k], 64 columns of V staged at a time
#pragma unroll
        for (int s = 0; s < kKS; ++s) {
            if (64 * s < K) {                                // block-uniform
                for (int idx = threadIdx.x; idx < kT * 64; idx += kThreads) {
                    const int c = idx >> 6, k = 64 * s + (idx & 63);
                    stage[idx] = (c < M && k < K) ? V[((int64_t)j * M + c) * K + k] : 0.0f;
                }
                __syncthreads();
                for (int c = 0; c < M; ++c) {
                    const float vk = stage[c * 64 + lane];
                    const float4* wr = reinterpret_cast<const float4*>(wt + c * kLdW + wave * 16);
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const float4 wv = wr[r4];
                        out[r4 * 4 + 0][s] = fmaf(wv.x, vk, out[r4 * 4 + 0][s]);
                        out[r4 * 4 + 1][s] = fmaf(wv.y, vk, out[r4 * 4 + 1][s]);
                        out[r4 * 4 + 2][s] = fmaf(wv.z, vk, out[r4 * 4 + 2][s]);
                        out[r4 * 4 + 3][s] = fmaf(wv.w, vk, out[r4 * 4 + 3][s]);
                    }
                }
                __syncthreads();
            }
        }
    }
    // this part's share: the gradient at the normalised rows and the rows' own coefficients; k_dimch_rows adds the parts in order
    float* pd = w.pd + ((int64_t)part * 2 + side) * N * K;
    if ((int)threadIdx.x < M) w.pr[((int64_t)part * 2 + side) * N + (int64_t)i * M + threadIdx.x] = racc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = wave * 16 + r;
        if (row >= M) continue;                                  // wave-uniform
#pragma unroll
        for (int s = 0; s < kKS; ++s) {
            const int k = lane + 64 * s;
            if (k < K) pd[((int64_t)i * M + row) * K + k] = out[r][s];
        }
    }
}

// One wave per token row: du = sum over the parts (in order) of the owner's shares + (sum of the coefficients) u, then the backward
// of F.normalize: d = (du - u (u . du)) / max(|v|, eps); a clamped row passes du / eps only, a NaN norm stays NaN.
__global__ __launch_bounds__(kThreads) void k_dimch_rows(Args a, Ws w, Grads gr, int accumulate, int P) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, K = a.K;
    const int64_t row = (int64_t)blockIdx.x * kWaves + wave, N = a.N;
    if (row >= 2 * N) return;
    const int side = row >= N;
    if (!gr.e[side]) return;
    float rc = 0.0f;
    for (int p = 0; p < P; ++p) rc += w.pr[(int64_t)p * 2 * N + row];
    const float* u = w.xn + row * K;
    float du[4], dot = 0.0f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int k = lane + 64 * s;
        du[s] = 0.0f;
        if (k < K) {
            float d = 0.0f;
            for (int p = 0; p < P; ++p) d += w.pd[((int64_t)p * 2 * N + row) * K + k];
            du[s] = fmaf(rc, u[k], d);
            dot = fmaf(u[k], du[s], dot);
        }
    }
    dot = wave_sum(dot);
    const float nv = w.nrm[row], iv = inv_norm(nv, kEps);
    if (nv < kEps) dot = 0.0f;
    float* out = gr.e[side] + (row - (int64_t)side * N) * K;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int k = lane + 64 * s;
        if (k < K) {
            const float d = (du[s] - u[k] * dot) * iv;
            out[k] = accumulate ? out[k] + d : d;
        }
    }
}

// shared argument checks: they run before any HIP call
int check_args(const char* who, const float* e_img, const float* e_txt, const float* h_img, const float* h_txt, int64_t B, int M, int K, int Kh,
               int C, const uint32_t* lab, const xmh_dimch_consts* cst, void* ws, size_t ws_bytes) {
    if (B <= 0 || M <= 0 || K <= 0 || Kh <= 0 || C <= 0)
        return xmh::fail(XMH_EINVAL, "%s: bad shape B=%lld M=%d K=%d Kh=%d C=%d", who, (long long)B, M, K, Kh, C);
    if (B > kMaxB || M > kMaxM || K > kMaxK || Kh > kMaxK || C > kMaxC)
        return xmh::fail(XMH_ENOTSUP, "%s: B=%lld M=%d K=%d Kh=%d C=%d outside B <= %d, M <= %d, K, Kh <= %d, C <= %d", who, (long long)B, M, K,
                         Kh, C, kMaxB, kMaxM, kMaxK, kMaxC);
    if (!e_img || !e_txt || !h_img || !h_txt || !lab || !cst || !ws) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (cst->mode < XMH_DIMCH_SMOOTH_CHAMFER || cst->mode > XMH_DIMCH_AVG) return xmh::fail(XMH_EINVAL, "%s: mode %d", who, cst->mode);
    if (cst->hash_func != XMH_DIMCH_TANH && cst->hash_func != XMH_DIMCH_SOFTMAX) return xmh::fail(XMH_EINVAL, "%s: hash_func %d", who, cst->hash_func);
    if (cst->mode == XMH_DIMCH_SMOOTH_CHAMFER && !(cst->temperature > 0.0f && cst->temperature_txt_scale > 0.0f))
        return xmh::fail(XMH_EINVAL, "%s: temperature %g and temperature_txt_scale %g must be positive", who, (double)cst->temperature,
                         (double)cst->temperature_txt_scale);
    if (cst->mode <= XMH_DIMCH_CHAMFER && !(cst->denominator != 0.0f)) return xmh::fail(XMH_EINVAL, "%s: denominator 0", who);
    return xmh::check_workspace(who, ws, ws_bytes, ws_layout(B, M, K, nullptr, nullptr), "xmh_dimch_loss_ws_bytes", XMH_ENOMEM);
}

Args make_args(const float* e_img, const float* e_txt, const float* h_img, const float* h_txt, int64_t B, int M, int K, int Kh, int C,
               const uint32_t* lab, const xmh_dimch_consts* cst) {
    Args a;
    a.e[0] = e_img, a.e[1] = e_txt, a.h[0] = h_img, a.h[1] = h_txt, a.lab = lab;
    a.B = (int)B, a.M = M, a.K = K, a.Kh = Kh, a.Lw = (C + 31) / 32, a.N = (int)B * M;
    a.c = *cst;
    return a;
}

// the three launches both entry points begin with
void launch_common(const Args& a, const Ws& v, hipStream_t st) {
    const int64_t rows = 2 * (int64_t)a.N + 2 * a.B;
    hipLaunchKernelGGL(k_dimch_prep, dim3((unsigned)((rows + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, a, v);
    hipLaunchKernelGGL(k_dimch_tiles, dim3((unsigned)(3 * a.B * a.B + a.B)), dim3(kThreads), 0, st, a, v);
    hipLaunchKernelGGL(k_dimch_triplet, dim3((unsigned)a.B), dim3(kThreads), 0, st, a, v);
}

}  // namespace

extern "C" size_t xmh_dimch_loss_ws_bytes(int64_t B, int M, int K, int C) {
    if (B <= 0 || M <= 0 || K <= 0 || C <= 0 || B > kMaxB || M > kMaxM || K > kMaxK || C > kMaxC) return 0;
    return ws_layout(B, M, K, nullptr, nullptr);
}

extern "C" int xmh_dimch_loss(const float* e_img, const float* e_txt, const float* h_img, const float* h_txt, int64_t B, int M, int K, int Kh,
                              int C, const uint32_t* lab, const xmh_dimch_consts* cst, void* ws, size_t ws_bytes, double* out12,
                              xmh_stream_t stream) {
    XMH_RANGE("xmh_dimch_loss");
    if (int rc = check_args("xmh_dimch_loss", e_img, e_txt, h_img, h_txt, B, M, K, Kh, C, lab, cst, ws, ws_bytes)) return rc;
    if (!out12) return xmh::fail(XMH_EINVAL, "xmh_dimch_loss: null pointer");
    Ws v;
    ws_layout(B, M, K, ws, &v);
    const Args a = make_args(e_img, e_txt, h_img, h_txt, B, M, K, Kh, C, lab, cst);
    hipStream_t st = xmh::as_stream(stream);
    launch_common(a, v, st);
    hipLaunchKernelGGL(k_dimch_finalize, dim3(1), dim3(kThreads), 0, st, a, v, out12);
    XMH_LAUNCH_CHECK("xmh_dimch_loss");
    return XMH_OK;
}

extern "C" int xmh_dimch_loss_grad(const float* e_img, const float* e_txt, const float* h_img, const float* h_txt, int64_t B, int M, int K, int Kh,
                                   int C, const uint32_t* lab, const xmh_dimch_consts* cst, const float* upstream, float* grad_e_img,
                                   float* grad_e_txt, float* grad_h_img, float* grad_h_txt, int accumulate, void* ws, size_t ws_bytes,
                                   xmh_stream_t stream) {
    XMH_RANGE("xmh_dimch_loss_grad");
    if (int rc = check_args("xmh_dimch_loss_grad", e_img, e_txt, h_img, h_txt, B, M, K, Kh, C, lab, cst, ws, ws_bytes)) return rc;
    if (!grad_e_img && !grad_e_txt && !grad_h_img && !grad_h_txt) return XMH_OK;
    Ws v;
    ws_layout(B, M, K, ws, &v);
    const Args a = make_args(e_img, e_txt, h_img, h_txt, B, M, K, Kh, C, lab, cst);
    Grads gr;
    gr.e[0] = grad_e_img, gr.e[1] = grad_e_txt, gr.h[0] = grad_h_img, gr.h[1] = grad_h_txt;
    hipStream_t st = xmh::as_stream(stream);
    launch_common(a, v, st);
    hipLaunchKernelGGL(k_dimch_triplet_grad, dim3((unsigned)B), dim3(kThreads), 0, st, a, v, upstream);
    const int P = parts_of(B);
    const dim3 grid((unsigned)(2 * B * P + 2 * B));
    if (K <= 64) hipLaunchKernelGGL(k_dimch_owner<1>, grid, dim3(kThreads), 0, st, a, v, upstream, gr, accumulate, P);
    else if (K <= 128) hipLaunchKernelGGL(k_dimch_owner<2>, grid, dim3(kThreads), 0, st, a, v, upstream, gr, accumulate, P);
    else hipLaunchKernelGGL(k_dimch_owner<4>, grid, dim3(kThreads), 0, st, a, v, upstream, gr, accumulate, P);
    hipLaunchKernelGGL(k_dimch_rows, dim3((unsigned)((2 * (int64_t)a.N + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, a, v, gr, accumulate, P);
    XMH_LAUNCH_CHECK("xmh_dimch_loss_grad");
    return XMH_OK;
}
