// MITH's training objective (reference models/MITH/MITH.py:116-232) and its gradient with respect to its eight inputs.
//
//   Y [N, K] the rolling code buffer (one tensor on the GPU, MITH.py:169-177), S = label_sim [N, B], codes c_i, c_t, t_i, t_t [B, K]
//   likelihood of code x:  s = 0.5 clamp(Y x^T, -64, 64),  -mean(S s - log(1 + exp(s)))  for x = t_i, t_t, c_t, c_i
//                          (intra_i, intra_t, i2t, t2i)
//   InfoNCE (tau 0.07):    cls:    one [B, B] problem  res_img_cls res_txt_cls^T / tau, CE over rows and over columns, averaged
//                          tokens: B [K, K] problems   T_i[:, b, :] T_t[:, b, :]^T / tau, read in place from the [K, B, D] layout
//   quantisation, distillation: elementwise over [B, K]
//
//   xmh_mith_loss       k_mith_lik<false>  (4B stacked code columns x N-row chunks: 64 x 64 dot tiles, per-block partials of the
//                                           four likelihood sums)
//                       k_mith_nce_logits  (64 x 64 logit tiles of the cls problem and of every sample's token problem -> ws)
//                       k_mith_nce_lse     (one wave per logit row and column: log-sum-exp as (max, log sum), its cross-entropy
//                                           term -> ws)
//                       k_mith_finalize    (one block: ordered sums of the partials, quantisation, distillation -> out10)
//   xmh_mith_loss_grad  k_mith_lik<true>   (the same dot tiles -> the weights (S - sigma(s)) m in LDS -> per-chunk partials of
//                                           sum_n w[n, b] Y[n] for each code column)
//                       k_mith_nce_logits, k_mith_nce_lse (as in the forward)
//                       k_mith_grad        (blocks of 64 x 64 tiles of dA = G T_t and dB = G^T T_i per problem, G formed on the fly
//                                           from the logits and the two lse vectors; then the [B, K] code gradients: the chunk
//                                           partials summed in order, plus quantisation and distillation)
//
// All products use fp32 FMA over 64 x 64 register-tiled output blocks (4 x 4 per thread, operands staged through LDS 16 reduction
// steps at a time).  Every output element is accumulated in one fixed order, sums of terms are double and cross blocks only through
// per-block partials summed in index order: no float atomics, two calls on the same inputs agree to the bit.  The forward and the
// gradient form the likelihood dot products with the same routine, so both see the same clamp mask.  No call allocates or
// synchronises with the host.
//
// Non-finite inputs pass through as they do through the reference's expression.  A NaN dot product (a NaN in a buffer or code row,
// or Inf entries of both signs) stays NaN through the clamp, so the likelihoods it enters and the loss are NaN: the buffer keeps such a
// row for the rest of the epoch, and every step that reads it must say so.  In the gradient the clamp's mask is a select, 0 for a NaN
// product as torch's clamp backward selects it, so only 0 * Y[n] of the non-finite entries of that buffer row turns NaN.
#include "xmh_common.h"
#include "xmh_device.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = 64, kKc = 16, kLd = kTile + 4;     // output tile, reduction chunk, LDS row stride (16-byte rows)
constexpr int64_t kMaxN = int64_t(1) << 22;
constexpr int kMaxB = 1024, kMaxK = 256, kMaxD = 2048;
constexpr int kLikTarget = 1024;                          // blocks the likelihood grid aims for (sets the N chunk count P)

// the likelihood grid: kTile-column tiles of the 4B stacked code columns x P chunks of `rows` rows of N (a whole number of tiles).
// Depends on the shape only, so the forward, the gradient and the workspace agree on it.
struct LikGrid {
    int ctiles, P, rows;
};

__host__ __device__ inline LikGrid lik_grid(int64_t N, int B) {
    LikGrid g;
    g.ctiles = (4 * B + kTile - 1) / kTile;
    const int64_t ntiles = (N + kTile - 1) / kTile;
    int64_t P = (kLikTarget + g.ctiles - 1) / g.ctiles;
    if (P > ntiles) P = ntiles;
    if (P < 1) P = 1;
    const int64_t per = (ntiles + P - 1) / P;            // row tiles per chunk
    g.rows = (int)(per * kTile);
    g.P = (int)((ntiles + per - 1) / per);
    return g;
}

struct WsView {
    double* lik;      // [P * ctiles][4] per-block likelihood sums of S s - log(1 + exp(s))
    double* ce;       // [2B + 2BK] cross-entropy term of each logit line (cls rows, cls cols, token rows, token cols)
    float2* lse;      // [2B + 2BK] log-sum-exp of each line in two parts: x = its largest logit m, y = log sum exp(logit - m).  One
                      // float for m + log(...) would carry the rounding of a number the size of the logits (up to 1 / tau = 14) into
                      // every softmax; log_softmax as torch forms it, (logit - m) - log(...), does not
    float* logits;    // [B * B] cls, then [B][K][K] tokens (already divided by tau)
    float* gpart;     // [P][4B][K] per-chunk likelihood gradient sums (gradient only)
};

__host__ __device__ inline size_t ws_layout(int64_t N, int B, int K, void* base, WsView* v) {
    const LikGrid g = lik_grid(N, B);
    const size_t lines = (size_t)2 * B + (size_t)2 * B * K;
    xmh::Arena ar(base);
    WsView w;
    w.lik = ar.take<double>((size_t)g.P * g.ctiles * 4);
    w.ce = ar.take<double>(lines);
    w.lse = ar.take<float2>(lines);
    w.logits = ar.take<float>((size_t)B * B + (size_t)B * K * K);
    w.gpart = ar.take<float>((size_t)g.P * 4 * B * K);
    if (v) *v = w;
    return ar.used;
}

// the kernels' view of xmh_mith_loss_args (device pointers), the codes stacked in likelihood order (t_i, t_t, c_t, c_i)
struct Args {
    int64_t N;
    int B, K, D;
    const float *rci, *rct, *ci, *ct, *ti, *tt, *Ti, *Tt, *Y, *S;
    double w_intra, w_distill, w_nce, w_inter, w_quan, alpha;
    float lambda, mu, tau;                                // fp32 lambda, 1 - lambda (taken in double) and temperature, as torch uses them
};

struct Grads {
    float* g[8];      // xmh_mith_loss_args input order: res_img_cls, res_txt_cls, img_cls_hash, txt_cls_hash, tokens_hash_i,
                      // tokens_hash_t, trans_tokens_i, trans_tokens_t (NULL = not needed)
};

using xmh::wave_max;
using xmh::wave_sum;

// ---- operands of the tile products: element (m, k), 0 outside [0, M) x [0, Kr) -------------------------------------------------
struct Strided {
    const float* p;
    int64_t sm, sk;
    int M, Kr;
    __device__ __forceinline__ float operator()(int m, int k) const {
        return (m < M && k < Kr) ? p[(int64_t)m * sm + (int64_t)k * sk] : 0.0f;
    }
};

// column c of the 4B stacked code columns: code c / B (t_i, t_t, c_t, c_i), row c % B
struct Stacked {
    const float* q[4];
    int B, K;
    __device__ __forceinline__ float operator()(int c, int k) const {
        if (c >= 4 * B || k >= K) return 0.0f;
        const int code = c / B;
        const float* p = code == 0 ? q[0] : code == 1 ? q[1] : code == 2 ? q[2] : q[3];
        return p[(int64_t)(c - code * B) * K + k];
    }
};

// InfoNCE gradient G[i][j] = coef (softmax_row[i][j] + softmax_col[i][j] - 2 [i == j]) from the stored logits and the two parts of
// each line's log-sum-exp (lr of the rows, lc of the columns); kT: element (m, k) is G[k][m] (for G^T products)
template <bool kT>
struct NceG {
    const float* L;
    const float2 *lr, *lc;
    int R;
    float coef;
    __device__ __forceinline__ float operator()(int m, int k) const {
        const int i = kT ? k : m, j = kT ? m : k;
        if (i >= R || j >= R) return 0.0f;
        const float x = L[(int64_t)i * R + j];
        const float2 r = lr[i], c = lc[j];
        const float p = expf((x - r.x) - r.y) + expf((x - c.x) - c.y) - (i == j ? 2.0f : 0.0f);
        return coef * p;
    }
};

// stage a kTile x kKc chunk of an operand into S[k][m]; kContig: the operand is contiguous along k (lanes walk k), else along m
template <bool kContig, class Op>
__device__ __forceinline__ void stage(const Op& op, int m0, int k0, float (*S)[kLd]) {
#pragma unroll
    for (int e = 0; e < kTile * kKc / kThreads; ++e) {
        const int idx = threadIdx.x + e * kThreads;
        const int k = kContig ? idx % kKc : idx / kTile;
        const int m = kContig ? idx / kKc : idx % kTile;
        S[k][m] = op(m0 + m, k0 + k);
    }
}

// acc[i][j] += sum_k A(m0 + 4 tm + i, k) B(n0 + 4 tn + j, k), k in [0, Kr) in increasing order (tm = tid % 16, tn = tid / 16)
template <bool cA, bool cB, class OpA, class OpB>
__device__ __forceinline__ void mm_tile(float (&acc)[4][4], const OpA& a, const OpB& b, int m0, int n0, int Kr, float (*As)[kLd],
                                        float (*Bs)[kLd]) {
    const int tm = threadIdx.x & 15, tn = threadIdx.x >> 4;
    for (int k0 = 0; k0 < Kr; k0 += kKc) {
        __syncthreads();
        stage<cA>(a, m0, k0, As);
        stage<cB>(b, n0, k0, Bs);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kKc; ++kk) {
            const float4 av = *reinterpret_cast<const float4*>(&As[kk][tm * 4]);
            const float4 bv = *reinterpret_cast<const float4*>(&Bs[kk][tn * 4]);
            const float ar[4] = {av.x, av.y, av.z, av.w}, br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(ar[i], br[j], acc[i][j]);
        }
    }
}

__device__ __forceinline__ void zero(float (&acc)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
}

// ---- likelihoods ---------------------------------------------------------------------------------------------------------------
// Block (x, y): stacked code columns [64 x, 64 x + 64), rows [y rows, (y + 1) rows) of N in 64-row tiles.
// kGrad = false: the four sums of S s - log(1 + exp(s)) over the block -> ws.lik.
// kGrad = true:  gpart[y][c][k] = sum_n w[n][c] Y[n][k], w = -(0.5 / (N B)) (S - sigma(s)) [|Y x| <= 64], n over the chunk in order.
template <bool kGrad, int KT>
__global__ __launch_bounds__(kThreads) void k_mith_lik(Args a, WsView ws, LikGrid g) {
    __shared__ __attribute__((aligned(16))) float As[kKc][kLd];
    __shared__ __attribute__((aligned(16))) float Bs[kKc][kLd];
    __shared__ __attribute__((aligned(16))) float Ws[kGrad ? kTile : 1][kLd];   // [n][c]
    __shared__ __attribute__((aligned(16))) float Ys[kGrad ? kTile : 1][kLd];   // [n][k]
    __shared__ double red[kWaves];
    const int tm = threadIdx.x & 15, tn = threadIdx.x >> 4;
    const int B = a.B, K = a.K, C4 = 4 * B;
    const int c0 = blockIdx.x * kTile;
    const int64_t r0 = (int64_t)blockIdx.y * g.rows, r1 = min(a.N, r0 + g.rows);
    const Stacked X{{a.ti, a.tt, a.ct, a.ci}, B, K};
    const float wcoef = (float)(-0.5 / ((double)a.N * (double)B));
    double part[4] = {0.0, 0.0, 0.0, 0.0};
    float gacc[KT][4][4];
#pragma unroll
    for (int t = 0; t < KT; ++t) zero(gacc[t]);

    for (int64_t n0 = r0; n0 < r1; n0 += kTile) {
        const int nrem = (int)min((int64_t)kTile, r1 - n0);
        const Strided Yt{a.Y + n0 * K, K, 1, nrem, K};
        float acc[4][4];
        zero(acc);
        mm_tile<true, true>(acc, Yt, X, 0, c0, K, As, Bs);     // acc[i][j] = Y[n0 + 4 tm + i] . x[c0 + 4 tn + j]
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int nl = tm * 4 + i;
            const int64_t n = n0 + nl;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + tn * 4 + j;
                const bool live = nl < nrem && c < C4;
                const int code = live ? c / B : 0;
                const float d = acc[i][j];
                const float s = 0.5f * (isnan(d) ? d : fminf(fmaxf(d, -64.0f), 64.0f));   // torch's clamp keeps a NaN, fmaxf drops it
                const float Sv = live ? a.S[n * B + (c - code * B)] : 0.0f;
                const float e = expf(s);
                if (!kGrad) {
                    const double v = live ? (double)(Sv * s) - (double)log1pf(e) : 0.0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) part[q] += code == q ? v : 0.0;
                } else {
                    const bool pass = d >= -64.0f && d <= 64.0f;                 // clamp' on the closed interval, as torch's; a
                    Ws[nl][tn * 4 + j] = live && pass ? wcoef * (Sv - e / (1.0f + e)) : 0.0f;   // select: 0 for a NaN d, not NaN * 0
                }
            }
        }
        if (kGrad) {
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                __syncthreads();                               // Ws written (t = 0) / Ys of the previous t consumed
                for (int e = threadIdx.x; e < kTile * kTile; e += kThreads) {
                    const int nl = e / kTile, kl = e % kTile, k = t * kTile + kl;
                    Ys[nl][kl] = (nl < nrem && k < K) ? a.Y[(n0 + nl) * K + k] : 0.0f;
                }
                __syncthreads();
                for (int nl = 0; nl < kTile; ++nl) {
                    const float4 wv = *reinterpret_cast<const float4*>(&Ws[nl][tm * 4]);
                    const float4 yv = *reinterpret_cast<const float4*>(&Ys[nl][tn * 4]);
                    const float wr[4] = {wv.x, wv.y, wv.z, wv.w}, yr[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) gacc[t][i][j] = fmaf(wr[i], yr[j], gacc[t][i][j]);
                }
            }
        }
    }
    if (!kGrad) {
        const int blk = blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double s = xmh::block_sum<kWaves>(part[q], red);
            if (threadIdx.x == 0) ws.lik[(int64_t)blk * 4 + q] = s;
        }
    } else {
        float* out = ws.gpart + (int64_t)blockIdx.y * C4 * K;
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = c0 + tm * 4 + i;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = t * kTile + tn * 4 + j;
                    if (c < C4 && k < K) out[(int64_t)c * K + k] = gacc[t][i][j];
                }
            }
    }
}

// ---- InfoNCE -------------------------------------------------------------------------------------------------------------------
// problem 0: cls, R = B rows of res_*_cls (row stride D); problem 1 + b: the tokens of sample b, R = K rows at stride B D, offset b D
struct Problem {
    const float *A, *Bm;
    int64_t rs;
    int R;
    float* L;          // its [R, R] logits
    int line;          // index of its first row line in ws.ce / ws.lse; its column lines follow after `cstride`
    int cstride;
};

__device__ __forceinline__ Problem problem(const Args& a, const WsView& ws, int p, bool grads_in, float* const* g, float** ga, float** gb) {
    Problem q;
    const int B = a.B, K = a.K, D = a.D;
    if (p == 0) {
        q.A = a.rci; q.Bm = a.rct; q.rs = D; q.R = B; q.L = ws.logits; q.line = 0; q.cstride = B;
        if (grads_in) { *ga = g[0]; *gb = g[1]; }
    } else {
        const int b = p - 1;
        q.A = a.Ti + (int64_t)b * D; q.Bm = a.Tt + (int64_t)b * D; q.rs = (int64_t)B * D; q.R = K;
        q.L = ws.logits + (int64_t)B * B + (int64_t)b * K * K;
        q.line = 2 * B + b * K; q.cstride = B * K;
        if (grads_in) {
            *ga = g[6] ? g[6] + (int64_t)b * D : nullptr;
            *gb = g[7] ? g[7] + (int64_t)b * D : nullptr;
        }
    }
    return q;
}

// one block per 64 x 64 logit tile: blocks [0, tc^2) the cls problem, then tk^2 per sample
__global__ __launch_bounds__(kThreads) void k_mith_nce_logits(Args a, WsView ws) {
    __shared__ __attribute__((aligned(16))) float As[kKc][kLd];
    __shared__ __attribute__((aligned(16))) float Bs[kKc][kLd];
    const int tc = (a.B + kTile - 1) / kTile, tk = (a.K + kTile - 1) / kTile;
    int blk = blockIdx.x, p, nt;
    if (blk < tc * tc) {
        p = 0;
        nt = tc;
    } else {
        blk -= tc * tc;
        p = 1 + blk / (tk * tk);
        blk %= tk * tk;
        nt = tk;
    }
    const Problem q = problem(a, ws, p, false, nullptr, nullptr, nullptr);
    const int m0 = (blk / nt) * kTile, n0 = (blk % nt) * kTile;
    const Strided opA{q.A, q.rs, 1, q.R, a.D}, opB{q.Bm, q.rs, 1, q.R, a.D};
    float acc[4][4];
    zero(acc);
    mm_tile<true, true>(acc, opA, opB, m0, n0, a.D, As, Bs);
    const int tm = threadIdx.x & 15, tn = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = m0 + tm * 4 + i, c = n0 + tn * 4 + j;
            if (r < q.R && c < q.R) q.L[(int64_t)r * q.R + c] = acc[i][j] / a.tau;     // scores /= temperature (MITH.py:121)
        }
}

// one wave per line: lines [0, B) cls rows, [B, 2B) cls columns, [2B, 2B + BK) token rows (sample-major), then token columns
__global__ __launch_bounds__(kThreads) void k_mith_nce_lse(Args a, WsView ws) {
    const int lane = threadIdx.x & 63;
    const int64_t line = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int B = a.B, K = a.K;
    const int64_t lines = 2 * (int64_t)B + 2 * (int64_t)B * K;
    if (line >= lines) return;
    const float* L;
    int R, idx;
    bool col;
    if (line < 2 * B) {
        L = ws.logits; R = B; col = line >= B; idx = (int)(col ? line - B : line);
    } else {
        int64_t t = line - 2 * B;
        col = t >= (int64_t)B * K;
        if (col) t -= (int64_t)B * K;
        const int b = (int)(t / K);
        idx = (int)(t % K);
        R = K;
        L = ws.logits + (int64_t)B * B + (int64_t)b * K * K;
    }
    const int64_t s0 = col ? idx : (int64_t)idx * R, st = col ? R : 1;
    float mx = -__builtin_huge_valf();
    for (int j = lane; j < R; j += 64) mx = fmaxf(mx, L[s0 + j * st]);
    mx = wave_max(mx);
    float se = 0.0f;
    for (int j = lane; j < R; j += 64) se += expf(L[s0 + j * st] - mx);
    se = wave_sum(se);
    if (lane == 0) {
        ws.lse[line] = make_float2(mx, logf(se));
        ws.ce[line] = (double)mx + log((double)se) - (double)L[(int64_t)idx * R + idx];
    }
}

// ---- forward finalize ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bsign(const Args& a, int64_t e) {
    // sign((c_i lambda + t_i (1 - lambda)) + (c_t lambda + t_t (1 - lambda))) on the detached codes, op for op (MITH.py:178-180):
    // every product rounded on its own (no contraction into an fma), so that c_t = -c_i, t_t = -t_i gives exactly 0, as in torch
#pragma clang fp contract(off)
    const float lam = a.lambda, mu = a.mu;
    const float u = (a.ci[e] * lam + a.ti[e] * mu) + (a.ct[e] * lam + a.tt[e] * mu);
    return u > 0.0f ? 1.0f : (u < 0.0f ? -1.0f : 0.0f);
}

__global__ __launch_bounds__(kThreads) void k_mith_finalize(Args a, WsView ws, LikGrid g, double* __restrict__ out10) {
    __shared__ double sh[kWaves];
    const int B = a.B, K = a.K;
    double lik[4] = {0.0, 0.0, 0.0, 0.0};
    const int nblk = g.P * g.ctiles;
    for (int r = threadIdx.x; r < nblk; r += kThreads)
        for (int q = 0; q < 4; ++q) lik[q] += ws.lik[(int64_t)r * 4 + q];
    double ce[4] = {0.0, 0.0, 0.0, 0.0};      // cls rows, cls cols, token rows, token cols
    for (int r = threadIdx.x; r < B; r += kThreads) {
        ce[0] += ws.ce[r];
        ce[1] += ws.ce[B + r];
    }
    const int64_t BK = (int64_t)B * K;
    for (int64_t r = threadIdx.x; r < BK; r += kThreads) {
        ce[2] += ws.ce[2 * B + r];
        ce[3] += ws.ce[2 * B + BK + r];
    }
    double qd[4] = {0.0, 0.0, 0.0, 0.0};      // sum (H_i - Bs)^2, (H_t - Bs)^2, (c_i - t_i)^2, (c_t - t_t)^2
    for (int64_t e = threadIdx.x; e < BK; e += kThreads) {
        const float bs = bsign(a, e);
        const float hi = 0.5f * a.ci[e] + 0.5f * a.ti[e], ht = 0.5f * a.ct[e] + 0.5f * a.tt[e];
        const double di = (double)hi - bs, dt = (double)ht - bs, xi = (double)a.ci[e] - a.ti[e], xt = (double)a.ct[e] - a.tt[e];
        qd[0] += di * di;
        qd[1] += dt * dt;
        qd[2] += xi * xi;
        qd[3] += xt * xt;
    }
    for (int q = 0; q < 4; ++q) {
        lik[q] = xmh::block_sum<kWaves>(lik[q], sh);
        ce[q] = xmh::block_sum<kWaves>(ce[q], sh);
        qd[q] = xmh::block_sum<kWaves>(qd[q], sh);
    }
    if (threadIdx.x == 0) {
        const double nb = (double)a.N * (double)B, bk = (double)BK;
        const double intra_i = -lik[0] / nb, intra_t = -lik[1] / nb, i2t = -lik[2] / nb, t2i = -lik[3] / nb;
        const double quan_i = qd[0] / bk, quan_t = qd[1] / bk;
        const double nce_cls = 0.5 * (ce[0] / B + ce[1] / B), nce_tok = 0.5 * (ce[2] / bk + ce[3] / bk);
        const double distill = a.w_distill * (1.1 * (qd[2] + qd[3])) / B;
        out10[0] = a.w_intra * (intra_i + intra_t) + a.w_inter * (i2t + t2i) + a.w_quan * (quan_i + quan_t) +
                   a.w_nce * (nce_cls + a.alpha * nce_tok) + distill;
        out10[1] = intra_i;
        out10[2] = intra_t;
        out10[3] = i2t;
        out10[4] = t2i;
        out10[5] = quan_i;
        out10[6] = quan_t;
        out10[7] = nce_cls;
        out10[8] = nce_tok;
        out10[9] = distill;
    }
}

// ---- gradient ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void store(float* p, float v, int accumulate) { *p = accumulate ? *p + v : v; }

// Blocks [0, nce_blocks): for each problem (cls, then the B token problems) and each of its two outputs, 64 x 64 tiles of
// dA = G B_m / tau (rows i, columns d) and dB = G^T A / tau; the remaining blocks: the [B, K] code gradients, one element per thread.
__global__ __launch_bounds__(kThreads) void k_mith_grad(Args a, WsView ws, LikGrid g, Grads gr, const float* __restrict__ up,
                                                        int accumulate, int nce_blocks) {
    __shared__ __attribute__((aligned(16))) float As[kKc][kLd];
    __shared__ __attribute__((aligned(16))) float Bs[kKc][kLd];
    const int B = a.B, K = a.K, D = a.D;
    const float u = up ? up[0] : 1.0f;
    if ((int)blockIdx.x < nce_blocks) {
        const int tc = (B + kTile - 1) / kTile, tk = (K + kTile - 1) / kTile, td = (D + kTile - 1) / kTile;
        int blk = blockIdx.x, p, nt;
        if (blk < 2 * tc * td) {
            p = 0;
            nt = tc;
        } else {
            blk -= 2 * tc * td;
            p = 1 + blk / (2 * tk * td);
            blk %= 2 * tk * td;
            nt = tk;
        }
        const bool second = blk >= nt * td;                   // d / d(text side)
        if (second) blk -= nt * td;
        float *ga = nullptr, *gb = nullptr;
        const Problem q = problem(a, ws, p, true, gr.g, &ga, &gb);
        float* out = second ? gb : ga;
        if (!out) return;
        const int m0 = (blk / td) * kTile, n0 = (blk % td) * kTile;
        const int64_t lines = (int64_t)(p == 0 ? B : B * K);
        const float coef = (float)(0.5 / (double)lines);
        const float2* lr = ws.lse + q.line;
        const float2* lc = ws.lse + q.line + q.cstride;
        float acc[4][4];
        zero(acc);
        if (!second) {
            const NceG<false> G{q.L, lr, lc, q.R, coef};
            const Strided Bt{q.Bm, 1, q.rs, D, q.R};          // element (d, j) = B_m[j][d]
            mm_tile<true, false>(acc, G, Bt, m0, n0, q.R, As, Bs);
        } else {
            const NceG<true> G{q.L, lr, lc, q.R, coef};
            const Strided At{q.A, 1, q.rs, D, q.R};           // element (d, i) = A[i][d]
            mm_tile<false, false>(acc, G, At, m0, n0, q.R, As, Bs);
        }
        const float w = (float)(p == 0 ? a.w_nce : a.w_nce * a.alpha) * u;
        const int tm = threadIdx.x & 15, tn = threadIdx.x >> 4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = m0 + tm * 4 + i, d = n0 + tn * 4 + j;
                if (r < q.R && d < D) store(out + (int64_t)r * q.rs + d, w * (acc[i][j] / a.tau), accumulate);
            }
        return;
    }
    const int64_t e = (int64_t)(blockIdx.x - nce_blocks) * kThreads + threadIdx.x;
    const int64_t BK = (int64_t)B * K;
    if (e >= BK) return;
    const int b = (int)(e / K), k = (int)(e % K);
    float lg[4] = {0.0f, 0.0f, 0.0f, 0.0f};                  // likelihood gradients of t_i, t_t, c_t, c_i: chunks in order
    for (int p = 0; p < g.P; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) lg[q] += ws.gpart[((int64_t)p * 4 * B + (int64_t)q * B + b) * K + k];
    const float ci = a.ci[e], ct = a.ct[e], ti = a.ti[e], tt = a.tt[e];
    const float bs = bsign(a, e);
    const float qc = (float)(a.w_quan / (double)BK);                    // d/dx of w_q sum (0.5 c + 0.5 t - Bs)^2 / (B K) = w_q (H - Bs) / (B K)
    const float dhi = qc * (0.5f * ci + 0.5f * ti - bs), dht = qc * (0.5f * ct + 0.5f * tt - bs);
    const float dc = (float)(2.0 * a.w_distill / B);          // w_d (sum (c' - t)^2 + 0.1 sum (c - t')^2) / B
    const float wi = (float)a.w_intra, wc = (float)a.w_inter;
    const float vals[4] = {wi * lg[0] + dhi + dc * (ti - ci),          // tokens_hash_i
                           wi * lg[1] + dht + dc * (tt - ct),          // tokens_hash_t
                           wc * lg[2] + dht + 0.1f * dc * (ct - tt),   // txt_cls_hash
                           wc * lg[3] + dhi + 0.1f * dc * (ci - ti)};  // img_cls_hash
    float* const dst[4] = {gr.g[4], gr.g[5], gr.g[3], gr.g[2]};
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (dst[q]) store(dst[q] + e, u * vals[q], accumulate);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
int check_args(const char* who, const xmh_mith_loss_args* p, void* ws, size_t ws_bytes) {
    if (!p) return xmh::fail(XMH_EINVAL, "%s: null pointer (args)", who);
    if (p->N <= 0 || p->B <= 0 || p->K <= 0 || p->D <= 0)
        return xmh::fail(XMH_EINVAL, "%s: bad shape N=%lld B=%d K=%d D=%d", who, (long long)p->N, p->B, p->K, p->D);
    if (p->N > kMaxN || p->B > kMaxB || p->K > kMaxK || p->D > kMaxD)
        return xmh::fail(XMH_ENOTSUP, "%s: N=%lld B=%d K=%d D=%d outside N <= %lld, B <= %d, K <= %d, D <= %d", who, (long long)p->N, p->B,
                         p->K, p->D, (long long)kMaxN, kMaxB, kMaxK, kMaxD);
    if (!p->res_img_cls || !p->res_txt_cls || !p->img_cls_hash || !p->txt_cls_hash || !p->tokens_hash_i || !p->tokens_hash_t ||
        !p->trans_tokens_i || !p->trans_tokens_t || !p->buffer || !p->label_sim || !ws)
        return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    const size_t need = ws_layout(p->N, p->B, p->K, nullptr, nullptr);
    if (ws_bytes < need) return xmh::fail(XMH_EINVAL, "%s: workspace of %zu bytes < %zu (xmh_mith_loss_ws_bytes)", who, ws_bytes, need);
    if (reinterpret_cast<uintptr_t>(ws) & 255u) return xmh::fail(XMH_EINVAL, "%s: workspace not 256-byte aligned", who);
    return XMH_OK;
}

Args device_args(const xmh_mith_loss_args* p) {
    return Args{p->N, p->B, p->K, p->D, p->res_img_cls, p->res_txt_cls, p->img_cls_hash, p->txt_cls_hash, p->tokens_hash_i,
                p->tokens_hash_t, p->trans_tokens_i, p->trans_tokens_t, p->buffer, p->label_sim, p->hyper_tokens_intra,
                p->hyper_distill, p->hyper_info_nce, p->hyper_cls_inter, p->hyper_quan, p->hyper_alpha, (float)p->hyper_lambda,
                (float)(1.0 - p->hyper_lambda), (float)p->temperature};
}

void launch_lik(bool grad, const Args& a, const WsView& v, const LikGrid& g, hipStream_t st) {
    const dim3 grid((unsigned)g.ctiles, (unsigned)g.P);
    if (!grad) {                                           // the forward keeps no gradient accumulators: one instance
        hipLaunchKernelGGL((k_mith_lik<false, 1>), grid, dim3(kThreads), 0, st, a, v, g);
        return;
    }
    switch ((a.K + kTile - 1) / kTile) {                   // KT = 64-column slices of K held in registers
        case 1: hipLaunchKernelGGL((k_mith_lik<true, 1>), grid, dim3(kThreads), 0, st, a, v, g); break;
        case 2: hipLaunchKernelGGL((k_mith_lik<true, 2>), grid, dim3(kThreads), 0, st, a, v, g); break;
        case 3: hipLaunchKernelGGL((k_mith_lik<true, 3>), grid, dim3(kThreads), 0, st, a, v, g); break;
        default: hipLaunchKernelGGL((k_mith_lik<true, 4>), grid, dim3(kThreads), 0, st, a, v, g); break;
    }
}

void launch_nce(const Args& a, const WsView& v, hipStream_t st) {
    const int tc = (a.B + kTile - 1) / kTile, tk = (a.K + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_mith_nce_logits, dim3((unsigned)(tc * tc + a.B * tk * tk)), dim3(kThreads), 0, st, a, v);
    const int64_t lines = 2 * (int64_t)a.B + 2 * (int64_t)a.B * a.K;
    hipLaunchKernelGGL(k_mith_nce_lse, dim3((unsigned)((lines + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, a, v);
}

}  // namespace

extern "C" size_t xmh_mith_loss_ws_bytes(int64_t N, int B, int K, int D) {
    if (N <= 0 || B <= 0 || K <= 0 || D <= 0 || N > kMaxN || B > kMaxB || K > kMaxK || D > kMaxD) return 0;
    return ws_layout(N, B, K, nullptr, nullptr);
}

extern "C" int xmh_mith_loss(const xmh_mith_loss_args* args, void* ws, size_t ws_bytes, double* out10, xmh_stream_t stream) {
    XMH_RANGE("xmh_mith_loss");
    if (int rc = check_args("xmh_mith_loss", args, ws, ws_bytes)) return rc;
    if (!out10) return xmh::fail(XMH_EINVAL, "xmh_mith_loss: null pointer (out10)");
    const Args a = device_args(args);
    WsView v;
    ws_layout(a.N, a.B, a.K, ws, &v);
    const LikGrid g = lik_grid(a.N, a.B);
    hipStream_t st = xmh::as_stream(stream);
    launch_lik(false, a, v, g, st);
    launch_nce(a, v, st);
    hipLaunchKernelGGL(k_mith_finalize, dim3(1), dim3(kThreads), 0, st, a, v, g, out10);
    XMH_LAUNCH_CHECK("xmh_mith_loss");
    return XMH_OK;
}

extern "C" int xmh_mith_loss_grad(const xmh_mith_loss_args* args, const float* upstream, float* const* grads, int accumulate, void* ws,
                                  size_t ws_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_mith_loss_grad");
    if (int rc = check_args("xmh_mith_loss_grad", args, ws, ws_bytes)) return rc;
    if (!grads) return xmh::fail(XMH_EINVAL, "xmh_mith_loss_grad: null pointer (grads)");
    const Args a = device_args(args);
    Grads gr;
    bool any = false, any_code = false, any_nce = false;
    for (int i = 0; i < 8; ++i) {
        gr.g[i] = grads[i];
        any = any || grads[i];
        if (grads[i] && i >= 2 && i < 6) any_code = true;
        if (grads[i] && (i < 2 || i >= 6)) any_nce = true;
    }
    if (!any) return XMH_OK;
    WsView v;
    ws_layout(a.N, a.B, a.K, ws, &v);
    const LikGrid g = lik_grid(a.N, a.B);
    hipStream_t st = xmh::as_stream(stream);
    if (any_code) launch_lik(true, a, v, g, st);
    if (any_nce) launch_nce(a, v, st);
    const int tc = (a.B + kTile - 1) / kTile, tk = (a.K + kTile - 1) / kTile, td = (a.D + kTile - 1) / kTile;
    const int nce_blocks = any_nce ? 2 * tc * td + a.B * 2 * tk * td : 0;
    const int code_blocks = any_code ? (int)(((int64_t)a.B * a.K + kThreads - 1) / kThreads) : 0;
    hipLaunchKernelGGL(k_mith_grad, dim3((unsigned)(nce_blocks + code_blocks)), dim3(kThreads), 0, st, a, v, g, gr, upstream, accumulate,
                       nce_blocks);
    XMH_LAUNCH_CHECK("xmh_mith_loss_grad");
    return XMH_OK;
}
