// Train-mode forward and backward of the two small hash heads.
//
//   DCMHT  models/DCMHT/hash/hash.py:15-46   v = x Wv^T + bv, o = v Wo^T + bo (MultiheadAttention on a length-1 sequence), BatchNorm1d
//          with BATCH statistics (image) or LayerNorm (text) -> nhat, n = nhat gamma + beta, f = relu(n W2^T + b2), pair softmax
//   DSPH   models/DSPH/hash/hash.py:6-15     y = tanh(keep * (x W^T + b) / (1 - p)), the keep mask handed in by the caller
//
//   forward   DCMHT 4 launches: k_mm<NT> (v), k_mm<NT> (o), k_bn_train | k_ln_train, k_mm<NT> with the relu + pair-softmax epilogue
//             DSPH  1 launch:   k_mm<NT> with the dropout + tanh epilogue
//   backward  DCMHT k_pair_relu_bwd (df), k_mm<TN> (dW2, db2), k_mm<NN> (dn), k_norm_bwd_cols (dgamma, dbeta; BatchNorm: do as well),
//             k_ln_bwd_rows (LayerNorm: do), k_mm<TN> (dWo, dbo), k_mm<NN> (dv), k_mm<TN> (dWv, dbv), k_mm<NN> (dx): 8 (BN) / 9 (LN)
//             launches with every gradient asked for, fewer with frozen parameters (a product nobody reads is not launched)
//             DSPH  k_tanh_drop_bwd (dz), k_mm<TN> (dW, db), k_mm<NN> (dx): 3 launches
//
// One product kernel, C[i][j] = sum_k A(i, k) B(j, k) over strided views, covers y = x W^T ("NT"), dx = dy W ("NN") and dW = dy^T x ("TN",
// the reduction runs over the batch: no alignment assumption, B = 1 works).  Exact fp32: every output element is a chain of fmaf over each 32 consecutive k,
// the 32-blocks added in index order -- one fixed order, so two calls agree to the bit and forward and backward see the same numbers.  The bias gradients
// (column sums of dy) ride on the TN kernel's pass over dy, summed in double in row order.  No float atomics, no host synchronisation, no
// allocation.  The relu mask of backward is the sign of the f that forward stored: nothing is evaluated twice.
// Shapes are small (B <= 1024, E = 512, N <= 512 in practice): launch- and latency-bound, a few hundred KB of L2-resident operands.
#include "xmh_common.h"
#include "xmh_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxB = 4096, kMaxE = 2048, kMaxN = 1024;
constexpr int kT = 32;                           // product tile: 32 x 32 outputs per block, 32 k per LDS stage, 2 x 2 outputs per thread
constexpr int kPad = kT + 1;
constexpr int kCols = 32, kGroups = kThreads / kCols;   // column kernels: 32 adjacent columns x 8 interleaved row groups per block

using xmh::group_sum;

// what forward keeps for backward (DCMHT)
struct Saved {
    float* v;      // [B, E]
    float* nhat;   // [B, E] normalised activations before the affine
    float* n;      // [B, E] after it (the operand of dW2 = df^T n)
    float* rstd;   // [E] (BatchNorm, per column) or [B] (LayerNorm, per row)
    float* f;      // [B, N] relu output: its sign is the mask
    float* p;      // [B, N] probabilities
};

__host__ __device__ inline size_t saved_layout(int64_t B, int E, int N, void* base, Saved* s) {
    xmh::Arena ar(base);
    Saved v;
    v.v = ar.take<float>((size_t)B * E);
    v.nhat = ar.take<float>((size_t)B * E);
    v.n = ar.take<float>((size_t)B * E);
    v.rstd = ar.take<float>((size_t)(B > E ? B : E));
    v.f = ar.take<float>((size_t)B * N);
    v.p = ar.take<float>((size_t)B * N);
    if (s) *s = v;
    return ar.used;
}

// workspace: a [B, E] (o in forward; dn, then do in place, in backward), b [B, E] (dv), c [B, N] (df)
struct Work {
    float *a, *b, *c;
};

__host__ __device__ inline size_t work_layout(int64_t B, int E, int N, void* base, Work* w) {
    xmh::Arena ar(base);
    Work v;
    v.a = ar.take<float>((size_t)B * E);
    v.b = ar.take<float>((size_t)B * E);
    v.c = ar.take<float>((size_t)B * N);
    if (w) *w = v;
    return ar.used;
}

enum { EPI_PLAIN = 0, EPI_RELU_PAIR = 1, EPI_DROP_TANH = 2 };

struct MmOut {
    float* C;                 // [I, J] row-major
    const float* bias;        // [J] added to every row, or NULL
    int accumulate;           // C += instead of C = (EPI_PLAIN), rowsum alike
    float* rowsum;            // [I]: sum_k A(i, k) in double, k in index order (the bias gradient of the TN product), or NULL
    int epi;
    float* aux;               // EPI_RELU_PAIR: the probabilities' second copy (saved); C receives the probabilities, f the relu output
    float* f;
    const uint8_t* keep;      // EPI_DROP_TANH: [I, J] keep mask or NULL
    float scale;              // 1 / (1 - p)
};

// C[i][j] = sum_k A[i * sai + k * sak] * B[j * sbj + k * sbk].  AK / BK: k is the unit-stride index of that operand (decides which
// index the lanes of a load walk; the arithmetic does not depend on it).
// SUM: also rowsum[i] = sum_k A(i, k) (only the TN instance that owes a bias gradient is compiled with it).
template <bool AK, bool BK, bool SUM>
__global__ __launch_bounds__(kThreads) void k_mm(const float* __restrict__ A, int64_t sai, int64_t sak, const float* __restrict__ Bm,
                                                 int64_t sbj, int64_t sbk, int I, int J, int Kd, MmOut o) {
    __shared__ float As[kT][kPad];               // [k][i]
    __shared__ float Bs[kT][kPad];               // [k][j]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * kT, j0 = blockIdx.x * kT;
    const int lo = tid & 31, hi = tid >> 5;      // a load: 32 lanes along the unit-stride index, 8 steps along the other, 4 rounds
    float ra[4], rb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ai = AK ? hi + 8 * r : lo, ak = AK ? lo : hi + 8 * r;
            const int bj = BK ? hi + 8 * r : lo, bk = BK ? lo : hi + 8 * r;
            ra[r] = (i0 + ai < I && k0 + ak < Kd) ? A[(int64_t)(i0 + ai) * sai + (int64_t)(k0 + ak) * sak] : 0.0f;
            rb[r] = (j0 + bj < J && k0 + bk < Kd) ? Bm[(int64_t)(j0 + bj) * sbj + (int64_t)(k0 + bk) * sbk] : 0.0f;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ai = AK ? hi + 8 * r : lo, ak = AK ? lo : hi + 8 * r;
            const int bj = BK ? hi + 8 * r : lo, bk = BK ? lo : hi + 8 * r;
            As[ak][ai] = ra[r];
            Bs[bk][bj] = rb[r];
        }
    };
    float c00 = 0.0f, c01 = 0.0f, c10 = 0.0f, c11 = 0.0f;
    double s0 = 0.0, s1 = 0.0;
    const bool sums = SUM && blockIdx.x == 0 && tx == 0;
    fetch(0);
    for (int k0 = 0; k0 < Kd; k0 += kT) {
        stash();
        __syncthreads();
        if (k0 + kT < Kd) fetch(k0 + kT);        // the next stage's loads fly over this stage's arithmetic
        float p00 = 0.0f, p01 = 0.0f, p10 = 0.0f, p11 = 0.0f;
#pragma unroll
        for (int k = 0; k < kT; ++k) {           // zero padding past Kd: fmaf(0, 0, p) == p
            const float a0 = As[k][2 * ty], a1 = As[k][2 * ty + 1], b0 = Bs[k][2 * tx], b1 = Bs[k][2 * tx + 1];
            p00 = fmaf(a0, b0, p00);
            p01 = fmaf(a0, b1, p01);
            p10 = fmaf(a1, b0, p10);
            p11 = fmaf(a1, b1, p11);
            if (SUM) {
                if (sums) {
                    s0 += (double)a0;
                    s1 += (double)a1;
                }
            }
        }
        c00 += p00;                              // two-level sum: a 32-term chain per stage, the stages in order -- the rounding
        c01 += p01;                              // error of a 512-term dot product grows with sqrt(32) + sqrt(16), not sqrt(512)
        c10 += p10;
        c11 += p11;
        __syncthreads();
    }
    const int j = j0 + 2 * tx;
    const float acc[2][2] = {{c00, c01}, {c10, c11}};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = i0 + 2 * ty + r;
        if (i >= I) continue;
        if (sums) {
            const float s = (float)(r ? s1 : s0);
            o.rowsum[i] = o.accumulate ? o.rowsum[i] + s : s;
        }
        if (j >= J) continue;
        const bool two = j + 1 < J;
        float z0 = acc[r][0], z1 = acc[r][1];
        if (o.bias) {
            z0 += o.bias[j];
            if (two) z1 += o.bias[j + 1];
        }
        float* c = o.C + (int64_t)i * J + j;
        if (o.epi == EPI_PLAIN) {
            c[0] = o.accumulate ? c[0] + z0 : z0;
            if (two) c[1] = o.accumulate ? c[1] + z1 : z1;
        } else if (o.epi == EPI_RELU_PAIR) {     // J is even (checked by the entry point) and j is: (j, j + 1) is one (off, on) pair
            const float f0 = fmaxf(z0, 0.0f), f1 = fmaxf(z1, 0.0f), m = fmaxf(f0, f1);
            const float e0 = expf(f0 - m), e1 = expf(f1 - m), inv = 1.0f / (e0 + e1);
            const int64_t at = (int64_t)i * J + j;
            o.f[at] = f0;
            o.f[at + 1] = f1;
            c[0] = o.aux[at] = e0 * inv;
            c[1] = o.aux[at + 1] = e1 * inv;
        } else {                                 // EPI_DROP_TANH
            const int64_t at = (int64_t)i * J + j;
            if (o.keep) {
                z0 = o.keep[at] ? z0 * o.scale : 0.0f;
                if (two) z1 = o.keep[at + 1] ? z1 * o.scale : 0.0f;
            }
            c[0] = tanhf(z0);
            if (two) c[1] = tanhf(z1);
        }
    }
}

// BatchNorm1d in training mode over o [B, E]: batch mean and BIASED variance (two passes, double), nhat, n, rstd per column, and the
// running statistics updated in place with `momentum` and the UNBIASED variance (either pointer may be NULL: track_running_stats=False)
__global__ __launch_bounds__(kThreads) void k_bn_train(const float* __restrict__ o, int B, int E, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float eps, float momentum, float* run_mean,
                                                       float* run_var, Saved s) {
    __shared__ double sh[kGroups][kCols];
    const int col = threadIdx.x % kCols, grp = threadIdx.x / kCols, e = blockIdx.x * kCols + col;
    const bool live = e < E;
    double a = 0.0;
    if (live)
        for (int b = grp; b < B; b += kGroups) a += (double)o[(int64_t)b * E + e];
    const double mean = group_sum(a, sh, col, grp) / (double)B;
    a = 0.0;
    if (live)
        for (int b = grp; b < B; b += kGroups) {
            const double d = (double)o[(int64_t)b * E + e] - mean;
            a += d * d;
        }
    const double m2 = group_sum(a, sh, col, grp);
    if (!live) return;
    const float var = (float)(m2 / (double)B), fmean = (float)mean;
    const float rstd = 1.0f / sqrtf(var + eps);
    const float g = gamma[e], bt = beta[e];
    for (int b = grp; b < B; b += kGroups) {
        const int64_t at = (int64_t)b * E + e;
        const float nh = (o[at] - fmean) * rstd;
        s.nhat[at] = nh;
        s.n[at] = fmaf(nh, g, bt);
    }
    if (grp == 0) {
        s.rstd[e] = rstd;
        if (run_mean) run_mean[e] = (1.0f - momentum) * run_mean[e] + momentum * fmean;
        if (run_var) run_var[e] = (1.0f - momentum) * run_var[e] + momentum * (float)(m2 / (double)(B - 1));
    }
}

using xmh::wave_sum;

// LayerNorm over the rows of o [B, E] (fp32 in, statistics in double, biased variance): one wave per row
__global__ __launch_bounds__(kThreads) void k_ln_train(const float* __restrict__ o, int B, int E, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float eps, Saved s) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (b >= B) return;
    const float* row = o + (int64_t)b * E;
    double a = 0.0;
    for (int e = lane; e < E; e += 64) a += (double)row[e];
    const double mean = wave_sum(a) / (double)E;
    a = 0.0;
    for (int e = lane; e < E; e += 64) {
        const double d = (double)row[e] - mean;
        a += d * d;
    }
    const float var = (float)(wave_sum(a) / (double)E), fmean = (float)mean;
    const float rstd = 1.0f / sqrtf(var + eps);
    for (int e = lane; e < E; e += 64) {
        const float nh = (row[e] - fmean) * rstd;
        s.nhat[(int64_t)b * E + e] = nh;
        s.n[(int64_t)b * E + e] = fmaf(nh, gamma[e], beta[e]);
    }
    if (lane == 0) s.rstd[b] = rstd;
}

// df from d probs: pair-softmax backward dz_a = p_a (g_a - p_a g_a - p_b g_b), then the relu mask of the f forward stored
__global__ __launch_bounds__(kThreads) void k_pair_relu_bwd(const float* __restrict__ g, const float* __restrict__ p,
                                                            const float* __restrict__ f, int64_t pairs, float* __restrict__ df) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= pairs) return;
    const float g0 = g[2 * q], g1 = g[2 * q + 1], p0 = p[2 * q], p1 = p[2 * q + 1];
    const float dot = fmaf(p1, g1, p0 * g0);
    df[2 * q] = f[2 * q] > 0.0f ? p0 * (g0 - dot) : 0.0f;
    df[2 * q + 1] = f[2 * q + 1] > 0.0f ? p1 * (g1 - dot) : 0.0f;
}

// dz = g (1 - y^2) keep / (1 - p)
__global__ __launch_bounds__(kThreads) void k_tanh_drop_bwd(const float* __restrict__ g, const float* __restrict__ y,
                                                            const uint8_t* __restrict__ keep, float scale, int64_t n,
                                                            float* __restrict__ dz) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float yy = y[i];
    float d = g[i] * fmaf(-yy, yy, 1.0f);
    if (keep) d = keep[i] ? d * scale : 0.0f;
    dz[i] = d;
}

// Column sums of the normalisation's backward: dgamma[e] = sum_b dn nhat, dbeta[e] = sum_b dn (double, fixed order; written or added
// to; either may be NULL).  kBN: also do = gamma rstd (dn - mean(dn) - nhat mean(dn nhat)), in place over dn.
template <bool kBN>
__global__ __launch_bounds__(kThreads) void k_norm_bwd_cols(float* dn, const float* __restrict__ nhat, int B, int E,
                                                            const float* __restrict__ gamma, const float* __restrict__ rstd,
                                                            float* dgamma, float* dbeta, int accumulate) {
    __shared__ double sh[kGroups][kCols];
    const int col = threadIdx.x % kCols, grp = threadIdx.x / kCols, e = blockIdx.x * kCols + col;
    const bool live = e < E;
    double a = 0.0, c = 0.0;
    if (live)
        for (int b = grp; b < B; b += kGroups) {
            const float d = dn[(int64_t)b * E + e];
            a += (double)d * (double)nhat[(int64_t)b * E + e];
            c += (double)d;
        }
    const double sg = group_sum(a, sh, col, grp), sb = group_sum(c, sh, col, grp);
    if (!live) return;
    if (grp == 0) {
        if (dgamma) dgamma[e] = accumulate ? dgamma[e] + (float)sg : (float)sg;
        if (dbeta) dbeta[e] = accumulate ? dbeta[e] + (float)sb : (float)sb;
    }
    if (kBN) {
        const float mg = (float)(sg / (double)B), mb = (float)(sb / (double)B), w = gamma[e] * rstd[e];
        for (int b = grp; b < B; b += kGroups) {
            const int64_t at = (int64_t)b * E + e;
            dn[at] = w * (dn[at] - mb - nhat[at] * mg);
        }
    }
}

// LayerNorm backward over one row (one wave): h = dn gamma, do = rstd (h - mean(h) - nhat mean(h nhat)), in place over dn
__global__ __launch_bounds__(kThreads) void k_ln_bwd_rows(float* dn, const float* __restrict__ nhat, int B, int E,
                                                          const float* __restrict__ gamma, const float* __restrict__ rstd) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (b >= B) return;
    float* row = dn + (int64_t)b * E;
    const float* nh = nhat + (int64_t)b * E;
    double a = 0.0, c = 0.0;
    for (int e = lane; e < E; e += 64) {
        const float h = row[e] * gamma[e];
        a += (double)h;
        c += (double)h * (double)nh[e];
    }
    const float mh = (float)(wave_sum(a) / (double)E), mc = (float)(wave_sum(c) / (double)E), r = rstd[b];
    for (int e = lane; e < E; e += 64) row[e] = r * (row[e] * gamma[e] - mh - nh[e] * mc);
}

// y [M, N] = x [M, K] w[N, K]^T (+ bias, epilogue)
void launch_nt(hipStream_t st, const float* x, const float* w, int M, int N, int K, MmOut o) {
    hipLaunchKernelGGL((k_mm<true, true, false>), dim3((N + kT - 1) / kT, (M + kT - 1) / kT), dim3(kThreads), 0, st, x, (int64_t)K, (int64_t)1, w,
                       (int64_t)K, (int64_t)1, M, N, K, o);
}

// dx [M, K] = dy [M, N] w [N, K]
void launch_nn(hipStream_t st, const float* dy, const float* w, int M, int N, int K, float* dx) {
    MmOut o = {};
    o.C = dx;
    hipLaunchKernelGGL((k_mm<true, false, false>), dim3((K + kT - 1) / kT, (M + kT - 1) / kT), dim3(kThreads), 0, st, dy, (int64_t)N, (int64_t)1, w,
                       (int64_t)1, (int64_t)K, M, K, N, o);
}

// dw [N, K] = dy [M, N]^T x [M, K] and, when db is not NULL, db [N] = column sums of dy from the same pass (weight_grads picks the route)
void launch_tn(hipStream_t st, const float* dy, const float* x, int M, int N, int K, float* dw, float* db, int accumulate) {
    MmOut o = {};
    o.C = dw;
    o.rowsum = db;
    o.accumulate = accumulate;
    const dim3 grid((K + kT - 1) / kT, (N + kT - 1) / kT);
    if (db)
        hipLaunchKernelGGL((k_mm<false, false, true>), grid, dim3(kThreads), 0, st, dy, (int64_t)1, (int64_t)N, x, (int64_t)1, (int64_t)K, N,
                           K, M, o);
    else
        hipLaunchKernelGGL((k_mm<false, false, false>), grid, dim3(kThreads), 0, st, dy, (int64_t)1, (int64_t)N, x, (int64_t)1, (int64_t)K, N,
                           K, M, o);
}

// ---- cross-rank BatchNorm: the column statistics of k_bn_train and k_norm_bwd_cols<true> split from their use, so that
// the ranks of a distributed step can exchange them in between.  A statistics row is kStatsRow(E) doubles: [E] [E] count 0.
__host__ __device__ constexpr int64_t kStatsRow(int E) { return 2 * (int64_t)E + 2; }

// forward, first half: per column the LOCAL mean and M2 = sum (o - mean)^2, the two passes of k_bn_train, and the local row count
__global__ __launch_bounds__(kThreads) void k_bn_stats(const float* __restrict__ o, int B, int E, double* __restrict__ row) {
    __shared__ double sh[kGroups][kCols];
    const int col = threadIdx.x % kCols, grp = threadIdx.x / kCols, e = blockIdx.x * kCols + col;
    const bool live = e < E;
    double a = 0.0;
    if (live)
        for (int b = grp; b < B; b += kGroups) a += (double)o[(int64_t)b * E + e];
    const double mean = group_sum(a, sh, col, grp) / (double)B;
    a = 0.0;
    if (live)
        for (int b = grp; b < B; b += kGroups) {
            const double d = (double)o[(int64_t)b * E + e] - mean;
            a += d * d;
        }
    const double m2 = group_sum(a, sh, col, grp);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        row[2 * (int64_t)E] = (double)B;
        row[2 * (int64_t)E + 1] = 0.0;
    }
    if (!live || grp != 0) return;
    row[e] = mean;
    row[E + e] = m2;
}

// forward, second half: the rows of all W ranks combined IN RANK ORDER by the pairwise update (n, mean, M2) + (n_r, mean_r, M2_r) -- the
// same chain of double operations in every thread of every rank, so all of them derive the same bits -- then k_bn_train's use of
// them on this rank's rows: global mean and BIASED variance, the running statistics towards the global mean and the UNBIASED global
// variance (n_total - 1).  One rank: the chain is empty and the numbers are k_bn_train's to the bit.
__global__ __launch_bounds__(kThreads) void k_bn_apply(const float* __restrict__ o, int B, int E, const double* __restrict__ table, int W,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                       float momentum, float* run_mean, float* run_var, Saved s) {
    const int col = threadIdx.x % kCols, grp = threadIdx.x / kCols, e = blockIdx.x * kCols + col;
    if (e >= E) return;
    const int64_t stride = kStatsRow(E);
    double n = table[2 * (int64_t)E], mean = table[e], m2 = table[E + e];
    for (int r = 1; r < W; ++r) {
        const double* row = table + r * stride;
        const double nr = row[2 * (int64_t)E];
        if (!(nr > 0.0)) continue;
        const double delta = row[e] - mean, nn = n + nr;
        mean += delta * (nr / nn);
        m2 += row[E + e] + delta * delta * (n * nr / nn);
        n = nn;
    }
    const float var = (float)(m2 / n), fmean = (float)mean;
    const float rstd = 1.0f / sqrtf(var + eps);
    const float g = gamma[e], bt = beta[e];
    for (int b = grp; b < B; b += kGroups) {
        const int64_t at = (int64_t)b * E + e;
        const float nh = (o[at] - fmean) * rstd;
        s.nhat[at] = nh;
        s.n[at] = fmaf(nh, g, bt);
    }
    if (grp == 0) {
        s.rstd[e] = rstd;
        if (run_mean) run_mean[e] = (1.0f - momentum) * run_mean[e] + momentum * fmean;
        if (run_var) run_var[e] = (1.0f - momentum) * run_var[e] + momentum * (float)(m2 / (n - 1.0));
    }
}

// backward, first half: the LOCAL column sums of k_norm_bwd_cols, sum_b dn nhat and sum_b dn, and the local row count
__global__ __launch_bounds__(kThreads) void k_bn_bwd_stats(const float* __restrict__ dn, const float* __restrict__ nhat, int B, int E,
                                                           double* __restrict__ row) {
    __shared__ double sh[kGroups][kCols];
    const int col = threadIdx.x % kCols, grp = threadIdx.x / kCols, e = blockIdx.x * kCols + col;
    const bool live = e < E;
    double a = 0.0, c = 0.0;
    if (live)
        for (int b = grp; b < B; b += kGroups) {
            const float d = dn[(int64_t)b * E + e];
            a += (double)d * (double)nhat[(int64_t)b * E + e];
            c += (double)d;
        }
    const double sg = group_sum(a, sh, col, grp), sb = group_sum(c, sh, col, grp);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        row[2 * (int64_t)E] = (double)B;
        row[2 * (int64_t)E + 1] = 0.0;
    }
    if (!live || grp != 0) return;
    row[e] = sg;
    row[E + e] = sb;
}

// backward, second half: dgamma / dbeta from THIS rank's sums (the gradient all-reduce averages them like every other gradient), the
// sums of all ranks added in rank order, do = gamma rstd (dn - mean(dn) - nhat mean(dn nhat)) with the means over n_total, in place
__global__ __launch_bounds__(kThreads) void k_bn_bwd_apply(float* dn, const float* __restrict__ nhat, int B, int E,
                                                           const double* __restrict__ table, int W, int rank,
                                                           const float* __restrict__ gamma, const float* __restrict__ rstd, float* dgamma,
                                                           float* dbeta, int accumulate) {
    const int col = threadIdx.x % kCols, grp = threadIdx.x / kCols, e = blockIdx.x * kCols + col;
    if (e >= E) return;
    const int64_t stride = kStatsRow(E);
    if (grp == 0) {
        const double* own = table + rank * stride;
        if (dgamma) dgamma[e] = accumulate ? dgamma[e] + (float)own[e] : (float)own[e];
        if (dbeta) dbeta[e] = accumulate ? dbeta[e] + (float)own[E + e] : (float)own[E + e];
    }
    double sg = table[e], sb = table[E + e], n = table[2 * (int64_t)E];
    for (int r = 1; r < W; ++r) {
        const double* row = table + r * stride;
        sg += row[e];
        sb += row[E + e];
        n += row[2 * (int64_t)E];
    }
    const float mg = (float)(sg / n), mb = (float)(sb / n), w = gamma[e] * rstd[e];
    for (int b = grp; b < B; b += kGroups) {
        const int64_t at = (int64_t)b * E + e;
        dn[at] = w * (dn[at] - mb - nhat[at] * mg);
    }
}

// bias gradient alone (its weight is frozen): column sums of dy [M, N] in double, row order
__global__ __launch_bounds__(kThreads) void k_col_sum(const float* __restrict__ dy, int M, int N, float* db, int accumulate) {
    __shared__ double sh[kGroups][kCols];
    const int col = threadIdx.x % kCols, grp = threadIdx.x / kCols, e = blockIdx.x * kCols + col;
    double a = 0.0;
    if (e < N)
        for (int b = grp; b < M; b += kGroups) a += (double)dy[(int64_t)b * N + e];
    const double s = group_sum(a, sh, col, grp);
    if (e < N && grp == 0) db[e] = accumulate ? db[e] + (float)s : (float)s;
}

void weight_grads(hipStream_t st, const float* dy, const float* x, int M, int N, int K, float* dw, float* db, int accumulate) {
    if (dw)
        launch_tn(st, dy, x, M, N, K, dw, db, accumulate);
    else if (db)
        hipLaunchKernelGGL(k_col_sum, dim3((N + kCols - 1) / kCols), dim3(kThreads), 0, st, dy, M, N, db, accumulate);
}

int check_shape(const char* who, int64_t B, int E, int N) {
    if (B <= 0 || E <= 0 || N <= 0) return xmh::fail(XMH_EINVAL, "%s: bad shape B=%lld E=%d N=%d", who, (long long)B, E, N);
    if (B > kMaxB || E > kMaxE || N > kMaxN)
        return xmh::fail(XMH_ENOTSUP, "%s: B=%lld E=%d N=%d outside B <= %d, E <= %d, N <= %d", who, (long long)B, E, N, kMaxB, kMaxE, kMaxN);
    return XMH_OK;
}

int check_buffer(const char* who, const char* what, const void* p, size_t have, size_t need) {
    if (!p) return xmh::fail(XMH_EINVAL, "%s: null %s", who, what);
    if (have < need) return xmh::fail(XMH_EINVAL, "%s: %s of %zu bytes < %zu (xmh_head_dcmht_train_bytes)", who, what, have, need);
    if (reinterpret_cast<uintptr_t>(p) & 255u) return xmh::fail(XMH_EINVAL, "%s: %s not 256-byte aligned", who, what);
    return XMH_OK;
}

int check_dcmht(const char* who, const xmh_dcmht_train* h, const float* x, int64_t B, int E, int N) {
    if (int rc = check_shape(who, B, E, N)) return rc;
    if (N & 1) return xmh::fail(XMH_EINVAL, "%s: N=%d is odd (N = 2K, one (off, on) pair per bit)", who, N);
    if (!h || !x || !h->wv || !h->bv || !h->wo || !h->bo || !h->norm_w || !h->norm_b || !h->w2 || !h->b2)
        return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    return XMH_OK;
}

}  // namespace

extern "C" size_t xmh_head_dcmht_train_bytes(int64_t B, int E, int N, size_t* workspace_bytes) {
    const bool ok = B > 0 && E > 0 && N > 0 && !(N & 1) && B <= kMaxB && E <= kMaxE && N <= kMaxN;
    if (workspace_bytes) *workspace_bytes = ok ? work_layout(B, E, N, nullptr, nullptr) : 0;
    return ok ? saved_layout(B, E, N, nullptr, nullptr) : 0;
}

extern "C" int xmh_head_dcmht_train_forward(const xmh_dcmht_train* h, const float* x, int64_t B, int E, int N, float* probs, void* saved,
                                            size_t saved_bytes, void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_head_dcmht_train_forward");
    const char* who = "xmh_head_dcmht_train_forward";
    if (int rc = check_dcmht(who, h, x, B, E, N)) return rc;
    if (!probs) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (h->norm_is_batchnorm && B < 2) return xmh::fail(XMH_EINVAL, "%s: BatchNorm in training mode needs more than 1 row", who);
    if (int rc = check_buffer(who, "saved buffer", saved, saved_bytes, saved_layout(B, E, N, nullptr, nullptr))) return rc;
    if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, work_layout(B, E, N, nullptr, nullptr))) return rc;
    Saved s;
    Work w;
    saved_layout(B, E, N, saved, &s);
    work_layout(B, E, N, workspace, &w);
    hipStream_t st = xmh::as_stream(stream);
    MmOut o = {};
    o.C = s.v;
    o.bias = h->bv;
    launch_nt(st, x, h->wv, (int)B, E, E, o);
    o.C = w.a;
    o.bias = h->bo;
    launch_nt(st, s.v, h->wo, (int)B, E, E, o);
    if (h->norm_is_batchnorm)
        hipLaunchKernelGGL(k_bn_train, dim3((E + kCols - 1) / kCols), dim3(kThreads), 0, st, w.a, (int)B, E, h->norm_w, h->norm_b, h->eps,
                           h->momentum, h->running_mean, h->running_var, s);
    else
        hipLaunchKernelGGL(k_ln_train, dim3((unsigned)((B + 3) / 4)), dim3(kThreads), 0, st, w.a, (int)B, E, h->norm_w, h->norm_b, h->eps, s);
    o.C = probs;
    o.bias = h->b2;
    o.epi = EPI_RELU_PAIR;
    o.aux = s.p;
    o.f = s.f;
    launch_nt(st, s.n, h->w2, (int)B, N, E, o);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

extern "C" int xmh_head_dcmht_backward(const xmh_dcmht_train* h, const float* x, const float* d_probs, int64_t B, int E, int N,
                                       const void* saved, size_t saved_bytes, const xmh_dcmht_grads* g, int accumulate, void* workspace,
                                       size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_head_dcmht_backward");
    const char* who = "xmh_head_dcmht_backward";
    if (int rc = check_dcmht(who, h, x, B, E, N)) return rc;
    if (!d_probs || !g) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (int rc = check_buffer(who, "saved buffer", saved, saved_bytes, saved_layout(B, E, N, nullptr, nullptr))) return rc;
    if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, work_layout(B, E, N, nullptr, nullptr))) return rc;
    Saved s;
    Work w;
    saved_layout(B, E, N, const_cast<void*>(saved), &s);
    work_layout(B, E, N, workspace, &w);
    hipStream_t st = xmh::as_stream(stream);
    const int M = (int)B;
    // what has to exist for the gradients asked for: each stage is needed by everything upstream of it
    const bool need_dv = g->d_wv || g->d_bv || g->d_x;
    const bool need_do = need_dv || g->d_wo || g->d_bo;
    const bool need_dn = need_do || g->d_norm_w || g->d_norm_b;
    if (!need_dn && !g->d_w2 && !g->d_b2) return XMH_OK;
    const int64_t pairs = B * (N / 2);
    hipLaunchKernelGGL(k_pair_relu_bwd, dim3((unsigned)((pairs + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_probs, s.p, s.f, pairs,
                       w.c);
    weight_grads(st, w.c, s.n, M, N, E, g->d_w2, g->d_b2, accumulate);
    if (need_dn) {
        launch_nn(st, w.c, h->w2, M, N, E, w.a);                                  // dn
        if (h->norm_is_batchnorm) {
            hipLaunchKernelGGL(k_norm_bwd_cols<true>, dim3((E + kCols - 1) / kCols), dim3(kThreads), 0, st, w.a, s.nhat, M, E, h->norm_w,
                               s.rstd, g->d_norm_w, g->d_norm_b, accumulate);
        } else {
            if (g->d_norm_w || g->d_norm_b)
                hipLaunchKernelGGL(k_norm_bwd_cols<false>, dim3((E + kCols - 1) / kCols), dim3(kThreads), 0, st, w.a, s.nhat, M, E,
                                   h->norm_w, s.rstd, g->d_norm_w, g->d_norm_b, accumulate);
            if (need_do)
                hipLaunchKernelGGL(k_ln_bwd_rows, dim3((unsigned)((B + 3) / 4)), dim3(kThreads), 0, st, w.a, s.nhat, M, E, h->norm_w, s.rstd);
        }
    }
    if (need_do) weight_grads(st, w.a, s.v, M, E, E, g->d_wo, g->d_bo, accumulate);
    if (need_dv) {
        launch_nn(st, w.a, h->wo, M, E, E, w.b);                                  // dv
        weight_grads(st, w.b, x, M, E, E, g->d_wv, g->d_bv, accumulate);
        if (g->d_x) launch_nn(st, w.b, h->wv, M, E, E, g->d_x);               // an activation gradient: written, never added to
    }
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

// ---- the same head with a cross-rank BatchNorm: each of the two calls above in two halves, the caller's all-gather of the statistics
// rows in between.  The workspace carries o (forward) / dn and df (backward) from the first half to the second: the caller keeps it.
namespace {

int check_sync(const char* who, const xmh_dcmht_train* h, const float* x, int64_t B, int E, int N, const void* saved, size_t saved_bytes,
               void* workspace, size_t workspace_bytes, const double* stats) {
    if (int rc = check_dcmht(who, h, x, B, E, N)) return rc;
    if (!h->norm_is_batchnorm) return xmh::fail(XMH_EINVAL, "%s: the head's norm is a LayerNorm (rows need no other rank)", who);
    if (!stats) return xmh::fail(XMH_EINVAL, "%s: null statistics", who);
    if (reinterpret_cast<uintptr_t>(stats) & 7u) return xmh::fail(XMH_EINVAL, "%s: statistics not 8-byte aligned", who);
    if (int rc = check_buffer(who, "saved buffer", saved, saved_bytes, saved_layout(B, E, N, nullptr, nullptr))) return rc;
    return check_buffer(who, "workspace", workspace, workspace_bytes, work_layout(B, E, N, nullptr, nullptr));
}

int check_world(const char* who, int64_t B, int world, int rank) {
    if (world < 1 || world > 4096 || rank < 0 || rank >= world) return xmh::fail(XMH_EINVAL, "%s: rank %d of %d", who, rank, world);
    // every rank has at least one row, so the global batch is a single row only when this rank is alone with one
    if (world == 1 && B < 2) return xmh::fail(XMH_EINVAL, "%s: BatchNorm in training mode needs more than 1 row over all ranks", who);
    return XMH_OK;
}

}  // namespace

extern "C" int64_t xmh_head_dcmht_stats_len(int E) { return E > 0 && E <= kMaxE ? kStatsRow(E) : 0; }

extern "C" int xmh_head_dcmht_train_forward_stats(const xmh_dcmht_train* h, const float* x, int64_t B, int E, int N, void* saved,
                                                  size_t saved_bytes, void* workspace, size_t workspace_bytes, double* stats_row,
                                                  xmh_stream_t stream) {
    XMH_RANGE("xmh_head_dcmht_train_forward_stats");
    const char* who = "xmh_head_dcmht_train_forward_stats";
    if (int rc = check_sync(who, h, x, B, E, N, saved, saved_bytes, workspace, workspace_bytes, stats_row)) return rc;
    Saved s;
    Work w;
    saved_layout(B, E, N, saved, &s);
    work_layout(B, E, N, workspace, &w);
    hipStream_t st = xmh::as_stream(stream);
    MmOut o = {};
    o.C = s.v;
    o.bias = h->bv;
    launch_nt(st, x, h->wv, (int)B, E, E, o);
    o.C = w.a;
    o.bias = h->bo;
    launch_nt(st, s.v, h->wo, (int)B, E, E, o);
    hipLaunchKernelGGL(k_bn_stats, dim3((E + kCols - 1) / kCols), dim3(kThreads), 0, st, w.a, (int)B, E, stats_row);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

extern "C" int xmh_head_dcmht_train_forward_apply(const xmh_dcmht_train* h, const float* x, int64_t B, int E, int N, const double* table,
                                                  int world, float* probs, void* saved, size_t saved_bytes, void* workspace,
                                                  size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_head_dcmht_train_forward_apply");
    const char* who = "xmh_head_dcmht_train_forward_apply";
    if (int rc = check_sync(who, h, x, B, E, N, saved, saved_bytes, workspace, workspace_bytes, table)) return rc;
    if (!probs) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (int rc = check_world(who, B, world, 0)) return rc;
    Saved s;
    Work w;
    saved_layout(B, E, N, saved, &s);
    work_layout(B, E, N, workspace, &w);
    hipStream_t st = xmh::as_stream(stream);
    hipLaunchKernelGGL(k_bn_apply, dim3((E + kCols - 1) / kCols), dim3(kThreads), 0, st, w.a, (int)B, E, table, world, h->norm_w, h->norm_b,
                       h->eps, h->momentum, h->running_mean, h->running_var, s);
    MmOut o = {};
    o.C = probs;
    o.bias = h->b2;
    o.epi = EPI_RELU_PAIR;
    o.aux = s.p;
    o.f = s.f;
    launch_nt(st, s.n, h->w2, (int)B, N, E, o);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

extern "C" int xmh_head_dcmht_backward_stats(const xmh_dcmht_train* h, const float* x, const float* d_probs, int64_t B, int E, int N,
                                             const void* saved, size_t saved_bytes, const xmh_dcmht_grads* g, int accumulate,
                                             void* workspace, size_t workspace_bytes, double* stats_row, xmh_stream_t stream) {
    XMH_RANGE("xmh_head_dcmht_backward_stats");
    const char* who = "xmh_head_dcmht_backward_stats";
    if (int rc = check_sync(who, h, x, B, E, N, saved, saved_bytes, workspace, workspace_bytes, stats_row)) return rc;
    if (!d_probs || !g) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    Saved s;
    Work w;
    saved_layout(B, E, N, const_cast<void*>(saved), &s);
    work_layout(B, E, N, workspace, &w);
    hipStream_t st = xmh::as_stream(stream);
    const int M = (int)B;
    const int64_t pairs = B * (N / 2);
    // dn and its sums are formed whatever is frozen: the other ranks wait for this rank's row
    hipLaunchKernelGGL(k_pair_relu_bwd, dim3((unsigned)((pairs + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_probs, s.p, s.f, pairs,
                       w.c);
    weight_grads(st, w.c, s.n, M, N, E, g->d_w2, g->d_b2, accumulate);
    launch_nn(st, w.c, h->w2, M, N, E, w.a);                                      // dn
    hipLaunchKernelGGL(k_bn_bwd_stats, dim3((E + kCols - 1) / kCols), dim3(kThreads), 0, st, w.a, s.nhat, M, E, stats_row);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

extern "C" int xmh_head_dcmht_backward_apply(const xmh_dcmht_train* h, const float* x, int64_t B, int E, int N, const double* table, int world,
                                             int rank, const void* saved, size_t saved_bytes, const xmh_dcmht_grads* g, int accumulate,
                                             void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_head_dcmht_backward_apply");
    const char* who = "xmh_head_dcmht_backward_apply";
    if (int rc = check_sync(who, h, x, B, E, N, saved, saved_bytes, workspace, workspace_bytes, table)) return rc;
    if (!g) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (int rc = check_world(who, B, world, rank)) return rc;
    Saved s;
    Work w;
    saved_layout(B, E, N, const_cast<void*>(saved), &s);
    work_layout(B, E, N, workspace, &w);
    hipStream_t st = xmh::as_stream(stream);
    const int M = (int)B;
    const bool need_dv = g->d_wv || g->d_bv || g->d_x;
    const bool need_do = need_dv || g->d_wo || g->d_bo;
    if (!need_do && !g->d_norm_w && !g->d_norm_b) return XMH_OK;
    hipLaunchKernelGGL(k_bn_bwd_apply, dim3((E + kCols - 1) / kCols), dim3(kThreads), 0, st, w.a, s.nhat, M, E, table, world, rank, h->norm_w,
                       s.rstd, g->d_norm_w, g->d_norm_b, accumulate);
    if (need_do) weight_grads(st, w.a, s.v, M, E, E, g->d_wo, g->d_bo, accumulate);
    if (need_dv) {
        launch_nn(st, w.a, h->wo, M, E, E, w.b);                                  // dv
        weight_grads(st, w.b, x, M, E, E, g->d_wv, g->d_bv, accumulate);
        if (g->d_x) launch_nn(st, w.b, h->wv, M, E, E, g->d_x);
    }
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

extern "C" int xmh_head_dsph_train_forward(const float* w, const float* b, const float* x, const uint8_t* keep, float p, int64_t B, int E,
                                           int K, float* y, xmh_stream_t stream) {
    XMH_RANGE("xmh_head_dsph_train_forward");
    const char* who = "xmh_head_dsph_train_forward";
    if (int rc = check_shape(who, B, E, K)) return rc;
    if (!w || !b || !x || !y) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (!(p >= 0.0f && p < 1.0f)) return xmh::fail(XMH_EINVAL, "%s: dropout p=%g outside [0, 1)", who, (double)p);
    MmOut o = {};
    o.C = y;
    o.bias = b;
    o.epi = EPI_DROP_TANH;
    o.keep = keep;
    o.scale = 1.0f / (1.0f - p);
    launch_nt(xmh::as_stream(stream), x, w, (int)B, K, E, o);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

extern "C" int xmh_head_dsph_backward(const float* w, const float* x, const float* y, const uint8_t* keep, float p, const float* d_y,
                                      int64_t B, int E, int K, float* d_w, float* d_b, float* d_x, int accumulate, void* workspace,
                                      size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_head_dsph_backward");
    const char* who = "xmh_head_dsph_backward";
    if (int rc = check_shape(who, B, E, K)) return rc;
    if (!w || !x || !y || !d_y) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (!(p >= 0.0f && p < 1.0f)) return xmh::fail(XMH_EINVAL, "%s: dropout p=%g outside [0, 1)", who, (double)p);
    if (!workspace) return xmh::fail(XMH_EINVAL, "%s: null workspace", who);
    if (workspace_bytes < (size_t)B * K * 4) return xmh::fail(XMH_EINVAL, "%s: workspace of %zu bytes < %zu (4 B K)", who, workspace_bytes, (size_t)B * K * 4);
    if (!d_w && !d_b && !d_x) return XMH_OK;
    hipStream_t st = xmh::as_stream(stream);
    float* dz = static_cast<float*>(workspace);
    const int64_t n = B * K;
    hipLaunchKernelGGL(k_tanh_drop_bwd, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_y, y, keep, 1.0f / (1.0f - p),
                       n, dz);
    weight_grads(st, dz, x, (int)B, K, E, d_w, d_b, accumulate);
    if (d_x) launch_nn(st, dz, w, (int)B, K, E, d_x);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

// A plain linear layer y = x w^T + b behind autograd (DNPH's class-prediction layers): d_w = d_y^T x with d_b from the same pass,
// d_x = d_y w, the products of the heads above.  Nothing is staged, so no workspace is needed: the two arguments are there for the
// calling convention of the other backward entries and a NULL / 0 pair is accepted; a non-NULL one must be 256-byte aligned.
extern "C" int xmh_linear_backward(const float* w, const float* x, const float* d_y, int64_t B, int E, int N, float* d_w, float* d_b, float* d_x,
                                   int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_linear_backward");
    const char* who = "xmh_linear_backward";
    if (int rc = check_shape(who, B, E, N)) return rc;
    if (!w || !x || !d_y) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (workspace && (reinterpret_cast<uintptr_t>(workspace) & 255u)) return xmh::fail(XMH_EINVAL, "%s: workspace not 256-byte aligned", who);
    if (!workspace && workspace_bytes) return xmh::fail(XMH_EINVAL, "%s: %zu workspace bytes at a null pointer", who, workspace_bytes);
    if (!d_w && !d_b && !d_x) return XMH_OK;
    hipStream_t st = xmh::as_stream(stream);
    weight_grads(st, d_y, x, (int)B, N, E, d_w, d_b, accumulate);
    if (d_x) launch_nn(st, d_y, w, (int)B, N, E, d_x);                             // an activation gradient: written, never added to
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

// ---- DIMCH token-set head (reference models/DIMCH/hash/hash.py:18-52) ---------------------------------------------------
//   tokens [B, T, E] -> c = relu(Conv1d(T -> M, kernel 3, padding 1) along E)  [B M, E]
//                    -> a = dropout(relu(c W1^T + b1))                          [B M, H]
//                    -> embeds = a W2^T + b2                                    [B, M, K]
//                    -> pooled = mean over the M set members, hash = tanh(pooled) or the pair softmax of it   [B, K]
//   forward   5 launches: k_dimch_conv, k_mm<NT>, k_dimch_relu_drop, k_mm<NT>, k_dimch_pool  (inference and train mode are the same
//             launches: inference keeps c and a in its workspace, train mode in the saved buffer, so eval == train at p = 0 to the bit)
//   backward  9 launches with every gradient asked for: k_dimch_pool_bwd (d embeds + d hash through the pooling), k_mm<TN> (dW2, db2),
//             k_mm<NN> (da), k_dimch_mask (dropout scale and relu mask), k_mm<TN> (dW1, db1), k_mm<NN> (dc), k_dimch_mask (relu mask),
//             k_dimch_conv_wgrad (dWc, dbc), k_dimch_conv_xgrad (d tokens)
// The convolution sums over t in index order, its three taps in order, one fmaf chain per output; its weight gradient sums in double,
// each thread over a strided subset of (b, e) and the 256 partial sums by a fixed tree.  No atomics: two calls agree to the bit.
namespace {

constexpr int kDimchMaxRows = 512 * 64, kDimchMaxT = 256, kDimchMaxK = 256;
constexpr int kConvM = 8;                        // set members per thread of k_dimch_conv: one load of the token row feeds 8 outputs

struct DimchSaved {
    float* c;        // [B M, E] relu output of the convolution
    float* a;        // [B M, H] relu output of the first linear layer, after the dropout
    float* pooled;   // [B, K] mean over the set, before tanh / softmax
};

size_t dimch_saved_layout(int64_t B, int E, int H, int M, int K, void* base, DimchSaved* s) {
    xmh::Arena ar(base);
    DimchSaved v;
    v.c = ar.take<float>((size_t)B * M * E);
    v.a = ar.take<float>((size_t)B * M * H);
    v.pooled = ar.take<float>((size_t)B * K);
    if (s) *s = v;
    return ar.used;
}

struct DimchWork {
    float *ge, *ga, *gc;   // d embeds [B M, K], d a [B M, H], d c [B M, E]
};

size_t dimch_work_layout(int64_t B, int E, int H, int M, int K, void* base, DimchWork* w) {
    xmh::Arena ar(base);
    DimchWork v;
    v.ge = ar.take<float>((size_t)B * M * K);
    v.ga = ar.take<float>((size_t)B * M * H);
    v.gc = ar.take<float>((size_t)B * M * E);
    if (w) *w = v;
    return ar.used;
}

// grid (ceil(E / 256), ceil(M / kConvM), B): thread = one column e of kConvM set members
__global__ __launch_bounds__(kThreads) void k_dimch_conv(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         int T, int E, int M, float* __restrict__ c) {
    const int e = blockIdx.x * kThreads + threadIdx.x, m0 = blockIdx.y * kConvM, b = blockIdx.z;
    if (e >= E) return;
    float acc[kConvM];
#pragma unroll
    for (int i = 0; i < kConvM; ++i) acc[i] = 0.0f;
    const float* xb = x + (int64_t)b * T * E;
    for (int t = 0; t < T; ++t) {
        const float* r = xb + (int64_t)t * E;
        const float xl = e > 0 ? r[e - 1] : 0.0f, xc = r[e], xr = e + 1 < E ? r[e + 1] : 0.0f;
#pragma unroll
        for (int i = 0; i < kConvM; ++i) {
            if (m0 + i < M) {
                const float* wt = w + ((int64_t)(m0 + i) * T + t) * 3;
                acc[i] = fmaf(wt[2], xr, fmaf(wt[1], xc, fmaf(wt[0], xl, acc[i])));
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kConvM; ++i)
        if (m0 + i < M) {
            const float z = acc[i] + bias[m0 + i];
            c[((int64_t)b * M + m0 + i) * E + e] = z > 0.0f ? z : (z != z ? z : 0.0f);      // relu that lets a NaN through
        }
}

// a = relu(a), then the dropout: a * scale where keep, 0 elsewhere (keep NULL: no dropout)
__global__ __launch_bounds__(kThreads) void k_dimch_relu_drop(float* a, const uint8_t* __restrict__ keep, float scale, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    float z = a[i];
    z = z > 0.0f ? z : (z != z ? z : 0.0f);
    if (keep) z = keep[i] ? z * scale : 0.0f;
    a[i] = z;
}

__device__ inline void dimch_pair(const float* pooled, int64_t row, int k, float* p0, float* p1) {
    const float z0 = pooled[row + (k & ~1)], z1 = pooled[row + (k | 1)], m = fmaxf(z0, z1);
    const float e0 = expf(z0 - m), e1 = expf(z1 - m), inv = 1.0f / (e0 + e1);
    *p0 = e0 * inv;
    *p1 = e1 * inv;
}

// thread = one (b, k): the mean over the M set members in index order, then tanh or the pair softmax over (2j, 2j + 1)
__global__ __launch_bounds__(kThreads) void k_dimch_pool(const float* __restrict__ embeds, int64_t B, int M, int K, int softmax,
                                                         float* pooled, float* __restrict__ hash) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= B * K) return;
    const int64_t b = i / K;
    const int k = (int)(i - b * K);
    auto mean = [&](int kk) {
        float s = 0.0f;
        for (int m = 0; m < M; ++m) s += embeds[(b * M + m) * K + kk];
        return s / (float)M;
    };
    const float z = mean(k);
    pooled[i] = z;
    if (!softmax) {
        hash[i] = tanhf(z);
    } else {
        const float zo = mean(k ^ 1), mx = fmaxf(z, zo);      // the partner of the pair, summed in the same order as its own thread does
        const float ez = expf(z - mx), eo = expf(zo - mx);
        const float e0 = (k & 1) ? eo : ez, e1 = (k & 1) ? ez : eo, inv = 1.0f / (e0 + e1);
        hash[i] = ((k & 1) ? e1 : e0) * inv;
    }
}

// ge [b, m, k] = d_embeds [b, m, k] + d pooled [b, k] / M, d pooled from d_hash through tanh or the pair softmax; either may be NULL
__global__ __launch_bounds__(kThreads) void k_dimch_pool_bwd(const float* __restrict__ d_embeds, const float* __restrict__ d_hash,
                                                             const float* __restrict__ pooled, int64_t B, int M, int K, int softmax,
                                                             float* __restrict__ ge) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= B * M * K) return;
    const int k = (int)(i % K);
    const int64_t b = i / ((int64_t)M * K), row = b * K;
    float g = d_embeds ? d_embeds[i] : 0.0f;
    if (d_hash) {
        float dz;
        if (!softmax) {
            const float h = tanhf(pooled[row + k]);
            dz = d_hash[row + k] * (1.0f - h * h);
        } else {
            float p0, p1;
            dimch_pair(pooled, row, k, &p0, &p1);
            const float g0 = d_hash[row + (k & ~1)], g1 = d_hash[row + (k | 1)], dot = g0 * p0 + g1 * p1;
            dz = (k & 1) ? p1 * (g1 - dot) : p0 * (g0 - dot);
        }
        g += dz / (float)M;
    }
    ge[i] = g;
}

// g = act > 0 ? g * scale : 0 in place (the relu mask is the sign of the stored output; after the dropout a dropped element is 0 too)
__global__ __launch_bounds__(kThreads) void k_dimch_mask(float* g, const float* __restrict__ act, float scale, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    g[i] = act[i] > 0.0f ? g[i] * scale : 0.0f;
}

// grid (T + 1, M): block (t, m) owns dWc [m, t, 0..2]; block (T, m) owns dbc [m].  Sums over (b, e) in double.
__global__ __launch_bounds__(kThreads) void k_dimch_conv_wgrad(const float* __restrict__ gc, const float* __restrict__ x, int64_t B, int T, int E,
                                                               int M, float* dw, float* db, int accumulate) {
    __shared__ double sh[3][kThreads];
    const int t = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;
    if (t == T ? !db : !dw) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const int64_t n = B * E;
    for (int64_t i = tid; i < n; i += kThreads) {
        const int64_t b = i / E;
        const int e = (int)(i - b * E);
        const double g = (double)gc[(b * M + m) * E + e];
        if (t == T) {
            s0 += g;
        } else {
            const float* r = x + (b * T + t) * E;
            if (e > 0) s0 += g * (double)r[e - 1];
            s1 += g * (double)r[e];
            if (e + 1 < E) s2 += g * (double)r[e + 1];
        }
    }
    sh[0][tid] = s0;
    sh[1][tid] = s1;
    sh[2][tid] = s2;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if (tid < h) {
            sh[0][tid] += sh[0][tid + h];
            sh[1][tid] += sh[1][tid + h];
            sh[2][tid] += sh[2][tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (t == T) {
            db[m] = accumulate ? db[m] + (float)sh[0][0] : (float)sh[0][0];
        } else {
            float* o = dw + ((int64_t)m * T + t) * 3;
            for (int k = 0; k < 3; ++k) o[k] = accumulate ? o[k] + (float)sh[k][0] : (float)sh[k][0];
        }
    }
}

// grid (ceil(E / 256), T, B): d tokens [b, t, e] = sum_m sum_k Wc [m, t, k] gc [b, m, e - k + 1], m in index order
__global__ __launch_bounds__(kThreads) void k_dimch_conv_xgrad(const float* __restrict__ gc, const float* __restrict__ w, int T, int E, int M,
                                                               float* __restrict__ dx) {
    const int e = blockIdx.x * kThreads + threadIdx.x, t = blockIdx.y, b = blockIdx.z;
    if (e >= E) return;
    float acc = 0.0f;
    for (int m = 0; m < M; ++m) {
        const float* g = gc + ((int64_t)b * M + m) * E;
        const float* wt = w + ((int64_t)m * T + t) * 3;
        const float gr = e + 1 < E ? g[e + 1] : 0.0f, gm = g[e], gl = e > 0 ? g[e - 1] : 0.0f;
        acc = fmaf(wt[2], gl, fmaf(wt[1], gm, fmaf(wt[0], gr, acc)));
    }
    dx[((int64_t)b * T + t) * E + e] = acc;
}

bool dimch_shape_ok(int64_t B, int T, int E, int H, int M, int K) {
    return B > 0 && T > 0 && E > 0 && H > 0 && M > 0 && K > 0 && B <= 65535 && B * M <= kDimchMaxRows && T <= kDimchMaxT && E <= kMaxE &&
           H <= kMaxE && K <= kDimchMaxK;
}

int check_dimch(const char* who, const xmh_dimch_head* h, const float* tokens, int64_t B) {
    if (!h || !tokens || !h->conv_w || !h->conv_b || !h->w1 || !h->b1 || !h->w2 || !h->b2) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (B <= 0 || h->T <= 0 || h->E <= 0 || h->H <= 0 || h->M <= 0 || h->K <= 0)
        return xmh::fail(XMH_EINVAL, "%s: bad shape B=%lld T=%d E=%d H=%d M=%d K=%d", who, (long long)B, h->T, h->E, h->H, h->M, h->K);
    if (h->hash_func != XMH_DIMCH_TANH && h->hash_func != XMH_DIMCH_SOFTMAX) return xmh::fail(XMH_EINVAL, "%s: hash_func=%d", who, h->hash_func);
    if (h->hash_func == XMH_DIMCH_SOFTMAX && (h->K & 1)) return xmh::fail(XMH_EINVAL, "%s: K=%d is odd (one (off, on) pair per bit)", who, h->K);
    if (!dimch_shape_ok(B, h->T, h->E, h->H, h->M, h->K))
        return xmh::fail(XMH_ENOTSUP, "%s: B=%lld T=%d E=%d H=%d M=%d K=%d outside B M <= %d, T <= %d, E, H <= %d, K <= %d", who, (long long)B,
                         h->T, h->E, h->H, h->M, h->K, kDimchMaxRows, kDimchMaxT, kMaxE, kDimchMaxK);
    return XMH_OK;
}

int dimch_forward(const char* who, const xmh_dimch_head* h, const float* tokens, const uint8_t* keep, float p, int64_t B, float* embeds,
                  float* hash, void* saved, size_t saved_bytes, xmh_stream_t stream) {
    if (int rc = check_dimch(who, h, tokens, B)) return rc;
    if (!embeds || !hash) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (!(p >= 0.0f && p < 1.0f)) return xmh::fail(XMH_EINVAL, "%s: dropout p=%g outside [0, 1)", who, (double)p);
    if (int rc = check_buffer(who, "buffer", saved, saved_bytes, dimch_saved_layout(B, h->E, h->H, h->M, h->K, nullptr, nullptr))) return rc;
    DimchSaved s;
    dimch_saved_layout(B, h->E, h->H, h->M, h->K, saved, &s);
    hipStream_t st = xmh::as_stream(stream);
    const int rows = (int)(B * h->M);
    hipLaunchKernelGGL(k_dimch_conv, dim3((h->E + kThreads - 1) / kThreads, (h->M + kConvM - 1) / kConvM, (unsigned)B), dim3(kThreads), 0, st,
                       tokens, h->conv_w, h->conv_b, h->T, h->E, h->M, s.c);
    MmOut o = {};
    o.C = s.a;
    o.bias = h->b1;
    launch_nt(st, s.c, h->w1, rows, h->H, h->E, o);
    const int64_t n = (int64_t)rows * h->H;
    hipLaunchKernelGGL(k_dimch_relu_drop, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, s.a, keep, 1.0f / (1.0f - p), n);
    o.C = embeds;
    o.bias = h->b2;
    launch_nt(st, s.a, h->w2, rows, h->K, h->H, o);
    hipLaunchKernelGGL(k_dimch_pool, dim3((unsigned)((B * h->K + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, embeds, B, h->M, h->K,
                       h->hash_func == XMH_DIMCH_SOFTMAX, s.pooled, hash);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

}  // namespace

extern "C" size_t xmh_head_dimch_bytes(int64_t B, int T, int E, int H, int M, int K, size_t* workspace_bytes) {
    const bool ok = dimch_shape_ok(B, T, E, H, M, K);
    if (workspace_bytes) *workspace_bytes = ok ? dimch_work_layout(B, E, H, M, K, nullptr, nullptr) : 0;
    return ok ? dimch_saved_layout(B, E, H, M, K, nullptr, nullptr) : 0;
}

extern "C" int xmh_head_dimch(const xmh_dimch_head* h, const float* tokens, int64_t B, float* embeds, float* hash, void* workspace,
                              size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_head_dimch");
    return dimch_forward("xmh_head_dimch", h, tokens, nullptr, 0.0f, B, embeds, hash, workspace, workspace_bytes, stream);
}

extern "C" int xmh_head_dimch_train_forward(const xmh_dimch_head* h, const float* tokens, const uint8_t* keep, float p, int64_t B,
                                            float* embeds, float* hash, void* saved, size_t saved_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_head_dimch_train_forward");
    return dimch_forward("xmh_head_dimch_train_forward", h, tokens, keep, keep ? p : 0.0f, B, embeds, hash, saved, saved_bytes, stream);
}

extern "C" int xmh_head_dimch_backward(const xmh_dimch_head* h, const float* tokens, int has_keep, float p, const float* d_embeds,
                                       const float* d_hash, int64_t B, const void* saved, size_t saved_bytes, const xmh_dimch_head_grads* g,
                                       int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_head_dimch_backward");
    const char* who = "xmh_head_dimch_backward";
    if (int rc = check_dimch(who, h, tokens, B)) return rc;
    if (!g) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (!(p >= 0.0f && p < 1.0f)) return xmh::fail(XMH_EINVAL, "%s: dropout p=%g outside [0, 1)", who, (double)p);
    const int E = h->E, H = h->H, M = h->M, K = h->K, T = h->T;
    if (int rc = check_buffer(who, "saved buffer", saved, saved_bytes, dimch_saved_layout(B, E, H, M, K, nullptr, nullptr))) return rc;
    if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, dimch_work_layout(B, E, H, M, K, nullptr, nullptr))) return rc;
    const bool need_c = g->d_conv_w || g->d_conv_b || g->d_tokens;
    const bool need_a = need_c || g->d_w1 || g->d_b1;
    if ((!d_embeds && !d_hash) || (!need_a && !g->d_w2 && !g->d_b2)) return XMH_OK;
    DimchSaved s;
    DimchWork w;
    dimch_saved_layout(B, E, H, M, K, const_cast<void*>(saved), &s);
    dimch_work_layout(B, E, H, M, K, workspace, &w);
    hipStream_t st = xmh::as_stream(stream);
    const int rows = (int)(B * M);
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); };
    hipLaunchKernelGGL(k_dimch_pool_bwd, blocks((int64_t)rows * K), dim3(kThreads), 0, st, d_embeds, d_hash, s.pooled, B, M, K,
                       h->hash_func == XMH_DIMCH_SOFTMAX, w.ge);
    weight_grads(st, w.ge, s.a, rows, K, H, g->d_w2, g->d_b2, accumulate);
    if (need_a) {
        launch_nn(st, w.ge, h->w2, rows, K, H, w.ga);
        hipLaunchKernelGGL(k_dimch_mask, blocks((int64_t)rows * H), dim3(kThreads), 0, st, w.ga, s.a, has_keep ? 1.0f / (1.0f - p) : 1.0f,
                           (int64_t)rows * H);
        weight_grads(st, w.ga, s.c, rows, H, E, g->d_w1, g->d_b1, accumulate);
    }
    if (need_c) {
        launch_nn(st, w.ga, h->w1, rows, H, E, w.gc);
        hipLaunchKernelGGL(k_dimch_mask, blocks((int64_t)rows * E), dim3(kThreads), 0, st, w.gc, s.c, 1.0f, (int64_t)rows * E);
        if (g->d_conv_w || g->d_conv_b)
            hipLaunchKernelGGL(k_dimch_conv_wgrad, dim3(T + 1, M), dim3(kThreads), 0, st, w.gc, tokens, B, T, E, M, g->d_conv_w, g->d_conv_b,
                               accumulate);
        if (g->d_tokens)
            hipLaunchKernelGGL(k_dimch_conv_xgrad, dim3((E + kThreads - 1) / kThreads, T, (unsigned)B), dim3(kThreads), 0, st, w.gc, h->conv_w, T, E,
                               M, g->d_tokens);
    }
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}
