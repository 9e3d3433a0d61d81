// UMoED: the soft-MoE decoder head in inference and the pairwise set objective with its gradient
// (reference models/UMoED/hash/hash_moe.py, hash/block/transformer.py, hash/block/SoftMoe.py, models/common/hash.py; UMoED.py similarity_loss
// with distance/__init__.py pairwise_distance and DIMCH's loss/triplet_loss.py).
//
// ---- the head (xmh_head_umoed), one modality, eval mode ---------------------------------------------------------------------------------
//   mem = tokens [B, T, E]  (relu(first_layer(tokens)) when a first layer is given);  x = the M learned query rows, repeated over B
//   per layer, post-norm:  x = LN1(x + out(MHA(x, x, x)));  x = LN2(x + out(MHA(x, mem, mem)));  h = relu(linear(x)) [B, M, F]
//     MoE:    logits = h phi [B, M, S];  D = softmax over the M rows (per sample and slot);  Cw = softmax over the S slots (per row)
//             Xs = D^T h [B, S, F];  Ys[b, n, p] = Xs[b, n, p] W_n + bias_n [B, S, d];  x = LN3(x + Cw Ys)
//     plain:  x = LN3(x + linear2(h))
//   embeds = classifier(x) [B, M, V];  code = linear-subspace bits of argmax_v, or tanh / pair softmax of the mean over M
//
//   launches per layer, MoE: 16 -- self-attention 4 (xmh_gemm_nt_f32 in_proj, xmh_attention_f32, xmh_gemm_nt_f32 out_proj + residual,
//     xmh_layernorm_f32), cross-attention 5 (gemm q, gemm k|v of mem, k_umoed_attn, gemm out_proj + residual, layernorm),
//     soft-MoE 7 (gemm linear + ReLU, k_umoed_bmm logits, k_umoed_route, k_umoed_bmm dispatch, k_umoed_bmm experts, k_umoed_bmm
//     combine + residual, layernorm).  Plain: 12 (gemm linear + ReLU, gemm linear2 + residual, layernorm in place of the seven).
//   per call: 1 (k_umoed_queries) + [1 first layer] + layers x 16 (12) + 1 (k_umoed_classify): 98 at the config's six MoE layers.
//   The kernels and the layer chain (forward_chain) are in xmh_umoed_head.h, shared with the train-mode head of xmh_umoed_grad.hip.
//
//   k_umoed_bmm wraps the 64 x 64 tile core that k_mfma_mm wraps (xmh_mfma_mm.h: v_mfma_f32_32x32x2_f32, a 32-term chain per slab, slabs
//   in order) with a batch on grid z, a two-level row stride for the A rows and the C rows (the experts' rows (b, p) of expert n lie
//   S F apart in b and F apart in p) and bias / residual in the epilogue; the four soft-MoE products are its four argument sets.  The
//   reduction is never split, so there is one summation order.  k_umoed_attn: one block per (sample, head), K and V of the head
//   in LDS, a thread per query row, scores in two passes (maximum, then sum and P V) so that no score table is kept; no mask.
//
// ---- the objective (xmh_umoed_loss / xmh_umoed_loss_grad), distance.mode pairwise, distance_mode cosine, triplet ---------------------
//   x, y = F.normalize(rows of e_img, e_txt);  a, b = softmax(x / T), softmax(y / T) when extreme, else x, y
//   D[i][k] = mean_t (1 - max(a[i, t] . b[k, t], 0));  D_i2t = D, D_t2i = D^T
//   T(D, m) the label-weighted triplet term (xmh_triplet.h);  U(u) = mean_b sum_{t < t'} exp(-20 |u[b, t] - u[b, t']|^2) / (M (M - 1) / 2)
//   loss = triplet_alpha (T_i2t + T_t2i) / 4 + unif_alpha (U(x) + U(y)) / 3
//   xmh_umoed_loss       4 launches: k_umoed_prep (a wave per row), k_umoed_table (block i: row i of D, U of set i of both sides),
//                        k_umoed_triplet (block a: anchor row a of both terms), k_umoed_finalize
//   xmh_umoed_loss_grad  5 launches: prep, table, triplet as above (the call stands alone), k_umoed_triplet_grad (d loss / d D per anchor
//                        row), k_umoed_rows (a wave per token row: the clamp, the set mean, U, the softmax and the normalisation backward)
//   Squared distances of U are always sums of squared differences: identical rows give exactly 0, and nothing cancels for near rows.
//
// No allocation, no host synchronisation, no float atomics; every sum has one fixed order, so two calls agree to the bit.
#include <limits.h>
#include <math.h>

#include "xmh_common.h"
#include "xmh_mfma_mm.h"
#include "xmh_rows.h"
#include "xmh_triplet.h"

#include "xmh_umoed_head.h"

namespace {

namespace trip = xmh::trip;
using xmh::wave_max;
using xmh::wave_sum;
using umoed::kMaxM;
using umoed::kMaxV;

constexpr int kThreads = trip::kThreads, kWaves = trip::kWaves;
static_assert(kThreads == umoed::kThreads, "one block size for the head and the objective");
constexpr int kMaxLossB = trip::kMaxB, kMaxC = 127;
constexpr float kEps = 1e-12f;                 // F.normalize's eps
constexpr float kUnifT = 20.0f;                // batchwise_uniformity_loss's t

struct HeadWs {
    float *x, *y, *qkv, *att, *q, *kv, *mem, *h, *lg, *Dw, *Cw, *Xs, *Ys;
};

size_t head_layout(int64_t B, int T, const xmh_umoed_head* h, void* base, HeadWs* v) {
    xmh::Arena ar(base);
    const size_t BM = (size_t)B * h->M, BT = (size_t)B * T, d = (size_t)h->d, S = (size_t)h->n_experts * h->slots;
    HeadWs w;
    w.x = ar.take<float>(BM * d);
    w.y = ar.take<float>(BM * d);
    w.qkv = ar.take<float>(BM * 3 * d);
    w.att = ar.take<float>(BM * d);
    w.q = ar.take<float>(BM * d);
    w.kv = ar.take<float>(BT * 2 * d);
    w.mem = ar.take<float>(h->first_w ? BT * d : 0);
    w.h = ar.take<float>(BM * h->F);
    w.lg = ar.take<float>(h->moe ? BM * S : 0);
    w.Dw = ar.take<float>(h->moe ? BM * S : 0);
    w.Cw = ar.take<float>(h->moe ? BM * S : 0);
    w.Xs = ar.take<float>(h->moe ? (size_t)B * S * h->F : 0);
    w.Ys = ar.take<float>(h->moe ? (size_t)B * S * d : 0);
    if (v) *v = w;
    return ar.used;
}

}  // namespace

extern "C" size_t xmh_head_umoed_bytes(int64_t B, int T, const xmh_umoed_head* h) {
    if (umoed::head_shape(nullptr, B, T, h)) return 0;
    return head_layout(B, T, h, nullptr, nullptr);
}

extern "C" int xmh_head_umoed(const xmh_umoed_head* h, const float* tokens, int64_t B, int T, float* embeds, float* code, void* ws, size_t ws_bytes,
                              xmh_stream_t stream) {
    XMH_RANGE("xmh_head_umoed");
    const char* who = "xmh_head_umoed";
    if (int rc = umoed::head_shape(who, B, T, h)) return rc;
    if (!tokens || !embeds || !code || !ws) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    XMH_TRY(umoed::head_pointers(who, h));
    XMH_TRY(xmh::check_workspace(who, ws, ws_bytes, head_layout(B, T, h, nullptr, nullptr), "xmh_head_umoed_bytes", XMH_ENOMEM));
    HeadWs w;
    head_layout(B, T, h, ws, &w);
    const float* mem = tokens;
    if (h->first_w) {
        XMH_TRY(umoed::gemm(tokens, h->E, h->first_w, h->first_b, nullptr, w.mem, B * T, h->d, XMH_ACT_RELU, stream));
        mem = w.mem;
    }
    // every layer works in the same buffers: x -> y -> x through each of the three post-norm sublayers
    const umoed::LayerBufs bufs = {w.qkv, w.att, w.y, w.x, w.q, w.kv, w.att, w.y, w.x, w.h, w.lg, w.Dw, w.Cw, w.Xs, w.Ys, w.y, w.x, nullptr};
    return umoed::forward_chain(who, h, mem, nullptr, 0.0f, B, T, w.x, [&](int) { return bufs; }, embeds, code, stream);
}

// =========================================================================================================================================
// the objective
// =========================================================================================================================================
namespace {

struct LossWs {
    float* xn;       // [2][N][V] normalised rows (x, then y)
    float* an;       // [2][N][V] softmax(xn / T) when extreme, else xn itself
    float* nrm;      // [2N] norms of the raw rows
    float* Dt;       // [B][B] the distance table
    float* gD[2];    // d loss / d D_i2t [a][p], d loss / d D_t2i [a][p]
    double* upart;   // [2][B] sum over the pairs of a set of exp(-20 q)
    double* tsum;    // [2][B] per anchor: sum of positive triplets
    double* tcnt;    // [2][B] per anchor: their count
};

size_t loss_layout(int64_t B, int M, int V, int extreme, void* base, LossWs* v) {
    xmh::Arena ar(base);
    const size_t N = (size_t)B * M, BB = (size_t)B * B;
    LossWs w;
    w.xn = ar.take<float>(2 * N * V);
    w.an = ar.take<float>(2 * N * V);            // sized for either setting: the size function does not know `extreme`
    if (!extreme) w.an = w.xn;
    w.nrm = ar.take<float>(2 * N);
    w.Dt = ar.take<float>(BB);
    w.gD[0] = ar.take<float>(BB);
    w.gD[1] = ar.take<float>(BB);
    w.upart = ar.take<double>(2 * (size_t)B);
    w.tsum = ar.take<double>(2 * (size_t)B);
    w.tcnt = ar.take<double>(2 * (size_t)B);
    if (v) *v = w;
    return ar.used;
}

struct LossArgs {
    const float* e[2];        // e_img, e_txt [B, M, V]
    const uint32_t* lab;      // [B][Lw]
    int B, M, V, Lw, N;
    xmh_umoed_consts c;
};

using xmh::inv_norm;
using trip::clamp0;

// One wave per row of [0, 2N): the normalised row, its norm, and softmax(row / T) when extreme.  V <= 256: four elements per lane.
__global__ __launch_bounds__(kThreads) void k_umoed_prep(LossArgs a, LossWs w) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, V = a.V;
    const int64_t row = (int64_t)blockIdx.x * kWaves + wave;
    if (row >= 2 * (int64_t)a.N) return;
    const int side = row >= a.N;
    const float* src = a.e[side] + (row - (int64_t)side * a.N) * V;
    float v[4], s = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j;
        v[j] = k < V ? src[k] : 0.0f;
        s = fmaf(v[j], v[j], s);
    }
    const float nv = sqrtf(wave_sum(s)), dn = nv < kEps ? kEps : nv;     // a NaN norm stays NaN
    if (lane == 0) w.nrm[row] = nv;
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j;
        v[j] = v[j] / dn;                                            // a division as F.normalize's: U = exp(-20 q) magnifies q's error
        if (k < V) {
            w.xn[row * V + k] = v[j];
            v[j] = v[j] / a.c.extreme_T;
            mx = fmaxf(mx, v[j]);
        }
    }
    if (!a.c.extreme) return;
    mx = wave_max(mx);
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j;
        v[j] = k < V ? expf(v[j] - mx) : 0.0f;                      // a NaN entry: fmaxf dropped it, it comes back here
        sum += v[j];
    }
    sum = wave_sum(sum);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j;
        if (k < V) w.an[row * V + k] = v[j] / sum;
    }
}

// Block i: row i of D (a wave per column k, lanes over the tokens t, each dot product an l-ordered fmaf chain) and the U sums of set i
// of both sides.
__global__ __launch_bounds__(kThreads) void k_umoed_table(LossArgs a, LossWs w) {
    __shared__ double dsh[kWaves];
    const int B = a.B, M = a.M, V = a.V, i = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* A = w.an + (int64_t)i * M * V;
    const float* Bm = w.an + (int64_t)a.N * V;
    for (int k = wave; k < B; k += kWaves) {
        float acc = 0.0f;
        for (int t = lane; t < M; t += 64) {
            const float* ar = A + (int64_t)t * V;
            const float* br = Bm + ((int64_t)k * M + t) * V;
            float s = 0.0f;
            for (int l = 0; l < V; ++l) s = fmaf(ar[l], br[l], s);
            acc += 1.0f - clamp0(s);
        }
        acc = wave_sum(acc);
        if (lane == 0) w.Dt[(int64_t)i * B + k] = acc / (float)M;
    }
    for (int side = 0; side < 2; ++side) {
        const float* U = w.xn + ((int64_t)side * a.N + (int64_t)i * M) * V;
        double uu = 0.0;
        for (int idx = threadIdx.x; idx < M * M; idx += kThreads) {
            const int t = idx / M, t2 = idx % M;
            if (t >= t2) continue;
            float q = 0.0f;
            for (int l = 0; l < V; ++l) {
                const float df = U[t * V + l] - U[t2 * V + l];
                q = fmaf(df, df, q);
            }
            uu += (double)expf(-kUnifT * q);
        }
        uu = xmh::block_sum<kWaves>(uu, dsh);
        if (threadIdx.x == 0) w.upart[side * B + i] = uu;
    }
}

// the distance row of anchor `row` of term t (0: D, 1: D^T) into ds [B]; ends with a barrier
__device__ __forceinline__ void distance_row(const LossArgs& a, const LossWs& w, int row, int t, float* ds) {
    for (int p = threadIdx.x; p < a.B; p += kThreads) ds[p] = t == 0 ? w.Dt[(int64_t)row * a.B + p] : w.Dt[(int64_t)p * a.B + row];
    __syncthreads();
}

__global__ __launch_bounds__(kThreads) void k_umoed_triplet(LossArgs a, LossWs w) {
    __shared__ int cs[kMaxLossB];
    __shared__ float wsh[kMaxLossB], sim[kMaxLossB], ds[kMaxLossB];
    __shared__ double dsh[kWaves];
    const int B = a.B, row = blockIdx.x;
    trip::weights(a.lab, a.Lw, B, row, cs, wsh, sim, dsh);
    for (int t = 0; t < 2; ++t) {
        distance_row(a, w, row, t, ds);
        double sum, cnt;
        trip::row_terms(wsh, sim, ds, B, a.c.token_triplet_margin, dsh, &sum, &cnt);
        if (threadIdx.x == 0) w.tsum[t * B + row] = sum, w.tcnt[t * B + row] = cnt;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void k_umoed_finalize(LossArgs a, LossWs w, double* __restrict__ out8) {
    __shared__ double dsh[kWaves];
    const int B = a.B;
    double T[2], U[2];
    for (int t = 0; t < 2; ++t) {
        const double s = trip::ordered_sum(w.tsum + t * B, B, dsh), c = trip::ordered_sum(w.tcnt + t * B, B, dsh);
        T[t] = s / (c + 1e-16);
        U[t] = trip::ordered_sum(w.upart + t * B, B, dsh);
    }
    if (threadIdx.x == 0) {
        const double pairs = 0.5 * a.M * (a.M - 1);
        for (int t = 0; t < 2; ++t) U[t] = a.M > 1 ? U[t] / pairs / (double)B : 0.0;
        out8[0] = a.c.triplet_alpha * ((T[0] + T[1]) / 4) + a.c.unif_alpha * ((U[0] + U[1]) / 3);
        out8[1] = T[0], out8[2] = T[1], out8[3] = U[0], out8[4] = U[1];
        out8[5] = out8[6] = out8[7] = 0.0;
    }
}

// Anchor row a of both terms: gD[t][a][p] = d loss / d D_t[a][p], upstream included.
__global__ __launch_bounds__(kThreads) void k_umoed_triplet_grad(LossArgs a, LossWs w, const float* __restrict__ up) {
    __shared__ int cs[kMaxLossB];
    __shared__ float wsh[kMaxLossB], sim[kMaxLossB], ds[kMaxLossB];
    __shared__ double dsh[kWaves];
    const int B = a.B, row = blockIdx.x;
    const float g = up ? up[0] : 1.0f;
    trip::weights(a.lab, a.Lw, B, row, cs, wsh, sim, dsh);
    for (int t = 0; t < 2; ++t) {
        const double total = trip::ordered_sum(w.tcnt + t * B, B, dsh);
        const float scale = g * 0.25f * a.c.triplet_alpha / (float)(total + 1e-16);
        distance_row(a, w, row, t, ds);
        for (int p = threadIdx.x; p < B; p += kThreads)
            w.gD[t][(int64_t)row * B + p] = trip::col_grad(wsh, sim, ds, B, a.c.token_triplet_margin, p) * scale;
        __syncthreads();
    }
}

// One wave per token row (side, i, t), four elements per lane.  d loss / d a of the row: over the B sets k of the other side,
// -(G / M) [a . b >= 0] b[k, t] with G = d loss / d D[i][k] (the row's own side first in D); the softmax backward when extreme;
// then U's share at the normalised row, and the backward of F.normalize: (du - u (u . du)) / max(|v|, eps), du / eps for a clamped row.
__global__ __launch_bounds__(kThreads) void k_umoed_rows(LossArgs a, LossWs w, const float* __restrict__ up, float* g_img, float* g_txt,
                                                         int accumulate) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, V = a.V, M = a.M, B = a.B;
    const int64_t row = (int64_t)blockIdx.x * kWaves + wave, N = a.N;
    if (row >= 2 * N) return;
    const int side = row >= N;
    float* gout = side ? g_txt : g_img;
    if (!gout) return;
    const int64_t r = row - (int64_t)side * N;
    const int i = (int)(r / M), t = (int)(r % M);
    const float g = up ? up[0] : 1.0f;
    float ar[4], da[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int l = lane + 64 * j;
        ar[j] = l < V ? w.an[row * V + l] : 0.0f;
        da[j] = 0.0f;
    }
    const float* other = w.an + (int64_t)(1 - side) * N * V;
    for (int k = 0; k < B; ++k) {
        const float* brow = other + ((int64_t)k * M + t) * V;
        float br[4], dot = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int l = lane + 64 * j;
            br[j] = l < V ? brow[l] : 0.0f;
            dot = fmaf(ar[j], br[j], dot);
        }
        dot = wave_sum(dot);
        const float G = side == 0 ? w.gD[0][(int64_t)i * B + k] + w.gD[1][(int64_t)k * B + i] : w.gD[0][(int64_t)k * B + i] + w.gD[1][(int64_t)i * B + k];
        const float coef = -(G / (float)M) * (dot >= 0.0f ? 1.0f : 0.0f);       // the set mean and clamp(min = 0) backward
#pragma unroll
        for (int j = 0; j < 4; ++j) da[j] = fmaf(coef, br[j], da[j]);
    }
    float u[4], du[4];
    const float* ur = w.xn + row * V;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int l = lane + 64 * j;
        u[j] = l < V ? ur[l] : 0.0f;
    }
    if (a.c.extreme) {
        float inner = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) inner = fmaf(ar[j], da[j], inner);
        inner = wave_sum(inner);
#pragma unroll
        for (int j = 0; j < 4; ++j) du[j] = ar[j] * (da[j] - inner) / a.c.extreme_T;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) du[j] = da[j];
    }
    if (M > 1) {
        const float cu = g * a.c.unif_alpha / 3.0f / ((float)B * (0.5f * (float)M * (float)(M - 1)));
        const float* set = w.xn + ((int64_t)side * N + (int64_t)i * M) * V;
        for (int t2 = 0; t2 < M; ++t2) {
            if (t2 == t) continue;
            float df[4], q = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int l = lane + 64 * j;
                df[j] = l < V ? u[j] - set[(int64_t)t2 * V + l] : 0.0f;
                q = fmaf(df[j], df[j], q);
            }
            q = wave_sum(q);
            const float e = cu * (-2.0f * kUnifT * expf(-kUnifT * q));
#pragma unroll
            for (int j = 0; j < 4; ++j) du[j] = fmaf(e, df[j], du[j]);
        }
    }
    float dot = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) dot = fmaf(u[j], du[j], dot);
    dot = wave_sum(dot);
    const float nv = w.nrm[row], iv = inv_norm(nv, kEps);
    if (nv < kEps) dot = 0.0f;
    float* out = gout + r * V;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int l = lane + 64 * j;
        if (l < V) {
            const float dv = (du[j] - u[j] * dot) * iv;
            out[l] = accumulate ? out[l] + dv : dv;
        }
    }
}

bool loss_shape_ok(int64_t B, int M, int V, int C) { return B > 0 && M > 0 && V > 0 && C > 0 && B <= kMaxLossB && M <= kMaxM && V <= kMaxV && C <= kMaxC; }

int check_loss(const char* who, const float* e_img, const float* e_txt, int64_t B, int M, int V, int C, const uint32_t* lab, const xmh_umoed_consts* cst,
               void* ws, size_t ws_bytes) {
    if (B <= 0 || M <= 0 || V <= 0 || C <= 0) return xmh::fail(XMH_EINVAL, "%s: bad shape B=%lld M=%d V=%d C=%d", who, (long long)B, M, V, C);
    if (!loss_shape_ok(B, M, V, C))
        return xmh::fail(XMH_ENOTSUP, "%s: B=%lld M=%d V=%d C=%d outside B <= %d, M <= %d, V <= %d, C <= %d", who, (long long)B, M, V, C, kMaxLossB, kMaxM,
                         kMaxV, kMaxC);
    if (!e_img || !e_txt || !lab || !cst || !ws) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (cst->extreme && !(cst->extreme_T > 0.0f)) return xmh::fail(XMH_EINVAL, "%s: extreme_T %g must be positive", who, (double)cst->extreme_T);
    return xmh::check_workspace(who, ws, ws_bytes, loss_layout(B, M, V, 1, nullptr, nullptr), "xmh_umoed_loss_ws_bytes", XMH_ENOMEM);
}

LossArgs make_loss_args(const float* e_img, const float* e_txt, int64_t B, int M, int V, int C, const uint32_t* lab, const xmh_umoed_consts* cst) {
    LossArgs a;
    a.e[0] = e_img, a.e[1] = e_txt, a.lab = lab;
    a.B = (int)B, a.M = M, a.V = V, a.Lw = (C + 31) / 32, a.N = (int)B * M;
    a.c = *cst;
    if (!a.c.extreme) a.c.extreme_T = 1.0f;       // unused then; keeps the division in k_umoed_prep defined
    return a;
}

// the three launches both entry points begin with
void launch_loss_common(const LossArgs& a, const LossWs& v, hipStream_t st) {
    const int64_t rows = 2 * (int64_t)a.N;
    hipLaunchKernelGGL(k_umoed_prep, dim3((unsigned)((rows + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, a, v);
    hipLaunchKernelGGL(k_umoed_table, dim3((unsigned)a.B), dim3(kThreads), 0, st, a, v);
    hipLaunchKernelGGL(k_umoed_triplet, dim3((unsigned)a.B), dim3(kThreads), 0, st, a, v);
}

}  // namespace

extern "C" size_t xmh_umoed_loss_ws_bytes(int64_t B, int M, int V, int C) {
    if (!loss_shape_ok(B, M, V, C)) return 0;
    return loss_layout(B, M, V, 1, nullptr, nullptr);
}

extern "C" int xmh_umoed_loss(const float* e_img, const float* e_txt, int64_t B, int M, int V, int C, const uint32_t* lab, const xmh_umoed_consts* cst,
                              void* ws, size_t ws_bytes, double* out8, xmh_stream_t stream) {
    XMH_RANGE("xmh_umoed_loss");
    if (int rc = check_loss("xmh_umoed_loss", e_img, e_txt, B, M, V, C, lab, cst, ws, ws_bytes)) return rc;
    if (!out8) return xmh::fail(XMH_EINVAL, "xmh_umoed_loss: null pointer");
    LossWs v;
    loss_layout(B, M, V, cst->extreme, ws, &v);
    const LossArgs a = make_loss_args(e_img, e_txt, B, M, V, C, lab, cst);
    hipStream_t st = xmh::as_stream(stream);
    launch_loss_common(a, v, st);
    hipLaunchKernelGGL(k_umoed_finalize, dim3(1), dim3(kThreads), 0, st, a, v, out8);
    XMH_LAUNCH_CHECK("xmh_umoed_loss");
    return XMH_OK;
}

extern "C" int xmh_umoed_loss_grad(const float* e_img, const float* e_txt, int64_t B, int M, int V, int C, const uint32_t* lab,
                                   const xmh_umoed_consts* cst, const float* upstream, float* g_img, float* g_txt, int accumulate, void* ws,
                                   size_t ws_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_umoed_loss_grad");
    if (int rc = check_loss("xmh_umoed_loss_grad", e_img, e_txt, B, M, V, C, lab, cst, ws, ws_bytes)) return rc;
    if (!g_img && !g_txt) return XMH_OK;
    LossWs v;
    loss_layout(B, M, V, cst->extreme, ws, &v);
    const LossArgs a = make_loss_args(e_img, e_txt, B, M, V, C, lab, cst);
    hipStream_t st = xmh::as_stream(stream);
    launch_loss_common(a, v, st);
    hipLaunchKernelGGL(k_umoed_triplet_grad, dim3((unsigned)B), dim3(kThreads), 0, st, a, v, upstream);
    hipLaunchKernelGGL(k_umoed_rows, dim3((unsigned)((2 * (int64_t)a.N + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, a, v, upstream, g_img, g_txt,
                       accumulate);
    XMH_LAUNCH_CHECK("xmh_umoed_loss_grad");
    return XMH_OK;
}
