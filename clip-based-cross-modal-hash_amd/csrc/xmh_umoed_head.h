// What the two UMoED head files share (xmh_umoed.hip: the inference entry point; xmh_umoed_grad.hip: the train-mode forward and the
// backward): the bounds, the batched exact-fp32 product k_umoed_bmm with its argument sets, the attention and routing kernels, the
// classifier, and forward_chain, the ONE layer chain behind xmh_head_umoed and xmh_head_umoed_train_forward.  Without a keep mask the
// chain issues the same kernels with the same arithmetic whoever calls it, so the two entry points agree to the bit; only where the
// buffers lie differs (a rotating workspace in inference, the record in training).
#pragma once
#include <limits.h>
#include <math.h>

#include "xmh_common.h"
#include "xmh_device.h"
#include "xmh_mfma_mm.h"

namespace {
namespace umoed {

namespace mm = xmh::mm;
using xmh::wave_max;
using xmh::wave_sum;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxM = 128, kMaxT = 128, kMaxE = 2048, kMaxD = 1024, kMaxF = 4096, kMaxS = 256, kMaxV = 256;
constexpr int64_t kMaxRows = 32768;            // B max(M, T), the row limit of the other heads
constexpr int kAttnThreads = 128;              // a thread per query (or key) row: M, T <= 128

// ---- batched exact-fp32 product -------------------------------------------------------------------------------------------------------
using mm::kTile;
static_assert(kThreads == mm::kThreads, "the tile core's block");

struct BmmArgs {
    const float* A;           // A(z; i, k) = A[z sab + (i / adiv) sah + (i % adiv) sai + k sak]
    int64_t sai, sak, sab, sah;
    int adiv;
    const float* B;           // B(z; j, k) = B[z sbb + j sbj + k sbk]
    int64_t sbj, sbk, sbb;
    int I, J, Kd;
    float* C;                 // C(z; i, j) = C[z scb + (i / cdiv) sch + (i % cdiv) sci + j]
    int64_t sci, scb, sch;
    int cdiv;
    const float* bias;        // bias[z sbias + j], or NULL
    int64_t sbias;
    const float* res;         // residual, addressed as C, or NULL (it may be C itself)
};

// AK / BK: k is the unit-stride index of that operand (which index the lanes of a load walk; the arithmetic is the same).  Grid
// (I tiles, J tiles, batch).  The reduction is the tile core's, whole: one chunk [0, Kd).
template <bool AK, bool BK>
__global__ __launch_bounds__(kThreads) void k_umoed_bmm(BmmArgs g) {
    const int i0 = blockIdx.x * kTile, j0 = blockIdx.y * kTile;
    const int64_t z = blockIdx.z;
    const mm::Operand a = mm::make_operand<AK>(g.A + z * g.sab, g.sak, i0, g.I,
                                               [&](int i) { return (int64_t)(i / g.adiv) * g.sah + (int64_t)(i % g.adiv) * g.sai; });
    const mm::Operand b = mm::make_operand<BK>(g.B + z * g.sbb, g.sbk, j0, g.J, [&](int j) { return (int64_t)j * g.sbj; });
    const mm::f32x16 tot = mm::tile_product<AK, BK>(a, b, 0, g.Kd, [](const auto&) {});
    const int j = mm::out_col(j0);
    if (j >= g.J) return;
    const float bj = g.bias ? g.bias[z * g.sbias + j] : 0.0f;
    const int64_t at0 = z * g.scb + j;
    mm::for_each_output(tot, i0, j0, g.I, g.J, [&](int i, int, float v) {
        const int64_t at = at0 + (int64_t)(i / g.cdiv) * g.sch + (int64_t)(i % g.cdiv) * g.sci;
        if (g.bias) v += bj;
        if (g.res) v += g.res[at];
        g.C[at] = v;
    });
}

template <bool AK, bool BK>
void launch_bmm(hipStream_t st, const BmmArgs& g, int64_t batch) {
    const dim3 grid((unsigned)((g.I + kTile - 1) / kTile), (unsigned)((g.J + kTile - 1) / kTile), (unsigned)batch);
    hipLaunchKernelGGL((k_umoed_bmm<AK, BK>), grid, dim3(kThreads), 0, st, g);
}

inline BmmArgs bmm_args() {
    BmmArgs g = {};
    g.adiv = g.cdiv = INT_MAX;
    return g;
}

// The argument sets of the soft-MoE products, forward and backward.  Xs and dYs lie expert-major, [n][B P][F] and [n][B P][d] (row
// (b, p) of expert n), so that an expert's rows are one contiguous matrix for its product and for its weight gradient; every other
// table is sample-major.
struct MoeDims {
    int64_t B;
    int M, d, F, P, N;        // S = N P
    int S() const { return N * P; }
};

inline BmmArgs logits_args(const MoeDims& m, const float* h, const float* phi, float* lg) {       // logits [B M, S] = h phi
    BmmArgs g = bmm_args();
    g.A = h, g.sai = m.F, g.sak = 1;
    g.B = phi, g.sbj = 1, g.sbk = m.S();
    g.I = (int)(m.B * m.M), g.J = m.S(), g.Kd = m.F;
    g.C = lg, g.sci = m.S();
    return g;
}
inline BmmArgs dispatch_args(const MoeDims& m, const float* Dw, const float* h, float* Xs) {       // Xs[b] [S, F] = D[b]^T h[b], batch B
    BmmArgs g = bmm_args();
    g.A = Dw, g.sai = 1, g.sak = m.S(), g.sab = (int64_t)m.M * m.S();
    g.B = h, g.sbj = 1, g.sbk = m.F, g.sbb = (int64_t)m.M * m.F;
    g.I = m.S(), g.J = m.F, g.Kd = m.M;
    g.C = Xs, g.sci = m.F, g.scb = (int64_t)m.P * m.F, g.cdiv = m.P, g.sch = m.B * m.P * m.F;
    return g;
}
inline BmmArgs experts_args(const MoeDims& m, const float* Xs, const float* W, const float* bias, float* Ys) {      // batch N
    BmmArgs g = bmm_args();
    g.A = Xs, g.sai = m.F, g.sak = 1, g.sab = m.B * m.P * m.F;                   // rows (b, p) of expert n
    g.B = W, g.sbj = 1, g.sbk = m.d, g.sbb = (int64_t)m.F * m.d;                 // W_n [F, d], "in, out"
    g.I = (int)(m.B * m.P), g.J = m.d, g.Kd = m.F;
    g.C = Ys, g.sci = m.d, g.scb = (int64_t)m.P * m.d, g.cdiv = m.P, g.sch = (int64_t)m.S() * m.d;      // Ys [B, S, d]
    g.bias = bias, g.sbias = m.d;
    return g;
}
inline BmmArgs combine_args(const MoeDims& m, const float* Cw, const float* Ys, const float* res, float* y) {       // y[b] = res[b] + Cw[b] Ys[b]
    BmmArgs g = bmm_args();
    g.A = Cw, g.sai = m.S(), g.sak = 1, g.sab = (int64_t)m.M * m.S();
    g.B = Ys, g.sbj = 1, g.sbk = m.d, g.sbb = (int64_t)m.S() * m.d;
    g.I = m.M, g.J = m.d, g.Kd = m.S();
    g.C = y, g.sci = m.d, g.scb = (int64_t)m.M * m.d;
    g.res = res;
    return g;
}

// ---- the learned queries, repeated over the batch --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_umoed_queries(const float* __restrict__ q, int64_t per, int64_t total, float* __restrict__ x) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e < total) x[e] = q[e % per];
}

// ---- attention with separate q and k | v rows: q row (b, i) at q + (b M + i) ldq, k row (b, j) at k + (b T + j) ldkv, v row voff behind
// it; out [B M, H 64].  Block (sample, head), thread = query row, dh = 64.  The cross-attention reads q [B M, d] and kv [B T, 2 d];
// the self-attention under a keep mask reads the packed qkv buffer three times (ld 3 d).  KEEP: keep [B, H, M, T] bytes on the
// probabilities, after the softmax and before P V, kept entries scaled by ks = 1 / (1 - p). ---------------------------------------------
template <bool KEEP>
__global__ __launch_bounds__(kAttnThreads) void k_umoed_attn(const float* __restrict__ q, int64_t ldq, const float* __restrict__ kp, int64_t ldkv, int voff,
                                                             int M, int T, int H, const uint8_t* __restrict__ keep, float ks, float* __restrict__ out) {
    constexpr int DH = 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int D = H * DH;
    float4* sK = reinterpret_cast<float4*>(smem);                    // [T][DH / 4]; every lane reads the same address: a broadcast
    float4* sV = sK + T * (DH / 4);                                  // [T][DH / 4]
    const float* kb = kp + (int64_t)b * T * ldkv + h * DH;
    for (int e = threadIdx.x; e < T * (DH / 4); e += blockDim.x) {
        const int j = e / (DH / 4), c4 = e % (DH / 4);
        sK[e] = *reinterpret_cast<const float4*>(kb + (int64_t)j * ldkv + c4 * 4);
        sV[e] = *reinterpret_cast<const float4*>(kb + (int64_t)j * ldkv + voff + c4 * 4);
    }
    __syncthreads();
    const int i = threadIdx.x;
    if (i >= M) return;
    const int64_t row = (int64_t)b * M + i;
    float qr[DH];
    const float scale = rsqrtf((float)DH);
#pragma unroll
    for (int c = 0; c < DH / 4; ++c) {                               // PyTorch scales q before Q K^T
        const float4 v = *reinterpret_cast<const float4*>(q + row * ldq + h * DH + c * 4);
        qr[4 * c + 0] = v.x * scale, qr[4 * c + 1] = v.y * scale, qr[4 * c + 2] = v.z * scale, qr[4 * c + 3] = v.w * scale;
    }
    auto score = [&](int j) {
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int c = 0; c < DH / 4; ++c) {
            const float4 kk = sK[j * (DH / 4) + c];
            s0 = fmaf(qr[4 * c + 0], kk.x, s0);
            s1 = fmaf(qr[4 * c + 1], kk.y, s1);
            s0 = fmaf(qr[4 * c + 2], kk.z, s0);
            s1 = fmaf(qr[4 * c + 3], kk.w, s1);
        }
        return s0 + s1;
    };
    float mx = -INFINITY;
    for (int j = 0; j < T; ++j) mx = fmaxf(mx, score(j));
    float o[DH];
#pragma unroll
    for (int c = 0; c < DH; ++c) o[c] = 0.0f;
    float sum = 0.0f;
    const uint8_t* kr = KEEP ? keep + ((int64_t)blockIdx.x * M + i) * T : nullptr;
    for (int j = 0; j < T; ++j) {
        float p = expf(score(j) - mx);                               // the same chain as in the first pass: the largest is exp(0)
        sum += p;
        if (KEEP && !kr[j]) p = 0.0f;                                // the sum is the softmax's: dropout acts on the probabilities
#pragma unroll
        for (int c = 0; c < DH / 4; ++c) {
            const float4 vv = sV[j * (DH / 4) + c];
            o[4 * c + 0] = fmaf(p, vv.x, o[4 * c + 0]);
            o[4 * c + 1] = fmaf(p, vv.y, o[4 * c + 1]);
            o[4 * c + 2] = fmaf(p, vv.z, o[4 * c + 2]);
            o[4 * c + 3] = fmaf(p, vv.w, o[4 * c + 3]);
        }
    }
    float inv = 1.0f / sum;
    if (KEEP) inv *= ks;
#pragma unroll
    for (int c = 0; c < DH / 4; ++c)
        *reinterpret_cast<float4*>(out + row * D + h * DH + c * 4) = make_float4(o[4 * c + 0] * inv, o[4 * c + 1] * inv, o[4 * c + 2] * inv, o[4 * c + 3] * inv);
}

inline size_t attn_lds(int rows) { return (size_t)2 * rows * 64 * sizeof(float); }

// ---- routing: block = sample; its logits [M, S] staged in LDS once; D = softmax down the columns, Cw = softmax along the rows -------------
__global__ __launch_bounds__(kThreads) void k_umoed_route(const float* __restrict__ logits, int M, int S, float* __restrict__ Dw, float* __restrict__ Cw) {
    extern __shared__ __attribute__((aligned(16))) float ls[];      // [M][S]: lanes walk s, consecutive banks in both phases
    const int64_t base = (int64_t)blockIdx.x * M * S;
    for (int e = threadIdx.x; e < M * S; e += kThreads) ls[e] = logits[base + e];
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += kThreads) {                // a thread per slot: the M rows in order
        float mx = -INFINITY;
        for (int m = 0; m < M; ++m) mx = fmaxf(mx, ls[m * S + s]);
        float sum = 0.0f;
        for (int m = 0; m < M; ++m) sum += expf(ls[m * S + s] - mx);
        for (int m = 0; m < M; ++m) Dw[base + (int64_t)m * S + s] = expf(ls[m * S + s] - mx) / sum;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int m = wave; m < M; m += kWaves) {                         // a wave per row
        float mx = -INFINITY;
        for (int s = lane; s < S; s += 64) mx = fmaxf(mx, ls[m * S + s]);
        mx = wave_max(mx);
        float sum = 0.0f;
        for (int s = lane; s < S; s += 64) sum += expf(ls[m * S + s] - mx);
        sum = wave_sum(sum);
        for (int s = lane; s < S; s += 64) Cw[base + (int64_t)m * S + s] = expf(ls[m * S + s] - mx) / sum;
    }
}

// ---- classifier and code: block = sample ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_umoed_classify(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                             int M, int d, int V, int hash_func, float* __restrict__ embeds, float* __restrict__ code) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = blockIdx.x;
    const float* xb = x + b * M * d;
    float* eb = embeds + b * M * V;
    for (int pair = wave; pair < M * V; pair += kWaves) {            // a wave per logit
        const int m = pair / V, v = pair % V;
        float s = 0.0f;
        for (int k = lane; k < d; k += 64) s = fmaf(xb[(int64_t)m * d + k], w[(int64_t)v * d + k], s);
        s = wave_sum(s);
        if (lane == 0) eb[pair] = s + bias[v];
    }
    __syncthreads();                                                 // the block's own global writes are visible to it behind the barrier
    if (hash_func == XMH_UMOED_LINEAR_SUBSPACE) {
        int bits = 0;
        while ((1 << bits) < V) ++bits;
        for (int m = threadIdx.x; m < M; m += kThreads) {
            float best = eb[m * V];
            int at = 0;
            for (int v = 1; v < V; ++v) {
                const float e = eb[m * V + v];
                if (e > best) best = e, at = v;                      // the first index on a tie
            }
            for (int j = 0; j < bits; ++j) code[(b * M + m) * bits + j] = ((at >> (bits - 1 - j)) & 1) ? 1.0f : -1.0f;      // most significant first
        }
        return;
    }
    auto mean_of = [&](int v) {
        float s = 0.0f;
        for (int m = 0; m < M; ++m) s += eb[m * V + v];
        return s / (float)M;
    };
    if (hash_func == XMH_UMOED_TANH) {
        for (int v = threadIdx.x; v < V; v += kThreads) code[b * V + v] = tanhf(mean_of(v));
        return;
    }
    for (int p = threadIdx.x; p < V / 2; p += kThreads) {             // pair softmax
        const float a0 = mean_of(2 * p), a1 = mean_of(2 * p + 1);
        const float mx = fmaxf(a0, a1), e0 = expf(a0 - mx), e1 = expf(a1 - mx);
        code[b * V + 2 * p] = e0 / (e0 + e1);
        code[b * V + 2 * p + 1] = e1 / (e0 + e1);
    }
}

// ---- dropout on a sublayer's output, fused into the residual add, and on the ReLU rows ---------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_umoed_res_drop(const float* __restrict__ x, const float* __restrict__ t, const uint8_t* __restrict__ keep,
                                                             float ks, int64_t n, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e < n) out[e] = x[e] + (keep[e] ? t[e] * ks : 0.0f);
}
__global__ __launch_bounds__(kThreads) void k_umoed_drop(float* __restrict__ h, const uint8_t* __restrict__ keep, float ks, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e < n) h[e] = keep[e] ? h[e] * ks : 0.0f;
}
inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// ---- the keep mask: per layer six sections, the layers one after the other ----------------------------------------------------------------
struct KeepLayout {
    size_t at[6], layer;      // byte offsets of drop1 .. drop6 inside a layer, and the bytes of a layer
};
inline KeepLayout keep_layout(int64_t B, int T, const xmh_umoed_head* h) {
    const size_t BM = (size_t)B * h->M, n[6] = {(size_t)B * h->heads * h->M * h->M, BM * h->d, (size_t)B * h->heads * h->M * T, BM * h->d, BM * h->F, BM * h->d};
    KeepLayout k;
    size_t at = 0;
    for (int i = 0; i < 6; ++i) k.at[i] = at, at += n[i];
    k.layer = at;
    return k;
}

inline bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// 0: fine; otherwise the status, with the text set when `who` is given
inline int head_shape(const char* who, int64_t B, int T, const xmh_umoed_head* h) {
#define UMOED_FAIL(code, ...) return who ? xmh::fail(code, __VA_ARGS__) : code
    if (!h) UMOED_FAIL(XMH_EINVAL, "%s: null pointer", who);
    if (B <= 0 || T <= 0 || h->E <= 0 || h->d <= 0 || h->heads <= 0 || h->F <= 0 || h->M <= 0 || h->V <= 0 || h->n_layers <= 0)
        UMOED_FAIL(XMH_EINVAL, "%s: bad shape B=%lld T=%d E=%d d=%d heads=%d F=%d M=%d V=%d layers=%d", who, (long long)B, T, h->E, h->d, h->heads,
                   h->F, h->M, h->V, h->n_layers);
    if (h->moe && (h->n_experts <= 0 || h->slots <= 0)) UMOED_FAIL(XMH_EINVAL, "%s: bad shape experts=%d slots=%d", who, h->n_experts, h->slots);
    if (h->hash_func < XMH_UMOED_LINEAR_SUBSPACE || h->hash_func > XMH_UMOED_SOFTMAX) UMOED_FAIL(XMH_EINVAL, "%s: hash_func %d", who, h->hash_func);
    if ((h->hash_func == XMH_UMOED_LINEAR_SUBSPACE) != (h->merge == XMH_UMOED_CONCATENATE) || h->merge < XMH_UMOED_CONCATENATE || h->merge > XMH_UMOED_MEAN)
        UMOED_FAIL(XMH_EINVAL, "%s: hash_func %d with merge %d (linear_subspace goes with concatenate, tanh and softmax with mean)", who, h->hash_func,
                   h->merge);
    if (!h->first_w && h->d != h->E) UMOED_FAIL(XMH_EINVAL, "%s: d=%d differs from E=%d and there is no first layer", who, h->d, h->E);
    if (h->hash_func == XMH_UMOED_SOFTMAX && h->V % 2) UMOED_FAIL(XMH_EINVAL, "%s: the pair softmax needs an even V (V=%d)", who, h->V);
    if (h->d % h->heads || h->d / h->heads != 64) UMOED_FAIL(XMH_ENOTSUP, "%s: head dim %d / %d (only 64, the attention kernels')", who, h->d, h->heads);
    if (h->M > kMaxM || T > kMaxT) UMOED_FAIL(XMH_ENOTSUP, "%s: M=%d T=%d outside M <= %d, T <= %d", who, h->M, T, kMaxM, kMaxT);
    if (h->E > kMaxE || h->d > kMaxD || h->F > kMaxF)
        UMOED_FAIL(XMH_ENOTSUP, "%s: E=%d d=%d F=%d outside E <= %d, d <= %d (the LayerNorm kernel's width), F <= %d", who, h->E, h->d, h->F, kMaxE, kMaxD,
                   kMaxF);
    if (h->moe && (int64_t)h->n_experts * h->slots > kMaxS)
        UMOED_FAIL(XMH_ENOTSUP, "%s: %d experts x %d slots outside S <= %d", who, h->n_experts, h->slots, kMaxS);
    if (h->V > kMaxV || (h->hash_func == XMH_UMOED_LINEAR_SUBSPACE && !is_pow2(h->V)))
        UMOED_FAIL(XMH_ENOTSUP, "%s: V=%d outside V <= %d (a power of two for linear_subspace)", who, h->V, kMaxV);
    if (B > 65535 || B * (int64_t)(h->M > T ? h->M : T) > kMaxRows)
        UMOED_FAIL(XMH_ENOTSUP, "%s: B=%lld with M=%d T=%d outside B max(M, T) <= %lld, B <= 65535", who, (long long)B, h->M, T, (long long)kMaxRows);
#undef UMOED_FAIL
    return XMH_OK;
}

// the pointers every entry point of the head needs
inline int head_pointers(const char* who, const xmh_umoed_head* h) {
    if (!h->layers || !h->queries || !h->cls_w || !h->cls_b || (h->first_w && !h->first_b)) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    for (int l = 0; l < h->n_layers; ++l) {
        const xmh_umoed_layer& y = h->layers[l];
        const bool common = y.ln1_g && y.ln1_b && y.sa_in_w && y.sa_in_b && y.sa_out_w && y.sa_out_b && y.ln2_g && y.ln2_b && y.ca_in_w && y.ca_in_b &&
                            y.ca_out_w && y.ca_out_b && y.ln3_g && y.ln3_b && y.lin_w && y.lin_b;
        if (!common || (h->moe ? !(y.phi && y.exp_w && y.exp_b) : !(y.lin2_w && y.lin2_b)))
            return xmh::fail(XMH_EINVAL, "%s: null pointer in layer %d", who, l);
    }
    return XMH_OK;
}

inline int gemm(const float* A, int64_t K, const float* W, const float* bias, const float* res, float* Cm, int64_t rows, int64_t N, int act, xmh_stream_t s) {
    return xmh_gemm_nt_f32(A, K, W, K, bias, res, N, Cm, N, rows, N, K, act, XMH_PREC_F32, s);
}

// Where one layer of the chain reads and writes.  x -> (qkv, att1) -> u1 -> x1 -> (q, kv, att2) -> u2 -> x2 -> h -> (lg, Dw, Cw, Xs, Ys) ->
// u3 -> xo.  Inference hands the same few buffers to every layer (u1 = u2 = u3, x1 = x2 = xo = x, att1 = att2); training hands out the
// record's.  tmp [B M, d] is a sublayer's output before its dropout (only read under a keep mask).
struct LayerBufs {
    float *qkv, *att1, *u1, *x1, *q, *kv, *att2, *u2, *x2, *h, *lg, *Dw, *Cw, *Xs, *Ys, *u3, *xo, *tmp;
};

// The chain: queries into x0, the layers, the classifier.  bufs(l) -> LayerBufs of layer l, whose input is layer l - 1's xo (x0 for the
// first).  keep == NULL: no dropout, and exactly the launches and arithmetic of inference.  mem: the tokens, or relu(first_layer(tokens)).
template <typename Bufs>
int forward_chain(const char* who, const xmh_umoed_head* h, const float* mem, const uint8_t* keep, float p, int64_t B, int T, float* x0, Bufs&& bufs,
                  float* embeds, float* code, xmh_stream_t stream) {
    hipStream_t st = xmh::as_stream(stream);
    const int M = h->M, d = h->d, F = h->F, H = h->heads, S = h->n_experts * h->slots;
    const int64_t BM = B * M, BT = B * T;
    const MoeDims md = {B, M, d, F, h->slots, h->n_experts};
    const float ks = keep ? 1.0f / (1.0f - p) : 1.0f;
    const KeepLayout kl = keep_layout(B, T, h);
    {
        const int64_t per = (int64_t)M * d, total = BM * d;
        hipLaunchKernelGGL(k_umoed_queries, dim3(blocks_for(total)), dim3(kThreads), 0, st, h->queries, per, total, x0);
    }
    const size_t route_lds = (size_t)M * S * sizeof(float);
    if (h->moe) XMH_TRY(xmh::raise_dynamic_lds(reinterpret_cast<const void*>(k_umoed_route), route_lds, who));
    // a sublayer's output t (bias included) into u = x + dropout(t)
    auto residual = [&](const float* x, const float* t, const uint8_t* kp, float* u) {
        hipLaunchKernelGGL(k_umoed_res_drop, dim3(blocks_for(BM * d)), dim3(kThreads), 0, st, x, t, kp, ks, BM * d, u);
    };
    const float* x = x0;
    for (int l = 0; l < h->n_layers; ++l) {
        const xmh_umoed_layer& y = h->layers[l];
        const LayerBufs w = bufs(l);
        const uint8_t* kp = keep ? keep + (size_t)l * kl.layer : nullptr;
        // self-attention over the M rows
        XMH_TRY(gemm(x, d, y.sa_in_w, y.sa_in_b, nullptr, w.qkv, BM, 3 * d, XMH_ACT_NONE, stream));
        if (!kp) {
            XMH_TRY(xmh_attention_f32(w.qkv, B, M, H, 64, 0, nullptr, w.att1, stream));
            XMH_TRY(gemm(w.att1, d, y.sa_out_w, y.sa_out_b, x, w.u1, BM, d, XMH_ACT_NONE, stream));
        } else {
            hipLaunchKernelGGL(k_umoed_attn<true>, dim3((unsigned)(B * H)), dim3(kAttnThreads), attn_lds(M), st, w.qkv, (int64_t)3 * d, w.qkv + d,
                               (int64_t)3 * d, d, M, M, H, kp + kl.at[0], ks, w.att1);
            XMH_TRY(gemm(w.att1, d, y.sa_out_w, y.sa_out_b, nullptr, w.tmp, BM, d, XMH_ACT_NONE, stream));
            residual(x, w.tmp, kp + kl.at[1], w.u1);
        }
        XMH_TRY(xmh_layernorm_f32(w.u1, d, y.ln1_g, y.ln1_b, h->ln_eps, w.x1, d, BM, d, stream));
        // cross-attention: queries from x1, keys and values from mem
        XMH_TRY(gemm(w.x1, d, y.ca_in_w, y.ca_in_b, nullptr, w.q, BM, d, XMH_ACT_NONE, stream));
        XMH_TRY(gemm(mem, d, y.ca_in_w + (size_t)d * d, y.ca_in_b + d, nullptr, w.kv, BT, 2 * d, XMH_ACT_NONE, stream));
        if (!kp) {
            hipLaunchKernelGGL(k_umoed_attn<false>, dim3((unsigned)(B * H)), dim3(kAttnThreads), attn_lds(T), st, w.q, (int64_t)d, w.kv, (int64_t)2 * d, d, M, T,
                               H, nullptr, 1.0f, w.att2);
            XMH_TRY(gemm(w.att2, d, y.ca_out_w, y.ca_out_b, w.x1, w.u2, BM, d, XMH_ACT_NONE, stream));
        } else {
            hipLaunchKernelGGL(k_umoed_attn<true>, dim3((unsigned)(B * H)), dim3(kAttnThreads), attn_lds(T), st, w.q, (int64_t)d, w.kv, (int64_t)2 * d, d, M, T,
                               H, kp + kl.at[2], ks, w.att2);
            XMH_TRY(gemm(w.att2, d, y.ca_out_w, y.ca_out_b, nullptr, w.tmp, BM, d, XMH_ACT_NONE, stream));
            residual(w.x1, w.tmp, kp + kl.at[3], w.u2);
        }
        XMH_TRY(xmh_layernorm_f32(w.u2, d, y.ln2_g, y.ln2_b, h->ln_eps, w.x2, d, BM, d, stream));
        // feed-forward
        XMH_TRY(gemm(w.x2, d, y.lin_w, y.lin_b, nullptr, w.h, BM, F, XMH_ACT_RELU, stream));
        if (kp) hipLaunchKernelGGL(k_umoed_drop, dim3(blocks_for(BM * F)), dim3(kThreads), 0, st, w.h, kp + kl.at[4], ks, BM * F);
        if (!h->moe) {
            XMH_TRY(gemm(w.h, F, y.lin2_w, y.lin2_b, w.x2, w.u3, BM, d, XMH_ACT_NONE, stream));
        } else {
            launch_bmm<true, false>(st, logits_args(md, w.h, y.phi, w.lg), 1);
            hipLaunchKernelGGL(k_umoed_route, dim3((unsigned)B), dim3(kThreads), route_lds, st, w.lg, M, S, w.Dw, w.Cw);
            launch_bmm<false, false>(st, dispatch_args(md, w.Dw, w.h, w.Xs), B);
            launch_bmm<true, false>(st, experts_args(md, w.Xs, y.exp_w, y.exp_b, w.Ys), h->n_experts);
            if (!kp) {
                launch_bmm<true, false>(st, combine_args(md, w.Cw, w.Ys, w.x2, w.u3), B);
            } else {
                launch_bmm<true, false>(st, combine_args(md, w.Cw, w.Ys, nullptr, w.tmp), B);
                residual(w.x2, w.tmp, kp + kl.at[5], w.u3);
            }
        }
        XMH_TRY(xmh_layernorm_f32(w.u3, d, y.ln3_g, y.ln3_b, h->ln_eps, w.xo, d, BM, d, stream));
        x = w.xo;
    }
    hipLaunchKernelGGL(k_umoed_classify, dim3((unsigned)B), dim3(kThreads), 0, st, x, h->cls_w, h->cls_b, M, d, h->V, h->hash_func, embeds, code);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

}  // namespace umoed
}  // namespace
