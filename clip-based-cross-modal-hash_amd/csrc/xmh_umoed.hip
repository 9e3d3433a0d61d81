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
//     xmh_layernorm_f32), cross-attention 5 (gemm q, gemm k|v of mem, k_umoed_cross_attn, gemm out_proj + residual, layernorm),
//     soft-MoE 7 (gemm linear + ReLU, k_umoed_bmm logits, k_umoed_route, k_umoed_bmm dispatch, k_umoed_bmm experts, k_umoed_bmm
//     combine + residual, layernorm).  Plain: 12 (gemm linear + ReLU, gemm linear2 + residual, layernorm in place of the seven).
//   per call: 1 (k_umoed_queries) + [1 first layer] + layers x 16 (12) + 1 (k_umoed_classify): 98 at the config's six MoE layers.
//
//   k_umoed_bmm wraps the 64 x 64 tile core that k_mfma_mm wraps (xmh_mfma_mm.h: v_mfma_f32_32x32x2_f32, a 32-term chain per slab, slabs
//   in order) with a batch on grid z, a two-level row stride for the A rows and the C rows (the experts' rows (b, p) of expert n lie
//   S F apart in b and F apart in p) and bias / residual in the epilogue; the four soft-MoE products are its four argument sets.  The
//   reduction is never split, so there is one summation order.  k_umoed_cross_attn: one block per (sample, head), K and V of the head
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

namespace {

namespace mm = xmh::mm;
namespace trip = xmh::trip;
using xmh::wave_max;
using xmh::wave_sum;

constexpr int kThreads = trip::kThreads, kWaves = trip::kWaves;
constexpr int kMaxM = 128, kMaxT = 128, kMaxE = 2048, kMaxD = 1024, kMaxF = 4096, kMaxS = 256, kMaxV = 256;
constexpr int64_t kMaxRows = 32768;            // B max(M, T), the row limit of the other heads
constexpr int kMaxLossB = trip::kMaxB, kMaxC = 127;
constexpr float kEps = 1e-12f;                 // F.normalize's eps
constexpr float kUnifT = 20.0f;                // batchwise_uniformity_loss's t

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
    const float* res;         // residual, addressed as C, or NULL
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
void launch_bmm(hipStream_t st, const BmmArgs& g, int batch) {
    const dim3 grid((unsigned)((g.I + kTile - 1) / kTile), (unsigned)((g.J + kTile - 1) / kTile), (unsigned)batch);
    hipLaunchKernelGGL((k_umoed_bmm<AK, BK>), grid, dim3(kThreads), 0, st, g);
}

// ---- the learned queries, repeated over the batch --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_umoed_queries(const float* __restrict__ q, int64_t per, int64_t total, float* __restrict__ x) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e < total) x[e] = q[e % per];
}

// ---- cross-attention: q [B M, d], kv [B T, 2 d] (k | v), out [B M, d]; block (sample, head), thread = query row, dh = 64 ---------------
__global__ __launch_bounds__(128) void k_umoed_cross_attn(const float* __restrict__ q, const float* __restrict__ kv, int M, int T, int H,
                                                          float* __restrict__ out) {
    constexpr int DH = 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int D = H * DH;
    float4* sK = reinterpret_cast<float4*>(smem);                    // [T][DH / 4]; every lane reads the same address: a broadcast
    float4* sV = sK + T * (DH / 4);                                  // [T][DH / 4]
    const float* kvb = kv + (int64_t)b * T * 2 * D;
    for (int e = threadIdx.x; e < T * (DH / 4); e += blockDim.x) {
        const int j = e / (DH / 4), c4 = e % (DH / 4);
        sK[e] = *reinterpret_cast<const float4*>(kvb + (int64_t)j * 2 * D + h * DH + c4 * 4);
        sV[e] = *reinterpret_cast<const float4*>(kvb + (int64_t)j * 2 * D + D + h * DH + c4 * 4);
    }
    __syncthreads();
    const int i = threadIdx.x;
    if (i >= M) return;
    const int64_t row = (int64_t)b * M + i;
    float qr[DH];
    const float scale = rsqrtf((float)DH);
#pragma unroll
    for (int c = 0; c < DH / 4; ++c) {                               // PyTorch scales q before Q K^T
        const float4 v = *reinterpret_cast<const float4*>(q + row * D + h * DH + c * 4);
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
    for (int j = 0; j < T; ++j) {
        const float p = expf(score(j) - mx);                         // the same chain as in the first pass: the largest is exp(0)
        sum += p;
#pragma unroll
        for (int c = 0; c < DH / 4; ++c) {
            const float4 vv = sV[j * (DH / 4) + c];
            o[4 * c + 0] = fmaf(p, vv.x, o[4 * c + 0]);
            o[4 * c + 1] = fmaf(p, vv.y, o[4 * c + 1]);
            o[4 * c + 2] = fmaf(p, vv.z, o[4 * c + 2]);
            o[4 * c + 3] = fmaf(p, vv.w, o[4 * c + 3]);
        }
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int c = 0; c < DH / 4; ++c)
        *reinterpret_cast<float4*>(out + row * D + h * DH + c * 4) = make_float4(o[4 * c + 0] * inv, o[4 * c + 1] * inv, o[4 * c + 2] * inv, o[4 * c + 3] * inv);
}

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

bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// 0: fine; otherwise the status, with the text set when `who` is given
int head_shape(const char* who, int64_t B, int T, const xmh_umoed_head* h) {
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

int gemm(const float* A, int64_t K, const float* W, const float* bias, const float* res, float* Cm, int64_t rows, int64_t N, int act, xmh_stream_t s) {
    return xmh_gemm_nt_f32(A, K, W, K, bias, res, N, Cm, N, rows, N, K, act, XMH_PREC_F32, s);
}

}  // namespace

extern "C" size_t xmh_head_umoed_bytes(int64_t B, int T, const xmh_umoed_head* h) {
    if (head_shape(nullptr, B, T, h)) return 0;
    return head_layout(B, T, h, nullptr, nullptr);
}

extern "C" int xmh_head_umoed(const xmh_umoed_head* h, const float* tokens, int64_t B, int T, float* embeds, float* code, void* ws, size_t ws_bytes,
                              xmh_stream_t stream) {
    XMH_RANGE("xmh_head_umoed");
    const char* who = "xmh_head_umoed";
    if (int rc = head_shape(who, B, T, h)) return rc;
    if (!tokens || !embeds || !code || !ws || !h->layers || !h->queries || !h->cls_w || !h->cls_b || (h->first_w && !h->first_b))
        return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    for (int l = 0; l < h->n_layers; ++l) {
        const xmh_umoed_layer& y = h->layers[l];
        const bool common = y.ln1_g && y.ln1_b && y.sa_in_w && y.sa_in_b && y.sa_out_w && y.sa_out_b && y.ln2_g && y.ln2_b && y.ca_in_w && y.ca_in_b &&
                            y.ca_out_w && y.ca_out_b && y.ln3_g && y.ln3_b && y.lin_w && y.lin_b;
        if (!common || (h->moe ? !(y.phi && y.exp_w && y.exp_b) : !(y.lin2_w && y.lin2_b)))
            return xmh::fail(XMH_EINVAL, "%s: null pointer in layer %d", who, l);
    }
    XMH_TRY(xmh::check_workspace(who, ws, ws_bytes, head_layout(B, T, h, nullptr, nullptr), "xmh_head_umoed_bytes", XMH_ENOMEM));
    HeadWs w;
    head_layout(B, T, h, ws, &w);
    hipStream_t st = xmh::as_stream(stream);
    const int M = h->M, d = h->d, F = h->F, H = h->heads, P = h->slots, S = h->n_experts * h->slots;
    const int64_t BM = B * M, BT = B * T;

    const float* mem = tokens;
    if (h->first_w) {
        XMH_TRY(gemm(tokens, h->E, h->first_w, h->first_b, nullptr, w.mem, BT, d, XMH_ACT_RELU, stream));
        mem = w.mem;
    }
    {
        const int64_t per = (int64_t)M * d, total = BM * d;
        hipLaunchKernelGGL(k_umoed_queries, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, h->queries, per, total, w.x);
    }
    const size_t attn_lds = (size_t)2 * T * 64 * sizeof(float), route_lds = (size_t)M * S * sizeof(float);
    if (h->moe) XMH_TRY(xmh::raise_dynamic_lds(reinterpret_cast<const void*>(k_umoed_route), route_lds, who));
    for (int l = 0; l < h->n_layers; ++l) {
        const xmh_umoed_layer& y = h->layers[l];
        // self-attention over the M rows
        XMH_TRY(gemm(w.x, d, y.sa_in_w, y.sa_in_b, nullptr, w.qkv, BM, 3 * d, XMH_ACT_NONE, stream));
        XMH_TRY(xmh_attention_f32(w.qkv, B, M, H, 64, 0, nullptr, w.att, stream));
        XMH_TRY(gemm(w.att, d, y.sa_out_w, y.sa_out_b, w.x, w.y, BM, d, XMH_ACT_NONE, stream));
        XMH_TRY(xmh_layernorm_f32(w.y, d, y.ln1_g, y.ln1_b, h->ln_eps, w.x, d, BM, d, stream));
        // cross-attention: queries from x, keys and values from mem
        XMH_TRY(gemm(w.x, d, y.ca_in_w, y.ca_in_b, nullptr, w.q, BM, d, XMH_ACT_NONE, stream));
        XMH_TRY(gemm(mem, d, y.ca_in_w + (size_t)d * d, y.ca_in_b + d, nullptr, w.kv, BT, 2 * d, XMH_ACT_NONE, stream));
        hipLaunchKernelGGL(k_umoed_cross_attn, dim3((unsigned)(B * H)), dim3(128), attn_lds, st, w.q, w.kv, M, T, H, w.att);
        XMH_TRY(gemm(w.att, d, y.ca_out_w, y.ca_out_b, w.x, w.y, BM, d, XMH_ACT_NONE, stream));
        XMH_TRY(xmh_layernorm_f32(w.y, d, y.ln2_g, y.ln2_b, h->ln_eps, w.x, d, BM, d, stream));
        // feed-forward
        XMH_TRY(gemm(w.x, d, y.lin_w, y.lin_b, nullptr, w.h, BM, F, XMH_ACT_RELU, stream));
        if (!h->moe) {
            XMH_TRY(gemm(w.h, F, y.lin2_w, y.lin2_b, w.x, w.y, BM, d, XMH_ACT_NONE, stream));
        } else {
            BmmArgs g = {};
            g.adiv = g.cdiv = INT_MAX;
            g.A = w.h, g.sai = F, g.sak = 1;                                     // logits [B M, S] = h phi
            g.B = y.phi, g.sbj = 1, g.sbk = S;
            g.I = (int)BM, g.J = S, g.Kd = F;
            g.C = w.lg, g.sci = S;
            launch_bmm<true, false>(st, g, 1);
            hipLaunchKernelGGL(k_umoed_route, dim3((unsigned)B), dim3(kThreads), route_lds, st, w.lg, M, S, w.Dw, w.Cw);
            g = BmmArgs{};
            g.adiv = g.cdiv = INT_MAX;
            g.A = w.Dw, g.sai = 1, g.sak = S, g.sab = (int64_t)M * S;            // Xs[b] [S, F] = D[b]^T h[b]
            g.B = w.h, g.sbj = 1, g.sbk = F, g.sbb = (int64_t)M * F;
            g.I = S, g.J = F, g.Kd = M;
            g.C = w.Xs, g.sci = F, g.scb = (int64_t)S * F;
            launch_bmm<false, false>(st, g, (int)B);
            g = BmmArgs{};
            g.A = w.Xs, g.sai = F, g.sak = 1, g.sab = (int64_t)P * F, g.adiv = P, g.sah = (int64_t)S * F;      // rows (b, p) of expert n
            g.B = y.exp_w, g.sbj = 1, g.sbk = d, g.sbb = (int64_t)F * d;         // W_n [F, d], "in, out"
            g.I = (int)(B * P), g.J = d, g.Kd = F;
            g.C = w.Ys, g.sci = d, g.scb = (int64_t)P * d, g.cdiv = P, g.sch = (int64_t)S * d;
            g.bias = y.exp_b, g.sbias = d;
            launch_bmm<true, false>(st, g, h->n_experts);
            g = BmmArgs{};
            g.adiv = g.cdiv = INT_MAX;
            g.A = w.Cw, g.sai = S, g.sak = 1, g.sab = (int64_t)M * S;            // y[b] = x[b] + Cw[b] Ys[b]
            g.B = w.Ys, g.sbj = 1, g.sbk = d, g.sbb = (int64_t)S * d;
            g.I = M, g.J = d, g.Kd = S;
            g.C = w.y, g.sci = d, g.scb = (int64_t)M * d;
            g.res = w.x;
            launch_bmm<true, false>(st, g, (int)B);
        }
        XMH_TRY(xmh_layernorm_f32(w.y, d, y.ln3_g, y.ln3_b, h->ln_eps, w.x, d, BM, d, stream));
    }
    hipLaunchKernelGGL(k_umoed_classify, dim3((unsigned)B), dim3(kThreads), 0, st, w.x, h->cls_w, h->cls_b, M, d, h->V, h->hash_func, embeds, code);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
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
