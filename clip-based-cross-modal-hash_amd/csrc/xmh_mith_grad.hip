// Training forward and backward of one modality of MITH's hash head (models/MITH/hash/hash.py:231-247).  Exact fp32
// throughout, for the reason xmh_block_grad.hip gives.  The token transformer runs through xmh_clip_blocks_forward_saved /
// xmh_clip_blocks_backward, the products, bias sums and LayerNorm backward are the kernels of xmh_grad_kernels.hip, the forward's
// LayerNorm, products and bitwise hash are the calls of xmh_head_mith in exact mode (same bits), and the LTA body is xmh_lta.h.
//
//   forward   cls path, kept per residual MLP: x_in | ln | fc_pre | fc_act (fc_pre from a second, epilogue-free product of the B
//             rows: the fused GELU product alone keeps the eval path's bits but not the pre-activation) -> y -> tanh(y Wc^T) (kept),
//             y / max(|y|, eps)
//             token scores: the same chain on the B L token rows in the workspace, nothing kept (detached in the reference)
//             k_lta_aggregate_saved: M = A X + pe, A [B, K, L] kept -> blocks, saved -> z (kept) -> xmh_bitwise_hash (kept)
//             p = z Wp^T + bp (kept) -> k_l2norm_fwd -> trans_tokens [K, B, D]
//   backward  k_l2norm_bwd dp (rows read in KND order) -> TN dWp, dbp -> NN dz = dp Wp
//             k_hash_bwd   dz (+)= g (1 - t^2) w_k; dw_k, db_k = sums over b in index order, in double
//             xmh_clip_blocks_backward: dz -> dM in place
//             k_lta_bwd    d_tokens[b,l,:] = sum_k A[b,k,l] dM[b,k,:]  (k in index order)
//             cls path: k_tanh_bwd -> TN dWc -> NN dy = gt Wc; k_l2norm_bwd dy += ...; per residual MLP from the top:
//             TN dW2, db2 -> NN -> k_gelu_erf_bwd -> TN dW1, db1 -> NN -> LayerNorm backward (dy += ..., dgamma, dbeta)
// No host synchronisation, no allocation, no float atomics; every sum has one fixed order.
#include "xmh_clip_record.h"
#include "xmh_grad_kernels.h"
#include "xmh_lta.h"

namespace {

using namespace xmh::grad;
using xmh::wave_sum;

constexpr int kMaxWidth = 1024;                  // the forward's LayerNorm kernel holds a row in 16 registers per lane
constexpr int kMaxRes = 4;
constexpr float kNormEps = 1e-12f;               // F.normalize's default

__global__ __launch_bounds__(256) void k_lta_aggregate_saved(const float* __restrict__ S, const float* __restrict__ X,
                                                             const uint8_t* __restrict__ mask, const float* __restrict__ pe,
                                                             float* __restrict__ M, float* __restrict__ A, int L, int K, int D, int topk) {
    extern __shared__ __attribute__((aligned(16))) float sm_lta[];
    xmh::lta_aggregate_block<true>(sm_lta, S, X, mask, pe, M, A, L, K, D, topk);
}

// d_tokens[b,l,:] = sum_k A[b,k,l] dM[b,k,:].  grid (B, ceil(D / 64)): A of the sample in LDS ([K][L], every read a broadcast: the
// four waves of a block own a quarter of the token groups each), thread = (column, token group), 16 tokens at a time in registers
// -- the forward's aggregation with the roles of l and k exchanged.  A is an exact zero where a token was not kept, so its row is.
__global__ __launch_bounds__(kThreads) void k_lta_bwd(const float* __restrict__ A, const float* __restrict__ dM, float* __restrict__ dT, int L,
                                                      int K, int D) {
    extern __shared__ __attribute__((aligned(16))) float sA[];
    const int b = blockIdx.x;
    for (int e = threadIdx.x; e < K * L; e += kThreads) sA[e] = A[(int64_t)b * K * L + e];
    __syncthreads();
    const int d = blockIdx.y * 64 + (threadIdx.x & 63);
    const int lq = threadIdx.x >> 6;
    if (d >= D) return;
    for (int l0 = lq * 16; l0 < L; l0 += 64) {
        float acc[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc[u] = 0.0f;
        for (int k = 0; k < K; ++k) {
            const float x = dM[((int64_t)b * K + k) * D + d];
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (l0 + u < L) acc[u] = fmaf(sA[k * L + l0 + u], x, acc[u]);
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (l0 + u < L) dT[((int64_t)b * L + l0 + u) * D + d] = acc[u];
    }
}

// where row r = (b, k) of a [B, K, D] tensor sits in the [K, B, D] layout the loss takes (K == 0: the same row)
__device__ __forceinline__ int64_t knd_row(int64_t r, int64_t B, int K) { return K ? (r % K) * B + r / K : r; }

// out[row] = x[row] / max(|x[row]|, eps), one wave per row (F.normalize)
__global__ __launch_bounds__(kThreads) void k_l2norm_fwd(const float* __restrict__ x, float* __restrict__ out, int64_t rows, int D, int64_t B,
                                                         int K) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * D;
    float ss = 0.0f;
    for (int e = lane; e < D; e += 64) ss = fmaf(xr[e], xr[e], ss);
    const float den = fmaxf(sqrtf(wave_sum(ss)), kNormEps);
    float* o = out + knd_row(row, B, K) * D;
    for (int e = lane; e < D; e += 64) o[e] = xr[e] / den;
}

// backward of the above from the saved input x: n = x / |x|, dx = (g - n (n . g)) / |x|; a row the eps clamps gets g / eps, as
// autograd's.  g is read at the row's place in the [K, B, D] layout.  add: dx is added to what out holds.
__global__ __launch_bounds__(kThreads) void k_l2norm_bwd(const float* __restrict__ x, const float* __restrict__ g, float* out, int64_t rows, int D,
                                                         int64_t B, int K, int add) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * D;
    const float* gr = g + knd_row(row, B, K) * D;
    double ss = 0.0, dot = 0.0;
    for (int e = lane; e < D; e += 64) {
        ss += (double)xr[e] * (double)xr[e];
        dot += (double)xr[e] * (double)gr[e];
    }
    const double nrm = sqrt(wave_sum(ss));
    dot = wave_sum(dot);
    float* o = out + row * D;
    const bool clamped = !(nrm > (double)kNormEps);
    const double inv = clamped ? 1.0 / (double)kNormEps : 1.0 / nrm, c = clamped ? 0.0 : dot / (nrm * nrm);
    for (int e = lane; e < D; e += 64) {
        const float v = (float)(((double)gr[e] - (double)xr[e] * c) * inv);
        o[e] = add ? o[e] + v : v;
    }
}

// gt = g (1 - t^2): backward of a tanh epilogue from its output
__global__ __launch_bounds__(kThreads) void k_tanh_bwd(const float* __restrict__ g, const float* __restrict__ t, float* __restrict__ gt, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e < n) gt[e] = g[e] * fmaf(-t[e], t[e], 1.0f);
}

// d *= GELU'(pre), the exact erf form: Phi(x) + x phi(x)
__global__ __launch_bounds__(kThreads) void k_gelu_erf_bwd(float* __restrict__ d, const float* __restrict__ pre, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const float x = pre[e];
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
    d[e] *= fmaf(x, pdf, cdf);
}

// Bitwise hashing backward, one concept per blockIdx.x and 256 columns per blockIdx.y: gt = g (1 - t^2);
// dz[b,k,:] (+)= gt w_k (dz may be NULL); dw_k = sum_b gt z[b,k,:], db_k = sum_b gt, b in index order, in double.
__global__ __launch_bounds__(kThreads) void k_hash_bwd(const float* __restrict__ g, const float* __restrict__ t, const float* __restrict__ z,
                                                       const float* __restrict__ w, float* dz, int add, float* dw, float* db, int accumulate,
                                                       int64_t B, int K, int D) {
    const int k = blockIdx.x;
    const int d = blockIdx.y * kThreads + threadIdx.x;
    if (d < D) {
        const float wv = w[(int64_t)k * D + d];
        double acc = 0.0;
        for (int64_t b = 0; b < B; ++b) {
            const float tv = t[b * K + k];
            const float gt = g[b * K + k] * fmaf(-tv, tv, 1.0f);
            const int64_t at = (b * K + k) * D + d;
            if (dz) dz[at] = add ? fmaf(gt, wv, dz[at]) : gt * wv;
            acc += (double)gt * (double)z[at];
        }
        if (dw) dw[(int64_t)k * D + d] = accumulate ? dw[(int64_t)k * D + d] + (float)acc : (float)acc;
    }
    if (db && blockIdx.y == 0 && threadIdx.x == 0) {
        double s = 0.0;
        for (int64_t b = 0; b < B; ++b) {
            const float tv = t[b * K + k];
            s += (double)(g[b * K + k] * fmaf(-tv, tv, 1.0f));
        }
        db[k] = accumulate ? db[k] + (float)s : (float)s;
    }
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }
unsigned row_blocks(int64_t rows) { return (unsigned)((rows + kThreads / 64 - 1) / (kThreads / 64)); }

struct Shape {
    int D, K, R, layers, heads;
};

// what a forward keeps beside the block record.  x[i] is the stream entering residual MLP i (x[0] is the caller's cls, not kept),
// x[R] = y.
struct Kept {
    float* record;
    size_t record_bytes;
    float *x[kMaxRes + 1], *ln[kMaxRes], *fc_pre[kMaxRes], *fc_act[kMaxRes];
    float *ch, *th;   // [B, K]    cls_hash, tokens_hash
    float* A;         // [B, K, L]
    float* z;         // [B, K, D] the blocks' output
    float* p;         // [B, K, D] z Wp^T + bp
};

void kept_small(xmh::Arena& ar, int64_t B, int L, const Shape& s, Kept* v) {
    const size_t bd = (size_t)B * s.D;
    v->x[0] = nullptr;
    for (int i = 0; i < s.R; ++i) {
        v->x[i + 1] = ar.take<float>(bd);
        v->ln[i] = ar.take<float>(bd);
        v->fc_pre[i] = ar.take<float>(4 * bd);
        v->fc_act[i] = ar.take<float>(4 * bd);
    }
    v->ch = ar.take<float>((size_t)B * s.K);
    v->th = ar.take<float>((size_t)B * s.K);
    v->A = ar.take<float>((size_t)B * s.K * L);
    v->z = ar.take<float>(bd * s.K);
    v->p = ar.take<float>(bd * s.K);
}

size_t kept_layout(int64_t B, int L, const Shape& s, void* base, Kept* k) {
    xmh::Arena ar(base);
    Kept v = {};
    v.record_bytes = xmh::saved_record_bytes(s.layers, B * s.K, s.D);
    v.record = ar.take<float>(v.record_bytes / sizeof(float));
    kept_small(ar, B, L, s, &v);
    if (k) *k = v;
    return ar.used;
}

// one workspace for the forward and the backward
struct Work {
    GradScratch gs;
    float *ty, *thb, *tf, *scores;   // forward: the token rows' chain, [M, D], [M, D], [M, 4D], [M, K]
    float *dz, *dp;                  // [B, K, D]
    float *dy, *t1, *t4, *gt;        // [B, D], [B, D], [B, 4D], [B, K]
    char* blocks;                    // scratch of the block stack's forward / workspace of its backward
    size_t blocks_bytes;
    Kept kept;                       // a forward without a record keeps its small tensors here
};

size_t work_layout(int64_t B, int L, const Shape& s, void* base, Work* w) {
    xmh::Arena ar(base);
    Work v = {};
    const int64_t M = B * L;
    const int D = s.D;
    const size_t bd = (size_t)B * D;
    if (s.R > 0) {
        v.ty = ar.take<float>((size_t)M * D);
        v.thb = ar.take<float>((size_t)M * D);
        v.tf = ar.take<float>((size_t)M * D * 4);
    }
    v.scores = ar.take<float>((size_t)M * s.K);
    v.dz = ar.take<float>(bd * s.K);
    v.dp = ar.take<float>(bd * s.K);
    v.dy = ar.take<float>(bd);
    v.t1 = ar.take<float>(bd);
    v.t4 = ar.take<float>(4 * bd);
    v.gt = ar.take<float>((size_t)B * s.K);
    const TnShape tn[] = {{B * s.K, D, D}, {B, s.K, D}, {B, D, 4 * D}, {B, 4 * D, D}};
    take_scratch(ar, B, D, 4 * D, tn, &v.gs);
    const size_t fwd = xmh_clip_workspace_bytes(B, s.K, D, 0, 0, 2), bwd = xmh_clip_blocks_backward_ws_bytes(B, s.K, D);
    v.blocks_bytes = fwd > bwd ? fwd : bwd;
    v.blocks = ar.take<char>(v.blocks_bytes);
    kept_small(ar, B, L, s, &v.kept);
    if (w) *w = v;
    return ar.used;
}

bool limits_ok(int64_t B, int L, int D, int K, int R) {
    return L > 0 && K > 0 && R >= 0 && R <= kMaxRes && D <= kMaxWidth && stack_limits_ok(B, K, D) && B * L <= kMaxRows &&
           xmh::lta_lds_bytes(L, K) <= xmh::kLtaMaxLds;
}

// the descriptor and the batch against the limits; fills s
int head_shape(const char* who, const xmh_mith_train* t, int64_t B, int L, Shape* s) {
    const xmh_mith_head& h = t->head;
    const int D = h.width, K = h.k_bits;
    if (D <= 0 || K <= 0 || L <= 0 || h.heads <= 0 || D % h.heads || h.res_layers < 0 || h.layers < 0 || h.top_k <= 0 || h.top_k > K ||
        h.concept.n != K || h.concept.k != D || t->proj.n != D || t->proj.k != D)
        return xmh::fail(XMH_EINVAL, "%s: head shapes do not fit (width %d, %d bits, %d heads, top_k %d)", who, D, K, h.heads, h.top_k);
    if (D % 4 || D > kMaxWidth) return xmh::fail(XMH_ENOTSUP, "%s: width %d (a multiple of 4, at most %d)", who, D, kMaxWidth);
    XMH_TRY(check_stack_limits(who, B, K, D, h.heads));      // the transformer's sequence is the K concepts
    if (h.res_layers > kMaxRes) return xmh::fail(XMH_ENOTSUP, "%s: %d residual MLPs (at most %d)", who, h.res_layers, kMaxRes);
    if (B * L > kMaxRows) return xmh::fail(XMH_ENOTSUP, "%s: %lld x %d tokens (at most 2^21)", who, (long long)B, L);
    if (xmh::lta_lds_bytes(L, K) > xmh::kLtaMaxLds) return xmh::fail(XMH_ENOTSUP, "%s: L (K + 2) = %d x %d exceeds the LDS", who, L, K + 2);
    if (!h.concept.w_f32 || !h.hash_w || !h.hash_b || !h.pos_enc || !t->proj.w_f32 || !t->proj.bias || (h.res_layers > 0 && !h.mlps) ||
        (h.layers > 0 && !h.blocks))
        return xmh::fail(XMH_EINVAL, "%s: the head lacks fp32 weights", who);
    for (int i = 0; i < h.res_layers; ++i) {
        const xmh_mith_mlp& m = h.mlps[i];
        if (m.fc1.k != D || m.fc1.n != 4 * D || m.fc2.n != D || m.fc2.k != 4 * D)
            return xmh::fail(XMH_EINVAL, "%s: MLP %d shapes do not fit width %d", who, i, D);
        if (!m.ln_w || !m.ln_b || !m.fc1.w_f32 || !m.fc1.bias || !m.fc2.w_f32 || !m.fc2.bias)
            return xmh::fail(XMH_EINVAL, "%s: MLP %d lacks fp32 weights", who, i);
        if (m.ln_eps != kLnEps) return xmh::fail(XMH_ENOTSUP, "%s: MLP %d LayerNorm eps %g (only 1e-5)", who, i, (double)m.ln_eps);
    }
    *s = Shape{D, K, h.res_layers, h.layers, h.heads};
    return XMH_OK;
}

int gemm(const xmh_linear& l, const float* a, const float* residual, float* c, int64_t rows, int act, xmh_stream_t st) {
    return xmh_gemm_nt_f32(a, l.k, l.w_f32, l.k, l.bias, residual, residual ? l.n : 0, c, l.n, rows, l.n, l.k, act, 0, st);
}

// a gradient whose path has no upstream: exact zeros, unless it is added to
int zero(hipStream_t st, float* p, size_t n, int accumulate) {
    if (p && !accumulate) XMH_HIP(hipMemsetAsync(p, 0, n * sizeof(float), st));
    return XMH_OK;
}

int zero_block(hipStream_t st, const xmh_clip_block_grads& g, size_t D, int accumulate) {
    float* const p[] = {g.ln1_w, g.ln1_b, g.qkv_w, g.qkv_b, g.out_w, g.out_b, g.ln2_w, g.ln2_b, g.fc_w, g.fc_b, g.proj_w, g.proj_b};
    const size_t n[] = {D, D, 3 * D * D, 3 * D, D * D, D, D, D, 4 * D * D, 4 * D, 4 * D * D, D};
    for (int i = 0; i < 12; ++i) XMH_TRY(zero(st, p[i], n[i], accumulate));
    return XMH_OK;
}

bool mlp_asked(const xmh_mith_mlp_grads& g) { return g.ln_w || g.ln_b || g.fc1_w || g.fc1_b || g.fc2_w || g.fc2_b; }

}  // namespace

extern "C" size_t xmh_mith_train_saved_bytes(int64_t B, int L, int width, int k_bits, int res_layers, int layers) {
    if (!limits_ok(B, L, width, k_bits, res_layers) || layers < 0) return 0;
    return kept_layout(B, L, Shape{width, k_bits, res_layers, layers, 0}, nullptr, nullptr);
}

extern "C" size_t xmh_mith_train_ws_bytes(int64_t B, int L, int width, int k_bits, int res_layers) {
    if (!limits_ok(B, L, width, k_bits, res_layers)) return 0;
    return work_layout(B, L, Shape{width, k_bits, res_layers, 0, 0}, nullptr, nullptr);
}

extern "C" int xmh_mith_train_forward(const xmh_mith_train* t, const float* cls, const float* tokens, const uint8_t* token_mask, int64_t B, int L,
                                      float* res_cls, float* cls_hash, float* tokens_hash, float* trans_tokens, void* saved, size_t saved_bytes,
                                      void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_mith_train_forward");
    const char* who = "xmh_mith_train_forward";
    if (B == 0) return XMH_OK;
    if (B < 0 || !t || !cls || !tokens || !res_cls || !cls_hash || !tokens_hash || !trans_tokens || !workspace)
        return xmh::fail(XMH_EINVAL, "%s: bad arguments", who);
    Shape s;
    XMH_TRY(head_shape(who, t, B, L, &s));
    Kept kp;
    if (saved) {
        const size_t kneed = kept_layout(B, L, s, saved, &kp);
        if (saved_bytes < kneed) return xmh::fail(XMH_ENOMEM, "%s: saved buffer of %zu bytes, %zu needed", who, saved_bytes, kneed);
    }
    Work wk;
    const size_t wneed = work_layout(B, L, s, workspace, &wk);
    if (workspace_bytes < wneed) return xmh::fail(XMH_ENOMEM, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, wneed);
    if (!saved) kp = wk.kept;
    const xmh_mith_head& h = t->head;
    const int D = s.D, K = s.K;
    const int64_t M = B * L;
    hipStream_t st = xmh::as_stream(stream);
    // the cls path, every intermediate kept
    const float* cur = cls;
    for (int i = 0; i < s.R; ++i) {
        const xmh_mith_mlp& m = h.mlps[i];
        XMH_TRY(xmh_layernorm_f32(cur, D, m.ln_w, m.ln_b, kLnEps, kp.ln[i], D, B, D, stream));
        XMH_TRY(gemm(m.fc1, kp.ln[i], nullptr, kp.fc_pre[i], B, XMH_ACT_NONE, stream));
        XMH_TRY(gemm(m.fc1, kp.ln[i], nullptr, kp.fc_act[i], B, XMH_ACT_GELU_ERF, stream));
        XMH_TRY(gemm(m.fc2, kp.fc_act[i], cur, kp.x[i + 1], B, XMH_ACT_NONE, stream));
        cur = kp.x[i + 1];
    }
    XMH_TRY(gemm(h.concept, cur, nullptr, kp.ch, B, XMH_ACT_TANH, stream));
    XMH_HIP(hipMemcpyAsync(cls_hash, kp.ch, (size_t)B * K * sizeof(float), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_l2norm_fwd, dim3(row_blocks(B)), dim3(kThreads), 0, st, cur, res_cls, B, D, B, 0);
    // concept scores of every token: xmh_head_mith's chain in exact mode
    cur = tokens;
    for (int i = 0; i < s.R; ++i) {
        const xmh_mith_mlp& m = h.mlps[i];
        XMH_TRY(xmh_layernorm_f32(cur, D, m.ln_w, m.ln_b, kLnEps, wk.thb, D, M, D, stream));
        XMH_TRY(gemm(m.fc1, wk.thb, nullptr, wk.tf, M, XMH_ACT_GELU_ERF, stream));
        XMH_TRY(gemm(m.fc2, wk.tf, cur, wk.ty, M, XMH_ACT_NONE, stream));
        cur = wk.ty;
    }
    XMH_TRY(gemm(h.concept, cur, nullptr, wk.scores, M, XMH_ACT_TANH, stream));
    const size_t lds = xmh::lta_lds_bytes(L, K);
    XMH_TRY(xmh::raise_dynamic_lds(reinterpret_cast<const void*>(k_lta_aggregate_saved), lds, who));
    hipLaunchKernelGGL(k_lta_aggregate_saved, dim3((unsigned)B, (unsigned)xmh::ceil_div(D, 64)), dim3(256), lds, st, wk.scores, tokens, token_mask,
                       h.pos_enc, kp.z, kp.A, L, K, D, h.top_k);
    if (s.layers > 0) {
        if (saved)
            XMH_TRY(xmh_clip_blocks_forward_saved(h.blocks, s.layers, D, s.heads, kp.z, B, K, 0, nullptr, 2, wk.blocks, wk.blocks_bytes, kp.record,
                                                  kp.record_bytes, stream));
        else
            XMH_TRY(xmh_clip_blocks_forward(h.blocks, s.layers, D, s.heads, kp.z, B, K, 0, nullptr, 2, wk.blocks, wk.blocks_bytes, stream));
    }
    XMH_TRY(xmh_bitwise_hash(kp.z, h.hash_w, h.hash_b, nullptr, kp.th, B, K, D, stream));
    XMH_HIP(hipMemcpyAsync(tokens_hash, kp.th, (size_t)B * K * sizeof(float), hipMemcpyDeviceToDevice, st));
    XMH_TRY(gemm(t->proj, kp.z, nullptr, kp.p, B * K, XMH_ACT_NONE, stream));
    hipLaunchKernelGGL(k_l2norm_fwd, dim3(row_blocks(B * K)), dim3(kThreads), 0, st, kp.p, trans_tokens, B * K, D, B, K);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

extern "C" int xmh_mith_train_backward(const xmh_mith_train* t, const float* cls, int64_t B, int L, const float* g_res_cls, const float* g_cls_hash,
                                       const float* g_tokens_hash, const float* g_trans_tokens, const void* saved, size_t saved_bytes,
                                       const xmh_mith_grads* grads, int accumulate, void* workspace, size_t workspace_bytes,
                                       xmh_stream_t stream) {
    XMH_RANGE("xmh_mith_train_backward");
    const char* who = "xmh_mith_train_backward";
    if (B == 0) return XMH_OK;
    if (B < 0 || !t || !cls || !saved || !grads || !workspace) return xmh::fail(XMH_EINVAL, "%s: bad arguments", who);
    Shape s;
    XMH_TRY(head_shape(who, t, B, L, &s));
    const xmh_mith_grads& gr = *grads;
    if ((s.R > 0 && !gr.mlps) || (s.layers > 0 && !gr.blocks)) return xmh::fail(XMH_EINVAL, "%s: null MLP / block gradients", who);
    Kept kp;
    const size_t kneed = kept_layout(B, L, s, const_cast<void*>(saved), &kp);
    if (saved_bytes < kneed) return xmh::fail(XMH_ENOMEM, "%s: saved buffer of %zu bytes, %zu needed", who, saved_bytes, kneed);
    Work wk;
    const size_t wneed = work_layout(B, L, s, workspace, &wk);
    if (workspace_bytes < wneed) return xmh::fail(XMH_ENOMEM, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, wneed);
    const xmh_mith_head& h = t->head;
    const int D = s.D, K = s.K;
    const int64_t BK = B * K;
    const size_t dd = (size_t)D * D;
    hipStream_t st = xmh::as_stream(stream);

    // ---- the token path: trans_tokens and tokens_hash -> z -> blocks -> M -> tokens ----
    bool blocks_asked = false;
    for (int i = 0; i < s.layers; ++i) blocks_asked = blocks_asked || block_asked(gr.blocks[i]);
    const bool need_dz = gr.d_tokens || blocks_asked;
    if (g_trans_tokens && (gr.proj_w || gr.proj_b || need_dz)) {
        hipLaunchKernelGGL(k_l2norm_bwd, dim3(row_blocks(BK)), dim3(kThreads), 0, st, kp.p, g_trans_tokens, wk.dp, BK, D, B, K, 0);
        weight_grads(st, wk.gs, wk.dp, kp.z, BK, D, D, gr.proj_w, gr.proj_b, accumulate);
        if (need_dz) launch_nn(st, wk.dp, t->proj.w_f32, BK, D, D, wk.dz, nullptr);
    } else if (!g_trans_tokens) {
        XMH_TRY(zero(st, gr.proj_w, dd, accumulate));
        XMH_TRY(zero(st, gr.proj_b, D, accumulate));
    }
    if (g_tokens_hash && (gr.hash_w || gr.hash_b || need_dz)) {
        hipLaunchKernelGGL(k_hash_bwd, dim3(K, (D + kThreads - 1) / kThreads), dim3(kThreads), 0, st, g_tokens_hash, kp.th, kp.z, h.hash_w,
                           need_dz ? wk.dz : nullptr, g_trans_tokens ? 1 : 0, gr.hash_w, gr.hash_b, accumulate, B, K, D);
    } else if (!g_tokens_hash) {
        XMH_TRY(zero(st, gr.hash_w, (size_t)K * D, accumulate));
        XMH_TRY(zero(st, gr.hash_b, K, accumulate));
    }
    if (!g_trans_tokens && !g_tokens_hash) {
        for (int i = 0; i < s.layers; ++i) XMH_TRY(zero_block(st, gr.blocks[i], D, accumulate));
        XMH_TRY(zero(st, gr.d_tokens, (size_t)B * L * D, 0));
    } else if (need_dz) {
        if (s.layers > 0)
            XMH_TRY(xmh_clip_blocks_backward(h.blocks, s.layers, D, s.heads, B, K, 0, nullptr, kp.record, kp.record_bytes, wk.dz, gr.d_tokens ? 1 : 0,
                                             gr.blocks, accumulate, wk.blocks, wk.blocks_bytes, stream));
        if (gr.d_tokens) {
            const size_t lds = (size_t)K * L * sizeof(float);
            XMH_TRY(xmh::raise_dynamic_lds(reinterpret_cast<const void*>(k_lta_bwd), lds, who));
            hipLaunchKernelGGL(k_lta_bwd, dim3((unsigned)B, (unsigned)xmh::ceil_div(D, 64)), dim3(kThreads), lds, st, kp.A, wk.dz, gr.d_tokens, L, K, D);
        }
    }

    // ---- the cls path: res_cls and cls_hash -> y -> residual MLPs -> cls ----
    bool mlps_asked = false;
    for (int i = 0; i < s.R; ++i) mlps_asked = mlps_asked || mlp_asked(gr.mlps[i]);
    const float* y = s.R > 0 ? kp.x[s.R] : cls;
    if (!g_res_cls && !g_cls_hash) {
        XMH_TRY(zero(st, gr.concept, (size_t)K * D, accumulate));
        for (int i = 0; i < s.R; ++i) {
            const xmh_mith_mlp_grads& g = gr.mlps[i];
            XMH_TRY(zero(st, g.ln_w, D, accumulate));
            XMH_TRY(zero(st, g.ln_b, D, accumulate));
            XMH_TRY(zero(st, g.fc1_w, 4 * dd, accumulate));
            XMH_TRY(zero(st, g.fc1_b, 4 * (size_t)D, accumulate));
            XMH_TRY(zero(st, g.fc2_w, 4 * dd, accumulate));
            XMH_TRY(zero(st, g.fc2_b, D, accumulate));
        }
        XMH_TRY(zero(st, gr.d_cls, (size_t)B * D, 0));
        XMH_LAUNCH_CHECK(who);
        return XMH_OK;
    }
    const bool need_dy = gr.d_cls || mlps_asked;
    float* dy = gr.d_cls ? gr.d_cls : wk.dy;                  // the gradient of the stream, walked down in place
    if (g_cls_hash && (gr.concept || need_dy)) {
        hipLaunchKernelGGL(k_tanh_bwd, dim3(blocks_for(BK)), dim3(kThreads), 0, st, g_cls_hash, kp.ch, wk.gt, BK);
        weight_grads(st, wk.gs, wk.gt, y, B, K, D, gr.concept, nullptr, accumulate);
        if (need_dy) launch_nn(st, wk.gt, h.concept.w_f32, B, K, D, dy, nullptr);
    } else if (!g_cls_hash) {
        XMH_TRY(zero(st, gr.concept, (size_t)K * D, accumulate));
    }
    if (need_dy && g_res_cls)
        hipLaunchKernelGGL(k_l2norm_bwd, dim3(row_blocks(B)), dim3(kThreads), 0, st, y, g_res_cls, dy, B, D, B, 0, g_cls_hash ? 1 : 0);
    if (need_dy) {
        int lowest = 0;                                       // below the lowest trained MLP only d_cls reads the stream's gradient
        if (!gr.d_cls)
            while (lowest < s.R && !mlp_asked(gr.mlps[lowest])) ++lowest;
        for (int i = s.R - 1; i >= lowest; --i) {
            const xmh_mith_mlp& m = h.mlps[i];
            const xmh_mith_mlp_grads& g = gr.mlps[i];
            const float* x_in = i > 0 ? kp.x[i] : cls;
            const bool need_in = i > lowest || gr.d_cls;
            const bool need_dln = g.ln_w || g.ln_b || need_in;
            const bool need_dfc = g.fc1_w || g.fc1_b || need_dln;
            weight_grads(st, wk.gs, dy, kp.fc_act[i], B, D, 4 * D, g.fc2_w, g.fc2_b, accumulate);
            if (!need_dfc) continue;
            launch_nn(st, dy, m.fc2.w_f32, B, D, 4 * D, wk.t4, nullptr);
            hipLaunchKernelGGL(k_gelu_erf_bwd, dim3(blocks_for(B * 4 * D)), dim3(kThreads), 0, st, wk.t4, kp.fc_pre[i], B * 4 * D);
            weight_grads(st, wk.gs, wk.t4, kp.ln[i], B, 4 * D, D, g.fc1_w, g.fc1_b, accumulate);
            if (!need_dln) continue;
            launch_nn(st, wk.t4, m.fc1.w_f32, B, 4 * D, D, wk.t1, nullptr);
            ln_bwd(st, wk.gs, x_in, wk.t1, m.ln_w, dy, need_in, g.ln_w, g.ln_b, B, D, accumulate);
        }
    }
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}
