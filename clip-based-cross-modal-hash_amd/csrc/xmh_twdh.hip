// Training objective of TwDH (reference models/TwDH/TwDH.py:125-230) and the backward of its short-code transforms.
//
// A "stream" is one code length: stream 0 the long code (K[0] = long_dim bits), then every short length.  The target bits of all
// streams stand side by side, stream s at bits [bit[s], bit[s] + K[s]) of K_tot; the probabilities come as two matrices per modality,
// long [B, 2 K[0]] and short [B, 2 (K_tot - K[0])] (the short streams side by side in the same order), one (off, on) pair per bit.
//
//   xmh_twdh_targets        hash_convert(hash_center_multilables(labels, centre)) of every stream, as bits: the sign of the INTEGER sum
//                           of the +-1 centres of the row's set labels (the sign of a sum is the sign of its mean, exactly); a zero sum
//                           takes tie[k]; a row without a label (the reference's NaN mean) gives bit 0.  1 launch.
//   xmh_twdh_loss           per modality and stream: nn.BCELoss (mean, each log clamped at -100) against the pair (1, 0) / (0, 1) of the
//                           target bit, and soft_argmax_hash_loss = 1 - mean((2 p - 1)^2); and the weighted total.  2 launches: row
//                           chunks into double partials, then one block that adds the chunks in index order.
//   xmh_twdh_loss_grad      d total / d p of one modality: (p - t) / max(p (1 - p), 1e-12) / n (what autograd returns for BCELoss)
//                           and -4 (2 p - 1) / n, with the weights 1/2, quan_alpha/2 (long) and low_rate/2 (short).  1 launch.
//   xmh_twdh_short_forward  p_short = pair_softmax(long . T_cat): xmh_gemm_nt_f32 (exact fp32 MFMA) + k_pair_softmax.  2 launches.
//   xmh_twdh_short_backward g_z = pair-softmax backward of g_short, g_long (+)= g_z . T_cat^T: k_pair_softmax_bwd + xmh_gemm_nt_f32.
//                           2 launches.
// Shapes are small (B <= 1024, K_tot <= 624 in the shipped config): launch- and latency-bound.  Sums are double, in one fixed order
// (two calls on equal inputs agree to the bit); no float atomics, no host synchronisation, no allocation.
#include "xmh_common.h"
#include "xmh_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxB = 4096, kMaxBits = 4096, kMaxC = 1024;
constexpr int kRows = 32;                         // rows per partial of the loss

struct Streams {                                  // xmh_twdh_streams by value, with the derived totals
    int n, ktot;
    int bit[XMH_TWDH_MAX_STREAMS], K[XMH_TWDH_MAX_STREAMS];
};

// one block per row; a wave decides 64 consecutive bits and its first lane stores them as two words
__global__ __launch_bounds__(kThreads) void k_twdh_targets(const uint32_t* __restrict__ lab, int Lw, int C, const int8_t* __restrict__ centres,
                                                          const int8_t* __restrict__ tie, int ktot, int Tw, uint32_t* __restrict__ out) {
    const int row = blockIdx.x, lane = threadIdx.x & 63;
    const uint32_t* lr = lab + (int64_t)row * Lw;
    for (int k0 = 0; k0 < Tw * 32; k0 += kThreads) {
        const int k = k0 + threadIdx.x;
        int sum = 0, count = 0;
        if (k < ktot)
            for (int w = 0; w < Lw; ++w) {
                uint32_t m = lr[w];
                while (m) {
                    const int c = w * 32 + __ffs(m) - 1;
                    m &= m - 1;
                    if (c < C) {
                        sum += centres[(int64_t)c * ktot + k];
                        ++count;
                    }
                }
            }
        const bool on = k < ktot && count > 0 && (sum > 0 || (sum == 0 && tie[k] > 0));
        const unsigned long long mask = __ballot(on);
        const int w0 = (k0 + (int)threadIdx.x - lane) >> 5;       // the wave's first word
        if (lane == 0) {
            if (w0 < Tw) out[(int64_t)row * Tw + w0] = (uint32_t)mask;
            if (w0 + 1 < Tw) out[(int64_t)row * Tw + w0 + 1] = (uint32_t)(mask >> 32);
        }
    }
}

__device__ __forceinline__ float clamped_log(float x) {
    const float l = logf(x);
    return l < -100.0f ? -100.0f : l;             // torch's clamp of BCELoss; a NaN stays a NaN
}

struct LossIn {
    const float* p_long[2];                       // [modality]; NULL: the modality is absent, its terms are 0
    const float* p_short[2];
};

// grid (row chunks, streams, 2 modalities): sum over the chunk's rows and the stream's pairs of the BCE terms and of (2 p - 1)^2
__global__ __launch_bounds__(kThreads) void k_twdh_loss_part(Streams st, LossIn in, const uint32_t* __restrict__ targets, int Tw, int B,
                                                            double* __restrict__ part) {
    __shared__ double sh[kThreads / 64];
    const int s = blockIdx.y, m = blockIdx.z, K = st.K[s];
    const float* p = s == 0 ? in.p_long[m] : in.p_short[m];
    const int ld = s == 0 ? 2 * st.K[0] : 2 * (st.ktot - st.K[0]);
    const int col = s == 0 ? 0 : 2 * (st.bit[s] - st.K[0]);
    const int r0 = blockIdx.x * kRows, r1 = r0 + kRows < B ? r0 + kRows : B;
    double bce = 0.0, quan = 0.0;
    if (p)
        for (int e = threadIdx.x; e < (r1 - r0) * K; e += kThreads) {
            const int r = r0 + e / K, k = e % K, kb = st.bit[s] + k;
            const float2 v = *reinterpret_cast<const float2*>(p + (int64_t)r * ld + col + 2 * k);
            const bool on = (targets[(int64_t)r * Tw + (kb >> 5)] >> (kb & 31)) & 1u;
            // target pair (0, 1) when the bit is on, (1, 0) when off: -log of the entry whose target is 1, -log(1 - .) of the other
            const float l0 = on ? clamped_log(1.0f - v.x) : clamped_log(v.x);
            const float l1 = on ? clamped_log(v.y) : clamped_log(1.0f - v.y);
            bce -= (double)l0 + (double)l1;
            const double t0 = 2.0 * (double)v.x - 1.0, t1 = 2.0 * (double)v.y - 1.0;
            quan += t0 * t0 + t1 * t1;
        }
    const double sb = xmh::block_sum<kThreads / 64>(bce, sh), sq = xmh::block_sum<kThreads / 64>(quan, sh);
    if (threadIdx.x == 0) {
        double* o = part + (((int64_t)m * st.n + s) * gridDim.x + blockIdx.x) * 2;
        o[0] = sb;
        o[1] = sq;
    }
}

// one block: thread (m, s, term) adds its chunks in index order; thread 0 then forms the total.  out[0] = total,
// out[1 + (m n + s) 2 + term]: term 0 the BCE mean, term 1 the quantisation term; out[1 + 4 n + 2 s + term]: their means over the modalities
__global__ __launch_bounds__(64) void k_twdh_loss_reduce(Streams st, LossIn in, const double* __restrict__ part, int chunks, int B,
                                                        double quan_alpha, double low_rate, double* __restrict__ out) {
    __shared__ double v[2 * XMH_TWDH_MAX_STREAMS * 2];
    const int t = threadIdx.x, total = 2 * st.n * 2;
    if (t < total) {
        const int term = t & 1, s = (t >> 1) % st.n, m = (t >> 1) / st.n;
        double a = 0.0;
        for (int c = 0; c < chunks; ++c) a += part[((int64_t)(t >> 1) * chunks + c) * 2 + term];
        const double mean = a / ((double)B * 2.0 * (double)st.K[s]);
        const bool have = (s == 0 ? in.p_long[m] : in.p_short[m]) != nullptr;
        v[t] = have ? (term ? 1.0 - mean : mean) : 0.0;
        out[1 + t] = v[t];
    }
    __syncthreads();
    if (t == 0) {
        double loss = 0.0;
        for (int s = 0; s < st.n; ++s) {
            const double* img = v + s * 2;
            const double* txt = v + (st.n + s) * 2;
            const double nce = (img[0] + txt[0]) / 2.0, q = (img[1] + txt[1]) / 2.0;
            loss += s == 0 ? nce + quan_alpha * q : low_rate * nce + low_rate * q;
            out[1 + total + 2 * s] = nce;
            out[1 + total + 2 * s + 1] = q;
        }
        out[0] = loss;
    }
}

// thread per (row, bit of K_tot); streams whose gradient matrix is NULL are skipped
__global__ __launch_bounds__(kThreads) void k_twdh_loss_grad(Streams st, const float* __restrict__ p_long, const float* __restrict__ p_short,
                                                            const uint32_t* __restrict__ targets, int Tw, int B, double quan_alpha,
                                                            double low_rate, const float* __restrict__ up, float* __restrict__ d_long,
                                                            float* __restrict__ d_short) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (int64_t)B * st.ktot) return;
    const int r = (int)(e / st.ktot), kb = (int)(e % st.ktot);
    int s = 0;
    while (s + 1 < st.n && kb >= st.bit[s + 1]) ++s;
    const bool is_long = s == 0;
    float* d = is_long ? d_long : d_short;
    if (!d) return;
    const int ld = is_long ? 2 * st.K[0] : 2 * (st.ktot - st.K[0]);
    const int64_t at = (int64_t)r * ld + 2 * (is_long ? kb : kb - st.K[0]);
    const float2 v = *reinterpret_cast<const float2*>((is_long ? p_long : p_short) + at);
    const bool on = (targets[(int64_t)r * Tw + (kb >> 5)] >> (kb & 31)) & 1u;
    // per element in double, rounded once: the saturated entries (p (1 - p) under the 1e-12 floor) reach 1e11 and set the tensor's scale
    const double n = (double)B * 2.0 * (double)st.K[s];
    const double g = up ? (double)up[0] : 1.0;
    const double gb = g * (is_long ? 0.5 : 0.5 * low_rate) / n;
    const double gq = g * (is_long ? 0.5 * quan_alpha : 0.5 * low_rate) * (-4.0 / n);
    const double t0 = on ? 0.0 : 1.0, t1 = on ? 1.0 : 0.0;
    const double x = (double)v.x, y = (double)v.y;
    float2 o;
    o.x = (float)(gq * (2.0 * x - 1.0) + gb * ((x - t0) / fmax((1.0 - x) * x, 1e-12)));
    o.y = (float)(gq * (2.0 * y - 1.0) + gb * ((y - t1) / fmax((1.0 - y) * y, 1e-12)));
    *reinterpret_cast<float2*>(d + at) = o;
}

// in place over the logits: the head's own pair softmax (xmh_head_grad.hip, EPI_RELU_PAIR without the relu)
__global__ __launch_bounds__(kThreads) void k_pair_softmax(float* z, int64_t pairs) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= pairs) return;
    const float2 v = reinterpret_cast<const float2*>(z)[q];
    const float m = fmaxf(v.x, v.y);
    const float e0 = expf(v.x - m), e1 = expf(v.y - m), inv = 1.0f / (e0 + e1);
    reinterpret_cast<float2*>(z)[q] = make_float2(e0 * inv, e1 * inv);
}

// g_z0 = p0 (g0 - (g0 p0 + g1 p1)), g_z1 alike
__global__ __launch_bounds__(kThreads) void k_pair_softmax_bwd(const float* __restrict__ g, const float* __restrict__ p, int64_t pairs,
                                                              float* __restrict__ gz) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= pairs) return;
    const float2 gv = reinterpret_cast<const float2*>(g)[q], pv = reinterpret_cast<const float2*>(p)[q];
    const float dot = fmaf(pv.y, gv.y, pv.x * gv.x);
    reinterpret_cast<float2*>(gz)[q] = make_float2(pv.x * (gv.x - dot), pv.y * (gv.y - dot));
}

// the stream table as the kernels take it; the streams must tile [0, K_tot) in order
int check_streams(const char* who, const xmh_twdh_streams* t, int64_t B, Streams* out) {
    if (!t) return xmh::fail(XMH_EINVAL, "%s: null stream table", who);
    if (B <= 0 || t->n <= 0) return xmh::fail(XMH_EINVAL, "%s: bad shape B=%lld streams=%d", who, (long long)B, t->n);
    if (t->n > XMH_TWDH_MAX_STREAMS) return xmh::fail(XMH_ENOTSUP, "%s: %d streams (at most %d)", who, t->n, XMH_TWDH_MAX_STREAMS);
    Streams s = {};
    s.n = t->n;
    int64_t at = 0;
    for (int i = 0; i < t->n; ++i) {
        if (t->K[i] <= 0 || t->bit[i] != at)
            return xmh::fail(XMH_EINVAL, "%s: stream %d (bit %d, K %d) does not follow bit %lld", who, i, t->bit[i], t->K[i], (long long)at);
        s.bit[i] = t->bit[i];
        s.K[i] = t->K[i];
        at += t->K[i];
        if (at > kMaxBits) return xmh::fail(XMH_ENOTSUP, "%s: more than %d bits over the streams", who, kMaxBits);
    }
    s.ktot = (int)at;
    if (B > kMaxB) return xmh::fail(XMH_ENOTSUP, "%s: B=%lld > %d", who, (long long)B, kMaxB);
    *out = s;
    return XMH_OK;
}

bool pairs_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

int check_short(const char* who, int64_t B, int L2, int S2) {
    if (B <= 0 || L2 <= 0 || S2 <= 0 || (L2 & 1) || (S2 & 1)) return xmh::fail(XMH_EINVAL, "%s: bad shape B=%lld 2L=%d 2S=%d", who, (long long)B, L2, S2);
    if (B > kMaxB || L2 > 2 * kMaxBits || S2 > 2 * kMaxBits)
        return xmh::fail(XMH_ENOTSUP, "%s: B=%lld 2L=%d 2S=%d outside B <= %d, widths <= %d", who, (long long)B, L2, S2, kMaxB, 2 * kMaxBits);
    return XMH_OK;
}

}  // namespace

extern "C" int xmh_twdh_targets(const uint32_t* lab, int C, const int8_t* centres, const int8_t* tie, int64_t B, int K_tot,
                                uint32_t* targets, xmh_stream_t stream) {
    XMH_RANGE("xmh_twdh_targets");
    const char* who = "xmh_twdh_targets";
    if (B <= 0 || C <= 0 || K_tot <= 0) return xmh::fail(XMH_EINVAL, "%s: bad shape B=%lld C=%d K_tot=%d", who, (long long)B, C, K_tot);
    if (!lab || !centres || !tie || !targets) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (B > kMaxB || C > kMaxC || K_tot > kMaxBits)
        return xmh::fail(XMH_ENOTSUP, "%s: B=%lld C=%d K_tot=%d outside B <= %d, C <= %d, K_tot <= %d", who, (long long)B, C, K_tot, kMaxB, kMaxC, kMaxBits);
    hipLaunchKernelGGL(k_twdh_targets, dim3((unsigned)B), dim3(kThreads), 0, xmh::as_stream(stream), lab, (C + 31) / 32, C, centres, tie, K_tot,
                       (K_tot + 31) / 32, targets);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

extern "C" size_t xmh_twdh_loss_ws_bytes(int64_t B, int n_streams) {
    if (B <= 0 || B > kMaxB || n_streams <= 0 || n_streams > XMH_TWDH_MAX_STREAMS) return 0;
    return xmh::align256((size_t)2 * n_streams * xmh::ceil_div(B, kRows) * 2 * sizeof(double));
}

extern "C" int xmh_twdh_loss(const xmh_twdh_streams* streams, const float* img_long, const float* img_short, const float* txt_long,
                             const float* txt_short, const uint32_t* targets, int64_t B, double quan_alpha, double low_rate, double* out,
                             void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_twdh_loss");
    const char* who = "xmh_twdh_loss";
    Streams st;
    if (int rc = check_streams(who, streams, B, &st)) return rc;
    if (!targets || !out || !workspace) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (!img_long && !txt_long) return xmh::fail(XMH_EINVAL, "%s: neither modality given", who);
    const bool shorts = st.n > 1;
    if ((img_long && shorts && !img_short) || (txt_long && shorts && !txt_short) || (!img_long && img_short) || (!txt_long && txt_short))
        return xmh::fail(XMH_EINVAL, "%s: a modality comes with its long and (with short streams) its short probabilities, or not at all", who);
    if (!pairs_aligned(img_long) || !pairs_aligned(img_short) || !pairs_aligned(txt_long) || !pairs_aligned(txt_short))
        return xmh::fail(XMH_EINVAL, "%s: probabilities not 8-byte aligned", who);
    const size_t need = xmh_twdh_loss_ws_bytes(B, st.n);
    if (workspace_bytes < need) return xmh::fail(XMH_ENOMEM, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    LossIn in = {{img_long, txt_long}, {img_short, txt_short}};
    const int chunks = (int)xmh::ceil_div(B, kRows), Tw = (st.ktot + 31) / 32;
    hipStream_t s = xmh::as_stream(stream);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(k_twdh_loss_part, dim3(chunks, st.n, 2), dim3(kThreads), 0, s, st, in, targets, Tw, (int)B, part);
    hipLaunchKernelGGL(k_twdh_loss_reduce, dim3(1), dim3(64), 0, s, st, in, part, chunks, (int)B, quan_alpha, low_rate, out);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

extern "C" int xmh_twdh_loss_grad(const xmh_twdh_streams* streams, const float* p_long, const float* p_short, const uint32_t* targets,
                                  int64_t B, double quan_alpha, double low_rate, const float* upstream, float* d_long, float* d_short,
                                  xmh_stream_t stream) {
    XMH_RANGE("xmh_twdh_loss_grad");
    const char* who = "xmh_twdh_loss_grad";
    Streams st;
    if (int rc = check_streams(who, streams, B, &st)) return rc;
    if (!targets || (d_long && !p_long) || (d_short && !p_short)) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (d_short && st.n < 2) return xmh::fail(XMH_EINVAL, "%s: a short gradient without short streams", who);
    if (!pairs_aligned(p_long) || !pairs_aligned(p_short) || !pairs_aligned(d_long) || !pairs_aligned(d_short))
        return xmh::fail(XMH_EINVAL, "%s: matrices not 8-byte aligned", who);
    if (!d_long && !d_short) return XMH_OK;
    const int64_t n = B * st.ktot;
    hipLaunchKernelGGL(k_twdh_loss_grad, dim3((unsigned)xmh::ceil_div(n, kThreads)), dim3(kThreads), 0, xmh::as_stream(stream), st, p_long, p_short,
                       targets, (st.ktot + 31) / 32, (int)B, quan_alpha, low_rate, upstream, d_long, d_short);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

extern "C" int xmh_twdh_short_forward(const float* long_probs, const float* trans_t, int64_t B, int L2, int S2, float* p_short,
                                      xmh_stream_t stream) {
    XMH_RANGE("xmh_twdh_short_forward");
    const char* who = "xmh_twdh_short_forward";
    if (int rc = check_short(who, B, L2, S2)) return rc;
    if (!long_probs || !trans_t || !p_short) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (!pairs_aligned(p_short)) return xmh::fail(XMH_EINVAL, "%s: p_short not 8-byte aligned", who);
    XMH_TRY(xmh_gemm_nt_f32(long_probs, L2, trans_t, L2, nullptr, nullptr, 0, p_short, S2, B, S2, L2, XMH_ACT_NONE, XMH_PREC_F32, stream));
    const int64_t pairs = B * (S2 / 2);
    hipLaunchKernelGGL(k_pair_softmax, dim3((unsigned)xmh::ceil_div(pairs, kThreads)), dim3(kThreads), 0, xmh::as_stream(stream), p_short, pairs);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

extern "C" int xmh_twdh_short_backward(const float* g_short, const float* p_short, const float* trans, int64_t B, int L2, int S2,
                                       float* g_long, int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_twdh_short_backward");
    const char* who = "xmh_twdh_short_backward";
    if (int rc = check_short(who, B, L2, S2)) return rc;
    if (!g_short || !p_short || !trans || !g_long || !workspace) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (!pairs_aligned(g_short) || !pairs_aligned(p_short) || !pairs_aligned(workspace))
        return xmh::fail(XMH_EINVAL, "%s: matrices not 8-byte aligned", who);
    const size_t need = (size_t)B * S2 * sizeof(float);
    if (workspace_bytes < need) return xmh::fail(XMH_ENOMEM, "%s: workspace of %zu bytes, %zu needed (4 B 2S)", who, workspace_bytes, need);
    float* gz = static_cast<float*>(workspace);
    const int64_t pairs = B * (S2 / 2);
    hipLaunchKernelGGL(k_pair_softmax_bwd, dim3((unsigned)xmh::ceil_div(pairs, kThreads)), dim3(kThreads), 0, xmh::as_stream(stream), g_short, p_short,
                       pairs, gz);
    XMH_LAUNCH_CHECK(who);
    // g_long [B, 2L] (+)= g_z [B, 2S] . trans^T, trans [2L, 2S] being the W [N, K] of the NT product
    return xmh_gemm_nt_f32(gz, S2, trans, S2, nullptr, accumulate ? g_long : nullptr, L2, g_long, L2, B, L2, S2, XMH_ACT_NONE, XMH_PREC_F32, stream);
}
