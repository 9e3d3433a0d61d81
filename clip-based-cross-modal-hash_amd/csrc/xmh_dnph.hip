// Objective of DNPH (reference models/DNPH/loss/loss.py:12-33 and models/DNPH/DNPH.py:72-99) and its gradient with respect to the two
// code matrices, the two class-prediction matrices and the proxies; and the assignment of its noise term (loss/b_reg.py:19-41).
//
//   n(v) = v / max(|v|, 1e-12) (F.normalize), u = n(cat(f_img, f_txt)) [2B, K], q = n(P) [C, K], labels l packed by xmh_pack_labels
//   D[n][c] = sum_k (u[n][k] - q[c][k])^2 + mrg l[n][c]            (a sum of squared differences: exactly 0 where a code is its proxy)
//   p_loss  = mean_n sum_c -l[n][c] log_softmax(-D[n][:])[c]        (2B rows, the row maximum subtracted)
//   d_loss  = CE(p_img, t) + CE(p_txt, t), t[b] = lowest set class of row b, 0 for a row without one (torch.argmax of a 0 / 1 row)
//   noise_m = mean_b sum_k f_m[b][k] noise_m[b][k]                  (noise_m == NULL: 0)
//   loss    = p_loss + d_loss - noise_alpha (noise_img + noise_txt)
//
//   xmh_dnph_loss       k_dnph_rows<true>   (block n < 2B: code row n -- its norm, its distances, its log-sum-exp, its share of p_loss, the
//                                            cross-entropy of its prediction row, its noise product; block 2B + c: the norm of proxy c)
//                       k_dnph_finalize     (one block: ordered sums of the per-row partials, the means, the total) -> out8
//   xmh_dnph_loss_grad  k_dnph_rows<false>  (norms, label counts, targets and log-sum-exps only)
//                       k_dnph_grad         (block n < 2B: d/df of code row n and d/dp of its prediction row; block 2B + c: d/dP_c)
//
// No host synchronisation, no allocation, no float atomics: every sum has one fixed order, so two calls on the same inputs agree to
// the bit.  The distances are formed in the same lane order by every kernel that needs them.  The gradient sums over the proxies (of a
// code row) and over the 2B code rows (of a proxy) run in double: their terms nearly cancel (sum_c dD = 0 for every row), and a float
// chain of 2B terms would carry the length of the batch in its error.
// Non-finite inputs pass through as they do through the reference's expression, they are not masked: the label weights multiply
// (0 * NaN = NaN, as -label * log_softmax does), nothing is skipped for a zero weight, a NaN norm stays NaN (clamp_min keeps it, fmaxf
// would drop it).  So a NaN in a code row makes p_loss and the loss NaN, that row's gradient NaN and every row of grad_P NaN; a NaN
// in a proxy makes every distance column, hence every softmax, hence every row of grad_f and grad_P NaN.  grad_p never sees either.
// Bound: B = 100, K = 16..128, C = 80 (COCO) is a few tens of KB of L2-resident operands: launch-latency bound, two launches each way.
//
// xmh_assign_min_cost is host code: the square linear sum assignment by shortest augmenting paths with dual potentials
// (Jonker-Volgenant), O(n^3), what the reference asks of scipy.optimize.linear_sum_assignment once per modality and step.
#include <math.h>

#include <limits>
#include <vector>

#include "xmh_common.h"
#include "xmh_rows.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxB = 4096, kMaxK = 4096, kMaxC = 1024;
constexpr int kSlots = kMaxK / kThreads;         // columns per thread in the column-parallel phases (K <= 4096)
constexpr int kChunk = 256;                      // code rows whose weights a proxy block stages in LDS at a time
constexpr float kEps = 1e-12f;                   // F.normalize's eps
constexpr int kMaxAssign = 4096;

// workspace: per-row partial sums (p_loss share, cross-entropy, noise product; padded to 4), the log-sum-exp of -D[n][:] and the norm
// of every code row, the norm of every proxy, and per label row its label count and its argmax target
struct WsView {
    double* part;
    float* lse;
    float* nf;
    float* np;
    int* cnt;
};

__host__ __device__ inline size_t ws_layout(int64_t B, int C, void* base, WsView* v) {
    xmh::Arena ar(base);
    WsView w;
    w.part = ar.take<double>((size_t)B * 2 * 4);
    w.lse = ar.take<float>((size_t)B * 2);
    w.nf = ar.take<float>((size_t)B * 2);
    w.np = ar.take<float>((size_t)C);
    w.cnt = ar.take<int>((size_t)B * 2);
    if (v) *v = w;
    return ar.used;
}

struct Args {
    const float* f[2];        // f_img, f_txt [B, K]
    const float* p[2];        // p_img, p_txt [B, Cp]
    const float* noise[2];    // [B, K] or NULL
    const float* P;           // [C, K]
    const uint32_t* lab;      // [B][Lw]
    int B, K, C, Cp, Lw;
    float mrg, noise_alpha;
};

using xmh::has_label;
using xmh::inv_norm;
using xmh::wave_norm;
using xmh::wave_sum;

// sum_k (u[k] - pc[k] ip)^2 by one wave: u the normalised code row, pc the raw proxy.  The products are rounded before the
// subtraction (no contraction into an fma), so a code that equals its proxy gives an exact 0 here and in the gradient.
__device__ __forceinline__ float wave_dist(const float* u, const float* pc, float ip, int K) {
    const int lane = threadIdx.x & 63;
    float d = 0.0f;
    for (int k = lane; k < K; k += 64) {
        const float df = u[k] - __fmul_rn(pc[k], ip);
        d = fmaf(df, df, d);
    }
    return wave_sum(d);
}

// lowest set class of a label row held one word per lane (lanes >= Lw hold 0); 0 for an empty row.  Wave-uniform.
__device__ __forceinline__ int lowest_label(uint32_t mine) {
    const unsigned long long any = __ballot(mine != 0u);
    if (any == 0ull) return 0;
    const int w = __ffsll((long long)any) - 1;
    const uint32_t word = (uint32_t)__shfl((int)mine, w);
    return w * 32 + __ffs((int)word) - 1;
}

// Code row n of the 2B: raw in vs, normalised in us, D[n][c] in ds (all LDS).  Returns the row's norm.  Ends with a barrier.
__device__ __forceinline__ float load_row_dists(const Args& a, int n, float* vs, float* us, float* ds) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = n >= a.B, b = n - m * a.B;
    const float* row = a.f[m] + (int64_t)b * a.K;
    for (int k = threadIdx.x; k < a.K; k += kThreads) vs[k] = row[k];
    __syncthreads();
    const float nv = wave_norm(vs, a.K);
    const float iv = inv_norm(nv, kEps);
    for (int k = threadIdx.x; k < a.K; k += kThreads) us[k] = __fmul_rn(vs[k], iv);
    __syncthreads();
    for (int c = wave; c < a.C; c += kWaves) {
        const float* pc = a.P + (int64_t)c * a.K;
        const float d = wave_dist(us, pc, inv_norm(wave_norm(pc, a.K), kEps), a.K);
        if (lane == 0) ds[c] = d + (has_label(a.lab, a.Lw, b, c) ? a.mrg : 0.0f);
    }
    __syncthreads();
    return nv;
}

// Blocks [0, 2B): code row n.  Blocks [2B, 2B + C): the norm of proxy c.
// kLoss: also the row's share of p_loss, its cross-entropy and its noise product (the forward); otherwise what k_dnph_grad reads.
template <bool kLoss>
__global__ __launch_bounds__(kThreads) void k_dnph_rows(Args a, WsView ws) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double dsh[kWaves];
    __shared__ float fsh[kWaves];
    const int lane = threadIdx.x & 63;
    if ((int)blockIdx.x >= 2 * a.B) {
        const int c = blockIdx.x - 2 * a.B;
        if (threadIdx.x < 64) {
            const float n = wave_norm(a.P + (int64_t)c * a.K, a.K);
            if (lane == 0) ws.np[c] = n;
        }
        return;
    }
    const int n = blockIdx.x, m = n >= a.B, b = n - m * a.B;
    float* vs = smem;
    float* us = vs + a.K;
    float* ds = us + a.K;                                        // [C] D[n][:], then -D[n][:]
    const float nv = load_row_dists(a, n, vs, us, ds);
    for (int c = threadIdx.x; c < a.C; c += kThreads) ds[c] = -ds[c];
    __syncthreads();
    const float lse = xmh::block_lse<kWaves>(ds, a.C, fsh, dsh);
    const uint32_t mine = lane < a.Lw ? a.lab[(int64_t)b * a.Lw + lane] : 0u;
    const int npos = wave_sum((int)__popc(mine)), low = lowest_label(mine), t = low < a.C ? low : 0;   // bits past C are never set
    if (threadIdx.x == 0) {
        ws.lse[n] = lse;
        ws.nf[n] = nv;
        if (!m) {
            ws.cnt[2 * b] = npos;
            ws.cnt[2 * b + 1] = t;
        }
    }
    if (!kLoss) return;
    double pl = 0.0;
    for (int c = threadIdx.x; c < a.C; c += kThreads) {
        const float l = has_label(a.lab, a.Lw, b, c) ? 1.0f : 0.0f;
        pl += (double)(-l * (ds[c] - lse));                        // -label * log_softmax: 0 * NaN stays NaN
    }
    pl = xmh::block_sum<kWaves>(pl, dsh);
    const float* pr = a.p[m] + (int64_t)b * a.Cp;
    const float ce = xmh::block_lse<kWaves>(pr, a.Cp, fsh, dsh) - pr[t];
    double nz = 0.0;
    if (a.noise[m]) {
        const float* nr = a.noise[m] + (int64_t)b * a.K;
        for (int k = threadIdx.x; k < a.K; k += kThreads) nz += (double)(vs[k] * nr[k]);
        nz = xmh::block_sum<kWaves>(nz, dsh);
    }
    if (threadIdx.x == 0) {
        ws.part[(int64_t)n * 4 + 0] = pl;
        ws.part[(int64_t)n * 4 + 1] = (double)ce;
        ws.part[(int64_t)n * 4 + 2] = nz;
    }
}

__global__ __launch_bounds__(kThreads) void k_dnph_finalize(int B, float noise_alpha, WsView ws, double* __restrict__ out8) {
    __shared__ double sh[kWaves];
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};               // p_loss, then (cross-entropy, noise) of the image and of the text rows
    for (int r = threadIdx.x; r < 2 * B; r += kThreads) {
        const int m = r >= B;
        s[0] += ws.part[(int64_t)r * 4];
        s[1 + 2 * m] += ws.part[(int64_t)r * 4 + 1];
        s[2 + 2 * m] += ws.part[(int64_t)r * 4 + 2];
    }
    for (int t = 0; t < 5; ++t) s[t] = xmh::block_sum<kWaves>(s[t], sh);
    if (threadIdx.x == 0) {
        const double p_loss = s[0] / (2.0 * B), d_img = s[1] / B, d_txt = s[3] / B, n_img = s[2] / B, n_txt = s[4] / B;
        out8[0] = p_loss + (d_img + d_txt) - (double)noise_alpha * (n_img + n_txt);
        out8[1] = p_loss;
        out8[2] = d_img;
        out8[3] = d_txt;
        out8[4] = n_img;
        out8[5] = n_txt;
        out8[6] = 0.0;
        out8[7] = 0.0;
    }
}

struct Grads {
    float* f[2];              // grad_f_img, grad_f_txt
    float* p[2];              // grad_p_img, grad_p_txt
    float* P;
};

// Blocks [0, 2B): grad_f row and grad_p row of code row n.  Blocks [2B, 2B + C): grad_P[c].  lse, norms and counts come from k_dnph_rows.
__global__ __launch_bounds__(kThreads) void k_dnph_grad(Args a, WsView ws, const float* __restrict__ up, Grads gr, int accumulate) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double dsh[kWaves];
    __shared__ float fsh[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float g = up ? up[0] : 1.0f;
    const float w2b = 1.0f / (2.0f * (float)a.B);               // d p_loss / d (row share)
    double acc[kSlots];
#pragma unroll
    for (int r = 0; r < kSlots; ++r) acc[r] = 0.0;
    float du[kSlots];

    if ((int)blockIdx.x < 2 * a.B) {
        const int n = blockIdx.x, m = n >= a.B, b = n - m * a.B;
        if (gr.p[m]) {                                           // (softmax(p) - onehot(t)) / B
            const float* pr = a.p[m] + (int64_t)b * a.Cp;
            float* out = gr.p[m] + (int64_t)b * a.Cp;
            // exp(p - max) / sum, not exp(p - lse): lse carries the rounding of the maximum's size (half an ulp of 375 is 1.5e-5
            // of every softmax entry when the logits are that large), the quotient does not
            float mx;
            const float sum = (float)xmh::block_exp_sum<kWaves>(pr, a.Cp, fsh, dsh, &mx);
            const int t = ws.cnt[2 * b + 1];
            for (int c = threadIdx.x; c < a.Cp; c += kThreads) {
                const float d = g * ((expf(pr[c] - mx) / sum - (c == t ? 1.0f : 0.0f)) / (float)a.B);
                out[c] = accumulate ? out[c] + d : d;
            }
        }
        if (!gr.f[m]) return;
        float* vs = smem;
        float* us = vs + a.K;
        float* ds = us + a.K;                                    // [C] D[n][:], then d p_loss / d D[n][:]
        float* ips = ds + a.C;                                   // [C] 1 / |P_c|
        const float nv = load_row_dists(a, n, vs, us, ds);
        const float lse = ws.lse[n], L = (float)ws.cnt[2 * b];
        for (int c = threadIdx.x; c < a.C; c += kThreads) {
            const float l = has_label(a.lab, a.Lw, b, c) ? 1.0f : 0.0f;
            ds[c] = (l - L * expf(-ds[c] - lse)) * w2b;          // 0 * NaN stays NaN, as in log_softmax's backward
            ips[c] = inv_norm(ws.np[c], kEps);
        }
        __syncthreads();
        for (int c = 0; c < a.C; ++c) {
            const double w = 2.0 * (double)ds[c];
            const float ip = ips[c];
            const float* pc = a.P + (int64_t)c * a.K;
#pragma unroll
            for (int r = 0; r < kSlots; ++r) {
                const int k = threadIdx.x + r * kThreads;
                if (k < a.K) acc[r] += w * (double)(us[k] - __fmul_rn(pc[k], ip));
            }
        }
#pragma unroll
        for (int r = 0; r < kSlots; ++r) du[r] = (float)acc[r];
        const float* nr = a.noise[m] ? a.noise[m] + (int64_t)b * a.K : nullptr;
        xmh::normalize_backward_store<kThreads, kSlots, true>(vs, nv, kEps, du, a.K, g, gr.f[m] + (int64_t)b * a.K, accumulate, fsh, nr,
                                                              -a.noise_alpha / (float)a.B);
    } else {
        if (!gr.P) return;
        const int c = blockIdx.x - 2 * a.B;
        float* ps = smem;                                        // P_c
        float* qs = ps + a.K;                                    // P_c / |P_c|
        float* wn = qs + a.K;                                    // [kChunk] d p_loss / d D[n][c]
        float* in = wn + kChunk;                                 // [kChunk] 1 / |f_n|
        for (int k = threadIdx.x; k < a.K; k += kThreads) ps[k] = a.P[(int64_t)c * a.K + k];
        const float np = ws.np[c], ip = inv_norm(np, kEps);
        __syncthreads();
        for (int k = threadIdx.x; k < a.K; k += kThreads) qs[k] = __fmul_rn(ps[k], ip);
        __syncthreads();
        for (int n0 = 0; n0 < 2 * a.B; n0 += kChunk) {
            const int cnt = min(kChunk, 2 * a.B - n0);
            for (int ii = wave; ii < cnt; ii += kWaves) {
                const int n = n0 + ii, m = n >= a.B, b = n - m * a.B;
                const float* row = a.f[m] + (int64_t)b * a.K;
                const float iv = inv_norm(ws.nf[n], kEps);
                float d = 0.0f;                                  // D[n][c] in the lane order of wave_dist
                for (int k = lane; k < a.K; k += 64) {
                    const float df = __fmul_rn(row[k], iv) - qs[k];
                    d = fmaf(df, df, d);
                }
                const bool l = has_label(a.lab, a.Lw, b, c);
                d = wave_sum(d) + (l ? a.mrg : 0.0f);
                if (lane == 0) {
                    wn[ii] = ((l ? 1.0f : 0.0f) - (float)ws.cnt[2 * b] * expf(-d - ws.lse[n])) * w2b;
                    in[ii] = iv;
                }
            }
            __syncthreads();
            for (int ii = 0; ii < cnt; ++ii) {
                const int n = n0 + ii, m = n >= a.B, b = n - m * a.B;
                const float* row = a.f[m] + (int64_t)b * a.K;
                const double w = -2.0 * (double)wn[ii];
                const float iv = in[ii];
#pragma unroll
                for (int r = 0; r < kSlots; ++r) {
                    const int k = threadIdx.x + r * kThreads;
                    if (k < a.K) acc[r] += w * (double)(__fmul_rn(row[k], iv) - qs[k]);
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < kSlots; ++r) du[r] = (float)acc[r];
        xmh::normalize_backward_store<kThreads>(ps, np, kEps, du, a.K, g, gr.P + (int64_t)c * a.K, accumulate, fsh);
    }
}

// shared argument checks of both entry points: they run before any HIP call
int check_args(const char* who, const float* f_img, const float* f_txt, const float* p_img, const float* p_txt, const float* P, int64_t B, int K,
               int C, int Cp, const uint32_t* lab, void* ws, size_t ws_bytes) {
    if (B <= 0 || K <= 0 || C <= 0 || Cp <= 0) return xmh::fail(XMH_EINVAL, "%s: bad shape B=%lld K=%d C=%d Cp=%d", who, (long long)B, K, C, Cp);
    if (Cp < C) return xmh::fail(XMH_EINVAL, "%s: Cp=%d prediction outputs for C=%d classes (the argmax targets need Cp >= C)", who, Cp, C);
    if (B > kMaxB || K > kMaxK || C > kMaxC || Cp > kMaxC)
        return xmh::fail(XMH_ENOTSUP, "%s: B=%lld K=%d C=%d Cp=%d outside B <= %d, K <= %d, C <= %d, Cp <= %d", who, (long long)B, K, C, Cp, kMaxB,
                         kMaxK, kMaxC, kMaxC);
    if (!f_img || !f_txt || !p_img || !p_txt || !P || !lab || !ws) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    return xmh::check_workspace(who, ws, ws_bytes, ws_layout(B, C, nullptr, nullptr), "xmh_dnph_loss_ws_bytes", XMH_ENOMEM);
}

Args make_args(const float* f_img, const float* f_txt, const float* p_img, const float* p_txt, const float* P, int64_t B, int K, int C, int Cp,
               const uint32_t* lab, float mrg, float noise_alpha, const float* noise_img, const float* noise_txt) {
    Args a;
    a.f[0] = f_img, a.f[1] = f_txt, a.p[0] = p_img, a.p[1] = p_txt, a.noise[0] = noise_img, a.noise[1] = noise_txt;
    a.P = P, a.lab = lab;
    a.B = (int)B, a.K = K, a.C = C, a.Cp = Cp, a.Lw = (C + 31) / 32;
    a.mrg = mrg, a.noise_alpha = noise_alpha;
    return a;
}

}  // namespace

extern "C" size_t xmh_dnph_loss_ws_bytes(int64_t B, int K, int C, int Cp) {
    if (B <= 0 || K <= 0 || C <= 0 || Cp < C || B > kMaxB || K > kMaxK || C > kMaxC || Cp > kMaxC) return 0;
    return ws_layout(B, C, nullptr, nullptr);
}

extern "C" int xmh_dnph_loss(const float* f_img, const float* f_txt, const float* p_img, const float* p_txt, const float* P, int64_t B, int K,
                             int C, int Cp, const uint32_t* lab, float mrg, float noise_alpha, const float* noise_img, const float* noise_txt,
                             void* ws, size_t ws_bytes, double* out8, xmh_stream_t stream) {
    XMH_RANGE("xmh_dnph_loss");
    if (int rc = check_args("xmh_dnph_loss", f_img, f_txt, p_img, p_txt, P, B, K, C, Cp, lab, ws, ws_bytes)) return rc;
    if (!out8) return xmh::fail(XMH_EINVAL, "xmh_dnph_loss: null pointer");
    WsView v;
    ws_layout(B, C, ws, &v);
    const Args a = make_args(f_img, f_txt, p_img, p_txt, P, B, K, C, Cp, lab, mrg, noise_alpha, noise_img, noise_txt);
    hipStream_t st = xmh::as_stream(stream);
    hipLaunchKernelGGL(k_dnph_rows<true>, dim3((unsigned)(2 * B + C)), dim3(kThreads), ((size_t)2 * K + C) * 4, st, a, v);
    hipLaunchKernelGGL(k_dnph_finalize, dim3(1), dim3(kThreads), 0, st, (int)B, noise_alpha, v, out8);
    XMH_LAUNCH_CHECK("xmh_dnph_loss");
    return XMH_OK;
}

extern "C" int xmh_dnph_loss_grad(const float* f_img, const float* f_txt, const float* p_img, const float* p_txt, const float* P, int64_t B,
                                  int K, int C, int Cp, const uint32_t* lab, float mrg, float noise_alpha, const float* noise_img,
                                  const float* noise_txt, const float* upstream, float* grad_f_img, float* grad_f_txt, float* grad_p_img,
                                  float* grad_p_txt, float* grad_P, int accumulate, void* ws, size_t ws_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_dnph_loss_grad");
    if (int rc = check_args("xmh_dnph_loss_grad", f_img, f_txt, p_img, p_txt, P, B, K, C, Cp, lab, ws, ws_bytes)) return rc;
    if (!grad_f_img && !grad_f_txt && !grad_p_img && !grad_p_txt && !grad_P) return XMH_OK;
    WsView v;
    ws_layout(B, C, ws, &v);
    const Args a = make_args(f_img, f_txt, p_img, p_txt, P, B, K, C, Cp, lab, mrg, noise_alpha, noise_img, noise_txt);
    Grads gr;
    gr.f[0] = grad_f_img, gr.f[1] = grad_f_txt, gr.p[0] = grad_p_img, gr.p[1] = grad_p_txt, gr.P = grad_P;
    hipStream_t st = xmh::as_stream(stream);
    hipLaunchKernelGGL(k_dnph_rows<false>, dim3((unsigned)(2 * B + C)), dim3(kThreads), ((size_t)2 * K + C) * 4, st, a, v);
    const size_t lds = ((size_t)2 * K + (size_t)(2 * C > 2 * kChunk ? 2 * C : 2 * kChunk)) * 4;   // <= 40 KB at K = 4096, C = 1024
    hipLaunchKernelGGL(k_dnph_grad, dim3((unsigned)(2 * B + C)), dim3(kThreads), lds, st, a, v, upstream, gr, accumulate);
    XMH_LAUNCH_CHECK("xmh_dnph_loss_grad");
    return XMH_OK;
}

// Square linear sum assignment, exact: rows are inserted one at a time; each insertion grows a shortest-path tree over the columns in
// reduced costs (u, v the dual potentials) until it reaches a free column, then the potentials are updated and the path is flipped.
// Columns are scanned in index order and a tie keeps the earlier one, so the result is a function of the matrix alone.
extern "C" int xmh_assign_min_cost(const double* cost, int n, int* col_of_row) {
    if (n <= 0) return xmh::fail(XMH_EINVAL, "xmh_assign_min_cost: n=%d", n);
    if (n > kMaxAssign) return xmh::fail(XMH_ENOTSUP, "xmh_assign_min_cost: n=%d above %d", n, kMaxAssign);
    if (!cost || !col_of_row) return xmh::fail(XMH_EINVAL, "xmh_assign_min_cost: null pointer");
    for (int64_t i = 0; i < (int64_t)n * n; ++i)
        if (!isfinite(cost[i])) return xmh::fail(XMH_EINVAL, "xmh_assign_min_cost: cost[%lld] is not finite", (long long)i);
    const double inf = std::numeric_limits<double>::infinity();
    // column n is the virtual column the row being inserted starts from
    std::vector<double> u(n, 0.0), v(n + 1, 0.0), dist(n + 1);
    std::vector<int> row_of_col(n + 1, -1), prev(n + 1);
    std::vector<char> done(n + 1);
    for (int i = 0; i < n; ++i) {
        row_of_col[n] = i;
        for (int j = 0; j <= n; ++j) dist[j] = inf, done[j] = 0, prev[j] = n;
        int j0 = n;
        do {
            done[j0] = 1;
            const int r = row_of_col[j0];
            const double* cr = cost + (int64_t)r * n;
            double best = inf;
            int j1 = -1;
            for (int j = 0; j < n; ++j) {
                if (done[j]) continue;
                const double red = cr[j] - u[r] - v[j];
                if (red < dist[j]) dist[j] = red, prev[j] = j0;
                if (dist[j] < best) best = dist[j], j1 = j;
            }
            for (int j = 0; j <= n; ++j) {
                if (done[j]) {
                    u[row_of_col[j]] += best;
                    v[j] -= best;
                } else {
                    dist[j] -= best;
                }
            }
            j0 = j1;
        } while (row_of_col[j0] != -1);
        do {
            const int j1 = prev[j0];
            row_of_col[j0] = row_of_col[j1];
            j0 = j1;
        } while (j0 != n);
    }
    for (int j = 0; j < n; ++j) col_of_row[row_of_col[j]] = j;
    return XMH_OK;
}
