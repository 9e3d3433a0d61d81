// HyP loss of DSPH (reference models/DSPH/loss/HyP.py:18-70) and its gradient with respect to the two code matrices and the proxies.
//
//   n(v) = v / max(|v|, 1e-12) (F.normalize), cos = n(x) n(P)^T, cos_t = n(y) n(P)^T, labels l packed by xmh_pack_labels
//   pos = sum_{l=1} (1 - cos) / P_num          neg = sum_{l=0} relu(cos - thr) / N_num          (and _t on cos_t)
//   alpha > 0: M = rows with >= 2 labels, Z = #ordered pairs of M x M with disjoint label sets,
//              reg / reg_t / reg_xt = sum_{pairs} alpha relu(sim - thr) / Z with sim = cos of x-x / y-y / x-y; 0 when Z == 0
//
//   xmh_hyp_loss       k_hyp_rows<true>  (one block per code row: its sums over the proxies and over its disjoint partners, its
//                                         label count, its Z share; one block per proxy: its norm) -> per-row partials in ws
//                      k_hyp_finalize    (one block: ordered sums of the partials, the divisions, the Z == 0 branch) -> out8
//   xmh_hyp_loss_grad  k_hyp_rows<false> (counts and norms only)
//                      k_hyp_grad        (blocks [0, B): d/dx_i and d/dy_i; blocks [B, B + C): d/dP_c, each a fixed-order sum)
//
// Every quantity the reference counts with nonzero() (P_num, N_num, M, Z) is counted here on the device, so neither call synchronises
// with the host.  There are no float atomics: every sum has one fixed order, so two calls on the same inputs agree to the bit.
// The dot products that decide a relu' mask ([cos > thr]) are formed in the same lane order by every kernel that needs them, so the
// forward, the row gradient and the proxy gradient see the same mask.
// Non-finite inputs pass through as they do through the reference's expression, they are not masked: a NaN similarity gives a NaN
// hinge (F.relu keeps it, fmaxf would drop it) and a NaN weight in the gradient ([NaN > thr] would drop it), a NaN norm gives a NaN
// 1 / norm (clamp_min keeps it), and a column is skipped for its zero weights only when the norm behind them is finite (1 / Inf = 0
// makes the weight of a label -0, and the reference multiplies that column in: 0 * Inf = NaN).
// So a NaN or Inf in a proxy makes neg, neg_t (pos, pos_t where a row carries its class) and the loss NaN, every row of grad_x and
// grad_y NaN and that proxy's row of grad_P NaN; a NaN or Inf in a code row makes the terms that row enters NaN, its own gradient
// row NaN and every row of grad_P NaN.
// The reference's backward multiplies every row of M into its pair products, the pairs that share a class with weight 0: a row of M
// whose norm is not finite therefore turns the x and y gradients of every row of M NaN (0 * NaN), here as there.
// Bound: B = 100, K = 16..128, C = 80 (COCO, configs[4]) is a few tens of KB of L2-resident operands: launch-latency bound.
#include "xmh_common.h"
#include "xmh_rows.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxB = 4096, kMaxK = 4096, kMaxC = 1024;
constexpr int kSlots = kMaxK / kThreads;         // columns per thread in the column-parallel phases (K <= 4096)
constexpr int kChunk = 256;                      // partner rows whose pair weights are staged in LDS at a time
constexpr float kEps = 1e-12f;                   // F.normalize's eps

// workspace: per-row partial sums (7 doubles, padded to 8), per-row counts (labels, Z share), row norms of x, y and P
struct WsView {
    double* part;
    int* cnt;
    float* nx;
    float* ny;
    float* np;
};

__host__ __device__ inline size_t ws_layout(int64_t B, int C, void* base, WsView* v) {
    xmh::Arena ar(base);
    WsView w;
    w.part = ar.take<double>((size_t)B * 8);
    w.cnt = ar.take<int>((size_t)B * 2);
    w.nx = ar.take<float>((size_t)B);
    w.ny = ar.take<float>((size_t)B);
    w.np = ar.take<float>((size_t)C);
    if (v) *v = w;
    return ar.used;
}

using xmh::has_label;
using xmh::inv_norm;
using xmh::wave_norm;
using xmh::wave_sum;

// relu(v) as F.relu forms it: NaN stays NaN
__device__ __forceinline__ float hinge(float v) { return isnan(v) ? v : fmaxf(v, 0.0f); }

// relu'(sim - thr) * w, with a NaN similarity handed on as the weight: the reference's backward ends in NaN wherever it enters
__device__ __forceinline__ float hinge_weight(float sim, float thr, float w) { return sim > thr ? w : (isnan(sim) ? sim : 0.0f); }

// Row j (lanes < Lw hold its label words in w) against the row whose words are `mine` (itself in M).  in_m: j is in M as well (>= 2
// labels).  disjoint: it is then a regulariser partner, sharing no class.  Wave-uniform.
struct Partner {
    bool in_m, disjoint;
};
__device__ __forceinline__ Partner partner_of(uint32_t mine, uint32_t w) {
    const bool in_m = wave_sum((int)__popc(w)) >= 2;
    return {in_m, in_m && __ballot((mine & w) != 0u) == 0ull};
}

// Blocks [0, B): row i of the codes.  Blocks [B, B + C): the norm of proxy c.
// kLoss: also the row's sums over the proxies and over its regulariser partners (the forward); otherwise counts and norms only.
template <bool kLoss>
__global__ __launch_bounds__(kThreads) void k_hyp_rows(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ P, int B, int K, int C,
                                                       const uint32_t* __restrict__ lab, int Lw, float thr, float alpha, WsView ws) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double red[kWaves][7];
    __shared__ int zred[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)blockIdx.x >= B) {
        const int c = blockIdx.x - B;
        if (wave == 0) {
            const float n = wave_norm(P + (int64_t)c * K, K);
            if (lane == 0) ws.np[c] = n;
        }
        return;
    }
    const int i = blockIdx.x;
    float* xs = smem;
    float* ys = smem + K;
    for (int k = threadIdx.x; k < K; k += kThreads) {
        xs[k] = x[(int64_t)i * K + k];
        ys[k] = y[(int64_t)i * K + k];
    }
    __syncthreads();
    const float nxi = wave_norm(xs, K), nyi = wave_norm(ys, K);
    const float ix = inv_norm(nxi, kEps), iy = inv_norm(nyi, kEps);
    const uint32_t mine = lane < Lw ? lab[(int64_t)i * Lw + lane] : 0u;
    const int npos = wave_sum((int)__popc(mine));

    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // pos, neg, pos_t, neg_t, reg, reg_t, reg_xt (before alpha / Z)
    if (kLoss) {
        for (int c = wave; c < C; c += kWaves) {
            const float* pc = P + (int64_t)c * K;
            float d = 0.0f, dt = 0.0f, pp = 0.0f;
            for (int k = lane; k < K; k += 64) {
                const float p = pc[k];
                d = fmaf(xs[k], p, d);
                dt = fmaf(ys[k], p, dt);
                pp = fmaf(p, p, pp);
            }
            d = wave_sum(d);
            dt = wave_sum(dt);
            const float ip = inv_norm(sqrtf(wave_sum(pp)), kEps);
            const float cs = d * ix * ip, ct = dt * iy * ip;
            if (has_label(lab, Lw, i, c)) {
                acc[0] += (double)(1.0f - cs);
                acc[2] += (double)(1.0f - ct);
            } else {
                acc[1] += (double)hinge(cs - thr);
                acc[3] += (double)hinge(ct - thr);
            }
        }
    }
    int z = 0;
    if (alpha > 0.0f && npos >= 2) {
        for (int j = wave; j < B; j += kWaves) {
            const uint32_t w = lane < Lw ? lab[(int64_t)j * Lw + lane] : 0u;
            if (!partner_of(mine, w).disjoint) continue;
            ++z;
            if (kLoss) {
                const float* xj = x + (int64_t)j * K;
                const float* yj = y + (int64_t)j * K;
                float dxx = 0.0f, dyy = 0.0f, dxy = 0.0f, nx2 = 0.0f, ny2 = 0.0f;
                for (int k = lane; k < K; k += 64) {
                    const float a = xj[k], b = yj[k];
                    dxx = fmaf(xs[k], a, dxx);
                    dyy = fmaf(ys[k], b, dyy);
                    dxy = fmaf(xs[k], b, dxy);
                    nx2 = fmaf(a, a, nx2);
                    ny2 = fmaf(b, b, ny2);
                }
                const float ixj = inv_norm(sqrtf(wave_sum(nx2)), kEps), iyj = inv_norm(sqrtf(wave_sum(ny2)), kEps);
                acc[4] += (double)hinge(wave_sum(dxx) * ix * ixj - thr);
                acc[5] += (double)hinge(wave_sum(dyy) * iy * iyj - thr);
                acc[6] += (double)hinge(wave_sum(dxy) * ix * iyj - thr);
            }
        }
    }
    if (lane == 0) {
        for (int t = 0; t < 7; ++t) red[wave][t] = acc[t];
        zred[wave] = z;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const int t = threadIdx.x;
        double s = 0.0;
        if (t < 7)
            for (int w = 0; w < kWaves; ++w) s += red[w][t];
        if (kLoss) ws.part[(int64_t)i * 8 + t] = s;
        if (t == 0) {
            int zs = 0;
            for (int w = 0; w < kWaves; ++w) zs += zred[w];
            ws.cnt[2 * i] = npos;
            ws.cnt[2 * i + 1] = zs;
            ws.nx[i] = nxi;
            ws.ny[i] = nyi;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_hyp_finalize(int B, int C, float alpha, WsView ws, double* __restrict__ out8) {
    __shared__ double sh[kWaves];
    double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = threadIdx.x; r < B; r += kThreads) {
        for (int t = 0; t < 7; ++t) s[t] += ws.part[(int64_t)r * 8 + t];
        s[7] += (double)ws.cnt[2 * r];
        s[8] += (double)ws.cnt[2 * r + 1];
    }
    for (int t = 0; t < 9; ++t) s[t] = xmh::block_sum<kWaves>(s[t], sh);   // counts: exact in double
    if (threadIdx.x == 0) {
        const double pn = s[7], nn = (double)B * (double)C - s[7], z = s[8];
        const double pos = s[0] / pn, neg = s[1] / nn, pos_t = s[2] / pn, neg_t = s[3] / nn;   // 0 / 0 = NaN, as the reference
        const double a = (double)alpha;
        const double reg = z > 0.0 ? a * s[4] / z : 0.0, reg_t = z > 0.0 ? a * s[5] / z : 0.0, reg_xt = z > 0.0 ? a * s[6] / z : 0.0;
        out8[0] = pos + neg + pos_t + neg_t + reg + reg_t + reg_xt;
        out8[1] = pos;
        out8[2] = neg;
        out8[3] = pos_t;
        out8[4] = neg_t;
        out8[5] = reg;
        out8[6] = reg_t;
        out8[7] = reg_xt;
    }
}

// Blocks [0, B): grad_x[i], grad_y[i].  Blocks [B, B + C): grad_P[c].  The global counts come from k_hyp_rows<false>.
__global__ __launch_bounds__(kThreads) void k_hyp_grad(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ P,
                                                       int B, int K, int C, const uint32_t* __restrict__ lab, int Lw, float thr, float alpha,
                                                       WsView ws, const float* __restrict__ up, float* __restrict__ gx,
                                                       float* __restrict__ gy, float* __restrict__ gP, int accumulate) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double dsh[kWaves];
    __shared__ float fsh[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double pn = 0.0, z = 0.0;
    for (int r = threadIdx.x; r < B; r += kThreads) {
        pn += (double)ws.cnt[2 * r];
        z += (double)ws.cnt[2 * r + 1];
    }
    pn = xmh::block_sum<kWaves>(pn, dsh);
    z = xmh::block_sum<kWaves>(z, dsh);
    const double nn = (double)B * (double)C - pn;
    // d loss / d cos: -1 / P_num on a label, [cos > thr] / N_num off it; d loss / d sim: alpha / Z on a pair
    const float wpos = pn > 0.0 ? (float)(-1.0 / pn) : 0.0f, wneg = nn > 0.0 ? (float)(1.0 / nn) : 0.0f;
    const float wreg = z > 0.0 ? (float)((double)alpha / z) : 0.0f;
    const float g = up ? up[0] : 1.0f;
    float ax[kSlots], ay[kSlots];
#pragma unroll
    for (int r = 0; r < kSlots; ++r) ax[r] = ay[r] = 0.0f;

    if ((int)blockIdx.x < B) {
        const int i = blockIdx.x;
        float* xs = smem;
        float* ys = xs + K;
        float* cw = ys + K;                                      // [C] weight of P_c in d/dx_i (d loss/d cos times 1/|P_c|)
        float* ctw = cw + C;                                     // [C] the same for y_i
        float* pw = ctw + C;                                     // [4][kChunk] pair weights of a chunk of partners
        for (int k = threadIdx.x; k < K; k += kThreads) {
            xs[k] = x[(int64_t)i * K + k];
            ys[k] = y[(int64_t)i * K + k];
        }
        const float ix = inv_norm(ws.nx[i], kEps), iy = inv_norm(ws.ny[i], kEps);
        __syncthreads();
        for (int c = wave; c < C; c += kWaves) {
            const float ip = inv_norm(ws.np[c], kEps);
            float a = wpos * ip, b = wpos * ip;
            if (!has_label(lab, Lw, i, c)) {
                const float* pc = P + (int64_t)c * K;
                float d = 0.0f, dt = 0.0f;
                for (int k = lane; k < K; k += 64) {
                    const float p = pc[k];
                    d = fmaf(xs[k], p, d);
                    dt = fmaf(ys[k], p, dt);
                }
                a = hinge_weight(wave_sum(d) * ix * ip, thr, wneg * ip);
                b = hinge_weight(wave_sum(dt) * iy * ip, thr, wneg * ip);
            }
            if (lane == 0) {
                cw[c] = a;
                ctw[c] = b;
            }
        }
        __syncthreads();
        for (int c = 0; c < C; ++c) {
            const float a = cw[c], b = ctw[c];
            // nothing to add; a NaN weight is not skipped, nor the +-0 weights of a proxy with an Inf norm (0 * Inf = NaN)
            if (a == 0.0f && b == 0.0f && !isinf(ws.np[c])) continue;
            const float* pc = P + (int64_t)c * K;
#pragma unroll
            for (int r = 0; r < kSlots; ++r) {
                const int k = threadIdx.x + r * kThreads;
                if (k < K) {
                    const float p = pc[k];
                    ax[r] = fmaf(a, p, ax[r]);
                    ay[r] = fmaf(b, p, ay[r]);
                }
            }
        }
        if (wreg != 0.0f && ws.cnt[2 * i] >= 2) {
            const uint32_t mine = lane < Lw ? lab[(int64_t)i * Lw + lane] : 0u;
            for (int j0 = 0; j0 < B; j0 += kChunk) {
                const int n = min(kChunk, B - j0);
                // The first chunk goes on from the proxies' sums; every later chunk is summed from zero and then added.  The partners of
                // a row point much the same way, so a running fp32 sum loses bits with its length: at B = 513 one chain over all
                // partners was 3.9 times the reference's own fp32 error in d/dx, against 2.5 - 3.7 at B <= 300.
                float tx[kSlots], ty[kSlots];
#pragma unroll
                for (int r = 0; r < kSlots; ++r) {
                    tx[r] = j0 == 0 ? ax[r] : 0.0f;
                    ty[r] = j0 == 0 ? ay[r] : 0.0f;
                }
                for (int jj = wave; jj < n; jj += kWaves) {
                    const int j = j0 + jj;
                    const uint32_t w = lane < Lw ? lab[(int64_t)j * Lw + lane] : 0u;
                    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
                    const Partner pj = partner_of(mine, w);
                    if (pj.disjoint) {
                        const float* xj = x + (int64_t)j * K;
                        const float* yj = y + (int64_t)j * K;
                        float dxx = 0.0f, dyy = 0.0f, dxy = 0.0f, dyx = 0.0f;
                        for (int k = lane; k < K; k += 64) {
                            const float a = xj[k], b = yj[k];
                            dxx = fmaf(xs[k], a, dxx);
                            dyy = fmaf(ys[k], b, dyy);
                            dxy = fmaf(xs[k], b, dxy);
                            dyx = fmaf(a, ys[k], dyx);               // x_j . y_i, the order the forward forms it for row j
                        }
                        const float ixj = inv_norm(ws.nx[j], kEps), iyj = inv_norm(ws.ny[j], kEps);
                        // x-x and y-y: the pair masks are symmetric, so row i collects both (i, j) and (j, i)
                        c0 = hinge_weight(wave_sum(dxx) * ix * ixj, thr, 2.0f * wreg * ixj);   // x_j into d/dx_i
                        c1 = hinge_weight(wave_sum(dxy) * ix * iyj, thr, wreg * iyj);          // y_j into d/dx_i (x-y term, i first)
                        c2 = hinge_weight(wave_sum(dyy) * iy * iyj, thr, 2.0f * wreg * iyj);   // y_j into d/dy_i
                        c3 = hinge_weight(wave_sum(dyx) * ixj * iy, thr, wreg * ixj);          // x_j into d/dy_i (x-y term, i second)
                    } else if (pj.in_m) {
                        // a masked pair of M x M (i itself among them): weight 0 in the reference's products n(x_M) n(x_M)^T ..., which still
                        // multiply row j in.  0 * norm is 0 for a finite norm (skipped below) and NaN for a NaN or Inf one.
                        c0 = c3 = 0.0f * ws.nx[j];
                        c1 = c2 = 0.0f * ws.ny[j];
                    }
                    if (lane == 0) {
                        pw[jj] = c0;
                        pw[kChunk + jj] = c1;
                        pw[2 * kChunk + jj] = c2;
                        pw[3 * kChunk + jj] = c3;
                    }
                }
                __syncthreads();
                for (int jj = 0; jj < n; ++jj) {
                    const float c0 = pw[jj], c1 = pw[kChunk + jj], c2 = pw[2 * kChunk + jj], c3 = pw[3 * kChunk + jj];
                    if (c0 == 0.0f && c1 == 0.0f && c2 == 0.0f && c3 == 0.0f) continue;
                    const float* xj = x + (int64_t)(j0 + jj) * K;
                    const float* yj = y + (int64_t)(j0 + jj) * K;
#pragma unroll
                    for (int r = 0; r < kSlots; ++r) {
                        const int k = threadIdx.x + r * kThreads;
                        if (k < K) {
                            const float a = xj[k], b = yj[k];
                            tx[r] = fmaf(c1, b, fmaf(c0, a, tx[r]));
                            ty[r] = fmaf(c3, a, fmaf(c2, b, ty[r]));
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < kSlots; ++r) {
                    ax[r] = j0 == 0 ? tx[r] : ax[r] + tx[r];
                    ay[r] = j0 == 0 ? ty[r] : ay[r] + ty[r];
                }
                __syncthreads();
            }
        }
        xmh::normalize_backward_store<kThreads>(xs, ws.nx[i], kEps, ax, K, g, gx + (int64_t)i * K, accumulate, fsh);
        xmh::normalize_backward_store<kThreads>(ys, ws.ny[i], kEps, ay, K, g, gy + (int64_t)i * K, accumulate, fsh);
    } else {
        const int c = blockIdx.x - B;
        float* ps = smem;                                        // P_c
        float* wx = ps + K;                                      // [kChunk] weight of x_i in d/dP_c
        float* wy = wx + kChunk;                                 // [kChunk] weight of y_i
        for (int k = threadIdx.x; k < K; k += kThreads) ps[k] = P[(int64_t)c * K + k];
        const float ip = inv_norm(ws.np[c], kEps);
        __syncthreads();
        for (int i0 = 0; i0 < B; i0 += kChunk) {
            const int n = min(kChunk, B - i0);
            for (int ii = wave; ii < n; ii += kWaves) {
                const int i = i0 + ii;
                const float ixi = inv_norm(ws.nx[i], kEps), iyi = inv_norm(ws.ny[i], kEps);
                float a = wpos * ixi, b = wpos * iyi;
                if (!has_label(lab, Lw, i, c)) {
                    const float* xi = x + (int64_t)i * K;
                    const float* yi = y + (int64_t)i * K;
                    float d = 0.0f, dt = 0.0f;
                    for (int k = lane; k < K; k += 64) {
                        const float p = ps[k];
                        d = fmaf(xi[k], p, d);
                        dt = fmaf(yi[k], p, dt);
                    }
                    a = hinge_weight(wave_sum(d) * ixi * ip, thr, wneg * ixi);
                    b = hinge_weight(wave_sum(dt) * iyi * ip, thr, wneg * iyi);
                }
                if (lane == 0) {
                    wx[ii] = a;
                    wy[ii] = b;
                }
            }
            __syncthreads();
            for (int ii = 0; ii < n; ++ii) {
                const float a = wx[ii], b = wy[ii];
                if (a == 0.0f && b == 0.0f && !isinf(ws.nx[i0 + ii]) && !isinf(ws.ny[i0 + ii])) continue;   // as in the row blocks
                const float* xi = x + (int64_t)(i0 + ii) * K;
                const float* yi = y + (int64_t)(i0 + ii) * K;
#pragma unroll
                for (int r = 0; r < kSlots; ++r) {
                    const int k = threadIdx.x + r * kThreads;
                    if (k < K) ax[r] = fmaf(b, yi[k], fmaf(a, xi[k], ax[r]));
                }
            }
            __syncthreads();
        }
        xmh::normalize_backward_store<kThreads>(ps, ws.np[c], kEps, ax, K, g, gP + (int64_t)c * K, accumulate, fsh);
    }
}

// shared argument checks of both entry points: they run before any HIP call
int check_args(const char* who, const float* x, const float* y, const float* P, int64_t B, int K, int C, const uint32_t* lab, void* ws,
               size_t ws_bytes) {
    if (B <= 0 || K <= 0 || C <= 0) return xmh::fail(XMH_EINVAL, "%s: bad shape B=%lld K=%d C=%d", who, (long long)B, K, C);
    if (B > kMaxB || K > kMaxK || C > kMaxC)
        return xmh::fail(XMH_ENOTSUP, "%s: B=%lld K=%d C=%d outside B <= %d, K <= %d, C <= %d", who, (long long)B, K, C, kMaxB, kMaxK, kMaxC);
    if (!x || !y || !P || !lab || !ws) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    return xmh::check_workspace(who, ws, ws_bytes, ws_layout(B, C, nullptr, nullptr), "xmh_hyp_loss_ws_bytes", XMH_EINVAL);
}

}  // namespace

extern "C" size_t xmh_hyp_loss_ws_bytes(int64_t B, int K, int C) {
    if (B <= 0 || K <= 0 || C <= 0 || B > kMaxB || K > kMaxK || C > kMaxC) return 0;
    return ws_layout(B, C, nullptr, nullptr);
}

extern "C" int xmh_hyp_loss(const float* x, const float* y, const float* P, int64_t B, int K, int C, const uint32_t* lab, float threshold,
                            float alpha, void* ws, size_t ws_bytes, double* out8, xmh_stream_t stream) {
    XMH_RANGE("xmh_hyp_loss");
    if (int rc = check_args("xmh_hyp_loss", x, y, P, B, K, C, lab, ws, ws_bytes)) return rc;
    if (!out8) return xmh::fail(XMH_EINVAL, "xmh_hyp_loss: null pointer");
    WsView v;
    ws_layout(B, C, ws, &v);
    hipStream_t st = xmh::as_stream(stream);
    hipLaunchKernelGGL(k_hyp_rows<true>, dim3((unsigned)(B + C)), dim3(kThreads), (size_t)2 * K * 4, st, x, y, P, (int)B, K, C, lab,
                       (C + 31) / 32, threshold, alpha, v);
    hipLaunchKernelGGL(k_hyp_finalize, dim3(1), dim3(kThreads), 0, st, (int)B, C, alpha, v, out8);
    XMH_LAUNCH_CHECK("xmh_hyp_loss");
    return XMH_OK;
}

extern "C" int xmh_hyp_loss_grad(const float* x, const float* y, const float* P, int64_t B, int K, int C, const uint32_t* lab,
                                 float threshold, float alpha, const float* upstream, float* grad_x, float* grad_y, float* grad_P,
                                 int accumulate, void* ws, size_t ws_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_hyp_loss_grad");
    if (int rc = check_args("xmh_hyp_loss_grad", x, y, P, B, K, C, lab, ws, ws_bytes)) return rc;
    if (!grad_x || !grad_y || !grad_P) return xmh::fail(XMH_EINVAL, "xmh_hyp_loss_grad: null pointer");
    WsView v;
    ws_layout(B, C, ws, &v);
    hipStream_t st = xmh::as_stream(stream);
    hipLaunchKernelGGL(k_hyp_rows<false>, dim3((unsigned)(B + C)), dim3(kThreads), (size_t)2 * K * 4, st, x, y, P, (int)B, K, C, lab,
                       (C + 31) / 32, threshold, alpha, v);
    const size_t lds = ((size_t)2 * K + (size_t)2 * C + 4 * kChunk) * 4;   // <= 45 KB at K = 4096, C = 1024
    hipLaunchKernelGGL(k_hyp_grad, dim3((unsigned)(B + C)), dim3(kThreads), lds, st, x, y, P, (int)B, K, C, lab, (C + 31) / 32,
                       threshold, alpha, v, upstream, grad_x, grad_y, grad_P, accumulate);
    XMH_LAUNCH_CHECK("xmh_hyp_loss_grad");
    return XMH_OK;
}
