// UMoED: the soft-MoE decoder head in train mode and its backward (reference models/UMoED/hash/block/transformer.py SoftMoEDecoderLayer,
// hash/block/SoftMoe.py, hash/hash_moe.py TokenHash).  MoE layers without a first layer.
//
//   forward (xmh_head_umoed_train_forward): forward_chain of xmh_umoed_head.h, the buffers of every layer in the caller's record.  Without a
//     keep mask: the launches and the arithmetic of xmh_head_umoed, 16 per layer.  With one: 20 per layer -- the self-attention runs in
//     k_umoed_attn<true> as the cross-attention does, and each of the three sublayer outputs and the ReLU rows takes one elementwise launch.
//   record, per layer: qkv, att1, u1, x1, q, kv, att2, u2, x2, h (after the dropout), D, Cw, Xs, Ys, u3, and the layer's output; u1, u2, u3
//     are the LayerNorm inputs.  The attention probabilities are NOT kept: k_umoed_attn_bwd recomputes them from q and k by the forward
//     kernel's own chain (2 (M + T) B H M floats per layer saved, 47 MB at the configuration's shape).
//   backward (xmh_head_umoed_backward), from d_embeds: the classifier, then the layers last to first.  Per layer
//     LN3'  ->  du3;  dY = du3 . keep6 / (1 - p)
//     dCw = dY Ys^T,  dYs = Cw^T dY (expert-major),  dW_n = Xs_n^T dYs_n per expert (grad::weight_grads: split in order),  db_n (k_umoed_expert_bias),
//     dXs = dYs W_n^T,  dD = h dXs^T,  k_umoed_route_bwd -> dlogits,  dh = D dXs + dlogits phi^T,  dphi = h^T dlogits,
//     relu' . keep5,  the linear's gradients,  dx2 = dpre W + du3
//     LN2'  ->  du2;  out_proj backward;  k_umoed_attn_bwd (dq, dk | dv);  the two halves of ca_in_w;  d_tokens (+)= dkv W_kv;  dx1 = dq W_q + du2
//     LN1'  ->  du1;  out_proj backward;  k_umoed_attn_bwd on the packed qkv;  sa_in_w;  dx = dqkv W + du1
//     d_queries = the ordered sum over B of layer 0's dx.
//   k_umoed_attn_bwd: block (sample, head).  Phase 1, a thread per query row i: the row's maximum and sum, then per key j P, dP =
//     (dO_i . V_j) keep / (1 - p), delta_i = sum_j dP P, then dS = P (dP - delta_i) and dq_i = sum_j dS K_j / 8; P and dS go to two
//     [M, T] tables in the workspace.  Phase 2, a thread per key row j: dk_j = sum_i dS_ij q_i / 8, dv_j = sum_i P_ij keep / (1 - p) dO_i,
//     i in order.  K, V (phase 1) and q, dO (phase 2) of the head share one LDS region of 2 max(M, T) 64 floats (64 KiB at 128).
//   k_umoed_route_bwd: block = sample.  A thread per slot sums dD . D down its column, a wave per row sums dCw . Cw along it (both into
//     LDS, 1.5 KB), then dlogits = D (dD - colsum) + Cw (dCw - rowsum) elementwise; the four tables are read from global memory twice
//     (the second time from L2) instead of staging 4 x 128 KiB in LDS.
//
// Exact fp32 (the tile core of xmh_mfma_mm.h, fmaf chains), no allocation, no host synchronisation, no float atomics, one fixed order per sum.
#include "xmh_grad_kernels.h"
#include "xmh_umoed_head.h"

namespace {

namespace grad = xmh::grad;
using namespace umoed;
static_assert(umoed::kThreads == grad::kThreads, "one block size");

// ---- the record -------------------------------------------------------------------------------------------------------------------------
struct Record {
    float* x0;                // [B M, d] the queries repeated
    size_t layer0, stride;    // byte offset of layer 0's buffers and the bytes of a layer
    char* base;
};

size_t layer_layout(int64_t B, int T, const xmh_umoed_head* h, void* base, LayerBufs* v) {
    xmh::Arena ar(base);
    const size_t BM = (size_t)B * h->M, BT = (size_t)B * T, d = (size_t)h->d, S = (size_t)h->n_experts * h->slots;
    LayerBufs w = {};
    w.qkv = ar.take<float>(BM * 3 * d);
    w.att1 = ar.take<float>(BM * d);
    w.u1 = ar.take<float>(BM * d);
    w.x1 = ar.take<float>(BM * d);
    w.q = ar.take<float>(BM * d);
    w.kv = ar.take<float>(BT * 2 * d);
    w.att2 = ar.take<float>(BM * d);
    w.u2 = ar.take<float>(BM * d);
    w.x2 = ar.take<float>(BM * d);
    w.h = ar.take<float>(BM * h->F);
    w.Dw = ar.take<float>(BM * S);
    w.Cw = ar.take<float>(BM * S);
    w.Xs = ar.take<float>((size_t)B * S * h->F);
    w.Ys = ar.take<float>((size_t)B * S * d);
    w.u3 = ar.take<float>(BM * d);
    w.xo = ar.take<float>(BM * d);
    if (v) *v = w;
    return ar.used;
}

size_t record_layout(int64_t B, int T, const xmh_umoed_head* h, void* base, Record* r) {
    xmh::Arena ar(base);
    Record v;
    v.base = static_cast<char*>(base);
    v.x0 = ar.take<float>((size_t)B * h->M * h->d);
    v.layer0 = ar.used;
    v.stride = layer_layout(B, T, h, nullptr, nullptr);
    if (r) *r = v;
    return v.layer0 + v.stride * (size_t)h->n_layers;
}

LayerBufs record_layer(int64_t B, int T, const xmh_umoed_head* h, const Record& r, int l) {
    LayerBufs w;
    layer_layout(B, T, h, r.base + r.layer0 + r.stride * (size_t)l, &w);
    return w;
}

// ---- the workspace: the forward's two buffers and the backward's ----------------------------------------------------------------------
struct TrainWs {
    float *lg, *tmp;                                              // forward
    float *dx, *du, *t1, *t2, *dqkv, *dkv, *dtok, *dh, *dCw, *dD, *dlg, *dYs, *dXs, *Pt, *dSt;
    grad::GradScratch gs;
};

size_t ws_layout(int64_t B, int T, const xmh_umoed_head* h, void* base, TrainWs* v) {
    xmh::Arena ar(base);
    const size_t BM = (size_t)B * h->M, BT = (size_t)B * T, d = (size_t)h->d, S = (size_t)h->n_experts * h->slots, F = (size_t)h->F;
    const size_t L = (size_t)(h->M > T ? h->M : T);
    TrainWs w;
    w.lg = ar.take<float>(BM * S);
    w.tmp = ar.take<float>(BM * d);
    w.dx = ar.take<float>(BM * d);
    w.du = ar.take<float>(BM * d);
    w.t1 = ar.take<float>(BM * d);
    w.t2 = ar.take<float>(BM * d);
    w.dqkv = ar.take<float>(BM * 3 * d);
    w.dkv = ar.take<float>(BT * 2 * d);
    w.dtok = ar.take<float>(BT * d);
    w.dh = ar.take<float>(BM * F);
    w.dCw = ar.take<float>(BM * S);
    w.dD = ar.take<float>(BM * S);
    w.dlg = ar.take<float>(BM * S);
    w.dYs = ar.take<float>((size_t)B * S * d);
    w.dXs = ar.take<float>((size_t)B * S * F);
    w.Pt = ar.take<float>((size_t)B * h->heads * h->M * L);
    w.dSt = ar.take<float>((size_t)B * h->heads * h->M * L);
    const int64_t rows = (int64_t)BM, trows = (int64_t)BT, erows = B * h->slots;
    const grad::TnShape tn[] = {{rows, h->V, h->d},     {rows, h->F, (int)S}, {erows, h->F, h->d},    {rows, h->F, h->d},
                                {rows, h->d, h->d},     {trows, 2 * h->d, h->d}, {rows, 3 * h->d, h->d}};
    const int bias_width = 3 * h->d > h->F ? 3 * h->d : h->F;
    grad::take_scratch(ar, rows, h->d, bias_width > h->V ? bias_width : h->V, tn, &w.gs);
    if (v) *v = w;
    return ar.used;
}

// what the train entry points take beyond head_shape
int train_shape(const char* who, const xmh_umoed_head* h) {
#define UMOED_FAIL(code, ...) return who ? xmh::fail(code, __VA_ARGS__) : code
    if (!h->moe) UMOED_FAIL(XMH_ENOTSUP, "%s: the plain decoder (moe == 0) has no train mode; only the Soft-MoE layers do", who);
    if (h->first_w) UMOED_FAIL(XMH_ENOTSUP, "%s: a first layer (first_w) has no train mode", who);
    if (h->ln_eps != grad::kLnEps) UMOED_FAIL(XMH_ENOTSUP, "%s: ln_eps %g (the LayerNorm backward assumes 1e-5)", who, (double)h->ln_eps);
#undef UMOED_FAIL
    return XMH_OK;
}

// ---- attention backward -----------------------------------------------------------------------------------------------------------------
// Rows as in k_umoed_attn; dO [B M, H 64]; dq row (b, i) at dq + (b M + i) lddq, dk row (b, j) at dk + (b T + j) lddkv, dv row dvoff behind
// it.  Pt, dSt: [B H][M][T] tables of the workspace.
template <bool KEEP>
__global__ __launch_bounds__(kAttnThreads) void k_umoed_attn_bwd(const float* __restrict__ q, int64_t ldq, const float* __restrict__ kp, int64_t ldkv, int voff,
                                                                 const float* __restrict__ dO, int M, int T, int H, const uint8_t* __restrict__ keep, float ks,
                                                                 float* Pt, float* dSt, float* __restrict__ dq, int64_t lddq, float* __restrict__ dk,
                                                                 int64_t lddkv, int dvoff) {
    constexpr int DH = 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int D = H * DH;
    const int L = M > T ? M : T;
    float4* sA = reinterpret_cast<float4*>(smem);                    // phase 1: K [T][16]; phase 2: q / 8 [M][16]
    float4* sB = sA + L * (DH / 4);                                  // phase 1: V [T][16]; phase 2: dO [M][16]
    const float scale = rsqrtf((float)DH);
    const float* kb = kp + (int64_t)b * T * ldkv + h * DH;
    for (int e = threadIdx.x; e < T * (DH / 4); e += blockDim.x) {
        const int j = e / (DH / 4), c4 = e % (DH / 4);
        sA[e] = *reinterpret_cast<const float4*>(kb + (int64_t)j * ldkv + c4 * 4);
        sB[e] = *reinterpret_cast<const float4*>(kb + (int64_t)j * ldkv + voff + c4 * 4);
    }
    __syncthreads();
    float* Pb = Pt + (int64_t)blockIdx.x * M * T;
    float* Sb = dSt + (int64_t)blockIdx.x * M * T;
    const uint8_t* kpb = KEEP ? keep + (int64_t)blockIdx.x * M * T : nullptr;
    if (const int i = threadIdx.x; i < M) {
        const int64_t row = (int64_t)b * M + i;
        float qr[DH];
#pragma unroll
        for (int c = 0; c < DH / 4; ++c) {
            const float4 v = *reinterpret_cast<const float4*>(q + row * ldq + h * DH + c * 4);
            qr[4 * c + 0] = v.x * scale, qr[4 * c + 1] = v.y * scale, qr[4 * c + 2] = v.z * scale, qr[4 * c + 3] = v.w * scale;
        }
        auto score = [&](int j) {                                    // k_umoed_attn's chain
            float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
            for (int c = 0; c < DH / 4; ++c) {
                const float4 kk = sA[j * (DH / 4) + c];
                s0 = fmaf(qr[4 * c + 0], kk.x, s0);
                s1 = fmaf(qr[4 * c + 1], kk.y, s1);
                s0 = fmaf(qr[4 * c + 2], kk.z, s0);
                s1 = fmaf(qr[4 * c + 3], kk.w, s1);
            }
            return s0 + s1;
        };
        float mx = -INFINITY;
        for (int j = 0; j < T; ++j) mx = fmaxf(mx, score(j));
        float sum = 0.0f;
        for (int j = 0; j < T; ++j) sum += expf(score(j) - mx);
        const float inv = 1.0f / sum;
        float delta = 0.0f;
        {
            float go[DH];
#pragma unroll
            for (int c = 0; c < DH / 4; ++c) {
                const float4 v = *reinterpret_cast<const float4*>(dO + row * D + h * DH + c * 4);
                go[4 * c + 0] = v.x, go[4 * c + 1] = v.y, go[4 * c + 2] = v.z, go[4 * c + 3] = v.w;
            }
            for (int j = 0; j < T; ++j) {
                const float P = expf(score(j) - mx) * inv;
                float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
                for (int c = 0; c < DH / 4; ++c) {
                    const float4 vv = sB[j * (DH / 4) + c];
                    s0 = fmaf(go[4 * c + 0], vv.x, s0);
                    s1 = fmaf(go[4 * c + 1], vv.y, s1);
                    s0 = fmaf(go[4 * c + 2], vv.z, s0);
                    s1 = fmaf(go[4 * c + 3], vv.w, s1);
                }
                float dP = s0 + s1;
                if (KEEP) dP = kpb[i * T + j] ? dP * ks : 0.0f;
                Pb[i * T + j] = P;
                Sb[i * T + j] = dP;
                delta = fmaf(dP, P, delta);
            }
        }
        float acc[DH];
#pragma unroll
        for (int c = 0; c < DH; ++c) acc[c] = 0.0f;
        for (int j = 0; j < T; ++j) {
            const float dS = Pb[i * T + j] * (Sb[i * T + j] - delta);
            Sb[i * T + j] = dS;
#pragma unroll
            for (int c = 0; c < DH / 4; ++c) {
                const float4 kk = sA[j * (DH / 4) + c];
                acc[4 * c + 0] = fmaf(dS, kk.x, acc[4 * c + 0]);
                acc[4 * c + 1] = fmaf(dS, kk.y, acc[4 * c + 1]);
                acc[4 * c + 2] = fmaf(dS, kk.z, acc[4 * c + 2]);
                acc[4 * c + 3] = fmaf(dS, kk.w, acc[4 * c + 3]);
            }
        }
#pragma unroll
        for (int c = 0; c < DH / 4; ++c)
            *reinterpret_cast<float4*>(dq + row * lddq + h * DH + c * 4) =
                make_float4(acc[4 * c + 0] * scale, acc[4 * c + 1] * scale, acc[4 * c + 2] * scale, acc[4 * c + 3] * scale);
    }
    __threadfence_block();
    __syncthreads();                                                 // the tables are complete and K, V are no longer read
    for (int e = threadIdx.x; e < M * (DH / 4); e += blockDim.x) {
        const int i = e / (DH / 4), c4 = e % (DH / 4);
        const int64_t row = (int64_t)b * M + i;
        const float4 v = *reinterpret_cast<const float4*>(q + row * ldq + h * DH + c4 * 4);
        sA[e] = make_float4(v.x * scale, v.y * scale, v.z * scale, v.w * scale);
        sB[e] = *reinterpret_cast<const float4*>(dO + row * D + h * DH + c4 * 4);
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j >= T) return;
    float gk[DH], gv[DH];
#pragma unroll
    for (int c = 0; c < DH; ++c) gk[c] = gv[c] = 0.0f;
    for (int i = 0; i < M; ++i) {                                    // lanes walk j: the table rows are read coalesced
        const float dS = Sb[i * T + j];
        float Pd = Pb[i * T + j];
        if (KEEP) Pd = kpb[i * T + j] ? Pd * ks : 0.0f;
#pragma unroll
        for (int c = 0; c < DH / 4; ++c) {
            const float4 qq = sA[i * (DH / 4) + c], oo = sB[i * (DH / 4) + c];
            gk[4 * c + 0] = fmaf(dS, qq.x, gk[4 * c + 0]);
            gk[4 * c + 1] = fmaf(dS, qq.y, gk[4 * c + 1]);
            gk[4 * c + 2] = fmaf(dS, qq.z, gk[4 * c + 2]);
            gk[4 * c + 3] = fmaf(dS, qq.w, gk[4 * c + 3]);
            gv[4 * c + 0] = fmaf(Pd, oo.x, gv[4 * c + 0]);
            gv[4 * c + 1] = fmaf(Pd, oo.y, gv[4 * c + 1]);
            gv[4 * c + 2] = fmaf(Pd, oo.z, gv[4 * c + 2]);
            gv[4 * c + 3] = fmaf(Pd, oo.w, gv[4 * c + 3]);
        }
    }
    float* out = dk + ((int64_t)b * T + j) * lddkv + h * DH;
#pragma unroll
    for (int c = 0; c < DH / 4; ++c) {
        *reinterpret_cast<float4*>(out + c * 4) = make_float4(gk[4 * c + 0], gk[4 * c + 1], gk[4 * c + 2], gk[4 * c + 3]);
        *reinterpret_cast<float4*>(out + dvoff + c * 4) = make_float4(gv[4 * c + 0], gv[4 * c + 1], gv[4 * c + 2], gv[4 * c + 3]);
    }
}

void attn_bwd(hipStream_t st, const float* q, int64_t ldq, const float* kp, int64_t ldkv, int voff, const float* dO, int64_t B, int M, int T, int H,
              const uint8_t* keep, float ks, const TrainWs& w, float* dq, int64_t lddq, float* dk, int64_t lddkv, int dvoff) {
    const size_t lds = attn_lds(M > T ? M : T);
    if (keep)
        hipLaunchKernelGGL(k_umoed_attn_bwd<true>, dim3((unsigned)(B * H)), dim3(kAttnThreads), lds, st, q, ldq, kp, ldkv, voff, dO, M, T, H, keep, ks, w.Pt,
                           w.dSt, dq, lddq, dk, lddkv, dvoff);
    else
        hipLaunchKernelGGL(k_umoed_attn_bwd<false>, dim3((unsigned)(B * H)), dim3(kAttnThreads), lds, st, q, ldq, kp, ldkv, voff, dO, M, T, H, keep, ks, w.Pt,
                           w.dSt, dq, lddq, dk, lddkv, dvoff);
}

// ---- routing backward: block = sample ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_umoed_route_bwd(const float* __restrict__ Dw, const float* __restrict__ Cw, const float* __restrict__ dD,
                                                              const float* __restrict__ dCw, int M, int S, float* __restrict__ dlg) {
    __shared__ float cs[kMaxS], rs[kMaxM];
    const int64_t base = (int64_t)blockIdx.x * M * S;
    for (int s = threadIdx.x; s < S; s += kThreads) {                // a thread per slot: the M rows in order, lanes walk s
        float a = 0.0f;
        for (int m = 0; m < M; ++m) a = fmaf(dD[base + (int64_t)m * S + s], Dw[base + (int64_t)m * S + s], a);
        cs[s] = a;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int m = wave; m < M; m += kWaves) {                         // a wave per row
        float a = 0.0f;
        for (int s = lane; s < S; s += 64) a = fmaf(dCw[base + (int64_t)m * S + s], Cw[base + (int64_t)m * S + s], a);
        a = wave_sum(a);
        if (lane == 0) rs[m] = a;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < M * S; e += kThreads) {
        const int m = e / S, s = e % S;
        dlg[base + e] = Dw[base + e] * (dD[base + e] - cs[s]) + Cw[base + e] * (dCw[base + e] - rs[m]);
    }
}

// ---- elementwise ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_umoed_keep_scale(const float* __restrict__ g, const uint8_t* __restrict__ keep, float ks, int64_t n,
                                                               float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e < n) out[e] = keep[e] ? g[e] * ks : 0.0f;
}
__global__ __launch_bounds__(kThreads) void k_umoed_add(float* __restrict__ a, const float* __restrict__ b, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e < n) a[e] += b[e];
}
// h is relu(pre) keep / (1 - p): positive exactly where the ReLU passed and the row was kept
__global__ __launch_bounds__(kThreads) void k_umoed_relu_bwd(float* __restrict__ dh, const float* __restrict__ h, float ks, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e < n) dh[e] = h[e] > 0.0f ? dh[e] * ks : 0.0f;
}
// db[n][c] (+)= sum over the rows (b, p) of expert n of dYs[n][(b, p)][c]: one launch for every expert.  Grid (column groups, experts); a
// block sums kCols columns in kGroups interleaved row groups, in double, the groups added in index order.
constexpr int kCols = 32, kGroups = kThreads / kCols;
__global__ __launch_bounds__(kThreads) void k_umoed_expert_bias(const float* __restrict__ dYs, int64_t rows, int d, float* db, int accumulate) {
    __shared__ double sh[kGroups][kCols];
    const int col = threadIdx.x % kCols, grp = threadIdx.x / kCols, c = blockIdx.x * kCols + col;
    const float* src = dYs + (int64_t)blockIdx.y * rows * d;
    double a = 0.0;
    if (c < d)
        for (int64_t r = grp; r < rows; r += kGroups) a += (double)src[r * d + c];
    const double s = xmh::group_sum(a, sh, col, grp);
    if (c < d && grp == 0) {
        float* out = db + (int64_t)blockIdx.y * d + c;
        *out = accumulate ? *out + (float)s : (float)s;
    }
}
// out[e] (+)= sum_b x[b per + e], b in order
__global__ __launch_bounds__(kThreads) void k_umoed_batch_sum(const float* __restrict__ x, int64_t B, int64_t per, float* __restrict__ out, int accumulate) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= per) return;
    float s = x[e];
    for (int64_t b = 1; b < B; ++b) s += x[b * per + e];
    out[e] = accumulate ? out[e] + s : s;
}

int check_train(const char* who, const xmh_umoed_head* h, const float* tokens, const uint8_t* keep, float p, int64_t B, int T, const void* saved,
                size_t saved_bytes, const void* ws, size_t ws_bytes) {
    if (int rc = head_shape(who, B, T, h)) return rc;
    if (int rc = train_shape(who, h)) return rc;
    if (keep && !(p >= 0.0f && p < 1.0f)) return xmh::fail(XMH_EINVAL, "%s: dropout p %g outside [0, 1)", who, (double)p);
    if (!tokens || !saved || !ws) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    XMH_TRY(head_pointers(who, h));
    XMH_TRY(xmh::check_workspace(who, saved, saved_bytes, record_layout(B, T, h, nullptr, nullptr), "xmh_head_umoed_train_bytes", XMH_ENOMEM));
    return xmh::check_workspace(who, ws, ws_bytes, ws_layout(B, T, h, nullptr, nullptr), "xmh_head_umoed_train_bytes", XMH_ENOMEM);
}

}  // namespace

extern "C" size_t xmh_head_umoed_train_bytes(int64_t B, int T, const xmh_umoed_head* h, size_t* workspace_bytes) {
    if (workspace_bytes) *workspace_bytes = 0;
    if (head_shape(nullptr, B, T, h) || train_shape(nullptr, h)) return 0;
    if (workspace_bytes) *workspace_bytes = ws_layout(B, T, h, nullptr, nullptr);
    return record_layout(B, T, h, nullptr, nullptr);
}

extern "C" size_t xmh_umoed_keep_bytes(int64_t B, int T, const xmh_umoed_head* h) {
    if (head_shape(nullptr, B, T, h) || train_shape(nullptr, h)) return 0;
    return keep_layout(B, T, h).layer * (size_t)h->n_layers;
}

extern "C" int xmh_head_umoed_train_forward(const xmh_umoed_head* h, const float* tokens, const uint8_t* keep, float p, int64_t B, int T, float* embeds,
                                            float* code, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_head_umoed_train_forward");
    const char* who = "xmh_head_umoed_train_forward";
    if (int rc = check_train(who, h, tokens, keep, p, B, T, saved, saved_bytes, ws, ws_bytes)) return rc;
    if (!embeds || !code) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    Record r;
    record_layout(B, T, h, saved, &r);
    TrainWs w;
    ws_layout(B, T, h, ws, &w);
    return forward_chain(who, h, tokens, keep, p, B, T, r.x0,
                         [&](int l) {
                             LayerBufs v = record_layer(B, T, h, r, l);
                             v.lg = w.lg, v.tmp = w.tmp;
                             return v;
                         },
                         embeds, code, stream);
}

extern "C" int xmh_head_umoed_backward(const xmh_umoed_head* h, const float* tokens, const uint8_t* keep, float p, const float* d_embeds, int64_t B, int T,
                                       const void* saved, size_t saved_bytes, const xmh_umoed_head_grads* grads, int accumulate, void* ws, size_t ws_bytes,
                                       xmh_stream_t stream) {
    XMH_RANGE("xmh_head_umoed_backward");
    const char* who = "xmh_head_umoed_backward";
    if (int rc = check_train(who, h, tokens, keep, p, B, T, saved, saved_bytes, ws, ws_bytes)) return rc;
    if (!d_embeds || !grads) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    Record r;
    record_layout(B, T, h, const_cast<void*>(saved), &r);
    TrainWs w;
    ws_layout(B, T, h, ws, &w);
    hipStream_t st = xmh::as_stream(stream);
    const int M = h->M, d = h->d, F = h->F, H = h->heads, P = h->slots, N = h->n_experts, S = N * P, V = h->V, nl = h->n_layers;
    const int64_t BM = B * M, BT = B * T, BP = B * P, nd = BM * d;
    const float ks = keep ? 1.0f / (1.0f - p) : 1.0f;
    const KeepLayout kl = keep_layout(B, T, h);
    static const xmh_umoed_layer_grads none = {};
    // dY = du . keep / (1 - p) of a sublayer's output, or du itself without a mask
    auto through_dropout = [&](const float* du, const uint8_t* kp, float* out) -> const float* {
        if (!kp) return du;
        hipLaunchKernelGGL(k_umoed_keep_scale, dim3(blocks_for(nd)), dim3(kThreads), 0, st, du, kp, ks, nd, out);
        return out;
    };
    auto add = [&](float* a, const float* b, int64_t n) { hipLaunchKernelGGL(k_umoed_add, dim3(blocks_for(n)), dim3(kThreads), 0, st, a, b, n); };
    // du = LN'(dx) of the LayerNorm whose input was u
    auto norm_bwd = [&](const float* u, const float* gamma, float* dg, float* db) -> int {
        XMH_HIP(hipMemsetAsync(w.du, 0, (size_t)nd * sizeof(float), st));                  // k_ln_bwd_rows adds
        grad::ln_bwd(st, w.gs, u, w.dx, gamma, w.du, true, dg, db, BM, d, accumulate);
        return XMH_OK;
    };

    // the classifier
    const float* x_last = record_layer(B, T, h, r, nl - 1).xo;
    grad::weight_grads(st, w.gs, d_embeds, x_last, BM, V, d, grads->d_cls_w, grads->d_cls_b, accumulate);
    grad::launch_nn(st, d_embeds, h->cls_w, BM, V, d, w.dx, nullptr);

    bool tokens_written = false;
    for (int l = nl - 1; l >= 0; --l) {
        const xmh_umoed_layer& y = h->layers[l];
        const xmh_umoed_layer_grads& g = grads->layers ? grads->layers[l] : none;
        const LayerBufs v = record_layer(B, T, h, r, l);
        const float* x_in = l ? record_layer(B, T, h, r, l - 1).xo : r.x0;
        const uint8_t* kp = keep ? keep + (size_t)l * kl.layer : nullptr;

        // ---- the Soft-MoE sublayer ----
        XMH_TRY(norm_bwd(v.u3, y.ln3_g, g.ln3_g, g.ln3_b));
        const float* dY = through_dropout(w.du, kp ? kp + kl.at[5] : nullptr, w.t1);
        {
            BmmArgs a = bmm_args();                                                        // dCw[b] [M, S] = dY[b] Ys[b]^T
            a.A = dY, a.sai = d, a.sak = 1, a.sab = (int64_t)M * d;
            a.B = v.Ys, a.sbj = d, a.sbk = 1, a.sbb = (int64_t)S * d;
            a.I = M, a.J = S, a.Kd = d;
            a.C = w.dCw, a.sci = S, a.scb = (int64_t)M * S;
            launch_bmm<true, true>(st, a, B);
            a = bmm_args();                                                                // dYs[b] [S, d] = Cw[b]^T dY[b], written expert-major
            a.A = v.Cw, a.sai = 1, a.sak = S, a.sab = (int64_t)M * S;
            a.B = dY, a.sbj = 1, a.sbk = d, a.sbb = (int64_t)M * d;
            a.I = S, a.J = d, a.Kd = M;
            a.C = w.dYs, a.sci = d, a.scb = (int64_t)P * d, a.cdiv = P, a.sch = BP * d;
            launch_bmm<false, false>(st, a, B);
        }
        for (int n = 0; g.exp_w && n < N; ++n)                                             // an expert's rows (b, p) are one matrix [B P, .]
            grad::weight_grads(st, w.gs, v.Xs + (size_t)n * BP * F, w.dYs + (size_t)n * BP * d, BP, F, d, g.exp_w + (size_t)n * F * d, nullptr, accumulate);
        if (g.exp_b)
            hipLaunchKernelGGL(k_umoed_expert_bias, dim3((unsigned)((d + kCols - 1) / kCols), (unsigned)N), dim3(kThreads), 0, st, w.dYs, BP, d, g.exp_b,
                               accumulate);
        {
            BmmArgs a = bmm_args();                                                        // dXs [B, S, F]: rows (b, p) of expert n times W_n^T
            a.A = w.dYs, a.sai = d, a.sak = 1, a.sab = BP * d;
            a.B = y.exp_w, a.sbj = d, a.sbk = 1, a.sbb = (int64_t)F * d;
            a.I = (int)BP, a.J = F, a.Kd = d;
            a.C = w.dXs, a.sci = F, a.scb = (int64_t)P * F, a.cdiv = P, a.sch = (int64_t)S * F;
            launch_bmm<true, true>(st, a, N);
            a = bmm_args();                                                                // dD[b] [M, S] = h[b] dXs[b]^T
            a.A = v.h, a.sai = F, a.sak = 1, a.sab = (int64_t)M * F;
            a.B = w.dXs, a.sbj = F, a.sbk = 1, a.sbb = (int64_t)S * F;
            a.I = M, a.J = S, a.Kd = F;
            a.C = w.dD, a.sci = S, a.scb = (int64_t)M * S;
            launch_bmm<true, true>(st, a, B);
        }
        hipLaunchKernelGGL(k_umoed_route_bwd, dim3((unsigned)B), dim3(kThreads), 0, st, v.Dw, v.Cw, w.dD, w.dCw, M, S, w.dlg);
        {
            BmmArgs a = bmm_args();                                                        // dh[b] [M, F] = D[b] dXs[b] ...
            a.A = v.Dw, a.sai = S, a.sak = 1, a.sab = (int64_t)M * S;
            a.B = w.dXs, a.sbj = 1, a.sbk = F, a.sbb = (int64_t)S * F;
            a.I = M, a.J = F, a.Kd = S;
            a.C = w.dh, a.sci = F, a.scb = (int64_t)M * F;
            launch_bmm<true, false>(st, a, B);
            a = bmm_args();                                                                // ... + dlogits phi^T
            a.A = w.dlg, a.sai = S, a.sak = 1;
            a.B = y.phi, a.sbj = S, a.sbk = 1;
            a.I = (int)BM, a.J = F, a.Kd = S;
            a.C = w.dh, a.sci = F;
            a.res = w.dh;
            launch_bmm<true, true>(st, a, 1);
        }
        grad::weight_grads(st, w.gs, v.h, w.dlg, BM, F, S, g.phi, nullptr, accumulate);    // dphi [F, S] = h^T dlogits
        hipLaunchKernelGGL(k_umoed_relu_bwd, dim3(blocks_for(BM * F)), dim3(kThreads), 0, st, w.dh, v.h, ks, BM * F);
        grad::weight_grads(st, w.gs, w.dh, v.x2, BM, F, d, g.lin_w, g.lin_b, accumulate);
        grad::launch_nn(st, w.dh, y.lin_w, BM, F, d, w.dx, nullptr);
        add(w.dx, w.du, nd);                                                               // dx2

        // ---- the cross-attention sublayer ----
        XMH_TRY(norm_bwd(v.u2, y.ln2_g, g.ln2_g, g.ln2_b));
        const float* dO2 = through_dropout(w.du, kp ? kp + kl.at[3] : nullptr, w.t1);
        grad::weight_grads(st, w.gs, dO2, v.att2, BM, d, d, g.ca_out_w, g.ca_out_b, accumulate);
        grad::launch_nn(st, dO2, y.ca_out_w, BM, d, d, w.t2, nullptr);
        float* dq = w.dqkv;                                                                // [B M, d]: the packed buffer is free here
        attn_bwd(st, v.q, d, v.kv, 2 * d, d, w.t2, B, M, T, H, kp ? kp + kl.at[2] : nullptr, ks, w, dq, d, w.dkv, 2 * d, d);
        grad::weight_grads(st, w.gs, dq, v.x1, BM, d, d, g.ca_in_w, g.ca_in_b, accumulate);                               // rows 0 : d
        grad::weight_grads(st, w.gs, w.dkv, tokens, BT, 2 * d, d, g.ca_in_w ? g.ca_in_w + (size_t)d * d : nullptr,
                           g.ca_in_b ? g.ca_in_b + d : nullptr, accumulate);                                                // rows d : 3 d
        if (grads->d_tokens) {                                                             // the layers' shares added last layer first
            grad::launch_nn(st, w.dkv, y.ca_in_w + (size_t)d * d, BT, 2 * d, d, tokens_written ? w.dtok : grads->d_tokens, nullptr);
            if (tokens_written) add(grads->d_tokens, w.dtok, BT * d);
            tokens_written = true;
        }
        grad::launch_nn(st, dq, y.ca_in_w, BM, d, d, w.dx, nullptr);
        add(w.dx, w.du, nd);                                                               // dx1

        // ---- the self-attention sublayer ----
        XMH_TRY(norm_bwd(v.u1, y.ln1_g, g.ln1_g, g.ln1_b));
        const float* dO1 = through_dropout(w.du, kp ? kp + kl.at[1] : nullptr, w.t1);
        grad::weight_grads(st, w.gs, dO1, v.att1, BM, d, d, g.sa_out_w, g.sa_out_b, accumulate);
        grad::launch_nn(st, dO1, y.sa_out_w, BM, d, d, w.t2, nullptr);
        attn_bwd(st, v.qkv, 3 * d, v.qkv + d, 3 * d, d, w.t2, B, M, M, H, kp ? kp + kl.at[0] : nullptr, ks, w, w.dqkv, 3 * d, w.dqkv + d, 3 * d, d);
        grad::weight_grads(st, w.gs, w.dqkv, x_in, BM, 3 * d, d, g.sa_in_w, g.sa_in_b, accumulate);
        if (l == 0 && !grads->d_queries) break;                                            // nothing reads the first layer's input gradient
        grad::launch_nn(st, w.dqkv, y.sa_in_w, BM, 3 * d, d, w.dx, nullptr);
        add(w.dx, w.du, nd);                                                               // the layer's input gradient
    }
    if (grads->d_queries) {
        const int64_t per = (int64_t)M * d;
        hipLaunchKernelGGL(k_umoed_batch_sum, dim3(blocks_for(per)), dim3(kThreads), 0, st, w.dx, B, per, grads->d_queries, accumulate);
    }
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}
