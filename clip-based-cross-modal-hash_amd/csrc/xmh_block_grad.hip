// Backward of a stack of CLIP ResidualAttentionBlocks (models/CLIP/model.py:167-211) from the per-layer record that
// xmh_clip_blocks_forward_saved keeps.  Exact fp32 products throughout: a train step changes the weights every step, so
// the fp16 operand planes of the inference path would be re-made per step.
//
//   block, top down (dy = gradient of the block's output, [M, D], updated in place; M = B L, D = width):
//     c_proj   k_mfma_mm<TN> dW = dy^T fc_act, db = colsum dy          k_mfma_mm<NN> dfc_pre = (dy W) . QuickGELU'(fc_pre)   (epilogue)
//     c_fc     k_mfma_mm<TN> dW = dfc_pre^T ln2, db                    k_mfma_mm<NN> dln2 = dfc_pre W
//     ln_2     k_ln_bwd_rows dy += LN'(dln2; x_mid)  (= dx_mid)        k_ln_bwd_cols + k_ln_cols_reduce  dgamma, dbeta
//     out_proj k_mfma_mm<TN> dW = dy^T attn, db                        k_mfma_mm<NN> dattn = dy W
//     attn     k_attn_bwd   dqkv from the saved qkv (S and P recomputed per query tile)
//     in_proj  k_mfma_mm<TN> dW = dqkv^T ln1, db                       k_mfma_mm<NN> dln1 = dqkv W
//     ln_1     k_ln_bwd_rows dy += LN'(dln1; x_in)   (= dx)            k_ln_bwd_cols + k_ln_cols_reduce
//   A TN product whose 64 x 64 tiles would not fill the chip splits its reduction (the tokens) over blockIdx.z; the partials go to
//   the workspace and k_reduce_parts adds them in index order.
//
// One product kernel, C[i][j] = sum_k A(i, k) B(j, k) over strided views (as k_mm of xmh_head_grad.hip), on v_mfma_f32_32x32x2_f32:
// an exact fmaf chain per 32 consecutive k, the 32-blocks added in index order.  Every reduction here runs in one fixed order (no
// float atomics), so two calls on equal inputs agree to the bit; no host synchronisation, no allocation.
// The product, bias and LayerNorm kernels and their launch helpers are in xmh_grad_kernels.hip (xmh_tower_grad.hip and xmh_mith_grad.hip use them).
#include "xmh_clip_record.h"
#include "xmh_grad_kernels.h"

namespace {

using namespace xmh::grad;

// Attention backward of one (batch, head) per block.  K and V of the head stay in LDS (rows padded to 65 floats, key rows up to
// LP = 4 NJ zero-filled); the queries go by in tiles of 32 rows: S = (q / sqrt(dh)) K^T + mask and P = softmax(S) are recomputed as
// the forward computes them, dP = dO V^T, dS = P (dP - rowsum(dP P)), dQ = dS K / sqrt(dh) goes straight out, and dV += P^T dO,
// dK += dS^T (q / sqrt(dh)) accumulate in registers -- thread (c, jg) owns column c of key rows jg, jg + 4, ... -- over the tiles in
// index order: no atomics, one fixed order.  A whole-head-resident plan (Q, K, V, dO and a 128 x 128 P) would need 192 KB of LDS.
constexpr int kDh = 64, kTq = 32, kKp = kDh + 1;

template <int NJ>
__global__ __launch_bounds__(kThreads) void k_attn_bwd(const float* __restrict__ qkv, const float* __restrict__ dO, float* __restrict__ dqkv,
                                                       int L, int H, int causal, const uint8_t* __restrict__ kpm) {
    constexpr int LP = 4 * NJ, PP = LP + 1, NS = NJ / 2;
    extern __shared__ __attribute__((aligned(16))) float sm_attn[];
    float* sK = sm_attn;                         // [LP][kKp]
    float* sV = sK + LP * kKp;                   // [LP][kKp]
    float* sQ = sV + LP * kKp;                   // [kTq][kKp], scaled
    float* sG = sQ + kTq * kKp;                  // [kTq][kKp], dO
    float* sP = sG + kTq * kKp;                  // [kTq][PP]
    float* sS = sP + kTq * PP;                   // [kTq][PP], dS
    const int tid = threadIdx.x;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int D = H * kDh;
    const float scale = rsqrtf((float)kDh);
    const float* base = qkv + (int64_t)b * L * 3 * D + h * kDh;
    const float* gbase = dO + (int64_t)b * L * D + h * kDh;
    float* obase = dqkv + (int64_t)b * L * 3 * D + h * kDh;
    for (int e = tid; e < LP * (kDh / 4); e += kThreads) {
        const int j = e / (kDh / 4), c = (e % (kDh / 4)) * 4;
        float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
        if (j < L) {
            kv = *reinterpret_cast<const float4*>(base + (int64_t)j * 3 * D + D + c);
            vv = *reinterpret_cast<const float4*>(base + (int64_t)j * 3 * D + 2 * D + c);
        }
        float* pk = sK + j * kKp + c;
        float* pv = sV + j * kKp + c;
        pk[0] = kv.x; pk[1] = kv.y; pk[2] = kv.z; pk[3] = kv.w;
        pv[0] = vv.x; pv[1] = vv.y; pv[2] = vv.z; pv[3] = vv.w;
    }
    float accK[NJ], accV[NJ];
#pragma unroll
    for (int t = 0; t < NJ; ++t) accK[t] = accV[t] = 0.0f;
    const int r = tid >> 3, sub = tid & 7;       // score phase and dQ: query row of the tile, 8 threads per row
    const int oc = tid & 63, jg = tid >> 6;      // dK / dV phase
    for (int i0 = 0; i0 < L; i0 += kTq) {
        __syncthreads();                         // the previous tile's reads are done (first pass: K and V are in place)
        for (int e = tid; e < kTq * (kDh / 4); e += kThreads) {
            const int rr = e / (kDh / 4), c = (e % (kDh / 4)) * 4;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f), gg = q;
            if (i0 + rr < L) {
                q = *reinterpret_cast<const float4*>(base + (int64_t)(i0 + rr) * 3 * D + c);
                gg = *reinterpret_cast<const float4*>(gbase + (int64_t)(i0 + rr) * D + c);
            }
            float* pq = sQ + rr * kKp + c;
            float* pg = sG + rr * kKp + c;
            pq[0] = q.x * scale; pq[1] = q.y * scale; pq[2] = q.z * scale; pq[3] = q.w * scale;      // PyTorch scales q before QK^T
            pg[0] = gg.x; pg[1] = gg.y; pg[2] = gg.z; pg[3] = gg.w;
        }
        __syncthreads();
        const int i = i0 + r;
        float s[NS], dp[NS];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const int j = sub + 8 * t;
            float a0 = 0.0f, a1 = 0.0f;
            const float* q = sQ + r * kKp;
            const float* gq = sG + r * kKp;
            const float* kj = sK + j * kKp;
            const float* vj = sV + j * kKp;
#pragma unroll 8
            for (int c = 0; c < kDh; ++c) {
                a0 = fmaf(q[c], kj[c], a0);
                a1 = fmaf(gq[c], vj[c], a1);
            }
            const bool dead = j >= L || (causal && j > i) || (kpm && kpm[(int64_t)b * L + j]);
            s[t] = dead ? -INFINITY : a0;
            dp[t] = a1;
            mx = fmaxf(mx, s[t]);
        }
#pragma unroll
        for (int off = 4; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        float sum = 0.0f;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            s[t] = expf(s[t] - mx);
            sum += s[t];
        }
#pragma unroll
        for (int off = 4; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        const float inv = i < L ? 1.0f / sum : 0.0f;         // rows past L contribute nothing to dK / dV
        float dot = 0.0f;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            s[t] *= inv;
            dot = fmaf(s[t], dp[t], dot);
        }
#pragma unroll
        for (int off = 4; off > 0; off >>= 1) dot += __shfl_xor(dot, off);
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const int j = sub + 8 * t;
            sP[r * PP + j] = s[t];
            sS[r * PP + j] = s[t] * (dp[t] - dot);
        }
        __syncthreads();
        {                                        // dQ[i][c] = scale sum_j dS[i][j] K[j][c], c = sub + 8 u
            float dq[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) dq[u] = 0.0f;
            for (int j = 0; j < L; ++j) {
                const float ds = sS[r * PP + j];
                const float* kj = sK + j * kKp + sub;
#pragma unroll
                for (int u = 0; u < 8; ++u) dq[u] = fmaf(ds, kj[8 * u], dq[u]);
            }
            if (i < L) {
#pragma unroll
                for (int u = 0; u < 8; ++u) obase[(int64_t)i * 3 * D + sub + 8 * u] = dq[u] * scale;
            }
        }
        for (int ii = 0; ii < kTq; ++ii) {       // rows past L hold P = dS = 0
            const float go = sG[ii * kKp + oc], q = sQ[ii * kKp + oc];
            const float* pr = sP + ii * PP + jg;
            const float* sr = sS + ii * PP + jg;
#pragma unroll
            for (int t = 0; t < NJ; ++t) {
                accV[t] = fmaf(pr[4 * t], go, accV[t]);
                accK[t] = fmaf(sr[4 * t], q, accK[t]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NJ; ++t) {
        const int j = jg + 4 * t;
        if (j < L) {
            obase[(int64_t)j * 3 * D + D + oc] = accK[t];
            obase[(int64_t)j * 3 * D + 2 * D + oc] = accV[t];
        }
    }
}

template <int NJ>
int launch_attn_bwd(hipStream_t st, const float* qkv, const float* dO, float* dqkv, int64_t B, int L, int H, int causal, const uint8_t* kpm) {
    constexpr int LP = 4 * NJ;
    const size_t lds = ((size_t)2 * LP * kKp + (size_t)2 * kTq * kKp + (size_t)2 * kTq * (LP + 1)) * sizeof(float);
    auto kern = k_attn_bwd<NJ>;
    if (lds > 64 * 1024) XMH_TRY(xmh::raise_dynamic_lds(reinterpret_cast<const void*>(kern), lds, "xmh_clip_blocks_backward"));
    hipLaunchKernelGGL(kern, dim3((unsigned)(B * H)), dim3(kThreads), lds, st, qkv, dO, dqkv, L, H, causal, kpm);
    return XMH_OK;
}

int attn_bwd(hipStream_t st, const float* qkv, const float* dO, float* dqkv, int64_t B, int L, int H, int causal, const uint8_t* kpm) {
    if (L <= 32) return launch_attn_bwd<8>(st, qkv, dO, dqkv, B, L, H, causal, kpm);
    if (L <= 64) return launch_attn_bwd<16>(st, qkv, dO, dqkv, B, L, H, causal, kpm);
    return launch_attn_bwd<32>(st, qkv, dO, dqkv, B, L, H, causal, kpm);
}

struct Work : GradScratch {
    float* t1;        // [M, D]   dln2, dattn, dln1
    float* t4;        // [M, 4D]  dfc_pre; dqkv [M, 3D] once dfc_pre is dead
};

size_t work_layout(int64_t M, int D, void* base, Work* w) {
    xmh::Arena ar(base);
    Work v;
    v.t1 = ar.take<float>((size_t)M * D);
    v.t4 = ar.take<float>((size_t)M * D * 4);
    const TnShape tn[] = {{M, D, 4 * D}, {M, 4 * D, D}, {M, D, D}, {M, 3 * D, D}};
    take_scratch(ar, M, D, 4 * D, tn, &v);
    if (w) *w = v;
    return ar.used;
}

}  // namespace

extern "C" size_t xmh_clip_blocks_backward_ws_bytes(int64_t B, int L, int width) {
    if (!stack_limits_ok(B, L, width)) return 0;
    return work_layout(B * L, width, nullptr, nullptr);
}

extern "C" int xmh_clip_blocks_backward(const xmh_clip_block* blocks, int layers, int width, int heads, int64_t B, int L, int causal,
                                        const uint8_t* key_padding_mask, const float* saved, size_t saved_bytes, float* dy, int need_dx,
                                        const xmh_clip_block_grads* grads, int accumulate, void* workspace, size_t workspace_bytes,
                                        xmh_stream_t stream) {
    XMH_RANGE("xmh_clip_blocks_backward");
    const char* who = "xmh_clip_blocks_backward";
    if (B == 0 || layers == 0) return XMH_OK;
    if (B < 0 || L <= 0 || layers < 0 || width <= 0 || heads <= 0 || width % heads) return xmh::fail(XMH_EINVAL, "%s: bad arguments", who);
    if (!blocks || !grads) return xmh::fail(XMH_EINVAL, "%s: null blocks / grads", who);
    if (!dy) return xmh::fail(XMH_EINVAL, "%s: null dy", who);
    if (!saved) return xmh::fail(XMH_EINVAL, "%s: null saved buffer", who);
    if (!workspace) return xmh::fail(XMH_EINVAL, "%s: null workspace", who);
    if (width % 4) return xmh::fail(XMH_ENOTSUP, "%s: width %d is not a multiple of 4", who, width);
    XMH_TRY(check_stack_limits(who, B, L, width, heads));
    const int64_t M = B * L;
    const int D = width;
    const size_t need = xmh::saved_record_bytes(layers, M, D);
    if (saved_bytes < need) return xmh::fail(XMH_ENOMEM, "%s: saved buffer of %zu bytes, %zu needed", who, saved_bytes, need);
    Work wk;
    const size_t ws_need = work_layout(M, D, workspace, &wk);
    if (workspace_bytes < ws_need) return xmh::fail(XMH_ENOMEM, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, ws_need);

    // the walk stops at the lowest layer anything is asked of: below it nothing is read, neither its record nor its weights
    int lowest = 0;
    if (!need_dx) {
        while (lowest < layers && !block_asked(grads[lowest])) ++lowest;
        if (lowest == layers) return XMH_OK;
    }
    for (int i = lowest; i < layers; ++i) {
        const xmh_clip_block& b = blocks[i];
        if (!xmh::block_fits(b, D)) return xmh::fail(XMH_EINVAL, "%s: block %d has layer shapes that do not fit width %d", who, i, D);
        if (!b.qkv.w_f32 || !b.out.w_f32 || !b.fc.w_f32 || !b.proj.w_f32 || !b.ln1_w || !b.ln2_w)
            return xmh::fail(XMH_EINVAL, "%s: block %d lacks fp32 weights", who, i);
    }
    hipStream_t st = xmh::as_stream(stream);
    for (int i = layers - 1; i >= lowest; --i) {
        const xmh_clip_block& b = blocks[i];
        const xmh_clip_block_grads& g = grads[i];
        const xmh::SavedRecord<const float> r = xmh::saved_record(saved, i, M, D);
        // what has to exist for what is asked for: each stage is needed by everything upstream of it
        const bool need_in = i > lowest || need_dx;
        const bool need_dln1 = g.ln1_w || g.ln1_b || need_in;
        const bool need_dqkv = g.qkv_w || g.qkv_b || need_dln1;
        const bool need_dxmid = g.out_w || g.out_b || need_dqkv;
        const bool need_dln2 = g.ln2_w || g.ln2_b || need_dxmid;
        const bool need_dfc = g.fc_w || g.fc_b || need_dln2;
        weight_grads(st, wk, dy, r.fc_act, M, D, 4 * D, g.proj_w, g.proj_b, accumulate);
        if (!need_dfc) continue;
        launch_nn(st, dy, b.proj.w_f32, M, D, 4 * D, wk.t4, r.fc_pre);                         // dfc_pre
        weight_grads(st, wk, wk.t4, r.ln2, M, 4 * D, D, g.fc_w, g.fc_b, accumulate);
        if (!need_dln2) continue;
        launch_nn(st, wk.t4, b.fc.w_f32, M, 4 * D, D, wk.t1, nullptr);                         // dln2
        ln_bwd(st, wk, r.x_mid, wk.t1, b.ln2_w, dy, need_dxmid, g.ln2_w, g.ln2_b, M, D, accumulate);    // dy = dx_mid
        if (!need_dxmid) continue;
        weight_grads(st, wk, dy, r.attn, M, D, D, g.out_w, g.out_b, accumulate);
        if (!need_dqkv) continue;
        launch_nn(st, dy, b.out.w_f32, M, D, D, wk.t1, nullptr);                               // dattn
        XMH_TRY(attn_bwd(st, r.qkv, wk.t1, wk.t4, B, L, heads, causal, key_padding_mask));                     // dqkv [M, 3D]
        weight_grads(st, wk, wk.t4, r.ln1, M, 3 * D, D, g.qkv_w, g.qkv_b, accumulate);
        if (!need_dln1) continue;
        launch_nn(st, wk.t4, b.qkv.w_f32, M, 3 * D, D, wk.t1, nullptr);                        // dln1
        ln_bwd(st, wk, r.x_in, wk.t1, b.ln1_w, dy, need_in, g.ln1_w, g.ln1_b, M, D, accumulate);  // dy = dx
    }
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}
