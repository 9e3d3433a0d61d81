// Training forward and backward of the two CLIP towers (models/CLIP/model.py:232-268, :373-396): the thin layers around the block
// stack.  Exact fp32 throughout, for the reason xmh_block_grad.hip gives; the blocks themselves run through
// xmh_clip_blocks_forward_saved / xmh_clip_blocks_backward, and the products, bias sums and LayerNorm backward are the kernels of
// xmh_grad_kernels.hip.
//
//   image forward   im2col -> conv1 (fp32 MFMA) -> cls / pos / ln_pre (the rows in front of ln_pre are kept) -> blocks, saved ->
//                   cls rows (kept) -> ln_post -> proj          the very calls of xmh_vit_b32_forward in exact mode: same bits
//   text forward    token + positional embedding, EOS = argmax -> blocks (causal), saved -> EOS rows (kept) -> ln_final -> text_projection
//   back end        ln_out = LN(rows) again; dproj = ln_out^T g (TN); dln_out = g proj^T (NN); LayerNorm backward on the B rows;
//                   the B row gradients are scattered into a zeroed dy [B, L, D] at row 0 / row eos[b]
//   image front     LayerNorm backward of ln_pre into a zeroed buffer (k_ln_bwd_rows adds; ln_pre has no residual);
//                   dpos [L, D] and dcls [D] = sums over the batch (k_batch_sum: double, items in index order, chunks added in order);
//                   dconv1 = dpatches^T cols (TN, K = 3 p p) with cols made again from the image and the patch rows gathered dense
//   text front      dpos likewise (rows at or beyond L zero); dtok [vocab, D] dense by k_tok_grad: one block per token row, the block
//                   of the FIRST row that holds an id owns it and adds the rows of every later occurrence in index order
//   token outputs   (MITH reads every projected row) the stack runs in the kept buffer, so all M = B L rows in front of the
//                   last LayerNorm are kept; LayerNorm and projection on the M rows as xmh_vit_b32_forward / xmh_text_forward run them
//                   for out_tokens.  Back end: dOut [B, L, out_dim] built in one pass from g_cls / g_eos and g_tokens
//                   (k_token_grads), then the same three products over M rows, the LayerNorm backward straight into a zeroed dy
// No host synchronisation, no allocation, no float atomics; every sum has one fixed order.
#include "xmh_clip_record.h"
#include "xmh_grad_kernels.h"
#include "xmh_planes.h"

namespace {

using namespace xmh::grad;

constexpr int kBatchChunk = 16;                  // items per partial of a sum over the batch
constexpr int kMaxWidth = 1024;                  // the forward's LayerNorm kernels hold a row in 16 registers per lane
constexpr int kTokCols = kMaxWidth / kThreads;

// dy[b][idx ? idx[b] : 0][:] = rows[b][:]   (dy zeroed before; an index outside [0, L) is clamped, as nothing upstream can check it)
__global__ __launch_bounds__(kThreads) void k_scatter_rows(const float* __restrict__ rows, const int32_t* __restrict__ idx, int64_t B, int L, int D,
                                                           float* __restrict__ dy) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= B * D) return;
    const int64_t b = e / D;
    const int c = (int)(e % D);
    int l = idx ? idx[b] : 0;
    l = l < 0 ? 0 : l >= L ? L - 1 : l;
    dy[(b * L + l) * D + c] = rows[e];
}

// The gradient of every projected row, dout [B, L, E], in one pass; a NULL input counts as zeros.
//   image (idx == NULL)   row 0 of item b = g_row[b], row 1 + p = g_tok[b][p]                  (g_tok [B, L - 1, E])
//   text                  row l = g_tok[b][l], plus g_row[b] at l == idx[b], clamped as k_scatter_rows clamps it   (g_tok [B, L, E])
__global__ __launch_bounds__(kThreads) void k_token_grads(const float* __restrict__ g_row, const float* __restrict__ g_tok,
                                                          const int32_t* __restrict__ idx, int64_t B, int L, int E, float* __restrict__ dout) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= B * L * E) return;
    const int64_t row = e / E;
    const int c = (int)(e % E);
    const int64_t b = row / L;
    const int l = (int)(row % L);
    float v;
    if (!idx) {
        v = l == 0 ? (g_row ? g_row[b * E + c] : 0.0f) : (g_tok ? g_tok[(b * (L - 1) + l - 1) * E + c] : 0.0f);
    } else {
        v = g_tok ? g_tok[e] : 0.0f;
        if (g_row) {
            int q = idx[b];
            q = q < 0 ? 0 : q >= L ? L - 1 : q;
            if (l == q) v += g_row[b * E + c];
        }
    }
    dout[e] = v;
}

// out[b P + p][:] = x[b][1 + p][:]: the patch rows of every item, dense
__global__ __launch_bounds__(kThreads) void k_gather_patch_rows(const float* __restrict__ x, int64_t B, int L, int D, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int P = L - 1;
    if (e >= B * P * D) return;
    const int64_t row = e / D;
    const int c = (int)(e % D);
    const int64_t b = row / P;
    const int p = (int)(row % P);
    out[e] = x[(b * L + 1 + p) * D + c];
}

// out[e] (+)= sum_b src[b * stride + e], e < n: the items of chunk blockIdx.y in index order, in double; several chunks leave their
// partials in part [chunks][n] for k_batch_reduce
__global__ __launch_bounds__(kThreads) void k_batch_sum(const float* __restrict__ src, int64_t B, int64_t n, int64_t stride, float* out, double* part,
                                                        int accumulate) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const int64_t b0 = (int64_t)blockIdx.y * kBatchChunk, b1 = b0 + kBatchChunk < B ? b0 + kBatchChunk : B;
    double a = 0.0;
    for (int64_t b = b0; b < b1; ++b) a += (double)src[b * stride + e];
    if (gridDim.y > 1) part[(int64_t)blockIdx.y * n + e] = a;
    else out[e] = accumulate ? out[e] + (float)a : (float)a;
}

__global__ __launch_bounds__(kThreads) void k_batch_reduce(const double* __restrict__ part, int chunks, int64_t n, float* out, int accumulate) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    double a = part[e];
    for (int c = 1; c < chunks; ++c) a += part[(int64_t)c * n + e];
    out[e] = accumulate ? out[e] + (float)a : (float)a;
}

// Gradient of the token embedding, dense and without atomics.  Block r looks at token row r = (b, l): if an earlier row holds the same
// id, that row's block owns it and this one leaves.  The owner walks the rows from r on in index order and adds, in double, dx of
// every row with its id; one write per element.  Ids outside the table are clamped as k_text_embed clamps them.  Rows of dtok whose
// id never occurs are not touched (the caller zeroes the table unless it accumulates).  D <= kMaxWidth.
__global__ __launch_bounds__(kThreads) void k_tok_grad(const int64_t* __restrict__ ids, const float* __restrict__ dx, int64_t M, int D, int vocab,
                                                       float* dtok, int accumulate) {
    const int64_t r = blockIdx.x;
    auto id_of = [&](int64_t q) {
        const int64_t v = ids[q];
        return v < 0 ? (int64_t)0 : v >= vocab ? (int64_t)vocab - 1 : v;
    };
    const int64_t id = id_of(r);
    int seen = 0;
    for (int64_t q = threadIdx.x; q < r; q += kThreads) seen |= id_of(q) == id;
    if (__syncthreads_or(seen)) return;
    double a[kTokCols];
#pragma unroll
    for (int u = 0; u < kTokCols; ++u) a[u] = 0.0;
    for (int64_t q = r; q < M; ++q) {
        if (id_of(q) != id) continue;                // uniform over the block
        const float* row = dx + q * D;
#pragma unroll
        for (int u = 0; u < kTokCols; ++u) {
            const int c = u * kThreads + threadIdx.x;
            if (c < D) a[u] += (double)row[c];
        }
    }
    float* out = dtok + id * D;
#pragma unroll
    for (int u = 0; u < kTokCols; ++u) {
        const int c = u * kThreads + threadIdx.x;
        if (c < D) out[c] = accumulate ? out[c] + (float)a[u] : (float)a[u];
    }
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// sum over the batch of src [B][stride] (first n of every item) -> out [n]
void batch_sum(hipStream_t st, const float* src, int64_t B, int64_t n, int64_t stride, float* out, double* part, int accumulate) {
    const int chunks = (int)xmh::ceil_div(B, kBatchChunk);
    hipLaunchKernelGGL(k_batch_sum, dim3(blocks_for(n), chunks), dim3(kThreads), 0, st, src, B, n, stride, out, part, accumulate);
    if (chunks > 1) hipLaunchKernelGGL(k_batch_reduce, dim3(blocks_for(n)), dim3(kThreads), 0, st, part, chunks, n, out, accumulate);
}

// what a call keeps for its backward, behind the block record: the rows in front of ln_pre (image) and the rows in front of the
// last LayerNorm -- the B cls / EOS rows, or with `tokens` all M of them, the stack's whole output
struct Kept {
    float* record;
    size_t record_bytes;
    float* pre;       // [M, D], image only
    float* rows;      // [B, D] or [M, D]
};

size_t kept_layout(int64_t B, int L, int D, int layers, bool image, bool tokens, void* base, Kept* k) {
    xmh::Arena ar(base);
    Kept v;
    v.record_bytes = xmh::saved_record_bytes(layers, B * L, D);
    v.record = ar.take<float>(v.record_bytes / sizeof(float));
    v.pre = image ? ar.take<float>((size_t)B * L * D) : nullptr;
    v.rows = ar.take<float>((size_t)(tokens ? B * L : B) * D);
    if (k) *k = v;
    return ar.used;
}

// one workspace for the forward and the backward of a tower (conv_k == 0: text)
struct TowerWork {
    GradScratch gs;
    float* x;          // [M, D]   the stream (forward), dy (backward)
    float* t;          // [M, D]   image: gradient of the rows in front of ln_pre
    float* cols;       // [B P, conv_k]
    float* patches;    // [B P, D] conv1's output (forward), its gradient (backward)
    float *ln_out, *dln;             // [R, D], R = B rows of the back end, or M with the token outputs
    float* drow;                     // [B, D], the B-row back end only
    float* y;          // [M, out_dim], token outputs only: the projected rows (image forward), their gradient (backward)
    double* bsum;      // [chunks][L D]
    char* blocks;      // scratch of the block stack's forward / workspace of its backward
    size_t blocks_bytes;
};

size_t work_layout(int64_t B, int L, int D, int conv_k, int out_dim, bool tokens, void* base, TowerWork* w) {
    xmh::Arena ar(base);
    TowerWork v;
    const int64_t M = B * L, BP = B * (L - 1), R = tokens ? M : B;
    v.x = ar.take<float>((size_t)M * D);
    v.t = conv_k ? ar.take<float>((size_t)M * D) : nullptr;
    v.cols = conv_k ? ar.take<float>((size_t)BP * conv_k) : nullptr;
    v.patches = conv_k ? ar.take<float>((size_t)BP * D) : nullptr;
    v.ln_out = ar.take<float>((size_t)R * D);
    v.dln = ar.take<float>((size_t)R * D);
    v.drow = tokens ? nullptr : ar.take<float>((size_t)B * D);
    v.y = tokens ? ar.take<float>((size_t)M * out_dim) : nullptr;
    v.bsum = ar.take<double>((size_t)xmh::ceil_div(B, kBatchChunk) * L * D);
    const TnShape tn[] = {{R, D, out_dim}, {BP, D, conv_k}};
    take_scratch(ar, M, D, D, tn, &v.gs);
    const size_t fwd = xmh_clip_workspace_bytes(B, L, D, 0, 0, 2), bwd = xmh_clip_blocks_backward_ws_bytes(B, L, D);
    v.blocks_bytes = fwd > bwd ? fwd : bwd;
    v.blocks = ar.take<char>(v.blocks_bytes);
    if (w) *w = v;
    return ar.used;
}

// the two buffers of a call, laid out and measured against what the caller handed in
int lay_out(const char* who, int64_t B, int L, int D, int layers, int conv_k, int out_dim, bool tokens, const void* saved, size_t saved_bytes,
            void* workspace, size_t workspace_bytes, Kept* kp, TowerWork* wk) {
    const size_t kneed = kept_layout(B, L, D, layers, conv_k > 0, tokens, const_cast<void*>(saved), kp);
    if (saved_bytes < kneed) return xmh::fail(XMH_ENOMEM, "%s: saved buffer of %zu bytes, %zu needed", who, saved_bytes, kneed);
    const size_t wneed = work_layout(B, L, D, conv_k, out_dim, tokens, workspace, wk);
    if (workspace_bytes < wneed) return xmh::fail(XMH_ENOMEM, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, wneed);
    return XMH_OK;
}

bool limits_ok(int64_t B, int L, int D) { return stack_limits_ok(B, L, D) && D <= kMaxWidth; }

int check_limits(const char* who, int64_t B, int L, int D, int heads) {
    if (D % 4 || D > kMaxWidth) return xmh::fail(XMH_ENOTSUP, "%s: width %d (a multiple of 4, at most %d)", who, D, kMaxWidth);
    return check_stack_limits(who, B, L, D, heads);
}

bool any_block_asked(const xmh_clip_block_grads* g, int layers) {
    for (int i = 0; g && i < layers; ++i)
        if (block_asked(g[i])) return true;
    return false;
}

// geometry of the image tower, checked once for the forward and the backward
struct VitShape {
    int P, L, D, conv_k;
};

int vit_shape(const char* who, const xmh_vit_weights* w, int64_t B, VitShape* s) {
    if (w->patch <= 0 || w->resolution <= 0 || w->resolution % w->patch || w->heads <= 0 || w->width <= 0 || w->width % w->heads || w->layers < 0 ||
        w->out_dim <= 0)
        return xmh::fail(XMH_EINVAL, "%s: resolution %d / patch %d / width %d / heads %d do not fit", who, w->resolution, w->patch, w->width, w->heads);
    const int G = w->resolution / w->patch;
    s->P = G * G;
    s->L = s->P + 1;
    s->D = w->width;
    s->conv_k = 3 * w->patch * w->patch;
    if (w->conv1.n != s->D || w->conv1.k != s->conv_k || w->proj.n != w->out_dim || w->proj.k != s->D)
        return xmh::fail(XMH_EINVAL, "%s: conv1 / proj shapes do not fit the tower", who);
    if (!w->conv1.w_f32 || !w->proj.w_f32 || !w->cls || !w->pos || !w->ln_pre_w || !w->ln_pre_b || !w->ln_post_w || !w->ln_post_b ||
        (w->layers > 0 && !w->blocks))
        return xmh::fail(XMH_EINVAL, "%s: the tower lacks fp32 weights", who);
    if (w->patch % 4) return xmh::fail(XMH_ENOTSUP, "%s: patch %d is not a multiple of 4", who, w->patch);
    return check_limits(who, B, s->L, s->D, w->heads);
}

int text_shape(const char* who, const xmh_text_weights* w, int64_t B, int L) {
    if (w->heads <= 0 || w->width <= 0 || w->width % w->heads || w->layers < 0 || w->out_dim <= 0 || w->vocab <= 0 || w->proj.n != w->out_dim ||
        w->proj.k != w->width)
        return xmh::fail(XMH_EINVAL, "%s: shapes do not fit the tower", who);
    if (L <= 0 || L > w->context) return xmh::fail(XMH_EINVAL, "%s: %d tokens, the positional embedding holds %d", who, L, w->context);
    if (!w->proj.w_f32 || !w->tok_emb || !w->pos || !w->ln_final_w || !w->ln_final_b || (w->layers > 0 && !w->blocks))
        return xmh::fail(XMH_EINVAL, "%s: the tower lacks fp32 weights", who);
    return check_limits(who, B, L, w->width, w->heads);
}

// rows [B, D] -> LayerNorm -> projection: the tail of both forwards, as ln_linear of xmh_forward.hip runs it in exact mode
int forward_tail(const float* rows, int64_t B, int D, const float* gamma, const float* beta, const xmh_linear& proj, float* ln_out, float* out,
                 xmh_stream_t stream) {
    XMH_TRY(xmh_layernorm_f32(rows, D, gamma, beta, kLnEps, ln_out, D, B, D, stream));
    return xmh_gemm_nt_f32(ln_out, D, proj.w_f32, proj.k, proj.bias, nullptr, 0, out, proj.n, B, proj.n, proj.k, 0, 0, stream);
}

// The back end of both towers: g [R, out_dim] -> dproj [D, out_dim], dgamma / dbeta of the last LayerNorm and, when need_dy, the
// gradient of the stack's output dy [B, L, D].  R = B: g belongs to row 0 / row idx[b] of every item, the other rows of dy are zero.
// every_row: R = B L, `rows` is the stack's whole output and dy is the LayerNorm backward of every row.
int back_end(const TowerWork& wk, const float* rows, const float* gamma, const float* beta, const xmh_linear& proj, const float* g, int64_t B,
             int L, int D, const int32_t* idx, bool every_row, float* dproj, float* dgamma, float* dbeta, bool need_dy, int accumulate,
             xmh_stream_t stream) {
    hipStream_t st = xmh::as_stream(stream);
    const int out_dim = (int)proj.n;
    const int64_t R = every_row ? B * L : B;
    if (dproj) {
        XMH_TRY(xmh_layernorm_f32(rows, D, gamma, beta, kLnEps, wk.ln_out, D, R, D, stream));
        weight_grads(st, wk.gs, wk.ln_out, g, R, D, out_dim, dproj, nullptr, accumulate);
    }
    if (!need_dy && !dgamma && !dbeta) return XMH_OK;
    launch_nn(st, g, proj.w_f32, R, out_dim, D, wk.dln, nullptr);                              // dln_out = g proj^T
    if (every_row) {
        if (need_dy) XMH_HIP(hipMemsetAsync(wk.x, 0, (size_t)R * D * sizeof(float), st));      // k_ln_bwd_rows adds
        ln_bwd(st, wk.gs, rows, wk.dln, gamma, wk.x, need_dy, dgamma, dbeta, R, D, accumulate);
        return XMH_OK;
    }
    if (need_dy) XMH_HIP(hipMemsetAsync(wk.drow, 0, (size_t)B * D * sizeof(float), st));      // k_ln_bwd_rows adds
    ln_bwd(st, wk.gs, rows, wk.dln, gamma, wk.drow, need_dy, dgamma, dbeta, B, D, accumulate);
    if (need_dy) {
        XMH_HIP(hipMemsetAsync(wk.x, 0, (size_t)B * L * D * sizeof(float), st));
        hipLaunchKernelGGL(k_scatter_rows, dim3(blocks_for(B * D)), dim3(kThreads), 0, st, wk.drow, idx, B, L, D, wk.x);
    }
    return XMH_OK;
}

// ---- the four calls, each in two forms: the B cls / EOS rows (tokens == false) or every projected row ---------------

size_t vit_saved_bytes(int64_t B, int L, int width, int layers, bool tokens) {
    if (!limits_ok(B, L, width) || layers < 0) return 0;
    return kept_layout(B, L, width, layers, true, tokens, nullptr, nullptr);
}

size_t text_saved_bytes(int64_t B, int L, int width, int layers, bool tokens) {
    if (!limits_ok(B, L, width) || layers < 0) return 0;
    return kept_layout(B, L, width, layers, false, tokens, nullptr, nullptr);
}

size_t vit_ws_bytes(int64_t B, int L, int width, int conv_k, int out_dim, bool tokens) {
    if (!limits_ok(B, L, width) || conv_k <= 0 || out_dim <= 0 || L < 2) return 0;
    return work_layout(B, L, width, conv_k, out_dim, tokens, nullptr, nullptr);
}

size_t text_ws_bytes(int64_t B, int L, int width, int out_dim, bool tokens) {
    if (!limits_ok(B, L, width) || out_dim <= 0) return 0;
    return work_layout(B, L, width, 0, out_dim, tokens, nullptr, nullptr);
}

// out_tokens == NULL: the cls rows alone are kept and projected
int vit_forward(const char* who, const xmh_vit_weights* w, const float* image, int64_t B, float* out_cls, float* out_tokens, bool tokens, void* saved,
                size_t saved_bytes, void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    if (B == 0) return XMH_OK;
    if (B < 0 || !w || !image || !out_cls || (tokens && !out_tokens) || !saved || !workspace) return xmh::fail(XMH_EINVAL, "%s: bad arguments", who);
    VitShape s;
    XMH_TRY(vit_shape(who, w, B, &s));
    Kept kp;
    TowerWork wk;
    XMH_TRY(lay_out(who, B, s.L, s.D, w->layers, s.conv_k, w->out_dim, tokens, saved, saved_bytes, workspace, workspace_bytes, &kp, &wk));
    float* x = tokens ? kp.rows : wk.x;              // the stack runs in place: with the token outputs, in the buffer that is kept
    XMH_TRY(xmh_im2col_patch(image, B, 3, w->resolution, w->patch, wk.cols, stream));
    XMH_TRY(xmh_gemm_nt_f32(wk.cols, s.conv_k, w->conv1.w_f32, s.conv_k, w->conv1.bias, nullptr, 0, wk.patches, s.D, B * s.P, s.D, s.conv_k, 0, 0, stream));
    XMH_TRY(xmh::vit_assemble_keep(wk.patches, w->cls, w->pos, w->ln_pre_w, w->ln_pre_b, kLnEps, x, kp.pre, B, s.P, s.D, xmh::as_stream(stream)));
    if (w->layers > 0)
        XMH_TRY(xmh_clip_blocks_forward_saved(w->blocks, w->layers, s.D, w->heads, x, B, s.L, 0, nullptr, 2, wk.blocks, wk.blocks_bytes, kp.record,
                                              kp.record_bytes, stream));
    if (!tokens) {
        XMH_TRY(xmh_gather_rows(x, s.D, nullptr, 0, s.L, kp.rows, B, s.D, stream));
        return forward_tail(kp.rows, B, s.D, w->ln_post_w, w->ln_post_b, w->proj, wk.ln_out, out_cls, stream);
    }
    const int E = w->out_dim;
    XMH_TRY(forward_tail(x, B * s.L, s.D, w->ln_post_w, w->ln_post_b, w->proj, wk.ln_out, wk.y, stream));
    XMH_TRY(xmh_gather_rows(wk.y, E, nullptr, 0, s.L, out_cls, B, E, stream));
    hipLaunchKernelGGL(k_gather_patch_rows, dim3(blocks_for(B * s.P * E)), dim3(kThreads), 0, xmh::as_stream(stream), wk.y, B, s.L, E, out_tokens);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

// tokens == false: g_row [B, out_dim] is the gradient of the cls feature and g_tokens is not read
int vit_backward(const char* who, const xmh_vit_weights* w, const float* image, int64_t B, const void* saved, size_t saved_bytes, const float* g_row,
                 const float* g_tokens, bool tokens, const xmh_vit_grads* grads, int accumulate, void* workspace, size_t workspace_bytes,
                 xmh_stream_t stream) {
    if (B == 0) return XMH_OK;
    if (B < 0 || !w || !image || !saved || !(g_row || (tokens && g_tokens)) || !grads || !workspace) return xmh::fail(XMH_EINVAL, "%s: bad arguments", who);
    VitShape s;
    XMH_TRY(vit_shape(who, w, B, &s));
    if (w->layers > 0 && !grads->blocks) return xmh::fail(XMH_EINVAL, "%s: null block gradients", who);
    Kept kp;
    TowerWork wk;
    XMH_TRY(lay_out(who, B, s.L, s.D, w->layers, s.conv_k, w->out_dim, tokens, saved, saved_bytes, workspace, workspace_bytes, &kp, &wk));
    const xmh_vit_grads& gr = *grads;
    const int64_t M = B * s.L;
    const int D = s.D;
    hipStream_t st = xmh::as_stream(stream);
    // each stage exists for what is asked of it or of anything below it
    const bool need_dpre = gr.pos || gr.cls || gr.conv1;
    const bool front = need_dpre || gr.ln_pre_w || gr.ln_pre_b;
    const bool need_dy = front || any_block_asked(gr.blocks, w->layers);
    const float* g = g_row;
    if (tokens) {
        if (!need_dy && !gr.proj && !gr.ln_post_w && !gr.ln_post_b) return XMH_OK;
        hipLaunchKernelGGL(k_token_grads, dim3(blocks_for(M * w->out_dim)), dim3(kThreads), 0, st, g_row, g_tokens, nullptr, B, s.L, w->out_dim, wk.y);
        g = wk.y;
    }
    XMH_TRY(back_end(wk, kp.rows, w->ln_post_w, w->ln_post_b, w->proj, g, B, s.L, D, nullptr, tokens, gr.proj, gr.ln_post_w, gr.ln_post_b, need_dy,
                     accumulate, stream));
    if (!need_dy) {
        XMH_LAUNCH_CHECK(who);
        return XMH_OK;
    }
    XMH_TRY(xmh_clip_blocks_backward(w->blocks, w->layers, D, w->heads, B, s.L, 0, nullptr, kp.record, kp.record_bytes, wk.x, front, gr.blocks,
                                     accumulate, wk.blocks, wk.blocks_bytes, stream));
    if (front) {
        if (need_dpre) XMH_HIP(hipMemsetAsync(wk.t, 0, (size_t)M * D * sizeof(float), st));       // ln_pre has no residual: add into zeros
        ln_bwd(st, wk.gs, kp.pre, wk.x, w->ln_pre_w, wk.t, need_dpre, gr.ln_pre_w, gr.ln_pre_b, M, D, accumulate);
        if (gr.pos) batch_sum(st, wk.t, B, (int64_t)s.L * D, (int64_t)s.L * D, gr.pos, wk.bsum, accumulate);
        if (gr.cls) batch_sum(st, wk.t, B, D, (int64_t)s.L * D, gr.cls, wk.bsum, accumulate);
        if (gr.conv1) {
            XMH_TRY(xmh_im2col_patch(image, B, 3, w->resolution, w->patch, wk.cols, stream));
            hipLaunchKernelGGL(k_gather_patch_rows, dim3(blocks_for(B * s.P * D)), dim3(kThreads), 0, st, wk.t, B, s.L, D, wk.patches);
            weight_grads(st, wk.gs, wk.patches, wk.cols, B * s.P, D, s.conv_k, gr.conv1, nullptr, accumulate);
        }
    }
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

int text_forward(const char* who, const xmh_text_weights* w, const int64_t* ids, const uint8_t* key_padding_mask, int64_t B, int L, float* out_eos,
                 float* out_tokens, bool tokens, int32_t* eos_index, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes,
                 xmh_stream_t stream) {
    if (B == 0) return XMH_OK;
    if (B < 0 || !w || !ids || !out_eos || (tokens && !out_tokens) || !eos_index || !saved || !workspace)
        return xmh::fail(XMH_EINVAL, "%s: bad arguments", who);
    XMH_TRY(text_shape(who, w, B, L));
    const int D = w->width;
    Kept kp;
    TowerWork wk;
    XMH_TRY(lay_out(who, B, L, D, w->layers, 0, w->out_dim, tokens, saved, saved_bytes, workspace, workspace_bytes, &kp, &wk));
    float* x = tokens ? kp.rows : wk.x;              // as in vit_forward
    XMH_TRY(xmh_text_embed(ids, w->tok_emb, w->pos, x, eos_index, B, L, D, w->vocab, stream));
    if (w->layers > 0)
        XMH_TRY(xmh_clip_blocks_forward_saved(w->blocks, w->layers, D, w->heads, x, B, L, 1, key_padding_mask, 2, wk.blocks, wk.blocks_bytes,
                                              kp.record, kp.record_bytes, stream));
    if (!tokens) {
        XMH_TRY(xmh_gather_rows(x, D, eos_index, 0, L, kp.rows, B, D, stream));
        return forward_tail(kp.rows, B, D, w->ln_final_w, w->ln_final_b, w->proj, wk.ln_out, out_eos, stream);
    }
    XMH_TRY(forward_tail(x, B * L, D, w->ln_final_w, w->ln_final_b, w->proj, wk.ln_out, out_tokens, stream));
    return xmh_gather_rows(out_tokens, w->out_dim, eos_index, 0, L, out_eos, B, w->out_dim, stream);
}

int text_backward(const char* who, const xmh_text_weights* w, const int64_t* ids, const uint8_t* key_padding_mask, const int32_t* eos_index, int64_t B,
                  int L, const void* saved, size_t saved_bytes, const float* g_row, const float* g_tokens, bool tokens, const xmh_text_grads* grads,
                  int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    if (B == 0) return XMH_OK;
    if (B < 0 || !w || !ids || !eos_index || !saved || !(g_row || (tokens && g_tokens)) || !grads || !workspace)
        return xmh::fail(XMH_EINVAL, "%s: bad arguments", who);
    XMH_TRY(text_shape(who, w, B, L));
    if (w->layers > 0 && !grads->blocks) return xmh::fail(XMH_EINVAL, "%s: null block gradients", who);
    const int D = w->width;
    Kept kp;
    TowerWork wk;
    XMH_TRY(lay_out(who, B, L, D, w->layers, 0, w->out_dim, tokens, saved, saved_bytes, workspace, workspace_bytes, &kp, &wk));
    const xmh_text_grads& gr = *grads;
    hipStream_t st = xmh::as_stream(stream);
    const bool front = gr.pos || gr.tok;
    const bool need_dy = front || any_block_asked(gr.blocks, w->layers);
    const float* g = g_row;
    if (tokens) {
        if (!need_dy && !gr.proj && !gr.ln_final_w && !gr.ln_final_b) return XMH_OK;
        hipLaunchKernelGGL(k_token_grads, dim3(blocks_for(B * L * w->out_dim)), dim3(kThreads), 0, st, g_row, g_tokens, eos_index, B, L, w->out_dim, wk.y);
        g = wk.y;
    }
    XMH_TRY(back_end(wk, kp.rows, w->ln_final_w, w->ln_final_b, w->proj, g, B, L, D, eos_index, tokens, gr.proj, gr.ln_final_w, gr.ln_final_b, need_dy,
                     accumulate, stream));
    if (!need_dy) {
        XMH_LAUNCH_CHECK(who);
        return XMH_OK;
    }
    XMH_TRY(xmh_clip_blocks_backward(w->blocks, w->layers, D, w->heads, B, L, 1, key_padding_mask, kp.record, kp.record_bytes, wk.x, front, gr.blocks,
                                     accumulate, wk.blocks, wk.blocks_bytes, stream));
    if (gr.pos) {
        batch_sum(st, wk.x, B, (int64_t)L * D, (int64_t)L * D, gr.pos, wk.bsum, accumulate);
        if (!accumulate && L < w->context)           // no token sits at these positions
            XMH_HIP(hipMemsetAsync(gr.pos + (size_t)L * D, 0, (size_t)(w->context - L) * D * sizeof(float), st));
    }
    if (gr.tok) {
        if (!accumulate) XMH_HIP(hipMemsetAsync(gr.tok, 0, (size_t)w->vocab * D * sizeof(float), st));
        hipLaunchKernelGGL(k_tok_grad, dim3((unsigned)(B * L)), dim3(kThreads), 0, st, ids, wk.x, B * L, D, w->vocab, gr.tok, accumulate);
    }
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

}  // namespace

extern "C" size_t xmh_vit_train_saved_bytes(int64_t B, int L, int width, int layers) { return vit_saved_bytes(B, L, width, layers, false); }
extern "C" size_t xmh_text_train_saved_bytes(int64_t B, int L, int width, int layers) { return text_saved_bytes(B, L, width, layers, false); }
extern "C" size_t xmh_vit_train_ws_bytes(int64_t B, int L, int width, int conv_k, int out_dim) { return vit_ws_bytes(B, L, width, conv_k, out_dim, false); }
extern "C" size_t xmh_text_train_ws_bytes(int64_t B, int L, int width, int out_dim) { return text_ws_bytes(B, L, width, out_dim, false); }
extern "C" size_t xmh_vit_train_tokens_saved_bytes(int64_t B, int L, int width, int layers) { return vit_saved_bytes(B, L, width, layers, true); }
extern "C" size_t xmh_text_train_tokens_saved_bytes(int64_t B, int L, int width, int layers) { return text_saved_bytes(B, L, width, layers, true); }
extern "C" size_t xmh_vit_train_tokens_ws_bytes(int64_t B, int L, int width, int conv_k, int out_dim) {
    return vit_ws_bytes(B, L, width, conv_k, out_dim, true);
}
extern "C" size_t xmh_text_train_tokens_ws_bytes(int64_t B, int L, int width, int out_dim) { return text_ws_bytes(B, L, width, out_dim, true); }

extern "C" int xmh_vit_train_forward(const xmh_vit_weights* w, const float* image, int64_t B, float* out_cls, void* saved, size_t saved_bytes,
                                     void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_vit_train_forward");
    return vit_forward("xmh_vit_train_forward", w, image, B, out_cls, nullptr, false, saved, saved_bytes, workspace, workspace_bytes, stream);
}

extern "C" int xmh_vit_train_forward_tokens(const xmh_vit_weights* w, const float* image, int64_t B, float* out_cls, float* out_tokens, void* saved,
                                            size_t saved_bytes, void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_vit_train_forward_tokens");
    return vit_forward("xmh_vit_train_forward_tokens", w, image, B, out_cls, out_tokens, true, saved, saved_bytes, workspace, workspace_bytes, stream);
}

extern "C" int xmh_vit_backward(const xmh_vit_weights* w, const float* image, int64_t B, const void* saved, size_t saved_bytes, const float* g,
                                const xmh_vit_grads* grads, int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_vit_backward");
    return vit_backward("xmh_vit_backward", w, image, B, saved, saved_bytes, g, nullptr, false, grads, accumulate, workspace, workspace_bytes, stream);
}

extern "C" int xmh_vit_backward_tokens(const xmh_vit_weights* w, const float* image, int64_t B, const void* saved, size_t saved_bytes,
                                       const float* g_cls, const float* g_tokens, const xmh_vit_grads* grads, int accumulate, void* workspace,
                                       size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_vit_backward_tokens");
    return vit_backward("xmh_vit_backward_tokens", w, image, B, saved, saved_bytes, g_cls, g_tokens, true, grads, accumulate, workspace,
                        workspace_bytes, stream);
}

extern "C" int xmh_text_train_forward(const xmh_text_weights* w, const int64_t* ids, const uint8_t* key_padding_mask, int64_t B, int L,
                                      float* out_eos, int32_t* eos_index, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes,
                                      xmh_stream_t stream) {
    XMH_RANGE("xmh_text_train_forward");
    return text_forward("xmh_text_train_forward", w, ids, key_padding_mask, B, L, out_eos, nullptr, false, eos_index, saved, saved_bytes, workspace,
                        workspace_bytes, stream);
}

extern "C" int xmh_text_train_forward_tokens(const xmh_text_weights* w, const int64_t* ids, const uint8_t* key_padding_mask, int64_t B, int L,
                                             float* out_eos, float* out_tokens, int32_t* eos_index, void* saved, size_t saved_bytes, void* workspace,
                                             size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_text_train_forward_tokens");
    return text_forward("xmh_text_train_forward_tokens", w, ids, key_padding_mask, B, L, out_eos, out_tokens, true, eos_index, saved, saved_bytes,
                        workspace, workspace_bytes, stream);
}

extern "C" int xmh_text_backward(const xmh_text_weights* w, const int64_t* ids, const uint8_t* key_padding_mask, const int32_t* eos_index, int64_t B,
                                 int L, const void* saved, size_t saved_bytes, const float* g, const xmh_text_grads* grads, int accumulate,
                                 void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_text_backward");
    return text_backward("xmh_text_backward", w, ids, key_padding_mask, eos_index, B, L, saved, saved_bytes, g, nullptr, false, grads, accumulate,
                         workspace, workspace_bytes, stream);
}

extern "C" int xmh_text_backward_tokens(const xmh_text_weights* w, const int64_t* ids, const uint8_t* key_padding_mask, const int32_t* eos_index,
                                        int64_t B, int L, const void* saved, size_t saved_bytes, const float* g_eos, const float* g_tokens,
                                        const xmh_text_grads* grads, int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_text_backward_tokens");
    return text_backward("xmh_text_backward_tokens", w, ids, key_padding_mask, eos_index, B, L, saved, saved_bytes, g_eos, g_tokens, true, grads,
                         accumulate, workspace, workspace_bytes, stream);
}
