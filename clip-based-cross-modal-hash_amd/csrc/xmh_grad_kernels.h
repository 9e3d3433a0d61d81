// What the three gradient files share (xmh_block_grad.hip: the block stack; xmh_tower_grad.hip: the towers' front and back ends;
// xmh_mith_grad.hip: MITH's hash head): the launchers of the exact-fp32 product kernel with its split reduction, of the bias column
// sums and of the LayerNorm backward, and the workspace and shape helpers.  The kernels and the launchers' bodies are in xmh_grad_kernels.hip,
// compiled once, not per including file.  One fixed order per reduction (no float atomics): two calls agree to the bit; no host sync, no allocation.
#pragma once
#include "xmh_common.h"
#include "xmh_device.h"

namespace xmh::grad {

constexpr int kThreads = 256, kMaxSplits = 16;
constexpr float kLnEps = 1e-5f;                  // nn.LayerNorm default, as in the forward
constexpr int kLnChunks = 64;                    // row chunks of the LayerNorm column sums
constexpr int64_t kMaxRows = 1ll << 21;

// what weight_grads and ln_bwd need beside their operands
struct GradScratch {
    double* stats;    // [M][2]   LayerNorm row statistics
    double* lnpart;   // [kLnChunks][2][D]
    float* part;      // partials of a split TN product
    double* bpart;    // [kMaxSplits][N] bias partials
};

// a product dW [N, K] = dY^T X over M rows that weight_grads will be asked for
struct TnShape {
    int64_t M;
    int N, K;
};

// how many chunks the token reduction of dW [N, K] = dY^T X is cut into, and their length (a multiple of the product's slab)
void tn_split(int64_t M, int N, int K, int* splits, int* chunk);

// dx [M, K] = dy [M, N] w [N, K] (. QuickGELU'(gelu_pre))
void launch_nn(hipStream_t st, const float* dy, const float* w, int64_t M, int N, int K, float* dx, const float* gelu_pre);

// dw [N, K] = dy [M, N]^T x [M, K] and, when db is not NULL, db [N] = column sums of dy from the same pass; either may be NULL
void weight_grads(hipStream_t st, const GradScratch& wk, const float* dy, const float* x, int64_t M, int N, int K, float* dw, float* db, int accumulate);

// LayerNorm backward: dres += LN'(dn; x) when need_dx, dgamma / dbeta when asked for
void ln_bwd(hipStream_t st, const GradScratch& wk, const float* x, const float* dn, const float* gamma, float* dres, bool need_dx, float* dgamma,
            float* dbeta, int64_t M, int D, int accumulate);

// GradScratch's four buffers from a workspace: `rows` LayerNorm rows of width D, bias gradients up to `bias_width` wide, and the
// partials of the largest split product among `tn` (one with no rows or no columns is never launched)
template <size_t n>
void take_scratch(xmh::Arena& ar, int64_t rows, int D, int bias_width, const TnShape (&tn)[n], GradScratch* gs) {
    gs->stats = ar.take<double>((size_t)rows * 2);
    gs->lnpart = ar.take<double>((size_t)kLnChunks * 2 * D);
    size_t most = 0;
    for (const TnShape& s : tn) {
        if (s.M <= 0 || s.K <= 0) continue;
        int splits, chunk;
        tn_split(s.M, s.N, s.K, &splits, &chunk);
        if (splits > 1 && (size_t)splits * s.N * s.K > most) most = (size_t)splits * s.N * s.K;
    }
    gs->part = ar.take<float>(most);
    gs->bpart = ar.take<double>((size_t)kMaxSplits * bias_width);
}

// is any gradient of this block asked for
inline bool block_asked(const xmh_clip_block_grads& g) {
    return g.ln1_w || g.ln1_b || g.qkv_w || g.qkv_b || g.out_w || g.out_b || g.ln2_w || g.ln2_b || g.fc_w || g.fc_b || g.proj_w || g.proj_b;
}

// the shapes the size functions of the three files answer for (the towers add their own bound on the width) ...
inline bool stack_limits_ok(int64_t B, int L, int width) { return B > 0 && L > 0 && width > 0 && width % 4 == 0 && L <= 128 && B * L <= kMaxRows; }

// ... and what the entry points say beyond them, after their own check of the width
inline int check_stack_limits(const char* who, int64_t B, int L, int width, int heads) {
    if (width / heads != 64) return xmh::fail(XMH_ENOTSUP, "%s: head dim %d (only 64, CLIP's width/heads)", who, width / heads);
    if (L > 128) return xmh::fail(XMH_ENOTSUP, "%s: L=%d > 128", who, L);
    if (B * L > kMaxRows) return xmh::fail(XMH_ENOTSUP, "%s: %lld x %d tokens (at most 2^21)", who, (long long)B, L);
    return XMH_OK;
}

}  // namespace xmh::grad
