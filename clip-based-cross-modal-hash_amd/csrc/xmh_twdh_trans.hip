// The stage that MAKES TwDH's short-code transforms (reference runners/TwDH/transform_matrix_generation/model.py:6-24 and
// train.py:44-96, 141-176): the objective of the matrix M [2L, 2S], its gradient, and the lossless check.
//
//   x = hash_convert(t_long) is one-hot per pair, so z = x . M is a GATHER: z[b][j] = sum_l M[2 l + bit_l(b)][j], L additions per
//   entry where the product would spend 2 L multiply-adds, half of them by zero; and dM = x^T . g_z is a gather too:
//   dM[2 l + c][j] = sum over the rows b whose long bit l is c of g_z[b][j].  x is never written: both read the packed target bits
//   (xmh_twdh_targets' words for the two streams bit = {0, L}, K = {L, S}; the short stream starts at bit L, inside a word when L is
//   no multiple of 32).  Neither product goes through xmh_mfma_mm.h (DESIGN 3.22 says why).
//
//   xmh_twdh_trans_loss   hash = 1 - mean_{b,s}((p0 - p1)^2), bce = nn.BCELoss()(p, hash_convert(t_short)) (mean over B 2S, each log
//                         clamped at -100), lasso = alpha |M|_1, p = pair_softmax(z).  2 launches: (row, 64-column chunk) blocks and
//                         the blocks of the L1 norm into double partials, then one block that adds them in index order.
//   xmh_twdh_trans_grad   g_z [B, 2S] (BCE's (p - t) / max(p (1 - p), 1e-12) / (B 2S), the quantisation term's -+ 2 (p0 - p1) / (B S),
//                         through the pair-softmax backward) into the workspace, then dM = up (x^T g_z + alpha sign(M)).  2 launches.
//   xmh_twdh_trans_check  argmax over each pair of hash_convert(long_centre) . M against short_centre > 0, equal logits giving bit 0:
//                         a count and a [C][ceil(S/32)] bitmap of the class / bit pairs that disagree.  A memset and 1 launch.
//
// Every element is computed in double and rounded once; every sum is double and runs in one fixed order (two calls on equal inputs
// agree to the bit); no float atomics (the check's count is an integer), no host synchronisation, no allocation.
//
// NaN: the gather reads only the selected row of a pair, so a NaN in M[r][j] reaches the logits z[b][j] of the rows b that select r
// (the matrix product's 0 * NaN would reach every row), from there both entries of that pair, the loss terms, and in dM the columns of
// that pair in the rows (2 l + c) some such b selects; |M|_1 and dM[r][j] itself (sign(NaN)) are NaN whichever rows select r.
#include "xmh_common.h"
#include "xmh_device.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxB = 4096, kMaxBits = 4096, kMaxC = 1024;
constexpr int kLassoBlocks = 64;                  // blocks of the L1 norm, each a grid-stride share
constexpr int kLPer = 4;                          // long bits per thread of the dM kernel

struct TargetBits {                               // a row of xmh_twdh_targets' words
    const uint32_t* w;
    __device__ __forceinline__ int operator()(int k) const { return (w[k >> 5] >> (k & 31)) & 1u; }
    __device__ __forceinline__ uint32_t word(int i, int) const { return w[i]; }
};
struct CentreBits {                               // centre > 0 of a row of the int8 centres
    const int8_t* c;
    __device__ __forceinline__ int operator()(int k) const { return c[k] > 0; }
    __device__ __forceinline__ uint32_t word(int i, int K) const {        // bits [32 i, 32 i + 32) below K, as a word
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 32; ++b) v |= (uint32_t)(32 * i + b < K && c[32 * i + b] > 0) << b;
        return v;
    }
};

// z[j] = sum_l M[2 l + bit(l)][j] of one row for the block's 64 columns j = col0 + lane: wave w adds its quarter of the long bits (whole
// 32-bit words of them) in index order, then the four quarters are added in wave order.  The bits come a word at a time, so that the 32
// row addresses of a word are known together and their loads are in flight together; the additions keep their order.  Valid on the
// threads of wave 0 with j < S2 (0 elsewhere).
template <typename Bits>
__device__ __forceinline__ double row_logit(const float* __restrict__ M, Bits bits, int L, int S2, int col0, double (*sh)[64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = col0 + lane;
    const int words = (L + 31) >> 5, per = (words + kWaves - 1) / kWaves;
    const int w0 = wave * per, w1 = w0 + per < words ? w0 + per : words;
    double acc = 0.0;
    if (j < S2)
        for (int wi = w0; wi < w1; ++wi) {
            const uint32_t word = bits.word(wi, L);
            const int n = L - 32 * wi < 32 ? L - 32 * wi : 32;
            float v[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int l = 32 * wi + (i < n ? i : 0);                  // past the end: a valid address whose value is not added
                v[i] = M[(size_t)(2 * l + ((word >> i) & 1u)) * S2 + j];
            }
#pragma unroll
            for (int i = 0; i < 32; ++i)
                if (i < n) acc += (double)v[i];
        }
    sh[wave][lane] = acc;
    __syncthreads();
    double z = 0.0;
    if (wave == 0 && j < S2) {
        z = sh[0][lane];
        for (int w = 1; w < kWaves; ++w) z += sh[w][lane];
    }
    __syncthreads();
    return z;
}

__device__ __forceinline__ double clamped_log(double x) {
    const double l = log(x);
    return l < -100.0 ? -100.0 : l;               // torch's clamp of BCELoss; a NaN stays a NaN
}

// the probability of this lane's entry and of its partner in the pair (lanes 2 s and 2 s + 1 hold one pair)
__device__ __forceinline__ void pair_probs(double z, double* p, double* q) {
    const double zo = __shfl_xor(z, 1);
    const double m = fmax(z, zo);
    const double e = exp(z - m), eo = exp(zo - m);
    *p = e / (e + eo);
    *q = eo / (e + eo);
}

// grid (B + kLassoBlocks, chunks): block (b, c) the row's BCE sum and quantisation sum over its 64 columns, into part[(b chunks + c) 2];
// block (B + i, 0) share i of |M|_1, into lasso[i]
__global__ __launch_bounds__(kThreads) void k_trans_loss_part(const float* __restrict__ M, const uint32_t* __restrict__ targets, int Tw, int B,
                                                             int L, int S2, double* __restrict__ part, double* __restrict__ lasso) {
    __shared__ double sh[kWaves][64];
    __shared__ double red[kWaves];
    if ((int)blockIdx.x >= B) {
        if (blockIdx.y) return;
        const size_t n = (size_t)2 * L * S2;
        const int i = blockIdx.x - B;
        double a = 0.0;
        for (size_t e = (size_t)i * kThreads + threadIdx.x; e < n; e += (size_t)kLassoBlocks * kThreads) a += fabs((double)M[e]);
        a = xmh::block_sum<kWaves>(a, red);
        if (threadIdx.x == 0) lasso[i] = a;
        return;
    }
    const int b = blockIdx.x, col0 = blockIdx.y * 64, j = col0 + (threadIdx.x & 63);
    const TargetBits bits{targets + (size_t)b * Tw};
    const double z = row_logit(M, bits, L, S2, col0, sh);
    double bce = 0.0, quan = 0.0;
    if (threadIdx.x < 64) {                       // the whole of wave 0 takes part in the shuffle
        double p, q;
        pair_probs(z, &p, &q);
        if (j < S2) {
            const bool one = (j & 1) == bits(L + (j >> 1));       // the target pair is (1, 0) for bit 0 and (0, 1) for bit 1
            bce = -(one ? clamped_log(p) : clamped_log(1.0 - p));
            if (!(j & 1)) quan = (p - q) * (p - q);
        }
    }
    bce = xmh::block_sum<kWaves>(bce, red);
    quan = xmh::block_sum<kWaves>(quan, red);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)b * gridDim.y + blockIdx.y) * 2;
        o[0] = bce;
        o[1] = quan;
    }
}

// one block: thread t adds the partials t, t + 256, .. in index order, the block sum joins them in a fixed order.  out: total, hash, bce,
// lasso
__global__ __launch_bounds__(kThreads) void k_trans_loss_reduce(const double* __restrict__ part, const double* __restrict__ lasso, int nparts,
                                                               int B, int S, double alpha, double* __restrict__ out) {
    __shared__ double red[kWaves];
    double bce = 0.0, quan = 0.0, l1 = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kThreads) {
        bce += part[2 * (size_t)i];
        quan += part[2 * (size_t)i + 1];
    }
    if (threadIdx.x < kLassoBlocks) l1 = lasso[threadIdx.x];
    bce = xmh::block_sum<kWaves>(bce, red);
    quan = xmh::block_sum<kWaves>(quan, red);
    l1 = xmh::block_sum<kWaves>(l1, red);
    if (threadIdx.x == 0) {
        const double hash = 1.0 - quan / ((double)B * S), b = bce / ((double)B * 2.0 * S), la = alpha * l1;
        out[0] = hash + b + la;
        out[1] = hash;
        out[2] = b;
        out[3] = la;
    }
}

// grid (B, chunks): g_z of the row's 64 columns, as doubles
__global__ __launch_bounds__(kThreads) void k_trans_gz(const float* __restrict__ M, const uint32_t* __restrict__ targets, int Tw, int B, int L,
                                                      int S2, double* __restrict__ gz) {
    __shared__ double sh[kWaves][64];
    const int b = blockIdx.x, col0 = blockIdx.y * 64, j = col0 + (threadIdx.x & 63);
    const TargetBits bits{targets + (size_t)b * Tw};
    const double z = row_logit(M, bits, L, S2, col0, sh);
    if (threadIdx.x >= 64) return;
    double p, q;
    pair_probs(z, &p, &q);
    const int jj = j < S2 ? j : 0;                // lanes past the width compute on column 0 and store nothing
    const double t = (jj & 1) == bits(L + (jj >> 1)) ? 1.0 : 0.0;
    const double n2 = (double)B * (double)S2, n1 = n2 * 0.5;
    // d loss / d p of this entry: BCE as autograd returns it, and d(1 - mean (p0 - p1)^2): -2 (p0 - p1) / (B S) for p0, + for p1
    const double d = (jj & 1) ? q - p : p - q;    // p0 - p1
    const double g = (p - t) / fmax(p * (1.0 - p), 1e-12) / n2 + ((jj & 1) ? 2.0 : -2.0) * d / n1;
    const double go = __shfl_xor(g, 1);
    const double dot = (jj & 1) ? go * q + g * p : g * p + go * q;        // g0 p0 + g1 p1, the same bits on both lanes
    if (j < S2) gz[(size_t)b * S2 + j] = p * (g - dot);
}

// thread per (group of kLPer long bits, column): dM[2 l + c][j] = up (sum over the rows b with bit l == c of g_z[b][j], b ascending,
// + alpha sign(M)), written or added
__global__ __launch_bounds__(kThreads) void k_trans_dm(const float* __restrict__ M, const uint32_t* __restrict__ targets, int Tw, int B, int L,
                                                      int S2, double alpha, const double* __restrict__ gz, const float* __restrict__ up,
                                                      float* __restrict__ dM, int accumulate) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int groups = (L + kLPer - 1) / kLPer;
    if (e >= (int64_t)groups * S2) return;
    const int j = (int)(e % S2), l0 = (int)(e / S2) * kLPer;     // kLPer divides 32: a group lies in one target word
    double s[kLPer][2] = {};
#pragma unroll 4
    for (int b = 0; b < B; ++b) {
        const uint32_t w = targets[(size_t)b * Tw + (l0 >> 5)] >> (l0 & 31);
        const double g = gz[(size_t)b * S2 + j];
#pragma unroll
        for (int i = 0; i < kLPer; ++i) {
            const bool on = (w >> i) & 1u;
            s[i][0] += on ? 0.0 : g;
            s[i][1] += on ? g : 0.0;
        }
    }
    const double u = up ? (double)up[0] : 1.0;
#pragma unroll
    for (int i = 0; i < kLPer; ++i) {
        if (l0 + i >= L) break;
        for (int c = 0; c < 2; ++c) {
            const size_t at = (size_t)(2 * (l0 + i) + c) * S2 + j;
            const double m = (double)M[at];
            const double sign = m > 0.0 ? 1.0 : m < 0.0 ? -1.0 : m;      // sign(0) = 0, and a NaN stays one
            const double v = u * (s[i][c] + alpha * sign);
            dM[at] = accumulate ? (float)((double)dM[at] + v) : (float)v;
        }
    }
}

// grid (C, chunks): the class's logits from its long centre; the even lane of a pair decides the bit (z1 > z0: equal logits give 0)
// and compares with the short centre; the ballot's even bits are squeezed into one 32-bit word of the bitmap per chunk
__global__ __launch_bounds__(kThreads) void k_trans_check(const float* __restrict__ M, const int8_t* __restrict__ centres, int L, int S,
                                                         int32_t* __restrict__ wrong) {
    __shared__ double sh[kWaves][64];
    const int c = blockIdx.x, col0 = blockIdx.y * 64, lane = threadIdx.x & 63, j = col0 + lane, S2 = 2 * S;
    const CentreBits bits{centres + (size_t)c * (L + S)};
    const double z = row_logit(M, bits, L, S2, col0, sh);
    if (threadIdx.x >= 64) return;
    const double zo = __shfl_xor(z, 1);
    const bool bad = j < S2 && !(j & 1) && (int)(zo > z) != bits(L + (j >> 1));
    const unsigned long long mask = __ballot(bad);
    if (lane == 0) {
        uint32_t word = 0;
        for (int s = 0; s < 32; ++s) word |= (uint32_t)((mask >> (2 * s)) & 1ull) << s;
        wrong[1 + (size_t)c * gridDim.y + blockIdx.y] = (int32_t)word;
        if (word) atomicAdd(wrong, __popc(word));
    }
}

int check_shape(const char* who, int64_t B, int L, int S) {
    if (B <= 0 || L <= 0 || S <= 0) return xmh::fail(XMH_EINVAL, "%s: bad shape B=%lld L=%d S=%d", who, (long long)B, L, S);
    if (B > kMaxB || (int64_t)L + S > kMaxBits)
        return xmh::fail(XMH_ENOTSUP, "%s: B=%lld L=%d S=%d outside B <= %d, L + S <= %d", who, (long long)B, L, S, kMaxB, kMaxBits);
    return XMH_OK;
}

struct Carve {
    double *part, *lasso, *gz;
    size_t bytes;
};

// the pieces of the workspace; the loss uses part and lasso, the gradient g_z
Carve carve(void* base, int64_t B, int S) {
    xmh::Arena a{static_cast<char*>(base)};
    Carve c;
    c.part = a.take<double>((size_t)B * xmh::ceil_div(2 * S, 64) * 2);
    c.lasso = a.take<double>(kLassoBlocks);
    c.gz = a.take<double>((size_t)B * 2 * S);
    c.bytes = a.used;
    return c;
}

}  // namespace

extern "C" size_t xmh_twdh_trans_ws_bytes(int64_t B, int L, int S) {
    if (B <= 0 || L <= 0 || S <= 0 || B > kMaxB || (int64_t)L + S > kMaxBits) return 0;
    return carve(nullptr, B, S).bytes;
}

extern "C" int xmh_twdh_trans_loss(const float* M, const uint32_t* targets, int64_t B, int L, int S, double alpha, void* workspace,
                                   size_t workspace_bytes, double* out4, xmh_stream_t stream) {
    XMH_RANGE("xmh_twdh_trans_loss");
    const char* who = "xmh_twdh_trans_loss";
    if (int rc = check_shape(who, B, L, S)) return rc;
    if (!M || !targets || !out4 || !workspace) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return xmh::fail(XMH_EINVAL, "%s: workspace not 8-byte aligned", who);
    const Carve c = carve(workspace, B, S);
    if (workspace_bytes < c.bytes) return xmh::fail(XMH_ENOMEM, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, c.bytes);
    const int chunks = (int)xmh::ceil_div(2 * S, 64), Tw = (L + S + 31) / 32;
    hipStream_t s = xmh::as_stream(stream);
    hipLaunchKernelGGL(k_trans_loss_part, dim3((unsigned)B + kLassoBlocks, chunks), dim3(kThreads), 0, s, M, targets, Tw, (int)B, L, 2 * S, c.part,
                       c.lasso);
    hipLaunchKernelGGL(k_trans_loss_reduce, dim3(1), dim3(kThreads), 0, s, c.part, c.lasso, (int)B * chunks, (int)B, S, alpha, out4);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

extern "C" int xmh_twdh_trans_grad(const float* M, const uint32_t* targets, int64_t B, int L, int S, double alpha, const float* upstream,
                                   float* dM, int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_twdh_trans_grad");
    const char* who = "xmh_twdh_trans_grad";
    if (int rc = check_shape(who, B, L, S)) return rc;
    if (!M || !targets || !dM || !workspace) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return xmh::fail(XMH_EINVAL, "%s: workspace not 8-byte aligned", who);
    const Carve c = carve(workspace, B, S);
    if (workspace_bytes < c.bytes) return xmh::fail(XMH_ENOMEM, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, c.bytes);
    const int chunks = (int)xmh::ceil_div(2 * S, 64), Tw = (L + S + 31) / 32;
    hipStream_t s = xmh::as_stream(stream);
    hipLaunchKernelGGL(k_trans_gz, dim3((unsigned)B, chunks), dim3(kThreads), 0, s, M, targets, Tw, (int)B, L, 2 * S, c.gz);
    const int64_t n = xmh::ceil_div(L, kLPer) * 2 * S;
    hipLaunchKernelGGL(k_trans_dm, dim3((unsigned)xmh::ceil_div(n, kThreads)), dim3(kThreads), 0, s, M, targets, Tw, (int)B, L, 2 * S, alpha, c.gz,
                       upstream, dM, accumulate);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}

extern "C" int xmh_twdh_trans_check(const float* M, const int8_t* centres, int C, int L, int S, int32_t* wrong, xmh_stream_t stream) {
    XMH_RANGE("xmh_twdh_trans_check");
    const char* who = "xmh_twdh_trans_check";
    if (C <= 0 || L <= 0 || S <= 0) return xmh::fail(XMH_EINVAL, "%s: bad shape C=%d L=%d S=%d", who, C, L, S);
    if (!M || !centres || !wrong) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if (C > kMaxC || (int64_t)L + S > kMaxBits)
        return xmh::fail(XMH_ENOTSUP, "%s: C=%d L=%d S=%d outside C <= %d, L + S <= %d", who, C, L, S, kMaxC, kMaxBits);
    hipStream_t s = xmh::as_stream(stream);
    XMH_HIP(hipMemsetAsync(wrong, 0, sizeof(int32_t), s));
    // a chunk of 64 columns is 32 short bits: one word of the bitmap
    hipLaunchKernelGGL(k_trans_check, dim3(C, (S + 31) / 32), dim3(kThreads), 0, s, M, centres, L, S, wrong);
    XMH_LAUNCH_CHECK(who);
    return XMH_OK;
}
