// BertAdam (reference models/common/optimizer.py:50-167) as one fused multi-tensor step: any number of fp32 tensors, two launches.
//
//   per tensor:  norm = |g|_2, coef = min(1, max_grad_norm / (norm + 1e-6)) when max_grad_norm > 0 (else 1), g' = g coef
//                m = m b1 + (1 - b1) g'      v = v b2 + (1 - b2) g' g'      u = m / (sqrt(v) + e) [+ weight_decay p]      p -= lr u
//
//   k_bertadam_sumsq   one block per chunk of kChunk elements: sum of g^2 in double -> partial[chunk]
//   k_bertadam_update  one block per chunk: re-adds the partials of ITS tensor (every block of a tensor in the same fixed order, so
//                      they all hold the same coef to the bit), then streams p, g, m, v once and writes p, m, v (and g' when clipped)
//
// The tensors are described by a device-resident table (xmh_bertadam_tensor) and a chunk map (xmh_bertadam_chunk_ref) the caller
// uploads; nothing here synchronises with the host or allocates, and there are no atomics: every sum has one fixed order.
// Bound: 32-36 bytes per parameter (g once for the norm; p, g, m, v read, p, m, v written; g written where clipped), pure HBM stream.
// Shape of the stream: kChunk = 16384 elements and 256 threads, so a block moves 64 KB per array in 16 rounds of one 16-byte access
// per lane; two rounds of the four arrays are loaded before the first is used (128 B in flight per lane, 32 KB per block, several
// blocks per CU).  ViT-B/32 + heads (151 M parameters) is about 9,300 chunks: 36 per CU, a tail of under 3 %.
#include "xmh_common.h"
#include "xmh_device.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kChunk = 16384;                    // elements per block; a multiple of 4 kThreads (whole float4 rounds)
constexpr int kRounds = kChunk / (4 * kThreads); // 16 float4 per lane and array
constexpr int kUnroll = 2;                       // rounds whose loads are issued before the first is consumed

using Tensor = xmh_bertadam_tensor;
using ChunkRef = xmh_bertadam_chunk_ref;

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__global__ __launch_bounds__(kThreads) void k_bertadam_sumsq(const Tensor* __restrict__ table, const ChunkRef* __restrict__ map,
                                                             double* __restrict__ partial) {
    __shared__ double sh[kWaves];
    const ChunkRef c = map[blockIdx.x];
    const Tensor t = table[c.tensor];
    if (!(t.max_grad_norm > 0.0f)) return;       // no clipping: the update never reads this tensor's partials
    const int64_t left = t.numel - c.start;
    const int n = left < kChunk ? (int)left : kChunk;
    const float* g = t.g + c.start;
    double s = 0.0;
    if (aligned16(g)) {
        const float4* g4 = reinterpret_cast<const float4*>(g);
        const int n4 = n >> 2;
#pragma unroll 4
        for (int i = threadIdx.x; i < n4; i += kThreads) {
            const float4 a = g4[i];
            s = fma((double)a.x, (double)a.x, s);
            s = fma((double)a.y, (double)a.y, s);
            s = fma((double)a.z, (double)a.z, s);
            s = fma((double)a.w, (double)a.w, s);
        }
        const int i = (n4 << 2) + threadIdx.x;
        if (i < n) s = fma((double)g[i], (double)g[i], s);
    } else {
#pragma unroll 4
        for (int i = threadIdx.x; i < n; i += kThreads) s = fma((double)g[i], (double)g[i], s);
    }
    s = xmh::block_sum<kWaves>(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

struct Coefs {
    float coef, b1, b2, c1, c2, e, wd, lr;
};

// one element, the reference's operation order: mul_ then add_ with alpha (a fused multiply-add on either side), addcmul_,
// the division, the decay added to the update, the product with lr rounded before it is subtracted
__device__ __forceinline__ void update_one(const Coefs& k, float& p, float& g, float& m, float& v) {
    g = __fmul_rn(g, k.coef);
    m = fmaf(k.c1, g, __fmul_rn(m, k.b1));
    v = fmaf(__fmul_rn(k.c2, g), g, __fmul_rn(v, k.b2));
    float u = m / (sqrtf(v) + k.e);
    if (k.wd > 0.0f) u = fmaf(k.wd, p, u);
    p = __fsub_rn(p, __fmul_rn(k.lr, u));
}

__device__ __forceinline__ void update_four(const Coefs& k, float4& p, float4& g, float4& m, float4& v) {
    update_one(k, p.x, g.x, m.x, v.x);
    update_one(k, p.y, g.y, m.y, v.y);
    update_one(k, p.z, g.z, m.z, v.z);
    update_one(k, p.w, g.w, m.w, v.w);
}

__global__ __launch_bounds__(kThreads) void k_bertadam_update(const Tensor* __restrict__ table, const ChunkRef* __restrict__ map,
                                                              const double* __restrict__ partial) {
    __shared__ double sh[kWaves];
    const ChunkRef c = map[blockIdx.x];
    const Tensor t = table[c.tensor];
    Coefs k = {1.0f, t.b1, t.b2, t.one_minus_b1, t.one_minus_b2, t.e, t.weight_decay, t.lr};
    bool clipped = false;
    if (t.max_grad_norm > 0.0f) {
        // lane j adds partials j, j + 256, ... of the tensor, then the block sum: the same order in every block of this tensor
        const int nchunk = (int)((t.numel + kChunk - 1) / kChunk);
        double s = 0.0;
        for (int j = threadIdx.x; j < nchunk; j += kThreads) s += partial[c.first_chunk + j];
        s = xmh::block_sum<kWaves>(s, sh);
        const float norm = (float)sqrt(s);
        const float q = t.max_grad_norm / (norm + 1e-6f);
        clipped = !(q >= 1.0f);                  // a NaN norm clips with a NaN coefficient, as torch.clamp(max=1) passes it on
        if (clipped) k.coef = q;
    }
    const int64_t left = t.numel - c.start;
    const int n = left < kChunk ? (int)left : kChunk;
    float* p = t.p + c.start;
    float* g = t.g + c.start;
    float* m = t.m + c.start;
    float* v = t.v + c.start;
    if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v)) {
        float4* p4 = reinterpret_cast<float4*>(p);
        float4* g4 = reinterpret_cast<float4*>(g);
        float4* m4 = reinterpret_cast<float4*>(m);
        float4* v4 = reinterpret_cast<float4*>(v);
        const int n4 = n >> 2;
        for (int base = 0; base < n4; base += kUnroll * kThreads) {
            float4 rp[kUnroll], rg[kUnroll], rm[kUnroll], rv[kUnroll];
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) {
                const int i = base + r * kThreads + threadIdx.x;
                if (i < n4) {
                    rp[r] = p4[i];
                    rg[r] = g4[i];
                    rm[r] = m4[i];
                    rv[r] = v4[i];
                }
            }
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) {
                const int i = base + r * kThreads + threadIdx.x;
                if (i < n4) {
                    update_four(k, rp[r], rg[r], rm[r], rv[r]);
                    p4[i] = rp[r];
                    m4[i] = rm[r];
                    v4[i] = rv[r];
                    if (clipped) g4[i] = rg[r];
                }
            }
        }
        const int i = (n4 << 2) + threadIdx.x;   // at most 3 elements past the last whole float4
        if (i < n) {
            float a = p[i], b = g[i], d = m[i], w = v[i];
            update_one(k, a, b, d, w);
            p[i] = a;
            m[i] = d;
            v[i] = w;
            if (clipped) g[i] = b;
        }
    } else {
        for (int i = threadIdx.x; i < n; i += kThreads) {
            float a = p[i], b = g[i], d = m[i], w = v[i];
            update_one(k, a, b, d, w);
            p[i] = a;
            m[i] = d;
            v[i] = w;
            if (clipped) g[i] = b;
        }
    }
}

static_assert(kRounds % kUnroll == 0, "whole unrolled rounds per chunk");
static_assert(sizeof(Tensor) == 72 &&sizeof(ChunkRef) == 16, "table layouts are part of the ABI (xmh/optim.py mirrors them)");

}  // namespace

extern "C" int64_t xmh_bertadam_chunk(void) { return kChunk; }

extern "C" size_t xmh_bertadam_ws_bytes(int64_t n_tensors, int64_t total_chunks) {
    if (n_tensors < 0 || total_chunks < 0 || total_chunks > INT32_MAX) return 0;
    return xmh::align256((size_t)total_chunks * sizeof(double));
}

extern "C" int xmh_bertadam_step(const xmh_bertadam_tensor* table, int64_t n_tensors, const xmh_bertadam_chunk_ref* chunk_map,
                                 int64_t total_chunks, void* ws, size_t ws_bytes, xmh_stream_t stream) {
    XMH_RANGE("xmh_bertadam_step");
    if (n_tensors < 0 || total_chunks < 0)
        return xmh::fail(XMH_EINVAL, "xmh_bertadam_step: negative count n_tensors=%lld total_chunks=%lld", (long long)n_tensors,
                         (long long)total_chunks);
    if (n_tensors == 0) return XMH_OK;
    if (total_chunks < n_tensors)
        return xmh::fail(XMH_EINVAL, "xmh_bertadam_step: %lld chunks for %lld tensors (every tensor has at least one)",
                         (long long)total_chunks, (long long)n_tensors);
    if (total_chunks > INT32_MAX) return xmh::fail(XMH_ENOTSUP, "xmh_bertadam_step: %lld chunks, at most 2^31 - 1", (long long)total_chunks);
    if (!table || !chunk_map || !ws) return xmh::fail(XMH_EINVAL, "xmh_bertadam_step: null pointer");
    const size_t need = xmh_bertadam_ws_bytes(n_tensors, total_chunks);
    if (ws_bytes < need) return xmh::fail(XMH_EINVAL, "xmh_bertadam_step: workspace of %zu bytes < %zu (xmh_bertadam_ws_bytes)", ws_bytes, need);
    if (reinterpret_cast<uintptr_t>(ws) & 255u) return xmh::fail(XMH_EINVAL, "xmh_bertadam_step: workspace not 256-byte aligned");
    if ((reinterpret_cast<uintptr_t>(table) & 7u) || (reinterpret_cast<uintptr_t>(chunk_map) & 7u))
        return xmh::fail(XMH_EINVAL, "xmh_bertadam_step: table or chunk map not 8-byte aligned");
    hipStream_t st = xmh::as_stream(stream);
    double* partial = static_cast<double*>(ws);
    hipLaunchKernelGGL(k_bertadam_sumsq, dim3((unsigned)total_chunks), dim3(kThreads), 0, st, table, chunk_map, partial);
    hipLaunchKernelGGL(k_bertadam_update, dim3((unsigned)total_chunks), dim3(kThreads), 0, st, table, chunk_map, partial);
    XMH_LAUNCH_CHECK("xmh_bertadam_step");
    return XMH_OK;
}
