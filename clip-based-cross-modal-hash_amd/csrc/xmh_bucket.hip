// Multi-tensor pack / unpack for the gradient bucket of distributed training (xmh/ddp.py): any number of fp32 tensors
// to or from ONE flat buffer in one launch, so that one collective per step carries every gradient.
//
//   k_bucket<true>   pack:   flat[offset_i + j] = t_i[j] * scale   (a row without a tensor writes zeros); the block of a tensor's first
//                            chunk also stores the row's flag at flat[flag_at_i] (the bucket's flag tail)
//   k_bucket<false>  unpack: t_i[j] = flat[offset_i + j]           (a row without a tensor is skipped)
//
// The design is BertAdam's (xmh_optim.hip): a device-resident table of rows, a chunk map with one block per chunk of kChunk elements
// (xmh_bertadam_chunk_ref's layout), nothing that synchronises with the host or allocates.  The flat side of a chunk is always 16-byte
// aligned (flat is, offsets are multiples of 64 floats, chunk starts multiples of kChunk), so it moves as float4; the tensor side
// moves as float4 where its address is 16-byte aligned too and as four dwords per float4 otherwise (a slice of a larger tensor), the
// last numel % 4 elements as dwords.  Bound: 8 bytes per element, pure HBM stream; four float4 loads per lane are issued before the
// first store (64 B in flight per lane, 16 KB per block).
#include "xmh_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 16384;                    // elements per block: xmh_bertadam_chunk(), one map layout for both
constexpr int kUnroll = 4;                       // float4 rounds whose loads are issued before the first store

using Row = xmh_bucket_tensor;
using ChunkRef = xmh_bertadam_chunk_ref;

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ float4 scaled(float4 a, float s) {
    return make_float4(__fmul_rn(a.x, s), __fmul_rn(a.y, s), __fmul_rn(a.z, s), __fmul_rn(a.w, s));
}

template <bool kPack>
__global__ __launch_bounds__(kThreads) void k_bucket(const Row* __restrict__ table, const ChunkRef* __restrict__ map, float scale,
                                                     float* flat) {   // no __restrict__: a tensor may be its own range of flat
    const ChunkRef c = map[blockIdx.x];
    const Row t = table[c.tensor];
    if (kPack && c.start == 0 && threadIdx.x == 0 && t.flag_at >= 0) flat[t.flag_at] = t.flag;
    const int64_t left = t.numel - c.start;
    const int n = left < kChunk ? (int)left : kChunk;
    const int n4 = n >> 2;
    float* f = flat + t.offset + c.start;
    float4* f4 = reinterpret_cast<float4*>(f);
    if (t.t == nullptr) {
        if (!kPack) return;
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int i = threadIdx.x; i < n4; i += kThreads) f4[i] = zero;
        const int i = (n4 << 2) + threadIdx.x;
        if (i < n) f[i] = 0.0f;
        return;
    }
    float* x = t.t + c.start;
    if (aligned16(x)) {
        float4* x4 = reinterpret_cast<float4*>(x);
        for (int base = 0; base < n4; base += kUnroll * kThreads) {
            float4 r[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int i = base + u * kThreads + threadIdx.x;
                if (i < n4) r[u] = kPack ? x4[i] : f4[i];
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int i = base + u * kThreads + threadIdx.x;
                if (i < n4) {
                    if (kPack) f4[i] = scaled(r[u], scale);
                    else x4[i] = r[u];
                }
            }
        }
    } else {
        for (int base = 0; base < n4; base += kUnroll * kThreads) {
            float4 r[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int i = base + u * kThreads + threadIdx.x;
                if (i < n4) r[u] = kPack ? make_float4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]) : f4[i];
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int i = base + u * kThreads + threadIdx.x;
                if (i < n4) {
                    if (kPack) {
                        f4[i] = scaled(r[u], scale);
                    } else {
                        x[4 * i] = r[u].x;
                        x[4 * i + 1] = r[u].y;
                        x[4 * i + 2] = r[u].z;
                        x[4 * i + 3] = r[u].w;
                    }
                }
            }
        }
    }
    const int i = (n4 << 2) + threadIdx.x;       // at most 3 elements past the last whole float4
    if (i < n) {
        if (kPack) f[i] = __fmul_rn(x[i], scale);
        else x[i] = f[i];
    }
}

static_assert(sizeof(Row) == 40 && sizeof(ChunkRef) == 16, "table layouts are part of the ABI (xmh/ddp.py mirrors them)");
static_assert(kChunk % (4 * kThreads * kUnroll) == 0, "whole unrolled rounds per chunk");

int check_args(const char* who, const Row* table, int64_t n_tensors, const ChunkRef* chunk_map, int64_t total_chunks, const float* flat) {
    if (n_tensors < 0 || total_chunks < 0)
        return xmh::fail(XMH_EINVAL, "%s: negative count n_tensors=%lld total_chunks=%lld", who, (long long)n_tensors, (long long)total_chunks);
    if (n_tensors == 0) return XMH_OK;
    if (total_chunks < n_tensors)
        return xmh::fail(XMH_EINVAL, "%s: %lld chunks for %lld tensors (every tensor has at least one)", who, (long long)total_chunks,
                         (long long)n_tensors);
    if (total_chunks > INT32_MAX) return xmh::fail(XMH_ENOTSUP, "%s: %lld chunks, at most 2^31 - 1", who, (long long)total_chunks);
    if (!table || !chunk_map || !flat) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if ((reinterpret_cast<uintptr_t>(table) & 7u) || (reinterpret_cast<uintptr_t>(chunk_map) & 7u))
        return xmh::fail(XMH_EINVAL, "%s: table or chunk map not 8-byte aligned", who);
    if (reinterpret_cast<uintptr_t>(flat) & 15u) return xmh::fail(XMH_EINVAL, "%s: the flat buffer is not 16-byte aligned", who);
    return XMH_OK;
}

}  // namespace

extern "C" int xmh_bucket_pack(const xmh_bucket_tensor* table, int64_t n_tensors, const xmh_bertadam_chunk_ref* chunk_map,
                               int64_t total_chunks, float scale, float* flat, xmh_stream_t stream) {
    XMH_RANGE("xmh_bucket_pack");
    XMH_TRY(check_args("xmh_bucket_pack", table, n_tensors, chunk_map, total_chunks, flat));
    if (n_tensors == 0) return XMH_OK;
    hipLaunchKernelGGL(k_bucket<true>, dim3((unsigned)total_chunks), dim3(kThreads), 0, xmh::as_stream(stream), table, chunk_map, scale, flat);
    XMH_LAUNCH_CHECK("xmh_bucket_pack");
    return XMH_OK;
}

extern "C" int xmh_bucket_unpack(const xmh_bucket_tensor* table, int64_t n_tensors, const xmh_bertadam_chunk_ref* chunk_map,
                                 int64_t total_chunks, const float* flat, xmh_stream_t stream) {
    XMH_RANGE("xmh_bucket_unpack");
    XMH_TRY(check_args("xmh_bucket_unpack", table, n_tensors, chunk_map, total_chunks, flat));
    if (n_tensors == 0) return XMH_OK;
    hipLaunchKernelGGL(k_bucket<false>, dim3((unsigned)total_chunks), dim3(kThreads), 0, xmh::as_stream(stream), table, chunk_map, 1.0f,
                       const_cast<float*>(flat));
    XMH_LAUNCH_CHECK("xmh_bucket_unpack");
    return XMH_OK;
}
