// The VALU kernels of the ranking scan and the small kernels around the two passes: k_scan_hist_s / k_scan_ap_s (the slotted scan, described at
// the top of xmh_scan.hip), the bucket tables between the passes (k_scan_below, k_scan_dpre), the lane-order probes, the offsets of the sharded
// evaluations (k_shard_*), the reductions behind pass 2 (k_ap_reduce*, k_map_finalize).  Device code only; xmh_scan.hip (the host side) includes it.
#pragma once
#include "xmh_scan_mfma.h"

namespace {
template <int W, int LW, bool TERN>
struct QueryRegs {
    uint32_t b[W];
    uint32_t z[TERN ? W : 1];
    uint32_t l[LW];
    __device__ __forceinline__ void load(const ScanArgs& a, int q) {
        const bool ok = q < a.Q;
#pragma unroll
        for (int w = 0; w < W; ++w) b[w] = ok ? a.qbits[(int64_t)q * W + w] : 0u;
        if (TERN) {
#pragma unroll
            for (int w = 0; w < W; ++w) z[w] = ok ? a.qzero[(int64_t)q * W + w] : 0xffffffffu;
        }
#pragma unroll
        for (int w = 0; w < LW; ++w) l[w] = ok ? a.qlab[(int64_t)q * LW + w] : 0u;
    }
};

// one gallery record as plain words (uniform across the wave)
template <int W, int LW, bool TERN>
struct Rec {
    uint32_t b[W];
    uint32_t z[TERN ? W : 1];
    uint32_t l[LW];
};

// distance bucket d and relevance (as 0/1 in `hit01`) of (this lane's query, record r); all operands in VGPRs
template <int W, int LW, bool TERN>
__device__ __forceinline__ void rec_eval01(const QueryRegs<W, LW, TERN>& qr, const Rec<W, LW, TERN>& r, int K, int& d, uint32_t& hit01) {
    if (!TERN) {
        int acc = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) acc += __popc(qr.b[w] ^ r.b[w]);
        d = acc;
    } else {
        int live_n = 0, diff_n = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint32_t live = ~(qr.z[w] | r.z[w]);
            live_n += __popc(live);
            diff_n += __popc((qr.b[w] ^ r.b[w]) & live);
        }
        d = K - live_n + 2 * diff_n;                           // 2 * (0.5 * (K - q.r)), in [0, 2K]
    }
    uint32_t hit = qr.l[0] & r.l[0];
#pragma unroll
    for (int w = 1; w < LW; ++w) asm("v_and_or_b32 %0, %1, %2, %0" : "+v"(hit) : "v"(qr.l[w]), "v"(r.l[w]));
    asm("v_min_u32 %0, %1, 1" : "=v"(hit01) : "v"(hit));
}

// ---------------------------------------------------------------------------------------------------
// bucket tables between the passes (tiny, latency-bound -> spread over many waves, loads independent)
//   below[c][d][q] = (#all, #relevant) items of bucket d in chunks < c of this shard
//   tot[d][q]      = (#all, #relevant) items of bucket d in this shard
// `below` has two forms.  The 64-bit one is a uint2 {all, relevant} per cell.  The PACKED one (k_scan_below's `packed`; the host's rule is
// tables_packed in xmh_scan.hip) is one uint32 per cell, all << 16 | relevant -- the word pass 1 counts a chunk in, kept through the prefix --
// at the same index of the same region, of which it fills the first half: half the bytes k_scan_below writes, half of what every block of
// k_scan_ap_c reads before its first pair.  A prefix is bounded by the shard total of its (bucket, query).  A thread whose total does not
// fit 16 bits raises the gate word kGateWide; its cells may then hold anything, and every block of k_scan_ap_c sums its start values from
// chunk_hist itself, which nothing overwrites between the passes: correct, slower, no launch more.  Only k_scan_ap_c reads this form.
// ---------------------------------------------------------------------------------------------------
// rel_scale: the format of the pass-1 counter words (chunk_counts, xmh_scan_mfma.h)
// words of the gate block of the workspace (cleared at the start of every xmh_hamming_hist): 0 = nrel_max, 1 = finalize ticket,
// 2 = gallery items over all shards, 3 = "a distance wrapped in the one-byte pair cache of 65..128-bit codes", 4 = "a bucket total does
// not fit the 16 bits of the packed `below` table"
constexpr int kGateWrapped = 3;
constexpr int kGateWide = 4;
// The block that finishes a 64-query tile LAST (ticket per tile, zeroed ahead of the launch) also writes what the unsharded pass 2
// needs from the totals -- dpre[d][q] = exclusive prefix of tot over d, nrel[q], the nrel_max gate word -- which used to be a
// launch of its own between the passes (k_scan_dpre: 9 us + a launch gap; kept for the sharded call and the histogram export).
// tickets == nullptr: none of that -- `below` and the totals only, no ticket, no wait for the stores, and the kernel is a stream of two
// load groups and their stores.  Round 11: the unsharded step on the packed table runs it so (no histogram export), and every block of
// k_scan_ap_c prefixes the 65 x 16 totals of its query tile over the buckets itself, in registers (xmh_scan_mfma.h); the host remembers that
// the workspace then holds no dpre / nrel (xmh_scan.hip, the rule for the packed table) and runs this kernel in full for a pass 2 that needs them.
__global__ __launch_bounds__(256) void k_scan_below(const uint32_t* __restrict__ chunk_hist, int qpad, int nb, int nchunk, uint32_t rel_scale,
                                                    uint2* __restrict__ below, uint2* __restrict__ tot, uint32_t* __restrict__ tickets, int Q,
                                                    uint2* __restrict__ dpre, uint32_t* __restrict__ nrel_ws, uint32_t* __restrict__ nrel_max,
                                                    uint32_t* __restrict__ hist_all, uint32_t* __restrict__ hist_rel, bool packed,
                                                    uint32_t* __restrict__ wide) {
    __shared__ uint2 part[4][64];
    __shared__ int last;
    const int lane = threadIdx.x & 63, wq = threadIdx.x >> 6;
    const int d = blockIdx.y * 4 + wq;
    const int q = blockIdx.x * 64 + lane;
    const bool hi16 = rel_scale == kRelHi16;
    if (d < nb && packed) {
        // the packed table (see the header): a thread loads the words of 16 chunks before the first store of the group -- two round trips at
        // the headline's 24 chunks, where the 64-bit form below makes six dependent ones -- and a cell is one 4-byte store.  (Groups of 32, all of
        // a thread's chunks in one trip, took 173 VGPRs for the 64 addresses: two waves per SIMD, and the kernel was 2 us slower than the 64-bit
        // form.)  Source and destination walk by one chunk's stride, so that an address is dead once its instruction has issued.
        const int64_t cell = (int64_t)d * qpad + q, step = (int64_t)nb * qpad;
        const uint32_t* __restrict__ src = chunk_hist + cell;
        uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(below) + cell;
        uint32_t ra = 0, rr = 0;
        for (int c0 = 0; c0 < nchunk; c0 += 16) {
            uint32_t h[16];
#pragma unroll
            for (int j = 0; j < 16; ++j, src += step) h[j] = c0 + j < nchunk ? *src : 0u;
#pragma unroll
            for (int j = 0; j < 16; ++j, dst += step) {
                if (c0 + j < nchunk) {
                    *dst = (ra << 16) | rr;
                    const uint2 n = chunk_counts(h[j], rel_scale);
                    ra += n.x;
                    rr += n.y;
                }
            }
        }
        // relevant <= all: the total of all items decides for both halves.  (The columns of the padding queries count for nothing: pass 1 may
        // have counted the padding items of the last batch in them, and no sum of theirs is read.)
        if (ra > 0xffffu && q < Q) *wide = 1u;
        // no tickets: no block of this launch reads the totals (their readers are a kernel boundary away), a plain store will do
        if (!tickets) tot[(int64_t)d * qpad + q] = make_uint2(ra, rr);
        else
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(tot + (int64_t)d * qpad + q), (unsigned long long)ra | ((unsigned long long)rr << 32),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (d < nb) {
        uint32_t ra = 0, rr = 0;
        int c = 0;
        for (; c + 4 <= nchunk; c += 4) {
            uint32_t h[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = chunk_hist[((int64_t)(c + j) * nb + d) * qpad + q];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                below[((int64_t)(c + j) * nb + d) * qpad + q] = make_uint2(ra, rr);
                const uint32_t rel = hi16 ? h[j] & 0xffffu : (rel_scale ? h[j] / rel_scale : h[j] >> 16);
                ra += hi16 ? h[j] >> 16 : (rel_scale ? h[j] - rel * rel_scale : h[j] & 0xffffu);
                rr += rel;
            }
        }
        for (; c < nchunk; ++c) {
            const uint32_t h = chunk_hist[((int64_t)c * nb + d) * qpad + q];
            below[((int64_t)c * nb + d) * qpad + q] = make_uint2(ra, rr);
            const uint32_t rel = hi16 ? h & 0xffffu : (rel_scale ? h / rel_scale : h >> 16);
            ra += hi16 ? h >> 16 : (rel_scale ? h - rel * rel_scale : h & 0xffffu);
            rr += rel;
        }
        // agent-scope store (sc1: written through this XCD's L2): the totals are the one thing another block of this launch reads
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(tot + (int64_t)d * qpad + q), (unsigned long long)ra | ((unsigned long long)rr << 32),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!tickets) return;
    // hand-off without fences (an agent-scope release writes back the whole L2 of the XCD -- with 84 MB of `below` in flight that
    // made this kernel 22 -> 152 us): the totals go out as agent-scope stores, every wave waits for their acknowledgement
    // (vmcnt(0)) before the barrier, then one thread takes the tile's ticket; the block that draws the last ticket reads the
    // totals with agent-scope loads, which do not hit in a stale L1 / L2 line.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = __hip_atomic_fetch_add(tickets + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = t == gridDim.y - 1;
    }
    __syncthreads();
    if (!last) return;
    auto tot_at = [&](int dd) {
        const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(tot + (int64_t)dd * qpad + q), __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
        return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
    };
    // 64 queries, the bucket axis split over the 4 waves: quarter sums, prefixed through LDS, then the exclusive prefixes
    const int nbq = (nb + 3) / 4;
    const int d0 = wq * nbq, d1 = (d0 + nbq < nb) ? d0 + nbq : nb;
    uint32_t sa = 0, sr = 0;
    for (int dd = d0; dd < d1; dd += 8) {
        uint2 t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = dd + j < d1 ? tot_at(dd + j) : make_uint2(0u, 0u);
#pragma unroll
        for (int j = 0; j < 8; ++j) { sa += t[j].x; sr += t[j].y; }
    }
    part[wq][lane] = make_uint2(sa, sr);
    __syncthreads();
    uint32_t ra = 0, rr = 0, tr = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint2 pw = part[w][lane];
        if (w < wq) { ra += pw.x; rr += pw.y; }
        tr += pw.y;
    }
    for (int dd = d0; dd < d1; dd += 8) {
        uint2 t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = dd + j < d1 ? tot_at(dd + j) : make_uint2(0u, 0u);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (dd + j < d1) {
                dpre[(int64_t)(dd + j) * qpad + q] = make_uint2(ra, rr);
                if (hist_all && q < Q) hist_all[(int64_t)q * nb + dd + j] = t[j].x;      // the shard totals a sharded evaluation gathers
                if (hist_rel && q < Q) hist_rel[(int64_t)q * nb + dd + j] = t[j].y;
                ra += t[j].x;
                rr += t[j].y;
            }
        }
    }
    if (wq == 0) {
        nrel_ws[q] = tr;
        if (q < Q) atomicMax(nrel_max, tr);
    }
}

//   dpre[d][q] = rank offset of bucket d from outside this shard's bucket d: all lower buckets
//                (locally: exclusive prefix of tot; sharded: the caller's base_all/base_rel)
//   nrel_ws[q] = relevant items of query q over all shards (pass 2 caps at min(nrel, k) itself), cap_out[q] = min(nrel, k)
__global__ __launch_bounds__(256) void k_scan_dpre(const uint2* __restrict__ tot, int Q, int qpad, int nb,
                                                   const uint32_t* __restrict__ base_all,
                                                   const uint32_t* __restrict__ base_rel,
                                                   const uint32_t* __restrict__ nrel_total, int64_t kcap,
                                                   uint2* __restrict__ dpre, uint32_t* __restrict__ cap_ws,
                                                   int32_t* __restrict__ cap_out, uint32_t* __restrict__ hist_all,
                                                   uint32_t* __restrict__ hist_rel, uint32_t* __restrict__ nrel_max,
                                                   uint32_t* __restrict__ rank_max = nullptr) {
    // rank_max (explicit-offsets form): the largest rank this shard can hand out, max over (q, d) of base_all + tot -- the word the
    // float-bit pass 2 is gated on, as the gallery size is for the totals-table form.
    // 64 queries per block, the bucket axis split over the 4 waves: each wave sums its quarter, the quarter sums are
    // prefixed through LDS, then each wave walks its quarter again (L2 hits) writing the exclusive prefixes.  One wave per
    // 64 queries walking all buckets was a 13 us latency chain of dependent-free but serialised load groups.
    __shared__ uint2 part[4][64];
    const int lane = threadIdx.x & 63, wq = threadIdx.x >> 6;
    const int q = blockIdx.x * 64 + lane;
    const bool qok = q < Q;
    const int nbq = (nb + 3) / 4;
    const int d0 = wq * nbq, d1 = (d0 + nbq < nb) ? d0 + nbq : nb;
    uint32_t sa = 0, sr = 0;
    for (int d = d0; d < d1; d += 8) {
        uint2 t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = d + j < d1 ? tot[(int64_t)(d + j) * qpad + q] : make_uint2(0u, 0u);
#pragma unroll
        for (int j = 0; j < 8; ++j) { sa += t[j].x; sr += t[j].y; }
    }
    part[wq][lane] = make_uint2(sa, sr);
    __syncthreads();
    uint32_t ra = 0, rr = 0, ta = 0, tr = 0, rmax = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint2 p = part[w][lane];
        if (w < wq) { ra += p.x; rr += p.y; }
        ta += p.x; tr += p.y;
    }
    for (int d = d0; d < d1; d += 8) {
        uint2 t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = d + j < d1 ? tot[(int64_t)(d + j) * qpad + q] : make_uint2(0u, 0u);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (d + j < d1) {
                uint2 o = make_uint2(ra, rr);
                if (base_all && qok) {
                    o = make_uint2(base_all[(int64_t)q * nb + d + j], base_rel[(int64_t)q * nb + d + j]);
                    rmax = max(rmax, o.x + t[j].x);
                }
                if (dpre) dpre[(int64_t)(d + j) * qpad + q] = o;
                if (qok && hist_all) hist_all[(int64_t)q * nb + d + j] = t[j].x;
                if (qok && hist_rel) hist_rel[(int64_t)q * nb + d + j] = t[j].y;
                ra += t[j].x;
                rr += t[j].y;
            }
        }
    }
    if (cap_ws && wq == 0) {
        const uint32_t nrel = nrel_total ? (qok ? nrel_total[q] : 0u) : tr;
        const uint32_t cap = (kcap > 0 && (uint64_t)kcap < (uint64_t)nrel) ? (uint32_t)kcap : nrel;
        cap_ws[q] = nrel;
        if (qok && cap_out) cap_out[q] = (int32_t)cap;
        if (qok && nrel_max) atomicMax(nrel_max, nrel);
    }
    if (rank_max) {
        for (int o = 32; o; o >>= 1) rmax = max(rmax, (uint32_t)__shfl_xor((int)rmax, o));
        if (lane == 0 && rmax) atomicMax(rank_max, rmax);
    }
    (void)ta;
}

// ---------------------------------------------------------------------------------------------------
// the 64-record gallery batch: one record per lane in registers, staged record-major ([item][RS]) in the LDS ring
// ---------------------------------------------------------------------------------------------------
template <int W, int LW, bool TERN>
struct AosBatch {
    static constexpr int RW = W * (TERN ? 2 : 1) + LW;
    static constexpr int RS = (RW + 3) / 4 * 4;
    using R = Rec<W, LW, TERN>;
    // Long records (W >= 16 words, 64..256 B): a lane loading "its" record would touch one cache line per lane and
    // instruction (64 lines per load, 8x traffic once the L1 thrashes -- measured 12x slower).  The 64-record batch is
    // one contiguous 64*W-dword range instead: piece j of lane l is dwords [j*256 + 4l, +4) of it, which belongs to record
    // (j*256 + 4l) / W; publish() scatters the pieces to the padded record rows of the ring.
    static constexpr bool COAL = W >= 16 && !TERN;
    uint32_t w[RS];
    // NW > 1: the NW waves of a block share the ring; wave `wave` brings pieces wave, wave + NW, ... and wave 0 the labels
    template <int NW = 1>
    __device__ __forceinline__ void load(const ScanArgs& a, int64_t base, int64_t hi, int lane, int wave = 0) {
        const int64_t i = base + lane;
        const bool ok = i < hi;
        if (COAL) {
#pragma unroll
            for (int jj = 0; jj < W / 4 / NW; ++jj) {
                const int o = (jj * NW + wave) * 256 + lane * 4;
                const bool okj = base + o / W < hi;
                const uint4 v = okj ? *reinterpret_cast<const uint4*>(a.rbits + base * W + o) : make_uint4(0u, 0u, 0u, 0u);
                w[4 * jj] = v.x; w[4 * jj + 1] = v.y; w[4 * jj + 2] = v.z; w[4 * jj + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int x = 0; x < W; ++x) w[x] = ok ? a.rbits[i * W + x] : 0u;
        }
        if (TERN) {
#pragma unroll
            for (int x = 0; x < W; ++x) w[W + x] = ok ? a.rzero[i * W + x] : 0xffffffffu;
        }
        if (NW == 1 || wave == 0) {
#pragma unroll
            for (int x = 0; x < LW; ++x) w[W * (TERN ? 2 : 1) + x] = ok ? a.rlab[i * LW + x] : 0u;
        }
#pragma unroll
        for (int x = RW; x < RS; ++x) w[x] = 0u;
    }
    template <int NW = 1>
    __device__ __forceinline__ void publish(uint32_t* ring, int lane, int wave = 0) const {
        if (COAL) {
#pragma unroll
            for (int jj = 0; jj < W / 4 / NW; ++jj) {
                const int o = (jj * NW + wave) * 256 + lane * 4;
                *reinterpret_cast<uint4*>(ring + (o / W) * RS + (o % W)) = make_uint4(w[4 * jj], w[4 * jj + 1], w[4 * jj + 2], w[4 * jj + 3]);
            }
            if (NW == 1 || wave == 0)                                // labels + padding (W % 4 == 0)
                *reinterpret_cast<uint4*>(ring + lane * RS + W) = make_uint4(w[W], w[W + 1], w[W + 2], w[W + 3]);
            return;
        }
#pragma unroll
        for (int x = 0; x < RS; x += 4) *reinterpret_cast<uint4*>(ring + lane * RS + x) = make_uint4(w[x], w[x + 1], w[x + 2], w[x + 3]);
    }
    // `mine` = ring + slot * RS (per lane); item = step * S + slot -> constant offset step * S * RS from it
    static __device__ __forceinline__ void get(R& r, const uint32_t* mine, int off_dwords) {
        uint32_t t[RS];
#pragma unroll
        for (int x = 0; x < RS; x += 4) {
            if (x + 4 <= RW || RW - x > 2) {
                const uint4 v = *reinterpret_cast<const uint4*>(mine + off_dwords + x);
                t[x] = v.x; t[x + 1] = v.y; t[x + 2] = v.z; t[x + 3] = v.w;
            } else if (RW - x == 2) {
                const uint2 v = *reinterpret_cast<const uint2*>(mine + off_dwords + x);
                t[x] = v.x; t[x + 1] = v.y; t[x + 2] = 0u; t[x + 3] = 0u;
            } else {
                t[x] = mine[off_dwords + x]; t[x + 1] = 0u; t[x + 2] = 0u; t[x + 3] = 0u;
            }
        }
#pragma unroll
        for (int x = 0; x < W; ++x) r.b[x] = t[x];
        if (TERN) {
#pragma unroll
            for (int x = 0; x < W; ++x) r.z[x] = t[W + x];
        }
#pragma unroll
        for (int x = 0; x < LW; ++x) r.l[x] = t[W * (TERN ? 2 : 1) + x];
    }
};

template <int S> struct SlotGeom {
    static constexpr int QW = 64 / S;
    static constexpr int LOG_QW = QW == 64 ? 6 : (QW == 32 ? 5 : (QW == 16 ? 4 : (QW == 8 ? 3 : (QW == 4 ? 2 : (QW == 2 ? 1 : 0)))));
    static constexpr int G = QW >= 16 ? 8 : (QW < 4 ? QW : 4);   // steps per pipelined group (at K = 64: 8 beats 4 by 4 %, 2 loses 4 %)
    static constexpr int NG = QW / G;                  // groups per 64-item batch (QW steps)
};

// NW = waves per block.  1 except for S = 64 (one query per wave): there every wave would stream its whole chunk for a
// single query -- the gallery re-read Q times from L2 / Infinity Cache (measured 6.5 TB/s, 10x the VALU time) -- so NW = 8
// waves (8 queries) share ONE staged batch: each wave loads an eighth of it, two barriers per batch.
// CACHE (S = 4, one wave per block, codes of at most 127 bits): pass 1 also writes one byte per pair, distance << 1 | relevant,
// so that pass 2 does not evaluate the pair again (XOR / popcount / label AND: 8 of its 15 VALU instructions) nor stage the
// gallery: lane l of the wave of (chunk, query tile) owns 16 consecutive bytes = its 16 steps of a 64-item batch, a wave
// stores 1 KB per batch.  Q x R bytes in all (593 MB at the COCO shape), streamed once each way while both passes are VALU-bound.
template <int W, int LW, bool TERN, int S, int NW, bool CACHE>
__global__ __launch_bounds__(64 * NW) void k_scan_hist_s(ScanArgs a, uint32_t* __restrict__ chunk_hist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];   // NW x [nb][QW] counters, then the ring
    using SG = SlotGeom<S>;
    constexpr int QW = SG::QW, G = SG::G, NG = SG::NG;
    int chunk_id, qtile;
    if (!map_block(a, chunk_id, qtile)) return;                      // a.nqt counts tiles of QW * NW queries here
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ql = lane & (QW - 1), slot = lane >> SG::LOG_QW;
    const int q0 = (qtile * NW + wave) * QW;                         // first query of this wave
    const int q = q0 + ql;
    const int ncell = a.nb * QW, cstride = (ncell + 3) & ~3;
    uint32_t* cnt = lds + wave * cstride;
    for (int e = lane; e < ncell; e += 64) cnt[e] = 0u;
    QueryRegs<W, LW, TERN> qr;
    qr.load(a, q);
    using R = Rec<W, LW, TERN>;
    using LB = AosBatch<W, LW, TERN>;
    uint32_t* ring = lds + NW * cstride;
    const uint32_t* mine = ring + slot * LB::RS;
    const int64_t lo = (int64_t)chunk_id * a.chunk;
    const int64_t hi = (lo + a.chunk < a.R) ? lo + a.chunk : a.R;

    // cache entry: EB bits = distance << 1 | relevant; a lane's QW steps of a batch fill exactly 16 bytes (8-bit entries at
    // 16 steps: codes up to 64 bits; 16-bit entries at 8 steps: 65..256 bits), each group of G steps two dwords
    constexpr int EB = 128 / QW, EPW = 32 / EB;
    static_assert(!CACHE || (NW == 1 && (S == 4 || S == 8) && NG == 2 && G == 2 * EPW), "pair cache geometry: 16 bytes per lane and batch, two groups");
    uint32_t cw0 = 0u, cw1 = 0u, cw2 = 0u, cw3 = 0u;                 // CACHE: this lane's 16 bytes of the current batch
    auto count = [&](const R (&g)[G], uint32_t& wa, uint32_t& wb) {
        int d[G];
        uint32_t hit[G];
#pragma unroll
        for (int u = 0; u < G; ++u) rec_eval01<W, LW, TERN>(qr, g[u], a.K, d[u], hit[u]);
#pragma unroll
        for (int u = 0; u < G; ++u) atomicAdd(&cnt[d[u] * QW + ql], (hit[u] << 16) + 1u);
        if (CACHE) {                                                 // append an entry per step: w = entry << (32 - EB) | w >> EB
            // (counters indexed by that byte, so that the add is a constant 1, were tried: 3x the LDS per wave, pass 1 0.27 -> 0.31 ms)
#pragma unroll
            for (int u = 0; u < G / 2; ++u) wa = __builtin_amdgcn_alignbyte(((uint32_t)d[u] << 1) | hit[u], wa, EB / 8);
#pragma unroll
            for (int u = G / 2; u < G; ++u) wb = __builtin_amdgcn_alignbyte(((uint32_t)d[u] << 1) | hit[u], wb, EB / 8);
        }
    };
    const int nbatch = (a.chunk + 63) >> 6;
    uint4* crow = CACHE ? a.pair_cache + ((int64_t)chunk_id * a.nqt + qtile) * nbatch * 64 + lane : nullptr;
    auto fetch = [&](R (&g)[G], int group) {
#pragma unroll
        for (int u = 0; u < G; ++u) LB::get(g[u], mine, (group * G + u) * S * LB::RS);
    };
    LB cur, nxt;                                                     // the next batch's global loads fly during this one
    cur.template load<NW>(a, lo, hi, lane, wave);
    for (int64_t base = lo; base < hi; base += 64) {
        if (NW > 1) __syncthreads();                                 // every wave is done reading the previous batch
        cur.template publish<NW>(ring, lane, wave);
        nxt.template load<NW>(a, base + 64, hi, lane, wave);
        if (NW > 1) __syncthreads();                                 // the batch is complete in the ring
        const int cntb = (hi - base < 64) ? (int)(hi - base) : 64;
        if (cntb == 64) {
            R ga[G], gb[G];
            fetch(ga, 0);
#pragma unroll
            for (int g = 0; g < NG; g += 2) {
                if (g + 1 < NG) fetch(gb, g + 1);
                count(ga, cw0, cw1);
                if (g + 2 < NG) fetch(ga, g + 2);
                if (g + 1 < NG) count(gb, cw2, cw3);
            }
        } else if (!CACHE) {
            for (int t = 0; t * S < cntb; ++t) {
                R r;
                LB::get(r, mine, t * S * LB::RS);
                int d;
                uint32_t hit;
                rec_eval01<W, LW, TERN>(qr, r, a.K, d, hit);
                if (t * S + slot < cntb) atomicAdd(&cnt[d * QW + ql], (hit << 16) + 1u);
            }
        } else {
#pragma unroll
            for (int t = 0; t < QW; ++t) {                           // unrolled: the bytes land in fixed registers
                uint32_t b = 0u;
                if (t * S < cntb) {
                    R r;
                    LB::get(r, mine, t * S * LB::RS);
                    int d;
                    uint32_t hit;
                    rec_eval01<W, LW, TERN>(qr, r, a.K, d, hit);
                    b = ((uint32_t)d << 1) | hit;
                    if (t * S + slot < cntb) atomicAdd(&cnt[d * QW + ql], (hit << 16) + 1u);
                }
                uint32_t& w = t < EPW ? cw0 : (t < 2 * EPW ? cw1 : (t < 3 * EPW ? cw2 : cw3));
                w = __builtin_amdgcn_alignbyte(b, w, EB / 8);
            }
        }
        if (CACHE && EB == 8) {                                      // streamed once: non-temporal, so that the 593 MB do not sit dirty in
            uint4* dst = crow + ((base - lo) >> 6) * 64;                 // L2 / Infinity Cache while the small table kernels run
            __builtin_nontemporal_store(cw0, &dst->x);
            __builtin_nontemporal_store(cw1, &dst->y);
            __builtin_nontemporal_store(cw2, &dst->z);
            __builtin_nontemporal_store(cw3, &dst->w);
        }
        if (CACHE && EB == 16) {                                     // two-byte class entries go out 12 bits each (xmh_common.h): the four words of
            // 16-bit pairs become three.  p = E_even | E_odd << 16 with both below 4096: bfi(0xfff, p, p >> 4) = E_even | E_odd << 12
            const uint32_t a0 = (cw0 & 0xfffu) | ((cw0 >> 4) & ~0xfffu), a1 = (cw1 & 0xfffu) | ((cw1 >> 4) & ~0xfffu);
            const uint32_t a2 = (cw2 & 0xfffu) | ((cw2 >> 4) & ~0xfffu), a3 = (cw3 & 0xfffu) | ((cw3 >> 4) & ~0xfffu);
            uint32_t* dst = reinterpret_cast<uint32_t*>(a.pair_cache) +
                            ((((int64_t)chunk_id * a.nqt + qtile) * nbatch + ((base - lo) >> 6)) * 64 + lane) * xmh::kCache12Dwords;
            __builtin_nontemporal_store(a0 | (a1 << 24), dst);
            __builtin_nontemporal_store((a1 >> 8) | (a2 << 16), dst + 1);
            __builtin_nontemporal_store((a2 >> 16) | (a3 << 8), dst + 2);
        }
        cur = nxt;
    }
    uint32_t* __restrict__ out = chunk_hist + ((int64_t)chunk_id * a.nb) * a.qpad + q0;
    for (int e = lane; e < ncell; e += 64) out[(int64_t)(e >> SG::LOG_QW) * a.qpad + (e & (QW - 1))] = cnt[e];
}

// P32 = packed 32-bit counters {lo rank_bits: rank, hi: ordinal} when both fit one word (known on the device after
// pass 1: the launch is gated by *nrel_max, no host sync), else 64-bit {lo: rank, hi: ordinal}.  Counters are 1-based
// and start at the global base of (bucket, chunk).  MASKED: see the header (lane-order fallback).
// CACHE: the pairs come from the byte cache of pass 1 (see k_scan_hist_s) instead of the gallery.
// items_total (sharded calls that also launch k_scan_ap_c): that kernel takes the call when the gallery over all shards is small enough for it
// run_if (65..128-bit codes with one-byte cache entries, k_scan_hist_r2w): this launch is the stand-in for k_scan_ap_c and runs
// only when pass 1 raised the word (a distance of 128 wrapped in the cache) -- or when items_total says the gallery is too large for it
template <int W, int LW, bool TERN, bool CAPPED, int S, bool P32, bool MASKED, int NW, bool CACHE>
__global__ __launch_bounds__(64 * NW) void k_scan_ap_s(ScanArgs a, const uint2* __restrict__ below, const uint2* __restrict__ dpre,
                                                  const uint32_t* __restrict__ cap_ws, float* __restrict__ ap_part,
                                                  const uint32_t* __restrict__ nrel_max, int rank_bits, uint32_t kcap,
                                                  const uint32_t* __restrict__ items_total, const uint32_t* __restrict__ run_if = nullptr) {
    using CT = typename std::conditional<P32, uint32_t, unsigned long long>::type;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    using SG = SlotGeom<S>;
    constexpr int QW = SG::QW, G = SG::G, NG = SG::NG;
    int chunk_id, qtile;
    if (!map_block(a, chunk_id, qtile)) return;
    {
        const bool fits32 = rank_bits > 0 && (uint64_t)(*nrel_max) + 2 < (1ull << (32 - rank_bits));
        if (P32 != fits32) return;                                   // the other variant takes this call
    }
    if (run_if) {
        const bool too_large = items_total && (int64_t)*items_total > kFloatBitsMaxItems;
        if (!too_large && *run_if == 0u) return;                     // k_scan_ap_c takes this call
    } else if (items_total && (int64_t)*items_total <= kFloatBitsMaxItems) return;      // k_scan_ap_c takes this call
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;    // NW waves share the ring, see k_scan_hist_s
    const int ql = lane & (QW - 1), slot = lane >> SG::LOG_QW;
    const int q0 = (qtile * NW + wave) * QW;
    const int q = q0 + ql;
    const int ncell = a.nb * QW;
    const int cstride = ((ncell * (int)(sizeof(CT) / 4) + 3) & ~3);  // dwords of one wave's counters [nb][QW]
    CT* cnt = reinterpret_cast<CT*>(lds + wave * cstride);
    auto pack = [&](uint2 x, uint2 y) -> CT {
        if (P32) return (CT)((x.x + y.x + 1u) | ((x.y + y.y + 1u) << rank_bits));
        return (CT)((unsigned long long)(x.x + y.x + 1u) | ((unsigned long long)(x.y + y.y + 1u) << 32));
    };
    {
        const uint2* __restrict__ pb = below + ((int64_t)chunk_id * a.nb) * a.qpad + q0;
        const uint2* __restrict__ pd = dpre + q0;
        int e = lane;
        for (; e + 7 * 64 < ncell; e += 8 * 64) {
            uint2 x[8], y[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int ee = e + j * 64;
                const int64_t at = (int64_t)(ee >> SG::LOG_QW) * a.qpad + (ee & (QW - 1));
                x[j] = pb[at];
                y[j] = pd[at];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) cnt[e + j * 64] = pack(x[j], y[j]);
        }
        for (; e < ncell; e += 64) {
            const int64_t at = (int64_t)(e >> SG::LOG_QW) * a.qpad + (e & (QW - 1));
            cnt[e] = pack(pb[at], pd[at]);
        }
    }
    const uint32_t cap = CAPPED ? min(cap_ws[q], kcap) : 0u;      // cap_ws[q] = relevant items of query q
    const uint32_t rmask = P32 ? (1u << rank_bits) - 1u : 0xffffffffu;

    QueryRegs<W, LW, TERN> qr;
    qr.load(a, q);
    using R = Rec<W, LW, TERN>;
    using LB = AosBatch<W, LW, TERN>;
    uint32_t* ring = lds + NW * cstride;
    const uint32_t* mine = ring + slot * LB::RS;
    const int64_t lo = (int64_t)chunk_id * a.chunk;
    const int64_t hi = (lo + a.chunk < a.R) ? lo + a.chunk : a.R;
    float acc = 0.0f;

    auto credit = [&](CT old, uint32_t hit) {
        uint32_t rank, ord;
        if (P32) { rank = (uint32_t)old & rmask; ord = (uint32_t)old >> rank_bits; }
        else { rank = (uint32_t)old; ord = (uint32_t)((unsigned long long)old >> 32); }
        if (CAPPED) hit = ord <= cap ? hit : 0u;
        const float of = (float)__umul24(ord, hit);
        acc = fmaf(of, __builtin_amdgcn_rcpf((float)rank), acc);
    };
    auto inc = [&](uint32_t hit) -> CT {
        if (P32) return (CT)((hit << rank_bits) + 1u);
        return (CT)(1ull | ((unsigned long long)hit << 32));
    };
    CT old[G];
    uint32_t hitp[G];
    auto eval_issue = [&](const R (&g)[G], bool have_prev) {
        int d[G];
        uint32_t hit[G];
#pragma unroll
        for (int u = 0; u < G; ++u) rec_eval01<W, LW, TERN>(qr, g[u], a.K, d[u], hit[u]);
        if (have_prev) {
#pragma unroll
            for (int u = 0; u < G; ++u) credit(old[u], hitp[u]);
        }
#pragma unroll
        for (int u = 0; u < G; ++u) {
            hitp[u] = hit[u];
            CT* cell = &cnt[d[u] * QW + ql];
            const CT v = inc(hit[u]);
            if (!MASKED) {
                old[u] = atomicAdd(cell, v);                          // same-address lanes resolve in lane = item order
            } else {
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    if (slot == s) old[u] = atomicAdd(cell, v);      // slot order = index order
                }
            }
        }
    };
    auto drain = [&]() {
#pragma unroll
        for (int u = 0; u < G; ++u) credit(old[u], hitp[u]);
    };
    auto fetch = [&](R (&g)[G], int group) {
#pragma unroll
        for (int u = 0; u < G; ++u) LB::get(g[u], mine, (group * G + u) * S * LB::RS);
    };

    if constexpr (CACHE) {
        constexpr int EB = 128 / QW, EPW = 32 / EB;                   // entry bits, entries per word (see k_scan_hist_s)
        static_assert(NW == 1 && (S == 4 || S == 8) && NG == 2 && G == 2 * EPW && !MASKED, "pair cache geometry");
        // one group of 8 steps from two cache words; the returned counters are credited while the next group's adds fly
        // entry k (a constant after unrolling) of a lane's batch record r: 8- and 16-bit class entries; the latter are stored 12 bits each in
        // three dwords (xmh_common.h), sx / sy = the two entries that straddle a dword, shifted down
        auto entry = [&](const uint4& r, uint32_t sx, uint32_t sy, int k, uint32_t& d, uint32_t& hit) {
            if constexpr (EB == 8) {
                const uint32_t w = k < EPW ? r.x : (k < 2 * EPW ? r.y : (k < 3 * EPW ? r.z : r.w));
                d = __builtin_amdgcn_ubfe(w, EB * (k % EPW) + 1, EB - 1);
                hit = __builtin_amdgcn_ubfe(w, EB * (k % EPW), 1);
            } else {
                const uint32_t w = XMH_CACHE12_WORD(k, r.x, r.y, r.z, sx, sy);
                d = __builtin_amdgcn_ubfe(w, XMH_CACHE12_BIT(k) + 1, 11);
                hit = __builtin_amdgcn_ubfe(w, XMH_CACHE12_BIT(k), 1);
            }
        };
        auto issue = [&](const uint4& r, uint32_t sx, uint32_t sy, int first, bool have_prev) {
            if (have_prev) {
#pragma unroll
                for (int u = 0; u < G; ++u) credit(old[u], hitp[u]);
            }
#pragma unroll
            for (int u = 0; u < G; ++u) {
                uint32_t d, hit;
                entry(r, sx, sy, first + u, d, hit);
                hitp[u] = hit;
                old[u] = atomicAdd(&cnt[d * QW + ql], inc(hit));      // same-address lanes resolve in lane = item order
            }
        };
        const int nbatch = (a.chunk + 63) >> 6;
        const uint4* crow = a.pair_cache + ((int64_t)chunk_id * a.nqt + qtile) * nbatch * 64 + lane;
        const uint32_t* crow12 = reinterpret_cast<const uint32_t*>(a.pair_cache) + (((int64_t)chunk_id * a.nqt + qtile) * nbatch * 64 + lane) * xmh::kCache12Dwords;
        const int nfull = (int)((hi - lo) >> 6);                     // whole batches of this chunk
        // read once, 1 KB (12-bit records: 768 B) contiguous per wave instruction: non-temporal (see k_scan_ap_c).  EB == 16: the record's three
        // dwords come back as x, y, z and its two straddling entries, shifted down, as w (low half: entry 2, high half: entry 5)
        auto cache_words = [&](int64_t batch) -> uint4 {
            if constexpr (EB == 8) {
                typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
                const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(crow + batch * 64));
                return make_uint4(v.x, v.y, v.z, v.w);
            } else {
                typedef uint32_t u32x3_t __attribute__((ext_vector_type(3)));
                const u32x3_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x3_t*>(crow12 + batch * 64 * xmh::kCache12Dwords));
                return make_uint4(v.x, v.y, v.z, 0u);
            }
        };
        uint4 cw = cache_words(0);
        bool prev = false;
        for (int bi = 0; bi < nfull; ++bi) {
            const uint4 nw = cache_words(bi + 1 < nbatch ? bi + 1 : bi);               // unconditional: counted vmcnt, no predication
            const uint32_t sx = EB == 16 ? __builtin_amdgcn_alignbit(cw.y, cw.x, 24) : 0u, sy = EB == 16 ? __builtin_amdgcn_alignbit(cw.z, cw.y, 28) : 0u;
            issue(cw, sx, sy, 0, prev);
            prev = true;
            issue(cw, sx, sy, G, true);
            cw = nw;
        }
        if (prev) drain();
        const int cntb = (int)(hi - lo) - nfull * 64;                // ragged last batch (cw holds its words)
        const uint32_t sx = EB == 16 ? __builtin_amdgcn_alignbit(cw.y, cw.x, 24) : 0u, sy = EB == 16 ? __builtin_amdgcn_alignbit(cw.z, cw.y, 28) : 0u;
#pragma unroll
        for (int t = 0; t < QW; ++t) {
            if (t * S + slot < cntb) {
                uint32_t d, hit;
                entry(cw, sx, sy, t, d, hit);
                const CT o = atomicAdd(&cnt[d * QW + ql], inc(hit));
                credit(o, hit);
            }
        }
#pragma unroll
        for (int o = QW; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
        if (slot == 0) ap_part[(int64_t)chunk_id * a.qpad + q] = acc;
        return;
    }
    LB cur, nxt;                                                     // the next batch's global loads fly during this one
    cur.template load<NW>(a, lo, hi, lane, wave);
    bool prev = false;
    for (int64_t base = lo; base < hi; base += 64) {
        if (NW > 1) __syncthreads();                                 // every wave is done reading the previous batch
        cur.template publish<NW>(ring, lane, wave);
        nxt.template load<NW>(a, base + 64, hi, lane, wave);
        if (NW > 1) __syncthreads();                                 // the batch is complete in the ring
        const int cntb = (hi - base < 64) ? (int)(hi - base) : 64;
        if (cntb == 64) {
            R ga[G], gb[G];
            fetch(ga, 0);
#pragma unroll
            for (int g = 0; g < NG; g += 2) {
                if (g + 1 < NG) fetch(gb, g + 1);
                eval_issue(ga, prev);
                prev = true;
                if (g + 2 < NG) fetch(ga, g + 2);
                if (g + 1 < NG) eval_issue(gb, true);
            }
        } else {
            if (prev) drain();
            prev = false;
            for (int t = 0; t * S < cntb; ++t) {
                R r;
                LB::get(r, mine, t * S * LB::RS);
                int d;
                uint32_t hit;
                rec_eval01<W, LW, TERN>(qr, r, a.K, d, hit);
                const bool valid = t * S + slot < cntb;
                CT o = 0;
                if (!MASKED) {
                    if (valid) o = atomicAdd(&cnt[d * QW + ql], inc(hit));       // lanes resolve in item order
                } else {
                    for (int s = 0; s < S; ++s) {
                        if (slot == s && valid) o = atomicAdd(&cnt[d * QW + ql], inc(hit));
                    }
                }
                if (valid) credit(o, hit);
            }
        }
        cur = nxt;
    }
    if (prev) drain();
#pragma unroll
    for (int o = QW; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
    if (slot == 0) ap_part[(int64_t)chunk_id * a.qpad + q] = acc;
}


// Does the LDS hand out same-address returning adds of one instruction in ascending lane order?  (see the header)
__global__ __launch_bounds__(64) void k_probe_lane_order(uint32_t* __restrict__ ok_out) {
    __shared__ unsigned long long c64[256];
    __shared__ uint32_t c32[256];
    const int lane = threadIdx.x;
    bool ok = true;
    for (int round = 0; round < 24; ++round) {
        const int S = 2 << (round % 3 == 2 ? (round % 6 == 5 ? 4 : 2) : round % 3);   // 2, 4, 8, 2, 4, 32, ...
        const int QW = 64 / S;
        const int ql = lane & (QW - 1);
        const int row = (lane * 7 + round * 5 + (lane >> 3)) % 3;                       // a few "buckets" per query
        const int cell = row * QW + ql;
        for (int e = lane; e < 256; e += 64) { c64[e] = 1000ull + round; c32[e] = 77u + round; }
        __syncthreads();
        int before = 0;
        for (int l = 0; l < lane; ++l) {
            const int lrow = (l * 7 + round * 5 + (l >> 3)) % 3;
            before += (lrow * QW + (l & (QW - 1))) == cell;
        }
        const unsigned long long r64 = atomicAdd(&c64[cell], 1ull | (1ull << 32));
        const uint32_t r32 = atomicAdd(&c32[cell], 0x10001u);
        ok = ok && r64 == (1000ull + round) + ((unsigned long long)before | ((unsigned long long)before << 32));
        ok = ok && r32 == 77u + round + (uint32_t)before * 0x10001u;
        __syncthreads();
    }
    const bool all_ok = __all(ok);
    if (lane == 0) *ok_out = all_ok ? 1u : 0u;
}

// The same question AT PASS 2'S GEOMETRY AND UNDER LOAD (round 6): one wave per block with k_scan_ap_c's counter
// array -- 65 bucket rows x 16 queries x 8 bytes, row stride 128 bytes, lane = slot * 16 + query --, five such waves per SIMD like
// the product launch, eight returning 64-bit adds {1, -relevant} in flight before a counted wait, and every fifth block an MFMA loop
// instead, so that probing waves share their SIMDs with matrix waves as pass 2 shares the chip with nothing less busy.  A few
// hundred million adds in all -- the size of the headline evaluation -- in a fraction of a millisecond, once per device and process.
// The check needs no model of the counters' history: the lanes of one instruction that hit the same cell must have been served in
// ascending slot order, i.e. a lane's return = the lowest such lane's return + {lower lanes of the cell, - relevant lower lanes}; a
// shadow array (one plain LDS update per cell and instruction) must equal the counters at the end.  `fault` (XMH_SCAN_PROBE_FAULT,
// the test hook) makes the expectation that of a device serving the lanes in DESCENDING order, which no device does: the probe then
// fails exactly as it would on hardware with another order.
constexpr int kProbeRows = 65, kProbeRounds = 96;
__global__ __launch_bounds__(64) void k_probe_lane_order_load(uint32_t* __restrict__ bad_out, int fault, float* __restrict__ sink) {
    __shared__ unsigned long long cnt[kProbeRows * 16];
    __shared__ unsigned long long shadow[kProbeRows * 16];
    const int lane = threadIdx.x;
    if (blockIdx.x % 5 == 4) {                                   // a matrix wave beside the probing ones
        typedef float v4f __attribute__((ext_vector_type(4)));
        typedef _Float16 v8h __attribute__((ext_vector_type(8)));
        v8h x, y;
        for (int i = 0; i < 8; ++i) { x[i] = (_Float16)(0.001f * (float)(lane + i)); y[i] = (_Float16)(0.002f * (float)(lane ^ i)); }
        v4f acc = {0.f, 0.f, 0.f, 0.f};
        for (int it = 0; it < kProbeRounds * 24; ++it) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(x, y, acc, 0, 0, 0);
        if (acc[0] == 12345.678f) sink[lane] = acc[1];           // (never: keeps the loop)
        return;
    }
    const int ql = lane & 15, slot = lane >> 4;
    for (int e = lane; e < kProbeRows * 16; e += 64) {
        cnt[e] = (unsigned long long)(0x4b000000u + 3u * e) | ((unsigned long long)(0x4b7fffffu - 5u * e) << 32);      // float-bit counters as pass 2 starts them
        shadow[e] = cnt[e];
    }
    __syncthreads();
    const uint32_t cntbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned long long*)cnt + ql * 8;
    uint32_t bad = 0;
    uint32_t h = 0x9E3779B9u * (blockIdx.x + 1) + 0x85ebca6bu * (uint32_t)lane;
    for (int round = 0; round < kProbeRounds; ++round) {
        uint32_t d[8], m[8];
        unsigned long long old[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            h ^= h << 13; h ^= h >> 17; h ^= h << 5;
            // few distinct rows per instruction: the four slots of a query collide often, in every pattern
            d[u] = ((uint32_t)(round * 8 + u) * 7u + ((h >> 9) % 3u) * 11u) % (uint32_t)kProbeRows;
            m[u] = (h & 0x70u) ? 0u : ~0u;                        // about one lane in eight "relevant"
            const uint32_t addr = cntbase + d[u] * 128u;
            const unsigned long long inc = 1ull | ((unsigned long long)m[u] << 32);
            asm volatile("ds_add_rtn_u64 %0, %1, %2" : "=v"(old[u]) : "v"(addr), "v"(inc) : "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(old[0]), "+v"(old[1]), "+v"(old[2]), "+v"(old[3]), "+v"(old[4]), "+v"(old[5]), "+v"(old[6]), "+v"(old[7])::"memory");
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            // the other three slots of this query, same instruction
            uint32_t before = 0, before_rel = 0, group = 0, group_rel = 0;
            unsigned long long first = old[u];
            int first_slot = slot;
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) {
                const int src = s2 * 16 + ql;
                const uint32_t d2 = (uint32_t)__shfl((int)d[u], src, 64), m2 = (uint32_t)__shfl((int)m[u], src, 64);
                const unsigned long long o2 = ((unsigned long long)(uint32_t)__shfl((int)(old[u] >> 32), src, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)old[u], src, 64);
                if (d2 != d[u]) continue;
                ++group;
                group_rel += m2 & 1u;
                const bool lower = fault ? s2 > slot : s2 < slot;     // the order this device is expected to serve the lanes in
                if (lower) { ++before; before_rel += m2 & 1u; }
                const bool firster = fault ? s2 > first_slot : s2 < first_slot;
                if (firster) { first = o2; first_slot = s2; }
            }
            const uint32_t want_lo = (uint32_t)first + before, want_hi = (uint32_t)(first >> 32) - before_rel;
            if ((uint32_t)old[u] != want_lo || (uint32_t)(old[u] >> 32) != want_hi) bad = 1;
            if (first_slot == slot) {                             // one lane per cell and instruction keeps the books
                const unsigned long long sv = shadow[d[u] * 16 + ql];
                shadow[d[u] * 16 + ql] = (unsigned long long)((uint32_t)sv + group) | ((unsigned long long)((uint32_t)(sv >> 32) - group_rel) << 32);
            }
        }
    }
    __syncthreads();
    for (int e = lane; e < kProbeRows * 16; e += 64)
        if (cnt[e] != shadow[e]) bad = 1;
    if (__any(bad != 0) && lane == 0) atomicOr(bad_out, 1u);
}

// sharded evaluation: the all-gathered per-shard bucket histograms hist_g[world][2][Q][nb] (plane 0 = all
// items, plane 1 = relevant) -> the rank offsets pass 2 starts from on shard `rank`:
//   base[q][d] = (# items in buckets < d on ANY shard) + (# items in bucket d on shards < rank);  nrel[q] = all relevant.
// One wave per query, lanes over buckets (coalesced), wave prefix scan per 64-bucket segment.
__global__ __launch_bounds__(64) void k_shard_offsets(const uint32_t* __restrict__ hist_g, int world, int rank, int Q, int nb,
                                                      uint32_t* __restrict__ base_all, uint32_t* __restrict__ base_rel,
                                                      uint32_t* __restrict__ nrel_total) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const int64_t plane = (int64_t)Q * nb;
    uint32_t carry_a = 0, carry_r = 0;
    for (int d0 = 0; d0 < nb; d0 += 64) {
        const int d = d0 + lane;
        uint32_t ta = 0, tr = 0, la = 0, lr = 0;
        if (d < nb) {
            for (int w = 0; w < world; ++w) {
                const uint32_t* h = hist_g + (int64_t)w * 2 * plane + (int64_t)q * nb + d;
                const uint32_t a = h[0], r = h[plane];
                ta += a; tr += r;
                if (w < rank) { la += a; lr += r; }
            }
        }
        uint32_t sa = ta, sr = tr;                              // inclusive scan over the segment
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t ua = __shfl_up(sa, o, 64), ur = __shfl_up(sr, o, 64);
            if (lane >= o) { sa += ua; sr += ur; }
        }
        if (d < nb) {
            base_all[(int64_t)q * nb + d] = carry_a + sa - ta + la;
            base_rel[(int64_t)q * nb + d] = carry_r + sr - tr + lr;
        }
        carry_a += __shfl(sa, 63, 64);
        carry_r += __shfl(sr, 63, 64);
    }
    if (lane == 0) nrel_total[q] = carry_r;
}

// The sharded call's offsets in one launch, from the all-gathered TOTALS TABLES of the shards in the workspace's own layout
// (tot_g[world][nb][qpad] {all, relevant}: what k_scan_below leaves behind, gathered as it is -- no export pass, no transposed
// copy): dpre[d][q] = items of lower buckets on any shard + items of bucket d on lower shards, cap_ws[q] = relevant items on all
// shards, cap_out[q] = min(that, k).  64 queries per block (lanes, coalesced), the bucket axis split over the 4 waves as in
// k_scan_dpre.
__global__ __launch_bounds__(256) void k_shard_offsets_dpre(const uint2* __restrict__ tot_g, int world, int rank, int Q, int qpad, int nb,
                                                            int64_t kcap, uint2* __restrict__ dpre, uint32_t* __restrict__ cap_ws,
                                                            int32_t* __restrict__ cap_out, uint32_t* __restrict__ items_total) {
    __shared__ uint2 part[4][64];
    const int lane = threadIdx.x & 63, wq = threadIdx.x >> 6;
    const int q = blockIdx.x * 64 + lane;
    const int64_t plane = (int64_t)nb * qpad;
    const int nbq = (nb + 3) / 4;
    const int d0 = wq * nbq, d1 = (d0 + nbq < nb) ? d0 + nbq : nb;
    uint32_t sa = 0, sr = 0;
    for (int d = d0; d < d1; ++d) {
        for (int w = 0; w < world; ++w) {
            const uint2 t = tot_g[(int64_t)w * plane + (int64_t)d * qpad + q];
            sa += t.x;
            sr += t.y;
        }
    }
    part[wq][lane] = make_uint2(sa, sr);
    __syncthreads();
    uint32_t ra = 0, rr = 0, tr = 0, ta_all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint2 pw = part[w][lane];
        if (w < wq) { ra += pw.x; rr += pw.y; }
        tr += pw.y;
        ta_all += pw.x;
    }
    if (items_total && blockIdx.x == 0 && threadIdx.x == 0) *items_total = ta_all;      // every query sees every item: the gallery size over all shards
    for (int d = d0; d < d1; ++d) {
        uint32_t ta = 0, tr2 = 0, la = 0, lr = 0;
        for (int w = 0; w < world; ++w) {
            const uint2 t = tot_g[(int64_t)w * plane + (int64_t)d * qpad + q];       // second walk: L2 hits
            ta += t.x; tr2 += t.y;
            if (w < rank) { la += t.x; lr += t.y; }
        }
        dpre[(int64_t)d * qpad + q] = make_uint2(ra + la, rr + lr);
        ra += ta;
        rr += tr2;
    }
    if (wq == 0) {
        cap_ws[q] = tr;
        if (q < Q) cap_out[q] = (int32_t)((kcap > 0 && (uint64_t)kcap < (uint64_t)tr) ? (uint32_t)kcap : tr);
    }
}

// The all-to-all form of the sharded exchange: instead of every rank receiving every shard's whole totals table
// (world x 2.6 MB at Q 5000, K 64), rank j receives from every shard only the column slice of ITS S = qpad / world queries
// (tot_s[world][nb][S] {all, relevant}), resolves the offsets of those queries for EVERY shard
//   out[w][d][s] = items of lower buckets on any shard + items of bucket d on shards < w        (d < nb)
//   out[w][nb][s] = {relevant items on all shards, items on all shards}
// and a second all-to-all hands shard w its rows back.  64 queries per block (lanes), the bucket axis split over the 4 waves.
__global__ __launch_bounds__(256) void k_shard_slice_offsets(const uint2* __restrict__ tot_s, int world, int nb, int S, uint2* __restrict__ out) {
    __shared__ uint2 part[4][64];
    const int lane = threadIdx.x & 63, wq = threadIdx.x >> 6;
    const int s = blockIdx.x * 64 + lane;
    const bool ok = s < S;
    const int64_t plane_in = (int64_t)nb * S, plane_out = (int64_t)(nb + 1) * S;
    const int nbq = (nb + 3) / 4;
    const int d0 = wq * nbq, d1 = (d0 + nbq < nb) ? d0 + nbq : nb;
    uint32_t sa = 0, sr = 0;
    for (int d = d0; d < d1; ++d) {
        for (int w = 0; w < world; ++w) {
            const uint2 t = ok ? tot_s[(int64_t)w * plane_in + (int64_t)d * S + s] : make_uint2(0u, 0u);
            sa += t.x;
            sr += t.y;
        }
    }
    part[wq][lane] = make_uint2(sa, sr);
    __syncthreads();
    uint32_t ra = 0, rr = 0, ta_all = 0, tr_all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint2 pw = part[w][lane];
        if (w < wq) { ra += pw.x; rr += pw.y; }
        ta_all += pw.x;
        tr_all += pw.y;
    }
    if (!ok) return;
    for (int d = d0; d < d1; ++d) {
        uint32_t la = 0, lr = 0;
        for (int w = 0; w < world; ++w) {                            // second walk: L2 hits
            const uint2 t = tot_s[(int64_t)w * plane_in + (int64_t)d * S + s];
            out[(int64_t)w * plane_out + (int64_t)d * S + s] = make_uint2(ra + la, rr + lr);
            la += t.x;
            lr += t.y;
        }
        ra += la;
        rr += lr;
    }
    if (wq == 0)
        for (int w = 0; w < world; ++w) out[(int64_t)w * plane_out + (int64_t)nb * S + s] = make_uint2(tr_all, ta_all);
}

// ... and on shard w the rows that came back, offs[owner][nb + 1][S], go where pass 2 reads them: dpre[d][q], the relevant count,
// the cap, and the gallery size over all shards (the gate word of k_scan_ap_c)
__global__ __launch_bounds__(256) void k_shard_scatter_offsets(const uint2* __restrict__ offs, int nb, int S, int Q, int qpad, int64_t kcap,
                                                               uint2* __restrict__ dpre, uint32_t* __restrict__ cap_ws, int32_t* __restrict__ cap_out,
                                                               uint32_t* __restrict__ items_total) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= qpad) return;
    const int owner = q / S, s = q - owner * S;
    const uint2* __restrict__ src = offs + (int64_t)owner * (nb + 1) * S + s;
    const int d = blockIdx.y;
    if (d < nb) {
        dpre[(int64_t)d * qpad + q] = src[(int64_t)d * S];
        return;
    }
    const uint2 t = src[(int64_t)nb * S];                           // {relevant items on all shards, items on all shards}
    cap_ws[q] = t.x;
    if (q < Q) cap_out[q] = (int32_t)((kcap > 0 && (uint64_t)kcap < (uint64_t)t.x) ? (uint32_t)kcap : t.x);
    if (q == 0) *items_total = t.y;
}

// Sum of a query's per-chunk credits.  A block takes 64 queries; its 4 waves take a quarter of the chunks each (all loads of a
// thread are issued together: one dependent load per chunk was a 13 us chain of misses for 32 chunks) and the quarters are added
// in a fixed order -- the same order in the sharded and the unsharded reduction, whatever the grid.
__device__ __forceinline__ double ap_chunk_sum(const float* __restrict__ ap_part, int qpad, int nchunk, int q, double (*quarter)[64]) {
    const int lane = threadIdx.x & 63, wq = threadIdx.x >> 6;
    const int per = (nchunk + 3) / 4;
    const int c0 = wq * per, c1 = (c0 + per < nchunk) ? c0 + per : nchunk;
    double s = 0.0;
    for (int c = c0; c < c1; c += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = c + j < c1 ? ap_part[(int64_t)(c + j) * qpad + q] : 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (c + j < c1) s += (double)v[j];
    }
    quarter[wq][lane] = s;
    __syncthreads();
    return ((quarter[0][lane] + quarter[1][lane]) + quarter[2][lane]) + quarter[3][lane];
}

// nrel_ws != null (unsharded call): cap_out[q] = min(nrel_ws[q], kcap) is written here; else the caller's cap_out is read.
// grid = qpad / 64 blocks of 256 threads.
__global__ __launch_bounds__(256) void k_ap_reduce(const float* __restrict__ ap_part, int Q, int qpad, int nchunk,
                                                   double* __restrict__ ap_sum, const uint32_t* __restrict__ nrel_ws, uint32_t kcap,
                                                   int32_t* __restrict__ cap_out) {
    __shared__ double quarter[4][64];
    const int q = blockIdx.x * 64 + (threadIdx.x & 63);
    const double s = ap_chunk_sum(ap_part, qpad, nchunk, q, quarter);
    if (threadIdx.x >= 64 || q >= Q) return;
    ap_sum[q] = s;
    if (nrel_ws) cap_out[q] = (int32_t)min(nrel_ws[q], kcap);
}

// k_ap_reduce + k_map_finalize in one launch (unsharded evaluation): every block also leaves the sum of ap/cap over its 64
// queries in part[], takes a ticket, and the block that draws the last ticket adds the partials IN BLOCK ORDER (deterministic)
// into the mean.  Hand-off as in k_scan_below: the partial goes out as an agent-scope store, vmcnt(0), then the ticket; the last
// block reads the partials with agent-scope loads, one per thread (a thread walking them was a chain of 20 dependent misses);
// no fence: a release would write back the XCD's whole L2.  The ticket word is zeroed by
// xmh_hamming_hist and put back to zero by the last block, so several evaluations can follow one pass 1.
// (One block doing all of it was tried: 40 us -- a single block cannot pull 1 MB fast.)
__global__ __launch_bounds__(256) void k_ap_reduce_map(const float* __restrict__ ap_part, int Q, int qpad, int nchunk,
                                                       const uint32_t* __restrict__ nrel_ws, uint32_t kcap, int32_t* __restrict__ cap_out,
                                                       double* __restrict__ ap_sum, double* __restrict__ part, uint32_t* __restrict__ ticket,
                                                       double* __restrict__ map_out) {
    __shared__ double quarter[4][64];
    __shared__ double red[64];
    __shared__ int last;
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 64 + lane;
    const double s = ap_chunk_sum(ap_part, qpad, nchunk, q, quarter);
    if (threadIdx.x < 64) {
        double term = 0.0;
        if (q < Q) {
            const int32_t cap = (int32_t)min(nrel_ws[q], kcap);
            ap_sum[q] = s;
            cap_out[q] = cap;
            term = s / (double)cap;                                  // cap == 0 -> NaN (0/0), like the reference
        }
        red[lane] = term;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double b = 0.0;
        for (int j = 0; j < 64; ++j) b += red[j];                    // in query order
        __hip_atomic_store(&part[blockIdx.x], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = t == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    double m = 0.0;                                                  // <= 4096 blocks: 16 rounds of 256 parallel loads, added in block order
    for (unsigned b0 = 0; b0 < gridDim.x; b0 += 256) {
        const unsigned b = b0 + threadIdx.x;
        __syncthreads();
        reinterpret_cast<double*>(quarter)[threadIdx.x] = b < gridDim.x ? __hip_atomic_load(&part[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned n = gridDim.x - b0 < 256u ? gridDim.x - b0 : 256u;
            for (unsigned j = 0; j < n; ++j) m += reinterpret_cast<double*>(quarter)[j];
        }
    }
    if (threadIdx.x == 0) {
        map_out[0] = m / (double)Q;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_map_finalize(const double* __restrict__ ap_sum, const int32_t* __restrict__ cap,
                                                      int64_t Q, double* __restrict__ map_out) {
    __shared__ double part[256];
    double s = 0.0;
    for (int64_t q = threadIdx.x; q < Q; q += 256) s += ap_sum[q] / (double)cap[q];   // cap == 0 -> NaN (0/0)
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) map_out[0] = part[0] / (double)Q;
}
}  // namespace
