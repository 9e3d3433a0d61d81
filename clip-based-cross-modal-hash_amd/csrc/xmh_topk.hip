// Exact per-query top-k over bit-packed codes in ONE streaming pass over the gallery shard
// (north_star: "fused bit-packed XOR-popcount + per-query top-k kernel with wavefront reductions and
// coalesced HBM reads over the gallery").  Order = (distance asc, gallery index asc).
//
// Shape: one lane per gallery item (16-byte coalesced loads, next tile prefetched into a second register
// set), up to 8 queries per block held in SGPRs.  Each persistent block owns a CONTIGUOUS range of tiles and
// walks it in index order, keeping for every query a small candidate buffer in LDS plus a bucket histogram
// of the buffer.  t_run = current k-th smallest distance; an item is a candidate only if d < t_run, so after
// the first few tiles almost every tile costs: loads + XOR/popcount + one ballot + ONE barrier.  Candidates
// are appended in index order (wave-local ballot prefix + one cross-wave exchange), which makes "first n
// ties in buffer order" the exact index tie-break -- no sort in the streaming loop.  A second tiny kernel
// merges the per-block lists with the same machinery and bitonic-sorts the final k keys.
//
// Bound: HBM for few queries.  Algorithmic bytes per launch = R*W*4 (gallery read once)
// + Q*W*4 + nblocks*Q*k*6 (partial lists) ; per pair 2W lane-ops.
//
// This file is the host side; the kernels are in xmh_topk_kernels.h.  A call goes plan_topk (shapes, the robust path's launch sizes and
// LDS layouts, the workspace) -> filter_route (which streaming filter) -> filter_geom (its grid) -> topk_call (the launches in stream order).
#include "xmh_common.h"
#include "xmh_device.h"
#include "xmh_topk_kernels.h"
#include <algorithm>
#include <type_traits>
#include <vector>

#include <stdlib.h>

namespace {

struct TopkPlan {
    int64_t Q;
    int k, W, ipt, tile, nblocks, tiles_per_block, nqg, nb;
    Layout L, Lm;
    size_t ws_bytes;
};

// The workspace as the kernels see it.  One Arena walk (bind_ws) sizes it and hands out the pieces.
struct TopkWs {
    int32_t* part_i;           // robust path: [Q][nblocks][k] indices and, behind them in the same piece,
    uint16_t* part_d;          //              [Q][nblocks][k] distances
    TopkCtl* ctl;              // ctl, hist, t_est, bound, cnt, fail are contiguous: one memset clears them (clear_fast_state)
    FastWs f;
    size_t bytes;
};

TopkWs bind_ws(const TopkPlan& p, void* ws) {
    static_assert(sizeof(TopkCtl) <= 256, "the control words take one 256-byte piece");
    const size_t Q = (size_t)p.Q, lists = Q * p.nblocks * p.k;
    xmh::Arena a(ws);
    TopkWs w;
    char* robust = a.take<char>(lists * 6);
    w.part_i = reinterpret_cast<int32_t*>(robust);
    w.part_d = robust ? reinterpret_cast<uint16_t*>(robust + lists * 4) : nullptr;
    w.ctl = a.take<TopkCtl>(1);
    w.f.hist = a.take<uint32_t>(Q * p.nb);
    w.f.t_est = a.take<uint32_t>(Q);
    w.f.bound = a.take<uint32_t>(Q);
    w.f.cnt = a.take<uint32_t>(Q * kSub * kCntStride);
    w.f.fail = a.take<int>(Q);
    w.f.cand = a.take<unsigned long long>(Q * kCandCap);
    w.bytes = a.used;
    return w;
}

// The control words and the sample histogram are zero on entry and left zero on exit (each consumer puts its word back): a prepared
// workspace (xmh_topk_ws_init) needs no memset launch, an unprepared call clears them itself.
int clear_fast_state(const TopkWs& w, hipStream_t st) {
    XMH_HIP(hipMemsetAsync(w.ctl, 0, reinterpret_cast<char*>(w.f.cand) - reinterpret_cast<char*>(w.ctl), st));
    return XMH_OK;
}

constexpr int ipt_for(int W) { return W >= 16 ? 1 : (W >= 8 ? 4 : 8); }      // long codes: one 64..256-byte record per thread and tile

int plan_topk(int64_t Q, int64_t R, int K, int k, TopkPlan* p, bool tern = false) {
    if (Q <= 0 || R <= 0 || K <= 0) return xmh::fail(XMH_EINVAL, "topk: bad shape Q=%lld R=%lld K=%d", (long long)Q, (long long)R, K);
    if (k <= 0 || k > 1024) return xmh::fail(XMH_EINVAL, "topk: k=%d out of range (1..1024)", k);
    if (R >= (1ll << 31) - 65536) return xmh::fail(XMH_ENOTSUP, "topk: shard of %lld rows (max 2^31-1)", (long long)R);
    const int W = (K + 31) / 32;
    if (W != 1 && W != 2 && W != 4 && W != 8 && W != 16 && W != 32 && W != 64)
        return xmh::fail(XMH_ENOTSUP, "topk: K=%d unsupported (code words must be a power of two up to 64, i.e. K <= 2048)", K);
    p->Q = Q;
    p->k = k;
    p->W = W;
    p->ipt = ipt_for(W);
    p->tile = kThreads * p->ipt;
    const int nb = tern ? 2 * K + 1 : K + 1;               // ternary codes: half-unit distances 0 ... 2K
    p->nb = nb;
    p->L.nb = nb;
    p->L.nq = kQG;
    p->L.cap = k + p->tile + 64;
    if (p->L.bytes() > 160 * 1024) return xmh::fail(XMH_ENOTSUP, "topk: k=%d, K=%d%s needs %zu B of LDS (max 163840)", k, K, tern ? " (ternary)" : "", p->L.bytes());
    if ((p->L.cap + kThreads - 1) / kThreads > 24) return xmh::fail(XMH_ENOTSUP, "topk: candidate buffer too large for the compaction segment");
    const int64_t ntiles = xmh::ceil_div(R, p->tile);
    int bpc = (int)((160 * 1024) / p->L.bytes());
    if (bpc > 4) bpc = 4;
    if (bpc < 1) bpc = 1;
    int64_t nblocks = (int64_t)xmh::device_cu_count() * bpc;
    if (nblocks > ntiles) nblocks = ntiles;
    p->tiles_per_block = (int)xmh::ceil_div(ntiles, nblocks);
    p->nblocks = (int)xmh::ceil_div(ntiles, p->tiles_per_block);
    p->nqg = (int)xmh::ceil_div(Q, kQG);
    p->Lm.nb = nb;
    p->Lm.nq = 3;
    p->Lm.cap = k + kThreads * 4 + 64;
    if (p->Lm.bytes() > 160 * 1024) return xmh::fail(XMH_ENOTSUP, "topk: k=%d, K=%d needs %zu B of LDS in the merge (max 163840)", k, K, p->Lm.bytes());
    p->ws_bytes = bind_ws(*p, nullptr).bytes;
    return XMH_OK;
}

size_t topk_ws_bytes(int64_t Q, int64_t R, int K, int k, bool tern) {
    TopkPlan p;
    return plan_topk(Q, R, K, k, &p, tern) == XMH_OK ? p.ws_bytes : 0;
}

int topk_ws_init(int64_t Q, int64_t R, int K, int k, bool tern, void* ws, size_t ws_bytes, xmh_stream_t stream) {
    const char* who = tern ? "xmh_topk_ternary_ws_init" : "xmh_topk_ws_init";
    TopkPlan p;
    if (const int rc = plan_topk(Q, R, K, k, &p, tern)) return rc;
    if (!ws) return xmh::fail(XMH_EINVAL, "%s: null workspace", who);
    if (ws_bytes < p.ws_bytes) return xmh::fail(XMH_EINVAL, "%s: workspace too small (%zu < %zu)", who, ws_bytes, p.ws_bytes);
    return clear_fast_state(bind_ws(p, ws), xmh::as_stream(stream));
}

// Which instance of the streaming filter a (code words, queries, ternary) call launches -- one decision for the launch and for xmh_topk_describe:
//   k_topk_filter_mfma<W, qt>      distances on the matrix cores: >= 5 queries at 128 / 256 / 512 bits, qt tiles of 16 queries per pass
//                                  (XMH_TOPK_MFMA, experiments builds only: the smallest query count that takes it, 0 = never); binary codes;
//   k_topk_filter_seq<W, 4, qn>    codes of whole 16-byte pieces (128 ... 2048 bits), every other case: qn queries per pass; ternary codes
//                                  read both planes piece for piece;
//   k_topk_filter_short<W, 4, qn>  32- and 64-bit codes, 4 / 2 items per 16-byte piece;
//   k_topk_filter_item_tern<W, 4, qn>  32- and 64-bit ternary codes, per item.
// Measured (10 M x 256 bit, filter launch): one matrix-core pass over 16 queries 62-64 us whatever their number; per-piece filter 49 / 50 /
// 51.5 / 52 us for 1 / 2 / 3 / 4 queries (3 run as 4; the matrix cores took 67) and 74-78 us for 5-8 as one group of 8 -- VALU-bound, so
// the matrix cores keep those.  The per-item filter of rounds 1-4 (k_topk_filter: one lane per item, 54 / 58 / 95 / 61 / 79 / 80 us for 1 /
// 2 / 3 / 4 / 6 / 8 queries; query groups sharing tiles through L1 for short codes) is gone: behind on every shape
// (tools/proto_stream_read.hip keeps its load form as "rec" for the record).
constexpr int kSeqLoads = 4;                                 // 16-byte loads in flight per lane and tile (8 measured 2-4 % behind)
enum class Filter { kMfma, kSeq, kShort, kItemTern };
struct FilterRoute { Filter kind; int qn, qt; };             // queries per pass (all but kMfma); tiles of 16 queries per pass (kMfma, else 0)
FilterRoute filter_route(int W, int64_t Q, bool tern) {
    static const int mfma_min_q = [] { const char* e = xmh_experiment_env("XMH_TOPK_MFMA"); return e ? atoi(e) : -1; }();
    FilterRoute r{W >= 4 ? Filter::kSeq : (tern ? Filter::kItemTern : Filter::kShort), 0, 0};
    r.qn = Q >= 5 ? 8 : (Q >= 3 ? 4 : (Q >= 2 ? 2 : 1));    // 4 query registers per query (pieces) / scalar registers (short codes)
    if (!tern && (W == 4 || W == 8 || W == 16) && (mfma_min_q < 0 ? Q >= 5 : (mfma_min_q > 0 && Q >= mfma_min_q))) {
        const int qtmax = W == 16 ? 2 : 4;                   // B operands: 16 * QT * W / 8 registers
        r.kind = Filter::kMfma;
        r.qt = Q <= 16 ? 1 : (Q <= 32 || qtmax == 2 ? 2 : 4);
    }
    return r;
}

// grid of the streaming filter: x = persistent blocks over the gallery, never more than there are tiles of work; y = query groups
dim3 filter_geom(const FilterRoute& r, int W, int64_t Q, int64_t R) {
    const int cus = xmh::device_cu_count();
    const int64_t tile = (int64_t)kThreads * kSeqLoads;
    unsigned gy = (unsigned)xmh::ceil_div(Q, r.qn);
    int64_t blocks = (int64_t)cus * 2, work = 0;
    switch (r.kind) {
    case Filter::kMfma:                                      // eight blocks per CU over all query groups, one per CU at least;
        gy = (unsigned)xmh::ceil_div(Q, 16 * r.qt);          // a step is 64 items per wave
        blocks = (int64_t)cus * 8 / gy;
        if (blocks < cus) blocks = cus;
        work = xmh::ceil_div(R, (int64_t)64 * (kThreads / 64));
        break;
    case Filter::kSeq: work = xmh::ceil_div(R * (W / 4), tile); break;                                  // 16-byte pieces, non-temporal, two blocks per CU
    case Filter::kShort: work = xmh::ceil_div(xmh::ceil_div(R * W + 3, (int64_t)4), tile); break;       // 32- and 64-bit codes: several items per 16 bytes
    case Filter::kItemTern: work = xmh::ceil_div(R, tile); break;                                       // ternary 32 / 64 bits: one item per lane and load
    }
    if (blocks > work) blocks = work;
    return dim3((unsigned)blocks, gy);
}

// a runtime word count / queries per pass -> a compile-time one (as dispatch_shape in xmh_scan.hip)
template <int N0, int... Ns, typename F>
auto dispatch_int(int v, F&& f) {                            // f(integral_constant<N>) of the N that equals v; plan and route admit no other v
    if constexpr (sizeof...(Ns) == 0) return f(std::integral_constant<int, N0>{});
    else return v == N0 ? f(std::integral_constant<int, N0>{}) : dispatch_int<Ns...>(v, f);
}
template <typename F> auto dispatch_words(int W, F&& f) { return dispatch_int<1, 2, 4, 8, 16, 32, 64>(W, f); }
template <typename F> auto dispatch_qn(int qn, F&& f) { return dispatch_int<1, 2, 4, 8>(qn, f); }

struct TopkCall {
    const uint32_t *qbits, *qzero, *rbits, *rzero;           // zero planes: both (ternary codes, distances in half units) or neither
    int64_t Q, R; int K, k;
    int64_t base_index;
    void* ws; size_t ws_bytes;
    uint16_t* dist; int32_t* idx;
    xmh_stream_t stream;
    bool prepared;                                           // the workspace went through ws_init or an earlier call
};

// What the sample of the fast path reads and what the pick asks of it.
struct SamplePlan {
    int sblocks, per_block; int64_t stride;                  // block b reads per_block consecutive rows from b * stride
    int fold_pick; unsigned gy;                              // few queries: the last sample block picks the thresholds itself; else query groups
    uint32_t target;                                         // sampled hits the threshold bucket has to reach
    int sqg; size_t lds;                                     // queries' histograms a sample block keeps in LDS per round, their bytes
    PickParams pp;
};
SamplePlan sample_plan(const TopkPlan& p, const TopkCall& c) {
    const int64_t Q = c.Q, R = c.R;
    SamplePlan s;
    s.fold_pick = Q <= kFoldPickQ;
    s.gy = s.fold_pick ? 1u : (unsigned)(xmh::ceil_div(Q, 16) < 4096 ? xmh::ceil_div(Q, 16) : 4096);
    s.sblocks = kSampleBlocks;
    s.stride = R / s.sblocks;
    // short codes: the sample grows with the gallery (2.6 % of it up to 80 M rows): at a fixed 262 144 rows the safety margin of the pick (+8
    // sampled hits) asked for 8 / fraction = 1 200 estimated candidates at 40 M rows, one bucket too far for short codes, where a
    // bucket more is 4-5 x the candidates and overflows the list (40 M x 32 bit, Q = 16: the robust path in most calls)
    // (codes of 128 bits and more have fine buckets and keep the fixed sample: at 256 bit, Q = 64 the larger one cost 6 % of the call)
    s.per_block = kSamplePerBlock * (p.W >= 4 ? 1 : (int)(R / 10000000 < 1 ? 1 : (R / 10000000 > 8 ? 8 : R / 10000000)));
    bool exact = false;
    if (s.stride <= s.per_block) {                        // small gallery: the "sample" is the whole gallery
        s.sblocks = (int)xmh::ceil_div(R, s.per_block);
        s.stride = s.per_block;
        exact = true;
    }
    const double frac = exact ? 1.0 : (double)((int64_t)s.sblocks * s.per_block) / (double)R;
    s.target = exact ? (uint32_t)((int64_t)c.k < R ? (int64_t)c.k : R) : (uint32_t)(2.0 * c.k * frac + 8.0);
    s.sqg = p.nb <= 2049 ? 16 : (32768 / p.nb > 0 ? 32768 / p.nb : 1);      // 128 KB of histograms per sample block at most (ternary 1024 / 2048 bits)
    s.lds = (size_t)s.sqg * p.nb * 4;
    s.pp = PickParams{(float)(1.0 / frac), (uint32_t)c.k, (uint32_t)R, exact ? 1 : 0};
    return s;
}

void launch_sample(const TopkPlan& p, const TopkCall& c, const TopkWs& w, int pad, hipStream_t st) {
    XMH_RANGE("topk: sample + threshold pick");
    const SamplePlan s = sample_plan(p, c);
    const FastWs& f = w.f;
    dispatch_words(p.W, [&](auto w_c) {
        constexpr int WW = decltype(w_c)::value;
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(s.sblocks, s.gy), dim3(kThreads), s.lds, st, c.qbits, c.qzero, c.rbits, c.rzero, pad, (int)c.Q, c.R, p.nb, s.stride,
                               s.per_block, f.hist, s.fold_pick, s.target, w.ctl, f.t_est, f.cnt, f.fail, s.pp, f.bound, s.sqg);
        };
        if (c.qzero) go(k_topk_sample<WW, true>);
        else go(k_topk_sample<WW, false>);
    });
    if (!s.fold_pick)
        hipLaunchKernelGGL(k_topk_pick, dim3((unsigned)c.Q), dim3(64), 0, st, f.hist, (int)c.Q, p.nb, s.target, f.t_est, f.cnt, f.fail, s.pp, f.bound);
}

// the streaming pass of the fast path: the instance filter_route names on the grid of filter_geom
void launch_filter(const TopkPlan& p, const TopkCall& c, const TopkWs& w, int pad, hipStream_t st) {
    XMH_RANGE("topk: streaming filter");
    const bool tern = c.qzero != nullptr;
    const FilterRoute r = filter_route(p.W, c.Q, tern);
    const dim3 grid = filter_geom(r, p.W, c.Q, c.R);
    const FastWs& f = w.f;
    xmh::ProfScope prof("topk_filter", st);
    const uint32_t *t_est = f.t_est, *bound = f.bound;
    auto mfma = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, st, c.qbits, c.rbits, (int)c.Q, c.R, t_est, f.cnt, f.cand); };
    auto planes = [&](auto kern, int pad_) {                 // both planes (null for binary codes) and the padding bits of the half-unit distance
        hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, st, c.qbits, c.qzero, c.rbits, c.rzero, pad_, (int)c.Q, c.R, t_est, bound, f.cnt, f.cand);
    };
    auto shrt = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, st, c.qbits, c.rbits, (int)c.Q, c.R, t_est, bound, f.cnt, f.cand); };
    dispatch_words(p.W, [&](auto w_c) {
        constexpr int WW = decltype(w_c)::value;
        if constexpr (WW == 4 || WW == 8 || WW == 16) {
            if (r.kind == Filter::kMfma) {
                if (r.qt == 1) mfma(k_topk_filter_mfma<WW, 1>);
                else if (r.qt == 2) mfma(k_topk_filter_mfma<WW, 2>);
                else if constexpr (WW != 16) mfma(k_topk_filter_mfma<WW, 4>);
                return;
            }
        }
        dispatch_qn(r.qn, [&](auto qn_c) {
            constexpr int QN = decltype(qn_c)::value;
            if constexpr (WW % 4 == 0) {
                if (tern) planes(k_topk_filter_seq<WW, kSeqLoads, QN, true>, pad);
                else planes(k_topk_filter_seq<WW, kSeqLoads, QN, false>, 0);
            } else {
                if (tern) planes(k_topk_filter_item_tern<WW, kSeqLoads, QN>, pad);
                else shrt(k_topk_filter_short<WW, kSeqLoads, QN>);
            }
        });
    });
}

int topk_call(const TopkCall& c) {
    if ((c.qzero == nullptr) != (c.rzero == nullptr)) return xmh::fail(XMH_EINVAL, "xmh_hamming_topk: zero planes for both sides or neither");
    const bool tern = c.qzero != nullptr;
    TopkPlan p;
    int rc = plan_topk(c.Q, c.R, c.K, c.k, &p, tern);
    if (rc) return rc;
    const int pad = 32 * p.W - c.K;                       // padding bits: set in both zero planes, taken out of the half-unit distance
    if (!c.qbits || !c.rbits || !c.ws || !c.dist || !c.idx) return xmh::fail(XMH_EINVAL, "xmh_hamming_topk: null pointer");
    if (c.ws_bytes < p.ws_bytes) return xmh::fail(XMH_EINVAL, "xmh_hamming_topk: workspace too small (%zu < %zu)", c.ws_bytes, p.ws_bytes);
    const TopkWs w = bind_ws(p, c.ws);
    hipStream_t st = xmh::as_stream(c.stream);
    const int* gate = nullptr;
    if (!getenv("XMH_TOPK_ROBUST_ONLY")) {                // (test hook, read per call: set, the fast path is skipped)
        // ---- fast path: sample -> threshold -> filter -> select (all stream-ordered, no host sync) ----
        if (!c.prepared && (rc = clear_fast_state(w, st))) return rc;
        launch_sample(p, c, w, pad, st);
        launch_filter(p, c, w, pad, st);
        XMH_LAUNCH_CHECK("xmh_hamming_topk fast path");
        {
            XMH_RANGE("topk: select");
            auto kern = k_topk_select;
            const size_t sel_lds = (size_t)kCandCap * 8 + 1024 * 8 + (size_t)(p.nb > 2048 ? p.nb : 2048) * 4 + 64;
            rc = xmh::raise_dynamic_lds(reinterpret_cast<const void*>(kern), sel_lds, "xmh_hamming_topk select");
            if (rc) return rc;
            hipLaunchKernelGGL(kern, dim3((unsigned)c.Q), dim3(kThreads), sel_lds, st, (const unsigned long long*)w.f.cand,
                               (const uint32_t*)w.f.cnt, c.R, c.k, p.nb, c.base_index, c.dist, c.idx, w.f.fail);
        }
        XMH_LAUNCH_CHECK("xmh_hamming_topk select");
        gate = w.f.fail;                                 // the robust kernels below run only if a query failed
    }
    XMH_RANGE("topk: robust path (gated on the fail flags)");
    rc = dispatch_words(p.W, [&](auto w_c) {
        constexpr int WW = decltype(w_c)::value, II = ipt_for(WW);
        auto go = [&](auto kern) -> int {
            const size_t lds = p.L.bytes();
            if (const int rc_ = xmh::raise_dynamic_lds(reinterpret_cast<const void*>(kern), lds, "xmh_hamming_topk")) return rc_;
            hipLaunchKernelGGL(kern, dim3(p.nblocks, p.nqg), dim3(kThreads), lds, st, c.qbits, c.qzero, c.rbits, c.rzero, pad, (int)c.Q, c.R, c.k, p.L,
                               p.tiles_per_block, p.nblocks, w.part_d, w.part_i, gate);
            return XMH_OK;
        };
        return tern ? go(k_topk_stream<WW, II, true>) : go(k_topk_stream<WW, II, false>);
    });
    if (rc) return rc;
    XMH_LAUNCH_CHECK("xmh_hamming_topk stream");
    {
        auto kern = k_topk_merge<4>;
        const size_t ldsm = p.Lm.bytes();
        rc = xmh::raise_dynamic_lds(reinterpret_cast<const void*>(kern), ldsm, "xmh_hamming_topk merge");
        if (rc) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)c.Q), dim3(kThreads), ldsm, st, w.part_d, w.part_i, p.nblocks, c.k, p.Lm, c.base_index, c.dist, c.idx, gate);
    }
    XMH_LAUNCH_CHECK("xmh_hamming_topk merge");
    return XMH_OK;
}
}  // namespace

extern "C" size_t xmh_topk_ws_bytes(int64_t Q, int64_t R, int K, int k) { return topk_ws_bytes(Q, R, K, k, false); }

extern "C" int xmh_topk_ws_init(int64_t Q, int64_t R, int K, int k, void* ws, size_t ws_bytes, xmh_stream_t stream) { return topk_ws_init(Q, R, K, k, false, ws, ws_bytes, stream); }

extern "C" int xmh_hamming_topk(const uint32_t* qbits, const uint32_t* rbits, int64_t Q, int64_t R, int K, int k, int64_t base_index, void* ws,
                                size_t ws_bytes, uint16_t* dist, int32_t* idx, xmh_stream_t stream) {
    XMH_RANGE("xmh_hamming_topk");
    return topk_call({qbits, nullptr, rbits, nullptr, Q, R, K, k, base_index, ws, ws_bytes, dist, idx, stream, false});
}

extern "C" int xmh_hamming_topk_prepared(const uint32_t* qbits, const uint32_t* rbits, int64_t Q, int64_t R, int K, int k, int64_t base_index,
                                         void* ws, size_t ws_bytes, uint16_t* dist, int32_t* idx, xmh_stream_t stream) {
    XMH_RANGE("xmh_hamming_topk_prepared");
    return topk_call({qbits, nullptr, rbits, nullptr, Q, R, K, k, base_index, ws, ws_bytes, dist, idx, stream, true});
}

// ---- ternary codes (round 6): the same call with the zero planes; distances come back in HALF units (2 d = K - q.r, 0 ... 2K) ----
extern "C" size_t xmh_topk_ternary_ws_bytes(int64_t Q, int64_t R, int K, int k) { return topk_ws_bytes(Q, R, K, k, true); }

extern "C" int xmh_topk_ternary_ws_init(int64_t Q, int64_t R, int K, int k, void* ws, size_t ws_bytes, xmh_stream_t stream) { return topk_ws_init(Q, R, K, k, true, ws, ws_bytes, stream); }

extern "C" int xmh_hamming_topk_ternary(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* rbits, const uint32_t* rzero, int64_t Q,
                                        int64_t R, int K, int k, int64_t base_index, void* ws, size_t ws_bytes, int prepared, uint16_t* dist2,
                                        int32_t* idx, xmh_stream_t stream) {
    XMH_RANGE("xmh_hamming_topk_ternary");
    if (!qzero || !rzero) return xmh::fail(XMH_EINVAL, "xmh_hamming_topk_ternary: needs both zero planes (binary codes: xmh_hamming_topk)");
    return topk_call({qbits, qzero, rbits, rzero, Q, R, K, k, base_index, ws, ws_bytes, dist2, idx, stream, prepared != 0});
}

// Diagnostics for the measurement harness, like xmh_scan_describe: "filter=<kernel instance>" of the fast path's streaming pass for
// this shape (binary codes), spelled as rocprofv3 prints it, so that a profile row is matched by its exact name.
extern "C" int xmh_topk_describe(int64_t Q, int64_t R, int K, int k, char* out, size_t out_bytes) {
    TopkPlan p;
    if (const int rc = plan_topk(Q, R, K, k, &p)) return rc;
    if (!out || out_bytes < 64) return xmh::fail(XMH_EINVAL, "xmh_topk_describe: buffer too small");
    const FilterRoute r = filter_route(p.W, Q, false);
    if (r.kind == Filter::kMfma) snprintf(out, out_bytes, "filter=k_topk_filter_mfma<%d, %d>", p.W, r.qt);
    else snprintf(out, out_bytes, "filter=k_topk_filter_%s<%d, %d, %d>", r.kind == Filter::kShort ? "short" : "seq", p.W, kSeqLoads, r.qn);
    return XMH_OK;
}

// ---------------------------------------------------------------------------------------------------
// host merge of per-shard lists (sharded retrieval): plain host code, a k-way merge with one cursor per shard
// -- world <= 8 comparisons per output slot instead of an argsort of [Q][world * k] 64-bit keys
// ---------------------------------------------------------------------------------------------------
extern "C" size_t xmh_topk_record_bytes(int64_t Q, int k) {
    if (Q < 0 || k <= 0) return 0;
    return ((size_t)Q * (size_t)k * 6 + 3) & ~(size_t)3;
}

extern "C" int xmh_topk_merge_host(const void* gathered_host, int world, int64_t Q, int k, int32_t* dist_out, int32_t* idx_out) {
    XMH_RANGE("xmh_topk_merge_host");
    if (world <= 0 || world > 4096 || Q < 0 || k <= 0) return xmh::fail(XMH_EINVAL, "xmh_topk_merge_host: bad shape world=%d Q=%lld k=%d", world, (long long)Q, k);
    if (Q == 0) return XMH_OK;
    if (!gathered_host || !dist_out || !idx_out) return xmh::fail(XMH_EINVAL, "xmh_topk_merge_host: null pointer");
    const size_t rec = xmh_topk_record_bytes(Q, k);
    const char* base = static_cast<const char*>(gathered_host);
    std::vector<int> cur((size_t)world);
    for (int64_t q = 0; q < Q; ++q) {
        std::fill(cur.begin(), cur.end(), 0);
        for (int o = 0; o < k; ++o) {
            int best = -1;
            uint64_t best_key = ~0ull;
            for (int w = 0; w < world; ++w) {
                if (cur[w] >= k) continue;
                const int32_t* idx = reinterpret_cast<const int32_t*>(base + (size_t)w * rec) + q * k;
                const int32_t id = idx[cur[w]];
                if (id < 0) { cur[w] = k; continue; }                                  // unused slots end a list
                const uint16_t* dist = reinterpret_cast<const uint16_t*>(base + (size_t)w * rec + (size_t)Q * k * 4) + q * k;
                const uint64_t key = ((uint64_t)dist[cur[w]] << 32) | (uint32_t)id;
                if (key < best_key) { best_key = key; best = w; }
            }
            if (best < 0) { dist_out[q * k + o] = 0xFFFF; idx_out[q * k + o] = -1; continue; }
            dist_out[q * k + o] = (int32_t)(best_key >> 32);
            idx_out[q * k + o] = (int32_t)(uint32_t)best_key;
            ++cur[best];
        }
    }
    return XMH_OK;
}
