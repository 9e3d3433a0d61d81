// Fused ranking scan: calc_map_k (reference common/calc_utils.py:58-92) as two streaming passes over
// bit-packed codes, no [Q,R] intermediate, no sort.
//
// Execution shape: a wave owns QW = 64/S queries and S "slots"; lane = slot * QW + ql holds query ql (code words and
// label masks in VGPRs) and, at step t of a 64-item batch, works on gallery item t*S + slot.  Per-query bucket counters
// sit in LDS as cnt[d][ql].  Walking the gallery in index order makes "number of same-distance items with a smaller
// index" a running counter, which is exactly the tie-break of the canonical (distance, index) order:
//   pass 1 (k_scan_hist_s)  histogram of (distance, relevant) per (chunk, query): one ds_add_u32 per pair;
//   tables                  exclusive prefixes over chunks and over buckets (k_scan_below, k_scan_dpre);
//   pass 2 (k_scan_ap_s)    counters start at the global base of (bucket, chunk); one returning ds_add per pair yields
//                           (rank, ordinal) of the item, relevant items add ordinal/rank to the query's AP sum.
// Codes of at most 256 bits, binary or ternary, take an MFMA-evaluated pass 1 (xmh_scan_mfma.h: k_scan_hist_r2 up to 64 bits, k_scan_hist_r2w
// for 65..128; xmh_scan_bits.hip: k_scan_hist_b for 129..256 bits and for ternary codes), which also leaves (distance << 1 | relevant) of
// every pair in the workspace; pass 2 then reads that pair cache instead of the gallery (k_scan_ap_c, the CACHE variant of k_scan_ap_s), or
// evaluates the pairs again on the MFMA where there is no cache (k_scan_ap_r2).  The table of which kernel takes which shape is at scan_route
// below.  This file is the host side.  What follows describes the VALU kernels (xmh_scan_kernels.h): long codes, > 128 classes, XMH_SCAN_MFMA=0.
// Why slots: with one query per lane (S = 1) the counters of a wave cost nb*64*{4,8} bytes -- 33 KB at K = 64 with
// 64-bit counters (one wave per SIMD), 131 KB at K = 256 (one wave per CU).  S lanes per query shrink the footprint by
// S: 3-4 waves per SIMD for every supported K, which is what hides the LDS round trips of this loop (measured at
// K=64/128/256: 0.55/3.6/13.3 ms for S = 1 against 0.34/0.47/0.77 ms).
// Ordering: the S lanes of a query may hit the same counter in one instruction.  Pass 1 only needs totals.  Pass 2 needs
// the returns in item order; the LDS serialises same-address lanes in ascending lane order (= item order, slot being the
// high lane bits).  That is observed behaviour, not an ISA promise, so xmh_hamming_ap probes it once per process
// (k_probe_lane_order) and otherwise issues the add once per slot under an exec mask (MASKED, ~2x slower).
//
// The gallery batch: lane i loads record base+i (coalesced, vmcnt; the next batch is in flight during the current one),
// the wave stages it record-major in a small LDS ring, and a lane reads the record of its own item with ds_read_b128s
// (S distinct addresses per instruction, each broadcast to QW lanes).  LDS ops of a wave complete in order, so every
// wait in the loop is a counted lgkmcnt; reads run one group of steps (SlotGeom::G) ahead of their use.  Records of 64 B
// and more (K >= 512) are loaded as one contiguous range and scattered to padded rows, and at one query per wave
// (S = 64) eight waves share each staged batch (see AosBatch, k_scan_hist_s).
//
// Bound: VALU issue.  tools/ubench_valu.hip measures ~4.0-4.4 cycles per wave64 instruction per SIMD for
// the instruction mix of these loops (v_xor/v_and/v_add alone reach 2.4, VOP3 ops such as v_bcnt_u32_b32 /
// v_and_or_b32 / v_lshl_add_u32 4.2, v_rcp_f32 8.2): 10 (pass 1) / 14-15 (pass 2) VALU instructions per pair-step of a
// wave at K=64, C=80.  The relevance test is one v_and_or_b32 per label word + one v_min_u32 (inline asm: hipcc does
// not form them).  Algorithmic HBM bytes per launch: R*(4W+4Lw) + Q*(4W+4Lw) (+ the bucket tables in the workspace).
#include "xmh_common.h"
#include <atomic>
#include <math.h>
#include <mutex>
#include <string.h>
#include <vector>
#include "xmh_scan_bits.h"
#include "xmh_scan_mfma.h"
#include "xmh_scan_kernels.h"

#include <stdlib.h>
#include <type_traits>
#include <unordered_map>

namespace {

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
// lanes per query (S): smallest power of two that brings the counters of a wave under the budget.  Budgets from a sweep
// on MI355X (K = 16..256, dense and sparse relevance): 9 KB for 64-bit counters, 5 KB for 32-bit ones (3-4 waves/SIMD).
constexpr int kSlotBudget64 = 9 * 1024;
constexpr int kSlotBudget32 = 5 * 1024;
// Long codes (W > 8 words: TwDH-style 512..2048 bits) go up to S = 64, i.e. one query per wave and one
// gallery item per lane.
constexpr int slots_for(int W, bool tern, int counter_bytes) {
    const int nbmax = (tern ? 64 : 32) * W + 1;
    const int budget = counter_bytes == 8 ? kSlotBudget64 : kSlotBudget32;
    const int cap = W > 8 ? 64 : 8;
    int S = 2;
    while (S < cap && nbmax * (64 / S) * counter_bytes > budget) S *= 2;
    return S;
}
// code words of the instance a length runs on: 1, 2, 4, 8, 16, 32, 64 (retrieval.widened pads the others)
inline int instance_words(int W) { return W <= 1 ? 1 : (W <= 2 ? 2 : (W <= 4 ? 4 : (W <= 8 ? 8 : (W <= 16 ? 16 : (W <= 32 ? 32 : 64))))); }
// the pair cache of k_scan_hist_s: two code words, binary, four slots in both passes and both counter widths
constexpr bool pair_cache_shape(int W, bool tern) { return !tern && (W == 1 || W == 2 || W == 4 || W == 8); }
template <int W, bool TERN>
constexpr bool kPairCacheShape = pair_cache_shape(W, TERN);
// ... and the slots both passes run with when the cache is in use: 4 x 16 queries with one-byte entries up to 64 bits (for codes of at
// most 32 bits that is NOT the geometry the uncached kernels pick, 2 x 32), 8 x 8 queries with two-byte entries beyond
constexpr int cache_slots(int W) { return W <= 2 ? 4 : 8; }
static_assert(slots_for(2, false, 4) == 4 && slots_for(2, false, 8) == 4 && slots_for(4, false, 4) == 8 && slots_for(4, false, 8) == 8 &&
              slots_for(8, false, 4) == 8 && slots_for(8, false, 8) == 8, "33..256 bits: the cache geometry is the uncached kernels' own");
// waves per block: 8 where a wave owns a single query (S = 64), so that 8 queries share each staged gallery batch
constexpr int waves_for(int W, bool tern) { return (W >= 32 && !tern) ? 8 : 1; }
inline size_t aos_ring_bytes(int W, int LW, bool tern) { return (size_t)64 * (((W * (tern ? 2 : 1) + LW) + 3) / 4 * 4) * 4; }

struct WsLayout {
    size_t chunk_hist, below, tot, dpre, cap, tick, gate, ap_part, pair_cache, total;
};

// ---- which kernels take a shape (round 5: one MFMA path + the VALU kernels per code-length band; DESIGN 3.1 has the table) ----------
//   binary, K <= 64        k_scan_hist_r2            one-byte pair cache -> k_scan_ap_c     (no cache: k_scan_ap_r2)
//   binary, 65 .. 128      k_scan_hist_r2w           one-byte pair cache -> k_scan_ap_c<., 8, HALF>; a distance of 128 wraps: stand-in k_scan_ap_s
//   binary, 129 .. 256     k_scan_hist_b             two-byte pair cache -> cached k_scan_ap_s
//   anything else, more than 128 classes, XMH_SCAN_MFMA=0, a failed self-check or lane-order probe: k_scan_hist_s / k_scan_ap_s (VALU)
// One function decides it for a call: scan_route (below), for both passes and for xmh_scan_describe; pass1_family is the part the plan
// depends on.
// k_scan_hist_r2 / r2w keep hazards the compiler cannot see apart by hand (s_nop counts, early-clobber operands, statement order: see
// the kernel), each of which was a wrong result on hardware before it was a comment.  A hipcc or ROCm change could break one of them
// silently, so the kernels have to EARN their place once per device and process: r2_selfcheck_ok runs a small scan (several chunks,
// ties, every geometry; 80 classes, and 128 with pairs whose only common class lies in label words 2 and 3 or that have none: the FP4
// label tile and its denormal chain start) with and without them and compares histograms and divisors bit for bit, AP sums to float rounding; a mismatch
// prints one line to stderr and every later plan of this process uses the VALU kernels, as XMH_SCAN_MFMA=0 does.
// XMH_SCAN_M2_SELFCHECK=0 skips it, =2 runs it and pretends it failed (the test of the fallback); its own evaluations pin the answer
// with Overrides::mfma.
bool r2_selfcheck_ok();
inline bool mfma_env_on() {                              // read per call: the tests compare the two families in one process
    const char* e = getenv("XMH_SCAN_MFMA");
    return !(e && atoi(e) == 0);
}
struct Overrides {            // what internal callers pin instead of the environment, the self-check and the lane-order probe
    int mfma = -1;            // -1: XMH_SCAN_MFMA and the self-check decide; 0: VALU pass 1 (and its plan); 1: the MFMA kernels unchecked (the self-check's own run)
    bool masked = false;      // the kernels that do not rely on the lane order (xmh_scan_verify's re-derivation)
    bool describe = false;    // xmh_scan_describe: lane order assumed (no probe), code words widened to an instance's count as retrieval.widened does
};
// Pass-1 kernel family of a shape.  k_scan_hist_b (xmh_scan_bits.hip, round 3): 129..256-bit binary codes build their MFMA operands from the
// packed bits in registers; counters in the (all << 16 | relevant) form of k_scan_hist_r2.  Compiler-scheduled intrinsics: no hand-kept
// hazard, no self-check.  Round 6: TERNARY codes (up to 256 bits: every length the zero planes exist for) on the same kernel
// (k_scan_hist_b<., ., ., TERN>): the operand is the 2K-bit pair of planes [+1 | -1], 2K + 1 bucket rows, two-byte cache entries -- so
// pass 2 is that of the 129..256-bit binary codes.  Before: the VALU kernels (one exact 0.0 among the code elements cost 2.7 x the binary
// evaluation).
enum class Family { kValu, kR2, kR2w, kBits, kTBits };
Family pass1_family(int K, bool ternary, const Overrides& ov) {
    if (ov.mfma == 0 || !mfma_env_on()) return Family::kValu;
    if (ternary) return K <= 256 ? Family::kTBits : Family::kValu;
    if (K > 128) return K <= 256 ? Family::kBits : Family::kValu;
    if (ov.mfma < 0 && !r2_selfcheck_ok()) return Family::kValu;
    return K <= 64 ? Family::kR2 : Family::kR2w;
}
inline int tbits_tiles(int K) { return K <= 64 ? 2 : (K <= 128 ? 4 : 8); }      // 64-bit tiles of the 2K-bit operand
// k_scan_ap_r2 (round 5): pass 2 evaluates the pairs again on the MFMA from the packed words instead of reading a pair cache (binary codes
// of at most 64 bits whose pass 1 is k_scan_hist_r2).  Measured at Q 5000 x R 117 218 x 64 bit: pass 1 without the cache stores 0.157 ->
// 0.128 ms, pass 2 0.173 (k_scan_ap_c on the cache) -> 0.262 ms, step 0.361 -> 0.416 ms -- so it is the pass 2 of evaluations that HAVE no
// cache (XMH_SCAN_CACHE_MB exceeded or 0, a workspace without room for it), where it replaces the VALU re-evaluation of k_scan_ap_s.
// XMH_SCAN_AP_R2=1 drops the cache for every such shape (the A/B of DESIGN 3.1), =0 never launches it (read per call; a histogram / ap
// call pair must see the same value).
inline int ap_r2_mode() {
    const char* e = getenv("XMH_SCAN_AP_R2");
    return e ? (atoi(e) != 0 ? 1 : 0) : 2;
}
constexpr int kAp2Waves = 4, kAp2Groups = 2;           // k_scan_ap_r2: waves per block x query groups of 16 per wave (66 KB of counters at 65 bucket rows, two
                                                       // blocks per CU; 2 x 2, 1 x 2 and 1 x 1 measured the same 0.262-0.275 ms at the headline shape)
constexpr int kMfmaWaves = 4;                          // k_scan_hist_b: waves (16 queries each) per block
static_assert(xmh::kScanBitsWaves == kMfmaWaves, "k_scan_hist_b takes the plan's query tiles of 64");
// largest chunk of k_scan_hist_b's plan, a multiple of 64.  Round 6: 8064 -> 24192.  The [chunk][bucket][query] tables weigh 257 (513) rows per
// chunk here: on configs[4]'s shard 159 chunks made k_scan_below 0.5 ms and the counter start values 1.7 GB of pass 2's reads; 8064 / 16128 /
// 24192 / 32256: 6.6 / 5.97 / 5.93 / 5.99 ms per step (COCO shape: ternary 128 bit 0.83 -> 0.78, 256-bit binary 0.75 -> 0.72)
constexpr int kBitsMaxChunk = 24192;
// waves per block x query groups of 16 per wave of k_scan_hist_r2 / r2w, and the blocks per CU the chunk count is sized for: codes of at
// most 32 bits have so few buckets that one block of 256 queries per CU measured best (Q 5000 x R 117 218, blocks per CU x rounds: K=16
// 0.416 / 0.350 / 0.367 / 0.352 / 0.368 ms per step for 1 / 2 / 3 / 4 / 6); 33..64 bits: 66 KB of counters per block, two per CU;
// 65..128 bits: 129 bucket rows, two groups per wave (66 KB), two blocks per CU.
struct R2Geom { int nw, nq, blocks_per_cu; int queries() const { return nw * nq * 16; } };
inline R2Geom r2_geom(int K) { return K <= 32 ? R2Geom{4, 4, 1} : (K <= 64 ? R2Geom{4, 4, 2} : R2Geom{4, 2, 2}); }

// Pair cache: binary codes of at most 64 bits and of 65..128 bits (one byte per pair: distance << 1 | relevant) and 129..256 bits (two
// bytes), while it stays under XMH_SCAN_CACHE_MB (default 131072: an MI355X has 288 GB of HBM and up to there the cache still pays --
// the UNSHARDED configs[4] gallery, Q 5000 x R 10 M x 256 bit = 100 GB of entries, runs 89.6 -> 67.3 ms per step with it; 0 = off).
// The VALU kernels write and read the same layouts (k_scan_hist_s / k_scan_ap_s<.., CACHE>: 33..256 bits).
inline long long cache_cap_mb() {
    const char* cap_env = getenv("XMH_SCAN_CACHE_MB");              // read per call
    return cap_env ? atoll(cap_env) : 131072;
}
inline bool ap_c_on() {                                  // XMH_SCAN_AP_C=0: the integer-counter kernels take every pass 2 (tests: the path of galleries beyond 2^23 items)
    const char* e = getenv("XMH_SCAN_AP_C");
    return !(e && atoi(e) == 0);
}
size_t pair_cache_bytes(const xmh_scan_plan& p, int K, bool ternary, Family f) {
    const long long cap_mb = cache_cap_mb();
    const bool tb = f == Family::kTBits;                            // ternary on the MFMA: two-byte entries, 8 slots (as 129..256-bit binary codes)
    if ((ternary && !tb) || K > 256 || cap_mb <= 0 || (!tb && K <= 32 && f != Family::kR2)) return 0;
    if (f == Family::kR2 && ap_r2_mode() == 1) return 0;            // k_scan_ap_r2 evaluates the pairs itself
    const int S = tb ? 8 : (K <= 64 ? 4 : 8);                      // slots of the kernels that use it: 64 / S queries per wave
    // records of 64 lanes per (chunk, tile of 64 / S queries, batch of 64 items): 16 B per lane for one-byte entries (S = 4), 12 B per lane for the
    // 12-bit entries of longer and of ternary codes (S = 8; xmh_common.h) -- 65..128-bit codes whose one-byte entries k_scan_hist_r2w writes use
    // two thirds of that region
    const size_t bytes = (size_t)p.nchunk * (size_t)(p.nqtile * S) * (size_t)((p.chunk + 63) / 64) * (S == 4 ? 1024 : 64 * 4 * xmh::kCache12Dwords);
    return bytes <= (size_t)cap_mb << 20 ? bytes : 0;
}

WsLayout ws_layout(const xmh_scan_plan& p, size_t cache_bytes) {
    WsLayout L;
    const size_t cells = (size_t)p.nchunk * p.nbuckets * p.qpad;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += (bytes + 255) & ~(size_t)255;
        return at;
    };
    L.chunk_hist = take(cells * 4);
    L.below = take(cells * 8);
    L.tot = take((size_t)p.nbuckets * p.qpad * 8);
    L.dpre = take((size_t)p.nbuckets * p.qpad * 8);
    L.cap = take((size_t)p.qpad * 4);
    L.tick = take((size_t)p.nqtile * 4);     // k_scan_below tickets, one per 64-query tile; ends where `gate` starts: one memset clears both
    L.gate = take(256 + 8 * 4096);           // [0]: nrel_max gate word, [1]: finalize ticket, +256: per-block partial sums (<= 4096 blocks)
    L.ap_part = take((size_t)p.nchunk * p.qpad * 4);
    L.pair_cache = take(cache_bytes);        // LAST: a workspace that ends in front of it is a workspace without a cache (cache_for_workspace)
    L.total = o;
    return L;
}

// The cache a call may use given the workspace it was handed: the plan's, or none when the caller's buffer ends in front of it (a device
// that has no room for Q x R bytes next to a resident encoder: xmh_scan_ws_bytes_nocache).  Both calls of a pair see the same ws_bytes
// and so take the same decision -- no process-wide state (round 4 lowered XMH_SCAN_CACHE_MB in the environment for this: ADVICE r4).
size_t cache_for_workspace(const xmh_scan_plan& p, int K, bool ternary, Family f, size_t ws_bytes) {
    const size_t c = pair_cache_bytes(p, K, ternary, f);
    return c && ws_bytes < ws_layout(p, c).total ? 0 : c;
}

int make_plan(int64_t Q, int64_t R, int K, int ternary, xmh_scan_plan* p, const Overrides& ov = {}) {
    if (Q <= 0 || R <= 0 || K <= 0) return xmh::fail(XMH_EINVAL, "scan plan: bad shape Q=%lld R=%lld K=%d", (long long)Q, (long long)R, K);
    if (R >= (1ll << 24) || Q >= (1ll << 24)) return xmh::fail(XMH_ENOTSUP, "scan plan: shard too large (R=%lld, Q=%lld)", (long long)R, (long long)Q);
    const int64_t nb = ternary ? 2 * (int64_t)K + 1 : (int64_t)K + 1;
    const int Wd = (K + 31) / 32;
    if (Wd > 64 || (ternary && Wd > 8))
        return xmh::fail(XMH_ENOTSUP, "scan plan: K=%d%s (at most 2048 code bits, 256 with zero planes)", K, ternary ? " ternary" : "");
    const int S64 = slots_for(instance_words(Wd), ternary != 0, 8);
    const int64_t lds_ap = nb * (64 / S64) * 8;
    if (lds_ap > 150 * 1024) return xmh::fail(XMH_ENOTSUP, "scan plan: %lld distance buckets need %lld B of LDS per wave; K=%d%s", (long long)nb, (long long)lds_ap, K, ternary ? " ternary" : "");
    const Family fam = pass1_family(K, ternary != 0, ov);
    const bool r2 = fam == Family::kR2 || fam == Family::kR2w;
    int64_t nqt = xmh::ceil_div(Q, 64);
    const int r2q = r2_geom(K).queries();
    if (r2) {                                     // whole blocks of k_scan_hist_r2 AND whole 64-query tiles
        int64_t l = r2q;
        while (l % 64) l += r2q;
        nqt = xmh::ceil_div(nqt * 64, l) * l / 64;
    }
    const int64_t wpc = 8;                        // resident waves per CU the VALU kernels are sized for (two per SIMD)
    // one chunk x 64-query tile per resident wave slot (`rounds` sets of them); slotted kernels run S waves per tile
    const int64_t slots = (int64_t)xmh::device_cu_count() * wpc;
    // two resident sets of waves balance the tail better, but the [chunk][bucket][query] tables double: pays up to 65 buckets
    // (K=64: 0.640 -> 0.624 ms, K=16: 0.502 -> 0.476), costs at 257 (K=256: 1.45 -> 1.54); with the pair cache (33..64 bits) the passes
    // are shorter and the tables weigh more: one set (0.543 -> 0.536 ms); codes of 32 bits and less: three sets
    const bool cache_shape = !ternary && K > 32 && K <= 64 && cache_cap_mb() > 0;
    const int64_t rounds = nb <= 33 ? 3 : (nb <= 65 && !cache_shape ? 2 : 1);
    int64_t nchunk = rounds * slots / nqt;
    if (S64 > 8) nchunk = nchunk * 8 / S64;       // long codes: S waves per tile already fill the slots; fewer chunks = smaller tables
    const bool mfma = fam != Family::kValu;
    bool fill = false;                            // the chunk count is kept as computed instead of rounded to whole groups of 8
    if (mfma) {
        // k_scan_hist_b: 257 (513) bucket rows: three sets of blocks (COCO shape, sets 2 / 3 / 4 / 6: ternary 128 bit 0.93 / 0.78 / 0.83 / 0.83 ms, 256-bit
        // binary 0.85 / 0.73 / 0.75 / 0.76); ternary codes of at most 64 bits have 129 rows and smaller tables: six (0.65 -> 0.62 ms)
        int64_t bsets = nb <= 129 ? 6 : 3;
        if (const char* e = xmh_experiment_env("XMH_BITS_SETS")) bsets = atoi(e) > 0 ? atoi(e) : bsets;
        nchunk = bsets * xmh::device_cu_count() / nqt;
        if (r2) {                                 // blocks of r2q queries, blocks_per_cu of them per CU, `sets` sets of them
            int sets = K > 32 && K <= 64 ? 1 : 2;                   // k_scan_hist_r2 at 33..64 bits: one set (1 / 2 / 3: 0.178 / 0.187 / 0.199 ms)
            if (const char* e = xmh_experiment_env("XMH_R2_SETS")) sets = atoi(e) > 0 ? atoi(e) : sets;
            nchunk = (int64_t)sets * xmh::device_cu_count() * r2_geom(K).blocks_per_cu / (nqt * 64 / r2q);
            // XMH_R2_FILL=1 (round 8, measured and NOT the default): k_scan_hist_r2 at 33..64 bits with a pair cache, one set, keeps the chunk
            // count as computed -- every block slot filled.  All blocks of the launch are resident and run in lockstep, so pass 1 takes one
            // block's time, and the rounding below leaves slots idle: Q 5000 x R 117 218 on 256 CUs is 20 query blocks, 512 slots, 25 chunks
            // of 4736 (74 batches) against 24 of 4928 (77); the 25th chunk's blocks are dealt over the XCDs (xmh_scan_map.h).  24 / 25
            // chunks: pass 1 0.1732-0.1740 / 0.1692-0.1706 ms in the ablation harness, the step 0.3346-0.3385 / 0.3328-0.3354 ms: 1.8 us
            // at the medians, inside the spread of either (profiles/r08_scan_fill.txt).  Not worth moving every chunk boundary for: the
            // per-chunk fp32 partial sums of pass 2 then add in another order than the ones every recorded result was computed with
            if (const char* e = xmh_experiment_env("XMH_R2_FILL")) fill = atoi(e) != 0 && fam == Family::kR2 && sets == 1 && cache_shape && ap_r2_mode() != 1;
        }
    }
    if (nchunk < 1) nchunk = 1;
    if (nchunk > 8 && !fill) nchunk = (nchunk + 4) / 8 * 8;      // whole XCD groups: every XCD gets the same number of chunks
    int64_t chunk = xmh::ceil_div(R, nchunk);
    if (chunk < kMinChunk) chunk = kMinChunk;
    if (chunk > kMaxChunk) chunk = kMaxChunk;
    chunk = xmh::ceil_div(chunk, 8) * 8;
    if (mfma) {                                   // batches of 64 items
        chunk = xmh::ceil_div(chunk, 64) * 64;
        int64_t bits_max = kBitsMaxChunk;
        if (const char* e = xmh_experiment_env("XMH_BITS_MAX_CHUNK")) bits_max = atoll(e) / 64 * 64 > 0 ? atoll(e) / 64 * 64 : bits_max;
        if (!r2 && chunk > bits_max) {                              // capped: whole XCD groups of equal chunks again
            nchunk = xmh::ceil_div(xmh::ceil_div(R, bits_max), 8) * 8;
            chunk = xmh::ceil_div(xmh::ceil_div(R, nchunk), 64) * 64;
        }
    }
    nchunk = xmh::ceil_div(R, chunk);
    p->chunk = chunk;
    p->nchunk = nchunk;
    p->nqtile = nqt;
    p->qpad = nqt * 64;
    p->nbuckets = nb;
    p->ws_bytes = ws_layout(*p, pair_cache_bytes(*p, K, ternary != 0, fam)).total;
    return XMH_OK;
}

// 1 if same-address returning LDS adds of one instruction come back in ascending lane order on this device (probed once
// per process with a 1-wave kernel and one blocking copy), 0 otherwise or when XMH_SCAN_MASKED is set
int lane_order_ok(hipStream_t st) {
    static int cached[64];
    static bool have[64];
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (getenv("XMH_SCAN_MASKED") != nullptr) return 0;           // read per call: the self-check test runs both paths in one process
    std::lock_guard<std::mutex> lock(mu);
    if (have[dev]) return cached[dev];
    int ok = 0;
    {
        // per DEVICE (not per process: a process may drive several), two probes: one wave alone, every counter geometry; then pass 2's own
        // geometry under load beside matrix waves (k_probe_lane_order_load).  Both must hold.
        const char* fe = getenv("XMH_SCAN_PROBE_FAULT");          // test hook, read once per device: expect an order no device serves
        const int fault = fe && atoi(fe) != 0;
        uint32_t* flag = nullptr;
        float* sink = nullptr;
        if (hipMalloc(&flag, 8) == hipSuccess && hipMalloc(&sink, 256) == hipSuccess) {
            uint32_t h[2] = {0, 1};
            int cus = xmh::device_cu_count();
            if (hipMemsetAsync(flag, 0, 8, st) == hipSuccess) {
                hipLaunchKernelGGL(k_probe_lane_order, dim3(1), dim3(64), 0, st, flag);
                hipLaunchKernelGGL(k_probe_lane_order_load, dim3((unsigned)(cus * 25)), dim3(64), 0, st, flag + 1, fault, sink);
                if (hipGetLastError() == hipSuccess && hipMemcpyAsync(h, flag, 8, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess)
                    ok = h[0] == 1u && h[1] == 0u;
            }
        }
        if (flag) (void)hipFree(flag);
        if (sink) (void)hipFree(sink);
        if (!ok)
            fprintf(stderr, "xmh: the lane-order probe FAILED on device %d%s: same-address returning LDS adds are not served in lane order here; "
                            "pass 2 runs the masked kernels (about 2x slower, same results).\n", dev, fault ? " (XMH_SCAN_PROBE_FAULT set: forced)" : "");
    }
    cached[dev] = ok;
    have[dev] = true;
    return ok;
}

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(size_t n) { return hipMalloc(&p, n) == hipSuccess; }
    template <typename T> T* as() { return static_cast<T*>(p); }
};

template <bool TERN, typename F>
int dispatch_shape(int W, int LW, F&& f) {
#define XMH_CASE(WW, LL) \
    if (W == WW && LW == LL) return f(std::integral_constant<int, WW>{}, std::integral_constant<int, LL>{});
    XMH_CASE(1, 1) XMH_CASE(1, 2) XMH_CASE(1, 3) XMH_CASE(1, 4)
    XMH_CASE(2, 1) XMH_CASE(2, 2) XMH_CASE(2, 3) XMH_CASE(2, 4)
    XMH_CASE(4, 1) XMH_CASE(4, 2) XMH_CASE(4, 3) XMH_CASE(4, 4)
    XMH_CASE(8, 1) XMH_CASE(8, 2) XMH_CASE(8, 3) XMH_CASE(8, 4)
    if constexpr (!TERN) {                                 // 129 ... 256 classes (IAPR TC-12 has 255) as EIGHT label words: binary codes up to 256 bits,
        XMH_CASE(1, 8) XMH_CASE(2, 8) XMH_CASE(4, 8) XMH_CASE(8, 8)      // the VALU kernels; callers with 5 ... 7 words pad to 8 (Python: RankingScan does)
    }
    if constexpr (!TERN) {                                 // long binary codes
        XMH_CASE(16, 1) XMH_CASE(16, 2) XMH_CASE(16, 3) XMH_CASE(16, 4)
        XMH_CASE(32, 1) XMH_CASE(32, 2) XMH_CASE(32, 3) XMH_CASE(32, 4)
        XMH_CASE(64, 1) XMH_CASE(64, 2) XMH_CASE(64, 3) XMH_CASE(64, 4)
    }
#undef XMH_CASE
    return xmh::fail(XMH_ENOTSUP, "scan: unsupported shape W=%d code words (K in {<=32,64,128,256}, binary also 512,1024,2048), Lw=%d label words (C<=128; binary codes up to 256 bits also exactly 8 words: 129..256 classes)%s",
                     W, LW, TERN ? ", ternary" : "");
}

// Width of the rank field of the packed 32-bit pass-2 counters for an UNSHARDED evaluation of this shape, 0 = only the 64-bit kernels
// are launched.
int packed_rank_bits(int K, int64_t R) {
    // XMH_SCAN_PACK32: "0" = never, "all" = every code length (tests); default: from 65 bits on (measured at Q 5000 x R 117 218, sparse
    // relevance, pass 2 packed / 64-bit: K=16 0.275 / 0.251 ms, K=32 0.278 / 0.253, K=64 0.199 / 0.195, K=128 0.274 / 0.286, K=256 0.347 / 0.412)
    const char* e = getenv("XMH_SCAN_PACK32");
    if (e && e[0] == '0') return 0;
    if (!(K > 64 || (e && e[0] == 'a'))) return 0;
    const int64_t rank_max = R + 2;
    int rank_bits = 0;
    while ((1ll << rank_bits) < rank_max) ++rank_bits;
    return rank_bits > 24 ? 0 : rank_bits;
}

// ---- the route of a call: every kernel instance of both passes, decided in one place ---------------------------------------------
// xmh_hamming_hist, hamming_ap_impl and xmh_scan_describe all read it: pass 2 reads a pair cache exactly when pass 1 wrote one, and the
// kernel name the bench looks up in a profile is the kernel that ran (a separate mirror had drifted from the launches twice).
// The launchers take slots, waves and geometry from the record (launch_geom) and refuse an instance that differs from it (start).
// Mode: where pass 2's offsets come from -- k_scan_below of the same workspace (unsharded), the caller (xmh_hamming_ap's base_all), the
// gathered totals tables of the shards (xmh_hamming_map_sharded), the all-to-all slices (xmh_hamming_map_sharded_offsets).
enum class Mode { kUnsharded, kBaseAll, kTotals, kAllToAll };
// The operands of one evaluation as every entry point receives them: built once there, read by everything below.
struct ScanCall {
    const uint32_t *qbits, *qzero, *qlab, *rbits, *rzero, *rlab;
    int64_t Q, R; int K, C;
    void* ws; size_t ws_bytes;
    bool tern;                      // zero planes given (check_common: for both sides or neither)
};
// ... and what pass 2 takes beyond them: the entry point names the mode and the outputs, then the inputs of its mode
struct Pass2 {
    Mode mode; int64_t k;
    double* ap_sum; int32_t* cap;
    double* map_out;                                     // null: sums and divisors only
    const uint32_t *base_all = nullptr, *base_rel = nullptr, *nrel_total = nullptr;      // kBaseAll: the caller's offsets (all three or none)
    const uint32_t* hist_g = nullptr;                    // kTotals: the gathered totals tables of the shards; kAllToAll: this shard's offset slices
    int world = 0, rank = 0;                             // (kAllToAll reads no rank: the slices are this shard's own)
};
enum class Kern { kHistS, kHistR2, kHistR2w, kHistB, kApS, kApC, kApR2 };
// device words that make a pass-2 launch return at once because another launch of the call takes the work
enum Gate : unsigned {
    kBySize = 1,     // the gallery size over all shards (word 2, from the offsets kernels): float-bit counters or the k_scan_ap_s behind them
    kByWrap = 2,     // kGateWrapped: k_scan_hist_r2w wrapped a distance of 128 in a one-byte entry; k_scan_ap_c returns, its stand-in runs
    kByWidth = 4,    // nrel_max against rank_bits: exactly one of the packed 32-bit and the 64-bit counter launches runs
};
struct Launch {                     // one kernel instance, template arguments as xmh_scan_describe prints them
    Kern kern = Kern::kHistS;
    int W = 0, LW = 0;              // code / label words the launch dispatches on (dispatch_shape)
    bool tern = false, cache = false;
    int S = 0, NW = 1;              // VALU kernels and k_scan_ap_c: slots, waves per block; k_scan_hist_r2 / r2w / ap_r2: query groups per wave, waves; k_scan_hist_b: code tiles
    int nml = 0;                    // k_scan_hist_r2 / r2w / ap_r2: the label tile (1: i8, at most 64 classes; 2: FP4, 65-128 classes)
    int eb = 0; bool half = false;  // k_scan_ap_c: entry bits (8: one byte, 16: the 12-bit entries of the two-byte layout); 8 slots x 8 queries on one-byte entries
    bool p32 = false, masked = false;
    unsigned gate = 0;
    bool stand_in = false;          // launched behind k_scan_ap_c for wrapped entries (it runs once in a blue moon): not described
};
struct ScanRoute {
    Launch p1;
    size_t cache_bytes = 0;         // the pair cache pass 1 writes and pass 2 reads; 0 = none
    int rank_bits = 0;              // rank field of the packed pass-2 counters handed to the launches (0: 64-bit counters only)
    Launch p2[3];                   // pass 2 in launch order
    int n2 = 0;
    bool tables32 = false;          // k_scan_below leaves the packed `below` table (xmh_scan_kernels.h) and k_scan_ap_c reads it: tables_packed
};

// THE RULE FOR THE PACKED `below` TABLE (one uint32 per cell, all << 16 | relevant, instead of a uint2): k_scan_below writes it and pass 2 reads
// it exactly when (1) the call is Mode::kUnsharded, (2) the pass 2 behind this xmh_hamming_hist is k_scan_ap_c ALONE -- one launch, no device
// word that hands the call to another kernel: in practice k_scan_ap_c<., 8, false>, codes of at most 64 bits with a pair cache -- and (3) the
// host expects every bucket total of the shard to fit 16 bits.  Everything else keeps the 64-bit table: the caller-offsets, totals and
// all-to-all modes, every route that launches k_scan_ap_s or k_scan_ap_r2, the routes where a device word picks one of two launches.
// (3) is an estimate, the device decides (kGateWide): the fullest bucket of uniformly random K-bit codes holds R * C(K, K / 2) / 2^K items of
// a query -- a tenth of the shard at 64 bits, a fifth at 16 -- and the table is packed while TWICE that fits, so that codes whose distances
// are twice as concentrated as random ones still take the fast path; R / nbuckets > 65 535, where no shard can fit, is implied.  Headline
// (117 218 x 64 bit): 11 645 -> packed.  16-bit codes on a shard of a million rows: 196 381 -> 64-bit table, not a fallback on every call.
// The factor of two is a margin chosen by reasoning, not a measured one: no gallery of real codes was profiled for it.
// WHO SAYS WHICH PASS 2 FOLLOWS.  xmh_hamming_hist cannot see it, so the caller says it: xmh_hamming_hist_for(..., pass2_sharded), and plain
// xmh_hamming_hist takes a call that exports its histograms (what a sharded evaluation gathers) for a sharded one.  A sharded pass 1 leaves
// the 64-bit table, so the sharded step has the launches and the table it had.  A caller that says one thing and does the other is still
// served: the host remembers per workspace which form the last pass 1 left (g_packed_ws below; calls on one workspace are in stream order,
// one stream at a time), and a pass 2 that finds the other form than its route reads either takes the 64-bit table as it is (k_scan_ap_c
// reads both) or, for the kernels that read only the 64-bit one, writes it again first (hamming_ap_impl: one launch more, on that mismatch
// only -- a pass 2 under another XMH_SCAN_* setting than its pass 1, a sharded pass 2 behind a pass 1 that was not told).
// ROUND 11, THE PACKED TABLE WITHOUT k_scan_below's TAIL.  Where the packed rule holds and the call exports no histograms, k_scan_below runs
// without tickets and leaves `below` (packed) and the totals only: no dpre, no nrel row, no nrel_max word.  k_scan_ap_c makes the first two from
// the totals in its prologue (nrel_out, xmh_scan_mfma.h) and nothing on that route reads the third.  The host remembers that as well, and a
// pass 2 of any other kind on such a workspace first gets the table kernels in their full form: the ticket words cleared, then k_scan_below
// with tickets, the 64-bit table and its tail (hamming_ap_impl) -- on that mismatch only, and the same values as if pass 1 had been told.
enum class Tables { k64, kPacked, kPackedNoTail };        // what the last pass 1 left: 64-bit `below` + tail; packed `below` + tail; packed, no tail
std::mutex g_packed_mu;
std::unordered_map<const void*, Tables> g_packed_ws;      // workspaces whose `below` table is in the packed form
Tables ws_tables(const void* ws) {
    std::lock_guard<std::mutex> lock(g_packed_mu);
    const auto it = g_packed_ws.find(ws);
    return it == g_packed_ws.end() ? Tables::k64 : it->second;
}
void ws_set_tables(const void* ws, Tables t) {
    std::lock_guard<std::mutex> lock(g_packed_mu);
    if (t == Tables::k64) g_packed_ws.erase(ws); else g_packed_ws[ws] = t;
}
bool counts_fit16(int K, int64_t R) {
    double peak = 1.0;                                    // C(K, K / 2) / 2^K
    for (int i = 1; i <= K / 2; ++i) peak *= (double)(K - K / 2 + i) / (double)i;
    peak = ldexp(peak, -K);
    return 2.0 * peak * (double)R <= 65535.0;
}
bool tables_packed(bool apc_alone, Mode mode, int K, int64_t R) { return apc_alone && mode == Mode::kUnsharded && counts_fit16(K, R); }

ScanRoute scan_route(const xmh_scan_plan& p, const ScanCall& c, Mode mode, const Overrides& ov, hipStream_t st) {
    ScanRoute r;
    const int K = c.K, C = c.C; const bool tern = c.tern; const int64_t R = c.R;
    const Family fam = pass1_family(K, tern, ov);
    const int W = ov.describe ? instance_words((K + 31) / 32) : (K + 31) / 32, LW = (C + 31) / 32;
    const bool lane_ok = ov.describe || (!ov.masked && lane_order_ok(st));
    r.cache_bytes = cache_for_workspace(p, K, tern, fam, c.ws_bytes);
    const bool cache = r.cache_bytes != 0;
    const bool mfma = fam != Family::kValu && LW <= 4 && lane_ok;          // pass 1 on the matrix cores
    Launch& h = r.p1;
    h.W = W; h.LW = LW; h.tern = tern; h.cache = cache; h.nml = LW <= 2 ? 1 : 2;
    if (!mfma) {
        h.cache = cache && pair_cache_shape(W, tern);
        h.S = h.cache ? cache_slots(W) : slots_for(W, tern, 4);
        h.NW = h.S == 64 ? waves_for(W, tern) : 1;
    } else if (fam == Family::kBits || fam == Family::kTBits) {
        h.kern = Kern::kHistB;
        h.S = fam == Family::kTBits ? tbits_tiles(K) : 4;
    } else {
        const R2Geom g = r2_geom(K);
        h.kern = fam == Family::kR2 ? Kern::kHistR2 : Kern::kHistR2w;
        h.NW = g.nw; h.S = g.nq;
    }
    const bool sharded = mode != Mode::kUnsharded;
    const bool masked = !lane_ok;
    const int rank_bits = sharded || masked ? 0 : packed_rank_bits(K, R);   // (the masked fallback has 64-bit counters only)
    const bool fits_fb = sharded || R <= kFloatBitsMaxItems;               // float-bit counters: sharded, the size word decides on the device
    const bool apc_on = ap_c_on();
    // 65..128-bit codes whose pass 1 left ONE-byte entries (k_scan_hist_r2w): k_scan_ap_c reads them like those of shorter codes, 8 slots x 8
    // queries wide; the cached k_scan_ap_s cannot.  A distance of 128 does not fit a byte and wrapped; pass 1 raised a control word then,
    // k_scan_ap_c returns at once and the kernel that evaluates the pairs from the codes (the stand-in, gated the other way) takes the call.
    const bool byte128 = cache && mfma && fam == Family::kR2w;
    // ternary codes whose pass 1 left two-byte entries: the cached pass-2 kernels read nothing but the entries and the tables, so the BINARY
    // 256-bit instances serve (the bucket count comes from the plan)
    const bool tb = cache && mfma && fam == Family::kTBits;
    // k_scan_ap_c (float-bit counters): pair cache, 64-bit counters, lane order, and the gallery over ALL shards small enough; the caller-
    // offsets form stays on k_scan_ap_s except on one-byte entries of 65..128-bit codes (k_scan_dpre leaves the largest rank in the word)
    const bool apc = cache && apc_on && (byte128 || (K <= 64 && rank_bits == 0)) && !tern && !masked && (mode != Mode::kBaseAll || byte128) && fits_fb;
    // k_scan_ap_r2: no pair cache, the pairs evaluated again on the MFMA from the packed words
    const bool apr2 = !cache && mfma && fam == Family::kR2 && ap_r2_mode() != 0 && !masked && mode != Mode::kBaseAll && rank_bits == 0 && fits_fb;
    // Round 6: 129..256-bit codes (two-byte entries) on k_scan_ap_c<., 16>, the 64-bit pass 2 of unsharded calls.  Where the shard is too large
    // or too relevant for packed 32-bit counters -- configs[4]: a shard of 1.25 M rows, 150 k relevant items per query -- it replaced the
    // integer-counter k_scan_ap_s (15 VALU instructions per pair; k_scan_ap_c: 9)
    const bool apc16 = cache && apc_on && ((K > 128 && K <= 256 && !tern) || tb) && !masked && !sharded && R <= kFloatBitsMaxItems;
    const unsigned size_gate = sharded && (apc || apr2) ? kBySize : 0u;
    r.rank_bits = byte128 && apc ? 0 : rank_bits;                           // behind k_scan_ap_c<., 8, true> only the 64-bit stand-in
    auto add = [&](Kern kern, unsigned gate) -> Launch& { Launch& l = r.p2[r.n2++]; l.kern = kern; l.gate = gate; return l; };
    if (apc) {
        Launch& l = add(Kern::kApC, size_gate | (byte128 ? kByWrap : 0u));
        l.eb = 8; l.half = byte128; l.S = byte128 ? 8 : 4;
    }
    if (apr2) {
        Launch& l = add(Kern::kApR2, size_gate);
        l.W = W; l.LW = LW; l.nml = h.nml; l.NW = kAp2Waves; l.S = kAp2Groups;
    }
    if (apc16) {
        Launch& l = add(Kern::kApC, kByWidth);
        l.eb = 16; l.S = 8;
    }
    if ((apc || apr2) && !size_gate && !byte128) {                          // k_scan_ap_c / k_scan_ap_r2 alone takes the call
        r.tables32 = tables_packed(apc, mode, K, R);
        return r;
    }
    Launch s;                                                               // k_scan_ap_s: both counter widths where packed ones apply
    s.kern = Kern::kApS; s.W = tb ? 8 : W; s.LW = LW; s.tern = tern && !tb; s.masked = masked;
    s.cache = cache && !byte128 && !masked && pair_cache_shape(s.W, s.tern);
    s.stand_in = byte128 && apc;
    s.gate = size_gate | (s.stand_in ? kByWrap : 0u) | (r.rank_bits ? kByWidth : 0u);
    for (const bool p32 : {true, false}) {
        if (p32 ? r.rank_bits == 0 : apc16) continue;                       // (k_scan_ap_c<., 16> is the 64-bit pass 2 of that shape)
        s.p32 = p32;
        s.S = s.cache ? cache_slots(s.W) : slots_for(s.W, s.tern, p32 ? 4 : 8);
        s.NW = s.S == 64 ? waves_for(s.W, s.tern) : 1;
        r.p2[r.n2++] = s;
    }
    return r;
}

// a launch of the route as rocprofv3 prints the instance (minus the namespace) for an uncapped call; XMH_ENOTSUP where dispatch_shape has none
int describe_launch(const Launch& l, char* out, size_t n) {
    static const char* const tf[2] = {"false", "true"};
    auto exists = [&](auto tern_c) { return dispatch_shape<decltype(tern_c)::value>(l.W, l.LW, [](auto, auto) { return (int)XMH_OK; }); };
    switch (l.kern) {
    case Kern::kHistS:
    case Kern::kApS:
        if (const int rc = l.tern ? exists(std::true_type{}) : exists(std::false_type{})) return rc;
        if (l.kern == Kern::kHistS) snprintf(out, n, "k_scan_hist_s<%d, %d, %s, %d, %d, %s>", l.W, l.LW, tf[l.tern], l.S, l.NW, tf[l.cache]);
        else                                // the cached kernel reads no label word; the uncached ones exist in the capped form only
            snprintf(out, n, "k_scan_ap_s<%d, %d, %s, %s, %d, %s, %s, %d, %s>", l.W, l.cache ? 1 : l.LW, tf[l.tern], tf[!l.cache], l.S, tf[l.p32], tf[l.masked],
                     l.NW, tf[l.cache]);
        break;
    case Kern::kHistR2:
    case Kern::kHistR2w:
        snprintf(out, n, "k_scan_hist_%s<%d, %d, %d, %s>", l.kern == Kern::kHistR2 ? "r2" : "r2w", l.nml, l.NW, l.S, tf[l.cache]);
        break;
    case Kern::kHistB: {
        int nsh, nqt;
        xmh::scan_hist_bits_shape(l.S, l.tern, &nsh, &nqt);
        snprintf(out, n, "k_scan_hist_b<%d, %d, %d, %d, %s, %s>", l.S, kMfmaWaves, nsh, nqt, tf[l.cache], tf[l.tern]);
        break;
    }
    case Kern::kApC: snprintf(out, n, "k_scan_ap_c<false, %d, %s>", l.eb, tf[l.half]); break;
    case Kern::kApR2: snprintf(out, n, "k_scan_ap_r2<%d, %d, %d, false>", l.nml, l.NW, l.S); break;
    }
    return XMH_OK;
}

int check_common(const char* who, const ScanCall& c, const xmh_scan_plan& p) {
    if (!c.qbits || !c.rbits || !c.qlab || !c.rlab || !c.ws) return xmh::fail(XMH_EINVAL, "%s: null pointer", who);
    if ((c.qzero == nullptr) != (c.rzero == nullptr)) return xmh::fail(XMH_EINVAL, "%s: zero masks must be given for both sides or neither", who);
    if (c.C <= 0) return xmh::fail(XMH_EINVAL, "%s: C=%d", who, c.C);
    const size_t need = ws_layout(p, 0).total;                       // at least the plan without its pair cache (xmh_scan_ws_bytes_nocache)
    if (c.ws_bytes < need) return xmh::fail(XMH_EINVAL, "%s: workspace too small (%zu < %zu; %zu with the pair cache)", who, c.ws_bytes, need, (size_t)p.ws_bytes);
    return XMH_OK;
}

ScanArgs make_args(const ScanCall& c, const xmh_scan_plan& p) {
    return ScanArgs{c.qbits, c.qzero, c.qlab, c.rbits, c.rzero, c.rlab, (int)c.Q, (int)c.R, c.K, (int)p.chunk, (int)p.nchunk, (int)p.nqtile, (int)p.qpad,
                    (int)p.nbuckets, nullptr, (int)p.nqtile};
}

MfmaArgs r2_args(const ScanCall& c, const Launch& l, const xmh_scan_plan& p, int nqt) {
    MfmaArgs a{c.qbits, (int)c.Q, (int)c.R, c.K, l.W, (int)p.chunk, (int)p.nchunk, nqt, (int)p.nbuckets, (int)p.qpad};
    a.rbits = c.rbits; a.rlab = c.rlab; a.qlab = c.qlab; a.LW = l.LW;
    return a;
}

// ---- the geometry of a launch: what a Launch record means on a plan, for every launcher ------------------------------------------
// nqt = query tiles of the kernel: a slotted wave owns 64 / S queries and a block NW waves; a block of k_scan_hist_r2 / r2w / ap_r2 owns NW x S
// groups of 16, one of k_scan_hist_b kMfmaWaves groups.  nrun = the tiles the launch runs: pass 1 all of them (it writes the padded tiles' cache
// entries and table columns: in a pass whose blocks run in lockstep they cost nothing), pass 2 only those that hold a query -- Q 5000 is padded
// to 5120 for pass 1's blocks of 256, and seven of pass 2's 320 tiles of 16 would load their counters and stream their pair cache for sums
// that nothing reads.  The layouts keep the padded count.  Grid (xmh_scan_map.h): tiles run x chunks.  LDS: the counters of a block -- u32 per
// (bucket, query) in pass 1 and the packed pass 2, two words otherwise, 16 B-rounded per wave in the VALU kernels -- plus their gallery ring.
struct Geom { unsigned grid, block; size_t lds; int nqt, nrun; };
Geom launch_geom(const Launch& l, const xmh_scan_plan& p, int64_t Q) {
    const size_t nb = (size_t)p.nbuckets;
    const bool ap = l.kern == Kern::kApS || l.kern == Kern::kApC || l.kern == Kern::kApR2;
    Geom g{0, 64u * (unsigned)l.NW, 0, 0};
    if (l.kern == Kern::kHistS || l.kern == Kern::kApS) {
        g.lds = ((nb * (64 / l.S) * (ap && !l.p32 ? 2 : 1) + 3) & ~(size_t)3) * 4 * l.NW + (ap && l.cache ? 0 : aos_ring_bytes(l.W, l.LW, l.tern));
        g.nqt = (int)p.nqtile * l.S / l.NW;
    } else if (l.kern == Kern::kApC) {
        g.lds = nb * (64 / l.S) * 8; g.nqt = (int)p.nqtile * l.S;
    } else if (l.kern == Kern::kHistB) {                 // (grid and LDS are launch_scan_hist_bits' own: xmh_scan_bits.hip)
        g.nqt = (int)(p.qpad / (16 * kMfmaWaves));
    } else if (l.kern == Kern::kHistR2 || l.kern == Kern::kHistR2w) {      // tables of bucket rows x 512 B, two query groups of every wave each (xmh_scan_mfma.h, r2_cell)
        g.lds = r2_lds_bytes(l.S, (int)nb); g.nqt = (int)(p.qpad / (l.NW * l.S * 16));
    } else {
        g.lds = (size_t)l.NW * l.S * nb * 16 * (ap ? 8 : 4); g.nqt = (int)(p.qpad / (l.NW * l.S * 16));
    }
    g.nrun = g.nqt;
    if (ap) {
        static const bool all_tiles = xmh_experiment_env("XMH_AP_TILES") && atoi(xmh_experiment_env("XMH_AP_TILES")) == 0;      // A/B switch: 0 = the padded tiles too
        if (!all_tiles) g.nrun = (int)xmh::ceil_div(Q, p.qpad / g.nqt);
    }
    g.grid = xmh::scan_grid_blocks(g.nrun, (int)p.nchunk);
    return g;
}

// Starts `kern` as the instance of record `l`.  S, NW and cache are what the instance was compiled with -- constexpr functions of the
// dispatched shape (slots_for, cache_slots, waves_for) or constants of a kernel family (r2_geom, kAp2Waves x kAp2Groups, k_scan_ap_c's slots):
// where they differ from the record the route filled and xmh_scan_describe prints, nothing is launched.
template <typename KernT, typename... Args>
int start(const char* who, const Launch& l, const Geom& g, hipStream_t st, KernT kern, int S, int NW, bool cache, Args... args) {
    if (l.S != S || l.NW != NW || l.cache != cache)
        return xmh::fail(XMH_ENOTSUP, "%s: the route names an instance with S=%d NW=%d cache=%d, the one compiled for W=%d LW=%d has S=%d NW=%d cache=%d", who, l.S,
                         l.NW, (int)l.cache, l.W, l.LW, S, NW, (int)cache);
    if (const int rc = xmh::raise_dynamic_lds(reinterpret_cast<const void*>(kern), g.lds, who)) return rc;
    hipLaunchKernelGGL(kern, dim3(g.grid), dim3(g.block), g.lds, st, args...);
    return XMH_OK;
}

// ---- what the stages of one call share: plan_call fills the plan and checks the operands, route_call the rest -------------------------
struct ScanCtx {
    const ScanCall& c;
    hipStream_t st;
    xmh_scan_plan p;
    ScanRoute r;
    WsLayout L;
    ScanArgs a;                                          // on the plan's tiles of 64 queries; args(): with a launch's own nqt and the pair cache
    uint32_t kcap = 0xffffffffu;                         // pass 2: k as the kernels take it (none: no ordinal exceeds it) and whether the call has one
    bool capped = false;
    bool no_tail = false;                                // pass 2 on a workspace without dpre / nrel (Tables::kPackedNoTail): k_scan_ap_c makes them from the totals
    template <typename T> T* at(size_t off) const { return reinterpret_cast<T*>(static_cast<char*>(c.ws) + off); }
    uint32_t* chunk_hist() const { return at<uint32_t>(L.chunk_hist); }
    uint32_t rel_scale() const { return r.p1.kern != Kern::kHistS ? kRelHi16 : 0u; }      // the format of pass 1's counter words (chunk_counts)
    const uint2* below() const { return at<uint2>(L.below); }
    uint2* tot() const { return at<uint2>(L.tot); }
    uint2* dpre() const { return at<uint2>(L.dpre); }
    uint32_t* cap_ws() const { return at<uint32_t>(L.cap); }
    float* ap_part() const { return at<float>(L.ap_part); }
    ScanArgs args(const Geom& g, bool cached) const { ScanArgs as = a; as.nqt = g.nqt; as.nrun = g.nrun; as.pair_cache = cached ? pair_cache() : nullptr; return as; }
    uint32_t* gate(int word = 0) const { return at<uint32_t>(L.gate) + word; }      // the control words: nrel_max, finalize ticket, size, kGateWrapped
    const uint32_t* gate_if(const Launch& l, unsigned g, int word) const { return (l.gate & g) ? gate(word) : nullptr; }
    uint4* pair_cache() const { return r.cache_bytes ? at<uint4>(L.pair_cache) : nullptr; }
};

int plan_call(const char* who, ScanCtx& x, const Overrides& ov) {
    if (const int rc = make_plan(x.c.Q, x.c.R, x.c.K, x.c.tern, &x.p, ov)) return rc;
    return check_common(who, x.c, x.p);
}
void route_call(ScanCtx& x, Mode mode, const Overrides& ov) {
    x.r = scan_route(x.p, x.c, mode, ov, x.st);
    x.a = make_args(x.c, x.p);
    x.L = ws_layout(x.p, x.r.cache_bytes);
}

// ---- pass 1 ------------------------------------------------------------------------------------------------------------------------
// k_scan_hist_s: the cached instance where pass 1 leaves the pairs in the workspace (the shapes the pair cache is laid out for)
int valu_hist(const ScanCtx& x) {
    const Launch& h = x.r.p1;
    const Geom g = launch_geom(h, x.p, x.c.Q);
    const ScanArgs as = x.args(g, h.cache);
    auto go = [&](auto kern, int S, int NW, bool cache) {
        xmh::ProfScope prof("scan_hist", x.st);
        return start("xmh_hamming_hist", h, g, x.st, kern, S, NW, cache, as, x.chunk_hist());
    };
    auto launch = [&](auto tern_c) {
        constexpr bool T = decltype(tern_c)::value;
        return dispatch_shape<T>(h.W, h.LW, [&](auto w, auto l) {
            constexpr int WW = decltype(w)::value, LL = decltype(l)::value;
            if constexpr (kPairCacheShape<WW, T>) {
                if (h.cache) return go(k_scan_hist_s<WW, LL, T, cache_slots(WW), 1, true>, cache_slots(WW), 1, true);
            }
            constexpr int S = slots_for(WW, T, 4);
            constexpr int NW = S == 64 ? waves_for(WW, T) : 1;
            return go(k_scan_hist_s<WW, LL, T, S, NW, false>, S, NW, false);
        });
    };
    return h.tern ? launch(std::true_type{}) : launch(std::false_type{});
}

// k_scan_hist_b, or k_scan_hist_r2 (at most 64 bits: 4 waves x 4 query groups) / k_scan_hist_r2w (65..128 bits: 4 x 2), the geometry of r2_geom
int mfma_hist(const ScanCtx& x) {
    const Launch& h = x.r.p1;
    const xmh_scan_plan& p = x.p;
    const Geom g = launch_geom(h, p, x.c.Q);
    uint32_t* chunk_hist = x.chunk_hist();
    uint4* cache = x.pair_cache();
    if (h.kern == Kern::kHistB) {
        xmh::ScanBitsArgs a{x.c.rbits, x.c.rlab, x.c.qbits, x.c.qlab, (int)x.c.Q, (int)x.c.R, x.c.K, h.W, h.LW, (int)p.chunk, (int)p.nchunk, g.nqt,
                            (int)p.nbuckets, (int)p.qpad};
        a.rzero = x.c.rzero; a.qzero = x.c.qzero;                    // ternary codes: the zero planes (null for binary ones)
        return xmh::launch_scan_hist_bits(a, h.S, chunk_hist, cache, x.st);
    }
    // the launch in front of pass 1: clears the control words of the call and reads every chunk's packed words on the XCD that will scan it
    hipLaunchKernelGGL(k_scan_touch, dim3(xmh::scan_grid_blocks(kTouchPerChunk, (int)p.nchunk)), dim3(256), 0, x.st, x.c.rbits, x.c.rlab, x.c.R, h.W, h.LW,
                       p.chunk, (int)p.nchunk, x.at<uint32_t>(x.L.tick), (int)((x.L.gate + 256 - x.L.tick) / 4));
    XMH_LAUNCH_CHECK("xmh_hamming_hist control words");
    const MfmaArgs a = r2_args(x.c, h, p, g.nqt);
    xmh::ProfScope prof("scan_hist", x.st);
    auto go = [&](auto kern, int NW, int NQ, bool cached, auto... wrap_word) { return start("xmh_hamming_hist", h, g, x.st, kern, NQ, NW, cached, a, chunk_hist, cache, wrap_word...); };
    if (h.kern == Kern::kHistR2w) {
        uint32_t* ovf = x.gate(kGateWrapped);
        return h.nml == 1 ? (h.cache ? go(k_scan_hist_r2w<1, 4, 2, true>, 4, 2, true, ovf) : go(k_scan_hist_r2w<1, 4, 2, false>, 4, 2, false, ovf))
                          : (h.cache ? go(k_scan_hist_r2w<2, 4, 2, true>, 4, 2, true, ovf) : go(k_scan_hist_r2w<2, 4, 2, false>, 4, 2, false, ovf));
    }
    return h.nml == 1 ? (h.cache ? go(k_scan_hist_r2<1, 4, 4, true>, 4, 4, true) : go(k_scan_hist_r2<1, 4, 4, false>, 4, 4, false))
                      : (h.cache ? go(k_scan_hist_r2<2, 4, 4, true>, 4, 4, true) : go(k_scan_hist_r2<2, 4, 4, false>, 4, 4, false));
}

int hamming_hist_impl(const ScanCall& c, uint32_t* hist_all, uint32_t* hist_rel, xmh_stream_t stream, const Overrides& ov, bool pass2_sharded = false) {
    ScanCtx x{c, xmh::as_stream(stream)};
    if (const int rc = plan_call("xmh_hamming_hist", x, ov)) return rc;
    route_call(x, Mode::kUnsharded, ov);
    const xmh_scan_plan& p = x.p;
    const Kern kern = x.r.p1.kern;
    const bool packed = x.r.tables32 && !pass2_sharded;              // the rule above scan_route
    const bool no_tail = packed && !hist_all && !hist_rel;           // k_scan_ap_c prefixes the totals itself (Tables::kPackedNoTail); the export keeps the tail
    // k_scan_below's tile tickets, the nrel_max gate word, the finalize ticket (k_scan_hist_r2 / r2w: k_scan_touch in front of them clears them)
    if (kern == Kern::kHistS || kern == Kern::kHistB) XMH_HIP(hipMemsetAsync(x.at<char>(x.L.tick), 0, x.L.gate + 256 - x.L.tick, x.st));
    if (const int rc = kern == Kern::kHistS ? valu_hist(x) : mfma_hist(x)) return rc;
    XMH_LAUNCH_CHECK("xmh_hamming_hist");
    hipLaunchKernelGGL(k_scan_below, dim3((unsigned)p.nqtile, (unsigned)xmh::ceil_div(p.nbuckets, 4)), dim3(256), 0, x.st, x.chunk_hist(), (int)p.qpad,
                       (int)p.nbuckets, (int)p.nchunk, x.rel_scale(), x.at<uint2>(x.L.below), x.tot(), no_tail ? (uint32_t*)nullptr : x.at<uint32_t>(x.L.tick), (int)c.Q,
                       x.dpre(), x.cap_ws(), x.gate(), hist_all, hist_rel, packed, x.gate(kGateWide));
    XMH_LAUNCH_CHECK("xmh_hamming_hist below");
    ws_set_tables(c.ws, no_tail ? Tables::kPackedNoTail : (packed ? Tables::kPacked : Tables::k64));
    return XMH_OK;
}

}  // namespace

extern "C" int xmh_scan_plan_make(int64_t Q, int64_t R, int K, int ternary, xmh_scan_plan* plan_host) {
    if (!plan_host) return xmh::fail(XMH_EINVAL, "xmh_scan_plan_make: null plan");
    return make_plan(Q, R, K, ternary, plan_host);
}

extern "C" size_t xmh_scan_pair_cache_bytes(int64_t Q, int64_t R, int K, int ternary) {
    xmh_scan_plan p;
    if (make_plan(Q, R, K, ternary, &p)) return 0;
    return pair_cache_bytes(p, K, ternary != 0, pass1_family(K, ternary != 0, {}));
}

extern "C" size_t xmh_scan_pair_cache_offset(int64_t Q, int64_t R, int K, int ternary) {
    xmh_scan_plan p;
    if (make_plan(Q, R, K, ternary, &p)) return (size_t)-1;
    return ws_layout(p, 0).pair_cache;                                  // (the cache is the last region: its size moves nothing)
}

// The workspace of the same plan WITHOUT the pair cache: a caller whose device has no room for xmh_scan_plan.ws_bytes (Q x R bytes of
// cache next to a resident encoder) hands xmh_hamming_hist / _ap a buffer of this size instead, and both passes run uncached (pass 2 of
// codes of at most 64 bits: k_scan_ap_r2).  The decision follows from the size handed in, per call: no process-wide state.
extern "C" size_t xmh_scan_ws_bytes_nocache(int64_t Q, int64_t R, int K, int ternary) {
    xmh_scan_plan p;
    if (make_plan(Q, R, K, ternary, &p)) return 0;
    return ws_layout(p, 0).total;
}

// Which kernel instances an UNSHARDED mAP@all evaluation of this shape launches for the two passes (as rocprofv3 prints them, minus
// the namespace): bench_roofline.py picks the PMC rows of exactly these -- a prefix match once took the 128-bit kernel's row for
// the 64-bit headline.  The route of the launches themselves (lane order assumed to hold, the plan's whole workspace); where both
// counter widths are launched, both names, packed first.
extern "C" int xmh_scan_describe(int64_t Q, int64_t R, int K, int C, int ternary, char* out, size_t out_bytes) {
    if (!out || out_bytes < 64) return xmh::fail(XMH_EINVAL, "xmh_scan_describe: buffer too small");
    xmh_scan_plan p;
    if (const int rc = make_plan(Q, R, K, ternary, &p)) return rc;
    Overrides ov;
    ov.describe = true;
    const ScanCall c{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, Q, R, K, C, nullptr, (size_t)p.ws_bytes, ternary != 0};
    const ScanRoute r = scan_route(p, c, Mode::kUnsharded, ov, nullptr);
    char p1[160], p2[200] = "", one[120];
    if (const int rc = describe_launch(r.p1, p1, sizeof(p1))) return rc;
    for (const bool p32 : {true, false})
        for (int i = 0; i < r.n2; ++i) {
            if (r.p2[i].stand_in || r.p2[i].p32 != p32) continue;
            if (const int rc = describe_launch(r.p2[i], one, sizeof(one))) return rc;
            const size_t at = strlen(p2);
            snprintf(p2 + at, sizeof(p2) - at, "%s%s", at ? "|" : "", one);
        }
    if ((size_t)snprintf(out, out_bytes, "pass1=%s;pass2=%s", p1, p2) >= out_bytes) return xmh::fail(XMH_EINVAL, "xmh_scan_describe: buffer too small");
    return XMH_OK;
}

// FOR TESTS ONLY -- the layout is no promise.  Where the control words of a call lie in its workspace (u32 words: kGateWide is word 4): what a test reads to see which form of the
// `below` table the device settled on.
extern "C" size_t xmh_scan_gate_offset(int64_t Q, int64_t R, int K, int ternary) {
    xmh_scan_plan p;
    if (make_plan(Q, R, K, ternary, &p)) return (size_t)-1;
    return ws_layout(p, 0).gate;                                        // (the cache is the last region: its size moves nothing)
}

// Does an evaluation of this shape run on the packed `below` table (tables_packed)?  1 / 0, or a negative error code.  mode: 0 unsharded
// (xmh_hamming_map, xmh_hamming_ap without offsets), 1 caller's offsets (xmh_hamming_ap), 2 gathered totals (xmh_hamming_map_sharded), 3
// all-to-all slices (xmh_hamming_map_sharded_offsets); R is the shard's row count.  The launches' own route, like xmh_scan_describe.
extern "C" int xmh_scan_tables_packed(int64_t Q, int64_t R, int K, int C, int ternary, int mode) {
    if (mode < 0 || mode > 3) return xmh::fail(XMH_EINVAL, "xmh_scan_tables_packed: mode=%d", mode);
    xmh_scan_plan p;
    if (const int rc = make_plan(Q, R, K, ternary, &p)) return rc;
    Overrides ov;
    ov.describe = true;
    const ScanCall c{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, Q, R, K, C, nullptr, (size_t)p.ws_bytes, ternary != 0};
    static const Mode modes[4] = {Mode::kUnsharded, Mode::kBaseAll, Mode::kTotals, Mode::kAllToAll};
    return scan_route(p, c, modes[mode], ov, nullptr).tables32 ? 1 : 0;
}

extern "C" int xmh_hamming_hist(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* qlab,
                                const uint32_t* rbits, const uint32_t* rzero, const uint32_t* rlab, int64_t Q, int64_t R,
                                int K, int C, void* ws, size_t ws_bytes, uint32_t* hist_all, uint32_t* hist_rel,
                                xmh_stream_t stream) {
    XMH_RANGE("xmh_hamming_hist (pass 1)");
    const ScanCall c{qbits, qzero, qlab, rbits, rzero, rlab, Q, R, K, C, ws, ws_bytes, qzero != nullptr};
    return hamming_hist_impl(c, hist_all, hist_rel, stream, {}, hist_all != nullptr || hist_rel != nullptr);
}

extern "C" int xmh_hamming_hist_for(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* qlab,
                                    const uint32_t* rbits, const uint32_t* rzero, const uint32_t* rlab, int64_t Q, int64_t R,
                                    int K, int C, void* ws, size_t ws_bytes, uint32_t* hist_all, uint32_t* hist_rel, int pass2_sharded,
                                    xmh_stream_t stream) {
    XMH_RANGE("xmh_hamming_hist (pass 1)");
    const ScanCall c{qbits, qzero, qlab, rbits, rzero, rlab, Q, R, K, C, ws, ws_bytes, qzero != nullptr};
    return hamming_hist_impl(c, hist_all, hist_rel, stream, {}, pass2_sharded != 0);
}

namespace {
// ---- pass 2 ------------------------------------------------------------------------------------------------------------------------
// Offsets stage.  Unsharded: k_scan_below left dpre, nrel and the gate word behind (xmh_hamming_hist).  Sharded: the offsets come from the caller.
int ap_offsets(const ScanCtx& x, const Pass2& o) {
    const xmh_scan_plan& p = x.p;
    if (o.mode == Mode::kUnsharded) return XMH_OK;
    if (o.mode == Mode::kAllToAll)                                   // this shard's offset rows, by slice owner
        hipLaunchKernelGGL(k_shard_scatter_offsets, dim3((unsigned)xmh::ceil_div(p.qpad, 256), (unsigned)p.nbuckets + 1), dim3(256), 0, x.st,
                           reinterpret_cast<const uint2*>(o.hist_g), (int)p.nbuckets, (int)(p.qpad / o.world), (int)x.c.Q, (int)p.qpad, o.k, x.dpre(), x.cap_ws(),
                           o.cap, x.gate(2));
    else if (o.mode == Mode::kTotals)                                // offsets straight from the gathered totals tables of the shards
        hipLaunchKernelGGL(k_shard_offsets_dpre, dim3((unsigned)p.nqtile), dim3(256), 0, x.st, reinterpret_cast<const uint2*>(o.hist_g), o.world, o.rank,
                           (int)x.c.Q, (int)p.qpad, (int)p.nbuckets, o.k, x.dpre(), x.cap_ws(), o.cap, x.gate(2));
    else
        hipLaunchKernelGGL(k_scan_dpre, dim3((unsigned)p.nqtile), dim3(256), 0, x.st, (const uint2*)x.tot(), (int)x.c.Q, (int)p.qpad, (int)p.nbuckets, o.base_all,
                           o.base_rel, o.nrel_total, o.k, x.dpre(), x.cap_ws(), o.cap, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, x.gate(2));
    XMH_LAUNCH_CHECK(o.mode == Mode::kAllToAll ? "xmh_hamming_map_sharded_offsets scatter" : (o.mode == Mode::kTotals ? "xmh_hamming_map_sharded offsets" : "xmh_hamming_ap dpre"));
    return XMH_OK;
}

// k_scan_ap_c (float-bit counters) on one-byte entries: 4 slots x 16 queries per wave, or 8 x 8 (k_scan_ap_c<., 8, HALF>) where the counter
// rows of 16 queries leave few waves per CU -- 65..128-bit codes (129 rows: 16.5 KB per wave); 16 / 64 / 128 bit, 4 x 16 against 8 x 8:
// 0.154 / 0.185, 0.171 / 0.182, 0.220 / 0.189 ms.  On the 12-bit entries of the two-byte layout: 8 x 8.
int ap_launch_c(const ScanCtx& x, const Launch& l) {
    const Geom g = launch_geom(l, x.p, x.c.Q);
    const ScanArgs as = x.args(g, true);
    const uint32_t* wide = x.r.tables32 ? x.gate(kGateWide) : nullptr;      // the packed `below` table and its gate word (tables_packed)
    xmh::ProfScope prof("scan_ap", x.st);
    auto go = [&](auto kc, int S) {                                  // S: the slots of the instance (64 / S queries per wave)
        return start("xmh_hamming_ap", l, g, x.st, kc, S, 1, l.cache, as, x.below(), (const uint2*)(x.no_tail ? x.tot() : x.dpre()), (const uint32_t*)x.cap_ws(), x.ap_part(),
                     x.gate_if(l, kBySize, 2), x.kcap, x.gate_if(l, kByWrap, kGateWrapped), x.gate_if(l, kByWidth, 0), l.gate & kByWidth ? x.r.rank_bits : 0, wide,
                     (const uint32_t*)x.chunk_hist(), x.rel_scale(), x.no_tail ? x.cap_ws() : (uint32_t*)nullptr);
    };
    if (l.eb == 16) return x.capped ? go(k_scan_ap_c<true, 16>, 8) : go(k_scan_ap_c<false, 16>, 8);
    if (l.half) return x.capped ? go(k_scan_ap_c<true, 8, true>, 8) : go(k_scan_ap_c<false, 8, true>, 8);
    return x.capped ? go(k_scan_ap_c<true, 8>, 4) : go(k_scan_ap_c<false, 8>, 4);
}

// k_scan_ap_r2: the pairs evaluated again on the MFMA from the packed words
int ap_launch_r2(const ScanCtx& x, const Launch& l) {
    const Geom g = launch_geom(l, x.p, x.c.Q);
    const MfmaArgs ma = r2_args(x.c, l, x.p, g.nrun);
    xmh::ProfScope prof("scan_ap", x.st);
    auto go = [&](auto kern) {
        return start("xmh_hamming_ap", l, g, x.st, kern, kAp2Groups, kAp2Waves, l.cache, ma, x.below(), (const uint2*)x.dpre(), (const uint32_t*)x.cap_ws(), x.ap_part(),
                     x.gate_if(l, kBySize, 2), x.kcap);
    };
    return l.nml == 1 ? (x.capped ? go(k_scan_ap_r2<1, kAp2Waves, kAp2Groups, true>) : go(k_scan_ap_r2<1, kAp2Waves, kAp2Groups, false>))
                      : (x.capped ? go(k_scan_ap_r2<2, kAp2Waves, kAp2Groups, true>) : go(k_scan_ap_r2<2, kAp2Waves, kAp2Groups, false>));
}

// k_scan_ap_s: the cached kernel or the one that evaluates the pairs from the codes, in one of the two counter widths
int ap_launch_s(const ScanCtx& x, const Launch& l) {
    const Geom g = launch_geom(l, x.p, x.c.Q);
    const ScanArgs as = x.args(g, l.cache);                           // cached: pass 1 of this call pair left the pairs in the workspace
    auto go = [&](auto kern, int S, int NW, bool cache, const uint32_t* run_if) {
        xmh::ProfScope prof(l.p32 ? "scan_ap32" : "scan_ap", x.st);
        return start("xmh_hamming_ap", l, g, x.st, kern, S, NW, cache, as, x.below(), (const uint2*)x.dpre(), (const uint32_t*)x.cap_ws(), x.ap_part(),
                     (const uint32_t*)x.gate(), x.r.rank_bits, x.kcap, x.gate_if(l, kBySize, 2), run_if);
    };
    auto by_shape = [&](auto tern_c, auto cap_c, auto p32_c, auto masked_c) {
        constexpr bool T = decltype(tern_c)::value, CP = decltype(cap_c)::value, P32 = decltype(p32_c)::value, MK = decltype(masked_c)::value;
        return dispatch_shape<T>(l.W, l.LW, [&](auto w, auto lw) {
            constexpr int WW = decltype(w)::value, LL = decltype(lw)::value;
            if constexpr (P32 && MK) return xmh::fail(XMH_ENOTSUP, "xmh_hamming_ap: the masked fallback runs 64-bit counters only");      // (never launched: rank_bits is 0 when masked)
            else {
                if constexpr (kPairCacheShape<WW, T> && !MK) {       // the cached kernel reads no label word: one instance for every class count;
                    if (l.cache)                                     // its LDS holds the counters only, no gallery ring
                        return go(k_scan_ap_s<WW, 1, T, CP, cache_slots(WW), P32, MK, 1, true>, cache_slots(WW), 1, true, nullptr);
                }
                // the kernels that evaluate the pairs from the codes exist in the capped form only: uncapped, kcap is 0xffffffff and the cap of a
                // query its relevant count, which no ordinal exceeds -- the same credits bit for bit, half the instances (round 5)
                (void)CP;
                constexpr int S = slots_for(WW, T, P32 ? 4 : 8);
                constexpr int NW = S == 64 ? waves_for(WW, T) : 1;
                return go(k_scan_ap_s<WW, LL, T, true, S, P32, MK, NW, false>, S, NW, false, x.gate_if(l, kByWrap, kGateWrapped));
            }
        });
    };
    using T1 = std::true_type; using T0 = std::false_type;
    auto by_mask = [&](auto t, auto c, auto w) { return l.masked ? by_shape(t, c, w, T1{}) : by_shape(t, c, w, T0{}); };
    auto by_width = [&](auto t, auto c) { return l.p32 ? by_mask(t, c, T1{}) : by_mask(t, c, T0{}); };
    auto by_cap = [&](auto t) { return x.capped ? by_width(t, T1{}) : by_width(t, T0{}); };
    return l.tern ? by_cap(T1{}) : by_cap(T0{});
}

// Reduce stage: the per-chunk partial sums of a query, its divisor and (map_out) the mean over the queries
int ap_reduce(const ScanCtx& x, const Pass2& o) {
    const int64_t Q = x.c.Q;
    const unsigned nred = (unsigned)xmh::ceil_div(Q, 64);
    if (o.map_out && nred <= 4096) {                                 // reduce + mean in one launch (last-ticket block finalises)
        hipLaunchKernelGGL(k_ap_reduce_map, dim3(nred), dim3(256), 0, x.st, (const float*)x.ap_part(), (int)Q, (int)x.p.qpad, (int)x.p.nchunk,
                           (const uint32_t*)x.cap_ws(), x.kcap, o.cap, o.ap_sum, x.at<double>(x.L.gate + 256), x.gate(1), o.map_out);
        XMH_LAUNCH_CHECK("xmh_hamming_map reduce+finalize");
        return XMH_OK;
    }
    hipLaunchKernelGGL(k_ap_reduce, dim3(nred), dim3(256), 0, x.st, (const float*)x.ap_part(), (int)Q, (int)x.p.qpad, (int)x.p.nchunk, o.ap_sum,
                       o.mode != Mode::kUnsharded ? (const uint32_t*)nullptr : (const uint32_t*)x.cap_ws(), x.kcap, o.cap);
    XMH_LAUNCH_CHECK("xmh_hamming_ap reduce");
    if (o.map_out) {
        hipLaunchKernelGGL(k_map_finalize, dim3(1), dim3(256), 0, x.st, (const double*)o.ap_sum, (const int32_t*)o.cap, Q, o.map_out);
        XMH_LAUNCH_CHECK("xmh_hamming_map finalize");
    }
    return XMH_OK;
}

// ---- xmh_scan_verify: re-derive an evaluation with the kernels that do not rely on the lane order (round 6) ----------------------------
// Debug mode, off by default.  While on, every UNSHARDED xmh_hamming_ap / xmh_hamming_map call is followed by a second evaluation of the
// same inputs in a scratch workspace with the masked VALU kernels (no returning-atomic lane order, no hand-scheduled MFMA statement),
// and the per-query AP sums and divisors are compared on the host: divisors bit for bit, sums to float rounding (the two families chunk
// the gallery differently, so pass 2's per-chunk fp32 partial sums add in another order; a wrong rank moves a sum by >= 1 / R relative).
// Synchronises the stream -- a diagnostic for a new device / compiler, not something to leave on.
static std::atomic<int> g_verify{0};
constexpr int XMH_EVERIFY_CODE = -74;                 // EBADMSG: the two derivations disagree

int hamming_ap_impl(const ScanCall& c, const Pass2& o, xmh_stream_t stream, const Overrides& ov);

int verify_against_masked(const ScanCall& c, const Pass2& o, xmh_stream_t stream) {
    hipStream_t st = xmh::as_stream(stream);
    const int64_t Q = c.Q;
    std::vector<double> a1((size_t)Q), a0((size_t)Q);
    std::vector<int32_t> c1((size_t)Q), c0((size_t)Q);
    XMH_HIP(hipMemcpyAsync(a1.data(), o.ap_sum, (size_t)Q * 8, hipMemcpyDeviceToHost, st));
    XMH_HIP(hipMemcpyAsync(c1.data(), o.cap, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
    XMH_HIP(hipStreamSynchronize(st));
    Overrides ov;
    ov.mfma = 0;                                          // VALU pass 1 too
    ov.masked = true;
    xmh_scan_plan p;
    if (const int rc = make_plan(Q, c.R, c.K, c.tern, &p, ov)) return rc;
    const size_t small = ws_layout(p, 0).total;           // without a pair cache: the re-derivation evaluates the pairs from the codes
    DevBuf ws2, ap2, cap2;
    if (!ws2.alloc(small) || !ap2.alloc((size_t)Q * 8) || !cap2.alloc((size_t)Q * 4))
        return xmh::fail(XMH_ENOMEM, "xmh_scan_verify: no room for the second evaluation (%zu bytes)", small);
    ScanCall again = c; again.ws = ws2.p; again.ws_bytes = small;
    const Pass2 o2{Mode::kUnsharded, o.k, ap2.as<double>(), cap2.as<int32_t>(), nullptr};
    if (const int rc = hamming_hist_impl(again, nullptr, nullptr, stream, ov)) return rc;
    if (const int rc = hamming_ap_impl(again, o2, stream, ov)) return rc;
    XMH_HIP(hipMemcpyAsync(a0.data(), ap2.p, (size_t)Q * 8, hipMemcpyDeviceToHost, st));
    XMH_HIP(hipMemcpyAsync(c0.data(), cap2.p, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
    XMH_HIP(hipStreamSynchronize(st));
    if (const char* fe = getenv("XMH_SCAN_VERIFY_FAULT")) {   // test hook: pretend the fast derivation got one query wrong
        const int64_t at = atoll(fe) % Q;
        a1[(size_t)at] *= 1.0 + 1e-3;
    }
    int64_t bad = -1, nbad = 0;
    for (int64_t i = 0; i < Q; ++i) {
        const bool same = c1[(size_t)i] == c0[(size_t)i] && fabs(a1[(size_t)i] - a0[(size_t)i]) <= 4e-6 * fabs(a0[(size_t)i]) + 1e-9;
        if (!same) { if (bad < 0) bad = i; ++nbad; }
    }
    if (nbad)
        return xmh::fail(XMH_EVERIFY_CODE, "xmh_scan_verify: %lld of %lld queries differ between the lane-order kernels and the masked re-derivation "
                         "(first: query %lld, AP sum %.9g vs %.9g, divisor %d vs %d)", (long long)nbad, (long long)Q, (long long)bad, a1[(size_t)bad], a0[(size_t)bad],
                         c1[(size_t)bad], c0[(size_t)bad]);
    return XMH_OK;
}

int hamming_ap_impl(const ScanCall& c, const Pass2& o, xmh_stream_t stream, const Overrides& ov) {
    ScanCtx x{c, xmh::as_stream(stream)};
    if (const int rc = plan_call("xmh_hamming_ap", x, ov)) return rc;
    if (!o.ap_sum || !o.cap) return xmh::fail(XMH_EINVAL, "xmh_hamming_ap: null output");
    const int ext = (o.base_all != nullptr) + (o.base_rel != nullptr) + (o.nrel_total != nullptr);
    if (ext != 0 && ext != 3) return xmh::fail(XMH_EINVAL, "xmh_hamming_ap: base_all, base_rel and nrel_total go together");
    route_call(x, o.mode, ov);
    // the form of `below` the last pass 1 left in this workspace against the form this route reads (the rule above scan_route)
    const Tables have = ws_tables(c.ws);
    const bool have_packed = have != Tables::k64;
    if (x.r.tables32 && !have_packed) x.r.tables32 = false;          // k_scan_ap_c reads the 64-bit table as it is
    x.no_tail = x.r.tables32 && have == Tables::kPackedNoTail;       // ... and prefixes the totals itself where pass 1 left no dpre / nrel
    x.kcap = o.k > 0 && o.k < (int64_t)0xffffffffll ? (uint32_t)o.k : 0xffffffffu;
    x.capped = o.k > 0;
    if (!x.r.tables32 && have_packed) {
        // pass 1 was taken for an unsharded k_scan_ap_c call and left the packed table, which no kernel of this route reads: the 64-bit table
        // again, from pass 1's counters, the same values.  Behind a pass 1 that ran the tail (dpre, nrel, nrel_max are there): no tickets,
        // `below` and the totals only.  Behind one that did not: the whole kernel, its ticket words cleared first.
        const xmh_scan_plan& p = x.p;
        const bool tail = have == Tables::kPackedNoTail;
        if (tail) XMH_HIP(hipMemsetAsync(x.at<char>(x.L.tick), 0, x.L.gate - x.L.tick, x.st));
        hipLaunchKernelGGL(k_scan_below, dim3((unsigned)p.nqtile, (unsigned)xmh::ceil_div(p.nbuckets, 4)), dim3(256), 0, x.st, x.chunk_hist(), (int)p.qpad,
                           (int)p.nbuckets, (int)p.nchunk, x.rel_scale(), x.at<uint2>(x.L.below), x.tot(), tail ? x.at<uint32_t>(x.L.tick) : (uint32_t*)nullptr, (int)x.c.Q,
                           tail ? x.dpre() : (uint2*)nullptr, tail ? x.cap_ws() : (uint32_t*)nullptr, tail ? x.gate() : (uint32_t*)nullptr, (uint32_t*)nullptr,
                           (uint32_t*)nullptr, false, (uint32_t*)nullptr);
        XMH_LAUNCH_CHECK("xmh_hamming_ap below");
        ws_set_tables(c.ws, Tables::k64);
    }
    if (const int rc = ap_offsets(x, o)) return rc;
    for (int i = 0; i < x.r.n2; ++i) {
        const Launch& l = x.r.p2[i];
        if (const int rc = l.kern == Kern::kApC ? ap_launch_c(x, l) : (l.kern == Kern::kApR2 ? ap_launch_r2(x, l) : ap_launch_s(x, l))) return rc;
        XMH_LAUNCH_CHECK("xmh_hamming_ap");
    }
    if (const int rc = ap_reduce(x, o)) return rc;
    if (g_verify.load(std::memory_order_relaxed) && !ov.masked && o.mode == Mode::kUnsharded) return verify_against_masked(c, o, stream);
    return XMH_OK;
}

// one evaluation of the self-check scan `c` (operands on the device, no workspace yet) with a pinned kernel choice, into host vectors; false on
// any HIP / library error
bool selfcheck_eval(const ScanCall& c, int force, std::vector<uint32_t>& hist, std::vector<double>& ap, std::vector<int32_t>& cap) {
    Overrides ov;
    ov.mfma = force;
    const int64_t Q = c.Q;
    xmh_scan_plan p;
    if (make_plan(Q, c.R, c.K, 0, &p, ov) != XMH_OK) return false;
    const size_t nb = (size_t)p.nbuckets;
    DevBuf ws, dh, dap, dcap;
    if (!ws.alloc(p.ws_bytes) || !dh.alloc(2 * Q * nb * 4) || !dap.alloc(Q * 8) || !dcap.alloc(Q * 4)) return false;
    ScanCall run = c; run.ws = ws.p; run.ws_bytes = p.ws_bytes;
    const Pass2 o{Mode::kUnsharded, 0, dap.as<double>(), dcap.as<int32_t>(), nullptr};
    uint32_t* h = dh.as<uint32_t>();
    if (hamming_hist_impl(run, h, h + Q * nb, nullptr, ov) != XMH_OK) return false;
    if (hamming_ap_impl(run, o, nullptr, ov) != XMH_OK) return false;
    hist.resize(2 * Q * nb); ap.resize(Q); cap.resize(Q);
    if (hipDeviceSynchronize() != hipSuccess) return false;
    return hipMemcpy(hist.data(), dh.p, hist.size() * 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(ap.data(), dap.p, Q * 8, hipMemcpyDeviceToHost) == hipSuccess &&
           hipMemcpy(cap.data(), dcap.p, Q * 4, hipMemcpyDeviceToHost) == hipSuccess;
}

bool r2_selfcheck_ok() {
    static int state[64];                                 // 0 unknown, 1 passed, 2 failed
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return true;     // no device: nothing can run, nothing to guard
    const char* e = getenv("XMH_SCAN_M2_SELFCHECK");
    if (e && atoi(e) == 0) return true;
    std::lock_guard<std::mutex> lock(mu);
    if (state[dev]) return state[dev] == 1;
    state[dev] = 1;                                       // the evaluations below pin Overrides::mfma and do not ask again
    const int64_t Q = 272, R = 9000;                      // one whole block of k_scan_hist_r2 (256 queries) and a ragged one
    bool same = true, ran = true;
    // k_scan_hist_r2 / r2w take their counter addresses as offsets from LDS address 0 (xmh_scan_mfma.h, r2_cell): the dynamic array has to
    // start there, so none of their instances may have static LDS
    {
        const void* const r2_kernels[] = {reinterpret_cast<const void*>(k_scan_hist_r2<1, 4, 4, true>), reinterpret_cast<const void*>(k_scan_hist_r2<1, 4, 4, false>),
                                          reinterpret_cast<const void*>(k_scan_hist_r2<2, 4, 4, true>), reinterpret_cast<const void*>(k_scan_hist_r2<2, 4, 4, false>),
                                          reinterpret_cast<const void*>(k_scan_hist_r2w<1, 4, 2, true>), reinterpret_cast<const void*>(k_scan_hist_r2w<1, 4, 2, false>),
                                          reinterpret_cast<const void*>(k_scan_hist_r2w<2, 4, 2, true>), reinterpret_cast<const void*>(k_scan_hist_r2w<2, 4, 2, false>)};
        for (const void* k : r2_kernels) {
            hipFuncAttributes fa;
            if (hipFuncGetAttributes(&fa, k) != hipSuccess) ran = false;
            else if (fa.sharedSizeBytes != 0) same = false;
        }
    }
    // two code words, one + a partial one, <= 32 bits (all k_scan_hist_r2), 65..128 bits (k_scan_hist_r2w), with 80 classes; then both
    // kernels with 128 classes and labels made for the FP4 label tile (below)
    const int cases[6][2] = {{64, 80}, {40, 80}, {16, 80}, {100, 80}, {64, 128}, {100, 128}};
    for (const auto& kc : cases) {
        if (!ran || !same) break;
        const int K = kc[0], C = kc[1], LW = (C + 31) / 32;
        const int W = (K + 31) / 32;
        std::vector<uint32_t> qb(Q * W), ql(Q * LW), rb(R * W), rl(R * LW);
        uint64_t x = 0x9E3779B97F4A7C15ull ^ (uint64_t)K;
        auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (uint32_t)(x >> 16); };
        const uint32_t last = K % 32 ? (1u << (K % 32)) - 1 : 0xffffffffu;
        for (auto& v : qb) v = rnd();
        for (int64_t i = 0; i < R; ++i)                   // a quarter of the gallery repeats earlier codes: ties inside and across chunks
            for (int w = 0; w < W; ++w) rb[i * W + w] = (i > 64 && (rnd() & 3) == 0) ? rb[(rnd() % 64) * W + w] : rnd();
        for (int64_t i = 0; i < Q; ++i) qb[i * W + W - 1] &= last;
        for (int64_t i = 0; i < R; ++i) rb[i * W + W - 1] &= last;
        const uint32_t lastl = C % 32 ? (1u << (C % 32)) - 1 : 0xffffffffu;
        for (int64_t i = 0; i < Q * LW; ++i) ql[i] = rnd() & rnd() & rnd() & (i % LW == LW - 1 ? lastl : 0xffffffffu);
        for (int64_t i = 0; i < R * LW; ++i) rl[i] = rnd() & rnd() & rnd() & (i % LW == LW - 1 ? lastl : 0xffffffffu);
        if (C == 80) {
            for (int64_t i = 0; i < Q; ++i) ql[i * LW] |= 1u;                        // every query has a relevant item
            for (int64_t i = 0; i < R; i += 7) rl[i * LW] |= 1u;
        } else {
            // 128 classes: the label overlap is ONE FP4 MFMA whose f32 chain starts at a denormal (xmh_scan_mfma.h, label_query_f4).  Every
            // other query and two items of three carry a single class, mostly in words 2 and 3: pairs whose only common class lies in bits
            // 64..127, pairs with none at all (every third item has no label), and full rows (count 128) next to the random ones
            auto one = [&](uint32_t* l, int c) { for (int w = 0; w < LW; ++w) l[w] = 0u; l[c >> 5] = 1u << (c & 31); };
            for (int64_t i = 0; i < Q; i += 2) one(&ql[i * LW], i % 8 == 0 ? (int)(i * 3 % 64) : 64 + (int)(i * 7 % 64));
            for (int64_t i = 0; i < R; ++i) {
                if (i % 3 == 0) one(&rl[i * LW], 64 + (int)(i * 5 % 64));
                else if (i % 3 == 1) for (int w = 0; w < LW; ++w) rl[i * LW + w] = 0u;
            }
            for (int w = 0; w < LW; ++w) ql[1 * LW + w] = rl[2 * LW + w] = rl[5000 * LW + w] = 0xffffffffu;
        }
        // the highest counter addresses of both kernels -- the last wave's last query group of a block: queries 240..255 of k_scan_hist_r2's 256,
        // 112..127 of k_scan_hist_r2w's 128 -- at both ends of the bucket range: items equal to the query (distance 0) and to its complement
        // (distance K), each once sharing a class with the query and once without a label, in whole batches and in the ragged last one
        {
            const int64_t q0 = K <= 64 ? 240 : 112;
            for (int64_t t = 0; t < 16; ++t) {
                const int64_t q = q0 + t;
                ql[q * LW] |= 1u;
                for (int set = 0; set < 2; ++set)
                    for (int v = 0; v < 4; ++v) {
                        const int64_t i = (set ? R - 64 : 128) + 4 * t + v;
                        for (int w = 0; w < W; ++w) rb[i * W + w] = (v & 2) ? ~qb[q * W + w] & (w == W - 1 ? last : 0xffffffffu) : qb[q * W + w];
                        for (int w = 0; w < LW; ++w) rl[i * LW + w] = (v & 1) ? 0u : ql[q * LW + w];
                    }
            }
        }
        std::vector<uint32_t> h1, h0;
        std::vector<double> a1, a0;
        std::vector<int32_t> c1, c0;
        DevBuf dq, dql, dr, drl;
        auto up = [](DevBuf& d, const std::vector<uint32_t>& v) { return d.alloc(v.size() * 4) && hipMemcpy(d.p, v.data(), v.size() * 4, hipMemcpyHostToDevice) == hipSuccess; };
        if (!up(dq, qb) || !up(dql, ql) || !up(dr, rb) || !up(drl, rl)) { ran = false; break; }
        const ScanCall c{dq.as<uint32_t>(), nullptr, dql.as<uint32_t>(), dr.as<uint32_t>(), nullptr, drl.as<uint32_t>(), Q, R, K, C, nullptr, 0, false};
        if (!selfcheck_eval(c, 1, h1, a1, c1) || !selfcheck_eval(c, 0, h0, a0, c0)) { ran = false; break; }
        // histograms and divisors bit for bit; the two kernels chunk the gallery differently, so pass 2's per-chunk float partial sums
        // add in another order: the AP sums to float rounding (a wrong pair moves one by >= 1 / R relative, far above it)
        bool ap_close = true;
        for (int64_t i = 0; i < Q; ++i) ap_close = ap_close && fabs(a1[i] - a0[i]) <= 4e-6 * fabs(a0[i]) + 1e-9;
        if (h1 != h0 || c1 != c0 || !ap_close) { same = false; break; }
    }
    if (e && atoi(e) == 2) same = false;
    if (!ran) {                                           // out of memory or a launch failure: no verdict, do not cache one
        state[dev] = 0;
        return true;
    }
    if (!same) {
        state[dev] = 2;
        fprintf(stderr, "xmh: k_scan_hist_r2 self-check FAILED on device %d (results differ from the VALU kernels): falling back to the VALU scan "
                        "for this process.  Please report the hipcc / ROCm versions.\n", dev);
    }
    return state[dev] == 1;
}
}  // namespace

extern "C" int xmh_scan_verify(int on) {
    g_verify.store(on != 0 ? 1 : 0, std::memory_order_relaxed);
    return XMH_OK;
}

extern "C" int xmh_hamming_ap(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* qlab, const uint32_t* rbits,
                              const uint32_t* rzero, const uint32_t* rlab, int64_t Q, int64_t R, int K, int C, void* ws,
                              size_t ws_bytes, const uint32_t* base_all, const uint32_t* base_rel,
                              const uint32_t* nrel_total, int64_t k, double* ap_sum, int32_t* cap, xmh_stream_t stream) {
    XMH_RANGE("xmh_hamming_ap (pass 2)");
    const ScanCall c{qbits, qzero, qlab, rbits, rzero, rlab, Q, R, K, C, ws, ws_bytes, qzero != nullptr};
    Pass2 o{base_all ? Mode::kBaseAll : Mode::kUnsharded, k, ap_sum, cap, nullptr};
    o.base_all = base_all; o.base_rel = base_rel; o.nrel_total = nrel_total;
    return hamming_ap_impl(c, o, stream, {});
}

extern "C" int xmh_hamming_map(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* qlab, const uint32_t* rbits,
                               const uint32_t* rzero, const uint32_t* rlab, int64_t Q, int64_t R, int K, int C, void* ws,
                               size_t ws_bytes, int64_t k, double* ap_sum, int32_t* cap, double* map_out, xmh_stream_t stream) {
    XMH_RANGE("xmh_hamming_map (pass 2 + mean)");
    if (!map_out) return xmh::fail(XMH_EINVAL, "xmh_hamming_map: null output");
    const ScanCall c{qbits, qzero, qlab, rbits, rzero, rlab, Q, R, K, C, ws, ws_bytes, qzero != nullptr};
    return hamming_ap_impl(c, Pass2{Mode::kUnsharded, k, ap_sum, cap, map_out}, stream, {});
}

extern "C" size_t xmh_scan_totals_offset(int64_t Q, int64_t R, int K, int ternary, size_t* bytes) {
    xmh_scan_plan p;
    if (make_plan(Q, R, K, ternary, &p)) return (size_t)-1;
    if (bytes) *bytes = (size_t)p.nbuckets * p.qpad * 8;
    return ws_layout(p, 0).tot;
}

extern "C" int xmh_hamming_map_sharded(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* qlab, const uint32_t* rbits,
                                       const uint32_t* rzero, const uint32_t* rlab, int64_t Q, int64_t R, int K, int C, void* ws,
                                       size_t ws_bytes, const uint32_t* hist_gathered, int world, int rank, int64_t k, double* ap_sum,
                                       int32_t* cap, double* map_partial, xmh_stream_t stream) {
    XMH_RANGE("xmh_hamming_map_sharded (pass 2)");
    if (!hist_gathered || !map_partial) return xmh::fail(XMH_EINVAL, "xmh_hamming_map_sharded: null pointer");
    if (world <= 0 || rank < 0 || rank >= world) return xmh::fail(XMH_EINVAL, "xmh_hamming_map_sharded: bad world=%d rank=%d", world, rank);
    const ScanCall c{qbits, qzero, qlab, rbits, rzero, rlab, Q, R, K, C, ws, ws_bytes, qzero != nullptr};
    Pass2 o{Mode::kTotals, k, ap_sum, cap, map_partial};
    o.hist_g = hist_gathered; o.world = world; o.rank = rank;
    return hamming_ap_impl(c, o, stream, {});
}

extern "C" int xmh_shard_slice_offsets(const uint32_t* totals_slices, int world, int nbuckets, int slice, uint32_t* offsets_out, xmh_stream_t stream) {
    XMH_RANGE("xmh_shard_slice_offsets");
    if (!totals_slices || !offsets_out) return xmh::fail(XMH_EINVAL, "xmh_shard_slice_offsets: null pointer");
    if (world <= 0 || nbuckets <= 0 || slice <= 0) return xmh::fail(XMH_EINVAL, "xmh_shard_slice_offsets: bad arguments (world=%d nb=%d slice=%d)", world, nbuckets, slice);
    hipLaunchKernelGGL(k_shard_slice_offsets, dim3((unsigned)xmh::ceil_div(slice, 64)), dim3(256), 0, xmh::as_stream(stream),
                       reinterpret_cast<const uint2*>(totals_slices), world, nbuckets, slice, reinterpret_cast<uint2*>(offsets_out));
    XMH_LAUNCH_CHECK("xmh_shard_slice_offsets");
    return XMH_OK;
}

extern "C" int xmh_hamming_map_sharded_offsets(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* qlab, const uint32_t* rbits,
                                               const uint32_t* rzero, const uint32_t* rlab, int64_t Q, int64_t R, int K, int C, void* ws,
                                               size_t ws_bytes, const uint32_t* offsets, int world, int64_t k, double* ap_sum, int32_t* cap,
                                               double* map_partial, xmh_stream_t stream) {
    XMH_RANGE("xmh_hamming_map_sharded_offsets (pass 2)");
    if (!offsets || !map_partial) return xmh::fail(XMH_EINVAL, "xmh_hamming_map_sharded_offsets: null pointer");
    const ScanCall c{qbits, qzero, qlab, rbits, rzero, rlab, Q, R, K, C, ws, ws_bytes, qzero != nullptr};
    xmh_scan_plan p;
    if (const int rc = make_plan(Q, R, K, c.tern, &p)) return rc;
    if (world <= 0 || p.qpad % world) return xmh::fail(XMH_EINVAL, "xmh_hamming_map_sharded_offsets: qpad=%lld is not a multiple of world=%d", (long long)p.qpad, world);
    Pass2 o{Mode::kAllToAll, k, ap_sum, cap, map_partial};
    o.hist_g = offsets; o.world = world;
    return hamming_ap_impl(c, o, stream, {});
}

extern "C" int xmh_map_finalize(const double* ap_sum, const int32_t* cap, int64_t Q, double* map_out, xmh_stream_t stream) {
    XMH_RANGE("xmh_map_finalize");
    if (!ap_sum || !cap || !map_out || Q <= 0) return xmh::fail(XMH_EINVAL, "xmh_map_finalize: bad arguments");
    hipLaunchKernelGGL(k_map_finalize, dim3(1), dim3(256), 0, xmh::as_stream(stream), ap_sum, cap, Q, map_out);
    XMH_LAUNCH_CHECK("xmh_map_finalize");
    return XMH_OK;
}

extern "C" int xmh_shard_offsets(const uint32_t* hist_gathered, int world, int rank, int64_t Q, int nbuckets, uint32_t* base_all,
                                 uint32_t* base_rel, uint32_t* nrel_total, xmh_stream_t stream) {
    XMH_RANGE("xmh_shard_offsets");
    if (!hist_gathered || !base_all || !base_rel || !nrel_total) return xmh::fail(XMH_EINVAL, "xmh_shard_offsets: null pointer");
    if (world <= 0 || rank < 0 || rank >= world || Q <= 0 || nbuckets <= 0 || Q >= (1ll << 24))
        return xmh::fail(XMH_EINVAL, "xmh_shard_offsets: bad arguments (world=%d rank=%d Q=%lld nb=%d)", world, rank, (long long)Q, nbuckets);
    hipLaunchKernelGGL(k_shard_offsets, dim3((unsigned)Q), dim3(64), 0, xmh::as_stream(stream), hist_gathered, world, rank, (int)Q, nbuckets,
                       base_all, base_rel, nrel_total);
    XMH_LAUNCH_CHECK("xmh_shard_offsets");
    return XMH_OK;
}
