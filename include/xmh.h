/*
 * xmh.h -- C ABI of libxmh.so, the MI355X (gfx950) encode-and-retrieve library that sits behind the
 * plugin surface of kalenforn/clip-based-cross-modal-hash.
 *
 * Conventions:
 *   - every entry point is extern "C", takes plain pointers and sizes, returns 0 on success or a
 *     negative errno-style code; nothing throws, nothing is owned by the library, no global state
 *     except a thread-local last-error string (xmh_last_error).
 *   - pointers are DEVICE pointers unless the parameter name ends in _host.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, stream-ordered, and the
 *     call returns without synchronising.
 *   - codes are bit-packed: word w bit j of `bits[n][W]` (W = ceil(K/32)) is 1 iff code[n][32w+j] > 0;
 *     `zero[n][W]` marks code == 0 (sign(0) = 0, reference runners/base.py:410) and has its padding
 *     bits (positions >= K) SET so that padded positions never count.
 *   - labels are bit-packed multi-hot masks `lab[n][Lw]`, Lw = ceil(C/32).
 *
 * Each declaration cites the reference interface it replaces (file:line under the reference repo).
 */
#ifndef XMH_H
#define XMH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XMH_OK 0
#define XMH_EINVAL (-22)
#define XMH_ENOMEM (-12)
#define XMH_ENOTSUP (-95)
#define XMH_EHIP (-5)

/* element types accepted for label / mask inputs */
#define XMH_DT_F32 0
#define XMH_DT_I64 1
#define XMH_DT_I32 2
#define XMH_DT_U8 3

typedef void* xmh_stream_t;

int xmh_version(void);
/* identity of the sources this library was built from: the first 16 hex digits of sha256 over the .hip and .h files of csrc/ and include/xmh.h
 * (the Makefile's SRCID).  bench.py recomputes it from the files beside the library and reports whether they match. */
const char* xmh_build_id(void);
/* thread-local description of the last failure on this thread ("" if none) */
const char* xmh_last_error(void);

/* Per-kernel timing for bench.py: when enabled, the library brackets its dominant kernels with HIP events
 * on the launch stream (names: "scan_hist", "scan_ap", "topk_filter", "gemm", ...).  xmh_prof_read blocks
 * on the last recorded event of that name and returns the mean launch duration since xmh_prof_enable(1). */
int xmh_prof_enable(int on);
int xmh_prof_read(const char* name_host, double* avg_ms_host, int64_t* launches_host);
/* roctx ranges (SURVEY 5 "Build adds"; round 6).  `on` of xmh_prof_enable is a bit set: 1 = the HIP events above, 2 = roctx ranges
 * around every phase of the path -- tower forward, head, pack, pass 1, pass 2, the top-k phases, the float route --, so that a
 * `rocprofv3 --marker-trace --kernel-trace` timeline of valid() (reference runners/base.py:307-357) carries phase markers.  The roctx
 * library (librocprofiler-sdk-roctx.so, else libroctx64.so) is looked up with dlopen when bit 2 is first asked for (XMH_ENOTSUP if
 * absent); libxmh.so does not link it.  xmh_range_push / _pop: the same ranges for the host layer above the C ABI (the collectives of
 * the sharded evaluation, the encode loop); no-ops while ranges are off. */
int xmh_range_push(const char* name_host);
int xmh_range_pop(void);
/* Debug mode for a new device / compiler (round 6).  The fast ranking kernels rely on two things no ISA document promises: same-address
 * lanes of one returning LDS add are served in lane order (probed per device: one wave alone, then pass 2's geometry under load beside
 * matrix waves), and hand-kept hazards around inline MFMA statements (a self-check scan per device).  While xmh_scan_verify(1) is on,
 * every UNSHARDED xmh_hamming_ap / xmh_hamming_map / xmh_calc_map_k is followed by a second derivation of the same evaluation with the
 * masked VALU kernels, which rely on neither; divisors must agree bit for bit and the per-query AP sums to float rounding, else the
 * call returns -74 with the first differing query in xmh_last_error().  Costs about three evaluations and a stream synchronisation
 * per call. */
int xmh_scan_verify(int on);

/* ---------------------------------------------------------------------------------------------
 * Quantisers (a-6).
 * xmh_pack_sign        replaces BaseTrainer.make_hash_code  (runners/base.py:407-410): sign -> -1/0/+1.
 *                      `flags` (device int32, nullable, caller zeroes it) gets bit0 OR-ed in if any element was
 *                      exactly 0 and bit1 if any element was not in {-1,0,+1} (un-quantised input: the
 *                      packed path does not apply).
 * xmh_pack_pair_argmax replaces DCMHTTrainer.make_hash_code (runners/DCMHT/runner.py:82-95):
 *                      probs[n][2K] -> bit j = (probs[2j+1] > probs[2j]) strictly (ties -> -1).
 * xmh_unpack_pm1       packed -> +-1/0 float32 [n][K] (the buffers get_code returns, runners/base.py:245-257,
 *                      and the .mat writer, :386-405).  `zero` may be NULL.
 * `row_index` (device int64[n], nullable): when given, row i of the input is written to packed row
 * row_index[i] (the scatter `buffer[index,:] = code` of runners/base.py:256-257).
 * ------------------------------------------------------------------------------------------- */
int xmh_pack_sign(const float* codes, int64_t n, int K, const int64_t* row_index,
                  uint32_t* bits, uint32_t* zero, int32_t* flags, xmh_stream_t stream);
int xmh_pack_pair_argmax(const float* probs, int64_t n, int K, const int64_t* row_index,
                         uint32_t* bits, xmh_stream_t stream);
int xmh_unpack_pm1(const uint32_t* bits, const uint32_t* zero, int64_t n, int K, float* out,
                   xmh_stream_t stream);
/* multi-hot labels [n][C] of dtype `dt` (XMH_DT_*) -> packed masks [n][ceil(C/32)] (label > 0).
 * Replaces the int64 label matmul operands of calc_map_k (common/calc_utils.py:72) and calc_label_sim (:8-10). */
int xmh_pack_labels(const void* labels, int dt, int64_t n, int C, uint32_t* lab, xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Materialised distances (a-1): calc_hammingDist (common/calc_utils.py:51-56).
 *   out_f32[Q][R] = 0.5 * (K - q.r)   (exact for -1/0/+1 codes; pass zero masks as NULL for binary)
 *   out_u16[Q][R] = popcount(q xor r) (binary codes only)
 * Exactly one of out_f32 / out_u16 must be non-NULL.
 * ------------------------------------------------------------------------------------------- */
int xmh_hamming_dist(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* rbits, const uint32_t* rzero,
                     int64_t Q, int64_t R, int K, float* out_f32, uint16_t* out_u16, xmh_stream_t stream);
/* calc_label_sim (common/calc_utils.py:8-10): out[Q][R] = 1.0f iff the two items share a label. */
int xmh_label_sim(const uint32_t* qlab, const uint32_t* rlab, int64_t Q, int64_t R, int C, float* out,
                  xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fused ranking scan (a-2): calc_map_k (common/calc_utils.py:58-92) without the [Q,R] intermediates.
 *
 * Canonical order = (distance asc, gallery index asc)  == torch.sort(stable=True).
 * Two streaming passes over the gallery shard (a wave owns 64/S queries x S item slots, per-query bucket counters in LDS):
 *   pass 1 (xmh_hamming_hist): per (query, gallery chunk) bucket counts of all / relevant items;
 *   pass 2 (xmh_hamming_ap):   rank of every relevant item = bucket base + running in-bucket count,
 *                              accumulates sum_j j/rank_j for ordinals j <= min(n_rel, k).
 * `xmh_scan_plan` reports the chunking and the workspace both passes share.
 * ------------------------------------------------------------------------------------------- */
typedef struct xmh_scan_plan {
    int64_t chunk;      /* gallery items per chunk                                  */
    int64_t nchunk;     /* chunks in this shard                                     */
    int64_t nqtile;     /* 64-query tiles                                           */
    int64_t qpad;       /* Q rounded up to 64                                       */
    int64_t nbuckets;   /* K+1 (binary) or 2K+1 (ternary, distances in half units)  */
    size_t ws_bytes;    /* workspace the caller must provide to hist/ap             */
} xmh_scan_plan;

int xmh_scan_plan_make(int64_t Q, int64_t R, int K, int ternary, xmh_scan_plan* plan_host);
/* Bytes of the workspace (included in plan.ws_bytes) that hold the PAIR CACHE: xmh_hamming_hist leaves one byte per (query,
 * gallery item) pair -- distance << 1 | relevant; two bytes for codes of 129..256 bits (and the region is sized for two bytes from
 * 65 bits on: codes of 65..128 bits use its first half with one-byte entries, where a distance of 128 wraps to 0 and a control word
 * tells pass 2 to evaluate the pairs itself; XMH_SCAN_BYTE128=0 brings their two-byte entries back) -- and xmh_hamming_ap reads it
 * instead of evaluating the pair again.  Used for binary codes of 33..256 bits while it stays under XMH_SCAN_CACHE_MB (default 131072 MB;
 * 0 = off); returns 0 when it is not used. */
size_t xmh_scan_pair_cache_bytes(int64_t Q, int64_t R, int K, int ternary);
/* Byte offset of that pair cache inside the workspace ((size_t)-1 on a bad shape) -- for tests and diagnostics, which decode it
 * and compare every entry with the oracle's distance and relevance.  Layout for codes of at most 64 bits:
 * [chunk][16-query tile][64-item batch of the chunk][lane 0..63][16 bytes]; lane = slot * 16 + query-in-tile, byte t of a lane
 * is the pair (that query, item 64 * batch + 4 * t + slot of the chunk); entry = distance << 1 | relevant (mod 256).  Longer and ternary codes:
 * [chunk][8-query tile][batch][lane][3 x u32], lane = slot * 8 + query-in-tile, entry t (12 bits, round 6: bits [12 t, 12 t + 12) of the
 * 96) = item 64 * batch + 8 * t + slot. */
size_t xmh_scan_pair_cache_offset(int64_t Q, int64_t R, int K, int ternary);
/* The workspace of the same plan WITHOUT its pair cache.  xmh_hamming_hist / xmh_hamming_ap / xmh_hamming_map take the size they are handed
 * as the decision: a buffer of at least xmh_scan_plan.ws_bytes runs with the cache, one of at least this size (and smaller than that) runs
 * the same plan uncached -- for devices that have no room for Q x R bytes next to a resident encoder.  Both calls of a pair must be given
 * the same size.  (The reference keeps a [Q, R] fp32 matrix and its sort on the host: common/calc_utils.py:76-77.) */
size_t xmh_scan_ws_bytes_nocache(int64_t Q, int64_t R, int K, int ternary);
/* Diagnostics for the measurement harness: writes "pass1=<kernel instance>;pass2=<kernel instance>[|<second width>]" -- the kernels
 * an unsharded mAP@all evaluation of this shape launches, spelled as rocprofv3 prints them -- so that a profile row is matched by
 * its exact name.  out_bytes >= 64. */
int xmh_scan_describe(int64_t Q, int64_t R, int K, int C, int ternary, char* out, size_t out_bytes);
/* Diagnostics, the same route: does an evaluation of this shape keep the chunk-offset table between the passes in its packed form (one
 * 32-bit word per cell)?  Returns 1 / 0, or a negative error code.  R: the rows of the shard.  mode: 0 unsharded
 * (xmh_hamming_map, xmh_hamming_ap without offsets), 1 xmh_hamming_ap with the caller's offsets, 2 xmh_hamming_map_sharded,
 * 3 xmh_hamming_map_sharded_offsets. */
int xmh_scan_tables_packed(int64_t Q, int64_t R, int K, int C, int ternary, int mode);
/* FOR TESTS ONLY; the layout of the workspace is no part of the interface and may change.  Byte offset of the call's control words (u32)
 * in the workspace; word 4 is raised by xmh_hamming_hist when a bucket total did not fit
 * the packed table and pass 2 sums its start values itself.  (size_t)-1 on a bad shape. */
size_t xmh_scan_gate_offset(int64_t Q, int64_t R, int K, int ternary);

/* pass 1.  hist_all / hist_rel: [Q][nbuckets] u32 totals over this shard (either may be NULL).
 * qzero / rzero NULL => binary codes.
 * Labels: [n][ceil(C / 32)] u32 masks.  C <= 128 (1..4 words) on every path; binary codes up to 256 bits also take exactly EIGHT words
 * (C in 225..256): a caller with 129..224 classes pads its masks to eight words with zero bits and passes C = 256 (Python:
 * RankingScan does).  More classes: XMH_ENOTSUP.
 * Also leaves in the workspace what a single-shard pass 2 needs from the totals (per-bucket rank offsets, the relevant count
 * of every query), so that xmh_hamming_ap / xmh_hamming_map with NULL offsets launch pass 2 and the reduction only. */
int xmh_hamming_hist(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* qlab,
                     const uint32_t* rbits, const uint32_t* rzero, const uint32_t* rlab,
                     int64_t Q, int64_t R, int K, int C, void* ws, size_t ws_bytes,
                     uint32_t* hist_all, uint32_t* hist_rel, xmh_stream_t stream);
/* The same, told which pass 2 follows: pass2_sharded != 0 = one with offsets from outside the shard (xmh_hamming_ap with offsets,
 * xmh_hamming_map_sharded, xmh_hamming_map_sharded_offsets), 0 = xmh_hamming_map / xmh_hamming_ap without offsets.  It decides the form of
 * the chunk-offset table left between the passes; a wrong word costs one launch in pass 2, never a result.  Plain
 * xmh_hamming_hist takes a call that asks for hist_all or hist_rel for a sharded one. */
int xmh_hamming_hist_for(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* qlab,
                         const uint32_t* rbits, const uint32_t* rzero, const uint32_t* rlab,
                         int64_t Q, int64_t R, int K, int C, void* ws, size_t ws_bytes,
                         uint32_t* hist_all, uint32_t* hist_rel, int pass2_sharded, xmh_stream_t stream);

/* pass 2 (needs the workspace pass 1 filled for the same inputs).
 *   base_all / base_rel [Q][nbuckets] u32 and nrel_total [Q] u32: rank offsets contributed by items
 *   OUTSIDE this shard (all lower buckets anywhere + same bucket on lower-ranked shards) and the global
 *   relevant count; all three NULL => single shard, the offsets xmh_hamming_hist left in the workspace are used.
 *   (A call WITH offsets overwrites them: run xmh_hamming_hist again before a single-shard evaluation on that workspace.)
 *   Any number of evaluations (different k) may follow one xmh_hamming_hist.
 *   k <= 0 means "all" (k = None in the reference).
 *   ap_sum[Q] (f64) = sum over this shard's relevant items of ordinal/rank, for ordinal <= cap;
 *   cap[Q] (i32)    = min(n_rel, k)  (the divisor, common/calc_utils.py:81). */
int xmh_hamming_ap(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* qlab,
                   const uint32_t* rbits, const uint32_t* rzero, const uint32_t* rlab,
                   int64_t Q, int64_t R, int K, int C, void* ws, size_t ws_bytes,
                   const uint32_t* base_all, const uint32_t* base_rel, const uint32_t* nrel_total,
                   int64_t k, double* ap_sum, int32_t* cap, xmh_stream_t stream);

/* xmh_hamming_ap of an UNSHARDED gallery followed by xmh_map_finalize in one call: ap_sum / cap as xmh_hamming_ap writes
 * them, map_out[0] = mean_q ap_sum[q] / cap[q]. */
int xmh_hamming_map(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* qlab, const uint32_t* rbits,
                    const uint32_t* rzero, const uint32_t* rlab, int64_t Q, int64_t R, int K, int C, void* ws,
                    size_t ws_bytes, int64_t k, double* ap_sum, int32_t* cap, double* map_out, xmh_stream_t stream);
/* calc_map_k (reference common/calc_utils.py:58-92) in ONE call, on the operands the reference's callers hold
 * (runners/base.py:259-264: float code matrices on the device): qB [Q][K] / rB [R][K] float32 codes (-1 / 0 / +1), qlab / rlab packed
 * label masks (xmh_pack_labels: the label matrices are the same for every call of an evaluation, pack them once), k <= 0 = all.
 * Packs both code matrices into the workspace, reads their value flags (first synchronisation), runs both passes with the binary or --
 * an exact zero among the codes -- the ternary kernels, and copies the mAP to *map_host (second synchronisation: the reference
 * returns a host scalar too).  *flags_host: bit 0 = an exact zero was seen, bit 1 = a value outside {-1, 0, +1}: then NOTHING is
 * evaluated (the codes are not quantised: common/calc_utils.py would rank the float inner products) and *map_host is left alone.
 * K must be a code length the kernels take as it is (<= 32, 64, 128, 256, 512, 1024, 2048 bits); C as for xmh_hamming_hist.
 * The same kernels and the same bits as pack + xmh_hamming_hist + xmh_hamming_map. */
size_t xmh_calc_map_k_ws_bytes(int64_t Q, int64_t R, int K, int C);
int xmh_calc_map_k(const float* qB, const float* rB, const uint32_t* qlab, const uint32_t* rlab, int64_t Q, int64_t R, int K, int C,
                   int64_t k, void* ws, size_t ws_bytes, double* map_host, int32_t* flags_host, xmh_stream_t stream);
/* mean over queries of ap_sum/cap -> map_out[0] (f64, device).  A query with cap == 0 makes the result
 * NaN, as torch.mean of an empty tensor does in the reference (common/calc_utils.py:87-89). */
int xmh_map_finalize(const double* ap_sum, const int32_t* cap, int64_t Q, double* map_out, xmh_stream_t stream);
/* Sharded evaluation (replaces the dense all_reduce gather of runners/base.py:259-264 on the retrieval side):
 * hist_gathered = the all-gathered shard totals of xmh_hamming_hist, [world][2][Q][nbuckets] u32 (plane 0 all items,
 * plane 1 relevant).  Writes the three inputs xmh_hamming_ap takes for shard `rank`: base_all/base_rel [Q][nbuckets] =
 * items in lower buckets on any shard + items of the same bucket on lower ranks; nrel_total [Q]. */
int xmh_shard_offsets(const uint32_t* hist_gathered, int world, int rank, int64_t Q, int nbuckets, uint32_t* base_all,
                      uint32_t* base_rel, uint32_t* nrel_total, xmh_stream_t stream);
/* Sharded evaluation without an export pass.  xmh_hamming_hist leaves this shard's totals table in the workspace:
 * [nbuckets][qpad] pairs of u32 {all items, relevant items} at byte offset xmh_scan_totals_offset() (*bytes = its size; the
 * offset depends on Q, K and ternary only through the plan of THIS shard, the table's shape on Q and K alone).  All-gather those
 * tables as they are -> totals_gathered[world][nbuckets][qpad][2], then xmh_hamming_map_sharded = offsets + pass 2 + this
 * shard's share of the mean (three launches): ap_sum[Q] = this shard's credits, cap[Q] = the global divisor,
 * map_partial[0] = (1/Q) sum_q ap_sum[q] / cap[q].  The mAP is the SUM of map_partial over the shards (one 8-byte all-reduce
 * instead of a [Q] f64 one and a finalize launch). */
size_t xmh_scan_totals_offset(int64_t Q, int64_t R, int K, int ternary, size_t* bytes);
int xmh_hamming_map_sharded(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* qlab, const uint32_t* rbits,
                            const uint32_t* rzero, const uint32_t* rlab, int64_t Q, int64_t R, int K, int C, void* ws,
                            size_t ws_bytes, const uint32_t* totals_gathered, int world, int rank, int64_t k, double* ap_sum,
                            int32_t* cap, double* map_partial, xmh_stream_t stream);

/* The same evaluation with an all-to-all exchange (2 x the table size per rank instead of world x): rank j receives from every
 * shard the columns of ITS slice of `slice` = qpad / world queries -> totals_slices[world][nbuckets][slice][2];
 * xmh_shard_slice_offsets resolves those queries for EVERY shard -> offsets_out[world][nbuckets + 1][slice][2]
 * ({lower buckets anywhere + same bucket on lower shards} per bucket; last row {relevant items, items} over all shards); a second
 * all-to-all returns shard w its rows, ordered by slice owner -> offsets[world][nbuckets + 1][slice][2], which
 * xmh_hamming_map_sharded_offsets turns into pass 2 + this shard's share of the mean exactly like xmh_hamming_map_sharded.
 * Needs qpad % world == 0 (qpad is a multiple of 64; 128 for codes of at most 64 bits). */
int xmh_shard_slice_offsets(const uint32_t* totals_slices, int world, int nbuckets, int slice, uint32_t* offsets_out, xmh_stream_t stream);
int xmh_hamming_map_sharded_offsets(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* qlab, const uint32_t* rbits,
                                    const uint32_t* rzero, const uint32_t* rlab, int64_t Q, int64_t R, int K, int C, void* ws,
                                    size_t ws_bytes, const uint32_t* offsets, int world, int64_t k, double* ap_sum, int32_t* cap,
                                    double* map_partial, xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Per-query top-k (north_star: "fused bit-packed XOR-popcount + per-query top-k kernel").
 * Exact top-k under the canonical order.  dist[Q][k] u16, idx[Q][k] i32 hold GLOBAL indices
 * (base_index + local row).  k <= 1024.  Workspace: xmh_topk_ws_bytes(Q, R, K, k).
 * ------------------------------------------------------------------------------------------- */
size_t xmh_topk_ws_bytes(int64_t Q, int64_t R, int K, int k);
int xmh_hamming_topk(const uint32_t* qbits, const uint32_t* rbits, int64_t Q, int64_t R, int K, int k,
                     int64_t base_index, void* ws, size_t ws_bytes, uint16_t* dist, int32_t* idx,
                     xmh_stream_t stream);
/* The same call on a PREPARED workspace: xmh_topk_ws_init zeroes the control words and the sample histogram at the head of the
 * workspace once, every xmh_hamming_topk_prepared call on it (same Q, R, K, k; one stream at a time) finds them zero and leaves
 * them zero, so a repeated query loop pays no memset launch.  xmh_hamming_topk == init + prepared call. */
int xmh_topk_ws_init(int64_t Q, int64_t R, int K, int k, void* ws, size_t ws_bytes, xmh_stream_t stream);
int xmh_hamming_topk_prepared(const uint32_t* qbits, const uint32_t* rbits, int64_t Q, int64_t R, int K, int k,
                              int64_t base_index, void* ws, size_t ws_bytes, uint16_t* dist, int32_t* idx,
                              xmh_stream_t stream);
/* Ternary codes (round 6).  BaseTrainer.make_hash_code is an in-place sign_() (reference runners/base.py:407-410): an activation of
 * exactly 0 stays 0, and MITH sums two saturating tanh terms before it (runners/MITH/runner.py:125-131), so the code sets of the
 * MITH / DSPH configs can hold -1 / 0 / +1.  Same call with the zero planes of both sides (bit set <=> the element is 0, padding
 * bits set: what xmh_pack_sign writes); the order is the same canonical (distance, index) order over the reference's
 * 0.5 * (K - q.r) (common/calc_utils.py:51-56), and dist2[Q][k] holds that distance in HALF units (K - q.r, 0 ... 2K; 0xFFFF =
 * unused slot) since it is a multiple of 1/2.  Workspace: xmh_topk_ternary_ws_bytes; `prepared` != 0: the workspace went through
 * xmh_topk_ternary_ws_init (or an earlier call) and needs no memset. */
size_t xmh_topk_ternary_ws_bytes(int64_t Q, int64_t R, int K, int k);
int xmh_topk_ternary_ws_init(int64_t Q, int64_t R, int K, int k, void* ws, size_t ws_bytes, xmh_stream_t stream);
int xmh_hamming_topk_ternary(const uint32_t* qbits, const uint32_t* qzero, const uint32_t* rbits, const uint32_t* rzero,
                             int64_t Q, int64_t R, int K, int k, int64_t base_index, void* ws, size_t ws_bytes, int prepared,
                             uint16_t* dist2, int32_t* idx, xmh_stream_t stream);
/* Diagnostics for the measurement harness: writes "filter=<kernel instance>" -- the streaming kernel the fast path of
 * xmh_hamming_topk launches for this shape, spelled as rocprofv3 prints it (the counterpart of xmh_scan_describe).  out_bytes >= 64. */
int xmh_topk_describe(int64_t Q, int64_t R, int K, int k, char* out, size_t out_bytes);
/* Host-side k-way merge of the shards' exact top-k lists (north_star: "partial top-k lists are merged on the host"; replaces the
 * reference's gather of the whole code matrix, runners/base.py:259-264, on the retrieval side).  HOST pointers, no GPU work:
 * gathered_host = `world` records as the ranks all-gathered them, each [Q][k] i32 global indices followed by [Q][k] u16
 * distances (xmh_topk_record_bytes(Q, k) bytes per record, 4-byte aligned); every list ascending in (distance, index) with unused
 * slots (index -1) at its end, which is what xmh_hamming_topk writes.  dist_out / idx_out [Q][k] i32: the k smallest (distance,
 * index) pairs over all shards; slots past the total number of rows carry distance 0xFFFF and index -1. */
size_t xmh_topk_record_bytes(int64_t Q, int k);
int xmh_topk_merge_host(const void* gathered_host, int world, int64_t Q, int k, int32_t* dist_out_host, int32_t* idx_out_host);

/* ---------------------------------------------------------------------------------------------
 * Encoder primitives (a-9 .. a-12).  fp32 activations, token-major [B, L, D].  The Python model classes
 * (xmh/models) chain them exactly like models/CLIP/model.py chains torch ops.
 * ------------------------------------------------------------------------------------------- */
#define XMH_ACT_NONE 0
#define XMH_ACT_QUICKGELU 1   /* x * sigmoid(1.702 x), models/CLIP/model.py:162-164 */
#define XMH_ACT_GELU_ERF 2    /* nn.GELU() of the MITH ResidualMLPs, models/MITH/hash/hash.py:22 */
#define XMH_ACT_TANH 3
#define XMH_ACT_RELU 4
#define XMH_PREC_F32 0        /* v_mfma_f32_32x32x2_f32: exact fp32 products */
#define XMH_PREC_F16 1        /* operands rounded to fp16, fp32 accumulate ("fast mode")     */

/* C[M,N] = act(A[M,K] . W[N,K]^T + bias[N]) (+ residual[M,N]).  W in nn.Linear layout.  bias / residual may
 * be NULL.  Replaces every nn.Linear / MultiheadAttention projection / x @ proj of the reference's encoder. */
int xmh_gemm_nt_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
                    const float* residual, int64_t ldr, float* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                    int act, int precision, xmh_stream_t stream);
/* Fast mode proper: the same contraction with A and W already stored as IEEE fp16 (K % 32 == 0, 16-byte aligned rows);
 * fp32 accumulate, fp32 bias/residual/output.  xmh_cast_f32_to_f16 is the HBM-bound conversion pass (n % 8 == 0). */
int xmh_gemm_nt_h16(const void* A_half, int64_t lda, const void* W_half, int64_t ldw, const float* bias,
                    const float* residual, int64_t ldr, float* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                    int act, xmh_stream_t stream);
int xmh_cast_f32_to_f16(const float* x, void* y_half, int64_t n, xmh_stream_t stream);
/* Parity-grade contraction at fp16-MFMA rate: fp32 A is split into two fp16 planes (a = hi + lo, 22 mantissa bits) by a pass
 * into stream-ordered scratch (hipMallocAsync) and multiplied by the LDS-DMA staged plane kernel; every fp16 x fp16 product is
 * exact in fp32, accumulation is fp32.  (The whole-tower entry points below never take this route: there the producing kernel
 * writes the planes.)
 *   W_lo_half == NULL: W_half must hold fp16-EXACT weights (true for CLIP weights after convert_weights,
 *                      models/CLIP/model.py:415-436): two MFMAs per product, relative error 2^-22;
 *   W_lo_half != NULL: any fp32 weight, given as w = W_half + W_lo_half (host: hi = half(w), lo = half(w - hi)): three MFMAs
 *                      per product (the lo*lo term, 2^-22 relative, is dropped).
 * Domain |a| < 65536: there a = hi + lo to 2^-21 |a| (2^-23 absolute below 2^-3, where the planes turn subnormal).  From 65536
 * up hi saturates at 65504: the result stays finite but is wrong.  inf and NaN in A make their output row non-finite.  (Fast
 * mode's single plane, half(a) rounded to nearest, is inf from 65520 up.)  Same shape rules as xmh_gemm_nt_h16 (16-byte aligned
 * rows, K % 32 == 0). */
int xmh_gemm_nt_split16(const float* A, int64_t lda, const void* W_half, const void* W_lo_half, int64_t ldw, const float* bias,
                        const float* residual, int64_t ldr, float* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                        int act, xmh_stream_t stream);
/* models/CLIP/model.py:153-159 (fp32 LayerNorm) */
int xmh_layernorm_f32(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, float* y,
                      int64_t ldy, int64_t rows, int D, xmh_stream_t stream);
/* nn.MultiheadAttention core inside ResidualAttentionBlock (models/CLIP/model.py:167-197):
 * qkv [B, L, 3*H*dh] -> out [B, L, H*dh]; causal != 0 applies build_attention_mask (:358-364);
 * key_padding_mask [B, L] bytes (non-zero = ignore key) or NULL. */
int xmh_attention_f32(const float* qkv, int64_t B, int L, int H, int dh, int causal, const uint8_t* key_padding_mask,
                      float* out, xmh_stream_t stream);
/* The same attention with the two products on the fp16 MFMA and hi/lo split operands (x = hi + lo, 22 mantissa bits; the scheme of
 * xmh_gemm_nt_split16): product error 2^-22, 5x less matrix time.  What parity and fast mode use; xmh_attention_f32 (exact fp32
 * products) is exact mode.  L > 64 runs the same fp32 kernel as xmh_attention_f32. */
int xmh_attention_split16(const float* qkv, int64_t B, int L, int H, int dh, int causal, const uint8_t* key_padding_mask,
                          float* out, xmh_stream_t stream);
/* Evaluation image transform (reference dataset/transformer_dataset.py:38-42: torchvision Resize((r, r), BICUBIC) +
 * ToTensor + Normalize on a PIL image), bit-exact with Pillow's two-pass 8-bit resample.  images [B][H][W][3] u8 RGB.
 * bounds_x [out][2] = (first input index, count), kk_x [out][ksize_x] = 22-bit fixed-point coefficients (device; built
 * once per image size by the host).  The horizontal pass (W != out_w) writes tmp [B][H][out_w][3] u8 (caller-owned).
 * Outputs (either may be NULL): resized_u8 [B][out_h][out_w][3]; out_chw [B][3][out_h][out_w] f32 =
 * ((u8 / 255) - mean) / std with mean3_host / std3_host three HOST floats each. */
int xmh_image_preprocess_u8(const uint8_t* images, int64_t B, int H, int W, int out_h, int out_w,
                            const int32_t* bounds_w, const int32_t* kk_w, int ksize_w,
                            const int32_t* bounds_h, const int32_t* kk_h, int ksize_h,
                            const float* mean3_host, const float* std3_host, uint8_t* tmp, uint8_t* resized_u8,
                            float* out_chw, xmh_stream_t stream);
/* Training image transform (reference dataset/transformer_dataset.py:34-40: torchvision RandomHorizontalFlip +
 * RandomResizedCrop(r) + ToTensor + Normalize on a PIL image) for a RAGGED batch, every image with its own crop and flip:
 *     Image.fromarray(a) [.transpose(FLIP_LEFT_RIGHT)] .crop((left, top, left + w, top + h)) .resize((r, r), Image.BILINEAR)
 * to the bit (Pillow's two-pass 8-bit resample; its coefficient tables are computed on the device, per image and axis, in
 * double), then ((u8 / 255) - mean) / std.  The random draw is the caller's.
 * One descriptor per image, a DEVICE array: `offset` = byte offset of the image's first uploaded pixel in `pixels` (rows of
 * W * 3 bytes, RGB); H, W = rows and columns uploaded; top, left, h, w = the crop box in the coordinates of the FLIPPED image
 * (the reference flips, then crops): crop column x reads source column flip ? W - 1 - (left + x) : left + x. */
typedef struct {
    int64_t offset;
    int32_t H, W;
    int32_t top, left, h, w;
    int32_t flip;
    int32_t reserved;
} xmh_crop_desc;
/* bytes of workspace for a batch of B crops of at most max_h x max_w pixels resized to r x r (coefficient tables of
 * 2 * ceil(max(max_x / r, 1)) + 1 taps per output pixel and the horizontal pass's uint8 rows); 0 for shapes the call refuses. */
size_t xmh_image_preprocess_train_ws_bytes(int64_t B, int max_h, int max_w, int r);
/* pixels: `pixel_bytes` bytes on the device; desc [B] on the device; max_h / max_w: upper bounds of desc[].h / desc[].w (they size
 * the launches and the tables: three launches whatever B is, no host synchronisation, no allocation).  Outputs (either may be
 * NULL): resized_u8 [B][r][r][3]; out_chw [B][3][r][r] f32 with mean3_host / std3_host three HOST floats each.  The host can only
 * check what it sees (B, r, the bounds, null pointers, the workspace size: XMH_EINVAL / XMH_ENOMEM); the kernels clamp every
 * source coordinate into its image and every byte index into `pixels`, so a bad descriptor never reads outside the buffer.
 * B == 0 is XMH_OK. */
int xmh_image_preprocess_train_u8(const uint8_t* pixels, int64_t pixel_bytes, const xmh_crop_desc* desc, int64_t B, int max_h,
                                  int max_w, int r, const float* mean3_host, const float* std3_host, void* workspace,
                                  size_t workspace_bytes, uint8_t* resized_u8, float* out_chw, xmh_stream_t stream);
/* VisionTransformer.conv1 input gather (models/CLIP/model.py:219,235): image [B,C,res,res] -> cols [B*G*G, C*P*P] */
int xmh_im2col_patch(const float* image, int64_t B, int channels, int resolution, int patch, float* cols,
                     xmh_stream_t stream);
/* class token + positional embedding + ln_pre (models/CLIP/model.py:237-243) -> x [B, n_patches+1, D] */
int xmh_vit_assemble(const float* patch_out, const float* cls, const float* pos, const float* gamma, const float* beta,
                     float eps, float* x, int64_t B, int n_patches, int D, xmh_stream_t stream);
/* token + positional embedding and EOS position = argmax(ids) (models/CLIP/model.py:374-379) */
int xmh_text_embed(const int64_t* ids, const float* tok_emb, const float* pos, float* x, int32_t* eos_index, int64_t B,
                   int L, int D, int vocab, xmh_stream_t stream);
/* out[r] = x[r*group + (idx ? idx[r] : offset)]   (cls row: offset 0, group L; EOS row: idx) */
int xmh_gather_rows(const float* x, int64_t ldx, const int32_t* idx, int offset, int group, float* out, int64_t rows,
                    int D, xmh_stream_t stream);
/* eval BatchNorm1d of the DCMHT image head (models/DCMHT/hash/hash.py:22,40) */
int xmh_affine_cols(const float* x, const float* mean, const float* var, const float* gamma, const float* beta,
                    float eps, float* y, int64_t rows, int D, xmh_stream_t stream);
/* softmax over each consecutive pair: softmax_hash (models/common/hash.py:21-31); x, y [rows, 2K] */
int xmh_pair_softmax(const float* x, float* y, int64_t rows, int K, xmh_stream_t stream);

/* MITH LocalizedTokenAggregation (models/MITH/hash/hash.py:109-169) + sin/cos positional encoding (:41-65):
 * scores [B,L,K] (tanh concept scores of every token), tokens [B,L,D] (raw CLIP tokens), token_mask [B,L] bytes
 * (non-zero = padded / EOS token, may be NULL), pos_enc [K,D] or NULL -> out [B,K,D]. */
int xmh_lta_aggregate(const float* scores, const float* tokens, const uint8_t* token_mask, const float* pos_enc,
                      float* out, int64_t B, int L, int K, int D, int top_k, xmh_stream_t stream);
/* MITH BitwiseHashing (models/MITH/hash/hash.py:68-85): out[b,k] = tanh(w[k,:] . z[b,k,:] + bias[k]) (+ addend[b,k],
 * the cls_hash + tokens_hash sum of runners/MITH/runner.py:129-130 when given). */
int xmh_bitwise_hash(const float* z, const float* w, const float* bias, const float* addend, float* out, int64_t B,
                     int K, int D, xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Whole-tower entry points: the CLIP ViT / text forward of models/CLIP/model.py as ONE call each (the kernel chain of
 * the primitives above, enqueued from C++: ~150 launches per tower without a host round trip per primitive).
 * All pointers are device pointers except the descriptor structs themselves and `blocks`, which live on the host.
 * ------------------------------------------------------------------------------------------- */
/* nn.Linear / MHA projection / `x @ proj` (W [N, K], row-major).  The three precisions of xmh_gemm_nt_* read different
 * members: exact (2) w_f32; parity (0) w_hi (+ w_lo for weights that are not fp16-exact), else w_f32 when w_hi is NULL or the
 * shape is unaligned; fast (1) w_hi. */
typedef struct xmh_linear {
    const float* w_f32;
    const void* w_hi;      /* IEEE fp16 [N, K] = half(W), or NULL */
    const void* w_lo;      /* IEEE fp16 [N, K] = half(W - w_hi) when W is not fp16-exact, else NULL */
    const float* bias;     /* [N] or NULL */
    int64_t n, k;
} xmh_linear;
/* ResidualAttentionBlock (models/CLIP/model.py:167-197) */
typedef struct xmh_clip_block {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b;
    xmh_linear qkv, out, fc, proj;
} xmh_clip_block;
/* VisionTransformer (models/CLIP/model.py:206-268) */
typedef struct xmh_vit_weights {
    int resolution, patch, width, heads, layers, out_dim;
    xmh_linear conv1;                                  /* [width, 3*patch*patch], no bias */
    const float *cls, *pos, *ln_pre_w, *ln_pre_b, *ln_post_w, *ln_post_b;
    xmh_linear proj;                                   /* visual.proj TRANSPOSED: [out_dim, width] */
    const xmh_clip_block* blocks;                      /* host array [layers] */
} xmh_vit_weights;
/* text tower of CLIP (models/CLIP/model.py:373-396) */
typedef struct xmh_text_weights {
    int vocab, context, width, heads, layers, out_dim;
    const float *tok_emb, *pos, *ln_final_w, *ln_final_b;
    xmh_linear proj;                                   /* text_projection TRANSPOSED: [out_dim, width] */
    const xmh_clip_block* blocks;
} xmh_text_weights;
/* bytes of caller-owned scratch the calls below need for B items of L tokens at `width` (conv_k = 3*patch*patch for the image
 * tower, 0 for text; out_dim > 0 only when all tokens are projected) */
size_t xmh_clip_workspace_bytes(int64_t B, int L, int width, int conv_k, int out_dim, int precision);
/* Transformer.forward (models/CLIP/model.py:200-211) on token-major x [B, L, width], in place. */
int xmh_clip_blocks_forward(const xmh_clip_block* blocks, int layers, int width, int heads, float* x, int64_t B, int L,
                            int causal, const uint8_t* key_padding_mask, int precision, void* workspace,
                            size_t workspace_bytes, xmh_stream_t stream);
/* The same forward with every activation a backward pass of ResidualAttentionBlock (models/CLIP/model.py:167-197) reads kept per
 * layer instead of in the shared scratch ("forward kernels with saved activations"; no backward is built here).
 * `saved` holds `layers` records of 16 * B*L*width floats (xmh_clip_saved_bytes), each record the row-major fp32 fields
 *     x_in [M, D] | ln1 [M, D] | qkv [M, 3D] | attn [M, D] | x_mid [M, D] | ln2 [M, D] | fc_pre [M, 4D] | fc_act [M, 4D]      (M = B*L, D = width)
 * x_in = the residual stream entering the block, ln1 = ln_1(x_in), qkv = in_proj(ln1), attn = the heads' outputs before out_proj,
 * x_mid = x_in + out_proj(attn), ln2 = ln_2(x_mid), fc_pre = c_fc(ln2), fc_act = QuickGELU(fc_pre); the block's output is the
 * next record's x_in, the last block's output is x (in place, bit-identical to xmh_clip_blocks_forward in every precision).
 * The library's own statement of this layout, shared by the forward and the backward: csrc/xmh_clip_record.h. */
size_t xmh_clip_saved_bytes(int64_t B, int L, int width, int layers);
int xmh_clip_blocks_forward_saved(const xmh_clip_block* blocks, int layers, int width, int heads, float* x, int64_t B, int L,
                                  int causal, const uint8_t* key_padding_mask, int precision, void* workspace,
                                  size_t workspace_bytes, float* saved, size_t saved_bytes, xmh_stream_t stream);
/* Backward of the block stack from the record of xmh_clip_blocks_forward_saved: exact fp32 products, the fp32 weights
 * (w_f32) of the descriptors, the record layout above exactly as it stands.
 * xmh_clip_block_grads: where the gradients of one layer's twelve parameters go (device pointers, the parameters' own shapes:
 * qkv_w [3D, D], out_w [D, D], fc_w [4D, D], proj_w [D, 4D]); NULL = a frozen parameter, and a product nothing downstream needs is
 * not launched.  dy [B, L, width] is the gradient of the stack's output; it is updated in place and holds dx, the gradient of the
 * residual stream entering the stack, on return (need_dx != 0).  accumulate != 0: every parameter gradient is added to what its
 * buffer holds, else overwritten.  need_dx == 0: the walk stops at the lowest layer with any non-NULL gradient pointer -- nothing
 * below it is read, neither its record nor its weights nor its descriptor -- and inside that layer the products that only feed dx
 * are skipped; dy is then scratch.  Limits as the forward's: width % 4 == 0, width / heads == 64, L <= 128 (XMH_ENOTSUP beyond;
 * B * L <= 2^21); -12 for a short saved buffer or workspace, -22 for null or misfitting arguments.  A key padding mask that hides
 * every key of a query gives NaN, as in the reference.  No host synchronisation, no allocation, no float atomics: every reduction
 * is summed in one fixed order, two calls on equal inputs agree to the bit. */
typedef struct xmh_clip_block_grads {
    float *ln1_w, *ln1_b, *qkv_w, *qkv_b, *out_w, *out_b, *ln2_w, *ln2_b, *fc_w, *fc_b, *proj_w, *proj_b;
} xmh_clip_block_grads;
size_t xmh_clip_blocks_backward_ws_bytes(int64_t B, int L, int width);
int xmh_clip_blocks_backward(const xmh_clip_block* blocks, int layers, int width, int heads, int64_t B, int L, int causal,
                             const uint8_t* key_padding_mask, const float* saved, size_t saved_bytes, float* dy, int need_dx,
                             const xmh_clip_block_grads* grads, int accumulate, void* workspace, size_t workspace_bytes,
                             xmh_stream_t stream);
/* VisionTransformer.forward: image [B, 3, r, r] f32 -> out_cls [B, out_dim]; out_tokens [B, L, out_dim] (L = patches + 1,
 * every token through ln_post and proj: the return_patches mode, row 0 of each item = the cls feature) or NULL.
 * Exactly one of out_cls / out_tokens may be NULL. */
int xmh_vit_b32_forward(const xmh_vit_weights* w, const float* image, int64_t B, int precision, float* out_cls,
                        float* out_tokens, void* workspace, size_t workspace_bytes, xmh_stream_t stream);
/* CLIP.encode_text: ids [B, L] i64 (+ key_padding_mask [B, L] bytes or NULL) -> out_eos [B, out_dim] (feature of the EOS
 * token, argmax(ids)); out_tokens [B, L, out_dim] or NULL; eos_index [B] i32 or NULL (the EOS positions). */
int xmh_text_forward(const xmh_text_weights* w, const int64_t* ids, const uint8_t* key_padding_mask, int64_t B, int L,
                     int precision, float* out_eos, float* out_tokens, int32_t* eos_index, void* workspace,
                     size_t workspace_bytes, xmh_stream_t stream);
/* The same tower when only out_eos is wanted, on PACKED rows: caption b takes part with its tokens up to and including EOS only
 * (row_offsets [B + 1] i32 on the device, row_offsets[b + 1] - row_offsets[b] = argmax(ids[b]) + 1; total_rows = row_offsets[B], a
 * HOST value that sizes the launches).  Under the causal mask of CLIP.encode_text (models/CLIP/model.py:358-364, :373-396) nothing
 * behind a caption's EOS token can reach the row :392 selects, so out_eos is bit-identical to xmh_text_forward's -- at
 * sum(lengths) / (B L) of the work.  No key padding mask, no token outputs (callers that need those use xmh_text_forward); L <= 64;
 * workspace as for xmh_text_forward (xmh_clip_workspace_bytes(B, L, width, 0, 0, precision)). */
int xmh_text_forward_packed(const xmh_text_weights* w, const int64_t* ids, const int32_t* row_offsets, int64_t total_rows, int64_t B,
                            int L, int precision, float* out_eos, void* workspace, size_t workspace_bytes, xmh_stream_t stream);
/* The packed tower with the caption lengths counted ON THE DEVICE: no host value sizes anything, so the call never synchronises (the
 * image and text towers' streams do not wait on a host thread; the call can be captured in a hipGraph).  Launches are sized for B * L
 * rows and return on the rows behind the real count.
 *   key_padding_mask [B, L] bytes or NULL (MITH: models/MITH/MITH.py:59-66 -> models/CLIP/model.py:378): applied to the keys as in
 *     xmh_text_forward.  Caption b keeps its rows up to EOS, or up to the last position the mask leaves visible if that lies further
 *     back: every row a consumer may read unmasked is computed exactly as in xmh_text_forward.
 *   out_tokens [B, L, out_dim] or NULL (return_patches, models/CLIP/model.py:391-395): kept rows bit-identical to xmh_text_forward's;
 *     the dropped rows -- all of them hidden by key_padding_mask, or behind EOS when there is no mask -- are returned as ZERO, where the
 *     reference returns what attention made of padding.  A caller that reads those rows (the reference's own consumers mask them:
 *     models/MITH/hash/hash.py:142-148) must use xmh_text_forward.
 *   out_eos [B, out_dim] or NULL: bit-identical to xmh_text_forward's.
 * Parity / fast mode only (-ENOTSUP in exact mode); L <= 64; workspace = xmh_clip_workspace_bytes(B, L, width, 0, out_tokens ? out_dim : 0, precision). */
int xmh_text_forward_packed_dev(const xmh_text_weights* w, const int64_t* ids, const uint8_t* key_padding_mask, int64_t B, int L,
                                int precision, float* out_eos, float* out_tokens, void* workspace, size_t workspace_bytes,
                                xmh_stream_t stream);

/* The two towers in TRAINING mode: a forward that keeps what backward reads, and the backward to every parameter of
 * the tower.  Exact fp32 throughout: the descriptors' w_f32 members point at the parameters in place (proj is still the TRANSPOSED
 * projection, [out_dim, width]), the other members are not read.  The forwards are the calls of xmh_vit_b32_forward /
 * xmh_text_forward in precision 2 with the block stack run through xmh_clip_blocks_forward_saved: same bits.  There is no
 * return_patches mode and no gradient to the image.
 * saved (xmh_*_train_saved_bytes, 256-byte aligned device memory): the block record of xmh_clip_blocks_forward_saved, the rows in
 * front of ln_pre [B, L, width] (image only), and the B rows entering ln_post / ln_final.  workspace: xmh_*_train_ws_bytes, one
 * size for the forward and the backward.  L of the image tower is (resolution / patch)^2 + 1, conv_k = 3 * patch * patch.
 * Gradients have the PARAMETERS' own shapes: proj [width, out_dim] (not the descriptor's), pos [L, width] (text: [context, width],
 * the rows at or beyond L zero), cls [width], conv1 [width, conv_k], tok [vocab, width] (dense; a row whose id does not occur is
 * zero; ids outside the table count for the row the forward reads, 0 or vocab - 1).  NULL = a frozen parameter, and a product that
 * nothing asked-for depends on is not launched.  `blocks`: host array [layers], as for xmh_clip_blocks_backward.  accumulate != 0:
 * every gradient is added to what its buffer holds, else overwritten.
 * Limits as the block stack's: width % 4 == 0, width <= 1024, width / heads == 64, L <= 128, B * L <= 2^21, patch % 4 == 0
 * (XMH_ENOTSUP beyond); -12 for a short saved buffer or workspace, -22 for null or misfitting arguments.  No host synchronisation,
 * no allocation, no float atomics: every reduction is summed in one fixed order, two calls on equal inputs agree to the bit. */
typedef struct xmh_vit_grads {
    float *proj, *ln_post_w, *ln_post_b, *ln_pre_w, *ln_pre_b, *pos, *cls, *conv1;
    const xmh_clip_block_grads* blocks;
} xmh_vit_grads;
typedef struct xmh_text_grads {
    float *proj, *ln_final_w, *ln_final_b, *pos, *tok;
    const xmh_clip_block_grads* blocks;
} xmh_text_grads;
size_t xmh_vit_train_saved_bytes(int64_t B, int L, int width, int layers);
size_t xmh_vit_train_ws_bytes(int64_t B, int L, int width, int conv_k, int out_dim);
/* image [B, 3, r, r] -> out_cls [B, out_dim] */
int xmh_vit_train_forward(const xmh_vit_weights* w, const float* image, int64_t B, float* out_cls, void* saved, size_t saved_bytes,
                          void* workspace, size_t workspace_bytes, xmh_stream_t stream);
/* g [B, out_dim] -> the gradients named in grads; image and saved are the forward's */
int xmh_vit_backward(const xmh_vit_weights* w, const float* image, int64_t B, const void* saved, size_t saved_bytes, const float* g,
                     const xmh_vit_grads* grads, int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream);
size_t xmh_text_train_saved_bytes(int64_t B, int L, int width, int layers);
size_t xmh_text_train_ws_bytes(int64_t B, int L, int width, int out_dim);
/* ids [B, L] i64 (+ key_padding_mask [B, L] bytes or NULL) -> out_eos [B, out_dim] and eos_index [B] i32 (both required) */
int xmh_text_train_forward(const xmh_text_weights* w, const int64_t* ids, const uint8_t* key_padding_mask, int64_t B, int L,
                           float* out_eos, int32_t* eos_index, void* saved, size_t saved_bytes, void* workspace,
                           size_t workspace_bytes, xmh_stream_t stream);
/* g [B, out_dim] -> the gradients named in grads; ids, key_padding_mask, eos_index and saved are the forward's */
int xmh_text_backward(const xmh_text_weights* w, const int64_t* ids, const uint8_t* key_padding_mask, const int32_t* eos_index,
                      int64_t B, int L, const void* saved, size_t saved_bytes, const float* g, const xmh_text_grads* grads,
                      int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream);

/* The same towers with their TOKEN outputs (return_patches=True, models/CLIP/model.py:257-267 and :386-395): the last
 * LayerNorm and the projection run on all B * L rows, as xmh_vit_b32_forward / xmh_text_forward run them for out_tokens in
 * precision 2 (same bits), and the backward takes a gradient for the one row and for the tokens.  Descriptors, grads structs,
 * limits, return codes and the conventions above are unchanged; `saved` holds all B * L rows entering the last LayerNorm instead
 * of B, and the workspace the B * L rows of the back end (xmh_*_train_tokens_saved_bytes / _ws_bytes: not the sizes above).
 *   image  out_cls [B, out_dim] (row 0) and out_tokens [B, L - 1, out_dim] (rows 1...), both dense and both required
 *   text   out_eos [B, out_dim] (row eos_index[b]), out_tokens [B, L, out_dim] and eos_index [B], all required
 *   backward  g_cls / g_eos [B, out_dim] and g_tokens (the shape of out_tokens); either may be NULL and counts as zeros, both NULL
 *             is -22.  g_eos[b] is added onto row eos_index[b] (clamped to [0, L)), which also carries its row of g_tokens. */
size_t xmh_vit_train_tokens_saved_bytes(int64_t B, int L, int width, int layers);
size_t xmh_vit_train_tokens_ws_bytes(int64_t B, int L, int width, int conv_k, int out_dim);
int xmh_vit_train_forward_tokens(const xmh_vit_weights* w, const float* image, int64_t B, float* out_cls, float* out_tokens, void* saved,
                                 size_t saved_bytes, void* workspace, size_t workspace_bytes, xmh_stream_t stream);
int xmh_vit_backward_tokens(const xmh_vit_weights* w, const float* image, int64_t B, const void* saved, size_t saved_bytes,
                            const float* g_cls, const float* g_tokens, const xmh_vit_grads* grads, int accumulate, void* workspace,
                            size_t workspace_bytes, xmh_stream_t stream);
size_t xmh_text_train_tokens_saved_bytes(int64_t B, int L, int width, int layers);
size_t xmh_text_train_tokens_ws_bytes(int64_t B, int L, int width, int out_dim);
int xmh_text_train_forward_tokens(const xmh_text_weights* w, const int64_t* ids, const uint8_t* key_padding_mask, int64_t B, int L,
                                  float* out_eos, float* out_tokens, int32_t* eos_index, void* saved, size_t saved_bytes,
                                  void* workspace, size_t workspace_bytes, xmh_stream_t stream);
int xmh_text_backward_tokens(const xmh_text_weights* w, const int64_t* ids, const uint8_t* key_padding_mask, const int32_t* eos_index,
                             int64_t B, int L, const void* saved, size_t saved_bytes, const float* g_eos, const float* g_tokens,
                             const xmh_text_grads* grads, int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream);

/* One modality of the DCMHT head in eval mode (models/DCMHT/hash/hash.py:15-82): MultiheadAttention over a length-1
 * sequence == out_proj(v_proj(x)) (softmax over one key is 1), BatchNorm1d with running statistics (image) or LayerNorm
 * (text), fc2 + relu, softmax over each (off, on) pair. */
typedef struct xmh_dcmht_head {
    xmh_linear v_proj;                                 /* rows [2E, 3E) of atten.in_proj_weight / in_proj_bias */
    xmh_linear out_proj;                               /* atten.out_proj */
    int norm_is_batchnorm;                             /* 1: bn_mean / bn_var are used; 0: LayerNorm */
    float norm_eps;
    const float *norm_w, *norm_b, *bn_mean, *bn_var;
    xmh_linear fc2;                                    /* [2K, E] */
} xmh_dcmht_head;
size_t xmh_head_workspace_bytes(int64_t B, int E, int precision);
/* emb [B, E] -> probs [B, 2K] (what DCMHT.encode_image / encode_text return) and/or the packed K-bit code of
 * DCMHTTrainer.make_hash_code (runners/DCMHT/runner.py:82-95: bit = p_on > p_off) scattered to rows row_index[i] (NULL:
 * row i).  probs or bits may be NULL, not both. */
int xmh_head_dcmht(const xmh_dcmht_head* h, const float* emb, int64_t B, int precision, float* probs, uint32_t* bits,
                   const int64_t* row_index, void* workspace, size_t workspace_bytes, xmh_stream_t stream);
/* DSPH head in eval mode (models/DSPH/hash/hash.py:6-45): out = tanh(fc(emb)) [B, K]; and/or the sign-quantised packed
 * code of BaseTrainer.make_hash_code (runners/base.py:407-410) with its zero plane and value flags (see xmh_pack_sign). */
int xmh_head_dsph(const xmh_linear* fc, const float* emb, int64_t B, int precision, float* out, uint32_t* bits,
                  uint32_t* zero, int32_t* flags, const int64_t* row_index, void* workspace, size_t workspace_bytes,
                  xmh_stream_t stream);

/* One modality of the MITH head in eval mode (models/MITH/hash/hash.py:172-254; dataflow SURVEY 2.4):
 *   GlobalConceptLearning: y = ResidualMLPs(x) (per layer x += fc2(gelu(fc1(LN(x))))), concept scores tanh(E y), on the cls /
 *   EOS feature -> cls_hash [B, K] and on every token -> scores [B, L, K];
 *   LocalConceptTransforming: localized token aggregation of the RAW tokens by those scores (+ positional encoding)
 *   -> [B, K, D], transformer blocks over the K concept tokens, bitwise hashing -> tokens_hash [B, K]. */
typedef struct xmh_mith_mlp {
    const float *ln_w, *ln_b;
    float ln_eps;
    xmh_linear fc1, fc2;                               /* [4D, D], [D, 4D] */
} xmh_mith_mlp;
typedef struct xmh_mith_head {
    int width, k_bits, top_k, res_layers, layers, heads;
    const xmh_mith_mlp* mlps;                          /* host array [res_layers] */
    xmh_linear concept;                                /* common_concept_embedding [K, D], no bias */
    const float* pos_enc;                              /* [K, D] (already divided by sqrt(D)) */
    const xmh_clip_block* blocks;                      /* host array [layers] */
    const float *hash_w, *hash_b;                      /* the K one-row linears stacked: [K, D], [K] */
} xmh_mith_head;
size_t xmh_head_mith_workspace_bytes(int64_t B, int L, int width, int k_bits, int precision);
/* cls [B, D], tokens [B, L, D] (contiguous), token_mask [B, L] bytes (non-zero = ignore) or NULL
 * -> cls_hash [B, K], tokens_hash [B, K] (what MITH.encode_image / encode_text return as elements 1 and 2). */
int xmh_head_mith(const xmh_mith_head* h, const float* cls, const float* tokens, const uint8_t* token_mask, int64_t B, int L,
                  int precision, float* cls_hash, float* tokens_hash, void* workspace, size_t workspace_bytes,
                  xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Float similarities of common/calc_utils.py on un-quantised inputs (a-3, a-4).
 * ------------------------------------------------------------------------------------------- */
/* y = x / ||x|| row-wise (cosine_similarity :38-49, no eps) and/or sqnorm[r] = ||x_r||^2; y or sqnorm may be NULL */
int xmh_row_l2normalize(const float* x, int64_t rows, int D, float* y, float* sqnorm, xmh_stream_t stream);
/* in place: gram[i][j] = sqrt(max(|a_i|^2 + |b_j|^2 - 2 gram[i][j], 0))   (euclidean_similarity :28-36) */
int xmh_pairwise_l2_from_gram(float* gram_inout, const float* sqnorm_a, const float* sqnorm_b, int64_t M, int64_t N,
                              xmh_stream_t stream);
/* in place: x = alpha * x + beta   (0.5 * (K - q.r) on float codes, calc_hammingDist :51-56) */
int xmh_affine_inplace(float* x, int64_t n, float alpha, float beta, xmh_stream_t stream);
/* calc_map_k on FLOAT "codes" (values outside {-1, 0, +1}: UMoED-style raw tanh outputs, reference runners/UMoED/runner.py:162-186) the
 * way the reference computes it (common/calc_utils.py:72-89): distances 0.5 * (K - qB . rB^T) by exact-fp32 GEMM (:51-56), ONE stable
 * sort per query (:76-77; a segmented LSD radix sort, ties in gallery-index order = torch.sort(stable=True)), the first min(n_rel, k)
 * relevant ranks (:81-89).  SURVEY 8(b)'s xmh_gemm_f32_sort_map.  qB [Q][K], rB [R][K] fp32 row-major, packed label masks as
 * xmh_pack_labels writes them; k <= 0: mAP@all.  Outputs like xmh_hamming_ap (ap_sum[Q] f64, cap[Q] i32) and, when map_out is not
 * NULL, the mean over the queries like xmh_map_finalize.  Also the route of every code set the bit-packed kernels have no instance for
 * (ternary codes above 256 bits, more than 2048 bits, more than 256 classes): the drop-in never refuses what the reference evaluates.
 * Workspace: xmh_gemm_f32_sort_ws_bytes(Q, R) (a query tile of at most 1.5 GB: 20 bytes per pair); any size from one row
 * (20 R + 1280 bytes) up is accepted and sets the tile.  R < 2^31. */
size_t xmh_gemm_f32_sort_ws_bytes(int64_t Q, int64_t R);
int xmh_gemm_f32_sort_map(const float* qB, const float* rB, const uint32_t* qlab, const uint32_t* rlab, int64_t Q, int64_t R,
                          int K, int C, int64_t k, void* ws, size_t ws_bytes, double* ap_sum, int32_t* cap, double* map_out,
                          xmh_stream_t stream);
/* The ranking half alone, for a distance matrix the caller holds: dist[Q][R] any floats, same order, same outputs.
 * Workspace: 16 Q R + 1280 bytes. */
int xmh_float_sort_ap(const float* dist, const uint32_t* qlab, const uint32_t* rlab, int64_t Q, int64_t R, int C, int64_t k,
                      void* ws, size_t ws_bytes, double* ap_sum, int32_t* cap, xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Loss of the DCMHT objective: forward, and its gradient with respect to the two code matrices (what
 * loss.backward() of runners/DCMHT/runner.py:124 hands to the hash heads).  The backward of the encoders is out of scope.
 * ------------------------------------------------------------------------------------------- */
/* similarity_loss (models/DCMHT/DCMHT.py:72-98) of one pair of code matrices a, b [B, D] with packed multi-hot labels lab
 * [B][ceil(C/32)] (label_sim = calc_label_sim(labels, labels), common/calc_utils.py:8-10).  cosine == 0: euclidean branch with
 * max_value = sqrt(2 K vartheta) (:81-88); cosine != 0: the cosine branch with `threshold` (:92-95).
 * out2 (device, 2 doubles) = (positive_loss, negative_loss).  A NaN distance or cosine (a NaN entry, a zero row under cosine) makes
 * both outputs NaN, as the reference's clip does; the gradient below is then NaN in every row that pairs with it.  D <= 12288. */
int xmh_pair_similarity_loss(const float* a, const float* b, int64_t B, int D, const uint32_t* lab, int C, int cosine,
                             float max_value, float threshold, double* out2, xmh_stream_t stream);
/* soft_argmax_hash_loss (models/DCMHT/DCMHT.py:100-105): out (device, 1 double) = 1 - mean((2 code - 1)^2) over n elements */
int xmh_quant_loss(const float* code, int64_t n, double* out, xmh_stream_t stream);
/* d(positive_loss + negative_loss)/da of xmh_pair_similarity_loss, as autograd derives it from models/DCMHT/DCMHT.py:72-98
 * (torch.cdist's backward: zero distances contribute nothing; clip passes the gradient on the closed interval).  grad_a [B, D]
 * (device) is written, or added to when accumulate != 0, with scale * upstream[0] (upstream: device float, NULL = 1) folded in.
 * The gradient with respect to b is the same call with a and b exchanged; for a term with a == b pass scale = 2.
 * (D + B) * 4 <= 65536 (one code row and one row of pair weights in LDS; XMH_ENOTSUP beyond). */
int xmh_pair_similarity_loss_grad(const float* a, const float* b, int64_t B, int D, const uint32_t* lab, int C, int cosine,
                                  float max_value, float threshold, float scale, const float* upstream, float* grad_a,
                                  int accumulate, xmh_stream_t stream);
/* d xmh_quant_loss / d code = -4 (2 code - 1) / n, times scale * upstream[0], written or accumulated like above */
int xmh_quant_loss_grad(const float* code, int64_t n, float scale, const float* upstream, float* grad, int accumulate,
                        xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * TwDH objective (models/TwDH/TwDH.py:125-230) and the backward of its short-code transforms.  A stream is one code
 * length: stream 0 the long code, then every short length; stream s owns bits [bit[s], bit[s] + K[s]) of the K_tot target bits, the
 * streams tiling [0, K_tot) in order.  Probabilities come per modality as long [B, 2 K[0]] and short [B, 2 (K_tot - K[0])] (the short
 * streams side by side), one (off, on) pair per bit, fp32, 8-byte aligned.  B <= 4096, K_tot <= 4096, C <= 1024 (XMH_ENOTSUP beyond).
 * No call synchronises with the host or allocates; every sum runs in one fixed order (two calls on equal inputs agree to the bit).
 * ------------------------------------------------------------------------------------------- */
#define XMH_TWDH_MAX_STREAMS 8
typedef struct {
    int32_t n;                               /* streams, the long one included */
    int32_t bit[XMH_TWDH_MAX_STREAMS];       /* first target bit of the stream */
    int32_t K[XMH_TWDH_MAX_STREAMS];         /* its code length */
} xmh_twdh_streams;
/* hash_convert(hash_center_multilables(labels, centre)) (:192-230) of all streams in one launch, as bits.  lab [B][ceil(C/32)] as
 * xmh_pack_labels writes it; centres [C][K_tot] int8, every entry +1 or -1 (the caller checks); tie [K_tot] int8 +-1, the
 * reference's random_center.  targets [B][ceil(K_tot/32)]: bit k = sign of the integer sum of the centres of the row's set labels,
 * tie[k] > 0 where the sum is zero, 0 for a row without a label (the reference's NaN mean); padding bits 0. */
int xmh_twdh_targets(const uint32_t* lab, int C, const int8_t* centres, const int8_t* tie, int64_t B, int K_tot, uint32_t* targets,
                     xmh_stream_t stream);
/* out (device, 1 + 6 * n doubles): out[0] the total (:160-164: (bce_img + bce_txt) / 2 + quan_alpha (q_img + q_txt) / 2 over
 * the long stream plus low_rate times each of the two for every short stream); out[1 + (m * n + s) * 2 + t]: modality m (0 image,
 * 1 text), stream s, t = 0 nn.BCELoss (mean over B * 2 K[s], each log clamped at -100) against the pair (1, 0) / (0, 1) of the
 * target bit, t = 1 soft_argmax_hash_loss = 1 - mean((2 p - 1)^2); out[1 + 4 * n + 2 * s + t]: the mean of the two modalities' term t
 * of stream s (the reference's short_nce_loss / short_quan_loss).  A modality whose pointers are NULL contributes zeros.  A NaN
 * probability makes its terms and the total NaN.  Workspace: xmh_twdh_loss_ws_bytes(B, n) (XMH_ENOMEM when shorter).  2 launches. */
size_t xmh_twdh_loss_ws_bytes(int64_t B, int n_streams);
int xmh_twdh_loss(const xmh_twdh_streams* streams, const float* img_long, const float* img_short, const float* txt_long,
                  const float* txt_short, const uint32_t* targets, int64_t B, double quan_alpha, double low_rate, double* out,
                  void* workspace, size_t workspace_bytes, xmh_stream_t stream);
/* d total / d p of ONE modality, times upstream[0] (device float, NULL = 1): weight * ((p - t) / max(p (1 - p), 1e-12) / n), what
 * autograd returns for nn.BCELoss, plus weight_q * (-4 (2 p - 1) / n), n = B * 2 K[s]; the weights 1/2 and quan_alpha / 2 for the
 * long stream, low_rate / 2 for both terms of a short one.  d_long [B, 2 K[0]] / d_short are written; either may be NULL (then its
 * streams are not computed: with low_rate == 0 the short gradient is an exact zero).  1 launch. */
int xmh_twdh_loss_grad(const xmh_twdh_streams* streams, const float* p_long, const float* p_short, const uint32_t* targets, int64_t B,
                       double quan_alpha, double low_rate, const float* upstream, float* d_long, float* d_short, xmh_stream_t stream);
/* quantization(long_hash.matmul(trans)) (:66-85) of every short length at once: p_short [B, 2S] = pair_softmax(long_probs [B, 2L] .
 * T_cat), the transforms concatenated along their columns; trans_t [2S, 2L] is T_cat TRANSPOSED (the nn.Linear layout
 * xmh_gemm_nt_f32 takes).  Exact fp32 products.  2 launches (the product, the softmax in place). */
int xmh_twdh_short_forward(const float* long_probs, const float* trans_t, int64_t B, int L2, int S2, float* p_short,
                           xmh_stream_t stream);
/* Its backward: g_z = p (g - (g0 p0 + g1 p1)) per pair, then g_long [B, 2L] = g_z . T_cat^T, added to g_long when accumulate != 0.
 * trans [2L, 2S] is T_cat itself.  Workspace: 4 * B * 2S bytes (g_z), 8-byte aligned (XMH_ENOMEM when shorter).  2 launches. */
int xmh_twdh_short_backward(const float* g_short, const float* p_short, const float* trans, int64_t B, int L2, int S2, float* g_long,
                            int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream);
/* The stage that makes a transform (runners/TwDH/transform_matrix_generation).  M [2L, 2S] fp32 is the matrix being
 * trained; targets [B][ceil((L + S) / 32)] are xmh_twdh_targets' words for the two streams bit = {0, L}, K = {L, S}.  With
 * x = hash_convert(t_long) (one-hot pairs, never written), z = x . M is the gather z[b][j] = sum_l M[2 l + bit_l(b)][j] and
 * p = pair_softmax(z).  B <= 4096, L + S <= 4096, C <= 1024 (XMH_ENOTSUP beyond); workspace of xmh_twdh_trans_ws_bytes(B, L, S)
 * bytes (0: out of range), 8-byte aligned (XMH_ENOMEM when shorter).  Elements are computed in double and rounded once.
 * out4 (device doubles): total = hash + bce + lasso, hash = 1 - mean_{b,s}((p[b,2s] - p[b,2s+1])^2), bce = nn.BCELoss()(p,
 * hash_convert(t_short)) (mean over B 2S, each log clamped at -100), lasso = alpha |M|_1.  A NaN in M makes the terms it reaches, and
 * the total, NaN (the gather reads only the selected row of a pair: the logits of the rows that select the entry).  2 launches. */
size_t xmh_twdh_trans_ws_bytes(int64_t B, int L, int S);
int xmh_twdh_trans_loss(const float* M, const uint32_t* targets, int64_t B, int L, int S, double alpha, void* workspace,
                        size_t workspace_bytes, double* out4, xmh_stream_t stream);
/* dM [2L, 2S] = upstream[0] (device float, NULL = 1) times (x^T g_z + alpha sign(M)), sign(0) = 0: g = (p - t) / max(p (1 - p), 1e-12)
 * / (B 2S) -+ 2 (p0 - p1) / (B S), g_z = p (g - (g0 p0 + g1 p1)), dM[2 l + c][j] = the sum of g_z[b][j] over the rows b whose long bit
 * l is c, b ascending.  Written, or added to dM when accumulate != 0.  2 launches. */
int xmh_twdh_trans_grad(const float* M, const uint32_t* targets, int64_t B, int L, int S, double alpha, const float* upstream, float* dM,
                        int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream);
/* The generator's stopping criterion (train.py:87-96): argmax over each pair of hash_convert(long_centre) . M against short_centre > 0,
 * equal logits (and a NaN) giving bit 0.  centres [C][L + S] int8 +-1, long then short.  wrong (device int32): wrong[0] the number of
 * class / bit pairs that disagree, then a [C][ceil(S/32)] bitmap of them (bit s of class c: word c * ceil(S/32) + s / 32, bit s % 32).
 * Logits are summed in double.  A memset of the count and 1 launch; no host synchronisation. */
int xmh_twdh_trans_check(const float* M, const int8_t* centres, int C, int L, int S, int32_t* wrong, xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * HyP loss of DSPH (models/DSPH/loss/HyP.py:18-70): forward, and its gradient with respect to the two code matrices and the
 * proxies (what loss.backward() of runners/DSPH/runner.py:123 hands to the hash heads and to the proxies' own optimiser).
 * x, y [B, K] fp32 (image / text codes), P [C, K] fp32 (proxies), lab [B][ceil(C/32)] as xmh_pack_labels writes it.
 * B <= 4096, K <= 4096, C <= 1024 (XMH_ENOTSUP beyond).  Both calls count P_num, N_num and the regulariser's pairs on the device
 * (no host synchronisation, no allocation) and sum in one fixed order (two calls on the same inputs agree to the bit).
 * Workspace: xmh_hyp_loss_ws_bytes(B, K, C) bytes of device memory, 256-byte aligned (0 for a shape outside the bounds).
 * ------------------------------------------------------------------------------------------- */
size_t xmh_hyp_loss_ws_bytes(int64_t B, int K, int C);
/* out8 (device, 8 doubles) = (loss, pos, neg, pos_t, neg_t, reg, reg_t, reg_xt); loss is their sum.  P_num == 0 or N_num == 0
 * gives NaN terms (0 / 0) as the reference does; alpha <= 0, or no pair of multi-label rows with disjoint labels, gives reg = 0.
 * Non-finite inputs are not masked: a NaN or Inf in a proxy or a code row makes every term NaN that one of its cosines enters (the
 * hinge keeps a NaN as F.relu does), and with it the loss; the other terms stay finite. */
int xmh_hyp_loss(const float* x, const float* y, const float* P, int64_t B, int K, int C, const uint32_t* lab,
                 float threshold, float alpha, void* ws, size_t ws_bytes, double* out8, xmh_stream_t stream);
/* d loss / d x, d y, d P as autograd derives them from the reference's expression (relu'(0) = 0; F.normalize's backward, a row
 * clamped by its eps receiving du / 1e-12).  grad_x [B, K], grad_y [B, K] and grad_P [C, K] (device, all required) are written,
 * or added to when accumulate != 0, with upstream[0] (device float, NULL = 1) folded in.
 * Non-finite inputs give the NaN rows of the reference's backward, not a finite gradient: a NaN or Inf in proxy c makes every row of
 * grad_x and grad_y and row c of grad_P NaN; one in a code row makes that row of its gradient and every row of grad_P NaN, and,
 * when the row has two or more labels and the regulariser is live, the grad_x and grad_y rows of every such row (the reference's pair
 * products multiply every multi-label row in, masked pairs with weight 0). */
int xmh_hyp_loss_grad(const float* x, const float* y, const float* P, int64_t B, int K, int C, const uint32_t* lab,
                      float threshold, float alpha, const float* upstream, float* grad_x, float* grad_y, float* grad_P,
                      int accumulate, void* ws, size_t ws_bytes, xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * MITH's training objective (models/MITH/MITH.py:116-232): forward, and its gradient with respect to its eight inputs (what
 * loss.backward() of runners/MITH/runner.py:121 hands to the hash heads).  All tensors are fp32, contiguous, on the device:
 *   res_img_cls, res_txt_cls [B, D]; img_cls_hash, txt_cls_hash, tokens_hash_i, tokens_hash_t [B, K];
 *   trans_tokens_i, trans_tokens_t [K, B, D] (the reference's LND layout, read in place);
 *   buffer [N, K] the rolling code buffer AFTER this step's row write (on the GPU the reference's four buffers are one tensor);
 *   label_sim [N, B] any float similarity.
 * The weights are the reference's hyper_* (defaults 1, 1, 50, 10, 8, 0.01, 0.99); temperature is InfoNCE's (0.07).
 * N <= 2^22, B <= 1024, K <= 256, D <= 2048 (XMH_ENOTSUP beyond); no alignment requirement on K or D.  Neither call
 * synchronises with the host or allocates; sums run in one fixed order (two calls on the same inputs agree to the bit).
 * Workspace: xmh_mith_loss_ws_bytes(N, B, K, D) bytes of device memory, 256-byte aligned (0 for a shape outside the bounds).
 * ------------------------------------------------------------------------------------------- */
typedef struct xmh_mith_loss_args {
    int64_t N;
    int B, K, D;
    const float* res_img_cls;
    const float* res_txt_cls;
    const float* img_cls_hash;
    const float* txt_cls_hash;
    const float* tokens_hash_i;
    const float* tokens_hash_t;
    const float* trans_tokens_i;
    const float* trans_tokens_t;
    const float* buffer;
    const float* label_sim;
    double hyper_tokens_intra, hyper_distill, hyper_info_nce, hyper_cls_inter, hyper_quan, hyper_alpha, hyper_lambda;
    double temperature;
} xmh_mith_loss_args;
size_t xmh_mith_loss_ws_bytes(int64_t N, int B, int K, int D);
/* out10 (device, 10 doubles) = (loss, intra_i, intra_t, i2t, t2i, quan_i, quan_t, nce_cls, nce_tokens, distillation): the
 * unweighted terms of the reference's loss_dict except distillation, which is weighted as there; loss is the weighted total.
 * Non-finite inputs are not masked: a NaN in a buffer row or a code row (or Inf entries that cancel to NaN in a dot product) stays NaN
 * through the clamp, as through torch's, and makes the likelihoods that product enters and the loss NaN; a NaN code or feature entry
 * makes the quantisation, distillation or InfoNCE terms it enters NaN; the other terms stay finite.  The buffer keeps a poisoned row
 * until that row is written again, so every step that reads it reports a NaN loss, as the reference does. */
int xmh_mith_loss(const xmh_mith_loss_args* args, void* ws, size_t ws_bytes, double* out10, xmh_stream_t stream);
/* grads: 8 device pointers in the input order (res_img_cls, res_txt_cls, img_cls_hash, txt_cls_hash, tokens_hash_i, tokens_hash_t,
 * trans_tokens_i, trans_tokens_t), each with its input's shape, or NULL when that gradient is not needed.  They are written, or
 * added to when accumulate != 0, with upstream[0] (device float, NULL = 1) folded in.  The clamp's gradient passes on the closed
 * interval [-64, 64], as torch's does, and is 0 for a NaN dot product (a select, as in torch's clamp backward): a non-finite entry
 * k of a buffer row turns entry k of every row of the four code gradients NaN (0 * NaN) and nothing else; a NaN code entry turns
 * that entry of the gradients it enters elementwise NaN; a NaN feature entry turns both gradients of its InfoNCE problem NaN. */
int xmh_mith_loss_grad(const xmh_mith_loss_args* args, const float* upstream, float* const* grads, int accumulate, void* ws,
                       size_t ws_bytes, xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * DCMHT / DSPH hash heads in TRAINING mode: forward that keeps what backward reads, and backward to every parameter of the head
 * and to the input embeddings (models/DCMHT/hash/hash.py:15-46, models/DSPH/hash/hash.py:6-15).  Plain fp32 weight
 * pointers, exact-fp32 FMA products (not the precision-tagged xmh_linear descriptors: cached weight planes go stale after every
 * optimiser step).  B <= 4096, E <= 2048, N <= 1024 (XMH_ENOTSUP beyond); no alignment requirement on B, E or K.  No call
 * synchronises with the host or allocates; every sum has one fixed order (two calls on the same inputs agree to the bit).
 * ------------------------------------------------------------------------------------------- */
typedef struct xmh_dcmht_train {
    const float *wv, *bv;                              /* rows [2E, 3E) of atten.in_proj_weight [E, E] / in_proj_bias [E] */
    const float *wo, *bo;                              /* atten.out_proj [E, E], [E] */
    const float *norm_w, *norm_b;                      /* [E] */
    float *running_mean, *running_var;                 /* BatchNorm: [E], updated in place by forward; NULL = not tracked */
    const float *w2, *b2;                              /* fc2 [N, E], [N] with N = 2K */
    int norm_is_batchnorm;                             /* 1: BatchNorm1d with batch statistics; 0: LayerNorm */
    float eps, momentum;
} xmh_dcmht_train;
/* where backward puts each gradient; NULL = not needed (its product is not launched) */
typedef struct xmh_dcmht_grads {
    float *d_wv, *d_bv, *d_wo, *d_bo, *d_norm_w, *d_norm_b, *d_w2, *d_b2;   /* shapes of the parameters above */
    float* d_x;                                        /* [B, E] */
} xmh_dcmht_grads;
/* bytes of the saved buffer (returned) and of the workspace (*workspace_bytes, may be NULL) for one head at this shape; both
 * 256-byte aligned device memory, both non-decreasing in B.  0 for a shape outside the bounds or an odd N.
 * Saved buffer, each section rounded up to 256 bytes: v [B, E], nhat [B, E] (normalised, before the affine), n [B, E] (after it),
 * rstd [max(B, E)] (per column for BatchNorm, per row for LayerNorm), f [B, N] (relu output: its sign is backward's mask),
 * probs [B, N].  x is not copied: the caller hands the same x to backward. */
size_t xmh_head_dcmht_train_bytes(int64_t B, int E, int N, size_t* workspace_bytes);
/* x [B, E] -> probs [B, N].  BatchNorm: batch mean and biased variance normalise; running_mean / running_var move by `momentum`
 * towards the batch mean / the UNBIASED batch variance (num_batches_tracked is the caller's); B = 1 is XMH_EINVAL. */
int xmh_head_dcmht_train_forward(const xmh_dcmht_train* h, const float* x, int64_t B, int E, int N, float* probs, void* saved,
                                 size_t saved_bytes, void* workspace, size_t workspace_bytes, xmh_stream_t stream);
/* d_probs [B, N] -> the gradients named in g.  Parameter gradients are written, or added to when accumulate != 0; d_x is always
 * written.  `saved` is what the forward of the SAME x and parameters filled (the relu mask is taken from it, never re-derived). */
int xmh_head_dcmht_backward(const xmh_dcmht_train* h, const float* x, const float* d_probs, int64_t B, int E, int N,
                            const void* saved, size_t saved_bytes, const xmh_dcmht_grads* g, int accumulate, void* workspace,
                            size_t workspace_bytes, xmh_stream_t stream);
/* The same head with a CROSS-RANK BatchNorm (distributed training; norm_is_batchnorm only, else XMH_EINVAL): each of
 * the two calls above in two halves, and between the halves the caller gathers one statistics row per rank.  A row is
 * xmh_head_dcmht_stats_len(E) = 2 E + 2 doubles on the device: a [E], b [E], the rank's row count, 0.  `table` is the rows of all
 * `world` ranks in rank order, contiguous.  saved and workspace are those of xmh_head_dcmht_train_bytes for THIS rank's B; the
 * workspace carries o (forward) / dn (backward) from the first half to the second and must be kept in between.
 *   forward_stats   the products up to o; row = local column mean, local M2 = sum (o - mean)^2 (the two double passes of the fused
 *                   call), B.
 *   forward_apply   (n, mean, M2) of the ranks combined in rank order by the pairwise update -- every rank derives the same bits --,
 *                   this rank's rows normalised with the global mean and biased variance, the running statistics moved by momentum
 *                   towards the global mean and the UNBIASED global variance (n_total - 1), then fc2 / relu / pair softmax; fills
 *                   the saved buffer as the fused call does (rstd is the same on every rank).
 *   backward_stats  d_w2, d_b2 and dn; row = local column sums of dn nhat and of dn, B.  They are formed whatever g leaves out: the
 *                   other ranks wait for this rank's row.
 *   backward_apply  d_norm_w / d_norm_b from row `rank`, THIS rank's sums (the gradient all-reduce averages them like every other
 *                   gradient); the rows added in rank order; do = gamma rstd (dn - mean(dn) - nhat mean(dn nhat)) with the means
 *                   over n_total; the remaining products.
 * B = 1 is legal when another rank brings rows; a global batch of one row (world == 1 and B == 1) is XMH_EINVAL.  With world == 1
 * the two halves compute what the fused call computes, to the bit. */
int64_t xmh_head_dcmht_stats_len(int E);
int xmh_head_dcmht_train_forward_stats(const xmh_dcmht_train* h, const float* x, int64_t B, int E, int N, void* saved, size_t saved_bytes,
                                       void* workspace, size_t workspace_bytes, double* stats_row, xmh_stream_t stream);
int xmh_head_dcmht_train_forward_apply(const xmh_dcmht_train* h, const float* x, int64_t B, int E, int N, const double* table, int world,
                                       float* probs, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes,
                                       xmh_stream_t stream);
int xmh_head_dcmht_backward_stats(const xmh_dcmht_train* h, const float* x, const float* d_probs, int64_t B, int E, int N,
                                  const void* saved, size_t saved_bytes, const xmh_dcmht_grads* g, int accumulate, void* workspace,
                                  size_t workspace_bytes, double* stats_row, xmh_stream_t stream);
int xmh_head_dcmht_backward_apply(const xmh_dcmht_train* h, const float* x, int64_t B, int E, int N, const double* table, int world,
                                  int rank, const void* saved, size_t saved_bytes, const xmh_dcmht_grads* g, int accumulate,
                                  void* workspace, size_t workspace_bytes, xmh_stream_t stream);
/* y [B, K] = tanh(keep * (x w^T + b) / (1 - p)): w [K, E], b [K], keep [B, K] bytes (non-zero = kept) or NULL for no dropout.
 * The library draws no random numbers. */
int xmh_head_dsph_train_forward(const float* w, const float* b, const float* x, const uint8_t* keep, float p, int64_t B, int E,
                                int K, float* y, xmh_stream_t stream);
/* d_y [B, K] and the forward's y, keep, p -> d_w [K, E], d_b [K] (written, or added to when accumulate != 0), d_x [B, E]
 * (written); each may be NULL.  Workspace: 4 B K bytes of device memory. */
int xmh_head_dsph_backward(const float* w, const float* x, const float* y, const uint8_t* keep, float p, const float* d_y,
                           int64_t B, int E, int K, float* d_w, float* d_b, float* d_x, int accumulate, void* workspace,
                           size_t workspace_bytes, xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * MITH hash head in TRAINING mode: one modality of HashLayer.encode_img / encode_txt (models/MITH/hash/hash.py:231-247) as a
 * forward that keeps what backward reads and a backward to every head parameter of that modality and to the two inputs
 * (DESIGN 3.14).  Exact fp32 over the parameters in place: only the w_f32 / bias members of the descriptors are read.
 *   cls path (carries gradient): y = ResidualMLPs(cls), cls_hash = tanh(y Wc^T), res_cls = y / max(|y|, 1e-12);
 *   token scores: the same GlobalConceptLearning on the B L token rows -> scores [B, L, K], detached as in the reference (:235);
 *   LTA: xmh_lta_aggregate's selection and softmax, M = A X + pe, the attention A [B, K, L] kept;
 *   z = the transformer blocks over M [B, K, D] (sequence length K, no mask), through xmh_clip_blocks_forward_saved;
 *   tokens_hash[b,k] = tanh(w_k . z[b,k,:] + b_k); trans_tokens = normalize(z Wp^T + bp), written [K, B, D].
 * cls_hash and tokens_hash carry the bits of xmh_head_mith in precision 2.  B = 1 returns [1, K] (the reference's torch.squeeze
 * collapses that shape).  saved == NULL (forward): no record is kept, same outputs.
 * Gradients have the parameters' shapes; the K one-row hash layers are stacked, hash_w [K, D], hash_b [K].  NULL = frozen, and a
 * product nothing asked-for depends on is not launched.  Each of the four upstream gradients may be NULL (that output was not used):
 * what only that path feeds is then written as exact zeros.  accumulate != 0: parameter gradients are added to what their buffers
 * hold; d_cls [B, D] and d_tokens [B, L, D] are always written.  d_tokens flows through A X only (the scores carry no gradient,
 * pos_enc is a buffer): rows of masked tokens, and the contribution of a concept no token of the sample scores positively for, are
 * exactly zero.
 * Limits: K <= 128, D % 4 == 0, D <= 1024, D / heads == 64, res_layers <= 4, LayerNorm eps 1e-5, B L and B K <= 2^21, L (K + 2) <=
 * 40960 (XMH_ENOTSUP beyond); -12 for a short saved buffer or workspace, -22 for null or misfitting arguments, all reported
 * without a GPU.  No host synchronisation, no allocation, no float atomics; every sum has one fixed order (two calls on equal
 * inputs agree to the bit).
 * ------------------------------------------------------------------------------------------- */
typedef struct xmh_mith_train {
    xmh_mith_head head;                                /* as for xmh_head_mith */
    xmh_linear proj;                                   /* img_concept_proj / txt_concept_proj [D, D] with bias */
} xmh_mith_train;
typedef struct xmh_mith_mlp_grads {
    float *ln_w, *ln_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} xmh_mith_mlp_grads;
typedef struct xmh_mith_grads {
    const xmh_mith_mlp_grads* mlps;                    /* host array [res_layers] (may be NULL when res_layers == 0) */
    float* concept;                                    /* [K, D] */
    const xmh_clip_block_grads* blocks;                /* host array [layers] (may be NULL when layers == 0) */
    float *hash_w, *hash_b;                            /* [K, D], [K] */
    float *proj_w, *proj_b;                            /* [D, D], [D] */
    float *d_cls, *d_tokens;                           /* [B, D], [B, L, D] */
} xmh_mith_grads;
/* 256-byte aligned device memory; 0 for a shape outside the limits.  One workspace size serves the forward and the backward. */
size_t xmh_mith_train_saved_bytes(int64_t B, int L, int width, int k_bits, int res_layers, int layers);
size_t xmh_mith_train_ws_bytes(int64_t B, int L, int width, int k_bits, int res_layers);
/* cls [B, D], tokens [B, L, D] (contiguous), token_mask [B, L] bytes (non-zero = ignore) or NULL
 * -> res_cls [B, D], cls_hash [B, K], tokens_hash [B, K], trans_tokens [K, B, D] (all required) */
int xmh_mith_train_forward(const xmh_mith_train* h, const float* cls, const float* tokens, const uint8_t* token_mask, int64_t B, int L,
                           float* res_cls, float* cls_hash, float* tokens_hash, float* trans_tokens, void* saved, size_t saved_bytes,
                           void* workspace, size_t workspace_bytes, xmh_stream_t stream);
/* upstream gradients g_* in the outputs' shapes (each may be NULL) -> the gradients named in grads; cls and saved are the forward's */
int xmh_mith_train_backward(const xmh_mith_train* h, const float* cls, int64_t B, int L, const float* g_res_cls, const float* g_cls_hash,
                            const float* g_tokens_hash, const float* g_trans_tokens, const void* saved, size_t saved_bytes,
                            const xmh_mith_grads* grads, int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * BertAdam (models/common/optimizer.py:50-167): one optimiser step over any number of fp32 tensors in two launches.
 * Per tensor: norm = |g|_2; coef = min(1, max_grad_norm / (norm + 1e-6)) when max_grad_norm > 0, else 1; g' = g coef;
 * m = m b1 + (1 - b1) g'; v = v b2 + (1 - b2) g' g'; u = m / (sqrt(v) + e), plus weight_decay p when weight_decay > 0; p -= lr u.
 * p, m, v are written; g' is written back only where coef < 1 (or NaN).  No bias correction.  A NaN or infinite gradient follows
 * IEEE as the reference does (NaN norm -> NaN coef -> that tensor's p, m, v, g NaN) and touches that tensor only.
 * table [n_tensors] and chunk_map [total_chunks] are DEVICE arrays the caller fills; the call does not read them on the host.
 *   chunk_map lists the chunks of tensor 0, then of tensor 1, ...: tensor t has ceil(numel / xmh_bertadam_chunk()) chunks, its
 *   j-th chunk is {start = j * chunk, tensor = t, first_chunk = index of the tensor's chunk 0 in the map}.
 * Limits: numel >= 1 per tensor (leave empty tensors out), total_chunks <= 2^31 - 1 (XMH_ENOTSUP beyond); p, g, m, v need 4-byte
 * alignment only (16-byte accesses where all four are 16-byte aligned, dword accesses otherwise) and must not overlap.
 * No host synchronisation, no allocation, no atomics, fixed summation order (two calls on the same inputs agree to the bit).
 * Workspace: xmh_bertadam_ws_bytes(n_tensors, total_chunks) bytes of device memory, 256-byte aligned (0 for bad counts).
 * ------------------------------------------------------------------------------------------- */
typedef struct xmh_bertadam_tensor {
    float *p, *g, *m, *v;                              /* parameter, its gradient, next_m, next_v: numel fp32 each, contiguous */
    int64_t numel;
    float lr;                                          /* this tensor's SCHEDULED rate (the host's double, cast) */
    float b1, b2;
    float one_minus_b1, one_minus_b2;                  /* (float)(1.0 - b1) of the host's doubles, as the reference's alpha / value */
    float e, weight_decay, max_grad_norm;
} xmh_bertadam_tensor;                                 /* 72 bytes */
typedef struct xmh_bertadam_chunk_ref {
    int64_t start;                                     /* first element of the chunk within its tensor */
    int32_t tensor;                                    /* index into table */
    int32_t first_chunk;                               /* map index of this tensor's first chunk */
} xmh_bertadam_chunk_ref;                              /* 16 bytes */
/* elements per chunk (one block each); fixed for a build */
int64_t xmh_bertadam_chunk(void);
size_t xmh_bertadam_ws_bytes(int64_t n_tensors, int64_t total_chunks);
/* n_tensors == 0 is a successful no-op; negative counts, null pointers, a short or misaligned workspace are XMH_EINVAL. */
int xmh_bertadam_step(const xmh_bertadam_tensor* table, int64_t n_tensors, const xmh_bertadam_chunk_ref* chunk_map,
                      int64_t total_chunks, void* ws, size_t ws_bytes, xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Gradient bucket of distributed training (xmh/ddp.py): any number of fp32 tensors packed into, or scattered out of, ONE
 * flat fp32 buffer in one launch.
 *   pack:   flat[offset_i + j] = t_i[j] * scale for j < numel_i (one fp32 product, round to nearest); a row whose t is NULL writes
 *           numel_i zeros; then flat[flag_at_i] = flag_i where flag_at_i >= 0 (the flag tail: one float per tensor behind the last one,
 *           1.0 = this rank had a gradient, 0.0 = it had none, so that a SUM all-reduce of the bucket also counts the ranks that had one).
 *   unpack: t_i[j] = flat[offset_i + j]; a row whose t is NULL is skipped; flag and flag_at are not read.
 * Elements of flat between the tensors (padding) are neither read nor written.
 * table [n_tensors] and chunk_map [total_chunks] are DEVICE arrays the caller fills; the chunk map is BertAdam's (above), over the
 * rows' numel, with xmh_bertadam_chunk() elements per chunk.
 * Limits: numel >= 1 per row; offset a multiple of 4 floats (the callers use 64) and flat 16-byte aligned, so the flat side moves in
 * 16-byte accesses; a tensor needs 4-byte alignment only (16-byte accesses where it is 16-byte aligned, dword accesses otherwise, the
 * last numel % 4 elements as dwords).  A tensor may be its own range of flat (pack in place).  total_chunks <= 2^31 - 1.
 * No host synchronisation, no allocation, no atomics.  n_tensors == 0 is a successful no-op; negative counts, null pointers and a
 * misaligned table, map or flat buffer are XMH_EINVAL.
 * ------------------------------------------------------------------------------------------- */
typedef struct xmh_bucket_tensor {
    float* t;                                          /* the tensor: source of pack, destination of unpack; NULL: see above */
    int64_t offset;                                    /* its first element in flat */
    int64_t numel;
    int64_t flag_at;                                   /* pack: the element of flat that receives flag, or -1 */
    float flag;
    int32_t reserved;                                  /* 0 */
} xmh_bucket_tensor;                                   /* 40 bytes */
int xmh_bucket_pack(const xmh_bucket_tensor* table, int64_t n_tensors, const xmh_bertadam_chunk_ref* chunk_map, int64_t total_chunks,
                    float scale, float* flat, xmh_stream_t stream);
int xmh_bucket_unpack(const xmh_bucket_tensor* table, int64_t n_tensors, const xmh_bertadam_chunk_ref* chunk_map, int64_t total_chunks,
                      const float* flat, xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * DNPH (reference models/DNPH): the proxy + class-prediction + noise objective, its gradients, the noise assignment, and the
 * backward of a plain linear layer (the class-prediction layers).  DESIGN 3.18.
 *
 * f_img, f_txt [B, K] fp32 (the codes), p_img, p_txt [B, Cp] fp32 (class logits), P [C, K] fp32 (proxies), lab [B][ceil(C/32)] as
 * xmh_pack_labels writes it for C classes, noise_img / noise_txt [B, K] fp32 +-1 or NULL (no noise term of that modality).
 *   u = normalize(cat(f_img, f_txt)), q = normalize(P) (eps 1e-12); D[n][c] = |u_n - q_c|^2 + mrg l[n][c]
 *   p_loss = mean over the 2B rows of sum_c -l log_softmax(-D[n][:])[c]
 *   d_loss_m = mean_b CE(p_m[b], t[b]), t[b] the lowest set class of row b (0 for a row without one)
 *   noise_m = mean_b sum_k f_m noise_m;  loss = p_loss + d_loss_img + d_loss_txt - noise_alpha (noise_img + noise_txt)
 * Cp is the width of the prediction layers (the reference always builds them with 80 outputs), C the number of proxies: Cp >= C,
 * else XMH_EINVAL.  B <= 4096, K <= 4096, C <= 1024, Cp <= 1024 (XMH_ENOTSUP beyond).  No host synchronisation, no allocation, no
 * float atomics, every sum in one fixed order (two calls agree to the bit); non-finite inputs pass through as through the
 * reference's expression.  Workspace: xmh_dnph_loss_ws_bytes(B, K, C, Cp) bytes of device memory, 256-byte aligned (0 for a shape
 * outside the bounds; XMH_ENOMEM when shorter).  Argument errors are reported before any launch.  2 launches per call.
 * ------------------------------------------------------------------------------------------- */
size_t xmh_dnph_loss_ws_bytes(int64_t B, int K, int C, int Cp);
/* out8 (device doubles): loss, p_loss, d_loss_img, d_loss_txt, noise_img, noise_txt, 0, 0 */
int xmh_dnph_loss(const float* f_img, const float* f_txt, const float* p_img, const float* p_txt, const float* P, int64_t B, int K,
                  int C, int Cp, const uint32_t* lab, float mrg, float noise_alpha, const float* noise_img, const float* noise_txt,
                  void* ws, size_t ws_bytes, double* out8, xmh_stream_t stream);
/* d loss times upstream[0] (a device float; NULL = 1) -> grad_f_img, grad_f_txt [B, K], grad_p_img, grad_p_txt [B, Cp], grad_P
 * [C, K]: written, or added to when accumulate != 0.  Each may be NULL: that gradient is not formed. */
int xmh_dnph_loss_grad(const float* f_img, const float* f_txt, const float* p_img, const float* p_txt, const float* P, int64_t B,
                       int K, int C, int Cp, const uint32_t* lab, float mrg, float noise_alpha, const float* noise_img,
                       const float* noise_txt, const float* upstream, float* grad_f_img, float* grad_f_txt, float* grad_p_img,
                       float* grad_p_txt, float* grad_P, int accumulate, void* ws, size_t ws_bytes, xmh_stream_t stream);
/* HOST function, no GPU call: the square linear sum assignment, exact (shortest augmenting paths, Jonker-Volgenant).  cost [n][n]
 * row-major host doubles, all finite; col_of_row [n] receives the column of every row, the total cost minimal.  n <= 4096
 * (XMH_ENOTSUP beyond).  A function of the matrix alone: ties are broken by column order. */
int xmh_assign_min_cost(const double* cost, int n, int* col_of_row);
/* y = x w^T + b backward: d_y [B, N], x [B, E], w [N, E] -> d_w [N, E], d_b [N] (written, or added to when accumulate != 0), d_x
 * [B, E] (written); each may be NULL.  The fixed-order exact-fp32 products of the hash heads' backward.  B <= 4096, E <= 2048,
 * N <= 1024 (XMH_ENOTSUP beyond).  No workspace is needed (NULL, 0 is accepted; a non-NULL one must be 256-byte aligned).
 * 2 launches with every gradient asked for. */
int xmh_linear_backward(const float* w, const float* x, const float* d_y, int64_t B, int E, int N, float* d_w, float* d_b, float* d_x,
                        int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * DIMCH: the objective over token sets and codes (reference models/DIMCH/DIMCH.py:152-234) and its gradients (csrc/xmh_dimch.hip).
 * e_img, e_txt [B, M, K] fp32 token embeddings (M set members per sample), h_img, h_txt [B, Kh] fp32 codes, lab: xmh_pack_labels
 * of the [B, C] 0 / 1 labels.  N = B M; x, y = F.normalize (eps 1e-12) of the token rows viewed as [N, K]; G = u v^T.
 *   s(u, v)[i][j] over the M x M block of G of set i of u and set j of v, by mode:
 *     smooth_chamfer  (1 / den) [ (1 / (M tau sigma)) sum_a log sum_b exp(tau sigma G_ab) + (1 / (M tau)) sum_b log sum_a exp(tau G_ab) ]
 *     chamfer         (1 / den) [ (1 / M) sum_a max_b G_ab + (1 / M) sum_b max_a G_ab ]
 *     max             max_ab G_ab          avg   mean_ab sigmoid(G_ab)
 *   D_i2t = clamp(1 - s(x, y), 0), D_t2i = clamp(1 - s(y, x), 0)
 *   T(D, m): c[a][p] label overlap, sim = c > 0, Z[a] = sum_j (2^c_(j) - 1) / log2(j + 2) over row a sorted descending,
 *            w = (2^c - 1) / Z, t[a][p][n] = (w[a][p] - w[a][n]) sim[a][p] (1 - sim[a][n]) (D[a][p] - D[a][n] + m),
 *            T = sum max(t, 0) / (#{t > 1e-16} + 1e-16).  A row without a label makes it NaN, as in the reference.
 *   MMD = mean exp(-gamma |x_a - x_b|) - 2 mean exp(-gamma |x_a - y_b|) + mean exp(-gamma |y_a - y_b|) over all N x N pairs
 *   U(u) = sum_{a < b} exp(-20 |u_a - u_b|^2) / (M (M - 1) / 2) over all N rows, 0 for M = 1
 *   Th_i2t = T(clamp(1 - cos(h_img, h_txt), 0), triplet_margin), Th_t2i with the roles swapped (cos clamps each norm at 1e-8)
 *   Q = mean (h - sign h)^2 (tanh) or 1 - mean (2 h - 1)^2 (softmax)
 *   loss = (T_i2t + T_t2i) / 2 triplet_alpha + mmd_alpha MMD + unif_alpha (U(x) + U(y)) + (Th_i2t + Th_t2i) / 2 hash_triplet_alpha
 *          + (Q_img + Q_txt) / 2 quan_alpha
 * B <= 512, M <= 64, K, Kh <= 256, C <= 127 (2^c leaves fp32 beyond) -- XMH_ENOTSUP outside.  No host synchronisation, no allocation,
 * no float atomics, every sum in one fixed order (two calls agree to the bit); non-finite inputs pass through.  For max and chamfer
 * the gradient goes to the first maximum.  Workspace: xmh_dimch_loss_ws_bytes(B, M, K, C) bytes of device memory, 256-byte aligned,
 * O(N K + B^2) (0 for a shape outside the bounds; XMH_ENOMEM when shorter).  Argument errors are reported before any launch.
 * xmh_dimch_loss: 4 launches.  xmh_dimch_loss_grad: 6 launches (it stands alone: nothing is kept from the forward call).
 * ------------------------------------------------------------------------------------------- */
#define XMH_DIMCH_SMOOTH_CHAMFER 0
#define XMH_DIMCH_CHAMFER 1
#define XMH_DIMCH_MAX 2
#define XMH_DIMCH_AVG 3
#define XMH_DIMCH_TANH 0
#define XMH_DIMCH_SOFTMAX 1
typedef struct xmh_dimch_consts {
    int mode;      /* XMH_DIMCH_SMOOTH_CHAMFER .. XMH_DIMCH_AVG */
    int hash_func; /* XMH_DIMCH_TANH or XMH_DIMCH_SOFTMAX: which quantisation term */
    float denominator, temperature, temperature_txt_scale;
    float token_triplet_margin, triplet_margin, mmd_gamma;
    float triplet_alpha, mmd_alpha, unif_alpha, hash_triplet_alpha, quan_alpha;
} xmh_dimch_consts;
size_t xmh_dimch_loss_ws_bytes(int64_t B, int M, int K, int C);
/* out12 (device doubles): loss, T_i2t, T_t2i, MMD, U(x) + U(y), Th_i2t, Th_t2i, Q_img, Q_txt, 0, 0, 0.  cst is read on the host. */
int xmh_dimch_loss(const float* e_img, const float* e_txt, const float* h_img, const float* h_txt, int64_t B, int M, int K, int Kh,
                   int C, const uint32_t* lab, const xmh_dimch_consts* cst, void* ws, size_t ws_bytes, double* out12,
                   xmh_stream_t stream);
/* d loss times upstream[0] (a device float; NULL = 1) -> grad_e_img, grad_e_txt [B, M, K], grad_h_img, grad_h_txt [B, Kh]: written,
 * or added to when accumulate != 0.  Each may be NULL: that gradient is not formed.  The backward of the normalisation and of both
 * clamps is included. */
int xmh_dimch_loss_grad(const float* e_img, const float* e_txt, const float* h_img, const float* h_txt, int64_t B, int M, int K, int Kh,
                        int C, const uint32_t* lab, const xmh_dimch_consts* cst, const float* upstream, float* grad_e_img,
                        float* grad_e_txt, float* grad_h_img, float* grad_h_txt, int accumulate, void* ws, size_t ws_bytes,
                        xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * DIMCH token-set head, one modality (reference models/DIMCH/hash/hash.py:18-52; csrc/xmh_head_grad.hip):
 *   tokens [B, T, E] -> relu(Conv1d(T -> M, kernel 3, padding 1) along E) -> relu(. w1^T + b1) [B M, H] -> dropout -> . w2^T + b2 =
 *   embeds [B, M, K] -> mean over the M set members -> tanh, or the softmax over the pairs (2j, 2j + 1) = hash [B, K].
 * All weights are plain fp32 device pointers in the reference's layouts; every product is exact fp32 with one fixed summation order.
 * B M <= 32768, B <= 65535, T <= 256, E, H <= 2048, K <= 256 (XMH_ENOTSUP beyond; K even for the softmax).
 * xmh_head_dimch_bytes -> bytes of the buffer that the forward fills (inference: its workspace; train mode: what backward reads -- the two
 * relu outputs and the pooled pre-activation) and, through *workspace_bytes, of backward's workspace; both 0 outside the bounds.
 * Buffers are device memory, 256-byte aligned.  The library draws no random numbers: keep is the caller's [B M, H] 0 / 1 byte mask.
 * xmh_head_dimch and xmh_head_dimch_train_forward: 5 launches (the same kernels: train mode with keep == NULL is inference to the bit).
 * xmh_head_dimch_backward: 9 launches with every gradient asked for, fewer otherwise.
 * ------------------------------------------------------------------------------------------- */
typedef struct xmh_dimch_head {
    const float* conv_w; /* [M, T, 3] */
    const float* conv_b; /* [M] */
    const float* w1;     /* [H, E] */
    const float* b1;     /* [H] */
    const float* w2;     /* [K, H] */
    const float* b2;     /* [K] */
    int T, E, H, M, K;
    int hash_func;       /* XMH_DIMCH_TANH or XMH_DIMCH_SOFTMAX */
} xmh_dimch_head;
typedef struct xmh_dimch_head_grads { /* each may be NULL: that gradient is not formed */
    float *d_conv_w, *d_conv_b, *d_w1, *d_b1, *d_w2, *d_b2; /* written, or added to when accumulate != 0 */
    float* d_tokens;                                        /* [B, T, E], always written */
} xmh_dimch_head_grads;
size_t xmh_head_dimch_bytes(int64_t B, int T, int E, int H, int M, int K, size_t* workspace_bytes);
int xmh_head_dimch(const xmh_dimch_head* h, const float* tokens, int64_t B, float* embeds, float* hash, void* workspace,
                   size_t workspace_bytes, xmh_stream_t stream);
/* keep == NULL: no dropout (p is ignored) */
int xmh_head_dimch_train_forward(const xmh_dimch_head* h, const float* tokens, const uint8_t* keep, float p, int64_t B, float* embeds,
                                 float* hash, void* saved, size_t saved_bytes, xmh_stream_t stream);
/* d_embeds [B, M, K] and d_hash [B, K] enter through the two outputs; either may be NULL.  has_keep: the forward had a keep mask. */
int xmh_head_dimch_backward(const xmh_dimch_head* h, const float* tokens, int has_keep, float p, const float* d_embeds,
                            const float* d_hash, int64_t B, const void* saved, size_t saved_bytes, const xmh_dimch_head_grads* g,
                            int accumulate, void* workspace, size_t workspace_bytes, xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * UMoED soft-MoE decoder head, one modality, eval mode (reference models/UMoED/hash/hash_moe.py, hash/block/transformer.py,
 * hash/block/SoftMoe.py, models/common/hash.py; csrc/xmh_umoed.hip).  d = width, M = setDim learned query rows, S = n_experts * slots:
 *   mem = tokens [B, T, E], or relu(tokens first_w^T + first_b) [B, T, d] when first_w is given;  x = queries [M, d] repeated over B
 *   per layer (post-norm):  x = LN1(x + out_proj(MHA(q = k = v = x)));  x = LN2(x + out_proj(MHA(q = x, k = v = mem)))  (no mask)
 *     h = relu(x lin_w^T + lin_b) [B, M, F]
 *     moe != 0:  logits = h phi [B, M, S];  D = softmax(logits) over the M rows, Cw = softmax(logits) over the S slots;
 *                Xs = D^T h [B, S, F];  Ys[b, n, p] = Xs[b, n, p] W_n + bias_n;  x = LN3(x + Cw Ys)
 *     moe == 0:  x = LN3(x + h lin2_w^T + lin2_b)
 *   embeds = x cls_w^T + cls_b [B, M, V]
 *   code: XMH_UMOED_LINEAR_SUBSPACE (merge XMH_UMOED_CONCATENATE): per row the argmax of the V logits (first index on a tie) written
 *         as log2 V bits, most significant first, 1 -> +1 and 0 -> -1: code [B, M log2 V];
 *         XMH_UMOED_TANH / XMH_UMOED_SOFTMAX (merge XMH_UMOED_MEAN): tanh, or the softmax over the pairs (2j, 2j + 1), of the mean of
 *         embeds over M: code [B, V].
 * All weights are plain fp32 device pointers in the reference's layouts; `layers` is a host array.  Every product is exact fp32
 * (v_mfma_f32_32x32x2_f32 or fmaf chains) in one fixed summation order: two calls agree to the bit.  No allocation, no host
 * synchronisation, no float atomics.  16 launches per MoE layer, 12 per plain layer, 2 (3 with a first layer) around them.
 * Bounds (XMH_ENOTSUP beyond): d / heads == 64; M, T <= 128; E <= 2048; d <= 1024 (the width xmh_layernorm_f32 takes); F <= 4096; S <= 256; V <= 256, a power of two for linear_subspace; B max(M, T) <= 32768, B <= 65535.
 * Workspace: xmh_head_umoed_bytes(B, T, h) bytes of device memory, 256-byte aligned (0 outside the bounds; XMH_ENOMEM when shorter).
 * Argument errors are reported before any launch.
 * ------------------------------------------------------------------------------------------- */
#define XMH_UMOED_LINEAR_SUBSPACE 0
#define XMH_UMOED_TANH 1
#define XMH_UMOED_SOFTMAX 2
#define XMH_UMOED_CONCATENATE 0
#define XMH_UMOED_MEAN 1
typedef struct xmh_umoed_layer {
    const float *ln1_g, *ln1_b, *sa_in_w /* [3d, d] */, *sa_in_b, *sa_out_w /* [d, d] */, *sa_out_b;
    const float *ln2_g, *ln2_b, *ca_in_w /* [3d, d] */, *ca_in_b, *ca_out_w /* [d, d] */, *ca_out_b;
    const float *ln3_g, *ln3_b, *lin_w /* [F, d] */, *lin_b;
    const float *phi /* [F, n, p] */, *exp_w /* [n, F, d] */, *exp_b /* [n, d] */; /* moe != 0 */
    const float *lin2_w /* [d, F] */, *lin2_b;                                      /* moe == 0 */
} xmh_umoed_layer;
typedef struct xmh_umoed_head {
    const xmh_umoed_layer* layers; /* host array [n_layers] */
    int n_layers;
    const float *first_w /* [d, E] */, *first_b; /* NULL when d == E */
    const float *queries /* [M, d] */, *cls_w /* [V, d] */, *cls_b;
    int E, d, heads, F, M, V, n_experts, slots, moe, hash_func, merge;
    float ln_eps;
} xmh_umoed_head;
size_t xmh_head_umoed_bytes(int64_t B, int T, const xmh_umoed_head* h);
int xmh_head_umoed(const xmh_umoed_head* h, const float* tokens, int64_t B, int T, float* embeds, float* code, void* ws, size_t ws_bytes,
                   xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * UMoED decoder head in train mode and its backward (reference hash/block/transformer.py SoftMoEDecoderLayer with its dropouts;
 * csrc/xmh_umoed_grad.hip).  One dropout probability p at six sites per layer, every kept entry scaled by 1 / (1 - p):
 *   u1 = x  + drop2(out_proj(drop1(softmax(q k^T / 8)) v))   q, k, v from x                 x1 = LN1(u1)
 *   u2 = x1 + drop4(out_proj(drop3(softmax(q k^T / 8)) v))   q from x1, k | v from tokens   x2 = LN2(u2)
 *   h  = drop5(relu(linear(x2)));  the Soft-MoE of h as in inference -> Y;  u3 = x2 + drop6(Y);  x = LN3(u3)
 * drop1 and drop3 act on the attention probabilities after the softmax and before P V.  No mask on the keys.
 * The library draws no random numbers: `keep` is the caller's buffer of 0 / 1 bytes, xmh_umoed_keep_bytes(B, T, h) long; per layer, in
 * this order, [B, heads, M, M] (drop1), [B M, d] (drop2), [B, heads, M, T] (drop3), [B M, d] (drop4), [B M, F] (drop5), [B M, d] (drop6),
 * and the layers follow one another.  keep == NULL: no dropout (p is ignored), and embeds and code equal xmh_head_umoed's to the bit
 * (the same launches in the same order).
 * xmh_head_umoed_train_bytes -> the bytes of the record `saved` that the forward fills and the backward reads, and through
 * workspace_bytes (may be NULL) the bytes of the workspace either call needs; both 0 outside the bounds.  Both buffers 256-byte aligned
 * (XMH_ENOMEM when shorter).  The record keeps every layer's intermediate rows but not the attention probabilities, which the backward
 * recomputes from q and k.
 * xmh_head_umoed_backward: d_embeds [B, M, V] is the upstream of embeds (the code carries no gradient).  grads: one
 * xmh_umoed_layer_grads per layer (host array, or NULL for none), d_queries [M, d], d_cls_w [V, d], d_cls_b [V], d_tokens [B, T, E].
 * Every pointer may be NULL: that gradient is not formed, and nothing is written there.  Parameter gradients are written, or added to
 * when accumulate != 0; d_tokens is always written.  ca_in_w's gradient: rows 0 : d from the queries' side, rows d : 3 d from the tokens'.
 * Scope (XMH_ENOTSUP otherwise, the text names the cause): moe != 0 (the plain decoder has no train mode); first_w == NULL (nor has a
 * first layer); ln_eps == 1e-5 (what the LayerNorm backward assumes); and the bounds of xmh_head_umoed: d / heads == 64; M, T <= 128
 * (a thread per attention row); d <= 1024; F <= 4096; S <= 256; V <= 256; B max(M, T) <= 32768, B <= 65535.  p in [0, 1) with a mask.
 * Exact fp32, no allocation, no host synchronisation, no float atomics, one fixed order per sum: two calls agree to the bit.  Argument and
 * bound errors are reported before any launch.
 * ------------------------------------------------------------------------------------------- */
typedef struct xmh_umoed_layer_grads {
    float *ln1_g, *ln1_b, *sa_in_w, *sa_in_b, *sa_out_w, *sa_out_b;
    float *ln2_g, *ln2_b, *ca_in_w, *ca_in_b, *ca_out_w, *ca_out_b;
    float *ln3_g, *ln3_b, *lin_w, *lin_b, *phi, *exp_w, *exp_b;
} xmh_umoed_layer_grads;
typedef struct xmh_umoed_head_grads {
    const xmh_umoed_layer_grads* layers; /* host array [n_layers], or NULL */
    float *d_queries, *d_cls_w, *d_cls_b, *d_tokens;
} xmh_umoed_head_grads;
size_t xmh_head_umoed_train_bytes(int64_t B, int T, const xmh_umoed_head* h, size_t* workspace_bytes);
size_t xmh_umoed_keep_bytes(int64_t B, int T, const xmh_umoed_head* h);
int xmh_head_umoed_train_forward(const xmh_umoed_head* h, const float* tokens, const uint8_t* keep, float p, int64_t B, int T, float* embeds,
                                 float* code, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, xmh_stream_t stream);
int xmh_head_umoed_backward(const xmh_umoed_head* h, const float* tokens, const uint8_t* keep, float p, const float* d_embeds, int64_t B, int T,
                            const void* saved, size_t saved_bytes, const xmh_umoed_head_grads* grads, int accumulate, void* ws, size_t ws_bytes,
                            xmh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * UMoED: the objective of the pairwise / cosine / triplet family (reference models/UMoED/UMoED.py similarity_loss with
 * distance/__init__.py pairwise_distance) and its gradient.  e_img, e_txt [B, M, V] fp32, lab: xmh_pack_labels of the [B, C] labels.
 *   x, y = F.normalize (eps 1e-12) of the rows;  a, b = softmax(x / extreme_T), softmax(y / extreme_T) when extreme, else x, y
 *   D[i][k] = mean_t (1 - max(a[i, t] . b[k, t], 0)): token t of one set meets token t of the other.  D_i2t = D, D_t2i = D^T.
 *   T(D, m) the weighted triplet term defined above xmh_dimch_loss (one implementation, csrc/xmh_triplet.h), m = token_triplet_margin
 *   U(u) = mean_b sum_{t < t'} exp(-20 |u[b, t] - u[b, t']|^2) / (M (M - 1) / 2), per set, on the normalised rows; 0 for M = 1.
 *          Squared distances are sums of squared differences at every distance: identical rows give exactly 0.
 *   loss = triplet_alpha (T_i2t + T_t2i) / 4 + unif_alpha (U(x) + U(y)) / 3
 * B <= 512, M <= 128, V <= 256, C <= 127 -- XMH_ENOTSUP outside.  No host synchronisation, no allocation, no float atomics, every sum
 * in one fixed order (two calls agree to the bit); a row without a label makes the triplet terms NaN, as in the reference.
 * Workspace: xmh_umoed_loss_ws_bytes(B, M, V, C), 256-byte aligned (0 outside the bounds; XMH_ENOMEM when shorter).
 * xmh_umoed_loss: 4 launches.  xmh_umoed_loss_grad: 5 launches (it stands alone).
 * ------------------------------------------------------------------------------------------- */
typedef struct xmh_umoed_consts {
    int extreme;
    float extreme_T, token_triplet_margin, triplet_alpha, unif_alpha;
} xmh_umoed_consts;
size_t xmh_umoed_loss_ws_bytes(int64_t B, int M, int V, int C);
/* out8 (device doubles): loss, T_i2t, T_t2i, U(x), U(y), 0, 0, 0.  cst is read on the host. */
int xmh_umoed_loss(const float* e_img, const float* e_txt, int64_t B, int M, int V, int C, const uint32_t* lab, const xmh_umoed_consts* cst,
                   void* ws, size_t ws_bytes, double* out8, xmh_stream_t stream);
/* d loss times upstream[0] (a device float; NULL = 1) -> g_img, g_txt [B, M, V]: written, or added to when accumulate != 0.  Either may
 * be NULL: that gradient is not formed.  The backward of the softmax, of the normalisation and of the clamp is included. */
int xmh_umoed_loss_grad(const float* e_img, const float* e_txt, int64_t B, int M, int V, int C, const uint32_t* lab,
                        const xmh_umoed_consts* cst, const float* upstream, float* g_img, float* g_txt, int accumulate, void* ws,
                        size_t ws_bytes, xmh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* XMH_H */
