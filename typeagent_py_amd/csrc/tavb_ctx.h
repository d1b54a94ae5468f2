// What the host files of libtavb.so share -- tavb_abi.hip (context, options, corpus, load path), tavb_lookup.hip (the fused-k lookups and the
// staging), tavb_lookup_topk.hip (the large-k and sorted lookups), tavb_lookup_masked.hip (the batched resident subset, the masked and
// scoped batches), tavb_row_edits.hip (row compaction, expansion and scattered writes), tavb_mask_entry.hip (the row masks and the scope
// algebra), tavb_lookup_rows.hip (rows of the corpus as queries), tavb_lookup_pairs.hip (the near-duplicate self-join), tavb_route.hip (the routing of a device-resident batch) and tavb_comm.hip (RCCL): error reporting, the workspaces, the
// context itself and the internal functions that cross files.  Private to csrc/; host code only.  Everything here but `struct tavb_ctx` (the C ABI's opaque handle) and
// tavb_search_device_dispatch lives in tavb::host, whose symbols stay inside the library.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "tavb_internal.h"

typedef unsigned long long u64_t;

namespace tavb {
namespace host __attribute__((visibility("hidden"))) {

extern thread_local std::string g_last_error;  // what tavb_last_error returns (tavb_abi.hip)
int fail(int code, const char* fmt, ...);      // sets it, returns `code`

#define TAVB_HIP(expr)                                                                                     \
  do {                                                                                                     \
    hipError_t e__ = (expr);                                                                               \
    if (e__ != hipSuccess)                                                                                 \
      return ::tavb::host::fail(TAVB_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// bumped by every (re)allocation or release of a workspace: captured HIP graphs hold raw pointers into these buffers
extern std::atomic<unsigned long long> g_alloc_epoch;  // (contexts on several threads share it; tavb_abi.hip)

struct Buffer {
  void* ptr = nullptr;
  size_t cap = 0;
  bool pinned_host = false;
  int reserve(size_t bytes) {
    if (bytes <= cap) return TAVB_OK;
    size_t want = std::max(bytes, cap * 2);
    want = (want + 255) & ~(size_t)255;
    ++g_alloc_epoch;
    if (ptr) {
      hipError_t e = pinned_host ? hipHostFree(ptr) : hipFree(ptr);
      ptr = nullptr;
      cap = 0;
      if (e != hipSuccess) return fail(TAVB_E_HIP, "free of workspace failed: %s", hipGetErrorString(e));
    }
    hipError_t e = pinned_host ? hipHostMalloc(&ptr, want, hipHostMallocDefault) : hipMalloc(&ptr, want);
    if (e != hipSuccess) {
      ptr = nullptr;
      return fail(TAVB_E_NOMEM, "workspace allocation of %zu bytes failed: %s", want, hipGetErrorString(e));
    }
    cap = want;
    return TAVB_OK;
  }
  void release() {
    if (ptr) ++g_alloc_epoch;
    if (ptr) (void)(pinned_host ? hipHostFree(ptr) : hipFree(ptr));
    ptr = nullptr;
    cap = 0;
  }
};

// the defaults of skinny_min_batch_f32 / skinny_min_batch_f16 (the measured break-even of the 32/64-query tile against the streaming tiers);
// tavb_plan_masked, which has no context, uses them as they ship
constexpr int64_t kSkinnyMinBatchF32 = 5, kSkinnyMinBatchF16 = 3;
// the default of mfma_min_batch (the unmasked dispatcher's own bound for the 128/256-query tile on fp16 corpora) and the compute units the
// planning functions that have no context assume (MI355X); tavb_plan_masked_wide uses both as they ship
constexpr int64_t kMfmaMinBatch = 65;
// fewest queries tavb_plan_top_messages_tile sends to the 32/64-query tile (option "top_messages_tile_min_batch"): the smallest batch
// measured -- at 8 queries over 1M x 1536 rows no cell loses, threshold 0 (every pair an atomic) included: 1.08 .. 3.2 x
// (profiles/r27_top_messages_tile.md); smaller batches were not measured
constexpr int64_t kTopMessagesTileMinBatch = 8;
// fewest rows tavb_plan_pairs_join sends to the self-join (option "pairs_join_min_rows"): PROVISIONAL, not measured -- tools/pairs_join_sweep.py
// finds the smallest swept row count at which the join beats the row lookups; tests/test_gpu_lookup_rows.py needs it above 2000
constexpr int64_t kPairsJoinMinRows = 8192;
constexpr int kPlanComputeUnits = 256;

struct PendingTiming {
  int kernel;
  hipEvent_t start, stop;
};

}  // namespace host
}  // namespace tavb

struct tavb_ctx {
  using Buffer = tavb::host::Buffer;
  using PendingTiming = tavb::host::PendingTiming;

  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int n_cu = 256;

  const void* corpus = nullptr;
  int64_t rows = 0;
  int32_t dim = 0;
  int32_t dtype = TAVB_F32;
  int64_t ordinal_base = 0;

  tavb::ScanGeometry geom{0, 16, 2, 1, 0, 0};
  int64_t mfma_min_batch = tavb::host::kMfmaMinBatch;  // batches from this size up use the 128/256-query tile + rescoring (smaller ones the 32/64-query tile) ...
  // ... and on corpora of `mfma_big_bytes` (256 MiB) or more already from `mfma_min_batch_big` = 33 queries (round 5): padded to 128 queries the wide
  // tile serves 33 / 48 / 64 queries over 10M fp16 rows in 5.42 / 5.48 / 5.46 ms against 5.54 / 5.81 / 5.91 ms on the 64-query split-plane tile,
  // and 64 queries over 1M fp32 rows (through the fp16 shadow) in 0.85 ms against 2.17 ms (profiles/r05_raw/b64.txt).  On small corpora its ~40
  // launches per batch cost more than the 64-query tile's pass.
  int64_t mfma_min_batch_big = 33;
  int64_t mfma_big_bytes = (int64_t)256 << 20;
  // ... and on FP32 corpora of `mfma_big_bytes_f32` (2 GiB) or more from `mfma_min_batch_big_f32` = 5 queries (round 6): the wide tile streams the fp16
  // shadow -- half the bytes of the fp32 rows the 32-query fp32 tile reads -- and its candidates are rescored with the fp32 rows: 5 / 8 / 16 / 32
  // queries over 1M x 1536 fp32 rows in 0.76 / 0.77 / 0.78 / 0.79 ms against 1.14 / 1.16 / 1.21 / 1.24 ms (profiles/r06_raw/f32_mid.txt); 32 queries
  // over 700k / 400k / 200k / 100k rows: 0.64 / 0.48 / 0.36 / 0.53 ms against 0.95 / 0.61 / 0.40 / 0.22 (f32_few.txt: the wide path's ~0.35 ms of
  // selection and rescoring launches against half a pass).  Batches of 2 .. 4 queries (one pass of the fp32 streaming scan) from TWICE that size:
  // 1M rows 0.77 against 0.92 .. 0.97 ms, 700k rows 0.64 against 0.68, 400k rows 0.48 against 0.39.  Single queries keep the fp32 scan (option
  // f32_shadow = 2 moves them too).  Needs the shadow (f32_shadow >= 1: +50 % device memory, built on first use); without the memory for it the fp32
  // kernels serve the batch.
  // End of round 6 (tools/regime_sweep.py, profiles/r06_raw/regime_sweep_before.md, after the wide path's launch diet): 5+ queries from 1e9 bytes
  // (165k x 1536 rows: 0.26 ms through the shadow against 0.27 .. 0.33 on the fp32 tile, whose workgroups start compacting with their second
  // tile; at 120k rows the fp32 tile still wins, 0.17 .. 0.21 against 0.24), 2 .. 4 queries from 4 GiB as before (500k rows: 0.45 either way),
  // and 33+ queries at ANY size (`mfma_min_batch_f32`): one tile of the 64-query fp32 kernel is 82 us of fp32 matrix work however small the
  // corpus -- 64 queries over 1000 / 5000 / 20000 fp32 rows 0.189 / 0.202 / 0.204 ms against 0.087 / 0.112 / 0.140 for 65 queries on the wide tile.
  int64_t mfma_min_batch_big_f32 = 5;
  int64_t mfma_big_bytes_f32 = 1000000000;
  int64_t mfma_few_bytes_f32 = (int64_t)4 << 30;
  int64_t mfma_min_batch_f32 = 33;
  int64_t mfma_splits = 0;  // 0 = auto
  int64_t mfma_ablate = 0;
  int64_t mfma_sched = 0;
  int64_t mfma_tile = 0;  // 0 = auto (128 queries per tile up to 128 queries, else 256)
  int64_t mfma_sample_rows = 0;  // rows of the first (threshold-seeding) phase: 0 = auto (two tiles per workgroup), -1 = one phase, no seeding
  int64_t skinny_min_batch_f32 = tavb::host::kSkinnyMinBatchF32;   // fp32 corpus: batches from this size up use the 32-query MFMA tile
  int64_t skinny_min_batch_f16 = tavb::host::kSkinnyMinBatchF16;   // fp16 corpus: batches from this size up to mfma_min_batch - 1 use it
  int64_t mfma_ladder = 4;            // each further phase scans this many times the rows scanned so far (0 = seed once)

  Buffer d_queries, d_queries_f16, d_lists, d_out, d_rows, d_cand, d_thr, d_sample_keys;
  Buffer d_counts;  // 256-query tile: keys left per candidate buffer
  Buffer d_delta, d_approx, d_flag, d_fb_queries, d_norm;  // exact rescoring of the 256-query tile (tavb_rescore.hip)
  Buffer d_minscores;      // per-query thresholds of a batch on the device: [nq_pad] min_scores, then [nq_pad] exclusive admission floors (the tile paths)
  Buffer d_fb_cand;        // what the 64-query exact tile ranked highest for the flagged queries: [slots][64] keys, rescored into the callers' rows
  Buffer d_shadow;         // fp32 corpora (and fp16 ones whose width is not a multiple of 64): fp16 copy of rows [0, norm_rows), each padded with zeros to a
                           // multiple of 64 halves -- the filter operand of the 128/256-query tile
  Buffer d_queries_pad;    // the queries of a batch zero-padded to that width (odd widths only)
  int64_t f32_shadow = 1;  // option: 1 = batches of mfma_min_batch+ queries on fp32 corpora go through that shadow (+50 % HBM); 2 = every lookup on
                           // fp32 corpora of f32_shadow_min_bytes and more (half the bytes per pass); 0 = never
  int64_t f32_shadow_min_bytes = (int64_t)2 << 30;  // level 2 only: fp32 corpora from this size up (below it the extra launches cost more than half a pass saves)
  int last_shadow = 0;     // the last lookup's filter pass read the shadow
  Buffer d_accept, d_bits;  // message re-rank: accepted message ordinals, their bitmap
  Buffer d_emit;            // survivors of tavb_search_all: a counter, then the keys
  // large-k lookups (tavb_search_topk, tavb_topk.hip): the dense score array of a group of queries and the workspace of the selection
  Buffer d_topk_scores, d_topk;
  int64_t large_k = 1;                       // option: 1 = the binding routes TAVB_MAX_FUSED_K < k <= TAVB_MAX_LARGE_K through tavb_search_topk
  int64_t topk_buckets = 1024;               // option: histogram buckets of the score pass
  int64_t topk_boundary_keys = 16384;        // option: capacity of a query's boundary list (more keys in the boundary bucket: refinement)
  int64_t topk_scores_bytes = (int64_t)1 << 30;  // option: most bytes of one group's score array (queries per corpus pass are cut to fit)
  // top-messages lookups (tavb_search_top_messages): per query of a group and message, the best passing score of the message's rows
  // ([queries of a group][n_messages] x 4 bytes: what d_topk_scores is to rows; the selection's workspace is d_topk as well)
  Buffer d_msg_best;
  int64_t top_messages = 1;                  // option: 1 = the binding sends lookup_top_messages_* through tavb_search_top_messages, 0 = through the all-survivor lookup and a collapse on the host
  int64_t top_messages_scoped = 1;           // option: 1 = the binding sends lookup_top_messages_by_embeddings_scoped through tavb_search_top_messages_scoped (while "top_messages" is on), 0 = it loops over the one-mask call
  int64_t top_messages_tile = 0;             // option: lookup_top_messages_* on the 32/64-query tile (tavb_search_top_messages_tile): 0 = never (the default: scores stay the row scan's bit for bit), 1 = follow tavb_plan_top_messages_tile, 2 = always where supported
  int64_t top_messages_tile_min_batch = tavb::host::kTopMessagesTileMinBatch;  // option: fewest queries tavb_plan_top_messages_tile sends to the tile
  int64_t last_topk_refine = 0;              // option "last_topk_refine" (get): refinement rounds the last large-k lookup needed (most of any query)
  // the asynchronous forms (tavb_search_topk_device, tavb_search_topk_allgather): the finish kernel writes every query's rounds here, and
  // the next tavb_synchronize folds the first topk_rounds_pending of them into last_topk_refine
  Buffer h_topk_rounds{nullptr, 0, true};
  int topk_rounds_pending = 0;
  // sorted lookups (tavb_search_sorted: every survivor, or any k): the keys of one query at or above its boundary, then their sort
  // (tavb_sort.hip); the decoded results leave through h_out in pieces of at most sort_stage_keys
  Buffer d_sort_keys, d_sort_ws;
  Buffer d_mask_counts;  // row masks (tavb_mask_expand, tavb_mask.hip): set rows per workgroup chunk of the mask
  Buffer d_compact;      // row compaction in place (tavb_compact_rows): the kept rows of one pass, densely, before they are written back further down
  int64_t compact_pass_rows = 0;  // option: rows per pass of an in-place compaction, rounded up to a multiple of 64 (0 = auto: about 64 MiB of rows)
  // rows of the corpus as queries (tavb_search_rows, tavb_lookup_rows.hip): the positions of a call, the float32 query batch of one wave of at
  // most rows_query_wave rows, that wave's lists of k + 1 keys, and the lists of k keys of the whole call before they are copied out
  Buffer d_rows_pos, d_rows_query, d_rows_keys, d_rows_out;
  int64_t rows_query = 1;            // option: 1 = the binding sends fuzzy_lookup_rows / near_duplicate_pairs through tavb_search_rows, 0 = through the host route (rows to the host, a query batch back)
  int64_t rows_query_wave = 4096;    // option: most rows one wave of tavb_search_rows gathers and looks up (its batch is wave x dim x 4 bytes)
  int64_t last_rows_query = 0;       // option "rows_query_launches" (get): gather launches of the last rows lookup; 0 after any other host-synchronous lookup of the unmasked routes
  // near-duplicate self-join (tavb_join_pairs, tavb_lookup_pairs.hip): two 64-bit counters (candidates, pairs kept), the candidate pairs and the
  // kept (i, j, score) of one call, each sized by the call's capacity
  Buffer d_pairs;
  int64_t pairs_join = 1;                          // option: 1 = the binding sends similarity_join / near_duplicate_pairs through tavb_join_pairs where tavb_plan_pairs_join says so, 0 = through the row lookups
  int64_t pairs_join_min_rows = tavb::host::kPairsJoinMinRows;  // option: fewest rows tavb_plan_pairs_join sends to the join
  int64_t pairs_join_capacity = (int64_t)1 << 22;  // option: candidate pairs a call reserves by default (20 bytes each)
  int64_t pairs_join_max_capacity = (int64_t)1 << 25;  // option: the most one retry of the binding may ask for
  int64_t last_pairs_join = 0;                     // option "pairs_join_launches" (get): join launches of the last tavb_join_pairs call; 0 after a refused one and after any row lookup
  int64_t pairs_join_candidates = 0;               // option (get): candidate pairs the last join launch counted
  Buffer d_scope;        // scope algebra (tavb_mask_from_ranges): the merged {start, end} intervals of a scope's collections, one after another
  // scoped batches (tavb_search_scoped_batch): per pass the union of its queries' masks, that union's ascending row list and one membership
  // byte per list position (tavb_mask.hip scope_member_kernel); pinned: every pass' total, then its chunks' MaskChunkInfo
  Buffer d_scope_bits, d_scope_rows, d_scope_member;
  Buffer h_scope{nullptr, 0, true};
  // scoped batches on the 32/64-query tile (tavb_search_scoped_tile) and on the 128/256-query filter tile (tavb_search_scoped_wide): the membership planes of one wave of query tiles -- per block of 32
  // queries one uint32 per row of the span (tavb_mask.hip scope_planes_kernel)
  Buffer d_scope_planes;
  int64_t scope_tile = 1;  // option: scoped batches on the 32/64-query tile: 1 = follow tavb_plan_scoped (with "mask_tile_min_bytes" / "mask_tile_pct"), 0 = never, 2 = always where supported
  int64_t scope_wide = 1;  // option: scoped batches on the 128/256-query filter tile (tavb_search_scoped_wide): 1 = follow tavb_plan_scoped_wide (same thresholds), 0 = never, 2 = always where supported
  int64_t scope_large_k = 1;  // option: 1 = the binding sends scoped batches at max_hits 0 and beyond TAVB_MAX_FUSED_K through tavb_search_scoped_topk / tavb_search_scoped_sorted, 0 = it loops per query
  int64_t scope_wave_bytes = (int64_t)64 << 20;  // option: most bytes of membership planes one wave of tavb_search_scoped_wide builds (at least one query tile's are built whatever this says)
  Buffer h_sort_info{nullptr, 0, true};  // pinned: meta [nq][4] + per-block key counts [nq][blocks] of one group
  int64_t sort_all = 1;                   // option: 1 = the binding routes max_hits == 0 and max_hits > TAVB_MAX_LARGE_K through tavb_search_sorted
  int64_t sort_stage_keys = (int64_t)1 << 21;  // option: most results decoded into pinned memory before they are copied to the caller (12 B each)
  int64_t sort_small_keys = 16384;        // option: sorts of up to this many keys run in one workgroup (0 .. tavb::kSortSmallMax); faster than
                                          // the multi-pass sort at every size up to the LDS limit (16384: 0.145 against 0.192 ms, profiles/r08_sort_all.md)
  // load path (tavb_upload_rows): two pinned staging slots + two device scratch slots, recycled through events
  Buffer h_ring[2] = {{nullptr, 0, true}, {nullptr, 0, true}};
  Buffer d_ring[2];
  hipEvent_t ring_done[2] = {nullptr, nullptr};
  const int32_t* row_to_msg = nullptr;  // borrowed device map chunk row -> message ordinal
  int64_t row_to_msg_rows = 0, n_messages = 0;
  int64_t norm_rows = 0;  // rows of the corpus covered by the cached row-norm maxima (d_norm) -- and, for fp32 corpora, by the fp16 shadow
  Buffer h_stage{nullptr, 0, true};
  Buffer h_out{nullptr, 0, true};  // pinned + device-visible: the last kernel of a synchronous lookup writes its keys straight here
  Buffer h_lists{nullptr, 0, true};  // pinned + device-visible: per-workgroup lists of a small single-query lookup (merged on the host)
  Buffer h_flag{nullptr, 0, true};   // pinned: the work list of flagged queries read back by the one route that needs a host round trip (fp32 corpus, k > 64)
  int64_t mfma_shape = 16;      // option: MFMA of the 256-query filter tile, 16 = v_mfma_f32_16x16x32_f16, 32 = v_mfma_f32_32x32x16_f16 (profiles/r09_mfma_shape.md)
  int64_t last_mfma_shape = 0;  // option "last_mfma_shape" (get): the MFMA shape the last filter launch of the 128/256-query tile ran on (0: none yet)
  // masked batches (tavb_search_masked_batch / _device): the binding's choice between the gather route (tavb_search_subset_batch_resident over the
  // expanded row list) and the 32/64-query tile with the bit test in its admission path; the rule is tavb_plan_masked
  int64_t mask_tile = 1;                            // option: 1 = follow tavb_plan_masked, 0 = never the tile, 2 = always where supported
  int64_t mask_tile_min_bytes = (int64_t)128 << 20;  // option: allowed rows x row bytes below which the gather route (one launch there) is kept; the default of small_direct_bytes
  int64_t mask_tile_pct = 100;                      // option: the tile when the gather route's bytes are at least this many % of the tile's (100 = byte parity)
  int64_t masked_route = 0;                         // option "masked_route" (get): 0 before the first masked lookup, 1 = gather, 2 = tile, 3 = the wide filter tile + rescoring, 4 = a scoped batch (one mask per query), 5 = a scoped batch on the 32/64-query tile, 6 = a scoped batch on the 128/256-query filter tile + rescoring, 7 / 8 = a scoped batch on the large-k / sorted route, 9 = a scoped top-messages batch, 10 = a top-messages batch on the 32/64-query tile
  int64_t mask_wide = 1;                            // option: masked batches on the 128/256-query filter tile (tavb_search_masked_wide): 1 = follow tavb_plan_masked_wide, 0 = never, 2 = always where supported
  int64_t last_skinny_kernel = 0;  // option "last_skinny_kernel" (get): what the last launch of the 32/64-query tile instantiated, tavb::skinny_kernel_id (0: none yet)
  int64_t mfma_bdirect = 0;  // option (measurement for now): the 256-query tile takes its query operand straight from L2 (fragment-major layout), not through LDS
  int64_t band_max = tavb::kBandMax;  // option: keys of a query's band the wide tile's selection hands to the rescoring (256 .. kBandMax); a band that does not fit flags the query
  int64_t early_exact = 1;    // option: ... and a batch found to be mostly such queries BEFORE the last filter phase skips that phase (needs wide_fallback)
  int64_t wide_fallback = 1;  // option: batches of 256+ queries re-run MANY (> 64) flagged queries on the 256-query tile's exact (split-plane) form
  int64_t small_direct_bytes = (int64_t)128 << 20;  // option: single-query lookups on corpora up to this size take the one-launch path (0 = never)
  int64_t small_direct_keys = 8192;                 // option: most keys the per-workgroup lists of such a lookup may hold (the grid is cut to fit; x 2 for a batch of 2 .. 8 queries)
  int64_t last_direct = 0;                          // option "last_direct" (get): 1 when the last lookup took it, 2 = with the query inside the kernel arguments
  int64_t inline_query = 1;                         // option: 1536-wide single queries of that path ride in the kernel arguments (no H2D copy before the launch)
  // the GROUPED form of that path (ScanParams::group): batches of 2 .. direct_group_max_nq queries in one launch of gridDim.y query groups
  int64_t direct_group_max_nq = TAVB_MAX_GROUPED_QUERIES;  // option: biggest batch that may take it (0 / 1 = never: batches of up to 8 keep the plain form, bigger ones the tiles)
  int64_t direct_group = 0;                         // option: queries per group, 1 / 2 / 4 / 8, taken whatever the cost model says (0 = plan_direct_group)
  int64_t direct_group_wgs = 0;                     // option: most workgroups of such a launch (row workgroups x groups); 0 = plan_direct_group (256 or 512)
  bool staged_overflow = false;                     // set by stage_queries_host: a staged query holds an element whose fp16 rounding is not finite (staged_overflow())
  bool dispatch_no_group = false;                   // set by tavb_search_batch around its fall-through: the host-synchronous cost model already said no
  int64_t direct_group_keys = 32768;                // option: most keys the lists of such a launch may hold (nq x workgroups-per-group x k; 256 KiB over PCIe)

  bool profiling = false;
  double total_ms[TAVB_KERNEL_COUNT] = {0};
  int64_t launches[TAVB_KERNEL_COUNT] = {0};
  std::vector<PendingTiming> pending;
  std::vector<hipEvent_t> free_events;

  int last_tier = 0;
  int pending_nq = 0, pending_k = 0;  // shape of the lookup enqueued by tavb_search_begin

  // small corpora (the reference's own scale: 10k x 1536, 41 us per call as three submissions): the H2D copy of the query, the scan and the merge
  // of a single-query lookup replayed as ONE captured HIP graph.  A few (corpus, k, min_score) shapes are kept.  OFF by default: measured on
  // MI355X / ROCm 7.2 (profiles/r03_latency_cfg1.md) the replay takes 48.3 us against 41.3 us for the three plain submissions -- hipGraphLaunch
  // costs more than it saves for a 3-node graph; the GPU-side floor of the lookup is the two kernels (scan 14.8 us + merge 11.8 us).
  struct SmallGraph {
    const void* corpus = nullptr;
    int64_t rows = 0;
    int32_t dim = 0, dtype = 0, k = 0;
    uint32_t thr_bits = 0;
    unsigned long long epoch = 0, geom_tag = 0;
    hipGraphExec_t exec = nullptr;
    int seen = 0;  // calls with this shape so far (the first one runs un-captured: it sizes the workspaces)
    unsigned long long last_used = 0;
  };
  SmallGraph graphs[4];
  unsigned long long graph_clock = 0;
  int64_t graph_max_bytes = 0;  // option "graph_max_bytes": single-query lookups on corpora up to this size replay a graph (0 = never, the default)
  int64_t last_graph = 0;                          // option "last_graph" (get): 1 when the last lookup was a graph replay

  // row-sharded corpora: this context's RCCL communicator (tavb_comm_init) and the buffers of the exchange
  void* comm = nullptr;  // an ncclComm_t: only tavb_comm.hip includes RCCL's header
  int comm_rank = 0, comm_world = 1;
  int64_t comm_force = 0;  // option: run the all-gather + merge even in a world of one (tests, dry runs of the N > 1 path)
  int64_t comm_fail_rank = -1;  // option (fault injection): the local search of tavb_search_allgather "fails" on this rank of the communicator
  int64_t comm_fail_alloc = 0;  // option (fault injection): the per-call allocations of tavb_search_allgather "fail" (lists beyond comm_reserve_keys)
  int64_t comm_stall_ms = 0;    // option (fault injection): the next exchange is held up on the stream for this long, as by a peer that is late
  int64_t comm_timeout_ms = 0;  // option: tavb_synchronize gives an exchange in flight this long before it aborts the communicator (0 = wait for ever)
  // keys of the exchange buffers reserved by tavb_comm_init (d_xlocal: that many, d_gather: x world): an exchange of up to that many keys per
  // rank allocates NOTHING between entering the call and ncclAllGather; a bigger one goes through the same buffers in chunks of whole queries
  int64_t comm_reserve_keys = (int64_t)1 << 20;
  int64_t comm_chunk_keys = 0;  // comm_reserve_keys as tavb_comm_init found it: what the chunks of a big exchange are cut by (not Buffer::cap, which
                                // depends on this context's allocation history -- every rank must cut the same chunks)
  bool comm_inflight = false;   // an exchange was enqueued since the last successful tavb_synchronize
  Buffer d_local;   // this shard's [nq, k] lists when they do not fit d_xlocal
  Buffer d_xlocal;  // this shard's lists of an exchange up to comm_reserve_keys keys; the TAVB_KEY_PEER_FAILED lists of a rank that failed
  Buffer d_gather;  // the all-gathered [world][chunk queries][k]

  // EVERY Buffer declared above, once: tavb_destroy releases through this, so a workspace that is listed here cannot be left behind (round 5
  // found the fp16 shadow -- half an fp32 corpus' bytes -- missing from the list tavb_destroy then kept by hand).
  // tests/test_abi_symbols.py checks the declarations against this body.
  template <class F>
  void for_each_buffer(F&& f) {
    for (Buffer* b : {&d_queries, &d_queries_f16, &d_lists, &d_out, &d_rows, &d_cand, &d_thr, &d_sample_keys, &d_counts, &d_delta, &d_approx, &d_flag,
                      &d_fb_queries, &d_norm, &d_minscores, &d_fb_cand, &d_shadow, &d_queries_pad, &d_accept, &d_bits, &d_emit, &d_topk_scores, &d_topk, &d_msg_best,
                      &d_sort_keys, &d_sort_ws, &d_rows_pos, &d_rows_query, &d_rows_keys, &d_rows_out, &d_pairs, &d_mask_counts, &d_compact, &d_scope, &d_scope_bits, &d_scope_rows, &d_scope_member, &d_scope_planes, &h_scope, &h_sort_info, &h_topk_rounds, &h_ring[0], &h_ring[1], &d_ring[0], &d_ring[1], &h_stage, &h_out, &h_lists, &h_flag,
                      &d_local, &d_xlocal, &d_gather})
      f(*b);
  }
};

namespace tavb {
namespace host __attribute__((visibility("hidden"))) {

struct Timed {
  tavb_ctx* c;
  int kernel;
  hipEvent_t a = nullptr, b = nullptr;
  Timed(tavb_ctx* ctx, int k) : c(ctx), kernel(k) {
    if (!c->profiling) return;
    auto get = [&](hipEvent_t* ev) {
      if (!c->free_events.empty()) {
        *ev = c->free_events.back();
        c->free_events.pop_back();
        return true;
      }
      return hipEventCreate(ev) == hipSuccess;
    };
    if (get(&a) && get(&b)) {
      (void)hipEventRecord(a, c->stream);
    } else {
      a = b = nullptr;
    }
  }
  ~Timed() {
    if (!a) return;
    (void)hipEventRecord(b, c->stream);
    c->pending.push_back({kernel, a, b});
  }
};

int drain_timings(tavb_ctx* c);                                // tavb_abi.hip
void parallel_copy(void* dst, const void* src, size_t bytes);  // tavb_abi.hip: host -> pinned, on a few threads when it is worth them

inline int check_ctx(const tavb_ctx* c) {
  if (!c) return fail(TAVB_E_INVALID, "null context");
  return TAVB_OK;
}

// after check_ctx, by every lookup that reads the corpus
inline int require_corpus(const tavb_ctx* c) {
  if (c->dim <= 0 || (!c->corpus && c->rows != 0)) return fail(TAVB_E_NO_CORPUS, "no corpus set (call tavb_set_corpus first)");
  return TAVB_OK;
}

inline u64_t host_key(float score, uint32_t index) {
  uint32_t bits;
  memcpy(&bits, &score, sizeof bits);
  return ((u64_t)bits << 32) | (u64_t)(0xFFFFFFFFu - index);
}

// key -> (position + base, score)
inline void decode_key(u64_t key, int64_t base, int64_t* ordinal, float* score) {
  const uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key;
  memcpy(score, &hi, sizeof *score);
  *ordinal = (int64_t)(0xFFFFFFFFu - lo) + base;
}

inline void decode(const u64_t* keys, int nq, int k, int64_t base, int64_t* ordinals, float* scores, int32_t* counts) {
  for (int q = 0; q < nq; ++q) {
    int m = 0;
    for (int i = 0; i < k; ++i) {
      const u64_t key = keys[(size_t)q * k + i];
      if (key == 0) break;  // lists are sorted: the first empty slot ends the list
      decode_key(key, base, &ordinals[(size_t)q * k + i], &scores[(size_t)q * k + i]);
      ++m;
    }
    counts[q] = m;
  }
}

// ---- tavb_route.hip
// the context's scan geometry with `waves` brought into 1 .. 16 (`blocks` is the caller's to set)
tavb::ScanGeometry clamped_geometry(const tavb_ctx* c);
int scan_blocks_for(const tavb_ctx* c, int64_t n_pos, int waves, int unroll);
// The arguments of a streaming-scan launch over the context's corpus: `nq` queries at d_q, n_pos positions (d_rows: a subset's rows, or
// null), per-workgroup lists at `lists` (null where the launch writes none).  min_score[0 .. fill) = the queries' thresholds, then +inf;
// the slots from `fill` on stay zero (TAVB_MAX_GROUPED_QUERIES in the one-launch and score-pass forms, TAVB_MAX_STREAM_QUERIES elsewhere).
// `group` and the topk_* members are left zero for the caller.
tavb::ScanParams scan_params(const tavb_ctx* c, const float* d_q, const int32_t* d_rows, int64_t n_pos, int nq, int k, uint32_t index_base,
                             u64_t key_bound, u64_t* lists, const float* min_scores /*host, nq*/, int fill);
struct DirectGroupPlan {
  int group;   // queries per group
  int blocks;  // row workgroups per group
  bool worth;  // predicted faster than the other routes (or forced by the `direct_group` option)
};
DirectGroupPlan plan_direct_group(const tavb_ctx* c, int nq, int k, int full_blocks, bool host);
// Core: queries on device (f32 [nq, dim]) -> sorted key lists d_out [nq, k] (async on the stream).
// The self-join's operand and bound (tavb_lookup_pairs.hip): the cached row-norm maxima in d_norm brought up to the corpus' rows and, for an
// fp32 corpus, its fp16 shadow in d_shadow -- reserved and filled the way the wide route does it; enqueued, nothing waited for.
int prepare_join_operand(tavb_ctx* c);
int search_device_impl(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const int32_t* d_row_ids, int64_t n_pos,
                       uint32_t index_base, u64_t* d_out, u64_t key_bound = ~0ull);

// Masked batch on the 32/64-query tile: dev_bits = the allow-mask over the corpus rows, [first_row, last_row] holds every set bit; keys carry
// index_base + row -> d_out [nq, k] (async on the stream).  The caller has checked skinny_supported and the bounds.
int search_masked_tile(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const uint32_t* dev_bits, int64_t first_row,
                       int64_t last_row, uint32_t index_base, u64_t* d_out);
// Masked batch on the 128/256-query filter tile + exact rescoring (fp16 corpora; masked_wide_supported): the same mask and span, plus the mask's
// resident row list (dev_rows, n_allowed: tavb_mask_expand) for the re-run of flagged queries on the gather route -- the one host round trip,
// taken by every call (the flag list is read back).  Scores are the streaming kernels' float32 scores: the gather route's answers bit for bit.
bool masked_wide_supported(const tavb_ctx* c, int k);
int search_masked_wide(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const uint32_t* dev_bits, int64_t first_row,
                       int64_t last_row, const int32_t* dev_rows, int64_t n_allowed, uint32_t index_base, u64_t* d_out);

// A scoped batch: query q searches the rows masks[q] names (HOST array of nq device pointers to packed masks over the corpus' rows, none
// null; the caller has checked 1 <= k <= TAVB_MAX_FUSED_K and 0 < rows < 2^31 - 1).  In passes of TAVB_MAX_STREAM_QUERIES queries (4 for
// k > 64): the union of the pass' masks, its row list and the membership bytes on the device, the scoped streaming scan over that list, the
// merge into `work` [nq, k] and the remap of the positions to index_base + row on the way to `out` [nq, k] (`work` == `out`: in place).
// ONE synchronise inside (the unions' counts); the scans, merges and remaps are enqueued and not waited for.
int search_scoped_impl(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const uint32_t* const* masks, uint32_t index_base,
                       u64_t* work, u64_t* out);

// What the row-list routes of a scoped batch share (search_scoped_impl, search_scoped_topk_impl, search_scoped_sorted_impl): a WAVE of
// passes of per_pass (at most 8) queries.  scope_wave_unions enqueues the union of every pass' masks, synchronises ONCE for their sizes
// and reserves d_scope_rows / d_scope_member for the wave (nothing when every union is empty: total == 0); scope_wave_lists then
// enqueues, for a pass whose union is not empty, the write pass of its ascending row list and its membership bytes (bit j = query j of the
// pass).  scoped_wave_queries: the queries of one wave -- at most 16 passes, fewer on corpora beyond 4M rows (the workspaces' bound).
struct ScopeWave {
  int nq, per_pass, passes;
  std::vector<tavb::MaskOperands> ops;       // per pass: its masks
  std::vector<int64_t> n_union, first_pos;  // per pass: rows of its union, where its list starts in the workspaces
  int64_t total, most;                       // the unions' total and largest length
};
int scope_wave_unions(tavb_ctx* c, int nq, int per_pass, const uint32_t* const* masks, ScopeWave* w);
int scope_wave_lists(tavb_ctx* c, const ScopeWave& w, int p, const int32_t** list_out, const uint8_t** member_out);
int scoped_wave_queries(const tavb_ctx* c, int per_pass);

// A scoped batch on the 32/64-query tile: the same masks; [first_row, last_row] holds every set bit of every mask.  Per wave of query tiles
// the membership planes (c->d_scope_planes), then the tile ladder over the span with the per-query test in its admission path; keys carry
// index_base + row -> d_out [nq, k].  Nothing is waited for.  The caller has checked skinny_supported and the bounds.
int search_scoped_tile(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const uint32_t* const* masks, int64_t first_row,
                       int64_t last_row, uint32_t index_base, u64_t* d_out);
// the planes alone (tavb_scope_planes): words from one block's plane to the next for that span, blocks of the tile-padded batch of n masks,
// and the launches that write n_blocks * stride words at `planes`
int64_t scope_plane_stride(int64_t first_row, int64_t last_row);
int scope_plane_blocks(int n);
int build_scope_planes(tavb_ctx* c, const uint32_t* const* masks, int n, int n_blocks, int64_t first_row, int64_t last_row, uint32_t* planes);
// A scoped batch on the 128/256-query filter tile + exact rescoring (fp16 corpora; masked_wide_supported): the same masks and span.  Per wave
// of query tiles the membership planes (c->d_scope_planes, at most "scope_wave_bytes" of them, at least one 256-query tile's), the filter
// ladder over the span with the per-query test in its admission path, the band selection and the rescoring; flagged queries are read back
// (one synchronise per wave) and re-run through search_scoped_impl with their own masks.  Scores are the streaming kernels' float32 scores:
// search_scoped_impl's answers bit for bit.  keys carry index_base + row -> d_out [nq, k].
int search_scoped_wide(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const uint32_t* const* masks, int64_t first_row,
                       int64_t last_row, uint32_t index_base, u64_t* d_out);

// ---- tavb_lookup.hip
// Staging: [nq, dim] queries of the caller -> pinned h_stage (stage_queries_host; *d_q = where submit_queries then copies them) -- stage_queries
// does both.  stage_subset: one query and a subset's rows (int64 on the host, checked against the corpus; int32 at *d_rows), both copies enqueued;
// the caller has checked 0 < n_subset < 2^31 - 1.
int stage_queries_host(tavb_ctx* c, const float* queries_host, int nq, const float** d_q);
// Queries the tiles must not multiply.  The 32/64-query tile on fp16 rows, both exact fallbacks and the filter see a query through fp16
// planes (hi = fp16(q), lo = fp16(q - hi)): a finite element of magnitude 65520 or more becomes an infinite high part, and two of them,
// or one over a zero of a row, make a NaN where the fp32 dot product is finite.  A query that holds +-inf or NaN itself leaves the tiles
// too: a dot product of -inf clips to the score 0.0, which passes min_score 0, but never passes the tiles' admission test on the raw dot
// product.  stage_queries_host looks at every element while it copies
// (the only place the host sees the queries; no launch, no synchronise) and the routes ask here: true when d_q points into the staging
// buffer of a batch that holds such a query -- the whole batch then runs on the streaming kernels, whose answer is the definition.
// Queries a caller keeps on the device are never seen: their elements must round to finite fp16 values (include/tavb.h).
inline bool staged_overflow(const tavb_ctx* c, const float* d_q) {
  const char* const p = reinterpret_cast<const char*>(d_q);
  const char* const b = reinterpret_cast<const char*>(c->d_queries.ptr);
  return c->staged_overflow && b != nullptr && p >= b && p < b + c->d_queries.cap;
}
hipError_t submit_queries(tavb_ctx* c, int nq);
int stage_queries(tavb_ctx* c, const float* queries_host, int nq, const float** d_q);
int stage_subset(tavb_ctx* c, const float* query_host, const int64_t* rows_host, int64_t n_subset, const float** d_q, const int32_t** d_rows);
// keys carry ordinal_base + row in 32 bits: TAVB_E_UNSUPPORTED where the corpus does not fit (the message names device-resident keys or not)
int check_key_ordinals(const tavb_ctx* c, bool device_resident);
// the empty result of a device-resident lookup that has nothing to scan: n zero keys at `out` (async on the stream)
int fill_empty_keys(tavb_ctx* c, u64_t* out, int64_t n);
// the tail of a host-synchronous lookup whose last kernel wrote [nq, k] keys into h_out: ONE synchronise, the keys decoded into the caller's arrays
int sync_decode(tavb_ctx* c, int nq, int k, int64_t base, int64_t* ordinals, float* scores, int32_t* counts);
// Where the keys of a batched host-synchronous lookup land: up to kPinnedKeysMax of them in pinned host memory (h_out: the last kernel
// writes them there, as in the single-query forms -- a remap of a few KiB runs on them in place); more are written in device memory (d_out)
// and copied out once -- no merge writes megabytes over PCIe.  rounds (optional): the rounds [nq] of a large-k lookup stay reserved
// behind the keys in h_out either way (reserve_topk_out).
constexpr size_t kPinnedKeysMax = 4096;
int reserve_key_target(tavb_ctx* c, int nq, int k, u64_t** target, int32_t** rounds = nullptr);
// the keys at `target` -> h_out (when they are not there already), ONE synchronise, the caller's arrays; rounds (optional): reported
// after the synchronise (note_rounds)
int collect_keys(tavb_ctx* c, const u64_t* target, int nq, int k, int64_t base, int64_t* ordinals, float* scores, int32_t* counts,
                 const int32_t* rounds = nullptr);
// the empty answer of a host form: every count zero, nothing launched
inline int empty_counts(int32_t* counts, int nq) {
  for (int q = 0; q < nq; ++q) counts[q] = 0;
  return TAVB_OK;
}
// What a lookup that is no plain fused-k lookup resets before it runs: the large-k rounds, "last_direct", "last_graph" (not where
// clear_graph is false: the gather route of a masked batch leaves it as it was) -- and "masked_route" = route.
inline void note_route(tavb_ctx* c, int64_t route, bool clear_graph = true) {
  c->last_topk_refine = 0;
  c->topk_rounds_pending = 0;
  c->last_direct = 0;
  if (clear_graph) c->last_graph = 0;
  c->masked_route = route;
}
// every mask of a list present and 4-byte aligned; `who` names one in the texts ("the mask of query", "mask")
int check_mask_list(const uint32_t* const* masks, int n, const char* who);
// positions -> base + rows[position] over n keys (launch_remap_positions; in == out: in place)
int remap_key_rows(tavb_ctx* c, const u64_t* in, u64_t* out, int64_t n, const int32_t* rows, int64_t n_rows, uint32_t base);
// the message lookups: the row -> message map is set and covers the corpus (check_message_map); that, plus context, corpus, 1 <= k <=
// TAVB_MAX_FUSED_K and max_messages >= 0 (check_message_args)
int check_message_map(const tavb_ctx* c);
int check_message_args(tavb_ctx* c, int k, int32_t max_messages);
// n_accept accepted message ordinals on the host -> their bitmap over n_messages ordinals in d_bits (zeroed first; ordinals outside
// [0, n_messages) are ignored), all enqueued on the stream
int stage_accept_bitmap(tavb_ctx* c, const int32_t* accept_msgs_host, int64_t n_accept, const uint32_t** d_bits);

// ---- tavb_lookup_topk.hip
int check_topk_args(tavb_ctx* c, int k);  // context, corpus, 1 <= k <= TAVB_MAX_LARGE_K
// check_topk_args, the row list's shape and a row -> message map that covers exactly the corpus; *empty: nothing to scan
int check_top_messages_args(tavb_ctx* c, int k, const int32_t* dev_rows, int64_t n_rows, bool* empty);
// The merge of top-messages lists (tavb_merge_top_messages_device): n_lists (1 .. 64) sorted, zero-padded device lists of k keys per query
// carrying MESSAGE ordinals below nm, laid out as launch_merge_topk takes them -> out_keys [nq][k], per message its largest key, the best k,
// sorted and zero-padded, + out_rounds [nq]; both device-writable.  A query one of whose lists leads with TAVB_KEY_PEER_FAILED is that key
// in every slot.  Uses d_msg_best and d_topk, not the row -> message map; nothing is waited for.  The caller has checked the shape.
int merge_top_messages_impl(tavb_ctx* c, const u64_t* lists, int n_lists, int nq, int k, bool query_major, int64_t nm, u64_t* out_keys, int32_t* out_rounds);
// the pinned keys [nq][k] + rounds [nq] of a large-k lookup (h_out), and what tavb_search_topk reports of the rounds ("last_topk_refine")
int reserve_topk_out(tavb_ctx* c, int nq, int k, u64_t** keys, int32_t** rounds);
void note_rounds(tavb_ctx* c, const int32_t* rounds, int nq);
// Exact top-k beyond the fused selection: queries on the device over n_pos positions (d_rows: a subset's rows, or null) -> out_keys [nq][k]
// sorted, zero-filled, + out_rounds [nq], both device-writable; nothing is read back before the caller's one synchronise.
int search_topk_impl(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const int32_t* d_rows, int64_t n_pos,
                     uint32_t index_base, u64_t* out_keys, int32_t* out_rounds);
// The large-k lookup (tavb_search_topk's passes) with the queries on the device and nothing waited for: nq sorted, zero-padded lists of k keys
// carrying index_base + position -> out_keys (device or device-writable pinned memory); d_rows: a subset's rows (nq == 1), or null.
int search_topk_async(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const int32_t* d_rows, int64_t n_pos,
                      uint32_t index_base, u64_t* out_keys);

// The best k MESSAGES of every query (tavb_search_top_messages): queries on the device over the corpus (d_rows null) or over n_rows valid
// rows at d_rows; the caller has checked the row -> message map (it covers the corpus, 1 <= n_messages < 2^31 - 1), 1 <= k <=
// TAVB_MAX_LARGE_K and that there is something to scan.  Per group of queries: two memsets, the score pass with the MessageMaxSink, the
// histogram pass over [queries][n_messages], then search_topk_impl's launches with the message ordinals as positions -> out_keys [nq][k]
// sorted, zero-filled keys carrying MESSAGE ordinals, + out_rounds [nq], both device-writable; nothing is waited for.
int search_top_messages_impl(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const int32_t* d_rows, int64_t n_rows,
                             u64_t* out_keys, int32_t* out_rounds);
// The same under one scope per query (tavb_search_top_messages_scoped; masks as for search_scoped_impl, the caller's checks as above plus
// 0 < rows < 2^31 - 1): waves and passes as in search_scoped_topk_impl, a pass being min(topk_queries_per_pass, 8) queries over the
// ascending row list of the union of its scopes; per sub-group of a pass (one, unless [queries][n_messages] would pass
// "topk_scores_bytes") the group above with the scoped score pass -- a row raises its message's slot for query j only when bit j of its
// membership byte is set.  Keys carry message ordinals: no remap.  out_rounds: pinned host memory (the queries of empty unions get their
// zero from the host).  ONE synchronise per wave (the unions' sizes); everything else is enqueued and not waited for.
int search_scoped_top_messages_impl(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const uint32_t* const* masks,
                                    u64_t* out_keys, int32_t* out_rounds);
// The same on the 32/64-query tile (tavb_search_top_messages_tile): groups of up to 64 queries, cut by "topk_scores_bytes" over
// [queries][n_messages]; per group the memset of its slots of d_msg_best and top_messages_tile_pass, then per eight queries the memset of the
// selection's head and search_top_messages_impl's histogram pass, refinement, compaction and finish.  dev_bits (optional): ONE packed mask
// over the corpus' rows whose set bits lie in [first_row, last_row].  The caller has checked what search_top_messages_impl's has, that rows
// are a multiple of 64 bytes and the alignment of the mask and the map.  Nothing is waited for unless the thresholds differ (their upload).
int search_top_messages_tile_impl(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const uint32_t* dev_bits,
                                  int64_t first_row, int64_t last_row, u64_t* out_keys, int32_t* out_rounds);
// tavb_route.hip: ONE launch of the 32/64-query tile in its top-messages form for n <= 64 queries at d_q over the mask's span (dev_bits
// null: the corpus) -> best [n][n_messages] (zeroed by the caller).  Sets last_tier, last_skinny_kernel and masked_route.
int top_messages_tile_pass(tavb_ctx* c, const float* d_q, int n, const float* min_scores /*host, n*/, const uint32_t* dev_bits, int64_t first_row,
                           int64_t last_row, unsigned* best);

// A scoped batch at 1 <= k <= TAVB_MAX_LARGE_K (masks as for search_scoped_impl): per pass of min(topk_queries_per_pass, 8) queries the
// scoped score pass over the pass' union list, the refinement rounds, the compaction and the finish into `work` [nq, k], and the remap of
// the positions to index_base + row on the way to `out` [nq, k] (`work` == `out`: in place; both device-writable); out_rounds [nq + 1]
// device-writable and 8-byte aligned.  A pass whose score array would pass "topk_scores_bytes" goes in sub-groups of its queries over the
// same list.  ONE synchronise per wave (the unions' sizes); everything else is enqueued and not waited for.
int search_scoped_topk_impl(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const uint32_t* const* masks,
                            uint32_t index_base, u64_t* work, u64_t* out, int32_t* out_rounds);

// tavb_search_sorted's passes with the queries on the device (k: 1 .. c->rows, the whole corpus; results carry base + row): synchronises per
// group of queries and per piece of results, as tavb_search_sorted does
int search_sorted_device(tavb_ctx* c, const float* d_q, int nq, int64_t k, const float* min_scores /*host, nq*/, int64_t base, int64_t max_total,
                         int64_t* out_ords, float* out_scores, int64_t* out_counts, int64_t* out_total);

// ---- tavb_lookup_masked.hip
// what the scoped entry points check after their own head: 1 <= k <= k_max, the masks; *empty: nothing to scan
int check_scoped_args(tavb_ctx* c, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k, int32_t k_max, bool* empty);
// the span of a masked lookup that has something to scan
int check_masked_span(bool empty, int64_t rows, int64_t first_row, int64_t last_row);

// ---- tavb_mask_entry.hip: the chunk infos a count pass leaves in pinned memory
// before the launch: every info unwritten (a chunk the kernel wrote holds a row or INT32_MAX in `first`)
void mark_chunk_infos(tavb::MaskChunkInfo* info, size_t n);
// after the synchronise: a chunk that wrote nothing is an internal error ("chunk %d of <what> wrote no info"); the counts' sum, the least
// first and the greatest last
struct ChunkSum {
  int64_t count = 0, first = 0x7FFFFFFFll, last = -1;
};
int sum_chunk_infos(const tavb::MaskChunkInfo* info, int blocks, const char* what, ChunkSum* sum);

// ---- tavb_comm.hip
int comm_wait_or_abort(tavb_ctx* c);

}  // namespace host
}  // namespace tavb

// tavb_route.hip.  Not part of the public ABI.
int tavb_search_device_dispatch(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores, uint32_t index_base, u64_t* d_out);
