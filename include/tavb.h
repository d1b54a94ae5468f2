/*
 * tavb.h -- C ABI of libtavb.so, the MI355X (gfx950) engine behind typeagent's
 * VectorBase nearest-neighbour lookup.
 *
 * The reference (microsoft/typeagent-py) has no FFI: the boundary it offers is the
 * Python class `typeagent.aitools.vectorbase.VectorBase`
 * (src/typeagent/aitools/vectorbase.py:82-287).  The entry points below are what a
 * ctypes binding for that class's numeric methods binds; each one cites the
 * reference lines whose arithmetic it replaces.  `typeagent_py_amd/_native.py` is
 * that binding; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - plain C types only; no torch / HIP types in signatures (a `void* stream` is an
 *    opaque hipStream_t, NULL = the context's own stream).
 *  - every function returns TAVB_OK (0) or a negative TAVB_E_* code; the message for
 *    the calling thread's last failure is `tavb_last_error()`.  The library never
 *    calls abort()/exit().
 *  - "dev" pointers are device memory owned by the caller (normally a torch tensor);
 *    the library never frees them and keeps `tavb_set_corpus`'s pointer only until
 *    the next tavb_set_corpus / tavb_destroy.  Host pointers are not retained after
 *    a call returns; all outputs are caller-allocated.
 *  - one in-flight call per context (the Python wrapper enforces this).
 *  - results are ordered by (score descending, ordinal ascending); the reference's
 *    order among exactly equal float32 scores is numpy-implementation-defined
 *    (vectorbase.py:183-187), ours is deterministic.
 *  - scores are the reference's public 0..1 scale: clip((cos + 1) / 2, 0, 1) evaluated
 *    in float32 (vectorbase.py:44-47); `min_score` is compared as float32
 *    (vectorbase.py:179 under NEP 50); NaN scores never pass (numpy `>=`).
 */
#ifndef TAVB_H
#define TAVB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point, a signature, an option or a kernel id changes incompatibly; the binding refuses a library of another version */
#define TAVB_ABI_VERSION 7

#define TAVB_OK 0
#define TAVB_E_INVALID (-1)     /* bad argument */
#define TAVB_E_HIP (-2)         /* a HIP runtime call failed; message has hipGetErrorString */
#define TAVB_E_NO_CORPUS (-3)   /* search before tavb_set_corpus */
#define TAVB_E_UNSUPPORTED (-4) /* shape outside what the kernels cover (see message) */
#define TAVB_E_NOMEM (-5)
#define TAVB_E_TIMEOUT (-7)     /* tavb_synchronize: an exchange did not complete within "comm_timeout_ms"; the communicator was aborted */
#define TAVB_E_PEER (-6)        /* tavb_decode_keys: the lists come from a collective lookup in which a rank's local search failed (they lead with TAVB_KEY_PEER_FAILED) */

#define TAVB_F32 0
#define TAVB_F16 1

/* Largest k served by the fused select-while-streaming kernels. */
#define TAVB_MAX_FUSED_K 256
/* Largest k of tavb_search_topk / tavb_search_subset_topk (exact top-k after one corpus pass, sorted in LDS). */
#define TAVB_MAX_LARGE_K 16384
/* Largest number of queries one streaming pass serves (bigger batches are split). */
#define TAVB_MAX_STREAM_QUERIES 8
/* Rows of a mask one workgroup of tavb_mask_expand covers (its two launches have ceil(rows / this) workgroups each). */
#define TAVB_MASK_ROWS_PER_WORKGROUP 16384
/* Scope algebra (tavb_mask_from_ranges, tavb_mask_combine): most range collections of one scope, most operands of one combination, the
 * operations, and the most merged intervals (all collections together) a workgroup of the range kernel stages in LDS -- one more and it
 * searches them in device memory. */
#define TAVB_MAX_SCOPE_COLLECTIONS 8
#define TAVB_MAX_MASK_OPERANDS 8
#define TAVB_MASK_AND 0
#define TAVB_MASK_OR 1
#define TAVB_MASK_ANDNOT 2
#define TAVB_SCOPE_LDS_RANGES 1024
/* The edits tavb_mask_remap carries masks through. */
#define TAVB_REMAP_REMOVE 0
#define TAVB_REMAP_INSERT 1
#define TAVB_REMAP_APPEND 2

typedef struct tavb_ctx tavb_ctx;

/* ---- library ---------------------------------------------------------------- */
int tavb_version(void);
const char* tavb_last_error(void);
int tavb_device_count(int* out_count);

/* ---- context ---------------------------------------------------------------- */
/* One context per (process, GPU).  `stream` = an existing hipStream_t to launch on
 * (e.g. torch.cuda.current_stream().cuda_stream) or NULL to create a private one. */
int tavb_create(int device, void* stream, tavb_ctx** out);
int tavb_destroy(tavb_ctx* ctx);
int tavb_synchronize(tavb_ctx* ctx);

/* Tunables (launch geometry etc.); unknown names -> TAVB_E_INVALID.
 *   "scan_blocks"   workgroups of the streaming scan (0 = auto: one per CU)
 *   "scan_waves"    waves per workgroup, 1..16 (default 16)
 *   "scan_unroll"   rows in flight per wave: 1, 2 or 4 (default 2)
 *   "scan_nt"       1 = non-temporal corpus loads (default 1)
 *   "scan_pipe"     1 = software-prefetch next rows before reducing current ones
 *   "force_tier"    0 = auto, 1 = fixed-D kernel, 2 = vector kernel, 3 = scalar kernel
 *   "mfma_min_batch" smallest batch routed to the 128/256-query MFMA tile (default 65; on corpora of "mfma_big_bytes" (default 256 MiB) or more: "mfma_min_batch_big", default 33; dim % 64 == 0 directly, other widths -- multiples of 8 on
 *                   fp16 corpora, of 16 on fp32 ones -- on a zero-padded fp16 copy of the rows (+ device memory: rows x pad64(dim) x 2 bytes); k up to TAVB_MAX_FUSED_K on either
 *                   (fp32 corpora through their fp16 shadow; beyond k = 64 a flagged query of an fp32 corpus is re-run on the streaming kernels after ONE
 *                   host round trip, so such a call may block before it returns); thresholds may differ per query; k > 64 rides the tile from 9 queries,
 *                   3 on corpora of mfma_big_bytes and more -- the streaming kernels take four such queries per corpus pass)
 *   "mfma_min_batch_f32", "mfma_min_batch_big_f32" / "mfma_big_bytes_f32", "mfma_few_bytes_f32"  FP32 corpora: batches that take the wide tile over the fp16 shadow
 *                   (needs "f32_shadow" >= 1) + exact fp32 rescoring instead of the fp32 kernels -- half the bytes per pass and fp16 matrix rates:
 *                   from mfma_min_batch_f32 (default 33) queries at any corpus size (64 queries over 5000 x 1536 rows: 0.11 against 0.20 ms on the 64-query
 *                   fp32 tile), from mfma_min_batch_big_f32 (default 5) queries on corpora of mfma_big_bytes_f32 (default 1e9 bytes) or more (32 queries over
 *                   1M x 1536 rows: 0.73 against 1.24 ms), and batches of 2 .. 4 queries on corpora of mfma_few_bytes_f32 (default 4 GiB) or more (0.78 against
 *                   0.97 ms at 1M rows x 1.5); mfma_min_batch_big_f32 > 64 switches the last two rules off
 *   "skinny_min_batch_f32" / "skinny_min_batch_f16"  smallest batch routed to the 32/64-query MFMA tile on fp32 / fp16
 *                   corpora (defaults 5 / 3, the measured break-even; used up to
 *                   mfma_min_batch - 1); smaller batches use the streaming tiers
 *   "mfma_sample_rows", "mfma_ladder"  phases of the MFMA paths' threshold ladder: rows of the first phase (0 = auto: one
 *                   tile per workgroup; -1 = a single phase, no seeding) and the growth factor of the following ones
 *   "f32_shadow"            1 (default): batches of mfma_min_batch+ queries on FP32 corpora run the fp16 tile over an fp16 shadow copy of the corpus
 *                           (built on first use, +50 % device memory, extended on append) and rescore the candidates with the fp32 rows: same
 *                           answers, ~6x the throughput of the fp32 matrix path; 0: fp32 kernels only (the shadow is freed); 2: EVERY lookup
 *                           (single queries included) on fp32 corpora of "f32_shadow_min_bytes" (default 2 GiB) and more filters on the
 *                           shadow with the 32/64-query tile: half the bytes per pass (1M x 1536: 0.93 -> 0.70 ms per query, 32 queries 1.46 -> 0.94 ms)
 *   "last_shadow"           (get) 1 when the last lookup's corpus pass read the shadow
 *   "norm_rows"             (get) the corpus rows the cached row-norm maxima (and the shadow, where there is one) cover: a large batch extends them
 *                           to every row, a rewrite of covered rows (tavb_corpus_modified) drops them to 0, tavb_scatter_rows keeps them
 *   "mfma_tile"             queries per workgroup tile of the wide fp16 kernel: 0 = auto (128 where that pads less: up to 128, 257..384, 513..640 queries; else 256), 128, 256
 *   "mfma_splits", "mfma_sched", "mfma_ablate"  measurement knobs: row ranges per launch; staging variant (256-query tile: 1 / 2 = other piece
 *                           schedules, 3 / 4 / 5 = other issue orders of a slice's MFMAs -- profiles/r06_mfma_power.md; 32-query tile: 7 = LDS-DMA ring (the default), 8 = deep corpus ring, 5 = register staging four K steps
 *                           deep, 9 = 64-byte K steps -- profiles/r05_mid_batch.md); parts of a tile kernel compiled out (answers are garbage)
 *   "graph_max_bytes"       single-query lookups (tavb_search / tavb_search_batch with nq = 1) on corpora of at most this many bytes replay ONE
 *                           captured HIP graph (query H2D, scan, merge into pinned host memory) instead of three submissions; the first call
 *                           of a (corpus, k, min_score) shape runs plain, the second captures, later ones replay.  Default 0 = never: on
 *                           ROCm 7.2 the replay measured SLOWER than the plain submissions (48 vs 41 us at 10k x 1536)
 *   "last_graph"            (get) 1 when the last lookup was such a replay
 *   "comm_force"            1: tavb_search_allgather runs its all-gather + merge even in a world of one rank (tests, dry runs)
 *   "comm_fail_rank"        fault injection (default -1 = off): on the rank of the communicator with this number the local search of
 *                           tavb_search_allgather fails as a launch or an allocation inside it would -- that rank still joins the all-gather
 *                           (with TAVB_KEY_PEER_FAILED lists) and returns its error, every other rank's lists decode to TAVB_E_PEER
 *   "comm_reserve_keys"     keys per rank of the exchange buffers tavb_comm_init reserves (default 2^20 = 8 MiB + world x 8 MiB; set BEFORE tavb_comm_init):
 *                           an exchange of up to that many keys (nq x k) allocates nothing between entering tavb_search_allgather and ncclAllGather;
 *                           bigger ones travel through the same buffers in chunks of whole queries (cut by the value tavb_comm_init read: set the same on every rank);
 *                           "up to that many" is judged by the value tavb_comm_init read, not by what the buffers happen to hold after a re-init with a smaller reserve
 *   "comm_timeout_ms"       0 (default) = tavb_synchronize waits for an exchange for ever; > 0: after that many milliseconds the communicator is
 *                           aborted (ncclCommAbort: the stream drains), the context is left without one and tavb_synchronize returns TAVB_E_TIMEOUT
 *   "comm_fail_alloc"       fault injection: 1 = the per-call list allocation of tavb_search_allgather (lists beyond comm_reserve_keys) fails; the rank
 *                           still joins every chunk of the exchange with TAVB_KEY_PEER_FAILED lists
 *   "comm_stall_ms"         fault injection (one shot, 0..5000): the next exchange is held up on the stream for that long, as by a late peer
 *   "comm_world", "comm_rank" (read only) shape of the context's communicator (0 / -1 without one)
 *   "last_tier" (read only) the kernel family of the last lookup: 1-3 streaming tiers, 4 = 256-query MFMA tile (exact
 *                   filter + fp32-query rescoring of its candidates), 5 = 32/64-query MFMA tile
 *   "last_flagged" (read only; synchronises) queries of the last 256-query-tile lookup whose candidate set could not be
 *                   proven complete and were re-run exactly (0 on ordinary data)
 *   "band_max"      256 .. 2048 (default 2048; 1024 until ABI 6): the most candidates per query the 128/256-query tile's selection hands to the exact
 *                   rescoring -- every row within 2 delta of the approximate k-th best.  A query with MORE rows than that inside its band (next to a
 *                   bigger cluster of near-duplicates) is flagged and re-run exactly; a band of 1500 near-duplicates per query (bench.py cfg3_dup) used
 *                   to cost the whole batch an exact pass of twice the MFMAs and now costs 1500 gathered rows per query in the rescoring
 *   "wide_fallback" 1 (default): when MORE than 64 queries of a batch of 256+ are flagged, they are re-run on the 256-query tile in its
 *                   exact split-plane form (fp32 queries as two fp16 planes) instead of 64 at a time on the 64-query exact tile; 0 = never
 *   "early_exact"   1 (default): with wide_fallback, a batch MOST of whose queries (> nq / 2) already hold, before the last and biggest filter phase, a band that
 *                   extrapolates past the band buffer (every query next to more near-duplicates than a band holds) skips that phase, its selection and the
 *                   rescoring, and all its queries take the exact split-plane form at once; "last_doomed" (read only; synchronises) = that count
 *   "mfma_shape"    16 (default) / 32: the MFMA of the 256-query filter tile, v_mfma_f32_16x16x32_f16 or v_mfma_f32_32x32x16_f16 (same tile, same
 *                   answers bit for bit; 16 is faster on cfg3, measured in profiles/r09_mfma_shape.md).  The routing: tavb_plan_filter_shape.  The SPLIT exact form, the 128-query
 *                   tile, "mfma_bdirect", "mfma_sched" and the ablations other than 256 / 258 always run 32x32x16.  "last_mfma_shape" (read only) = the
 *                   shape the last filter launch of the 128/256-query tile ran on (0 before the first)
 *   "last_skinny_kernel" (read only) what the last launch of the 32/64-query tile instantiated (0 before the first): variant * 10000 + bytes per K
 *                   step * 100 + queries per tile.  Variant 0 = the LDS-DMA ring (ships); under "mfma_sched" 8 / 6 / 5 on whole-line widths and 32 queries
 *                   1 = deep ring, 2 = half tiles of 128 rows, 4 = register staging (K steps a multiple of 4; else the ring).  The step is 128 bytes
 *                   when a row is a multiple of that and "mfma_sched" is not 9, else 64: 12832, 12864, 6432, 6464, 22832, 32832, 52832
 *   "mfma_bdirect"  0 (default) / 1: the 256-query tile takes its query operand in MFMA-fragment-major order straight from L2 into registers
 *                   (no LDS staging; three corpus slots instead of two): measured +0.8 %, kept as an option (profiles/r04_cfg3_kernel.md section 10)
 *   "small_direct_bytes" host-synchronous lookups of one query (tavb_search) or a few (tavb_search_batch with nq <= 8; <= 4 for k > 64) on corpora up
 *                   to this many bytes (default 128 MiB; 0 = never) are ONE launch ("small_direct_keys", default 8192: the most keys the lists may hold
 *                   -- the grid is cut to fit; twice that for a batch, which goes the usual way when its share would starve the grid): the scan's per-workgroup lists go to pinned host memory and are merged
 *                   on the host; "last_direct" (read only) = 1 when the last lookup took that path, 2 when in addition the query rode
 *                   inside the kernel arguments ("inline_query", default 1: 1536-wide queries on the default scan form; no H2D copy before the launch)
 *   "direct_group_max_nq" (default 128; 0 = never) batches of 2 .. this many queries (k <= 64) on corpora up to "small_direct_bytes" take that ONE launch
 *                   in its GROUPED form wherever a fitted cost model expects it to beat the 32/64-query and wide tiles (a corpus of a few
 *                   thousand rows is one or two busy CUs for a tile): a 2-D grid of row workgroups x query groups of one or two queries
 *                   ("direct_group": 1 / 2 / 4 / 8 forces the group size and the form, 0 = pick), "direct_group_wgs" workgroups in all (0 = pick:
 *                   256 or 512), lists of up to "direct_group_keys" keys (default 32768) merged on the host; "last_direct" = 3.  The
 *                   device-resident calls (tavb_search_device, tavb_search_allgather) take the same scan + ONE merge launch ("last_direct" = 4).
 *                   Either way the answers are the single-query lookups' bit for bit.  profiles/r06_group_sweep.md
 *   "large_k"       1 (default): the Python binding routes lookups of TAVB_MAX_FUSED_K < k <= TAVB_MAX_LARGE_K through tavb_search_topk /
 *                   tavb_search_subset_topk (a device group: tavb_search_topk_device on every shard); 0: through the emit-all pass of tavb_search_all as before (the library itself reads it nowhere else)
 *   "topk_buckets"  64-multiple in 256 .. 4096 (default 1024): histogram buckets of a large-k lookup's score pass, linear over
 *                   [max(min_score, 0), 1] (LDS per workgroup: 4 bytes per bucket and query of the pass)
 *   "topk_boundary_keys" 64 .. TAVB_MAX_LARGE_K (default 16384): keys a query's boundary list holds; a boundary bucket with more keys is
 *                   refined (re-bucketed from the score array) until it fits -- rounds are enqueued up front, about 3 to 5 on corpora of more rows
 *                   than this, none on smaller ones
 *   "topk_scores_bytes" >= 4096 (default 1 GiB): most bytes of the dense score array of one corpus pass (4 bytes per row and query): a
 *                   large-k batch serves fewer than TAVB_MAX_STREAM_QUERIES queries per pass where 8 would need more
 *   "last_topk_refine" (read only) refinement rounds the last large-k lookup needed (the most of any of its queries; 0 on ordinary data
 *                   up to ~16k rows per boundary bucket)
 *   "sort_all"      1 (default): the Python binding routes lookups without a predicate whose max_hits is 0 (every survivor) or above
 *                   TAVB_MAX_LARGE_K through tavb_search_sorted / tavb_search_subset_sorted; 0: through the emit-all pass of tavb_search_all
 *                   and a host sort as before (the library itself reads it nowhere else)
 *   "sort_stage_keys" 1 .. 2^30 (default 2^21): most results of a sorted lookup decoded into pinned memory (12 bytes each) before they
 *                   are copied into the caller's arrays; more results take several such pieces, one synchronise each
 *   "mask_tile"     masked batches (the binding reads it; the rule is tavb_plan_masked): 1 (default) = a batch takes the 32/64-query tile with the bit test in
 *                   its admission path (tavb_search_masked_batch) where tavb_plan_masked says so, else the gather route (the mask expanded to a row list,
 *                   the queries over it eight per pass); 0 = never the tile; 2 = the tile wherever it serves the shape (tests)
 *   "mask_tile_min_bytes"  (default 128 MiB, the default of "small_direct_bytes") allowed rows x row bytes below which a masked batch keeps the gather
 *                   route -- one launch there -- and everything behaves as before the tile route existed
 *   "mask_tile_pct" (default 100 = byte parity) the tile is taken when the gather route's bytes (allowed rows once per 8 queries) are at least this
 *                   many per cent of the tile's (the mask's span once per 64 queries)
 *   "masked_route"  (read only) 0 before the first masked lookup, 1 = the last one took the gather route (tavb_search_subset_batch_resident / _device), 2 = the
 *                   32/64-query tile, 3 = the 128/256-query filter tile + rescoring (tavb_search_masked_wide), 4 = a scoped batch (one mask per
 *                   query: tavb_search_scoped_batch / _device, tavb_search_messages_scoped), 5 = a scoped batch on the 32/64-query tile
 *                   (tavb_search_scoped_tile / _device, tavb_search_messages_scoped_tile), 6 = a scoped batch on the 128/256-query filter tile +
 *                   rescoring (tavb_search_scoped_wide / _device, tavb_search_messages_scoped_wide), 7 = a scoped batch on the large-k route
 *                   (tavb_search_scoped_topk / _device), 8 = a scoped batch on the sorted route (tavb_search_scoped_sorted),
 *                   9 = a scoped top-messages batch (tavb_search_top_messages_scoped / _device), 10 = a top-messages batch on the
 *                   32/64-query tile (tavb_search_top_messages_tile / _device);
 *                   tavb_search_subset_batch_sorted is the gather route: 1
 *   "scope_large_k" (default 1; the binding reads it) 1 = a scoped batch at max_hits beyond TAVB_MAX_FUSED_K, or 0, is ONE call of
 *                   tavb_search_scoped_topk / tavb_search_scoped_sorted (while "large_k" / "sort_all" are on); 0 = the binding loops over
 *                   the per-query masked lookups, as before those calls existed
 *   "top_messages"  (default 1; the binding reads it) 1 = lookup_top_messages_by_embedding(s) is ONE call of tavb_search_top_messages (1 <=
 *                   max_messages <= TAVB_MAX_LARGE_K); 0 = the binding takes the all-survivor lookup and collapses rows to messages on the host
 *   "top_messages_scoped"  (default 1; the binding reads it) 1 = lookup_top_messages_by_embeddings_scoped (one scope per query) is ONE call
 *                   of tavb_search_top_messages_scoped (while "top_messages" is on, 1 <= max_messages <= TAVB_MAX_LARGE_K); 0 = the binding
 *                   loops over the one-mask lookup, as before that call existed
 *   "top_messages_tile"  (default 0; the binding reads it) lookup_top_messages_by_embedding(s), unmasked or under one mask that holds its
 *                   packed bits, on the 32/64-query tile (tavb_search_top_messages_tile): 0 = never -- scores stay tavb_search's bit for bit;
 *                   1 = where tavb_plan_top_messages_tile says so (with "top_messages_tile_min_batch", "mask_tile_min_bytes" /
 *                   "mask_tile_pct"); 2 = wherever the tile serves the shape.  1 and 2 trade the bit-for-bit scores for the tile's own
 *   "top_messages_tile_min_batch"  (default 8, >= 1) fewest queries the plan sends to the tile: the smallest batch measured (profiles/r27_top_messages_tile.md)
 *   "scope_wide"    scoped batches on fp16 corpora (the binding reads it; the rule is tavb_plan_scoped_wide, with "mask_tile_min_bytes" /
 *                   "mask_tile_pct"): 1 (default) = the 128/256-query filter tile + exact rescoring (tavb_search_scoped_wide) where
 *                   tavb_plan_scoped_wide says so -- it then wins over "scope_tile"; 0 = never; 2 = wherever that route serves the shape
 *   "scope_wave_bytes"  most bytes of membership planes one wave of tavb_search_scoped_wide builds (default 64 MiB, >= 1; one query tile's
 *                   planes are built whatever this says: tests set it to 1 to split a small batch into waves)
 *   "scope_tile"    scoped batches, one mask per query (the binding reads it; the rule is tavb_plan_scoped, with "mask_tile_min_bytes" /
 *                   "mask_tile_pct"): 1 (default) = the 32/64-query tile (tavb_search_scoped_tile) where tavb_plan_scoped says so, else the
 *                   row-list route (tavb_search_scoped_batch); 0 = never; 2 = wherever the tile serves the shape (tests, measurements)
 *   "mask_wide"     masked batches on fp16 corpora (the binding reads it; the rule is tavb_plan_masked_wide, with "mask_tile_min_bytes" / "mask_tile_pct"):
 *                   1 (default) = a batch takes the 128/256-query filter tile with the bit test in its admission path + exact rescoring
 *                   (tavb_search_masked_wide) where tavb_plan_masked_wide says so -- it then wins over "mask_tile"; 0 = never; 2 = wherever that route
 *                   serves the shape (tests).  It never changes what "mask_tile" does for the batches this route does not take.
 *                   "last_flagged" after such a lookup: its queries that were re-run on the gather route
 *   "sort_small_keys" 0 .. 16384 (default 16384): a sort of up to this many keys (tavb_search_sorted, tavb_sort_keys_device) runs in ONE
 *                   workgroup in LDS; bigger ones take the multi-pass radix sort (3 launches per 8-bit digit that is not the same for
 *                   every key, + 2)
 *   "compact_pass_rows" 0 .. 2^31 - 2 (default 0 = auto: about 64 MiB of rows): rows per pass of an in-place tavb_compact_rows or tavb_expand_rows,
 *                   rounded up to a multiple of 64; their staging workspace holds one pass
 *   "rows_query"    (default 1; the binding reads it) 1 = fuzzy_lookup_rows / near_duplicate_pairs of a single-GPU index are calls of
 *                   tavb_search_rows / tavb_search_rows_sorted; 0 = the binding takes its host route (the rows to the host, widened to float32,
 *                   back as a query batch of max_hits + 1, the own row taken out by hand) -- for A/B runs in one process
 *   "rows_query_wave"  1 .. 2^20 (default 4096): most rows one wave of tavb_search_rows gathers and looks up; the float32 query batch of a
 *                   wave is rows_query_wave x dim x 4 bytes whatever n is (tests set it small to split a small call into waves)
 *   "rows_query_launches"  (read only) gather launches (= waves) of the last tavb_search_rows / _device / _sorted / tavb_gather_rows_f32 call; 0
 *                   before the first and after any tavb_search_batch, tavb_search_topk or tavb_search_sorted (what the host route calls)
 *   "pairs_join"    (default 1; the binding reads it) 1 = similarity_join / near_duplicate_pairs of a single-GPU index are calls of tavb_join_pairs
 *                   where tavb_plan_pairs_join says so; 0 = the binding keeps the row lookups (tavb_search_rows) -- for A/B runs in one process
 *   "pairs_join_min_rows"  1 .. 2^31 - 2 (default 8192, PROVISIONAL: not measured yet, tools/pairs_join_sweep.py): fewest rows
 *                   tavb_plan_pairs_join sends to the join (tests set it to 1)
 *   "pairs_join_capacity"  1 .. 2^30 (default 2^22): candidate pairs the binding reserves for a call of tavb_join_pairs (20 bytes each)
 *   "pairs_join_max_capacity"  1 .. 2^30 (default 2^25): the most the binding's ONE retry of a call that did not fit may reserve; a call
 *                   that needs more keeps the row lookups
 *   "pairs_join_launches"  (read only) join launches of the last tavb_join_pairs call (1, or 0 when it refused or had nothing to do); 0 after any
 *                   tavb_search_rows / tavb_search_batch / tavb_search_topk / tavb_search_sorted (what the other route calls)
 *   "pairs_join_candidates"  (read only) candidate pairs the last join launch counted (more than the call's capacity: it did not fit)
 */
int tavb_set_option(tavb_ctx* ctx, const char* name, int64_t value);
int tavb_get_option(tavb_ctx* ctx, const char* name, int64_t* out_value);

/* ---- corpus ----------------------------------------------------------------- */
/* Borrow a row-major [rows, dim] matrix in device memory as the corpus
 * (replaces the host ndarray `VectorBase._vectors`, vectorbase.py:84, 176).
 * dtype TAVB_F32 (the reference's layout) or TAVB_F16 (our storage extension: the
 * values the kernels see are the fp16 values widened to f32).  `ordinal_base` is
 * added to every returned ordinal (row-sharded corpora: the shard's first row). */
int tavb_set_corpus(tavb_ctx* ctx, const void* dev_rows, int64_t rows, int32_t dim, int32_t dtype,
                    int64_t ordinal_base);

/* Load path (what knowpro/serialization.py:207-221 and the BLOB reload loops of
 * storage/sqlite/messageindex.py:33-45 / reltermsindex.py:144-156 feed): float32 host rows [n_rows, dim] -> device
 * memory at dev_dst (inside the caller's capacity-doubling corpus buffer) as dst_dtype.  The rows go through two pinned
 * 16 MiB staging slots (filled by a few host threads) and asynchronous copies, so the host-side copy of chunk i+1 overlaps
 * the DMA of chunk i; for TAVB_F16 the conversion (round to nearest even) runs on the device from a scratch slot, the
 * host never builds an fp16 (or a second fp32) copy.  Returns when the rows are in place. */
int tavb_upload_rows(tavb_ctx* ctx, const float* rows_host, int64_t n_rows, int32_t dim, void* dev_dst, int32_t dst_dtype);

/* Tell the library that rows [first_row, rows) of the borrowed corpus buffer were rewritten in place (e.g. an append into
 * spare capacity followed by tavb_set_corpus with the new row count, or a re-upload after the host matrix was edited):
 * per-corpus quantities it caches (the row-norm maxima of the batched path's exactness proof; the fp16 shadow copy of an
 * fp32 corpus, see "f32_shadow") are refreshed on the next lookup.  tavb_set_corpus with a different pointer / shape /
 * dtype implies it; the caches are keyed on the ADDRESS, so a new buffer that happens to sit where a freed one lived needs
 * tavb_corpus_modified(ctx, 0) (the Python binding does that whenever it is handed a different tensor object). */
int tavb_corpus_modified(tavb_ctx* ctx, int64_t first_row);

/* K1: rows / ||row||_2 in float32, zero rows unchanged
 * (model_adapters.py:181-183; tools/benchmark_vectorbase.py:85-86).  in == out allowed. */
int tavb_normalize_rows_f32(tavb_ctx* ctx, const float* dev_in, float* dev_out, int64_t rows, int32_t dim);

/* float32 -> float16 (round to nearest even), used to build f16 corpora on device. */
int tavb_convert_f32_to_f16(tavb_ctx* ctx, const float* dev_in, void* dev_out, int64_t count);

/* A packed result key: (float32 score bits << 32) | (0xFFFFFFFF - ordinal); 0 = empty
 * slot.  Bigger key = better hit, so per-shard lists merge with integer compares. */
typedef uint64_t tavb_key;
/* Not a result: what a rank whose local search FAILED contributes to the all-gather of tavb_search_allgather, in every slot of its lists.  All
 * bits set sorts above every real key (scores are in [0, 1]), so it leads every merged list on every rank: no rank can mistake a result that
 * is missing a shard for an answer.  tavb_decode_keys returns TAVB_E_PEER for lists that carry it. */
#define TAVB_KEY_PEER_FAILED (~(tavb_key)0)

/* ---- synchronous lookups (host in, host out) ---------------------------------- */
/* fuzzy_lookup_embedding without predicate (vectorbase.py:163-190):
 * up to k best rows with score >= min_score.  out_* hold k entries; *out_count = M. */
int tavb_search(tavb_ctx* ctx, const float* query_host, int32_t k, float min_score, int64_t* out_ordinals,
                float* out_scores, int32_t* out_count);

/* fuzzy_lookup_embedding_in_subset (vectorbase.py:203-230).  `rows_host[i]` is the
 * (already wrapped, range-checked) corpus row of subset position i; the call returns
 * POSITIONS into the subset list (the wrapper maps them back through the caller's
 * list, reproducing `subset[indices[i]]`, :229).  Ties: ascending position. */
int tavb_search_subset(tavb_ctx* ctx, const float* query_host, const int64_t* rows_host, int64_t n_subset,
                       int32_t k, float min_score, int64_t* out_positions, float* out_scores,
                       int32_t* out_count);

/* Q independent lookups in one submission (the batching the reference leaves as a TODO,
 * storage/sqlite/reltermsindex.py:259-271).  Semantics == Q calls of tavb_search.
 * queries_host: float32 [nq, dim].  min_scores: nq thresholds -- one per query, as Q calls of the reference have Q `min_score`
 * arguments (vectorbase.py:163-173); a mixed batch runs on the same kernels as a uniform one.  Outputs [nq, k] / [nq]. */
int tavb_search_batch(tavb_ctx* ctx, const float* queries_host, int32_t nq, int32_t k, const float* min_scores,
                      int64_t* out_ordinals, float* out_scores, int32_t* out_counts);

/* ---- message re-rank on the device (the step right after the lookup in both providers) -------- */
/* Chunk row -> message ordinal map of the corpus: device int32 [rows], borrowed like the corpus (-1 = the row belongs to
 * no message).  n_messages bounds the ordinals (size of the accept bitmap). */
int tavb_set_row_messages(tavb_ctx* ctx, const int32_t* dev_row_to_msg, int64_t rows, int64_t n_messages);

/* SqliteMessageTextIndex.lookup_by_embedding / lookup_in_subset_by_embedding (storage/sqlite/messageindex.py:296-326,
 * 182-257) in one submission: the best k chunk rows with score >= min_score over the WHOLE corpus, THEN the
 * set-membership filter on their message ordinals (accept_msgs_host: n_accept ordinals, the provider's
 * `ordinals_set`; n_accept = -1: no filter), THEN the best score per message, sorted by score (stable: ties keep hit
 * order), cut at max_messages -- the provider's order of operations, so it returns exactly what the provider returns
 * (possibly fewer than max_messages).  out_* hold k entries. */
int tavb_search_messages(tavb_ctx* ctx, const float* query_host, int32_t k, float min_score, const int32_t* accept_msgs_host, int64_t n_accept,
                         int32_t max_messages, int64_t* out_messages, float* out_scores, int32_t* out_count);

/* The in-memory provider's form (storage/memory/messageindex.py:173-207 via knowpro/textlocindex.py:164-177): a true
 * subset gather (rows_host: corpus row per subset position, as tavb_search_subset), then the same aggregation. */
int tavb_search_messages_subset(tavb_ctx* ctx, const float* query_host, const int64_t* rows_host, int64_t n_subset, int32_t k, float min_score,
                                int32_t max_messages, int64_t* out_messages, float* out_scores, int32_t* out_count);

/* Split form of tavb_search_batch for a caller that drives SEVERAL contexts (one per GPU, row shards of one corpus) from
 * one thread: tavb_search_begin copies the queries and enqueues the kernels on the context's stream, tavb_search_end
 * waits for them and returns nq sorted lists of k keys.  Keys carry ordinal_base + row (must stay below 2^32 - 1), so the
 * lists of the shards merge with tavb_merge_keys_host (lists [n_lists, nq, k] -> out [nq, k]; a pure host helper) and
 * decode with tavb_decode_keys.  `cursor` (optional, nq == 1): only hits strictly AFTER that key in the result order,
 * i.e. the paging cursor of tavb_search_after as a key -- the same key on every shard. */
int tavb_search_begin(tavb_ctx* ctx, const float* queries_host, int32_t nq, int32_t k, const float* min_scores, const tavb_key* cursor);
int tavb_search_end(tavb_ctx* ctx, int32_t nq, int32_t k, tavb_key* out_keys_host);
int tavb_merge_keys_host(const tavb_key* lists, int32_t n_lists, int32_t nq, int32_t k, tavb_key* out);
/* tavb_merge_keys_host for lists of any length up to TAVB_MAX_LARGE_K (the lists of tavb_search_topk_device, one per shard): n_lists
 * (1 .. 64) sorted, zero-padded lists per query, [n_lists, nq, k] -> out [nq, k], the best k of their union, sorted and zero-padded.  Real
 * keys must be unique (they carry global ordinals or positions).  A query one of whose lists leads with TAVB_KEY_PEER_FAILED comes back as
 * that key in every slot.  A pure host helper: no context, no GPU. */
int tavb_merge_topk_host(const tavb_key* lists, int32_t n_lists, int32_t nq, int32_t k, tavb_key* out);
/* tavb_merge_topk_host for lists whose keys carry MESSAGE ordinals (the lists of tavb_search_top_messages_device, one per shard): a message
 * whose chunks lie on several shards stands in several lists, with several scores, so the keys are NOT unique in their low half.  n_lists
 * (1 .. 64) sorted, zero-padded lists per query, [n_lists, nq, k], 1 <= k <= TAVB_MAX_LARGE_K -> out [nq, k]: per message its largest key,
 * the best min(k, distinct messages) of those, sorted descending and zero-padded.  With every shard's own top k as input this is the
 * whole-corpus answer of tavb_search_top_messages: a message of the global top k is in the top k of the shard that holds its best row, with
 * that score.  A query one of whose lists leads with TAVB_KEY_PEER_FAILED comes back as that key in every slot.  A pure host helper: no
 * context, no GPU, no n_messages. */
int tavb_merge_top_messages_host(const tavb_key* lists, int32_t n_lists, int32_t nq, int32_t k, tavb_key* out);

/* Every row with score >= min_score in ONE pass -- the reference's `np.flatnonzero(scores >= min_score)`
 * (vectorbase.py:179, 219) -- sorted best first on the host; the first min(total, max_out) are returned, *out_total is the
 * number of survivors.  This is the candidate set of the predicate path (vectorbase.py:191-201), of max_hits >
 * TAVB_MAX_FUSED_K and of the max_hits == 0 quirk (`[-0:]`: all survivors, sorted).  Call with max_out = 0 to learn the
 * count first.  The subset form returns subset POSITIONS (like tavb_search_subset). */
int tavb_search_all(tavb_ctx* ctx, const float* query_host, float min_score, int64_t max_out, int64_t* out_ordinals, float* out_scores,
                    int64_t* out_count, int64_t* out_total);
int tavb_search_subset_all(tavb_ctx* ctx, const float* query_host, const int64_t* rows_host, int64_t n_subset, float min_score, int64_t max_out,
                           int64_t* out_positions, float* out_scores, int64_t* out_count, int64_t* out_total);

/* Exact top-k beyond the fused selection: TAVB_MAX_FUSED_K < k <= TAVB_MAX_LARGE_K (any k from 1 is accepted) after ONE corpus pass per
 * group of up to TAVB_MAX_STREAM_QUERIES queries -- the reference's argpartition + argsort (vectorbase.py:176-187) for the top-1000
 * candidates a re-ranker takes.  The pass is the streaming scan's arithmetic (scores equal tavb_search's bit for bit), writes one 4-byte
 * score per row and query and a histogram of the passing scores; a boundary search, its refinement, a compaction and a sort in LDS follow
 * on the device without a host round trip (tavb_topk.hip).  Device memory beyond the corpus: the score array of one group (options
 * "topk_scores_bytes", "topk_buckets", "topk_boundary_keys") and O(nq (k + boundary keys)).  Semantics, ordering, `ordinal_base`, outputs:
 * those of tavb_search_batch; any nq, one synchronise per call.  The subset form returns subset POSITIONS (like tavb_search_subset). */
int tavb_search_topk(tavb_ctx* ctx, const float* queries_host, int32_t nq, int32_t k, const float* min_scores, int64_t* out_ordinals, float* out_scores,
                     int32_t* out_counts);
int tavb_search_subset_topk(tavb_ctx* ctx, const float* query_host, const int64_t* rows_host, int64_t n_subset, int32_t k, float min_score,
                            int64_t* out_positions, float* out_scores, int32_t* out_count);

/* Every survivor (k = 0), or the best k for ANY k >= 1, sorted on the device: what tavb_search_all returns, bit for bit (ordinals,
 * float32 score bits, order), without the host sort -- the reference's `[-0:]` quirk (range search: "everything above 0.85") and
 * max_hits > TAVB_MAX_LARGE_K.  ONE corpus pass per group of up to TAVB_MAX_STREAM_QUERIES queries (the score pass of tavb_search_topk;
 * thresholds per query), then per query on the device: the boundary search and refinement of tavb_search_topk when k < the rows, a
 * compaction in position order, a stable radix sort on the score bits (tavb_sort.hip) and the decode into pinned memory, copied to
 * the caller in pieces of "sort_stage_keys".  Results are CONCATENATED in query order: query q's out_counts[q] results follow those of
 * queries < q; *out_total = their sum.  If that sum would pass max_total the call fails with TAVB_E_INVALID before it writes the
 * results of the group of queries that passes it (a caller sizing the arrays by nq x min(k or rows, rows) never sees this).  Device
 * memory beyond tavb_search_topk's: about 2 x 8 bytes per key of the biggest query.  Synchronous; a synchronise after each group's
 * score pass and per piece of results.  The subset form returns subset POSITIONS (like tavb_search_subset). */
int tavb_search_sorted(tavb_ctx* ctx, const float* queries_host, int32_t nq, int64_t k, const float* min_scores, int64_t max_total,
                       int64_t* out_ordinals, float* out_scores, int64_t* out_counts, int64_t* out_total);
int tavb_search_subset_sorted(tavb_ctx* ctx, const float* query_host, const int64_t* rows_host, int64_t n_subset, int64_t k, float min_score,
                              int64_t max_total, int64_t* out_positions, float* out_scores, int64_t* out_count);
/* The sort of tavb_search_sorted on its own: n (< 2^32) keys in device memory sorted in place, descending, on the context's stream;
 * returns after it finished.  Timed under TAVB_KERNEL_TOPK. */
int tavb_sort_keys_device(tavb_ctx* ctx, tavb_key* dev_keys, int64_t n);

/* Continuation ("cursor") forms: the next k hits strictly AFTER the hit
 * (after_score, after_ordinal) in the (score descending, ordinal ascending) order.
 * Feeding the last hit of one page as the cursor of the next enumerates every row
 * with score >= min_score, best first, k (<= TAVB_MAX_FUSED_K) at a time.  This is the
 * candidate stream of the predicate path (vectorbase.py:191-201), of max_hits >
 * TAVB_MAX_FUSED_K and of the max_hits == 0 quirk (all survivors, sorted).  For the
 * subset form the cursor is a subset POSITION.  Each page is one corpus pass. */
int tavb_search_after(tavb_ctx* ctx, const float* query_host, int32_t k, float min_score, float after_score,
                      int64_t after_ordinal, int64_t* out_ordinals, float* out_scores, int32_t* out_count);
int tavb_search_subset_after(tavb_ctx* ctx, const float* query_host, const int64_t* rows_host, int64_t n_subset,
                             int32_t k, float min_score, float after_score, int64_t after_position,
                             int64_t* out_positions, float* out_scores, int32_t* out_count);


/* ---- asynchronous device-resident lookups (sharding, benchmarking) -------------- */
/* Queries already on the device (float32 [nq, dim]); writes nq sorted lists of k keys to
 * dev_out_keys [nq, k] on the context's stream and returns without synchronising.
 * Keys carry ordinal_base + row (must stay below 2^32 - 1).
 *
 * PRECONDITION on the queries of EVERY *_device entry point that can take an MFMA tile route (tavb_search_device, tavb_search_allgather,
 * tavb_search_masked_device, tavb_search_masked_wide_device, tavb_search_scoped_tile_device, tavb_search_scoped_wide_device,
 * tavb_search_top_messages_tile_device): every element must round to a FINITE fp16 value, i.e. be finite with magnitude < 65520.  The
 * tiles see a query through fp16 planes; an element beyond that becomes an infinity there and that query's answer is unspecified (rows
 * may be missing).  The library never sees device-resident queries on the host and does not check this.  The host-synchronous entry
 * points (queries_host) do check, while they stage the queries, and run a batch that holds such an element -- or +-inf / NaN -- on the
 * streaming kernels: their answers are the fp32 answers for every query.  The *_device forms that only run the streaming kernels
 * (tavb_search_topk_device, tavb_search_subset_batch_device, tavb_search_scoped_device, tavb_search_top_messages_device) multiply fp32
 * queries and have no such precondition. */
int tavb_search_device(tavb_ctx* ctx, const float* dev_queries, int32_t nq, int32_t k, float min_score,
                       tavb_key* dev_out_keys);

/* tavb_search_topk / tavb_search_subset_topk with the queries already on the device (float32 [nq, dim]) and nothing waited for: 1 <= k <=
 * TAVB_MAX_LARGE_K, min_scores: nq thresholds on the HOST (read before the call returns), out_keys [nq, k]: sorted, zero-padded lists in
 * device memory or device-writable pinned memory, written on the context's stream.  dev_rows == NULL (n_subset 0): the whole corpus, keys
 * carry ordinal_base + row (ordinal_base + rows must stay below 2^32 - 1, as for tavb_search_device).  dev_rows: device int32 [n_subset],
 * wrapped and range-checked by the caller, with nq == 1: the subset form, keys carry subset POSITIONS.  An empty corpus or subset gives
 * empty lists.  "last_topk_refine" is valid after the next tavb_synchronize. */
int tavb_search_topk_device(tavb_ctx* ctx, const float* dev_queries, int32_t nq, int32_t k, const float* min_scores, const int32_t* dev_rows,
                            int64_t n_subset, tavb_key* out_keys);

/* Subset form of tavb_search_device: one query (device, float32 [dim]) against the rows listed in
 * dev_rows (device int32 [n_subset], already wrapped / range-checked by the caller); keys carry
 * subset POSITIONS.  Asynchronous.  Used by the fused multi-index submission. */
int tavb_search_subset_device(tavb_ctx* ctx, const float* dev_query, const int32_t* dev_rows, int64_t n_subset,
                              int32_t k, float min_score, tavb_key* dev_out_keys);
/* Host-synchronous tavb_search_subset (vectorbase.py:203-230) over a subset whose row list is ALREADY on the device: callers that search the
 * same subset again and again (the memory provider hands `lookup_in_subset_by_embedding` the same scope list per query term,
 * storage/memory/messageindex.py:173-183; tools/benchmark_vectorbase.py:133-163 passes one list for every round) upload and range-check it
 * once.  query_host float32 [dim]; dev_rows device int32 [n_subset], wrapped and range-checked by the caller; positions / scores / count as
 * tavb_search_subset.  A subset of up to "small_direct_bytes" of rows is ONE launch (per-workgroup lists into pinned memory, merged on the host;
 * a 1536-wide query rides in the kernel arguments), like tavb_search on small corpora: 21 us against 28 for the 1000-of-10k case. */
int tavb_search_subset_resident(tavb_ctx* ctx, const float* query_host, const int32_t* dev_rows, int64_t n_subset, int32_t k, float min_score,
                                int64_t* out_positions, float* out_scores, int32_t* out_count);

/* ---- row masks: "search only among the rows I allow" ---------------------------------------------------------------------
 * An allow-mask is one bit per corpus row in device memory, held as uint32 words: row r is bit (r & 31) of word (r >> 5), `rows` valid
 * bits, (rows + 31) / 32 words; bits at or beyond `rows` in the last word may hold anything and are ignored.  A time range or a thread
 * scope over 10M rows is 1.25 MB as a mask against 40 - 80 MB as ordinals, and a mask computed on the device never visits the host.
 *
 * tavb_mask_expand: the set rows in ASCENDING order -> dev_rows_out (device int32 [cap]), their number -> *out_count (host).  Ascending
 * rows keep "equal scores order by ascending ordinal" when the list is searched (keys carry list positions), and are what
 * np.flatnonzero gives.  Two launches on the context's stream (a popcount per chunk of TAVB_MASK_ROWS_PER_WORKGROUP rows; a write pass
 * in which every workgroup starts at the sum of the counts before it -- no atomics on the output order, nothing read back in between),
 * then ONE synchronise.  cap < count: TAVB_E_INVALID, *out_count is still the count and nothing is written at or beyond dev_rows_out
 * [cap]; dev_rows_out == NULL with cap == 0 asks for the count alone (the write pass then only sums the counts) and is no error.  rows == 0: count 0, no launch.
 * tavb_mask_pack: device bytes [rows] (non-zero = allowed; the storage of a torch.bool tensor) -> the bit form at dev_bits_out
 * ((rows + 31) / 32 words, tail bits zero).  Asynchronous on the context's stream. */
int tavb_mask_expand(tavb_ctx* ctx, const uint32_t* dev_bits, int64_t rows, int32_t* dev_rows_out, int64_t cap, int64_t* out_count);
int tavb_mask_pack(tavb_ctx* ctx, const uint8_t* dev_bytes, int64_t rows, uint32_t* dev_bits_out);

/* tavb_search_subset_resident for nq queries over ONE resident row list (the output of tavb_mask_expand, or any wrapped, range-checked
 * device int32 [n_subset]): what nq calls of tavb_search_subset_resident (k <= TAVB_MAX_FUSED_K) or tavb_search_subset_topk (up to
 * TAVB_MAX_LARGE_K) return, bit for bit, in one submission -- a consumer with T scope-restricted term lookups
 * (storage/memory/messageindex.py:173-183) makes one call instead of T.  queries_host float32 [nq, dim]; min_scores [nq]; the
 * queries go over the list in groups of at most TAVB_MAX_STREAM_QUERIES per pass (4 for 64 < k <= TAVB_MAX_FUSED_K, as everywhere).
 * remap = 0: out holds POSITIONS into dev_rows (like tavb_search_subset).  remap = 1: the keys' positions are turned into corpus rows on
 * the device (dev_rows[position]) before they come back and `ordinal_base` is added at decode: out holds corpus ORDINALS and the caller
 * needs no host copy of the list; dev_rows must then be ascending for equal scores to stay in ascending-ordinal order.  Outputs
 * [nq, k] / [nq] as tavb_search_batch.  n_subset == 0, nq == 0 or an empty corpus: zero counts, nothing launched.  One synchronise. */
int tavb_search_subset_batch_resident(tavb_ctx* ctx, const float* queries_host, int32_t nq, const int32_t* dev_rows, int64_t n_subset, int32_t k,
                                      const float* min_scores, int32_t remap, int64_t* out, float* out_scores, int32_t* out_counts);

/* The no-wait twin of tavb_search_subset_batch_resident (what tavb_search_topk_device is to tavb_search_topk): dev_queries device float32
 * [nq, dim], nq >= 1 queries over ONE resident row list -- tavb_search_topk_device takes a row list with one query only -- 1 <= k <=
 * TAVB_MAX_LARGE_K: the same passes (the fused selection up to TAVB_MAX_FUSED_K, the exact top-k beyond; "last_topk_refine" is then valid
 * after the next tavb_synchronize), so the keys are those of the host-synchronous call bit for bit.  min_scores: nq thresholds on the HOST,
 * read before the call returns.  out_keys [nq, k]: sorted, zero-padded lists in device memory or device-writable pinned memory, written on
 * the context's stream; nothing is waited for.  remap = 0: keys carry POSITIONS into dev_rows.  remap = 1: keys carry GLOBAL ordinals,
 * ordinal_base + dev_rows[position] -- the form every key merge takes (tavb_merge_keys_host, tavb_merge_topk_host, tavb_merge_device,
 * tavb_merge_topk_device, tavb_allgather_merge, tavb_allgather_merge_topk): a shard of a device group or a rank of a row-sharded index
 * searches ITS slice of a row mask and hands the lists on as they are; ordinal_base + rows must stay below 2^32 - 1 (TAVB_E_UNSUPPORTED
 * otherwise), and dev_rows must be ascending for equal scores to stay in ascending-ordinal order.  n_subset == 0 (dev_rows may then be
 * NULL) or an empty corpus: all-zero keys are enqueued, no error. */
int tavb_search_subset_batch_device(tavb_ctx* ctx, const float* dev_queries, int32_t nq, const int32_t* dev_rows, int64_t n_subset, int32_t k,
                                    const float* min_scores, int32_t remap, tavb_key* out_keys);

/* A masked batch on the 32/64-query MFMA tile: nq queries over the rows an allow-mask names, the corpus read ONCE per 64 queries with the bit
 * test in the tile's admission path, instead of the allowed rows gathered once per TAVB_MAX_STREAM_QUERIES queries -- the route for a DENSE mask
 * under a real batch (a time range, a thread scope).  dev_bits: the mask over the whole corpus in the bit form above, `rows` == the corpus' rows;
 * [first_row, last_row] must contain every set bit (0, rows - 1 is always valid): the tile scans rows [first_row rounded down to a multiple of
 * 256, last_row] only, so a contiguous range costs its own bytes.  Serves 1 <= k <= 64 and rows of a multiple of 64 bytes; anything else returns
 * TAVB_E_UNSUPPORTED and the caller keeps the gather route (tavb_search_subset_batch_resident / _device over tavb_mask_expand's list).  The
 * corpus' own rows are multiplied -- fp32 x fp32, or the fp32 queries as split fp16 planes x fp16 rows, as on the unmasked tile route; no
 * shadow -- and the scores are final.  Outputs and ordering: tavb_search_batch / tavb_search_device (min_scores: nq thresholds on the HOST;
 * the device form's keys carry ordinal_base + row and nothing is waited for).  Against the gather route the answers agree the way the tile
 * agrees with the streaming kernels everywhere: the same ordinals except among float32 near-ties, scores within 1e-5 -- not bit for bit.  An
 * empty corpus, nq == 0 or first_row > last_row: zero counts / zero keys, no tile launch. */
int tavb_search_masked_batch(tavb_ctx* ctx, const float* queries_host, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row,
                             int64_t last_row, int32_t k, const float* min_scores, int64_t* out_ordinals, float* out_scores, int32_t* out_counts);
int tavb_search_masked_device(tavb_ctx* ctx, const float* dev_queries, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row,
                              int64_t last_row, int32_t k, const float* min_scores /*host*/, tavb_key* out_keys);

/* A masked batch on the 128/256-query filter tile + exact rescoring -- the route every large unmasked batch on an fp16 corpus takes, with the
 * mask's bit tested in the filter's admission path: the mask's span is read once per 128 or 256 queries.  dev_bits (4-byte aligned), rows,
 * [first_row, last_row]: as for tavb_search_masked_batch.  dev_rows / n_allowed: the mask's resident row list (tavb_mask_expand: the set rows in
 * ascending order, device memory) -- a query whose band of candidates does not provably fit (more near-duplicates around its k-th best than
 * option "band_max" holds: rare) is re-run over it on the gather route; the list of such queries is read back, so BOTH forms synchronise the
 * stream once per call ("last_flagged" counts them).  Serves fp16 corpora of any width up to 16384 and 1 <= k <= TAVB_MAX_FUSED_K; an fp32
 * corpus and any other k return TAVB_E_UNSUPPORTED.  The filter multiplies fp16-rounded queries (an odd width: over a zero-padded copy of the
 * rows), every candidate is scored again with the fp32 queries in the streaming kernels' arithmetic: ordinals, float32 scores and counts EQUAL
 * those of the gather route (tavb_search_subset_batch_resident over dev_rows, remap = 1) bit for bit.  Outputs and ordering as
 * tavb_search_masked_batch / tavb_search_masked_device (min_scores: nq thresholds on the HOST; the device form's keys carry ordinal_base + row).
 * An empty corpus, nq == 0, first_row > last_row or n_allowed == 0: zero counts / zero keys, no tile launch. */
int tavb_search_masked_wide(tavb_ctx* ctx, const float* queries_host, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row,
                            int64_t last_row, const int32_t* dev_rows, int64_t n_allowed, int32_t k, const float* min_scores, int64_t* out_ordinals,
                            float* out_scores, int32_t* out_counts);
int tavb_search_masked_wide_device(tavb_ctx* ctx, const float* dev_queries, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row,
                                   int64_t last_row, const int32_t* dev_rows, int64_t n_allowed, int32_t k, const float* min_scores /*host*/,
                                   tavb_key* out_keys);

/* ---- scoped message lookups: a scope of MESSAGE ordinals searched as a row mask, batches of queries aggregated to messages ----------------
 * tavb_mask_from_messages: the row mask of a set of messages, built on the device from the context's row -> message map
 * (tavb_set_row_messages) -- the scope never becomes a host row list.  accept_msgs_host [n_accept] (n_accept >= 0): the accepted message
 * ordinals; duplicates are harmless, ordinals below 0 or at or beyond n_messages are ignored.  dev_bits_out [(rows + 31) / 32] words in the bit
 * form above, rows == the corpus' rows: row r is set when 0 <= map[r] < n_messages and message map[r] is accepted -- rows mapped to -1 are
 * never allowed -- and the bits at or beyond `rows` in the last word are ZERO (whole words compare equal to a host-packed mask).  Fails as
 * tavb_search_messages does without a map (TAVB_E_NO_CORPUS) or with a map shorter than the corpus (TAVB_E_INVALID).  The accepted ordinals
 * are copied to the device and turned into the accept bitmap there, then ONE launch (a wave takes 64 rows, its ballot is two words; no
 * atomics on the mask) writes the words.  Asynchronous on the context's stream; the result feeds tavb_mask_expand and the masked lookups.
 * Timed under TAVB_KERNEL_CONVERT.
 *
 * tavb_search_messages_masked: nq queries over the rows a mask names, aggregated to messages, in ONE submission: the masked batch on the
 * route the caller names -- route 1 = the row list (dev_rows / n_allowed: tavb_search_subset_batch_resident's passes), 2 = the 32/64-query
 * tile (tavb_search_masked_batch's; dev_rows may be NULL), 3 = the 128/256-query filter tile + rescoring (tavb_search_masked_wide's) --
 * leaves [nq, k] key lists carrying ordinal_base + row on the device; one launch of the message re-rank with nq workgroups turns each into
 * the accepted first occurrence of every message in hit order, cut at max_messages (rows without a message are skipped); one device-to-host
 * copy brings the [nq, k] message keys back.  Per query this is tavb_search_messages_subset over the mask's rows: bit for bit on routes 1
 * and 3, and on route 2 up to what the 32/64-query tile differs from the streaming kernels by (float32 near-ties, scores within 1e-5).
 * 1 <= k <= TAVB_MAX_FUSED_K.  The arguments of the route are checked as that route's own entry point checks them, and a shape it does
 * not serve returns TAVB_E_UNSUPPORTED: the caller (the binding's planners, tavb_plan_masked / tavb_plan_masked_wide) picks another.
 * min_scores: nq thresholds on the host.  out_messages / out_scores [nq, k], out_counts [nq].  "masked_route" reports the route.  The
 * re-rank is timed under TAVB_KERNEL_MERGE.
 *
 * tavb_search_messages_batch: tavb_search_messages for nq queries in one submission: the full-corpus top-k of every query by the route any
 * device-resident batch takes, THEN the optional accept filter (n_accept = -1: none; >= 0: that set, as tavb_search_messages), THEN the
 * re-rank of all nq lists in one launch, one copy back.  Per query it equals tavb_search_messages wherever the batch route is bit-exact
 * against the streaming kernels (the grouped streaming scan, the wide tile + rescoring); on the 32/64-query tile up to near-ties. */
int tavb_mask_from_messages(tavb_ctx* ctx, const int32_t* accept_msgs_host, int64_t n_accept, int64_t rows, uint32_t* dev_bits_out);
int tavb_search_messages_masked(tavb_ctx* ctx, const float* queries_host, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row,
                                int64_t last_row, const int32_t* dev_rows, int64_t n_allowed, int32_t k, const float* min_scores,
                                int32_t max_messages, int32_t route, int64_t* out_messages, float* out_scores, int32_t* out_counts);
int tavb_search_messages_batch(tavb_ctx* ctx, const float* queries_host, int32_t nq, int32_t k, const float* min_scores,
                               const int32_t* accept_msgs_host, int64_t n_accept, int32_t max_messages, int64_t* out_messages, float* out_scores,
                               int32_t* out_counts);

/* ---- scope algebra: masks from ranges, and AND / OR / NOT of masks, on the device ------------------------------------------------------
 * Both calls write a mask in the bit form above -- every word of (rows + 31) / 32, the bits at or beyond `rows` ZERO -- and, in the same
 * launch, the per-chunk popcounts tavb_mask_expand's count pass would write and every chunk's count, first and last set row (pinned host
 * memory, summed on the host after the call's one synchronise) -> *out_info: the mask's count and span (an empty mask: 0, 0, -1).
 * rows == the corpus' rows.  dev_rows_out / cap as for tavb_mask_expand: NULL with cap == 0 asks for the mask and its info only (ONE
 * launch); otherwise the write pass of tavb_mask_expand follows on the counts already made (TWO launches) and leaves the set rows in
 * ascending order in dev_rows_out [0, count); cap < count returns TAVB_E_INVALID with *out_info filled and nothing written at or beyond
 * cap.  rows == 0: empty info, nothing launched.  Each call synchronises the context's stream once.  No atomics on mask words.  Timed under
 * TAVB_KERNEL_CONVERT.
 *
 * tavb_mask_from_ranges: the mask of a scope given as n_collections (0 .. TAVB_MAX_SCOPE_COLLECTIONS) collections of half-open integer
 * ranges [start, end): ranges_host [total][2] holds the collections one after another, collection_sizes_host [n_collections] their
 * lengths (total = their sum, at most 2^20).  domain 0 = rows: x = r; domain 1 = messages: x = map[r], the context's row -> message map
 * (tavb_set_row_messages) -- a row whose map value is below 0 or at or beyond n_messages is never allowed, and the call fails as
 * tavb_mask_from_messages does without a map or with one shorter than the corpus.  Row r is set when, for EVERY collection, x lies in one
 * of its ranges: zero collections allow everything the domain can name, a collection with no non-empty range allows nothing.  Ranges may
 * be unsorted, overlapping, duplicated or empty (start >= end) and may reach below 0 or beyond the domain: each collection is sorted,
 * clipped and merged into disjoint ascending intervals on the host, copied to the device (8 bytes per interval), and the kernel does one
 * binary search per collection and row -- in LDS when at most TAVB_SCOPE_LDS_RANGES intervals are left, else in device memory.
 *
 * tavb_mask_combine: dev_bits_out = op(m0 .. m(n-1)) word by word for 1 <= n_masks <= TAVB_MAX_MASK_OPERANDS masks of `rows` rows
 * (dev_masks: a HOST array of n_masks device pointers): TAVB_MASK_AND, TAVB_MASK_OR, or TAVB_MASK_ANDNOT = m0 & ~(m1 | ..) -- with one
 * operand the complement of m0.  Input bits at or beyond `rows` are ignored (they may hold anything).  dev_bits_out may be any of the
 * operands: a thread reads its word of every operand before it writes it. */
typedef struct {
  int64_t count, first_row, last_row; /* an empty mask: 0, 0, -1 */
} tavb_mask_info;
int tavb_mask_from_ranges(tavb_ctx* ctx, const int64_t* ranges_host, const int32_t* collection_sizes_host, int32_t n_collections, int32_t domain,
                          int64_t rows, uint32_t* dev_bits_out, int32_t* dev_rows_out, int64_t cap, tavb_mask_info* out_info);
int tavb_mask_combine(tavb_ctx* ctx, int32_t op, const uint32_t* const* dev_masks, int32_t n_masks, int64_t rows, uint32_t* dev_bits_out,
                      int32_t* dev_rows_out, int64_t cap, tavb_mask_info* out_info);

/* ---- masks carried through a row edit: np.delete / np.insert of packed masks under the edit's packed flags, on the device ------------------
 * tavb_mask_remap pushes 1 <= n_masks <= TAVB_MAX_MASK_OPERANDS masks in the bit form above through ONE edit of the row space, in one
 * submission on the context's stream.  dev_masks / dev_bits_out: HOST arrays of n_masks device pointers (tavb_mask_combine's convention);
 * mask j is read from dev_masks[j] over old_rows rows and written to dev_bits_out[j] over new_rows rows.
 *   TAVB_REMAP_REMOVE  dev_flags covers old_rows, a SET bit means the row goes (tavb_compact_rows' mask).  The kept rows are numbered
 *                      k = 0, 1, .. in ascending order and output bit k is the input bit of the k-th kept row.  new_rows must equal the
 *                      number of clear flag bits below old_rows, else TAVB_E_INVALID.
 *   TAVB_REMAP_INSERT  dev_flags covers new_rows, a SET bit means a hole (tavb_expand_rows' mask).  Output bit p is `fill` (0 or non-zero)
 *                      where flag p is set, else input bit p - popcount(flags[0, p)).  The clear bits must number old_rows, else
 *                      TAVB_E_INVALID.
 *   TAVB_REMAP_APPEND  no flags (dev_flags is ignored).  Output bits [0, old_rows) are the input's, bits [old_rows, new_rows) are `fill`.
 * The flags are counted and checked first (the call's first synchronise): a mismatch returns before any output is written.  Input bits at
 * or beyond old_rows are ignored (they may hold anything; with old_rows == 0 the input pointers may be NULL); every word of (new_rows +
 * 31) / 32 of every output is written, the bits at or beyond new_rows ZERO.  An output overlaps neither the flags nor any input nor
 * another output (TAVB_E_INVALID): the removal flags may be one of the carried masks, and tavb_compact_rows reads them afterwards.  The
 * masks need not be the corpus' length -- the call does not look at the corpus, so it may run before or after the edit itself.  new_rows
 * == 0 is legal: empty infos, nothing written.  The result is deterministic, and no workgroup waits for another: the popcount prefix over
 * the flags is the per-chunk counts of tavb_compact_rows' count pass, made once per call and shared by all masks, and a workgroup sums
 * the counts in front of its chunk itself.  A lane squeezes (REMOVE) or spreads (INSERT) its word of every mask under its flag word in
 * registers.  REMOVE: a workgroup owns a chunk of input words; a lane's piece straddles at most two output words, the pieces of a chunk
 * are assembled by OR in LDS and only the first and last word of a chunk's output -- the ones two chunks may share -- go through a
 * global atomic OR on zeroed output.  INSERT / APPEND: a workgroup owns a chunk of output words and gathers its source bits; plain stores.
 * Per output the call leaves what tavb_mask_combine leaves: out_info[j] = its count and span (an empty mask: 0, 0, -1), and the per-chunk
 * counts tavb_mask_expand's write pass needs -- so with dev_rows_out != NULL, dev_rows_out[j] != NULL and caps[j] > 0 the set rows of output
 * j follow in ascending order in dev_rows_out[j] [0, count) at the cost of ONE more launch; caps[j] bounds the count (REMOVE: at most the
 * input's count; INSERT / APPEND: exactly the input's count, plus the number of new rows when fill is set), a smaller one returns
 * TAVB_E_INVALID with out_info filled and nothing written at or beyond it.  Two synchronises in all; timed under TAVB_KERNEL_CONVERT. */
int tavb_mask_remap(tavb_ctx* ctx, int32_t mode, const uint32_t* dev_flags, int64_t old_rows, int64_t new_rows, const uint32_t* const* dev_masks,
                    uint32_t* const* dev_bits_out, int32_t n_masks, int32_t fill, int32_t* const* dev_rows_out, const int64_t* caps,
                    tavb_mask_info* out_info);

/* ---- scoped batches: one row mask PER QUERY in a single submission ----------------------------------------------------------------------
 * A compiled question is a handful of lookups, each under its own scope (a time range, a thread, a set of messages): query q searches the
 * rows dev_masks[q] names.  dev_masks: a HOST array of nq device pointers (tavb_mask_combine's convention) to packed masks in the bit form
 * above over `rows` == the corpus' rows, 4-byte aligned, none NULL; pointers may repeat; bits at or beyond `rows` are ignored.  Per query the
 * result is tavb_search_subset_batch_resident over that mask's row list (remap = 1), bit for bit: ordinals, float32 scores and counts.
 * 1 <= k <= TAVB_MAX_FUSED_K.  The queries go in passes of TAVB_MAX_STREAM_QUERIES (4 for 64 < k), as everywhere -- fewer where eight queries of
 * the corpus' width do not fit the vector tier's LDS (from about 4.7k floats per row on: 4, 2 or 1), so that a pass runs on the tier ONE query
 * of this corpus runs on and the bit-for-bit equality holds at every width; option "force_tier" = 3 sends both to the scalar tier (1 and 2 leave a scoped pass on this rule).  Per pass, on the device:
 * the OR of the pass' masks (tavb_mask_combine's kernel) and its ascending row list (tavb_mask_expand's write pass); one membership byte per
 * list position (bit j = the pass' query j holds the row; tavb_mask_membership's kernel); ONE streaming scan over the union list -- every
 * row of the union is read once per pass, however many scopes hold it -- in which a row is offered to a query only when its bit is set; the
 * merge; the remap of list positions to rows.  Equal scores keep ascending-ordinal order because the union list is ascending and the keys
 * carry list positions, as for tavb_mask_expand.  No mask word visits the host.  The passes go in WAVES of at most 16 (128 queries; fewer on
 * corpora beyond 4M rows: at most 64M union positions per wave, at least one pass): a wave's unions are enqueued first and ONE synchronise
 * reads their counts; everything else is enqueued behind it.  A batch of up to a wave therefore waits once for its counts, a longer one once per
 * wave.  Workspace, kept by the context: rows / 8 bytes per pass of a wave and 5 bytes per union position of a wave -- at most 2 x rows + 5 x
 * max(64M, rows) bytes however many queries.  "masked_route" reports 4.  Timed under TAVB_KERNEL_CONVERT (unions,
 * lists, membership), TAVB_KERNEL_SCAN and TAVB_KERNEL_MERGE (merge, remap, re-rank).
 *   tavb_search_scoped_batch: queries on the host, one more synchronise at the end; outputs [nq, k] / [nq] as tavb_search_batch (ordinals
 *     carry ordinal_base).
 *   tavb_search_scoped_device: dev_queries device float32 [nq, dim]; out_keys [nq, k] sorted, zero-padded keys carrying ordinal_base + row, in
 *     device memory or device-writable pinned memory; waits only for the unions' counts.  min_scores: nq thresholds on the HOST.
 *   tavb_search_messages_scoped: the batch, its keys left on the device, then tavb_search_messages_masked's re-rank launch for all queries
 *     and one copy back: per query tavb_search_messages_masked on route 1 over that mask.  Needs the row -> message map.
 * NULL arguments, rows != the corpus' rows, k outside 1 .. TAVB_MAX_FUSED_K and a NULL mask pointer are TAVB_E_INVALID with a message.  nq
 * == 0 or an empty corpus: zero counts / zero keys, nothing launched.  A query whose mask is empty gets an empty list.
 *
 * tavb_mask_membership: the membership bytes alone -- dev_member_out[p] (device uint8 [n]) = bit j set when dev_masks[j] (HOST array of 1 ..
 * TAVB_MAX_MASK_OPERANDS device pointers, masks over `rows` rows) holds row dev_rows[p] (device int32 [n], n <= rows; a value outside
 * [0, rows) gives 0).  One launch, asynchronous on the context's stream.  Timed under TAVB_KERNEL_CONVERT. */
int tavb_search_scoped_batch(tavb_ctx* ctx, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                             const float* min_scores, int64_t* out_ordinals, float* out_scores, int32_t* out_counts);
int tavb_search_scoped_device(tavb_ctx* ctx, const float* dev_queries, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                              const float* min_scores /*host*/, tavb_key* out_keys);
int tavb_search_messages_scoped(tavb_ctx* ctx, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                                const float* min_scores, int32_t max_messages, int64_t* out_messages, float* out_scores, int32_t* out_counts);
int tavb_mask_membership(tavb_ctx* ctx, const uint32_t* const* dev_masks, int32_t n_masks, int64_t rows, const int32_t* dev_rows, int64_t n,
                         uint8_t* dev_member_out);

/* ---- scoped and one-mask batches beyond TAVB_MAX_FUSED_K: the large-k and the sorted route under scopes ------------------------------------
 * The same dev_masks / rows convention as tavb_search_scoped_batch; per query the result is what the single-query call over that mask's row
 * list returns -- tavb_search_subset_topk / tavb_search_subset_sorted with the positions turned into corpus ordinals -- bit for bit:
 * ordinals, float32 scores and counts.  Waves and passes as above (one synchronise per wave for the unions' sizes), a pass being min(8,
 * the queries of one score pass) queries: eight bits of a membership byte.  Per pass, over the ascending row list of the union of its
 * scopes: tavb_search_topk's score pass in its scoped form -- a row's score is written and counted for query j only when bit j of the
 * row's membership byte is set, every other slot holds "no score" -- and then that route's own launches, unchanged: the histograms saw
 * members only, so a query's need is min(k, survivors of ITS scope).  Keys carry union-list positions (the list is ascending, so equal
 * scores leave by ascending row) and are turned into rows at the end.  "topk_scores_bytes" holds: where the score array of a whole pass
 * (queries x union rows x 4 bytes) would exceed it, the pass' queries go in sub-groups over the same list (at least one query each).
 *   tavb_search_scoped_topk: 1 <= k <= TAVB_MAX_LARGE_K.  Per pass: write pass, membership bytes, then per sub-group memset, score pass,
 *     refinement rounds, compaction, finish; one remap.  Queries on the host, one more synchronise at the end; outputs [nq, k] / [nq] as
 *     tavb_search_topk (ordinals carry ordinal_base).  "masked_route" reports 7, "last_topk_refine" the most rounds of any query.
 *   tavb_search_scoped_topk_device: dev_queries device float32 [nq, dim]; out_keys [nq, k] sorted, zero-padded keys carrying ordinal_base +
 *     row, device or device-writable pinned memory; waits only for the unions' sizes ("last_topk_refine" at the next tavb_synchronize).
 *   tavb_search_scoped_sorted: k = 0 (every survivor of the query's scope) or ANY k >= 1.  Per sub-group the sorted route's group
 *     (tavb_search_sorted): score pass, refinement only where k < the union's rows, counts, ONE synchronise, then per query compaction, sort
 *     and decode -- the decode reads the row list.  max_total, the concatenated out_ordinals / out_scores, out_counts [nq] and *out_total
 *     follow tavb_search_sorted; more than max_total results are TAVB_E_INVALID.  "masked_route" reports 8.
 *   tavb_search_subset_batch_sorted: the one-mask batch on the sorted route -- nq queries over ONE resident row list (dev_rows device int32
 *     [n_subset], valid corpus rows, e.g. tavb_mask_expand's), eight per pass; per query tavb_search_subset_sorted with out_ordinals =
 *     ordinal_base + dev_rows[position].  "masked_route" reports 1 (the gather route).
 * NULL arguments, rows != the corpus' rows, k out of range, max_total < 0 and a NULL mask pointer are TAVB_E_INVALID with a message.  nq == 0,
 * an empty corpus or subset: zero counts / zero keys, nothing launched.  A query whose mask is empty gets an empty list.  Timed under
 * TAVB_KERNEL_CONVERT (unions, lists, membership), TAVB_KERNEL_SCAN (score pass) and TAVB_KERNEL_TOPK (everything behind it). */
int tavb_search_scoped_topk(tavb_ctx* ctx, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                            const float* min_scores, int64_t* out_ordinals, float* out_scores, int32_t* out_counts);
int tavb_search_scoped_topk_device(tavb_ctx* ctx, const float* dev_queries, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                                   const float* min_scores /*host*/, tavb_key* out_keys);
int tavb_search_scoped_sorted(tavb_ctx* ctx, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t k,
                              const float* min_scores, int64_t max_total, int64_t* out_ordinals, float* out_scores, int64_t* out_counts,
                              int64_t* out_total);
int tavb_search_subset_batch_sorted(tavb_ctx* ctx, const float* queries_host, int32_t nq, const int32_t* dev_rows, int64_t n_subset, int64_t k,
                                    const float* min_scores, int64_t max_total, int64_t* out_ordinals, float* out_scores, int64_t* out_counts,
                                    int64_t* out_total);

/* ---- the best k MESSAGES: per-message best score and top-k on the device ("collapsing") ----------------------------------------------------
 * The message lookups above take the best k chunk ROWS and then collapse them to messages: possibly far fewer than k messages.  These calls
 * return, per query, the k messages with the highest best(m) = max score(r) over the rows r of message m (tavb_set_row_messages) that pass
 * score(r) >= min_score (NaN never passes) and, with dev_rows, are in that list -- min(k, messages with a passing row) of them, sorted by
 * best descending, ties by ascending message ordinal.  Rows whose map value is below 0 or at or beyond n_messages belong to no message.
 * Scores are tavb_search's float32 scores bit for bit.  1 <= k <= TAVB_MAX_LARGE_K; dev_rows == NULL (n_rows 0): the whole corpus; dev_rows:
 * device int32 [n_rows], valid corpus rows (e.g. tavb_mask_expand's list; order and repeats do not matter), any nq.
 * On the device, per group of up to TAVB_MAX_STREAM_QUERIES queries: ONE pass over the corpus or the list with the streaming scan's
 * arithmetic that writes nothing per row -- a passing row does one atomic max on its message's slot of a [queries][n_messages] array
 * (zeroed first; 4 bytes per query and message, cut to groups of at least one query by "topk_scores_bytes") -- then one pass over that
 * array that counts the messages into tavb_search_topk's histograms, then tavb_search_topk's boundary search, refinement, compaction and
 * sort with the message ordinals as positions ("topk_buckets", "topk_boundary_keys"; "last_topk_refine" reports the rounds).  A max does not
 * depend on the order of its operands: the result is deterministic.  No host round trip before the results.
 *   tavb_search_top_messages: queries on the host, one synchronise; out_messages / out_scores [nq, k], out_counts [nq] as tavb_search_batch,
 *     the ordinals being MESSAGE ordinals (no ordinal_base).
 *   tavb_search_top_messages_device: dev_queries device float32 [nq, dim], nq >= 1; out_keys [nq, k] sorted, zero-padded keys carrying message
 *     ordinals, device or device-writable pinned memory; nothing waited for ("last_topk_refine" at the next tavb_synchronize).
 * No map set: TAVB_E_NO_CORPUS; a map that does not cover exactly the corpus' rows, NULL arguments, k out of range, a bad row list length:
 * TAVB_E_INVALID; n_messages >= 2^31 - 1: TAVB_E_UNSUPPORTED -- each with a message.  nq == 0, an empty corpus, n_messages == 0 or an empty
 * list: zero counts / zero keys, nothing launched.  Timed under TAVB_KERNEL_SCAN (score pass) and TAVB_KERNEL_TOPK (everything behind it). */
int tavb_search_top_messages(tavb_ctx* ctx, const float* queries_host, int32_t nq, int32_t k, const float* min_scores, const int32_t* dev_rows,
                             int64_t n_rows, int64_t* out_messages, float* out_scores, int32_t* out_counts);
int tavb_search_top_messages_device(tavb_ctx* ctx, const float* dev_queries, int32_t nq, int32_t k, const float* min_scores /*host*/,
                                    const int32_t* dev_rows, int64_t n_rows, tavb_key* out_keys);

/* ---- the best k MESSAGES under one scope PER QUERY, in one submission ---------------------------------------------------------------------
 * tavb_search_top_messages takes one row list for the whole batch; these calls take one mask per query -- the lookups of one compiled
 * question, each under its own `when` filter.  Per query the result is tavb_search_top_messages' over that mask's row list
 * (tavb_mask_expand), bit for bit: message ordinals, float32 scores and counts.  dev_masks / rows follow tavb_search_scoped_batch (HOST array
 * of nq device pointers to packed masks over the corpus' rows, none NULL, 4-byte aligned, repeats allowed; rows = the corpus' rows), waves
 * and passes follow tavb_search_scoped_topk: one synchronise per wave for the unions' sizes, a pass being min(8, the queries of one score
 * pass) queries -- eight bits of a membership byte.  Per pass, over the ascending row list of the union of its scopes: the top-messages
 * score pass in its scoped form -- a passing row raises its message's slot for query j only when bit j of the row's membership byte is
 * set, a clear bit does nothing -- so a message whose chunks lie in several queries' scopes gets, for each query, the best score among
 * the rows of THAT query's scope.  Then tavb_search_top_messages' own launches, unchanged: the histogram pass over [queries][n_messages],
 * boundary search, refinement, compaction and sort with the message ordinals as positions.  "topk_scores_bytes" holds: where
 * [queries of a pass][n_messages] x 4 bytes would exceed it the pass' queries go in sub-groups over the same list (at least one query
 * each).  A row several scopes of a pass share is read once per pass.
 *   tavb_search_top_messages_scoped: queries on the host, one more synchronise at the end; out_messages / out_scores [nq, k], out_counts
 *     [nq] as tavb_search_top_messages: MESSAGE ordinals, no ordinal_base.  "masked_route" reports 9, "last_topk_refine" the most rounds
 *     of any query.
 *   tavb_search_top_messages_scoped_device: dev_queries device float32 [nq, dim]; out_keys [nq, k] sorted, zero-padded keys carrying message
 *     ordinals, device or device-writable pinned memory; waits only for the unions' sizes ("last_topk_refine" at the next tavb_synchronize).
 * 1 <= k <= TAVB_MAX_LARGE_K.  Errors are tavb_search_top_messages' (no map, a map that does not cover the corpus, k out of range, NULL
 * arguments) and the scoped calls' (rows != the corpus' rows, a NULL or misaligned mask pointer), each with a message.  nq == 0, an empty
 * corpus or n_messages == 0: zero counts / zero keys, nothing launched.  A query whose mask is empty gets an empty list.  Timed under
 * TAVB_KERNEL_CONVERT (unions, lists, membership), TAVB_KERNEL_SCAN (score pass) and TAVB_KERNEL_TOPK (everything behind it). */
int tavb_search_top_messages_scoped(tavb_ctx* ctx, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                                    const float* min_scores, int64_t* out_messages, float* out_scores, int32_t* out_counts);
int tavb_search_top_messages_scoped_device(tavb_ctx* ctx, const float* dev_queries, int32_t nq, const uint32_t* const* dev_masks, int64_t rows,
                                           int32_t k, const float* min_scores /*host*/, tavb_key* out_keys);

/* ---- the best k MESSAGES on the 32/64-query tile: one corpus pass per 64 queries -----------------------------------------------------------
 * tavb_search_top_messages reads the corpus once per eight queries.  These calls read it -- or the span of ONE packed mask -- once per 64, on
 * the 32/64-query MFMA tile in its top-messages form: the tile's own admission test on its own score (score > the float just below the
 * query's min_score; NaN or a threshold above 1 admits nothing), then ONE unsigned atomic max per admitted (row, query) pair on the same
 * zeroed [queries][n_messages] array, in the same encoding, that tavb_search_top_messages' score pass writes.  The tile keeps no candidate
 * lists here, so its k <= 64 bound does not apply: 1 <= k <= TAVB_MAX_LARGE_K.  Behind the tile launch come tavb_search_top_messages' own
 * launches, unchanged, eight queries at a time: the histogram pass over [queries][n_messages], boundary search, refinement, compaction and
 * sort with the message ordinals as positions.  Groups are up to 64 queries, cut further by "topk_scores_bytes" over [queries][n_messages]
 * (at least one query); per group two memsets and one tile launch over the span -- no sample pass and no phases: no threshold ever rises.
 * SCORES ARE THE TILE'S OWN (fp32 rows: v_mfma_f32_32x32x2_f32 in the tile's summation order; fp16 rows: the fp32 query split into an fp16
 * high and low plane), as on every other route of the 32/64-query tile: within a few ulp of tavb_search_top_messages', not bit for bit --
 * which is why the binding's option "top_messages_tile" defaults to 0.  The fp16 shadow of an fp32 corpus is not used.
 * dev_bits / rows / first_row / last_row follow tavb_search_masked_batch (packed mask over the corpus' rows, 4-byte aligned, rows = the
 * corpus' rows, [first_row, last_row] holds every set bit; first_row > last_row: nothing to scan); dev_bits == NULL: the whole corpus (rows,
 * first_row and last_row are then not read).  The row -> message map must be 64-byte aligned (the tile reads 16 entries per scalar load).
 *   tavb_search_top_messages_tile: queries on the host, one synchronise; outputs as tavb_search_top_messages.
 *   tavb_search_top_messages_tile_device: dev_queries device float32 [nq, dim], nq >= 1; out_keys as tavb_search_top_messages_device; nothing
 *     waited for unless the thresholds differ between the queries (their upload is waited for, as on the masked tile).
 * "masked_route" reports 10, "last_tier" 5, "last_skinny_kernel" the instantiation (one of the four ring variants: 12832, 12864, 6432, 6464).
 * Errors are tavb_search_top_messages' (no map, a map that does not cover the corpus, k out of range, NULL arguments) plus the tile's own:
 * rows that are not a multiple of 64 bytes, or a map that is not 64-byte aligned: TAVB_E_UNSUPPORTED; a misaligned mask, rows != the corpus'
 * rows, a span outside the corpus: TAVB_E_INVALID -- each with a message.  Timed under TAVB_KERNEL_SKINNY (the tile) and TAVB_KERNEL_TOPK.
 * tavb_plan_top_messages_tile: the binding's rule under "top_messages_tile" = 1, a pure function: 1 = the tile, 0 = tavb_search_top_messages
 * (negative: an error).  allowed == span == the corpus' rows for an unmasked lookup.  The tile where the row size is a multiple of 64 bytes,
 * nq >= min_batch ("top_messages_tile_min_batch") and -- under a mask -- allowed x row bytes >= min_bytes and the row list's bytes
 * (ceil(nq / 8) x allowed) are at least pct % of the tile's (ceil(nq / 64) x span): "mask_tile_min_bytes" / "mask_tile_pct". */
int tavb_search_top_messages_tile(tavb_ctx* ctx, const float* queries_host, int32_t nq, int32_t k, const float* min_scores, const uint32_t* dev_bits,
                                  int64_t rows, int64_t first_row, int64_t last_row, int64_t* out_messages, float* out_scores, int32_t* out_counts);
int tavb_search_top_messages_tile_device(tavb_ctx* ctx, const float* dev_queries, int32_t nq, int32_t k, const float* min_scores /*host*/,
                                         const uint32_t* dev_bits, int64_t rows, int64_t first_row, int64_t last_row, tavb_key* out_keys);
int tavb_plan_top_messages_tile(int32_t nq, int32_t dim, int32_t dtype, int64_t allowed, int64_t span, int64_t min_batch, int64_t min_bytes,
                                int64_t pct);

/* ---- scoped batches on the 32/64-query tile: one scope per query on the matrix cores ----------------------------------------------------
 * The scoped batch above reads, per pass of eight queries, the union of the pass' scopes; dense, independent or disjoint scopes make that
 * union most of the span once per eight queries.  These calls read the SPAN of the batch's union once per 64 queries instead, on the
 * 32/64-query MFMA tile (the tile of tavb_search_masked_batch), with the per-query test in the tile's admission path.  Same dev_masks (HOST
 * array of nq device pointers, none NULL, 4-byte aligned, repeats allowed); [first_row, last_row] must hold every set bit of every mask
 * (first_row > last_row: every scope is empty -- zero counts / zero keys, nothing launched).  1 <= k <= 64 and rows of a multiple of 64
 * bytes, else TAVB_E_UNSUPPORTED; NULL arguments, a NULL mask pointer, rows != the corpus' rows and a span outside the corpus are
 * TAVB_E_INVALID, each with a message.
 * CONTRACT: the tile's, not the row list's.  Scores are the tile's float32 dot products (fp32 accumulation inside the matrix pipe), so per
 * query the answer equals the streaming routes' (tavb_search_scoped_batch, tavb_search_subset_batch_resident over that mask's row list)
 * except among float32 near-ties, scores within a few 1e-7.  A batch whose masks all hold the same bits returns tavb_search_masked_device's
 * keys for that batch and mask bit for bit; with every mask all ones, the keys of the unmasked 32/64-query tile.
 * On the device, in WAVES of query tiles: the membership PLANES of the wave -- per block of 32 queries one uint32 per row of the span, bit i
 * = the scope of query i of the block holds the row (a 32 x 32 bit transpose of the masks' words, one launch per 64 queries) -- then the
 * tile's phases over rows [first_row / 256 * 256, last_row].  A wave is as many 64-query tiles as fit 64 MiB of planes, at least one (1M
 * rows: 512 queries); the workspace is max(64 MiB, 8 bytes x span) whatever the batch.  Nothing is waited for before the result.
 * "masked_route" reports 5, "last_tier" 5, "last_skinny_kernel" the tile's instantiation.  Timed under TAVB_KERNEL_CONVERT (planes),
 * TAVB_KERNEL_SKINNY / TAVB_KERNEL_MFMA_SAMPLE and TAVB_KERNEL_MERGE.
 *   tavb_search_scoped_tile / _device / tavb_search_messages_scoped_tile: the three forms of the scoped batch above.
 *   tavb_scope_planes: the planes alone.  With span_begin = first_row / 256 * 256, stride = (last_row + 32) / 32 * 32 - span_begin and n_blocks =
 *     1 for n_masks <= 32, else 2 * ceil(n_masks / 64) (the tile-padded batch): dev_planes_out (device uint32 [n_blocks * stride], 64-byte
 *     aligned) [b * stride + r - span_begin] has bit i set when dev_masks[32 b + i] holds row r, r <= last_row; zero for padding queries and
 *     behind last_row, whatever the masks' last words hold at or beyond `rows`.  Asynchronous on the context's stream. */
int tavb_search_scoped_tile(tavb_ctx* ctx, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row,
                            int64_t last_row, int32_t k, const float* min_scores, int64_t* out_ordinals, float* out_scores, int32_t* out_counts);
int tavb_search_scoped_tile_device(tavb_ctx* ctx, const float* dev_queries, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row,
                                   int64_t last_row, int32_t k, const float* min_scores /*host*/, tavb_key* out_keys);
int tavb_search_messages_scoped_tile(tavb_ctx* ctx, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row,
                                     int64_t last_row, int32_t k, const float* min_scores, int32_t max_messages, int64_t* out_messages, float* out_scores,
                                     int32_t* out_counts);
int tavb_scope_planes(tavb_ctx* ctx, const uint32_t* const* dev_masks, int32_t n_masks, int64_t rows, int64_t first_row, int64_t last_row,
                      uint32_t* dev_planes_out);

/* ---- scoped batches on the 128/256-query filter tile: exact, 1 <= k <= 256 ---------------------------------------------------------------
 * The per-query-scope twin of tavb_search_masked_wide, for fp16 corpora of any width (one that is no multiple of 64 filters on the zero-padded
 * copy of the rows) and 1 <= k <= TAVB_MAX_FUSED_K, else TAVB_E_UNSUPPORTED (the message names the row-list route).  The arguments, the span
 * rule and the argument errors of tavb_search_scoped_tile.  In WAVES of query tiles: the membership planes of the wave (as
 * tavb_scope_planes writes them, 8 blocks per 256-query tile, 4 per 128-query tile), the filter ladder of the 128/256-query tile over rows
 * [first_row / 256 * 256, last_row] with the per-query test in the tile's admission path, the band selection and the rescoring with the
 * streaming kernels' arithmetic.  A query with more near-duplicates around its k-th best than "band_max" keys is flagged; the flagged
 * queries are read back -- one synchronise per wave -- and re-run on the row-list scoped route with their own masks ("last_flagged" counts
 * them).  CONTRACT: tavb_search_scoped_batch's answers BIT FOR BIT -- ordinals, float32 scores, counts.  A wave is as many whole 256-query
 * tiles as fit "scope_wave_bytes" (64 MiB) of planes, at least one tile; the planes' workspace is at most max(64 MiB, 32 bytes x span rows)
 * whatever the batch.  "masked_route" reports 6, "last_tier" 4, "last_mfma_shape" the filter's MFMA.  Timed under TAVB_KERNEL_CONVERT
 * (planes), TAVB_KERNEL_MFMA / TAVB_KERNEL_MFMA_SAMPLE, TAVB_KERNEL_MERGE and TAVB_KERNEL_RESCORE. */
int tavb_search_scoped_wide(tavb_ctx* ctx, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row,
                            int64_t last_row, int32_t k, const float* min_scores, int64_t* out_ordinals, float* out_scores, int32_t* out_counts);
int tavb_search_scoped_wide_device(tavb_ctx* ctx, const float* dev_queries, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row,
                                   int64_t last_row, int32_t k, const float* min_scores /*host*/, tavb_key* out_keys);
int tavb_search_messages_scoped_wide(tavb_ctx* ctx, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row,
                                     int64_t last_row, int32_t k, const float* min_scores, int32_t max_messages, int64_t* out_messages, float* out_scores,
                                     int32_t* out_counts);

/* ---- removing rows: compaction of the corpus on the device ---------------------------------------------------------------------------
 * The removal the reference leaves as a TODO (storage/sqlite/reltermsindex.py:181-192 `remove_term`; knowpro/fuzzyindex.py:113-127, the
 * commented `remove_at` around np.delete): dev_remove_bits is a mask in the bit form above in which a SET bit means "remove"; rows must equal
 * the corpus' rows; bits at or beyond `rows` may hold anything.  Afterwards rows [0, kept) hold the kept rows in their old order, bit for
 * bit -- np.delete(corpus, flatnonzero(mask), axis=0) -- *out_rows = kept, and the call has ended with tavb_set_corpus(.., kept, ..) (same
 * dim, dtype and ordinal_base; the pointer is dev_dst when that is given) and tavb_corpus_modified(first removed row).
 *   dev_dst == NULL: IN PLACE.  Rows only move down.  From the 64-row tile of the first removed row on, the corpus is taken in passes of
 *     "compact_pass_rows" rows (option; rounded up to a multiple of 64; 0 = auto, the default: about 64 MiB of rows): one launch gathers a
 *     pass' kept rows densely into a staging workspace of that size, a second copies them to their final place, which ends at or below the
 *     end of the pass -- every later pass reads only rows beyond it.  The order between the launches is stream order and nothing else: no
 *     workgroup waits for another.  Two launches per pass; bytes moved: four times the bytes from the first removed row to the end, at most.
 *   dev_dst != NULL: OUT OF PLACE, one launch: the kept rows are gathered into dev_dst (device memory for at least `kept` rows -- `rows`
 *     rows always do -- that does not overlap the corpus, aligned to the element size); the old corpus is read only.  The route for a corpus
 *     buffer the caller may not write.
 * A workgroup takes 64 rows, finds its first slot from the per-chunk counts (TAVB_MASK_ROWS_PER_WORKGROUP rows a chunk, as tavb_mask_expand's
 * write pass does) and a wave copies a row with the widest of 16-, 8-, 4- and 2-byte accesses that the row bytes and the addresses allow.
 * A mask with no bit set is a no-op: nothing moves, no cache is touched, dev_dst is neither written nor adopted.  Every bit set leaves 0
 * rows.  rows == 0: *out_rows = 0.  The count pass is waited for (ONE synchronise: the host needs `kept`); the moves are enqueued on the
 * context's stream and NOT waited for -- lookups on this context follow in stream order, anything else calls tavb_synchronize first.  The
 * mask must stay alive until then.  Timed under TAVB_KERNEL_CONVERT.  The row -> message map (tavb_set_row_messages) is the caller's to
 * compact and set again. */
int tavb_compact_rows(tavb_ctx* ctx, const uint32_t* dev_remove_bits, int64_t rows, void* dev_dst /* NULL = in place */, int64_t* out_rows);

/* ---- inserting and overwriting rows: expansion of the corpus on the device, scattered row writes ---------------------------------------
 * The insertion the reference keeps commented out (knowpro/fuzzyindex.py:50-83, `insert_at` around np.vstack), in two calls: tavb_expand_rows
 * opens the holes, tavb_scatter_rows fills them (and, alone, overwrites rows).
 * tavb_expand_rows: dev_hole_bits is a mask in the bit form above over the NEW row count new_rows, in which a SET bit means "a hole for a new
 * row"; its clear bits below new_rows must number exactly the corpus' rows -- else the call fails with TAVB_E_INVALID and moves nothing; bits
 * at or beyond new_rows may hold anything.  Afterwards old row i stands, bit for bit, at the i-th row whose bit is clear -- the old rows of
 * np.insert's result -- the holes hold whatever was there, *out_old_rows = the clear bits counted, and the call has ended with
 * tavb_set_corpus(.., new_rows, ..) (same dim, dtype and ordinal_base; the pointer is dev_dst when that is given) and
 * tavb_corpus_modified(first hole).
 *   dev_dst == NULL: IN PLACE.  The corpus buffer must hold new_rows rows (the caller's to guarantee).  Rows only move up.  From the 64-row
 *     tile of the first hole on, the new rows are taken in passes of "compact_pass_rows" rows, FROM THE TAIL: the old rows of a pass are one
 *     contiguous range; one launch copies it into the staging workspace, a second writes its rows to their new places inside the pass.  A pass
 *     reads only old rows at or below its own first new row, and writes only its own new rows, which every later (lower) pass neither reads
 *     nor writes.  The order between the launches is stream order and nothing else: no workgroup waits for another.  Two launches per pass;
 *     every row moves at most twice.  Holes only behind the last old row move nothing.
 *   dev_dst != NULL: OUT OF PLACE, one launch: the old rows are written to their new places in dev_dst (device memory for at least new_rows
 *     rows that does not overlap the corpus, aligned to the element size); the old corpus is read only.  The route for a corpus buffer the
 *     caller may not write, or one that is too small.
 * A mask with no bit set (new_rows == the corpus' rows) is a no-op: nothing moves, no cache is touched, dev_dst is neither written nor
 * adopted.  An empty corpus takes every row as a hole.  The count pass is waited for (ONE synchronise); the moves are enqueued on the context's
 * stream and NOT waited for, as tavb_compact_rows' are.  Timed under TAVB_KERNEL_CONVERT.  The row -> message map is the caller's to set again.
 * tavb_scatter_rows: n host rows [n, dim] (fp32; dim must be the corpus') -> corpus rows dev_positions[j] (int32, in device memory, each in
 * [0, rows) and no two alike: the caller resolves duplicates), converted to the corpus dtype exactly as tavb_upload_rows converts, through the
 * same staging slots.  The positions are checked on the device before anything is written: one outside the corpus fails the call with
 * TAVB_E_INVALID.  The per-corpus caches are KEPT: a row that the cached row-norm maxima cover also gets its fp16 shadow row (fp32 corpora,
 * and fp16 corpora whose width is not a multiple of 64) and folds its norms into the maxima, which stay upper bounds (a replaced row's old
 * norm is not taken out).  Returns when the rows are written (rows_host may be reused).  Timed under TAVB_KERNEL_CONVERT. */
int tavb_expand_rows(tavb_ctx* ctx, const uint32_t* dev_hole_bits, int64_t new_rows, void* dev_dst /* NULL = in place */, int64_t* out_old_rows);
int tavb_scatter_rows(tavb_ctx* ctx, const float* rows_host_f32, int64_t n, int32_t dim, const int32_t* dev_positions_i32);

/* Merge `n_lists` sorted key lists per query (dev_lists [n_lists, nq, k], e.g. the
 * all-gathered per-shard results) into one list per query: dev_out_keys [nq, k]. */
int tavb_merge_device(tavb_ctx* ctx, const tavb_key* dev_lists, int32_t n_lists, int32_t nq, int32_t k,
                      tavb_key* dev_out_keys);

/* tavb_merge_device for lists of any length up to TAVB_MAX_LARGE_K: n_lists (1 .. 64) sorted, zero-padded lists per query of up to 65535,
 * dev_lists [n_lists, nq, k] -- or, with n_lists NEGATIVE, -n_lists lists in query-major order [nq, -n_lists, k] -- -> out_keys [nq, k]
 * (device or device-writable pinned memory), what tavb_merge_topk_host returns for the same lists, the rule for TAVB_KEY_PEER_FAILED
 * included.  Every key finds its own rank with binary searches in the other lists (tavb_topk.hip): real keys must be unique.
 * Asynchronous; timed under TAVB_KERNEL_MERGE. */
int tavb_merge_topk_device(tavb_ctx* ctx, const tavb_key* dev_lists, int32_t n_lists, int32_t nq, int32_t k, tavb_key* out_keys);

/* tavb_merge_topk_device for lists whose keys carry MESSAGE ordinals below n_messages (1 <= n_messages < 2^31 - 1): the same shapes and the
 * two layouts (n_lists negative: query-major), up to 65535 queries -> out_keys [nq, k] (device or device-writable pinned memory), what
 * tavb_merge_top_messages_host returns for the same lists, the rule for TAVB_KEY_PEER_FAILED included; a key whose message is at or beyond
 * n_messages is dropped.  Per group of up to TAVB_MAX_STREAM_QUERIES queries (cut by "topk_scores_bytes" over [queries][n_messages], at
 * least one): the [queries][n_messages] array of tavb_search_top_messages zeroed, ONE launch in which every key does one atomic max on its
 * message's slot (tavb_topk.hip), then that lookup's histogram pass, boundary search, refinement, compaction and sort unchanged
 * ("last_topk_refine" reports the rounds at the next tavb_synchronize).  A max does not depend on the order of its operands: the result is
 * deterministic.  The cost is a pass over n_messages slots per query, whatever n_lists x k is.  Uses the workspaces of
 * tavb_search_top_messages; needs no row -> message map.  Asynchronous; the scatter and the failure fill are timed under
 * TAVB_KERNEL_MERGE, the selection under TAVB_KERNEL_TOPK. */
int tavb_merge_top_messages_device(tavb_ctx* ctx, const tavb_key* dev_lists, int32_t n_lists, int32_t nq, int32_t k, int64_t n_messages,
                                   tavb_key* out_keys);

/* Decode host copies of keys into ordinals/scores/counts (pure host helper). */
int tavb_decode_keys(const tavb_key* keys_host, int32_t nq, int32_t k, int64_t* out_ordinals, float* out_scores,
                     int32_t* out_counts);

/* ---- row-sharded corpora: one process per GPU, RCCL over xGMI ------------------------------------------------------------
 * Every rank holds a contiguous range of the corpus rows in its own context (tavb_set_corpus with ordinal_base = the shard's first
 * row); a lookup is every rank scanning its shard for the same queries, ONE all-gather of the per-shard [nq, k] key lists
 * (nq * k * 8 bytes per rank: 256 KiB at 1024 x 32) and a merge kernel on every rank, so that every rank returns the whole-corpus
 * answer of vectorbase.py:163-190 (keys carry global ordinals and order by (score desc, ordinal asc): the merged answer is the
 * single-device one, ties included).  A rank whose local search fails still joins the all-gather -- the peers are never left waiting -- with
 * TAVB_KEY_PEER_FAILED lists, returns its own error, and every other rank's merged lists decode to TAVB_E_PEER (tavb_decode_keys): a lookup
 * either returns the whole-corpus answer on a rank or an error, never an answer that silently misses a shard.  That covers every failure
 * local to a rank between entering the call and the all-gather: the state of its shard, its launches, its allocations (the exchange buffers
 * themselves are reserved by tavb_comm_init, option "comm_reserve_keys", so the exchange path allocates nothing).  What it cannot cover -- a
 * peer that never makes the call, or dies inside it -- is bounded by "comm_timeout_ms": tavb_synchronize aborts the communicator and returns
 * TAVB_E_TIMEOUT instead of waiting for ever.
 * The collective is issued by the library itself, on the context's stream, behind the scan and
 * in front of the merge -- RCCL (librccl.so.1, resolved with dlopen at tavb_comm_init: no link-time dependency) is the only
 * communication layer; torch.distributed is not needed on the lookup path.
 *
 * tavb_comm_unique_id: rank 0 creates the 128-byte rendezvous id (ncclGetUniqueId) and hands it to the other ranks by any means
 * (a file, a socket, an existing torch.distributed / MPI broadcast).  tavb_comm_init: collective over all `world` ranks
 * (ncclCommInitRank on the context's device).  One communicator per context; tavb_destroy / tavb_comm_destroy release it. */
#define TAVB_COMM_ID_BYTES 128
int tavb_comm_unique_id(void* out_id /* TAVB_COMM_ID_BYTES */);
int tavb_comm_init(tavb_ctx* ctx, const void* id /* TAVB_COMM_ID_BYTES */, int32_t rank, int32_t world);
int tavb_comm_destroy(tavb_ctx* ctx);
/* Collective tavb_search_device: queries (device float32 [nq, dim], the same on every rank) -> out_keys [nq, k] = the merged
 * whole-corpus lists, on every rank.  out_keys may be device memory or pinned host memory the device can write (the merge kernel
 * writes it directly).  Asynchronous on the context's stream; tavb_synchronize before reading.  Every rank must call with the same
 * nq and k.  Without a communicator (or world == 1) this is tavb_search_device. */
int tavb_search_allgather(tavb_ctx* ctx, const float* dev_queries, int32_t nq, int32_t k, float min_score, tavb_key* out_keys);
/* The exchange on its own, for lists a rank produced by other means (its part of a subset search, vectorbase.py:203-230; its survivors
 * of a predicate, :191-201): dev_local_keys [nq, k] sorted lists with GLOBAL ordinals / positions -> out_keys [nq, k] merged over all
 * ranks (device or device-writable pinned memory).  Asynchronous; collective. */
int tavb_allgather_merge(tavb_ctx* ctx, const tavb_key* dev_local_keys, int32_t nq, int32_t k, tavb_key* out_keys);
/* The two calls above for 1 <= k <= TAVB_MAX_LARGE_K (the top 1000 of a corpus too big for one GPU): tavb_search_topk_device on every
 * rank (min_scores: nq thresholds on the host, the same on every rank), the all-gather, the merge of tavb_merge_topk_device.  The
 * protocol is that of tavb_search_allgather step by step: argument errors every rank makes alike return at once -- among them a k above
 * "comm_reserve_keys" (one query's list must fit the reserved buffers) and a world of more than 64 ranks; whatever fails on one rank, the
 * workspaces of its local lookup included, still joins every chunk of the exchange with TAVB_KEY_PEER_FAILED lists; nothing allocates
 * between entry and ncclAllGather while nq x k keys fit the reserve, bigger exchanges travel in chunks of whole queries (64 queries per
 * chunk at k = 16384 and the default reserve); "comm_fail_rank", "comm_fail_alloc", "comm_stall_ms", "comm_force" and "comm_timeout_ms"
 * act as they do there.  Without a communicator: tavb_search_topk_device / a copy. */
int tavb_search_topk_allgather(tavb_ctx* ctx, const float* dev_queries, int32_t nq, int32_t k, const float* min_scores, tavb_key* out_keys);
int tavb_allgather_merge_topk(tavb_ctx* ctx, const tavb_key* dev_local_keys, int32_t nq, int32_t k, tavb_key* out_keys);
/* The two calls above for the best k MESSAGES (1 <= k <= TAVB_MAX_LARGE_K): tavb_search_top_messages_device on every rank over its shard
 * -- dev_rows NULL (n_rows 0): the whole shard; dev_rows: this rank's part of a mask as shard-local rows, and a non-NULL dev_rows with
 * n_rows 0 (or a shard without rows) joins with zero lists -- then the all-gather, then the merge of tavb_merge_top_messages_device over the
 * context's n_messages.  Message ordinals are global: every rank sets its slice of ONE map with the SAME n_messages (tavb_set_row_messages;
 * a rank without rows too), and every shard's own top k suffices for the whole-corpus answer (tavb_merge_top_messages_host).  The protocol
 * is that of tavb_search_topk_allgather step by step: argument errors every rank makes alike return at once -- k out of range, NULL
 * pointers, a k above "comm_reserve_keys", more than 64 ranks, n_messages 0 (no map: TAVB_E_NO_CORPUS) or >= 2^31 - 1; whatever fails on
 * one rank -- a map that does not cover its shard, a bad row list, the workspaces of its lookup -- still joins every chunk of the exchange
 * with TAVB_KEY_PEER_FAILED lists; the merge's own workspaces (no larger than the rank's lookup reserved) are reserved behind a chunk's
 * all-gather, and a rank whose merge fails still joins the all-gathers of every later chunk before it returns its error; chunks, "comm_fail_rank",
 * "comm_fail_alloc", "comm_stall_ms", "comm_force" and "comm_timeout_ms" act as they do there.  The all-gather is timed under
 * TAVB_KERNEL_EXCHANGE.  Without a communicator: tavb_search_top_messages_device / a copy. */
int tavb_search_top_messages_allgather(tavb_ctx* ctx, const float* dev_queries, int32_t nq, int32_t k, const float* min_scores /*host*/,
                                       const int32_t* dev_rows, int64_t n_rows, tavb_key* out_keys);
int tavb_allgather_merge_top_messages(tavb_ctx* ctx, const tavb_key* dev_local_keys, int32_t nq, int32_t k, tavb_key* out_keys);
/* keys [count] that carry POSITIONS into a list -> the same keys carrying dev_map[position] (int32 [map_len]): a rank's subset search
 * (tavb_search_subset_device) numbers the part of the caller's subset that lies in its shard; the map leads back to the positions in the
 * caller's whole list.  In place, asynchronous.  The map must be monotonic for the lists to stay sorted among equal scores. */
int tavb_remap_key_positions(tavb_ctx* ctx, tavb_key* dev_keys, int64_t count, const int32_t* dev_map, int64_t map_len);

/* ---- rows of the corpus as queries: "more like row 17", near-duplicate detection ------------------------------------------------
 * The nearest neighbours of rows ALREADY in the corpus, without a round trip of the rows through the host (a device-only corpus has no
 * host matrix at all).  Per wave of at most "rows_query_wave" rows: ONE gather launch (the rows -> a dense float32 query batch in a
 * workspace of the context; fp16 rows widened exactly, fp32 rows copied: bit for bit the values the kernels multiply), the lookup every
 * device-resident batch takes -- tavb_search_device's routing up to TAVB_MAX_FUSED_K keys, tavb_search_topk's passes beyond -- and, with
 * exclude_self, ONE launch that takes the query's own row out of its list.  exclude_self != 0: the lookup asks for k + 1 keys, the key
 * whose ordinal is the query's own row is removed where the list holds it, the gap closed, the first k kept.  That is exact, no tolerance:
 * the k + 1 best of all rows always hold the k best of the OTHER rows -- with the own row in the list the rest are those, without it
 * (more than k exact duplicates of lower ordinal tie with it; a zero or un-normalised row that is not its own best match; an own score
 * below min_score) the first k are.  exclude_self == 0: the plain lookup with the rows as queries, k keys, nothing removed.
 * The rows follow the PRECONDITION on device-resident queries above (every element rounds to a finite fp16 value): the library never sees
 * them on the host.  A row listed twice is answered twice.
 *
 * tavb_search_rows: positions_host int32 [n], each in [0, rows) (checked here: TAVB_E_INVALID), min_scores float32 [n] on the host, 1 <= k <=
 * TAVB_MAX_LARGE_K - 1 with exclude_self (k + 1 stays inside what tavb_search_topk serves), TAVB_MAX_LARGE_K without; outputs [n, k] / [n] as
 * tavb_search_batch (ordinals carry ordinal_base).  The positions are staged, every wave enqueued, the keys copied back ONCE: one
 * synchronise at the end and none in between on routes that have none.  n == 0 or an empty corpus: zero counts, nothing launched.
 * tavb_search_rows_device: the positions on the device (int32 [n]; the CALLER guarantees their range -- a position outside [0, rows) is
 * gathered as a row of zeros), out keys [n, k] sorted and zero-padded, carrying ordinal_base + row (below 2^32 - 1), and counts int32 [n]
 * (optional, NULL: not written) in device or device-writable pinned memory.  Asynchronous, like the other *_device forms.
 * tavb_search_rows_sorted: every survivor per row (max_hits == 0, the `[-0:]` quirk) through tavb_search_sorted's passes; outputs,
 * max_total and the synchronises are that call's.  Its results are concatenated lists of any length, which the drop launch does not take:
 * with exclude_self the own row is removed ON THE HOST, after the copy (one pass over the results).
 * tavb_gather_rows_f32: the gather on its own -- dev_positions int32 [n] -> dev_out float32 [n, dim].  Asynchronous. */
int tavb_search_rows(tavb_ctx* ctx, const int32_t* positions_host, int64_t n, int32_t k, int32_t exclude_self, const float* min_scores,
                     int64_t* out_ordinals, float* out_scores, int32_t* out_counts);
int tavb_search_rows_device(tavb_ctx* ctx, const int32_t* dev_positions, int64_t n, int32_t k, int32_t exclude_self, const float* min_scores /*host*/,
                            tavb_key* dev_out_keys, int32_t* dev_out_counts);
int tavb_search_rows_sorted(tavb_ctx* ctx, const int32_t* positions_host, int64_t n, int32_t exclude_self, const float* min_scores, int64_t max_total,
                            int64_t* out_ordinals, float* out_scores, int64_t* out_counts, int64_t* out_total);
int tavb_gather_rows_f32(tavb_ctx* ctx, const int32_t* dev_positions, int64_t n, float* dev_out);

/* ---- near-duplicate self-join (additive) ----------------------------------------
 * Every pair of corpus rows i < j whose score reaches min_score -- the whole-corpus form of "which rows are near-duplicates", which the row
 * lookups above answer with one unrestricted top-k per row.  No reference counterpart.
 *
 * tavb_join_pairs: ONE launch computes the tiles tj >= ti of X16 . X16^T on the matrix cores (X16: an fp16 corpus itself, an fp32 corpus'
 * fp16 shadow -- built as the 128/256-query filter tile builds it, option "f32_shadow") and admits, per element, the pairs j > i whose
 * approximate score reaches min_score - 2 delta; delta is ONE rigorous bound for the whole launch on |approximate - exact| (the filter
 * tile's bound with the query replaced by a corpus row: csrc/tavb_pairs_join.hip).  A second launch scores every candidate exactly -- row j
 * against row i as the query, in the streaming kernels' arithmetic -- and keeps those reaching min_score (compared as float32): the score of a
 * pair is bit for bit what tavb_search_sorted reports for row j with row i as the query.  dev_mask_bits (optional, NULL: every row): a packed
 * mask over the corpus' rows (tavb_mask_expand's layout, 4-byte aligned); only pairs whose BOTH rows are set are reported.
 * Host-synchronous.  out_i / out_j (int64, carrying ordinal_base) / out_scores (float32): room for `capacity` (1 .. 2^30) entries each;
 * *out_total pairs are written, in ARBITRARY order.  *out_needed = the candidate pairs the join counted.  Returns
 *   TAVB_OK             the pairs are complete (also: fewer than two rows, or a NaN min_score -- no pairs, nothing launched);
 *   TAVB_PAIRS_NO_FIT   *out_needed > capacity: nothing was written (*out_total = 0); a call with capacity >= *out_needed fits;
 *   TAVB_PAIRS_REFUSED  delta is not finite (a row holds inf / NaN, or overflows fp16), or there is no memory for the shadow or the
 *                       workspace: nothing can be proven or built, nothing was launched, the caller keeps the row lookups;
 * both positive: they are answers, not failures, and set no message.  rows that are not a multiple of 64 elements, an fp32 corpus under
 * "f32_shadow" = 0: TAVB_E_UNSUPPORTED; NULL outputs, a capacity out of range, a misaligned mask: TAVB_E_INVALID.  Timed under
 * TAVB_KERNEL_MFMA (the join) and TAVB_KERNEL_RESCORE (the maxima, the rescoring).
 *
 * tavb_plan_pairs_join: whether the binding sends an index to the join under option "pairs_join" = 1.  1 when dim is a multiple of 64 (up
 * to 16384: the filter tile's width rule), 2 <= rows < 2^31 - 1, rows >= min_rows (the option "pairs_join_min_rows"), the engine is a single
 * GPU (single_gpu != 0: device groups and row shards keep the row lookups) and, for TAVB_F32, the shadow exists or may be built (has_shadow
 * != 0: "f32_shadow" >= 1).  0 otherwise; negative: an argument out of range.  A pure function, needs no context and no GPU. */
#define TAVB_PAIRS_NO_FIT 1
#define TAVB_PAIRS_REFUSED 2
int tavb_join_pairs(tavb_ctx* ctx, float min_score, const uint32_t* dev_mask_bits, int64_t capacity, int64_t* out_i, int64_t* out_j, float* out_scores,
                    int64_t* out_total, int64_t* out_needed);
int tavb_plan_pairs_join(int64_t rows, int32_t dim, int32_t dtype, int32_t has_shadow, int32_t single_gpu, int64_t min_rows);

/* ---- measurement ------------------------------------------------------------ */
/* HIP-event timing of the kernels this context launches, on the stream they run on.
 * kernel ids: 0 = streaming scan (dot + score + select), 1 = list merge,
 *             2 = MFMA batched scan (256-query tile: the last phase of the threshold ladder), 3 = normalise,
 *             4 = f32->f16 convert, 5 = the earlier phases of the ladder (either MFMA tile), 6 = 32-query MFMA tile
 *             (last phase), 7 = candidate rescoring of the 256-query tile, 8 = the all-gather of tavb_search_allgather,
 *             9 = the selection of a large-k lookup (refinement, compaction, finish; its score pass counts as 0). */
#define TAVB_KERNEL_SCAN 0
#define TAVB_KERNEL_MERGE 1
#define TAVB_KERNEL_MFMA 2
#define TAVB_KERNEL_NORMALIZE 3
#define TAVB_KERNEL_CONVERT 4
#define TAVB_KERNEL_MFMA_SAMPLE 5 /* threshold-seeding phases of the MFMA paths (all ladder phases but the last) */
#define TAVB_KERNEL_SKINNY 6 /* 32-query MFMA tile (small batches; every batch on fp32 corpora) */
#define TAVB_KERNEL_RESCORE 7 /* exact fp32-query rescoring of the 256-query tile's candidates (+ query preparation) */
#define TAVB_KERNEL_EXCHANGE 8 /* the RCCL all-gather of tavb_search_allgather (stream time between its two events: includes waiting for the slowest rank) */
#define TAVB_KERNEL_TOPK 9 /* boundary refinement + compaction + exact finish of tavb_search_topk / tavb_search_subset_topk; the same and the
                             * sort + decode of tavb_search_sorted / tavb_search_subset_sorted / tavb_sort_keys_device */
#define TAVB_KERNEL_COUNT 10
int tavb_profile_enable(tavb_ctx* ctx, int32_t on);
int tavb_profile_reset(tavb_ctx* ctx);
int tavb_profile_read(tavb_ctx* ctx, int32_t kernel_id, double* out_total_ms, int64_t* out_launches);

/* How the library scans a corpus of `rows` rows for a batch of `nq` (>= 65) queries on a part with `n_cu` compute units, with default
 * options: the phase boundaries of the threshold ladder of the 128/256-query tile (phase i scans rows [out_bounds[i], out_bounds[i+1]);
 * at most `cap` entries are written, out_bounds may be NULL).  Returns the number of phases = tile-kernel launches per lookup (> 0), or
 * a negative error code.  No reference counterpart (the reference scans once, vectorbase.py:176); a pure function, needs no context and no
 * GPU -- what lets a committed profile be checked against the code that ships (tests/test_bench_contract.py). */
int tavb_plan_ladder(int64_t rows, int32_t nq, int32_t n_cu, int64_t* out_bounds, int32_t cap);

/* The MFMA shape (16 = v_mfma_f32_16x16x32_f16, 32 = v_mfma_f32_32x32x16_f16) a filter launch of the 128/256-query tile runs on, given the
 * option "mfma_shape" (16 or 32), the query tile (128 or 256), whether the launch is the SPLIT exact form, whether "mfma_bdirect" is on, and the
 * measurement options "mfma_sched" and "mfma_ablate".  Returns 16 or 32, or a negative error code for a shape or tile out of range (the
 * rule "mfma_shape" is validated by).  A pure function, needs no context and no GPU. */
int tavb_plan_filter_shape(int32_t shape, int32_t query_tile, int32_t split, int32_t bdirect, int32_t sched, int32_t ablate);

/* Which route a masked batch takes under option "mask_tile" = 1: 1 = the 32/64-query tile (tavb_search_masked_batch), 0 = the gather route.
 * nq queries, k, the corpus' dim and dtype (TAVB_F32 / TAVB_F16), `allowed` set rows inside a span of `span` rows (last allowed row + 1 - the
 * first allowed row rounded down to a multiple of 256), and the options "mask_tile_min_bytes" / "mask_tile_pct".  The tile when it serves the shape
 * (1 <= k <= 64, rows of a multiple of 64 bytes), nq is at least the unmasked tile's own lower bound (the defaults of "skinny_min_batch_f32" /
 * "skinny_min_batch_f16"), allowed x row bytes >= min_bytes, and ceil(nq / 8) x allowed x 100 >= ceil(nq / 64) x span x pct -- the gather
 * route's bytes are at least pct % of the tile's.  Negative: an argument out of range.  A pure function, needs no context and no GPU. */
int tavb_plan_masked(int32_t nq, int32_t k, int32_t dim, int32_t dtype, int64_t allowed, int64_t span, int64_t min_bytes, int64_t pct);

/* Which route a scoped batch (one mask per query) takes under option "scope_tile" = 1: 1 = the 32/64-query tile (tavb_search_scoped_tile), 0 =
 * the row-list route (tavb_search_scoped_batch).  gather_rows: over the row-list route's passes of eight queries, in the order they are
 * submitted, the sum of each pass' LARGEST scope -- a lower bound of the rows that route reads; span: rows from the first set row of any
 * scope, rounded down to a multiple of 256, to the last.  1 when the tile serves the shape (1 <= k <= 64, rows of a multiple of 64 bytes,
 * nq at least the unmasked tile's lower bound), gather_rows x row bytes >= ceil(nq / 8) x min_bytes, and gather_rows x 100 >= ceil(nq / 64)
 * x span x pct.  0 otherwise; negative: an argument out of range.  Needs no GPU. */
int tavb_plan_scoped(int32_t nq, int32_t k, int32_t dim, int32_t dtype, int64_t gather_rows, int64_t span, int64_t min_bytes, int64_t pct);

/* Whether a scoped batch takes the 128/256-query filter tile + rescoring (tavb_search_scoped_wide) under option "scope_wide" = 1; where this
 * and tavb_plan_scoped both say yes the wide route wins.  The arguments of tavb_plan_scoped, except that gather_rows counts passes of FOUR
 * queries for k > 64 (the row-list route's passes there), eight otherwise.  1 when the corpus is fp16 and the route serves the shape (dim <=
 * 16384, 1 <= k <= TAVB_MAX_FUSED_K), nq is at least the shipped default of "mfma_min_batch" (65), gather_rows x row bytes >= passes x
 * min_bytes, and gather_rows x 100 >= ceil(nq / qt) x span x pct, qt = the query tile the filter picks for nq queries over `span` rows on 256
 * compute units.  0 otherwise; negative: an argument out of range.  Needs no GPU. */
int tavb_plan_scoped_wide(int32_t nq, int32_t k, int32_t dim, int32_t dtype, int64_t gather_rows, int64_t span, int64_t min_bytes, int64_t pct);

/* Whether a masked batch takes the 128/256-query filter tile + rescoring (tavb_search_masked_wide) under option "mask_wide" = 1; the arguments
 * of tavb_plan_masked.  1 when the corpus is fp16 and the route serves the shape (dim <= 16384, 1 <= k <= TAVB_MAX_FUSED_K), nq is at least the
 * shipped default of "mfma_min_batch" (65: the unmasked dispatcher's own bound for that tile), allowed x row bytes >= min_bytes, and
 * ceil(nq / 8) x allowed x 100 >= ceil(nq / qt) x span x pct, qt = the query tile (128 or 256) the filter picks for nq queries over `span` rows
 * on 256 compute units.  0 otherwise (an fp32 corpus: always); negative: an argument out of range.  Where this and tavb_plan_masked both say
 * 1 the binding takes this route.  A pure function, needs no context and no GPU. */
int tavb_plan_masked_wide(int32_t nq, int32_t k, int32_t dim, int32_t dtype, int64_t allowed, int64_t span, int64_t min_bytes, int64_t pct);

#ifdef __cplusplus
}
#endif
#endif /* TAVB_H */
