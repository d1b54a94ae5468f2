// Host-side declarations shared by the translation units of libtavb.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/tavb.h"

#define TAVB_MAX_GROUPED_QUERIES 128  // most queries of one grouped streaming launch (ScanParams::group)

namespace tavb {

struct ScanParams {
  const void* corpus;      // [rows, dim] row-major, f32 or f16
  const int32_t* row_ids;  // optional gather list (subset search): position -> row
  const float* queries;    // device, f32 [nq, dim]
  unsigned long long* lists;  // out: [nq, blocks, k] sorted keys, one list per workgroup
  int64_t n_pos;           // number of candidate positions (rows, or subset length)
  int32_t dim;
  int32_t dtype;  // TAVB_F32 / TAVB_F16
  int32_t nq;     // 1..TAVB_MAX_STREAM_QUERIES; with `group` > 0: 1..TAVB_MAX_GROUPED_QUERIES
  int32_t k;      // 1..TAVB_MAX_FUSED_K
  uint32_t index_base;  // added to the position before it is packed into the key
  unsigned long long key_bound;  // exclusive upper bound on accepted keys (~0 = none): paging cursor
  // grouped form (small corpora, 2 .. 128 queries in ONE launch): gridDim.y = ceil(nq / group) query groups, workgroup (x, y) scans the rows
  // of workgroup x for queries y * group .. -- `group` (1, 2, 4 or 8) queries per pass of a wave over a row, as many passes over the (L2-resident)
  // rows as there are groups.  The launch order puts workgroup (x, y) on XCD x % 8 whatever y (gridDim.x a multiple of 8): every group finds the
  // rows of "its" x in that XCD's L2 after the first one read them.  0 = the plain form (gridDim.y = 1, nq <= TAVB_MAX_STREAM_QUERIES).
  int32_t group;
  float min_score[TAVB_MAX_GROUPED_QUERIES];  // one per query (the plain form reads the first TAVB_MAX_STREAM_QUERIES)
  // score pass of a large-k lookup (launch_scan_topk, plain form only): instead of selecting, every row's score goes to topk_scores [nq][n_pos]
  // (kScoreNone: did not pass) and every passing score is counted in topk_hist [nq][topk_buckets] (topk_bucket with topk_lo / topk_scale)
  unsigned* topk_scores;
  unsigned* topk_hist;
  int32_t topk_buckets;
  float topk_lo[TAVB_MAX_STREAM_QUERIES];
  float topk_scale[TAVB_MAX_STREAM_QUERIES];
  // scoped batch (launch_scan_scoped, plain form only): [n_pos] bytes, bit q of byte p = query q of the pass may take position p
  // (launch_scope_member); read by no other launch
  const uint8_t* scope_member;
  // scoped score pass (launch_scan_topk_scoped, launch_scan_top_messages_scoped): query q of the launch is bit scope_bit0 + q of a membership byte -- the launch's queries
  // may be a sub-group of the pass the bytes were written for
  int32_t scope_bit0;
  // score pass of a top-messages lookup (launch_scan_top_messages, plain form only): topk_scores is msg_best [nq][n_messages], zeroed by the
  // caller; a passing row whose message row_to_msg[row] lies in [0, n_messages) raises that message's slot (MessageMaxSink, tavb_scan.hip)
  const int32_t* row_to_msg;
  int64_t n_messages;
};

struct ScanGeometry {
  int blocks;
  int waves;   // per block
  int unroll;  // rows in flight per wave
  int nt;      // non-temporal loads
  int pipe;    // software prefetch
  int tier;    // 0 auto, 1 fixed, 2 vector, 3 scalar
};

// returns hipSuccess or the launch error; `*tier_used` reports the kernel family chosen
hipError_t launch_scan(const ScanParams& p, const ScanGeometry& g, hipStream_t stream, int* tier_used);

// single 1536-wide query handed over INSIDE the kernel arguments (`host_query`: 1536 floats on the host; `p.queries` is not read): no copy in front of
// the launch.  Returns false -- nothing launched -- when the shape or geometry has no such variant; otherwise `*err` is the launch result.
bool launch_scan_inline_query(const ScanParams& p, const ScanGeometry& g, hipStream_t stream, const float* host_query, int* tier_used, hipError_t* err);

// the score pass of a large-k lookup (tavb_scan.hip): p.nq (1 .. TAVB_MAX_STREAM_QUERIES) queries, index_base 0, the streaming kernels'
// arithmetic row for row -- the scores are those the fused selection sees, bit for bit -- with ScanParams::topk_* as the output
hipError_t launch_scan_topk(const ScanParams& p, const ScanGeometry& g, hipStream_t stream, int* tier_used);
// the score pass of a scoped large-k or sorted batch (tavb_scan.hip): launch_scan_topk over p.row_ids, the ascending row list of the union of
// the pass' scopes, with p.scope_member / p.scope_bit0 set (scope_bit0 + nq <= 8) -- a position whose member bit is clear gets kScoreNone
// for that query and is counted nowhere; a member's score and bucket are launch_scan_topk's.  Vector tier for aligned rows, else scalar.
hipError_t launch_scan_topk_scoped(const ScanParams& p, const ScanGeometry& g, hipStream_t stream, int* tier_used);
// the score pass of a top-messages lookup (tavb_scan.hip): launch_scan_topk's kernels, tiers and per-row arithmetic over the corpus or over
// p.row_ids (n_pos positions), with the MessageMaxSink in place of the ScoreSink -- nothing is written per row; p.topk_scores [nq][n_messages]
// (zero when the pass starts) ends with, per query and message, 1 + the score bits of the message's best passing row, 0 where no row of
// it passed.  p.row_to_msg covers every row the pass visits; p.topk_hist / p.topk_buckets are unused (0): launch_message_hist counts afterwards.
hipError_t launch_scan_top_messages(const ScanParams& p, const ScanGeometry& g, hipStream_t stream, int* tier_used);
// the score pass of a scoped top-messages batch (tavb_scan.hip): launch_scan_top_messages over p.row_ids, the ascending row list of the
// union of the pass' scopes, with p.scope_member / p.scope_bit0 set (scope_bit0 + nq <= 8) -- a position whose member bit is clear does
// nothing for that query; a member raises its message's slot as launch_scan_top_messages does.  Vector tier for aligned rows, else scalar.
hipError_t launch_scan_top_messages_scoped(const ScanParams& p, const ScanGeometry& g, hipStream_t stream, int* tier_used);
// one pass of a scoped batch (tavb_scan.hip): p.nq (1 .. TAVB_MAX_STREAM_QUERIES; 4 for k > 64) queries over p.row_ids, the ascending row
// list of the union of their scopes, index_base 0; query q is offered position pos only when bit q of p.scope_member[pos] is set.
// Otherwise launch_scan's plain form: the same lists at p.lists, the same per-row arithmetic on the vector or the scalar tier.
hipError_t launch_scan_scoped(const ScanParams& p, const ScanGeometry& g, hipStream_t stream, int* tier_used);
// queries per scoped pass: TAVB_MAX_STREAM_QUERIES (4 for k > 64), halved until they fit the vector tier's LDS wherever ONE query of this
// corpus runs on the vector tier -- a pass then has the single-query lookup's per-row arithmetic at every width
int scoped_queries_per_pass(const void* corpus, int dim, int dtype, int k, const ScanGeometry& g);
// queries per score pass that keep the vector tier's LDS (queries + histograms) within budget: 1, 2, 4 or 8
int topk_queries_per_pass(int dim, int dtype, int buckets);

// After the score pass of `nq` queries over n_pos positions: boundary search, refinement, compaction and the exact finish -> out_keys
// [nq][k] (sorted best first, zero-filled) and out_rounds [nq] (refinement rounds each query needed), both device-writable (pinned host
// memory).  Workspace: topk_workspace_bytes(); the score pass's histograms [nq][buckets] lead it, and its first topk_head_bytes() bytes
// must be zero when the score pass starts (one memset).  tavb_topk.hip
struct TopkLaunch {
  const unsigned* scores;  // [nq][n_pos]
  void* workspace;
  int64_t n_pos;
  int32_t nq, k, buckets, cap, rounds;  // rounds: refinement launches enqueued (topk_refine_rounds)
  int32_t blocks;                      // workgroups per query of the refinement and compaction passes
  float lo[TAVB_MAX_STREAM_QUERIES], scale[TAVB_MAX_STREAM_QUERIES];
  unsigned long long* out_keys;
  int32_t* out_rounds;
  uint32_t index_base;  // added to the position packed into every key that leaves (0: positions; the device-resident forms: ordinal_base)
};
constexpr int kTopkRefineBuckets = 4096;  // sub-buckets of one refinement round
size_t topk_workspace_bytes(int nq, int k, int buckets, int cap, int rounds);
size_t topk_head_bytes(int nq, int buckets, int rounds);
int topk_refine_rounds(int64_t n_pos, int cap);
// refinement round r (0 .. rounds - 1; returns at once for a query whose boundary already fits `cap`), then the compaction, then the finish
hipError_t launch_topk_refine(const TopkLaunch& t, int round, hipStream_t stream);
hipError_t launch_topk_compact(const TopkLaunch& t, hipStream_t stream);
hipError_t launch_topk_finish(const TopkLaunch& t, hipStream_t stream);
// Between launch_scan_top_messages and the launches above (t.n_pos = n_messages, positions = message ordinals): best [nq][n_pos], the
// array t.scores names, is decoded in place -- 1 + score bits -> score bits, 0 -> kScoreNone -- and every message that has a score is counted
// in the workspace's histograms with topk_bucket over t.lo / t.scale, as the ScoreSink counts rows.  One launch; t.buckets <= 4096.
hipError_t launch_message_hist(const TopkLaunch& t, unsigned* best, hipStream_t stream);

// Merge of LONG sorted lists (any k up to TAVB_MAX_LARGE_K; launch_merge stops at TAVB_MAX_FUSED_K): n_lists (1 .. 64) lists of k keys per
// query, sorted descending and zero-padded, [n_lists, nq, k] or query-major [nq, n_lists, k] -> out [nq, k], the best k of their union,
// sorted and zero-padded (device or device-writable pinned memory).  Real keys must be unique.  A query one of whose lists leads with
// TAVB_KEY_PEER_FAILED gets that key in every slot.  tavb_topk.hip
hipError_t launch_merge_topk(const unsigned long long* lists, int n_lists, int nq, int k, bool query_major, unsigned long long* out,
                             hipStream_t stream);
// out[0 .. n) = value, with vector stores (out: device or device-writable pinned memory)
hipError_t launch_fill_keys(unsigned long long* out, int64_t n, unsigned long long value, hipStream_t stream);
// the rows [q * k, (q + 1) * k) of out [nq][k] whose flags[q] (device) is set = value; the other rows stay as they are
hipError_t launch_fill_flagged_rows(unsigned long long* out, int nq, int k, unsigned long long value, const unsigned* flags, hipStream_t stream);
// First half of the merge of TOP-MESSAGES lists (keys carrying message ordinals, one list per shard: a message may stand in several): for the
// queries [q0, q0 + n) of lists laid out as launch_merge_topk takes them (nq queries in all; n <= TAVB_MAX_STREAM_QUERIES), every non-zero
// key raises best [n][n_messages] (zeroed by the caller) at its message to 1 + its score bits -- what launch_scan_top_messages leaves, so
// that launch_message_hist and the selection follow unchanged.  Keys whose message is >= n_messages are dropped.  flags [n] (device; written
// for every query): 1 where a list of the query leads with TAVB_KEY_PEER_FAILED -- such a query raises nothing.  tavb_topk.hip
hipError_t launch_message_keys_max(const unsigned long long* lists, int n_lists, int nq, int k, bool query_major, int q0, int n, int64_t n_messages,
                                   unsigned* best, unsigned* flags, hipStream_t stream);

// The sorted route (tavb_search_sorted) over the same score pass and workspace head, after the refinement rounds (t.k: any 1 .. n_pos,
// n_pos = every survivor; t.out_keys / t.out_rounds unused): sorted_count writes, per query and block of positions, how many keys lie at
// or above the boundary range's lower end (counts [nq][blocks], blocks fixed by n_pos) and meta [q][0] = need, [q][1] = rounds (the
// workspace head, tavb_topk.hip Layout); sorted_compact writes query q's keys to out [0 .. sum of its counts) in ascending position order.
hipError_t launch_sorted_count(const TopkLaunch& t, unsigned* counts, hipStream_t stream);
hipError_t launch_sorted_compact(const TopkLaunch& t, int q, const unsigned* counts, unsigned long long* out, hipStream_t stream);
int sorted_blocks(int64_t n_pos, int64_t* chunk);
inline size_t topk_meta_offset(int nq, int buckets, int rounds) {  // bytes from the workspace start to meta [nq][4] (int)
  return ((size_t)nq * buckets + (size_t)rounds * nq * kTopkRefineBuckets + (size_t)nq * 4) * 4;
}

// Descending sort of n 64-bit keys in place on the device (tavb_sort.hip): one workgroup in LDS up to small_max (<= kSortSmallMax)
// keys, beyond a stable LSD radix sort over the 8-bit digits first_pass .. 7 -- first_pass 4 when the keys arrive in descending order
// of their low 32 bits (the sorted route's position order), 0 for any keys.  Workspace: sort_workspace_bytes(n).  After a multi-pass
// sort the result lies in keys or in the workspace (decided on the device): read it through launch_sort_decode, or
// launch_sort_copy_back it into keys.
constexpr int kSortSmallMax = 16384;  // 128 KiB of LDS
struct SortJob {
  unsigned long long* keys;
  int64_t n;
  int first_pass;
  void* workspace;
  int small_max;
  bool multi;  // set by launch_sort_desc
};
size_t sort_workspace_bytes(int64_t n);
hipError_t launch_sort_desc(SortJob& j, hipStream_t stream);
// sorted keys [off, off + len) -> ords [0, len) (position + base) and scs [0, len) (score bits), e.g. pinned host memory
// map (optional, map_len entries): the positions are those of a row list, and ords = map[position] + base
hipError_t launch_sort_decode(const SortJob& j, int64_t off, int64_t len, int64_t base, int64_t* ords, float* scs, hipStream_t stream,
                              const int32_t* map = nullptr, int64_t map_len = 0);
hipError_t launch_sort_copy_back(const SortJob& j, hipStream_t stream);

// every row with score >= min_score[0] (and key < key_bound), unsorted: out[0 .. *counter) (entries past `capacity` are dropped, still counted)
hipError_t launch_scan_emit(const ScanParams& p, int blocks, unsigned long long* out, unsigned long long capacity, unsigned long long* counter,
                            hipStream_t stream);

// lists: [n_lists, nq, k] (list-major) or [nq, n_lists, k] (query-major) sorted keys -> out [nq, k]
hipError_t launch_merge(const unsigned long long* lists, int n_lists, int nq, int k, bool query_major,
                        unsigned long long* out, hipStream_t stream);
// the same over a device-side work list: query slot s is merged only if s < *active, into out[scatter[s]] (scatter == nullptr: out[s])
hipError_t launch_merge_scatter(const unsigned long long* lists, int n_lists, int nq, int k, const int* active, const int* scatter,
                                unsigned long long* out, hipStream_t stream);

// keys carrying list positions -> keys carrying base + map[position], src -> dst (the same array: in place) (tavb_misc.hip)
hipError_t launch_remap_positions(const unsigned long long* src, unsigned long long* dst, int64_t n, const int32_t* map, int64_t map_len, uint32_t base,
                                  hipStream_t stream);

// Rows of the corpus as queries (tavb_rows_query.hip).  rows_to_queries: corpus rows positions[j] (each in [0, rows); anything else gives a row
// of zeros) -> out [n, dim] float32, fp16 rows widened exactly.  drop_self: lists in [n][k + 1] (with_self) of sorted, zero-padded keys carrying
// index_base + row -> out [n][k] without the key of row index_base + positions[q], the gap closed, the first k kept, + counts [n] (optional:
// keys left per query); without with_self the lists hold k keys, nothing is removed (in == out allowed) and only the counts are written.
hipError_t launch_rows_to_queries(const void* corpus, bool f16, int64_t rows, int dim, const int32_t* positions, int64_t n, float* out, hipStream_t stream);
hipError_t launch_drop_self(const unsigned long long* in, bool with_self, const int32_t* positions, uint32_t index_base, int64_t n, int k,
                            unsigned long long* out, int32_t* counts, hipStream_t stream);

// Near-duplicate self-join (tavb_pairs_join.hip; geometry, work list and the bound are described there).  launch_pairs_join: rows16 = the n x dim
// fp16 operand (16-byte aligned, dim a multiple of 64), mask optional (packed, word aligned), thr the inclusive admission threshold on the
// approximate score; *counter (zeroed by the caller) counts every admitted pair, the first `capacity` of them are stored at cand as
// (uint32 i, uint32 j).  n_tiles / work / per_wg are filled in by the launcher.  launch_rescore_pairs: counters[0] = that count, counters[1]
// (zeroed by the caller) = the pairs whose exact score reaches min_score, compacted to out_i / out_j / out_s (room for `capacity` each);
// nothing is scored when the count passed the capacity.
struct PairsJoinParams {
  const void* rows16;
  int64_t n;
  int32_t dim;
  const uint32_t* mask;
  float thr;
  unsigned long long capacity;
  unsigned long long* counter;
  uint2* cand;
  int64_t n_tiles, work, per_wg;
};
bool pairs_join_supported(int dim);
hipError_t launch_pairs_join(PairsJoinParams p, int n_cu, hipStream_t stream);
hipError_t launch_rescore_pairs(const void* corpus, bool f32_rows, int dim, unsigned long long* counters, unsigned long long capacity, const void* cand,
                                float min_score, uint32_t* out_i, uint32_t* out_j, float* out_s, int n_cu, hipStream_t stream);
// The join's one bound and its threshold, in float32 as query_prepare_kernel computes its own (the derivation heads tavb_pairs_join.hip):
// norm_sq = the cached maxima {max ||x16||^2, max ||x - x16||^2}.  delta is +inf where it is not finite (nothing can be proven).
inline float pairs_join_delta(const float norm_sq[2], int dim) {
  const float R = __builtin_sqrtf(norm_sq[0]), E = __builtin_sqrtf(norm_sq[1]);
  const float d = 0.5f * (E * R * 1.0001f + E * (R + E) * 1.0001f + 2.0f * (float)(dim / 8 + 8) * 5.9604645e-8f * (R + E) * (R + E)) + 1.2e-7f;
  return (d < __builtin_inff()) ? d : __builtin_inff();
}
inline float pairs_join_threshold(float min_score, float delta) {
  const float lo = min_score - 2.0f * delta;
  if (!(lo > 0.0f)) return -__builtin_inff();
  uint32_t bits;
  __builtin_memcpy(&bits, &lo, sizeof bits);
  --bits;  // one ulp down, as the filter's own threshold
  float t;
  __builtin_memcpy(&t, &bits, sizeof t);
  return t;
}

// Row masks (tavb_mask.hip). mask_expand: bits (uint32 words, row r = bit r & 31 of word r >> 5; bits at or beyond `rows` ignored) -> out
// [0 .. min(total, cap)) = the set rows ascending, *total_out = their number (device-writable memory, e.g. pinned); counts: workspace of
// mask_blocks(rows) words.  Two launches, grids fixed by `rows`.  mask_pack: bytes [rows] (non-zero = set) -> those words.
int mask_blocks(int64_t rows);
hipError_t launch_mask_expand(const uint32_t* bits, int64_t rows, unsigned* counts, int32_t* out, int64_t cap, long long* total_out,
                              hipStream_t stream);
hipError_t launch_mask_pack(const uint8_t* bytes, int64_t rows, uint32_t* bits, hipStream_t stream);
// mask_from_messages: the mask of a scope of messages -- row r set when 0 <= row_to_msg[r] < n_bits and the accept bitmap (launch_accept_bitmap's
// words over n_bits message ordinals) has that message's bit -> every word of (rows + 31) / 32, the bits at or beyond `rows` ZERO.  One launch.
hipError_t launch_mask_from_messages(const int32_t* row_to_msg, int64_t rows, const uint32_t* accept_bits, int64_t n_bits, uint32_t* bits,
                                     hipStream_t stream);
// Scope algebra (tavb_mask.hip).  Both kernels write every word of the mask (tail bits zero) and, per chunk of TAVB_MASK_ROWS_PER_WORKGROUP
// rows, counts[chunk] (mask_count_kernel's layout: launch_mask_write may follow) and info[chunk] (device-writable memory, e.g. pinned).
// One launch of mask_blocks(rows) workgroups each.
struct MaskChunkInfo {
  uint32_t count;
  int32_t first, last;  // the chunk's first and last set row; count == 0: INT32_MAX and -1
};
// the merged intervals of a scope: collection c is intervals [offset[c], offset[c + 1]) of `intervals` ({start, end} pairs, disjoint, ascending)
struct ScopeCollections {
  int32_t n;
  int32_t offset[TAVB_MAX_SCOPE_COLLECTIONS + 1];
};
struct MaskOperands {
  const uint32_t* m[TAVB_MAX_MASK_OPERANDS];
  int32_t n, op;
};
// row_to_msg == nullptr: the rows domain (x = r); else x = row_to_msg[r], allowed only when 0 <= x < n_messages
hipError_t launch_mask_from_ranges(const int32_t* intervals, const ScopeCollections& cols, const int32_t* row_to_msg, int64_t n_messages, int64_t rows,
                                   uint32_t* bits, unsigned* counts, MaskChunkInfo* info, hipStream_t stream);
hipError_t launch_mask_combine(const MaskOperands& ops, int64_t rows, uint32_t* bits, unsigned* counts, MaskChunkInfo* info, hipStream_t stream);
// Masks carried through a row edit (tavb_mask.hip; tavb_mask_remap): operand j is read from in[j] (old_rows rows; bits at or beyond them may hold
// anything; may be NULL when old_rows == 0) and written to out[j] (every word of new_rows rows, tail bits zero), which overlaps no input and not
// the flags.  squeeze: REMOVE -- flags over old_rows, set = the row goes; kept_counts: launch_compact_count's over them, and the kept rows must
// number new_rows (the caller has checked).  Memset + two launches.  spread: INSERT -- flags over new_rows, set = a hole that takes `fill`;
// clear_counts: launch_compact_count's over them, and the clear bits must number old_rows -- or, flags == NULL, APPEND: the holes are the rows
// [old_rows, new_rows).  One launch.  Both leave counts[j * mask_blocks(new_rows) + chunk] (launch_mask_write's input) and info[the same]
// (device-writable memory) per output.  1 <= new_rows; nothing waits on another workgroup.
struct RemapOperands {
  const uint32_t* in[TAVB_MAX_MASK_OPERANDS];
  uint32_t* out[TAVB_MAX_MASK_OPERANDS];
  int32_t n;
};
hipError_t launch_mask_remap_squeeze(const RemapOperands& ops, const uint32_t* flags, const unsigned* kept_counts, int64_t old_rows, int64_t new_rows,
                                     unsigned* counts, MaskChunkInfo* info, hipStream_t stream);
hipError_t launch_mask_remap_spread(const RemapOperands& ops, const uint32_t* flags, const unsigned* clear_counts, int64_t old_rows, int64_t new_rows, bool fill,
                                    unsigned* counts, MaskChunkInfo* info, hipStream_t stream);
// mask_expand's second launch alone, over counts one of the two kernels above (or its own count pass) wrote
hipError_t launch_mask_write(const uint32_t* bits, int64_t rows, const unsigned* counts, int32_t* out, int64_t cap, long long* total_out,
                             hipStream_t stream);
// Scoped batches (tavb_mask.hip): member[p] = the scopes of rows[p], p < n -- bit j set when mask ops.m[j] (j < ops.n; ops.op unused) holds
// row rows[p]; bits from ops.n on are zero.  rows: n valid rows of masks over `n_rows` rows.  One launch.
hipError_t launch_scope_member(const MaskOperands& ops, const int32_t* rows, int64_t n, int64_t n_rows, uint8_t* member, hipStream_t stream);
// Scoped batches on the 32/64-query tile (tavb_mask.hip): the membership planes of up to kScopePlaneMasks masks over `rows` rows for
// the rows [span_begin, span_begin + stride) -- span_begin and stride multiples of 32 -- planes[b * stride + r - span_begin], b < n_blocks: bit
// i = mask 32 b + i (i < ms.n - 32 b) holds row r and r <= last_row (< rows); every other bit zero, whatever the masks' last words hold behind
// `rows`.  Every one of the n_blocks * stride words is written.  One launch.
constexpr int kScopePlaneMasks = 64;  // masks per launch: one 64-query tile (two blocks of 32)
struct ScopeMasks {
  const uint32_t* m[kScopePlaneMasks];
  int32_t n;
};
hipError_t launch_scope_planes(const ScopeMasks& ms, int n_blocks, int64_t rows, int64_t span_begin, int64_t last_row, int64_t stride, uint32_t* planes,
                               hipStream_t stream);
// Row compaction (tavb_mask.hip; `bits` names the rows to REMOVE).  compact_count: counts[chunk] = the chunk's KEPT rows, info[chunk] = that
// count and the chunk's first and last removed row (device-writable memory).  compact_gather: the kept rows of src rows [r0, r1) -> dst rows
// from (kept rows in [from, r0)) on, densely and in order; from <= r0, both multiples of 64, r1 a multiple of 64 or `rows`; src and dst
// must not overlap.  compact_scatter: staging rows [0, kept in [r0, r1)) -> corpus rows from (kept in [0, r0)) on.  One launch each;
// row_bytes even; nothing waits on another workgroup.
hipError_t launch_compact_count(const uint32_t* bits, int64_t rows, unsigned* counts, MaskChunkInfo* info, hipStream_t stream);
hipError_t launch_compact_gather(const void* src, void* dst, const uint32_t* bits, const unsigned* counts, int64_t rows, int64_t from, int64_t r0,
                                 int64_t r1, int64_t row_bytes, hipStream_t stream);
hipError_t launch_compact_scatter(const void* staging, void* corpus, const uint32_t* bits, const unsigned* counts, int64_t rows, int64_t r0, int64_t r1,
                                  int64_t row_bytes, hipStream_t stream);
// Row expansion (tavb_mask.hip; `bits` covers the NEW `rows` and names the HOLES; counts: launch_compact_count's over the same mask, so
// "kept" reads "clear bit" = an old row).  expand_stage: the old rows of new rows [r0, r1) -- corpus rows [clear bits in [0, r0), clear bits
// in [0, r1)) -> staging rows from 0 on.  expand_scatter: src rows from (clear bits in [from, r0)) on -> the rows of dst rows [r0, r1) whose
// bit is clear, in order; holes are left as they are.  The same rules for from, r0, r1 and row_bytes as above; src and dst must not overlap.
hipError_t launch_expand_stage(const void* corpus, void* staging, const uint32_t* bits, const unsigned* counts, int64_t rows, int64_t r0, int64_t r1,
                               int64_t row_bytes, hipStream_t stream);
hipError_t launch_expand_scatter(const void* src, void* dst, const uint32_t* bits, const unsigned* counts, int64_t rows, int64_t from, int64_t r0,
                                 int64_t r1, int64_t row_bytes, hipStream_t stream);
// Scattered row writes (tavb_mask.hip).  scatter_check: *bad = 1 (memory the device can write; zeroed by the caller) when a position is outside
// [0, rows).  scatter_rows: fp32 device rows src [n, dim] -> corpus rows positions[j] (unique), converted as launch_f32_to_f16 converts; rows
// below norm_rows also get their fp16 shadow row (shadow != NULL: sdim halves per row) and fold their norms into stats (the cached maxima).
hipError_t launch_scatter_check(const int32_t* positions, int64_t n, int64_t rows, int* bad, hipStream_t stream);
hipError_t launch_scatter_rows(const float* src, int64_t n, int dim, const int32_t* positions, int64_t rows, void* corpus, bool f16, void* shadow, int sdim,
                               int64_t norm_rows, float* stats, hipStream_t stream);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize), once per (device, kernel) (tavb_misc.hip)
hipError_t ensure_dynamic_lds(const void* kernel, int bytes);

// fault injection: holds the stream for `ms` milliseconds (tavb_misc.hip)
hipError_t launch_stall(int ms, hipStream_t stream);

// chunk-row hits -> message hits (tavb_misc.hip)
hipError_t launch_accept_bitmap(const int32_t* msgs, int64_t n, uint32_t* bits, int64_t n_bits, hipStream_t stream);
hipError_t launch_message_rerank(const unsigned long long* hits, int nq, int k, uint32_t index_base, const int32_t* pos_to_row, const int32_t* row_to_msg,
                                 int64_t n_rows, const uint32_t* accept_bits, int64_t n_bits, int max_messages, unsigned long long* out,
                                 hipStream_t stream);

// exact fp32-query semantics for the 256-query tile (tavb_rescore.hip)
hipError_t launch_corpus_max_norm(const void* rows_f16, int64_t n, int dim, float* out_sq, hipStream_t stream);
// The prologue of the wide path in one launch (tavb_rescore.hip::query_prepare_kernel): nq live queries, slots up to nq_pad zeroed.
// q16 may be null (rows_only: the filter uses the exact queries, only the rows' rounding enters the bound)
// band (optional, [nq_pad]): 2 * delta, the width of the band selection
// frag_major: q16 in MFMA-fragment-major order for 256-query tiles (tavb_mfma_wide.hip, BD) instead of row-major
// min_scores: device [nq], the callers' thresholds per query (float32 values, NaN allowed) -- or, ms_fill: ONE threshold for the whole batch,
//   written to ms_out / ms_floor_out [nq_pad] (+inf for the padding) by this launch
// aux (optional): [3][nq_pad] ints zeroed (band counts, lost levels, verdicts); flag64 (optional): 64 ints zeroed (the work list's header)
hipError_t launch_query_prepare(const float* q, int nq, int nq_pad, int dim, const float* min_scores, bool rows_only, const float* max_norm_sq, void* q16,
                                float* delta, float* thr, float* band, hipStream_t stream, bool frag_major, int* aux, int* flag64, bool ms_fill, float ms_value,
                                float ms_floor, float* ms_out, float* ms_floor_out);
// candidates [nq, stride] (+ cand_cnt [nq]: band mode, the set is complete by construction unless incomplete[q]; cand_cnt == nullptr: the
// sorted best `stride` = 64 by approximate score, complete when rank 63 + delta < the exact k-th best) -> exact top k [nq, k]
// (*n_flagged must be zero when the launch starts: the prologue's flag64)
hipError_t launch_rescore(const void* corpus, bool f32_rows, int dim, uint32_t index_base, const float* queries, const unsigned long long* approx,
                          int stride, const int* cand_cnt, const int* incomplete, const float* delta, const float* min_scores, int nq, int k,
                          unsigned long long* out, int* n_flagged, int* flagged, hipStream_t stream, const int* gate = nullptr, int gate_max = 0);
// the same scoring over the device-side work list of flagged queries: slot s (live when s < *slot_active, slot_min < *slot_active <= slot_max) holds
// the candidates an exact tile ranked highest for query slot_query[s] (cand [n_slots, stride]; cand_cnt [n_slots] or nullptr = `stride` each);
// their best k by the streaming kernels' arithmetic go to row slot_query[s] of out [nq, k]
hipError_t launch_rescore_slots(const void* corpus, bool f32_rows, int dim, uint32_t index_base, const float* queries, const unsigned long long* cand,
                                int stride, const int* cand_cnt, const float* min_scores, int n_slots, int k, unsigned long long* out,
                                const int* slot_query, const int* slot_active, int slot_min, int slot_max, hipStream_t stream);
// (gate: device-side counter; when *gate > gate_max there are no candidates -- the last filter phase was skipped -- and EVERY query is flagged)
hipError_t launch_shadow_convert(const float* rows_f32, int64_t n, int dim, void* out_f16, int out_pitch /*halves per shadow row*/, float* stats /*[2]*/, hipStream_t stream);
// seed / delta (optional, [nq]): the filter's cut per query and its error bound -- the exact fallbacks' admission thresholds start from seed - 2 delta;
// band_out (optional, [cap]) <- band_v: the band width of every slot of the wide exact form
hipError_t launch_gather_flagged_f32(const float* queries, int dim, const float* min_scores, const int* n_flagged, const int* flagged, int cap, float* out,
                                     float* thr, const float* seed, const float* delta, hipStream_t stream);
hipError_t launch_gather_flagged(const float* queries, int dim, const float* min_scores, const int* n_flagged, const int* flagged, int cap, void* hi, void* lo,
                                 float* thr, const float* seed, const float* delta, float* band_out, float band_v, hipStream_t stream);

hipError_t launch_normalize_f32(const float* in, float* out, int64_t rows, int dim, hipStream_t stream);
hipError_t launch_f32_to_f16(const float* in, void* out, int64_t count, hipStream_t stream);
hipError_t launch_f32_split_f16(const float* in, void* hi, void* lo, int64_t count, hipStream_t stream);

// MFMA batched scan (f16 corpus, f16 queries staged by the launcher)
struct MfmaParams {
  const void* corpus;   // f16 [rows, dim] row-major (skinny kernel: f32 or f16)
  const void* queries;  // f16 [nq_padded, dim] device
  unsigned long long* lists;  // out [nq, n_splits, k]
  unsigned long long* workspace;  // candidate buffers, mfma_workspace_bytes() bytes
  int* counts;                    // 256-query tile only: [n_splits * nq_padded] keys left per candidate buffer (the tile writes no lists)
  int64_t rows;
  int32_t dim;
  int32_t nq;
  int32_t nq_padded;
  int32_t k;
  uint32_t index_base;
  float min_score;
  int32_t n_splits;  // row ranges the corpus is cut into (one list per (query, split))
  int32_t list_stride;  // lists per query in `lists`; 0 = n_splits (extra slots are the caller's, e.g. a carried-over top-k)
  int32_t sched;     // measurement: staging schedule of the 256-query tile (1, 2); 9 = 64-byte K steps in the 32/64-query tile
  int32_t ablate;    // measurement only (garbage results): see launch_mfma_scan
  const float* thr_in;  // optional per-query admission thresholds (device, [nq_padded]) from the earlier ladder phases
  const int* active;    // optional: device-side count of live queries (query tiles past it return at once) -- a fixed-shape launch over a work list
  int32_t active_min;   // ... and the whole launch returns at once unless active_min < *active <= active_max (0 = no upper bound)
  int32_t active_max;
  const int* gate;      // 256-query kernel only, optional: device-side counter; the launch returns at once when *gate > gate_max
  int32_t gate_max;
  int32_t bdirect;      // 256-query kernel only: `queries` are in MFMA-fragment-major order and go straight from L2 into registers (no LDS staging)
  int64_t split_plane;  // 256-query kernel only: > 0 = the SPLIT form, queries = [2][nq_padded][dim] fp16 planes this many bytes apart (q = hi + lo)
  int32_t f32;          // skinny kernel only: corpus and queries are fp32 (else fp16)
  int32_t skinny_tile;  // skinny kernel only: queries per tile, 32 or 64
  int32_t wide_tile;    // 128/256-query kernel only: queries per tile, 128 or 256 (0 = 256)
  const float* band;    // 128/256-query kernel only, optional [nq_padded]: band selection (keep every key within band[q] of the k-th best)
  unsigned* lost;       // ... [nq_padded]: atomicMax of the score level (bits) below which a query lost band rows to a buffer that could not hold its band
  int32_t shape;        // 256-query filter tile: 16 = v_mfma_f32_16x16x32_f16, anything else = v_mfma_f32_32x32x16_f16 (see mfma_tile_shape)
  // optional (the skinny kernel; the shipping filter variants of the 128/256-query kernel): allow-mask (tavb.h "row masks"), the word that holds the bit of row 0 of `corpus` -- the launch's first row must
  // be a multiple of 32 in the mask's numbering, so that bit 0 of that word IS row 0.  Rows whose bit is clear are never candidates.
  const uint32_t* mask;
  // optional (the skinny kernel; the shipping filter variants of the 128/256-query kernel; never together with `mask`): one scope PER QUERY as membership planes (launch_scope_planes) -- the word
  // of row 0 of `corpus` in the plane of query block 0 (64-byte aligned, a multiple of 32 rows into the planes), scope_stride words (a multiple
  // of 32, at least `rows` rounded up to 32) from one block's plane to the next; nq_padded / 32 planes.  A row is a candidate of query q only
  // where bit q & 31 of its word in plane q >> 5 is set.
  const uint32_t* scope_planes;
  int64_t scope_stride;
  // optional (the skinny kernel's four ring variants; with `mask` or without, never with scope_planes or a work list): the TOP-MESSAGES form --
  // msg_best [nq_padded or more][n_messages], zero when the launch starts: an admitted (row, query) pair raises the slot of the row's message to
  // 1 + the bits of its clamped score (MessageMaxSink's encoding; launch_message_hist follows).  msg_map: the map entry of row 0 of `corpus`
  // (64-byte aligned), msg_map_rows (>= rows) entries readable from there; entries outside [0, n_messages) are skipped.  No candidates and no
  // lists: workspace, lists and k are unused; thresholds never rise (min_score and thr_in as given).
  const int32_t* msg_map;
  unsigned* msg_best;
  int64_t msg_map_rows;
  int64_t n_messages;
};
hipError_t launch_mfma_scan(const MfmaParams& p, hipStream_t stream);
int mfma_tile_shape(const MfmaParams& p);  // M = N of the MFMA the 128/256-query kernel launch_mfma_scan picks for p runs on: 16 or 32
hipError_t launch_sample_thresholds(const unsigned long long* keys, int nq, int k, const float* floor, float* thr, hipStream_t stream);
int mfma_query_tile(int nq);              // queries per workgroup tile: 128 where that leaves less padding (<= 128, 257..384, 513..640 queries), else 256
int mfma_query_tile_for(int nq, int64_t rows, int n_cu);  // ... and 128 on a corpus so small that 256-query tiles leave half of the CUs idle
int mfma_pick_splits(int64_t rows, int nq_padded, int tile, int n_cu);
bool mfma_supported(int dim, int k);
size_t mfma_workspace_bytes(int n_splits, int nq_padded, bool wide);
// the BAND of every query (all keys within band[q] of its k-th best; at most kc_max, else the strict best k) over the 128/256-query tile's
// candidate buffers (+ an optional carried-over band [nq, kc_max] / carried_cnt [nq]) -> out [nq, kc_max] unsorted, out_cnt [nq];
// thr_out[q] = just below the band's cut (or floor[q]); lost [nq]: highest score level (bits) at which band rows were dropped so far
// (in/out); verdict (optional, last phase) [nq]: 1 = the band handed over is not provably complete; tavb_select.hip
constexpr int kBandMax = 2048;  // most candidates per query the rescoring accepts (kc_max <= kBandMax: the context's "band_max" option; also the most the select
                                // kernel's cache keeps when it cuts mid-stream).  1024 until round 6: a band of 1500 near-duplicates cost a 2x exact pass
hipError_t launch_select_band(const unsigned long long* cand, const int* counts, int n_splits, int nq, int nq_padded, int k, int kc_max,
                              const unsigned long long* carried, const int* carried_cnt, const float* floor, const float* band, unsigned long long* out,
                              int* out_cnt, float* thr_out, unsigned* lost, int* verdict, hipStream_t stream, const int* active = nullptr,
                              int active_min = 0, int active_max = 0x7fffffff, const int* gate = nullptr, int gate_max = 0, int* doomed = nullptr,
                              int doom_limit = 0);
// 32-query tiles at HBM speed, fp32 or fp16 corpora (same parameter block; `queries` in the corpus dtype)
hipError_t launch_skinny_scan(const MfmaParams& p, hipStream_t stream);
int skinny_kernel_id(const MfmaParams& p);  // the instantiation launch_skinny_scan picks for p: variant * 10000 + K step in bytes * 100 + queries per tile
int skinny_query_tile(int nq);  // 32, or 64 for batches of 33 and more
int skinny_pick_splits(int64_t rows, int nq_padded, int tile, int n_cu, int dim, bool f32, int sched);
bool skinny_supported(int dim, int k, bool f32);

}  // namespace tavb
