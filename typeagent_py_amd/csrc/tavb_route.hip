// Routing of a device-resident query batch (tavb_search_device_dispatch): the grouped one-launch form and its cost model, the streaming
// passes, the tile kernels (tavb_mfma_wide.hip, tavb_mfma_skinny.hip) behind the threshold ladder, the wide tile as an exact filter with its rescoring and fallbacks
// (tavb_rescore.hip) -- and the two pure planning functions of the C ABI that expose its decisions.  Host code only.

#include "tavb_ctx.h"

using namespace tavb::host;

namespace tavb {
namespace host __attribute__((visibility("hidden"))) {

tavb::ScanGeometry clamped_geometry(const tavb_ctx* c) {
  tavb::ScanGeometry g = c->geom;
  if (g.waves < 1) g.waves = 1;
  if (g.waves > 16) g.waves = 16;
  return g;
}

tavb::ScanParams scan_params(const tavb_ctx* c, const float* d_q, const int32_t* d_rows, int64_t n_pos, int nq, int k, uint32_t index_base,
                             u64_t key_bound, u64_t* lists, const float* min_scores, int fill) {
  tavb::ScanParams p{};
  p.corpus = c->corpus;
  p.row_ids = d_rows;
  p.queries = d_q;
  p.lists = lists;
  p.n_pos = n_pos;
  p.dim = c->dim;
  p.dtype = c->dtype;
  p.nq = nq;
  p.k = k;
  p.index_base = index_base;
  p.key_bound = key_bound;
  for (int i = 0; i < fill; ++i) p.min_score[i] = (i < nq) ? min_scores[i] : INFINITY;
  return p;
}

// Shape of a grouped one-launch lookup (tavb_search_batch on a small corpus, 2 .. 128 queries; ScanParams::group) and whether it is expected to
// beat the tiles.  Fitted to tools/group_sweep.py on MI355X (profiles/r06_group_sweep.md: rows 1000 .. 40000, D = 384 / 1536 / 3072, k = 10 at
// min_score 0 and k = 50 at 0.85), all in us per host-synchronous call:
//  * queries per group: ONE on fp16 corpora (1536-wide rows: the query stays in registers) and for up to ~10k (row, query) pairs, two on fp32
//    corpora beyond -- the smaller the group, the less a workgroup does besides reading rows (query staging, one 16-wave list merge per query),
//    and the rows are L2 / Infinity-Cache resident from the second group on;
//  * one workgroup per CU in all (256); two (512) for groups of two when one would walk a wave over more than ~6 row pairs;
//  * both routes pay 20 + 0.4 nq around their kernels on the host-synchronous call (staging and H2D copy of the queries, host merges / decode);
//  * grouped: 12 (launch + synchronise) + c x (rows x nq / 1000) for the scan, c = 0.08 / 0.19 / 0.41 (fp32) and 0.08 / 0.14 / 0.34 (fp16) at
//    D = 384 / 1536 / 3072 (with temporal row loads; a fifth more with the evict-first hint the single-query scan uses), + 0.6 per 1000 list
//    keys beyond 5000 (their way over PCIe and the host merge);
//  * the tiles (32/64-query tile, wide tile over the shadow) depend on how many rows survive `min_score` (fp16, 64 queries over 1000 rows: 154 at
//    min_score 0, 77 at 0.85) -- the estimate sits between the two: 35 + 0.035 D - 0.2 nq on fp32 corpora, 18 + 0.008 D + 0.4 nq on fp16 ones.
//    Up to 4 queries (2 on fp16) the alternative is the plain one-launch form or the streaming passes: the grouped form is never slower there;
//  * k <= 64 only (the 64-deep lists are what was measured).
DirectGroupPlan plan_direct_group(const tavb_ctx* c, int nq, int k, int full_blocks, bool host) {
  const bool f16 = c->dtype == TAVB_F16;
  DirectGroupPlan p{};
  p.group = (f16 || (double)c->rows * nq <= 10000.0) ? 1 : 2;
  if (c->direct_group > 0) p.group = (int)c->direct_group;
  const int n_groups = (nq + p.group - 1) / p.group;
  int wgs = (p.group >= 2 && (double)c->rows * n_groups / (256.0 * 32.0) > 6.0) ? 512 : 256;
  if (c->direct_group_wgs > 0) wgs = (int)c->direct_group_wgs;
  // lists: nq x blocks x k keys over PCIe into pinned memory (`direct_group_keys`, 32768 = 256 KiB); blocks in whole rounds of the eight XCDs
  // (the device-resident form keeps its lists in device memory and merges them with a second launch: no such budget)
  int blocks = host ? (int)std::min<int64_t>(full_blocks, c->direct_group_keys / ((int64_t)k * nq)) : full_blocks;
  // whole rounds of the XCDs, within `wgs` in all (3 groups of 88 = 264 workgroups leave 8 CUs with two: 39 us against 27 for 4 groups of 64) --
  // except that 15 per group are 16, not 8 (33 groups of two at 512)
  const int per_group = wgs / n_groups;
  blocks = std::min(blocks, std::max(8, per_group >= 12 && per_group < 16 ? 16 : per_group / 8 * 8));
  p.blocks = blocks >= 8 ? blocks / 8 * 8 : blocks;
  if (p.blocks < 1 || (p.blocks < 8 && p.blocks != full_blocks)) return p;  // (worth = false)
  const double d = c->dim, wide = std::max(0.0, d - 1536.0);
  const double per_kpair = f16 ? 0.065 + 0.00005 * d + 0.00008 * wide : 0.045 + 0.000095 * d + 0.00005 * wide;
  const double keys = (double)nq * p.blocks * k;
  // what both routes pay around their kernels on the host-synchronous call (staging + H2D copy of the queries, Python-free part of the call);
  // the device-resident form pays a second launch (the merge) instead of the lists' way over PCIe
  const double around = host ? 20.0 + 0.4 * nq : 0.0;
  const double grouped_us = around + 12.0 + (host ? 0.0006 * std::max(0.0, keys - 5000.0) : 0.0) + per_kpair * ((double)c->rows * nq / 1000.0);
  // (device-resident form, measured as back-to-back submissions: 32 queries over 1000 fp32 rows 109 -> 18 us, 64 over 1000 fp16 rows 112 -> 20)
  const double tiles_us = around + (host ? (f16 ? 18.0 + 0.008 * d + 0.4 * nq : 35.0 + 0.035 * d - 0.2 * nq)
                                         : (f16 ? 0.85 * (22.0 + 0.008 * d + 0.8 * nq) : 38.0 + 0.03 * d));
  p.worth = c->direct_group > 0 || (host && nq <= (f16 ? 2 : 4)) || grouped_us <= tiles_us;
  return p;
}

int scan_blocks_for(const tavb_ctx* c, int64_t n_pos, int waves, int unroll) {
  int blocks = c->geom.blocks > 0 ? c->geom.blocks : c->n_cu;
  const int64_t per_block = (int64_t)waves * unroll;
  const int64_t needed = (n_pos + per_block - 1) / per_block;
  if (needed < blocks) blocks = (int)std::max<int64_t>(needed, 1);
  return blocks;
}

// Core: queries on device (f32 [nq, dim]) -> sorted key lists d_out [nq, k] (async on the stream).
int search_device_impl(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/,
                       const int32_t* d_row_ids, int64_t n_pos, uint32_t index_base, u64_t* d_out,
                       u64_t key_bound) {
  if (!c->corpus && c->rows != 0) return fail(TAVB_E_NO_CORPUS, "no corpus set (call tavb_set_corpus first)");
  if (n_pos <= 0) {
    TAVB_HIP(hipMemsetAsync(d_out, 0, (size_t)nq * k * sizeof(u64_t), c->stream));
    return TAVB_OK;
  }
  const int per_pass = (k > 64) ? 4 : TAVB_MAX_STREAM_QUERIES;
  tavb::ScanGeometry g = clamped_geometry(c);
  g.blocks = scan_blocks_for(c, n_pos, g.waves, g.unroll);
  const size_t list_bytes = (size_t)per_pass * g.blocks * k * sizeof(u64_t);
  int rc = c->d_lists.reserve(list_bytes);
  if (rc) return rc;
  for (int q0 = 0; q0 < nq; q0 += per_pass) {
    const int n = std::min(per_pass, nq - q0);
    const tavb::ScanParams p = scan_params(c, d_q + (size_t)q0 * c->dim, d_row_ids, n_pos, n, k, index_base, key_bound, reinterpret_cast<u64_t*>(c->d_lists.ptr),
                                           min_scores + q0, TAVB_MAX_STREAM_QUERIES);
    {
      Timed t(c, TAVB_KERNEL_SCAN);
      hipError_t e = tavb::launch_scan(p, g, c->stream, &c->last_tier);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "scan kernel launch failed: %s", hipGetErrorString(e));
    }
    {
      Timed t(c, TAVB_KERNEL_MERGE);
      hipError_t e = tavb::launch_merge(p.lists, g.blocks, n, k, /*query_major=*/true, d_out + (size_t)q0 * k, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "merge kernel launch failed: %s", hipGetErrorString(e));
    }
  }
  return TAVB_OK;
}

// A scoped batch (tavb_search_scoped_batch and its twins), in WAVES of passes.  A wave's unions are enqueued first (mask_combine_kernel, OR:
// one launch each, which also leaves the per-chunk counts the write pass starts from and the chunks' infos in pinned memory), ONE
// synchronise brings their counts, and only then is anything sized: the row lists and the membership bytes of the wave's passes share two
// workspaces of exactly the unions' total length.  Per pass then: the write pass, the membership bytes, the scoped scan, the merge, the
// remap -- five launches, nothing waited for.  No mask word visits the host.
// A wave is at most kScopedWavePasses passes (128 queries) and at most kScopedWavePositions union positions in the worst case (every union
// the whole corpus), which bounds the workspaces whatever the batch: rows / 8 bytes of union mask per pass of the wave, 5 bytes per union
// position -- at most 2 x rows + 5 x max(64M, rows) bytes, about 0.34 GB for any corpus of up to 64M rows, and only when every scope is
// dense; the workspaces grow to what the largest wave so far needed and are released with the context.
// Batches of up to a wave synchronise once for their counts; longer ones once per wave.
constexpr int kScopedWavePasses = 16;
constexpr int64_t kScopedWavePositions = (int64_t)64 << 20;

// The unions of one wave (nq queries, at most kScopedWavePasses passes of per_pass; masks at the wave's first query): one
// mask_combine launch per pass, the ONE synchronise of the wave, the unions' sizes and -- unless every union is empty -- the two
// workspaces of exactly their total length.
int scope_wave_unions(tavb_ctx* c, int nq, int per_pass, const uint32_t* const* masks, ScopeWave* w) {
  static_assert(TAVB_MAX_STREAM_QUERIES <= TAVB_MAX_MASK_OPERANDS, "a pass' masks are the operands of one mask_combine launch and the bits of one membership byte");
  const int passes = (nq + per_pass - 1) / per_pass;
  const int64_t rows = c->rows, n_words = (rows + 31) >> 5;
  const int chunks = tavb::mask_blocks(rows);
  w->nq = nq;
  w->per_pass = per_pass;
  w->passes = passes;
  if (int rc = c->d_scope_bits.reserve((size_t)passes * n_words * sizeof(uint32_t))) return rc;
  if (int rc = c->d_mask_counts.reserve((size_t)passes * chunks * sizeof(unsigned))) return rc;
  constexpr size_t info_at = kScopedWavePasses * sizeof(long long);  // (fixed: the totals of an earlier, longer wave never lie under this wave's infos)
  if (int rc = c->h_scope.reserve(info_at + (size_t)passes * chunks * sizeof(tavb::MaskChunkInfo))) return rc;
  uint32_t* const bits = reinterpret_cast<uint32_t*>(c->d_scope_bits.ptr);
  unsigned* const counts = reinterpret_cast<unsigned*>(c->d_mask_counts.ptr);
  tavb::MaskChunkInfo* const info = reinterpret_cast<tavb::MaskChunkInfo*>(reinterpret_cast<char*>(c->h_scope.ptr) + info_at);
  for (int i = 0; i < passes * chunks; ++i) info[i].first = -1;  // (a chunk the kernel wrote holds a row or INT32_MAX here)
  w->ops.assign((size_t)passes, tavb::MaskOperands{});
  {
    Timed t(c, TAVB_KERNEL_CONVERT);
    for (int p = 0; p < passes; ++p) {
      const int q0 = p * per_pass, n = std::min(per_pass, nq - q0);
      w->ops[p].n = n;
      w->ops[p].op = TAVB_MASK_OR;
      for (int j = 0; j < n; ++j) w->ops[p].m[j] = masks[q0 + j];
      hipError_t e = tavb::launch_mask_combine(w->ops[p], rows, bits + (size_t)p * n_words, counts + (size_t)p * chunks, info + (size_t)p * chunks, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "scope union launch failed: %s", hipGetErrorString(e));
    }
  }
  TAVB_HIP(hipStreamSynchronize(c->stream));
  w->n_union.assign((size_t)passes, 0);
  w->first_pos.assign((size_t)passes, 0);
  w->total = w->most = 0;
  for (int p = 0; p < passes; ++p) {
    for (int b = 0; b < chunks; ++b) {
      const tavb::MaskChunkInfo ci = info[(size_t)p * chunks + b];
      if (ci.first < 0) return fail(TAVB_E_HIP, "chunk %d of the union of pass %d wrote no info (internal error)", b, p);
      w->n_union[p] += ci.count;
    }
    if (w->n_union[p] > rows)
      return fail(TAVB_E_HIP, "the union of pass %d counted %lld of %lld rows (internal error)", p, (long long)w->n_union[p], (long long)rows);
    w->first_pos[p] = w->total;
    w->total += w->n_union[p];
    w->most = std::max(w->most, w->n_union[p]);
  }
  if (w->total == 0) return TAVB_OK;
  if (int rc = c->d_scope_rows.reserve((size_t)w->total * sizeof(int32_t))) return rc;
  return c->d_scope_member.reserve((size_t)w->total);
}

// The row list and the membership bytes of pass p (its union is not empty): the write pass and scope_member, enqueued.
int scope_wave_lists(tavb_ctx* c, const ScopeWave& w, int p, const int32_t** list_out, const uint8_t** member_out) {
  const int64_t rows = c->rows, n_words = (rows + 31) >> 5;
  const int chunks = tavb::mask_blocks(rows);
  const uint32_t* const bits = reinterpret_cast<const uint32_t*>(c->d_scope_bits.ptr);
  const unsigned* const counts = reinterpret_cast<const unsigned*>(c->d_mask_counts.ptr);
  long long* const totals = reinterpret_cast<long long*>(c->h_scope.ptr);  // (the write passes leave their totals here; nothing reads them: a pass of
                                                                            //  an earlier wave may still be writing its own)
  int32_t* const list = reinterpret_cast<int32_t*>(c->d_scope_rows.ptr) + w.first_pos[p];
  uint8_t* const member = reinterpret_cast<uint8_t*>(c->d_scope_member.ptr) + w.first_pos[p];
  Timed t(c, TAVB_KERNEL_CONVERT);
  hipError_t e = tavb::launch_mask_write(bits + (size_t)p * n_words, rows, counts + (size_t)p * chunks, list, w.n_union[p], totals + p, c->stream);
  if (e == hipSuccess) e = tavb::launch_scope_member(w.ops[p], list, w.n_union[p], rows, member, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "scope list launch failed: %s", hipGetErrorString(e));
  *list_out = list;
  *member_out = member;
  return TAVB_OK;
}

int scoped_wave_queries(const tavb_ctx* c, int per_pass) {
  return per_pass * (int)std::min<int64_t>(kScopedWavePasses, std::max<int64_t>(1, kScopedWavePositions / std::max<int64_t>(c->rows, 1)));
}

// one wave: nq queries (at most kScopedWavePasses passes of per_pass), every pointer at the wave's first query
static int scoped_wave(tavb_ctx* c, const float* d_q, int nq, int k, int per_pass, const float* min_scores, const uint32_t* const* masks, uint32_t index_base,
                       u64_t* work, u64_t* out) {
  ScopeWave w;
  if (int rc = scope_wave_unions(c, nq, per_pass, masks, &w)) return rc;
  if (w.total == 0) return fill_empty_keys(c, out, (int64_t)nq * k);
  tavb::ScanGeometry g = clamped_geometry(c);
  if (int rc = c->d_lists.reserve((size_t)per_pass * scan_blocks_for(c, w.most, g.waves, g.unroll) * k * sizeof(u64_t))) return rc;
  for (int p = 0; p < w.passes; ++p) {
    const int q0 = p * per_pass, n = std::min(per_pass, nq - q0);
    const int64_t n_pos = w.n_union[p];
    if (n_pos == 0) {  // every scope of the pass is empty
      if (int rc = fill_empty_keys(c, out + (size_t)q0 * k, (int64_t)n * k)) return rc;
      continue;
    }
    const int32_t* list;
    const uint8_t* member;
    if (int rc = scope_wave_lists(c, w, p, &list, &member)) return rc;
    g.blocks = scan_blocks_for(c, n_pos, g.waves, g.unroll);
    tavb::ScanParams sp = scan_params(c, d_q + (size_t)q0 * c->dim, list, n_pos, n, k, 0u, ~0ull, reinterpret_cast<u64_t*>(c->d_lists.ptr), min_scores + q0,
                                      TAVB_MAX_STREAM_QUERIES);
    sp.scope_member = member;
    {
      Timed t(c, TAVB_KERNEL_SCAN);
      hipError_t e = tavb::launch_scan_scoped(sp, g, c->stream, &c->last_tier);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "scoped scan launch failed: %s", hipGetErrorString(e));
    }
    {
      Timed t(c, TAVB_KERNEL_MERGE);
      hipError_t e = tavb::launch_merge(sp.lists, g.blocks, n, k, /*query_major=*/true, work + (size_t)q0 * k, c->stream);
      if (e == hipSuccess) e = tavb::launch_remap_positions(work + (size_t)q0 * k, out + (size_t)q0 * k, (int64_t)n * k, list, n_pos, index_base, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "merge / remap launch failed: %s", hipGetErrorString(e));
    }
  }
  return TAVB_OK;
}

int search_scoped_impl(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores, const uint32_t* const* masks, uint32_t index_base, u64_t* work,
                       u64_t* out) {
  const int per_pass = tavb::scoped_queries_per_pass(c->corpus, c->dim, c->dtype, k, clamped_geometry(c));
  const int wave = scoped_wave_queries(c, per_pass);
  for (int q0 = 0; q0 < nq; q0 += wave) {
    if (int rc = scoped_wave(c, d_q + (size_t)q0 * c->dim, std::min(wave, nq - q0), k, per_pass, min_scores + q0, masks + q0, index_base, work + (size_t)q0 * k,
                             out + (size_t)q0 * k))
      return rc;
  }
  return TAVB_OK;
}

}  // namespace host
}  // namespace tavb

namespace {

// Small corpus, 2 .. 128 device-resident queries: ONE grouped scan launch (ScanParams::group; plan_direct_group) + ONE merge launch -> d_out [nq, k]
// (async on the stream).  Bit for bit the answers of nq single-query scans.
int search_device_grouped(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, uint32_t index_base, u64_t* d_out,
                          const DirectGroupPlan& plan) {
  tavb::ScanGeometry g = clamped_geometry(c);
  g.blocks = plan.blocks;
  g.nt = 0;  // (the rows are read again by every further group: no evict-first hint)
  if (int rc = c->d_lists.reserve((size_t)nq * g.blocks * k * sizeof(u64_t))) return rc;
  tavb::ScanParams p = scan_params(c, d_q, nullptr, c->rows, nq, k, index_base, ~0ull, reinterpret_cast<u64_t*>(c->d_lists.ptr) /*[nq][blocks][k]*/,
                                   min_scores, TAVB_MAX_GROUPED_QUERIES);
  p.group = plan.group;
  {
    Timed t(c, TAVB_KERNEL_SCAN);
    hipError_t e = tavb::launch_scan(p, g, c->stream, &c->last_tier);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "scan kernel launch failed: %s", hipGetErrorString(e));
  }
  {
    Timed t(c, TAVB_KERNEL_MERGE);
    hipError_t e = tavb::launch_merge(p.lists, g.blocks, nq, k, /*query_major=*/true, d_out, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "merge kernel launch failed: %s", hipGetErrorString(e));
  }
  return TAVB_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Tile kernels (tavb_mfma_wide.hip, tavb_mfma_skinny.hip) behind the threshold ladder.
// ---------------------------------------------------------------------------------------------------------------
struct TileRun {
  bool skinny;            // 32/64-query tile (fp32 or split-fp16 queries) instead of the 256-query fp16 tile
  bool q32;               // skinny tile on an fp32 corpus
  int qt;                 // queries per tile
  int nq, nq_pad, k;
  uint32_t index_base;
  float kernel_min_score; // uniform threshold applied inside the kernel
  const float* floor;     // optional device [nq_pad]: per-query exclusive admission thresholds valid from the first row on
  const void* queries;    // operand in the kernel's layout
  const void* corpus;     // corpus operand (nullptr: the context's corpus; the fp16 shadow of an fp32 corpus for the filter pass)
  int dim;                // halves / floats per row of that operand and of `queries` (0: the context's dim; the zero-padded width of a shadow whose corpus is not a multiple of 64 wide)
  const int* active;      // optional device-side live-query count (fixed-shape launch over a work list)
  int active_min, active_max;  // ... served only when active_min < *active <= active_max (0 = no upper bound): two fallbacks share one list
  bool bdirect;           // 256-query tile: `queries` are in fragment-major order (straight from L2 into registers)
  int64_t split_plane;    // 128/256-query tile: > 0 = exact form, `queries` = [2][nq_pad][dim] fp16 planes this many bytes apart (final scores, no band)
  bool ladder;            // scan in phases of growing size (else one phase)
  // 128/256-query tile only: band selection (tavb_select.hip::select_band_kernel).  d_out then receives [nq, kBandMax] unsorted keys,
  const float* band;      // device [nq_pad]: width of the band below the k-th best
  int* band_cnt;          // device [nq]: out, keys per query in d_out
  unsigned* lost;         // device [nq_pad]: scratch (zeroed by the caller), score level below which a query lost band rows
  int* verdict;           // device [nq]: out, 1 where the band handed over is not provably complete
  // ... early verdict on the whole batch: after the phase before the last, queries whose band over the rows seen so far extrapolates to more than
  // the band buffer are counted in *doomed (zeroed by the caller); with more than doomed_max of them the last phase's launches return at once
  int* doomed;
  int doomed_max;
  // a work-list run of the 128/256-query tile (r.active: the SPLIT fallback) ends with its candidates rescored by the streaming kernels' arithmetic
  // (tavb_rescore.hip, slot mode): the callers' fp32 queries [*, dim], their thresholds [*] (device), indexed by scatter[slot]
  const float* rs_queries;
  const float* rs_min_scores;
  // the 32/64-query tile and the filter pass of the 128/256-query tile (no work-list run): an allow-mask over the corpus rows (tavb.h "row masks"; word 0 = rows 0 .. 31) and the row span [span_begin, span_end)
  // that holds every set bit, span_begin a multiple of 256: the phases run over the span instead of [0, rows) -- a contiguous time range costs its
  // own bytes -- and only rows whose bit is set are candidates.  nullptr: no mask, the whole corpus.
  const uint32_t* mask;
  int64_t span_begin, span_end;
  // instead of `mask` (the 32/64-query tile; the filter pass of the 128/256-query tile): one scope per query as membership planes
  // (launch_scope_planes) over the same span -- word 0 of a plane = row span_begin, plane_stride words from one block of 32 queries to the next
  const uint32_t* planes;
  int64_t plane_stride;
};

// Width (in score) of the band the exact fallbacks keep below their k-th best before the candidates are scored again with the streaming
// kernels' arithmetic: the two arithmetics (fp32 accumulation inside the matrix pipe vs the streaming kernels' per-lane fma chains) differ by
// a few 1e-7 on unit vectors of 1536 dimensions (measured: <= 4e-7 against float64), the hi + lo split of a query carries it to 2^-22.
// Ten times that: a row the streaming arithmetic ranks in the top k is inside the band unless the two disagree by more than 4e-6.
constexpr float kExactBand = 4e-6f;

// Phase boundaries of the threshold ladder (see run_tile_ladder): phase i scans rows [b[i], b[i+1]).  `sample_opt` / `growth` = the options
// mfma_sample_rows (0 = auto, -1 = one phase) / mfma_ladder.  A pure function of its arguments: tavb_plan_ladder() hands it to callers that
// want to know how many tile launches a lookup makes (tests/test_bench_contract.py checks the committed PMC pass against it).
std::vector<int64_t> ladder_bounds(int64_t rows, int splits, int nq_pad, bool skinny, bool ladder, int64_t sample_opt, int64_t growth) {
  std::vector<int64_t> bounds;
  bounds.push_back(0);
  // first phase: `mfma_sample_rows`, or (0 = auto) part of ONE tile per workgroup of the 128/256-query kernel -- nothing compacts while
  // everything is still being admitted, and every unfiltered row of this phase is a key the select kernel has to stream (one workgroup per
  // QUERY).  Round 2 used two tiles per workgroup (40960 rows), round 3 one (20480: 4 % faster on a 1.25M-row shard, the same on 10M rows;
  // profiles/r03_shard_ladder.md).  Round 4: with one LDS atomic per admitted row (tavb_mfma_wide.hip) the all-admitted first phase is best kept
  // to 32 ranges' worth, 10240 rows -- 1 % faster on the shard, the same on 10M rows, half the keys for the select kernel
  // (profiles/r04_cfg3_kernel.md).  (The 32/64-query tile keeps round 2's 40960 rows.)
  // One or two query tiles (up to 256 queries: 128 .. 256 row ranges) keep 64 ranges' worth: 1 - 2 % faster there (profiles/r04_raw/mid_batch.txt).
  const int64_t auto_sample = skinny ? (int64_t)std::min(splits, 64) * 320 * 2 : (int64_t)std::min(splits, nq_pad >= 512 ? 32 : 64) * 320;
  const int64_t sample = sample_opt > 0 ? (sample_opt + 255) / 256 * 256 : (sample_opt == 0 ? auto_sample : 0);
  // 32/64-query tile on corpora of a few hundred thousand to ~2M rows: the default ladder's first phases are smaller than one tile per
  // workgroup (40960 rows = 160 tiles for 512 resident workgroups) and each costs a launch + ~one tile time whatever its size; ONE seeding
  // phase of exactly one tile per workgroup, then the rest, is faster (1M x 1536 fp32, 32 queries: 1.18 -> 1.07 ms of kernels per batch,
  // profiles/r03_mid_batch.md); a single un-seeded phase is slower still (1.23 ms: every workgroup pays the cold start)
  const int64_t one_tile_each = (int64_t)splits * 256;
  if (ladder && skinny && sample_opt == 0 && rows >= 4 * one_tile_each && rows < 2048000) {
    bounds.push_back(one_tile_each);
  } else if (ladder && skinny && sample_opt == 0 && rows >= 2048000 && rows >= 32 * one_tile_each) {
    // ... and on bigger corpora THREE phases: one tile per workgroup, twelve times that, the rest (10M rows: 65536 / 851968 / 9.08M).  The
    // 32-query tile is HBM-bound and admits little (k ln(n / seen) rows per query): what its early phases cost is their launches and tails,
    // 0.62 ms for three phases over 1.02M rows against 0.51 ms for two over 0.92M (profiles/r05_mid_batch.md; one phase fewer than the
    // generic ladder below, +1.5 % on cfg3_b32)
    bounds.push_back(one_tile_each);
    if (growth > 0) bounds.push_back(13 * one_tile_each);
  } else if (ladder && sample > 0 && rows >= 8 * sample) {
    int64_t done = sample;
    bounds.push_back(done);
    while (growth > 0 && done * (growth + 1) * 2 <= rows && bounds.size() < 8) {
      done += done * growth;
      bounds.push_back(done);
    }
  } else if (ladder && !skinny && sample_opt == 0 && growth > 0 && rows >= 8 * 320 && (rows >= 12 * 2560 || rows > (int64_t)splits * 640)) {
    // the wide tile on a SMALL corpus (below eight first phases' worth: 82k rows at 1024 queries, 164k at up to 128): until the end of round 6
    // ONE un-seeded phase -- every row admitted; at 1024 queries the candidate buffers compact every other tile from the third tile of a row
    // range on (50k rows: 0.99 ms of tile kernel, twice what 100k rows took), at up to 128 queries the select kernel streams every row of the
    // corpus per query (150k rows: 0.29 ms of selection next to 0.16 ms of tile kernel).  Two phases instead: an eighth of the rows in whole
    // tiles, then the rest behind its thresholds: 1024 queries over 50k rows 1.13 -> 0.47 ms, 128 over 150k rows 0.52 -> 0.28 ms; from 30720
    // rows up (20k rows: one phase is as fast; profiles/r06_raw/small_wide.txt) -- and below that whenever a workgroup would walk more than
    // two tiles un-seeded (many query tiles leave few row ranges: 2048 queries over 20000 rows are 16 ranges of four tiles, 0.68 ms in one
    // phase against 0.44).
    bounds.push_back((rows / 8 / 320) * 320);
  }
  bounds.push_back(rows);
  return bounds;
}

// Threshold ladder.  The corpus is scanned in phases of growing size -- the first `mfma_sample_rows` rows, then
// `mfma_ladder` times everything scanned so far, ..., then the rest -- every row exactly once.  After each phase the
// exact top-k so far is merged; its k-th best score is a valid admission threshold for every later row (the k-th best
// of a subset never exceeds the k-th best of the whole corpus), so each phase starts selective instead of admitting
// whatever comes first and compacting, and the running top-k rides along as one more list of the next phase's merge.
// Expected admissions per query drop from k * rows / sample (one seeding phase) to ~k * ladder per phase.  Results do
// not depend on the phase boundaries.  Output: sorted key lists [nq, k] at `d_out` (or, with `scatter`, rows
// scatter[slot] of it for the slots below *active; a work-list run of the wide tile rescoring its band first: TileRun::rs_queries).
int run_tile_ladder(tavb_ctx* c, const TileRun& r, u64_t* d_out, const int* scatter, bool scatter_identity = false) {
  const int dim = r.dim > 0 ? r.dim : c->dim;  // of the tile's operands (the candidates' ordinals are the corpus' own either way)
  auto pick_splits = [&](int64_t rows) {
    return r.skinny ? tavb::skinny_pick_splits(rows, r.nq_pad, r.qt, c->n_cu, dim, r.q32, (int)c->mfma_sched) : tavb::mfma_pick_splits(rows, r.nq_pad, r.qt, c->n_cu);
  };
  auto launch = [&](const tavb::MfmaParams& q) { return r.skinny ? tavb::launch_skinny_scan(q, c->stream) : tavb::launch_mfma_scan(q, c->stream); };
  const int nq = r.nq, k = r.k;
  const bool wide = !r.skinny;  // the 256-query tile leaves unsorted buffers + counts, one select kernel picks the best k over them
  const bool spanned = r.mask || r.planes;
  const int64_t row_first = spanned ? r.span_begin : 0;  // the rows the phases cover: the mask's span, or the corpus
  const int64_t n_rows = (spanned ? r.span_end : c->rows) - row_first;
  if (r.planes && (r.mask || r.active)) return fail(TAVB_E_INVALID, "bad scoped tile run (internal error)");
  if (spanned && ((wide && (r.active || r.split_plane > 0)) || row_first % 256 != 0 || n_rows < 1 || r.span_end > c->rows)) return fail(TAVB_E_INVALID, "bad masked tile run (internal error)");
  const int splits = c->mfma_splits > 0 ? (int)c->mfma_splits : pick_splits(n_rows);
  if (!wide)
    if (int rc = c->d_lists.reserve((size_t)nq * (splits + 1) * k * sizeof(u64_t))) return rc;  // + the carried-over top-k
  if (int rc = c->d_cand.reserve(tavb::mfma_workspace_bytes(splits, r.nq_pad, wide))) return rc;
  if (wide)
    if (int rc = c->d_counts.reserve((size_t)splits * r.nq_pad * sizeof(int))) return rc;
  tavb::MfmaParams p{};
  p.corpus = r.corpus ? r.corpus : c->corpus;
  p.queries = r.queries;
  p.lists = reinterpret_cast<u64_t*>(c->d_lists.ptr);
  p.workspace = reinterpret_cast<u64_t*>(c->d_cand.ptr);
  p.counts = reinterpret_cast<int*>(c->d_counts.ptr);
  p.rows = n_rows;
  p.dim = dim;
  p.nq = nq;
  p.nq_padded = r.nq_pad;
  p.k = k;
  p.index_base = r.index_base;
  p.min_score = r.kernel_min_score;
  p.n_splits = splits;
  p.ablate = (int)c->mfma_ablate;
  p.sched = (int)c->mfma_sched;
  p.f32 = r.q32 ? 1 : 0;
  p.skinny_tile = r.skinny ? r.qt : 0;
  p.wide_tile = r.skinny ? 0 : r.qt;
  p.active = r.active;
  p.active_min = r.active_min;
  p.active_max = r.active_max;
  p.split_plane = r.split_plane;
  p.bdirect = r.bdirect ? 1 : 0;
  p.shape = (int)c->mfma_shape;
  const std::vector<int64_t> bounds = ladder_bounds(n_rows, splits, r.nq_pad, r.skinny, r.ladder, c->mfma_sample_rows, c->mfma_ladder);  // phase i scans rows row_first + [bounds[i], bounds[i+1])
  const int n_phases = (int)bounds.size() - 1;
  const int kc = wide ? (int)c->band_max : k;  // keys per query of the running selection between phases
  if (wide)  // (every phase's selection leaves its cut here -- the last one's seeds the exact fallbacks' admission thresholds, search_wide_exact)
    if (int rc = c->d_thr.reserve((size_t)r.nq_pad * sizeof(float))) return rc;
  if (n_phases > 1 || (wide && r.active)) {
    if (int rc = c->d_thr.reserve((size_t)r.nq_pad * sizeof(float))) return rc;
    if (int rc = c->d_sample_keys.reserve((size_t)2 * nq * kc * sizeof(u64_t) + (size_t)2 * nq * sizeof(int))) return rc;  // running selection: two copies (ping-pong) + counts
  }
  p.band = r.band;
  p.lost = r.lost;
  const float* floor = r.floor;  // per-query thresholds valid for every row
  const size_t row_bytes = (size_t)dim * (r.q32 ? 4 : 2);  // of the corpus operand
  for (int ph = 0; ph < n_phases; ++ph) {
    const bool last = (ph == n_phases - 1);
    tavb::MfmaParams pp = p;
    const int64_t ph_first = row_first + bounds[ph];
    pp.corpus = reinterpret_cast<const char*>(p.corpus) + (size_t)ph_first * row_bytes;
    pp.rows = bounds[ph + 1] - bounds[ph];
    pp.index_base = r.index_base + (uint32_t)ph_first;
    if (spanned) {  // whole words: a 32-row block of the tile's epilogue is one word of the mask (ladder_bounds gives multiples of 640 or 256; the wide tile's: of 320 or 256)
      if (ph_first % 32 != 0) return fail(TAVB_E_INVALID, "masked tile phase %d starts at row %lld, not a multiple of 32 (internal error)", ph, (long long)ph_first);
      if (r.mask) pp.mask = r.mask + (ph_first >> 5);
      if (r.planes) {  // (the planes start at the span: one word per row)
        pp.scope_planes = r.planes + (ph_first - row_first);
        pp.scope_stride = r.plane_stride;
      }
    }
    pp.n_splits = pick_splits(pp.rows);
    if (c->mfma_splits > 0 || pp.n_splits > splits) pp.n_splits = splits;  // lists / candidate buffers are sized for `splits`
    const int carried = ph > 0 ? 1 : 0;  // the running top-k of the earlier phases occupies one more list slot
    pp.list_stride = pp.n_splits + carried;
    pp.thr_in = ph > 0 ? reinterpret_cast<const float*>(c->d_thr.ptr) : floor;
    // the early verdict (r.doomed): the select launch of the phase before the last counts, the last phase's launches gate themselves on the count
    const bool doom_count = wide && r.doomed && n_phases >= 2 && ph == n_phases - 2;
    const bool doom_gate = wide && r.doomed && n_phases >= 2 && last;
    // a band of c keys over `seen` of `rows` rows grows to about c * rows / seen when its rows are spread evenly (a cluster of near-duplicates around
    // the k-th best; on ordinary data the band is k plus a key or two whatever the row count): counted when that is 1.25 x the band buffer,
    // and only with at least 16 keys beyond k in hand
    const int doom_limit = std::max(k + 15, (int)std::min<int64_t>(1 << 30, (int64_t)(1.25 * kc * (double)bounds[ph + 1] / (double)n_rows)));
    if (doom_gate) {
      pp.gate = r.doomed;
      pp.gate_max = r.doomed_max;
    }
    u64_t* const running = reinterpret_cast<u64_t*>(c->d_sample_keys.ptr);  // [2][nq][kc] (+ [2][nq] counts); not allocated for a single phase
    const u64_t* const run_in = running ? running + (size_t)((ph + 1) & 1) * nq * kc : nullptr;  // what phase ph - 1 left
    u64_t* const run_out = running ? running + (size_t)(ph & 1) * nq * kc : nullptr;
    int* const run_cnt = running ? reinterpret_cast<int*>(running + (size_t)2 * nq * kc) : nullptr;
    const int* const cnt_in = run_cnt ? run_cnt + (size_t)((ph + 1) & 1) * nq : nullptr;
    int* const cnt_out = run_cnt ? run_cnt + (size_t)(ph & 1) * nq : nullptr;
    if (carried && !wide) {
      TAVB_HIP(hipMemcpy2DAsync(pp.lists + (size_t)pp.n_splits * k, (size_t)pp.list_stride * k * sizeof(u64_t), run_in,
                                (size_t)k * sizeof(u64_t), (size_t)k * sizeof(u64_t), (size_t)nq, hipMemcpyDeviceToDevice, c->stream));
    }
    {
      Timed t(c, r.active ? TAVB_KERNEL_RESCORE : !last ? TAVB_KERNEL_MFMA_SAMPLE : (r.skinny ? TAVB_KERNEL_SKINNY : TAVB_KERNEL_MFMA));
      hipError_t e = launch(pp);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "mfma scan launch failed (phase %d): %s", ph, hipGetErrorString(e));
      if (wide && pp.split_plane == 0) c->last_mfma_shape = tavb::mfma_tile_shape(pp);
      if (!wide) c->last_skinny_kernel = tavb::skinny_kernel_id(pp);
    }
    if (wide) {
      Timed t(c, r.active ? TAVB_KERNEL_RESCORE : TAVB_KERNEL_MERGE);
      // (thresholds of the padding queries are never read: the tiles give every query past the live ones +inf themselves.  Until round 6 a
      //  memset per phase filled them with NaNs -- one launch per phase for nothing.)
      float* d_thr = reinterpret_cast<float*>(c->d_thr.ptr);
      // a work-list run (r.active: the SPLIT fallback) ends in its own band buffer; the strict best k of it is scattered to the callers' rows below
      u64_t* const last_out = r.active ? run_out : d_out;
      int* const last_cnt = r.active ? cnt_out : r.band_cnt;
      hipError_t e = tavb::launch_select_band(pp.workspace, pp.counts, pp.n_splits, nq, r.nq_pad, k, kc, carried ? run_in : nullptr, carried ? cnt_in : nullptr,
                                              floor, r.band, last ? last_out : run_out, last ? last_cnt : cnt_out, (last && r.active) ? nullptr : d_thr, r.lost,
                                              last ? r.verdict : nullptr, c->stream, r.active, r.active_min, r.active_max > 0 ? r.active_max : 0x7fffffff,
                                              doom_gate ? r.doomed : nullptr, r.doomed_max, doom_count ? r.doomed : nullptr, doom_limit);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "select launch failed: %s", hipGetErrorString(e));
      if (last && r.active) {  // the band of every live slot, scored again the streaming kernels' way: its best k go to the caller's row scatter[slot]
        e = tavb::launch_rescore_slots(c->corpus, /*f32_rows=*/false, c->dim, r.index_base, r.rs_queries, last_out, kc, last_cnt, r.rs_min_scores, nq, k, d_out,
                                       scatter, r.active, r.active_min, r.active_max > 0 ? r.active_max : 0x7fffffff, c->stream);
        if (e != hipSuccess) return fail(TAVB_E_HIP, "fallback rescore launch failed: %s", hipGetErrorString(e));
      }
    } else if (last) {
      Timed t(c, r.active ? TAVB_KERNEL_RESCORE : TAVB_KERNEL_MERGE);
      // (scatter_identity: a work-list run whose lists stay slot-indexed -- merged only for the live slots)
      hipError_t e = (scatter || scatter_identity) ? tavb::launch_merge_scatter(pp.lists, pp.list_stride, nq, k, r.active, scatter, d_out, c->stream)
                                                    : tavb::launch_merge(pp.lists, pp.list_stride, nq, k, /*query_major=*/true, d_out, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "merge launch failed: %s", hipGetErrorString(e));
    } else {
      hipError_t e = tavb::launch_merge(pp.lists, pp.list_stride, nq, k, /*query_major=*/true, run_out, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "phase merge launch failed: %s", hipGetErrorString(e));
      e = tavb::launch_sample_thresholds(run_out, nq, k, r.floor, reinterpret_cast<float*>(c->d_thr.ptr), c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "threshold launch failed: %s", hipGetErrorString(e));
    }
  }
  return TAVB_OK;
}

// The lowest threshold of a batch (NaN thresholds aside; NaN when every one is NaN): the ONE threshold a tile launch takes -- the per-query
// thresholds ride in the `floor` array.
float lowest_min_score(const float* min_scores, int nq) {
  float lo = NAN;
  for (int i = 0; i < nq; ++i)
    if (min_scores[i] == min_scores[i]) lo = (lo != lo || min_scores[i] < lo) ? min_scores[i] : lo;
  return lo;
}

// The exclusive admission floor that goes with a threshold: `score > floor` <=> `score >= min_score` (+inf for NaN / > 1: nothing passes).
float floor_of_min_score(float ms) {
  if (ms != ms || ms > 1.0f) return INFINITY;
  if (!(ms > 0.0f)) return -INFINITY;
  uint32_t bits;
  memcpy(&bits, &ms, sizeof bits);
  --bits;
  float f;
  memcpy(&f, &bits, sizeof f);
  return f;
}

// every query of the batch has the same threshold, bit for bit (a batch of NaNs is uniform)
bool uniform_min_scores(const float* min_scores, int nq) {
  for (int i = 1; i < nq; ++i)
    if (memcmp(&min_scores[i], &min_scores[0], sizeof(float)) != 0) return false;
  return true;
}

// min_scores (host, [nq]) -> c->d_minscores: [nq_pad] the thresholds themselves (padding: +inf), then [nq_pad] the exclusive admission floors
// that go with them (+inf for NaN / > 1 / padding).  A mixed batch is copied from pageable memory (staged by the runtime before the call
// returns).  A uniform one -- every caller of the reference -- needs no host buffer in flight (the device-resident forms stay asynchronous):
// *uniform_out = true, NOTHING is written here, and the caller's prologue kernel fills both arrays from the one value (query_prepare_kernel).
int upload_min_scores(tavb_ctx* c, const float* min_scores, int nq, int nq_pad, float** d_ms_out, float** d_floor_out, bool* uniform_out) {
  if (int rc = c->d_minscores.reserve((size_t)2 * nq_pad * sizeof(float))) return rc;
  float* d_ms = reinterpret_cast<float*>(c->d_minscores.ptr);
  float* d_floor = d_ms + nq_pad;
  const bool uniform = uniform_min_scores(min_scores, nq);
  if (!uniform) {
    std::vector<float> h((size_t)2 * nq_pad, INFINITY);
    for (int i = 0; i < nq; ++i) {
      h[i] = min_scores[i];
      h[(size_t)nq_pad + i] = floor_of_min_score(min_scores[i]);
    }
    TAVB_HIP(hipMemcpyAsync(d_ms, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    TAVB_HIP(hipStreamSynchronize(c->stream));  // (pageable source: be sure the runtime is done with `h` before it goes out of scope)
  }
  *d_ms_out = d_ms;
  *d_floor_out = d_floor;
  *uniform_out = uniform;
  return TAVB_OK;
}

// The 128/256-query fp16 tile as an exact filter + fp32-query rescoring of its candidates (tavb_rescore.hip).  fp32 corpora:
// the filter reads the fp16 shadow (d_shadow, reserved by the caller), the rescoring and the fallback tile the fp32 rows.
// `small` (fp32 corpora only): the filter is the 32/64-query tile over the shadow with the EXACT queries (split fp16 planes), for batches
// below the wide tile's range -- half the bytes of an fp32 pass.
// min_scores: host [nq], one threshold per query (the reference takes `min_score` per call, vectorbase.py:163-173: a batch of Q calls has Q of them).
// `mw` (fp16 corpora, not `small`): a MASKED batch -- the filter pass runs over the mask's span with the bit test in its admission path (the corpus
// max-norm bound stays valid for any subset of the rows), the rescoring as ever; neither exact fallback has a masked form, so there is no early
// verdict, and the flagged queries -- read back, one round trip -- are re-run on the gather route over the mask's resident row list.
// `sw` (the same, never with `mw`): a SCOPED batch -- one mask per query; the filter reads the batch's membership planes, built here, and the
// flagged queries are re-run on the row-list scoped route with their own masks.
// The flagged queries of search_wide_exact's work list (d_nflag: their count, from slot 64 on their indices; `cap` slots), read back -- the one
// host round trip of this file -- and re-run on the streaming kernels, their lists scattered back into the callers' rows of d_out.  fq32: where
// their fp32 queries stand side by side -- `gathered`: already (gather_flagged_f32_kernel), else copied there from d_q here.  rows / n_rows:
// the row list the re-run goes over, its positions then remapped to index_base + row; null: the whole corpus, keys carrying index_base.
int rerun_flagged(tavb_ctx* c, const int* d_nflag, int cap, const float* d_q, float* fq32, bool gathered, int k, const float* min_scores /*host*/,
                  const int32_t* rows, int64_t n_rows, uint32_t index_base, u64_t* d_out) {
  int* h = reinterpret_cast<int*>(c->h_flag.ptr);
  TAVB_HIP(hipMemcpyAsync(h, d_nflag, (size_t)(64 + cap) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  TAVB_HIP(hipStreamSynchronize(c->stream));
  const int n_flagged = h[0] < cap ? h[0] : cap;
  if (n_flagged == 0) return TAVB_OK;
  std::vector<float> ms_f((size_t)n_flagged);
  for (int i = 0; i < n_flagged; ++i) {
    ms_f[i] = min_scores[h[64 + i]];
    if (!gathered)
      TAVB_HIP(hipMemcpyAsync(fq32 + (size_t)i * c->dim, d_q + (size_t)h[64 + i] * c->dim, (size_t)c->dim * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  }
  u64_t* d_redo = reinterpret_cast<u64_t*>(c->d_fb_cand.ptr);
  const int tier = c->last_tier;  // (the batch's route stays what "last_tier" reports: the re-run is a detail of it)
  const int rc_redo = search_device_impl(c, fq32, n_flagged, k, ms_f.data(), rows, rows ? n_rows : c->rows, rows ? 0u : index_base, d_redo);
  c->last_tier = tier;
  if (rc_redo) return rc_redo;
  if (rows) {
    const hipError_t e = tavb::launch_remap_positions(d_redo, d_redo, (int64_t)n_flagged * k, rows, n_rows, index_base, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "remap launch failed: %s", hipGetErrorString(e));
  }
  for (int i = 0; i < n_flagged; ++i)
    TAVB_HIP(hipMemcpyAsync(d_out + (size_t)h[64 + i] * k, d_redo + (size_t)i * k, (size_t)k * sizeof(u64_t), hipMemcpyDefault, c->stream));
  return TAVB_OK;
}

// The per-corpus caches brought up to the corpus' rows: the row-norm maxima (d_norm, reserved by the caller) and, from norm_rows on, the fp16
// shadow of an fp32 corpus or the zero-padded copy of an fp16 one of an odd width (`padded`; d_shadow, reserved by the caller).
int update_corpus_stats(tavb_ctx* c, bool padded) {
  const bool f32c = (c->dtype == TAVB_F32);
  float* d_norm = reinterpret_cast<float*>(c->d_norm.ptr);
  if (c->norm_rows > c->rows || c->norm_rows == 0) {  // first use on this corpus (or it shrank: the old maxima are still upper bounds, but start over)
    TAVB_HIP(hipMemsetAsync(d_norm, 0, 2 * sizeof(float), c->stream));
    c->norm_rows = 0;
  }
  if (c->norm_rows < c->rows) {  // rows appended since: extend the maxima (and the shadow)
    hipError_t e;
    const int sdim = ((c->dim + 63) / 64) * 64;  // halves per shadow row
    char* shadow_new = c->d_shadow.ptr ? reinterpret_cast<char*>(c->d_shadow.ptr) + (size_t)c->norm_rows * sdim * 2 : nullptr;
    if (f32c) {
      e = tavb::launch_shadow_convert(reinterpret_cast<const float*>(c->corpus) + (size_t)c->norm_rows * c->dim, c->rows - c->norm_rows, c->dim, shadow_new, sdim,
                                      d_norm, c->stream);
    } else {
      if (padded) {  // fp16 rows of an odd width: the same values, rows zero-padded to whole K steps
        const size_t n_new = (size_t)(c->rows - c->norm_rows);
        TAVB_HIP(hipMemsetAsync(shadow_new, 0, n_new * sdim * 2, c->stream));
        TAVB_HIP(hipMemcpy2DAsync(shadow_new, (size_t)sdim * 2, reinterpret_cast<const char*>(c->corpus) + (size_t)c->norm_rows * c->dim * 2, (size_t)c->dim * 2,
                                  (size_t)c->dim * 2, n_new, hipMemcpyDeviceToDevice, c->stream));
      }
      // (the norm kernel loads 16 bytes at a time: widths that are no multiple of 8 are read from the padded copy -- zeros add nothing to a norm)
      const bool norm_from_pad = padded && (c->dim % 8 != 0);
      e = norm_from_pad ? tavb::launch_corpus_max_norm(shadow_new, c->rows - c->norm_rows, sdim, d_norm, c->stream)
                        : tavb::launch_corpus_max_norm(reinterpret_cast<const char*>(c->corpus) + (size_t)c->norm_rows * c->dim * 2, c->rows - c->norm_rows,
                                                       c->dim, d_norm, c->stream);
    }
    if (e != hipSuccess) return fail(TAVB_E_HIP, "corpus norm / shadow launch failed: %s", hipGetErrorString(e));
    c->norm_rows = c->rows;
  }
  return TAVB_OK;
}

// ... of a SCOPED batch (search_wide_exact with `sw`): re-run on the row-list scoped route with their own masks (search_scoped_impl: what
// tavb_search_scoped_batch would have answered for them), their lists copied into the callers' rows of d_out.  *n_out: how many there were.
int rerun_flagged_scoped(tavb_ctx* c, const int* d_nflag, int cap, const float* d_q, float* fq32, int k, const float* min_scores /*host*/,
                         const uint32_t* const* masks /*host*/, uint32_t index_base, u64_t* d_out, int* n_out) {
  int* h = reinterpret_cast<int*>(c->h_flag.ptr);
  TAVB_HIP(hipMemcpyAsync(h, d_nflag, (size_t)(64 + cap) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  TAVB_HIP(hipStreamSynchronize(c->stream));
  const int n_flagged = h[0] < cap ? h[0] : cap;
  *n_out = n_flagged;
  if (n_flagged == 0) return TAVB_OK;
  std::vector<float> ms_f((size_t)n_flagged);
  std::vector<const uint32_t*> masks_f((size_t)n_flagged);
  std::vector<int> slot((size_t)n_flagged);  // (h is pinned memory the re-run may use again)
  for (int i = 0; i < n_flagged; ++i) {
    slot[i] = h[64 + i];
    ms_f[i] = min_scores[slot[i]];
    masks_f[i] = masks[slot[i]];
    TAVB_HIP(hipMemcpyAsync(fq32 + (size_t)i * c->dim, d_q + (size_t)slot[i] * c->dim, (size_t)c->dim * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  }
  u64_t* d_redo = reinterpret_cast<u64_t*>(c->d_fb_cand.ptr);
  const int tier = c->last_tier;  // (the batch's route stays what "last_tier" reports: the re-run is a detail of it)
  const int rc_redo = tavb::host::search_scoped_impl(c, fq32, n_flagged, k, ms_f.data(), masks_f.data(), index_base, d_redo, d_redo);
  c->last_tier = tier;
  if (rc_redo) return rc_redo;
  for (int i = 0; i < n_flagged; ++i)
    TAVB_HIP(hipMemcpyAsync(d_out + (size_t)slot[i] * k, d_redo + (size_t)i * k, (size_t)k * sizeof(u64_t), hipMemcpyDefault, c->stream));
  return TAVB_OK;
}

struct MaskedWide {
  const uint32_t* bits;           // the mask over the corpus rows
  int64_t span_begin, span_end;   // rows [span_begin, span_end) hold every set bit; span_begin a multiple of 256
  const int32_t* dev_rows;        // the allowed rows in ascending order (device), n_allowed of them
  int64_t n_allowed;
};
// the scoped twin: one mask per query (HOST array of nq device pointers); [first_row, last_row] holds every set bit of every mask
struct ScopedWide {
  const uint32_t* const* masks;
  int64_t first_row, last_row;
  int* n_flagged;  // out: the queries that were re-run
};
int search_wide_exact(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores, uint32_t index_base, u64_t* d_out, bool small = false,
                      const MaskedWide* mw = nullptr, const ScopedWide* sw = nullptr) {
  // candidates per query handed to the rescoring: the wide tile selects a BAND (every row within 2 delta of the approximate k-th best: as many
  // as the data makes it, up to kBandMax), the 32/64-query tile (`small`) the best 64 by approximate score
  const int KC = small ? 64 : (int)c->band_max;
  const bool f32c = (c->dtype == TAVB_F32);
  // a corpus whose width is not a multiple of 64 (the tile's K step is a whole 128-byte line): the filter -- and, on fp16 corpora, the exact
  // fallbacks -- read a zero-padded fp16 copy of the rows (d_shadow, `fdim` halves per row; for fp32 corpora the shadow they have anyway) and a
  // zero-padded copy of the queries: zeros add nothing to a dot product or a norm, the delta bound is unchanged.  The candidates are rescored
  // with the corpus' own rows and the callers' own queries.
  const bool padded = !small && (c->dim % 64 != 0);
  const int fdim = padded ? ((c->dim + 63) / 64) * 64 : c->dim;
  const bool shadow_ops = f32c || padded;  // the filter's corpus operand is d_shadow
  const bool big_k = k > 64;  // beyond what the 64-query exact tile ranks: every flagged query goes to the wide split-plane form (fp16 corpora only: the caller checked)
  const int64_t scan_rows = mw ? mw->span_end - mw->span_begin : sw ? sw->last_row + 1 - sw->first_row / 256 * 256 : c->rows;  // the rows the filter walks
  const int qt = small ? tavb::skinny_query_tile(nq) : (c->mfma_tile > 0 ? (int)c->mfma_tile : tavb::mfma_query_tile_for(nq, scan_rows, c->n_cu));
  const int nq_pad = ((nq + qt - 1) / qt) * qt;
  const bool bdirect = !small && qt == 256 && c->mfma_bdirect && c->mfma_ablate == 0;
  // Work list of queries that need an exact pass (a band that did not fit).  Few of them (<= 64): ONE pass of the 64-query exact tile.  Many: the
  // 256-query tile in its SPLIT form (fp32 queries as two fp16 planes, the K loop run once per plane: twice the MFMAs of a filter pass, exact) --
  // 16 passes of the 64-query tile per 1024 flagged queries otherwise (round 2-3: "stated, not solved").  Both are fixed-shape
  // launches over the same device-side list and return at once when it is empty or is the other one's share.  Either one hands its best rows
  // (and a small band below them) to the rescoring kernel in slot mode: a query served by a fallback gets the streaming kernels' float32 scores.
  const bool wide_fallback = !mw && !sw && !small && !f32c && c->wide_fallback && (nq >= 256 || big_k);
  // k > 64 on an FP32 corpus (end of round 6): the filter, the band and the rescoring serve any k up to TAVB_MAX_FUSED_K, but no exact tile ranks
  // more than 64 fp32 rows per query.  A flagged query -- more than band_max near-duplicates around its k-th best: rare -- is therefore re-run on
  // the streaming kernels, which takes the one host round trip of this file (the work list is read back; nothing flagged: nothing more to do).
  // Until then such batches took the streaming kernels four queries per corpus pass: 128 queries over 2M x 1536 fp32 rows, k = 65: 66 ms against 1.3.
  const bool f32_big_k = !small && f32c && big_k;
  if (big_k && !wide_fallback && !f32_big_k && !mw && !sw) return fail(TAVB_E_UNSUPPORTED, "k > 64 on the batched tile of an fp16 corpus needs the wide_fallback option");
  const int cap = wide_fallback ? ((nq + 255) / 256) * 256 : ((nq + 63) / 64) * 64;  // slots of the work list
  const size_t q16_bytes = (size_t)nq_pad * fdim * 2 * (small ? 2 : 1);  // small: high and low plane
  if (int rc = c->d_queries_f16.reserve(q16_bytes)) return rc;
  if (int rc = c->d_delta.reserve((size_t)nq_pad * 6 * sizeof(float))) return rc;  // delta, the relaxed thresholds, the band widths; band counts, lost levels, verdicts
  if (int rc = c->d_approx.reserve((size_t)nq * KC * sizeof(u64_t))) return rc;
  if (int rc = c->d_flag.reserve((size_t)(cap + 64) * sizeof(int))) return rc;
  if (int rc = c->d_fb_queries.reserve((size_t)2 * cap * fdim * 2 + (size_t)2 * cap * sizeof(float))) return rc;  // + per-slot thresholds, per-slot band widths
  const float* fq = d_q;  // the queries as the filter and the padded fallbacks read them
  if (padded) {
    if (int rc = c->d_queries_pad.reserve((size_t)nq * fdim * sizeof(float))) return rc;
    TAVB_HIP(hipMemsetAsync(c->d_queries_pad.ptr, 0, (size_t)nq * fdim * sizeof(float), c->stream));
    TAVB_HIP(hipMemcpy2DAsync(c->d_queries_pad.ptr, (size_t)fdim * sizeof(float), d_q, (size_t)c->dim * sizeof(float), (size_t)c->dim * sizeof(float), (size_t)nq,
                              hipMemcpyDeviceToDevice, c->stream));
    fq = reinterpret_cast<const float*>(c->d_queries_pad.ptr);
  }
  if (!big_k || f32_big_k)
    if (int rc = c->d_fb_cand.reserve((size_t)cap * (f32_big_k ? k : 64) * sizeof(u64_t))) return rc;
  if (f32_big_k || mw || sw)
    if (int rc = c->h_flag.reserve((size_t)(64 + cap) * sizeof(int))) return rc;
  if (mw || sw)  // the re-run's lists
    if (int rc = c->d_fb_cand.reserve((size_t)cap * k * sizeof(u64_t))) return rc;
  if (int rc = c->d_norm.reserve(256)) return rc;
  float *d_ms = nullptr, *d_ms_floor = nullptr;
  bool ms_uniform = false;
  if (int rc = upload_min_scores(c, min_scores, nq, nq_pad, &d_ms, &d_ms_floor, &ms_uniform)) return rc;
  const float ms_lo = lowest_min_score(min_scores, nq);
  float* d_norm = reinterpret_cast<float*>(c->d_norm.ptr);
  float* d_delta = reinterpret_cast<float*>(c->d_delta.ptr);
  float* d_floor = d_delta + nq_pad;
  float* d_band = d_floor + nq_pad;
  int* d_band_cnt = reinterpret_cast<int*>(d_band + nq_pad);
  unsigned* d_lost = reinterpret_cast<unsigned*>(d_band_cnt + nq_pad);
  int* d_verdict = d_band_cnt + 2 * nq_pad;
  int* d_nflag = reinterpret_cast<int*>(c->d_flag.ptr);
  int* d_flagged = d_nflag + 64;
  {
    Timed t(c, TAVB_KERNEL_RESCORE);
    if (int rc = update_corpus_stats(c, padded)) return rc;
    // ONE launch: the filter's query operand (padding slots zero), delta / relaxed thresholds / band widths, the selection's counters zeroed,
    // the work list's header zeroed, a uniform batch's thresholds filled in (round 6: a fill kernel, three memsets and this kernel until then)
    if (small) TAVB_HIP(hipMemsetAsync(c->d_queries_f16.ptr, 0, q16_bytes, c->stream));  // (the split planes' padding queries: launch_f32_split_f16 writes the live ones)
    hipError_t e = tavb::launch_query_prepare(fq, nq, nq_pad, fdim, d_ms, small, d_norm, small ? nullptr : c->d_queries_f16.ptr, d_delta, d_floor,
                                              small ? nullptr : d_band, c->stream, bdirect, d_band_cnt, d_nflag, ms_uniform, min_scores[0],
                                              floor_of_min_score(min_scores[0]), d_ms, d_ms_floor);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "query prepare launch failed: %s", hipGetErrorString(e));
    if (small) {
      e = tavb::launch_f32_split_f16(d_q, c->d_queries_f16.ptr, reinterpret_cast<char*>(c->d_queries_f16.ptr) + q16_bytes / 2, (int64_t)nq * c->dim, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "query split launch failed: %s", hipGetErrorString(e));
    }
  }
  TileRun filt{};
  filt.skinny = small;
  filt.q32 = false;
  filt.qt = qt;
  filt.nq = nq;
  filt.nq_pad = nq_pad;
  filt.k = small ? KC : k;  // the wide tile ranks by the caller's k and keeps the band below it
  filt.band = small ? nullptr : d_band;
  filt.band_cnt = small ? nullptr : d_band_cnt;
  filt.lost = small ? nullptr : d_lost;
  filt.verdict = small ? nullptr : d_verdict;
  filt.index_base = index_base;
  filt.kernel_min_score = (ms_lo > 0.0f) ? 0.0f : ms_lo;  // the per-query relaxed thresholds (floor) do the filtering; NaN stays NaN
  filt.floor = d_floor;
  filt.bdirect = bdirect;
  filt.queries = c->d_queries_f16.ptr;
  filt.corpus = shadow_ops ? c->d_shadow.ptr : nullptr;
  filt.dim = fdim;
  filt.ladder = true;
  if (mw) {
    filt.mask = mw->bits;
    filt.span_begin = mw->span_begin;
    filt.span_end = mw->span_end;
  }
  if (sw) {  // the membership planes of this batch: one per block of 32 queries of the padded batch, over the span (the padding queries' are zero)
    const int64_t stride = tavb::host::scope_plane_stride(sw->first_row, sw->last_row);
    if (int rc = c->d_scope_planes.reserve((size_t)(nq_pad / 32) * stride * sizeof(uint32_t))) return rc;
    uint32_t* const planes = reinterpret_cast<uint32_t*>(c->d_scope_planes.ptr);
    if (int rc = tavb::host::build_scope_planes(c, sw->masks, nq, nq_pad / 32, sw->first_row, sw->last_row, planes)) return rc;
    filt.planes = planes;
    filt.plane_stride = stride;
    filt.span_begin = sw->first_row / 256 * 256;
    filt.span_end = sw->last_row + 1;
  }
  // a batch MOST of whose bands are not going to fit (every query next to more near-duplicates than a band holds) is found out before the last --
  // the big -- filter phase and goes straight to the exact split-plane form: the filter's last phase, its selection and the rescoring return at once
  const bool early = wide_fallback && c->early_exact;
  filt.doomed = early ? d_nflag + 1 : nullptr;
  filt.doomed_max = nq / 2;
  c->last_shadow = shadow_ops ? 1 : 0;
  if (int rc = run_tile_ladder(c, filt, reinterpret_cast<u64_t*>(c->d_approx.ptr), nullptr)) return rc;
  char* fb = reinterpret_cast<char*>(c->d_fb_queries.ptr);
  // behind the gathered operand: fp32 [cap][dim] on fp32 corpora, two fp16 planes of [cap][fdim] otherwise (fdim, not dim: an odd width's planes are padded)
  float* fb_thr = reinterpret_cast<float*>(fb + (size_t)2 * cap * (f32c ? c->dim : fdim) * 2);
  float* fb_band = fb_thr + cap;
  {
    Timed t(c, TAVB_KERNEL_RESCORE);
    hipError_t e = tavb::launch_rescore(c->corpus, f32c, c->dim, index_base, d_q, reinterpret_cast<const u64_t*>(c->d_approx.ptr), KC,
                                        small ? nullptr : d_band_cnt, small ? nullptr : d_verdict, d_delta, d_ms, nq, k, d_out, d_nflag, d_flagged,
                                        c->stream, filt.doomed, filt.doomed_max);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "rescore launch failed: %s", hipGetErrorString(e));
    // (the exact tiles of an fp32 corpus read its own rows -- the dispatch admits only widths they take; those of an fp16 corpus of an odd
    //  width read the padded copy, which holds the same values)
    // the exact fallbacks start from what the filter has proven: the cut its last selection left in d_thr (the one before it when the early
    // verdict skipped the last phase) less the filter's error bound is a valid admission threshold on exact scores, so ONE phase each
    const float* seed = small ? nullptr : reinterpret_cast<const float*>(c->d_thr.ptr);
    if (!mw && !sw)  // (a masked or scoped batch re-runs its flagged queries from their fp32 rows in d_q: nothing to gather)
      e = f32c ? tavb::launch_gather_flagged_f32(d_q, c->dim, d_ms, d_nflag, d_flagged, cap, reinterpret_cast<float*>(fb), fb_thr, seed, d_delta, c->stream)
               : tavb::launch_gather_flagged(fq, fdim, d_ms, d_nflag, d_flagged, cap, fb, fb + (size_t)cap * fdim * 2, fb_thr, seed, d_delta,
                                             wide_fallback ? fb_band : nullptr, kExactBand, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "gather launch failed: %s", hipGetErrorString(e));
  }
  if (mw)  // their fp32 queries side by side in fb (cap x fdim x 4 bytes and more), their lists by position, then as index_base + row
    return rerun_flagged(c, d_nflag, cap, d_q, reinterpret_cast<float*>(fb), /*gathered=*/false, k, min_scores, mw->dev_rows, mw->n_allowed, index_base, d_out);
  if (sw)  // the same, each with its own mask
    return rerun_flagged_scoped(c, d_nflag, cap, d_q, reinterpret_cast<float*>(fb), k, min_scores, sw->masks, index_base, d_out, sw->n_flagged);
  if (f32_big_k)  // (gather_flagged_f32_kernel has put their fp32 queries into fb)
    return rerun_flagged(c, d_nflag, cap, d_q, reinterpret_cast<float*>(fb), /*gathered=*/true, k, min_scores, nullptr, 0, index_base, d_out);
  {  // (run_tile_ladder times its own launches, in the same bucket)
    if (!big_k) {
      // the exact tile over the work list: returns at once when the list is empty (the normal case).  It ranks 64 rows per slot whatever k: the
      // rows beyond the k-th are the band the rescoring (slot mode) re-orders with the streaming kernels' arithmetic
      TileRun ex{};
      ex.skinny = true;
      ex.q32 = f32c;
      ex.qt = 64;
      ex.nq = cap;
      ex.nq_pad = cap;
      ex.k = 64;
      ex.index_base = index_base;
      ex.kernel_min_score = ms_lo;
      ex.floor = fb_thr;
      ex.queries = fb;
      if (!f32c && padded) {
        ex.corpus = c->d_shadow.ptr;
        ex.dim = fdim;
      }
      ex.active = d_nflag;
      ex.active_min = 0;
      ex.active_max = wide_fallback ? 64 : 0;
      ex.ladder = false;
      u64_t* fb_cand = reinterpret_cast<u64_t*>(c->d_fb_cand.ptr);
      if (int rc = run_tile_ladder(c, ex, fb_cand, nullptr, /*scatter_identity=*/true)) return rc;
      Timed t(c, TAVB_KERNEL_RESCORE);
      hipError_t e = tavb::launch_rescore_slots(c->corpus, f32c, c->dim, index_base, d_q, fb_cand, 64, nullptr, d_ms, wide_fallback ? 64 : cap, k, d_out,
                                                d_flagged, d_nflag, 0, wide_fallback ? 64 : 0x7fffffff, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "fallback rescore launch failed: %s", hipGetErrorString(e));
    }
    if (wide_fallback) {
      TileRun wx{};
      wx.skinny = false;
      wx.q32 = false;
      wx.qt = 256;
      wx.nq = cap;
      wx.nq_pad = cap;
      wx.k = k;
      wx.index_base = index_base;
      wx.kernel_min_score = ms_lo;
      wx.floor = fb_thr;  // (+inf for the unused slots: they admit nothing)
      wx.band = fb_band;  // kExactBand below the k-th best: what the rescoring re-orders
      wx.queries = fb;    // [2][cap][dim]: the high plane, then the low plane
      wx.split_plane = (int64_t)cap * fdim * 2;
      if (padded) {
        wx.corpus = c->d_shadow.ptr;
        wx.dim = fdim;
      }
      wx.active = d_nflag;
      wx.active_min = big_k ? 0 : 64;
      wx.active_max = 0;
      wx.ladder = false;  // one phase, seeded by the filter's cut (fb_thr): three launches that return at once when the list is not this form's share
      wx.rs_queries = d_q;
      wx.rs_min_scores = d_ms;
      if (int rc = run_tile_ladder(c, wx, d_out, d_flagged)) return rc;
    }
  }
  return TAVB_OK;
}

// A batch on the 32/64-query tile over the corpus' own rows (no shadow): fp32 queries on an fp32 corpus, split into an fp16 high and low plane
// on an fp16 one; per-query thresholds ride as exclusive admission floors valid from the first row on.  mask (optional): the allow-mask
// over the corpus rows, whose set bits all lie in [span_begin, span_end), span_begin a multiple of 256 -- the phases run over the span with
// the bit test in the tile's admission path.  Scores are final -> sorted key lists d_out [nq, k] (async on the stream).
int run_skinny_tile(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, uint32_t index_base, u64_t* d_out,
                    const uint32_t* mask = nullptr, int64_t span_begin = 0, int64_t span_end = 0, const uint32_t* planes = nullptr, int64_t plane_stride = 0) {
  const bool q32 = c->dtype != TAVB_F16;
  const int qt = tavb::skinny_query_tile(nq);
  const int nq_pad = ((nq + qt - 1) / qt) * qt;
  const size_t plane = (size_t)nq_pad * c->dim * (q32 ? 4 : 2);
  const size_t qbytes = plane * (q32 ? 1 : 2);
  if (int rc = c->d_queries_f16.reserve(qbytes)) return rc;
  const bool uniform_thr = uniform_min_scores(min_scores, nq);
  float *d_ms = nullptr, *d_ms_floor = nullptr;
  if (!uniform_thr) {
    bool uni = false;
    if (int rc = upload_min_scores(c, min_scores, nq, nq_pad, &d_ms, &d_ms_floor, &uni)) return rc;
  }
  TAVB_HIP(hipMemsetAsync(c->d_queries_f16.ptr, 0, qbytes, c->stream));
  if (q32) {
    TAVB_HIP(hipMemcpyAsync(c->d_queries_f16.ptr, d_q, (size_t)nq * c->dim * 4, hipMemcpyDeviceToDevice, c->stream));
  } else {
    hipError_t e = tavb::launch_f32_split_f16(d_q, c->d_queries_f16.ptr, reinterpret_cast<char*>(c->d_queries_f16.ptr) + plane, (int64_t)nq * c->dim, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "query split launch failed: %s", hipGetErrorString(e));
  }
  c->last_tier = 5;
  TileRun r{};
  r.skinny = true;
  r.q32 = q32;
  r.qt = qt;
  r.nq = nq;
  r.nq_pad = nq_pad;
  r.k = k;
  r.index_base = index_base;
  r.kernel_min_score = uniform_thr ? min_scores[0] : lowest_min_score(min_scores, nq);
  r.floor = d_ms_floor;
  r.queries = c->d_queries_f16.ptr;
  r.ladder = true;
  r.mask = mask;
  r.span_begin = span_begin;
  r.span_end = span_end;
  r.planes = planes;
  r.plane_stride = plane_stride;
  return run_tile_ladder(c, r, d_out, nullptr);
}

// Room for the wide filter's fp16 operand, d_shadow: the fp16 copy of an fp32 corpus, or the zero-padded copy of rows whose width is not a
// multiple of 64 -- every row, search_wide_exact fills it in from norm_rows on.
int reserve_shadow(tavb_ctx* c) {
  const size_t need = (size_t)c->rows * (((size_t)c->dim + 63) / 64 * 64) * 2;
  if (c->d_shadow.cap >= need) return TAVB_OK;
  c->norm_rows = 0;  // reserve() does not keep the old contents
  return c->d_shadow.reserve(need);
}

}  // namespace

// tavb_lookup_pairs.hip: the self-join's operand and bound -- the maxima, and for an fp32 corpus its fp16 shadow, as the wide route builds them
int tavb::host::prepare_join_operand(tavb_ctx* c) {
  if (c->dtype == TAVB_F32)
    if (int rc = reserve_shadow(c)) return rc;
  if (int rc = c->d_norm.reserve(256)) return rc;
  Timed t(c, TAVB_KERNEL_RESCORE);
  return update_corpus_stats(c, false);
}

// Routes a device-resident query batch: streaming scan (few queries), 32/64-query tile (small batches; every batch on
// fp32 corpora), or the 256-query fp16 tile with exact rescoring (large batches on fp16 corpora).  Not part of the public ABI.
// min_scores: one threshold per query -- the tiles take them per query (a batch of Q `fuzzy_lookup_embedding` calls has Q of them,
// vectorbase.py:163-173), so a mixed batch takes the same route as a uniform one.
int tavb_search_device_dispatch(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores,
                                uint32_t index_base, u64_t* d_out) {
  const bool f16c = (c->dtype == TAVB_F16);
  c->last_direct = 0;
  {  // small corpora, 2 .. 128 queries: the grouped streaming scan + one merge where it beats the tiles (plan_direct_group)
    const int64_t bytes = (int64_t)c->rows * c->dim * (f16c ? 2 : 4);
    const bool shadow2 = !f16c && c->f32_shadow >= 2 && bytes >= c->f32_shadow_min_bytes;
    if (c->corpus && c->rows > 0 && !c->dispatch_no_group && nq >= 2 && nq <= std::min<int64_t>(c->direct_group_max_nq, TAVB_MAX_GROUPED_QUERIES) && !shadow2 &&
        c->small_direct_bytes > 0 && bytes <= c->small_direct_bytes && k <= 64) {
      const DirectGroupPlan plan = plan_direct_group(c, nq, k, scan_blocks_for(c, c->rows, clamped_geometry(c).waves, c->geom.unroll), /*host=*/false);
      if (plan.worth) {
        c->last_direct = 4;
        return search_device_grouped(c, d_q, nq, k, min_scores, index_base, d_out, plan);
      }
    }
  }
  // A staged query the tiles cannot serve (tavb_ctx.h): the WHOLE batch on the streaming kernels.  Behind the grouped scan, which is fp32
  // throughout.  Whole batch, not a re-run of the marked queries in groups of 8: that needs the per-query scatter of rerun_flagged on
  // every tile route (masked, scoped and top-messages included) for inputs no embedding produces; the price is nq / 8 corpus passes for
  // such a batch.  fp32 rows too: their tile multiplies fp32 queries, but its admission test on the raw dot product drops the rows an
  // infinite query scores 0.0, and one rule for both dtypes keeps the answer the scan's wherever the flag is up.
  if (staged_overflow(c, d_q)) {
    c->last_shadow = 0;
    return search_device_impl(c, d_q, nq, k, min_scores, nullptr, c->rows, index_base, d_out);
  }
  // the wide tile keeps a band below the k-th best (any k the fused selections serve: the reference's max_matches = 50, convsettings.py:61-63,
  // included).  Its flagged queries need an exact tile: the 64-query one up to k = 64, beyond that the wide split-plane form (fp16 corpora).
  // A width that is not a multiple of 64 (the tile's K step) rides the wide tile on a zero-padded copy of the rows (search_wide_exact): any
  // width on fp16 corpora (the exact fallbacks read the padded copy too: the same values), multiples of 16 on fp32 ones (their exact
  // tile reads the corpus' own fp32 rows).
  const bool odd_width = c->dim % 64 != 0;
  const int wide_dim = ((c->dim + 63) / 64) * 64;
  // (round 6: ANY width on fp16 corpora -- the rescoring reads rows that are not 16-byte aligned element by element, in the scalar streaming
  //  kernel's order)
  const bool width_ok = !odd_width || f16c || c->dim % 16 == 0;
  const bool exact_tile = (k <= 64) ? ((f16c && odd_width) ? tavb::skinny_supported(wide_dim, k, false) : tavb::skinny_supported(c->dim, k, !f16c))
                                    : (f16c ? c->wide_fallback != 0 : true);  // (fp32, k > 64: flagged queries are re-run on the streaming kernels)
  const int64_t corpus_bytes = (int64_t)c->rows * c->dim * (f16c ? 2 : 4);
  // k > 64: the 32/64-query tile does not serve it and the streaming kernels take FOUR such queries per corpus pass -- from 9 queries (more than two
  // passes), or 3 on corpora of mfma_big_bytes and more, the wide tile (32 queries over 2M x 1536 fp16 rows, k = 65: 12.5 ms against 1.3)
  const bool big_k_batch = k > 64 && (nq >= 9 || (nq >= 3 && corpus_bytes >= c->mfma_big_bytes));
  // (narrow rows: the streaming scan's cost per row does not shrink with the row -- 3 queries over 1M x 384 fp32 rows 0.39 ms against 0.28 on the
  //  wide tile, profiles/r06_raw/regime_sweep_d384.md -- so the byte thresholds measured at D = 1536 scale down with the width)
  const int64_t few_bytes_f32 = c->dim < 1536 ? c->mfma_few_bytes_f32 / 1536 * c->dim : c->mfma_few_bytes_f32;
  const bool wide_batch = nq >= c->mfma_min_batch || big_k_batch || (nq >= c->mfma_min_batch_big && corpus_bytes >= c->mfma_big_bytes) ||
                          (!f16c && nq >= c->mfma_min_batch_f32) ||
                          (!f16c && nq >= c->mfma_min_batch_big_f32 && corpus_bytes >= c->mfma_big_bytes_f32) ||
                          (!f16c && nq >= 2 && c->mfma_min_batch_big_f32 <= 64 && corpus_bytes >= few_bytes_f32);
  bool wide = (f16c || c->f32_shadow) && c->corpus && wide_batch && width_ok && tavb::mfma_supported(wide_dim, k) && c->rows > 0 && exact_tile;
  // f32_shadow = 2: smaller batches (and single queries) on big fp32 corpora filter on the shadow too, with the 32/64-query tile
  // (it keeps the best 64 candidates per query: k up to 48 leaves the slack the completeness test needs)
  bool shadow_small = !wide && !f16c && c->f32_shadow >= 2 && c->corpus && nq <= 64 && tavb::mfma_supported(c->dim, 64) && k <= 48 &&
                      tavb::skinny_supported(c->dim, k, false) && (int64_t)c->rows * c->dim * 4 >= c->f32_shadow_min_bytes;
  if ((wide || shadow_small) && (!f16c || odd_width))  // the filter needs the fp16 shadow / padded copy; without the memory for it the other kernels serve the batch
    if (reserve_shadow(c) != TAVB_OK) wide = shadow_small = false;
  c->last_shadow = 0;
  if (shadow_small) {
    c->last_tier = 5;
    return search_wide_exact(c, d_q, nq, k, min_scores, index_base, d_out, /*small=*/true);
  }
  // 32/64-query tiles at HBM speed: small batches on fp16 corpora, every batch from `skinny_min_batch_f32` up on fp32 ones
  const bool skinny = !wide && c->corpus && c->rows > 0 && tavb::skinny_supported(c->dim, k, !f16c) &&
                      nq >= (f16c ? ((c->dim <= 768 && c->rows >= 200000) ? std::min<int64_t>(2, c->skinny_min_batch_f16) : c->skinny_min_batch_f16)
                                  : c->skinny_min_batch_f32);  // (two queries over 1M x 384 fp16 rows: 0.23 ms on the streaming scan, 0.17 on the tile)
  if (wide) {
    c->last_tier = 4;  // 1-3 = streaming tiers, 4 = 256-query MFMA tile, 5 = 32/64-query MFMA tile
    return search_wide_exact(c, d_q, nq, k, min_scores, index_base, d_out);
  }
  if (skinny) return run_skinny_tile(c, d_q, nq, k, min_scores, index_base, d_out);  // (last_tier = 5)
  return search_device_impl(c, d_q, nq, k, min_scores, nullptr, c->rows, index_base, d_out);
}

namespace tavb {
namespace host __attribute__((visibility("hidden"))) {
// Masked batch on the 32/64-query tile (tavb_search_masked_batch / tavb_search_masked_device; the callers have checked the arguments and that
// skinny_supported holds): run_skinny_tile over the span of the mask.
int search_masked_tile(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores, const uint32_t* dev_bits, int64_t first_row, int64_t last_row,
                       uint32_t index_base, u64_t* d_out) {
  c->last_shadow = 0;
  c->last_direct = 0;
  c->masked_route = 2;
  if (staged_overflow(c, d_q)) {  // (tavb_ctx.h) the row-list scoped route, every query under the one mask
    const std::vector<const uint32_t*> masks((size_t)nq, dev_bits);
    return search_scoped_impl(c, d_q, nq, k, min_scores, masks.data(), index_base, d_out, d_out);
  }
  return run_skinny_tile(c, d_q, nq, k, min_scores, index_base, d_out, dev_bits, first_row / 256 * 256, last_row + 1);
}

// A scoped batch on the 32/64-query tile (tavb_search_scoped_tile and its twins; the callers have checked the arguments and that
// skinny_supported holds), in WAVES of query tiles: a wave's membership planes are built (one scope_planes_kernel launch per 64 queries) and
// its tile ladder runs over the span of the union, then the next wave reuses the workspace -- everything on the one stream, nothing waited
// for.  A plane is 4 bytes per row of the span per 32 queries, so a wave is as many 64-query tiles as fit kScopeWavePlaneBytes of planes (at
// least one): at 1M rows 8 MiB per tile, 8 tiles = 512 queries per wave.  64 MiB: what a wave costs beyond its tiles' passes is one
// ladder's launches (about ten), which eight passes over any span that fills the budget outweigh many times; a longer wave would only
// grow the workspace.  The workspace is max(64 MiB, 8 bytes x span rows) whatever the batch.
constexpr int64_t kScopeWavePlaneBytes = (int64_t)64 << 20;

int64_t scope_plane_stride(int64_t first_row, int64_t last_row) { return ((last_row + 32) & ~(int64_t)31) - first_row / 256 * 256; }

// the planes of masks[0 .. n) (HOST array of device pointers), padded to n_blocks blocks of 32, at `planes`: one launch per 64 masks
int build_scope_planes(tavb_ctx* c, const uint32_t* const* masks, int n, int n_blocks, int64_t first_row, int64_t last_row, uint32_t* planes) {
  const int64_t span_begin = first_row / 256 * 256, stride = scope_plane_stride(first_row, last_row);
  Timed t(c, TAVB_KERNEL_CONVERT);
  for (int b0 = 0; b0 < n_blocks; b0 += tavb::kScopePlaneMasks / 32) {
    const int blocks = std::min(tavb::kScopePlaneMasks / 32, n_blocks - b0);
    tavb::ScopeMasks ms{};
    ms.n = std::max(0, std::min(32 * blocks, n - 32 * b0));
    for (int j = 0; j < ms.n; ++j) ms.m[j] = masks[32 * b0 + j];
    if (ms.n == 0) {  // (blocks of padding only: a batch the caller padded beyond a tile)
      TAVB_HIP(hipMemsetAsync(planes + (size_t)b0 * stride, 0, (size_t)blocks * stride * sizeof(uint32_t), c->stream));
      continue;
    }
    hipError_t e = tavb::launch_scope_planes(ms, blocks, c->rows, span_begin, last_row, stride, planes + (size_t)b0 * stride, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "scope plane launch failed: %s", hipGetErrorString(e));
  }
  return TAVB_OK;
}

int scope_plane_blocks(int n) { return tavb::skinny_query_tile(n) == 32 ? 1 : ((n + 63) / 64) * 2; }

int search_scoped_tile(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores, const uint32_t* const* masks, int64_t first_row, int64_t last_row,
                       uint32_t index_base, u64_t* d_out) {
  c->last_shadow = 0;
  c->last_direct = 0;
  c->last_topk_refine = 0;
  c->topk_rounds_pending = 0;
  c->masked_route = 5;
  if (staged_overflow(c, d_q)) return search_scoped_impl(c, d_q, nq, k, min_scores, masks, index_base, d_out, d_out);  // (tavb_ctx.h)
  const int64_t stride = scope_plane_stride(first_row, last_row);
  const int64_t tile_bytes = 2 * stride * (int64_t)sizeof(uint32_t);
  const int wave = 64 * (int)std::max<int64_t>(1, std::min<int64_t>(kScopeWavePlaneBytes / tile_bytes, 1 << 20));
  for (int q0 = 0; q0 < nq; q0 += wave) {
    const int n = std::min(wave, nq - q0), n_blocks = scope_plane_blocks(n);
    if (int rc = c->d_scope_planes.reserve((size_t)n_blocks * stride * sizeof(uint32_t))) return rc;
    uint32_t* const planes = reinterpret_cast<uint32_t*>(c->d_scope_planes.ptr);
    if (int rc = build_scope_planes(c, masks + q0, n, n_blocks, first_row, last_row, planes)) return rc;
    if (int rc = run_skinny_tile(c, d_q + (size_t)q0 * c->dim, n, k, min_scores + q0, index_base, d_out + (size_t)q0 * k, nullptr, first_row / 256 * 256, last_row + 1,
                                 planes, stride))
      return rc;
  }
  return TAVB_OK;
}

// Top messages on the 32/64-query tile (tavb_search_top_messages_tile; search_top_messages_tile_impl groups the queries and runs the
// selection): the queries staged as run_skinny_tile stages them (fp32 rows: as they are; fp16 rows: split into a high and a low plane), the
// per-query thresholds as exclusive admission floors, ONE launch over the span of the mask -- launch_skinny_scan's row ranges and XCD mapping;
// no sample pass and no phases, there is no threshold to hand on.  The measurement variants of "mfma_sched" have no top-messages form: only
// 9 (64-byte K steps) is passed on.
int top_messages_tile_pass(tavb_ctx* c, const float* d_q, int n, const float* min_scores, const uint32_t* dev_bits, int64_t first_row, int64_t last_row,
                           unsigned* best) {
  const bool q32 = c->dtype != TAVB_F16;
  const int qt = tavb::skinny_query_tile(n);
  const int nq_pad = ((n + qt - 1) / qt) * qt;
  const size_t plane = (size_t)nq_pad * c->dim * (q32 ? 4 : 2);
  const size_t qbytes = plane * (q32 ? 1 : 2);
  if (int rc = c->d_queries_f16.reserve(qbytes)) return rc;
  const bool uniform_thr = uniform_min_scores(min_scores, n);
  float *d_ms = nullptr, *d_ms_floor = nullptr;
  if (!uniform_thr) {
    bool uni = false;
    if (int rc = upload_min_scores(c, min_scores, n, nq_pad, &d_ms, &d_ms_floor, &uni)) return rc;
  }
  TAVB_HIP(hipMemsetAsync(c->d_queries_f16.ptr, 0, qbytes, c->stream));
  if (q32) {
    TAVB_HIP(hipMemcpyAsync(c->d_queries_f16.ptr, d_q, (size_t)n * c->dim * 4, hipMemcpyDeviceToDevice, c->stream));
  } else {
    hipError_t e = tavb::launch_f32_split_f16(d_q, c->d_queries_f16.ptr, reinterpret_cast<char*>(c->d_queries_f16.ptr) + plane, (int64_t)n * c->dim, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "query split launch failed: %s", hipGetErrorString(e));
  }
  const int64_t span_begin = dev_bits ? first_row / 256 * 256 : 0, span_end = dev_bits ? last_row + 1 : c->rows;
  if (span_begin < 0 || span_end > c->rows || span_end <= span_begin) return fail(TAVB_E_INVALID, "bad top-messages tile span (internal error)");
  const int sched = c->mfma_sched == 9 ? 9 : 0;
  tavb::MfmaParams p{};
  p.corpus = reinterpret_cast<const char*>(c->corpus) + (size_t)span_begin * c->dim * (q32 ? 4 : 2);
  p.queries = c->d_queries_f16.ptr;
  p.rows = span_end - span_begin;
  p.dim = c->dim;
  p.nq = n;
  p.nq_padded = nq_pad;
  p.k = 1;  // (unused: the form keeps no lists)
  p.min_score = uniform_thr ? min_scores[0] : lowest_min_score(min_scores, n);
  p.thr_in = d_ms_floor;
  p.n_splits = c->mfma_splits > 0 ? (int)c->mfma_splits : tavb::skinny_pick_splits(p.rows, nq_pad, qt, c->n_cu, c->dim, q32, sched);
  p.sched = sched;
  p.f32 = q32 ? 1 : 0;
  p.skinny_tile = qt;
  p.mask = dev_bits ? dev_bits + (span_begin >> 5) : nullptr;
  p.msg_map = c->row_to_msg + span_begin;
  p.msg_best = best;
  p.msg_map_rows = c->rows - span_begin;
  p.n_messages = c->n_messages;
  c->last_tier = 5;
  c->last_shadow = 0;
  c->last_direct = 0;
  c->masked_route = 10;
  Timed t(c, TAVB_KERNEL_SKINNY);
  hipError_t e = tavb::launch_skinny_scan(p, c->stream);
  if (e != hipSuccess)
    return fail(TAVB_E_HIP, "top-messages tile launch failed: %s (kernel %d, %lld rows in %d ranges, %d of %d queries)", hipGetErrorString(e), tavb::skinny_kernel_id(p),
                (long long)p.rows, p.n_splits, p.nq, p.nq_padded);
  c->last_skinny_kernel = tavb::skinny_kernel_id(p);
  return TAVB_OK;
}

// fp16 corpora of any width (one that is no multiple of 64 filters on the zero-padded copy of the rows, as the unmasked route does), every k the
// filter's band and the rescoring serve
bool masked_wide_supported(const tavb_ctx* c, int k) {
  return c->dtype == TAVB_F16 && c->dim > 0 && c->dim <= 16384 && tavb::mfma_supported(((c->dim + 63) / 64) * 64, k);
}

int search_masked_wide(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores, const uint32_t* dev_bits, int64_t first_row, int64_t last_row,
                       const int32_t* dev_rows, int64_t n_allowed, uint32_t index_base, u64_t* d_out) {
  if (c->dim % 64 != 0)  // the filter reads the padded copy (search_wide_exact fills it in; the unmasked dispatcher reserves it the same way)
    if (int rc = reserve_shadow(c)) return rc;
  c->last_tier = 4;
  c->last_direct = 0;
  c->masked_route = 3;
  if (staged_overflow(c, d_q)) {  // (tavb_ctx.h) the gather route over the mask's row list, as for a flagged query
    if (int rc = search_device_impl(c, d_q, nq, k, min_scores, dev_rows, n_allowed, 0u, d_out)) return rc;
    return remap_key_rows(c, d_out, d_out, (int64_t)nq * k, dev_rows, n_allowed, index_base);
  }
  const MaskedWide mw{dev_bits, first_row / 256 * 256, last_row + 1, dev_rows, n_allowed};
  return search_wide_exact(c, d_q, nq, k, min_scores, index_base, d_out, /*small=*/false, &mw);
}

// A scoped batch on the 128/256-query filter tile + exact rescoring (tavb_search_scoped_wide and its twins; the callers have checked the
// arguments and masked_wide_supported), in WAVES of query tiles like search_scoped_tile: per wave search_wide_exact builds the membership
// planes, runs the filter ladder over the span of the union with the per-query test in its admission path, selects the bands, rescores, and
// re-runs the wave's flagged queries on the row-list scoped route (one synchronise per wave: the flag list is read back).  A plane is 4 bytes
// per row of the span per 32 queries: a 256-query tile takes 32 bytes per row, a 128-query tile 16.  A wave is as many whole 256-query tiles as
// fit "scope_wave_bytes" (64 MiB) of planes, at least one tile: at 1M rows two tiles, 512 queries.  Whole multiples of 256 queries, so that
// whichever tile width search_wide_exact picks for a wave pads it to no more than the wave; where not even one 256-query tile fits (spans
// beyond 2M rows) and the batch runs on 128-query tiles, one of those.  The planes' workspace is therefore at most max(64 MiB, 32 bytes x
// span rows) whatever the batch.
int search_scoped_wide(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores, const uint32_t* const* masks, int64_t first_row, int64_t last_row,
                       uint32_t index_base, u64_t* d_out) {
  if (c->dim % 64 != 0)  // the filter reads the padded copy, as for one mask
    if (int rc = reserve_shadow(c)) return rc;
  c->last_tier = 4;
  c->last_direct = 0;
  c->last_topk_refine = 0;
  c->topk_rounds_pending = 0;
  c->masked_route = 6;
  if (staged_overflow(c, d_q)) return search_scoped_impl(c, d_q, nq, k, min_scores, masks, index_base, d_out, d_out);  // (tavb_ctx.h)
  const int64_t stride = scope_plane_stride(first_row, last_row);
  const int qt_all = c->mfma_tile > 0 ? (int)c->mfma_tile : tavb::mfma_query_tile_for(nq, stride, c->n_cu);
  const int64_t fit256 = c->scope_wave_bytes / (8 * stride * (int64_t)sizeof(uint32_t));  // whole 256-query tiles in the budget
  const int wave = fit256 >= 1 ? 256 * (int)std::min<int64_t>(fit256, 1 << 20) : qt_all;
  int flagged = 0, waves = 0;
  for (int q0 = 0; q0 < nq; q0 += wave, ++waves) {
    int n_flagged = 0;
    const ScopedWide sw{masks + q0, first_row, last_row, &n_flagged};
    if (int rc = search_wide_exact(c, d_q + (size_t)q0 * c->dim, std::min(wave, nq - q0), k, min_scores + q0, index_base, d_out + (size_t)q0 * k, /*small=*/false,
                                   nullptr, &sw))
      return rc;
    flagged += n_flagged;
  }
  if (waves > 1) {  // "last_flagged" reads the work list's header: the batch's count, not the last wave's
    int* h = reinterpret_cast<int*>(c->h_flag.ptr);
    h[0] = flagged;  // (every wave has synchronised behind its read-back: nothing in flight reads or writes h)
    TAVB_HIP(hipMemcpyAsync(c->d_flag.ptr, h, sizeof(int), hipMemcpyHostToDevice, c->stream));
  }
  return TAVB_OK;
}
}  // namespace host
}  // namespace tavb

extern "C" int tavb_plan_masked_wide(int32_t nq, int32_t k, int32_t dim, int32_t dtype, int64_t allowed, int64_t span, int64_t min_bytes, int64_t pct) {
  if (dtype != TAVB_F32 && dtype != TAVB_F16) return fail(TAVB_E_INVALID, "dtype must be TAVB_F32 or TAVB_F16");
  if (nq < 0 || allowed < 0 || span < allowed || min_bytes < 0 || pct < 0) return fail(TAVB_E_INVALID, "bad shape");
  if (dtype != TAVB_F16) return 0;  // (an fp32 corpus would filter on its shadow: not built)
  if (dim <= 0 || dim > 16384 || !tavb::mfma_supported(((dim + 63) / 64) * 64, k)) return 0;
  if (nq < kMfmaMinBatch) return 0;  // (the unmasked dispatcher's own lower bound for the wide tile, as it ships)
  if ((__int128)allowed * dim * 2 < (__int128)min_bytes) return 0;
  // the gather route reads the allowed rows once per 8 queries, the wide tile the span once per query tile (128 or 256 queries: what the filter
  // pass picks for this batch over `span` rows): the tile when the gather's bytes are at least pct % of the tile's
  const int qt = tavb::mfma_query_tile_for(nq, span, kPlanComputeUnits);
  const __int128 gather = (__int128)((nq + 7) / 8) * allowed * 100;
  const __int128 tile = (__int128)((nq + qt - 1) / qt) * span * pct;
  return gather >= tile ? 1 : 0;
}

extern "C" int tavb_plan_masked(int32_t nq, int32_t k, int32_t dim, int32_t dtype, int64_t allowed, int64_t span, int64_t min_bytes, int64_t pct) {
  if (dtype != TAVB_F32 && dtype != TAVB_F16) return fail(TAVB_E_INVALID, "dtype must be TAVB_F32 or TAVB_F16");
  if (nq < 0 || allowed < 0 || span < allowed || min_bytes < 0 || pct < 0) return fail(TAVB_E_INVALID, "bad shape");
  const bool f32 = dtype == TAVB_F32;
  if (dim <= 0 || !tavb::skinny_supported(dim, k, f32)) return 0;
  if (nq < (f32 ? kSkinnyMinBatchF32 : kSkinnyMinBatchF16)) return 0;  // (the unmasked tile's own lower bounds, as they ship)
  const __int128 row_bytes = (__int128)dim * (f32 ? 4 : 2);
  if ((__int128)allowed * row_bytes < (__int128)min_bytes) return 0;
  // the gather route reads the allowed rows once per 8 queries, the tile the span once per 64: the tile when the gather's bytes are at least
  // pct % of the tile's
  const __int128 gather = (__int128)((nq + 7) / 8) * allowed * 100;
  const __int128 tile = (__int128)((nq + 63) / 64) * span * pct;
  return gather >= tile ? 1 : 0;
}

extern "C" int tavb_plan_top_messages_tile(int32_t nq, int32_t dim, int32_t dtype, int64_t allowed, int64_t span, int64_t min_batch, int64_t min_bytes,
                                           int64_t pct) {
  if (dtype != TAVB_F32 && dtype != TAVB_F16) return fail(TAVB_E_INVALID, "dtype must be TAVB_F32 or TAVB_F16");
  if (nq < 0 || allowed < 0 || span < allowed || min_batch < 0 || min_bytes < 0 || pct < 0) return fail(TAVB_E_INVALID, "bad shape");
  const bool f32 = dtype == TAVB_F32;
  if (dim <= 0 || !tavb::skinny_supported(dim, 1, f32)) return 0;  // (rows of a multiple of 64 bytes; the form keeps no lists: any k)
  if (nq < 1 || nq < min_batch) return 0;
  if (allowed == span) return 1;  // every row of the span is allowed (an unmasked lookup): one pass per 64 queries against one per eight
  // under a mask the row scan reads the allowed rows once per 8 queries, the tile the span once per 64: tavb_plan_masked's rule and floor
  if ((__int128)allowed * dim * (f32 ? 4 : 2) < (__int128)min_bytes) return 0;
  const __int128 gather = (__int128)((nq + 7) / 8) * allowed * 100;
  const __int128 tile = (__int128)((nq + 63) / 64) * span * pct;
  return gather >= tile ? 1 : 0;
}

extern "C" int tavb_plan_scoped(int32_t nq, int32_t k, int32_t dim, int32_t dtype, int64_t gather_rows, int64_t span, int64_t min_bytes, int64_t pct) {
  if (dtype != TAVB_F32 && dtype != TAVB_F16) return fail(TAVB_E_INVALID, "dtype must be TAVB_F32 or TAVB_F16");
  if (nq < 0 || gather_rows < 0 || span < 0 || min_bytes < 0 || pct < 0) return fail(TAVB_E_INVALID, "bad shape");
  const bool f32 = dtype == TAVB_F32;
  if (dim <= 0 || !tavb::skinny_supported(dim, k, f32)) return 0;
  if (nq < (f32 ? kSkinnyMinBatchF32 : kSkinnyMinBatchF16)) return 0;  // (the unmasked tile's own lower bounds, as they ship)
  // gather_rows: over the row-list route's passes of eight queries, the sum of each pass' LARGEST scope -- a lower bound of the rows that
  // route reads (a pass reads the union of its scopes), so the rule errs towards the route that is there already.  The floor is per pass:
  // a pass below it is a launch-bound scan the tile's ladder does not beat.  The tile reads the span once per 64 queries.
  const __int128 passes = (nq + 7) / 8;
  if ((__int128)gather_rows * dim * (f32 ? 4 : 2) < passes * min_bytes) return 0;
  return (__int128)gather_rows * 100 >= (__int128)((nq + 63) / 64) * span * pct ? 1 : 0;
}

extern "C" int tavb_plan_scoped_wide(int32_t nq, int32_t k, int32_t dim, int32_t dtype, int64_t gather_rows, int64_t span, int64_t min_bytes, int64_t pct) {
  if (dtype != TAVB_F32 && dtype != TAVB_F16) return fail(TAVB_E_INVALID, "dtype must be TAVB_F32 or TAVB_F16");
  if (nq < 0 || gather_rows < 0 || span < 0 || min_bytes < 0 || pct < 0) return fail(TAVB_E_INVALID, "bad shape");
  if (dtype != TAVB_F16) return 0;  // (an fp32 corpus would filter on its shadow: not built)
  if (dim <= 0 || dim > 16384 || !tavb::mfma_supported(((dim + 63) / 64) * 64, k)) return 0;
  if (nq < kMfmaMinBatch) return 0;  // (the unmasked dispatcher's own lower bound for the wide tile, as it ships)
  // tavb_plan_scoped's rule with the wide tile's reads: gather_rows is the lower bound of what the row-list route reads -- over its passes
  // (of four queries for k > 64, else eight) the sum of each pass' largest scope; the floor is per pass; the wide tile reads the span once
  // per query tile (128 or 256 queries: what the filter pass picks for this batch over `span` rows)
  const int per_pass = k > 64 ? 4 : 8;
  const __int128 passes = (nq + per_pass - 1) / per_pass;
  if ((__int128)gather_rows * dim * 2 < passes * min_bytes) return 0;
  const int qt = tavb::mfma_query_tile_for(nq, span, kPlanComputeUnits);
  return (__int128)gather_rows * 100 >= (__int128)((nq + qt - 1) / qt) * span * pct ? 1 : 0;
}

extern "C" int tavb_plan_filter_shape(int32_t shape, int32_t query_tile, int32_t split, int32_t bdirect, int32_t sched, int32_t ablate) {
  if (shape != 16 && shape != 32) return fail(TAVB_E_INVALID, "mfma_shape must be 16 or 32");
  if (query_tile != 128 && query_tile != 256) return fail(TAVB_E_INVALID, "query_tile must be 128 or 256");
  tavb::MfmaParams p{};
  p.shape = shape;
  p.wide_tile = query_tile;
  p.split_plane = split ? 1 : 0;
  p.bdirect = bdirect ? 1 : 0;
  p.sched = sched;
  p.ablate = ablate;
  return tavb::mfma_tile_shape(p);
}

extern "C" int tavb_plan_ladder(int64_t rows, int32_t nq, int32_t n_cu, int64_t* out_bounds, int32_t cap) {
  if (rows < 0 || nq < 1 || n_cu < 8) return fail(TAVB_E_INVALID, "bad shape");
  const int qt = tavb::mfma_query_tile_for(nq, rows, n_cu);
  const int nq_pad = ((nq + qt - 1) / qt) * qt;
  const int splits = tavb::mfma_pick_splits(rows, nq_pad, qt, n_cu);
  const std::vector<int64_t> b = ladder_bounds(rows, splits, nq_pad, /*skinny=*/false, /*ladder=*/true, /*sample_opt=*/0, /*growth=*/4);
  for (size_t i = 0; out_bounds && i < b.size() && (int)i < cap; ++i) out_bounds[i] = b[i];
  return (int)b.size() - 1;
}

