// The large-k and sorted lookups of the C ABI (include/tavb.h): tavb_search_topk and its subset / device forms, tavb_search_sorted,
// tavb_search_subset_sorted, tavb_search_subset_batch_sorted, tavb_sort_keys_device, their scoped forms (one mask per query:
// tavb_search_scoped_topk / _device, tavb_search_scoped_sorted), the top-messages lookups (tavb_search_top_messages / _device), their scoped forms
// (tavb_search_top_messages_scoped / _device) and their forms on the 32/64-query tile (tavb_search_top_messages_tile / _device) -- and the score pass they share.  Host code only: the kernels live in tavb_scan.hip,
// tavb_topk.hip and tavb_sort.hip, the staging in tavb_lookup.hip.

#include <optional>

#include "tavb_ctx.h"

using namespace tavb::host;

namespace {

// ---- the score pass of the large-k and sorted lookups: the queries go over the n_pos positions in groups of up to TAVB_MAX_STREAM_QUERIES
// (fewer where the score array would pass topk_scores_bytes or the vector tier's LDS would overflow); per group a memset, ONE score pass
// and the refinement rounds.  Every launch's grid is fixed on the host.
struct ScorePlan {
  int64_t n_pos;
  int nb, cap;           // histogram buckets, capacity of a query's boundary list
  int64_t per;           // queries per group
  int rounds;            // refinement rounds of a group (0: nothing to refine)
  int sel_blocks;        // grid of the passes over the score array
  tavb::ScanGeometry g;  // of the score pass
};

// Groups of at most `most` queries over n_pos positions, cut to what "topk_scores_bytes" lets one score array hold (at least one), and
// the score array of one group reserved; d_topk, the selection's workspace, is the caller's to reserve.
int shape_score_pass(tavb_ctx* c, int64_t most, int64_t n_pos, bool refine, ScorePlan* s) {
  s->n_pos = n_pos;
  s->nb = (int)c->topk_buckets;
  s->cap = (int)c->topk_boundary_keys;
  s->per = std::min<int64_t>(most, std::max<int64_t>(1, c->topk_scores_bytes / (n_pos * (int64_t)sizeof(uint32_t))));
  s->rounds = refine ? tavb::topk_refine_rounds(n_pos, s->cap) : 0;
  if (int rc = c->d_topk_scores.reserve((size_t)s->per * n_pos * sizeof(uint32_t))) return rc;
  s->g = clamped_geometry(c);
  s->g.blocks = scan_blocks_for(c, n_pos, s->g.waves, 2);
  // the passes over the score array: 4 bytes per row and query, ~8 rows per thread and a grid of a few workgroups per CU in all
  s->sel_blocks = (int)std::min<int64_t>(std::max<int64_t>(1, (n_pos + 2047) / 2048), std::max<int64_t>(1, 2048 / s->per));
  return TAVB_OK;
}

// the groups of an unscoped batch of nq queries: as many queries as the score pass takes
int plan_score_pass(tavb_ctx* c, int nq, int64_t n_pos, bool refine, ScorePlan* s) {
  return shape_score_pass(c, std::min<int64_t>(tavb::topk_queries_per_pass(c->dim, c->dtype, (int)c->topk_buckets), nq), n_pos, refine, s);
}

// queries per pass of the scoped routes: the score pass' own, within the bits of a membership byte
int scoped_topk_per_pass(const tavb_ctx* c) { return std::min(tavb::topk_queries_per_pass(c->dim, c->dtype, (int)c->topk_buckets), 8); }

// the bucket maps of n queries (topk_bucket, tavb_device.h): lo = the threshold brought into [0, 1], scale = nb / (1 - lo); slots from n on: nothing passes
void bucket_maps(const float* min_scores /*host, n*/, int n, int nb, tavb::TopkLaunch* t) {
  for (int i = 0; i < TAVB_MAX_STREAM_QUERIES; ++i) {
    const float ms = i < n ? min_scores[i] : INFINITY;
    float lo = ms > 0.0f ? ms : 0.0f;  // (NaN: nothing passes; the bucket map is never used)
    if (lo > 1.0f) lo = 1.0f;
    t->lo[i] = lo;
    t->scale[i] = lo < 1.0f ? (float)nb / (1.0f - lo) : 0.0f;
  }
}

// The pass for the queries [q0, q0 + n) of the batch (d_q, min_scores: the whole batch's; d_rows: a subset's rows, or null).  *t arrives
// with the caller's own members set (k, out_keys, out_rounds, index_base) and leaves filled in, ready for the caller's selection launches.
// `what` names the caller in the messages.  *tm: the TAVB_KERNEL_TOPK interval, opened in front of the refinement rounds -- the caller's
// launches of the group that follow belong to it, and the caller closes it.
// member (optional): the scoped form -- d_rows is the union list of a scoped pass, member its membership bytes, and the n queries are its
// member bits bit0 .. bit0 + n - 1 (launch_scan_topk_scoped).
int run_score_pass(tavb_ctx* c, const ScorePlan& s, const char* what, const float* d_q, const float* min_scores /*host*/, const int32_t* d_rows, int q0, int n,
                   tavb::TopkLaunch* t, std::optional<Timed>* tm, const uint8_t* member = nullptr, int bit0 = 0) {
  TAVB_HIP(hipMemsetAsync(c->d_topk.ptr, 0, tavb::topk_head_bytes(n, s.nb, s.rounds), c->stream));
  tavb::ScanParams p = scan_params(c, d_q + (size_t)q0 * c->dim, d_rows, s.n_pos, n, 1, 0u, ~0ull, nullptr, min_scores + q0, TAVB_MAX_GROUPED_QUERIES);
  p.topk_scores = reinterpret_cast<unsigned*>(c->d_topk_scores.ptr);
  p.topk_hist = reinterpret_cast<unsigned*>(c->d_topk.ptr);
  p.topk_buckets = s.nb;
  p.scope_member = member;
  p.scope_bit0 = bit0;
  bucket_maps(min_scores + q0, n, s.nb, t);
  for (int i = 0; i < TAVB_MAX_STREAM_QUERIES; ++i) {
    p.topk_lo[i] = t->lo[i];
    p.topk_scale[i] = t->scale[i];
  }
  {
    Timed scan(c, TAVB_KERNEL_SCAN);
    hipError_t e = member ? tavb::launch_scan_topk_scoped(p, s.g, c->stream, &c->last_tier) : tavb::launch_scan_topk(p, s.g, c->stream, &c->last_tier);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "%s score pass launch failed: %s", what, hipGetErrorString(e));
  }
  t->scores = p.topk_scores;
  t->workspace = c->d_topk.ptr;
  t->n_pos = s.n_pos;
  t->nq = n;
  t->buckets = s.nb;
  t->cap = s.cap;
  t->rounds = s.rounds;
  t->blocks = s.sel_blocks;
  tm->emplace(c, TAVB_KERNEL_TOPK);
  for (int r = 0; r < s.rounds; ++r) {
    hipError_t e = tavb::launch_topk_refine(*t, r, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "%s refinement launch failed: %s", what, hipGetErrorString(e));
  }
  return TAVB_OK;
}

}  // namespace

namespace tavb {
namespace host __attribute__((visibility("hidden"))) {

// ---- exact top-k beyond the fused selection (tavb_topk.hip): queries on the device (d_q [nq, dim]) over n_pos positions (d_rows: the
// subset's rows, or null) -> out_keys [nq][k] sorted, zero-filled, + out_rounds [nq], both in pinned host memory.  Per group of the score
// pass: the compaction and the finish -- nothing is read back before the caller's one synchronise.
int search_topk_impl(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const int32_t* d_rows, int64_t n_pos,
                     uint32_t index_base, u64_t* out_keys, int32_t* out_rounds) {
  ScorePlan s;
  if (int rc = plan_score_pass(c, nq, n_pos, /*refine=*/true, &s)) return rc;
  if (int rc = c->d_topk.reserve(tavb::topk_workspace_bytes((int)s.per, k, s.nb, s.cap, s.rounds))) return rc;
  for (int q0 = 0; q0 < nq; q0 += (int)s.per) {
    const int n = (int)std::min<int64_t>(s.per, nq - q0);
    tavb::TopkLaunch t{};
    t.k = k;
    t.out_keys = out_keys + (size_t)q0 * k;
    t.out_rounds = out_rounds + q0;
    t.index_base = index_base;
    std::optional<Timed> tm;
    if (int rc = run_score_pass(c, s, "top-k", d_q, min_scores, d_rows, q0, n, &t, &tm)) return rc;
    hipError_t e = tavb::launch_topk_compact(t, c->stream);
    if (e == hipSuccess) e = tavb::launch_topk_finish(t, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "top-k selection launch failed: %s", hipGetErrorString(e));
  }
  return TAVB_OK;
}

// ---- the same under one scope per query (tavb_search_scoped_topk): waves of passes as in search_scoped_impl (tavb_route.hip).  Per pass
// whose union is not empty: the write pass and the membership bytes, then per sub-group of its queries (one, unless the score array of the
// whole pass would exceed "topk_scores_bytes") a memset, the scoped score pass, the refinement rounds, the compaction and the finish --
// keys carrying union-list positions into `work` -- and ONE remap of the pass' keys to index_base + row into `out`.  The histograms saw
// members only, so need = min(k, survivors of the query's own scope) falls out of the boundary search as it stands.
// out_rounds: pinned host memory; the queries of empty unions get their zero from the host, after the wave's synchronise.
int search_scoped_topk_impl(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const uint32_t* const* masks,
                            uint32_t index_base, u64_t* work, u64_t* out, int32_t* out_rounds) {
  const int per = scoped_topk_per_pass(c);
  const int wave = scoped_wave_queries(c, per);
  for (int w0 = 0; w0 < nq; w0 += wave) {
    const int wn = std::min(wave, nq - w0);
    ScopeWave w;
    if (int rc = scope_wave_unions(c, wn, per, masks + w0, &w)) return rc;
    for (int p = 0; p < w.passes; ++p) {
      const int q0 = w0 + p * per, n = std::min(per, wn - p * per);
      const int64_t n_pos = w.n_union[p];
      if (n_pos == 0) {  // every scope of the pass is empty
        for (int q = 0; q < n; ++q) out_rounds[q0 + q] = 0;
        if (int rc = fill_empty_keys(c, out + (size_t)q0 * k, (int64_t)n * k)) return rc;
        continue;
      }
      const int32_t* list;
      const uint8_t* member;
      if (int rc = scope_wave_lists(c, w, p, &list, &member)) return rc;
      ScorePlan s;
      if (int rc = shape_score_pass(c, n, n_pos, /*refine=*/true, &s)) return rc;
      if (int rc = c->d_topk.reserve(tavb::topk_workspace_bytes((int)s.per, k, s.nb, s.cap, s.rounds))) return rc;
      for (int s0 = 0; s0 < n; s0 += (int)s.per) {
        const int m = (int)std::min<int64_t>(s.per, n - s0);
        tavb::TopkLaunch t{};
        t.k = k;
        t.out_keys = work + (size_t)(q0 + s0) * k;
        t.out_rounds = out_rounds + q0 + s0;
        t.index_base = 0u;
        std::optional<Timed> tm;
        if (int rc = run_score_pass(c, s, "scoped top-k", d_q, min_scores, list, q0 + s0, m, &t, &tm, member, s0)) return rc;
        hipError_t e = tavb::launch_topk_compact(t, c->stream);
        if (e == hipSuccess) e = tavb::launch_topk_finish(t, c->stream);
        if (e != hipSuccess) return fail(TAVB_E_HIP, "scoped top-k selection launch failed: %s", hipGetErrorString(e));
      }
      Timed tm(c, TAVB_KERNEL_TOPK);
      hipError_t e = tavb::launch_remap_positions(work + (size_t)q0 * k, out + (size_t)q0 * k, (int64_t)n * k, list, n_pos, index_base, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "scoped top-k remap launch failed: %s", hipGetErrorString(e));
    }
  }
  return TAVB_OK;
}

// ---- the best k messages (tavb_search_top_messages): the group-by-message step between the score pass and the selection.  Groups of
// queries as in search_topk_impl, sized by the queries' LDS alone (the MessageMaxSink keeps no histogram there) and by "topk_scores_bytes"
// over [queries][n_messages].  Per group: the head of d_topk and the group's slots of d_msg_best zeroed, ONE pass over the corpus or the row
// list, the histogram pass over the messages, then the refinement rounds, the compaction and the finish with n_pos = n_messages.
namespace {

// Groups of at most `most` queries over nm = n_messages slots, cut to what "topk_scores_bytes" lets [queries][n_messages] hold (at least
// one), with d_msg_best and the selection's workspace reserved for one group at depth k -- d_msg_best with TAVB_MAX_STREAM_QUERIES words
// behind the group's slots (the per-query failure flags of merge_top_messages_impl), so that the merge of a lookup's lists never asks for
// more than the lookup itself did.  s->g.blocks is the caller's to set per pass.
int plan_top_messages(tavb_ctx* c, int64_t nm, int64_t most, int k, ScorePlan* s) {
  s->n_pos = nm;
  s->nb = (int)c->topk_buckets;
  s->cap = (int)c->topk_boundary_keys;
  s->per = std::min<int64_t>(most, std::max<int64_t>(1, c->topk_scores_bytes / (nm * (int64_t)sizeof(uint32_t))));
  s->rounds = tavb::topk_refine_rounds(nm, s->cap);
  s->g = clamped_geometry(c);
  s->sel_blocks = (int)std::min<int64_t>(std::max<int64_t>(1, (nm + 2047) / 2048), std::max<int64_t>(1, 2048 / s->per));
  if (int rc = c->d_msg_best.reserve(((size_t)s->per * nm + TAVB_MAX_STREAM_QUERIES) * sizeof(uint32_t))) return rc;
  return c->d_topk.reserve(tavb::topk_workspace_bytes((int)s->per, k, s->nb, s->cap, s->rounds));
}

// The second half of a group, shared with the tile route: best [n][n_messages] as a top-messages score pass left it (n <= s.per <= 8 queries
// whose thresholds are min_scores[0 .. n)) and the zeroed head of d_topk -> the histogram pass, the refinement rounds, the compaction and the
// finish -> out_keys [n][k] and out_rounds [n].
int top_messages_select(tavb_ctx* c, const ScorePlan& s, unsigned* best, const float* min_scores /*host, n*/, int n, int k, u64_t* out_keys, int32_t* out_rounds) {
  tavb::TopkLaunch t{};
  bucket_maps(min_scores, n, s.nb, &t);
  t.scores = best;
  t.workspace = c->d_topk.ptr;
  t.n_pos = s.n_pos;
  t.nq = n;
  t.k = k;
  t.buckets = s.nb;
  t.cap = s.cap;
  t.rounds = s.rounds;
  t.blocks = s.sel_blocks;
  t.out_keys = out_keys;
  t.out_rounds = out_rounds;
  t.index_base = 0u;
  Timed tm(c, TAVB_KERNEL_TOPK);
  hipError_t e = tavb::launch_message_hist(t, best, c->stream);
  for (int r = 0; r < s.rounds && e == hipSuccess; ++r) e = tavb::launch_topk_refine(t, r, c->stream);
  if (e == hipSuccess) e = tavb::launch_topk_compact(t, c->stream);
  if (e == hipSuccess) e = tavb::launch_topk_finish(t, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "top-messages selection launch failed: %s", hipGetErrorString(e));
  return TAVB_OK;
}

// One group: the queries [q0, q0 + n) of the batch, n <= s.per, over the n_scan positions of d_rows (null: the corpus) -> out_keys [n][k]
// and out_rounds [n], both at the group's first query.  member (optional): the scoped form -- d_rows is the union list of a scoped pass,
// member its membership bytes, and the n queries are its member bits bit0 .. bit0 + n - 1 (launch_scan_top_messages_scoped).
int top_messages_group(tavb_ctx* c, const ScorePlan& s, const float* d_q, const float* min_scores /*host*/, const int32_t* d_rows, int64_t n_scan, int q0,
                       int n, int k, u64_t* out_keys, int32_t* out_rounds, const uint8_t* member = nullptr, int bit0 = 0) {
  const int64_t nm = s.n_pos;
  unsigned* const best = reinterpret_cast<unsigned*>(c->d_msg_best.ptr);
  TAVB_HIP(hipMemsetAsync(c->d_topk.ptr, 0, tavb::topk_head_bytes(n, s.nb, s.rounds), c->stream));
  TAVB_HIP(hipMemsetAsync(best, 0, (size_t)n * nm * sizeof(uint32_t), c->stream));
  tavb::ScanParams p = scan_params(c, d_q + (size_t)q0 * c->dim, d_rows, n_scan, n, 1, 0u, ~0ull, nullptr, min_scores + q0, TAVB_MAX_GROUPED_QUERIES);
  p.topk_scores = best;
  p.row_to_msg = c->row_to_msg;
  p.n_messages = nm;
  p.scope_member = member;
  p.scope_bit0 = bit0;
  {
    Timed scan(c, TAVB_KERNEL_SCAN);
    hipError_t e = member ? tavb::launch_scan_top_messages_scoped(p, s.g, c->stream, &c->last_tier) : tavb::launch_scan_top_messages(p, s.g, c->stream, &c->last_tier);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "top-messages score pass launch failed: %s", hipGetErrorString(e));
  }
  return top_messages_select(c, s, best, min_scores + q0, n, k, out_keys, out_rounds);
}

}  // namespace

int search_top_messages_impl(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const int32_t* d_rows, int64_t n_rows,
                             u64_t* out_keys, int32_t* out_rounds) {
  const int64_t n_scan = d_rows ? n_rows : c->rows;
  ScorePlan s;
  if (int rc = plan_top_messages(c, c->n_messages, std::min<int64_t>(tavb::topk_queries_per_pass(c->dim, c->dtype, 0), nq), k, &s)) return rc;
  s.g.blocks = scan_blocks_for(c, n_scan, s.g.waves, 2);
  for (int q0 = 0; q0 < nq; q0 += (int)s.per) {
    const int n = (int)std::min<int64_t>(s.per, nq - q0);
    if (int rc = top_messages_group(c, s, d_q, min_scores, d_rows, n_scan, q0, n, k, out_keys + (size_t)q0 * k, out_rounds + q0)) return rc;
  }
  return TAVB_OK;
}

// ---- the merge of the top-messages lists of several shards (tavb_merge_top_messages_device): groups of up to TAVB_MAX_STREAM_QUERIES queries,
// cut by "topk_scores_bytes" over [queries][nm] as above.  Per group: the two memsets, ONE launch that raises every key's message slot to
// its score (launch_message_keys_max -- the score pass' place), then the second half of the group above.  Thresholds: 0 -- the keys have
// passed theirs on their shards, and a bucket map only has to be monotone.  A query one of whose lists leads with the failure key raises
// nothing, its selection leaves an empty row, and the flagged fill behind it writes the failure key into every slot.  The flags of a group
// live behind its slots of d_msg_best (plan_top_messages reserves them).
int merge_top_messages_impl(tavb_ctx* c, const u64_t* lists, int n_lists, int nq, int k, bool query_major, int64_t nm, u64_t* out_keys, int32_t* out_rounds) {
  ScorePlan s;
  if (int rc = plan_top_messages(c, nm, std::min(TAVB_MAX_STREAM_QUERIES, nq), k, &s)) return rc;
  unsigned* const best = reinterpret_cast<unsigned*>(c->d_msg_best.ptr);
  unsigned* const flags = best + (size_t)s.per * nm;
  const float zeros[TAVB_MAX_STREAM_QUERIES] = {};
  for (int q0 = 0; q0 < nq; q0 += (int)s.per) {
    const int n = (int)std::min<int64_t>(s.per, nq - q0);
    TAVB_HIP(hipMemsetAsync(c->d_topk.ptr, 0, tavb::topk_head_bytes(n, s.nb, s.rounds), c->stream));
    TAVB_HIP(hipMemsetAsync(best, 0, (size_t)n * nm * sizeof(uint32_t), c->stream));
    {
      Timed tm(c, TAVB_KERNEL_MERGE);
      hipError_t e = tavb::launch_message_keys_max(lists, n_lists, nq, k, query_major, q0, n, nm, best, flags, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "top-messages merge launch failed: %s", hipGetErrorString(e));
    }
    if (int rc = top_messages_select(c, s, best, zeros, n, k, out_keys + (size_t)q0 * k, out_rounds + q0)) return rc;
    Timed tm(c, TAVB_KERNEL_MERGE);
    hipError_t e = tavb::launch_fill_flagged_rows(out_keys + (size_t)q0 * k, n, k, TAVB_KEY_PEER_FAILED, flags, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "top-messages merge fill launch failed: %s", hipGetErrorString(e));
  }
  return TAVB_OK;
}

// ---- the same on the 32/64-query tile (tavb_search_top_messages_tile): groups of up to 64 queries -- fewer where [queries][n_messages]
// would pass "topk_scores_bytes" -- each ONE tile launch over the corpus or the span of the one mask (top_messages_tile_pass, tavb_route.hip)
// into the group's zeroed slots of d_msg_best; then, eight queries at a time (the selection's launches take no more), the zeroed head of d_topk
// and the second half of the group above over those queries' slots.
int search_top_messages_tile_impl(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const uint32_t* dev_bits,
                                  int64_t first_row, int64_t last_row, u64_t* out_keys, int32_t* out_rounds) {
  const int64_t nm = c->n_messages;
  if (staged_overflow(c, d_q)) {  // (tavb_ctx.h) the row scan's forms: every query under the one mask, or over the whole corpus
    if (!dev_bits) return search_top_messages_impl(c, d_q, nq, k, min_scores, nullptr, 0, out_keys, out_rounds);
    const std::vector<const uint32_t*> masks((size_t)nq, dev_bits);
    return search_scoped_top_messages_impl(c, d_q, nq, k, min_scores, masks.data(), out_keys, out_rounds);
  }
  const int per_tile = (int)std::min<int64_t>(std::min(64, nq), std::max<int64_t>(1, c->topk_scores_bytes / (nm * (int64_t)sizeof(uint32_t))));
  ScorePlan s;
  if (int rc = plan_top_messages(c, nm, std::min(TAVB_MAX_STREAM_QUERIES, per_tile), k, &s)) return rc;
  if (int rc = c->d_msg_best.reserve((size_t)per_tile * nm * sizeof(uint32_t))) return rc;
  unsigned* const best = reinterpret_cast<unsigned*>(c->d_msg_best.ptr);
  for (int q0 = 0; q0 < nq; q0 += per_tile) {
    const int n = std::min(per_tile, nq - q0);
    TAVB_HIP(hipMemsetAsync(best, 0, (size_t)n * nm * sizeof(uint32_t), c->stream));
    if (int rc = top_messages_tile_pass(c, d_q + (size_t)q0 * c->dim, n, min_scores + q0, dev_bits, first_row, last_row, best)) return rc;
    for (int s0 = 0; s0 < n; s0 += (int)s.per) {
      const int m = (int)std::min<int64_t>(s.per, n - s0);
      TAVB_HIP(hipMemsetAsync(c->d_topk.ptr, 0, tavb::topk_head_bytes(m, s.nb, s.rounds), c->stream));
      if (int rc = top_messages_select(c, s, best + (size_t)s0 * nm, min_scores + q0 + s0, m, k, out_keys + (size_t)(q0 + s0) * k, out_rounds + q0 + s0)) return rc;
    }
  }
  return TAVB_OK;
}

// ---- the same under one scope per query (tavb_search_top_messages_scoped): the waves and passes of search_scoped_topk_impl around the
// group above.  Per pass whose union is not empty: the write pass and the membership bytes, then per sub-group of its queries (one, unless
// [queries][n_messages] would exceed "topk_scores_bytes") the two memsets, the scoped score pass over the union list with bit0 = the
// sub-group's first query of the pass, the histogram pass and the selection.  Keys carry message ordinals, not union positions: nothing
// is remapped.  out_rounds: pinned host memory; the queries of empty unions get their zero from the host, after the wave's synchronise.
int search_scoped_top_messages_impl(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores /*host, nq*/, const uint32_t* const* masks,
                                    u64_t* out_keys, int32_t* out_rounds) {
  const int per = scoped_topk_per_pass(c);
  const int wave = scoped_wave_queries(c, per);
  ScorePlan s;
  if (int rc = plan_top_messages(c, c->n_messages, std::min(per, nq), k, &s)) return rc;
  for (int w0 = 0; w0 < nq; w0 += wave) {
    const int wn = std::min(wave, nq - w0);
    ScopeWave w;
    if (int rc = scope_wave_unions(c, wn, per, masks + w0, &w)) return rc;
    for (int p = 0; p < w.passes; ++p) {
      const int q0 = w0 + p * per, n = std::min(per, wn - p * per);
      const int64_t n_pos = w.n_union[p];
      if (n_pos == 0) {  // every scope of the pass is empty
        for (int q = 0; q < n; ++q) out_rounds[q0 + q] = 0;
        if (int rc = fill_empty_keys(c, out_keys + (size_t)q0 * k, (int64_t)n * k)) return rc;
        continue;
      }
      const int32_t* list;
      const uint8_t* member;
      if (int rc = scope_wave_lists(c, w, p, &list, &member)) return rc;
      s.g.blocks = scan_blocks_for(c, n_pos, s.g.waves, 2);
      for (int s0 = 0; s0 < n; s0 += (int)s.per) {
        const int m = (int)std::min<int64_t>(s.per, n - s0);
        if (int rc = top_messages_group(c, s, d_q, min_scores, list, n_pos, q0 + s0, m, k, out_keys + (size_t)(q0 + s0) * k, out_rounds + q0 + s0, member, s0))
          return rc;
      }
    }
  }
  return TAVB_OK;
}

// what both top-messages entry points check: context, corpus, 1 <= k <= TAVB_MAX_LARGE_K, the row list's shape, and a row -> message map
// that covers exactly the corpus and whose ordinals fit a key's position.  *empty: nothing to scan -- every list is empty.
int check_top_messages_args(tavb_ctx* c, int k, const int32_t* dev_rows, int64_t n_rows, bool* empty) {
  if (int rc = check_topk_args(c, k)) return rc;
  if (n_rows < 0 || n_rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "bad row list length");
  if (!dev_rows && n_rows != 0) return fail(TAVB_E_INVALID, "null dev_rows");
  if (!c->row_to_msg && c->rows > 0) return fail(TAVB_E_NO_CORPUS, "no row -> message map set (call tavb_set_row_messages first)");
  if (c->row_to_msg_rows != c->rows)
    return fail(TAVB_E_INVALID, "the row -> message map covers %lld rows, the corpus has %lld", (long long)c->row_to_msg_rows, (long long)c->rows);
  if (c->n_messages >= 0x7FFFFFFFll) return fail(TAVB_E_UNSUPPORTED, "top-messages keys hold message ordinals: n_messages must be < 2^31 - 1");
  if (c->rows >= 0xFFFFFFFFll) return fail(TAVB_E_UNSUPPORTED, "the score pass indexes rows in 32 bits: rows must be < 2^32 - 1");
  *empty = c->rows == 0 || c->n_messages == 0 || (dev_rows && n_rows == 0);
  return TAVB_OK;
}

int check_topk_args(tavb_ctx* c, int k) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = require_corpus(c)) return rc;
  if (k < 1 || k > TAVB_MAX_LARGE_K) return fail(TAVB_E_INVALID, "k must be 1 .. %d (got %d)", TAVB_MAX_LARGE_K, k);
  return TAVB_OK;
}

// the pinned keys [nq][k] + rounds [nq] of a large-k lookup
int reserve_topk_out(tavb_ctx* c, int nq, int k, u64_t** keys, int32_t** rounds) {
  const size_t kbytes = (size_t)nq * k * sizeof(u64_t);
  if (int rc = c->h_out.reserve(kbytes + (size_t)nq * sizeof(int32_t))) return rc;
  *keys = reinterpret_cast<u64_t*>(c->h_out.ptr);
  *rounds = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(c->h_out.ptr) + kbytes);
  return TAVB_OK;
}

void note_rounds(tavb_ctx* c, const int32_t* rounds, int nq) {
  int m = 0;
  for (int q = 0; q < nq; ++q) m = std::max(m, (int)rounds[q]);
  c->last_topk_refine = m;
}

// queries already on the device, keys to device (or device-writable pinned) memory, nothing waited for: the refinement rounds of the queries
// land in the context's own pinned words and become "last_topk_refine" at the next tavb_synchronize
int search_topk_async(tavb_ctx* c, const float* d_q, int nq, int k, const float* min_scores, const int32_t* d_rows, int64_t n_pos, uint32_t index_base,
                      u64_t* out_keys) {
  c->topk_rounds_pending = 0;
  c->last_topk_refine = 0;
  if (int rc = c->h_topk_rounds.reserve((size_t)nq * sizeof(int32_t))) return rc;
  if (n_pos == 0 || c->rows == 0) return fill_empty_keys(c, out_keys, (int64_t)nq * k);  // nothing to scan
  if (int rc = search_topk_impl(c, d_q, nq, k, min_scores, d_rows, n_pos, index_base, out_keys, reinterpret_cast<int32_t*>(c->h_topk_rounds.ptr))) return rc;
  c->topk_rounds_pending = nq;
  return TAVB_OK;
}

}  // namespace host
}  // namespace tavb

extern "C" {

int tavb_search_topk(tavb_ctx* c, const float* queries_host, int32_t nq, int32_t k, const float* min_scores, int64_t* out_ordinals, float* out_scores,
                     int32_t* out_counts) {
  if (int rc = check_topk_args(c, k)) return rc;
  if (nq < 0) return fail(TAVB_E_INVALID, "nq must be >= 0");
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_ordinals || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  c->last_topk_refine = 0;
  c->topk_rounds_pending = 0;  // (an asynchronous large-k call before this one no longer reports: the option speaks of the LAST lookup)
  c->last_rows_query = 0;
  c->last_pairs_join = 0;
  if (c->rows == 0) return empty_counts(out_counts, nq);
  DeviceGuard guard(c->device);
  const float* d_q;
  u64_t* keys;
  int32_t* rounds;
  if (int rc = reserve_topk_out(c, nq, k, &keys, &rounds)) return rc;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  if (int rc = search_topk_impl(c, d_q, nq, k, min_scores, nullptr, c->rows, 0u, keys, rounds)) return rc;
  return collect_keys(c, keys, nq, k, c->ordinal_base, out_ordinals, out_scores, out_counts, rounds);
}

int tavb_search_subset_topk(tavb_ctx* c, const float* query_host, const int64_t* rows_host, int64_t n_subset, int32_t k, float min_score,
                            int64_t* out_positions, float* out_scores, int32_t* out_count) {
  if (int rc = check_topk_args(c, k)) return rc;
  if (n_subset < 0) return fail(TAVB_E_INVALID, "n_subset must be >= 0");
  if (!query_host || !out_positions || !out_scores || !out_count) return fail(TAVB_E_INVALID, "null argument");
  c->last_topk_refine = 0;
  c->topk_rounds_pending = 0;
  if (n_subset == 0 || c->rows == 0) {
    *out_count = 0;
    return TAVB_OK;
  }
  if (!rows_host) return fail(TAVB_E_INVALID, "null rows_host");
  if (n_subset >= 0x7FFFFFFFll) return fail(TAVB_E_UNSUPPORTED, "subset too long");
  DeviceGuard guard(c->device);
  const float* d_q;
  const int32_t* d_rows;
  u64_t* keys;
  int32_t* rounds;
  if (int rc = reserve_topk_out(c, 1, k, &keys, &rounds)) return rc;
  if (int rc = stage_subset(c, query_host, rows_host, n_subset, &d_q, &d_rows)) return rc;
  if (int rc = search_topk_impl(c, d_q, 1, k, &min_score, d_rows, n_subset, 0u, keys, rounds)) return rc;
  return collect_keys(c, keys, 1, k, 0, out_positions, out_scores, out_count, rounds);
}

int tavb_search_topk_device(tavb_ctx* c, const float* dev_queries, int32_t nq, int32_t k, const float* min_scores, const int32_t* dev_rows,
                            int64_t n_subset, tavb_key* out_keys) {
  if (int rc = check_topk_args(c, k)) return rc;
  if (nq < 1) return fail(TAVB_E_INVALID, "nq must be >= 1");
  if (!dev_queries || !min_scores || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  if (n_subset < 0 || n_subset >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "bad subset length");
  if (dev_rows && nq != 1) return fail(TAVB_E_INVALID, "a subset goes with exactly one query");
  if (!dev_rows && n_subset != 0) return fail(TAVB_E_INVALID, "null dev_rows");
  if (!dev_rows)
    if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  return dev_rows ? search_topk_async(c, dev_queries, 1, k, min_scores, dev_rows, n_subset, 0u, reinterpret_cast<u64_t*>(out_keys))
                  : search_topk_async(c, dev_queries, nq, k, min_scores, nullptr, c->rows, (uint32_t)c->ordinal_base, reinterpret_cast<u64_t*>(out_keys));
}

// ---- sorted lookups: every survivor (k = 0) or the best k for any k, sorted on the device.  Per group of the score pass (refined
// only when k < n_pos): the per-block key counts -> pinned, ONE synchronise; the host checks max_total and then, query by query: compaction in position order, the sort, and the decode of the
// best `need` keys into h_out, which is copied to the caller's arrays whenever the next piece would not fit sort_stage_keys.
namespace {
struct SortedOut {  // the caller's concatenated results and how far they are filled
  int64_t* ords;
  float* scs;
  int64_t done = 0;    // results copied to the caller
  int64_t staged = 0;  // results decoded into h_out, not yet copied
};

int flush_staged(tavb_ctx* c, SortedOut& o, int64_t cap) {
  if (o.staged == 0) return TAVB_OK;
  TAVB_HIP(hipStreamSynchronize(c->stream));
  const char* base = reinterpret_cast<const char*>(c->h_out.ptr);
  parallel_copy(o.ords + o.done, base, (size_t)o.staged * sizeof(int64_t));
  parallel_copy(o.scs + o.done, base + (size_t)cap * sizeof(int64_t), (size_t)o.staged * sizeof(float));
  o.done += o.staged;
  o.staged = 0;
  return TAVB_OK;
}
// one sorted lookup, over all its groups: the caller's outputs, the totals so far, the staging
struct SortedRun {
  SortedOut o;
  int64_t* out_counts;  // [nq] of the whole batch
  int64_t max_total, stage;
  int64_t total = 0;
  int max_rounds = 0;
};

int start_sorted_run(tavb_ctx* c, int64_t max_total, int64_t* out_ords, float* out_scores, int64_t* out_counts, SortedRun* r) {
  r->o = SortedOut{out_ords, out_scores};
  r->out_counts = out_counts;
  r->max_total = max_total;
  r->stage = c->sort_stage_keys;
  return c->h_out.reserve((size_t)r->stage * (sizeof(int64_t) + sizeof(float)));
}

int end_sorted_run(tavb_ctx* c, SortedRun& r, int64_t* out_total) {
  if (int rc = flush_staged(c, r.o, r.stage)) return rc;
  c->last_topk_refine = r.max_rounds;
  *out_total = r.total;
  return TAVB_OK;
}

// the selection workspace and the pinned words of one group of up to s.per queries
int reserve_sorted_group(tavb_ctx* c, const ScorePlan& s) {
  int64_t chunk;
  const int cblocks = tavb::sorted_blocks(s.n_pos, &chunk);
  if (int rc = c->d_topk.reserve(tavb::topk_head_bytes((int)s.per, s.nb, s.rounds) + (size_t)s.per * cblocks * sizeof(unsigned))) return rc;
  return c->h_sort_info.reserve((size_t)s.per * (4 + cblocks) * sizeof(int32_t));
}

// One group of a sorted lookup: the queries [q0, q0 + n) of the batch, n <= s.per, best k each (k = s.n_pos: every survivor), over the
// s.n_pos positions of d_rows (null: the corpus).  member / bit0: the scoped form of run_score_pass.  remap: the results are base +
// d_rows[position] instead of base + position.
int sorted_group(tavb_ctx* c, const ScorePlan& s, const float* d_q, const float* min_scores /*host*/, const int32_t* d_rows, const uint8_t* member, int bit0,
                 int q0, int n, int64_t k, int64_t base, bool remap, SortedRun& r) {
  const int nb = s.nb, rounds = s.rounds;
  int64_t chunk;
  const int cblocks = tavb::sorted_blocks(s.n_pos, &chunk);
  const size_t head = tavb::topk_head_bytes((int)s.per, nb, rounds);
  const int64_t stage = r.stage, max_total = r.max_total;
  SortedOut& o = r.o;
  int64_t* const out_counts = r.out_counts;
  int64_t& total = r.total;
  int& max_rounds = r.max_rounds;
  {
    unsigned* d_counts = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(c->d_topk.ptr) + head);
    tavb::TopkLaunch t{};
    t.k = (int32_t)k;
    {
      std::optional<Timed> tm;
      if (int rc = run_score_pass(c, s, "sorted", d_q, min_scores, d_rows, q0, n, &t, &tm, member, bit0)) return rc;
      hipError_t e = tavb::launch_sorted_count(t, d_counts, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "sorted count launch failed: %s", hipGetErrorString(e));
    }
    int32_t* meta = reinterpret_cast<int32_t*>(c->h_sort_info.ptr);
    unsigned* counts = reinterpret_cast<unsigned*>(meta + (size_t)n * 4);
    TAVB_HIP(hipMemcpyAsync(meta, reinterpret_cast<char*>(c->d_topk.ptr) + tavb::topk_meta_offset(n, nb, rounds), (size_t)n * 4 * sizeof(int32_t),
                            hipMemcpyDeviceToHost, c->stream));
    TAVB_HIP(hipMemcpyAsync(counts, d_counts, (size_t)n * cblocks * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    TAVB_HIP(hipStreamSynchronize(c->stream));
    int64_t group_total = 0, most = 0;
    for (int q = 0; q < n; ++q) {
      int64_t kept = 0;
      for (int b = 0; b < cblocks; ++b) kept += counts[(size_t)q * cblocks + b];
      group_total += meta[q * 4 + 0];
      most = std::max(most, kept);
      max_rounds = std::max(max_rounds, (int)meta[q * 4 + 1]);
    }
    if (total + group_total > max_total)
      return fail(TAVB_E_INVALID, "the lookup has more than max_total = %lld results (%lld so far)", (long long)max_total,
                  (long long)(total + group_total));
    if (most > 0) {
      if (int rc = c->d_sort_keys.reserve((size_t)most * sizeof(u64_t))) return rc;
      if (int rc = c->d_sort_ws.reserve(tavb::sort_workspace_bytes(most))) return rc;
    }
    for (int q = 0; q < n; ++q) {
      const int64_t need = meta[q * 4 + 0];
      out_counts[q0 + q] = need;
      if (need == 0) continue;
      int64_t kept = 0;
      for (int b = 0; b < cblocks; ++b) kept += counts[(size_t)q * cblocks + b];
      if (kept < need) return fail(TAVB_E_HIP, "sorted lookup: %lld keys kept for %lld results (internal error)", (long long)kept, (long long)need);
      tavb::SortJob j{reinterpret_cast<u64_t*>(c->d_sort_keys.ptr), kept, 4, c->d_sort_ws.ptr, (int)c->sort_small_keys, false};
      {
        Timed tm(c, TAVB_KERNEL_TOPK);
        hipError_t e = tavb::launch_sorted_compact(t, q, d_counts, j.keys, c->stream);
        if (e == hipSuccess) e = tavb::launch_sort_desc(j, c->stream);
        if (e != hipSuccess) return fail(TAVB_E_HIP, "sorted compaction / sort launch failed: %s", hipGetErrorString(e));
      }
      for (int64_t off = 0; off < need;) {
        if (o.staged == stage) {
          if (int rc = flush_staged(c, o, stage)) return rc;
        }
        const int64_t len = std::min(need - off, stage - o.staged);
        char* hb = reinterpret_cast<char*>(c->h_out.ptr);
        Timed tm(c, TAVB_KERNEL_TOPK);
        hipError_t e = tavb::launch_sort_decode(j, off, len, base, reinterpret_cast<int64_t*>(hb) + o.staged,
                                                reinterpret_cast<float*>(hb + (size_t)stage * sizeof(int64_t)) + o.staged, c->stream,
                                                remap ? d_rows : nullptr, remap ? s.n_pos : 0);
        if (e != hipSuccess) return fail(TAVB_E_HIP, "sorted decode launch failed: %s", hipGetErrorString(e));
        o.staged += len;
        off += len;
      }
    }
    total += group_total;
  }
  return TAVB_OK;
}
}  // namespace

// remap: the results are base + d_rows[position] (the one-mask batch: corpus ordinals) instead of base + position
static int search_sorted_impl(tavb_ctx* c, const float* d_q, int nq, int64_t k /*1 .. n_pos*/, const float* min_scores /*host, nq*/,
                              const int32_t* d_rows, int64_t n_pos, int64_t base, int64_t max_total, int64_t* out_ords, float* out_scores,
                              int64_t* out_counts, int64_t* out_total, bool remap = false) {
  ScorePlan s;
  if (int rc = plan_score_pass(c, nq, n_pos, /*refine=*/k < n_pos, &s)) return rc;  // (k = n_pos: every survivor, nothing to refine)
  if (int rc = reserve_sorted_group(c, s)) return rc;
  SortedRun r;
  if (int rc = start_sorted_run(c, max_total, out_ords, out_scores, out_counts, &r)) return rc;
  for (int q0 = 0; q0 < nq; q0 += (int)s.per) {
    if (int rc = sorted_group(c, s, d_q, min_scores, d_rows, nullptr, 0, q0, (int)std::min<int64_t>(s.per, nq - q0), k, base, remap, r)) return rc;
  }
  return end_sorted_run(c, r, out_total);
}

// ---- the same under one scope per query (tavb_search_scoped_sorted): waves and passes as in search_scoped_topk_impl, each sub-group of a
// pass one group of the sorted route over the pass' union list -- its own synchronise, max_total check, compactions, sorts and decodes,
// the decode going through the list to ordinal base + row.  k: 0 = every survivor; per pass it is clamped to the union's length, and
// need = min(k, survivors of the query's own scope) is the boundary search's as it stands.  out_counts arrives zeroed.
static int search_scoped_sorted_impl(tavb_ctx* c, const float* d_q, int nq, int64_t k, const float* min_scores /*host, nq*/, const uint32_t* const* masks,
                                     int64_t base, int64_t max_total, int64_t* out_ords, float* out_scores, int64_t* out_counts, int64_t* out_total) {
  const int per = scoped_topk_per_pass(c);
  const int wave = scoped_wave_queries(c, per);
  SortedRun r;
  if (int rc = start_sorted_run(c, max_total, out_ords, out_scores, out_counts, &r)) return rc;
  for (int w0 = 0; w0 < nq; w0 += wave) {
    const int wn = std::min(wave, nq - w0);
    ScopeWave w;
    if (int rc = scope_wave_unions(c, wn, per, masks + w0, &w)) return rc;
    for (int p = 0; p < w.passes; ++p) {
      const int q0 = w0 + p * per, n = std::min(per, wn - p * per);
      const int64_t n_pos = w.n_union[p];
      if (n_pos == 0) continue;  // every scope of the pass is empty
      const int32_t* list;
      const uint8_t* member;
      if (int rc = scope_wave_lists(c, w, p, &list, &member)) return rc;
      const int64_t kk = (k == 0 || k > n_pos) ? n_pos : k;
      ScorePlan s;
      if (int rc = shape_score_pass(c, n, n_pos, /*refine=*/kk < n_pos, &s)) return rc;
      if (int rc = reserve_sorted_group(c, s)) return rc;
      for (int s0 = 0; s0 < n; s0 += (int)s.per) {
        if (int rc = sorted_group(c, s, d_q, min_scores, list, member, s0, q0 + s0, (int)std::min<int64_t>(s.per, n - s0), kk, base, /*remap=*/true, r)) return rc;
      }
    }
  }
  return end_sorted_run(c, r, out_total);
}

static int check_sorted_args(tavb_ctx* c, int64_t k, int64_t max_total, const void* out_total) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = require_corpus(c)) return rc;
  if (k < 0) return fail(TAVB_E_INVALID, "k must be >= 0 (0 = every survivor)");
  if (max_total < 0) return fail(TAVB_E_INVALID, "max_total must be >= 0");
  if (!out_total) return fail(TAVB_E_INVALID, "null argument");
  return TAVB_OK;
}

int tavb_search_sorted(tavb_ctx* c, const float* queries_host, int32_t nq, int64_t k, const float* min_scores, int64_t max_total, int64_t* out_ordinals,
                       float* out_scores, int64_t* out_counts, int64_t* out_total) {
  if (int rc = check_sorted_args(c, k, max_total, out_total)) return rc;
  if (nq < 0) return fail(TAVB_E_INVALID, "nq must be >= 0");
  *out_total = 0;
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_counts || (max_total > 0 && (!out_ordinals || !out_scores))) return fail(TAVB_E_INVALID, "null argument");
  c->last_topk_refine = 0;
  c->topk_rounds_pending = 0;
  c->last_rows_query = 0;
  c->last_pairs_join = 0;
  for (int q = 0; q < nq; ++q) out_counts[q] = 0;
  if (c->rows == 0) return TAVB_OK;
  DeviceGuard guard(c->device);
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  const int64_t kk = (k == 0 || k > c->rows) ? c->rows : k;
  return search_sorted_impl(c, d_q, nq, kk, min_scores, nullptr, c->rows, c->ordinal_base, max_total, out_ordinals, out_scores, out_counts, out_total);
}

int tavb_search_subset_sorted(tavb_ctx* c, const float* query_host, const int64_t* rows_host, int64_t n_subset, int64_t k, float min_score,
                              int64_t max_total, int64_t* out_positions, float* out_scores, int64_t* out_count) {
  if (int rc = check_sorted_args(c, k, max_total, out_count)) return rc;
  if (n_subset < 0) return fail(TAVB_E_INVALID, "n_subset must be >= 0");
  *out_count = 0;
  if (!query_host || (max_total > 0 && (!out_positions || !out_scores))) return fail(TAVB_E_INVALID, "null argument");
  c->last_topk_refine = 0;
  c->topk_rounds_pending = 0;
  if (n_subset == 0 || c->rows == 0) return TAVB_OK;
  if (!rows_host) return fail(TAVB_E_INVALID, "null rows_host");
  if (n_subset >= 0x7FFFFFFFll) return fail(TAVB_E_UNSUPPORTED, "subset too long");
  DeviceGuard guard(c->device);
  const float* d_q;
  const int32_t* d_rows;
  if (int rc = stage_subset(c, query_host, rows_host, n_subset, &d_q, &d_rows)) return rc;
  const int64_t kk = (k == 0 || k > n_subset) ? n_subset : k;
  int64_t count = 0;
  return search_sorted_impl(c, d_q, 1, kk, &min_score, d_rows, n_subset, 0, max_total, out_positions, out_scores, &count, out_count);
}

// ---- the one-mask batch, sorted: nq queries over one resident row list, corpus ordinals out (the gather route of a masked batch)
int tavb_search_subset_batch_sorted(tavb_ctx* c, const float* queries_host, int32_t nq, const int32_t* dev_rows, int64_t n_subset, int64_t k,
                                    const float* min_scores, int64_t max_total, int64_t* out_ordinals, float* out_scores, int64_t* out_counts,
                                    int64_t* out_total) {
  if (int rc = check_sorted_args(c, k, max_total, out_total)) return rc;
  if (nq < 0) return fail(TAVB_E_INVALID, "nq must be >= 0");
  if (n_subset < 0 || n_subset >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "bad subset length");
  *out_total = 0;
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_counts || (max_total > 0 && (!out_ordinals || !out_scores))) return fail(TAVB_E_INVALID, "null argument");
  note_route(c, 1, /*clear_graph=*/false);  // the gather route of a masked batch
  for (int q = 0; q < nq; ++q) out_counts[q] = 0;
  if (n_subset == 0 || c->rows == 0) return TAVB_OK;
  if (!dev_rows) return fail(TAVB_E_INVALID, "null dev_rows");
  DeviceGuard guard(c->device);
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  const int64_t kk = (k == 0 || k > n_subset) ? n_subset : k;
  return search_sorted_impl(c, d_q, nq, kk, min_scores, dev_rows, n_subset, c->ordinal_base, max_total, out_ordinals, out_scores, out_counts, out_total,
                            /*remap=*/true);
}

// ---- scoped batches beyond the fused selection: one mask per query at any max_hits (search_scoped_topk_impl, search_scoped_sorted_impl);
// "masked_route" = 7 on the large-k route, 8 on the sorted route
int tavb_search_scoped_topk(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                            const float* min_scores, int64_t* out_ordinals, float* out_scores, int32_t* out_counts) {
  bool empty = false;
  if (int rc = check_scoped_args(c, nq, dev_masks, rows, k, TAVB_MAX_LARGE_K, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_ordinals || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  note_route(c, 7);
  if (empty) return empty_counts(out_counts, nq);
  DeviceGuard guard(c->device);
  u64_t* target;
  int32_t* rounds;
  if (int rc = reserve_key_target(c, nq, k, &target, &rounds)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  if (int rc = search_scoped_topk_impl(c, d_q, nq, k, min_scores, dev_masks, 0u, target, target, rounds)) return rc;
  return collect_keys(c, target, nq, k, c->ordinal_base, out_ordinals, out_scores, out_counts, rounds);
}

int tavb_search_scoped_topk_device(tavb_ctx* c, const float* dev_queries, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                                   const float* min_scores, tavb_key* out_keys) {
  bool empty = false;
  if (int rc = check_scoped_args(c, nq, dev_masks, rows, k, TAVB_MAX_LARGE_K, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!dev_queries || !min_scores || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  note_route(c, 7);
  DeviceGuard guard(c->device);
  u64_t* const out = reinterpret_cast<u64_t*>(out_keys);
  if (empty) return fill_empty_keys(c, out, (int64_t)nq * k);
  if (int rc = c->h_topk_rounds.reserve((size_t)nq * sizeof(int32_t))) return rc;
  // (the finish kernels write positions into d_out and the remaps turn them into ordinal_base + row on the way to out_keys: a pinned
  //  out_keys is written once and never read over PCIe)
  if (int rc = c->d_out.reserve((size_t)nq * k * sizeof(u64_t))) return rc;
  if (int rc = search_scoped_topk_impl(c, dev_queries, nq, k, min_scores, dev_masks, (uint32_t)c->ordinal_base, reinterpret_cast<u64_t*>(c->d_out.ptr), out,
                                       reinterpret_cast<int32_t*>(c->h_topk_rounds.ptr)))
    return rc;
  c->topk_rounds_pending = nq;
  return TAVB_OK;
}

int tavb_search_scoped_sorted(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t k,
                              const float* min_scores, int64_t max_total, int64_t* out_ordinals, float* out_scores, int64_t* out_counts,
                              int64_t* out_total) {
  if (int rc = check_sorted_args(c, k, max_total, out_total)) return rc;
  bool empty = false;
  if (int rc = check_scoped_args(c, nq, dev_masks, rows, /*k: checked above*/ 1, TAVB_MAX_LARGE_K, &empty)) return rc;
  *out_total = 0;
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_counts || (max_total > 0 && (!out_ordinals || !out_scores))) return fail(TAVB_E_INVALID, "null argument");
  note_route(c, 8);
  for (int q = 0; q < nq; ++q) out_counts[q] = 0;
  if (empty) return TAVB_OK;
  DeviceGuard guard(c->device);
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  return search_scoped_sorted_impl(c, d_q, nq, k, min_scores, dev_masks, c->ordinal_base, max_total, out_ordinals, out_scores, out_counts, out_total);
}

// ---- the best k messages: per-message best score and top-k on the device (search_top_messages_impl)
int tavb_search_top_messages(tavb_ctx* c, const float* queries_host, int32_t nq, int32_t k, const float* min_scores, const int32_t* dev_rows,
                             int64_t n_rows, int64_t* out_messages, float* out_scores, int32_t* out_counts) {
  bool empty = false;
  if (int rc = check_top_messages_args(c, k, dev_rows, n_rows, &empty)) return rc;
  if (nq < 0) return fail(TAVB_E_INVALID, "nq must be >= 0");
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_messages || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  note_route(c, c->masked_route);  // ("masked_route" stays: this is no masked lookup)
  if (empty) return empty_counts(out_counts, nq);
  DeviceGuard guard(c->device);
  u64_t* target;
  int32_t* rounds;
  if (int rc = reserve_key_target(c, nq, k, &target, &rounds)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  if (int rc = search_top_messages_impl(c, d_q, nq, k, min_scores, dev_rows, n_rows, target, rounds)) return rc;
  return collect_keys(c, target, nq, k, 0, out_messages, out_scores, out_counts, rounds);
}

int tavb_search_top_messages_device(tavb_ctx* c, const float* dev_queries, int32_t nq, int32_t k, const float* min_scores, const int32_t* dev_rows,
                                    int64_t n_rows, tavb_key* out_keys) {
  bool empty = false;
  if (int rc = check_top_messages_args(c, k, dev_rows, n_rows, &empty)) return rc;
  if (nq < 1) return fail(TAVB_E_INVALID, "nq must be >= 1");
  if (!dev_queries || !min_scores || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  note_route(c, c->masked_route);  // ("masked_route" stays: this is no masked lookup)
  DeviceGuard guard(c->device);
  u64_t* const out = reinterpret_cast<u64_t*>(out_keys);
  if (empty) return fill_empty_keys(c, out, (int64_t)nq * k);
  if (int rc = c->h_topk_rounds.reserve((size_t)nq * sizeof(int32_t))) return rc;
  if (int rc = search_top_messages_impl(c, dev_queries, nq, k, min_scores, dev_rows, n_rows, out, reinterpret_cast<int32_t*>(c->h_topk_rounds.ptr))) return rc;
  c->topk_rounds_pending = nq;
  return TAVB_OK;
}

// ---- the top-messages lists of several shards -> one list per query (merge_top_messages_impl)
int tavb_merge_top_messages_device(tavb_ctx* c, const tavb_key* dev_lists, int32_t n_lists, int32_t nq, int32_t k, int64_t n_messages, tavb_key* out_keys) {
  if (int rc = check_ctx(c)) return rc;
  const bool query_major = n_lists < 0;
  if (query_major) n_lists = -n_lists;
  if (n_lists < 1 || n_lists > 64 || nq < 1 || nq > 65535 || k < 1 || k > TAVB_MAX_LARGE_K)
    return fail(TAVB_E_INVALID, "bad merge shape (1 .. 64 lists of 1 .. %d keys, 1 .. 65535 queries)", TAVB_MAX_LARGE_K);
  if (n_messages < 1) return fail(TAVB_E_INVALID, "n_messages must be >= 1");
  if (n_messages >= 0x7FFFFFFFll) return fail(TAVB_E_UNSUPPORTED, "top-messages keys hold message ordinals: n_messages must be < 2^31 - 1");
  if (!dev_lists || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  DeviceGuard guard(c->device);
  c->topk_rounds_pending = 0;
  if (int rc = c->h_topk_rounds.reserve((size_t)nq * sizeof(int32_t))) return rc;
  if (int rc = merge_top_messages_impl(c, reinterpret_cast<const u64_t*>(dev_lists), n_lists, nq, k, query_major, n_messages, reinterpret_cast<u64_t*>(out_keys),
                                       reinterpret_cast<int32_t*>(c->h_topk_rounds.ptr)))
    return rc;
  c->topk_rounds_pending = nq;
  return TAVB_OK;
}

// ---- the best k messages on the 32/64-query tile (search_top_messages_tile_impl)
// check_top_messages_args (no row list), the one mask's shape as tavb_search_masked_batch checks it, and the tile's own refusals
static int check_top_messages_tile_args(tavb_ctx* c, int32_t nq, int32_t k, const uint32_t* dev_bits, int64_t rows, int64_t first_row, int64_t last_row, bool* empty) {
  if (int rc = check_top_messages_args(c, k, nullptr, 0, empty)) return rc;
  if (nq < 0) return fail(TAVB_E_INVALID, "nq must be >= 0");
  const int row_bytes = c->dim * (c->dtype == TAVB_F16 ? 2 : 4);
  if (row_bytes % 64 != 0)
    return fail(TAVB_E_UNSUPPORTED, "the top-messages tile serves rows of a multiple of 64 bytes (%d bytes): use tavb_search_top_messages", row_bytes);
  if ((reinterpret_cast<uintptr_t>(c->row_to_msg) & 63) != 0)
    return fail(TAVB_E_UNSUPPORTED, "the top-messages tile reads the row -> message map 16 entries at a time: the map must be 64-byte aligned");
  if (dev_bits) {
    if ((reinterpret_cast<uintptr_t>(dev_bits) & 3) != 0) return fail(TAVB_E_INVALID, "misaligned mask (dev_bits must be 4-byte aligned)");
    if (rows != c->rows) return fail(TAVB_E_INVALID, "the mask covers %lld rows, the corpus has %lld", (long long)rows, (long long)c->rows);
    if (first_row > last_row) *empty = true;
    else if (first_row < 0 || last_row >= rows) return fail(TAVB_E_INVALID, "mask span [%lld, %lld] outside the corpus", (long long)first_row, (long long)last_row);
  }
  return TAVB_OK;
}

int tavb_search_top_messages_tile(tavb_ctx* c, const float* queries_host, int32_t nq, int32_t k, const float* min_scores, const uint32_t* dev_bits, int64_t rows,
                                  int64_t first_row, int64_t last_row, int64_t* out_messages, float* out_scores, int32_t* out_counts) {
  bool empty = false;
  if (int rc = check_top_messages_tile_args(c, nq, k, dev_bits, rows, first_row, last_row, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_messages || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  note_route(c, 10);  // a top-messages batch on the 32/64-query tile
  if (empty) return empty_counts(out_counts, nq);
  DeviceGuard guard(c->device);
  u64_t* target;
  int32_t* rounds;
  if (int rc = reserve_key_target(c, nq, k, &target, &rounds)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  if (int rc = search_top_messages_tile_impl(c, d_q, nq, k, min_scores, dev_bits, first_row, last_row, target, rounds)) return rc;
  return collect_keys(c, target, nq, k, 0, out_messages, out_scores, out_counts, rounds);
}

int tavb_search_top_messages_tile_device(tavb_ctx* c, const float* dev_queries, int32_t nq, int32_t k, const float* min_scores, const uint32_t* dev_bits,
                                         int64_t rows, int64_t first_row, int64_t last_row, tavb_key* out_keys) {
  bool empty = false;
  if (int rc = check_top_messages_tile_args(c, nq, k, dev_bits, rows, first_row, last_row, &empty)) return rc;
  if (nq < 1) return fail(TAVB_E_INVALID, "nq must be >= 1");
  if (!dev_queries || !min_scores || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  note_route(c, 10);
  DeviceGuard guard(c->device);
  u64_t* const out = reinterpret_cast<u64_t*>(out_keys);
  if (empty) return fill_empty_keys(c, out, (int64_t)nq * k);
  if (int rc = c->h_topk_rounds.reserve((size_t)nq * sizeof(int32_t))) return rc;
  if (int rc = search_top_messages_tile_impl(c, dev_queries, nq, k, min_scores, dev_bits, first_row, last_row, out, reinterpret_cast<int32_t*>(c->h_topk_rounds.ptr)))
    return rc;
  c->topk_rounds_pending = nq;
  return TAVB_OK;
}

// ---- the best k messages under one scope per query (search_scoped_top_messages_impl)
// check_top_messages_args (no row list) and check_scoped_args; *empty: nothing to scan
static int check_scoped_top_messages_args(tavb_ctx* c, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k, bool* empty) {
  bool no_messages = false, no_rows = false;
  if (int rc = check_top_messages_args(c, k, nullptr, 0, &no_messages)) return rc;
  if (int rc = check_scoped_args(c, nq, dev_masks, rows, k, TAVB_MAX_LARGE_K, &no_rows)) return rc;
  *empty = no_messages || no_rows;
  return TAVB_OK;
}

int tavb_search_top_messages_scoped(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                                    const float* min_scores, int64_t* out_messages, float* out_scores, int32_t* out_counts) {
  bool empty = false;
  if (int rc = check_scoped_top_messages_args(c, nq, dev_masks, rows, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_messages || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  note_route(c, 9);  // a scoped top-messages batch
  if (empty) return empty_counts(out_counts, nq);
  DeviceGuard guard(c->device);
  u64_t* target;
  int32_t* rounds;
  if (int rc = reserve_key_target(c, nq, k, &target, &rounds)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  if (int rc = search_scoped_top_messages_impl(c, d_q, nq, k, min_scores, dev_masks, target, rounds)) return rc;
  return collect_keys(c, target, nq, k, 0, out_messages, out_scores, out_counts, rounds);
}

int tavb_search_top_messages_scoped_device(tavb_ctx* c, const float* dev_queries, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                                           const float* min_scores, tavb_key* out_keys) {
  bool empty = false;
  if (int rc = check_scoped_top_messages_args(c, nq, dev_masks, rows, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!dev_queries || !min_scores || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  note_route(c, 9);  // a scoped top-messages batch
  DeviceGuard guard(c->device);
  u64_t* const out = reinterpret_cast<u64_t*>(out_keys);
  if (empty) return fill_empty_keys(c, out, (int64_t)nq * k);
  if (int rc = c->h_topk_rounds.reserve((size_t)nq * sizeof(int32_t))) return rc;
  if (int rc = search_scoped_top_messages_impl(c, dev_queries, nq, k, min_scores, dev_masks, out, reinterpret_cast<int32_t*>(c->h_topk_rounds.ptr))) return rc;
  c->topk_rounds_pending = nq;
  return TAVB_OK;
}

int tavb_sort_keys_device(tavb_ctx* c, tavb_key* dev_keys, int64_t n) {
  if (int rc = check_ctx(c)) return rc;
  if (n < 0 || n >= ((int64_t)1 << 32)) return fail(TAVB_E_INVALID, "n must be 0 .. 2^32 - 1");
  if (n == 0) return TAVB_OK;
  if (!dev_keys) return fail(TAVB_E_INVALID, "null dev_keys");
  DeviceGuard guard(c->device);
  if (int rc = c->d_sort_ws.reserve(tavb::sort_workspace_bytes(n))) return rc;
  tavb::SortJob j{reinterpret_cast<u64_t*>(dev_keys), n, 0, c->d_sort_ws.ptr, (int)c->sort_small_keys, false};
  {
    Timed tm(c, TAVB_KERNEL_TOPK);
    hipError_t e = tavb::launch_sort_desc(j, c->stream);
    if (e == hipSuccess) e = tavb::launch_sort_copy_back(j, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "sort launch failed: %s", hipGetErrorString(e));
  }
  TAVB_HIP(hipStreamSynchronize(c->stream));
  return TAVB_OK;
}

}  // extern "C"

namespace tavb {
namespace host __attribute__((visibility("hidden"))) {
int search_sorted_device(tavb_ctx* c, const float* d_q, int nq, int64_t k, const float* min_scores, int64_t base, int64_t max_total, int64_t* out_ords,
                         float* out_scores, int64_t* out_counts, int64_t* out_total) {
  return search_sorted_impl(c, d_q, nq, k, min_scores, nullptr, c->rows, base, max_total, out_ords, out_scores, out_counts, out_total);
}
}  // namespace host
}  // namespace tavb
