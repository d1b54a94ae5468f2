// The fused-k lookups of the C ABI (include/tavb.h): the host-synchronous and device-resident tavb_search_* entry points up to
// TAVB_MAX_FUSED_K keys per query, the one-launch form and the captured graph of a small corpus, the host merges, the message re-rank -- and
// the staging and the small helpers every lookup file shares (declared in tavb_ctx.h).  The large-k and sorted forms are in
// tavb_lookup_topk.hip, the batched resident subset and the masked and scoped batches in tavb_lookup_masked.hip, the row edits in
// tavb_row_edits.hip, the row masks in tavb_mask_entry.hip.  Host code only -- a device-resident batch is routed by tavb_route.hip, the
// kernels live in tavb_scan.hip / tavb_misc.hip.

#include <functional>

#include "tavb_ctx.h"

using namespace tavb::host;

namespace {

int check_search_args(tavb_ctx* c, int k) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = require_corpus(c)) return rc;
  if (k < 1) return fail(TAVB_E_INVALID, "k must be >= 1 (got %d)", k);
  if (k > TAVB_MAX_FUSED_K)
    return fail(TAVB_E_UNSUPPORTED, "k=%d exceeds the fused-select limit %d; page with tavb_search_after / tavb_search_subset_after", k,
                TAVB_MAX_FUSED_K);
  return TAVB_OK;
}

int cursor_key(float after_score, int64_t after_index, int64_t limit, u64_t* out) {
  if (!(after_score >= 0.0f && after_score <= 1.0f)) return fail(TAVB_E_INVALID, "cursor score must be in [0, 1]");
  if (after_index < 0 || after_index >= limit) return fail(TAVB_E_INVALID, "cursor index out of range");
  *out = host_key(after_score, (uint32_t)after_index);
  return TAVB_OK;
}

}  // namespace

namespace tavb {
namespace host __attribute__((visibility("hidden"))) {

// ---- staging: the caller's queries (and a subset's rows) -> pinned h_stage -> d_queries (d_rows)

// [nq, dim] queries -> h_stage; *d_q = where submit_queries puts them.  Nothing is submitted here: the one-launch forms (direct_one_launch)
// enqueue the copy only when the query does not ride in the kernel arguments.
int stage_queries_host(tavb_ctx* c, const float* queries_host, int nq, const float** d_q) {
  const size_t qbytes = (size_t)nq * c->dim * sizeof(float);
  if (int rc = c->h_stage.reserve(qbytes)) return rc;
  if (int rc = c->d_queries.reserve(qbytes)) return rc;
  parallel_copy(c->h_stage.ptr, queries_host, qbytes);  // (a 1024 x 1536 batch is 6 MiB: 0.6 ms on one core, a few threads from 4 MiB up)
  // staged_overflow (tavb_ctx.h): an element of magnitude >= 65520 rounds to an fp16 infinity; +-inf and NaN lie above it.  One compare
  // per element on the bits without the sign, right behind the copy; an OR reduction with no branch, so the compiler may vectorise it.
  const uint32_t* const bits = reinterpret_cast<const uint32_t*>(c->h_stage.ptr);
  const size_t n = (size_t)nq * c->dim;
  uint32_t over = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t a = bits[i] & 0x7FFFFFFFu;
    over |= (uint32_t)(a >= 0x477FF000u);  // 65520.0f and beyond
  }
  c->staged_overflow = over != 0;
  *d_q = reinterpret_cast<const float*>(c->d_queries.ptr);
  return TAVB_OK;
}

hipError_t submit_queries(tavb_ctx* c, int nq) {
  return hipMemcpyAsync(c->d_queries.ptr, c->h_stage.ptr, (size_t)nq * c->dim * sizeof(float), hipMemcpyHostToDevice, c->stream);
}

int stage_queries(tavb_ctx* c, const float* queries_host, int nq, const float** d_q) {
  if (int rc = stage_queries_host(c, queries_host, nq, d_q)) return rc;
  TAVB_HIP(submit_queries(c, nq));
  return TAVB_OK;
}

// One query over a subset of the rows: the rows (int64 on the host, checked against the corpus; int32 on the device) lead h_stage, the query
// follows at the next multiple of 256 bytes; the rows' copy is enqueued first.  The caller has checked 0 < n_subset < 2^31 - 1 (the entry
// points report a subset that is too long each in its own way).
int stage_subset(tavb_ctx* c, const float* query_host, const int64_t* rows_host, int64_t n_subset, const float** d_q, const int32_t** d_rows) {
  const size_t qbytes = (size_t)c->dim * sizeof(float);
  const size_t rbytes = (size_t)n_subset * sizeof(int32_t);
  const size_t qoff = (rbytes + 255) & ~(size_t)255;
  if (int rc = c->h_stage.reserve(qoff + qbytes)) return rc;
  if (int rc = c->d_queries.reserve(qbytes)) return rc;
  if (int rc = c->d_rows.reserve(rbytes)) return rc;
  int32_t* r32 = reinterpret_cast<int32_t*>(c->h_stage.ptr);
  for (int64_t i = 0; i < n_subset; ++i) {
    const int64_t r = rows_host[i];
    if (r < 0 || r >= c->rows) return fail(TAVB_E_INVALID, "subset row %lld out of range [0, %lld)", (long long)r, (long long)c->rows);
    r32[i] = (int32_t)r;
  }
  char* q_stage = reinterpret_cast<char*>(c->h_stage.ptr) + qoff;
  memcpy(q_stage, query_host, qbytes);
  c->staged_overflow = false;  // (one query over a row list: the streaming kernels, fp32 throughout)
  TAVB_HIP(hipMemcpyAsync(c->d_rows.ptr, c->h_stage.ptr, rbytes, hipMemcpyHostToDevice, c->stream));
  TAVB_HIP(hipMemcpyAsync(c->d_queries.ptr, q_stage, qbytes, hipMemcpyHostToDevice, c->stream));
  *d_q = reinterpret_cast<const float*>(c->d_queries.ptr);
  *d_rows = reinterpret_cast<const int32_t*>(c->d_rows.ptr);
  return TAVB_OK;
}

// ---- what the entry points of every lookup file repeat
int check_key_ordinals(const tavb_ctx* c, bool device_resident) {
  if (c->ordinal_base + c->rows < 0xFFFFFFFFll) return TAVB_OK;
  return fail(TAVB_E_UNSUPPORTED, "%skeys hold 32-bit ordinals: ordinal_base + rows must be < 2^32 - 1", device_resident ? "device-resident " : "");
}

int fill_empty_keys(tavb_ctx* c, u64_t* out, int64_t n) {
  const hipError_t e = tavb::launch_fill_keys(out, n, 0ull, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "fill launch failed: %s", hipGetErrorString(e));
  return TAVB_OK;
}

int sync_decode(tavb_ctx* c, int nq, int k, int64_t base, int64_t* ordinals, float* scores, int32_t* counts) {
  TAVB_HIP(hipStreamSynchronize(c->stream));
  decode(reinterpret_cast<const u64_t*>(c->h_out.ptr), nq, k, base, ordinals, scores, counts);
  return TAVB_OK;
}

int reserve_key_target(tavb_ctx* c, int nq, int k, u64_t** target, int32_t** rounds) {
  const size_t n_keys = (size_t)nq * k;
  if (rounds) {
    if (int rc = reserve_topk_out(c, nq, k, target, rounds)) return rc;
  } else {
    if (int rc = c->h_out.reserve(n_keys * sizeof(u64_t))) return rc;
    *target = reinterpret_cast<u64_t*>(c->h_out.ptr);
  }
  if (n_keys <= kPinnedKeysMax) return TAVB_OK;
  if (int rc = c->d_out.reserve(n_keys * sizeof(u64_t))) return rc;
  *target = reinterpret_cast<u64_t*>(c->d_out.ptr);
  return TAVB_OK;
}

int collect_keys(tavb_ctx* c, const u64_t* target, int nq, int k, int64_t base, int64_t* ordinals, float* scores, int32_t* counts, const int32_t* rounds) {
  if (target != c->h_out.ptr) TAVB_HIP(hipMemcpyAsync(c->h_out.ptr, target, (size_t)nq * k * sizeof(u64_t), hipMemcpyDeviceToHost, c->stream));
  if (int rc = sync_decode(c, nq, k, base, ordinals, scores, counts)) return rc;
  if (rounds) note_rounds(c, rounds, nq);
  return TAVB_OK;
}

int check_mask_list(const uint32_t* const* masks, int n, const char* who) {
  for (int j = 0; j < n; ++j) {
    if (!masks[j]) return fail(TAVB_E_INVALID, "%s %d is null", who, j);
    if ((reinterpret_cast<uintptr_t>(masks[j]) & 3) != 0) return fail(TAVB_E_INVALID, "%s %d must be 4-byte aligned", who, j);
  }
  return TAVB_OK;
}

int remap_key_rows(tavb_ctx* c, const u64_t* in, u64_t* out, int64_t n, const int32_t* rows, int64_t n_rows, uint32_t base) {
  const hipError_t e = tavb::launch_remap_positions(in, out, n, rows, n_rows, base, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "remap launch failed: %s", hipGetErrorString(e));
  return TAVB_OK;
}

// ---- what the message lookups of both lookup files repeat
int check_message_map(const tavb_ctx* c) {
  if (!c->row_to_msg && c->rows > 0) return fail(TAVB_E_NO_CORPUS, "no row -> message map set (call tavb_set_row_messages first)");
  if (c->row_to_msg_rows < c->rows) return fail(TAVB_E_INVALID, "the row -> message map covers %lld rows, the corpus has %lld", (long long)c->row_to_msg_rows, (long long)c->rows);
  return TAVB_OK;
}

int check_message_args(tavb_ctx* c, int k, int32_t max_messages) {
  if (int rc = check_search_args(c, k)) return rc;
  if (int rc = check_message_map(c)) return rc;
  if (max_messages < 0) return fail(TAVB_E_INVALID, "max_messages must be >= 0");
  return TAVB_OK;
}

int stage_accept_bitmap(tavb_ctx* c, const int32_t* accept_msgs_host, int64_t n_accept, const uint32_t** d_bits) {
  const size_t words = (size_t)((c->n_messages + 31) / 32) + 1;
  if (int rc = c->d_bits.reserve(words * 4)) return rc;
  TAVB_HIP(hipMemsetAsync(c->d_bits.ptr, 0, words * 4, c->stream));
  if (n_accept > 0) {
    if (int rc = c->d_accept.reserve((size_t)n_accept * 4)) return rc;
    // (pageable source: the copy is staged by the runtime before the call returns)
    TAVB_HIP(hipMemcpyAsync(c->d_accept.ptr, accept_msgs_host, (size_t)n_accept * 4, hipMemcpyHostToDevice, c->stream));
    hipError_t e = tavb::launch_accept_bitmap(reinterpret_cast<const int32_t*>(c->d_accept.ptr), n_accept, reinterpret_cast<uint32_t*>(c->d_bits.ptr),
                                              c->n_messages, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "bitmap launch failed: %s", hipGetErrorString(e));
  }
  *d_bits = reinterpret_cast<const uint32_t*>(c->d_bits.ptr);
  return TAVB_OK;
}

}  // namespace host
}  // namespace tavb

namespace {

// ---- the one-launch lookup of a small corpus or subset (tavb_search_batch, tavb_search_subset_resident; the callers decide whether, and
// cut the grid): the scan's per-workgroup lists [p.nq][g.blocks][p.k] go straight into pinned host memory and are merged here.  The queries
// are in h_stage (stage_queries_host), not submitted yet.
int direct_one_launch(tavb_ctx* c, tavb::ScanParams& p, const tavb::ScanGeometry& g, const float* queries_host, bool grouped, int64_t base,
                      int64_t* out_ordinals, float* out_scores, int32_t* out_counts) {
  const int nq = p.nq, k = p.k;
  const size_t list_keys = (size_t)nq * g.blocks * k;
  if (int rc = c->h_lists.reserve((list_keys + (size_t)nq * k) * sizeof(u64_t))) return rc;  // + the merged keys
  p.lists = reinterpret_cast<u64_t*>(c->h_lists.ptr);  // [nq][blocks][k]
  {
    // one 1536-wide query (the embedding size typeagent runs at): it rides in the kernel arguments -- one submission, no copy in front of the launch
    hipError_t e = hipSuccess;
    bool launched = false;
    if (c->inline_query && nq == 1) {
      Timed t(c, TAVB_KERNEL_SCAN);
      launched = tavb::launch_scan_inline_query(p, g, c->stream, queries_host, &c->last_tier, &e);
    }
    if (!launched) {
      TAVB_HIP(submit_queries(c, nq));
      Timed t(c, TAVB_KERNEL_SCAN);
      e = tavb::launch_scan(p, g, c->stream, &c->last_tier);
    }
    if (e != hipSuccess) return fail(TAVB_E_HIP, "scan kernel launch failed: %s", hipGetErrorString(e));
    c->last_direct = launched ? 2 : (grouped ? 3 : 1);
  }
  TAVB_HIP(hipStreamSynchronize(c->stream));
  tavb_key* merged = reinterpret_cast<tavb_key*>(c->h_lists.ptr) + list_keys;
  // The lists were just written by the device: every cache line of them is a miss to DRAM for this core (~100 ns), and a merge hops between
  // its lists -- 16 lines per query one after the other were 1.6 us per query, 51 us of a 32-term batch.  The heads of the NEXT query's lists
  // are prefetched while this one is merged (two lines per list: the merge rarely reads further), so the misses overlap.
  const tavb_key* all = reinterpret_cast<const tavb_key*>(c->h_lists.ptr);
  auto prefetch_query = [&](int q) {
    const tavb_key* base = all + (size_t)q * g.blocks * k;
    const int n = std::min(g.blocks, 256);
    for (int l = 0; l < n; ++l) {
      __builtin_prefetch(base + (size_t)l * k);
      if (k > 8 && g.blocks <= 64) __builtin_prefetch(base + (size_t)l * k + 8);
    }
  };
  prefetch_query(0);
  for (int q = 0; q < nq; ++q) {
    if (q + 1 < nq) prefetch_query(q + 1);
    if (int rc = tavb_merge_keys_host(all + (size_t)q * g.blocks * k, g.blocks, 1, k, merged + (size_t)q * k)) return rc;
  }
  decode(reinterpret_cast<const u64_t*>(merged), nq, k, base, out_ordinals, out_scores, out_counts);
  return TAVB_OK;
}

// ---- small corpora (tavb_ctx::SmallGraph), one query: the captured (H2D copy, scan, merge) graph -- one submission instead of three.
// The slot of this shape (a new shape takes the least recently used one), a capture whose workspaces have moved since dropped;
// slot->exec: ready to replay.
tavb_ctx::SmallGraph* graph_slot(tavb_ctx* c, int k, float min_score) {
  uint32_t thr_bits;
  memcpy(&thr_bits, &min_score, sizeof thr_bits);
  tavb_ctx::SmallGraph* slot = nullptr;
  const unsigned long long geom_tag = ((unsigned long long)c->geom.blocks << 40) ^ ((unsigned long long)c->geom.waves << 32) ^ ((unsigned long long)c->geom.unroll << 24) ^
                                      ((unsigned long long)c->geom.nt << 16) ^ ((unsigned long long)c->geom.pipe << 8) ^ (unsigned long long)c->geom.tier;
  tavb_ctx::SmallGraph* oldest = &c->graphs[0];
  for (auto& g : c->graphs) {
    if (g.corpus == c->corpus && g.rows == c->rows && g.dim == c->dim && g.dtype == c->dtype && g.k == k && g.thr_bits == thr_bits && g.geom_tag == geom_tag) slot = &g;
    if (g.last_used < oldest->last_used) oldest = &g;
  }
  if (!slot) {  // a new shape takes the least recently used slot
    slot = oldest;
    if (slot->exec) (void)hipGraphExecDestroy(slot->exec);
    *slot = tavb_ctx::SmallGraph{};
    slot->corpus = c->corpus;
    slot->rows = c->rows;
    slot->dim = c->dim;
    slot->dtype = c->dtype;
    slot->k = k;
    slot->thr_bits = thr_bits;
    slot->geom_tag = geom_tag;
  }
  slot->last_used = ++c->graph_clock;
  if (slot->exec && slot->epoch != g_alloc_epoch) {  // a workspace moved since the capture: the graph holds stale pointers
    (void)hipGraphExecDestroy(slot->exec);
    slot->exec = nullptr;
    slot->seen = 1;
  }
  return slot;
}

// The H2D copy of the staged queries and their dispatch into h_out.  With a slot whose shape has been seen before both are captured, not
// run, and the graph instantiated from the capture is launched instead.
int dispatch_staged(tavb_ctx* c, tavb_ctx::SmallGraph* slot, const float* d_q, int nq, int k, const float* min_scores) {
  u64_t* const out = reinterpret_cast<u64_t*>(c->h_out.ptr);
  const bool capture = slot != nullptr && slot->seen >= 1;  // (the first call of a shape sizes the workspaces: no allocation may happen inside a capture)
  if (slot) ++slot->seen;
  if (capture) TAVB_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  const hipError_t copy_err = submit_queries(c, nq);
  const int rc = copy_err == hipSuccess ? tavb_search_device_dispatch(c, d_q, nq, k, min_scores, 0u, out)
                                        : fail(TAVB_E_HIP, "hipMemcpyAsync of the query failed: %s", hipGetErrorString(copy_err));
  if (!capture) return rc;
  hipGraph_t graph = nullptr;
  hipError_t e = hipStreamEndCapture(c->stream, &graph);
  if (rc == TAVB_OK && e == hipSuccess && graph) {
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (e == hipSuccess) {
      slot->exec = exec;
      slot->epoch = g_alloc_epoch;
    }
  }
  if (graph) (void)hipGraphDestroy(graph);
  if (rc) return rc;
  if (!slot->exec) {  // capture or instantiation failed: this shape stays on the plain path
    (void)hipGetLastError();
    slot->seen = -1000000;
    TAVB_HIP(submit_queries(c, nq));
    return tavb_search_device_dispatch(c, d_q, nq, k, min_scores, 0u, out);
  }
  TAVB_HIP(hipGraphLaunch(slot->exec, c->stream));  // nothing ran during the capture: this is the lookup
  c->last_graph = 1;
  return TAVB_OK;
}

}  // namespace

extern "C" {

int tavb_search_batch(tavb_ctx* c, const float* queries_host, int32_t nq, int32_t k, const float* min_scores,
                      int64_t* out_ordinals, float* out_scores, int32_t* out_counts) {
  if (int rc = check_search_args(c, k)) return rc;
  if (nq < 0) return fail(TAVB_E_INVALID, "nq must be >= 0");
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_ordinals || !out_scores || !out_counts)
    return fail(TAVB_E_INVALID, "null argument");
  if (c->rows == 0) {
    for (int q = 0; q < nq; ++q) out_counts[q] = 0;
    return TAVB_OK;
  }
  DeviceGuard guard(c->device);
  const float* d_q;
  if (int rc = stage_queries_host(c, queries_host, nq, &d_q)) return rc;
  if (int rc = c->h_out.reserve((size_t)nq * k * sizeof(u64_t))) return rc;
  c->last_graph = 0;
  c->last_direct = 0;
  c->last_rows_query = 0;
  c->last_pairs_join = 0;
  // ---- small corpus, one query: replay the captured (H2D, scan, merge) graph -- one submission instead of three
  const int64_t corpus_bytes = c->rows * c->dim * (c->dtype == TAVB_F16 ? 2 : 4);
  const bool streaming = nq == 1 && !(c->dtype == TAVB_F32 && c->f32_shadow >= 2 && corpus_bytes >= c->f32_shadow_min_bytes);
  tavb_ctx::SmallGraph* slot = nullptr;
  if (streaming && !c->profiling && c->graph_max_bytes > 0 && corpus_bytes <= c->graph_max_bytes) {
    slot = graph_slot(c, k, min_scores[0]);
    if (slot->exec) {
      TAVB_HIP(hipGraphLaunch(slot->exec, c->stream));
      if (int rc = sync_decode(c, nq, k, c->ordinal_base, out_ordinals, out_scores, out_counts)) return rc;
      c->last_graph = 1;
      return TAVB_OK;
    }
  }
  // ---- small corpus (the scale typeagent itself runs at: ~1.3k .. 10k rows), one query or a FEW (batched related-term lookups,
  //      adapters.install_batched_lookup_terms): ONE launch.  The scan's per-workgroup lists go straight into pinned host memory and are merged
  //      here -- the second launch that merged them on the device cost 11.8 us of a 41 us lookup (profiles/r03_latency_cfg1.md), and a batch of
  //      2 .. 8 queries took 36 .. 110 us through the device merge or the 32-query MFMA tile (profiles/r04_latency_small.md).  The grid is cut to
  //      what keeps the lists within `small_direct_keys` keys (8192 = 64 KiB over PCIe; twice that for a batch): 163 workgroups at k = 50,
  //      all of them at k <= 32.  A batch takes this path when its share of that budget still covers the rows in two rounds of the grid, and on
  //      fp16 corpora up to 4 queries: beyond that the multi-query scan (6 us more per query) loses to the 32-query tile (measured).
  //      Batches of up to `direct_group_max_nq` (128) queries take it in its GROUPED form (end of round 6): gridDim.y query groups of `group` queries each
  //      (ScanParams::group), every group a pass of its own over the rows -- which sit in L2 after the first one (workgroup (x, y) runs on XCD
  //      x % 8 for every y) -- wherever plan_direct_group expects it to beat the tiles.  Until then 9 .. 64 queries (5+ on fp16) went to
  //      the 32/64-query tile or the wide tile, both several launches and, on a corpus of a few thousand rows, one or two busy CUs:
  //      32 queries over 1000 fp32 rows 141 -> 52 us, 64 over 1000 fp16 rows 153 -> 62 us, the answers now the sequential lookups' bit for bit.
  const int direct_nq_max = (k > 64) ? 4 : TAVB_MAX_STREAM_QUERIES;  // queries one pass of the streaming kernels serves
  const bool shadow2 = c->dtype == TAVB_F32 && c->f32_shadow >= 2 && corpus_bytes >= c->f32_shadow_min_bytes;
  const bool few = nq >= 2 && nq <= direct_nq_max && !shadow2;
  const bool many = nq >= 2 && nq <= std::min<int64_t>(c->direct_group_max_nq, TAVB_MAX_GROUPED_QUERIES) && !shadow2 && k <= 64;  // (fitted for the 64-deep lists only)
  if ((streaming || few || many) && slot == nullptr && c->small_direct_bytes > 0 && corpus_bytes <= c->small_direct_bytes) {
    tavb::ScanGeometry g = clamped_geometry(c);
    const int full_blocks = scan_blocks_for(c, c->rows, g.waves, g.unroll);
    // the grouped form (plan_direct_group): a launch of (row workgroups) x (query groups), every group a pass of its own over the rows
    DirectGroupPlan plan{};
    if (many) plan = plan_direct_group(c, nq, k, full_blocks, /*host=*/true);
    const bool grouped = many && plan.worth;
    bool take = grouped;
    if (grouped) {
      g.blocks = plan.blocks;
      g.nt = 0;  // the rows are read again by every further group: no evict-first hint (16 queries over 10k fp32 rows: scan 47 -> 41 us)
    }
    if (!take && (streaming || few)) {
      const int64_t budget = c->small_direct_keys * (nq > 1 ? 2 : 1);
      g.blocks = std::min(full_blocks, (int)std::max<int64_t>(8, budget / ((int64_t)k * nq)));
      const int64_t rounds = (c->rows + (int64_t)g.blocks * g.waves * g.unroll - 1) / ((int64_t)g.blocks * g.waves * g.unroll);
      // one query: only while the cut grid keeps at least half of the full one (k = 256 would leave 32 workgroups to stream up to 128 MiB: slower
      // than the full grid + the device merge; measured at k <= 50, where 163+ of 204 workgroups stay)
      take = (nq == 1 && 2 * g.blocks >= full_blocks) || (nq > 1 && rounds <= 2 && (c->dtype == TAVB_F32 || nq <= 4));
    }
    if (take) {
      tavb::ScanParams p = scan_params(c, d_q, nullptr, c->rows, nq, k, 0u, ~0ull, nullptr, min_scores, TAVB_MAX_GROUPED_QUERIES);
      p.group = grouped ? plan.group : 0;
      return direct_one_launch(c, p, g, queries_host, grouped, c->ordinal_base, out_ordinals, out_scores, out_counts);
    }
  }
  // (a batch the host-synchronous cost model kept off the grouped form stays off it: the device-resident model below prices submissions that
  //  are not waited for one by one)
  struct NoGroup {
    tavb_ctx* c;
    explicit NoGroup(tavb_ctx* ctx) : c(ctx) { c->dispatch_no_group = true; }
    ~NoGroup() { c->dispatch_no_group = false; }
  } no_group(c);
  if (int rc = dispatch_staged(c, slot, d_q, nq, k, min_scores)) return rc;
  return sync_decode(c, nq, k, c->ordinal_base, out_ordinals, out_scores, out_counts);  // (no D2H copy: the merge kernel wrote the keys into pinned host memory)
}

int tavb_search_begin(tavb_ctx* c, const float* queries_host, int32_t nq, int32_t k, const float* min_scores, const tavb_key* cursor) {
  if (int rc = check_search_args(c, k)) return rc;
  if (nq < 1) return fail(TAVB_E_INVALID, "nq must be >= 1");
  if (!queries_host || !min_scores) return fail(TAVB_E_INVALID, "null argument");
  if (cursor && nq != 1) return fail(TAVB_E_INVALID, "a cursor goes with exactly one query");
  if (int rc = check_key_ordinals(c, /*device_resident=*/false)) return rc;
  DeviceGuard guard(c->device);
  const size_t obytes = (size_t)nq * k * sizeof(u64_t);
  if (int rc = c->h_out.reserve(obytes)) return rc;
  u64_t* const out = reinterpret_cast<u64_t*>(c->h_out.ptr);
  c->pending_nq = c->pending_k = 0;
  if (c->rows == 0) {
    memset(out, 0, obytes);
  } else {
    const float* d_q;
    if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
    const int rc = cursor ? search_device_impl(c, d_q, 1, k, min_scores, nullptr, c->rows, (uint32_t)c->ordinal_base, out, (u64_t)*cursor)
                          : tavb_search_device_dispatch(c, d_q, nq, k, min_scores, (uint32_t)c->ordinal_base, out);
    if (rc) return rc;
  }
  c->pending_nq = nq;
  c->pending_k = k;
  return TAVB_OK;
}

int tavb_search_end(tavb_ctx* c, int32_t nq, int32_t k, tavb_key* out_keys_host) {
  if (int rc = check_ctx(c)) return rc;
  if (!out_keys_host) return fail(TAVB_E_INVALID, "null argument");
  if (nq != c->pending_nq || k != c->pending_k || nq < 1) return fail(TAVB_E_INVALID, "tavb_search_end does not match the pending tavb_search_begin");
  DeviceGuard guard(c->device);
  TAVB_HIP(hipStreamSynchronize(c->stream));
  memcpy(out_keys_host, c->h_out.ptr, (size_t)nq * k * sizeof(u64_t));
  c->pending_nq = c->pending_k = 0;
  return TAVB_OK;
}

// lists [n_lists, nq, k] sorted best first -> out [nq, k], any k.  Every list's j-th key bounds j of its keys from below.  With
// j = ceil(k / n_lists) and t = the m-th largest of the lists' j-th keys, m = ceil(k / j), at least m * j >= k keys are >= t: the k best
// overall all are, and they sit in the prefixes (down to t) of the lists whose head is >= t.  One pass over n_lists keys, a selection among
// them, a sort of the keys that are left: 0.6 us for the 204 lists of a 10k-row lookup and 0.9 us for 40 lists of 50, where picking the
// maximum head k times took k * n_lists steps (3.1 us of a 30 us call; profiles/r04_latency_small.md).
static void merge_pruned(const tavb_key* lists, int n_lists, int nq, int k, tavb_key* out) {
  static thread_local std::vector<u64_t> pool;
  const int j = (k + n_lists - 1) / n_lists;
  const int m = (k + j - 1) / j;  // <= n_lists
  for (int q = 0; q < nq; ++q) {
    pool.resize((size_t)n_lists);
    for (int l = 0; l < n_lists; ++l) pool[l] = lists[((size_t)l * nq + q) * k + (j - 1)];
    std::nth_element(pool.begin(), pool.begin() + (m - 1), pool.end(), std::greater<u64_t>());
    const u64_t t = std::max<u64_t>(pool[m - 1], 1);  // (0 = an empty slot, never a result: fewer than k keys in all, take whatever there is)
    pool.clear();
    for (int l = 0; l < n_lists; ++l) {
      const tavb_key* list = lists + ((size_t)l * nq + q) * k;
      for (int i = 0; i < k && list[i] >= t; ++i) pool.push_back(list[i]);
    }
    const size_t take = std::min<size_t>((size_t)k, pool.size());
    std::partial_sort(pool.begin(), pool.begin() + take, pool.end(), std::greater<u64_t>());
    for (size_t i = 0; i < (size_t)k; ++i) out[(size_t)q * k + i] = i < take ? pool[i] : 0;  // 0 once every list is exhausted
  }
}

int tavb_merge_keys_host(const tavb_key* lists, int32_t n_lists, int32_t nq, int32_t k, tavb_key* out) {
  if (n_lists < 1 || nq < 0 || k < 1) return fail(TAVB_E_INVALID, "bad merge shape");
  if (nq == 0) return TAVB_OK;
  if (!lists || !out) return fail(TAVB_E_INVALID, "null argument");
  // A FEW lists (the grouped one-launch form leaves 8 .. 32 per query, and there are up to 64 queries to merge): a plain k-way merge, the
  // largest head k times -- with 8 lists of 50 the selection of merge_pruned keeps most of their 400 keys for the sort (~2 us per query, 64 us
  // for a 32-term batch of a 91 us call); k * n_lists steps are ~0.3 us.
  if (n_lists <= 16 && nq == 1) {
    const tavb_key* head[16];
    int left[16];
    for (int l = 0; l < n_lists; ++l) {
      head[l] = lists + (size_t)l * k;
      left[l] = k;
    }
    for (int i = 0; i < k; ++i) {
      int best = -1;
      u64_t best_key = 0;
      for (int l = 0; l < n_lists; ++l)
        if (left[l] > 0 && *head[l] > best_key) {
          best_key = *head[l];
          best = l;
        }
      out[i] = best_key;  // 0 once every list is exhausted (an empty slot of a list is 0 too, and the lists are sorted: nothing behind it)
      if (best >= 0) {
        ++head[best];
        --left[best];
      }
    }
    return TAVB_OK;
  }
  merge_pruned(lists, n_lists, nq, k, out);
  return TAVB_OK;
}

int tavb_merge_topk_host(const tavb_key* lists, int32_t n_lists, int32_t nq, int32_t k, tavb_key* out) {
  if (n_lists < 1 || n_lists > 64 || nq < 0 || k < 1 || k > TAVB_MAX_LARGE_K)
    return fail(TAVB_E_INVALID, "bad merge shape (1 .. 64 lists of 1 .. %d keys)", TAVB_MAX_LARGE_K);
  if (nq == 0) return TAVB_OK;
  if (!lists || !out) return fail(TAVB_E_INVALID, "null argument");
  merge_pruned(lists, n_lists, nq, k, out);
  // the rule of the device merge (launch_merge_topk): a query one of whose lists leads with the failure key is that key in every slot
  for (int q = 0; q < nq; ++q)
    for (int l = 0; l < n_lists; ++l)
      if (lists[((size_t)l * nq + q) * k] == TAVB_KEY_PEER_FAILED) {
        std::fill(out + (size_t)q * k, out + (size_t)(q + 1) * k, TAVB_KEY_PEER_FAILED);
        break;
      }
  return TAVB_OK;
}

// Lists whose keys carry MESSAGE ordinals: a message may stand in several lists, with several scores.  Per query: every real key, grouped by
// message (the low half) with the largest first, one key per message kept, the best k of those sorted descending.  The rule of the device
// merge (merge_top_messages_impl) for the failure key.
int tavb_merge_top_messages_host(const tavb_key* lists, int32_t n_lists, int32_t nq, int32_t k, tavb_key* out) {
  if (n_lists < 1 || n_lists > 64 || nq < 0 || k < 1 || k > TAVB_MAX_LARGE_K)
    return fail(TAVB_E_INVALID, "bad merge shape (1 .. 64 lists of 1 .. %d keys)", TAVB_MAX_LARGE_K);
  if (nq == 0) return TAVB_OK;
  if (!lists || !out) return fail(TAVB_E_INVALID, "null argument");
  std::vector<u64_t> pool;
  for (int q = 0; q < nq; ++q) {
    tavb_key* o = out + (size_t)q * k;
    bool failed = false;
    pool.clear();
    for (int l = 0; l < n_lists; ++l) {
      const tavb_key* list = lists + ((size_t)l * nq + q) * k;
      failed = failed || list[0] == TAVB_KEY_PEER_FAILED;
      for (int i = 0; i < k && list[i] != 0; ++i) pool.push_back(list[i]);  // (sorted, zero-padded: nothing behind the first zero)
    }
    if (failed) {
      std::fill(o, o + k, TAVB_KEY_PEER_FAILED);
      continue;
    }
    std::sort(pool.begin(), pool.end(), [](u64_t a, u64_t b) { return (uint32_t)a != (uint32_t)b ? (uint32_t)a < (uint32_t)b : a > b; });
    pool.erase(std::unique(pool.begin(), pool.end(), [](u64_t a, u64_t b) { return (uint32_t)a == (uint32_t)b; }), pool.end());
    const size_t n = std::min<size_t>((size_t)k, pool.size());
    std::partial_sort(pool.begin(), pool.begin() + n, pool.end(), std::greater<u64_t>());
    std::copy(pool.begin(), pool.begin() + n, o);
    std::fill(o + n, o + k, (tavb_key)0);
  }
  return TAVB_OK;
}

int tavb_search(tavb_ctx* c, const float* query_host, int32_t k, float min_score, int64_t* out_ordinals,
                float* out_scores, int32_t* out_count) {
  return tavb_search_batch(c, query_host, 1, k, &min_score, out_ordinals, out_scores, out_count);
}

static int search_subset_impl(tavb_ctx* c, const float* query_host, const int64_t* rows_host, int64_t n_subset, int32_t k,
                              float min_score, bool has_cursor, float after_score, int64_t after_position,
                              int64_t* out_positions, float* out_scores, int32_t* out_count) {
  if (int rc = check_search_args(c, k)) return rc;
  if (n_subset < 0) return fail(TAVB_E_INVALID, "n_subset must be >= 0");
  if (!query_host || !out_positions || !out_scores || !out_count) return fail(TAVB_E_INVALID, "null argument");
  if (n_subset == 0 || c->rows == 0) {
    *out_count = 0;
    return TAVB_OK;
  }
  if (!rows_host) return fail(TAVB_E_INVALID, "null rows_host");
  if (n_subset >= 0x7FFFFFFFll) return fail(TAVB_E_UNSUPPORTED, "subset too long");
  u64_t bound = ~0ull;
  if (has_cursor) {
    if (int rc = cursor_key(after_score, after_position, n_subset, &bound)) return rc;
  }
  DeviceGuard guard(c->device);
  const float* d_q;
  const int32_t* d_rows;
  if (int rc = c->h_out.reserve((size_t)k * sizeof(u64_t))) return rc;
  if (int rc = stage_subset(c, query_host, rows_host, n_subset, &d_q, &d_rows)) return rc;
  if (int rc = search_device_impl(c, d_q, 1, k, &min_score, d_rows, n_subset, 0u, reinterpret_cast<u64_t*>(c->h_out.ptr), bound)) return rc;
  return sync_decode(c, 1, k, 0, out_positions, out_scores, out_count);
}

// one pass, every survivor: keys on the device -> host, sorted best first, the first max_out decoded
static int search_all_impl(tavb_ctx* c, const float* query_host, const int64_t* rows_host, int64_t n_subset, bool subset, float min_score,
                           int64_t max_out, int64_t* out_items, float* out_scores, int64_t* out_count, int64_t* out_total) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = require_corpus(c)) return rc;
  if (!query_host || !out_count || !out_total || max_out < 0 || (max_out > 0 && (!out_items || !out_scores)))
    return fail(TAVB_E_INVALID, "bad argument");
  *out_count = 0;
  *out_total = 0;
  const int64_t n_pos = subset ? n_subset : c->rows;
  if (n_pos < 0 || n_pos >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "bad subset length");
  if (n_pos == 0 || c->rows == 0) return TAVB_OK;
  if (subset && !rows_host) return fail(TAVB_E_INVALID, "null rows_host");
  DeviceGuard guard(c->device);
  if (int rc = c->d_emit.reserve(256 + (size_t)n_pos * sizeof(u64_t))) return rc;
  const float* d_q;
  const int32_t* d_rows = nullptr;
  if (int rc = subset ? stage_subset(c, query_host, rows_host, n_subset, &d_q, &d_rows) : stage_queries(c, query_host, 1, &d_q)) return rc;
  unsigned long long* d_counter = reinterpret_cast<unsigned long long*>(c->d_emit.ptr);
  u64_t* d_keys = reinterpret_cast<u64_t*>(reinterpret_cast<char*>(c->d_emit.ptr) + 256);
  TAVB_HIP(hipMemsetAsync(d_counter, 0, sizeof(unsigned long long), c->stream));
  const tavb::ScanParams p = scan_params(c, d_q, d_rows, n_pos, 1, 1, 0u, ~0ull, nullptr, &min_score, 1);
  {
    Timed t(c, TAVB_KERNEL_SCAN);
    const int blocks = (int)std::min<int64_t>(c->n_cu, (n_pos + 15) / 16);
    hipError_t e = tavb::launch_scan_emit(p, std::max(blocks, 1), d_keys, (unsigned long long)n_pos, d_counter, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "emit scan launch failed: %s", hipGetErrorString(e));
  }
  unsigned long long total = 0;
  TAVB_HIP(hipMemcpyAsync(&total, d_counter, sizeof total, hipMemcpyDeviceToHost, c->stream));
  TAVB_HIP(hipStreamSynchronize(c->stream));
  *out_total = (int64_t)total;
  if (total == 0 || max_out == 0) return TAVB_OK;
  std::vector<u64_t> keys((size_t)total);
  TAVB_HIP(hipMemcpy(keys.data(), d_keys, (size_t)total * sizeof(u64_t), hipMemcpyDeviceToHost));
  const size_t want = (size_t)std::min<int64_t>((int64_t)total, max_out);
  if (want < keys.size())
    std::partial_sort(keys.begin(), keys.begin() + want, keys.end(), std::greater<u64_t>());
  else
    std::sort(keys.begin(), keys.end(), std::greater<u64_t>());
  const int64_t base = subset ? 0 : c->ordinal_base;
  for (size_t i = 0; i < want; ++i) decode_key(keys[i], base, &out_items[i], &out_scores[i]);
  *out_count = (int64_t)want;
  return TAVB_OK;
}

int tavb_search_all(tavb_ctx* c, const float* query_host, float min_score, int64_t max_out, int64_t* out_ordinals, float* out_scores,
                    int64_t* out_count, int64_t* out_total) {
  return search_all_impl(c, query_host, nullptr, 0, false, min_score, max_out, out_ordinals, out_scores, out_count, out_total);
}

int tavb_search_subset_all(tavb_ctx* c, const float* query_host, const int64_t* rows_host, int64_t n_subset, float min_score, int64_t max_out,
                           int64_t* out_positions, float* out_scores, int64_t* out_count, int64_t* out_total) {
  return search_all_impl(c, query_host, rows_host, n_subset, true, min_score, max_out, out_positions, out_scores, out_count, out_total);
}


int tavb_set_row_messages(tavb_ctx* c, const int32_t* dev_row_to_msg, int64_t rows, int64_t n_messages) {
  if (int rc = check_ctx(c)) return rc;
  if (rows < 0 || n_messages < 0) return fail(TAVB_E_INVALID, "bad shape");
  if (rows > 0 && !dev_row_to_msg) return fail(TAVB_E_INVALID, "null map with rows > 0");
  if (n_messages >= 0xFFFFFFFFll) return fail(TAVB_E_UNSUPPORTED, "message ordinals must stay below 2^32 - 1");
  c->row_to_msg = dev_row_to_msg;
  c->row_to_msg_rows = rows;
  c->n_messages = n_messages;
  return TAVB_OK;
}

// hits (device keys [k]) -> message keys in pinned host memory -> caller's arrays
static int rerank_and_return(tavb_ctx* c, const u64_t* d_hits, int k, const int32_t* d_pos_to_row, const int32_t* accept_msgs_host, int64_t n_accept,
                             bool filtered, int32_t max_messages, int64_t* out_messages, float* out_scores, int32_t* out_count) {
  const uint32_t* d_bits = nullptr;
  if (filtered)
    if (int rc = stage_accept_bitmap(c, accept_msgs_host, n_accept, &d_bits)) return rc;
  hipError_t e = tavb::launch_message_rerank(d_hits, 1, k, 0u, d_pos_to_row, c->row_to_msg, c->row_to_msg_rows, d_bits, c->n_messages, max_messages,
                                             reinterpret_cast<u64_t*>(c->h_out.ptr), c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "re-rank launch failed: %s", hipGetErrorString(e));
  return sync_decode(c, 1, k, 0, out_messages, out_scores, out_count);
}

int tavb_search_messages(tavb_ctx* c, const float* query_host, int32_t k, float min_score, const int32_t* accept_msgs_host, int64_t n_accept,
                         int32_t max_messages, int64_t* out_messages, float* out_scores, int32_t* out_count) {
  if (int rc = check_message_args(c, k, max_messages)) return rc;
  if (!query_host || !out_messages || !out_scores || !out_count) return fail(TAVB_E_INVALID, "null argument");
  if (n_accept < -1 || (n_accept > 0 && !accept_msgs_host)) return fail(TAVB_E_INVALID, "bad accept list");
  *out_count = 0;
  if (c->rows == 0) return TAVB_OK;
  DeviceGuard guard(c->device);
  const size_t obytes = (size_t)k * sizeof(u64_t);
  if (int rc = c->h_out.reserve(obytes)) return rc;
  if (int rc = c->d_out.reserve(obytes)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, query_host, 1, &d_q)) return rc;
  u64_t* const d_hits = reinterpret_cast<u64_t*>(c->d_out.ptr);
  // keys carry LOCAL rows here (index_base 0): they only index the map
  if (int rc = search_device_impl(c, d_q, 1, k, &min_score, nullptr, c->rows, 0u, d_hits)) return rc;
  return rerank_and_return(c, d_hits, k, nullptr, accept_msgs_host, n_accept, n_accept >= 0, max_messages, out_messages, out_scores, out_count);
}

int tavb_search_messages_subset(tavb_ctx* c, const float* query_host, const int64_t* rows_host, int64_t n_subset, int32_t k, float min_score,
                                int32_t max_messages, int64_t* out_messages, float* out_scores, int32_t* out_count) {
  if (int rc = check_message_args(c, k, max_messages)) return rc;
  if (!query_host || !out_messages || !out_scores || !out_count) return fail(TAVB_E_INVALID, "null argument");
  if (n_subset < 0 || n_subset >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "bad subset length");
  *out_count = 0;
  if (n_subset == 0 || c->rows == 0) return TAVB_OK;
  if (!rows_host) return fail(TAVB_E_INVALID, "null rows_host");
  DeviceGuard guard(c->device);
  const size_t obytes = (size_t)k * sizeof(u64_t);
  if (int rc = c->h_out.reserve(obytes)) return rc;
  if (int rc = c->d_out.reserve(obytes)) return rc;
  const float* d_q;
  const int32_t* d_rows;
  if (int rc = stage_subset(c, query_host, rows_host, n_subset, &d_q, &d_rows)) return rc;
  u64_t* const d_hits = reinterpret_cast<u64_t*>(c->d_out.ptr);
  if (int rc = search_device_impl(c, d_q, 1, k, &min_score, d_rows, n_subset, 0u, d_hits)) return rc;
  return rerank_and_return(c, d_hits, k, d_rows, nullptr, 0, false, max_messages, out_messages, out_scores, out_count);
}

int tavb_search_subset(tavb_ctx* c, const float* query_host, const int64_t* rows_host, int64_t n_subset, int32_t k,
                       float min_score, int64_t* out_positions, float* out_scores, int32_t* out_count) {
  return search_subset_impl(c, query_host, rows_host, n_subset, k, min_score, false, 0.f, 0, out_positions, out_scores,
                            out_count);
}

int tavb_search_subset_after(tavb_ctx* c, const float* query_host, const int64_t* rows_host, int64_t n_subset,
                             int32_t k, float min_score, float after_score, int64_t after_position,
                             int64_t* out_positions, float* out_scores, int32_t* out_count) {
  return search_subset_impl(c, query_host, rows_host, n_subset, k, min_score, true, after_score, after_position,
                            out_positions, out_scores, out_count);
}

int tavb_search_device(tavb_ctx* c, const float* dev_queries, int32_t nq, int32_t k, float min_score,
                       tavb_key* dev_out_keys) {
  if (int rc = check_search_args(c, k)) return rc;
  if (nq < 1) return fail(TAVB_E_INVALID, "nq must be >= 1");
  if (!dev_queries || !dev_out_keys) return fail(TAVB_E_INVALID, "null argument");
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  std::vector<float> ms((size_t)nq, min_score);
  return tavb_search_device_dispatch(c, dev_queries, nq, k, ms.data(), (uint32_t)c->ordinal_base,
                                     reinterpret_cast<u64_t*>(dev_out_keys));
}

int tavb_search_subset_device(tavb_ctx* c, const float* dev_query, const int32_t* dev_rows, int64_t n_subset, int32_t k,
                              float min_score, tavb_key* dev_out_keys) {
  if (int rc = check_search_args(c, k)) return rc;
  if (!dev_query || !dev_out_keys) return fail(TAVB_E_INVALID, "null argument");
  if (n_subset < 0 || n_subset >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "bad subset length");
  if (n_subset > 0 && !dev_rows) return fail(TAVB_E_INVALID, "null dev_rows");
  DeviceGuard guard(c->device);
  return search_device_impl(c, dev_query, 1, k, &min_score, dev_rows, c->rows == 0 ? 0 : n_subset, 0u,
                            reinterpret_cast<u64_t*>(dev_out_keys));
}

int tavb_search_subset_resident(tavb_ctx* c, const float* query_host, const int32_t* dev_rows, int64_t n_subset, int32_t k, float min_score,
                                int64_t* out_positions, float* out_scores, int32_t* out_count) {
  if (int rc = check_search_args(c, k)) return rc;
  if (n_subset < 0 || n_subset >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "bad subset length");
  if (!query_host || !out_positions || !out_scores || !out_count) return fail(TAVB_E_INVALID, "null argument");
  if (n_subset == 0 || c->rows == 0) {
    *out_count = 0;
    return TAVB_OK;
  }
  if (!dev_rows) return fail(TAVB_E_INVALID, "null dev_rows");
  DeviceGuard guard(c->device);
  const float* d_q;
  if (int rc = stage_queries_host(c, query_host, 1, &d_q)) return rc;
  if (int rc = c->h_out.reserve((size_t)k * sizeof(u64_t))) return rc;
  c->last_direct = 0;
  // a small subset (the reference script's 1000 of 10k; the memory provider's scope lists): ONE launch, as tavb_search does it for small corpora --
  // the scan's per-workgroup lists land in pinned host memory and are merged here; a 1536-wide query rides in the kernel arguments
  const int64_t subset_bytes = n_subset * c->dim * (c->dtype == TAVB_F16 ? 2 : 4);
  if (c->small_direct_bytes > 0 && subset_bytes <= c->small_direct_bytes) {
    tavb::ScanGeometry g = clamped_geometry(c);
    const int full_blocks = scan_blocks_for(c, n_subset, g.waves, g.unroll);
    g.blocks = std::min(full_blocks, (int)std::max<int64_t>(8, c->small_direct_keys / (int64_t)k));
    if (2 * g.blocks >= full_blocks) {
      tavb::ScanParams p = scan_params(c, d_q, dev_rows, n_subset, 1, k, 0u, ~0ull, nullptr, &min_score, TAVB_MAX_STREAM_QUERIES);
      return direct_one_launch(c, p, g, query_host, /*grouped=*/false, 0, out_positions, out_scores, out_count);
    }
  }
  TAVB_HIP(submit_queries(c, 1));
  if (int rc = search_device_impl(c, d_q, 1, k, &min_score, dev_rows, n_subset, 0u, reinterpret_cast<u64_t*>(c->h_out.ptr))) return rc;
  return sync_decode(c, 1, k, 0, out_positions, out_scores, out_count);
}


int tavb_search_after(tavb_ctx* c, const float* query_host, int32_t k, float min_score, float after_score,
                      int64_t after_ordinal, int64_t* out_ordinals, float* out_scores, int32_t* out_count) {
  if (int rc = check_search_args(c, k)) return rc;
  if (!query_host || !out_ordinals || !out_scores || !out_count) return fail(TAVB_E_INVALID, "null argument");
  if (c->rows == 0) {
    *out_count = 0;
    return TAVB_OK;
  }
  u64_t bound;
  if (int rc = cursor_key(after_score, after_ordinal - c->ordinal_base, c->rows, &bound)) return rc;
  DeviceGuard guard(c->device);
  if (int rc = c->h_out.reserve((size_t)k * sizeof(u64_t))) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, query_host, 1, &d_q)) return rc;
  if (int rc = search_device_impl(c, d_q, 1, k, &min_score, nullptr, c->rows, 0u, reinterpret_cast<u64_t*>(c->h_out.ptr), bound)) return rc;
  return sync_decode(c, 1, k, c->ordinal_base, out_ordinals, out_scores, out_count);
}

}  // extern "C"
