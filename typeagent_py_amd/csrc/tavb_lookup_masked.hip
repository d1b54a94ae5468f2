// The batched and masked lookups of the C ABI (include/tavb.h): the batched resident subset (the gather route of a masked batch), masked
// batches on the 32/64-query tile and on the 128/256-query filter tile, scoped batches (one mask per query) on the row-list route and on
// both tiles -- each in its host, device and messages form -- and tavb_search_messages_batch.  Host code only: the routes are
// tavb_route.hip's, the large-k passes tavb_lookup_topk.hip's, the staging and the key targets tavb_lookup.hip's; the row masks themselves
// are made in tavb_mask_entry.hip.

#include "tavb_ctx.h"

using namespace tavb::host;

namespace {

// ---- what the entry points check
// what every masked entry point checks first
int check_masked_head(tavb_ctx* c, int32_t nq, int64_t rows, int32_t k) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = require_corpus(c)) return rc;
  if (k < 1) return fail(TAVB_E_INVALID, "k must be >= 1 (got %d)", k);
  if (nq < 0) return fail(TAVB_E_INVALID, "nq must be >= 0");
  if (rows != c->rows) return fail(TAVB_E_INVALID, "the mask covers %lld rows, the corpus has %lld", (long long)rows, (long long)c->rows);
  return TAVB_OK;
}

// the last check of a tile route: the shapes it serves.  who: "masked" / "scoped"; instead: where the text sends the caller
int check_route_shape(const tavb_ctx* c, bool wide, const char* who, const char* instead, int32_t k) {
  if (wide) {
    if (!masked_wide_supported(c, k))
      return fail(TAVB_E_UNSUPPORTED, "the %s wide route serves fp16 corpora of up to 16384 halves per row and 1 <= k <= %d (k = %d): use %s", who, TAVB_MAX_FUSED_K, k,
                  instead);
  } else if (!tavb::skinny_supported(c->dim, k, c->dtype != TAVB_F16)) {
    return fail(TAVB_E_UNSUPPORTED, "the %s tile serves 1 <= k <= 64 and rows of a multiple of 64 bytes (k = %d, %d bytes): use %s", who, k,
                c->dim * (c->dtype == TAVB_F16 ? 2 : 4), instead);
  }
  return TAVB_OK;
}

// A masked batch on the 32/64-query tile, or (wide) on the 128/256-query filter tile, which also takes the mask's row list.
// *empty: nothing to scan (an empty corpus, no query, an empty span, an empty row list).
int check_masked_args(tavb_ctx* c, bool wide, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row, int64_t last_row, const int32_t* dev_rows,
                      int64_t n_allowed, int32_t k, bool* empty) {
  if (int rc = check_masked_head(c, nq, rows, k)) return rc;
  if (wide && (n_allowed < 0 || n_allowed > rows)) return fail(TAVB_E_INVALID, "bad row list length");
  *empty = rows == 0 || nq == 0 || first_row > last_row || (wide && n_allowed == 0);
  if (int rc = check_masked_span(*empty, rows, first_row, last_row)) return rc;
  if (!*empty && (!dev_bits || (wide && !dev_rows))) return fail(TAVB_E_INVALID, wide ? "null dev_bits / dev_rows" : "null dev_bits");
  if (wide && (reinterpret_cast<uintptr_t>(dev_bits) & 3) != 0) return fail(TAVB_E_INVALID, "dev_bits must be 4-byte aligned");
  return check_route_shape(c, wide, "masked", wide ? "another masked route" : "the gather route", k);
}

int check_query_masks(const uint32_t* const* dev_masks, int32_t nq) {
  if (!dev_masks) return fail(TAVB_E_INVALID, "null dev_masks");
  return check_mask_list(dev_masks, nq, "the mask of query");
}

// the same with one mask per query; *empty: nothing to scan (an empty corpus, no query, an empty span)
int check_scoped_span_args(tavb_ctx* c, bool wide, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row, int64_t last_row, int32_t k,
                           bool* empty) {
  if (int rc = check_masked_head(c, nq, rows, k)) return rc;
  if (rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "rows must be 0 .. 2^31 - 2");
  *empty = rows == 0 || nq == 0 || first_row > last_row;
  if (int rc = check_masked_span(*empty, rows, first_row, last_row)) return rc;
  if (!*empty)
    if (int rc = check_query_masks(dev_masks, nq)) return rc;
  return check_route_shape(c, wide, "scoped", "the row-list route", k);
}

int check_host_io(const void* queries, const void* min_scores, const void* out, const void* out_scores, const void* out_counts) {
  if (!queries || !min_scores || !out || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  return TAVB_OK;
}

int check_device_io(const void* dev_queries, const void* min_scores, const void* out_keys) {
  if (!dev_queries || !min_scores || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  return TAVB_OK;
}

// ---- batched message lookups: nq key lists [nq, k] on the device (keys carrying index_base + row) -> ONE message_rerank_kernel launch of nq
// workgroups -> ONE device-to-host copy -> the callers' arrays.  d_out holds both: the hits in its first nq * k keys, the message keys behind.
int rerank_batch_and_return(tavb_ctx* c, const u64_t* d_hits, int nq, int k, uint32_t index_base, const uint32_t* d_accept_bits, int32_t max_messages,
                            int64_t* out_messages, float* out_scores, int32_t* out_counts) {
  const size_t n_keys = (size_t)nq * k;
  u64_t* const d_msgs = reinterpret_cast<u64_t*>(c->d_out.ptr) + n_keys;
  {
    Timed t(c, TAVB_KERNEL_MERGE);
    hipError_t e = tavb::launch_message_rerank(d_hits, nq, k, index_base, nullptr, c->row_to_msg, c->row_to_msg_rows, d_accept_bits, c->n_messages,
                                               max_messages, d_msgs, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "re-rank launch failed: %s", hipGetErrorString(e));
  }
  TAVB_HIP(hipMemcpyAsync(c->h_out.ptr, d_msgs, n_keys * sizeof(u64_t), hipMemcpyDeviceToHost, c->stream));
  return sync_decode(c, nq, k, 0, out_messages, out_scores, out_counts);
}

// the buffers of such a lookup: pinned room for the message keys, device room for the hits and the message keys; *d_hits = the hits
int reserve_message_batch(tavb_ctx* c, int nq, int k, u64_t** d_hits) {
  const size_t n_keys = (size_t)nq * k;
  if (int rc = c->h_out.reserve(n_keys * sizeof(u64_t))) return rc;
  if (int rc = c->d_out.reserve(2 * n_keys * sizeof(u64_t))) return rc;
  *d_hits = reinterpret_cast<u64_t*>(c->d_out.ptr);
  return TAVB_OK;
}

// The tail of the messages form of a masked or scoped batch that has something to scan: the buffers, the queries, then
// search(d_q, index_base, d_hits) -- the route's own search, keys carrying ordinal_base + row -- and the re-rank.
template <class Search>
int search_messages_and_return(tavb_ctx* c, const float* queries_host, int nq, int k, int32_t max_messages, int64_t* out_messages, float* out_scores,
                               int32_t* out_counts, Search&& search) {
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  u64_t* d_hits;
  if (int rc = reserve_message_batch(c, nq, k, &d_hits)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  c->last_graph = 0;
  const uint32_t base = (uint32_t)c->ordinal_base;
  if (int rc = search(d_q, base, d_hits)) return rc;
  return rerank_batch_and_return(c, d_hits, nq, k, base, nullptr, max_messages, out_messages, out_scores, out_counts);
}

}  // namespace

namespace tavb {
namespace host __attribute__((visibility("hidden"))) {

int check_masked_span(bool empty, int64_t rows, int64_t first_row, int64_t last_row) {
  if (!empty && (first_row < 0 || last_row >= rows)) return fail(TAVB_E_INVALID, "mask span [%lld, %lld] outside the corpus", (long long)first_row, (long long)last_row);
  return TAVB_OK;
}

// (shared with the scoped large-k, sorted and top-messages entry points of tavb_lookup_topk.hip, whose k_max is TAVB_MAX_LARGE_K)
int check_scoped_args(tavb_ctx* c, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k, int32_t k_max, bool* empty) {
  if (int rc = check_masked_head(c, nq, rows, k)) return rc;
  if (k > k_max) return fail(TAVB_E_INVALID, "a scoped batch serves 1 <= k <= %d (got %d)", k_max, k);
  if (rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "rows must be 0 .. 2^31 - 2");
  *empty = rows == 0 || nq == 0;
  return *empty ? TAVB_OK : check_query_masks(dev_masks, nq);
}

}  // namespace host
}  // namespace tavb

extern "C" {

// ---- the batched resident subset
// nq queries over one resident row list: the passes of search_device_impl (k <= TAVB_MAX_FUSED_K: a scan + a merge per group of queries) or of
// search_topk_impl (beyond), both of which take a row list with any number of queries; the remap runs on the keys wherever they landed.
int tavb_search_subset_batch_resident(tavb_ctx* c, const float* queries_host, int32_t nq, const int32_t* dev_rows, int64_t n_subset, int32_t k,
                                      const float* min_scores, int32_t remap, int64_t* out, float* out_scores, int32_t* out_counts) {
  if (int rc = check_topk_args(c, k)) return rc;
  if (nq < 0) return fail(TAVB_E_INVALID, "nq must be >= 0");
  if (n_subset < 0 || n_subset >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "bad subset length");
  if (remap != 0 && remap != 1) return fail(TAVB_E_INVALID, "remap must be 0 (positions) or 1 (corpus ordinals)");
  if (nq == 0) return TAVB_OK;
  if (int rc = check_host_io(queries_host, min_scores, out, out_scores, out_counts)) return rc;
  note_route(c, 1, /*clear_graph=*/false);  // the gather route of a masked batch
  if (n_subset == 0 || c->rows == 0) return empty_counts(out_counts, nq);
  if (!dev_rows) return fail(TAVB_E_INVALID, "null dev_rows");
  DeviceGuard guard(c->device);
  u64_t* target;
  int32_t* rounds;
  if (int rc = reserve_key_target(c, nq, k, &target, &rounds)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  if (k <= TAVB_MAX_FUSED_K) {
    if (int rc = search_device_impl(c, d_q, nq, k, min_scores, dev_rows, n_subset, 0u, target)) return rc;
  } else {
    if (int rc = search_topk_impl(c, d_q, nq, k, min_scores, dev_rows, n_subset, 0u, target, rounds)) return rc;
  }
  if (remap)
    if (int rc = remap_key_rows(c, target, target, (int64_t)nq * k, dev_rows, n_subset, 0u)) return rc;
  return collect_keys(c, target, nq, k, remap ? c->ordinal_base : 0, out, out_scores, out_counts, k > TAVB_MAX_FUSED_K ? rounds : nullptr);
}

// The no-wait twin of the call above: queries already on the device, keys to device (or device-writable pinned) memory.  remap = 1: the passes
// write their positions into d_out and the remap kernel turns them into ordinal_base + dev_rows[position] on the way to out_keys -- one
// launch either way, and a pinned out_keys is written once and never read over PCIe.
int tavb_search_subset_batch_device(tavb_ctx* c, const float* dev_queries, int32_t nq, const int32_t* dev_rows, int64_t n_subset, int32_t k,
                                    const float* min_scores, int32_t remap, tavb_key* out_keys) {
  if (int rc = check_topk_args(c, k)) return rc;
  if (nq < 1) return fail(TAVB_E_INVALID, "nq must be >= 1");
  if (n_subset < 0 || n_subset >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "bad subset length");
  if (remap != 0 && remap != 1) return fail(TAVB_E_INVALID, "remap must be 0 (positions) or 1 (global ordinals)");
  if (int rc = check_device_io(dev_queries, min_scores, out_keys)) return rc;
  if (remap)
    if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  note_route(c, 1, /*clear_graph=*/false);  // the gather route of a masked batch
  DeviceGuard guard(c->device);
  u64_t* const out = reinterpret_cast<u64_t*>(out_keys);
  const size_t n_keys = (size_t)nq * k;
  if (n_subset == 0 || c->rows == 0) return fill_empty_keys(c, out, (int64_t)n_keys);  // nothing to scan (dev_rows may be null)
  if (!dev_rows) return fail(TAVB_E_INVALID, "null dev_rows");
  u64_t* target = out;
  if (remap) {
    if (int rc = c->d_out.reserve(n_keys * sizeof(u64_t))) return rc;
    target = reinterpret_cast<u64_t*>(c->d_out.ptr);
  }
  if (k <= TAVB_MAX_FUSED_K) {
    if (int rc = search_device_impl(c, dev_queries, nq, k, min_scores, dev_rows, n_subset, 0u, target)) return rc;
  } else {
    if (int rc = search_topk_async(c, dev_queries, nq, k, min_scores, dev_rows, n_subset, 0u, target)) return rc;
  }
  return remap ? remap_key_rows(c, target, out, (int64_t)n_keys, dev_rows, n_subset, (uint32_t)c->ordinal_base) : TAVB_OK;
}

// ---- masked batches on the 32/64-query tile (tavb_route.hip::search_masked_tile)
int tavb_search_masked_batch(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row, int64_t last_row,
                             int32_t k, const float* min_scores, int64_t* out_ordinals, float* out_scores, int32_t* out_counts) {
  bool empty = false;
  if (int rc = check_masked_args(c, /*wide=*/false, nq, dev_bits, rows, first_row, last_row, nullptr, 0, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (int rc = check_host_io(queries_host, min_scores, out_ordinals, out_scores, out_counts)) return rc;
  if (empty) return empty_counts(out_counts, nq);
  DeviceGuard guard(c->device);
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  if (int rc = c->h_out.reserve((size_t)nq * k * sizeof(u64_t))) return rc;
  c->last_graph = 0;
  if (int rc = search_masked_tile(c, d_q, nq, k, min_scores, dev_bits, first_row, last_row, 0u, reinterpret_cast<u64_t*>(c->h_out.ptr))) return rc;
  return sync_decode(c, nq, k, c->ordinal_base, out_ordinals, out_scores, out_counts);  // (no D2H copy: the merge kernel wrote the keys into pinned host memory)
}

int tavb_search_masked_device(tavb_ctx* c, const float* dev_queries, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row, int64_t last_row,
                              int32_t k, const float* min_scores, tavb_key* out_keys) {
  bool empty = false;
  if (int rc = check_masked_args(c, /*wide=*/false, nq, dev_bits, rows, first_row, last_row, nullptr, 0, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (int rc = check_device_io(dev_queries, min_scores, out_keys)) return rc;
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  if (empty) return fill_empty_keys(c, reinterpret_cast<u64_t*>(out_keys), (int64_t)nq * k);  // no tile launch
  return search_masked_tile(c, dev_queries, nq, k, min_scores, dev_bits, first_row, last_row, (uint32_t)c->ordinal_base, reinterpret_cast<u64_t*>(out_keys));
}

// ---- masked batches on the 128/256-query filter tile + rescoring (tavb_route.hip::search_masked_wide)
int tavb_search_masked_wide(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row, int64_t last_row,
                            const int32_t* dev_rows, int64_t n_allowed, int32_t k, const float* min_scores, int64_t* out_ordinals, float* out_scores,
                            int32_t* out_counts) {
  bool empty = false;
  if (int rc = check_masked_args(c, /*wide=*/true, nq, dev_bits, rows, first_row, last_row, dev_rows, n_allowed, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (int rc = check_host_io(queries_host, min_scores, out_ordinals, out_scores, out_counts)) return rc;
  if (empty) return empty_counts(out_counts, nq);
  DeviceGuard guard(c->device);
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  u64_t* target;
  if (int rc = reserve_key_target(c, nq, k, &target)) return rc;
  c->last_graph = 0;
  if (int rc = search_masked_wide(c, d_q, nq, k, min_scores, dev_bits, first_row, last_row, dev_rows, n_allowed, 0u, target)) return rc;
  return collect_keys(c, target, nq, k, c->ordinal_base, out_ordinals, out_scores, out_counts);
}

int tavb_search_masked_wide_device(tavb_ctx* c, const float* dev_queries, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row, int64_t last_row,
                                   const int32_t* dev_rows, int64_t n_allowed, int32_t k, const float* min_scores, tavb_key* out_keys) {
  bool empty = false;
  if (int rc = check_masked_args(c, /*wide=*/true, nq, dev_bits, rows, first_row, last_row, dev_rows, n_allowed, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (int rc = check_device_io(dev_queries, min_scores, out_keys)) return rc;
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  if (empty) return fill_empty_keys(c, reinterpret_cast<u64_t*>(out_keys), (int64_t)nq * k);  // no tile launch
  return search_masked_wide(c, dev_queries, nq, k, min_scores, dev_bits, first_row, last_row, dev_rows, n_allowed, (uint32_t)c->ordinal_base,
                            reinterpret_cast<u64_t*>(out_keys));
}

// ---- the messages form of a one-mask batch, on the route the caller names
int tavb_search_messages_masked(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row, int64_t last_row,
                                const int32_t* dev_rows, int64_t n_allowed, int32_t k, const float* min_scores, int32_t max_messages, int32_t route,
                                int64_t* out_messages, float* out_scores, int32_t* out_counts) {
  if (int rc = check_message_args(c, k, max_messages)) return rc;
  if (route < 1 || route > 3) return fail(TAVB_E_INVALID, "route must be 1 (row list), 2 (32/64-query tile) or 3 (wide filter tile), got %d", route);
  bool empty = false;
  if (route == 1) {
    if (int rc = check_masked_head(c, nq, rows, k)) return rc;
    if (n_allowed < 0 || n_allowed >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "bad row list length");
    empty = rows == 0 || nq == 0 || n_allowed == 0;
    if (!empty && !dev_rows) return fail(TAVB_E_INVALID, "null dev_rows");
  } else {
    if (int rc = check_masked_args(c, /*wide=*/route == 3, nq, dev_bits, rows, first_row, last_row, dev_rows, n_allowed, k, &empty)) return rc;
  }
  if (nq == 0) return TAVB_OK;
  if (int rc = check_host_io(queries_host, min_scores, out_messages, out_scores, out_counts)) return rc;
  if (empty) return empty_counts(out_counts, nq);
  return search_messages_and_return(c, queries_host, nq, k, max_messages, out_messages, out_scores, out_counts, [&](const float* d_q, uint32_t base, u64_t* d_hits) {
    if (route == 2) return search_masked_tile(c, d_q, nq, k, min_scores, dev_bits, first_row, last_row, base, d_hits);
    if (route == 3) return search_masked_wide(c, d_q, nq, k, min_scores, dev_bits, first_row, last_row, dev_rows, n_allowed, base, d_hits);
    note_route(c, 1, /*clear_graph=*/false);  // the gather route of a masked batch
    if (int rc = search_device_impl(c, d_q, nq, k, min_scores, dev_rows, n_allowed, 0u, d_hits)) return rc;
    return remap_key_rows(c, d_hits, d_hits, (int64_t)nq * k, dev_rows, n_allowed, base);
  });
}

// ---- scoped batches: one mask per query (tavb_route.hip::search_scoped_impl); "masked_route" = 4
int tavb_search_scoped_batch(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                             const float* min_scores, int64_t* out_ordinals, float* out_scores, int32_t* out_counts) {
  bool empty = false;
  if (int rc = check_scoped_args(c, nq, dev_masks, rows, k, TAVB_MAX_FUSED_K, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (int rc = check_host_io(queries_host, min_scores, out_ordinals, out_scores, out_counts)) return rc;
  note_route(c, 4);
  if (empty) return empty_counts(out_counts, nq);
  DeviceGuard guard(c->device);
  u64_t* target;
  if (int rc = reserve_key_target(c, nq, k, &target)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  if (int rc = search_scoped_impl(c, d_q, nq, k, min_scores, dev_masks, 0u, target, target)) return rc;
  return collect_keys(c, target, nq, k, c->ordinal_base, out_ordinals, out_scores, out_counts);
}

int tavb_search_scoped_device(tavb_ctx* c, const float* dev_queries, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                              const float* min_scores, tavb_key* out_keys) {
  bool empty = false;
  if (int rc = check_scoped_args(c, nq, dev_masks, rows, k, TAVB_MAX_FUSED_K, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (int rc = check_device_io(dev_queries, min_scores, out_keys)) return rc;
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  note_route(c, 4);
  DeviceGuard guard(c->device);
  u64_t* const out = reinterpret_cast<u64_t*>(out_keys);
  if (empty) return fill_empty_keys(c, out, (int64_t)nq * k);
  // (the merges write positions into d_out and the remaps turn them into ordinal_base + row on the way to out_keys: a pinned out_keys is
  //  written once and never read over PCIe)
  if (int rc = c->d_out.reserve((size_t)nq * k * sizeof(u64_t))) return rc;
  return search_scoped_impl(c, dev_queries, nq, k, min_scores, dev_masks, (uint32_t)c->ordinal_base, reinterpret_cast<u64_t*>(c->d_out.ptr), out);
}

int tavb_search_messages_scoped(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                                const float* min_scores, int32_t max_messages, int64_t* out_messages, float* out_scores, int32_t* out_counts) {
  if (int rc = check_message_args(c, k, max_messages)) return rc;
  bool empty = false;
  if (int rc = check_scoped_args(c, nq, dev_masks, rows, k, TAVB_MAX_FUSED_K, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (int rc = check_host_io(queries_host, min_scores, out_messages, out_scores, out_counts)) return rc;
  note_route(c, 4);
  if (empty) return empty_counts(out_counts, nq);
  return search_messages_and_return(c, queries_host, nq, k, max_messages, out_messages, out_scores, out_counts, [&](const float* d_q, uint32_t base, u64_t* d_hits) {
    return search_scoped_impl(c, d_q, nq, k, min_scores, dev_masks, base, d_hits, d_hits);
  });
}

// ---- scoped batches on the 32/64-query tile (tavb_route.hip::search_scoped_tile)
int tavb_search_scoped_tile(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row, int64_t last_row,
                            int32_t k, const float* min_scores, int64_t* out_ordinals, float* out_scores, int32_t* out_counts) {
  bool empty = false;
  if (int rc = check_scoped_span_args(c, /*wide=*/false, nq, dev_masks, rows, first_row, last_row, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (int rc = check_host_io(queries_host, min_scores, out_ordinals, out_scores, out_counts)) return rc;
  if (empty) return empty_counts(out_counts, nq);
  DeviceGuard guard(c->device);
  u64_t* target;
  if (int rc = reserve_key_target(c, nq, k, &target)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  c->last_graph = 0;
  if (int rc = search_scoped_tile(c, d_q, nq, k, min_scores, dev_masks, first_row, last_row, 0u, target)) return rc;
  return collect_keys(c, target, nq, k, c->ordinal_base, out_ordinals, out_scores, out_counts);
}

int tavb_search_scoped_tile_device(tavb_ctx* c, const float* dev_queries, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row,
                                   int64_t last_row, int32_t k, const float* min_scores, tavb_key* out_keys) {
  bool empty = false;
  if (int rc = check_scoped_span_args(c, /*wide=*/false, nq, dev_masks, rows, first_row, last_row, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (int rc = check_device_io(dev_queries, min_scores, out_keys)) return rc;
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  if (empty) return fill_empty_keys(c, reinterpret_cast<u64_t*>(out_keys), (int64_t)nq * k);  // no tile launch
  return search_scoped_tile(c, dev_queries, nq, k, min_scores, dev_masks, first_row, last_row, (uint32_t)c->ordinal_base, reinterpret_cast<u64_t*>(out_keys));
}

int tavb_search_messages_scoped_tile(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row,
                                     int64_t last_row, int32_t k, const float* min_scores, int32_t max_messages, int64_t* out_messages, float* out_scores,
                                     int32_t* out_counts) {
  if (int rc = check_message_args(c, k, max_messages)) return rc;
  bool empty = false;
  if (int rc = check_scoped_span_args(c, /*wide=*/false, nq, dev_masks, rows, first_row, last_row, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (int rc = check_host_io(queries_host, min_scores, out_messages, out_scores, out_counts)) return rc;
  if (empty) return empty_counts(out_counts, nq);
  return search_messages_and_return(c, queries_host, nq, k, max_messages, out_messages, out_scores, out_counts, [&](const float* d_q, uint32_t base, u64_t* d_hits) {
    return search_scoped_tile(c, d_q, nq, k, min_scores, dev_masks, first_row, last_row, base, d_hits);
  });
}

// ---- scoped batches on the 128/256-query filter tile + rescoring (tavb_route.hip::search_scoped_wide)
int tavb_search_scoped_wide(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row, int64_t last_row,
                            int32_t k, const float* min_scores, int64_t* out_ordinals, float* out_scores, int32_t* out_counts) {
  bool empty = false;
  if (int rc = check_scoped_span_args(c, /*wide=*/true, nq, dev_masks, rows, first_row, last_row, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (int rc = check_host_io(queries_host, min_scores, out_ordinals, out_scores, out_counts)) return rc;
  if (empty) return empty_counts(out_counts, nq);
  DeviceGuard guard(c->device);
  u64_t* target;
  if (int rc = reserve_key_target(c, nq, k, &target)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  c->last_graph = 0;
  if (int rc = search_scoped_wide(c, d_q, nq, k, min_scores, dev_masks, first_row, last_row, 0u, target)) return rc;
  return collect_keys(c, target, nq, k, c->ordinal_base, out_ordinals, out_scores, out_counts);
}

int tavb_search_scoped_wide_device(tavb_ctx* c, const float* dev_queries, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row,
                                   int64_t last_row, int32_t k, const float* min_scores, tavb_key* out_keys) {
  bool empty = false;
  if (int rc = check_scoped_span_args(c, /*wide=*/true, nq, dev_masks, rows, first_row, last_row, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (int rc = check_device_io(dev_queries, min_scores, out_keys)) return rc;
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  if (empty) return fill_empty_keys(c, reinterpret_cast<u64_t*>(out_keys), (int64_t)nq * k);  // no tile launch
  c->last_graph = 0;  // (the one device form of a tile route that clears it)
  return search_scoped_wide(c, dev_queries, nq, k, min_scores, dev_masks, first_row, last_row, (uint32_t)c->ordinal_base, reinterpret_cast<u64_t*>(out_keys));
}

int tavb_search_messages_scoped_wide(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row,
                                     int64_t last_row, int32_t k, const float* min_scores, int32_t max_messages, int64_t* out_messages, float* out_scores,
                                     int32_t* out_counts) {
  if (int rc = check_message_args(c, k, max_messages)) return rc;
  bool empty = false;
  if (int rc = check_scoped_span_args(c, /*wide=*/true, nq, dev_masks, rows, first_row, last_row, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (int rc = check_host_io(queries_host, min_scores, out_messages, out_scores, out_counts)) return rc;
  if (empty) return empty_counts(out_counts, nq);
  return search_messages_and_return(c, queries_host, nq, k, max_messages, out_messages, out_scores, out_counts, [&](const float* d_q, uint32_t base, u64_t* d_hits) {
    return search_scoped_wide(c, d_q, nq, k, min_scores, dev_masks, first_row, last_row, base, d_hits);
  });
}

// ---- the messages form of an unmasked batch: the accepted messages' bitmap is staged behind the search (its own tail, not
// search_messages_and_return's), and the keys carry LOCAL rows (index_base 0): they only index the map
int tavb_search_messages_batch(tavb_ctx* c, const float* queries_host, int32_t nq, int32_t k, const float* min_scores, const int32_t* accept_msgs_host,
                               int64_t n_accept, int32_t max_messages, int64_t* out_messages, float* out_scores, int32_t* out_counts) {
  if (int rc = check_message_args(c, k, max_messages)) return rc;
  if (nq < 0) return fail(TAVB_E_INVALID, "nq must be >= 0");
  if (n_accept < -1 || (n_accept > 0 && !accept_msgs_host)) return fail(TAVB_E_INVALID, "bad accept list");
  if (nq == 0) return TAVB_OK;
  if (int rc = check_host_io(queries_host, min_scores, out_messages, out_scores, out_counts)) return rc;
  if (c->rows == 0) return empty_counts(out_counts, nq);
  DeviceGuard guard(c->device);
  u64_t* d_hits;
  if (int rc = reserve_message_batch(c, nq, k, &d_hits)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  c->last_graph = 0;
  if (int rc = tavb_search_device_dispatch(c, d_q, nq, k, min_scores, 0u, d_hits)) return rc;
  const uint32_t* d_accept_bits = nullptr;
  if (n_accept >= 0)
    if (int rc = stage_accept_bitmap(c, accept_msgs_host, n_accept, &d_accept_bits)) return rc;
  return rerank_batch_and_return(c, d_hits, nq, k, 0u, d_accept_bits, max_messages, out_messages, out_scores, out_counts);
}

}  // extern "C"
