// Rows of the corpus as queries (include/tavb.h): tavb_search_rows, tavb_search_rows_device, tavb_search_rows_sorted and tavb_gather_rows_f32.
// Per wave of at most "rows_query_wave" rows: ONE gather launch (rows -> a float32 query batch in d_rows_query), the lookup every other
// device-resident batch takes (tavb_search_device_dispatch up to TAVB_MAX_FUSED_K keys, the large-k route beyond) for k + 1 keys, and ONE
// drop_self launch that takes the query's own row out of its list.  Host code only: the kernels live in tavb_rows_query.hip.

#include "tavb_ctx.h"

using namespace tavb::host;

namespace {

// context, corpus, n, the range of k: with the own row taken out the lookup asks for k + 1 keys, which tavb_search_topk serves up to TAVB_MAX_LARGE_K
int check_rows_head(tavb_ctx* c, int64_t n, int32_t k, bool exclude_self) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = require_corpus(c)) return rc;
  if (n < 0 || n >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "n must be 0 .. 2^31 - 2 (got %lld)", (long long)n);
  const int k_max = exclude_self ? TAVB_MAX_LARGE_K - 1 : TAVB_MAX_LARGE_K;
  if (k < 1 || k > k_max) return fail(TAVB_E_INVALID, "k must be 1 .. %d (got %d)", k_max, k);
  return TAVB_OK;
}

// positions on the host, each checked against the corpus -> pinned h_stage -> d_rows_pos (the copy is enqueued)
int stage_positions(tavb_ctx* c, const int32_t* positions_host, int64_t n, const int32_t** d_pos) {
  const size_t bytes = (size_t)n * sizeof(int32_t);
  if (int rc = c->h_stage.reserve(bytes)) return rc;
  if (int rc = c->d_rows_pos.reserve(bytes)) return rc;
  int32_t* staged = reinterpret_cast<int32_t*>(c->h_stage.ptr);
  for (int64_t i = 0; i < n; ++i) {
    const int32_t p = positions_host[i];
    if (p < 0 || (int64_t)p >= c->rows) return fail(TAVB_E_INVALID, "position %lld: row %d out of range [0, %lld)", (long long)i, p, (long long)c->rows);
    staged[i] = p;
  }
  TAVB_HIP(hipMemcpyAsync(c->d_rows_pos.ptr, staged, bytes, hipMemcpyHostToDevice, c->stream));
  *d_pos = reinterpret_cast<const int32_t*>(c->d_rows_pos.ptr);
  return TAVB_OK;
}

int gather_wave(tavb_ctx* c, const int32_t* d_pos, int64_t n, float* d_q) {
  Timed t(c, TAVB_KERNEL_CONVERT);
  const hipError_t e = tavb::launch_rows_to_queries(c->corpus, c->dtype == TAVB_F16, c->rows, c->dim, d_pos, n, d_q, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "row gather launch failed: %s", hipGetErrorString(e));
  ++c->last_rows_query;
  return TAVB_OK;
}

// The waves of one call: positions on the device -> out [n][k] sorted, zero-padded keys carrying index_base + row (+ counts [n], optional), both
// device-writable; nothing is waited for on routes that wait for nothing.  The workspaces are sized once, by the first (largest) wave.
int search_rows_impl(tavb_ctx* c, const int32_t* d_pos, int64_t n, int k, bool exclude_self, const float* min_scores /*host, n*/, uint32_t index_base,
                     u64_t* out, int32_t* counts) {
  const int kk = k + (exclude_self ? 1 : 0);
  const int64_t wave = std::min<int64_t>(c->rows_query_wave, n);
  if (int rc = c->d_rows_query.reserve((size_t)wave * c->dim * sizeof(float))) return rc;
  if (exclude_self)
    if (int rc = c->d_rows_keys.reserve((size_t)wave * kk * sizeof(u64_t))) return rc;
  float* const d_q = reinterpret_cast<float*>(c->d_rows_query.ptr);
  c->last_rows_query = 0;
  c->last_pairs_join = 0;
  c->last_graph = 0;
  c->last_direct = 0;
  for (int64_t w0 = 0; w0 < n; w0 += wave) {
    const int wn = (int)std::min<int64_t>(wave, n - w0);
    u64_t* const wave_out = out + (size_t)w0 * k;
    u64_t* const lists = exclude_self ? reinterpret_cast<u64_t*>(c->d_rows_keys.ptr) : wave_out;
    if (int rc = gather_wave(c, d_pos + w0, wn, d_q)) return rc;
    if (kk <= TAVB_MAX_FUSED_K) {
      if (int rc = tavb_search_device_dispatch(c, d_q, wn, kk, min_scores + w0, index_base, lists)) return rc;
    } else {
      if (int rc = search_topk_async(c, d_q, wn, kk, min_scores + w0, nullptr, c->rows, index_base, lists)) return rc;
    }
    if (exclude_self || counts) {
      Timed t(c, TAVB_KERNEL_MERGE);
      const hipError_t e = tavb::launch_drop_self(lists, exclude_self, d_pos + w0, index_base, wn, k, wave_out, counts ? counts + w0 : nullptr, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "drop-self launch failed: %s", hipGetErrorString(e));
    }
  }
  return TAVB_OK;
}

}  // namespace

extern "C" {

int tavb_gather_rows_f32(tavb_ctx* c, const int32_t* dev_positions, int64_t n, float* dev_out) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = require_corpus(c)) return rc;
  if (n < 0 || n >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "n must be 0 .. 2^31 - 2 (got %lld)", (long long)n);
  if (n == 0) return TAVB_OK;
  if (!dev_positions || !dev_out) return fail(TAVB_E_INVALID, "null argument");
  if (c->rows == 0) return fail(TAVB_E_INVALID, "the corpus has no rows to gather");
  DeviceGuard guard(c->device);
  c->last_rows_query = 0;
  c->last_pairs_join = 0;
  return gather_wave(c, dev_positions, n, dev_out);
}

int tavb_search_rows(tavb_ctx* c, const int32_t* positions_host, int64_t n, int32_t k, int32_t exclude_self, const float* min_scores, int64_t* out_ordinals,
                     float* out_scores, int32_t* out_counts) {
  if (int rc = check_rows_head(c, n, k, exclude_self != 0)) return rc;
  if (n == 0) return TAVB_OK;
  if (!positions_host || !min_scores || !out_ordinals || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  if ((size_t)n * (size_t)k >= ((size_t)1 << 31)) return fail(TAVB_E_UNSUPPORTED, "n x k must stay below 2^31 keys (ask for the rows in several calls)");
  if (c->rows == 0) return empty_counts(out_counts, (int)n);
  DeviceGuard guard(c->device);
  const int32_t* d_pos;
  if (int rc = stage_positions(c, positions_host, n, &d_pos)) return rc;
  // the keys carry LOCAL rows (index_base 0); ordinal_base is added at the decode, as in every host-synchronous form
  const size_t kbytes = (size_t)n * k * sizeof(u64_t);
  if (int rc = c->h_out.reserve(kbytes)) return rc;
  if (int rc = c->d_rows_out.reserve(kbytes)) return rc;
  u64_t* const d_keys = reinterpret_cast<u64_t*>(c->d_rows_out.ptr);
  if (int rc = search_rows_impl(c, d_pos, n, k, exclude_self != 0, min_scores, 0u, d_keys, nullptr)) return rc;
  TAVB_HIP(hipMemcpyAsync(c->h_out.ptr, d_keys, kbytes, hipMemcpyDeviceToHost, c->stream));
  return sync_decode(c, (int)n, k, c->ordinal_base, out_ordinals, out_scores, out_counts);
}

int tavb_search_rows_device(tavb_ctx* c, const int32_t* dev_positions, int64_t n, int32_t k, int32_t exclude_self, const float* min_scores,
                            tavb_key* dev_out_keys, int32_t* dev_out_counts) {
  if (int rc = check_rows_head(c, n, k, exclude_self != 0)) return rc;
  if (n == 0) return TAVB_OK;
  if (!dev_positions || !min_scores || !dev_out_keys) return fail(TAVB_E_INVALID, "null argument");
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  if (c->rows == 0) {
    if (dev_out_counts) TAVB_HIP(hipMemsetAsync(dev_out_counts, 0, (size_t)n * sizeof(int32_t), c->stream));
    return fill_empty_keys(c, reinterpret_cast<u64_t*>(dev_out_keys), n * (int64_t)k);
  }
  return search_rows_impl(c, dev_positions, n, k, exclude_self != 0, min_scores, (uint32_t)c->ordinal_base, reinterpret_cast<u64_t*>(dev_out_keys), dev_out_counts);
}

int tavb_search_rows_sorted(tavb_ctx* c, const int32_t* positions_host, int64_t n, int32_t exclude_self, const float* min_scores, int64_t max_total,
                            int64_t* out_ordinals, float* out_scores, int64_t* out_counts, int64_t* out_total) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = require_corpus(c)) return rc;
  if (n < 0 || n >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "n must be 0 .. 2^31 - 2 (got %lld)", (long long)n);
  if (max_total < 0) return fail(TAVB_E_INVALID, "max_total must be >= 0");
  if (!out_total) return fail(TAVB_E_INVALID, "null argument");
  *out_total = 0;
  if (n == 0) return TAVB_OK;
  if (!positions_host || !min_scores || !out_counts || (max_total > 0 && (!out_ordinals || !out_scores))) return fail(TAVB_E_INVALID, "null argument");
  for (int64_t q = 0; q < n; ++q) out_counts[q] = 0;
  if (c->rows == 0) return TAVB_OK;
  DeviceGuard guard(c->device);
  const int32_t* d_pos;
  if (int rc = stage_positions(c, positions_host, n, &d_pos)) return rc;
  const int64_t wave = std::min<int64_t>(c->rows_query_wave, n);
  if (int rc = c->d_rows_query.reserve((size_t)wave * c->dim * sizeof(float))) return rc;
  float* const d_q = reinterpret_cast<float*>(c->d_rows_query.ptr);
  c->last_rows_query = 0;
  c->last_pairs_join = 0;
  c->last_graph = 0;
  c->last_direct = 0;
  int64_t total = 0;
  for (int64_t w0 = 0; w0 < n; w0 += wave) {
    const int wn = (int)std::min<int64_t>(wave, n - w0);
    if (int rc = gather_wave(c, d_pos + w0, wn, d_q)) return rc;
    int64_t wave_total = 0;
    // (synchronises inside, per group of queries and per piece of results: the batch may be overwritten by the next wave's gather)
    if (int rc = search_sorted_device(c, d_q, wn, c->rows, min_scores + w0, c->ordinal_base, max_total - total, out_ordinals + total, out_scores + total,
                                      out_counts + w0, &wave_total))
      return rc;
    total += wave_total;
  }
  if (exclude_self) {  // on the HOST, after the copy: the sorted route's results are concatenated lists of any length, which drop_self_kernel does not take
    int64_t rd = 0, wr = 0;
    for (int64_t q = 0; q < n; ++q) {
      const int64_t own = c->ordinal_base + positions_host[q], m = out_counts[q];
      int64_t kept = 0;
      bool dropped = false;
      for (int64_t i = 0; i < m; ++i, ++rd) {
        if (!dropped && out_ordinals[rd] == own) {
          dropped = true;
          continue;
        }
        out_ordinals[wr] = out_ordinals[rd];
        out_scores[wr] = out_scores[rd];
        ++wr;
        ++kept;
      }
      out_counts[q] = kept;
    }
    total = wr;
  }
  *out_total = total;
  return TAVB_OK;
}

}  // extern "C"
