// The batched and masked lookups of the C ABI (include/tavb.h): the batched resident subset (the gather route of a masked batch), masked
// batches on the 32/64-query tile and on the 128/256-query filter tile, and the row masks themselves.  Host code only: the tile routes are
// tavb_route.hip's, the large-k passes tavb_lookup_topk.hip's, the staging tavb_lookup.hip's, the mask kernels live in tavb_mask.hip.

#include "tavb_ctx.h"

using namespace tavb::host;

namespace {

// ---- where the keys of a batched host-synchronous lookup land: up to kPinnedKeysMax of them in pinned host memory (h_out: the last kernel
// writes them there, as in the single-query forms -- a remap of a few KiB runs on them in place); more are written in device memory
// (d_out) and copied out once -- no merge writes megabytes over PCIe.
constexpr size_t kPinnedKeysMax = 4096;

int reserve_key_target(tavb_ctx* c, size_t n_keys, u64_t** target) {
  if (int rc = c->h_out.reserve(n_keys * sizeof(u64_t))) return rc;
  *target = reinterpret_cast<u64_t*>(c->h_out.ptr);
  if (n_keys <= kPinnedKeysMax) return TAVB_OK;
  if (int rc = c->d_out.reserve(n_keys * sizeof(u64_t))) return rc;
  *target = reinterpret_cast<u64_t*>(c->d_out.ptr);
  return TAVB_OK;
}

// the keys at `target` -> h_out (when they are not there already), ONE synchronise, the caller's arrays
int collect_keys(tavb_ctx* c, const u64_t* target, int nq, int k, int64_t base, int64_t* ordinals, float* scores, int32_t* counts) {
  if (target != c->h_out.ptr) TAVB_HIP(hipMemcpyAsync(c->h_out.ptr, target, (size_t)nq * k * sizeof(u64_t), hipMemcpyDeviceToHost, c->stream));
  return sync_decode(c, nq, k, base, ordinals, scores, counts);
}

}  // namespace

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
  if (!queries_host || !min_scores || !out || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  c->last_topk_refine = 0;
  c->topk_rounds_pending = 0;
  c->last_direct = 0;
  c->masked_route = 1;  // the gather route of a masked batch
  if (n_subset == 0 || c->rows == 0) {
    for (int q = 0; q < nq; ++q) out_counts[q] = 0;
    return TAVB_OK;
  }
  if (!dev_rows) return fail(TAVB_E_INVALID, "null dev_rows");
  DeviceGuard guard(c->device);
  const size_t n_keys = (size_t)nq * k;
  u64_t* keys;
  int32_t* rounds;
  if (int rc = reserve_topk_out(c, nq, k, &keys, &rounds)) return rc;
  u64_t* target;
  if (int rc = reserve_key_target(c, n_keys, &target)) return rc;  // (h_out: the rounds behind the keys stay reserved)
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  if (k <= TAVB_MAX_FUSED_K) {
    if (int rc = search_device_impl(c, d_q, nq, k, min_scores, dev_rows, n_subset, 0u, target)) return rc;
  } else {
    if (int rc = search_topk_impl(c, d_q, nq, k, min_scores, dev_rows, n_subset, 0u, target, rounds)) return rc;
  }
  if (remap) {
    hipError_t e = tavb::launch_remap_positions(target, target, (int64_t)n_keys, dev_rows, n_subset, 0u, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "remap launch failed: %s", hipGetErrorString(e));
  }
  if (int rc = collect_keys(c, target, nq, k, remap ? c->ordinal_base : 0, out, out_scores, out_counts)) return rc;
  if (k > TAVB_MAX_FUSED_K) note_rounds(c, rounds, nq);
  return TAVB_OK;
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
  if (!dev_queries || !min_scores || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  if (remap)
    if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  c->last_topk_refine = 0;
  c->topk_rounds_pending = 0;
  c->last_direct = 0;
  c->masked_route = 1;  // the gather route of a masked batch
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
  if (remap) {
    hipError_t e = tavb::launch_remap_positions(target, out, (int64_t)n_keys, dev_rows, n_subset, (uint32_t)c->ordinal_base, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "remap launch failed: %s", hipGetErrorString(e));
  }
  return TAVB_OK;
}

// ---- masked batches on the 32/64-query tile (tavb_route.hip::search_masked_tile)
// what every masked entry point checks first
static int check_masked_head(tavb_ctx* c, int32_t nq, int64_t rows, int32_t k) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = require_corpus(c)) return rc;
  if (k < 1) return fail(TAVB_E_INVALID, "k must be >= 1 (got %d)", k);
  if (nq < 0) return fail(TAVB_E_INVALID, "nq must be >= 0");
  if (rows != c->rows) return fail(TAVB_E_INVALID, "the mask covers %lld rows, the corpus has %lld", (long long)rows, (long long)c->rows);
  return TAVB_OK;
}

// the span of a masked lookup that has something to scan
static int check_masked_span(bool empty, int64_t rows, int64_t first_row, int64_t last_row) {
  if (!empty && (first_row < 0 || last_row >= rows)) return fail(TAVB_E_INVALID, "mask span [%lld, %lld] outside the corpus", (long long)first_row, (long long)last_row);
  return TAVB_OK;
}

// *empty: nothing to scan (an empty corpus, no query, an empty span).
static int check_masked_args(tavb_ctx* c, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row, int64_t last_row, int32_t k, bool* empty) {
  if (int rc = check_masked_head(c, nq, rows, k)) return rc;
  *empty = rows == 0 || nq == 0 || first_row > last_row;
  if (int rc = check_masked_span(*empty, rows, first_row, last_row)) return rc;
  if (!*empty && !dev_bits) return fail(TAVB_E_INVALID, "null dev_bits");
  if (!tavb::skinny_supported(c->dim, k, c->dtype != TAVB_F16))
    return fail(TAVB_E_UNSUPPORTED, "the masked tile serves 1 <= k <= 64 and rows of a multiple of 64 bytes (k = %d, %d bytes): use the gather route", k,
                c->dim * (c->dtype == TAVB_F16 ? 2 : 4));
  return TAVB_OK;
}

int tavb_search_masked_batch(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row, int64_t last_row,
                             int32_t k, const float* min_scores, int64_t* out_ordinals, float* out_scores, int32_t* out_counts) {
  bool empty = false;
  if (int rc = check_masked_args(c, nq, dev_bits, rows, first_row, last_row, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_ordinals || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  if (empty) {
    for (int q = 0; q < nq; ++q) out_counts[q] = 0;
    return TAVB_OK;
  }
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
  if (int rc = check_masked_args(c, nq, dev_bits, rows, first_row, last_row, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!dev_queries || !min_scores || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  if (empty) return fill_empty_keys(c, reinterpret_cast<u64_t*>(out_keys), (int64_t)nq * k);  // no tile launch
  return search_masked_tile(c, dev_queries, nq, k, min_scores, dev_bits, first_row, last_row, (uint32_t)c->ordinal_base, reinterpret_cast<u64_t*>(out_keys));
}

// ---- masked batches on the 128/256-query filter tile + rescoring (tavb_route.hip::search_masked_wide)
static int check_masked_wide_args(tavb_ctx* c, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row, int64_t last_row, const int32_t* dev_rows,
                                  int64_t n_allowed, int32_t k, bool* empty) {
  if (int rc = check_masked_head(c, nq, rows, k)) return rc;
  if (n_allowed < 0 || n_allowed > rows) return fail(TAVB_E_INVALID, "bad row list length");
  *empty = rows == 0 || nq == 0 || first_row > last_row || n_allowed == 0;
  if (int rc = check_masked_span(*empty, rows, first_row, last_row)) return rc;
  if (!*empty && (!dev_bits || !dev_rows)) return fail(TAVB_E_INVALID, "null dev_bits / dev_rows");
  if ((reinterpret_cast<uintptr_t>(dev_bits) & 3) != 0) return fail(TAVB_E_INVALID, "dev_bits must be 4-byte aligned");
  if (!masked_wide_supported(c, k))
    return fail(TAVB_E_UNSUPPORTED, "the masked wide route serves fp16 corpora of up to 16384 halves per row and 1 <= k <= %d (k = %d): use another masked route",
                TAVB_MAX_FUSED_K, k);
  return TAVB_OK;
}

int tavb_search_masked_wide(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row, int64_t last_row,
                            const int32_t* dev_rows, int64_t n_allowed, int32_t k, const float* min_scores, int64_t* out_ordinals, float* out_scores,
                            int32_t* out_counts) {
  bool empty = false;
  if (int rc = check_masked_wide_args(c, nq, dev_bits, rows, first_row, last_row, dev_rows, n_allowed, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_ordinals || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  if (empty) {
    for (int q = 0; q < nq; ++q) out_counts[q] = 0;
    return TAVB_OK;
  }
  DeviceGuard guard(c->device);
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  u64_t* target;
  if (int rc = reserve_key_target(c, (size_t)nq * k, &target)) return rc;
  c->last_graph = 0;
  if (int rc = search_masked_wide(c, d_q, nq, k, min_scores, dev_bits, first_row, last_row, dev_rows, n_allowed, 0u, target)) return rc;
  return collect_keys(c, target, nq, k, c->ordinal_base, out_ordinals, out_scores, out_counts);
}

int tavb_search_masked_wide_device(tavb_ctx* c, const float* dev_queries, int32_t nq, const uint32_t* dev_bits, int64_t rows, int64_t first_row, int64_t last_row,
                                   const int32_t* dev_rows, int64_t n_allowed, int32_t k, const float* min_scores, tavb_key* out_keys) {
  bool empty = false;
  if (int rc = check_masked_wide_args(c, nq, dev_bits, rows, first_row, last_row, dev_rows, n_allowed, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!dev_queries || !min_scores || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  if (empty) return fill_empty_keys(c, reinterpret_cast<u64_t*>(out_keys), (int64_t)nq * k);  // no tile launch
  return search_masked_wide(c, dev_queries, nq, k, min_scores, dev_bits, first_row, last_row, dev_rows, n_allowed, (uint32_t)c->ordinal_base,
                            reinterpret_cast<u64_t*>(out_keys));
}

// ---- row masks (tavb_mask.hip)
int tavb_mask_expand(tavb_ctx* c, const uint32_t* dev_bits, int64_t rows, int32_t* dev_rows_out, int64_t cap, int64_t* out_count) {
  if (int rc = check_ctx(c)) return rc;
  if (!out_count) return fail(TAVB_E_INVALID, "null argument");
  *out_count = 0;
  if (rows < 0 || rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "rows must be 0 .. 2^31 - 2");
  if (cap < 0 || (cap > 0 && !dev_rows_out)) return fail(TAVB_E_INVALID, "bad capacity");
  if (rows == 0) return TAVB_OK;
  if (!dev_bits) return fail(TAVB_E_INVALID, "null dev_bits");
  DeviceGuard guard(c->device);
  if (int rc = c->d_mask_counts.reserve((size_t)tavb::mask_blocks(rows) * sizeof(unsigned))) return rc;
  if (int rc = c->h_out.reserve(sizeof(long long))) return rc;
  long long* total = reinterpret_cast<long long*>(c->h_out.ptr);
  *total = -1;
  hipError_t e = tavb::launch_mask_expand(dev_bits, rows, reinterpret_cast<unsigned*>(c->d_mask_counts.ptr), dev_rows_out, cap, total, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "mask expansion launch failed: %s", hipGetErrorString(e));
  TAVB_HIP(hipStreamSynchronize(c->stream));
  if (*total < 0) return fail(TAVB_E_HIP, "mask expansion wrote no count (internal error)");
  *out_count = (int64_t)*total;
  if (dev_rows_out && *total > cap)
    return fail(TAVB_E_INVALID, "the mask has %lld rows set, dev_rows_out holds %lld", *total, (long long)cap);
  return TAVB_OK;
}

int tavb_mask_pack(tavb_ctx* c, const uint8_t* dev_bytes, int64_t rows, uint32_t* dev_bits_out) {
  if (int rc = check_ctx(c)) return rc;
  if (rows < 0 || rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "rows must be 0 .. 2^31 - 2");
  if (rows == 0) return TAVB_OK;
  if (!dev_bytes || !dev_bits_out) return fail(TAVB_E_INVALID, "null argument");
  DeviceGuard guard(c->device);
  hipError_t e = tavb::launch_mask_pack(dev_bytes, rows, dev_bits_out, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "mask pack launch failed: %s", hipGetErrorString(e));
  return TAVB_OK;
}

// ---- row compaction (the kernels are tavb_mask.hip's): the count pass, ONE synchronise for the kept count and the first removed row, then
// the moves, enqueued and not waited for.  In place the corpus goes through d_compact in passes: pass p's scatter writes only rows below
// the end of pass p (it holds no more rows than the pass kept, and they start at or below the pass' first row), every later pass reads
// only rows at or above that end, and the launches run in stream order -- so no row is overwritten before it was read.
int tavb_compact_rows(tavb_ctx* c, const uint32_t* dev_remove_bits, int64_t rows, void* dev_dst, int64_t* out_rows) {
  if (int rc = check_ctx(c)) return rc;
  if (!out_rows) return fail(TAVB_E_INVALID, "null argument");
  *out_rows = 0;
  if (int rc = require_corpus(c)) return rc;
  if (rows != c->rows) return fail(TAVB_E_INVALID, "the mask covers %lld rows, the corpus has %lld", (long long)rows, (long long)c->rows);
  if (rows == 0) return TAVB_OK;
  if (!dev_remove_bits) return fail(TAVB_E_INVALID, "null dev_remove_bits");
  if ((reinterpret_cast<uintptr_t>(dev_remove_bits) & 3) != 0) return fail(TAVB_E_INVALID, "dev_remove_bits must be 4-byte aligned");
  const int64_t row_bytes = (int64_t)c->dim * (c->dtype == TAVB_F16 ? 2 : 4);
  if ((reinterpret_cast<uintptr_t>(c->corpus) | reinterpret_cast<uintptr_t>(dev_dst)) % (c->dtype == TAVB_F16 ? 2 : 4) != 0)
    return fail(TAVB_E_INVALID, "the corpus and dev_dst must be aligned to their element size");
  DeviceGuard guard(c->device);
  const int blocks = tavb::mask_blocks(rows);
  if (int rc = c->d_mask_counts.reserve((size_t)blocks * sizeof(unsigned))) return rc;
  if (int rc = c->h_out.reserve((size_t)blocks * sizeof(tavb::MaskChunkInfo))) return rc;
  unsigned* counts = reinterpret_cast<unsigned*>(c->d_mask_counts.ptr);
  tavb::MaskChunkInfo* info = reinterpret_cast<tavb::MaskChunkInfo*>(c->h_out.ptr);
  for (int b = 0; b < blocks; ++b) info[b].first = -1;  // (a chunk the kernel wrote holds a row or INT32_MAX here)
  Timed t(c, TAVB_KERNEL_CONVERT);
  hipError_t e = tavb::launch_compact_count(dev_remove_bits, rows, counts, info, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "compaction count launch failed: %s", hipGetErrorString(e));
  TAVB_HIP(hipStreamSynchronize(c->stream));
  int64_t kept = 0, first = 0x7FFFFFFFll;
  for (int b = 0; b < blocks; ++b) {
    if (info[b].first < 0) return fail(TAVB_E_HIP, "chunk %d of the mask wrote no info (internal error)", b);
    kept += info[b].count;
    first = std::min<int64_t>(first, info[b].first);
  }
  *out_rows = kept;
  if (kept == rows) return TAVB_OK;  // nothing to remove: no row moves, no cache is touched, dev_dst is not written and not adopted
  if (kept > rows || first >= rows) return fail(TAVB_E_HIP, "the count pass kept %lld of %lld rows (internal error)", (long long)kept, (long long)rows);
  const char* src = reinterpret_cast<const char*>(c->corpus);
  if (dev_dst) {
    const char* d = reinterpret_cast<const char*>(dev_dst);
    if (d < src + rows * row_bytes && src < d + kept * row_bytes) return fail(TAVB_E_INVALID, "dev_dst overlaps the corpus: pass NULL to compact in place");
    if (kept > 0) {
      e = tavb::launch_compact_gather(src, dev_dst, dev_remove_bits, counts, rows, 0, 0, rows, row_bytes, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "compaction gather launch failed: %s", hipGetErrorString(e));
    }
  } else if (kept > first) {  // (rows below `first` stay where they are; with none kept beyond them there is nothing to move)
    int64_t pass = c->compact_pass_rows > 0 ? c->compact_pass_rows : std::max<int64_t>(((int64_t)64 << 20) / row_bytes, 1);
    pass = std::min<int64_t>((pass + 63) & ~(int64_t)63, (int64_t)1 << 31);
    const int64_t start = first & ~(int64_t)63;  // whole tiles of 64 rows; the rows of the first tile below `first` are rewritten with themselves
    if (int rc = c->d_compact.reserve((size_t)(std::min(pass, rows - start) * row_bytes))) return rc;
    for (int64_t r0 = start; r0 < rows; r0 += pass) {
      const int64_t r1 = std::min(r0 + pass, rows);
      e = tavb::launch_compact_gather(src, c->d_compact.ptr, dev_remove_bits, counts, rows, r0, r0, r1, row_bytes, c->stream);
      if (e == hipSuccess) e = tavb::launch_compact_scatter(c->d_compact.ptr, const_cast<char*>(src), dev_remove_bits, counts, rows, r0, r1, row_bytes, c->stream);
      if (e != hipSuccess) {
        // rows may already have moved: the corpus is in no state to search
        c->norm_rows = 0;
        return fail(TAVB_E_HIP, "compaction launch failed with rows [%lld, %lld) pending: %s", (long long)r0, (long long)rows, hipGetErrorString(e));
      }
    }
  }
  if (int rc = tavb_set_corpus(c, dev_dst ? dev_dst : c->corpus, kept, c->dim, c->dtype, c->ordinal_base)) return rc;
  return tavb_corpus_modified(c, first);
}

// ---- row expansion, the mirror image of the compaction above (the kernels are tavb_mask.hip's): the count pass over the NEW row count -- a
// clear bit is an old row, a set bit a hole -- ONE synchronise for the number of old rows and the first hole, then the moves, enqueued and not
// waited for.  In place the corpus goes through d_compact in passes FROM THE TAIL.  Every row moves to a position at or above its own, so the
// old rows [o0, o1) of the pass for new rows [r0, r1) have o0 <= r0 and o1 <= r1.  The pass stages [o0, o1) and then writes only [r0, r1);
// every later pass lies lower and reads only old rows below ITS o1 <= this pass' o0 <= r0, which no pass so far has written (they wrote only
// at or above r0); and the launches run in stream order -- so no row is overwritten before it was read.  Rows below the tile of the first
// hole never move.
int tavb_expand_rows(tavb_ctx* c, const uint32_t* dev_hole_bits, int64_t new_rows, void* dev_dst, int64_t* out_old_rows) {
  if (int rc = check_ctx(c)) return rc;
  if (!out_old_rows) return fail(TAVB_E_INVALID, "null argument");
  *out_old_rows = 0;
  if (int rc = require_corpus(c)) return rc;
  const int64_t old_rows = c->rows;
  if (new_rows < old_rows) return fail(TAVB_E_INVALID, "the mask covers %lld rows, the corpus has %lld already", (long long)new_rows, (long long)old_rows);
  if (new_rows >= 0x7FFFFFFFll) return fail(TAVB_E_UNSUPPORTED, "at most 2^31-2 rows per device shard (got %lld)", (long long)new_rows);
  if (new_rows == 0) return TAVB_OK;
  if (!dev_hole_bits) return fail(TAVB_E_INVALID, "null dev_hole_bits");
  if ((reinterpret_cast<uintptr_t>(dev_hole_bits) & 3) != 0) return fail(TAVB_E_INVALID, "dev_hole_bits must be 4-byte aligned");
  const int64_t row_bytes = (int64_t)c->dim * (c->dtype == TAVB_F16 ? 2 : 4);
  if ((reinterpret_cast<uintptr_t>(c->corpus) | reinterpret_cast<uintptr_t>(dev_dst)) % (c->dtype == TAVB_F16 ? 2 : 4) != 0)
    return fail(TAVB_E_INVALID, "the corpus and dev_dst must be aligned to their element size");
  DeviceGuard guard(c->device);
  const int blocks = tavb::mask_blocks(new_rows);
  if (int rc = c->d_mask_counts.reserve((size_t)blocks * sizeof(unsigned))) return rc;
  if (int rc = c->h_out.reserve((size_t)blocks * sizeof(tavb::MaskChunkInfo))) return rc;
  unsigned* counts = reinterpret_cast<unsigned*>(c->d_mask_counts.ptr);
  tavb::MaskChunkInfo* info = reinterpret_cast<tavb::MaskChunkInfo*>(c->h_out.ptr);
  for (int b = 0; b < blocks; ++b) info[b].first = -1;  // (a chunk the kernel wrote holds a row or INT32_MAX here)
  Timed t(c, TAVB_KERNEL_CONVERT);
  hipError_t e = tavb::launch_compact_count(dev_hole_bits, new_rows, counts, info, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "expansion count launch failed: %s", hipGetErrorString(e));
  TAVB_HIP(hipStreamSynchronize(c->stream));
  int64_t clear = 0, first = 0x7FFFFFFFll;
  for (int b = 0; b < blocks; ++b) {
    if (info[b].first < 0) return fail(TAVB_E_HIP, "chunk %d of the mask wrote no info (internal error)", b);
    clear += info[b].count;
    first = std::min<int64_t>(first, info[b].first);
  }
  *out_old_rows = clear;
  if (clear != old_rows)
    return fail(TAVB_E_INVALID, "the mask leaves %lld of %lld rows to the old rows, the corpus has %lld", (long long)clear, (long long)new_rows, (long long)old_rows);
  if (new_rows == old_rows) return TAVB_OK;  // no hole: no row moves, no cache is touched, dev_dst is not written and not adopted
  if (first >= new_rows) return fail(TAVB_E_HIP, "the count pass found no hole among %lld rows (internal error)", (long long)new_rows);
  const char* src = reinterpret_cast<const char*>(c->corpus);
  if (dev_dst) {
    const char* d = reinterpret_cast<const char*>(dev_dst);
    if (src && d < src + old_rows * row_bytes && src < d + new_rows * row_bytes) return fail(TAVB_E_INVALID, "dev_dst overlaps the corpus: pass NULL to expand in place");
    if (old_rows > 0) {
      e = tavb::launch_expand_scatter(src, dev_dst, dev_hole_bits, counts, new_rows, 0, 0, new_rows, row_bytes, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "expansion scatter launch failed: %s", hipGetErrorString(e));
    }
  } else {
    if (!src) return fail(TAVB_E_NO_CORPUS, "no corpus buffer to expand in place: pass dev_dst");
    if (first < old_rows) {  // (rows below `first` stay where they are; with holes only behind the last old row there is nothing to move)
      int64_t pass = c->compact_pass_rows > 0 ? c->compact_pass_rows : std::max<int64_t>(((int64_t)64 << 20) / row_bytes, 1);
      pass = std::min<int64_t>((pass + 63) & ~(int64_t)63, (int64_t)1 << 31);
      const int64_t start = first & ~(int64_t)63;  // whole tiles of 64 rows; the rows of the first tile below `first` are rewritten with themselves
      if (int rc = c->d_compact.reserve((size_t)(std::min(pass, new_rows - start) * row_bytes))) return rc;
      for (int64_t r0 = start + (new_rows - 1 - start) / pass * pass; r0 >= start; r0 -= pass) {
        const int64_t r1 = std::min(r0 + pass, new_rows);
        e = tavb::launch_expand_stage(src, c->d_compact.ptr, dev_hole_bits, counts, new_rows, r0, r1, row_bytes, c->stream);
        if (e == hipSuccess)
          e = tavb::launch_expand_scatter(c->d_compact.ptr, const_cast<char*>(src), dev_hole_bits, counts, new_rows, r0, r0, r1, row_bytes, c->stream);
        if (e != hipSuccess) {
          // rows may already have moved: the corpus is in no state to search
          c->norm_rows = 0;
          return fail(TAVB_E_HIP, "expansion launch failed with rows [%lld, %lld) pending: %s", (long long)start, (long long)r1, hipGetErrorString(e));
        }
      }
    }
  }
  if (int rc = tavb_set_corpus(c, dev_dst ? dev_dst : c->corpus, new_rows, c->dim, c->dtype, c->ordinal_base)) return rc;
  return tavb_corpus_modified(c, first);
}

// ---- scattered row writes: the rows go through the load path's pinned ring and its device slots (tavb_upload_rows), one kernel per chunk
// converts and places them (scatter_rows_kernel, tavb_mask.hip).  The positions are checked on the device first -- ONE synchronise -- so
// that a bad one writes nothing.  The caches of rows below norm_rows are brought up to date, not dropped: norm_rows stays.
int tavb_scatter_rows(tavb_ctx* c, const float* rows_host, int64_t n, int32_t dim, const int32_t* dev_positions) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = require_corpus(c)) return rc;
  if (n < 0) return fail(TAVB_E_INVALID, "bad shape");
  if (dim != c->dim) return fail(TAVB_E_INVALID, "the rows are %d wide, the corpus %d", (int)dim, (int)c->dim);
  if (n == 0) return TAVB_OK;
  if (!rows_host || !dev_positions) return fail(TAVB_E_INVALID, "null pointer");
  if ((reinterpret_cast<uintptr_t>(dev_positions) & 3) != 0) return fail(TAVB_E_INVALID, "dev_positions must be 4-byte aligned");
  if (n > c->rows) return fail(TAVB_E_INVALID, "%lld positions for %lld rows: they cannot be unique", (long long)n, (long long)c->rows);
  DeviceGuard guard(c->device);
  if (int rc = c->h_out.reserve(256)) return rc;
  int* bad = reinterpret_cast<int*>(c->h_out.ptr);
  *bad = 0;
  Timed t(c, TAVB_KERNEL_CONVERT);
  hipError_t e = tavb::launch_scatter_check(dev_positions, n, c->rows, bad, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "position check launch failed: %s", hipGetErrorString(e));
  TAVB_HIP(hipStreamSynchronize(c->stream));
  if (*bad) return fail(TAVB_E_INVALID, "a position is outside the corpus' %lld rows", (long long)c->rows);
  // what the caches cover: the maxima rows [0, norm_rows); the shadow the same rows of an fp32 corpus, or of an fp16 one of an odd width
  const bool f16 = c->dtype == TAVB_F16;
  const int sdim = ((c->dim + 63) / 64) * 64;
  const bool shadowed = !f16 || c->dim % 64 != 0;
  if (c->norm_rows > 0 && (!c->d_norm.ptr || (shadowed && (!c->d_shadow.ptr || c->d_shadow.cap < (size_t)c->norm_rows * sdim * 2)))) c->norm_rows = 0;
  void* shadow = (c->norm_rows > 0 && shadowed) ? c->d_shadow.ptr : nullptr;
  const size_t row_bytes = (size_t)dim * sizeof(float);
  constexpr size_t kSlot = 16u << 20;  // the load path's 16 MiB per staging slot
  const int64_t rows_per_chunk = std::max<int64_t>(1, (int64_t)(kSlot / row_bytes));
  const size_t slot_bytes = (size_t)std::min(rows_per_chunk, n) * row_bytes;
  for (int i = 0; i < 2; ++i) {
    if (int rc = c->h_ring[i].reserve(slot_bytes)) return rc;
    if (int rc = c->d_ring[i].reserve(slot_bytes)) return rc;
    if (!c->ring_done[i]) TAVB_HIP(hipEventCreateWithFlags(&c->ring_done[i], hipEventDisableTiming));
  }
  int64_t done = 0;
  for (int chunk = 0; done < n; ++chunk) {
    const int slot = chunk & 1;
    const int64_t m = std::min(rows_per_chunk, n - done);
    const size_t bytes = (size_t)m * row_bytes;
    if (chunk >= 2) TAVB_HIP(hipEventSynchronize(c->ring_done[slot]));  // the copy and the kernel that used this slot two chunks ago are done
    parallel_copy(c->h_ring[slot].ptr, reinterpret_cast<const char*>(rows_host) + (size_t)done * row_bytes, bytes);
    TAVB_HIP(hipMemcpyAsync(c->d_ring[slot].ptr, c->h_ring[slot].ptr, bytes, hipMemcpyHostToDevice, c->stream));
    e = tavb::launch_scatter_rows(reinterpret_cast<const float*>(c->d_ring[slot].ptr), m, c->dim, dev_positions + done, c->rows, const_cast<void*>(c->corpus), f16, shadow,
                                  sdim, c->norm_rows, reinterpret_cast<float*>(c->d_norm.ptr), c->stream);
    if (e != hipSuccess) {
      c->norm_rows = 0;  // (rows of earlier chunks are written: their caches may be half done)
      return fail(TAVB_E_HIP, "scatter launch failed: %s", hipGetErrorString(e));
    }
    TAVB_HIP(hipEventRecord(c->ring_done[slot], c->stream));
    done += m;
  }
  TAVB_HIP(hipStreamSynchronize(c->stream));  // the caller may free / reuse rows_host
  return TAVB_OK;
}

int tavb_mask_from_messages(tavb_ctx* c, const int32_t* accept_msgs_host, int64_t n_accept, int64_t rows, uint32_t* dev_bits_out) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = require_corpus(c)) return rc;
  if (rows != c->rows) return fail(TAVB_E_INVALID, "the mask covers %lld rows, the corpus has %lld", (long long)rows, (long long)c->rows);
  if (int rc = check_message_map(c)) return rc;
  if (rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "rows must be 0 .. 2^31 - 2");
  if (n_accept < 0 || (n_accept > 0 && !accept_msgs_host)) return fail(TAVB_E_INVALID, "bad accept list");
  if (rows == 0) return TAVB_OK;
  if (!dev_bits_out) return fail(TAVB_E_INVALID, "null argument");
  DeviceGuard guard(c->device);
  const uint32_t* d_accept_bits;
  if (int rc = stage_accept_bitmap(c, accept_msgs_host, n_accept, &d_accept_bits)) return rc;
  Timed t(c, TAVB_KERNEL_CONVERT);
  hipError_t e = tavb::launch_mask_from_messages(c->row_to_msg, rows, d_accept_bits, c->n_messages, dev_bits_out, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "message mask launch failed: %s", hipGetErrorString(e));
  return TAVB_OK;
}

// ---- scope algebra (tavb_mask_from_ranges, tavb_mask_combine; the kernels are tavb_mask.hip's)
// What a call leaves in pinned memory (h_out): the write pass' total, then one MaskChunkInfo per chunk of the mask.
struct AlgebraOut {
  unsigned* counts;  // device: the chunks' popcounts, mask_count_kernel's layout
  long long* total;
  tavb::MaskChunkInfo* info;
  int blocks;
};

static void empty_mask_info(tavb_mask_info* info) {
  info->count = 0;
  info->first_row = 0;
  info->last_row = -1;
}

// what both calls check after the context and their own arguments
static int check_algebra_args(tavb_ctx* c, int64_t rows, int32_t* dev_rows_out, int64_t cap) {
  if (int rc = require_corpus(c)) return rc;
  if (rows != c->rows) return fail(TAVB_E_INVALID, "the mask covers %lld rows, the corpus has %lld", (long long)rows, (long long)c->rows);
  if (rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "rows must be 0 .. 2^31 - 2");
  if (cap < 0 || (cap > 0 && !dev_rows_out)) return fail(TAVB_E_INVALID, "bad capacity");
  return TAVB_OK;
}

static int reserve_algebra(tavb_ctx* c, int64_t rows, AlgebraOut* o) {
  o->blocks = tavb::mask_blocks(rows);
  if (int rc = c->d_mask_counts.reserve((size_t)o->blocks * sizeof(unsigned))) return rc;
  if (int rc = c->h_out.reserve(16 + (size_t)o->blocks * sizeof(tavb::MaskChunkInfo))) return rc;
  o->counts = reinterpret_cast<unsigned*>(c->d_mask_counts.ptr);
  o->total = reinterpret_cast<long long*>(c->h_out.ptr);
  o->info = reinterpret_cast<tavb::MaskChunkInfo*>(reinterpret_cast<char*>(c->h_out.ptr) + 16);
  *o->total = -1;
  for (int b = 0; b < o->blocks; ++b) o->info[b].first = -1;  // (a chunk the kernel wrote holds a row or INT32_MAX here)
  return TAVB_OK;
}

// the row list, when the caller wants one: mask_expand's write pass over the counts the mask's own launch made
static int algebra_write_pass(tavb_ctx* c, const AlgebraOut& o, const uint32_t* dev_bits, int64_t rows, int32_t* dev_rows_out, int64_t cap) {
  if (!dev_rows_out || cap == 0) return TAVB_OK;
  hipError_t e = tavb::launch_mask_write(dev_bits, rows, o.counts, dev_rows_out, cap, o.total, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "mask write launch failed: %s", hipGetErrorString(e));
  return TAVB_OK;
}

// ONE synchronise, then the chunks' infos -> *out_info
static int algebra_collect(tavb_ctx* c, const AlgebraOut& o, int32_t* dev_rows_out, int64_t cap, tavb_mask_info* out_info) {
  TAVB_HIP(hipStreamSynchronize(c->stream));
  int64_t count = 0, first = 0x7FFFFFFFll, last = -1;
  for (int b = 0; b < o.blocks; ++b) {
    const tavb::MaskChunkInfo ci = o.info[b];
    if (ci.first < 0) return fail(TAVB_E_HIP, "chunk %d of the mask wrote no info (internal error)", b);
    count += ci.count;
    first = std::min<int64_t>(first, ci.first);
    last = std::max<int64_t>(last, ci.last);
  }
  if (count > 0) {
    out_info->count = count;
    out_info->first_row = first;
    out_info->last_row = last;
  }
  if (dev_rows_out && cap > 0 && *o.total != count) return fail(TAVB_E_HIP, "the write pass counted %lld rows, the mask has %lld (internal error)", *o.total, (long long)count);
  if (dev_rows_out && count > cap) return fail(TAVB_E_INVALID, "the mask has %lld rows set, dev_rows_out holds %lld", (long long)count, (long long)cap);
  return TAVB_OK;
}

int tavb_mask_from_ranges(tavb_ctx* c, const int64_t* ranges_host, const int32_t* collection_sizes_host, int32_t n_collections, int32_t domain, int64_t rows,
                          uint32_t* dev_bits_out, int32_t* dev_rows_out, int64_t cap, tavb_mask_info* out_info) {
  if (int rc = check_ctx(c)) return rc;
  if (!out_info) return fail(TAVB_E_INVALID, "null argument");
  empty_mask_info(out_info);
  if (domain != 0 && domain != 1) return fail(TAVB_E_INVALID, "domain must be 0 (rows) or 1 (messages), got %d", domain);
  if (n_collections < 0 || n_collections > TAVB_MAX_SCOPE_COLLECTIONS)
    return fail(TAVB_E_INVALID, "a scope has 0 .. %d collections (got %d)", TAVB_MAX_SCOPE_COLLECTIONS, n_collections);
  if (n_collections > 0 && !collection_sizes_host) return fail(TAVB_E_INVALID, "null collection sizes");
  int64_t total = 0;
  for (int i = 0; i < n_collections; ++i) {
    if (collection_sizes_host[i] < 0) return fail(TAVB_E_INVALID, "collection %d has a negative size", i);
    total += collection_sizes_host[i];
  }
  if (total > ((int64_t)1 << 20)) return fail(TAVB_E_INVALID, "a scope has at most 2^20 ranges (got %lld)", (long long)total);
  if (total > 0 && !ranges_host) return fail(TAVB_E_INVALID, "null ranges");
  if (int rc = check_algebra_args(c, rows, dev_rows_out, cap)) return rc;
  if (domain == 1)
    if (int rc = check_message_map(c)) return rc;
  if (rows == 0) return TAVB_OK;
  if (!dev_bits_out) return fail(TAVB_E_INVALID, "null dev_bits_out");
  // every collection sorted, clipped to the domain and merged into disjoint ascending intervals
  const int64_t domain_n = domain == 1 ? c->n_messages : rows;
  tavb::ScopeCollections cols{};
  cols.n = n_collections;
  std::vector<int32_t> merged;
  std::vector<std::pair<int64_t, int64_t>> one;
  const int64_t* r = ranges_host;
  for (int i = 0; i < n_collections; ++i) {
    one.clear();
    for (int j = 0; j < collection_sizes_host[i]; ++j, r += 2) {
      const int64_t s = std::max<int64_t>(r[0], 0), e = std::min<int64_t>(r[1], domain_n);
      if (s < e) one.emplace_back(s, e);
    }
    std::sort(one.begin(), one.end());
    size_t kept = merged.size();
    for (const auto& iv : one) {
      if (merged.size() > kept && iv.first <= merged.back()) {
        merged.back() = (int32_t)std::max<int64_t>(merged.back(), iv.second);
      } else {
        merged.push_back((int32_t)iv.first);
        merged.push_back((int32_t)iv.second);
      }
    }
    cols.offset[i + 1] = (int32_t)(merged.size() / 2);
  }
  for (int i = n_collections; i < TAVB_MAX_SCOPE_COLLECTIONS; ++i) cols.offset[i + 1] = cols.offset[n_collections];
  DeviceGuard guard(c->device);
  AlgebraOut o;
  if (int rc = reserve_algebra(c, rows, &o)) return rc;
  if (!merged.empty()) {
    if (int rc = c->d_scope.reserve(merged.size() * sizeof(int32_t))) return rc;
    // (pageable source: the copy is staged by the runtime before the call returns)
    TAVB_HIP(hipMemcpyAsync(c->d_scope.ptr, merged.data(), merged.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  }
  {
    Timed t(c, TAVB_KERNEL_CONVERT);
    hipError_t e = tavb::launch_mask_from_ranges(reinterpret_cast<const int32_t*>(c->d_scope.ptr), cols, domain == 1 ? c->row_to_msg : nullptr, c->n_messages,
                                                 rows, dev_bits_out, o.counts, o.info, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "range mask launch failed: %s", hipGetErrorString(e));
    if (int rc = algebra_write_pass(c, o, dev_bits_out, rows, dev_rows_out, cap)) return rc;
  }
  return algebra_collect(c, o, dev_rows_out, cap, out_info);
}

int tavb_mask_combine(tavb_ctx* c, int32_t op, const uint32_t* const* dev_masks, int32_t n_masks, int64_t rows, uint32_t* dev_bits_out, int32_t* dev_rows_out,
                      int64_t cap, tavb_mask_info* out_info) {
  if (int rc = check_ctx(c)) return rc;
  if (!out_info) return fail(TAVB_E_INVALID, "null argument");
  empty_mask_info(out_info);
  if (op < TAVB_MASK_AND || op > TAVB_MASK_ANDNOT) return fail(TAVB_E_INVALID, "op must be 0 (and), 1 (or) or 2 (and-not), got %d", op);
  if (n_masks < 1 || n_masks > TAVB_MAX_MASK_OPERANDS) return fail(TAVB_E_INVALID, "a combination has 1 .. %d operands (got %d)", TAVB_MAX_MASK_OPERANDS, n_masks);
  if (!dev_masks) return fail(TAVB_E_INVALID, "null dev_masks");
  if (int rc = check_algebra_args(c, rows, dev_rows_out, cap)) return rc;
  if (rows == 0) return TAVB_OK;
  if (!dev_bits_out) return fail(TAVB_E_INVALID, "null dev_bits_out");
  tavb::MaskOperands ops{};
  ops.n = n_masks;
  ops.op = op;
  for (int j = 0; j < n_masks; ++j) {
    if (!dev_masks[j]) return fail(TAVB_E_INVALID, "operand %d is null", j);
    ops.m[j] = dev_masks[j];
  }
  DeviceGuard guard(c->device);
  AlgebraOut o;
  if (int rc = reserve_algebra(c, rows, &o)) return rc;
  {
    Timed t(c, TAVB_KERNEL_CONVERT);
    hipError_t e = tavb::launch_mask_combine(ops, rows, dev_bits_out, o.counts, o.info, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "mask combine launch failed: %s", hipGetErrorString(e));
    if (int rc = algebra_write_pass(c, o, dev_bits_out, rows, dev_rows_out, cap)) return rc;
  }
  return algebra_collect(c, o, dev_rows_out, cap, out_info);
}

// ---- masks carried through a row edit (the kernels are tavb_mask.hip's).  The count pass over the flags and ONE synchronise for the check
// that they describe an edit from old_rows to new_rows -- before anything is written -- then the remap, one write pass per row list that is
// asked for, and a second synchronise for the outputs' counts and spans.  Pinned (h_out): a total per mask, the flags' chunk infos, every
// output's chunk infos.
int tavb_mask_remap(tavb_ctx* c, int32_t mode, const uint32_t* dev_flags, int64_t old_rows, int64_t new_rows, const uint32_t* const* dev_masks,
                    uint32_t* const* dev_bits_out, int32_t n_masks, int32_t fill, int32_t* const* dev_rows_out, const int64_t* caps, tavb_mask_info* out_info) {
  if (int rc = check_ctx(c)) return rc;
  if (n_masks < 1 || n_masks > TAVB_MAX_MASK_OPERANDS) return fail(TAVB_E_INVALID, "a remap carries 1 .. %d masks (got %d)", TAVB_MAX_MASK_OPERANDS, n_masks);
  if (!out_info) return fail(TAVB_E_INVALID, "null argument");
  for (int j = 0; j < n_masks; ++j) empty_mask_info(&out_info[j]);
  if (mode < TAVB_REMAP_REMOVE || mode > TAVB_REMAP_APPEND) return fail(TAVB_E_INVALID, "mode must be 0 (remove), 1 (insert) or 2 (append), got %d", mode);
  if (old_rows < 0 || old_rows >= 0x7FFFFFFFll || new_rows < 0 || new_rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "rows must be 0 .. 2^31 - 2");
  if (mode == TAVB_REMAP_REMOVE ? new_rows > old_rows : new_rows < old_rows)
    return fail(TAVB_E_INVALID, "%s %lld rows cannot leave %lld", mode == TAVB_REMAP_REMOVE ? "a removal from" : "an insertion into", (long long)old_rows, (long long)new_rows);
  const int64_t flag_rows = mode == TAVB_REMAP_REMOVE ? old_rows : mode == TAVB_REMAP_INSERT ? new_rows : 0;
  if (flag_rows > 0 && !dev_flags) return fail(TAVB_E_INVALID, "null dev_flags");
  if ((reinterpret_cast<uintptr_t>(dev_flags) & 3) != 0) return fail(TAVB_E_INVALID, "dev_flags must be 4-byte aligned");
  if (!dev_masks || !dev_bits_out) return fail(TAVB_E_INVALID, "null argument");
  if (dev_rows_out && !caps) return fail(TAVB_E_INVALID, "row lists without capacities");
  const size_t old_bytes = (size_t)((old_rows + 31) >> 5) * 4, new_bytes = (size_t)((new_rows + 31) >> 5) * 4, flag_bytes = (size_t)((flag_rows + 31) >> 5) * 4;
  auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return na > 0 && nb > 0 && x < y + nb && y < x + na;
  };
  tavb::RemapOperands ops{};
  ops.n = n_masks;
  for (int j = 0; j < n_masks; ++j) {
    if (old_rows > 0 && !dev_masks[j]) return fail(TAVB_E_INVALID, "mask %d is null", j);
    if (new_rows > 0 && !dev_bits_out[j]) return fail(TAVB_E_INVALID, "output %d is null", j);
    if (((reinterpret_cast<uintptr_t>(dev_masks[j]) | reinterpret_cast<uintptr_t>(dev_bits_out[j])) & 3) != 0) return fail(TAVB_E_INVALID, "mask %d must be 4-byte aligned", j);
    if (dev_rows_out && caps[j] < 0) return fail(TAVB_E_INVALID, "bad capacity");
    ops.in[j] = dev_masks[j];
    ops.out[j] = dev_bits_out[j];
  }
  for (int j = 0; j < n_masks; ++j) {  // an output is nobody's input: the removal flags may be carried themselves, and are read again by the compaction
    if (overlap(ops.out[j], new_bytes, dev_flags, flag_bytes)) return fail(TAVB_E_INVALID, "output %d overlaps the flags", j);
    for (int i = 0; i < n_masks; ++i)
      if (overlap(ops.out[j], new_bytes, ops.in[i], old_bytes) || (i != j && overlap(ops.out[j], new_bytes, ops.out[i], new_bytes)))
        return fail(TAVB_E_INVALID, "output %d overlaps mask or output %d", j, i);
  }
  DeviceGuard guard(c->device);
  const int flag_blocks = flag_rows > 0 ? tavb::mask_blocks(flag_rows) : 0, blocks = new_rows > 0 ? tavb::mask_blocks(new_rows) : 0;
  const size_t totals_bytes = 64, n_infos = (size_t)flag_blocks + (size_t)n_masks * blocks;
  if (int rc = c->d_mask_counts.reserve(n_infos * sizeof(unsigned))) return rc;
  if (int rc = c->h_out.reserve(totals_bytes + n_infos * sizeof(tavb::MaskChunkInfo))) return rc;
  static_assert(TAVB_MAX_MASK_OPERANDS * sizeof(long long) <= 64, "the totals come first");
  unsigned* const flag_counts = reinterpret_cast<unsigned*>(c->d_mask_counts.ptr);
  unsigned* const counts = flag_counts + flag_blocks;
  long long* const totals = reinterpret_cast<long long*>(c->h_out.ptr);
  tavb::MaskChunkInfo* const flag_info = reinterpret_cast<tavb::MaskChunkInfo*>(reinterpret_cast<char*>(c->h_out.ptr) + totals_bytes);
  tavb::MaskChunkInfo* const info = flag_info + flag_blocks;
  for (int j = 0; j < n_masks; ++j) totals[j] = -1;
  for (size_t b = 0; b < n_infos; ++b) flag_info[b].first = -1;  // (a chunk a kernel wrote holds a row or INT32_MAX here)
  Timed t(c, TAVB_KERNEL_CONVERT);
  if (flag_blocks > 0) {
    hipError_t e = tavb::launch_compact_count(dev_flags, flag_rows, flag_counts, flag_info, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "remap count launch failed: %s", hipGetErrorString(e));
    TAVB_HIP(hipStreamSynchronize(c->stream));
    int64_t clear = 0;
    for (int b = 0; b < flag_blocks; ++b) {
      if (flag_info[b].first < 0) return fail(TAVB_E_HIP, "chunk %d of the flags wrote no info (internal error)", b);
      clear += flag_info[b].count;
    }
    const int64_t want = mode == TAVB_REMAP_REMOVE ? new_rows : old_rows;
    if (clear != want)
      return fail(TAVB_E_INVALID, "the flags have %lld clear bits among %lld rows, the edit needs %lld", (long long)clear, (long long)flag_rows, (long long)want);
  }
  if (new_rows == 0) return TAVB_OK;
  hipError_t e = mode == TAVB_REMAP_REMOVE ? tavb::launch_mask_remap_squeeze(ops, dev_flags, flag_counts, old_rows, new_rows, counts, info, c->stream)
                                           : tavb::launch_mask_remap_spread(ops, mode == TAVB_REMAP_INSERT ? dev_flags : nullptr, flag_counts, old_rows, new_rows, fill != 0,
                                                                            counts, info, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "mask remap launch failed: %s", hipGetErrorString(e));
  for (int j = 0; j < n_masks; ++j) {
    if (!dev_rows_out || !dev_rows_out[j] || caps[j] == 0) continue;
    e = tavb::launch_mask_write(ops.out[j], new_rows, counts + (size_t)j * blocks, dev_rows_out[j], caps[j], &totals[j], c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "mask write launch failed: %s", hipGetErrorString(e));
  }
  TAVB_HIP(hipStreamSynchronize(c->stream));
  for (int j = 0; j < n_masks; ++j) {
    int64_t count = 0, first = 0x7FFFFFFFll, last = -1;
    for (int b = 0; b < blocks; ++b) {
      const tavb::MaskChunkInfo ci = info[(size_t)j * blocks + b];
      if (ci.first < 0) return fail(TAVB_E_HIP, "chunk %d of output %d wrote no info (internal error)", b, j);
      count += ci.count;
      first = std::min<int64_t>(first, ci.first);
      last = std::max<int64_t>(last, ci.last);
    }
    if (count > 0) {
      out_info[j].count = count;
      out_info[j].first_row = first;
      out_info[j].last_row = last;
    }
  }
  for (int j = 0; j < n_masks; ++j) {
    if (!dev_rows_out || !dev_rows_out[j] || caps[j] == 0) continue;
    if (totals[j] != out_info[j].count)
      return fail(TAVB_E_HIP, "the write pass of output %d counted %lld rows, the mask has %lld (internal error)", j, totals[j], (long long)out_info[j].count);
    if (out_info[j].count > caps[j])
      return fail(TAVB_E_INVALID, "output %d has %lld rows set, its row list holds %lld", j, (long long)out_info[j].count, (long long)caps[j]);
  }
  return TAVB_OK;
}

// ---- batched message lookups: nq key lists [nq, k] on the device (keys carrying index_base + row) -> ONE message_rerank_kernel launch of nq
// workgroups -> ONE device-to-host copy -> the callers' arrays.  d_out holds both: the hits in its first nq * k keys, the message keys behind.
static int rerank_batch_and_return(tavb_ctx* c, const u64_t* d_hits, int nq, int k, uint32_t index_base, const uint32_t* d_accept_bits, int32_t max_messages,
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
static int reserve_message_batch(tavb_ctx* c, int nq, int k, u64_t** d_hits) {
  const size_t n_keys = (size_t)nq * k;
  if (int rc = c->h_out.reserve(n_keys * sizeof(u64_t))) return rc;
  if (int rc = c->d_out.reserve(2 * n_keys * sizeof(u64_t))) return rc;
  *d_hits = reinterpret_cast<u64_t*>(c->d_out.ptr);
  return TAVB_OK;
}

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
  } else if (route == 2) {
    if (int rc = check_masked_args(c, nq, dev_bits, rows, first_row, last_row, k, &empty)) return rc;
  } else {
    if (int rc = check_masked_wide_args(c, nq, dev_bits, rows, first_row, last_row, dev_rows, n_allowed, k, &empty)) return rc;
  }
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_messages || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  if (empty) {
    for (int q = 0; q < nq; ++q) out_counts[q] = 0;
    return TAVB_OK;
  }
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  u64_t* d_hits;
  if (int rc = reserve_message_batch(c, nq, k, &d_hits)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  c->last_graph = 0;
  const uint32_t base = (uint32_t)c->ordinal_base;
  if (route == 1) {
    c->last_topk_refine = 0;
    c->topk_rounds_pending = 0;
    c->last_direct = 0;
    c->masked_route = 1;  // the gather route of a masked batch
    if (int rc = search_device_impl(c, d_q, nq, k, min_scores, dev_rows, n_allowed, 0u, d_hits)) return rc;
    hipError_t e = tavb::launch_remap_positions(d_hits, d_hits, (int64_t)nq * k, dev_rows, n_allowed, base, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "remap launch failed: %s", hipGetErrorString(e));
  } else if (route == 2) {
    if (int rc = search_masked_tile(c, d_q, nq, k, min_scores, dev_bits, first_row, last_row, base, d_hits)) return rc;
  } else {
    if (int rc = search_masked_wide(c, d_q, nq, k, min_scores, dev_bits, first_row, last_row, dev_rows, n_allowed, base, d_hits)) return rc;
  }
  return rerank_batch_and_return(c, d_hits, nq, k, base, nullptr, max_messages, out_messages, out_scores, out_counts);
}

// ---- scoped batches: one mask per query (tavb_route.hip::search_scoped_impl)
// what the three entry points check after their own head; *empty: nothing to scan (an empty corpus, no query)
}  // extern "C"
// (shared with the scoped large-k and sorted entry points of tavb_lookup_topk.hip, whose k_max is TAVB_MAX_LARGE_K)
int tavb::host::check_scoped_args(tavb_ctx* c, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k, int32_t k_max, bool* empty) {
  if (int rc = check_masked_head(c, nq, rows, k)) return rc;
  if (k > k_max) return fail(TAVB_E_INVALID, "a scoped batch serves 1 <= k <= %d (got %d)", k_max, k);
  if (rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "rows must be 0 .. 2^31 - 2");
  *empty = rows == 0 || nq == 0;
  if (*empty) return TAVB_OK;
  if (!dev_masks) return fail(TAVB_E_INVALID, "null dev_masks");
  for (int q = 0; q < nq; ++q) {
    if (!dev_masks[q]) return fail(TAVB_E_INVALID, "the mask of query %d is null", q);
    if ((reinterpret_cast<uintptr_t>(dev_masks[q]) & 3) != 0) return fail(TAVB_E_INVALID, "the mask of query %d must be 4-byte aligned", q);
  }
  return TAVB_OK;
}
extern "C" {

static int check_scoped_args(tavb_ctx* c, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k, bool* empty) {
  return check_scoped_args(c, nq, dev_masks, rows, k, TAVB_MAX_FUSED_K, empty);
}

static void note_scoped_route(tavb_ctx* c) {
  c->last_topk_refine = 0;
  c->topk_rounds_pending = 0;
  c->last_direct = 0;
  c->last_graph = 0;
  c->masked_route = 4;  // a scoped batch
}

int tavb_search_scoped_batch(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                             const float* min_scores, int64_t* out_ordinals, float* out_scores, int32_t* out_counts) {
  bool empty = false;
  if (int rc = check_scoped_args(c, nq, dev_masks, rows, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_ordinals || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  note_scoped_route(c);
  if (empty) {
    for (int q = 0; q < nq; ++q) out_counts[q] = 0;
    return TAVB_OK;
  }
  DeviceGuard guard(c->device);
  u64_t* target;
  if (int rc = reserve_key_target(c, (size_t)nq * k, &target)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  if (int rc = search_scoped_impl(c, d_q, nq, k, min_scores, dev_masks, 0u, target, target)) return rc;
  return collect_keys(c, target, nq, k, c->ordinal_base, out_ordinals, out_scores, out_counts);
}

int tavb_search_scoped_device(tavb_ctx* c, const float* dev_queries, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int32_t k,
                              const float* min_scores, tavb_key* out_keys) {
  bool empty = false;
  if (int rc = check_scoped_args(c, nq, dev_masks, rows, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!dev_queries || !min_scores || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  note_scoped_route(c);
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
  if (int rc = check_scoped_args(c, nq, dev_masks, rows, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_messages || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  note_scoped_route(c);
  if (empty) {
    for (int q = 0; q < nq; ++q) out_counts[q] = 0;
    return TAVB_OK;
  }
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  u64_t* d_hits;
  if (int rc = reserve_message_batch(c, nq, k, &d_hits)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  const uint32_t base = (uint32_t)c->ordinal_base;
  if (int rc = search_scoped_impl(c, d_q, nq, k, min_scores, dev_masks, base, d_hits, d_hits)) return rc;
  return rerank_batch_and_return(c, d_hits, nq, k, base, nullptr, max_messages, out_messages, out_scores, out_counts);
}

// ---- scoped batches on the 32/64-query tile (tavb_route.hip::search_scoped_tile)
// check_masked_args with one mask per query; *empty: nothing to scan (an empty corpus, no query, an empty span)
static int check_scoped_tile_args(tavb_ctx* c, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row, int64_t last_row, int32_t k,
                                  bool* empty) {
  if (int rc = check_masked_head(c, nq, rows, k)) return rc;
  if (rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "rows must be 0 .. 2^31 - 2");
  *empty = rows == 0 || nq == 0 || first_row > last_row;
  if (int rc = check_masked_span(*empty, rows, first_row, last_row)) return rc;
  if (!*empty) {
    if (!dev_masks) return fail(TAVB_E_INVALID, "null dev_masks");
    for (int q = 0; q < nq; ++q) {
      if (!dev_masks[q]) return fail(TAVB_E_INVALID, "the mask of query %d is null", q);
      if ((reinterpret_cast<uintptr_t>(dev_masks[q]) & 3) != 0) return fail(TAVB_E_INVALID, "the mask of query %d must be 4-byte aligned", q);
    }
  }
  if (!tavb::skinny_supported(c->dim, k, c->dtype != TAVB_F16))
    return fail(TAVB_E_UNSUPPORTED, "the scoped tile serves 1 <= k <= 64 and rows of a multiple of 64 bytes (k = %d, %d bytes): use the row-list route", k,
                c->dim * (c->dtype == TAVB_F16 ? 2 : 4));
  return TAVB_OK;
}

int tavb_search_scoped_tile(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row, int64_t last_row,
                            int32_t k, const float* min_scores, int64_t* out_ordinals, float* out_scores, int32_t* out_counts) {
  bool empty = false;
  if (int rc = check_scoped_tile_args(c, nq, dev_masks, rows, first_row, last_row, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_ordinals || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  if (empty) {
    for (int q = 0; q < nq; ++q) out_counts[q] = 0;
    return TAVB_OK;
  }
  DeviceGuard guard(c->device);
  u64_t* target;
  if (int rc = reserve_key_target(c, (size_t)nq * k, &target)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  c->last_graph = 0;
  if (int rc = search_scoped_tile(c, d_q, nq, k, min_scores, dev_masks, first_row, last_row, 0u, target)) return rc;
  return collect_keys(c, target, nq, k, c->ordinal_base, out_ordinals, out_scores, out_counts);
}

int tavb_search_scoped_tile_device(tavb_ctx* c, const float* dev_queries, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row,
                                   int64_t last_row, int32_t k, const float* min_scores, tavb_key* out_keys) {
  bool empty = false;
  if (int rc = check_scoped_tile_args(c, nq, dev_masks, rows, first_row, last_row, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!dev_queries || !min_scores || !out_keys) return fail(TAVB_E_INVALID, "null argument");
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
  if (int rc = check_scoped_tile_args(c, nq, dev_masks, rows, first_row, last_row, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_messages || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  if (empty) {
    for (int q = 0; q < nq; ++q) out_counts[q] = 0;
    return TAVB_OK;
  }
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  u64_t* d_hits;
  if (int rc = reserve_message_batch(c, nq, k, &d_hits)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  c->last_graph = 0;
  const uint32_t base = (uint32_t)c->ordinal_base;
  if (int rc = search_scoped_tile(c, d_q, nq, k, min_scores, dev_masks, first_row, last_row, base, d_hits)) return rc;
  return rerank_batch_and_return(c, d_hits, nq, k, base, nullptr, max_messages, out_messages, out_scores, out_counts);
}

int tavb_scope_planes(tavb_ctx* c, const uint32_t* const* dev_masks, int32_t n_masks, int64_t rows, int64_t first_row, int64_t last_row, uint32_t* dev_planes_out) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = require_corpus(c)) return rc;
  if (n_masks < 1) return fail(TAVB_E_INVALID, "n_masks must be >= 1");
  if (rows != c->rows) return fail(TAVB_E_INVALID, "the masks cover %lld rows, the corpus has %lld", (long long)rows, (long long)c->rows);
  if (rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "rows must be 0 .. 2^31 - 2");
  const bool empty = rows == 0 || first_row > last_row;
  if (int rc = check_masked_span(empty, rows, first_row, last_row)) return rc;
  if (empty) return TAVB_OK;  // no plane word to write
  if (!dev_masks || !dev_planes_out) return fail(TAVB_E_INVALID, "null argument");
  if ((reinterpret_cast<uintptr_t>(dev_planes_out) & 63) != 0) return fail(TAVB_E_INVALID, "dev_planes_out must be 64-byte aligned");
  for (int j = 0; j < n_masks; ++j) {
    if (!dev_masks[j]) return fail(TAVB_E_INVALID, "mask %d is null", j);
    if ((reinterpret_cast<uintptr_t>(dev_masks[j]) & 3) != 0) return fail(TAVB_E_INVALID, "mask %d must be 4-byte aligned", j);
  }
  DeviceGuard guard(c->device);
  return build_scope_planes(c, dev_masks, n_masks, scope_plane_blocks(n_masks), first_row, last_row, dev_planes_out);
}

// ---- scoped batches on the 128/256-query filter tile + rescoring (tavb_route.hip::search_scoped_wide)
// check_scoped_tile_args with the wide route's shapes
static int check_scoped_wide_args(tavb_ctx* c, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row, int64_t last_row, int32_t k,
                                  bool* empty) {
  if (int rc = check_masked_head(c, nq, rows, k)) return rc;
  if (rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "rows must be 0 .. 2^31 - 2");
  *empty = rows == 0 || nq == 0 || first_row > last_row;
  if (int rc = check_masked_span(*empty, rows, first_row, last_row)) return rc;
  if (!*empty) {
    if (!dev_masks) return fail(TAVB_E_INVALID, "null dev_masks");
    for (int q = 0; q < nq; ++q) {
      if (!dev_masks[q]) return fail(TAVB_E_INVALID, "the mask of query %d is null", q);
      if ((reinterpret_cast<uintptr_t>(dev_masks[q]) & 3) != 0) return fail(TAVB_E_INVALID, "the mask of query %d must be 4-byte aligned", q);
    }
  }
  if (!masked_wide_supported(c, k))
    return fail(TAVB_E_UNSUPPORTED, "the scoped wide route serves fp16 corpora of up to 16384 halves per row and 1 <= k <= %d (k = %d): use the row-list route",
                TAVB_MAX_FUSED_K, k);
  return TAVB_OK;
}

int tavb_search_scoped_wide(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row, int64_t last_row,
                            int32_t k, const float* min_scores, int64_t* out_ordinals, float* out_scores, int32_t* out_counts) {
  bool empty = false;
  if (int rc = check_scoped_wide_args(c, nq, dev_masks, rows, first_row, last_row, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_ordinals || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  if (empty) {
    for (int q = 0; q < nq; ++q) out_counts[q] = 0;
    return TAVB_OK;
  }
  DeviceGuard guard(c->device);
  u64_t* target;
  if (int rc = reserve_key_target(c, (size_t)nq * k, &target)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  c->last_graph = 0;
  if (int rc = search_scoped_wide(c, d_q, nq, k, min_scores, dev_masks, first_row, last_row, 0u, target)) return rc;
  return collect_keys(c, target, nq, k, c->ordinal_base, out_ordinals, out_scores, out_counts);
}

int tavb_search_scoped_wide_device(tavb_ctx* c, const float* dev_queries, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row,
                                   int64_t last_row, int32_t k, const float* min_scores, tavb_key* out_keys) {
  bool empty = false;
  if (int rc = check_scoped_wide_args(c, nq, dev_masks, rows, first_row, last_row, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!dev_queries || !min_scores || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  if (empty) return fill_empty_keys(c, reinterpret_cast<u64_t*>(out_keys), (int64_t)nq * k);  // no tile launch
  c->last_graph = 0;
  return search_scoped_wide(c, dev_queries, nq, k, min_scores, dev_masks, first_row, last_row, (uint32_t)c->ordinal_base, reinterpret_cast<u64_t*>(out_keys));
}

int tavb_search_messages_scoped_wide(tavb_ctx* c, const float* queries_host, int32_t nq, const uint32_t* const* dev_masks, int64_t rows, int64_t first_row,
                                     int64_t last_row, int32_t k, const float* min_scores, int32_t max_messages, int64_t* out_messages, float* out_scores,
                                     int32_t* out_counts) {
  if (int rc = check_message_args(c, k, max_messages)) return rc;
  bool empty = false;
  if (int rc = check_scoped_wide_args(c, nq, dev_masks, rows, first_row, last_row, k, &empty)) return rc;
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_messages || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  if (empty) {
    for (int q = 0; q < nq; ++q) out_counts[q] = 0;
    return TAVB_OK;
  }
  if (int rc = check_key_ordinals(c, /*device_resident=*/true)) return rc;
  DeviceGuard guard(c->device);
  u64_t* d_hits;
  if (int rc = reserve_message_batch(c, nq, k, &d_hits)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  c->last_graph = 0;
  const uint32_t base = (uint32_t)c->ordinal_base;
  if (int rc = search_scoped_wide(c, d_q, nq, k, min_scores, dev_masks, first_row, last_row, base, d_hits)) return rc;
  return rerank_batch_and_return(c, d_hits, nq, k, base, nullptr, max_messages, out_messages, out_scores, out_counts);
}

int tavb_mask_membership(tavb_ctx* c, const uint32_t* const* dev_masks, int32_t n_masks, int64_t rows, const int32_t* dev_rows, int64_t n, uint8_t* dev_member_out) {
  if (int rc = check_ctx(c)) return rc;
  if (n_masks < 1 || n_masks > TAVB_MAX_MASK_OPERANDS) return fail(TAVB_E_INVALID, "a membership test has 1 .. %d masks (got %d)", TAVB_MAX_MASK_OPERANDS, n_masks);
  if (rows < 0 || rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "rows must be 0 .. 2^31 - 2");
  if (n < 0 || n > rows) return fail(TAVB_E_INVALID, "bad row list length");
  if (n == 0) return TAVB_OK;
  if (!dev_masks || !dev_rows || !dev_member_out) return fail(TAVB_E_INVALID, "null argument");
  if ((reinterpret_cast<uintptr_t>(dev_rows) & 3) != 0) return fail(TAVB_E_INVALID, "dev_rows must be 4-byte aligned");
  tavb::MaskOperands ops{};
  ops.n = n_masks;
  ops.op = TAVB_MASK_OR;
  for (int j = 0; j < n_masks; ++j) {
    if (!dev_masks[j]) return fail(TAVB_E_INVALID, "mask %d is null", j);
    if ((reinterpret_cast<uintptr_t>(dev_masks[j]) & 3) != 0) return fail(TAVB_E_INVALID, "mask %d must be 4-byte aligned", j);
    ops.m[j] = dev_masks[j];
  }
  DeviceGuard guard(c->device);
  Timed t(c, TAVB_KERNEL_CONVERT);
  hipError_t e = tavb::launch_scope_member(ops, dev_rows, n, rows, dev_member_out, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "membership launch failed: %s", hipGetErrorString(e));
  return TAVB_OK;
}

int tavb_search_messages_batch(tavb_ctx* c, const float* queries_host, int32_t nq, int32_t k, const float* min_scores, const int32_t* accept_msgs_host,
                               int64_t n_accept, int32_t max_messages, int64_t* out_messages, float* out_scores, int32_t* out_counts) {
  if (int rc = check_message_args(c, k, max_messages)) return rc;
  if (nq < 0) return fail(TAVB_E_INVALID, "nq must be >= 0");
  if (n_accept < -1 || (n_accept > 0 && !accept_msgs_host)) return fail(TAVB_E_INVALID, "bad accept list");
  if (nq == 0) return TAVB_OK;
  if (!queries_host || !min_scores || !out_messages || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  if (c->rows == 0) {
    for (int q = 0; q < nq; ++q) out_counts[q] = 0;
    return TAVB_OK;
  }
  DeviceGuard guard(c->device);
  u64_t* d_hits;
  if (int rc = reserve_message_batch(c, nq, k, &d_hits)) return rc;
  const float* d_q;
  if (int rc = stage_queries(c, queries_host, nq, &d_q)) return rc;
  c->last_graph = 0;
  // keys carry LOCAL rows here (index_base 0): they only index the map
  if (int rc = tavb_search_device_dispatch(c, d_q, nq, k, min_scores, 0u, d_hits)) return rc;
  const uint32_t* d_accept_bits = nullptr;
  if (n_accept >= 0)
    if (int rc = stage_accept_bitmap(c, accept_msgs_host, n_accept, &d_accept_bits)) return rc;
  return rerank_batch_and_return(c, d_hits, nq, k, 0u, d_accept_bits, max_messages, out_messages, out_scores, out_counts);
}

}  // extern "C"
