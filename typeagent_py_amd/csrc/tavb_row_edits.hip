// The row edits of the C ABI (include/tavb.h): tavb_compact_rows (remove rows), tavb_expand_rows (open holes for inserted rows) and
// tavb_scatter_rows (write rows at given positions).  Host code only: the kernels live in tavb_mask.hip, the load path's staging ring in
// tavb_abi.hip.

#include <optional>

#include "tavb_ctx.h"

using namespace tavb::host;

namespace {

// ---- what compaction and expansion share.  Both make a count pass over a packed mask -- ONE synchronise for the number of clear bits and
// the first set one -- and then enqueue their moves, which are not waited for; in place the corpus goes through d_compact in passes.
int64_t row_bytes_of(const tavb_ctx* c) { return (int64_t)c->dim * (c->dtype == TAVB_F16 ? 2 : 4); }

int check_edit_buffers(const tavb_ctx* c, const void* dev_dst) {
  if ((reinterpret_cast<uintptr_t>(c->corpus) | reinterpret_cast<uintptr_t>(dev_dst)) % (c->dtype == TAVB_F16 ? 2 : 4) != 0)
    return fail(TAVB_E_INVALID, "the corpus and dev_dst must be aligned to their element size");
  return TAVB_OK;
}

struct EditCount {
  unsigned* counts;      // device: the chunks' clear bits, mask_count_kernel's layout
  int64_t clear, first;  // clear bits of the mask; its first set bit (INT32_MAX: none)
};

// `what` names the edit in the message.  *tm: the TAVB_KERNEL_CONVERT interval, opened in front of the launch -- the caller's moves belong to it.
int edit_count_pass(tavb_ctx* c, const uint32_t* dev_bits, int64_t rows, const char* what, std::optional<Timed>* tm, EditCount* n) {
  const int blocks = tavb::mask_blocks(rows);
  if (int rc = c->d_mask_counts.reserve((size_t)blocks * sizeof(unsigned))) return rc;
  if (int rc = c->h_out.reserve((size_t)blocks * sizeof(tavb::MaskChunkInfo))) return rc;
  n->counts = reinterpret_cast<unsigned*>(c->d_mask_counts.ptr);
  tavb::MaskChunkInfo* info = reinterpret_cast<tavb::MaskChunkInfo*>(c->h_out.ptr);
  mark_chunk_infos(info, blocks);
  tm->emplace(c, TAVB_KERNEL_CONVERT);
  hipError_t e = tavb::launch_compact_count(dev_bits, rows, n->counts, info, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "%s count launch failed: %s", what, hipGetErrorString(e));
  TAVB_HIP(hipStreamSynchronize(c->stream));
  ChunkSum sum;
  if (int rc = sum_chunk_infos(info, blocks, "the mask", &sum)) return rc;
  n->clear = sum.count;
  n->first = sum.first;
  return TAVB_OK;
}

// The passes of an in-place edit of `rows` rows whose first moved row is `first`: *pass rows each ("compact_pass_rows", or 64 MiB worth of
// rows; whole tiles of 64 rows, at most 2^31), from *start on -- the rows of the first tile below `first` are rewritten with themselves --
// and d_compact reserved for one pass.
int reserve_edit_passes(tavb_ctx* c, int64_t rows, int64_t first, int64_t row_bytes, int64_t* pass, int64_t* start) {
  *pass = c->compact_pass_rows > 0 ? c->compact_pass_rows : std::max<int64_t>(((int64_t)64 << 20) / row_bytes, 1);
  *pass = std::min<int64_t>((*pass + 63) & ~(int64_t)63, (int64_t)1 << 31);
  *start = first & ~(int64_t)63;
  return c->d_compact.reserve((size_t)(std::min(*pass, rows - *start) * row_bytes));
}

}  // namespace

extern "C" {

// ---- row compaction: the count pass for the kept count and the first removed row, then the moves.  In place the corpus goes through
// d_compact in passes: pass p's scatter writes only rows below the end of pass p (it holds no more rows than the pass kept, and they start
// at or below the pass' first row), every later pass reads only rows at or above that end, and the launches run in stream order -- so no
// row is overwritten before it was read.
int tavb_compact_rows(tavb_ctx* c, const uint32_t* dev_remove_bits, int64_t rows, void* dev_dst, int64_t* out_rows) {
  if (int rc = check_ctx(c)) return rc;
  if (!out_rows) return fail(TAVB_E_INVALID, "null argument");
  *out_rows = 0;
  if (int rc = require_corpus(c)) return rc;
  if (rows != c->rows) return fail(TAVB_E_INVALID, "the mask covers %lld rows, the corpus has %lld", (long long)rows, (long long)c->rows);
  if (rows == 0) return TAVB_OK;
  if (!dev_remove_bits) return fail(TAVB_E_INVALID, "null dev_remove_bits");
  if ((reinterpret_cast<uintptr_t>(dev_remove_bits) & 3) != 0) return fail(TAVB_E_INVALID, "dev_remove_bits must be 4-byte aligned");
  const int64_t row_bytes = row_bytes_of(c);
  if (int rc = check_edit_buffers(c, dev_dst)) return rc;
  DeviceGuard guard(c->device);
  std::optional<Timed> t;
  EditCount n;
  if (int rc = edit_count_pass(c, dev_remove_bits, rows, "compaction", &t, &n)) return rc;
  const int64_t kept = n.clear, first = n.first;
  *out_rows = kept;
  if (kept == rows) return TAVB_OK;  // nothing to remove: no row moves, no cache is touched, dev_dst is not written and not adopted
  if (kept > rows || first >= rows) return fail(TAVB_E_HIP, "the count pass kept %lld of %lld rows (internal error)", (long long)kept, (long long)rows);
  const char* src = reinterpret_cast<const char*>(c->corpus);
  hipError_t e = hipSuccess;
  if (dev_dst) {
    const char* d = reinterpret_cast<const char*>(dev_dst);
    if (d < src + rows * row_bytes && src < d + kept * row_bytes) return fail(TAVB_E_INVALID, "dev_dst overlaps the corpus: pass NULL to compact in place");
    if (kept > 0) {
      e = tavb::launch_compact_gather(src, dev_dst, dev_remove_bits, n.counts, rows, 0, 0, rows, row_bytes, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "compaction gather launch failed: %s", hipGetErrorString(e));
    }
  } else if (kept > first) {  // (rows below `first` stay where they are; with none kept beyond them there is nothing to move)
    int64_t pass, start;
    if (int rc = reserve_edit_passes(c, rows, first, row_bytes, &pass, &start)) return rc;
    for (int64_t r0 = start; r0 < rows; r0 += pass) {
      const int64_t r1 = std::min(r0 + pass, rows);
      e = tavb::launch_compact_gather(src, c->d_compact.ptr, dev_remove_bits, n.counts, rows, r0, r0, r1, row_bytes, c->stream);
      if (e == hipSuccess) e = tavb::launch_compact_scatter(c->d_compact.ptr, const_cast<char*>(src), dev_remove_bits, n.counts, rows, r0, r1, row_bytes, c->stream);
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

// ---- row expansion, the mirror image of the compaction above: the count pass over the NEW row count -- a clear bit is an old row, a set
// bit a hole -- for the number of old rows and the first hole, then the moves.  In place the corpus goes through d_compact in passes FROM
// THE TAIL.  Every row moves to a position at or above its own, so the old rows [o0, o1) of the pass for new rows [r0, r1) have o0 <= r0
// and o1 <= r1.  The pass stages [o0, o1) and then writes only [r0, r1); every later pass lies lower and reads only old rows below ITS
// o1 <= this pass' o0 <= r0, which no pass so far has written (they wrote only at or above r0); and the launches run in stream order -- so
// no row is overwritten before it was read.  Rows below the tile of the first hole never move.
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
  const int64_t row_bytes = row_bytes_of(c);
  if (int rc = check_edit_buffers(c, dev_dst)) return rc;
  DeviceGuard guard(c->device);
  std::optional<Timed> t;
  EditCount n;
  if (int rc = edit_count_pass(c, dev_hole_bits, new_rows, "expansion", &t, &n)) return rc;
  const int64_t clear = n.clear, first = n.first;
  *out_old_rows = clear;
  if (clear != old_rows)
    return fail(TAVB_E_INVALID, "the mask leaves %lld of %lld rows to the old rows, the corpus has %lld", (long long)clear, (long long)new_rows, (long long)old_rows);
  if (new_rows == old_rows) return TAVB_OK;  // no hole: no row moves, no cache is touched, dev_dst is not written and not adopted
  if (first >= new_rows) return fail(TAVB_E_HIP, "the count pass found no hole among %lld rows (internal error)", (long long)new_rows);
  const char* src = reinterpret_cast<const char*>(c->corpus);
  hipError_t e = hipSuccess;
  if (dev_dst) {
    const char* d = reinterpret_cast<const char*>(dev_dst);
    if (src && d < src + old_rows * row_bytes && src < d + new_rows * row_bytes) return fail(TAVB_E_INVALID, "dev_dst overlaps the corpus: pass NULL to expand in place");
    if (old_rows > 0) {
      e = tavb::launch_expand_scatter(src, dev_dst, dev_hole_bits, n.counts, new_rows, 0, 0, new_rows, row_bytes, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "expansion scatter launch failed: %s", hipGetErrorString(e));
    }
  } else {
    if (!src) return fail(TAVB_E_NO_CORPUS, "no corpus buffer to expand in place: pass dev_dst");
    if (first < old_rows) {  // (rows below `first` stay where they are; with holes only behind the last old row there is nothing to move)
      int64_t pass, start;
      if (int rc = reserve_edit_passes(c, new_rows, first, row_bytes, &pass, &start)) return rc;
      for (int64_t r0 = start + (new_rows - 1 - start) / pass * pass; r0 >= start; r0 -= pass) {
        const int64_t r1 = std::min(r0 + pass, new_rows);
        e = tavb::launch_expand_stage(src, c->d_compact.ptr, dev_hole_bits, n.counts, new_rows, r0, r1, row_bytes, c->stream);
        if (e == hipSuccess)
          e = tavb::launch_expand_scatter(c->d_compact.ptr, const_cast<char*>(src), dev_hole_bits, n.counts, new_rows, r0, r0, r1, row_bytes, c->stream);
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

}  // extern "C"
