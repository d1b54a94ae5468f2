// The row-mask entry points of the C ABI (include/tavb.h): tavb_mask_expand / _pack / _from_messages, the scope algebra
// (tavb_mask_from_ranges, tavb_mask_combine), masks carried through a row edit (tavb_mask_remap) and what a scoped batch is made of
// (tavb_mask_membership, tavb_scope_planes).  Host code only: the kernels live in tavb_mask.hip, the planes' launches in tavb_route.hip.

#include <cstdio>

#include "tavb_ctx.h"

using namespace tavb::host;

namespace tavb {
namespace host __attribute__((visibility("hidden"))) {

void mark_chunk_infos(tavb::MaskChunkInfo* info, size_t n) {
  for (size_t b = 0; b < n; ++b) info[b].first = -1;
}

int sum_chunk_infos(const tavb::MaskChunkInfo* info, int blocks, const char* what, ChunkSum* sum) {
  for (int b = 0; b < blocks; ++b) {
    const tavb::MaskChunkInfo ci = info[b];
    if (ci.first < 0) return fail(TAVB_E_HIP, "chunk %d of %s wrote no info (internal error)", b, what);
    sum->count += ci.count;
    sum->first = std::min<int64_t>(sum->first, ci.first);
    sum->last = std::max<int64_t>(sum->last, ci.last);
  }
  return TAVB_OK;
}

}  // namespace host
}  // namespace tavb

namespace {

void empty_mask_info(tavb_mask_info* info) {
  info->count = 0;
  info->first_row = 0;
  info->last_row = -1;
}

// a mask with rows set: its count and span (an empty one keeps what empty_mask_info wrote)
void fill_mask_info(const ChunkSum& sum, tavb_mask_info* info) {
  if (sum.count == 0) return;
  info->count = sum.count;
  info->first_row = sum.first;
  info->last_row = sum.last;
}

// ---- scope algebra (tavb_mask_from_ranges, tavb_mask_combine)
// What a call leaves in pinned memory (h_out): the write pass' total, then one MaskChunkInfo per chunk of the mask.
struct AlgebraOut {
  unsigned* counts;  // device: the chunks' popcounts, mask_count_kernel's layout
  long long* total;
  tavb::MaskChunkInfo* info;
  int blocks;
};

// what both calls check after the context and their own arguments
int check_algebra_args(tavb_ctx* c, int64_t rows, int32_t* dev_rows_out, int64_t cap) {
  if (int rc = require_corpus(c)) return rc;
  if (rows != c->rows) return fail(TAVB_E_INVALID, "the mask covers %lld rows, the corpus has %lld", (long long)rows, (long long)c->rows);
  if (rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "rows must be 0 .. 2^31 - 2");
  if (cap < 0 || (cap > 0 && !dev_rows_out)) return fail(TAVB_E_INVALID, "bad capacity");
  return TAVB_OK;
}

int reserve_algebra(tavb_ctx* c, int64_t rows, AlgebraOut* o) {
  o->blocks = tavb::mask_blocks(rows);
  if (int rc = c->d_mask_counts.reserve((size_t)o->blocks * sizeof(unsigned))) return rc;
  if (int rc = c->h_out.reserve(16 + (size_t)o->blocks * sizeof(tavb::MaskChunkInfo))) return rc;
  o->counts = reinterpret_cast<unsigned*>(c->d_mask_counts.ptr);
  o->total = reinterpret_cast<long long*>(c->h_out.ptr);
  o->info = reinterpret_cast<tavb::MaskChunkInfo*>(reinterpret_cast<char*>(c->h_out.ptr) + 16);
  *o->total = -1;
  mark_chunk_infos(o->info, o->blocks);
  return TAVB_OK;
}

// the row list, when the caller wants one: mask_expand's write pass over the counts the mask's own launch made
int algebra_write_pass(tavb_ctx* c, const AlgebraOut& o, const uint32_t* dev_bits, int64_t rows, int32_t* dev_rows_out, int64_t cap) {
  if (!dev_rows_out || cap == 0) return TAVB_OK;
  hipError_t e = tavb::launch_mask_write(dev_bits, rows, o.counts, dev_rows_out, cap, o.total, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "mask write launch failed: %s", hipGetErrorString(e));
  return TAVB_OK;
}

// ONE synchronise, then the chunks' infos -> *out_info
int algebra_collect(tavb_ctx* c, const AlgebraOut& o, int32_t* dev_rows_out, int64_t cap, tavb_mask_info* out_info) {
  TAVB_HIP(hipStreamSynchronize(c->stream));
  ChunkSum sum;
  if (int rc = sum_chunk_infos(o.info, o.blocks, "the mask", &sum)) return rc;
  fill_mask_info(sum, out_info);
  if (dev_rows_out && cap > 0 && *o.total != sum.count)
    return fail(TAVB_E_HIP, "the write pass counted %lld rows, the mask has %lld (internal error)", *o.total, (long long)sum.count);
  if (dev_rows_out && sum.count > cap) return fail(TAVB_E_INVALID, "the mask has %lld rows set, dev_rows_out holds %lld", (long long)sum.count, (long long)cap);
  return TAVB_OK;
}

}  // namespace

extern "C" {

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
  for (int j = 0; j < n_masks; ++j) {  // (its own wording, and no alignment check: not check_mask_list)
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

// ---- masks carried through a row edit.  The count pass over the flags and ONE synchronise for the check that they describe an edit from
// old_rows to new_rows -- before anything is written -- then the remap, one write pass per row list that is asked for, and a second
// synchronise for the outputs' counts and spans.  Pinned (h_out): a total per mask, the flags' chunk infos, every output's chunk infos.
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
  for (int j = 0; j < n_masks; ++j) {  // (a mask may be null while there is no old row, and the two pointers share one alignment text: not check_mask_list)
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
  mark_chunk_infos(flag_info, n_infos);
  Timed t(c, TAVB_KERNEL_CONVERT);
  if (flag_blocks > 0) {
    hipError_t e = tavb::launch_compact_count(dev_flags, flag_rows, flag_counts, flag_info, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "remap count launch failed: %s", hipGetErrorString(e));
    TAVB_HIP(hipStreamSynchronize(c->stream));
    ChunkSum flags;
    if (int rc = sum_chunk_infos(flag_info, flag_blocks, "the flags", &flags)) return rc;
    const int64_t want = mode == TAVB_REMAP_REMOVE ? new_rows : old_rows;
    if (flags.count != want)
      return fail(TAVB_E_INVALID, "the flags have %lld clear bits among %lld rows, the edit needs %lld", (long long)flags.count, (long long)flag_rows, (long long)want);
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
    char what[32];
    snprintf(what, sizeof what, "output %d", j);
    ChunkSum sum;
    if (int rc = sum_chunk_infos(info + (size_t)j * blocks, blocks, what, &sum)) return rc;
    fill_mask_info(sum, &out_info[j]);
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

// ---- what a scoped batch is made of: the membership bytes of a row list, the membership planes of a span
int tavb_mask_membership(tavb_ctx* c, const uint32_t* const* dev_masks, int32_t n_masks, int64_t rows, const int32_t* dev_rows, int64_t n, uint8_t* dev_member_out) {
  if (int rc = check_ctx(c)) return rc;
  if (n_masks < 1 || n_masks > TAVB_MAX_MASK_OPERANDS) return fail(TAVB_E_INVALID, "a membership test has 1 .. %d masks (got %d)", TAVB_MAX_MASK_OPERANDS, n_masks);
  if (rows < 0 || rows >= 0x7FFFFFFFll) return fail(TAVB_E_INVALID, "rows must be 0 .. 2^31 - 2");
  if (n < 0 || n > rows) return fail(TAVB_E_INVALID, "bad row list length");
  if (n == 0) return TAVB_OK;
  if (!dev_masks || !dev_rows || !dev_member_out) return fail(TAVB_E_INVALID, "null argument");
  if ((reinterpret_cast<uintptr_t>(dev_rows) & 3) != 0) return fail(TAVB_E_INVALID, "dev_rows must be 4-byte aligned");
  if (int rc = check_mask_list(dev_masks, n_masks, "mask")) return rc;
  tavb::MaskOperands ops{};
  ops.n = n_masks;
  ops.op = TAVB_MASK_OR;
  for (int j = 0; j < n_masks; ++j) ops.m[j] = dev_masks[j];
  DeviceGuard guard(c->device);
  Timed t(c, TAVB_KERNEL_CONVERT);
  hipError_t e = tavb::launch_scope_member(ops, dev_rows, n, rows, dev_member_out, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "membership launch failed: %s", hipGetErrorString(e));
  return TAVB_OK;
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
  if (int rc = check_mask_list(dev_masks, n_masks, "mask")) return rc;
  DeviceGuard guard(c->device);
  return build_scope_planes(c, dev_masks, n_masks, scope_plane_blocks(n_masks), first_row, last_row, dev_planes_out);
}

}  // extern "C"
