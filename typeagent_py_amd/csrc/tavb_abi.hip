// C ABI of libtavb.so (declared in include/tavb.h), the part that is not a lookup: version and error string, the context and its options,
// corpus, load path, normalise / convert / merge / remap, profiling.  Host code only -- the lookups are in tavb_lookup.hip / tavb_lookup_topk.hip / tavb_lookup_masked.hip, the row
// edits in tavb_row_edits.hip, the row masks in tavb_mask_entry.hip, the routing in tavb_route.hip, the RCCL binding in tavb_comm.hip, the kernels in tavb_scan.hip / tavb_misc.hip / tavb_mfma_wide.hip / ...

#include <cstdarg>
#include <cstdio>
#include <thread>

#include "tavb_ctx.h"

using namespace tavb::host;

namespace tavb {
namespace host __attribute__((visibility("hidden"))) {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

// bumped by every (re)allocation or release of a workspace: captured HIP graphs hold raw pointers into these buffers
std::atomic<unsigned long long> g_alloc_epoch{1};

int drain_timings(tavb_ctx* c) {
  if (c->pending.empty()) return TAVB_OK;
  TAVB_HIP(hipStreamSynchronize(c->stream));
  for (auto& p : c->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.start, p.stop) == hipSuccess) {
      c->total_ms[p.kernel] += ms;
      c->launches[p.kernel] += 1;
    }
    c->free_events.push_back(p.start);
    c->free_events.push_back(p.stop);
  }
  c->pending.clear();
  return TAVB_OK;
}

// host -> pinned copy on a few threads: one core moves ~10 GB/s, PCIe Gen5 x16 takes ~50
void parallel_copy(void* dst, const void* src, size_t bytes) {
  constexpr size_t kMinPerThread = 2u << 20;
  if (bytes < 2 * kMinPerThread) {  // one thread's worth (a single query is 6 KiB): not even the question how many cores there are
    memcpy(dst, src, bytes);
    return;
  }
  unsigned hw = std::thread::hardware_concurrency();
  size_t n = std::min<size_t>(std::min<size_t>(hw ? hw : 1, 8), bytes / kMinPerThread);
  if (n <= 1) {
    memcpy(dst, src, bytes);
    return;
  }
  const size_t per = ((bytes / n) + 63) & ~(size_t)63;
  std::vector<std::thread> pool;
  for (size_t i = 1; i < n; ++i) {
    const size_t off = i * per;
    if (off >= bytes) break;
    const size_t len = std::min(per, bytes - off);
    pool.emplace_back([=] { memcpy(static_cast<char*>(dst) + off, static_cast<const char*>(src) + off, len); });
  }
  memcpy(dst, src, std::min(per, bytes));
  for (auto& t : pool) t.join();
}

}  // namespace host
}  // namespace tavb

extern "C" {

int tavb_version(void) { return TAVB_ABI_VERSION; }

const char* tavb_last_error(void) { return g_last_error.c_str(); }

int tavb_device_count(int* out_count) {
  if (!out_count) return fail(TAVB_E_INVALID, "null out_count");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *out_count = 0;
    return fail(TAVB_E_HIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
  }
  *out_count = n;
  return TAVB_OK;
}

int tavb_create(int device, void* stream, tavb_ctx** out) {
  if (!out) return fail(TAVB_E_INVALID, "null out");
  *out = nullptr;
  int n = 0;
  TAVB_HIP(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(TAVB_E_INVALID, "device %d out of range (have %d)", device, n);
  DeviceGuard guard(device);
  if (!guard.ok) return fail(TAVB_E_HIP, "hipSetDevice(%d) failed", device);
  hipDeviceProp_t prop;
  TAVB_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(TAVB_E_UNSUPPORTED, "device %d is %s; libtavb is built for gfx950 (MI355X) only", device, prop.gcnArchName);
  tavb_ctx* c = new (std::nothrow) tavb_ctx();
  if (!c) return fail(TAVB_E_NOMEM, "out of host memory");
  c->device = device;
  c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (stream) {
    c->stream = reinterpret_cast<hipStream_t>(stream);
    c->own_stream = false;
  } else {
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete c;
      return fail(TAVB_E_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    }
    c->own_stream = true;
  }
  *out = c;
  return TAVB_OK;
}

int tavb_destroy(tavb_ctx* c) {
  if (!c) return TAVB_OK;
  DeviceGuard guard(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (auto& p : c->pending) {
    (void)hipEventDestroy(p.start);
    (void)hipEventDestroy(p.stop);
  }
  for (auto& e : c->free_events) (void)hipEventDestroy(e);
  for (auto& e : c->ring_done)
    if (e) (void)hipEventDestroy(e);
  for (auto& g : c->graphs)
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
  (void)tavb_comm_destroy(c);
  c->for_each_buffer([](Buffer& b) { b.release(); });  // (no destructor does this: the device must be current)
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return TAVB_OK;
}

int tavb_synchronize(tavb_ctx* c) {
  if (int rc = check_ctx(c)) return rc;
  DeviceGuard guard(c->device);
  if (c->comm && c->comm_inflight && c->comm_timeout_ms > 0) {
    if (int rc = comm_wait_or_abort(c)) return rc;
  } else {
    TAVB_HIP(hipStreamSynchronize(c->stream));
    c->comm_inflight = false;
  }
  if (c->topk_rounds_pending > 0) {  // an asynchronous large-k lookup has finished: its refinement rounds
    const int32_t* rounds = reinterpret_cast<const int32_t*>(c->h_topk_rounds.ptr);
    int64_t most = 0;
    for (int q = 0; q < c->topk_rounds_pending; ++q) most = std::max<int64_t>(most, rounds[q]);
    c->last_topk_refine = most;
    c->topk_rounds_pending = 0;
  }
  return TAVB_OK;
}

}  // extern "C"

// ---- options: ONE table for tavb_set_option and tavb_get_option (the meanings are in include/tavb.h and next to the members of tavb_ctx).
// A row names the option, where its value lives and what may be stored there; every row can be read, every row that is not read-only set.
namespace {
constexpr int64_t kBool = INT64_MIN;  // Option::lo of a switch: any value is taken, stored as 0 / 1
constexpr int64_t kNoMax = INT64_MAX;
struct Option {
  const char* name;
  int64_t (*slot)(tavb_ctx*, const int64_t* store);  // reads the value, after storing *store if there is one (AT)
  int64_t lo, hi;               // the values taken: lo .. hi (kNoMax: lo and up; kBool: see above) ...
  bool (*taken)(int64_t);       // ... or, for the odd ones, whatever this accepts,
  const char* taken_text;       // described by this in the error message
  int (*on_set)(tavb_ctx*, int64_t);  // optional, runs first: may refuse the call, or do what has to go with the new value
  bool read_only;
};
#define AT(member)                                                     \
  [](tavb_ctx* c, const int64_t* store) -> int64_t {                   \
    if (store) c->member = static_cast<decltype(c->member)>(*store);   \
    return c->member;                                                  \
  }
#define RANGE(name, member, lo, hi) {name, AT(member), lo, hi, nullptr, nullptr, nullptr, false}
#define AT_LEAST(name, member, lo) RANGE(name, member, lo, kNoMax)
#define SWITCH(name, member) RANGE(name, member, kBool, 0)
#define ODD(name, member, text, ...) {name, AT(member), 0, 0, [](int64_t v) -> bool { return __VA_ARGS__; }, text, nullptr, false}
#define READ_ONLY(name, member) {name, AT(member), 0, 0, nullptr, nullptr, nullptr, true}

const Option kOptions[] = {
    RANGE("scan_blocks", geom.blocks, 0, 65535),
    RANGE("scan_waves", geom.waves, 1, 16),
    ODD("scan_unroll", geom.unroll, "1, 2 or 4", v == 1 || v == 2 || v == 4),
    SWITCH("scan_nt", geom.nt),
    SWITCH("scan_pipe", geom.pipe),
    RANGE("force_tier", geom.tier, 0, 3),
    AT_LEAST("mfma_min_batch", mfma_min_batch, 1),
    AT_LEAST("mfma_min_batch_big", mfma_min_batch_big, 1),
    AT_LEAST("mfma_big_bytes", mfma_big_bytes, 0),
    AT_LEAST("mfma_min_batch_big_f32", mfma_min_batch_big_f32, 1),
    AT_LEAST("mfma_big_bytes_f32", mfma_big_bytes_f32, 0),
    AT_LEAST("mfma_few_bytes_f32", mfma_few_bytes_f32, 0),
    AT_LEAST("mfma_min_batch_f32", mfma_min_batch_f32, 1),
    AT_LEAST("mfma_sample_rows", mfma_sample_rows, -1),
    {"f32_shadow", AT(f32_shadow), 0, 2, nullptr, nullptr,
     [](tavb_ctx* c, int64_t v) {
       if (v == 0) {  // the shadow goes at once; on fp32 corpora the cached norms cover the same rows
         c->d_shadow.release();
         if (c->dtype == TAVB_F32) c->norm_rows = 0;
       }
       return (int)TAVB_OK;
     },
     false},
    AT_LEAST("f32_shadow_min_bytes", f32_shadow_min_bytes, 0),
    ODD("mfma_tile", mfma_tile, "0 (auto), 128 or 256", v == 0 || v == 128 || v == 256),
    RANGE("mfma_sched", mfma_sched, 0, 9),
    AT_LEAST("skinny_min_batch_f32", skinny_min_batch_f32, 1),
    AT_LEAST("skinny_min_batch_f16", skinny_min_batch_f16, 1),
    RANGE("mfma_ladder", mfma_ladder, 0, 64),
    RANGE("mfma_ablate", mfma_ablate, 0, 4095),
    RANGE("mfma_splits", mfma_splits, 0, 4096),
    RANGE("band_max", band_max, TAVB_MAX_FUSED_K, tavb::kBandMax),
    SWITCH("early_exact", early_exact),
    SWITCH("wide_fallback", wide_fallback),
    SWITCH("mfma_bdirect", mfma_bdirect),
    ODD("mfma_shape", mfma_shape, "16 or 32", tavb_plan_filter_shape((int32_t)v, 256, 0, 0, 0, 0) >= 0),
    RANGE("small_direct_keys", small_direct_keys, 64, 1 << 20),
    SWITCH("inline_query", inline_query),
    RANGE("direct_group_max_nq", direct_group_max_nq, 0, TAVB_MAX_GROUPED_QUERIES),
    ODD("direct_group", direct_group, "0, 1, 2, 4 or 8", v == 0 || v == 1 || v == 2 || v == 4 || v == 8),
    ODD("direct_group_wgs", direct_group_wgs, "0 or 8 .. 65536", v == 0 || (v >= 8 && v <= 65536)),
    RANGE("direct_group_keys", direct_group_keys, 64, 1 << 22),
    AT_LEAST("small_direct_bytes", small_direct_bytes, 0),
    SWITCH("comm_force", comm_force),
    AT_LEAST("comm_fail_rank", comm_fail_rank, -1),
    SWITCH("comm_fail_alloc", comm_fail_alloc),
    RANGE("comm_stall_ms", comm_stall_ms, 0, 5000),
    AT_LEAST("comm_timeout_ms", comm_timeout_ms, 0),
    {"comm_reserve_keys", AT(comm_reserve_keys), TAVB_MAX_FUSED_K, (int64_t)1 << 28, nullptr, nullptr,
     [](tavb_ctx* c, int64_t) { return c->comm ? fail(TAVB_E_INVALID, "comm_reserve_keys is read by tavb_comm_init: set it before") : (int)TAVB_OK; }, false},
    AT_LEAST("graph_max_bytes", graph_max_bytes, 0),
    SWITCH("large_k", large_k),
    ODD("topk_buckets", topk_buckets, "a multiple of 64 in 256 .. 4096", v >= 256 && v <= 4096 && v % 64 == 0),
    RANGE("topk_boundary_keys", topk_boundary_keys, 64, TAVB_MAX_LARGE_K),
    AT_LEAST("topk_scores_bytes", topk_scores_bytes, 4096),
    SWITCH("sort_all", sort_all),
    RANGE("sort_stage_keys", sort_stage_keys, 1, (int64_t)1 << 30),
    RANGE("sort_small_keys", sort_small_keys, 0, tavb::kSortSmallMax),
    READ_ONLY("last_shadow", last_shadow),
    READ_ONLY("last_mfma_shape", last_mfma_shape),
    READ_ONLY("last_skinny_kernel", last_skinny_kernel),
    RANGE("mask_tile", mask_tile, 0, 2),
    AT_LEAST("mask_tile_min_bytes", mask_tile_min_bytes, 0),
    RANGE("mask_tile_pct", mask_tile_pct, 0, 1000000),
    READ_ONLY("masked_route", masked_route),
    RANGE("mask_wide", mask_wide, 0, 2),
    RANGE("scope_tile", scope_tile, 0, 2),
    RANGE("scope_wide", scope_wide, 0, 2),
    SWITCH("scope_large_k", scope_large_k),
    SWITCH("top_messages", top_messages),
    SWITCH("top_messages_scoped", top_messages_scoped),
    RANGE("top_messages_tile", top_messages_tile, 0, 2),
    RANGE("top_messages_tile_min_batch", top_messages_tile_min_batch, 1, 1 << 20),
    RANGE("scope_wave_bytes", scope_wave_bytes, 1, (int64_t)1 << 40),
    RANGE("compact_pass_rows", compact_pass_rows, 0, 0x7FFFFFFE),
    SWITCH("rows_query", rows_query),
    RANGE("rows_query_wave", rows_query_wave, 1, 1 << 20),
    READ_ONLY("rows_query_launches", last_rows_query),
    SWITCH("pairs_join", pairs_join),
    RANGE("pairs_join_min_rows", pairs_join_min_rows, 1, 0x7FFFFFFE),
    RANGE("pairs_join_capacity", pairs_join_capacity, 1, (int64_t)1 << 30),
    RANGE("pairs_join_max_capacity", pairs_join_max_capacity, 1, (int64_t)1 << 30),
    READ_ONLY("pairs_join_launches", last_pairs_join),
    READ_ONLY("pairs_join_candidates", pairs_join_candidates),
    READ_ONLY("norm_rows", norm_rows),
    READ_ONLY("last_direct", last_direct),
    READ_ONLY("last_graph", last_graph),
    READ_ONLY("last_topk_refine", last_topk_refine),
    READ_ONLY("last_tier", last_tier),
    READ_ONLY("compute_units", n_cu),
};
#undef AT
#undef RANGE
#undef AT_LEAST
#undef SWITCH
#undef ODD
#undef READ_ONLY

const Option* find_option(const char* name) {
  for (const Option& o : kOptions)
    if (strcmp(o.name, name) == 0) return &o;
  return nullptr;
}

// "last_flagged" / "last_doomed": word `index` of the last 256-query-tile lookup's work-list header (synchronises)
int read_flag_word(tavb_ctx* c, int index, int64_t* out) {
  *out = 0;
  if (!c->d_flag.ptr) return TAVB_OK;
  DeviceGuard guard(c->device);
  int v = 0;
  TAVB_HIP(hipStreamSynchronize(c->stream));
  TAVB_HIP(hipMemcpy(&v, reinterpret_cast<const int*>(c->d_flag.ptr) + index, sizeof v, hipMemcpyDeviceToHost));
  *out = v;
  return TAVB_OK;
}
}  // namespace

extern "C" {

int tavb_set_option(tavb_ctx* c, const char* name, int64_t v) {
  if (int rc = check_ctx(c)) return rc;
  if (!name) return fail(TAVB_E_INVALID, "null option name");
  const Option* o = find_option(name);
  if (!o || o->read_only) return fail(TAVB_E_INVALID, "unknown option '%s'", name);
  if (o->on_set)
    if (int rc = o->on_set(c, v)) return rc;
  if (o->taken) {
    if (!o->taken(v)) return fail(TAVB_E_INVALID, "%s must be %s", name, o->taken_text);
  } else if (o->lo == kBool) {
    v = v ? 1 : 0;
  } else if (v < o->lo || v > o->hi) {
    if (o->hi == kNoMax) return fail(TAVB_E_INVALID, "%s must be >= %lld", name, (long long)o->lo);
    return fail(TAVB_E_INVALID, "%s must be %lld .. %lld", name, (long long)o->lo, (long long)o->hi);
  }
  o->slot(c, &v);
  return TAVB_OK;
}

int tavb_get_option(tavb_ctx* c, const char* name, int64_t* out) {
  if (int rc = check_ctx(c)) return rc;
  if (!name || !out) return fail(TAVB_E_INVALID, "null argument");
  // the four that compute their answer
  const std::string n(name);
  if (n == "last_flagged") return read_flag_word(c, 0, out);  // queries of the last 256-query-tile lookup that were re-run on the exact tile
  if (n == "last_doomed") return read_flag_word(c, 1, out);   // ... counted by the early verdict; above nq / 2 the last filter phase was skipped
  if (n == "comm_world") {
    *out = c->comm ? c->comm_world : 0;
  } else if (n == "comm_rank") {
    *out = c->comm ? c->comm_rank : -1;
  } else if (const Option* o = find_option(name)) {
    *out = o->slot(c, nullptr);
  } else {
    return fail(TAVB_E_INVALID, "unknown option '%s'", name);
  }
  return TAVB_OK;
}

int tavb_set_corpus(tavb_ctx* c, const void* dev_rows, int64_t rows, int32_t dim, int32_t dtype, int64_t ordinal_base) {
  if (int rc = check_ctx(c)) return rc;
  if (rows < 0) return fail(TAVB_E_INVALID, "rows must be >= 0");
  if (dim < 1) return fail(TAVB_E_INVALID, "dim must be >= 1");
  if (dtype != TAVB_F32 && dtype != TAVB_F16) return fail(TAVB_E_INVALID, "dtype must be TAVB_F32 or TAVB_F16");
  if (rows > 0 && !dev_rows) return fail(TAVB_E_INVALID, "null corpus pointer with rows > 0");
  if (rows >= 0x7FFFFFFFll) return fail(TAVB_E_UNSUPPORTED, "at most 2^31-2 rows per device shard (got %lld)", (long long)rows);
  if (ordinal_base < 0) return fail(TAVB_E_INVALID, "ordinal_base must be >= 0");
  if (dev_rows != c->corpus || dim != c->dim || dtype != c->dtype || rows < c->norm_rows) c->norm_rows = 0;  // cached row-norm maximum: keep it across appends only
  if ((dtype != TAVB_F32 && dim % 64 == 0) || rows == 0) c->d_shadow.release();  // the fp16 shadow belongs to an fp32 corpus, or to an fp16 one of an odd width
  c->corpus = dev_rows;
  c->rows = rows;
  c->dim = dim;
  c->dtype = dtype;
  c->ordinal_base = ordinal_base;
  return TAVB_OK;
}

int tavb_upload_rows(tavb_ctx* c, const float* rows_host, int64_t n_rows, int32_t dim, void* dev_dst, int32_t dst_dtype) {
  if (int rc = check_ctx(c)) return rc;
  if (n_rows < 0 || dim < 1) return fail(TAVB_E_INVALID, "bad shape");
  if (dst_dtype != TAVB_F32 && dst_dtype != TAVB_F16) return fail(TAVB_E_INVALID, "dtype must be TAVB_F32 or TAVB_F16");
  if (n_rows == 0) return TAVB_OK;
  if (!rows_host || !dev_dst) return fail(TAVB_E_INVALID, "null pointer");
  DeviceGuard guard(c->device);
  const size_t row_bytes = (size_t)dim * sizeof(float);
  constexpr size_t kSlot = 16u << 20;  // 16 MiB per staging slot
  const int64_t rows_per_chunk = std::max<int64_t>(1, (int64_t)(kSlot / row_bytes));
  const size_t slot_bytes = (size_t)rows_per_chunk * row_bytes;
  for (int i = 0; i < 2; ++i) {
    if (int rc = c->h_ring[i].reserve(slot_bytes)) return rc;
    if (dst_dtype == TAVB_F16)
      if (int rc = c->d_ring[i].reserve(slot_bytes)) return rc;
    if (!c->ring_done[i]) TAVB_HIP(hipEventCreateWithFlags(&c->ring_done[i], hipEventDisableTiming));
  }
  const size_t dst_elem = dst_dtype == TAVB_F16 ? 2 : 4;
  int64_t done = 0;
  for (int chunk = 0; done < n_rows; ++chunk) {
    const int slot = chunk & 1;
    const int64_t n = std::min(rows_per_chunk, n_rows - done);
    const size_t bytes = (size_t)n * row_bytes;
    if (chunk >= 2) TAVB_HIP(hipEventSynchronize(c->ring_done[slot]));  // the copy (and convert) that used this slot two chunks ago are done
    parallel_copy(c->h_ring[slot].ptr, reinterpret_cast<const char*>(rows_host) + (size_t)done * row_bytes, bytes);  // overlaps the previous chunk's DMA
    char* dst = reinterpret_cast<char*>(dev_dst) + (size_t)done * dim * dst_elem;
    if (dst_dtype == TAVB_F32) {
      TAVB_HIP(hipMemcpyAsync(dst, c->h_ring[slot].ptr, bytes, hipMemcpyHostToDevice, c->stream));
    } else {
      TAVB_HIP(hipMemcpyAsync(c->d_ring[slot].ptr, c->h_ring[slot].ptr, bytes, hipMemcpyHostToDevice, c->stream));
      Timed t(c, TAVB_KERNEL_CONVERT);
      hipError_t e = tavb::launch_f32_to_f16(reinterpret_cast<const float*>(c->d_ring[slot].ptr), dst, n * dim, c->stream);
      if (e != hipSuccess) return fail(TAVB_E_HIP, "convert launch failed: %s", hipGetErrorString(e));
    }
    TAVB_HIP(hipEventRecord(c->ring_done[slot], c->stream));
    done += n;
  }
  TAVB_HIP(hipStreamSynchronize(c->stream));  // the caller may free / reuse rows_host and read dev_dst from other streams
  return TAVB_OK;
}

int tavb_corpus_modified(tavb_ctx* c, int64_t first_row) {
  if (int rc = check_ctx(c)) return rc;
  if (first_row < 0) return fail(TAVB_E_INVALID, "first_row must be >= 0");
  if (first_row < c->norm_rows) c->norm_rows = 0;  // the cached row-norm maximum may be stale: recompute on the next batched lookup
  return TAVB_OK;
}

int tavb_normalize_rows_f32(tavb_ctx* c, const float* dev_in, float* dev_out, int64_t rows, int32_t dim) {
  if (int rc = check_ctx(c)) return rc;
  if (rows < 0 || dim < 1) return fail(TAVB_E_INVALID, "bad shape");
  if (rows == 0) return TAVB_OK;
  if (!dev_in || !dev_out) return fail(TAVB_E_INVALID, "null pointer");
  DeviceGuard guard(c->device);
  Timed t(c, TAVB_KERNEL_NORMALIZE);
  hipError_t e = tavb::launch_normalize_f32(dev_in, dev_out, rows, dim, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "normalize launch failed: %s", hipGetErrorString(e));
  return TAVB_OK;
}

int tavb_convert_f32_to_f16(tavb_ctx* c, const float* dev_in, void* dev_out, int64_t count) {
  if (int rc = check_ctx(c)) return rc;
  if (count < 0) return fail(TAVB_E_INVALID, "bad count");
  if (count == 0) return TAVB_OK;
  if (!dev_in || !dev_out) return fail(TAVB_E_INVALID, "null pointer");
  DeviceGuard guard(c->device);
  Timed t(c, TAVB_KERNEL_CONVERT);
  hipError_t e = tavb::launch_f32_to_f16(dev_in, dev_out, count, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "convert launch failed: %s", hipGetErrorString(e));
  return TAVB_OK;
}

int tavb_merge_device(tavb_ctx* c, const tavb_key* dev_lists, int32_t n_lists, int32_t nq, int32_t k,
                      tavb_key* dev_out_keys) {
  if (int rc = check_ctx(c)) return rc;
  if (n_lists < 1 || nq < 1 || k < 1 || k > TAVB_MAX_FUSED_K) return fail(TAVB_E_INVALID, "bad merge shape");
  if (!dev_lists || !dev_out_keys) return fail(TAVB_E_INVALID, "null argument");
  DeviceGuard guard(c->device);
  Timed t(c, TAVB_KERNEL_MERGE);
  hipError_t e = tavb::launch_merge(reinterpret_cast<const u64_t*>(dev_lists), n_lists, nq, k, /*query_major=*/false,
                                    reinterpret_cast<u64_t*>(dev_out_keys), c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "merge launch failed: %s", hipGetErrorString(e));
  return TAVB_OK;
}

int tavb_merge_topk_device(tavb_ctx* c, const tavb_key* dev_lists, int32_t n_lists, int32_t nq, int32_t k, tavb_key* out_keys) {
  if (int rc = check_ctx(c)) return rc;
  const bool query_major = n_lists < 0;
  if (query_major) n_lists = -n_lists;
  if (n_lists < 1 || n_lists > 64 || nq < 1 || nq > 65535 || k < 1 || k > TAVB_MAX_LARGE_K)
    return fail(TAVB_E_INVALID, "bad merge shape (1 .. 64 lists of 1 .. %d keys, 1 .. 65535 queries)", TAVB_MAX_LARGE_K);
  if (!dev_lists || !out_keys) return fail(TAVB_E_INVALID, "null argument");
  DeviceGuard guard(c->device);
  Timed t(c, TAVB_KERNEL_MERGE);
  hipError_t e = tavb::launch_merge_topk(reinterpret_cast<const u64_t*>(dev_lists), n_lists, nq, k, query_major, reinterpret_cast<u64_t*>(out_keys), c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "merge launch failed: %s", hipGetErrorString(e));
  return TAVB_OK;
}

int tavb_decode_keys(const tavb_key* keys_host, int32_t nq, int32_t k, int64_t* out_ordinals, float* out_scores,
                     int32_t* out_counts) {
  if (nq < 0 || k < 1) return fail(TAVB_E_INVALID, "bad shape");
  if (nq == 0) return TAVB_OK;
  if (!keys_host || !out_ordinals || !out_scores || !out_counts) return fail(TAVB_E_INVALID, "null argument");
  // a rank whose local search failed joins the collective with TAVB_KEY_PEER_FAILED in every slot of its lists; the key sorts above every
  // real one, so it leads every merged list on every rank: the answer is missing a shard and must not be used
  for (int q = 0; q < nq; ++q)
    if (keys_host[(size_t)q * k] == TAVB_KEY_PEER_FAILED) {
      for (int i = 0; i < nq; ++i) out_counts[i] = 0;
      return fail(TAVB_E_PEER, "a rank of the collective lookup failed in its local search: the merged lists are missing its shard");
    }
  decode(reinterpret_cast<const u64_t*>(keys_host), nq, k, 0, out_ordinals, out_scores, out_counts);
  return TAVB_OK;
}

int tavb_remap_key_positions(tavb_ctx* c, tavb_key* dev_keys, int64_t count, const int32_t* dev_map, int64_t map_len) {
  if (int rc = check_ctx(c)) return rc;
  if (count < 0 || map_len < 0) return fail(TAVB_E_INVALID, "bad shape");
  if (count == 0) return TAVB_OK;
  if (!dev_keys || (map_len > 0 && !dev_map)) return fail(TAVB_E_INVALID, "null argument");
  DeviceGuard guard(c->device);
  hipError_t e = tavb::launch_remap_positions(reinterpret_cast<u64_t*>(dev_keys), reinterpret_cast<u64_t*>(dev_keys), count, dev_map, map_len, 0u, c->stream);
  if (e != hipSuccess) return fail(TAVB_E_HIP, "remap launch failed: %s", hipGetErrorString(e));
  return TAVB_OK;
}

int tavb_profile_enable(tavb_ctx* c, int32_t on) {
  if (int rc = check_ctx(c)) return rc;
  DeviceGuard guard(c->device);
  if (!on) {
    if (int rc = drain_timings(c)) return rc;
  }
  c->profiling = on != 0;
  return TAVB_OK;
}

int tavb_profile_reset(tavb_ctx* c) {
  if (int rc = check_ctx(c)) return rc;
  DeviceGuard guard(c->device);
  if (int rc = drain_timings(c)) return rc;
  for (int i = 0; i < TAVB_KERNEL_COUNT; ++i) {
    c->total_ms[i] = 0;
    c->launches[i] = 0;
  }
  return TAVB_OK;
}

int tavb_profile_read(tavb_ctx* c, int32_t kernel_id, double* out_total_ms, int64_t* out_launches) {
  if (int rc = check_ctx(c)) return rc;
  if (kernel_id < 0 || kernel_id >= TAVB_KERNEL_COUNT) return fail(TAVB_E_INVALID, "bad kernel id");
  DeviceGuard guard(c->device);
  if (int rc = drain_timings(c)) return rc;
  if (out_total_ms) *out_total_ms = c->total_ms[kernel_id];
  if (out_launches) *out_launches = c->launches[kernel_id];
  return TAVB_OK;
}

}  // extern "C"
