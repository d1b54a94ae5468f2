// The near-duplicate self-join (include/tavb.h): tavb_join_pairs and tavb_plan_pairs_join.  One call: the cached row-norm maxima (and an fp32
// corpus' fp16 shadow) brought up to date and read back -- the one bound of the launch is computed HERE, on the host, so that a bound that
// proves nothing refuses the call before anything is launched --, ONE launch of the triangular join, ONE launch of the exact rescoring, the two
// counters read back, then the kept pairs.  Host code only: the kernels live in tavb_pairs_join.hip.

#include "tavb_ctx.h"

using namespace tavb::host;

extern "C" {

int tavb_plan_pairs_join(int64_t rows, int32_t dim, int32_t dtype, int32_t has_shadow, int32_t single_gpu, int64_t min_rows) {
  if (dtype != TAVB_F32 && dtype != TAVB_F16) return fail(TAVB_E_INVALID, "dtype must be TAVB_F32 or TAVB_F16");
  if (rows < 0 || min_rows < 1) return fail(TAVB_E_INVALID, "bad shape");
  if (dim <= 0 || !tavb::pairs_join_supported(dim)) return 0;  // (the filter tile's width rule: whole K steps of 64 halves)
  if (!single_gpu) return 0;
  if (rows < 2 || rows < min_rows || rows >= 0x7FFFFFFFll) return 0;
  if (dtype == TAVB_F32 && !has_shadow) return 0;  // (the join multiplies the fp16 shadow: "f32_shadow" = 0 keeps the row lookups)
  return 1;
}

int tavb_join_pairs(tavb_ctx* c, float min_score, const uint32_t* dev_mask_bits, int64_t capacity, int64_t* out_i, int64_t* out_j, float* out_scores,
                    int64_t* out_total, int64_t* out_needed) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = require_corpus(c)) return rc;
  if (!out_i || !out_j || !out_scores || !out_total || !out_needed) return fail(TAVB_E_INVALID, "null argument");
  if (capacity < 1 || capacity > ((int64_t)1 << 30)) return fail(TAVB_E_INVALID, "capacity must be 1 .. 2^30 (got %lld)", (long long)capacity);
  if ((reinterpret_cast<uintptr_t>(dev_mask_bits) & 3) != 0) return fail(TAVB_E_INVALID, "the mask must be 4-byte aligned");
  *out_total = 0;
  *out_needed = 0;
  c->last_pairs_join = 0;
  c->pairs_join_candidates = 0;
  c->last_rows_query = 0;
  const bool f32c = (c->dtype == TAVB_F32);
  if (!tavb::pairs_join_supported(c->dim)) return fail(TAVB_E_UNSUPPORTED, "the self-join needs rows of a multiple of 64 elements (dim %d): use the row lookups", c->dim);
  if (f32c && c->f32_shadow == 0) return fail(TAVB_E_UNSUPPORTED, "the self-join of an fp32 corpus needs the fp16 shadow (option f32_shadow)");
  if (c->rows >= 0x7FFFFFFFll) return fail(TAVB_E_UNSUPPORTED, "the self-join serves corpora below 2^31 - 1 rows");
  if (c->rows < 2 || min_score != min_score) return TAVB_OK;  // no pair, or a threshold nothing passes
  DeviceGuard guard(c->device);
  note_route(c, c->masked_route);

  // the bound: R^2 and E^2 from the device, delta and the threshold here
  if (int rc = prepare_join_operand(c)) return rc == TAVB_E_NOMEM ? TAVB_PAIRS_REFUSED : rc;
  if (int rc = c->h_flag.reserve(64)) return rc;
  float* const h_norm = reinterpret_cast<float*>(c->h_flag.ptr);
  TAVB_HIP(hipMemcpyAsync(h_norm, c->d_norm.ptr, 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  TAVB_HIP(hipStreamSynchronize(c->stream));
  const float delta = tavb::pairs_join_delta(h_norm, c->dim);
  if (!(delta < __builtin_inff())) return TAVB_PAIRS_REFUSED;  // a non-finite row: nothing can be proven

  // workspace: counters | candidates [capacity] (i, j) | kept i | kept j | kept scores
  const size_t cap = (size_t)capacity;
  if (int rc = c->d_pairs.reserve(256 + cap * 20)) return rc == TAVB_E_NOMEM ? TAVB_PAIRS_REFUSED : rc;
  char* const ws = reinterpret_cast<char*>(c->d_pairs.ptr);
  unsigned long long* const d_counters = reinterpret_cast<unsigned long long*>(ws);
  uint2* const d_cand = reinterpret_cast<uint2*>(ws + 256);
  uint32_t* const d_i = reinterpret_cast<uint32_t*>(ws + 256 + cap * 8);
  uint32_t* const d_j = d_i + cap;
  float* const d_s = reinterpret_cast<float*>(d_j + cap);
  TAVB_HIP(hipMemsetAsync(d_counters, 0, 2 * sizeof(unsigned long long), c->stream));
  {
    Timed t(c, TAVB_KERNEL_MFMA);
    tavb::PairsJoinParams p{};
    p.rows16 = f32c ? c->d_shadow.ptr : c->corpus;
    p.n = c->rows;
    p.dim = c->dim;
    p.mask = dev_mask_bits;
    p.thr = tavb::pairs_join_threshold(min_score, delta);
    p.capacity = cap;
    p.counter = d_counters;
    p.cand = d_cand;
    const hipError_t e = tavb::launch_pairs_join(p, c->n_cu, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "pairs join launch failed: %s", hipGetErrorString(e));
    c->last_pairs_join = 1;
  }
  {
    Timed t(c, TAVB_KERNEL_RESCORE);
    const hipError_t e = tavb::launch_rescore_pairs(c->corpus, f32c, c->dim, d_counters, cap, d_cand, min_score, d_i, d_j, d_s, c->n_cu, c->stream);
    if (e != hipSuccess) return fail(TAVB_E_HIP, "pairs rescoring launch failed: %s", hipGetErrorString(e));
  }
  unsigned long long* const h_counters = reinterpret_cast<unsigned long long*>(c->h_flag.ptr) + 2;
  TAVB_HIP(hipMemcpyAsync(h_counters, d_counters, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  TAVB_HIP(hipStreamSynchronize(c->stream));
  c->pairs_join_candidates = (int64_t)h_counters[0];
  *out_needed = (int64_t)h_counters[0];
  if (h_counters[0] > cap) return TAVB_PAIRS_NO_FIT;  // nothing was scored, nothing is written
  const size_t total = (size_t)h_counters[1];
  if (total == 0) return TAVB_OK;
  if (int rc = c->h_out.reserve(total * 12)) return rc;
  uint32_t* const h_i = reinterpret_cast<uint32_t*>(c->h_out.ptr);
  uint32_t* const h_j = h_i + total;
  float* const h_s = reinterpret_cast<float*>(h_j + total);
  TAVB_HIP(hipMemcpyAsync(h_i, d_i, total * 4, hipMemcpyDeviceToHost, c->stream));
  TAVB_HIP(hipMemcpyAsync(h_j, d_j, total * 4, hipMemcpyDeviceToHost, c->stream));
  TAVB_HIP(hipMemcpyAsync(h_s, d_s, total * 4, hipMemcpyDeviceToHost, c->stream));
  TAVB_HIP(hipStreamSynchronize(c->stream));
  for (size_t t = 0; t < total; ++t) {
    out_i[t] = c->ordinal_base + (int64_t)h_i[t];
    out_j[t] = c->ordinal_base + (int64_t)h_j[t];
    out_scores[t] = h_s[t];
  }
  *out_total = (int64_t)total;
  return TAVB_OK;
}

}  // extern "C"
