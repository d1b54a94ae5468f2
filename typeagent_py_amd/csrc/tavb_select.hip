// The band selection behind the 128/256-query tile (tavb_mfma_wide.hip): `select_band_kernel` picks every query's band over the
// candidate buffers of all row ranges, `sample_threshold_kernel` turns a sample pass into admission thresholds.  The buffers' layout
// (CAPW keys each) and the band cut it shares with the tile's own compaction are in tavb_tile.h.

#include <hip/hip_runtime.h>

#include <type_traits>

#include "tavb_tile.h"

namespace tavb {

namespace {

// ---------------------------------------------------------------------------------------------
// BAND of ONE query over the (unsorted) candidate buffers that the workgroups of all row ranges left behind, plus the band
// carried over from the earlier ladder phases -- and, from it, the admission threshold of the next phase.
// The band = every key whose score is within band[q] (= 2 delta_q, tavb_rescore.hip) of the query's k-th best score: exactly
// the rows that can still be in the exact top k once the candidates are rescored with the fp32 query.  Its size is whatever the
// data makes it (k + a few on isotropic data, a whole cluster of near-duplicates on clustered data), up to kc_max.  Where a
// band did not fit on the way (a candidate buffer in the tile kernel, the cache here) the keys were cut to the strict best k and
// lost[q] holds the highest score level at which rows were dropped; with `verdict` (the last phase) the query is declared
// incomplete -- verdict[q] = 1, the caller re-runs it on the exact tile -- when the final band does not fit kc_max or reaches
// down to that level.
// One workgroup per query, so the selection work of a launch is spread over 1024 workgroups x 256 threads instead of
// being the serial tail of 256 workgroups.
//   * the keys of the query (a few hundred after a selective phase; every row of the phase after the cold first one)
//     stream ONCE through an LDS cache of SEL_CACHE keys.  Whenever the cache is nearly full it is cut down to its band,
//     and that cut -- a valid lower bound on the final one -- filters the keys that follow (expected survivors on data in
//     random order: k * remaining / seen), so the exact selection always runs on a few thousand keys held in registers.
//   * exact selection of the k-th best = bisection on the bit pattern of the score (scores are in [0, 1]: the patterns order
//     like the floats), block-wide counts per bit, only on the bits in which the keys differ; in the strict (overflow) form
//     ties at the k-th best score are cut the same way on the ordinal half (smaller ordinal wins): exactly min(k, total) keys.
//   * output: the band's keys, UNSORTED, + their count; thr = just below the band cut (or the caller's floor).
// ---------------------------------------------------------------------------------------------
constexpr int SEL_CACHE = 4096;  // keys of a query held in LDS (32 KiB: four workgroups per CU, so the 1024 queries of a batch are all resident at
                                 // once -- the streaming is latency-bound; 8192 keys / two workgroups per CU: 0.53 ms per cfg3 batch instead of 0.29)
constexpr int SEL_PER = SEL_CACHE / 256;

__global__ void __launch_bounds__(256) select_band_kernel(const u64* __restrict__ cand, const int* __restrict__ counts, int n_splits, int nq_padded, int k,
                                                          int kc_max, const u64* __restrict__ carried, const int* __restrict__ carried_cnt,
                                                          const float* __restrict__ floor, const float* __restrict__ band, u64* __restrict__ out,
                                                          int* __restrict__ out_cnt, float* __restrict__ thr_out, unsigned* __restrict__ lost,
                                                          int* __restrict__ verdict, const int* __restrict__ active, int active_min, int active_max,
                                                          const int* __restrict__ gate, int gate_max, int* __restrict__ doomed, int doom_limit) {
  if (gate != nullptr && *gate > gate_max) return;  // the tile launch in front of this one was skipped too (see MfmaDeviceParams::gate)
  if (active != nullptr) {  // fixed-shape launch over a device-side work list: slots past it (or a list that is not this fallback's share) have no buffers
    const int live = *active;
    if (live <= active_min || live > active_max || (int)blockIdx.x >= live) return;
  }
  extern __shared__ __align__(16) unsigned char sel_smem[];
  u64* cache = reinterpret_cast<u64*>(sel_smem);  // [SEL_CACHE]
  __shared__ int off[260];  // exclusive prefix of the per-split counts (+ the carried band as one more "split")
  __shared__ float red[4];
  __shared__ int n_picked, n_cached;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;
  const int n_src = n_splits + (carried != nullptr ? 1 : 0);  // <= 257
  const float band_q = band ? band[q] : 0.0f;

  auto block_sum = [&](int v) -> int {  // exact: counts stay far below 2^24
    const float w = wave_sum((float)v);
    if (lane == 0) red[wave] = w;
    __syncthreads();
    const int total = (int)(red[0] + red[1] + red[2] + red[3]);
    __syncthreads();
    return total;
  };
  // ---- flat order of the query's keys: source s holds count(s) keys at flat positions off[s] .. off[s+1)
  __shared__ int cnt_of[260];
  for (int sp = tid; sp < n_src; sp += 256)  // (n_splits <= 256: one load per thread, all in flight at once)
    cnt_of[sp] = (sp < n_splits) ? counts[(size_t)sp * nq_padded + q] : carried_cnt[q];  // buffers are laid out [row range][padded query] whatever the tile width
  if (tid == 0) n_picked = 0;
  __syncthreads();
  for (int sp = tid; sp <= n_src; sp += 256) {
    int run = 0;
    for (int j = 0; j < sp; ++j) run += cnt_of[j];
    off[sp] = run;
  }
  __syncthreads();
  const int total = off[n_src];
  // the source of flat position `flat` = the last one with off[s] <= flat.  A thread's positions only grow, so on a long stream (the all-admitted
  // first ladder phase: thousands of keys per source) it walks forward from the source of its previous key -- one LDS read per key instead of a
  // binary search's seven or eight dependent ones, which is what that selection's time was made of; a short stream (a few keys per source, one
  // round) keeps the binary search.
  const bool walk = total > 2 * SEL_CACHE;
  int src_at = 0;
  auto key_at = [&](int flat) -> u64 {
    int lo = src_at;
    if (walk) {
      while (lo + 1 < n_src && off[lo + 1] <= flat) ++lo;
      src_at = lo;
    } else {
      int hi = n_src - 1;
      lo = 0;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= flat) lo = mid; else hi = mid - 1;
      }
    }
    const int i = flat - off[lo];
    if (lo == n_splits) return carried[(size_t)q * kc_max + i];
    return cand[((size_t)lo * nq_padded + q) * (size_t)CAPW + i];
  };

  u64 key[SEL_PER];
  int n_keys = 0;  // keys in the cache (block-uniform)
  auto count = [&](auto&& pred) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < SEL_PER; ++j) c += (key[j] != 0ull && pred(key[j])) ? 1 : 0;
    return block_sum(c);
  };
  // loads cache[0 .. n) into key[] and finds the exact (t_hi, t_lo): the need-th best key among them is the smallest key with score > t_hi or
  // (score == t_hi and low >= t_lo) [t_lo only when `strict`]; returns false when n < need (everything is wanted)
  auto kth_of_cache = [&](int n, int need, bool strict, uint32_t* t_hi_out, uint32_t* t_lo_out) -> bool {
#pragma unroll
    for (int j = 0; j < SEL_PER; ++j) {
      const int i = tid + 256 * j;
      key[j] = (i < n) ? cache[i] : 0ull;
    }
    if (n < need) return false;
    uint32_t mx = 0u, mn_inv = 0u;
#pragma unroll
    for (int j = 0; j < SEL_PER; ++j) {
      const uint32_t sc = (uint32_t)(key[j] >> 32);
      mx = max(mx, sc);
      if (key[j] != 0ull) mn_inv = max(mn_inv, ~sc);
    }
    mx = wave_max_u32(mx, lane);
    mn_inv = wave_max_u32(mn_inv, lane);
    if (lane == 0) red[wave] = __uint_as_float(mx);
    __syncthreads();
    mx = max(max(__float_as_uint(red[0]), __float_as_uint(red[1])), max(__float_as_uint(red[2]), __float_as_uint(red[3])));
    __syncthreads();
    if (lane == 0) red[wave] = __uint_as_float(mn_inv);
    __syncthreads();
    const uint32_t mn = ~max(max(__float_as_uint(red[0]), __float_as_uint(red[1])), max(__float_as_uint(red[2]), __float_as_uint(red[3])));
    __syncthreads();
    uint32_t t = mn;
    if (mx != mn) {
      const int top = 31 - __builtin_clz(mx ^ mn);
      t = (top == 31) ? 0u : (mx & ~((2u << top) - 1u));
      for (int b = top; b >= 0; --b) {
        const uint32_t trial = t | (1u << b);
        if (count([&](u64 kk) { return (uint32_t)(kk >> 32) >= trial; }) >= need) t = trial;
      }
    }
    uint32_t t_lo = 0u;
    if (strict) {
      const int above = count([&](u64 kk) { return (uint32_t)(kk >> 32) > t; });
      const int ties = count([&](u64 kk) { return (uint32_t)(kk >> 32) == t; });
      if (above + ties > need) {  // cut the ties by ordinal (low word: bigger = smaller ordinal)
        const int need_ties = need - above;
        for (int b = 31; b >= 0; --b) {
          const uint32_t trial = t_lo | (1u << b);
          if (count([&](u64 kk) { return (uint32_t)(kk >> 32) == t && (uint32_t)kk >= trial; }) >= need_ties) t_lo = trial;
        }
      }
    }
    *t_hi_out = t;
    *t_lo_out = t_lo;
    return true;
  };
  // the cut that goes with the k-th best of the n cached keys (which kth_of_cache leaves in key[]): the band below it, or -- when the
  // band holds more than `room` keys -- the strict best k (*was_strict; the level below which keys were dropped goes to lost_here);
  // (f_hi, f_lo): keep a key iff score > f_hi or (score == f_hi and low >= f_lo)
  uint32_t lost_here = 0u;
  auto cut_of_cache = [&](int n, int room, uint32_t* f_hi, uint32_t* f_lo, bool* was_strict) -> bool {
    uint32_t t_hi = 0u, t_lo = 0u;
    *was_strict = false;
    if (!kth_of_cache(n, k, false, &t_hi, &t_lo)) return false;
    const uint32_t cut = band_cut_bits(t_hi, band_q);
    if (count([&](u64 kk) { return (uint32_t)(kk >> 32) >= cut; }) <= room) {
      *f_hi = cut;
      *f_lo = 0u;
      return true;
    }
    *was_strict = true;
    kth_of_cache(n, k, true, &t_hi, &t_lo);
    lost_here = max(lost_here, t_hi > 0u ? t_hi : 1u);
    *f_hi = t_hi;
    *f_lo = t_lo;
    return true;
  };

  // ---- stream the keys through the cache: whenever it is nearly full, it is cut down to its band, and that cut -- a valid
  //      lower bound on the final one -- filters what comes next.  On data in random order the first cut is the only one
  //      (the filter then passes k * remaining / seen keys); adversarial orders just cut more often.
  uint32_t f_hi = 0u, f_lo = 0u;
  bool have_filter = false;
  if (tid == 0) n_cached = 0;
  __syncthreads();
  constexpr int UNR = 8;  // keys per thread per round: their loads are all in flight together (the loop is latency-bound otherwise)
  for (int base = 0; base < total; base += 256 * UNR) {
    if (n_cached > SEL_CACHE - 256 * UNR) {  // block-uniform (read after a barrier)
      const int n = n_cached;
      __syncthreads();
      bool mid_strict;
      // (room for the band a cut keeps: a quarter of the cache, or the whole band buffer when that is wider -- what is left of the cache still
      //  takes the 2048 keys of the next round)
      have_filter = cut_of_cache(n, kc_max > SEL_CACHE / 4 ? kc_max : SEL_CACHE / 4, &f_hi, &f_lo, &mid_strict);  // n >= k here
      if (tid == 0) n_cached = 0;
      __syncthreads();
#pragma unroll
      for (int j = 0; j < SEL_PER; ++j) {  // keep the band (the keys sit in this thread's registers)
        const u64 kk = key[j];
        const uint32_t hi = (uint32_t)(kk >> 32);
        if (kk != 0ull && (hi > f_hi || (hi == f_hi && (uint32_t)kk >= f_lo))) cache[atomicAdd(&n_cached, 1)] = kk;
      }
      __syncthreads();
    }
    u64 kk[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int i = base + u * 256 + tid;
      kk[u] = (i < total) ? key_at(i) : 0ull;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const uint32_t hi = (uint32_t)(kk[u] >> 32);
      const bool keep = kk[u] != 0ull && (!have_filter || hi > f_hi || (hi == f_hi && (uint32_t)kk[u] >= f_lo));
      const u64 m = __builtin_amdgcn_ballot_w64(keep);
      int wbase = 0;
      if (lane == 0 && m != 0ull) wbase = atomicAdd(&n_cached, __popcll(m));
      wbase = __builtin_amdgcn_readfirstlane(wbase);
      if (keep) cache[wbase + __popcll(m & ((1ull << lane) - 1ull))] = kk[u];
    }
    __syncthreads();
  }
  n_keys = n_cached;
  __syncthreads();
  uint32_t t_hi = 0u, t_lo = 0u;
  bool strict = false;
  const bool enough = cut_of_cache(n_keys, kc_max, &t_hi, &t_lo, &strict);  // (fewer than k keys: all of them are the band; key[] is loaded either way)
  // ---- write the band (unsorted) and its size
#pragma unroll
  for (int j = 0; j < SEL_PER; ++j) {
    const u64 kv = key[j];
    const uint32_t hi = (uint32_t)(kv >> 32);
    const bool take = kv != 0ull && (!enough || hi > t_hi || (hi == t_hi && (uint32_t)kv >= t_lo));
    if (take) {
      const int idx = atomicAdd(&n_picked, 1);
      if (idx < kc_max) out[(size_t)q * kc_max + idx] = kv;
    }
  }
  __syncthreads();
  if (tid == 0) {
    out_cnt[q] = n_picked < kc_max ? n_picked : kc_max;
    // a band over the rows seen so far that is already this full will not fit at the end (the caller extrapolates: doom_limit): counted, and the
    // launches of the last filter phase gate themselves on the count
    if (doomed != nullptr && (n_picked > doom_limit || strict)) atomicAdd(doomed, 1);  // (strict: it does not even fit now)
    uint32_t lost_all = lost_here;
    if (lost != nullptr) {
      if (lost_here != 0u) atomicMax(&lost[q], lost_here);
      lost_all = max(lost_all, lost[q]);  // (the tile kernels of this and the earlier phases are done: plain read)
    }
    // incomplete: the final band itself did not fit, or rows were dropped somewhere at a level the final band reaches (its cut is t_hi when
    // there are k keys, 0 -- everything counts -- when there are fewer)
    if (verdict != nullptr) verdict[q] = (strict || (lost_all != 0u && lost_all >= (enough ? t_hi : 0u))) ? 1 : 0;
    if (thr_out != nullptr) {
      float t = -__builtin_inff();
      if (enough && t_hi > 0u) t = __uint_as_float(t_hi - (strict ? 0u : 1u));  // strict: later rows tie-lose (score > t); band: score >= cut
      if (floor != nullptr && floor[q] > t) t = floor[q];
      thr_out[q] = t;
    }
  }
}

}  // namespace

// thr[q] = the largest float below the k-th best score of the sample pass (so that `score > thr` admits
// every row scoring >= that k-th best), or -inf when the sample did not yield k hits.
// `floor` (optional, [nq]): per-query thresholds that hold from the start (the relaxed min_score of the filter pass).
__global__ void sample_threshold_kernel(const u64* __restrict__ keys, int nq, int k, const float* __restrict__ floor, float* __restrict__ thr) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const u64 kth = keys[(size_t)q * k + (k - 1)];
  float t = -__builtin_inff();
  if (kth != 0ull) {
    const uint32_t bits = (uint32_t)(kth >> 32);
    t = bits ? __uint_as_float(bits - 1u) : -__builtin_inff();
  }
  if (floor != nullptr && floor[q] > t) t = floor[q];
  thr[q] = t;
}

hipError_t launch_sample_thresholds(const unsigned long long* keys, int nq, int k, const float* floor, float* thr, hipStream_t stream) {
  hipLaunchKernelGGL(sample_threshold_kernel, dim3((nq + 255) / 256), dim3(256), 0, stream, keys, nq, k, floor, thr);
  return hipGetLastError();
}

hipError_t launch_select_band(const unsigned long long* cand, const int* counts, int n_splits, int nq, int nq_padded, int k, int kc_max,
                              const unsigned long long* carried, const int* carried_cnt, const float* floor, const float* band, unsigned long long* out,
                              int* out_cnt, float* thr_out, unsigned* lost, int* verdict, hipStream_t stream, const int* active, int active_min,
                              int active_max, const int* gate, int gate_max, int* doomed, int doom_limit) {
  if (nq < 1 || k < 1 || k > TAVB_MAX_FUSED_K || n_splits < 1 || n_splits > 256 || nq_padded < nq || kc_max < k || kc_max > SEL_CACHE / 2 || kc_max > kBandMax) return hipErrorInvalidValue;
  constexpr int lds = SEL_CACHE * (int)sizeof(u64);
  hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(select_band_kernel), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(select_band_kernel, dim3(nq), dim3(256), lds, stream, cand, counts, n_splits, nq_padded, k, kc_max, carried, carried_cnt, floor, band,
                     out, out_cnt, thr_out, lost, verdict, active, active_min, active_max, gate, gate_max, doomed, doom_limit);
  return hipGetLastError();
}

}  // namespace tavb
