// Device-side pieces shared by the tile kernels' three translation units -- tavb_mfma_wide.hip (the 128/256-query filter tile),
// tavb_mfma_skinny.hip (the 32/64-query tile) and tavb_select.hip (the band selection) -- and included by nothing else: the parameter
// block of a tile launch and its one filler, the constants the families share, the LDS / wait-count primitives that go behind the
// compiler's back, and the compaction of a candidate buffer.
#pragma once

#include <hip/hip_runtime.h>

#include "tavb_device.h"
#include "tavb_internal.h"

namespace tavb {

namespace {

constexpr int BM = 256;   // corpus rows per tile of the 32/64-query kernel
constexpr int BN = 256;   // queries per tile of the 256-query kernel
constexpr int BK = 64;    // dim must be a multiple of this
constexpr int CAP = 512;    // candidate keys per (workgroup, query) of the 32/64-query tile; must be >= BM + max k
constexpr int CAPW = 1024;  // ... of the 256-query tile: three 320-row tiles fit before the first compaction, so a short first
                            // ladder phase (<= 2 tiles per workgroup) never compacts at all

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void global_void;
typedef __attribute__((address_space(3))) volatile int lds_flag;  // (LDS-typed: through a generic pointer the read is a FLAT load, see skinny_scan_kernel)

constexpr int BM6 = 320;   // corpus rows per tile of the 128/256-query kernel
constexpr int NT6 = 256;   // ... and its threads

struct MfmaDeviceParams {
  const _Float16* corpus;
  const _Float16* queries;  // [nq_padded, dim]
  u64* cand;                // [blocks][queries per tile][CAP or CAPW]
  int* counts;              // 256-query tile: [blocks][BN] keys left in each candidate buffer when the launch ends
  u64* lists;               // [nq][n_splits][k]
  int64_t rows;
  int64_t rows_per_split;   // multiple of BM
  int32_t dim;
  int32_t nq;
  int32_t n_qtiles;
  int32_t n_splits;
  int32_t list_stride;      // lists per query in `lists` (>= n_splits; extra slots belong to the caller)
  int32_t k;
  uint32_t index_base;
  float min_score;
  const float* thr_in;  // optional [nq_padded] admission thresholds from a sample pass (exclusive bound)
  const int* active;    // optional: number of live queries, read on the device; query tiles past it return at once
  int32_t active_min;   // ... and the launch as a whole returns at once unless active_min < *active <= active_max (two fallbacks share one work list)
  int32_t active_max;
  int64_t split_plane;  // 256-query tile, SPLIT form: bytes from the high to the low plane of the queries ([2][nq_padded][dim] fp16); 0 otherwise
  const int* gate;      // optional device-side counter: the whole launch returns at once when *gate > gate_max (a filter phase of a batch already known to need
  int32_t gate_max;     // the exact form: tavb_route.hip::run_tile_ladder)
  const float* band;    // 128/256-query tile, optional [nq_padded]: keep every key within band[q] below the k-th best (band selection)
  unsigned* lost;       // ... [nq_padded]: atomicMax of the score bits below which a query LOST band rows (a band that did not fit a buffer)
};

// Pin a wave-uniform pointer into SGPRs.  Without this the compiler strength-reduces the eight
// LDS-DMA source addresses of a K step into eight 64-bit VGPR induction variables (16 VGPRs, spilled
// in this kernel); with it each address is "SGPR base + 32-bit VGPR offset" (the saddr form).
__device__ __forceinline__ const char* sgpr_ptr(const char* p) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return reinterpret_cast<const char*>(((unsigned long long)hi << 32) | lo);
}

// LDS read-modify-write / store that the compiler cannot see as LDS traffic.  hipcc's wait-count pass orders every LDS
// write or atomic behind all in-flight LDS-DMA (`s_waitcnt vmcnt(0)`): it cannot tell that the fill counters and flags
// never alias the operand rings.  In these kernels that wait sits in the admission slow path and drains up to twenty
// 1 KiB loads (1-2 us) every time a 32 x 32 block admits a row.
__device__ __forceinline__ int lds_add_rtn(int* counter, int v) {
  const uint32_t addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) int*)counter;
  int old;
  asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(old) : "v"(addr), "v"(v) : "memory");
  return old;
}
__device__ __forceinline__ void lds_store_i32(__attribute__((address_space(3))) volatile int* flag, int v) {
  const uint32_t addr = (uint32_t)(uintptr_t)flag;
  asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_store_i32(volatile int* flag, int v) {
  lds_store_i32((__attribute__((address_space(3))) volatile int*)flag, v);
}

#define TAVB_SB() __builtin_amdgcn_sched_barrier(0)
#define TAVB_BARRIER()            \
  do {                            \
    TAVB_SB();                    \
    __builtin_amdgcn_s_barrier(); \
    TAVB_SB();                    \
  } while (0)

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Reduce one query's candidate buffer (n unsorted keys) to its best 64, sorted best-first and
// spread over the lanes (rank r in lane r).  One wave; wave-uniform arguments.
__device__ __forceinline__ WaveTopK<1> best_of_buffer(const u64* buf, int n, int lane) {
  WaveTopK<1> best;
  best.clear();
  for (int off = 0; off < n; off += 64) {
    const u64 key = (off + lane < n) ? buf[off + lane] : 0ull;
    WaveTopK<1> chunk;
    chunk.key[0] = sort64_ascending(key, lane);  // ascending == "reversed best-first"
    best.merge_reversed(chunk, lane);
  }
  return best;
}

// Compaction of one query's candidate buffer (n <= CAPACITY unsorted keys) to the keys that can still make the top k:
// everything at or above the k-th best key.  No sort: the k-th best SCORE is found by bisection on its bit pattern
// (scores are in [0, 1]: the patterns order like the floats) -- one ballot per 64 keys per bit, on the bits below the
// highest bit in which the buffer's scores differ (~20 of them) -- and the survivors are packed to the front with ballot
// prefix sums.  When more than k + 32 keys tie at that score (duplicate rows), the same bisection on the ordinal half of
// the key cuts the ties exactly (smaller ordinal wins), so a buffer always shrinks to about k and cannot overflow.
// ~5x cheaper than sorting 64-key chunks and merging them (the cold start of a launch compacts every buffer of the
// workgroup after its first tile).  One wave; wave-uniform arguments; returns the number of keys kept.
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v, int lane) {
  v = max(v, (uint32_t)xor_lane_i32<1>((int)v, lane));
  v = max(v, (uint32_t)xor_lane_i32<2>((int)v, lane));
  v = max(v, (uint32_t)xor_lane_i32<4>((int)v, lane));
  v = max(v, (uint32_t)xor_lane_i32<8>((int)v, lane));
  v = max(v, (uint32_t)xor_lane_i32<16>((int)v, lane));
  v = max(v, (uint32_t)xor_lane_i32<32>((int)v, lane));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// Score bits of the BAND cut that goes with a k-th best score `t_bits`: a key is kept when its score bits are >= the result.
// cut = t - band, rounded DOWN one more ulp (the subtraction rounds to nearest); 0 = keep everything (band wider than the score,
// or infinite: nothing can be ruled out).
__device__ __forceinline__ uint32_t band_cut_bits(uint32_t t_bits, float band) {
  const float c = __uint_as_float(t_bits) - band;
  if (!(c > 0.0f)) return 0u;
  const uint32_t b = __float_as_uint(c);
  return b > 0u ? b - 1u : 0u;
}

// Band compaction of one query's candidate buffer (the 128/256-query tile as an exact FILTER, tavb_rescore.hip): keep every key
// whose score is within `band` (= 2 delta_q, the filter's rigorous error bound both ways) of the k-th best score of the buffer --
// all of them, not a fixed number -- because exactly those rows can still be among the query's exact top k.  On ordinary data
// that is k + a handful; on clustered data (near-duplicate rows around rank k) it is the cluster, whatever its size, as long as
// it fits: when more than `limit` keys would stay, the buffer is cut to its strict best k (by key: smaller ordinal wins ties)
// and *lost_bits = the score bits of that k-th best: rows scoring <= it were (and, through the raised threshold, will be) dropped
// although they may lie inside the band.  That only matters if the query's FINAL band reaches down to that level -- the select
// kernel compares (a big cluster of near-duplicates inside one row range overflows the buffers of every query whose local k-th
// best is below the cluster's score, but it is irrelevant to all those whose final k-th best is far above it).
// Returns the number of keys kept; *thr_excl = the exclusive admission bound that goes with the cut (score > *thr_excl), or
// -inf when everything qualifies; *lost_bits = 0 when nothing was lost.  One wave; wave-uniform arguments.
// Both compactions are this one function: BAND = false is the compaction to the k-th best described above (the 32/64-query tile: *thr = the
// k-th best score, -1 when n <= k; band, limit and lost_bits unused), BAND = true the band compaction (*thr = the exclusive admission bound).
// They share the key load, the bisection, the tie cut and the pack loop; only the cut between them differs.  The kernels call it directly:
// behind one more forwarding function the same text compiles to different (equivalent) code in every kernel (profiles/r11_tile_split.md).
template <int CAPACITY, bool BAND>
__device__ __forceinline__ int compact_buffer(u64* buf, int n, int k, int lane, float band, int limit, float* thr, uint32_t* lost_bits) {
  constexpr int PER = CAPACITY / 64;
  u64 key[PER];
  uint32_t sc[PER];
  uint32_t mx = 0u, mn_inv = 0u;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int idx = j * 64 + lane;
    key[j] = (idx < n) ? buf[idx] : 0ull;
    sc[j] = (uint32_t)(key[j] >> 32);
    mx = max(mx, sc[j]);
    if (key[j] != 0ull) mn_inv = max(mn_inv, ~sc[j]);
  }
  if constexpr (BAND) {
    *lost_bits = 0u;
    *thr = -__builtin_inff();
    if (n <= k) return n;
  } else {
    if (n <= k) {
      *thr = -1.0f;
      return n;
    }
  }
  mx = wave_max_u32(mx, lane);
  const uint32_t mn = ~wave_max_u32(mn_inv, lane);
  auto count_ge = [&](uint32_t t) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) c += __popcll(__builtin_amdgcn_ballot_w64(key[j] != 0ull && sc[j] >= t));
    return c;
  };
  uint32_t t = mn;  // every key is >= mn: count = n > k
  if (mx != mn) {
    const int top = 31 - __builtin_clz(mx ^ mn);
    t = (top == 31) ? 0u : (mx & ~((2u << top) - 1u));  // the common leading bits
    for (int b = top; b >= 0; --b) {
      const uint32_t trial = t | (1u << b);
      if (count_ge(trial) >= k) t = trial;
    }
  }
  // t = the k-th best score
  uint32_t cut = t;
  if constexpr (BAND) cut = band_cut_bits(t, band);
  uint32_t t_lo = 0u;
  bool strict = !BAND;
  if (!BAND || count_ge(cut) > limit) {  // BAND: the band does not fit -- strict best k (ties at t cut by ordinal, the low word: bigger = smaller ordinal)
    if constexpr (BAND) {
      strict = true;
      *lost_bits = t > 0u ? t : 1u;
      cut = t;
    }
    int above = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) above += __popcll(__builtin_amdgcn_ballot_w64(key[j] != 0ull && sc[j] > t));
    if (count_ge(t) > k + 32) {
      const int need = k - above;  // >= 1 of the tied keys are still needed
      for (int b = 31; b >= 0; --b) {
        const uint32_t trial = t_lo | (1u << b);
        int c = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) c += __popcll(__builtin_amdgcn_ballot_w64(sc[j] == t && key[j] != 0ull && (uint32_t)key[j] >= trial));
        if (c >= need) t_lo = trial;
      }
    }
  }
  int base = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const bool keep = key[j] != 0ull && (sc[j] > cut || (sc[j] == cut && (uint32_t)key[j] >= t_lo));
    const u64 m = __builtin_amdgcn_ballot_w64(keep);
    const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
    if (keep) buf[pos] = key[j];
    base += __popcll(m);
  }
  // BAND: rows that come later in this row range have bigger ordinals than everything kept: at a strict cut a tie at t loses (score > t);
  // at a band cut every score >= cut stays welcome (score > the float just below cut)
  if constexpr (BAND)
    *thr = strict ? __uint_as_float(t) : (cut > 0u ? __uint_as_float(cut - 1u) : -__builtin_inff());
  else
    *thr = __uint_as_float(t);
  return base;
}

// The fields of a tile launch that both families set the same way; `tile` = queries per tile, `rows_per_tile` = corpus rows per tile (a row
// range is a whole number of tiles).  What only one family uses (counts, band, lost, the split plane, the gate) stays with its launcher.
inline MfmaDeviceParams fill_device_params(const MfmaParams& p, int tile, int rows_per_tile) {
  MfmaDeviceParams d{};
  d.corpus = reinterpret_cast<const _Float16*>(p.corpus);
  d.queries = reinterpret_cast<const _Float16*>(p.queries);
  d.cand = p.workspace;
  d.lists = p.lists;
  d.rows = p.rows;
  d.dim = p.dim;
  d.nq = p.nq;
  d.n_qtiles = p.nq_padded / tile;
  d.n_splits = p.n_splits;
  d.list_stride = p.list_stride > p.n_splits ? p.list_stride : p.n_splits;
  d.k = p.k;
  d.index_base = p.index_base;
  d.min_score = p.min_score;
  d.thr_in = p.thr_in;
  d.active = p.active;
  d.active_min = p.active_min;
  d.active_max = p.active_max > 0 ? p.active_max : 0x7fffffff;
  const int64_t per = (p.rows + p.n_splits - 1) / p.n_splits;
  d.rows_per_split = ((per + rows_per_tile - 1) / rows_per_tile) * rows_per_tile;
  return d;
}

}  // namespace

}  // namespace tavb
