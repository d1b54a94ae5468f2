// Rows of the corpus as queries (tavb_search_rows and its twins, tavb_lookup_rows.hip): the step in front of a lookup -- corpus rows named by
// a position list -> a dense float32 query batch -- and the step behind it -- the query's own row taken out of its list of k + 1 keys.
//   rows_to_queries_kernel  one wave per row, grid-stride.  fp16 rows are widened ((float)h: exact), fp32 rows copied: the batch holds, bit for
//                           bit, the values the kernels multiply when they read those rows.  16-byte loads and stores when a row is a
//                           multiple of 16 bytes and both arrays are 16-byte aligned, element by element otherwise.  A position outside
//                           [0, rows) (the entry points have checked, or the caller guarantees: never taken) gives a row of zeros.
//   drop_self_kernel        one wave per query.  in [n][k + 1]: sorted (score descending, ordinal ascending), zero-padded keys carrying
//                           index_base + row; the query's own key -- ordinal index_base + positions[q] -- is found by a ballot over the
//                           list, 64 slots at a time, and lane l copies slot s + (s >= self slot) to slot s of out [n][k].  The k + 1 best of
//                           all rows hold the k best of the others: with the own key in the list the rest ARE those, without it (more than
//                           k equal rows in front of it, a row that is not its own best match, an own score below the threshold) the first k
//                           are.  The padding stays zero (the list's zeros move up).  counts [n] (optional): keys left per query.
//                           k1 == k (lists of k keys, in == out allowed): nothing is looked for or moved, only the counts are written.
// No workgroup waits for another; vector stores only.

#include <algorithm>

#include "tavb_device.h"
#include "tavb_internal.h"

namespace tavb {
namespace {

constexpr int kRowsQueryWaves = 4;  // waves per workgroup of both kernels
constexpr int kRowsQueryThreads = kRowsQueryWaves * kWave;

template <typename T>
__global__ void __launch_bounds__(kRowsQueryThreads) rows_to_queries_kernel(const T* __restrict__ corpus, int64_t rows, int dim,
                                                                            const int32_t* __restrict__ positions, int64_t n,
                                                                            float* __restrict__ out) {
  constexpr bool kF32 = sizeof(T) == 4;
  constexpr int G = kF32 ? 4 : 8;  // elements of one 16-byte load
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * kRowsQueryWaves + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * kRowsQueryWaves;
  const bool whole = dim % G == 0 && ((uintptr_t)corpus | (uintptr_t)out) % 16 == 0;  // (rows and batch rows are then 16-byte multiples)
  for (int64_t j = wave; j < n; j += n_waves) {  // (wave-uniform)
    const int64_t p = positions[j];
    float* y = out + j * (int64_t)dim;
    if (p < 0 || p >= rows) {
      for (int i = lane; i < dim; i += 64) y[i] = 0.0f;
      continue;
    }
    const T* x = corpus + p * (int64_t)dim;
    if (whole) {
      for (int i0 = lane * G; i0 < dim; i0 += 64 * G) {
        if constexpr (kF32) {
          *reinterpret_cast<f32x4*>(y + i0) = *reinterpret_cast<const f32x4*>(x + i0);
        } else {
          const f16x8 h = *reinterpret_cast<const f16x8*>(x + i0);
          *reinterpret_cast<f32x4*>(y + i0) = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
          *reinterpret_cast<f32x4*>(y + i0 + 4) = f32x4{(float)h[4], (float)h[5], (float)h[6], (float)h[7]};
        }
      }
    } else {
      for (int i = lane; i < dim; i += 64) y[i] = (float)x[i];
    }
  }
}

__global__ void __launch_bounds__(kRowsQueryThreads) drop_self_kernel(const u64* in, int k1, const int32_t* __restrict__ positions, uint32_t index_base,
                                                                      int64_t n, int k, u64* out, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * kRowsQueryWaves + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * kRowsQueryWaves;
  for (int64_t q = wave; q < n; q += n_waves) {  // (wave-uniform)
    const u64* list = in + q * (int64_t)k1;
    const uint32_t own = 0xFFFFFFFFu - (index_base + (uint32_t)positions[q]);  // the low word of the query's own key
    int self_slot = k1;  // not in the list: nothing moves
    for (int s0 = 0; s0 < k1 && k1 > k; s0 += 64) {
      const int s = s0 + lane;
      const u64 key = s < k1 ? list[s] : 0ull;
      const u64 hit = __ballot(key != 0ull && (uint32_t)key == own);
      if (hit != 0ull) {
        self_slot = s0 + __builtin_ctzll(hit);
        break;
      }
      if (__ballot(s < k1 && key == 0ull) != 0ull) break;  // sorted, zero-padded: nothing behind the first empty slot
    }
    u64* o = out + q * (int64_t)k;
    int left = 0;
    for (int s0 = 0; s0 < k; s0 += 64) {
      const int s = s0 + lane;
      u64 key = 0ull;
      if (s < k) {
        key = list[s + (s >= self_slot ? 1 : 0)];  // (s + 1 <= k: inside the k + 1 slots)
        if (o != list) o[s] = key;
      }
      left += __popcll(__ballot(key != 0ull));
    }
    if (counts != nullptr && lane == 0) counts[q] = left;
  }
}

unsigned rows_query_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + kRowsQueryWaves - 1) / kRowsQueryWaves, 256 * 8); }

}  // namespace

hipError_t launch_rows_to_queries(const void* corpus, bool f16, int64_t rows, int dim, const int32_t* positions, int64_t n, float* out, hipStream_t stream) {
  if (!corpus || !positions || !out || rows < 1 || dim < 1 || n < 1) return hipErrorInvalidValue;
  if (f16)
    hipLaunchKernelGGL(rows_to_queries_kernel<_Float16>, dim3(rows_query_blocks(n)), dim3(kRowsQueryThreads), 0, stream, reinterpret_cast<const _Float16*>(corpus),
                       rows, dim, positions, n, out);
  else
    hipLaunchKernelGGL(rows_to_queries_kernel<float>, dim3(rows_query_blocks(n)), dim3(kRowsQueryThreads), 0, stream, reinterpret_cast<const float*>(corpus), rows,
                       dim, positions, n, out);
  return hipGetLastError();
}

hipError_t launch_drop_self(const unsigned long long* in, bool with_self, const int32_t* positions, uint32_t index_base, int64_t n, int k,
                            unsigned long long* out, int32_t* counts, hipStream_t stream) {
  if (!in || !positions || !out || n < 1 || k < 1 || k + (with_self ? 1 : 0) > TAVB_MAX_LARGE_K || (with_self && in == out)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(drop_self_kernel, dim3(rows_query_blocks(n)), dim3(kRowsQueryThreads), 0, stream, in, with_self ? k + 1 : k, positions, index_base, n, k, out,
                     counts);
  return hipGetLastError();
}

}  // namespace tavb
