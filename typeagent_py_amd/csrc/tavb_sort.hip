// Device-wide descending sort of 64-bit keys, and the decode of sorted keys into the caller's (pinned) result arrays.  Serves the sorted
// route (tavb_search_sorted: every survivor of a query, or the best k of them for any k) and tavb_sort_keys_device.
//
// Up to `small_max` keys: ONE workgroup sorts them in LDS (bitonic, block_sort_desc) -- one launch.
// Beyond: a stable LSD radix sort, 8 bits per pass over the digit passes first_pass .. 7 (pass p = bits 8p .. 8p + 7).  A digit is
// 255 - the bits, so ascending digit order is descending key order.  The sorted route hands over keys already in DESCENDING order of
// their low 32 bits (position order, compacted without atomics), so its first_pass is 4: four passes over the score bits only.
//   digits   one launch: the histogram of every pass's digit over all keys (order-independent).
//   plan     one workgroup: a pass whose digit is the same for every key is skipped (on [min_score, 1] usually the top one or two);
//            which of the two buffers each pass reads, and which one holds the result.
//   per pass count (per-block digit counts) -> scan (one workgroup, exclusive, digit-major) -> scatter (stable: each block walks its
//            range in order, ranks a key among the lanes of its wave with the same digit by 8 ballots, and among the waves through LDS).
// The kernel boundaries are the only synchronisation between workgroups: no look-back, no spin on another workgroup's flag.
// Every launch is enqueued up front; the host reads nothing back.  Indices are 64-bit, counts per sort below 2^32.

#include "tavb_device.h"
#include "tavb_internal.h"

namespace tavb {

namespace {

constexpr int kRadix = 256;
constexpr int kSortThreads = 256;  // count / scatter workgroups: 4 waves, one key per lane per tile
constexpr int kMaxSortBlocks = 1024;

// Workspace: alt [n] keys (the second buffer) | dig [8][256] | bh [256][blocks] | plan [16]
struct SortWs {
  u64* alt;
  unsigned* dig;
  unsigned* bh;
  int* plan;  // plan[p]: buffer pass p reads (0 = keys, 1 = alt), -1 = skipped; plan[8]: buffer holding the result
};

__host__ __device__ inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

__host__ __device__ inline SortWs sort_ws(void* w, int64_t n, int blocks) {
  SortWs s;
  char* p = reinterpret_cast<char*>(w);
  s.alt = reinterpret_cast<u64*>(p);
  p += align256((size_t)n * sizeof(u64));
  s.dig = reinterpret_cast<unsigned*>(p);
  p += align256((size_t)8 * kRadix * sizeof(unsigned));
  s.bh = reinterpret_cast<unsigned*>(p);
  p += align256((size_t)kRadix * blocks * sizeof(unsigned));
  s.plan = reinterpret_cast<int*>(p);
  return s;
}

struct RadixArgs {
  u64* buf[2];
  SortWs ws;
  int64_t n, chunk;  // keys; keys per block (a multiple of kSortThreads)
  int blocks, first_pass;
};

__device__ __forceinline__ unsigned digit_of(u64 key, int pass) { return 255u - (unsigned)((key >> (8 * pass)) & 255u); }

__global__ void __launch_bounds__(kSortThreads) sort_digits_kernel(const RadixArgs a) {
  __shared__ unsigned h[8][kRadix];
  for (int i = threadIdx.x; i < 8 * kRadix; i += blockDim.x) (&h[0][0])[i] = 0u;
  __syncthreads();
  const u64* __restrict__ src = a.buf[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
    const u64 key = src[i];
    for (int p = a.first_pass; p < 8; ++p) atomicAdd(&h[p][digit_of(key, p)], 1u);
  }
  __syncthreads();
  for (int i = a.first_pass * kRadix + threadIdx.x; i < 8 * kRadix; i += blockDim.x) {
    const unsigned v = (&h[0][0])[i];
    if (v) atomicAdd(&a.ws.dig[i], v);
  }
}

__global__ void __launch_bounds__(kRadix) sort_plan_kernel(const RadixArgs a) {
  __shared__ int uniform[8];
  for (int p = 0; p < 8; ++p) {
    const int u = p < a.first_pass ? 1 : __syncthreads_or(a.ws.dig[p * kRadix + threadIdx.x] == (unsigned)a.n);
    if (threadIdx.x == 0) uniform[p] = u;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int cur = 0;
    for (int p = 0; p < 8; ++p) {
      if (uniform[p]) {
        a.ws.plan[p] = -1;
      } else {
        a.ws.plan[p] = cur;
        cur ^= 1;
      }
    }
    a.ws.plan[8] = cur;
  }
}

__global__ void __launch_bounds__(kSortThreads) radix_count_kernel(const RadixArgs a, int pass) {
  __shared__ unsigned h[kRadix];
  const int src_i = a.ws.plan[pass];
  if (src_i < 0) return;  // (uniform: every key has the same digit)
  const u64* __restrict__ src = a.buf[src_i];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * a.chunk;
  const int64_t hi = lo + a.chunk < a.n ? lo + a.chunk : a.n;
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) atomicAdd(&h[digit_of(src[i], pass)], 1u);
  __syncthreads();
  a.ws.bh[(size_t)threadIdx.x * a.blocks + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of bh [256][blocks] (digit-major: the offset of digit d in block b = keys of smaller digits + digit d in blocks < b).
// One workgroup walks it in tiles of 4096 counts, four per lane in one 16-byte load (256 x blocks is a multiple of 4): coalesced, and the
// running total of the tiles before stays in a register.
__global__ void __launch_bounds__(1024) radix_scan_kernel(const RadixArgs a, int pass) {
  __shared__ unsigned wsum[16];
  if (a.ws.plan[pass] < 0) return;
  const int m4 = kRadix * a.blocks / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint4* __restrict__ bh = reinterpret_cast<uint4*>(a.ws.bh);
  unsigned carry = 0;
  for (int base = 0; base < m4; base += 1024) {  // (block-uniform trip count)
    const int i = base + threadIdx.x;
    const uint4 v = i < m4 ? bh[i] : make_uint4(0u, 0u, 0u, 0u);
    const unsigned sum = v.x + v.y + v.z + v.w;
    unsigned inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned before = carry + inc - sum, total = 0;
    for (int w = 0; w < 16; ++w) {
      const unsigned t = wsum[w];
      before += w < wave ? t : 0u;
      total += t;
    }
    if (i < m4) bh[i] = make_uint4(before, before + v.x, before + v.x + v.y, before + v.x + v.y + v.z);
    carry += total;
    __syncthreads();  // (wsum is rewritten by the next tile)
  }
}

__global__ void __launch_bounds__(kSortThreads) radix_scatter_kernel(const RadixArgs a, int pass) {
  constexpr int W = kSortThreads / 64;
  __shared__ unsigned base[kRadix];
  __shared__ unsigned cnt[W][kRadix];
  __shared__ unsigned off[W][kRadix];
  const int src_i = a.ws.plan[pass];
  if (src_i < 0) return;
  const u64* __restrict__ src = a.buf[src_i];
  u64* __restrict__ dst = a.buf[src_i ^ 1];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  base[t] = a.ws.bh[(size_t)t * a.blocks + blockIdx.x];
  for (int w = 0; w < W; ++w) cnt[w][t] = 0u;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * a.chunk;
  const int64_t hi = lo + a.chunk < a.n ? lo + a.chunk : a.n;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t start = lo; start < hi; start += kSortThreads) {  // (block-uniform trip count)
    const int64_t i = start + t;
    const bool live = i < hi;
    const u64 key = live ? src[i] : 0ull;
    const unsigned d = digit_of(key, pass);
    unsigned long long same = __ballot(live);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const unsigned long long ones = __ballot((d >> b) & 1u);
      same &= ((d >> b) & 1u) ? ones : ~ones;
    }
    const unsigned rank = (unsigned)__popcll(same & below);
    if (live && rank == 0) cnt[wave][d] = (unsigned)__popcll(same);
    __syncthreads();
    {  // thread t: digit t -- where each wave's keys of that digit go, in wave order
      unsigned run = base[t];
      for (int w = 0; w < W; ++w) {
        const unsigned c = cnt[w][t];
        off[w][t] = run;
        cnt[w][t] = 0u;
        run += c;
      }
      base[t] = run;
    }
    __syncthreads();
    if (live) dst[off[wave][d] + rank] = key;
  }
}

__global__ void __launch_bounds__(1024) sort_small_kernel(u64* keys, int n) {
  extern __shared__ __align__(16) unsigned char smem[];
  block_sort_desc(keys, n, reinterpret_cast<u64*>(smem), keys, n);
}

// sorted keys [off, off + len) -> ordinal (position + base) and score of each, at ords / scs [0, len)
__global__ void __launch_bounds__(256) sort_decode_kernel(const u64* b0, const u64* b1, const int* which, int64_t off, int64_t len, int64_t base,
                                                          int64_t* __restrict__ ords, float* __restrict__ scs, const int32_t* __restrict__ map,
                                                          int64_t map_len) {
  const u64* __restrict__ src = (which && *which) ? b1 : b0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x) {
    const u64 key = src[off + i];
    int64_t pos = (int64_t)(0xFFFFFFFFu - (uint32_t)key);
    if (map) pos = pos < map_len ? (int64_t)map[pos] : -1 - base;  // (a position outside the list: ordinal -1, never a read past it)
    ords[i] = pos + base;
    scs[i] = __uint_as_float((uint32_t)(key >> 32));
  }
}

__global__ void __launch_bounds__(256) sort_copy_back_kernel(u64* keys, const u64* alt, const int* which, int64_t n) {
  if (*which == 0) return;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) keys[i] = alt[i];
}

void sort_shape(int64_t n, int* blocks, int64_t* chunk) {
  int64_t b = (n + 4095) / 4096;
  if (b > kMaxSortBlocks) b = kMaxSortBlocks;
  if (b < 1) b = 1;
  int64_t c = (n + b - 1) / b;
  c = (c + kSortThreads - 1) / kSortThreads * kSortThreads;
  *chunk = c;
  *blocks = (int)((n + c - 1) / c);
}

int pow2_at_least(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

int grid_for(int64_t n, int per_block) {
  const int64_t b = (n + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : b > 2048 ? 2048 : b);
}

RadixArgs radix_args(const SortJob& j) {
  RadixArgs a{};
  a.buf[0] = j.keys;
  sort_shape(j.n, &a.blocks, &a.chunk);
  a.ws = sort_ws(j.workspace, j.n, a.blocks);
  a.buf[1] = a.ws.alt;
  a.n = j.n;
  a.first_pass = j.first_pass;
  return a;
}

}  // namespace

size_t sort_workspace_bytes(int64_t n) {
  int blocks;
  int64_t chunk;
  sort_shape(n, &blocks, &chunk);
  return align256((size_t)n * sizeof(u64)) + align256((size_t)8 * kRadix * sizeof(unsigned)) + align256((size_t)kRadix * blocks * sizeof(unsigned)) +
         256;
}

hipError_t launch_sort_desc(SortJob& j, hipStream_t stream) {
  if (!j.keys || !j.workspace || j.n < 1 || j.n >= ((int64_t)1 << 32) || j.first_pass < 0 || j.first_pass > 7 || j.small_max < 0 ||
      j.small_max > kSortSmallMax)
    return hipErrorInvalidValue;
  j.multi = j.n > j.small_max;
  if (!j.multi) {
    if (j.n == 1) return hipSuccess;
    const size_t lds = (size_t)pow2_at_least((int)j.n) * sizeof(u64);
    if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(sort_small_kernel), (int)lds)) return e;
    hipLaunchKernelGGL(sort_small_kernel, dim3(1), dim3(1024), lds, stream, j.keys, (int)j.n);
    return hipGetLastError();
  }
  const RadixArgs a = radix_args(j);
  if (hipError_t e = hipMemsetAsync(a.ws.dig, 0, (size_t)8 * kRadix * sizeof(unsigned), stream)) return e;
  hipLaunchKernelGGL(sort_digits_kernel, dim3(grid_for(a.n, 8 * kSortThreads)), dim3(kSortThreads), 0, stream, a);
  hipLaunchKernelGGL(sort_plan_kernel, dim3(1), dim3(kRadix), 0, stream, a);
  for (int p = a.first_pass; p < 8; ++p) {
    hipLaunchKernelGGL(radix_count_kernel, dim3(a.blocks), dim3(kSortThreads), 0, stream, a, p);
    hipLaunchKernelGGL(radix_scan_kernel, dim3(1), dim3(1024), 0, stream, a, p);
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(a.blocks), dim3(kSortThreads), 0, stream, a, p);
  }
  return hipGetLastError();
}

hipError_t launch_sort_decode(const SortJob& j, int64_t off, int64_t len, int64_t base, int64_t* ords, float* scs, hipStream_t stream, const int32_t* map,
                              int64_t map_len) {
  if (off < 0 || len < 1 || off + len > j.n || !ords || !scs) return hipErrorInvalidValue;
  const u64* alt = j.keys;
  const int* which = nullptr;
  if (j.multi) {
    const RadixArgs a = radix_args(j);
    alt = a.ws.alt;
    which = a.ws.plan + 8;
  }
  hipLaunchKernelGGL(sort_decode_kernel, dim3(grid_for(len, 4 * 256)), dim3(256), 0, stream, j.keys, alt, which, off, len, base, ords, scs, map, map_len);
  return hipGetLastError();
}

hipError_t launch_sort_copy_back(const SortJob& j, hipStream_t stream) {
  if (!j.multi) return hipSuccess;
  const RadixArgs a = radix_args(j);
  hipLaunchKernelGGL(sort_copy_back_kernel, dim3(grid_for(j.n, 4 * 256)), dim3(256), 0, stream, j.keys, a.ws.alt, a.ws.plan + 8, j.n);
  return hipGetLastError();
}

}  // namespace tavb
