// Row masks (tavb_mask_expand, tavb_mask_pack, tavb_mask_from_messages): an allow-mask of one bit per corpus row -> the int32 row list the
// subset lookups gather by, in ascending row order, without a trip to the host; and the mask of a SCOPE -- a set of message ordinals -- built
// from the row -> message map on the device (mask_from_messages_kernel), so that a scoped message lookup never makes a host row list.
// Scope algebra (tavb_mask_from_ranges, tavb_mask_combine): the mask of a scope of range collections (mask_from_ranges_kernel) and AND /
// OR / ANDNOT of masks (mask_combine_kernel), both of which also leave the counts mask_write_kernel needs and the mask's count and span.
// Row compaction (tavb_compact_rows): the rows a mask names are removed and the others moved down, by the same per-chunk counts (further down).
// Masks carried through such an edit (tavb_mask_remap): packed masks squeezed or spread under the edit's flags, by the same counts again.
//
// The mask is uint32 words, row r = bit (r & 31) of word (r >> 5).  Two launches, both grids fixed on the host:
//   mask_count_kernel   workgroup b popcounts its kMaskWordsPerBlock words -> counts[b]
//   mask_write_kernel   workgroup b starts at the sum of the counts before it (as sorted_compact_kernel in tavb_topk.hip does); a lane
//                       takes one word, an inclusive scan of the popcounts over the wave (cross-lane shuffles) and the waves' totals
//                       through LDS give the lane's first slot, and the lane writes the rows of its set bits from there.
// N / 8 bytes read twice, 4 bytes written per set row, no atomics on the output order: the list is deterministic and ascending, which
// is what keeps "equal scores order by ascending ordinal" once the keys carry list positions.

#include <algorithm>

#include "tavb_device.h"
#include "tavb_internal.h"
#include "tavb_remap_bits.h"

namespace tavb {

namespace {

constexpr int kMaskThreads = 256;
constexpr int kMaskWordsPerBlock = TAVB_MASK_ROWS_PER_WORKGROUP / 32;
static_assert(kMaskWordsPerBlock % kMaskThreads == 0, "a workgroup takes its words in whole rounds of its threads");

// word w of the mask with the bits at or beyond `rows` cleared (they may hold anything); 0 past the last word
__device__ __forceinline__ uint32_t mask_word(const uint32_t* __restrict__ bits, int64_t w, int64_t n_words, int64_t rows) {
  if (w >= n_words) return 0u;
  uint32_t v = bits[w];
  const int tail = (int)(rows & 31);
  if (w == n_words - 1 && tail != 0) v &= (1u << tail) - 1u;
  return v;
}

__global__ void __launch_bounds__(kMaskThreads) mask_count_kernel(const uint32_t* __restrict__ bits, int64_t rows, int64_t n_words,
                                                                  unsigned* __restrict__ counts) {
  __shared__ unsigned wc[kMaskThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w0 = (int64_t)blockIdx.x * kMaskWordsPerBlock;
  unsigned n = 0;
  for (int i = threadIdx.x; i < kMaskWordsPerBlock; i += kMaskThreads) n += (unsigned)__popc(mask_word(bits, w0 + i, n_words, rows));
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_down(n, d, 64);
  if (lane == 0) wc[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned all = 0;
    for (int w = 0; w < kMaskThreads / 64; ++w) all += wc[w];
    counts[blockIdx.x] = all;
  }
}

// out [0 .. min(total, cap)) = the set rows in ascending order; *total_out = total (written by the last workgroup; device-writable memory).
// cap == 0: only the total, from the counts.
__global__ void __launch_bounds__(kMaskThreads) mask_write_kernel(const uint32_t* __restrict__ bits, int64_t rows, int64_t n_words,
                                                                  const unsigned* __restrict__ counts, int32_t* __restrict__ out, int64_t cap,
                                                                  long long* __restrict__ total_out) {
  __shared__ unsigned start_sh;
  __shared__ unsigned wc[kMaskThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) start_sh = 0u;
  __syncthreads();
  {  // where this workgroup's rows start: the counts of the workgroups before it
    unsigned part = 0;
    for (unsigned b = threadIdx.x; b < blockIdx.x; b += kMaskThreads) part += counts[b];
    if (part) atomicAdd(&start_sh, part);
  }
  __syncthreads();
  unsigned base = start_sh;
  if (cap == 0) {  // the count alone (block-uniform): nothing to write, the mask is not read again
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total_out = (long long)base + counts[blockIdx.x];
    return;
  }
  const int64_t w0 = (int64_t)blockIdx.x * kMaskWordsPerBlock;
  for (int i = 0; i < kMaskWordsPerBlock; i += kMaskThreads) {  // (block-uniform trip count)
    const int64_t w = w0 + i + threadIdx.x;
    uint32_t v = mask_word(bits, w, n_words, rows);
    const unsigned mine = (unsigned)__popc(v);
    unsigned incl = mine;  // inclusive scan over the wave
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wc[wave] = incl;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int x = 0; x < kMaskThreads / 64; ++x) {
      before += x < wave ? wc[x] : 0u;
      all += wc[x];
    }
    int64_t slot = (int64_t)base + before + (incl - mine);
    const int32_t row0 = (int32_t)(w << 5);  // (w < n_words <= 2^26 wherever v != 0)
    while (v) {
      const int bit = __ffs((int)v) - 1;
      if (slot < cap) out[slot] = row0 + bit;
      ++slot;
      v &= v - 1u;
    }
    base += all;
    __syncthreads();  // wc is rewritten by the next round
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total_out = (long long)base;
}

// bytes [rows] (non-zero = allowed: a torch.bool tensor) -> mask words: a wave takes 64 rows per round, one byte per lane, and its ballot IS
// the two words
__global__ void __launch_bounds__(kMaskThreads) mask_pack_kernel(const uint8_t* __restrict__ bytes, int64_t rows, int64_t n_words,
                                                                 uint32_t* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * kMaskThreads + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * kMaskThreads) >> 6;
  const int64_t groups = (rows + 63) >> 6;
  for (int64_t g = wave; g < groups; g += n_waves) {  // (wave-uniform trip count)
    const int64_t r = (g << 6) + lane;
    const bool on = r < rows && bytes[r] != 0;
    const unsigned long long m = __ballot(on);
    const int64_t w = (g << 1) + lane;
    if (lane < 2 && w < n_words) bits[w] = (uint32_t)(m >> (32 * lane));
  }
}

// The mask of a scope: row r is set when its message (row_to_msg[r]; -1 = none) has its bit in the accept bitmap (accept_bitmap_kernel's
// words, n_bits message ordinals).  A wave takes 64 rows per round, one entry of the map per lane (coalesced), and its ballot IS the two
// words: every word of (rows + 31) / 32 is written, the bits at or beyond `rows` as zeros (their lanes vote no).  No atomics.
__global__ void __launch_bounds__(kMaskThreads) mask_from_messages_kernel(const int32_t* __restrict__ row_to_msg, int64_t rows,
                                                                          const uint32_t* __restrict__ accept_bits, int64_t n_bits,
                                                                          uint32_t* __restrict__ bits_out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * kMaskThreads + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * kMaskThreads) >> 6;
  const int64_t n_words = (rows + 31) >> 5;
  const int64_t groups = (rows + 63) >> 6;
  for (int64_t g = wave; g < groups; g += n_waves) {  // (wave-uniform trip count)
    const int64_t r = (g << 6) + lane;
    bool on = false;
    if (r < rows) {
      const int64_t m = row_to_msg[r];
      if (m >= 0 && m < n_bits) on = ((accept_bits[m >> 5] >> (m & 31)) & 1u) != 0u;
    }
    const unsigned long long v = __ballot(on);
    const int64_t w = (g << 1) + lane;
    if (lane < 2 && w < n_words) bits_out[w] = (uint32_t)(v >> (32 * lane));
  }
}

// ---- scope algebra: a mask from ranges, and AND / OR / ANDNOT of masks.  Unlike the two kernels above, a WORKGROUP here owns one chunk of
// TAVB_MASK_ROWS_PER_WORKGROUP rows (mask_count_kernel's chunk), so that it can leave that chunk's popcount where mask_write_kernel reads it
// and the chunk's count, first and last set row where the host sums them: no count pass, no read-back of the row list's ends.

constexpr int kMaskWaves = kMaskThreads / 64;
constexpr int kMaskRoundsPerBlock = TAVB_MASK_ROWS_PER_WORKGROUP / 64;
static_assert(kMaskRoundsPerBlock % kMaskWaves == 0, "a workgroup's waves take its rounds of 64 rows in turn");

// (n, first, last) of every wave (lane 0 holds them) -> counts[chunk], info[chunk]; every thread of the workgroup calls it
__device__ __forceinline__ void mask_chunk_reduce(unsigned n, int first, int last, unsigned* __restrict__ counts, MaskChunkInfo* __restrict__ info) {
  __shared__ unsigned wn[kMaskWaves];
  __shared__ int wf[kMaskWaves], wl[kMaskWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    wn[wave] = n;
    wf[wave] = first;
    wl[wave] = last;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    MaskChunkInfo ci{0u, 0x7FFFFFFF, -1};
    for (int w = 0; w < kMaskWaves; ++w) {
      ci.count += wn[w];
      ci.first = min(ci.first, wf[w]);
      ci.last = max(ci.last, wl[w]);
    }
    counts[blockIdx.x] = ci.count;
    info[blockIdx.x] = ci;
  }
}

// The mask of a scope of ranges.  Row r votes yes when x (r itself, or its message: 0 <= row_to_msg[r] < n_messages) lies in an interval of
// EVERY collection: one binary search per collection over that collection's disjoint ascending {start, end} pairs (the last start <= x,
// then x < its end).  kLds: the workgroup first copies all intervals (at most TAVB_SCOPE_LDS_RANGES) into LDS and searches there.  A wave
// takes 64 rows per round and its ballot IS the two words, as above; the ballots' popcounts, lowest and highest bits are the chunk's info.
template <bool kLds>
__global__ void __launch_bounds__(kMaskThreads) mask_from_ranges_kernel(const int2* __restrict__ intervals, ScopeCollections cols,
                                                                        const int32_t* __restrict__ row_to_msg, int64_t n_messages, int64_t rows,
                                                                        int64_t n_words, uint32_t* __restrict__ bits_out,
                                                                        unsigned* __restrict__ counts, MaskChunkInfo* __restrict__ info) {
  __shared__ int2 staged[kLds ? TAVB_SCOPE_LDS_RANGES : 1];
  if (kLds) {
    const int total = min(cols.offset[cols.n], TAVB_SCOPE_LDS_RANGES);
    for (int i = threadIdx.x; i < total; i += kMaskThreads) staged[i] = intervals[i];
    __syncthreads();
  }
  auto at = [&](int i) -> int2 {
    if constexpr (kLds) return staged[i];
    else return intervals[i];
  };
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g0 = (int64_t)blockIdx.x * kMaskRoundsPerBlock;
  const int64_t groups = (rows + 63) >> 6;
  unsigned n = 0;
  int first = 0x7FFFFFFF, last = -1;
  for (int i = wave; i < kMaskRoundsPerBlock; i += kMaskWaves) {  // (wave-uniform trip count)
    const int64_t g = g0 + i;
    if (g >= groups) break;
    const int64_t r = (g << 6) + lane;
    bool on = false;
    if (r < rows) {
      int64_t x = r;
      on = true;
      if (row_to_msg) {
        x = row_to_msg[r];
        on = x >= 0 && x < n_messages;
      }
      for (int c = 0; c < cols.n && on; ++c) {
        const int begin = cols.offset[c];
        int lo = begin, hi = cols.offset[c + 1];
        while (lo < hi) {  // the number of intervals that start at or before x
          const int mid = (lo + hi) >> 1;
          if ((int64_t)at(mid).x <= x) lo = mid + 1;
          else hi = mid;
        }
        on = lo > begin && x < (int64_t)at(lo - 1).y;
      }
    }
    const unsigned long long v = __ballot(on);
    const int64_t w = (g << 1) + lane;
    if (lane < 2 && w < n_words) bits_out[w] = (uint32_t)(v >> (32 * lane));
    if (v) {
      n += (unsigned)__popcll(v);
      first = min(first, (int)(g << 6) + __ffsll(v) - 1);
      last = max(last, (int)(g << 6) + 63 - __clzll((long long)v));
    }
  }
  mask_chunk_reduce(n, first, last, counts, info);
}

// out = op(m0 .. m(n-1)) word by word: a thread reads its word of EVERY operand (through mask_word: their bits at or beyond `rows` may hold
// anything) before it writes it, so `out` may be any of them; the complement (ANDNOT) is cut at `rows`, so the output's tail bits are zero.
__global__ void __launch_bounds__(kMaskThreads) mask_combine_kernel(MaskOperands ops, int64_t rows, int64_t n_words, uint32_t* out,
                                                                    unsigned* __restrict__ counts, MaskChunkInfo* __restrict__ info) {
  const int64_t w0 = (int64_t)blockIdx.x * kMaskWordsPerBlock;
  unsigned n = 0;
  int first = 0x7FFFFFFF, last = -1;
  for (int i = threadIdx.x; i < kMaskWordsPerBlock; i += kMaskThreads) {
    const int64_t w = w0 + i;
    if (w >= n_words) break;
    uint32_t v = mask_word(ops.m[0], w, n_words, rows), rest = 0u;
#pragma unroll
    for (int j = 1; j < TAVB_MAX_MASK_OPERANDS; ++j) {
      if (j < ops.n) {
        const uint32_t t = mask_word(ops.m[j], w, n_words, rows);
        if (ops.op == TAVB_MASK_AND) v &= t;
        else if (ops.op == TAVB_MASK_OR) v |= t;
        else rest |= t;
      }
    }
    if (ops.op == TAVB_MASK_ANDNOT) {
      v = ops.n == 1 ? ~v : v & ~rest;
      const int tail = (int)(rows & 31);
      if (w == n_words - 1 && tail != 0) v &= (1u << tail) - 1u;
    }
    out[w] = v;
    if (v) {
      n += (unsigned)__popc(v);
      first = min(first, (int)(w << 5) + __ffs((int)v) - 1);
      last = max(last, (int)(w << 5) + 31 - __clz((int)v));
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {  // lane 0 of every wave: the wave's sum, lowest and highest row
    n += __shfl_down(n, d, 64);
    first = min(first, __shfl_down(first, d, 64));
    last = max(last, __shfl_down(last, d, 64));
  }
  mask_chunk_reduce(n, first, last, counts, info);
}

// ---- scoped batches (tavb_search_scoped_batch): which of a pass' scopes hold each row of their union.  A thread takes one position of the
// union's row list (coalesced) and reads that row's word of every operand -- the masks are rows / 8 bytes each and stay in L2 -- and writes
// one byte: bit j = operand j holds the row.  The scan then needs one byte per row, not a word of every mask.  A row outside [0, n_rows)
// (there is none in a list the write pass made) gets 0: no query takes it.
__global__ void __launch_bounds__(kMaskThreads) scope_member_kernel(MaskOperands ops, const int32_t* __restrict__ rows, int64_t n, int64_t n_rows,
                                                                    uint8_t* __restrict__ member) {
  static_assert(TAVB_MAX_MASK_OPERANDS <= 8, "one bit of the byte per operand");
  const int64_t stride = (int64_t)gridDim.x * kMaskThreads;
  for (int64_t p = (int64_t)blockIdx.x * kMaskThreads + threadIdx.x; p < n; p += stride) {
    const int64_t r = rows[p];
    unsigned m = 0u;
    if (r >= 0 && r < n_rows) {
#pragma unroll
      for (int j = 0; j < TAVB_MAX_MASK_OPERANDS; ++j)
        if (j < ops.n) m |= ((ops.m[j][r >> 5] >> (r & 31)) & 1u) << j;
    }
    member[p] = (uint8_t)m;
  }
}

// ---- scoped batches on the 32/64-query tile (tavb_search_scoped_tile): the membership PLANES the tile's admission path reads -- per block of
// 32 queries one word per row, bit i = the scope of query i of the block holds the row: a 32 x 32 bit transpose of the masks' words per
// 32-row block.  A wave takes two 32-row blocks of one query block at a time: lane l reads word (block pair * 2 + (l >> 5)) of mask l & 31 --
// 32 masks x 8 bytes -- clears the bits behind last_row (the stray bits of a mask's last word among them) and the words of missing masks
// (padding queries), then 32 ballots turn the columns into rows: ballot r is {bit r of every lane's word} = the plane word of row r of the
// lower block in its low half and of the upper block in its high half.  Lane l keeps ballot l & 31's half l >> 5 and the wave stores 64
// consecutive plane words.  Reads n masks x span / 8 bytes, writes as much.
__global__ void __launch_bounds__(kMaskThreads) scope_planes_kernel(ScopeMasks ms, int n_blocks, int64_t span_begin, int64_t last_row, int64_t stride,
                                                                    uint32_t* __restrict__ planes) {
  const int lane = threadIdx.x & 63;
  const int64_t pairs = (stride + 63) >> 6;  // pairs of 32-row blocks per plane
  const int64_t n_items = pairs * n_blocks;
  const int64_t wave0 = (int64_t)blockIdx.x * kMaskWaves + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * kMaskWaves;
  for (int64_t item = wave0; item < n_items; item += n_waves) {
    const int b = (int)(item / pairs);
    const int64_t rel = (item % pairs) * 64 + (lane >> 5) * 32;  // this half-wave's 32-row block, relative to span_begin
    const int64_t row = span_begin + rel;
    const int q = 32 * b + (lane & 31);
    uint32_t w = 0u;
    if (q < ms.n && rel < stride && row <= last_row) {
      w = ms.m[q][row >> 5];
      if (last_row - row < 31) w &= (2u << (int)(last_row - row)) - 1u;
    }
    uint32_t mine = 0u;
#pragma unroll
    for (int r = 0; r < 32; ++r) {
      const unsigned long long col = __ballot((w >> r) & 1u);
      if ((lane & 31) == r) mine = (uint32_t)(col >> (lane & 32));
    }
    if (rel < stride) planes[(int64_t)b * stride + rel + (lane & 31)] = mine;
  }
}

// ---- row compaction (tavb_compact_rows): the mask names the rows to REMOVE, the kept rows move down in their old order.
//   compact_count_kernel    chunk b -> counts[b] = its KEPT rows, info[b] = that count and the chunk's first and last removed row
//   compact_gather_kernel   a workgroup takes a tile of 64 rows (two mask words) of the row range [r0, r1): the tile's first slot is the
//                           number of kept rows in [from, tile) -- whole chunks from the counts, the rest from the mask's words -- a row's
//                           slot the popcount of the tile's kept bits below it, and a wave copies a kept row to dst + slot
//   compact_scatter_kernel  staging [0, kept in [r0, r1)) -> corpus rows from (kept in [0, r0)) on: a flat copy whose ends every workgroup
//                           works out for itself from the counts and the mask
// No workgroup waits for another: the order between a pass' gather, its scatter and the next pass is stream order between launches.  The
// copies move V (16, 8, 4 or 2 bytes: the launchers pick the widest that divides the row bytes and every address) at a time.

constexpr int kCompactTileRows = 64;

// the kept rows of word w: the complement of the removal bits, cut at `rows`; 0 past the last word
__device__ __forceinline__ uint32_t kept_word(const uint32_t* __restrict__ bits, int64_t w, int64_t n_words, int64_t rows) {
  if (w >= n_words) return 0u;
  uint32_t v = ~bits[w];
  const int tail = (int)(rows & 31);
  if (w == n_words - 1 && tail != 0) v &= (1u << tail) - 1u;
  return v;
}

// Kept rows in [a, b), the same value on every thread of the workgroup (all of them call it): a is a multiple of 32, b a multiple of 32 or
// `rows`, a <= b.  Whole chunks come from counts[], the ends from the words.  sh: one LDS word, free again on return.
__device__ __forceinline__ unsigned kept_between(const uint32_t* __restrict__ bits, const unsigned* __restrict__ counts, int64_t a, int64_t b,
                                                 int64_t n_words, int64_t rows, unsigned* sh) {
  constexpr int64_t kChunk = TAVB_MASK_ROWS_PER_WORKGROUP;
  const int64_t wa = a >> 5, wb = (b + 31) >> 5;
  const int64_t ca = (a + kChunk - 1) / kChunk, cb = b / kChunk;  // the whole chunks inside: [ca, cb)
  unsigned part = 0;
  if (ca <= cb) {
    for (int64_t w = wa + threadIdx.x; w < ca * kMaskWordsPerBlock; w += kMaskThreads) part += (unsigned)__popc(kept_word(bits, w, n_words, rows));
    for (int64_t ch = ca + threadIdx.x; ch < cb; ch += kMaskThreads) part += counts[ch];
    for (int64_t w = cb * kMaskWordsPerBlock + threadIdx.x; w < wb; w += kMaskThreads) part += (unsigned)__popc(kept_word(bits, w, n_words, rows));
  } else {  // no chunk boundary in [a, b]
    for (int64_t w = wa + threadIdx.x; w < wb; w += kMaskThreads) part += (unsigned)__popc(kept_word(bits, w, n_words, rows));
  }
  if (threadIdx.x == 0) *sh = 0u;
  __syncthreads();
  if (part) atomicAdd(sh, part);
  __syncthreads();
  const unsigned all = *sh;
  __syncthreads();
  return all;
}

__global__ void __launch_bounds__(kMaskThreads) compact_count_kernel(const uint32_t* __restrict__ bits, int64_t rows, int64_t n_words,
                                                                     unsigned* __restrict__ counts, MaskChunkInfo* __restrict__ info) {
  const int64_t w0 = (int64_t)blockIdx.x * kMaskWordsPerBlock;
  unsigned n = 0;
  int first = 0x7FFFFFFF, last = -1;
  for (int i = threadIdx.x; i < kMaskWordsPerBlock; i += kMaskThreads) {
    const int64_t w = w0 + i;
    if (w >= n_words) break;
    const uint32_t v = mask_word(bits, w, n_words, rows);
    n += (unsigned)__popc(kept_word(bits, w, n_words, rows));
    if (v) {
      first = min(first, (int)(w << 5) + __ffs((int)v) - 1);
      last = max(last, (int)(w << 5) + 31 - __clz((int)v));
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    n += __shfl_down(n, d, 64);
    first = min(first, __shfl_down(first, d, 64));
    last = max(last, __shfl_down(last, d, 64));
  }
  mask_chunk_reduce(n, first, last, counts, info);
}

// n V's from s to d (disjoint), a wave's 64 lanes side by side; four loads in flight per lane
template <typename V>
__device__ __forceinline__ void wave_copy(const V* __restrict__ s, V* __restrict__ d, int64_t n, int lane) {
  int64_t j = lane;
  for (; j + 192 < n; j += 256) {
    const V a = s[j], b = s[j + 64], c = s[j + 128], e = s[j + 192];
    d[j] = a;
    d[j + 64] = b;
    d[j + 128] = c;
    d[j + 192] = e;
  }
  for (; j < n; j += 64) d[j] = s[j];
}

// n V's from s to d (disjoint), the whole grid side by side: a grid-stride copy, four loads in flight per thread
template <typename V>
__device__ __forceinline__ void grid_copy(const V* __restrict__ s, V* __restrict__ d, int64_t n) {
  const int64_t step = (int64_t)gridDim.x * kMaskThreads;
  int64_t j = (int64_t)blockIdx.x * kMaskThreads + threadIdx.x;
  for (; j + 3 * step < n; j += 4 * step) {
    const V a = s[j], b = s[j + step], c = s[j + 2 * step], e = s[j + 3 * step];
    d[j] = a;
    d[j + step] = b;
    d[j + 2 * step] = c;
    d[j + 3 * step] = e;
  }
  for (; j < n; j += step) d[j] = s[j];
}

// kept rows of src rows [r0, r1) -> dst rows [kept in [from, r0), ..), densely, in order.  r0 and `from` are multiples of 64, from <= r0, r1
// a multiple of 64 or `rows`; src and dst do not overlap.  Workgroup b takes rows [r0 + 64 b, r0 + 64 b + 64).
template <typename V>
__global__ void __launch_bounds__(kMaskThreads) compact_gather_kernel(const char* __restrict__ src, char* __restrict__ dst,
                                                                      const uint32_t* __restrict__ bits, const unsigned* __restrict__ counts,
                                                                      int64_t rows, int64_t n_words, int64_t from, int64_t r0, int64_t r1,
                                                                      int64_t row_bytes) {
  __shared__ unsigned sh;
  const int64_t t0 = r0 + (int64_t)blockIdx.x * kCompactTileRows;
  if (t0 >= r1) return;  // (block-uniform)
  const int64_t base = kept_between(bits, counts, from, t0, n_words, rows, &sh);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = t0 >> 5;
  const unsigned long long km = (unsigned long long)kept_word(bits, w, n_words, rows) | ((unsigned long long)kept_word(bits, w + 1, n_words, rows) << 32);
  const int64_t n_vec = row_bytes / (int64_t)sizeof(V);
  for (int i = wave; i < kCompactTileRows; i += kMaskWaves) {  // (wave-uniform)
    if (!((km >> i) & 1ull)) continue;
    const int64_t slot = base + __popcll(km & ((1ull << i) - 1ull));
    wave_copy(reinterpret_cast<const V*>(src + (t0 + i) * row_bytes), reinterpret_cast<V*>(dst + slot * row_bytes), n_vec, lane);
  }
}

// staging rows [0, kept in [r0, r1)) -> corpus rows [kept in [0, r0), ..): a grid-stride copy
template <typename V>
__global__ void __launch_bounds__(kMaskThreads) compact_scatter_kernel(const char* __restrict__ staging, char* __restrict__ corpus,
                                                                       const uint32_t* __restrict__ bits, const unsigned* __restrict__ counts,
                                                                       int64_t rows, int64_t n_words, int64_t r0, int64_t r1, int64_t row_bytes) {
  __shared__ unsigned sh;
  const int64_t dst_row = kept_between(bits, counts, 0, r0, n_words, rows, &sh);
  const int64_t kept = kept_between(bits, counts, r0, r1, n_words, rows, &sh);
  grid_copy(reinterpret_cast<const V*>(staging), reinterpret_cast<V*>(corpus + dst_row * row_bytes), kept * (row_bytes / (int64_t)sizeof(V)));
}

// the widest of 16, 8, 4, 2 bytes that divides `x` (row bytes or'ed with the addresses)
int compact_vector_bytes(uint64_t x) {
  for (int v = 16; v > 2; v >>= 1)
    if (x % (uint64_t)v == 0) return v;
  return 2;
}

// ---- row expansion (tavb_expand_rows): the mirror image.  The mask covers the NEW row count and names the HOLES that new rows will fill; the
// old rows -- as many as the mask has clear bits -- move up, in order, to the rows whose bit is clear.  kept_word / kept_between count clear
// bits, so "kept rows before r" is old row o(r) = the source of new row r.
//   expand_stage_kernel    the old rows of new rows [r0, r1) are the contiguous range [o(r0), o(r1)): a flat copy of them into staging,
//                          whose ends every workgroup works out for itself (in place only)
//   expand_scatter_kernel  a workgroup takes a tile of 64 new rows of [r0, r1): the tile's first source slot is the number of clear bits in
//                          [from, tile) -- from = r0 over the staging of the pass, 0 over the whole old corpus (out of place) -- and a wave
//                          copies source row slot + (clear bits of the tile below i) to row tile + i for every clear bit i.  Holes are not
//                          written: tavb_scatter_rows fills them.
// In place the passes run FROM THE TAIL (tavb_expand_rows says why that is safe); the order between launches is stream order, nothing else.

template <typename V>
__global__ void __launch_bounds__(kMaskThreads) expand_stage_kernel(const char* __restrict__ corpus, char* __restrict__ staging,
                                                                    const uint32_t* __restrict__ bits, const unsigned* __restrict__ counts,
                                                                    int64_t rows, int64_t n_words, int64_t r0, int64_t r1, int64_t row_bytes) {
  __shared__ unsigned sh;
  const int64_t o0 = kept_between(bits, counts, 0, r0, n_words, rows, &sh);
  const int64_t n_old = kept_between(bits, counts, r0, r1, n_words, rows, &sh);
  grid_copy(reinterpret_cast<const V*>(corpus + o0 * row_bytes), reinterpret_cast<V*>(staging), n_old * (row_bytes / (int64_t)sizeof(V)));
}

// src rows [clear bits in [from, r0), ..) -> the rows of dst rows [r0, r1) whose bit is clear, in order.  r0 and `from` are multiples of 64,
// from <= r0, r1 a multiple of 64 or `rows`; src and dst do not overlap.  Workgroup b takes rows [r0 + 64 b, r0 + 64 b + 64).
template <typename V>
__global__ void __launch_bounds__(kMaskThreads) expand_scatter_kernel(const char* __restrict__ src, char* __restrict__ dst,
                                                                      const uint32_t* __restrict__ bits, const unsigned* __restrict__ counts,
                                                                      int64_t rows, int64_t n_words, int64_t from, int64_t r0, int64_t r1,
                                                                      int64_t row_bytes) {
  __shared__ unsigned sh;
  const int64_t t0 = r0 + (int64_t)blockIdx.x * kCompactTileRows;
  if (t0 >= r1) return;  // (block-uniform)
  const int64_t base = kept_between(bits, counts, from, t0, n_words, rows, &sh);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = t0 >> 5;
  const unsigned long long km = (unsigned long long)kept_word(bits, w, n_words, rows) | ((unsigned long long)kept_word(bits, w + 1, n_words, rows) << 32);
  const int64_t n_vec = row_bytes / (int64_t)sizeof(V);
  for (int i = wave; i < kCompactTileRows; i += kMaskWaves) {  // (wave-uniform)
    if (!((km >> i) & 1ull)) continue;
    const int64_t slot = base + __popcll(km & ((1ull << i) - 1ull));
    wave_copy(reinterpret_cast<const V*>(src + slot * row_bytes), reinterpret_cast<V*>(dst + (t0 + i) * row_bytes), n_vec, lane);
  }
}

// ---- masks carried through a row edit (tavb_mask_remap): np.delete / np.insert of packed masks under the edit's packed flags, up to
// TAVB_MAX_MASK_OPERANDS masks per launch.  The flags' per-chunk counts of clear bits (compact_count_kernel: kept rows of a removal, old
// rows of an insertion) are made once per call; a workgroup sums the counts of the chunks before its own, scans its 512 flag words once,
// works out the moves of every flag word once (tavb_remap_bits.h) and applies them to that word of every operand, in registers.
//   mask_remap_squeeze_kernel  REMOVE.  The flags cover the OLD rows, so a workgroup owns a chunk of INPUT words: a lane squeezes its word of
//                              an operand under the kept bits and ORs the piece -- it straddles at most two words -- into an LDS image of
//                              the chunk's output bits [kept before the chunk, + kept in it).  The image's inner words are stored; its
//                              first and last word, which the neighbouring chunks may share, go out through an atomic OR: the output
//                              was zeroed by the launcher's memset, and an OR does not care about order, so the result is deterministic.
//   mask_remap_info_kernel     the counts and infos of those outputs per chunk of NEW rows (the chunks of the two row spaces do not line up)
//   mask_remap_spread_kernel   INSERT and APPEND.  The flags cover the NEW rows, so a workgroup owns a chunk of OUTPUT words: a lane's source
//                              bits are the popcount(clear) bits from bit (clear bits before its word) of the input on -- two words through a
//                              funnel shift -- spread under the clear bits; the holes take `fill`.  Plain stores, and the chunk's count and
//                              info in the same launch.  APPEND has no flags: the holes are the bits [old_rows, new_rows).
// No workgroup waits for another.  Inputs are read through mask_word (bits at or beyond old_rows may hold anything); output bits at or beyond
// new_rows are zero.

constexpr int kRemapRounds = kMaskWordsPerBlock / kMaskThreads;
constexpr int kRemapPieceWords = kMaskWordsPerBlock + 2;  // a chunk's output bits start anywhere in a word: up to 31 bits in front, as many behind

__device__ __forceinline__ uint32_t low_bits(int64_t k) { return k >= 32 ? 0xFFFFFFFFu : k <= 0 ? 0u : (1u << (int)k) - 1u; }

// The exclusive prefix of `mine` over the workgroup in thread order, *total = the sum; every thread calls it.  wc: kMaskWaves LDS words,
// free again on return.
__device__ __forceinline__ unsigned block_prefix(unsigned mine, unsigned* wc, unsigned* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned incl = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wc[wave] = incl;
  __syncthreads();
  unsigned before = 0, all = 0;
  for (int x = 0; x < kMaskWaves; ++x) {
    before += x < wave ? wc[x] : 0u;
    all += wc[x];
  }
  __syncthreads();
  *total = all;
  return before + (incl - mine);
}

// the sum of counts[0 .. blockIdx.x), the same value on every thread (all of them call it); sh: one LDS word, free again on return
__device__ __forceinline__ unsigned counts_before(const unsigned* __restrict__ counts, unsigned* sh) {
  if (threadIdx.x == 0) *sh = 0u;
  __syncthreads();
  unsigned part = 0;
  for (unsigned b = threadIdx.x; b < blockIdx.x; b += kMaskThreads) part += counts[b];
  if (part) atomicAdd(sh, part);
  __syncthreads();
  const unsigned all = *sh;
  __syncthreads();
  return all;
}

__global__ void __launch_bounds__(kMaskThreads) mask_remap_squeeze_kernel(RemapOperands ops, const uint32_t* __restrict__ flags,
                                                                          const unsigned* __restrict__ kept_counts, int64_t old_rows,
                                                                          int64_t old_words, int64_t new_words) {
  __shared__ uint32_t piece[kRemapPieceWords];
  __shared__ unsigned sh;
  __shared__ unsigned wc[kMaskWaves];
  const unsigned kept = kept_counts[blockIdx.x];
  if (kept == 0) return;  // (block-uniform) the chunk leaves no bit
  const int64_t base = counts_before(kept_counts, &sh);  // the chunk's first output bit
  const unsigned head = (unsigned)(base & 31);
  const int64_t word0 = base >> 5;
  const int n_piece = (int)((head + kept + 31u) >> 5);
  const int64_t w0 = (int64_t)blockIdx.x * kMaskWordsPerBlock + threadIdx.x;
  uint32_t kw[kRemapRounds];
  unsigned off[kRemapRounds];  // where the lane's piece starts, in bits of the image
  BitMoves mv[kRemapRounds];
  unsigned run = head;
#pragma unroll
  for (int r = 0; r < kRemapRounds; ++r) {
    kw[r] = kept_word(flags, w0 + r * kMaskThreads, old_words, old_rows);
    unsigned all;
    off[r] = run + block_prefix((unsigned)__popc(kw[r]), wc, &all);
    run += all;
    mv[r] = bit_moves(kw[r]);
  }
  for (int j = 0; j < ops.n; ++j) {  // (block-uniform)
    for (int i = threadIdx.x; i < n_piece; i += kMaskThreads) piece[i] = 0u;
    __syncthreads();
    const uint32_t* __restrict__ in = ops.in[j];
#pragma unroll
    for (int r = 0; r < kRemapRounds; ++r) {
      if (kw[r] == 0u) continue;
      const uint32_t x = squeeze_bits(mask_word(in, w0 + r * kMaskThreads, old_words, old_rows), kw[r], mv[r]);
      if (x == 0u) continue;
      const unsigned lo = off[r] >> 5, s = off[r] & 31u;
      atomicOr(&piece[lo], x << s);
      if (s != 0u && (x >> (32u - s)) != 0u) atomicOr(&piece[lo + 1], x >> (32u - s));
    }
    __syncthreads();
    uint32_t* out = ops.out[j];
    for (int i = threadIdx.x; i < n_piece; i += kMaskThreads) {
      const uint32_t v = piece[i];
      const int64_t gw = word0 + i;
      if (gw >= new_words) continue;  // (never: the host has checked that the kept rows number new_rows)
      const bool shared = (i == 0 && head != 0u) || (i == n_piece - 1 && ((head + kept) & 31u) != 0u);
      if (!shared) out[gw] = v;
      else if (v != 0u) atomicOr(&out[gw], v);
    }
    __syncthreads();  // the image is zeroed again for the next operand
  }
}

// counts[j * chunks + b], info[j * chunks + b] of output j (blockIdx.y) over its chunk b of NEW rows
__global__ void __launch_bounds__(kMaskThreads) mask_remap_info_kernel(RemapOperands ops, int64_t rows, int64_t n_words, unsigned* __restrict__ counts,
                                                                       MaskChunkInfo* __restrict__ info) {
  const uint32_t* __restrict__ bits = ops.out[blockIdx.y];
  const int64_t w0 = (int64_t)blockIdx.x * kMaskWordsPerBlock;
  unsigned n = 0;
  int first = 0x7FFFFFFF, last = -1;
  for (int i = threadIdx.x; i < kMaskWordsPerBlock; i += kMaskThreads) {
    const int64_t w = w0 + i;
    if (w >= n_words) break;
    const uint32_t v = mask_word(bits, w, n_words, rows);
    if (v) {
      n += (unsigned)__popc(v);
      first = min(first, (int)(w << 5) + __ffs((int)v) - 1);
      last = max(last, (int)(w << 5) + 31 - __clz((int)v));
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    n += __shfl_down(n, d, 64);
    first = min(first, __shfl_down(first, d, 64));
    last = max(last, __shfl_down(last, d, 64));
  }
  const size_t at = (size_t)blockIdx.y * gridDim.x;
  mask_chunk_reduce(n, first, last, counts + at, info + at);
}

__global__ void __launch_bounds__(kMaskThreads) mask_remap_spread_kernel(RemapOperands ops, const uint32_t* __restrict__ flags,
                                                                         const unsigned* __restrict__ clear_counts, int64_t old_rows,
                                                                         int64_t old_words, int64_t new_rows, int64_t new_words, int fill,
                                                                         unsigned* __restrict__ counts, MaskChunkInfo* __restrict__ info) {
  __shared__ unsigned sh;
  __shared__ unsigned wc[kMaskWaves];
  // the chunk's first source bit: the clear bits in front of it
  const int64_t chunk0 = (int64_t)blockIdx.x * TAVB_MASK_ROWS_PER_WORKGROUP;
  const int64_t base = flags ? (int64_t)counts_before(clear_counts, &sh) : (chunk0 < old_rows ? chunk0 : old_rows);
  const int64_t w0 = (int64_t)blockIdx.x * kMaskWordsPerBlock + threadIdx.x;
  uint32_t hole[kRemapRounds], clear[kRemapRounds];
  int64_t src[kRemapRounds];  // the lane's first source bit
  BitMoves mv[kRemapRounds];
  int64_t run = base;
#pragma unroll
  for (int r = 0; r < kRemapRounds; ++r) {
    const int64_t w = w0 + r * kMaskThreads;
    const uint32_t valid = w < new_words ? low_bits(new_rows - (w << 5)) : 0u;
    hole[r] = flags ? mask_word(flags, w, new_words, new_rows) : valid & ~low_bits(old_rows - (w << 5));
    clear[r] = valid & ~hole[r];
    unsigned all;
    src[r] = run + block_prefix((unsigned)__popc(clear[r]), wc, &all);
    run += all;
    mv[r] = bit_moves(clear[r]);
  }
  for (int j = 0; j < ops.n; ++j) {  // (block-uniform)
    const uint32_t* __restrict__ in = ops.in[j];
    uint32_t* __restrict__ out = ops.out[j];
    unsigned n = 0;
    int first = 0x7FFFFFFF, last = -1;
#pragma unroll
    for (int r = 0; r < kRemapRounds; ++r) {
      const int64_t w = w0 + r * kMaskThreads;
      if (w >= new_words) continue;
      uint32_t v = fill ? hole[r] : 0u;
      if (clear[r] != 0u) {
        const int64_t lo = src[r] >> 5;
        const uint32_t x = funnel_bits(mask_word(in, lo, old_words, old_rows), mask_word(in, lo + 1, old_words, old_rows), (int)(src[r] & 31));
        v |= spread_bits(x & low_bits(__popc(clear[r])), clear[r], mv[r]);
      }
      out[w] = v;
      if (v) {
        n += (unsigned)__popc(v);
        first = min(first, (int)(w << 5) + __ffs((int)v) - 1);
        last = max(last, (int)(w << 5) + 31 - __clz((int)v));
      }
    }
    for (int d = 32; d >= 1; d >>= 1) {
      n += __shfl_down(n, d, 64);
      first = min(first, __shfl_down(first, d, 64));
      last = max(last, __shfl_down(last, d, 64));
    }
    const size_t at = (size_t)j * gridDim.x;
    mask_chunk_reduce(n, first, last, counts + at, info + at);
    __syncthreads();  // (the reduction's LDS words are written again for the next operand)
  }
}

// ---- scattered row writes (tavb_scatter_rows): n staged fp32 rows -> corpus rows positions[j], converted to the corpus' dtype as the load
// path converts them ((_Float16)x: v_cvt_f16_f32, round to nearest even), so a row written here equals the same row uploaded.
//   scatter_check_kernel   *bad = 1 when a position lies outside [0, rows) (host memory the device writes; the host zeroes it first)
//   scatter_rows_kernel    one wave per row.  A row BELOW norm_rows is covered by the per-corpus caches, which are kept up to date instead of
//                          thrown away: its fp16 shadow row is written where there is a shadow (`shadow`, sdim halves per row, the tail zero),
//                          and its squared norms are folded into the cached maxima (stats[0] = max sum(x16^2), fp32 corpora also stats[1] =
//                          max sum((x - x16)^2)) -- summed in the order shadow_convert_kernel / corpus_max_norm_kernel sum them (a lane takes
//                          groups of 4 floats, or 8 halves, 64 groups apart), folded with the same atomic maximum.  The old norm of a replaced
//                          row stays in the maximum: it is an upper bound, which is all the filter needs.

__global__ void __launch_bounds__(kMaskThreads) scatter_check_kernel(const int32_t* __restrict__ positions, int64_t n, int64_t rows, int* __restrict__ bad) {
  for (int64_t j = (int64_t)blockIdx.x * kMaskThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kMaskThreads) {
    const int32_t p = positions[j];
    if (p < 0 || (int64_t)p >= rows) *bad = 1;
  }
}

template <typename T>
__global__ void __launch_bounds__(kMaskThreads) scatter_rows_kernel(const float* __restrict__ src, int64_t n, int dim,
                                                                    const int32_t* __restrict__ positions, int64_t rows, T* __restrict__ corpus,
                                                                    _Float16* __restrict__ shadow, int sdim, int64_t norm_rows,
                                                                    float* __restrict__ stats) {
  constexpr bool kF32 = sizeof(T) == 4;
  constexpr int G = kF32 ? 4 : 8;  // elements of one lane's step: shadow_convert_kernel's (fp32 rows) and corpus_max_norm_kernel's (fp16 rows)
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * kMaskWaves + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * kMaskWaves;
  const int groups = (dim + G - 1) / G;
  const bool whole = dim % G == 0 && ((uintptr_t)src | (uintptr_t)corpus) % 16 == 0;  // 16-byte loads and stores (rows are then 16-byte multiples)
  float best16 = 0.f, best_err = 0.f;
  bool folded = false;
  for (int64_t j = wave; j < n; j += n_waves) {  // (wave-uniform)
    const int64_t p = positions[j];
    if (p < 0 || p >= rows) continue;  // (the host has checked: never taken)
    const bool cached = p < norm_rows;
    const float* x = src + j * (int64_t)dim;
    T* y = corpus + p * (int64_t)dim;
    _Float16* s = (cached && shadow) ? shadow + p * (int64_t)sdim : nullptr;
    float ss = 0.f, se = 0.f;
    for (int g = lane; g < groups; g += 64) {
      float e[G];
      _Float16 h[G];
      const int i0 = g * G;
      if (whole) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + i0);
        e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w;
        if constexpr (!kF32) {
          const f32x4 b = *reinterpret_cast<const f32x4*>(x + i0 + 4);
          e[4] = b.x; e[5] = b.y; e[6] = b.z; e[7] = b.w;
        }
      } else {
#pragma unroll
        for (int t = 0; t < G; ++t) e[t] = (i0 + t < dim) ? x[i0 + t] : 0.0f;
      }
#pragma unroll
      for (int t = 0; t < G; ++t) {
        h[t] = (_Float16)e[t];
        const float hf = (float)h[t];
        ss = fmaf(hf, hf, ss);
        if constexpr (kF32) {
          const float d = e[t] - hf;
          se = fmaf(d, d, se);
        }
      }
      if (whole) {
        if constexpr (kF32) {
          *reinterpret_cast<f32x4*>(y + i0) = f32x4{e[0], e[1], e[2], e[3]};
          if (s) *reinterpret_cast<uint2*>(s + i0) = *reinterpret_cast<const uint2*>(h);
        } else {
          *reinterpret_cast<uint4*>(y + i0) = *reinterpret_cast<const uint4*>(h);
          if (s) *reinterpret_cast<uint4*>(s + i0) = *reinterpret_cast<const uint4*>(h);
        }
      } else {
#pragma unroll
        for (int t = 0; t < G; ++t) {
          if (i0 + t >= dim) break;
          if constexpr (kF32) y[i0 + t] = e[t]; else y[i0 + t] = h[t];
          if (s) s[i0 + t] = h[t];
        }
      }
    }
    if (s)
      for (int i = dim + lane; i < sdim; i += 64) s[i] = (_Float16)0.0f;
    if (!cached) continue;
    ss = wave_sum(ss);
    se = wave_sum(se);
    if (!(ss < __builtin_inff())) ss = __builtin_inff();  // NaN / inf rows: the bound is useless, every query takes the exact path
    if (!(se < __builtin_inff())) se = __builtin_inff();
    best16 = fmaxf(best16, ss);
    best_err = fmaxf(best_err, se);
    folded = true;
  }
  if (folded && lane == 0) {
    // non-negative floats (and +inf) order like their bit patterns
    atomicMax(reinterpret_cast<unsigned int*>(stats), __float_as_uint(best16));
    if constexpr (kF32) atomicMax(reinterpret_cast<unsigned int*>(stats + 1), __float_as_uint(best_err));
  }
}

}  // namespace

hipError_t launch_expand_stage(const void* corpus, void* staging, const uint32_t* bits, const unsigned* counts, int64_t rows, int64_t r0, int64_t r1,
                               int64_t row_bytes, hipStream_t stream) {
  if (!corpus || !staging || !bits || !counts || rows < 1 || rows >= 0x7FFFFFFFll || row_bytes < 2 || row_bytes % 2 != 0 || r0 < 0 || r0 >= r1 || r1 > rows ||
      r0 % kCompactTileRows != 0 || (r1 % kCompactTileRows != 0 && r1 != rows))
    return hipErrorInvalidValue;
  const int vb = compact_vector_bytes((uint64_t)row_bytes | reinterpret_cast<uintptr_t>(staging) | reinterpret_cast<uintptr_t>(corpus));
  const int64_t most = (r1 - r0) * (row_bytes / vb);  // V's to copy when the pass has no hole
  const unsigned blocks = (unsigned)std::min<int64_t>((most + 4 * kMaskThreads - 1) / (4 * kMaskThreads), 2048);
  const int64_t n_words = (rows + 31) >> 5;
  const char* s = reinterpret_cast<const char*>(corpus);
  char* d = reinterpret_cast<char*>(staging);
#define TAVB_STAGE(V) hipLaunchKernelGGL(expand_stage_kernel<V>, dim3(blocks), dim3(kMaskThreads), 0, stream, s, d, bits, counts, rows, n_words, r0, r1, row_bytes)
  switch (vb) {
    case 16: TAVB_STAGE(uint4); break;
    case 8: TAVB_STAGE(uint2); break;
    case 4: TAVB_STAGE(uint32_t); break;
    default: TAVB_STAGE(uint16_t); break;
  }
#undef TAVB_STAGE
  return hipGetLastError();
}

hipError_t launch_expand_scatter(const void* src, void* dst, const uint32_t* bits, const unsigned* counts, int64_t rows, int64_t from, int64_t r0,
                                 int64_t r1, int64_t row_bytes, hipStream_t stream) {
  if (!src || !dst || !bits || !counts || rows < 1 || rows >= 0x7FFFFFFFll || row_bytes < 2 || row_bytes % 2 != 0 || from < 0 || from > r0 || r0 >= r1 ||
      r1 > rows || from % kCompactTileRows != 0 || r0 % kCompactTileRows != 0 || (r1 % kCompactTileRows != 0 && r1 != rows))
    return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((r1 - r0 + kCompactTileRows - 1) / kCompactTileRows);
  const int64_t n_words = (rows + 31) >> 5;
  const char* s = reinterpret_cast<const char*>(src);
  char* d = reinterpret_cast<char*>(dst);
#define TAVB_EXPAND(V) hipLaunchKernelGGL(expand_scatter_kernel<V>, dim3(blocks), dim3(kMaskThreads), 0, stream, s, d, bits, counts, rows, n_words, from, r0, r1, row_bytes)
  switch (compact_vector_bytes((uint64_t)row_bytes | reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst))) {
    case 16: TAVB_EXPAND(uint4); break;
    case 8: TAVB_EXPAND(uint2); break;
    case 4: TAVB_EXPAND(uint32_t); break;
    default: TAVB_EXPAND(uint16_t); break;
  }
#undef TAVB_EXPAND
  return hipGetLastError();
}

hipError_t launch_scatter_check(const int32_t* positions, int64_t n, int64_t rows, int* bad, hipStream_t stream) {
  if (!positions || !bad || n < 1 || rows < 0) return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)std::min<int64_t>((n + kMaskThreads - 1) / kMaskThreads, 1024);
  hipLaunchKernelGGL(scatter_check_kernel, dim3(blocks), dim3(kMaskThreads), 0, stream, positions, n, rows, bad);
  return hipGetLastError();
}

hipError_t launch_scatter_rows(const float* src, int64_t n, int dim, const int32_t* positions, int64_t rows, void* corpus, bool f16, void* shadow, int sdim,
                               int64_t norm_rows, float* stats, hipStream_t stream) {
  if (!src || !positions || !corpus || n < 1 || dim < 1 || rows < 1 || (norm_rows > 0 && !stats) || (shadow && sdim < dim)) return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)std::min<int64_t>((n + kMaskWaves - 1) / kMaskWaves, 256 * 8);
  _Float16* sh = reinterpret_cast<_Float16*>(shadow);
  if (f16)
    hipLaunchKernelGGL(scatter_rows_kernel<_Float16>, dim3(blocks), dim3(kMaskThreads), 0, stream, src, n, dim, positions, rows, reinterpret_cast<_Float16*>(corpus), sh,
                       sdim, norm_rows, stats);
  else
    hipLaunchKernelGGL(scatter_rows_kernel<float>, dim3(blocks), dim3(kMaskThreads), 0, stream, src, n, dim, positions, rows, reinterpret_cast<float*>(corpus), sh, sdim,
                       norm_rows, stats);
  return hipGetLastError();
}

hipError_t launch_compact_count(const uint32_t* bits, int64_t rows, unsigned* counts, MaskChunkInfo* info, hipStream_t stream) {
  if (!bits || !counts || !info || rows < 1 || rows >= 0x7FFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(compact_count_kernel, dim3(mask_blocks(rows)), dim3(kMaskThreads), 0, stream, bits, rows, (rows + 31) >> 5, counts, info);
  return hipGetLastError();
}

hipError_t launch_compact_gather(const void* src, void* dst, const uint32_t* bits, const unsigned* counts, int64_t rows, int64_t from, int64_t r0,
                                 int64_t r1, int64_t row_bytes, hipStream_t stream) {
  if (!src || !dst || !bits || !counts || rows < 1 || rows >= 0x7FFFFFFFll || row_bytes < 2 || row_bytes % 2 != 0 || from < 0 || from > r0 || r0 >= r1 ||
      r1 > rows || from % kCompactTileRows != 0 || r0 % kCompactTileRows != 0 || (r1 % kCompactTileRows != 0 && r1 != rows))
    return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((r1 - r0 + kCompactTileRows - 1) / kCompactTileRows);
  const int64_t n_words = (rows + 31) >> 5;
  const char* s = reinterpret_cast<const char*>(src);
  char* d = reinterpret_cast<char*>(dst);
#define TAVB_GATHER(V) hipLaunchKernelGGL(compact_gather_kernel<V>, dim3(blocks), dim3(kMaskThreads), 0, stream, s, d, bits, counts, rows, n_words, from, r0, r1, row_bytes)
  switch (compact_vector_bytes((uint64_t)row_bytes | reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst))) {
    case 16: TAVB_GATHER(uint4); break;
    case 8: TAVB_GATHER(uint2); break;
    case 4: TAVB_GATHER(uint32_t); break;
    default: TAVB_GATHER(uint16_t); break;
  }
#undef TAVB_GATHER
  return hipGetLastError();
}

hipError_t launch_compact_scatter(const void* staging, void* corpus, const uint32_t* bits, const unsigned* counts, int64_t rows, int64_t r0, int64_t r1,
                                  int64_t row_bytes, hipStream_t stream) {
  if (!staging || !corpus || !bits || !counts || rows < 1 || rows >= 0x7FFFFFFFll || row_bytes < 2 || row_bytes % 2 != 0 || r0 < 0 || r0 >= r1 || r1 > rows ||
      r0 % kCompactTileRows != 0 || (r1 % kCompactTileRows != 0 && r1 != rows))
    return hipErrorInvalidValue;
  const int vb = compact_vector_bytes((uint64_t)row_bytes | reinterpret_cast<uintptr_t>(staging) | reinterpret_cast<uintptr_t>(corpus));
  const int64_t most = (r1 - r0) * (row_bytes / vb);  // V's to copy when every row of the pass is kept
  const unsigned blocks = (unsigned)std::min<int64_t>((most + 4 * kMaskThreads - 1) / (4 * kMaskThreads), 2048);
  const int64_t n_words = (rows + 31) >> 5;
  const char* s = reinterpret_cast<const char*>(staging);
  char* d = reinterpret_cast<char*>(corpus);
#define TAVB_SCATTER(V) hipLaunchKernelGGL(compact_scatter_kernel<V>, dim3(blocks), dim3(kMaskThreads), 0, stream, s, d, bits, counts, rows, n_words, r0, r1, row_bytes)
  switch (vb) {
    case 16: TAVB_SCATTER(uint4); break;
    case 8: TAVB_SCATTER(uint2); break;
    case 4: TAVB_SCATTER(uint32_t); break;
    default: TAVB_SCATTER(uint16_t); break;
  }
#undef TAVB_SCATTER
  return hipGetLastError();
}

int mask_blocks(int64_t rows) { return (int)((rows + TAVB_MASK_ROWS_PER_WORKGROUP - 1) / TAVB_MASK_ROWS_PER_WORKGROUP); }

hipError_t launch_scope_member(const MaskOperands& ops, const int32_t* rows, int64_t n, int64_t n_rows, uint8_t* member, hipStream_t stream) {
  if (!rows || !member || n < 1 || n_rows < 1 || n_rows >= 0x7FFFFFFFll || ops.n < 1 || ops.n > TAVB_MAX_MASK_OPERANDS) return hipErrorInvalidValue;
  for (int j = 0; j < ops.n; ++j)
    if (!ops.m[j]) return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)std::min<int64_t>((n + kMaskThreads - 1) / kMaskThreads, 2048);
  hipLaunchKernelGGL(scope_member_kernel, dim3(blocks), dim3(kMaskThreads), 0, stream, ops, rows, n, n_rows, member);
  return hipGetLastError();
}

hipError_t launch_scope_planes(const ScopeMasks& ms, int n_blocks, int64_t rows, int64_t span_begin, int64_t last_row, int64_t stride, uint32_t* planes,
                               hipStream_t stream) {
  if (!planes || rows < 1 || rows >= 0x7FFFFFFFll || ms.n < 1 || ms.n > kScopePlaneMasks || n_blocks < (ms.n + 31) / 32 || n_blocks > kScopePlaneMasks / 32)
    return hipErrorInvalidValue;
  if (span_begin < 0 || span_begin % 32 != 0 || stride < 32 || stride % 32 != 0 || last_row < span_begin || last_row >= rows || last_row >= span_begin + stride)
    return hipErrorInvalidValue;
  for (int j = 0; j < ms.n; ++j)
    if (!ms.m[j]) return hipErrorInvalidValue;
  const int64_t items = ((stride + 63) >> 6) * n_blocks;
  const unsigned blocks = (unsigned)std::min<int64_t>((items + kMaskWaves - 1) / kMaskWaves, 4096);
  hipLaunchKernelGGL(scope_planes_kernel, dim3(blocks), dim3(kMaskThreads), 0, stream, ms, n_blocks, span_begin, last_row, stride, planes);
  return hipGetLastError();
}

hipError_t launch_mask_expand(const uint32_t* bits, int64_t rows, unsigned* counts, int32_t* out, int64_t cap, long long* total_out,
                              hipStream_t stream) {
  if (!bits || !counts || !total_out || rows < 1 || rows >= 0x7FFFFFFFll || cap < 0 || (cap > 0 && !out)) return hipErrorInvalidValue;
  const int64_t n_words = (rows + 31) >> 5;
  const int blocks = mask_blocks(rows);
  hipLaunchKernelGGL(mask_count_kernel, dim3(blocks), dim3(kMaskThreads), 0, stream, bits, rows, n_words, counts);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mask_write_kernel, dim3(blocks), dim3(kMaskThreads), 0, stream, bits, rows, n_words, counts, out, cap, total_out);
  return hipGetLastError();
}

hipError_t launch_mask_write(const uint32_t* bits, int64_t rows, const unsigned* counts, int32_t* out, int64_t cap, long long* total_out,
                             hipStream_t stream) {
  if (!bits || !counts || !total_out || rows < 1 || rows >= 0x7FFFFFFFll || cap < 0 || (cap > 0 && !out)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mask_write_kernel, dim3(mask_blocks(rows)), dim3(kMaskThreads), 0, stream, bits, rows, (rows + 31) >> 5, counts, out, cap, total_out);
  return hipGetLastError();
}

hipError_t launch_mask_from_ranges(const int32_t* intervals, const ScopeCollections& cols, const int32_t* row_to_msg, int64_t n_messages, int64_t rows,
                                   uint32_t* bits, unsigned* counts, MaskChunkInfo* info, hipStream_t stream) {
  if (!bits || !counts || !info || rows < 1 || rows >= 0x7FFFFFFFll || n_messages < 0 || cols.n < 0 || cols.n > TAVB_MAX_SCOPE_COLLECTIONS || cols.offset[0] != 0)
    return hipErrorInvalidValue;
  for (int c = 0; c < cols.n; ++c)
    if (cols.offset[c + 1] < cols.offset[c]) return hipErrorInvalidValue;
  const int total = cols.offset[cols.n];
  if (total > 0 && !intervals) return hipErrorInvalidValue;
  const int64_t n_words = (rows + 31) >> 5;
  const int2* iv = reinterpret_cast<const int2*>(intervals);
  if (total <= TAVB_SCOPE_LDS_RANGES)
    hipLaunchKernelGGL(mask_from_ranges_kernel<true>, dim3(mask_blocks(rows)), dim3(kMaskThreads), 0, stream, iv, cols, row_to_msg, n_messages, rows, n_words,
                       bits, counts, info);
  else
    hipLaunchKernelGGL(mask_from_ranges_kernel<false>, dim3(mask_blocks(rows)), dim3(kMaskThreads), 0, stream, iv, cols, row_to_msg, n_messages, rows, n_words,
                       bits, counts, info);
  return hipGetLastError();
}

hipError_t launch_mask_combine(const MaskOperands& ops, int64_t rows, uint32_t* bits, unsigned* counts, MaskChunkInfo* info, hipStream_t stream) {
  if (!bits || !counts || !info || rows < 1 || rows >= 0x7FFFFFFFll || ops.n < 1 || ops.n > TAVB_MAX_MASK_OPERANDS || ops.op < TAVB_MASK_AND ||
      ops.op > TAVB_MASK_ANDNOT)
    return hipErrorInvalidValue;
  for (int j = 0; j < ops.n; ++j)
    if (!ops.m[j]) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mask_combine_kernel, dim3(mask_blocks(rows)), dim3(kMaskThreads), 0, stream, ops, rows, (rows + 31) >> 5, bits, counts, info);
  return hipGetLastError();
}

static bool remap_operands_ok(const RemapOperands& ops, int64_t old_rows, int64_t new_rows) {
  if (ops.n < 1 || ops.n > TAVB_MAX_MASK_OPERANDS || old_rows < 0 || old_rows >= 0x7FFFFFFFll || new_rows < 1 || new_rows >= 0x7FFFFFFFll) return false;
  for (int j = 0; j < ops.n; ++j)
    if (!ops.out[j] || (old_rows > 0 && !ops.in[j])) return false;
  return true;
}

hipError_t launch_mask_remap_squeeze(const RemapOperands& ops, const uint32_t* flags, const unsigned* kept_counts, int64_t old_rows, int64_t new_rows,
                                     unsigned* counts, MaskChunkInfo* info, hipStream_t stream) {
  if (!remap_operands_ok(ops, old_rows, new_rows) || !flags || !kept_counts || !counts || !info || new_rows > old_rows) return hipErrorInvalidValue;
  const int64_t new_words = (new_rows + 31) >> 5;
  for (int j = 0; j < ops.n; ++j) {  // the kernel ORs into the words two chunks share
    hipError_t e = hipMemsetAsync(ops.out[j], 0, (size_t)new_words * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(mask_remap_squeeze_kernel, dim3(mask_blocks(old_rows)), dim3(kMaskThreads), 0, stream, ops, flags, kept_counts, old_rows, (old_rows + 31) >> 5,
                     new_words);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mask_remap_info_kernel, dim3(mask_blocks(new_rows), ops.n), dim3(kMaskThreads), 0, stream, ops, new_rows, new_words, counts, info);
  return hipGetLastError();
}

hipError_t launch_mask_remap_spread(const RemapOperands& ops, const uint32_t* flags, const unsigned* clear_counts, int64_t old_rows, int64_t new_rows, bool fill,
                                    unsigned* counts, MaskChunkInfo* info, hipStream_t stream) {
  if (!remap_operands_ok(ops, old_rows, new_rows) || (flags && !clear_counts) || !counts || !info || new_rows < old_rows) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mask_remap_spread_kernel, dim3(mask_blocks(new_rows)), dim3(kMaskThreads), 0, stream, ops, flags, clear_counts, old_rows, (old_rows + 31) >> 5,
                     new_rows, (new_rows + 31) >> 5, fill ? 1 : 0, counts, info);
  return hipGetLastError();
}

hipError_t launch_mask_pack(const uint8_t* bytes, int64_t rows, uint32_t* bits, hipStream_t stream) {
  if (!bytes || !bits || rows < 1 || rows >= 0x7FFFFFFFll) return hipErrorInvalidValue;
  const int64_t n_words = (rows + 31) >> 5;
  const int64_t groups = (rows + 63) >> 6;
  const int64_t blocks = std::min<int64_t>((groups + kMaskThreads / 64 - 1) / (kMaskThreads / 64), 2048);
  hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)blocks), dim3(kMaskThreads), 0, stream, bytes, rows, n_words, bits);
  return hipGetLastError();
}

hipError_t launch_mask_from_messages(const int32_t* row_to_msg, int64_t rows, const uint32_t* accept_bits, int64_t n_bits, uint32_t* bits,
                                     hipStream_t stream) {
  if (!row_to_msg || !accept_bits || !bits || rows < 1 || rows >= 0x7FFFFFFFll || n_bits < 0) return hipErrorInvalidValue;
  const int64_t groups = (rows + 63) >> 6;
  const int64_t blocks = std::min<int64_t>((groups + kMaskThreads / 64 - 1) / (kMaskThreads / 64), 2048);
  hipLaunchKernelGGL(mask_from_messages_kernel, dim3((unsigned)blocks), dim3(kMaskThreads), 0, stream, row_to_msg, rows, accept_bits, n_bits, bits);
  return hipGetLastError();
}

}  // namespace tavb
