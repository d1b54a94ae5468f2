// Near-duplicate self-join (tavb_join_pairs, tavb_lookup_pairs.hip): every pair of corpus rows i < j scoring at least min_score, found by
// the matrix cores over the UPPER TRIANGLE of X . X^T and scored exactly afterwards.
//
//   pairs_join_kernel     Both operands are the SAME fp16 matrix X16 -- the corpus itself (fp16 corpora) or its fp16 shadow (fp32 ones).
//                         A step is a 128 (rows i) x 128 (rows j) tile of X16 . X16^T: 256 threads, each of the four waves a 64 x 64 quarter
//                         as 2 x 2 blocks of v_mfma_f32_32x32x16_f16.  The K loop runs in steps of 64 halves through LDS, double buffered:
//                         two operands x two buffers x 16 KiB; the global loads of step s + 1 are issued before the MFMAs of step s and
//                         stored behind them, one barrier per step.  An LDS row is 128 bytes, its eight 16-byte chunks XORed with row & 7.
//                         Fragments: lane l (r = l & 31, h = l >> 5) holds A[row r][k = 8 h + e] and B[k = 8 h + e][col r], e = 0 .. 7 -- for
//                         both operands 16 bytes of row r at halves 8 h of the k16 slice; C[row][col]: col = l & 31, row = (reg & 3) +
//                         8 (reg >> 2) + 4 h.  Rows at or beyond N are loaded from row N - 1 (the buffer need not reach a tile multiple)
//                         and never admitted.
//                         TRIANGLE: only tile pairs tj >= ti, T = ceil(N / 128) tile rows.  Row ti has T - ti pairs; it is laid behind
//                         row T - 1 - ti, which has ti + 1: every folded row is T + 1 pairs long, the folded rows one after another are the
//                         work list, and a workgroup takes `per_wg` consecutive entries of it -- a contiguous range of j tiles of one i
//                         tile (of two where it crosses the fold).  Long rows are split, every workgroup has the same amount of work, none
//                         waits for another.
//                         EPILOGUE: s = cosine_to_score(acc); the pair is admitted when s >= thr, j > i (diagonal tiles), j < N and, with
//                         a mask, both rows' bits are set.  A wave counts its admissions, adds them to the global counter with ONE atomic
//                         and stores its (i, j) behind each other with plain vector stores; the counter keeps counting past the capacity
//                         and nothing is stored past it, so the host learns the size a retry needs.  A NaN score fails >=.  With a
//                         mask, a 128-row block whose four mask words are zero is skipped as a whole.
//   rescore_pairs_kernel  one wave per candidate: the exact score of row j against row i AS THE QUERY in the streaming kernels' arithmetic
//                         (dot_slice per 16-byte slice, lane l the slices l, l + 64, ..., then wave_sum: tavb_device.h).  Row i is read in
//                         place -- fp16 widened exactly, as rows_to_queries_kernel does; fp32 rows from the fp32 corpus -- no query batch
//                         is built.  Pairs with score >= min_score are compacted to (i, j, score): bit for bit what
//                         fuzzy_lookup_embedding(row i, 0, min_score) reports for row j.
//
// THE BOUND (one delta for the whole launch; tavb_rescore.hip's query_prepare_kernel with the query replaced by a corpus row).  The exact
// dot product of a pair is x_i . x_j over the stored rows, the filter's is x16_i . x16_j:
//     |x_i . x_j - x16_i . x16_j| <= |x_i . (x_j - x16_j)| + |(x_i - x16_i) . x16_j| <= E ||x_i|| + E R,
// R = max ||x16||, E = max ||x - x16|| over the rows (the cached maxima; E = 0 for fp16 corpora), ||x_i|| <= R + E.  In that kernel's terms
// the query's rounding err = ||q - q16||^2 <= E^2 and its norm qq = ||q||^2 <= (R + E)^2, and every term is kept:
//     delta = 0.5 ( E R 1.0001                                  the query's rounding against a shadow row
//                 + E (R + E) 1.0001                            the row's rounding against the query
//                 + 2 (dim / 8 + 8) 2^-24 (R + E) (R + E) )     summation slack of two fp32 dot products (blocked accumulation)
//             + 1.2e-7                                           the score's own rounding ((c + 1) / 2)
// in score units (a score is half a dot product).  thr = min_score - 2 delta, one ulp down, -inf when that is not positive
// (pairs_join_threshold in tavb_internal.h, on the host: the maxima are read back once).  A pair with exact score >= min_score has an
// approximate score >= min_score - delta >= thr: the candidates hold every answer.  delta not finite: nothing can be proven, the caller
// takes the lookup route.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "tavb_device.h"
#include "tavb_internal.h"

namespace tavb {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 128;     // rows of either operand per step
constexpr int kBK = 64;        // halves per K step
constexpr int kRowBytes = kBK * 2;
constexpr int kOperandBytes = kTile * kRowBytes;  // 16 KiB

__device__ __forceinline__ int lds_offset(int row, int chunk) { return row * kRowBytes + ((chunk ^ (row & 7)) << 4); }

__device__ __forceinline__ bool block_has_rows(const uint32_t* __restrict__ mask, int64_t n_words, int64_t tile) {
  uint32_t any = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int64_t idx = tile * 4 + w;
    if (idx < n_words) any |= mask[idx];
  }
  return any != 0;
}

__global__ void __launch_bounds__(256) pairs_join_kernel(const PairsJoinParams p) {
  __shared__ __align__(16) unsigned char lds[2][2][kOperandBytes];  // [buffer][operand i / j]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 1, wc = wave & 1;  // the wave's 64 x 64 quarter: rows i 64 wr .., rows j 64 wc ..
  const _Float16* __restrict__ X = reinterpret_cast<const _Float16*>(p.rows16);
  const int64_t N = p.n, T = p.n_tiles;
  const int dim = p.dim, steps = dim / kBK;
  const int64_t n_words = (N + 31) >> 5;
  const int64_t w_begin = (int64_t)blockIdx.x * p.per_wg;
  const int64_t w_end = (w_begin + p.per_wg < p.work) ? w_begin + p.per_wg : p.work;

  // staging: thread t moves the 16-byte chunks t, t + 256, t + 512, t + 768 of a 128 x 64 operand tile (chunk q: row q >> 3, chunk q & 7)
  int st_row[4], st_off[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int q = threadIdx.x + 256 * u;
    st_row[u] = q >> 3;
    st_off[u] = lds_offset(q >> 3, q & 7);
  }
  const int st_col = (threadIdx.x & 7) * 8;  // (q & 7 is the same for the four: 256 is a multiple of 8)

  for (int64_t w = w_begin; w < w_end; ++w) {
    // the work list: folded row y holds tile row y (T - y pairs), then tile row T - 1 - y (y + 1 pairs)
    const int64_t y = w / (T + 1), pos = w - y * (T + 1);
    int64_t ti = y, tj;
    if (pos < T - y) {
      tj = ti + pos;
    } else {
      ti = T - 1 - y;
      if (ti == y) continue;  // (T odd: the middle row is folded onto itself)
      tj = ti + (pos - (T - y));
    }
    if (p.mask != nullptr && !(block_has_rows(p.mask, n_words, ti) && block_has_rows(p.mask, n_words, tj))) continue;  // (block-uniform)
    const int64_t i0 = ti * kTile, j0 = tj * kTile;

    const _Float16* src_i[4];
    const _Float16* src_j[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t ri = i0 + st_row[u], rj = j0 + st_row[u];
      src_i[u] = X + (size_t)(ri < N ? ri : N - 1) * dim + st_col;
      src_j[u] = X + (size_t)(rj < N ? rj : N - 1) * dim + st_col;
    }
    f16x8 ra[4], rb[4];
    auto load_global = [&](int s) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ra[u] = *reinterpret_cast<const f16x8*>(src_i[u] + s * kBK);
        rb[u] = *reinterpret_cast<const f16x8*>(src_j[u] + s * kBK);
      }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        *reinterpret_cast<f16x8*>(&lds[buf][0][st_off[u]]) = ra[u];
        *reinterpret_cast<f16x8*>(&lds[buf][1][st_off[u]]) = rb[u];
      }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    load_global(0);
    store_lds(0);
    __syncthreads();
    const int fr = lane & 31, fh = lane >> 5;
    for (int s = 0; s < steps; ++s) {
      const int buf = s & 1;
      if (s + 1 < steps) load_global(s + 1);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        f16x8 a[2], b[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          a[m] = *reinterpret_cast<const f16x8*>(&lds[buf][0][lds_offset(64 * wr + 32 * m + fr, 2 * kk + fh)]);
          b[m] = *reinterpret_cast<const f16x8*>(&lds[buf][1][lds_offset(64 * wc + 32 * m + fr, 2 * kk + fh)]);
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
      }
      if (s + 1 < steps) store_lds(buf ^ 1);
      __syncthreads();  // the next step's tile is written, this step's is read: the buffer after next may be overwritten
    }

    // epilogue: bit (mi * 2 + ni) * 16 + reg of `mine` = this lane admits that accumulator element
    const int64_t wi = i0 + 64 * wr + 4 * fh, wj = j0 + 64 * wc + fr;
    if (wj - fr + 63 <= wi - 4 * fh) continue;  // (wave-uniform: every j of the quarter is at or below every i -- the lower quarter of a diagonal tile)
    u64 mine = 0;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float s = cosine_to_score(acc[mi][ni][r]);
          const int64_t i = wi + 32 * mi + (r & 3) + 8 * (r >> 2), j = wj + 32 * ni;
          if (s >= p.thr && j > i && j < N) mine |= 1ull << ((mi * 2 + ni) * 16 + r);
        }
    if (p.mask != nullptr) {
      u64 left = mine;
      while (left) {
        const int b = __ffsll((long long)left) - 1;
        left &= left - 1;
        const int q = b >> 4, r = b & 15;
        const int64_t i = wi + 32 * (q >> 1) + (r & 3) + 8 * (r >> 2), j = wj + 32 * (q & 1);
        if (!((p.mask[i >> 5] >> (i & 31)) & (p.mask[j >> 5] >> (j & 31)) & 1u)) mine &= ~(1ull << b);
      }
    }
    const int n_mine = __popcll(mine);
    if (__ballot(n_mine != 0) == 0) continue;  // (wave-uniform)
    int incl = n_mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d, kWave);
      if (lane >= d) incl += t;
    }
    const int total = __shfl(incl, 63, kWave);
    u64 base = 0;
    if (lane == 0) base = atomicAdd(p.counter, (u64)total);
    base = shfl_u64(base, 0);
    u64 at = base + (u64)(incl - n_mine);
    while (mine) {
      const int b = __ffsll((long long)mine) - 1;
      mine &= mine - 1;
      const int q = b >> 4, r = b & 15;
      const int64_t i = wi + 32 * (q >> 1) + (r & 3) + 8 * (r >> 2), j = wj + 32 * (q & 1);
      if (at < p.capacity) p.cand[at] = make_uint2((uint32_t)i, (uint32_t)j);
      ++at;
    }
  }
}

// counters[0]: the candidates the join counted (more than `capacity`: they did not fit, nothing is scored); counters[1]: the pairs kept
template <typename T>
__global__ void __launch_bounds__(256) rescore_pairs_kernel(const T* __restrict__ corpus, int dim, u64* __restrict__ counters, u64 capacity,
                                                            const uint2* __restrict__ cand, float min_score, uint32_t* __restrict__ out_i,
                                                            uint32_t* __restrict__ out_j, float* __restrict__ out_s) {
  constexpr int EPL = Elem<T>::EPL;
  const int lane = threadIdx.x & 63;
  const u64 n = counters[0];
  if (n > capacity) return;
  const u64 n_waves = (u64)gridDim.x * (blockDim.x >> 6);
  const int n_slices = dim / EPL;
  for (u64 c = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); c < n; c += n_waves) {
    const uint2 pr = cand[c];  // wave-uniform
    const T* xi = corpus + (size_t)pr.x * dim;  // the query
    const T* xj = corpus + (size_t)pr.y * dim;  // the row
    float acc = 0.f;
    for (int sl = lane; sl < n_slices; sl += 64) {
      const f32x4 raw = *reinterpret_cast<const f32x4*>(xj + (size_t)sl * EPL);
      float qf[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) qf[e] = (float)xi[(size_t)sl * EPL + e];  // fp16: widened exactly
      acc = dot_slice<T>(raw, qf, acc);
    }
    const float s = cosine_to_score(wave_sum(acc));
    if (lane == 0 && s >= min_score) {
      const u64 at = atomicAdd(counters + 1, 1ull);
      out_i[at] = pr.x;
      out_j[at] = pr.y;
      out_s[at] = s;
    }
  }
}

}  // namespace

bool pairs_join_supported(int dim) { return mfma_supported(dim, 1); }

hipError_t launch_pairs_join(PairsJoinParams p, int n_cu, hipStream_t stream) {
  if (!p.rows16 || !p.counter || !p.cand || p.n < 2 || p.n >= 0x7FFFFFFFll || !pairs_join_supported(p.dim) || (reinterpret_cast<uintptr_t>(p.rows16) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(p.mask) & 3) != 0)
    return hipErrorInvalidValue;
  p.n_tiles = (p.n + kTile - 1) / kTile;
  p.work = ((p.n_tiles + 1) / 2) * (p.n_tiles + 1);
  // sixteen workgroups per compute unit where the triangle has them (two are resident at 64 KiB of LDS each); never more than 2^30 workgroups
  const int64_t target = (int64_t)(n_cu > 0 ? n_cu : 256) * 16;
  int64_t per_wg = std::min<int64_t>((p.work + target - 1) / target, 256);
  per_wg = std::max<int64_t>(per_wg, (p.work + ((int64_t)1 << 30) - 1) >> 30);
  p.per_wg = std::max<int64_t>(per_wg, 1);
  const int64_t blocks = (p.work + p.per_wg - 1) / p.per_wg;
  hipLaunchKernelGGL(pairs_join_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_rescore_pairs(const void* corpus, bool f32_rows, int dim, unsigned long long* counters, unsigned long long capacity, const void* cand,
                                float min_score, uint32_t* out_i, uint32_t* out_j, float* out_s, int n_cu, hipStream_t stream) {
  if (!corpus || !counters || !cand || !out_i || !out_j || !out_s || dim % 8 != 0 || capacity < 1) return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)std::min<unsigned long long>((capacity + 3) / 4, (unsigned long long)(n_cu > 0 ? n_cu : 256) * 8);
  if (f32_rows)
    hipLaunchKernelGGL(rescore_pairs_kernel<float>, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const float*>(corpus), dim, counters, capacity,
                       reinterpret_cast<const uint2*>(cand), min_score, out_i, out_j, out_s);
  else
    hipLaunchKernelGGL(rescore_pairs_kernel<_Float16>, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const _Float16*>(corpus), dim, counters, capacity,
                       reinterpret_cast<const uint2*>(cand), min_score, out_i, out_j, out_s);
  return hipGetLastError();
}

}  // namespace tavb
