// Exact top-k for k beyond the fused selection (TAVB_MAX_FUSED_K < k <= TAVB_MAX_LARGE_K), after ONE corpus pass.
//
// The score pass (launch_scan_topk, tavb_scan.hip) leaves, per query, the score bits of every row (kScoreNone for rows below min_score)
// and a histogram of the passing scores in `buckets` linear buckets over [max(min_score, 0), 1].  From there, with no host round trip:
//   boundary   the bucket b* where the count from the top first reaches need = min(k, survivors): every key above it is a sure hit
//              (fewer than need of them), the keys inside it hold the rest.  Recomputed by every workgroup that needs it (a few
//              thousand L2-resident counters, one wave) instead of a launch of its own.
//   refine     while b* holds more keys than the boundary list takes (`cap`): the keys inside it -- a range of 64-bit keys, score bits
//              and position -- are counted again in kTopkRefineBuckets sub-ranges, read from the score array, and the boundary moves
//              into the sub-range where the count reaches need.  Every round divides the range by 4096, so a fixed number of rounds
//              (topk_refine_rounds, enqueued up front; a round whose query already fits returns at once) ends with at most `cap` keys
//              whatever the data: 5000 identical rows need three.
//   compact    keys above the range -> the sure list, keys inside it -> the boundary list (wave-aggregated appends).
//   finish     one workgroup per query: the sure keys sorted (bitonic, LDS), then the best need - sure of the boundary keys (sorted the
//              same way: every boundary key ranks below every sure key), written straight into the caller's pinned [nq, k] keys.
// Keys are (score bits << 32) | (0xFFFFFFFF - position): unique, so the boundary search always ends and equal scores order by
// ascending position, as everywhere in this library.
//
// Also here: the merge of long sorted lists (merge_topk_kernel), which puts the lists of several shards -- each the output of the passes
// above -- together for k beyond what the register merge of tavb_misc.hip holds, and the first half of the merge of top-messages lists
// (message_keys_max_kernel), whose keys are not unique across shards: one maximum per message, then the selection above.

#include "tavb_device.h"
#include "tavb_internal.h"

namespace tavb {

namespace {

constexpr int kB2 = kTopkRefineBuckets;
constexpr uint32_t kOneBits = 0x3F800000u;  // 1.0f: the largest score

struct TopkState {
  u64 ka, kb;      // the boundary range of keys (inclusive)
  unsigned above;  // keys above kb: the sure hits
  unsigned inb;    // keys inside [ka, kb]
  unsigned need;   // min(k, survivors)
  int rounds;      // refinement rounds applied
  int empty;       // no survivor at all
};

// Workspace: hist [nq][buckets] | rhist [rounds][nq][kB2] | cnt [nq][4] | meta [nq][4]  (the head, zeroed before the score pass)
//            | sure [nq][k] | bnd [nq][cap]
struct Layout {
  unsigned* hist;
  unsigned* rhist;
  unsigned* cnt;  // [q][0] sure keys, [q][1] boundary keys
  int* meta;      // [q][0] need, [q][1] refinement rounds
  u64* sure;
  u64* bnd;
};

__host__ __device__ inline size_t head_bytes(int nq, int buckets, int rounds) {
  const size_t words = (size_t)nq * buckets + (size_t)rounds * nq * kB2 + (size_t)nq * 8;
  return (words * 4 + 255) & ~(size_t)255;
}

__host__ __device__ inline Layout layout(const TopkLaunch& t) {
  Layout l;
  unsigned* w = reinterpret_cast<unsigned*>(t.workspace);
  l.hist = w;
  l.rhist = l.hist + (size_t)t.nq * t.buckets;
  l.cnt = l.rhist + (size_t)t.rounds * t.nq * kB2;
  l.meta = reinterpret_cast<int*>(l.cnt + (size_t)t.nq * 4);
  l.sure = reinterpret_cast<u64*>(reinterpret_cast<char*>(t.workspace) + head_bytes(t.nq, t.buckets, t.rounds));
  l.bnd = l.sure + (size_t)t.nq * t.k;
  return l;
}

// One wave: in h[0 .. n) (n a multiple of 64, counts per bucket, bucket n - 1 the best), the bucket j where the count from the top first
// reaches `need` (1 <= need <= total): *above = keys in buckets above j, *in = keys in j.  Lane l sums buckets [n - (l+1) n/64, n - l n/64).
__device__ void find_from_top(const unsigned* __restrict__ h, int n, unsigned need, int lane, int* j_out, unsigned* above_out, unsigned* in_out,
                              unsigned* total_out) {
  const int per = n / 64;
  const int top = n - lane * per;
  unsigned sum = 0;
  for (int b = top - per; b < top; ++b) sum += h[b];
  unsigned pre = sum;  // inclusive prefix over lanes 0 .. lane
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned t = __shfl_up(pre, d, 64);
    if (lane >= d) pre += t;
  }
  const unsigned total = __shfl(pre, 63, 64);
  const unsigned long long hit = __ballot(pre >= need);
  const int L = hit ? __ffsll(hit) - 1 : 63;
  unsigned cum = __shfl(pre - sum, L, 64);
  const int topL = n - L * per;
  int j = topL - per;
  unsigned above = cum, in = 0;
  for (int b = topL - 1; b >= topL - per; --b) {  // (the same walk in every lane)
    const unsigned v = h[b];
    if (cum + v >= need) {
      j = b;
      above = cum;
      in = v;
      break;
    }
    cum += v;
  }
  *j_out = j;
  *above_out = above;
  *in_out = in;
  *total_out = total;
}

// smallest score bits x in [0, 1.0f] whose bucket is >= target (kOneBits + 1 when there is none)
__device__ uint32_t first_bits_at_least(int target, float lo, float scale, int nb) {
  uint32_t a = 0, b = kOneBits + 1;
  while (a < b) {
    const uint32_t m = a + (b - a) / 2;
    if (topk_bucket(__uint_as_float(m), lo, scale, nb) >= target)
      b = m;
    else
      a = m + 1;
  }
  return a;
}

// The boundary of query q after `rounds` refinement rounds (fewer when it fits `cap` sooner).  One wave, every lane gets the result.
__device__ TopkState resolve(const TopkLaunch& t, const Layout& l, int q, int rounds, int lane) {
  TopkState s{};
  int j;
  unsigned above, in, total;
  const unsigned* h0 = l.hist + (size_t)q * t.buckets;
  // total first (need = min(k, total)), then the search with that need
  find_from_top(h0, t.buckets, 0xFFFFFFFFu, lane, &j, &above, &in, &total);
  if (total == 0) {
    s.empty = 1;
    s.ka = 1;
    s.kb = 0;
    return s;
  }
  s.need = total < (unsigned)t.k ? total : (unsigned)t.k;
  find_from_top(h0, t.buckets, s.need, lane, &j, &above, &in, &total);
  const float lo = t.lo[q], scale = t.scale[q];
  const uint32_t a = first_bits_at_least(j, lo, scale, t.buckets);
  const uint32_t b = first_bits_at_least(j + 1, lo, scale, t.buckets) - 1;
  s.ka = (u64)a << 32;
  s.kb = ((u64)b << 32) | 0xFFFFFFFFull;
  s.above = above;
  s.inb = in;
  for (int r = 0; r < rounds && s.inb > (unsigned)t.cap; ++r) {
    const u64 w = s.kb - s.ka + 1;
    const u64 step = w / kB2 + (w % kB2 != 0);
    find_from_top(l.rhist + ((size_t)r * t.nq + q) * kB2, kB2, s.need - s.above, lane, &j, &above, &in, &total);
    const u64 ka = s.ka + (u64)j * step;
    const u64 kb = ka + step - 1;
    s.ka = ka;
    s.kb = kb < s.kb ? kb : s.kb;
    s.above += above;
    s.inb = in;
    s.rounds = r + 1;
  }
  return s;
}

__device__ __forceinline__ u64 row_key(uint32_t bits, int64_t pos) { return ((u64)bits << 32) | (u64)(0xFFFFFFFFu - (uint32_t)pos); }

__global__ void __launch_bounds__(256) topk_refine_kernel(const TopkLaunch t, int round) {
  __shared__ unsigned lh[kB2];
  __shared__ TopkState st;
  const Layout l = layout(t);
  const int q = blockIdx.y;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < 64) {
    const TopkState s = resolve(t, l, q, round, lane);
    if (lane == 0) st = s;
  }
  for (int i = threadIdx.x; i < kB2; i += blockDim.x) lh[i] = 0u;
  __syncthreads();
  const TopkState s = st;
  if (s.empty || s.inb <= (unsigned)t.cap) return;  // (the whole workgroup: this query's boundary fits already)
  const u64 w = s.kb - s.ka + 1;
  const u64 step = w / kB2 + (w % kB2 != 0);
  const unsigned* __restrict__ sc = t.scores + (size_t)q * t.n_pos;
  for (int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pos < t.n_pos; pos += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t v = sc[pos];
    if (v == kScoreNone) continue;
    const u64 key = row_key(v, pos);
    if (key >= s.ka && key <= s.kb) atomicAdd(&lh[(key - s.ka) / step], 1u);
  }
  __syncthreads();
  unsigned* gh = l.rhist + ((size_t)round * t.nq + q) * kB2;
  for (int i = threadIdx.x; i < kB2; i += blockDim.x) {
    const unsigned v = lh[i];
    if (v) atomicAdd(&gh[i], v);
  }
}

// ---- top-messages lookups (tavb_search_top_messages): the score pass left best [nq][n_pos] -- n_pos = n_messages, position = message ordinal
// -- holding 1 + the score bits of each message's best passing row, 0 for a message none of whose rows passed (MessageMaxSink,
// tavb_scan.hip).  The pass could not count: a message's value kept rising.  This one decodes every slot in place (`slot - 1`: the bits, and
// 0 becomes kScoreNone) and counts the messages that have a score into the workspace's histograms -- LDS histogram, nonzero buckets flushed
// with atomics, topk_bucket over the same lo / scale a score pass would use -- so that what follows (resolve, refine, compact, finish) finds
// what the ScoreSink leaves over rows, and runs unchanged.
constexpr int kMessageHistBuckets = 4096;  // the most "topk_buckets" allows

__global__ void __launch_bounds__(256) message_hist_kernel(const TopkLaunch t, unsigned* __restrict__ best) {
  __shared__ unsigned lh[kMessageHistBuckets];
  const Layout l = layout(t);
  const int q = blockIdx.y;
  const int nb = t.buckets;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) lh[i] = 0u;
  __syncthreads();
  const float lo = t.lo[q], scale = t.scale[q];
  unsigned* __restrict__ sc = best + (size_t)q * t.n_pos;
  for (int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pos < t.n_pos; pos += (int64_t)gridDim.x * blockDim.x) {
    const unsigned v = sc[pos];
    const uint32_t bits = v - 1u;  // (0 -> kScoreNone)
    sc[pos] = bits;
    if (v) atomicAdd(&lh[topk_bucket(__uint_as_float(bits), lo, scale, nb)], 1u);
  }
  __syncthreads();
  unsigned* gh = l.hist + (size_t)q * nb;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) {
    const unsigned v = lh[i];
    if (v) atomicAdd(&gh[i], v);
  }
}

// append `key` (where `flag`) to list[0 .. limit) through *counter: one atomic per wave (all 64 lanes must be here)
__device__ __forceinline__ void wave_append(bool flag, u64 key, unsigned* counter, u64* list, unsigned limit, int lane) {
  const unsigned long long m = __ballot(flag);
  if (!m) return;
  unsigned base = 0;
  if (lane == 0) base = atomicAdd(counter, (unsigned)__popcll(m));
  base = __shfl(base, 0, 64);
  if (flag) {
    const unsigned idx = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (idx < limit) list[idx] = key;
  }
}

__global__ void __launch_bounds__(256) topk_compact_kernel(const TopkLaunch t) {
  __shared__ TopkState st;
  const Layout l = layout(t);
  const int q = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (threadIdx.x < 64) {
    const TopkState s = resolve(t, l, q, t.rounds, lane);
    if (lane == 0) {
      st = s;
      if (blockIdx.x == 0) {
        l.meta[q * 4 + 0] = (int)s.need;
        l.meta[q * 4 + 1] = s.rounds;
      }
    }
  }
  __syncthreads();
  const TopkState s = st;
  if (s.empty) return;
  const unsigned* __restrict__ sc = t.scores + (size_t)q * t.n_pos;
  u64* sure = l.sure + (size_t)q * t.k;
  u64* bnd = l.bnd + (size_t)q * t.cap;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + wave * 64; base < t.n_pos; base += stride) {  // wave-uniform trip count
    const int64_t pos = base + lane;
    const uint32_t v = pos < t.n_pos ? sc[pos] : kScoreNone;
    const u64 key = row_key(v, pos);
    const bool live = v != kScoreNone;
    // (keys leave with index_base added to their position: the same amount off the low half of every key, no borrow -- the order stays)
    wave_append(live && key > s.kb, key - t.index_base, &l.cnt[q * 4 + 0], sure, (unsigned)t.k, lane);
    wave_append(live && key >= s.ka && key <= s.kb, key - t.index_base, &l.cnt[q * 4 + 1], bnd, (unsigned)t.cap, lane);
  }
}

// ---- the sorted route (tavb_search_sorted): the same boundary for need = min(k, survivors) -- k = n_pos for every survivor, then with
// no refinement: the boundary bucket is the lowest non-empty one -- and then EVERY key at or above the boundary range's lower end
// (the sure keys and the whole boundary range: need .. need + topk_boundary_keys keys after refinement), in ascending position order.
// Block b of a query owns positions [b * chunk, (b + 1) * chunk): sorted_count counts its keys, sorted_compact writes them at the sum
// of the counts of blocks < b -- no atomic appends, so the keys leave in position order, i.e. descending in their low 32 bits, and a
// stable sort on the score bits alone (tavb_sort.hip, first_pass 4) orders them as the keys themselves order.

struct SortedState {
  u64 ka;
  int empty;
};

__device__ SortedState sorted_state(const TopkLaunch& t, const Layout& l, int q, int lane, bool note) {
  const TopkState s = resolve(t, l, q, t.rounds, lane);
  if (note && lane == 0) {
    l.meta[q * 4 + 0] = s.empty ? 0 : (int)s.need;
    l.meta[q * 4 + 1] = s.rounds;
  }
  return SortedState{s.ka, s.empty};
}

__global__ void __launch_bounds__(256) sorted_count_kernel(const TopkLaunch t, int64_t chunk, unsigned* counts /*[nq][blocks]*/) {
  __shared__ SortedState st;
  __shared__ unsigned total;
  const Layout l = layout(t);
  const int q = blockIdx.y;
  if (threadIdx.x < 64) {
    const SortedState s = sorted_state(t, l, q, threadIdx.x, blockIdx.x == 0);
    if (threadIdx.x == 0) {
      st = s;
      total = 0u;
    }
  }
  __syncthreads();
  const SortedState s = st;
  unsigned n = 0;
  if (!s.empty) {
    const unsigned* __restrict__ sc = t.scores + (size_t)q * t.n_pos;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = lo + chunk < t.n_pos ? lo + chunk : t.n_pos;
    for (int64_t pos = lo + threadIdx.x; pos < hi; pos += blockDim.x) {
      const uint32_t v = sc[pos];
      n += (v != kScoreNone && row_key(v, pos) >= s.ka) ? 1u : 0u;
    }
  }
  if (n) atomicAdd(&total, n);
  __syncthreads();
  if (threadIdx.x == 0) counts[(size_t)q * gridDim.x + blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) sorted_compact_kernel(const TopkLaunch t, int q, int64_t chunk, const unsigned* counts, u64* out) {
  __shared__ SortedState st;
  __shared__ unsigned start_sh;
  __shared__ unsigned wc[4];
  const Layout l = layout(t);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < 64) {
    const SortedState s = sorted_state(t, l, q, lane, false);
    if (lane == 0) {
      st = s;
      start_sh = 0u;
    }
  }
  __syncthreads();
  {  // where this block's keys start: the counts of the blocks before it
    const unsigned* c = counts + (size_t)q * gridDim.x;
    unsigned part = 0;
    for (unsigned b = threadIdx.x; b < blockIdx.x; b += blockDim.x) part += c[b];
    if (part) atomicAdd(&start_sh, part);
  }
  __syncthreads();
  const SortedState s = st;
  if (s.empty) return;
  unsigned base = start_sh;
  const unsigned* __restrict__ sc = t.scores + (size_t)q * t.n_pos;
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < t.n_pos ? lo + chunk : t.n_pos;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t tile = lo; tile < hi; tile += blockDim.x) {  // (block-uniform trip count)
    const int64_t pos = tile + threadIdx.x;
    const uint32_t v = pos < hi ? sc[pos] : kScoreNone;
    const u64 key = row_key(v, pos);
    const bool keep = v != kScoreNone && key >= s.ka;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wc[wave] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int w = 0; w < 4; ++w) {
      before += w < wave ? wc[w] : 0u;
      all += wc[w];
    }
    if (keep) out[base + before + (unsigned)__popcll(m & below)] = key;
    base += all;
    __syncthreads();  // (wc is rewritten by the next tile)
  }
}

__global__ void __launch_bounds__(1024) topk_finish_kernel(const TopkLaunch t) {
  extern __shared__ __align__(16) unsigned char smem[];
  u64* sk = reinterpret_cast<u64*>(smem);
  const Layout l = layout(t);
  const int q = blockIdx.x;
  const unsigned need = (unsigned)l.meta[q * 4 + 0];
  const unsigned n_sure = min(l.cnt[q * 4 + 0], need);
  const unsigned n_bnd = min(l.cnt[q * 4 + 1], (unsigned)t.cap);
  const unsigned take = min(need - n_sure, n_bnd);
  u64* out = t.out_keys + (size_t)q * t.k;
  block_sort_desc(l.sure + (size_t)q * t.k, (int)n_sure, sk, out, (int)n_sure);
  block_sort_desc(l.bnd + (size_t)q * t.cap, (int)n_bnd, sk, out + n_sure, (int)take);
  for (int i = (int)(n_sure + take) + threadIdx.x; i < t.k; i += blockDim.x) out[i] = 0ull;
  if (threadIdx.x == 0) t.out_rounds[q] = l.meta[q * 4 + 1];
}

// ---- merge of long sorted lists (launch_merge_topk): every key of the n_lists x k input finds its own place.  Real keys are unique (their
// low half is a global ordinal or position), so the final rank of a key is its position in its own list plus, for every other list, the
// number of keys greater than it -- a binary search of at most 15 steps in an L2-resident list -- and a key of rank < k is stored at
// out[rank]: no sort, no atomics, no waiting between workgroups, and one query spreads over as many workgroups as its keys ask for.
// Most keys never search: with j = ceil(k / n_lists) and m = ceil(k / j), the m-th largest of the lists' j-th keys has at least k keys at or
// above it (the bound of tavb_merge_keys_host), so whatever is smaller cannot rank.  The first wave of every workgroup works that bound out
// again (n_lists loads and a count over the lanes), together with the number of real keys in all (slots past it are zeroed: zeros are
// padding and never rank) and whether a list leads with TAVB_KEY_PEER_FAILED (then the whole output row is that key: duplicates of it would
// break the rank arithmetic, and no rank may take such a row for an answer).
constexpr u64 kPeerFailed = ~0ull;
constexpr int kMergeTopkPerThread = 4;

// keys greater than x among L[0 .. hi), L sorted descending
__device__ __forceinline__ int count_greater(const u64* __restrict__ L, int hi, u64 x) {
  int lo = 0;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (L[mid] > x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256) merge_topk_kernel(const u64* __restrict__ lists, int n_lists, int nq, int k, int query_major,
                                                         u64* __restrict__ out) {
  __shared__ u64 floor_sh;
  __shared__ int total_sh, failed_sh;
  const int q = blockIdx.y;
  const size_t stride = query_major ? (size_t)k : (size_t)nq * k;  // from one list of this query to the next
  const u64* __restrict__ base = lists + (query_major ? (size_t)q * n_lists * k : (size_t)q * k);
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const int j = (k + n_lists - 1) / n_lists;
    const int m = (k + j - 1) / j;  // <= n_lists
    const bool live = lane < n_lists;
    const u64* __restrict__ L = base + (size_t)(live ? lane : 0) * stride;
    const u64 head = live ? L[0] : 0ull;
    const u64 jth = live ? L[j - 1] : 0ull;
    int total = live ? count_greater(L, k, 0ull) : 0;  // real keys of this lane's list
    int at_least = 0;
    for (int d = 0; d < n_lists; ++d) at_least += __shfl(jth, d, 64) >= jth ? 1 : 0;
    u64 t = (live && at_least >= m) ? jth : 0ull;  // the largest of these is the m-th largest j-th key
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const u64 o = __shfl_xor(t, d, 64);
      t = o > t ? o : t;
      total += __shfl_xor(total, d, 64);
    }
    const unsigned long long failed = __ballot(head == kPeerFailed);
    if (lane == 0) {
      floor_sh = t > 1ull ? t : 1ull;  // (0 = fewer than k real keys: every real key ranks)
      total_sh = total < k ? total : k;
      failed_sh = failed != 0ull;
    }
  }
  __syncthreads();
  const u64 floor = floor_sh;
  const int total = total_sh;
  const bool failed = failed_sh != 0;
  const int n_keys = n_lists * k;
  u64* __restrict__ o = out + (size_t)q * k;
#pragma unroll
  for (int r = 0; r < kMergeTopkPerThread; ++r) {
    const int e = (blockIdx.x * kMergeTopkPerThread + r) * 256 + threadIdx.x;
    if (e >= n_keys) break;
    if (e < k) {  // the slots no key will claim
      if (failed)
        o[e] = kPeerFailed;
      else if (e >= total)
        o[e] = 0ull;
    }
    if (failed) continue;
    const int l = e / k, i = e - l * k;
    const u64 key = base[(size_t)l * stride + i];
    if (key < floor) continue;
    int rank = i;
    for (int other = 0; other < n_lists && rank < k; ++other)
      if (other != l) rank += count_greater(base + (size_t)other * stride, k - rank, key);  // (searching k - rank keys is enough to learn rank >= k)
    if (rank < k) o[rank] = key;
  }
}

// ---- merge of top-messages lists (launch_message_keys_max + the selection of a top-messages lookup): the lists of several shards carry
// MESSAGE ordinals, and a message whose chunks lie on two shards stands in two lists with two scores -- the rank arithmetic above does not
// hold.  Every non-zero key instead raises best[q][message] to its score, in the MessageMaxSink's encoding (1 + score bits over an array the
// caller zeroed; a plain load in front skips the atomic where the slot holds as much already: slots only rise), and what follows is the
// second half of a top-messages lookup as it stands (message_hist_kernel, refinement, compaction, finish).  A max does not depend on the
// order of its operands: the result is deterministic.  A key whose message is at or beyond n_messages, or whose score bits exceed 1.0f's,
// is dropped -- nothing is ever written outside [0, n_messages).  The first wave of every workgroup works out whether a list of the query
// leads with TAVB_KEY_PEER_FAILED: such a query scatters nothing (its selection finds no message) and block 0 raises flags[q], by which
// fill_keys_kernel writes the failure key into every slot of its row afterwards; flags[q] is written for every query, 0 or 1.
// Query q of the launch is query q0 + q of the lists.
__global__ void __launch_bounds__(256) message_keys_max_kernel(const u64* __restrict__ lists, int n_lists, int nq, int k, int query_major, int q0,
                                                               int64_t n_messages, unsigned* __restrict__ best, unsigned* __restrict__ flags) {
  __shared__ int failed_sh;
  const int q = blockIdx.y;
  const int gq = q0 + q;
  const size_t stride = query_major ? (size_t)k : (size_t)nq * k;  // from one list of this query to the next
  const u64* __restrict__ base = lists + (query_major ? (size_t)gq * n_lists * k : (size_t)gq * k);
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const u64 head = lane < n_lists ? base[(size_t)lane * stride] : 0ull;
    const unsigned long long failed = __ballot(head == kPeerFailed);
    if (lane == 0) {
      failed_sh = failed != 0ull;
      if (blockIdx.x == 0) flags[q] = failed != 0ull ? 1u : 0u;
    }
  }
  __syncthreads();
  if (failed_sh) return;  // (the whole workgroup)
  const int n_keys = n_lists * k;
  unsigned* __restrict__ b = best + (size_t)q * n_messages;
#pragma unroll
  for (int r = 0; r < kMergeTopkPerThread; ++r) {
    const int e = (blockIdx.x * kMergeTopkPerThread + r) * 256 + threadIdx.x;
    if (e >= n_keys) break;
    const int l = e / k, i = e - l * k;
    const u64 key = base[(size_t)l * stride + i];
    if (key == 0ull) continue;  // padding
    const uint32_t bits = (uint32_t)(key >> 32);
    const int64_t m = (int64_t)(0xFFFFFFFFu - (uint32_t)key);
    if (bits > kOneBits || m >= n_messages) continue;
    const unsigned v = bits + 1u;
    if (b[m] < v) atomicMax(&b[m], v);
  }
}

// out[0 .. n) = value; with flags: only the rows [q * k, (q + 1) * k) whose flags[q] is set
__global__ void __launch_bounds__(256) fill_keys_kernel(u64* __restrict__ out, int64_t n, u64 value, const unsigned* __restrict__ flags, int k) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (!flags || flags[i / k]) out[i] = value;
}

int pow2_at_least(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

// what the boundary search and the refinement read (the sorted route's k may be any 1 .. n_pos; it has no out_keys)
bool valid_head(const TopkLaunch& t) {
  return t.nq >= 1 && t.nq <= TAVB_MAX_STREAM_QUERIES && t.k >= 1 && t.buckets >= 64 && t.buckets % 64 == 0 && t.cap >= 64 &&
         t.cap <= TAVB_MAX_LARGE_K && t.rounds >= 0 && t.blocks >= 1 && t.n_pos > 0 && t.scores && t.workspace;
}

bool valid(const TopkLaunch& t) { return valid_head(t) && t.k <= TAVB_MAX_LARGE_K && t.out_keys && t.out_rounds; }

}  // namespace

size_t topk_workspace_bytes(int nq, int k, int buckets, int cap, int rounds) {
  return head_bytes(nq, buckets, rounds) + (size_t)nq * ((size_t)k + cap) * sizeof(u64);
}

size_t topk_head_bytes(int nq, int buckets, int rounds) { return head_bytes(nq, buckets, rounds); }

int topk_refine_rounds(int64_t n_pos, int cap) {
  if (n_pos <= cap) return 0;  // the boundary bucket can never hold more than the list takes
  // the first boundary range spans < 2^62 keys (score bits <= 1.0f = 0x3F800000 < 2^30, then the 32 position bits); every round leaves at
  // most ceil(width / kB2) of them
  unsigned long long w = 1ull << 62;
  int r = 0;
  while (w > (unsigned long long)cap) {
    w = w / kB2 + 1;
    ++r;
  }
  return r;
}

hipError_t launch_message_hist(const TopkLaunch& t, unsigned* best, hipStream_t stream) {
  if (!valid_head(t) || !best || best != t.scores || t.buckets > kMessageHistBuckets) return hipErrorInvalidValue;
  hipLaunchKernelGGL(message_hist_kernel, dim3(t.blocks, t.nq), dim3(256), 0, stream, t, best);
  return hipGetLastError();
}

hipError_t launch_topk_refine(const TopkLaunch& t, int round, hipStream_t stream) {
  if (!valid_head(t) || round < 0 || round >= t.rounds) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topk_refine_kernel, dim3(t.blocks, t.nq), dim3(256), 0, stream, t, round);
  return hipGetLastError();
}

hipError_t launch_topk_compact(const TopkLaunch& t, hipStream_t stream) {
  if (!valid(t)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topk_compact_kernel, dim3(t.blocks, t.nq), dim3(256), 0, stream, t);
  return hipGetLastError();
}

hipError_t launch_topk_finish(const TopkLaunch& t, hipStream_t stream) {
  if (!valid(t)) return hipErrorInvalidValue;
  const size_t lds = (size_t)pow2_at_least(t.k > t.cap ? t.k : t.cap) * sizeof(u64);  // <= 16384 keys: 128 KiB
  if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(topk_finish_kernel), (int)lds)) return e;
  hipLaunchKernelGGL(topk_finish_kernel, dim3(t.nq), dim3(1024), lds, stream, t);
  return hipGetLastError();
}

hipError_t launch_merge_topk(const unsigned long long* lists, int n_lists, int nq, int k, bool query_major, unsigned long long* out,
                             hipStream_t stream) {
  if (!lists || !out || n_lists < 1 || n_lists > 64 || nq < 1 || nq > 65535 || k < 1 || k > TAVB_MAX_LARGE_K) return hipErrorInvalidValue;
  const int per_block = 256 * kMergeTopkPerThread;
  const int blocks = (n_lists * k + per_block - 1) / per_block;
  hipLaunchKernelGGL(merge_topk_kernel, dim3(blocks, nq), dim3(256), 0, stream, lists, n_lists, nq, k, query_major ? 1 : 0, out);
  return hipGetLastError();
}

hipError_t launch_message_keys_max(const unsigned long long* lists, int n_lists, int nq, int k, bool query_major, int q0, int n, int64_t n_messages,
                                   unsigned* best, unsigned* flags, hipStream_t stream) {
  if (!lists || !best || !flags || n_lists < 1 || n_lists > 64 || nq < 1 || k < 1 || k > TAVB_MAX_LARGE_K || q0 < 0 || n < 1 ||
      n > TAVB_MAX_STREAM_QUERIES || q0 + n > nq || n_messages < 1 || n_messages >= 0x7FFFFFFFll)
    return hipErrorInvalidValue;
  const int per_block = 256 * kMergeTopkPerThread;
  const int blocks = (n_lists * k + per_block - 1) / per_block;
  hipLaunchKernelGGL(message_keys_max_kernel, dim3(blocks, n), dim3(256), 0, stream, lists, n_lists, nq, k, query_major ? 1 : 0, q0, n_messages, best, flags);
  return hipGetLastError();
}

hipError_t launch_fill_keys(unsigned long long* out, int64_t n, unsigned long long value, hipStream_t stream) {
  if (!out || n < 1) return hipErrorInvalidValue;
  const int blocks = n > 1024 * 256 ? 1024 : (int)((n + 255) / 256);
  hipLaunchKernelGGL(fill_keys_kernel, dim3(blocks), dim3(256), 0, stream, out, n, value, static_cast<const unsigned*>(nullptr), 1);
  return hipGetLastError();
}

hipError_t launch_fill_flagged_rows(unsigned long long* out, int nq, int k, unsigned long long value, const unsigned* flags, hipStream_t stream) {
  if (!out || !flags || nq < 1 || k < 1) return hipErrorInvalidValue;
  const int64_t n = (int64_t)nq * k;
  const int blocks = n > 1024 * 256 ? 1024 : (int)((n + 255) / 256);
  hipLaunchKernelGGL(fill_keys_kernel, dim3(blocks), dim3(256), 0, stream, out, n, value, flags, k);
  return hipGetLastError();
}

int sorted_blocks(int64_t n_pos, int64_t* chunk) {
  int64_t b = (n_pos + 2047) / 2048;
  if (b > 1024) b = 1024;
  if (b < 1) b = 1;
  int64_t c = (n_pos + b - 1) / b;
  c = (c + 255) / 256 * 256;
  *chunk = c;
  return (int)((n_pos + c - 1) / c);
}

hipError_t launch_sorted_count(const TopkLaunch& t, unsigned* counts, hipStream_t stream) {
  if (!valid_head(t) || !counts) return hipErrorInvalidValue;
  int64_t chunk;
  const int blocks = sorted_blocks(t.n_pos, &chunk);
  hipLaunchKernelGGL(sorted_count_kernel, dim3(blocks, t.nq), dim3(256), 0, stream, t, chunk, counts);
  return hipGetLastError();
}

hipError_t launch_sorted_compact(const TopkLaunch& t, int q, const unsigned* counts, unsigned long long* out, hipStream_t stream) {
  if (!valid_head(t) || q < 0 || q >= t.nq || !counts || !out) return hipErrorInvalidValue;
  int64_t chunk;
  const int blocks = sorted_blocks(t.n_pos, &chunk);
  hipLaunchKernelGGL(sorted_compact_kernel, dim3(blocks), dim3(256), 0, stream, t, q, chunk, counts, out);
  return hipGetLastError();
}

}  // namespace tavb
