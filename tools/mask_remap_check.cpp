// Host check of the arithmetic of tavb_mask_remap (typeagent_py_amd/csrc/tavb_mask.hip), no GPU: the squeeze / spread helpers of
// tavb_remap_bits.h against a bit-by-bit loop, and a serial twin of the two kernels' placement rules -- per-chunk counts, the prefix inside
// a chunk, a piece OR-ed into at most two words of the chunk's image, the image's shared end words OR-ed into zeroed output; the funnel
// shift over the source bits -- against np.delete / np.insert written as loops over single bits.  Build and run (the sanitizers are the point):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I typeagent_py_amd/csrc tools/mask_remap_check.cpp -o /tmp/mask_remap_check && /tmp/mask_remap_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "tavb_remap_bits.h"

using tavb::BitMoves;
using Words = std::vector<uint32_t>;

static constexpr int64_t kChunk = 16384, kChunkWords = kChunk / 32;
static int failures = 0;

#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (++failures < 20) {             \
        std::printf("FAILED: %s: ", #cond); \
        std::printf(__VA_ARGS__);        \
        std::printf("\n");               \
      }                                  \
    }                                    \
  } while (0)

static int popc(uint32_t x) { return __builtin_popcount(x); }
static uint32_t low_bits(int64_t k) { return k >= 32 ? 0xFFFFFFFFu : k <= 0 ? 0u : (1u << (int)k) - 1u; }
static bool bit(const Words& m, int64_t r) { return (m[r >> 5] >> (r & 31)) & 1u; }
static int64_t n_words(int64_t rows) { return (rows + 31) >> 5; }

// mask_word of the kernels: the bits at or beyond `rows` cleared, 0 past the last word
static uint32_t mask_word(const Words& m, int64_t w, int64_t rows) {
  if (w >= n_words(rows)) return 0u;
  return m[w] & low_bits(rows - (w << 5));
}

static Words random_mask(std::mt19937& rng, int64_t rows, int density_pct, bool garbage_tail) {
  Words m(n_words(rows) + 1);
  for (auto& w : m) {
    w = 0;
    for (int i = 0; i < 32; ++i) w |= (uint32_t)((int)(rng() % 100) < density_pct) << i;
  }
  if (!garbage_tail) {
    for (int64_t w = 0; w < (int64_t)m.size(); ++w) m[w] = mask_word(m, w, rows);
  }
  return m;
}

static void check_helpers(std::mt19937& rng) {
  for (int t = 0; t < 200000; ++t) {
    uint32_t m = rng(), x = rng();
    if (t % 7 == 0) m &= rng();
    if (t % 11 == 0) m |= rng();
    if (t == 0) m = 0;
    if (t == 1) m = 0xFFFFFFFFu;
    const BitMoves b = tavb::bit_moves(m);
    uint32_t sq = 0, sp = 0;
    int k = 0;
    for (int i = 0; i < 32; ++i)
      if ((m >> i) & 1u) {
        sq |= ((x >> i) & 1u) << k;
        sp |= ((x >> k) & 1u) << i;
        ++k;
      }
    CHECK(tavb::squeeze_bits(x, m, b) == sq, "m=%08x x=%08x", m, x);
    CHECK(tavb::spread_bits(x & low_bits(k), m, b) == sp, "m=%08x x=%08x", m, x);
    const int sh = (int)(rng() % 32);
    const uint64_t both = ((uint64_t)m << 32) | x;
    CHECK(tavb::funnel_bits(x, m, sh) == (uint32_t)(both >> sh), "sh=%d", sh);
  }
}

// REMOVE as mask_remap_squeeze_kernel does it
static Words remove_twin(const Words& flags, const Words& in, int64_t old_rows, int64_t new_rows) {
  Words out(n_words(new_rows), 0u);
  const int64_t chunks = (old_rows + kChunk - 1) / kChunk;
  std::vector<unsigned> kept(chunks, 0u);
  for (int64_t c = 0; c < chunks; ++c)
    for (int64_t w = c * kChunkWords; w < (c + 1) * kChunkWords; ++w) kept[c] += popc(~(w < n_words(old_rows) ? flags[w] : ~0u) & (w < n_words(old_rows) ? low_bits(old_rows - (w << 5)) : 0u));
  int64_t base = 0;
  for (int64_t c = 0; c < chunks; base += kept[c], ++c) {
    if (kept[c] == 0) continue;
    const unsigned head = (unsigned)(base & 31);
    const int n_piece = (int)((head + kept[c] + 31u) >> 5);
    std::vector<uint32_t> piece(kChunkWords + 2, 0u);
    unsigned off = head;
    for (int64_t w = c * kChunkWords; w < (c + 1) * kChunkWords; ++w) {
      const uint32_t kw = w < n_words(old_rows) ? ~flags[w] & low_bits(old_rows - (w << 5)) : 0u;
      const uint32_t x = tavb::squeeze_bits(mask_word(in, w, old_rows), kw, tavb::bit_moves(kw));
      const unsigned lo = off >> 5, s = off & 31u;
      if (x) {
        piece.at(lo) |= x << s;
        if (s != 0u && (x >> (32u - s)) != 0u) piece.at(lo + 1) |= x >> (32u - s);
      }
      off += popc(kw);
    }
    for (int i = 0; i < n_piece; ++i) out.at((base >> 5) + i) |= piece[i];  // (stores and ORs give the same on zeroed output)
  }
  CHECK(base == new_rows, "kept %lld of %lld, expected %lld", (long long)base, (long long)old_rows, (long long)new_rows);
  return out;
}

// INSERT (flags != nullptr) and APPEND as mask_remap_spread_kernel does them
static Words insert_twin(const Words* flags, const Words& in, int64_t old_rows, int64_t new_rows, bool fill) {
  Words out(n_words(new_rows), 0u);
  int64_t src = 0;
  for (int64_t w = 0; w < n_words(new_rows); ++w) {
    const uint32_t valid = low_bits(new_rows - (w << 5));
    const uint32_t hole = flags ? (*flags)[w] & valid : valid & ~low_bits(old_rows - (w << 5));
    const uint32_t clear = valid & ~hole;
    if (flags == nullptr && w % kChunkWords == 0) CHECK(src == std::min(w * 32, old_rows), "append base of chunk %lld", (long long)(w / kChunkWords));
    uint32_t v = fill ? hole : 0u;
    if (clear) {
      const int64_t lo = src >> 5;
      const uint32_t x = tavb::funnel_bits(mask_word(in, lo, old_rows), mask_word(in, lo + 1, old_rows), (int)(src & 31));
      v |= tavb::spread_bits(x & low_bits(popc(clear)), clear, tavb::bit_moves(clear));
    }
    out[w] = v;
    src += popc(clear);
  }
  CHECK(src == old_rows, "%lld clear bits, %lld old rows", (long long)src, (long long)old_rows);
  return out;
}

static void check_edit(std::mt19937& rng, int64_t old_rows, int flag_pct, int mask_pct) {
  // removal
  Words flags = random_mask(rng, old_rows, flag_pct, true), in = random_mask(rng, old_rows, mask_pct, true);
  std::vector<bool> want;
  for (int64_t r = 0; r < old_rows; ++r)
    if (!bit(flags, r)) want.push_back(bit(in, r));
  const int64_t kept = (int64_t)want.size();
  Words got = remove_twin(flags, in, old_rows, kept);
  for (int64_t k = 0; k < kept; ++k) CHECK(bit(got, k) == want[k], "remove %lld rows at %d%%: bit %lld", (long long)old_rows, flag_pct, (long long)k);
  if (kept & 31) CHECK((got.back() >> (kept & 31)) == 0u, "remove: tail bits of %lld rows", (long long)kept);
  // insertion: the same flags name the holes of a row space of old_rows rows, the clear bits number the input's rows
  Words src = random_mask(rng, kept, mask_pct, true);
  for (int fill = 0; fill < 2; ++fill) {
    got = insert_twin(&flags, src, kept, old_rows, fill != 0);
    int64_t o = 0;
    for (int64_t p = 0; p < old_rows; ++p) {
      const bool w = bit(flags, p) ? fill != 0 : bit(src, o++);
      CHECK(bit(got, p) == w, "insert to %lld rows at %d%%: bit %lld", (long long)old_rows, flag_pct, (long long)p);
    }
    if (old_rows & 31) CHECK((got.back() >> (old_rows & 31)) == 0u, "insert: tail bits of %lld rows", (long long)old_rows);
    // append: from `kept` rows to old_rows
    got = insert_twin(nullptr, src, kept, old_rows, fill != 0);
    for (int64_t p = 0; p < old_rows; ++p) CHECK(bit(got, p) == (p < kept ? bit(src, p) : fill != 0), "append %lld -> %lld: bit %lld", (long long)kept, (long long)old_rows, (long long)p);
    if (old_rows & 31) CHECK((got.back() >> (old_rows & 31)) == 0u, "append: tail bits of %lld rows", (long long)old_rows);
  }
}

int main() {
  std::mt19937 rng(24);
  check_helpers(rng);
  const int64_t rows[] = {1, 2, 31, 32, 33, 63, 64, 65, kChunk - 1, kChunk, kChunk + 1, 2 * kChunk + 17, 3 * kChunk + 31};
  for (int64_t n : rows)
    for (int flag_pct : {0, 1, 3, 50, 97, 99, 100})
      for (int mask_pct : {0, 1, 50, 100}) check_edit(rng, n, flag_pct, mask_pct);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("mask remap arithmetic: ok\n");
  return 0;
}
