// The bit arithmetic of tavb_mask_remap (tavb_mask.hip), in plain C++ so that the host can run it too (tools/mask_remap_check.cpp checks
// it against a bit-by-bit loop): a mask word is SQUEEZED under a selector word -- the bits the selector names move down, in order, into
// the low popcount(selector) bits -- or SPREAD under it, the inverse.  Both go through the five move masks of the selector (Hacker's
// Delight 7-4 / 7-5, "compress" and "expand"): the moves depend on the selector alone, so a thread works them out once per flag word and
// applies them to the word of every carried mask, five steps of three operations each, in registers.
#ifndef TAVB_REMAP_BITS_H
#define TAVB_REMAP_BITS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define TAVB_BITS_FN __host__ __device__ __forceinline__
#else
#define TAVB_BITS_FN inline
#endif

namespace tavb {

struct BitMoves {
  uint32_t mv[5];  // step i moves the bits of mv[i] down (squeeze) or up (spread) by 1 << i
};

// the moves of selector m: a selected bit goes down by the number of unselected bits below it
TAVB_BITS_FN BitMoves bit_moves(uint32_t m) {
  BitMoves b;
  uint32_t mk = ~m << 1;  // the unselected bits, one up: their parallel-prefix parity below is "an odd number of them lies below this bit"
  for (int i = 0; i < 5; ++i) {
    uint32_t mp = mk ^ (mk << 1);
    mp ^= mp << 2;
    mp ^= mp << 4;
    mp ^= mp << 8;
    mp ^= mp << 16;
    const uint32_t mv = mp & m;  // selected bits with an odd number (in units of 1 << i) of unselected bits below them
    b.mv[i] = mv;
    m = (m ^ mv) | (mv >> (1 << i));
    mk &= ~mp;
  }
  return b;
}

// the bits of x that selector m names, packed into the low popcount(m) bits in their order; the other bits zero
TAVB_BITS_FN uint32_t squeeze_bits(uint32_t x, uint32_t m, const BitMoves& b) {
  x &= m;
  for (int i = 0; i < 5; ++i) {
    const uint32_t t = x & b.mv[i];
    x = (x ^ t) | (t >> (1 << i));
  }
  return x;
}

// the low popcount(m) bits of x moved, in their order, to the bits selector m names; the other bits zero
TAVB_BITS_FN uint32_t spread_bits(uint32_t x, uint32_t m, const BitMoves& b) {
  for (int i = 4; i >= 0; --i) {
    const uint32_t t = x << (1 << i);
    x = (x & ~b.mv[i]) | (t & b.mv[i]);
  }
  return x & m;
}

// 32 bits of a packed mask from bit `sh` (0 .. 31) of word pair (lo, hi) on
TAVB_BITS_FN uint32_t funnel_bits(uint32_t lo, uint32_t hi, int sh) { return sh ? (lo >> sh) | (hi << (32 - sh)) : lo; }

}  // namespace tavb

#endif
