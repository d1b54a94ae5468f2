// The 32/64-query tile (`skinny_scan_kernel`) for fp32 and fp16 corpora and its launcher: small batches -- and every batch on the
// reference's fp32 layout -- at HBM speed.  The parameter block and the compaction it shares with the 128/256-query
// tile (tavb_mfma_wide.hip) are in tavb_tile.h.

#include <hip/hip_runtime.h>

#include <tuple>
#include <type_traits>

#include "tavb_tile.h"

namespace tavb {

namespace {

// ---------------------------------------------------------------------------------------------
// SKINNY kernel: 3 .. 32 queries per pass at HBM speed (32-query tile), 33+ on 64-query tiles; fp32 AND fp16 corpora.
//
// The streaming tiers keep the queries in LDS and every lane re-reads them for every row, so beyond four
// queries they are LDS-bound (6.9 TB/s of corpus at one query, 4.8 at eight, then one more pass per eight
// queries); the 256-query MFMA tile (tavb_mfma_wide.hip) wastes 7/8 of its operand traffic on padding at 32 queries and
// only exists for fp16.  This kernel is the piece in between -- and the only matrix-core path for the
// reference's own dtype, fp32: `v_mfma_f32_32x32x2_f32` multiplies fp32 exactly and accumulates in fp32
// (157 TFLOP/s peak, enough to keep up with HBM at 32 queries: 1M x 1536 x 32 x 2 = 98 GFLOP per 6.1 GB pass).
//   * tile = 256 corpus rows x 32 (or 64) queries, 4 waves, each wave owns 64 rows (two, or four, 32 x 32 MFMA tiles).
//   * K advances STEP bytes per row per step for either dtype: 128 (a whole cache line per row and staging lane group:
//     the texture-address path serves eight 128-byte lines twice as fast as sixteen 64-byte half lines,
//     profiles/r02_operand_path.md) whenever a row is a multiple of 128 bytes, else 64.  A wave stages the 1 KiB pieces of
//     ITS OWN 64 rows by LDS-DMA, so the corpus operand needs no cross-wave synchronisation; the waves also share out
//     the pieces of the query operand, which all of them read: one barrier per step.  Ring of 2 .. 4 slots, counted vmcnt;
//     72 KiB configurations run two workgroups per CU, the others one.
//   * LDS rows are STEP bytes; 16-byte slot j of row r sits at physical slot j ^ ((r >> 1) & 7) (128-byte rows) or
//     j ^ ((r >> 2) & 3) (64-byte rows) -- on the global SOURCE address of the staging loads and on the fragment reads --
//     so the 16 lanes of a ds_read_b128 group hit 16 different bank slots.  For fp32 a lane's 16-byte fragment is four
//     consecutive k of its row -- lanes 0-31 take k = 8g .. 8g+3, lanes 32-63 k = 8g+4 .. 8g+7 -- and feeds four
//     MFMAs: MFMA e multiplies k = 8g+e (lower half-wave) and 8g+4+e (upper), the same pairing on both operands, which
//     is all a dot product needs.
//   * fp16 corpora: the fp32 queries are split into an fp16 high and an fp16 low plane (q = hi + lo to 2^-22; both are
//     multiplied -- the kernel is load-bound, the second MFMA is free), so a lookup on an fp16 corpus means the same
//     thing here as in the streaming tiers (fp32 query x fp16 rows).
//   * NI = 2 (64 queries per tile): twice the MFMAs per operand byte -- for batches of 33+ queries, which would
//     otherwise stream the corpus once per 32 queries (fp32) or pay for a 256-query tile (fp16, 33 .. 64 queries).
//   * epilogue / candidate buffers / compaction as in the 256-query tile (32 or 64 queries per block); at the end every
//     buffer is sorted into a list, tavb::merge_kernel merges the lists of the row ranges.
// ---------------------------------------------------------------------------------------------
constexpr int SQ32 = 32;            // queries per 32 x 32 MFMA block; a tile is NI of them (32 or 64 queries)
constexpr int S_THREADS = 256;
typedef const __attribute__((address_space(1))) f32x4 global_f32x4;
template <typename T, int NI, int STEP, bool DEEP = false, int DR = 0, bool HALF = false>
struct SkinnyGeom {
  // HALF: 128-row tiles (a wave owns 32 rows = one 32 x 32 block per 32 queries) -- half the corpus slot, so that a ring of three fits twice
  // into a CU's LDS and TWO workgroups share a CU (one waits at its barrier, the other multiplies), as the fp32 32-query tile always did
  static constexpr int BMT = HALF ? BM / 2 : BM;   // corpus rows per tile
  static constexpr int RW = BMT / 4;               // ... per wave
  static constexpr int MI = RW / 32;               // 32-row blocks per wave
  static constexpr bool F32 = sizeof(T) == 4;
  static constexpr int SQ = NI * SQ32;
  static constexpr int PLANES = F32 ? 1 : 2;
  static constexpr int LPR = STEP / 16;            // lanes (16-byte slots) per row of a staging piece
  static constexpr int RPP = 64 / LPR;             // rows per 1 KiB piece: 16 or 8
  static constexpr int NPA = RW / RPP;             // corpus pieces per wave per step: 4 or 8 (2 or 4 with half tiles)
  static constexpr int SH = STEP == 64 ? 2 : 1;    // swizzle term = (row >> SH) & (LPR - 1)
  static constexpr int NG = STEP / 32;             // 32-byte k slices per step: 2 or 4
  static constexpr int SLOT_A = BMT * STEP;        // 16 or 32 KiB (half tiles: 8 or 16)
  static constexpr int PLANE_B = SQ * STEP;        // one query operand plane, one step
  static constexpr int SLOT_B = PLANES * PLANE_B;
  // ring depth: measured (profiles/r02_mid_batch.md) -- for 32 fp32 queries two workgroups per CU with two slots each beat one
  // workgroup with three or four slots (the depth in flight is not what limits this tile)
  static constexpr int RING = STEP == 64 ? ((F32 && NI == 1) ? 4 : 3) : ((F32 && NI == 1) ? 2 : 3);
  // DEEP (32-query tile, whole-line steps): the corpus ring one slot deeper than the query ring -- 4 x 32 KiB of corpus + 3 query slots
  // (152 KiB fp16, 140 KiB fp32), one workgroup per CU.  The tile is HBM-bound and what it lacks is bytes in flight: with a ring of three,
  // 32 .. 64 KiB of corpus per CU are on their way at any time (8 TB/s x ~2 us of loaded latency / 256 CUs = 62 KiB: the edge); with four
  // corpus slots 64 .. 96 KiB.  The query slabs come out of L2 and need no deeper ring.
  // DR > 0 (whole-line steps): REGISTER staging.  Every byte that is on its way from HBM needs somewhere to land; with LDS-DMA that is an LDS
  // slot, and 160 KiB of LDS hold 80 .. 110 KiB in flight however the ring is cut -- the edge of what 8 TB/s x ~2 us / 256 CUs asks for.  The
  // register file is three times the LDS: the loads of the next DR K steps (corpus AND query pieces, the same coalesced 1 KiB pieces) land in
  // DR x (NPA + PLANES * NPB) x 4 VGPRs per lane and are written to LDS (ds_write_b128, the layout the LDS-DMA would have produced) when
  // their step comes up.  LDS then holds ONE corpus slot (each wave's 64 rows are its own: DS operations of a wave execute in order, nothing
  // to synchronise) and two query slots; the compiler counts the waits (plain register dependencies).
  static constexpr int RA = DR > 0 ? 1 : DEEP ? 4 : RING;       // corpus slots
  static constexpr int RB = DR > 0 ? 2 : DEEP ? 3 : RING;       // query slots (RB <= RA for the LDS-DMA rings)
  static constexpr int B_RING = RA * SLOT_A;
  static constexpr int CTRL = RA * SLOT_A + RB * SLOT_B;
  static constexpr int LDS = CTRL + SQ * 8 + 16;
  static constexpr int WG_PER_CU = LDS <= 76 * 1024 ? 2 : 1;
  static constexpr int B_PIECES = SQ / RPP;        // query pieces per plane per step: 2 .. 8
  static constexpr int NPB = (B_PIECES + 3) / 4;   // ... per wave (waves >= B_PIECES stage none when there are fewer than 4)
  static_assert((DR > 0 || RB <= RA) && RB >= 2 && LDS <= 160 * 1024, "ring does not fit");
  static_assert(DR == 0 || STEP == 128, "register staging is built for whole-line steps");
};

// MASKED: a row is a candidate only if its bit is set in an allow-mask (tavb.h "row masks": uint32 words, row r = bit r & 31 of word r >> 5).  The
// mask is the ONE extra kernel argument of the masked instantiations (`mask_arg`: empty, or one `const uint32_t*`) -- MfmaDeviceParams, which the
// 128/256-query tile shares, does not know about it, and MASKED = false compiles to what it compiled to before the parameter existed.  The
// pointer names the word of the launch's first row (a multiple of 32: the launcher checks), so a 32-row block of the epilogue is exactly one
// word.  The word is wave-uniform and comes in through the SCALAR data path (a constant-address-space load: it counts in lgkmcnt, which every
// K step waits out anyway) -- a vector or flat load the compiler can see among the staging loads would make its wait-count pass drain the whole
// staging queue (see `need_compact` and the candidate store).
typedef const __attribute__((address_space(4))) uint32_t const_u32;
// SCOPED: the third mask mode -- one scope PER QUERY (tavb.h "scoped batches on the tile").  The extra argument of a MASKED instantiation is
// then not a mask but the membership PLANES of the batch (scope_planes_kernel, tavb_mask.hip): for every block of 32 queries one uint32 per row
// of the span, bit i = the scope of query 32 * block + i holds the row; `stride` words from one block's plane to the next.  The mode is the
// TYPE of the argument (`const uint32_t*`: one mask; ScopePlanes: per-query scopes), so the unmasked and the one-mask instantiations keep
// their names and compile to what they compiled to before the mode existed.  `words` names the word of the launch's first row (a multiple of
// 32 rows into the span), as the one mask's pointer does.  A lane of the admission path is (half << 5) | query_in_block and tests row
// r_off (+ 4 in the upper half) of its 32-row block: the lanes a row pair may admit are plane[row] | plane[row + 4] << 32 -- one scalar AND
// into the compare's wave mask.  The 32 words of a (block, ni) pair are wave-uniform and come through the scalar data path like the one
// mask's word (two 16-word loads, lgkmcnt), only behind a non-zero ballot.
struct ScopePlanes {
  const uint32_t* words;
  int64_t stride;
};
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
typedef const __attribute__((address_space(4))) u32x16 const_u32x16;
// TOPMSG: the top-messages form (tavb.h "top messages on the tile") -- the epilogue keeps no candidates: an admitted (row, query) pair raises
// best[query][message of the row] to 1 + the bits of its clamped score (MessageMaxSink's encoding, tavb_scan.hip, over the same zeroed array;
// message_hist_kernel and the selection run behind it unchanged).  Like SCOPED the mode is the TYPE of an extra argument, the LAST one (after
// the one mask of a MASKED instantiation) -- the pack is empty by default, so every other instantiation keeps its name and compiles to what it
// compiled to before the mode existed (a template parameter in front of the pack would be part of every mangled name).  `map` names the entry
// of the launch's first row (64-byte aligned: the launcher checks); map_rows entries from there on are readable.  The 32 entries of an
// admitting block are wave-uniform and come through the scalar data path like the SCOPED form's plane words (two 16-word loads, lgkmcnt), only
// behind a non-zero ballot; a block that reaches behind map_rows loads its entries one by one.  Thresholds never rise: no k-th best, no
// cnt_lds, no need_compact, no candidate buffer, no lists -- p.cand and p.lists may be null.  Never together with SCOPED.
struct TopMessages {
  const int32_t* map;
  unsigned* best;      // [nq_padded or more][n_messages], zero when the launch starts
  int64_t map_rows;
  int64_t n_messages;
};
template <typename T, int NI, int STEP, bool DEEP = false, int DR = 0, bool HALF = false, bool MASKED = false, typename... MaskArg>
__global__ void __launch_bounds__(S_THREADS, ((DR >= 4 || (DR == 3 && sizeof(T) == 2)) ? 1 : 2)) skinny_scan_kernel(const MfmaDeviceParams p, MaskArg... mask_arg) {
  constexpr bool TOPMSG = (std::is_same_v<MaskArg, TopMessages> || ...);  // the top-messages form: the LAST argument is the message map and the best array
  static_assert(sizeof...(MaskArg) == (MASKED ? 1 : 0) + (TOPMSG ? 1 : 0), "the mask is an argument of the masked instantiations only");
  constexpr bool SCOPED = (std::is_same_v<MaskArg, ScopePlanes> || ...);  // per-query scopes: the argument is the membership planes
  static_assert(!(SCOPED && TOPMSG), "no top-messages form of the scoped tile");
  // the one mask of a MASKED instantiation: its first extra argument (the top-messages form has one more behind it)
  [[maybe_unused]] const auto mask_of = [](auto a, auto...) { return a; };
  using G = SkinnyGeom<T, NI, STEP, DEEP, DR, HALF>;
  constexpr int BMT = G::BMT, RW = G::RW, MI = G::MI;
  constexpr int SQ = G::SQ;
  constexpr bool F32 = G::F32;
  constexpr int RA = G::RA, RB = G::RB, S_SLOT_A = G::SLOT_A, S_SLOT_B = G::SLOT_B, S_B_RING = G::B_RING, S_CTRL = G::CTRL;
  constexpr int NPA = G::NPA, NPB = G::NPB, RPP = G::RPP, LPR = G::LPR, NG = G::NG;
  extern __shared__ __align__(16) unsigned char smem[];
  float* thr_lds = reinterpret_cast<float*>(smem + S_CTRL);
  int* cnt_lds = reinterpret_cast<int*>(smem + S_CTRL + SQ * 4);
  // (an LDS-typed pointer: through a generic one the per-tile read below is a FLAT load, which counts in vmcnt AND lgkmcnt and cannot be waited
  // for by count -- the compiler drained the whole staging queue behind it once per tile, and with a flat access pending anywhere in the loop
  // it turns the first counted wait of every K-loop iteration into vmcnt(0) as well)
  lds_flag* need_compact = (lds_flag*)(smem + S_CTRL + SQ * 8);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // rows wave * 64 .. of the tile

  const int b = blockIdx.x;
  const int xcd = b & 7;
  const int t = b >> 3;
  const int qtile = t % p.n_qtiles;
  const int split = (t / p.n_qtiles) * 8 + xcd;
  if (split >= p.n_splits) return;
  int live_q = p.nq;
  if (p.active != nullptr) {  // fixed-shape launch over a device-side work list (tavb_rescore.hip)
    const int live = *p.active;
    if (live <= p.active_min || live > p.active_max || qtile * SQ >= live) return;
    live_q = live < live_q ? live : live_q;
  }
  const int64_t r_begin = (int64_t)split * p.rows_per_split;
  const int64_t r_end = (r_begin + p.rows_per_split < p.rows) ? r_begin + p.rows_per_split : p.rows;
  const int logical_block = split * p.n_qtiles + qtile;
  [[maybe_unused]] u64* my_cand = TOPMSG ? nullptr : p.cand + (size_t)logical_block * SQ * CAP;

  const float thr0 = (p.min_score > 0.0f) ? __uint_as_float(__float_as_uint(p.min_score) - 1u) : -__builtin_inff();
  if (tid < SQ) {  // SQ <= 64 < S_THREADS
    float t0 = (p.min_score != p.min_score || p.min_score > 1.0f) ? __builtin_inff() : thr0;  // NaN threshold admits nothing, nor one above 1 (as in the 256-query tile)
    const int qg0 = qtile * SQ + tid;
    if (qg0 >= live_q) t0 = __builtin_inff();  // padding queries (and unused work-list slots) admit nothing
    else if (p.thr_in && p.thr_in[qg0] > t0) t0 = p.thr_in[qg0];  // k-th best so far: a valid lower bound
    thr_lds[tid] = t0;
    if constexpr (!TOPMSG) cnt_lds[tid] = 0;
  }
  if constexpr (!TOPMSG)
    if (tid == 0) *need_compact = 0;

  const size_t row_bytes = (size_t)p.dim * sizeof(T);
  const int steps_per_tile = (int)(row_bytes / STEP);
  const char* corpus = reinterpret_cast<const char*>(p.corpus);
  const char* qbase = reinterpret_cast<const char*>(p.queries) + (size_t)qtile * SQ * row_bytes;
  const size_t plane_bytes = (size_t)p.n_qtiles * SQ * row_bytes;  // fp16: the low plane follows the high plane
  const int n_tiles = (r_end > r_begin) ? (int)((r_end - r_begin + BMT - 1) / BMT) : 0;
  if (n_tiles == 0) {
    if constexpr (TOPMSG) return;  // (no lists to zero)
    for (int q = wave; q < SQ; q += S_THREADS / 64) {
      const int qg = qtile * SQ + q;
      if (qg < p.nq && lane < p.k) p.lists[((size_t)qg * p.list_stride + split) * (size_t)p.k + lane] = 0ull;
    }
    return;
  }

  // ---- stager: piece j of this wave = corpus rows wave * 64 + j * RPP .. of the tile (its own rows); lane l = row
  //      l / LPR, PHYSICAL 16-byte slot l % LPR, which holds the logical slot (l % LPR) ^ ((row >> SH) & (LPR - 1)).
  //      Query piece pb = wave + 4 i covers query rows pb * RPP ..
  const int st_row_in_piece = lane / LPR;
  uint32_t st_off[NPA];
  auto set_offsets = [&](int64_t row0) {
#pragma unroll
    for (int j = 0; j < NPA; ++j) {
      const int row = wave * RW + j * RPP + st_row_in_piece;  // row of the tile: fixes the swizzle term
      int64_t r = row;
      if (row0 + r >= p.rows) r = p.rows - 1 - row0;  // stay in bounds; masked in the epilogue
      st_off[j] = (uint32_t)r * (uint32_t)row_bytes + (uint32_t)((((lane % LPR) ^ ((row >> G::SH) & (LPR - 1)))) * 16);
    }
  };
  uint32_t st_off_b[NPB];
#pragma unroll
  for (int i = 0; i < NPB; ++i) {
    const int row = (wave + 4 * i) * RPP + st_row_in_piece;
    st_off_b[i] = (uint32_t)row * (uint32_t)row_bytes + (uint32_t)((((lane % LPR) ^ ((row >> G::SH) & (LPR - 1)))) * 16);
  }
  const bool stages_b = G::B_PIECES >= 4 || wave < G::B_PIECES;  // (with fewer than four query pieces the last waves stage none)
  // Two rings: corpus slabs run RA - 1 steps ahead of the multiply, query slabs RB - 1 (RB <= RA).  A "round" = what one K step issues:
  // the query slab of step S + RB - 1 FIRST, then the corpus slab of step S + RA - 1 -- loads return in order, so with that order the
  // counted wait below leaves the newest corpus slabs in flight.
  int st_tile = 0, st_kt = 0, st_slot = 0;  // corpus slab being staged
  int sb_kt = 0, sb_slot = 0;               // query slab being staged
  set_offsets(r_begin);

  auto stage_b = [&]() {
    if (stages_b) {
      const char* gb = sgpr_ptr(qbase + (size_t)sb_kt * STEP);
#pragma unroll
      for (int i = 0; i < NPB; ++i) {
        unsigned char* lb = smem + S_B_RING + sb_slot * S_SLOT_B + (wave + 4 * i) * 1024;
        __builtin_amdgcn_global_load_lds((global_void*)(gb + (size_t)st_off_b[i]), (lds_void*)lb, 16, 0, 0);
        if constexpr (!F32)  // the low plane of the split queries
          __builtin_amdgcn_global_load_lds((global_void*)(gb + plane_bytes + (size_t)st_off_b[i]), (lds_void*)(lb + G::PLANE_B), 16, 0, 0);
      }
    }
    if (++sb_slot == RB) sb_slot = 0;
    if (++sb_kt == steps_per_tile) sb_kt = 0;
  };
  auto stage_a = [&]() {
    const int tile = st_tile < n_tiles ? st_tile : n_tiles - 1;  // past the end: harmless reloads of the last tile
    const int64_t src_row0 = r_begin + (int64_t)tile * BMT;
    const char* ga = sgpr_ptr(corpus + (size_t)src_row0 * row_bytes + (size_t)st_kt * STEP);
    unsigned char* la = smem + st_slot * S_SLOT_A + wave * (RW * STEP);
#pragma unroll
    for (int j = 0; j < NPA; ++j)
      __builtin_amdgcn_global_load_lds((global_void*)(ga + (size_t)st_off[j]), (lds_void*)(la + j * 1024), 16, 0, 0);  // (a non-temporal policy here measured 30 % slower)
    if (++st_slot == RA) st_slot = 0;
    if (++st_kt == steps_per_tile) {
      st_kt = 0;
      ++st_tile;
      if (st_tile < n_tiles) set_offsets(r_begin + (int64_t)st_tile * BMT);
    }
  };
  auto stage_next = [&]() {
    stage_b();
    stage_a();
  };
  // this wave's loads of step S have landed.  Issue order per round: NB query loads, then NA corpus loads.  Query slab S is the first thing
  // of round S - RB + 1: behind it come that round's corpus slab and RB - 2 whole rounds; corpus slab S is the last thing of round
  // S - RA + 1, with RA - 2 whole rounds behind it.  Whatever is younger than BOTH may still be in flight.
  auto wait_landed = [&]() {
    constexpr int NB = G::PLANES * NPB;
    if (stages_b)
      wait_vmcnt<((RA - 2) * (NPA + NB) < NPA + (RB - 2) * (NPA + NB)) ? (RA - 2) * (NPA + NB) : NPA + (RB - 2) * (NPA + NB)>();
    else
      wait_vmcnt<((RA - 2) < (RB - 1) ? (RA - 2) : (RB - 1)) * NPA>();
  };

  // ---- register staging (DR > 0): slot u of the register ring holds the pieces of the K steps congruent to u mod DR
  constexpr int DRN = DR > 0 ? DR : 1;
  constexpr int NBR = G::PLANES * NPB;
  f32x4 areg[DRN][NPA];
  f32x4 breg[DRN][NBR];
  auto load_regs = [&](auto u_tag) {  // the pieces of the next un-issued K step -> register slot U
    constexpr int U = decltype(u_tag)::value;
    const int tile = st_tile < n_tiles ? st_tile : n_tiles - 1;  // past the end: harmless reloads of the last tile
    const char* ga = sgpr_ptr(corpus + (size_t)(r_begin + (int64_t)tile * BMT) * row_bytes + (size_t)st_kt * STEP);
#pragma unroll
    for (int j = 0; j < NPA; ++j) areg[U][j] = *(global_f32x4*)(ga + (size_t)st_off[j]);  // (global, not flat: a flat load counts in lgkmcnt too and cannot be waited for by count)
    if (stages_b) {
      const char* gb = sgpr_ptr(qbase + (size_t)st_kt * STEP);
#pragma unroll
      for (int i = 0; i < NPB; ++i) {
        breg[U][G::PLANES * i] = *(global_f32x4*)(gb + (size_t)st_off_b[i]);
        if constexpr (!F32) breg[U][G::PLANES * i + 1] = *(global_f32x4*)(gb + plane_bytes + (size_t)st_off_b[i]);
      }
    }
    if (++st_kt == steps_per_tile) {
      st_kt = 0;
      ++st_tile;
      if (st_tile < n_tiles) set_offsets(r_begin + (int64_t)st_tile * BMT);
    }
  };
  auto commit_regs = [&](auto u_tag, int bslot) {  // register slot U -> LDS, where the LDS-DMA of the other variants would have put it
    constexpr int U = decltype(u_tag)::value;
    unsigned char* la = smem + wave * (RW * STEP) + lane * 16;
#pragma unroll
    for (int j = 0; j < NPA; ++j) *reinterpret_cast<f32x4*>(la + j * 1024) = areg[U][j];
    if (stages_b) {
#pragma unroll
      for (int i = 0; i < NPB; ++i) {
        unsigned char* lb = smem + S_B_RING + bslot * S_SLOT_B + (wave + 4 * i) * 1024 + lane * 16;
        *reinterpret_cast<f32x4*>(lb) = breg[U][G::PLANES * i];
        if constexpr (!F32) *reinterpret_cast<f32x4*>(lb + G::PLANE_B) = breg[U][G::PLANES * i + 1];
      }
    }
  };

  // ---- fragment addresses: row (lane & 31) of a 32-row block, logical 16-byte slot 2 * g + (lane >> 5)
  const int frag_row = lane & 31;
  const uint32_t frag_x = (uint32_t)(((lane >> 5) ^ ((frag_row >> G::SH) & (LPR - 1))) << 4);
  const uint32_t a_lane = (uint32_t)((wave * RW + frag_row) * STEP);  // + mi * 32 * STEP
  const uint32_t b_lane = (uint32_t)(S_B_RING + frag_row * STEP);    // + ni * 32 * STEP

  // ---- prologue: RA - 1 corpus slabs and RB - 1 query slabs in flight, in the order of the rounds that would have issued them
  //      (register staging: the first DR steps, one per register slot)
  if constexpr (DR > 0) {
    [&]<int... U>(std::integer_sequence<int, U...>) { (load_regs(std::integral_constant<int, U>{}), ...); }
    (std::make_integer_sequence<int, DRN>{});
  } else {
#pragma unroll
    for (int i = 0; i < RA - 1; ++i) {
      if (i >= RA - RB) stage_b();
      stage_a();
    }
  }

  int rd = 0, rd_b = 0;
  for (int tile = 0; tile < n_tiles; ++tile) {
    const int64_t row0 = r_begin + (int64_t)tile * BMT;
    const bool tile_full = row0 + BMT <= r_end;  // wave-uniform: every row of this tile belongs to the row range
    f32x16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    auto k_step = [&](auto u_tag) {  // one K step; U = register slot (register staging only)
      if constexpr (DR > 0) {
        // this step's pieces out of the registers (the compiler waits for exactly these loads: whatever was issued after them -- the next
        // DR - 1 steps -- stays in flight), the registers refilled with the step DR ahead; the query slot written here was last read two steps
        // ago, with a barrier in between
        commit_regs(u_tag, rd_b);
        load_regs(u_tag);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        TAVB_BARRIER();  // the query pieces of step S are visible
      } else {
        wait_landed();  // this wave's share of step S is in LDS
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        TAVB_BARRIER();  // the query pieces of step S are visible; everybody is done with the slot of step S - 1
        stage_next();  // query slab S + RB - 1, corpus slab S + RA - 1 -> the slots of step S - 1
      }
      const unsigned char* abase = smem + rd * S_SLOT_A;
      const unsigned char* bbase = smem + rd_b * S_SLOT_B;
#pragma unroll
      for (int gh = 0; gh < NG / 2; ++gh) {  // two 32-byte k slices at a time
        f32x4 af[2][MI], bf[2][NI], bl[2][NI];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const uint32_t kx = (uint32_t)((gh * 2 + g) << 5) ^ frag_x;
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) {
            bf[g][ni] = *reinterpret_cast<const f32x4*>(bbase + (b_lane + kx) + ni * 32 * STEP);
            if constexpr (!F32) bl[g][ni] = *reinterpret_cast<const f32x4*>(bbase + (b_lane + kx) + ni * 32 * STEP + G::PLANE_B);
          }
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) af[g][mi] = *reinterpret_cast<const f32x4*>(abase + (a_lane + kx) + mi * 32 * STEP);
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          if constexpr (F32) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
                  acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[g][mi][e], bf[g][ni][e], acc[mi][ni], 0, 0, 0);
          } else {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
              for (int ni = 0; ni < NI; ++ni) {
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, af[g][mi]), __builtin_bit_cast(f16x8, bl[g][ni]),
                                                                     acc[mi][ni], 0, 0, 0);
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, af[g][mi]), __builtin_bit_cast(f16x8, bf[g][ni]),
                                                                     acc[mi][ni], 0, 0, 0);
              }
          }
        }
      }
      if (++rd == RA) rd = 0;
      if (++rd_b == RB) rd_b = 0;
    };
    if constexpr (DR > 0) {  // (the launcher checks steps_per_tile % DR == 0: a tile starts on register slot 0)
#pragma unroll 1
      for (int kt = 0; kt < steps_per_tile; kt += DR)
        [&]<int... U>(std::integer_sequence<int, U...>) { (k_step(std::integral_constant<int, U>{}), ...); }
      (std::make_integer_sequence<int, DRN>{});
    } else {
#pragma unroll 1
      for (int kt = 0; kt < steps_per_tile; ++kt) k_step(std::integral_constant<int, 0>{});
    }

    // ---- epilogue: admission test on the raw dot products, append (as in the 256-query tile)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int ql = ni * 32 + (lane & 31);
      const float thr = thr_lds[ql];
      const float thr_pre = fmaf(thr, 2.0f, -1.0f) - 4.8e-7f;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        float top = acc[mi][ni][0];
#pragma unroll
        for (int r = 1; r < 16; ++r) top = __builtin_fmaxf(top, acc[mi][ni][r]);
        const bool any = top > thr_pre;
        if (__builtin_amdgcn_ballot_w64(any) != 0ull) {
          [[maybe_unused]] uint32_t allow = ~0u;  // MASKED: the word of this 32-row block; bit r_off + 4 * (lane >> 5) is the row a lane tests
          [[maybe_unused]] u32x16 plane[2];       // SCOPED: the plane words of this block's 32 rows for the 32 queries of `ni`
          if constexpr (SCOPED) {
            const int64_t block_row = row0 + wave * RW + mi * 32;  // (a multiple of 32, as r_begin and the tile are)
            if (block_row >= r_end) continue;  // wave-uniform: a block behind the row range has no plane words (and admits nothing either way)
            const ScopePlanes sp = (mask_arg, ...);
            const char* words = sgpr_ptr(reinterpret_cast<const char*>(sp.words) + ((size_t)(qtile * NI + ni) * (size_t)sp.stride + (size_t)block_row) * sizeof(uint32_t));
            plane[0] = *(const const_u32x16*)(uintptr_t)words;  // s_load_dwordx16 x 2: lgkmcnt, not vmcnt
            plane[1] = *(const const_u32x16*)(uintptr_t)(words + 16 * sizeof(uint32_t));
            uint32_t any_row = 0u;
#pragma unroll
            for (int w = 0; w < 16; ++w) any_row |= plane[0][w] | plane[1][w];
            if (any_row == 0u) continue;  // no scope of these 32 queries holds a row of this block
          } else if constexpr (MASKED) {
            const int64_t block_row = row0 + wave * RW + mi * 32;  // (a multiple of 32, as r_begin and the tile are)
            if (block_row >= r_end) continue;  // wave-uniform: a block behind the row range has no word (and admits nothing either way)
            const char* word = sgpr_ptr(reinterpret_cast<const char*>(mask_of(mask_arg...)) + (size_t)(block_row >> 5) * sizeof(uint32_t));
            allow = *(const const_u32*)(uintptr_t)word;  // s_load_dword: lgkmcnt, not vmcnt
            if (allow == 0u) continue;  // nothing of this block is allowed
          }
          [[maybe_unused]] u32x16 msgw[2];  // TOPMSG: the message of each of this block's 32 rows
          [[maybe_unused]] TopMessages tm{};
          if constexpr (TOPMSG) {
            tm = std::get<sizeof...(MaskArg) - 1>(std::tuple<MaskArg...>(mask_arg...));  // the last argument
            const int64_t block_row = row0 + wave * RW + mi * 32;  // (a multiple of 32, as r_begin and the tile are)
            if (block_row >= r_end) continue;  // wave-uniform: a block behind the row range admits nothing (and may lie behind the map)
            const char* words = sgpr_ptr(reinterpret_cast<const char*>(tm.map) + (size_t)block_row * sizeof(int32_t));
            if (block_row + 32 <= tm.map_rows) {
              msgw[0] = *(const const_u32x16*)(uintptr_t)words;  // s_load_dwordx16 x 2: lgkmcnt, not vmcnt
              msgw[1] = *(const const_u32x16*)(uintptr_t)(words + 16 * sizeof(int32_t));
            } else {  // the last block of a map whose length is no multiple of 32: entry by entry, nothing behind the map's end is read
#pragma unroll
              for (int w = 0; w < 32; ++w) {
                uint32_t m = 0xFFFFFFFFu;  // (no message)
                if (block_row + w < tm.map_rows) m = *(const const_u32*)(uintptr_t)(words + w * sizeof(int32_t));
                msgw[w >> 4][w & 15] = m;
              }
            }
          }
          // (the admission path of the 256-query tile: wave masks in scalar registers, four rows at a time, one LDS atomic per admitted row)
          const int64_t row_base = row0 + wave * RW + mi * 32 + 4 * (lane >> 5);
          const int64_t left64 = r_end - row_base;
          const int rows_left = tile_full ? 64 : (int)(left64 < 64 ? left64 : 64);
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            float sc[4];
            u64 m[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              sc[j] = fmaf(acc[mi][ni][4 * g + j], 0.5f, 0.5f);
              asm volatile("v_cmp_gt_f32 %0, %1, %2" : "=s"(m[j]) : "v"(sc[j]), "v"(thr));
            }
            if constexpr (SCOPED) {  // rows 8g .. 8g + 7 are words 8 (g & 1) .. of half g >> 1: lanes 0-31 test row r_off, lanes 32-63 row r_off + 4
#pragma unroll
              for (int j = 0; j < 4; ++j) m[j] &= (u64)plane[g >> 1][8 * (g & 1) + j] | ((u64)plane[g >> 1][8 * (g & 1) + j + 4] << 32);
            }
            if ((m[0] | m[1] | m[2] | m[3]) == 0ull) continue;  // wave-uniform
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int r_off = j + 8 * g;
              if (m[j] == 0ull) continue;
              // (MASKED: bits at or beyond `rows` in the last word may hold anything -- rows_left cuts those rows.  SCOPED: m[j] is already cut
              //  to the lanes whose query holds the row; the planes are zero behind the corpus, rows_left cuts the rows of a later phase)
              if (((m[j] >> lane) & 1ull) != 0ull && r_off < rows_left && (!MASKED || SCOPED || ((allow >> (r_off + 4 * (lane >> 5))) & 1u) != 0u)) {
                if constexpr (TOPMSG) {
                  float s1 = (sc[j] > 0.0f) ? sc[j] : 0.0f;
                  s1 = (s1 > 1.0f) ? 1.0f : s1;
                  // rows 8g .. 8g + 7 are entries 8 (g & 1) .. of half g >> 1: lanes 0-31 test row r_off, lanes 32-63 row r_off + 4 -- a select
                  // between two scalars
                  const uint32_t msg = (lane >> 5) ? msgw[g >> 1][8 * (g & 1) + j + 4] : msgw[g >> 1][8 * (g & 1) + j];
                  if ((u64)msg < (u64)tm.n_messages) {  // (-1 = no message, and whatever else lies outside [0, n_messages))
                    unsigned* slot = tm.best + (size_t)(qtile * SQ + ql) * (size_t)tm.n_messages + msg;
                    const uint32_t v = __float_as_uint(s1) + 1u;
                    // no return value, and behind the compiler's back like the candidate store below, for the same reason
                    asm volatile("global_atomic_umax %0, %1, off" ::"v"(slot), "v"(v) : "memory");
                  }
                  continue;
                }
                const int pos = lds_add_rtn(&cnt_lds[ql], 1);
                if (pos + 1 > CAP - BMT) lds_store_i32(need_compact, 1);  // this buffer could overflow on the next tile
                float s1 = (sc[j] > 0.0f) ? sc[j] : 0.0f;
                s1 = (s1 > 1.0f) ? 1.0f : s1;
                if (pos < CAP) {
                  const u64 key = make_key(s1, (uint32_t)(row_base + r_off) + p.index_base);
                  // issued behind the compiler's back: a store it can see among the pending staging loads makes its wait-count pass drain the
                  // whole queue at the next loop header (on gfx9 loads and stores share vmcnt and are not ordered against each other) -- once
                  // per tile in the LDS-DMA variants, at every K-loop iteration with register staging, whose waits the compiler counts.  An
                  // extra entry in the queue only makes a counted wait wait longer.
                  u64* dst = my_cand + (size_t)ql * CAP + pos;
                  asm volatile("global_store_dwordx2 %0, %1, off" ::"v"(dst), "v"(key) : "memory");
                }
              }
            }
          }
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    TAVB_BARRIER();
    if constexpr (TOPMSG) continue;  // (no buffer to compact; the barrier stays: the waves enter the next tile together, as in every other form)
    if (*need_compact != 0) {  // workgroup-uniform: read after the barrier
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), through the builtin: the compiler's wait-count pass sees the queue empty from here on
      TAVB_BARRIER();
      for (int q = wave; q < SQ; q += S_THREADS / 64) {
        const int n = cnt_lds[q];
        if (n > CAP - BMT) {
          u64* buf = my_cand + (size_t)q * CAP;
          float kth_score;
          const int kept = compact_buffer<CAP, false>(buf, n < CAP ? n : CAP, p.k, lane, 0.0f, 0, &kth_score, nullptr);
          if (lane == 0) {
            cnt_lds[q] = kept;
            if (kept >= p.k && kth_score > thr_lds[q]) thr_lds[q] = kth_score;
          }
          __builtin_amdgcn_s_waitcnt(0x0F70);
        }
      }
      __builtin_amdgcn_s_waitcnt(0x0F70);  // (whatever the compaction left pending: the loop headers see staging loads only)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      TAVB_BARRIER();
      if (tid == 0) *need_compact = 0;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      TAVB_BARRIER();
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the run-ahead LDS-DMA before the block retires
  __syncthreads();
  if constexpr (TOPMSG) return;  // (no lists: p.cand and p.lists are never touched)

  for (int q = wave; q < SQ; q += S_THREADS / 64) {
    const int qg = qtile * SQ + q;
    if (qg >= p.nq) continue;
    const int n = cnt_lds[q];
    const WaveTopK<1> best = best_of_buffer(my_cand + (size_t)q * CAP, n < CAP ? n : CAP, lane);
    u64* out = p.lists + ((size_t)qg * p.list_stride + split) * (size_t)p.k;
    if (lane < p.k) out[lane] = best.key[0];
  }
}

}  // namespace

int skinny_query_tile(int nq) { return nq > SQ32 ? 2 * SQ32 : SQ32; }  // 64-query tiles for batches of 33 and more

bool skinny_supported(int dim, int k, bool f32) {
  return (dim * (f32 ? 4 : 2)) % 64 == 0 && dim > 0 && k >= 1 && k <= 64;
}

// Staging variant of the 32/64-query tile (whole-line steps only): 0 = LDS-DMA ring (ships), 1 = deep corpus ring (4 + 3 slots), 4 = register
// staging four K steps deep, 2 = half tiles (128 rows, two or three workgroups per CU).  The others are measurement variants behind option mfma_sched (8 / 5 / 6; 7 = ring, explicitly): with the per-tile
// drains gone (see the kernel) the ring, the deep ring and register staging 3 / 4 / 6 steps deep all stream 10M x 1536 fp16 rows under 32 queries
// at 6.4 .. 6.5 TB/s -- 40 .. 240 KiB in flight per CU make no difference, the tile is not short of bytes in flight (profiles/r05_mid_batch.md).
constexpr int kSkinnyVariantDefault[2] = {0, 0};  // {fp16, fp32}
// K step of the tile: whole 128-byte lines whenever a row is a multiple of that
static bool skinny_line_steps(int dim, bool f32) { return (dim * (f32 ? 4 : 2)) % 128 == 0; }

static int skinny_variant(int dim, bool f32, int tile, int sched) {
  if (!skinny_line_steps(dim, f32) || sched == 9 || sched == 7) return 0;
  int v = sched == 8 ? 1 : sched == 5 ? 4 : sched == 6 ? 2 : kSkinnyVariantDefault[f32 ? 1 : 0];
  if (tile != 32 && v != 0) v = 0;  // (the 64-query tile keeps the ring)
  const int steps = dim * (f32 ? 4 : 2) / 128;
  if (v >= 3 && steps % v != 0) v = 0;  // a tile starts on register slot 0
  return v;
}

// What launch_skinny_scan instantiates for p (option "last_skinny_kernel"): variant * 10000 + bytes per K step * 100 + queries per tile --
// 12832 = the ring at whole-line steps on 32 queries, 6464 = 64-byte steps on 64 queries, 52832 = register staging.  The launcher switches on it.
int skinny_kernel_id(const MfmaParams& p) {
  const bool f32 = p.f32 != 0;
  const int tile = p.skinny_tile == 64 ? 64 : 32;
  const int step = (skinny_line_steps(p.dim, f32) && p.sched != 9) ? 128 : 64;  // (sched 9: force the 64-byte steps, measurement)
  return skinny_variant(p.dim, f32, tile, p.sched) * 10000 + step * 100 + tile;
}

static int skinny_wg_per_cu(int dim, bool f32, int tile, int sched) {
  const bool line = skinny_line_steps(dim, f32);
  const int v = skinny_variant(dim, f32, tile, sched);
  if (v == 1 || v >= 4) return 1;
  if (v == 2) return f32 ? 3 : 2;  // half tiles: 72 KiB (fp16) / 40 KiB (fp32) of LDS per workgroup
  if (f32) {
    if (tile == 64) return line ? SkinnyGeom<float, 2, 128>::WG_PER_CU : SkinnyGeom<float, 2, 64>::WG_PER_CU;
    return line ? SkinnyGeom<float, 1, 128>::WG_PER_CU : SkinnyGeom<float, 1, 64>::WG_PER_CU;
  }
  if (tile == 64) return line ? SkinnyGeom<_Float16, 2, 128>::WG_PER_CU : SkinnyGeom<_Float16, 2, 64>::WG_PER_CU;
  return line ? SkinnyGeom<_Float16, 1, 128>::WG_PER_CU : SkinnyGeom<_Float16, 1, 64>::WG_PER_CU;
}

int skinny_pick_splits(int64_t rows, int nq_padded, int tile, int n_cu, int dim, bool f32, int sched) {
  const int n_qtiles = nq_padded / tile;
  int splits = (skinny_wg_per_cu(dim, f32, tile, sched) * n_cu) / (n_qtiles > 0 ? n_qtiles : 1);  // every workgroup resident at once
  splits = (splits / 8) * 8;                                                               // whole groups of 8 (one row range per XCD)
  if (splits < 8) splits = 8;
  const int64_t tiles = (rows + BM - 1) / BM;
  if (splits > tiles) splits = (int)tiles;
  return splits;
}

// Same contract as launch_mfma_scan, except that the tile writes sorted lists (p.lists) itself.  p.queries: fp32 corpus ->
// [nq_padded, dim] fp32; fp16 corpus -> [2, nq_padded, dim] fp16, the high and the low plane of the split fp32 queries
// (launch_f32_split_f16).  nq_padded is a multiple of the tile (p.skinny_tile = 32 or 64 queries).
hipError_t launch_skinny_scan(const MfmaParams& p, hipStream_t stream) {
  const bool f32 = p.f32 != 0;
  const int tile = p.skinny_tile == 64 ? 64 : 32;
  const bool topmsg = p.msg_best != nullptr;  // the top-messages form: no candidates, no lists, any k
  if (!skinny_supported(p.dim, topmsg ? 1 : p.k, f32) || p.nq_padded % tile != 0 || p.n_splits < 1 || (!topmsg && !p.workspace)) return hipErrorInvalidValue;
  // top messages: a map aligned for the 16-word scalar loads that covers the launch's rows; one mask or none; the four ring variants only
  if (topmsg && (!p.msg_map || (reinterpret_cast<uintptr_t>(p.msg_map) & 63) != 0 || p.msg_map_rows < p.rows || p.n_messages < 1 || p.scope_planes || p.active ||
                 skinny_variant(p.dim, f32, tile, p.sched) != 0))
    return hipErrorInvalidValue;
  const TopMessages tmsg{p.msg_map, p.msg_best, p.msg_map_rows, p.n_messages};
  if (p.mask && (p.active || (reinterpret_cast<uintptr_t>(p.mask) & 3) != 0)) return hipErrorInvalidValue;  // (no work-list form of the masked tile)
  // per-query scopes: 64-byte aligned plane words (the 16-word scalar loads), whole 32-row blocks per plane, never together with one mask
  if (p.scope_planes && (p.mask || p.active || (reinterpret_cast<uintptr_t>(p.scope_planes) & 63) != 0 || p.scope_stride % 32 != 0 || p.scope_stride < ((p.rows + 31) & ~(int64_t)31)))
    return hipErrorInvalidValue;
  const ScopePlanes planes{p.scope_planes, p.scope_stride};
  const MfmaDeviceParams d = fill_device_params(p, tile, BM);
  const int groups = (p.n_splits + 7) / 8;
  const int grid = groups * d.n_qtiles * 8;
  auto go = [&](auto kern, int lds, auto... mask) -> hipError_t {
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(S_THREADS), lds, stream, d, mask...);
    return hipGetLastError();
  };
  // (one case per instantiation, keyed by the value the "last_skinny_kernel" getter reports: the getter cannot drift from the dispatch)
  // (p.mask: the same seven variants in their MASKED form, the mask as their second argument; p.scope_planes: in their SCOPED form, the planes)
#define TAVB_SKINNY_T(T, NI, STEP, DEEP, DR, HALF)                                                                                   \
  (p.scope_planes ? go(skinny_scan_kernel<T, NI, STEP, DEEP, DR, HALF, true, ScopePlanes>, SkinnyGeom<T, NI, STEP, DEEP, DR, HALF>::LDS, planes) \
   : p.mask ? go(skinny_scan_kernel<T, NI, STEP, DEEP, DR, HALF, true, const uint32_t*>, SkinnyGeom<T, NI, STEP, DEEP, DR, HALF>::LDS, p.mask) \
          : go(skinny_scan_kernel<T, NI, STEP, DEEP, DR, HALF>, SkinnyGeom<T, NI, STEP, DEEP, DR, HALF>::LDS))
#define TAVB_SKINNY(NI, STEP, DEEP, DR, HALF) (f32 ? TAVB_SKINNY_T(float, NI, STEP, DEEP, DR, HALF) : TAVB_SKINNY_T(_Float16, NI, STEP, DEEP, DR, HALF))
  // (top messages: the four ring variants in their unmasked and one-mask form, the map and the best array as their last argument)
#define TAVB_SKINNY_TM_T(T, NI, STEP)                                                                                                                   \
  (p.mask ? go(skinny_scan_kernel<T, NI, STEP, false, 0, false, true, const uint32_t*, TopMessages>, SkinnyGeom<T, NI, STEP>::LDS, p.mask, tmsg) \
          : go(skinny_scan_kernel<T, NI, STEP, false, 0, false, false, TopMessages>, SkinnyGeom<T, NI, STEP>::LDS, tmsg))
#define TAVB_SKINNY_TM(NI, STEP) (f32 ? TAVB_SKINNY_TM_T(float, NI, STEP) : TAVB_SKINNY_TM_T(_Float16, NI, STEP))
  if (topmsg) {
    switch (skinny_kernel_id(p)) {
      case 12832: return TAVB_SKINNY_TM(1, 128);
      case 12864: return TAVB_SKINNY_TM(2, 128);
      case 6432: return TAVB_SKINNY_TM(1, 64);
      case 6464: return TAVB_SKINNY_TM(2, 64);
      default: return hipErrorInvalidValue;
    }
  }
#undef TAVB_SKINNY_TM
#undef TAVB_SKINNY_TM_T
  switch (skinny_kernel_id(p)) {
    case 12832: return TAVB_SKINNY(1, 128, false, 0, false);
    case 12864: return TAVB_SKINNY(2, 128, false, 0, false);
    case 6432: return TAVB_SKINNY(1, 64, false, 0, false);
    case 6464: return TAVB_SKINNY(2, 64, false, 0, false);
    case 22832: return TAVB_SKINNY(1, 128, true, 0, false);   // deep ring
    case 32832: return TAVB_SKINNY(1, 128, false, 0, true);   // half tiles
    case 52832: return TAVB_SKINNY(1, 128, false, 4, false);  // register staging
    default: return hipErrorInvalidValue;
  }
#undef TAVB_SKINNY
#undef TAVB_SKINNY_T
}

}  // namespace tavb
