// Batched lookup on fp16 corpora: S = X . Q^T as a dense (rows x D) . (D x queries)
// contraction on the matrix cores (v_mfma_f32_32x32x16_f16, fp32 accumulate), with the
// score map, threshold and per-query top-k selection fused into the epilogue so that
// the [queries x rows] score matrix (41 GB at 1024 x 10M) never exists.
//
// This is the batch the reference leaves as a TODO (storage/sqlite/reltermsindex.py:259-271);
// its semantics are Q independent `fuzzy_lookup_embedding` calls (vectorbase.py:163-190).
// Products of two fp16 values are exact in fp32, so against an oracle fed the same
// fp16-rounded values only the accumulation order differs (fp32 noise ~5e-8).
//
// Decomposition (256-query tile, `mfma_scan_kernel`)
//   * operand roles: A = corpus tile (M = 320 rows), B = query tile (N = 256 queries).  With this orientation the MFMA
//     result layout puts ONE query in each lane (col = lane & 31) and 16 corpus rows in its 16 accumulator registers,
//     so the epilogue's "does this score beat the query's current k-th best" test needs one threshold register per
//     lane and one max3 chain + compare per 32 x 32 block.
//   * workgroup = 4 waves (2 along rows x 2 along queries), one per SIMD with the whole 512-register budget: a
//     160 x 128 sub-tile = 5 x 4 MFMA tiles each.  K advances in steps of 64 halves (whole 128-byte lines); both operand
//     slabs are staged into a two-slot LDS ring by LDS-DMA (`buffer_load ... lds`, 16 B per lane) that runs ahead of the
//     MFMAs across tile boundaries, with raw `s_barrier` and explicit `s_waitcnt`.  Details in the kernel's header.
//   * a workgroup owns one query tile and one contiguous range of corpus rows and walks that range tile by tile
//     (persistent); the workgroups that share a row range (one per query tile) get block ids congruent mod 8 so they
//     run on the same XCD at the same time and the corpus tile is fetched from HBM once and re-read from that XCD's L2.
//   * selection: per (workgroup, query) a candidate buffer of CAPW keys in global memory plus, in LDS, its fill count
//     and the current admission threshold.  A score that beats the threshold is clipped, packed into a key and
//     appended (one LDS atomic per lane per block).  A buffer that could overflow on the next tile is compacted to its
//     BAND (`compact_buffer<CAPW, true>`: the k-th best score by bisection on the score bits, no sort; everything within 2 delta_q below it
//     stays) and the threshold rises to the band's cut.  At the end of a launch the buffers are left as they are;
//     `select_band_kernel` (one workgroup per QUERY) picks the band over all row ranges and derives the next admission threshold.
//   * the host scans the corpus in phases of growing size (threshold ladder, tavb_route.hip): the k-th best score after a
//     phase seeds the admission thresholds of the next (`thr_in`).
//
// Two kernel families share the parameter block and the compaction of tavb_tile.h: the 256-query fp16 tile described
// above (this file) and a 32/64-query tile (`skinny_scan_kernel`, tavb_mfma_skinny.hip) for fp32 and fp16 corpora that carries small
// batches -- and every batch on the reference's fp32 layout -- at HBM speed; `select_band_kernel` is in tavb_select.hip.  On fp16
// corpora the 256-query tile multiplies fp16-ROUNDED queries: it is used as an exact filter, its candidates are rescored with the
// fp32 queries (tavb_rescore.hip).

#include <hip/hip_runtime.h>

#include <type_traits>

#include "tavb_tile.h"

namespace tavb {

namespace {

// ---------------------------------------------------------------------------------------------
// The 256-query tile: four waves with the whole register file each, K steps of whole cache lines.
// (Round 1 shipped an 8-wave 256 x 256 tile with K steps of 32 halves -- "variant 3" -- and a 4-wave 384 x 256 one --
// "variant 5"; this kernel, "variant 6" in the profiles, replaced both: profiles/r02_cfg3_ablation.md.)
//
// Why four waves: an 8-wave 256 x 256 tile sits on the machine balance between the L2 -> CU operand path and the
// matrix pipe (32 KiB of operands per 256 x 256 x 32 step).  Fewer operand bytes per flop needs a bigger tile per CU,
// and the biggest one the register file allows is held by FOUR waves (2 x 2), one per SIMD, each with the full
// 512-register budget.  hipcc picks the AGPR or the VGPR form of an MFMA builtin per FUNCTION, so > 256 accumulators
// cannot be split over the two files through the builtin (hundreds of spills); the MFMAs are therefore inline asm with
// explicit register classes ("+a" / "+v").  A volatile asm is ordered against memory operations, so the program order
// -- MFMA, LDS read, MFMA, ..., MFMA, LDS-DMA -- IS the schedule (no sched_group_barrier).  The asm MFMAs are invisible
// to the compiler's hazard recognizer: the epilogue opens with the wait states an MFMA result needs.
//
// Why whole lines: with K steps of 32 halves a staging piece is sixteen 64-byte HALF lines; the CU's
// texture-address path serves a 1 KiB piece of that shape in ~14 ns from L2 against ~7.7 ns for eight whole 128-byte
// lines (tools/microbench/load_paths.hip, all CUs pulling; profiles/r02_operand_path.md).  A round-1 four-wave kernel
// with 32-half steps kept that path ~90 % busy and its waves stalled at the ISSUE of their staging loads.  Here a K
// step is 64 halves = one 128-byte line per row:
//   * tile = 320 corpus rows x 256 queries; a wave owns 160 x 128 = 5 x 4 MFMA tiles (320 accumulator registers: 15
//     tiles in AGPRs, 5 in VGPRs; the spare AGPRs are where the register allocator parks VGPR values during the
//     epilogue -- with all 256 taken it parks them in scratch, and a scratch reload is a VMEM load queued behind the
//     whole in-flight LDS-DMA).  (384 rows at K = 64 need 2 x 80 KiB of LDS: all 160 KiB, nothing left for the
//     selection state.)
//   * LDS: two slots per operand (A 40 KiB, B 32 KiB each) = 144 KiB.  Rows are 128 bytes; 16-byte slot j of row r
//     sits at physical slot j ^ ((r >> 1) & 7) (applied to the global SOURCE address of the staging loads, because
//     LDS-DMA writes lane-linear, and to the fragment reads), which spreads the 16 lanes of every ds_read_b128 group
//     over the 16 bank slots: SQ_LDS_BANK_CONFLICT = 0 measured.
//   * staging goes through buffer descriptors (`buffer_load_dwordx4 ... lds`): the per-lane part of an address is one
//     of two persistent 32-bit VGPR offsets (even / odd piece: the swizzle term has a piece-parity bit), the piece and the
//     K step are the scalar offset, the tile is the descriptor base, and rows past the end of the corpus are cut off by
//     the descriptor's size (they read as zero; the epilogue masks them anyway).  A piece = 8 rows x 128 bytes; per
//     step 40 A + 32 B pieces = 18 per wave (the 32-half form needed 40 per wave for the same K range).
//   * a step is four quarters (k16 slices) of 20 MFMAs.  Quarter q multiplies fragment set q & 1 while the 9
//     fragment reads of the next quarter fill the other set; one barrier per step, in front of quarter 3:
//       q0, q1, q2: multiply slices 0-2 of slot P; fetch slices 1-3 of slot P
//       ---- vmcnt(0): this wave's pieces of step S+1 landed; lgkmcnt(0): slot P read out; s_barrier ----
//       q3: multiply slice 3; fetch slice 0 of slot P^1 (step S+1, across tile boundaries too)
//     Slot P is then free: the pieces of step S+2 are issued behind the MFMAs of q3 (N3 of them), of the next q0 (N0)
//     and q1 (N1) -- corpus pieces first, they have the longest way -- and have until the next barrier to land.
//   * the first quarter of a tile multiplies into a ZERO C operand instead of clearing 320 registers.
//   * NI = 2 (the 128-query width, WideGeom<2>): a wave owns 160 x 64 = 10 accumulator blocks, all in AGPRs; half the MFMAs per
//     step no longer cover the loaded HBM latency with one corpus slab in flight, and this width has the LDS for a THIRD
//     corpus slot (3 x 40 + 2 x 16 KiB): a round then stages query slab S + 1 first and corpus slab S + 2 behind it, and the
//     wait in front of quarter 3 is counted (`vmcnt(10)`: everything but the ten corpus pieces of slab S + 2 has landed).
//     HBM-bound: 5.8 TB/s at 128 queries (profiles/r02_mid_batch.md).
//   * M16 (the default of the 256-query filter tile, option mfma_shape = 16; profiles/r09_mfma_shape.md): the same tile, ring, barrier and
//     epilogue on v_mfma_f32_16x16x32_f16.  The kernel runs at the board's power limit; in bare MFMA loops on random data the chip held a
//     higher clock on this shape at the same cycles per flop, which is the expected source of the gain (profiles/r09_mfma_shape.md).  A wave's 160 x 128 is 10 x 8 blocks of 16 x 16 (f32x4: the same 320 registers, 60 blocks in AGPRs, 20 in
//     VGPRs); a quarter is one k32 slice x one 80-row half x the 8 query fragments = 40 MFMAs, the four quarters of a step (rows 0-79, k32 #0)
//     (80-159, #0) (0-79, #1) | barrier | (80-159, #1).  Row fragments double-buffer (5 + 5); the 8 query fragments serve two quarters and are
//     reloaded in place in quarters 1 and 3, so the operands stay at 72 registers.  Per k32 slice a wave still reads 10 row and 8 query
//     fragments of 1 KiB: LDS bytes per flop are unchanged.  The SPLIT and BD forms and the 128-query tile stay on 32x32x16.
// Measured and rejected (profiles/r02_cfg3_ablation.md): touching the corpus lines of the step 1 / 2 / 4 steps ahead
// into L2 with one 4-byte load per line (-3 .. -6 %); other piece-per-quarter schedules (no difference).
// ---------------------------------------------------------------------------------------------
constexpr int SLOT_A6 = BM6 * 128;  // 40 KiB
constexpr int PIECES_A6 = BM6 / 8 / 4;  // per wave per step: 10

// NI = 32-query MFMA blocks per wave along the query axis: 4 (256-query workgroup tile) or 2 (128-query tile, for batches of
// 65 .. 128 queries: half the MFMAs and half the query-operand traffic per corpus byte -- HBM-bound instead of padding-bound)
template <int NI>
struct WideGeom {
  static constexpr int QT = 64 * NI;           // queries per workgroup tile
  static constexpr int WQ = 32 * NI;           // ... per wave
  static constexpr int NT = 5 * NI;            // 32 x 32 accumulator blocks per wave: 20 or 10
  static constexpr int NA = NI == 4 ? 15 : NT; // blocks 0 .. NA-1 accumulate in AGPRs, the rest in VGPRs (the spare AGPRs are where the allocator parks VGPR values in the epilogue: no scratch)
  static constexpr int SLOT_B = QT * 128;      // 32 or 16 KiB
  // corpus ring: the 128-query tile is HBM-bound and has the LDS for a third slot (3 x 40 + 2 x 16 KiB): the corpus slab of
  // step S + 2 is in flight while step S is multiplied (one slab in flight left the tile latency-bound at 5.2 TB/s)
  static constexpr int RA = NI == 2 ? 3 : 2;
  static constexpr int B_RING = RA * SLOT_A6;  // the query ring (always two slots) sits behind the corpus ring
  static constexpr int CTRL = B_RING + 2 * SLOT_B;
  static constexpr int LDS = CTRL + QT * 8 + 16;
  static constexpr int PIECES_B = QT / 8 / 4;  // per wave per step: 8 or 4
  static constexpr int PIECES = PIECES_A6 + PIECES_B;
};

// index of the staging piece issued behind MFMA `i` of quarter `q` (-1: none): n pieces spread evenly over the NT MFMAs
template <int NT, int N3, int N0, int N1>
constexpr int staging_piece_at(int q, int i) {
  const int n = q == 3 ? N3 : q == 0 ? N0 : q == 1 ? N1 : 0;
  const int base = q == 3 ? 0 : q == 0 ? N3 : N3 + N0;
  for (int j = 0; j < n; ++j)
    if ((j * NT + NT / 2) / n == i) return base + j;
  return -1;
}

// M16 issue order of a 40-MFMA quarter: MFMA i multiplies row fragment m16_row_frag(i) by query fragment m16_query_frag(i) (query fragment
// outermost); m16_last_reader: the last MFMA of a quarter that reads a given query (or row) fragment as an operand
constexpr int m16_query_frag(int i) { return i / 5; }
constexpr int m16_row_frag(int i) { return i % 5; }
constexpr int m16_last_reader(bool query, int f) {
  int last = -1;
  for (int i = 0; i < 40; ++i)
    if ((query ? m16_query_frag(i) : m16_row_frag(i)) == f) last = i;
  return last;
}

// One MFMA of the K loop as inline asm with an explicit register class for the accumulator (see "Why four waves"): the 16x16x32 or the 32x32x16
// shape, C / D in AGPRs or VGPRs, accumulating or -- the first quarter of a tile -- multiplying into a zero C operand.
template <bool M16, bool AGPR, bool ZERO_C, typename Acc>
__device__ __forceinline__ void mfma_f16(Acc& acc, const f16x8& a, const f16x8& b) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
#define TAVB_MFMA_ASM(OP)                                                                                                                          \
  if constexpr (ZERO_C && AGPR) asm volatile(OP " %0, %1, %2, 0" : "=a"(acc) : "v"(__builtin_bit_cast(i32x4, a)), "v"(__builtin_bit_cast(i32x4, b)));    \
  else if constexpr (ZERO_C) asm volatile(OP " %0, %1, %2, 0" : "=&v"(acc) : "v"(__builtin_bit_cast(i32x4, a)), "v"(__builtin_bit_cast(i32x4, b)));      \
  else if constexpr (AGPR) asm volatile(OP " %0, %1, %2, %0" : "+a"(acc) : "v"(__builtin_bit_cast(i32x4, a)), "v"(__builtin_bit_cast(i32x4, b)));        \
  else asm volatile(OP " %0, %1, %2, %0" : "+v"(acc) : "v"(__builtin_bit_cast(i32x4, a)), "v"(__builtin_bit_cast(i32x4, b)))
  if constexpr (M16) {
    TAVB_MFMA_ASM("v_mfma_f32_16x16x32_f16");
  } else {
    TAVB_MFMA_ASM("v_mfma_f32_32x32x16_f16");
  }
#undef TAVB_MFMA_ASM
}

// SPLIT: the queries arrive as TWO fp16 planes (q = hi + lo to 2^-22) and a tile runs its K loop twice over the corpus rows, once per plane, into
// the same accumulators: fp32 query x fp16 row like the 64-query exact tile, at the wide tile's rate -- the bounded fallback for batches in which
// MANY queries have more near-duplicates than a band holds (tavb_rescore.hip).  Twice the MFMAs; only this instantiation pays for it.
// BD ("B direct"): the query operand does not go through LDS at all.  The library lays the fp16 queries out in MFMA-FRAGMENT-MAJOR order (1 KiB per
// (K step, k16 slice, 32-query block): lane l = query l & 31, halves 8 (l >> 5) .. + 7 of the slice -- query_prepare_kernel), so a fragment is ONE
// coalesced 16 B-per-lane load out of L2 straight into the registers the MFMA reads; four register sets rotate, the loads run three quarters
// (~1.2 us) ahead.  Per K step the LDS then moves 120 KiB instead of 216 (no query slab written, no query fragments read); the price is that
// both row halves of the workgroup load the same fragments (L2 -> CU traffic 104 KiB per step instead of 72).
// MASKED (the filter pass of a masked batch, tavb_route.hip::search_masked_wide): a row is a candidate only if its bit is set in an allow-mask
// (tavb.h "row masks": uint32 words, row r = bit r & 31 of word r >> 5).  The kernel's text is tavb_mfma_wide_body.inc, the body of two __global__
// templates: `mfma_scan_kernel` (MASKED = false: its name, its one argument and its instructions are what they were before the parameter
// existed -- a shared function inlined into both changed the unmasked code) and `mfma_scan_masked_kernel`, whose ONE extra argument is the
// mask -- MfmaDeviceParams does not know about it.  The pointer names the word of the launch's first row, a multiple of 32 in the
// mask's numbering (the launcher and run_tile_ladder check); every row0 is then a multiple of 32 too (row ranges are whole 320-row tiles).  The
// bit test sits in the admission SLOW path only, behind the ballot: the words are wave-uniform and come in through the scalar data path
// (constant address space: lgkmcnt, never vmcnt -- the staging queue is not drained), the K loop and the `top > thr_pre` test are untouched.
// SCOPED (the filter pass of a scoped batch, tavb_route.hip::search_scoped_wide): one scope PER QUERY.  A third __global__ template around the
// same text, `mfma_scan_scoped_kernel`, whose one extra argument is the membership PLANES of the batch (scope_planes_kernel, tavb_mask.hip): for
// every block of 32 queries of the tile-padded batch one uint32 per row of the span, bit i = the scope of query 32 * block + i holds the row;
// `stride` words from one block's plane to the next; `words` names the word of the launch's first row in plane 0 (a multiple of 32 rows into
// the span, 64-byte aligned).  Like the one mask's word, the plane words are read only in the admission slow path, behind the ballot, through
// the scalar data path (lgkmcnt); nothing is stored that the other forms do not store.
//   * 32 x 32 form: a lane is (half << 5) | query of the 32-query block ni and tests row r_off + 4 * half of the 32-row block mi; the lanes row
//     pair (r_off, r_off + 4) may admit are plane[r_off] | plane[r_off + 4] << 32 of plane block (qtile * BN + wn * WQ) / 32 + ni -- one
//     scalar AND into the compare's wave mask.  The block's 32 words come in as two 16-word loads; all zero: the block is skipped.
//   * 16 x 16 form: lane l holds query l & 15 of query fragment n and rows 16 m + j + 4 (l >> 4) of its 80-row group; fragment n is half n & 1
//     of plane block (qtile * BN + wn * WQ) / 32 + n / 2.  The lanes row quadruple (m, j) may admit are the 16-bit halves
//     (plane[16 m + j + 4 g] >> 16 (n & 1)) & 0xffff at bits 16 g, g = 0 .. 3: one 16-word scalar load per m that has a candidate at all (64-byte
//     aligned: a group starts at a multiple of 16 rows), the four masks assembled in scalar registers.
struct ScopePlanes {
  const uint32_t* words;
  int64_t stride;
};
typedef const __attribute__((address_space(4))) uint32_t const_u32;
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
typedef const __attribute__((address_space(4))) u32x16 const_u32x16;
template <int ABL, int NI, int N3, int N0, int N1, bool SPLIT = false, bool BD = false, bool M16 = false>
__global__ void __launch_bounds__(NT6) mfma_scan_kernel(const MfmaDeviceParams p) {
  constexpr bool MASKED = false, SCOPED = false;
  [[maybe_unused]] const uint32_t* const mask = nullptr;
  [[maybe_unused]] constexpr ScopePlanes planes{nullptr, 0};
#include "tavb_mfma_wide_body.inc"
}

// the MASKED form of the shipping filter variants (launch_mfma_scan): the same text with the bit test compiled in
template <int NI, int N3, int N0, int N1, bool BD = false, bool M16 = false>
__global__ void __launch_bounds__(NT6) mfma_scan_masked_kernel(const MfmaDeviceParams p, const uint32_t* mask) {
  constexpr int ABL = 0;
  constexpr bool SPLIT = false, MASKED = true, SCOPED = false;
  [[maybe_unused]] constexpr ScopePlanes planes{nullptr, 0};
#include "tavb_mfma_wide_body.inc"
}

// the SCOPED form of the same four variants: the per-query test compiled in instead
template <int NI, int N3, int N0, int N1, bool BD = false, bool M16 = false>
__global__ void __launch_bounds__(NT6) mfma_scan_scoped_kernel(const MfmaDeviceParams p, const ScopePlanes planes) {
  constexpr int ABL = 0;
  constexpr bool SPLIT = false, MASKED = false, SCOPED = true;
  [[maybe_unused]] const uint32_t* const mask = nullptr;
#include "tavb_mfma_wide_body.inc"
}

}  // namespace

// 128-query tiles when they leave less padding than 256-query tiles (up to 128 queries: one HBM-bound pass instead of a
// half-empty 256-query tile; 257 .. 384 and 513 .. 640: measured 6 % and 3.5 % faster, profiles/r02_mid_batch.md)
int mfma_query_tile(int nq) {
  const int n128 = (nq + 127) / 128;
  return ((n128 & 1) && n128 <= 5) ? 128 : BN;
}

// ... and 128-query tiles on a corpus so small that 256-query tiles would give a CU fewer than four tiles to walk (query tiles x corpus
// tiles <= 4 n_cu): twice the workgroups or half the tile, half the all-admitted epilogue of a workgroup's first tile -- 256 queries over
// 1000 / 5000 / 20000 / 50000 fp16 rows 0.131 / 0.157 / 0.181 / 0.238 -> 0.090 / 0.116 / 0.141 / 0.197 ms (257 queries took three 128-query
// tiles all along and were faster than 256), 1024 queries over 30720 / 50000 rows 0.317 / 0.380 -> 0.264 / 0.342 ms, 512 over 120000 rows
// 0.392 -> 0.367; beyond that the wider tile's operand reuse wins (1024 queries over 250k rows: 0.910 against 0.927 ms).  tools/regime_sweep.py,
// profiles/r06_regime_sweep.md
int mfma_query_tile_for(int nq, int64_t rows, int n_cu) {
  const int qt = mfma_query_tile(nq);
  if (qt == 128) return qt;
  const int64_t corpus_tiles = (rows + BM6 - 1) / BM6;
  const int64_t wgs = (int64_t)((nq + BN - 1) / BN) * corpus_tiles;
  return wgs <= 4 * (int64_t)n_cu ? 128 : qt;
}

// k: the band selection holds any k the fused selections serve (a band of k + its 2-delta neighbourhood has to fit the 640 keys a candidate
// buffer keeps between compactions and the 1024 of the select kernel: k = 256 leaves the same slack as k = 32 on isotropic data)
bool mfma_supported(int dim, int k) { return dim % BK == 0 && dim >= BK && dim <= 16384 && k >= 1 && k <= TAVB_MAX_FUSED_K; }

int mfma_pick_splits(int64_t rows, int nq_padded, int tile, int n_cu) {
  // One workgroup per CU and all of them resident at once: the grid is (groups of 8 row ranges) x query tiles x 8, so the
  // number of row ranges is a multiple of 8 with groups * n_qtiles * 8 <= n_cu.  (85 ranges for 3 query tiles made 264
  // workgroups on 256 CUs: a second scheduling round for the last 8, and a 768-query batch slower than a 1024-query one.)
  const int n_qtiles = nq_padded / tile > 0 ? nq_padded / tile : 1;
  int splits = (n_cu / (8 * n_qtiles)) * 8;
  if (splits < 8) splits = 8;
  const int64_t tiles = (rows + BM - 1) / BM;
  if (splits > tiles) splits = (int)tiles;
  return splits;
}

// candidate buffers of a launch: nq_padded = tiles x queries per tile; the 256-query tile has the deeper buffers
size_t mfma_workspace_bytes(int n_splits, int nq_padded, bool wide) {
  return (size_t)n_splits * (size_t)nq_padded * (wide ? CAPW : CAP) * sizeof(u64);
}

int mfma_tile_shape(const MfmaParams& p) {
  // the 16x16x32 form exists for the 256-query filter tile (not SPLIT, not BD) and its two like-for-like ablations; everything else is 32x32x16
  if (p.shape != 16 || p.wide_tile == 128 || p.split_plane > 0) return 32;
  if (p.ablate != 0) return (p.ablate == 256 || p.ablate == 258) ? 16 : 32;
  return (p.bdirect || p.sched != 0) ? 32 : 16;
}

hipError_t launch_mfma_scan(const MfmaParams& p, hipStream_t stream) {
  const int tile = p.wide_tile == 128 ? 128 : BN;
  if (!mfma_supported(p.dim, p.k) || p.nq_padded % tile != 0 || p.n_splits < 1) return hipErrorInvalidValue;
  if (!p.workspace || !p.counts) return hipErrorInvalidValue;
  // a masked launch: the shipping filter variants only (no work list, no exact SPLIT form, no measurement variant), a word-aligned pointer
  if (p.mask && (p.active || p.split_plane > 0 || p.ablate != 0 || p.sched != 0 || (reinterpret_cast<uintptr_t>(p.mask) & 3) != 0)) return hipErrorInvalidValue;
  // a scoped launch: the same restrictions, never together with one mask; 64-byte aligned plane words (the 16-word scalar loads), whole
  // 32-row blocks per plane, a plane for every block of 32 queries of the padded batch
  if (p.scope_planes && (p.mask || p.active || p.split_plane > 0 || p.ablate != 0 || p.sched != 0 || (reinterpret_cast<uintptr_t>(p.scope_planes) & 63) != 0 ||
                         p.scope_stride % 32 != 0 || p.scope_stride < ((p.rows + 31) & ~(int64_t)31)))
    return hipErrorInvalidValue;
  const ScopePlanes planes{p.scope_planes, p.scope_stride};
  MfmaDeviceParams d = fill_device_params(p, tile, BM6);
  if ((p.mask || p.scope_planes) && d.rows_per_split % 32 != 0) return hipErrorInvalidValue;  // (a whole number of 320-row tiles: every row0 is a multiple of 32)
  d.counts = p.counts;
  d.band = p.band;
  d.lost = p.lost;
  d.split_plane = p.split_plane;
  d.gate = p.gate;
  d.gate_max = p.gate_max;
  // grid: groups of 8 consecutive block ids = 8 different row ranges (one per XCD)
  const int groups = (p.n_splits + 7) / 8;
  const int grid = groups * d.n_qtiles * 8;
  auto go = [&](auto kern, int threads, int lds, auto... mask) -> hipError_t {
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, stream, d, mask...);
    return hipGetLastError();
  };
  // `ablate` modes exist to time parts of a kernel (results are garbage): see profiles/r02_cfg3_ablation.md
  {
    if (p.dim % 64 != 0) return hipErrorInvalidValue;
    constexpr int LDS256 = WideGeom<4>::LDS, LDS128 = WideGeom<2>::LDS;
    if (p.split_plane > 0) {
      if (tile != BN) return hipErrorInvalidValue;
      return go(mfma_scan_kernel<0, 4, 8, 6, 4, true>, NT6, LDS256);
    }
    if (p.mask) {  // the four variants the filter pass selects at default options, in their MASKED form: the mask is their second argument
      if (tile == 128) return go(mfma_scan_masked_kernel<2, 6, 4, 4>, NT6, LDS128, p.mask);
      if (mfma_tile_shape(p) == 16) return go(mfma_scan_masked_kernel<4, 8, 6, 4, false, true>, NT6, LDS256, p.mask);
      if (p.bdirect) return go(mfma_scan_masked_kernel<4, 4, 3, 3, true>, NT6, 3 * SLOT_A6 + BN * 8 + 16, p.mask);
      return go(mfma_scan_masked_kernel<4, 8, 6, 4>, NT6, LDS256, p.mask);
    }
    if (p.scope_planes) {  // ... and in their SCOPED form: the membership planes are their second argument
      if (tile == 128) return go(mfma_scan_scoped_kernel<2, 6, 4, 4>, NT6, LDS128, planes);
      if (mfma_tile_shape(p) == 16) return go(mfma_scan_scoped_kernel<4, 8, 6, 4, false, true>, NT6, LDS256, planes);
      if (p.bdirect) return go(mfma_scan_scoped_kernel<4, 4, 3, 3, true>, NT6, 3 * SLOT_A6 + BN * 8 + 16, planes);
      return go(mfma_scan_scoped_kernel<4, 8, 6, 4>, NT6, LDS256, planes);
    }
    if (tile == 128) {
      switch (p.ablate) {  // (measurement: what bounds the 128-query width, profiles/r05_mid_batch.md)
        case 1: return go(mfma_scan_kernel<1, 2, 6, 4, 4>, NT6, LDS128);      // no MFMAs
        case 256: return go(mfma_scan_kernel<256, 2, 6, 4, 4>, NT6, LDS128);  // no admissions
        case 257: return go(mfma_scan_kernel<257, 2, 6, 4, 4>, NT6, LDS128);  // neither: staging, fragment reads, barriers
        case 264: return go(mfma_scan_kernel<264, 2, 6, 4, 4>, NT6, LDS128);  // no admissions, query operand cache resident
        default: return go(mfma_scan_kernel<0, 2, 6, 4, 4>, NT6, LDS128);
      }
    }
    if (mfma_tile_shape(p) == 16) {  // v_mfma_f32_16x16x32_f16: the default
      switch (p.ablate) {
        case 256: return go(mfma_scan_kernel<256, 4, 8, 6, 4, false, false, true>, NT6, LDS256);  // everything except admissions
        case 258: return go(mfma_scan_kernel<258, 4, 8, 6, 4, false, false, true>, NT6, LDS256);  // no LDS-DMA, no admissions
        default: return go(mfma_scan_kernel<0, 4, 8, 6, 4, false, false, true>, NT6, LDS256);
      }
    }
    if (p.bdirect && p.ablate == 0) return go(mfma_scan_kernel<0, 4, 4, 3, 3, false, true>, NT6, 3 * SLOT_A6 + BN * 8 + 16);  // queries in fragment-major order (query_prepare_kernel)
    switch (p.ablate) {
      case 256: return go(mfma_scan_kernel<256, 4, 8, 6, 4>, NT6, LDS256);  // everything except admissions
      case 260: return go(mfma_scan_kernel<260, 4, 8, 6, 4>, NT6, LDS256);  // same, corpus tile 0 re-read by every block (L2 resident)
      case 264: return go(mfma_scan_kernel<264, 4, 8, 6, 4>, NT6, LDS256);  // same as 256, query operand K step 0 re-read (cache resident)
      case 268: return go(mfma_scan_kernel<268, 4, 8, 6, 4>, NT6, LDS256);  // both operands cache resident
      case 258: return go(mfma_scan_kernel<258, 4, 8, 6, 4>, NT6, LDS256);  // no LDS-DMA, no admissions
      case 1282: return go(mfma_scan_kernel<1282, 4, 8, 6, 4>, NT6, LDS256);  // the same in the other MFMA issue orders (sched 3 / 4 / 5)
      case 2306: return go(mfma_scan_kernel<2306, 4, 8, 6, 4>, NT6, LDS256);
      case 3330: return go(mfma_scan_kernel<3330, 4, 8, 6, 4>, NT6, LDS256);
      default: break;
    }
    switch (p.sched) {  // staging pieces per quarter (q3, q0, q1), MFMA issue order: measurement
      case 1: return go(mfma_scan_kernel<0, 4, 10, 8, 0>, NT6, LDS256);
      case 2: return go(mfma_scan_kernel<0, 4, 6, 6, 6>, NT6, LDS256);
      case 3: return go(mfma_scan_kernel<1024, 4, 8, 6, 4>, NT6, LDS256);  // query fragment outermost
      case 4: return go(mfma_scan_kernel<2048, 4, 8, 6, 4>, NT6, LDS256);  // corpus fragment outermost, boustrophedon
      case 5: return go(mfma_scan_kernel<3072, 4, 8, 6, 4>, NT6, LDS256);  // query fragment outermost, boustrophedon
      default: return go(mfma_scan_kernel<0, 4, 8, 6, 4>, NT6, LDS256);
    }
  }
  return hipErrorInvalidValue;
}

}  // namespace tavb
