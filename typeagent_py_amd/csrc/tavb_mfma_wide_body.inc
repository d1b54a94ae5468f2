// The body of the 128/256-query tile kernel (tavb_mfma_wide.hip: read its header first), included once into each of its three __global__ templates:
// `mfma_scan_kernel` (MASKED = SCOPED = false, mask = nullptr), `mfma_scan_masked_kernel` (MASKED = true, ABL = 0, SPLIT = false) and
// `mfma_scan_scoped_kernel` (SCOPED = true, ABL = 0, SPLIT = false).  In scope where it is included: ABL, NI, N3, N0, N1, SPLIT, BD, M16, MASKED,
// SCOPED, the parameter block `p`, `mask` and `planes`.  Not a header: no include guard, nothing else includes it.
  static_assert(!(MASKED || SCOPED) || (ABL == 0 && !SPLIT), "masked and scoped forms exist for the shipping filter variants only");
  static_assert(!(MASKED && SCOPED), "one mask or one scope per query, not both");
  static_assert(BM6 % 32 == 0 && 160 % 32 == 0 && 80 % 16 == 0, "a 32-row block is one mask word, an 80-row group starts at bit 0 or 16 of one");
  using G = WideGeom<NI>;
  constexpr int BN = G::QT, NT = G::NT, SLOT_B6 = G::SLOT_B, PIECES_B6 = G::PIECES_B, B_RING6 = G::B_RING;
  // BD: the 64 KiB the query ring occupied pay for a THIRD corpus slot -- a corpus piece then has more than a whole K step (~2 us) to land instead
  // of 0.4 .. 1 step (the last pieces of a slab are issued in quarter 1 and needed behind quarter 2: an HBM round trip does not fit)
  constexpr int RA = BD ? 3 : G::RA;
  constexpr int CTRL6 = BD ? 3 * SLOT_A6 : G::CTRL;
  constexpr int PIECES6 = BD ? PIECES_A6 : G::PIECES;
  static_assert(!BD || (NI == 4 && !SPLIT), "the direct query operand is built for the 256-query tile");
  static_assert(!M16 || (NI == 4 && !SPLIT && !BD), "the 16x16x32 form is built for the 256-query filter tile");
  constexpr int QM = M16 ? 40 : NT;  // MFMAs per quarter
  static_assert(N3 + N0 + N1 == PIECES6, "every piece of a step is issued exactly once");
  static_assert(N3 <= QM && N0 <= QM && N1 <= QM && NI + 5 <= NT, "one piece / one fragment read behind an MFMA at most");
  // ABL: what a measurement variant leaves out or changes (launch_mfma_scan; results are garbage unless only the issue order changes)
  constexpr bool NO_MFMA = (ABL & 1) != 0;            // no MFMAs
  constexpr bool NO_STAGING = (ABL & 2) != 0;         // no LDS-DMA
  constexpr bool CORPUS_RESIDENT = (ABL & 4) != 0;    // corpus tile 0 re-read by every block (L2 resident)
  constexpr bool QUERY_RESIDENT = (ABL & 8) != 0;     // the query operand's K step 0 every time (cache resident)
  constexpr bool NO_FRAG_READS = (ABL & 32) != 0;     // no fragment reads
  constexpr bool QUERY_MAJOR = (ABL & 1024) != 0;     // MFMA issue order: query fragment outermost
  constexpr bool SERPENTINE = (ABL & 2048) != 0;      // ... either order walked boustrophedon
  constexpr bool NO_ADMIT = (ABL & ~(1024 | 2048)) != 0;  // no admissions (bit 256 alone, and with every other ablation; the issue order is no ablation)
  extern __shared__ __align__(16) unsigned char smem[];
  float* thr_lds = reinterpret_cast<float*>(smem + CTRL6);
  int* cnt_lds = reinterpret_cast<int*>(smem + CTRL6 + BN * 4);
  lds_flag* need_compact = (lds_flag*)(smem + CTRL6 + BN * 8);

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1;  // rows wm * 160 ..
  const int wn = wave & 1;   // queries wn * 32 * NI ..

  const int b = blockIdx.x;
  const int xcd = b & 7;
  const int t = b >> 3;
  const int qtile = t % p.n_qtiles;
  const int split = (t / p.n_qtiles) * 8 + xcd;
  if (split >= p.n_splits) return;
  if (p.gate != nullptr && *p.gate > p.gate_max) return;  // most of the batch is going to the exact form anyway: this filter phase would be wasted work
  int live_q = p.nq;  // queries that exist: the batch, or -- for a fixed-shape launch over a device-side work list (tavb_rescore.hip) -- the slots in use
  if (p.active != nullptr) {  // nothing to do, or not this kernel's share
    const int live = *p.active;
    if (live <= p.active_min || live > p.active_max || qtile * BN >= live) return;
    live_q = live < live_q ? live : live_q;
  }
  const int64_t r_begin = (int64_t)split * p.rows_per_split;
  const int64_t r_end = (r_begin + p.rows_per_split < p.rows) ? r_begin + p.rows_per_split : p.rows;
  const int logical_block = split * p.n_qtiles + qtile;
  u64* my_cand = p.cand + (size_t)logical_block * BN * CAPW;
  int* my_counts = p.counts + (size_t)logical_block * BN;

  const float thr0 = (p.min_score > 0.0f) ? __uint_as_float(__float_as_uint(p.min_score) - 1u) : -__builtin_inff();
  for (int i = tid; i < BN; i += NT6) {
    // NaN threshold admits nothing; neither does one above 1 (scores are clipped to [0, 1]) -- with that, `score > thr` alone implies
    // `clip(score) >= min_score` (thr >= the float below min_score), and the epilogue needs no second test per row
    float t0 = (p.min_score != p.min_score || p.min_score > 1.0f) ? __builtin_inff() : thr0;
    const int qg0 = qtile * BN + i;
    // padding queries -- and the unused slots of the last live tile of a work list: zero queries, every row scores 0.5, and from the second
    // ladder phase on their thr_in is NaN (the select kernel skips them), so without this they would admit every row of the big phases --
    // admit nothing
    if (qg0 >= live_q) t0 = __builtin_inff();
    else if (p.thr_in && p.thr_in[qg0] > t0) t0 = p.thr_in[qg0];  // k-th best so far: a valid lower bound
    thr_lds[i] = t0;
    cnt_lds[i] = 0;
  }
  if (tid == 0) *need_compact = 0;

  const int D = p.dim;
  const int steps_per_plane = D / 64;
  const int steps_per_tile = SPLIT ? 2 * steps_per_plane : steps_per_plane;
  const uint32_t row_bytes = (uint32_t)D * 2u;
  const char* corpus = reinterpret_cast<const char*>(p.corpus);
  const char* qbase = reinterpret_cast<const char*>(p.queries) + (size_t)qtile * BN * row_bytes;
  const int n_tiles = (r_end > r_begin) ? (int)((r_end - r_begin + BM6 - 1) / BM6) : 0;
  if (n_tiles == 0) {
    for (int i = tid; i < BN; i += NT6) my_counts[i] = 0;  // empty row range: empty buffers
    return;
  }

  // ---- per-lane constants of the K loop: two staging offsets (even / odd piece), three fragment-address terms.
  //      Staging: lane l = row l >> 3 of an 8-row piece, PHYSICAL 16-byte slot l & 7, which holds logical slot
  //      (l & 7) ^ ((row >> 1) & 7); with row = 8 * piece + (l >> 3) that is (l & 7) ^ (4 * (piece & 1) + (l >> 4)).
  int st_even, st_odd;
  uint32_t frag_x, a_lane, b_lane;
  uint32_t frag_x16, a_lane16, b_lane16;  // M16: lane l = row / query l & 15 of a 16-row fragment, halves 8 (l >> 4) .. + 7 of a k32 slice
  {
    int zero = 0;
    asm volatile("" : "+v"(zero));
    const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (unsigned)zero));
    const uint32_t lane_row = (uint32_t)(ln >> 3);
    st_even = (int)(lane_row * row_bytes + (uint32_t)(((ln & 7) ^ (ln >> 4)) * 16));
    st_odd = (int)(lane_row * row_bytes + (uint32_t)(((ln & 7) ^ (4 + (ln >> 4))) * 16));
    const int frag_row = ln & 31;
    frag_x = (uint32_t)(((ln >> 5) ^ ((frag_row >> 1) & 7)) << 4);  // byte (k16 << 5) ^ frag_x within the 128-byte row
    a_lane = (uint32_t)((wm * 160 + frag_row) * 128);              // + mi * 4096
    b_lane = (uint32_t)(B_RING6 + (wn * G::WQ + frag_row) * 128);    // + ni * 4096
    const int frag_row16 = ln & 15;
    frag_x16 = (uint32_t)(((ln >> 4) ^ ((frag_row16 >> 1) & 7)) << 4);  // byte (k32 << 6) ^ frag_x16 within the 128-byte row
    a_lane16 = (uint32_t)((wm * 160 + frag_row16) * 128);              // + row fragment * 2048
    b_lane16 = (uint32_t)(B_RING6 + (wn * G::WQ + frag_row16) * 128);    // + query fragment * 2048
  }
  const __amdgpu_buffer_rsrc_t rsrc_b =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(sgpr_ptr(qbase)), 0, (int)(BN * row_bytes) + (SPLIT ? (int)p.split_plane : 0), 0x00020000);

  // ---- stager.  A "round" is what one K step issues: two slots deep (256-query tile) round S = corpus slab S + 1 then query
  //      slab S + 1; three corpus slots deep (128-query tile) round S = query slab S + 1 FIRST, then corpus slab S + 2, so that
  //      the counted wait of step S ("everything but the newest PIECES_A6 loads has landed") covers query slab S + 1 and corpus
  //      slab S + 1 while corpus slab S + 2 stays in flight.  Piece IDX of a round: its position in that order.
  //      What a piece needs is kept as RUNNING scalar state, advanced once per slab behind its last piece, so that a piece costs its load and
  //      two scalar adds (profiles/r12_kloop_issue.md: recomputed per use, the corpus descriptor alone stood as two clumps of 33 and 27
  //      instructions in front of an MFMA in every K step):
  //        * the corpus descriptor of the tile being staged -- base = its first row, size = its rows that exist (rows past the end of the corpus
  //          read as zero; the epilogue masks them anyway) -- moves on only where the slab wraps to the next tile; past the last tile of the row
  //          range it stays there (harmless reloads of the last tile);
  //        * the scalar offset of a wave's piece 0 (K step x 128 bytes + the wave's first row of the slab) and its LDS address (ring slot + the
  //          wave's first piece); piece J adds J x 8 rows and J KiB.
  const int piece_stride = 8 * (int)row_bytes;                 // global bytes from a piece to the next: 8 rows
  const int sa_soff0 = wave * PIECES_A6 * piece_stride;        // K step 0
  const int sb_soff0 = wave * PIECES_B6 * piece_stride;
  const int sa_lds0 = wave * PIECES_A6 * 1024;                 // ring slot 0
  const int sb_lds0 = B_RING6 + wave * PIECES_B6 * 1024;
  const int tile_bytes = BM6 * (int)row_bytes;
  int sa_kt = 0, sa_tiles_left = n_tiles - 1;  // corpus slab being staged: its K step, tiles of the row range behind its tile
  int sb_kt = 0;                               // query slab being staged
  int sa_soff = sa_soff0, sa_lds = sa_lds0, sb_soff = sb_soff0, sb_lds = sb_lds0;
  const char* sa_base = sgpr_ptr(corpus + (size_t)(CORPUS_RESIDENT ? 0 : r_begin) * row_bytes);
  int64_t sa_left = p.rows - (CORPUS_RESIDENT ? 0 : r_begin);  // rows of the corpus from the staged tile's first row on (> 0)
  auto corpus_rsrc = [&]() {
    // min(sa_left, BM6) on the two halves: there is no scalar 64-bit ordered compare, and the vector one costs a VALU slot and a readfirstlane
    const uint32_t lo = (uint32_t)sa_left, hi = (uint32_t)((uint64_t)sa_left >> 32);
    const int valid = (hi != 0u || lo >= (uint32_t)BM6) ? BM6 : (int)lo;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(sa_base), 0, valid * (int)row_bytes, 0x00020000);
  };
  __amdgpu_buffer_rsrc_t rsrc_a = corpus_rsrc();
  auto stage_a = [&](auto j_tag) {
    constexpr int J = decltype(j_tag)::value;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, (lds_void*)(smem + sa_lds + J * 1024), 16, (J & 1) ? st_odd : st_even, sa_soff + J * piece_stride, 0, 0);
    if constexpr (J == PIECES_A6 - 1) {
      sa_lds = (sa_lds + SLOT_A6 == sa_lds0 + RA * SLOT_A6) ? sa_lds0 : sa_lds + SLOT_A6;
      ++sa_kt;
      sa_soff += 128;
      if constexpr (SPLIT) sa_soff = (sa_kt == steps_per_plane) ? sa_soff0 : sa_soff;  // second plane: the same corpus columns again
      if (sa_kt == steps_per_tile) {  // the slab wraps to the next tile (once in dim / 64 steps)
        sa_kt = 0;
        sa_soff = sa_soff0;
        if (!CORPUS_RESIDENT && sa_tiles_left > 0) {
          --sa_tiles_left;
          sa_base += tile_bytes;
          sa_left -= BM6;
          rsrc_a = corpus_rsrc();
        }
      }
    }
  };
  auto stage_b = [&](auto j_tag) {
    constexpr int BJ = decltype(j_tag)::value;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_b, (lds_void*)(smem + sb_lds + BJ * 1024), 16, (BJ & 1) ? st_odd : st_even, sb_soff + BJ * piece_stride, 0, 0);
    if constexpr (BJ == PIECES_B6 - 1) {
      sb_lds = (sb_lds == sb_lds0) ? sb_lds0 + SLOT_B6 : sb_lds0;
      if constexpr (!QUERY_RESIDENT) {  // ablation 8: the query operand's K step 0 every time (cache resident)
        ++sb_kt;
        sb_soff += 128;
        if constexpr (SPLIT) sb_soff = (sb_kt == steps_per_plane) ? sb_soff0 + (int)p.split_plane : sb_soff;  // on to the low plane
        if (sb_kt == steps_per_tile) {
          sb_kt = 0;
          sb_soff = sb_soff0;
        }
      }
    }
  };
  auto stage_piece = [&](auto idx_tag) {
    constexpr int IDX = decltype(idx_tag)::value;
    if constexpr (BD) {
      stage_a(std::integral_constant<int, IDX>{});
    } else if constexpr (RA == 2) {
      if constexpr (IDX < PIECES_A6) stage_a(std::integral_constant<int, IDX>{});
      else stage_b(std::integral_constant<int, IDX - PIECES_A6>{});
    } else {
      if constexpr (IDX < PIECES_B6) stage_b(std::integral_constant<int, IDX>{});
      else stage_a(std::integral_constant<int, IDX - PIECES_B6>{});
    }
  };
  auto stage_range = [&]<int... I>(std::integer_sequence<int, I...>) { (stage_piece(std::integral_constant<int, I>{}), ...); };
  auto stage_a_all = [&]<int... I>(std::integer_sequence<int, I...>) { (stage_a(std::integral_constant<int, I>{}), ...); };

  // ---- prologue: step 0 whole (three slots: and corpus slab 1), then the first N3 pieces of round 0 (what quarter 3 of a
  //      step "-1" would have issued)
  if constexpr (RA == 2) {
    stage_range(std::make_integer_sequence<int, PIECES6>{});
    stage_range(std::make_integer_sequence<int, N3>{});
    wait_vmcnt<N3>();
  } else {
    stage_a_all(std::make_integer_sequence<int, PIECES_A6>{});  // corpus slab 0
    stage_range(std::make_integer_sequence<int, PIECES6>{});    // "round -1": query slab 0, corpus slab 1
    stage_range(std::make_integer_sequence<int, N3>{});
    wait_vmcnt<PIECES_A6 + N3>();
  }
  __syncthreads();  // step 0 landed everywhere, thresholds initialised (the waits above are counted: nothing is drained)

  // M16: 10 x 8 blocks of 16 x 16 (f32x4) per wave, the same 320 registers; the 20 blocks of rows 80 .. 159 x queries 64 .. 127 of the wave
  // accumulate in VGPRs, the other 60 in AGPRs (the 32 x 32 form's 15 / 5 split)
  using Acc = std::conditional_t<M16, f32x4, f32x16>;
  constexpr int NACC = M16 ? 80 : NT;
  constexpr int NA_TILES = M16 ? 60 : G::NA;
  Acc acc_a[NA_TILES];
  Acc acc_v[NACC - NA_TILES > 0 ? NACC - NA_TILES : 1];

  f16x8 a0[5], b0[M16 ? 2 * NI : NI], a1[5], b1[M16 ? 1 : NI];  // M16: b0 = the wave's 8 query fragments of a k32 slice (b1 unused)
  f16x8 b2[BD ? NI : 1], b3[BD ? NI : 1];  // BD: four rotating sets of query fragments (quarter q multiplies set q, the loads for quarter q + 3 fill set (q + 3) & 3)
  constexpr int BQ_SLICE = (BN / 32) * 1024;  // bytes of one k16 slice of the tile's queries in fragment-major order
  int bq_soff = 0;                            // BD: byte offset (from the tile's queries) of the slice to load next; wraps with the tile
  const int bq_tile_bytes = BN * (int)row_bytes;
  int bq_voff = 0;
  auto bq_load = [&](f16x8(&dst)[BD ? NI : 1]) {  // one slice: this wave's NI fragments (its half of the tile's query blocks)
    if constexpr (BD) {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        dst[ni] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc_b, bq_voff + ni * 1024, bq_soff, 0));
      bq_soff = (bq_soff + BQ_SLICE == bq_tile_bytes) ? 0 : bq_soff + BQ_SLICE;
    }
  };
  {
    const unsigned char* abase = smem + (a_lane + frag_x);
    const unsigned char* bbase = smem + (b_lane + frag_x);
    if constexpr (BD) {
      int zero_b = 0;
      asm volatile("" : "+v"(zero_b));
      const int ln_b = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (unsigned)zero_b));
      bq_voff = ln_b * 16 + wn * NI * 1024;
      bq_load(b0);
      bq_load(b1);
      bq_load(b2);
    } else if constexpr (M16) {
      const unsigned char* abase16 = smem + (a_lane16 + frag_x16);
      const unsigned char* bbase16 = smem + (b_lane16 + frag_x16);
#pragma unroll
      for (int n = 0; n < 2 * NI; ++n) b0[n] = *reinterpret_cast<const f16x8*>(bbase16 + n * 2048);
#pragma unroll
      for (int m = 0; m < 5; ++m) a0[m] = *reinterpret_cast<const f16x8*>(abase16 + m * 2048);
    } else {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) b0[ni] = *reinterpret_cast<const f16x8*>(bbase + ni * 4096);
    }
    if constexpr (!M16) {
#pragma unroll
      for (int mi = 0; mi < 5; ++mi) a0[mi] = *reinterpret_cast<const f16x8*>(abase + mi * 4096);
    }
  }
  int rd = 0, rd_a = 0;  // ring slots (query, corpus) of the step being multiplied, as byte offsets into their rings

  // One quarter: the NT MFMAs of one k16 slice on (fa, fb); behind them, in program order, the NI + 5 fragment reads of the
  // next quarter (ring offsets `noff_a` / `noff_b`, slice NKK) into (na, nb) and the staging pieces the schedule puts into quarter Q.
  auto quarter = [&](auto q_tag, auto first_tag, f16x8(&fa)[5], f16x8(&fb)[NI], f16x8(&na)[5], f16x8(&nb)[NI], int noff_a, int noff_b, auto nkk_tag) {
    constexpr int Q = decltype(q_tag)::value;
    constexpr bool FIRST = decltype(first_tag)::value;  // first quarter of a tile: C = 0
    constexpr int NKK = decltype(nkk_tag)::value;
    const uint32_t kx = (uint32_t)(NKK << 5) ^ frag_x;
    const unsigned char* abase = smem + noff_a + (a_lane + kx);
    const unsigned char* bbase = smem + noff_b + (b_lane + kx);
    auto mfma_at = [&](auto i_tag) {
      constexpr int I = decltype(i_tag)::value;
      // issue order of the NT MFMAs of a slice (measurement, profiles/r06_mfma_power.md): corpus fragment outermost (ships), query fragment
      // outermost (QUERY_MAJOR: the operand whose bits the board's power follows more closely stays put for five MFMAs), and either walked
      // boustrophedon (SERPENTINE: exactly one operand changes between any two consecutive MFMAs)
      constexpr int outer = QUERY_MAJOR ? I / 5 : I / NI;
      constexpr int inner0 = QUERY_MAJOR ? I % 5 : I % NI;
      constexpr int inner = (SERPENTINE && (outer & 1)) ? (QUERY_MAJOR ? 4 : NI - 1) - inner0 : inner0;
      constexpr int mi = QUERY_MAJOR ? inner : outer, ni = QUERY_MAJOR ? outer : inner;
      constexpr int J = mi * NI + ni;  // the accumulator block
      if constexpr (!NO_MFMA) {
        if constexpr (J < NA_TILES)
          mfma_f16<false, true, FIRST>(acc_a[J], fa[mi], fb[ni]);
        else
          mfma_f16<false, false, FIRST>(acc_v[J - NA_TILES], fa[mi], fb[ni]);
      }
      if constexpr (!NO_FRAG_READS) {
        if constexpr (BD) {  // the slice three quarters ahead, straight from L2 into the set the previous quarter has just finished with
          if constexpr (I < NI) nb[I] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc_b, bq_voff + I * 1024, bq_soff, 0));
        } else {
          if constexpr (I < NI) nb[I] = *reinterpret_cast<const f16x8*>(bbase + I * 4096);
        }
        if constexpr (I >= NI && I < NI + 5) na[I - NI] = *reinterpret_cast<const f16x8*>(abase + (I - NI) * 4096);
      }
      if constexpr (!NO_STAGING) {
        constexpr int PC = staging_piece_at<NT, N3, N0, N1>(Q, I);
        if constexpr (PC >= 0) stage_piece(std::integral_constant<int, PC>{});
      }
    };
    [&]<int... I>(std::integer_sequence<int, I...>) { (mfma_at(std::integral_constant<int, I>{}), ...); }
    (std::make_integer_sequence<int, NT>{});
    if constexpr (BD) bq_soff = (bq_soff + BQ_SLICE == bq_tile_bytes) ? 0 : bq_soff + BQ_SLICE;
    if constexpr (NO_MFMA) asm volatile("" ::"v"(fa[0]), "v"(fa[4]), "v"(fb[0]), "v"(fb[NI - 1]));
  };
  // M16 quarter Q: the 5 row fragments of rows 80 H .. 80 H + 79 (H = Q & 1) of k32 slice Q >> 1 (fa) x the 8 query fragments of that slice (b0),
  // query fragment outermost: MFMA i = 5 n + m multiplies row fragment m by query fragment n.  Behind them, in program order: the 5 row fragments of
  // the next quarter (the other row half; ring offset `noff_a`, k32 slice NKK) into na, and the query fragments IN PLACE -- in quarters 1 and 3 all
  // eight, of slice NKK (the next quarter's), b0[n] behind MFMA 5 n + 9, the last one, b0[7], behind MFMA 5 of the next quarter.  Every fragment
  // read thus sits at least five MFMAs behind the last MFMA that reads its register as SrcA / SrcB (the row fragments: a0[m] / a1[m] is last read
  // by MFMA 35 + m and reloaded behind MFMA m of the next quarter).  The ISA's table of required wait states for XDL (MFMA) operations has a
  // write-after-read row for SrcC only ("XDL read VGPR SrcC, VALU write of the same VGPR": 3 wait states at four passes); SrcA / SrcB are read
  // when the MFMA issues.  Five MFMA issues cover even the SrcC figure, so no s_nop is needed anywhere in the loop (the static_asserts below
  // measure each distance from the issue order, m16_query_frag / m16_row_frag).
  auto quarter16 = [&](auto q_tag, auto first_tag, f16x8(&fa)[5], f16x8(&na)[5], int noff_a, int noff_b, auto nkk_tag) {
    constexpr int Q = decltype(q_tag)::value;
    constexpr bool FIRST = decltype(first_tag)::value;  // first quarter of a tile for these accumulators: C = 0
    constexpr int NKK = decltype(nkk_tag)::value;
    constexpr int H = Q & 1;
    const uint32_t kx = (uint32_t)(NKK << 6) ^ frag_x16;
    const unsigned char* abase = smem + noff_a + (a_lane16 + (H ^ 1) * 5 * 2048 + kx);
    const unsigned char* bbase = smem + noff_b + (b_lane16 + kx);
    auto mfma_at = [&](auto i_tag) {
      constexpr int I = decltype(i_tag)::value;
      constexpr int n = m16_query_frag(I), m = m16_row_frag(I), mr = 5 * H + m;
      constexpr bool VB = mr >= 5 && n >= 4;  // accumulator block in VGPRs
      constexpr int J = VB ? (mr - 5) * 4 + (n - 4) : (mr < 5 ? mr * 8 + n : 40 + (mr - 5) * 4 + n);
      if constexpr (!NO_MFMA) {
        if constexpr (VB)
          mfma_f16<true, false, FIRST>(acc_v[J], fa[m], b0[n]);
        else
          mfma_f16<true, true, FIRST>(acc_a[J], fa[m], b0[n]);
      }
      if constexpr (!NO_FRAG_READS) {
        // a reload sits behind MFMA I of this quarter; its register was last read by MFMA m16_last_reader(...) of the previous quarter (row
        // fragments, b0[7]) or of this one (b0[0 .. 6]): the distance counts the MFMAs issued in between, from the issue order itself
        if constexpr (I < 5) {
          static_assert(I + QM - m16_last_reader(false, I) >= 5, "five MFMAs between the last read of a row fragment and its reload");
          na[I] = *reinterpret_cast<const f16x8*>(abase + I * 2048);
        }
        if constexpr ((Q & 1) == 1 && I >= 9 && (I - 9) % 5 == 0) {
          static_assert(I - m16_last_reader(true, (I - 9) / 5) >= 5, "five MFMAs between the last read of a query fragment and its reload");
          b0[(I - 9) / 5] = *reinterpret_cast<const f16x8*>(bbase + ((I - 9) / 5) * 2048);
        }
        if constexpr ((Q & 1) == 0 && I == 5) {
          static_assert(I + QM - m16_last_reader(true, 7) >= 5, "five MFMAs between the last read of a query fragment and its reload");
          b0[7] = *reinterpret_cast<const f16x8*>(bbase + 7 * 2048);
        }
      }
      if constexpr (!NO_STAGING) {
        constexpr int PC = staging_piece_at<QM, N3, N0, N1>(Q, I);
        if constexpr (PC >= 0) stage_piece(std::integral_constant<int, PC>{});
      }
    };
    [&]<int... I>(std::integer_sequence<int, I...>) { (mfma_at(std::integral_constant<int, I>{}), ...); }
    (std::make_integer_sequence<int, QM>{});
    if constexpr (NO_MFMA) asm volatile("" ::"v"(fa[0]), "v"(fa[4]), "v"(b0[0]), "v"(b0[7]));
  };
  using Q0 = std::integral_constant<int, 0>;
  using Q1 = std::integral_constant<int, 1>;
  using Q2 = std::integral_constant<int, 2>;
  using Q3 = std::integral_constant<int, 3>;
  auto step = [&](auto first_tag) {
    if constexpr (M16) {
      // (rows 0-79, k32 #0) (rows 80-159, #0) (rows 0-79, #1) | barrier | (rows 80-159, #1): the first two quarters of a tile start the accumulators
      quarter16(Q0{}, first_tag, a0, a1, rd_a, rd, Q0{});
      quarter16(Q1{}, first_tag, a1, a0, rd_a, rd, Q1{});
      quarter16(Q2{}, std::false_type{}, a0, a1, rd_a, rd, Q1{});
      if constexpr (!NO_STAGING) wait_vmcnt<0>();
      __builtin_amdgcn_s_waitcnt(0xC07F);
      TAVB_BARRIER();
      const int nxt_a = rd_a ^ SLOT_A6;
      quarter16(Q3{}, std::false_type{}, a1, a0, nxt_a, rd ^ SLOT_B6, Q0{});
      rd ^= SLOT_B6;
      rd_a = nxt_a;
    } else if constexpr (BD) {
      quarter(Q0{}, first_tag, a0, b0, a1, b3, rd_a, rd, Q1{});
      quarter(Q1{}, std::false_type{}, a1, b1, a0, b0, rd_a, rd, Q2{});
      quarter(Q2{}, std::false_type{}, a0, b2, a1, b1, rd_a, rd, Q3{});
      // corpus slab S+1 has landed in this wave: behind its last piece (quarter 1 of the PREVIOUS step) came five quarters' query-fragment loads
      // (5 NI) and the ten pieces of slab S+2, which may all still be in flight (loads return in order: the count is exact)
      if constexpr (!NO_STAGING) wait_vmcnt<5 * NI + PIECES_A6>();
      __builtin_amdgcn_s_waitcnt(0xC07F);
      TAVB_BARRIER();
      const int nxt_a = rd_a + SLOT_A6 == RA * SLOT_A6 ? 0 : rd_a + SLOT_A6;
      quarter(Q3{}, std::false_type{}, a1, b3, a0, b2, nxt_a, rd, Q0{});
      rd_a = nxt_a;
    } else {
      quarter(Q0{}, first_tag, a0, b0, a1, b1, rd_a, rd, Q1{});
      quarter(Q1{}, std::false_type{}, a1, b1, a0, b0, rd_a, rd, Q2{});
      quarter(Q2{}, std::false_type{}, a0, b0, a1, b1, rd_a, rd, Q3{});
      // ---- step S+1 has landed in this wave (two slots: nothing newer is in flight; three: only corpus slab S+2 is); the
      //      slots of step S are read out; meet
      if constexpr (!NO_STAGING) wait_vmcnt<(RA == 2 ? 0 : PIECES_A6)>();
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0) through the builtin: visible to the compiler's wait-count pass
      TAVB_BARRIER();
      const int nxt_a = (RA == 2) ? (rd_a ^ SLOT_A6) : (rd_a + SLOT_A6 == RA * SLOT_A6 ? 0 : rd_a + SLOT_A6);
      quarter(Q3{}, std::false_type{}, a1, b1, a0, b0, nxt_a, rd ^ SLOT_B6, Q0{});
      rd ^= SLOT_B6;
      rd_a = nxt_a;
    }
  };

  for (int tile = 0; tile < n_tiles; ++tile) {
    const int64_t row0 = r_begin + (int64_t)tile * BM6;
    const bool tile_full = row0 + BM6 <= r_end;  // wave-uniform: every row of this tile belongs to the row range
    if constexpr (NO_MFMA) {  // MFMAs ablated: give the accumulators a value
#pragma unroll
      for (int i = 0; i < NA_TILES; ++i) acc_a[i] = Acc{};
#pragma unroll
      for (int i = 0; i < NACC - NA_TILES; ++i) acc_v[i] = Acc{};
    }
    step(std::true_type{});
#pragma unroll 1
    for (int kt = 1; kt < steps_per_tile; ++kt) step(std::false_type{});

    // ---- epilogue: admission test on the raw dot products, append .  The asm MFMAs are invisible
    //      to the compiler's hazard recognizer: a 32x32x16 MFMA needs 18 wait states before its result may be read (a 16x16x32 one fewer).
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    int zero_e = 0;
    asm volatile("" : "+v"(zero_e));
    const int lane_e = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (unsigned)zero_e));
    if constexpr (M16) {
      // 16 x 16 blocks: lane l holds query l & 15 of its block, rows 4 (l >> 4) + r, r = 0 .. 3.  One test per (query fragment n, row half h): the
      // 20 scores a lane holds there, 1280 per wave, all against the lane's one threshold.  Pass 0: the VGPR blocks (h = 1, n >= 4), pass 1: the rest.
#pragma unroll
      for (int pass = 0; pass < 2; ++pass)
#pragma unroll
        for (int n = 0; n < 8; ++n) {
          const int ql = wn * G::WQ + n * 16 + (lane_e & 15);
          const float thr = thr_lds[ql];
          const float thr_pre = fmaf(thr, 2.0f, -1.0f) - 4.8e-7f;  // score > thr implies dot > thr_pre (as in the 32 x 32 form)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            constexpr int VT = NACC - NA_TILES;
            const bool vb = h == 1 && n >= 4;
            if (vb != (pass == 0)) continue;
            f32x4 dots[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) {
              const int mr = 5 * h + m;
              dots[m] = vb ? acc_v[((mr - 5) * 4 + (n - 4) + VT) % VT] : acc_a[(mr < 5 ? mr * 8 + n : 40 + (mr - 5) * 4 + n) % NA_TILES];
            }
            float top = dots[0][0];
#pragma unroll
            for (int m = 0; m < 5; ++m)
#pragma unroll
              for (int r = 0; r < 4; ++r) top = __builtin_fmaxf(top, dots[m][r]);
            TAVB_SB();  // one group at a time
            const bool any = !NO_ADMIT && (top > thr_pre);
            if constexpr (NO_ADMIT) asm volatile("" ::"v"(top));
            if (__builtin_amdgcn_ballot_w64(any) != 0ull) {
              // MASKED: the 80 bits of this group, bit i = row group_row + i, in allow[0] (rows 0 .. 31), allow[1] (32 .. 63) and the low half of
              // allow[2] (64 .. 79).  group_row is a multiple of 16: the group starts at bit 0 (h = 0) or 16 (h = 1) of word group_row >> 5 and
              // covers THREE words either way (bits 0 .. 79 or 16 .. 95), W, W + 1 and W + 2; of those only the ones below
              // ceil(r_end / 32) -- the words that hold a row of this row range, never more than ceil(rows / 32) words of the phase -- are
              // loaded, the others read as zero (their rows are behind r_end).  A lane tests bit 16 m + j + 4 (lane >> 4).
              [[maybe_unused]] uint32_t allow[3] = {~0u, ~0u, ~0u};
              if constexpr (MASKED) {
                const int64_t group_row = row0 + wm * 160 + h * 80;
                if (group_row >= r_end) continue;  // wave-uniform: a group behind the row range has no word (and admits nothing either way)
                const int64_t w_first = group_row >> 5, w_end = (r_end + 31) >> 5;  // (w_first < w_end)
                const const_u32* words = (const const_u32*)(uintptr_t)sgpr_ptr(reinterpret_cast<const char*>(mask) + (size_t)w_first * sizeof(uint32_t));
                const uint32_t w0 = words[0];
                const uint32_t w1 = (w_first + 1 < w_end) ? words[1] : 0u;
                const uint32_t w2 = (w_first + 2 < w_end) ? words[2] : 0u;
                const int sh = (int)(group_row & 31);  // 0 or 16
                allow[0] = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);  // a 64-bit funnel shift per word
                allow[1] = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
                allow[2] = (w2 >> sh) & 0xffffu;
                if ((allow[0] | allow[1] | allow[2]) == 0u) continue;  // nothing of this group is allowed
              }
              // as in the 32 x 32 form: one v_cmp per accumulator register gives a wave mask of four rows x 16 queries in an SGPR pair
              const int64_t row_base = row0 + wm * 160 + h * 80 + 4 * (lane_e >> 4);  // + 16 m + r
              const int64_t left64 = r_end - row_base;
              const int rows_left = tile_full ? 80 : (int)(left64 < 80 ? left64 : 80);
#pragma unroll
              for (int m = 0; m < 5; ++m) {
                float sc[4];
                u64 mk[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                  sc[j] = fmaf(dots[m][j], 0.5f, 0.5f);
                  asm volatile("v_cmp_gt_f32 %0, %1, %2" : "=s"(mk[j]) : "v"(sc[j]), "v"(thr));
                }
                if ((mk[0] | mk[1] | mk[2] | mk[3]) == 0ull) continue;  // wave-uniform
                if constexpr (SCOPED) {
                  // the 16 plane words of rows 16 m .. 16 m + 15 of this group for the 32-query block that holds fragment n (half n & 1 of it): lane l
                  // tests row 16 m + j + 4 (l >> 4) for query l & 15, so the lanes (m, j) may admit are four 16-bit halves, one per g = l >> 4
                  const int64_t quad_row = row0 + wm * 160 + h * 80 + 16 * m;  // (a multiple of 16: the load is 64-byte aligned)
                  if (quad_row >= r_end) continue;  // wave-uniform: rows behind the row range have no plane word (and rows_left cuts them either way)
                  const char* words = sgpr_ptr(reinterpret_cast<const char*>(planes.words) +
                                               ((size_t)((qtile * BN + wn * G::WQ) / 32 + n / 2) * (size_t)planes.stride + (size_t)quad_row) * sizeof(uint32_t));
                  const u32x16 pw = *(const const_u32x16*)(uintptr_t)words;  // s_load_dwordx16: lgkmcnt, not vmcnt
                  const int sh = 16 * (n & 1);
#pragma unroll
                  for (int j = 0; j < 4; ++j) {
                    const uint32_t lo = ((pw[j] >> sh) & 0xffffu) | (((pw[j + 4] >> sh) & 0xffffu) << 16);
                    const uint32_t hi = ((pw[j + 8] >> sh) & 0xffffu) | (((pw[j + 12] >> sh) & 0xffffu) << 16);
                    mk[j] &= ((u64)hi << 32) | lo;
                  }
                  if ((mk[0] | mk[1] | mk[2] | mk[3]) == 0ull) continue;  // no scope of these 16 queries holds a row that beats its threshold
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                  const int r_off = 16 * m + j;
                  if (mk[j] == 0ull) continue;
                  // (MASKED: bits at or beyond `rows` in the last word may hold anything -- rows_left cuts those rows)
                  if (((mk[j] >> lane_e) & 1ull) != 0ull && r_off < rows_left &&
                      (!MASKED || ((allow[m >> 1] >> ((m & 1) * 16 + j + 4 * (lane_e >> 4))) & 1u) != 0u)) {
                    const int pos = lds_add_rtn(&cnt_lds[ql], 1);
                    if (pos + 1 > CAPW - BM6) lds_store_i32(need_compact, 1);
                    float s1 = (sc[j] > 0.0f) ? sc[j] : 0.0f;
                    s1 = (s1 > 1.0f) ? 1.0f : s1;
                    if (pos < CAPW) my_cand[(size_t)ql * CAPW + pos] = make_key(s1, (uint32_t)(row_base + r_off) + p.index_base);
                  }
                }
              }
            }
          }
        }
    } else {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int ql = wn * G::WQ + ni * 32 + (lane_e & 31);
        const float thr = thr_lds[ql];
        const float thr_pre = fmaf(thr, 2.0f, -1.0f) - 4.8e-7f;  // score > thr implies dot > thr_pre: fma(dot, 0.5, 0.5) is monotone, the margin covers both roundings
#pragma unroll
        for (int mi = 0; mi < 5; ++mi) {
          constexpr int VT = NT - NA_TILES > 0 ? NT - NA_TILES : 1;
          if ((mi * NI + ni >= NA_TILES) != (pass == 0)) continue;  // pass 0: VGPR tiles, pass 1: AGPR tiles
          const f32x16 dots = (mi * NI + ni < NA_TILES) ? acc_a[mi * NI + ni] : acc_v[(mi * NI + ni - NA_TILES + VT) % VT];
          float top = dots[0];
#pragma unroll
          for (int r = 1; r < 16; ++r) top = __builtin_fmaxf(top, dots[r]);
          TAVB_SB();  // one block at a time
          const bool any = !NO_ADMIT && (top > thr_pre);
          if constexpr (NO_ADMIT) asm volatile("" ::"v"(top));
          if (__builtin_amdgcn_ballot_w64(any) != 0ull) {
            [[maybe_unused]] uint32_t allow = ~0u;  // MASKED: the word of this 32-row block; bit r_off + 4 * (lane >> 5) is the row a lane tests
            [[maybe_unused]] u32x16 plane[2];       // SCOPED: the plane words of this block's 32 rows for the 32 queries of `ni`
            if constexpr (SCOPED) {
              const int64_t block_row = row0 + wm * 160 + mi * 32;  // (a multiple of 32, as r_begin, the tile and the wave's 160 rows are)
              if (block_row >= r_end) continue;  // wave-uniform: a block behind the row range has no plane words (and admits nothing either way)
              const char* words = sgpr_ptr(reinterpret_cast<const char*>(planes.words) +
                                           ((size_t)((qtile * BN + wn * G::WQ) / 32 + ni) * (size_t)planes.stride + (size_t)block_row) * sizeof(uint32_t));
              plane[0] = *(const const_u32x16*)(uintptr_t)words;  // s_load_dwordx16 x 2: lgkmcnt, not vmcnt
              plane[1] = *(const const_u32x16*)(uintptr_t)(words + 16 * sizeof(uint32_t));
              uint32_t any_row = 0u;
#pragma unroll
              for (int w = 0; w < 16; ++w) any_row |= plane[0][w] | plane[1][w];
              if (any_row == 0u) continue;  // no scope of these 32 queries holds a row of this block
            }
            if constexpr (MASKED) {
              const int64_t block_row = row0 + wm * 160 + mi * 32;  // (a multiple of 32, as r_begin, the tile and the wave's 160 rows are)
              if (block_row >= r_end) continue;  // wave-uniform: a block behind the row range has no word (and admits nothing either way)
              const char* word = sgpr_ptr(reinterpret_cast<const char*>(mask) + (size_t)(block_row >> 5) * sizeof(uint32_t));
              allow = *(const const_u32*)(uintptr_t)word;  // a scalar load: lgkmcnt, waited out by the compiler before the test below
              if (allow == 0u) continue;  // nothing of this block is allowed
            }
            // (rare: ~1 % of the blocks once the ladder's thresholds are in -- but each costs the workgroup ~0.3 us, and a batch has a few hundred
            //  thousand of them.)  One compare per row whose result is a WAVE mask in scalar registers (v_cmp into an SGPR pair: no per-lane
            //  bit twiddling); a row nobody admits -- 15 of 16 in the usual case -- costs one scalar test.  An admitted row takes its slot
            //  with one LDS atomic per admitting lane.  Rows past the end of the row range exist only in a range's last tile (wave-uniform).
            const int64_t row_base = row0 + wm * 160 + mi * 32 + 4 * (lane_e >> 5);
            // rows of this block that belong to the row range, seen from this lane's first row (>= 32: all of them)
            const int64_t left64 = r_end - row_base;
            const int rows_left = tile_full ? 64 : (int)(left64 < 64 ? left64 : 64);
#pragma unroll
            for (int g = 0; g < 4; ++g) {  // four rows at a time: their masks stay in scalar registers
              float sc[4];
              u64 m[4];
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                sc[j] = fmaf(dots[4 * g + j], 0.5f, 0.5f);
                asm volatile("v_cmp_gt_f32 %0, %1, %2" : "=s"(m[j]) : "v"(sc[j]), "v"(thr));  // (the builtin ballot goes through a 0/1 VGPR and back)
              }
              if constexpr (SCOPED) {  // rows 8g .. 8g + 7 are words 8 (g & 1) .. of half g >> 1: lanes 0-31 test row r_off, lanes 32-63 row r_off + 4
#pragma unroll
                for (int j = 0; j < 4; ++j) m[j] &= (u64)plane[g >> 1][8 * (g & 1) + j] | ((u64)plane[g >> 1][8 * (g & 1) + j + 4] << 32);
              }
              if ((m[0] | m[1] | m[2] | m[3]) == 0ull) continue;  // wave-uniform: nobody admits any of the four
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int r_off = j + 8 * g;  // row 4 g + j of the accumulator = tile row (r & 3) + 8 (r >> 2) from row_base
                if (m[j] == 0ull) continue;
                // (MASKED: bits at or beyond `rows` in the last word may hold anything -- rows_left cuts those rows)
                if (((m[j] >> lane_e) & 1ull) != 0ull && r_off < rows_left && (!MASKED || ((allow >> (r_off + 4 * (lane_e >> 5))) & 1u) != 0u)) {
                  const int pos = lds_add_rtn(&cnt_lds[ql], 1);
                  if (pos + 1 > CAPW - BM6) lds_store_i32(need_compact, 1);  // this buffer could overflow on the next tile
                  float s1 = (sc[j] > 0.0f) ? sc[j] : 0.0f;
                  s1 = (s1 > 1.0f) ? 1.0f : s1;
                  if (pos < CAPW) my_cand[(size_t)ql * CAPW + pos] = make_key(s1, (uint32_t)(row_base + r_off) + p.index_base);
                }
              }
            }
          }
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    TAVB_BARRIER();
    if (*need_compact != 0) {  // workgroup-uniform: read after the barrier
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      TAVB_BARRIER();
      for (int q = wave; q < BN; q += NT6 / 64) {
        const int n = cnt_lds[q];
        if (n > CAPW - BM6) {
          u64* buf = my_cand + (size_t)q * CAPW;
          const int qg = qtile * BN + q;  // (a padding query admits nothing: never here)
          const float band = p.band ? p.band[qg] : 0.0f;
          float thr_excl;
          uint32_t lost;
          const int kept = compact_buffer<CAPW, true>(buf, n < CAPW ? n : CAPW, p.k, lane_e, band, CAPW - BM6 - 64, &thr_excl, &lost);
          if (lane_e == 0) {
            cnt_lds[q] = kept;
            if (thr_excl > thr_lds[q]) thr_lds[q] = thr_excl;
            if (lost != 0u && p.lost) atomicMax(&p.lost[qg], lost);  // (n > CAPW cannot happen: a tile appends at most BM6 keys)
          }
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      TAVB_BARRIER();
      if (tid == 0) *need_compact = 0;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      TAVB_BARRIER();
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the run-ahead LDS-DMA before the block retires
  __syncthreads();

  // the buffers stay unsorted: tavb::select_band_kernel picks the band over all workgroups' buffers of a query
  for (int i = tid; i < BN; i += NT6) my_counts[i] = cnt_lds[i] < CAPW ? cnt_lds[i] : CAPW;
