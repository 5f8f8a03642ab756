// gemm_bf16_lay_loop.inc — the K loop of the bf16 128^2-tile GEMM for
// operands in any of the four layouts, double buffered in 64 KiB of LDS. A
// body fragment, not a header: a kernel #includes it where its K loop
// stands. It is text and not a function because a function moves the
// register allocation of the kernels (docs/findings.md #28,
// profiles/gemm_loop_fold.md); included, every kernel compiles to the code
// it had with the loop written out. Used by k_gemm_bf16_lay
// (gemm_layout.hip), k_gemm_bf16_lay_splitk (gemm_layout_splitk.hip),
// k_gemm_bf16_lay_out (gemm_epilogue.hip), k_gemm_bf16_lay_act
// (gemm_act.hip) and k_gemm_bf16_batched (gemm_batched.hip).
//
// In scope at the include:
//   A_T, B_N        bool constants: A is stored [K,M], B is stored [K,N]
//   In              __hip_bfloat16
//   lds             __shared__ In[2 * 2 * TILE_HALF], 16-byte aligned
//   acc             f32x4[MREP][NREP], zeroed; the loop leaves the tile's
//                   sums in it, in the C/D mapping
//   A, B            operand base pointers (batch offset already added)
//   brow, bcol      long: first row and column of this workgroup's tile
//   lane, wid, wr, wc
//   MREP = 4, NREP = 2, WTM = 64, WTN = 32, elems_per_issue, ISSUES
// and, #defined by the kernel before the include (the fragment #undefs
// them at its end, so every kernel states all seven):
//   GEMM_LAY_LDA_KM, GEMM_LAY_LDA_MK   row stride of A stored [K,M], [M,K]
//   GEMM_LAY_LDB_KN, GEMM_LAY_LDB_NK   row stride of B stored [K,N], [N,K]
//   GEMM_LAY_K_FIRST   k of the first tile (0, or a split's first k)
//   GEMM_LAY_K_NEXT    k of tile t + 1, t being the loop's counter
//   GEMM_LAY_TRIPS     number of K-tiles, >= 1
// All strides and k are 64-bit. k is absolute: an operand stored [K, X]
// starts at ROW k with its full row stride, a K-contiguous one at column k.
//
// ds_read_b64_tr_b16 needs EXEC all ones (the gather crosses lanes): the
// fragment has no divergent branch, and the kernel around it must have
// none before it, no early return and an exact grid.

  // lane-linear LDS write; the image is in the global chunk each lane takes
  auto stage = [&](int buf, long k0) {
    In* dst = lds + (long)buf * 2 * TILE_HALF;
    for (int issue = 0; issue < ISSUES; ++issue) {
      long o_base = (long)issue * elems_per_issue + (long)wid * (64 * 8);
      // K-contiguous: [128 rows][64 k], skewed
      long o = lds_unskew(o_base + (long)lane * 8);
      int row = (int)(o / BK);
      int kk = (int)(o % BK);
      // X-contiguous: [64 k-rows][128 x]; slot = 16-byte chunk index
      int slot = (int)(o_base / 8) + lane;
      int krow = slot >> 4;
      int x = 8 * ((slot & 15) ^ lay_key(krow));
      const In* ga = A_T ? A + (k0 + krow) * GEMM_LAY_LDA_KM + brow + x
                         : A + (brow + row) * GEMM_LAY_LDA_MK + k0 + kk;
      const In* gb = B_N ? B + (k0 + krow) * GEMM_LAY_LDB_KN + bcol + x
                         : B + (bcol + row) * GEMM_LAY_LDB_NK + k0 + kk;
      glds16(ga, dst + o_base);
      glds16(gb, dst + TILE_HALF + o_base);
    }
  };

  stage(0, GEMM_LAY_K_FIRST);
  const int trips = GEMM_LAY_TRIPS;
  for (int t = 0; t < trips; ++t) {
    const int cur = t & 1;
    const bool more = t + 1 < trips;
    if (more) stage(cur ^ 1, GEMM_LAY_K_NEXT);
    // retire exactly the CURRENT tile's DMAs (2*ISSUES per thread, issued
    // first; FIFO), leaving the prefetch in flight across the barrier. A
    // single-trip loop takes the vmcnt(0) arm at once.
    if (more)
      asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2 * ISSUES) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier(); // current buffer complete for all waves

    const In* la = lds + (long)cur * 2 * TILE_HALF;
    const In* lb = la + TILE_HALF;
    // both k-steps' transposed reads are started at once; step 0 waits
    // for all but step 1's (TR_STEP of them, the most recent), step 1
    // for the rest. nt has none: TR_STEP == 0, and no wait of its own.
    constexpr int KSTEPS = BK / 32;
    constexpr int TR_STEP = 2 * ((A_T ? MREP : 0) + (B_N ? NREP : 0));
    static_assert(KSTEPS == 2 && TR_STEP <= 15, "lgkmcnt is a 4-bit count");
    TrFrag atr[KSTEPS][MREP], btr[KSTEPS][NREP];
    for (int ks = 0; ks < KSTEPS; ++ks) {
      if (A_T)
        for (int m = 0; m < MREP; ++m)
          lay_issue(atr[ks][m], lds_addr(la), wr * WTM + m * 16, 32 * ks,
                    lane);
      if (B_N)
        for (int n = 0; n < NREP; ++n)
          lay_issue(btr[ks][n], lds_addr(lb), wc * WTN + n * 16, 32 * ks,
                    lane);
    }
    for (int ks = 0; ks < KSTEPS; ++ks) {
      const int kfrag = 32 * ks + 8 * (lane >> 4);
      if (A_T || B_N) {
        if (ks == 0)
          asm volatile("s_waitcnt lgkmcnt(%0)" ::"i"(TR_STEP) : "memory");
        else
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      bf16x8 afrag[MREP], bfrag[NREP];
      for (int m = 0; m < MREP; ++m) {
        int row = wr * WTM + m * 16 + (lane & 15);
        if (A_T)
          afrag[m] = lay_take(atr[ks][m]);
        else
          afrag[m] = *(const bf16x8*)(la + lds_skew(row * BK + kfrag));
      }
      for (int n = 0; n < NREP; ++n) {
        int col = wc * WTN + n * 16 + (lane & 15);
        if (B_N)
          bfrag[n] = lay_take(btr[ks][n]);
        else
          bfrag[n] = *(const bf16x8*)(lb + lds_skew(col * BK + kfrag));
      }
      for (int m = 0; m < MREP; ++m)
        for (int n = 0; n < NREP; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[m], bfrag[n], acc[m][n], 0, 0, 0);
    }
    // every wave done READING buf[cur] before the next iteration's
    // prefetch overwrites it — and, behind the last tile, before an
    // epilogue's staged image does
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

#undef GEMM_LAY_LDA_KM
#undef GEMM_LAY_LDA_MK
#undef GEMM_LAY_LDB_KN
#undef GEMM_LAY_LDB_NK
#undef GEMM_LAY_K_FIRST
#undef GEMM_LAY_K_NEXT
#undef GEMM_LAY_TRIPS
