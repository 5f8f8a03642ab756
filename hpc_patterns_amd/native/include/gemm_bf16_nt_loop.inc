// gemm_bf16_nt_loop.inc — the K loop of the bf16 128^2-tile NT GEMM (both
// operands K-contiguous), double buffered in 64 KiB of LDS. A body
// fragment, not a header: a kernel #includes it where its K loop stands. It
// is text and not a function because a function moves the register
// allocation of the kernels (docs/findings.md #28,
// profiles/gemm_loop_fold.md); included, every kernel compiles to the code
// it had with the loop written out. Used by k_gemm_bf16_nt_db<WM,WN>
// (gemm.hip), k_gemm_bf16_nt_out (gemm_epilogue.hip) and k_gemm_bf16_nt_act
// (gemm_act.hip).
//
// K-tile t+1's 16-byte global_load_lds DMAs are issued BEFORE tile t is
// waited for. The DMAs of a wave retire in order, so a counted vmcnt
// retires exactly tile t's and leaves t+1's in flight; the barriers are raw
// s_barrier + lgkmcnt(0), so nothing drains the queue again (a
// __syncthreads() carries a vmcnt(0)).
//
// In scope at the include:
//   lds             __shared__ __hip_bfloat16[2 * 2 * TILE_HALF]
//   acc             f32x4[MREP][NREP], zeroed; the loop leaves the tile's
//                   sums in it, in the C/D mapping
//   A, B            operand base pointers, rows of K elements; K: int
//   brow, bcol      long: first row and column of this workgroup's tile
//   lane, wid, wr, wc
//   MREP, NREP, WTM, WTN, elems_per_issue, ISSUES
// Nothing is #defined for it: the three kernels differ outside the loop.

  auto stage = [&](int buf, int k0) {
    __hip_bfloat16* dst = lds + (long)buf * 2 * TILE_HALF;
    for (int issue = 0; issue < ISSUES; ++issue) {
      long o_base = (long)issue * elems_per_issue + (long)wid * (64 * 8);
      long o = lds_unskew(o_base + (long)lane * 8);
      int row = (int)(o / BK);
      int kk = (int)(o % BK);
      const __hip_bfloat16* ga = A + (brow + row) * (long)K + k0 + kk;
      const __hip_bfloat16* gb = B + (bcol + row) * (long)K + k0 + kk;
      glds16(ga, dst + o_base);
      glds16(gb, dst + TILE_HALF + o_base);
    }
  };

  stage(0, 0);
  for (int k0 = 0; k0 < K; k0 += BK) {
    const int cur = (k0 / BK) & 1;
    const bool more = (k0 + BK) < K;
    if (more) stage(cur ^ 1, k0 + BK); // next tile's DMA, other buffer
    // retire exactly the CURRENT tile's DMAs (2*ISSUES per thread issued
    // first; FIFO), leaving the prefetch in flight across the barrier
    if (more)
      asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2 * ISSUES) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier(); // current buffer complete for all waves

    const __hip_bfloat16* la = lds + (long)cur * 2 * TILE_HALF;
    const __hip_bfloat16* lb = la + TILE_HALF;
    for (int kk = 0; kk < BK; kk += 32) {
      const int kfrag = kk + 8 * (lane >> 4);
      bf16x8 afrag[MREP], bfrag[NREP];
      for (int m = 0; m < MREP; ++m) {
        int row = wr * WTM + m * 16 + (lane & 15);
        afrag[m] = *(const bf16x8*)(la + lds_skew(row * BK + kfrag));
      }
      for (int n = 0; n < NREP; ++n) {
        int col = wc * WTN + n * 16 + (lane & 15);
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
