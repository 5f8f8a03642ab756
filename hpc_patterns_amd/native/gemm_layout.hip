// gemm_layout.hip — K7 operand layouts: the bf16 128^2-tile GEMM for
// operands that are NOT K-contiguous, C[M,N] = op(A) @ op(B) with
//
//   layout  A as stored  B as stored  template <A_T, B_N>
//   nn      [M,K]        [K,N]        <false, true>
//   tn      [K,M]        [K,N]        <true,  true>
//   tt      [K,M]        [N,K]        <true,  false>
//
// (row-major names, transA then transB; nt is every other kernel of the
// family). These are the two backward products of a linear layer on the
// tensors as they are stored: no t().contiguous() copy in HBM.
//
// One body in the double-buffered 8-wave structure of
// k_gemm_bf16_nt_db<2,4>: tile t+1's 16-byte global_load_lds DMAs are
// issued before tile t is waited for, a counted vmcnt retires exactly
// tile t, raw barriers, 64 KiB LDS, the same C/D epilogue.
//
// A K-contiguous operand is staged and read as in the NT kernels
// (lds_skew image, ds_read_b128). An operand stored [K, X] (X = M or N
// contiguous) has the K-tile [64 k-rows][128 x]: 256-byte rows, 16 KiB,
// the same TILE_HALF and the same 2 DMAs per thread, so the vmcnt count
// is the NT kernels'. global_load_lds writes lane-linear, so the LDS
// image is made by WHICH global 16-byte chunk each lane fetches: LDS
// chunk slot p of row r holds global chunk p ^ lay_key(r) (lay_off
// below; an involution per row, so store and read share it). One wave
// issue covers 4 whole rows. The fragments come out of
// ds_read_b64_tr_b16, which hands each 16-lane group a 4-row x 16-column
// block column-major: two of them per 16x16x32 operand fragment put
// k = kk + 8*(lane>>4) + 0..7 of column x0 + (lane&15) into the lane —
// the k, in the slot, that the NT kernels' ds_read_b128 delivers. The
// MFMAs therefore see the same operands in the same order, and the
// result is bit-identical to bf16_db8 on a materialised transpose.
//
// The instruction needs every lane's address 8-byte aligned and in the
// tile, and EXEC all ones (the gather crosses lanes): the kernel has no
// divergent branch and no early return, the grid is exact, and the
// launcher refuses every shape that is not a whole number of tiles.
// Derivation of the image and the bank count: docs/gemm.md, "Operand
// layouts"; tests/test_gemm_layout_logic.py enumerates every read.

#include "include/hpk.h"
#include "include/gemm_device.h"
#include "include/gemm_layout_device.h"

#include <hip/hip_bf16.h>

#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace hpk {
namespace {

// lay_key, lay_off, TrFrag, lay_issue, lay_take and lds_addr — the image
// and its transposed reads — are in include/gemm_layout_device.h, shared
// with gemm_layout_splitk.hip.

// 8 waves as 2(M) x 4(N), 64x32 per wave. A_T: A is stored [K,M];
// B_N: B is stored [K,N]. LDS: 2 buffers x (A|B) tile = 64 KiB.
template <bool A_T, bool B_N>
__global__ __launch_bounds__(512) void k_gemm_bf16_lay(
    float* __restrict__ C, const __hip_bfloat16* __restrict__ A,
    const __hip_bfloat16* __restrict__ B, int M, int N, int K, int tiles_n,
    int nwg, int xcd_swizzle, int group) {
  using In = __hip_bfloat16;
  constexpr int WAVES_N = 4, THREADS = 512;
  constexpr int MREP = 4, NREP = 2;
  constexpr int WTM = 64, WTN = 32;
  __shared__ __attribute__((aligned(16))) In lds[2 * 2 * TILE_HALF];

  const int wg = hpk_tile_id(tiles_n, nwg, xcd_swizzle, group);
  const long brow = (long)(wg / tiles_n) * BM;
  const long bcol = (long)(wg % tiles_n) * BN;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid / WAVES_N;
  const int wc = wid % WAVES_N;

  constexpr long elems_per_issue = (long)THREADS * 8;
  constexpr int ISSUES = TILE_HALF / (THREADS * 8);
  f32x4 acc[MREP][NREP] = {};

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
      const In* ga = A_T ? A + (k0 + krow) * (long)M + brow + x
                         : A + (brow + row) * (long)K + k0 + kk;
      const In* gb = B_N ? B + (k0 + krow) * (long)N + bcol + x
                         : B + (bcol + row) * (long)K + k0 + kk;
      glds16(ga, dst + o_base);
      glds16(gb, dst + TILE_HALF + o_base);
    }
  };

  stage(0, 0);
  const int trips = K / BK;
  for (int t = 0; t < trips; ++t) {
    const int cur = t & 1;
    const bool more = t + 1 < trips;
    if (more) stage(cur ^ 1, (long)(t + 1) * BK);
    // retire exactly the CURRENT tile's DMAs (2*ISSUES per thread, issued
    // first; FIFO), leaving the prefetch in flight across the barrier
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
    // for the rest
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
      if (ks == 0)
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"i"(TR_STEP) : "memory");
      else
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
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
    // prefetch overwrites it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  // C/D mapping row = 4*(lane>>4)+r, col = lane&15
  for (int m = 0; m < MREP; ++m)
    for (int n = 0; n < NREP; ++n) {
      long row0 = brow + wr * WTM + m * 16 + 4 * (lane >> 4);
      long col = bcol + wc * WTN + n * 16 + (lane & 15);
      for (int r = 0; r < 4; ++r)
        C[(row0 + r) * (long)N + col] = acc[m][n][r];
    }
}

template <bool A_T, bool B_N>
void launch_lay(const char* label, float* C, const void* A, const void* B,
                long M, long N, long K, hipStream_t stream, int xcd_swizzle) {
  // tile order: row-major unless HPK_GEMM_GROUP asks for bands
  const char* genv = std::getenv("HPK_GEMM_GROUP");
  const int group = genv ? std::atoi(genv) : 1;
  const int tiles_n = (int)(N / BN);
  const int nwg = (int)(M / BM) * tiles_n;
  hipLaunchKernelGGL((k_gemm_bf16_lay<A_T, B_N>), dim3(nwg), dim3(512), 0,
                     stream, C, (const __hip_bfloat16*)A,
                     (const __hip_bfloat16*)B, (int)M, (int)N, (int)K, tiles_n,
                     nwg, xcd_swizzle, group);
  check_hip(hipGetLastError(), label);
}

} // namespace

void launch_gemm_bf16_layout(float* C, const void* A, const void* B, long M,
                             long N, long K, const char* layout,
                             hipStream_t stream, int xcd_swizzle) {
  const std::string lay = layout ? layout : "";
  if (lay == "nt")
    throw std::invalid_argument("gemm_bf16_layout: layout 'nt' belongs to "
                                "launch_gemm_bf16_nt");
  if (lay != "nn" && lay != "tn" && lay != "tt")
    throw std::invalid_argument("gemm_bf16_layout: unknown layout '" + lay +
                                "' (nn|tn|tt)");
  if (M <= 0 || N <= 0 || K <= 0 || M % BM != 0 || N % BN != 0 ||
      K % BK != 0 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX)
    throw std::runtime_error("gemm_bf16_layout requires M,N % 128 == 0 and "
                             "K % 64 == 0");
  if (C == nullptr || A == nullptr || B == nullptr)
    throw std::runtime_error("gemm_bf16_layout: null operand");
  if ((uintptr_t)A % 16 != 0 || (uintptr_t)B % 16 != 0)
    throw std::runtime_error("gemm_bf16_layout requires A and B on 16-byte "
                             "boundaries");
  if (lay == "nn")
    return launch_lay<false, true>("launch_gemm_bf16_layout(nn)", C, A, B, M,
                                   N, K, stream, xcd_swizzle);
  if (lay == "tn")
    return launch_lay<true, true>("launch_gemm_bf16_layout(tn)", C, A, B, M, N,
                                  K, stream, xcd_swizzle);
  return launch_lay<true, false>("launch_gemm_bf16_layout(tt)", C, A, B, M, N,
                                 K, stream, xcd_swizzle);
}

} // namespace hpk
