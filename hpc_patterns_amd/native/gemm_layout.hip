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
// tile t, raw barriers, 64 KiB LDS, the same C/D epilogue. The K loop is
// include/gemm_bf16_lay_loop.inc, which the split-K, bf16-output,
// activation and batched kernels of these layouts include as well.
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
#include "include/gemm_host.h"
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

#define GEMM_LAY_LDA_KM (long)M
#define GEMM_LAY_LDA_MK (long)K
#define GEMM_LAY_LDB_KN (long)N
#define GEMM_LAY_LDB_NK (long)K
#define GEMM_LAY_K_FIRST 0
#define GEMM_LAY_K_NEXT (long)(t + 1) * BK
#define GEMM_LAY_TRIPS K / BK
#include "include/gemm_bf16_lay_loop.inc"

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
  const int tiles_n = (int)(N / BN);
  const int nwg = (int)(M / BM) * tiles_n;
  hipLaunchKernelGGL((k_gemm_bf16_lay<A_T, B_N>), dim3(nwg), dim3(512), 0,
                     stream, C, (const __hip_bfloat16*)A,
                     (const __hip_bfloat16*)B, (int)M, (int)N, (int)K, tiles_n,
                     nwg, xcd_swizzle, gemm_tile_group());
  check_hip(hipGetLastError(), label);
}

} // namespace

void launch_gemm_bf16_layout(float* C, const void* A, const void* B, long M,
                             long N, long K, const char* layout,
                             hipStream_t stream, int xcd_swizzle) {
  if (layout != nullptr && std::string(layout) == "nt")
    throw std::invalid_argument("gemm_bf16_layout: layout 'nt' belongs to "
                                "launch_gemm_bf16_nt");
  const GemmLayout lay = gemm_parse_layout("gemm_bf16_layout", layout, false);
  gemm_require_tile_shape("gemm_bf16_layout", M, N, K);
  if (C == nullptr || A == nullptr || B == nullptr)
    throw std::runtime_error("gemm_bf16_layout: null operand");
  if ((uintptr_t)A % 16 != 0 || (uintptr_t)B % 16 != 0)
    throw std::runtime_error("gemm_bf16_layout requires A and B on 16-byte "
                             "boundaries");
  if (!lay.a_t)
    return launch_lay<false, true>("launch_gemm_bf16_layout(nn)", C, A, B, M,
                                   N, K, stream, xcd_swizzle);
  if (lay.b_n)
    return launch_lay<true, true>("launch_gemm_bf16_layout(tn)", C, A, B, M, N,
                                  K, stream, xcd_swizzle);
  return launch_lay<true, false>("launch_gemm_bf16_layout(tt)", C, A, B, M, N,
                                 K, stream, xcd_swizzle);
}

} // namespace hpk
