// gemm_batched.hip — K7 batched and strided: the bf16 128^2-tile GEMM of all
// four operand layouts over a batch, every operand with a leading dimension
// and a batch stride of its own,
//
//   C_b[M,N] = alpha * op(A_b) @ op(B_b),   b = 0 .. batch-1,
//
//   layout  A_b as stored  B_b as stored  template <A_T, B_N>
//   nt      [M,K]          [N,K]          <false, false>
//   nn      [M,K]          [K,N]          <false, true>
//   tn      [K,M]          [K,N]          <true,  true>
//   tt      [K,M]          [N,K]          <true,  false>
//
// so that one head of a [tokens, heads*dim] activation — row stride
// heads*dim, batch stride dim — is read where it lies: the attention
// products S_h = Q_h K_h^T and O_h = P_h V_h and their backward products
// need neither a loop over heads nor a contiguous() copy of each head.
//
// k_gemm_bf16_batched<A_T, B_N, Out> runs the K loop of k_gemm_bf16_lay
// (gemm_layout.hip), include/gemm_bf16_lay_loop.inc, with lda and ldb for
// its row strides: the 2x4 waves of 64x32, the prefetch of tile t+1, the
// counted vmcnt / lgkmcnt, the raw barriers, 64 KiB LDS, the lay_off image
// with ds_read_b64_tr_b16 reads. <false, false> is that loop with both
// operands K-contiguous, which is k_gemm_bf16_nt_db<2,4>'s operand order
// (gemm.hip). The MFMAs see the same operands in the same order, so with
// alpha == 1 the accumulators, and the fp32 C, are those kernels' bit for
// bit. These are kernels of their own, not a stride switch inside the
// parents: that changes the register allocation of the kernels that exist
// (docs/findings.md #28).
//
// What differs is where a tile comes from and goes to. The grid is
// (nwg, batch): blockIdx.x goes through hpk_tile_id per batch, blockIdx.y
// is the batch, whose offsets b * bs are added to the three base pointers
// once (scalar). A K-contiguous operand is read at
//   P + b*bs + (row0 + row)*ld + k0 + kk,
// an operand stored [K, X] at
//   P + b*bs + (k0 + krow)*ld + x0 + x,
// all in 64-bit arithmetic. ld % 8 == 0, bs % 8 == 0 and a base on a
// 16-byte boundary keep every 16-byte chunk of every batch aligned; bs == 0
// broadcasts one operand to every batch.
//
// Epilogue: one fp32 multiply by alpha on every accumulator, always
// executed (x 1.0f is exact and keeps -0.0 and NaN, so there is no branch
// on it). fp32 C: the parents' dword stores, at ldc. bf16 C: one
// v_cvt_pk_bf16_f32 rounding after the multiply and the staged store of
// gemm_epilogue.hip (gemm_out_lds_offset / gemm_out_read in the LDS the K
// loop has finished with, one barrier, whole 256-byte rows) at ldc.
//
// ds_read_b64_tr_b16 needs EXEC all ones: no divergent branch and no early
// return anywhere; the grid is exact and the launcher refuses every shape
// that is not a whole number of tiles. Contract: docs/gemm.md, "Batched and
// strided operands".

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

// fp32 C: the C/D mapping row = 4*(lane>>4)+r, col = lane&15, dword stores
__device__ __forceinline__ void store_tile(float* __restrict__ C,
                                           const f32x4 (&acc)[4][2],
                                           __hip_bfloat16*, long brow,
                                           long bcol, long ldc, int, int lane,
                                           int wr, int wc) {
  constexpr int MREP = 4, NREP = 2, WTM = 64, WTN = 32;
  for (int m = 0; m < MREP; ++m)
    for (int n = 0; n < NREP; ++n) {
      long row0 = brow + wr * WTM + m * 16 + 4 * (lane >> 4);
      long col = bcol + wc * WTN + n * 16 + (lane & 15);
      for (int r = 0; r < 4; ++r) C[(row0 + r) * ldc + col] = acc[m][n][r];
    }
}

// bf16 C: store_tile_bf16 of gemm_epilogue.hip without a bias and with a
// row stride. Every wave must be done with `lds` (the K loop's last
// barrier).
__device__ __forceinline__ void store_tile(__hip_bfloat16* __restrict__ C,
                                           const f32x4 (&acc)[4][2],
                                           __hip_bfloat16* lds, long brow,
                                           long bcol, long ldc, int tid,
                                           int lane, int wr, int wc) {
  constexpr int MREP = 4, NREP = 2, WTM = 64, WTN = 32;
  char* img = (char*)lds;
  for (int m = 0; m < MREP; ++m)
    for (int n = 0; n < NREP; ++n) {
      const int row = wr * WTM + m * 16 + 4 * (lane >> 4);
      const int col = wc * WTN + n * 16 + (lane & 15);
      for (int r = 0; r < 4; r += 2)
        *(lds_u32*)(img + gemm_out_lds_offset(row + r, col)) =
            pack_bf16(acc[m][n][r], acc[m][n][r + 1]);
    }
  __syncthreads();
  flush_tile(C, img, brow, bcol, ldc, tid);
}

// 8 waves as 2(M) x 4(N), 64x32 per wave. A_T: A_b is stored [K,M];
// B_N: B_b is stored [K,N]. LDS: 2 buffers x (A|B) tile = 64 KiB.
template <bool A_T, bool B_N, typename Out>
__global__ __launch_bounds__(512) void k_gemm_bf16_batched(
    Out* __restrict__ C, const __hip_bfloat16* __restrict__ A,
    const __hip_bfloat16* __restrict__ B, int K, long lda, long bsA, long ldb,
    long bsB, long ldc, long bsC, float alpha, int tiles_n, int nwg,
    int xcd_swizzle, int group) {
  using In = __hip_bfloat16;
  constexpr int WAVES_N = 4, THREADS = 512;
  constexpr int MREP = 4, NREP = 2;
  constexpr int WTM = 64, WTN = 32;
  __shared__ __attribute__((aligned(16))) In lds[2 * 2 * TILE_HALF];

  const int wg = hpk_tile_id(tiles_n, nwg, xcd_swizzle, group);
  const long brow = (long)(wg / tiles_n) * BM;
  const long bcol = (long)(wg % tiles_n) * BN;
  const long batch = (long)blockIdx.y;
  A += batch * bsA;
  B += batch * bsB;
  C += batch * bsC;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid / WAVES_N;
  const int wc = wid % WAVES_N;

  constexpr long elems_per_issue = (long)THREADS * 8;
  constexpr int ISSUES = TILE_HALF / (THREADS * 8);
  f32x4 acc[MREP][NREP] = {};

#define GEMM_LAY_LDA_KM lda
#define GEMM_LAY_LDA_MK lda
#define GEMM_LAY_LDB_KN ldb
#define GEMM_LAY_LDB_NK ldb
#define GEMM_LAY_K_FIRST 0
#define GEMM_LAY_K_NEXT (long)(t + 1) * BK
#define GEMM_LAY_TRIPS K / BK
#include "include/gemm_bf16_lay_loop.inc"

  for (int m = 0; m < MREP; ++m)
    for (int n = 0; n < NREP; ++n) acc[m][n] = acc[m][n] * alpha;
  store_tile(C, acc, lds, brow, bcol, ldc, tid, lane, wr, wc);
}

struct BatchedArgs {
  void* C;
  const void *A, *B;
  long M, N, K, batch, lda, bsA, ldb, bsB, ldc, bsC;
  float alpha;
  hipStream_t stream;
  int xcd_swizzle;
};

template <bool A_T, bool B_N, typename Out>
void launch_one(const char* label, const BatchedArgs& g) {
  const int tiles_n = (int)(g.N / BN);
  const int nwg = (int)(g.M / BM) * tiles_n;
  hipLaunchKernelGGL((k_gemm_bf16_batched<A_T, B_N, Out>),
                     dim3(nwg, (unsigned)g.batch), dim3(512), 0, g.stream,
                     (Out*)g.C, (const __hip_bfloat16*)g.A,
                     (const __hip_bfloat16*)g.B, (int)g.K, g.lda, g.bsA, g.ldb,
                     g.bsB, g.ldc, g.bsC, g.alpha, tiles_n, nwg, g.xcd_swizzle,
                     gemm_tile_group());
  check_hip(hipGetLastError(), label);
}

template <bool A_T, bool B_N>
void launch_out(const char* label, bool c_is_bf16, const BatchedArgs& g) {
  if (c_is_bf16) return launch_one<A_T, B_N, __hip_bfloat16>(label, g);
  launch_one<A_T, B_N, float>(label, g);
}

} // namespace

void launch_gemm_bf16_batched(void* C, int c_is_bf16, const void* A,
                              const void* B, long M, long N, long K,
                              long batch, long lda, long bsA, long ldb,
                              long bsB, long ldc, long bsC, const char* layout,
                              float alpha, hipStream_t stream,
                              int xcd_swizzle) {
  const GemmLayout lay = gemm_parse_layout("gemm_bf16_batched", layout, true);
  gemm_require_tile_shape("gemm_bf16_batched", M, N, K);
  if (batch < 1 || batch > kGemmBatchedMaxBatch)
    throw std::runtime_error("gemm_bf16_batched requires 1 <= batch <= 65535 "
                             "(got " + std::to_string(batch) + ")");
  if (C == nullptr || A == nullptr || B == nullptr)
    throw std::runtime_error("gemm_bf16_batched: null operand");
  if ((uintptr_t)A % 16 != 0 || (uintptr_t)B % 16 != 0)
    throw std::runtime_error("gemm_bf16_batched requires A and B on 16-byte "
                             "boundaries");
  if (batch == 1) bsA = bsB = bsC = 0; // one image: the stride names nothing
  if (lda % 8 != 0 || ldb % 8 != 0 || bsA % 8 != 0 || bsB % 8 != 0)
    throw std::runtime_error("gemm_bf16_batched requires lda, ldb and the "
                             "batch strides of A and B to be multiples of 8 "
                             "elements");
  if (lda < (lay.a_t ? M : K) || ldb < (lay.b_n ? N : K) || bsA < 0 ||
      bsB < 0)
    throw std::runtime_error("gemm_bf16_batched requires lda and ldb of at "
                             "least the stored row length and batch strides "
                             ">= 0");
  if (!gemm_batched_c_disjoint(batch, M, N, ldc, bsC))
    throw std::runtime_error(
        "gemm_bf16_batched requires ldc >= N and pairwise disjoint C images: "
        "bsC >= (M-1)*ldc + N, or bsC >= N and ldc >= (batch-1)*bsC + N");
  if ((uintptr_t)C % (c_is_bf16 ? 16 : 4) != 0)
    throw std::runtime_error(c_is_bf16
                                 ? "gemm_bf16_batched requires a bf16 C on a "
                                   "16-byte boundary"
                                 : "gemm_bf16_batched requires an fp32 C on "
                                   "a 4-byte boundary");
  if (c_is_bf16 && (ldc % 8 != 0 || bsC % 8 != 0))
    throw std::runtime_error("gemm_bf16_batched requires ldc and bsC to be "
                             "multiples of 8 elements for a bf16 C (its rows "
                             "are written as 16-byte stores)");

  const BatchedArgs g{C, A, B, M, N, K, batch, lda, bsA, ldb, bsB, ldc, bsC,
                      alpha, stream, xcd_swizzle};
  if (!lay.a_t && !lay.b_n)
    return launch_out<false, false>("launch_gemm_bf16_batched(nt)", c_is_bf16,
                                    g);
  if (!lay.a_t)
    return launch_out<false, true>("launch_gemm_bf16_batched(nn)", c_is_bf16,
                                   g);
  if (lay.b_n)
    return launch_out<true, true>("launch_gemm_bf16_batched(tn)", c_is_bf16,
                                  g);
  return launch_out<true, false>("launch_gemm_bf16_batched(tt)", c_is_bf16, g);
}

} // namespace hpk
