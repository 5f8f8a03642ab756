// gemm_layout_splitk.hip — K7 operand layouts, split-K: the nn/tn/tt bf16
// 128^2-tile GEMM (gemm_layout.hip) with its K loop cut into S parts that
// run as separate workgroups (gemm_splitk.hip). The shape it is for is the
// dW product of a linear layer, dW[N,K] = dy[M,N]^T @ x[M,K]: layout tn on
// the tensors as stored, a weight-sized output and a sum over the tokens —
// a 256x256 weight with 65536 tokens is 4 workgroups without the split.
//
// The kernel is k_gemm_bf16_lay — the same K loop,
// include/gemm_bf16_lay_loop.inc, given a first k and a trip count — with
// the changes of k_gemm_splitk_nt: grid (tiles, S), blockIdx.y = s walks
// only the K-tiles
// gemm_splitk_ktiles() gives split s and writes its 128x128 partial to
// slice s of a workspace [S][M][N]; launch_splitk_reduce_f32, behind it on
// the same stream, folds the slices in ascending s. S == 1 writes C
// directly. For an operand stored [K, X] the split's first k is a ROW of
// the tensor (the row stride stays the full M or N); for a K-contiguous
// one it is a column, as in the NT split-K kernel. Partition, MFMA order
// inside a split and fold order are those of k_gemm_splitk_nt<SkBf16>, so
// the result is its bits on materialised transposes.
//
// It is a kernel of its own, not an S == 1 / S > 1 switch inside
// k_gemm_bf16_lay: a switch inside a GEMM body changes the register
// allocation of the kernels that exist (docs/findings.md #28).
//
// ds_read_b64_tr_b16 needs EXEC all ones: no divergent branch, no early
// return, an exact grid, and trips >= 1 for every split because the
// launcher keeps S <= K / 64.

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

// 8 waves as 2(M) x 4(N), 64x32 per wave. A_T: A is stored [K,M];
// B_N: B is stored [K,N]. P is C when S == 1, else the workspace; this
// workgroup writes slice blockIdx.y of it. LDS: 2 buffers x (A|B) tile =
// 64 KiB.
template <bool A_T, bool B_N>
__global__ __launch_bounds__(512) void k_gemm_bf16_lay_splitk(
    float* __restrict__ P, const __hip_bfloat16* __restrict__ A,
    const __hip_bfloat16* __restrict__ B, int M, int N, int K, int S,
    int tiles_n, int nwg, int xcd_swizzle, int group) {
  using In = __hip_bfloat16;
  constexpr int WAVES_N = 4, THREADS = 512;
  constexpr int MREP = 4, NREP = 2;
  constexpr int WTM = 64, WTN = 32;
  __shared__ __attribute__((aligned(16))) In lds[2 * 2 * TILE_HALF];

  const int wg = hpk_tile_id(tiles_n, nwg, xcd_swizzle, group);
  const long brow = (long)(wg / tiles_n) * BM;
  const long bcol = (long)(wg % tiles_n) * BN;
  const int s = (int)blockIdx.y;
  const SplitKRange range = gemm_splitk_ktiles(K / BK, S, s);
  // this split's first k; range.count >= 1: the launcher keeps S <= K / 64
  const long kbeg = range.first * BK;
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
#define GEMM_LAY_K_FIRST kbeg
#define GEMM_LAY_K_NEXT kbeg + (long)(t + 1) * BK
#define GEMM_LAY_TRIPS (int)range.count
#include "include/gemm_bf16_lay_loop.inc"

  // C/D mapping row = 4*(lane>>4)+r, col = lane&15, into slice s
  float* out = P + (long)s * M * N;
  for (int m = 0; m < MREP; ++m)
    for (int n = 0; n < NREP; ++n) {
      long row0 = brow + wr * WTM + m * 16 + 4 * (lane >> 4);
      long col = bcol + wc * WTN + n * 16 + (lane & 15);
      for (int r = 0; r < 4; ++r)
        out[(row0 + r) * (long)N + col] = acc[m][n][r];
    }
}

// the tile kernel of layout `lay` on grid (tiles, splits), writing `out`
void launch_tiles(const char* label, GemmLayout lay, float* out, const void* A,
                  const void* B, long M, long N, long K, int splits,
                  hipStream_t stream, int xcd_swizzle) {
  const int tiles_n = (int)(N / BN);
  const int nwg = (int)(M / BM) * tiles_n;
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(nwg, splits), dim3(512), 0, stream, out,
                       (const __hip_bfloat16*)A, (const __hip_bfloat16*)B,
                       (int)M, (int)N, (int)K, splits, tiles_n, nwg,
                       xcd_swizzle, gemm_tile_group());
    check_hip(hipGetLastError(), label);
  };
  if (!lay.a_t) return go(k_gemm_bf16_lay_splitk<false, true>);
  if (lay.b_n) return go(k_gemm_bf16_lay_splitk<true, true>);
  go(k_gemm_bf16_lay_splitk<true, false>);
}

} // namespace

void launch_gemm_bf16_layout_splitk(float* C, const void* A, const void* B,
                                    long M, long N, long K,
                                    const char* layout, int splits,
                                    void* workspace, hipStream_t stream,
                                    int xcd_swizzle) {
  if (layout != nullptr && std::string(layout) == "nt")
    throw std::invalid_argument("gemm_bf16_layout_splitk: layout 'nt' "
                                "belongs to launch_gemm_splitk_bf16_nt");
  const GemmLayout lay =
      gemm_parse_layout("gemm_bf16_layout_splitk", layout, false);
  gemm_require_tile_shape("gemm_bf16_layout_splitk", M, N, K);
  if (splits < 1 || splits > K / BK || splits > 65535)
    throw std::runtime_error(
        "gemm_bf16_layout_splitk requires 1 <= splits <= K / 64 (" +
        std::to_string(splits) + " splits, K = " + std::to_string(K) + ")");
  if (C == nullptr || A == nullptr || B == nullptr)
    throw std::runtime_error("gemm_bf16_layout_splitk: null operand");
  if ((uintptr_t)A % 16 != 0 || (uintptr_t)B % 16 != 0)
    throw std::runtime_error("gemm_bf16_layout_splitk requires A and B on "
                             "16-byte boundaries");
  if (splits > 1 && workspace == nullptr)
    throw std::runtime_error("gemm_bf16_layout_splitk requires a workspace "
                             "when splits > 1");
  if (splits > 1 && ((uintptr_t)workspace % 16 != 0 || (uintptr_t)C % 16 != 0))
    throw std::runtime_error("gemm_bf16_layout_splitk requires C and the "
                             "workspace on 16-byte boundaries when "
                             "splits > 1");
  const std::string label =
      std::string("launch_gemm_bf16_layout_splitk(") + layout + ")";
  launch_tiles(label.c_str(), lay, splits == 1 ? C : (float*)workspace, A, B,
               M, N, K, splits, stream, xcd_swizzle);
  if (splits == 1) return;
  launch_splitk_reduce_f32(C, workspace, M * N / 4, splits, stream);
}

// The tile kernel alone, for a caller that folds the slices itself
// (gemm_epilogue.hip: fold, bias and bf16 conversion in one pass).
void launch_gemm_bf16_layout_splitk_partials(float* workspace, const void* A,
                                             const void* B, long M, long N,
                                             long K, const char* layout,
                                             int splits, hipStream_t stream,
                                             int xcd_swizzle) {
  const GemmLayout lay =
      gemm_parse_layout("gemm_bf16_layout_splitk_partials", layout, false);
  gemm_require_tile_shape("gemm_bf16_layout_splitk_partials", M, N, K);
  if (splits < 2 || splits > K / BK || splits > 65535)
    throw std::runtime_error("gemm_bf16_layout_splitk_partials requires "
                             "2 <= splits <= K / 64");
  if (workspace == nullptr || A == nullptr || B == nullptr)
    throw std::runtime_error("gemm_bf16_layout_splitk_partials: null operand");
  if ((uintptr_t)A % 16 != 0 || (uintptr_t)B % 16 != 0 ||
      (uintptr_t)workspace % 16 != 0)
    throw std::runtime_error("gemm_bf16_layout_splitk_partials requires A, B "
                             "and the workspace on 16-byte boundaries");
  launch_tiles("launch_gemm_bf16_layout_splitk_partials", lay, workspace, A, B,
               M, N, K, splits, stream, xcd_swizzle);
}

} // namespace hpk
