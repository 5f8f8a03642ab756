// gemm_layout_splitk.hip — K7 operand layouts, split-K: the nn/tn/tt bf16
// 128^2-tile GEMM (gemm_layout.hip) with its K loop cut into S parts that
// run as separate workgroups (gemm_splitk.hip). The shape it is for is the
// dW product of a linear layer, dW[N,K] = dy[M,N]^T @ x[M,K]: layout tn on
// the tensors as stored, a weight-sized output and a sum over the tokens —
// a 256x256 weight with 65536 tokens is 4 workgroups without the split.
//
// The kernel is the body of k_gemm_bf16_lay with the changes of
// k_gemm_splitk_nt: grid (tiles, S), blockIdx.y = s walks only the K-tiles
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
// k_gemm_bf16_lay: folding GEMM bodies changes the register allocation of
// the kernels that exist (docs/findings.md #28).
//
// ds_read_b64_tr_b16 needs EXEC all ones: no divergent branch, no early
// return, an exact grid, and trips >= 1 for every split because the
// launcher keeps S <= K / 64.

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
  const long kbeg = range.first * BK; // this split's first k
  const int trips = (int)range.count; // >= 1: the launcher keeps S <= K / 64
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid / WAVES_N;
  const int wc = wid % WAVES_N;

  constexpr long elems_per_issue = (long)THREADS * 8;
  constexpr int ISSUES = TILE_HALF / (THREADS * 8);
  f32x4 acc[MREP][NREP] = {};

  // lane-linear LDS write; the image is in the global chunk each lane
  // takes. k0 is absolute: a [K, X] operand starts at ROW k0 with the full
  // row stride, a K-contiguous one at column k0
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

  stage(0, kbeg);
  for (int t = 0; t < trips; ++t) {
    const int cur = t & 1;
    const bool more = t + 1 < trips;
    if (more) stage(cur ^ 1, kbeg + (long)(t + 1) * BK);
    // retire exactly the CURRENT tile's DMAs (2*ISSUES per thread, issued
    // first; FIFO), leaving the prefetch in flight across the barrier. A
    // single-trip split takes the vmcnt(0) arm at once.
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

template <bool A_T, bool B_N>
void launch_lay_splitk(const char* label, float* C, const void* A,
                       const void* B, long M, long N, long K, int splits,
                       void* workspace, hipStream_t stream, int xcd_swizzle) {
  // tile order: row-major unless HPK_GEMM_GROUP asks for bands
  const char* genv = std::getenv("HPK_GEMM_GROUP");
  const int group = genv ? std::atoi(genv) : 1;
  const int tiles_n = (int)(N / BN);
  const int nwg = (int)(M / BM) * tiles_n;
  float* out = splits == 1 ? C : (float*)workspace;
  hipLaunchKernelGGL((k_gemm_bf16_lay_splitk<A_T, B_N>), dim3(nwg, splits),
                     dim3(512), 0, stream, out, (const __hip_bfloat16*)A,
                     (const __hip_bfloat16*)B, (int)M, (int)N, (int)K, splits,
                     tiles_n, nwg, xcd_swizzle, group);
  check_hip(hipGetLastError(), label);
  if (splits == 1) return;
  launch_splitk_reduce_f32(C, workspace, M * N / 4, splits, stream);
}

} // namespace

void launch_gemm_bf16_layout_splitk(float* C, const void* A, const void* B,
                                    long M, long N, long K,
                                    const char* layout, int splits,
                                    void* workspace, hipStream_t stream,
                                    int xcd_swizzle) {
  const std::string lay = layout ? layout : "";
  if (lay == "nt")
    throw std::invalid_argument("gemm_bf16_layout_splitk: layout 'nt' "
                                "belongs to launch_gemm_splitk_bf16_nt");
  if (lay != "nn" && lay != "tn" && lay != "tt")
    throw std::invalid_argument("gemm_bf16_layout_splitk: unknown layout '" +
                                lay + "' (nn|tn|tt)");
  if (M <= 0 || N <= 0 || K <= 0 || M % BM != 0 || N % BN != 0 ||
      K % BK != 0 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX)
    throw std::runtime_error("gemm_bf16_layout_splitk requires M,N % 128 == 0 "
                             "and K % 64 == 0");
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
  if (lay == "nn")
    return launch_lay_splitk<false, true>(
        "launch_gemm_bf16_layout_splitk(nn)", C, A, B, M, N, K, splits,
        workspace, stream, xcd_swizzle);
  if (lay == "tn")
    return launch_lay_splitk<true, true>(
        "launch_gemm_bf16_layout_splitk(tn)", C, A, B, M, N, K, splits,
        workspace, stream, xcd_swizzle);
  return launch_lay_splitk<true, false>(
      "launch_gemm_bf16_layout_splitk(tt)", C, A, B, M, N, K, splits,
      workspace, stream, xcd_swizzle);
}

// The tile kernel alone, for a caller that folds the slices itself
// (gemm_epilogue.hip: fold, bias and bf16 conversion in one pass).
void launch_gemm_bf16_layout_splitk_partials(float* workspace, const void* A,
                                             const void* B, long M, long N,
                                             long K, const char* layout,
                                             int splits, hipStream_t stream,
                                             int xcd_swizzle) {
  const std::string lay = layout ? layout : "";
  if (lay != "nn" && lay != "tn" && lay != "tt")
    throw std::invalid_argument("gemm_bf16_layout_splitk_partials: unknown "
                                "layout '" + lay + "' (nn|tn|tt)");
  if (M <= 0 || N <= 0 || K <= 0 || M % BM != 0 || N % BN != 0 ||
      K % BK != 0 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX)
    throw std::runtime_error("gemm_bf16_layout_splitk_partials requires "
                             "M,N % 128 == 0 and K % 64 == 0");
  if (splits < 2 || splits > K / BK || splits > 65535)
    throw std::runtime_error("gemm_bf16_layout_splitk_partials requires "
                             "2 <= splits <= K / 64");
  if (workspace == nullptr || A == nullptr || B == nullptr)
    throw std::runtime_error("gemm_bf16_layout_splitk_partials: null operand");
  if ((uintptr_t)A % 16 != 0 || (uintptr_t)B % 16 != 0 ||
      (uintptr_t)workspace % 16 != 0)
    throw std::runtime_error("gemm_bf16_layout_splitk_partials requires A, B "
                             "and the workspace on 16-byte boundaries");
  const char* genv = std::getenv("HPK_GEMM_GROUP");
  const int group = genv ? std::atoi(genv) : 1;
  const int tiles_n = (int)(N / BN);
  const int nwg = (int)(M / BM) * tiles_n;
  const dim3 grid(nwg, splits);
  const __hip_bfloat16* a = (const __hip_bfloat16*)A;
  const __hip_bfloat16* b = (const __hip_bfloat16*)B;
  if (lay == "nn")
    hipLaunchKernelGGL((k_gemm_bf16_lay_splitk<false, true>), grid, dim3(512),
                       0, stream, workspace, a, b, (int)M, (int)N, (int)K,
                       splits, tiles_n, nwg, xcd_swizzle, group);
  else if (lay == "tn")
    hipLaunchKernelGGL((k_gemm_bf16_lay_splitk<true, true>), grid, dim3(512),
                       0, stream, workspace, a, b, (int)M, (int)N, (int)K,
                       splits, tiles_n, nwg, xcd_swizzle, group);
  else
    hipLaunchKernelGGL((k_gemm_bf16_lay_splitk<true, false>), grid, dim3(512),
                       0, stream, workspace, a, b, (int)M, (int)N, (int)K,
                       splits, tiles_n, nwg, xcd_swizzle, group);
  check_hip(hipGetLastError(), "launch_gemm_bf16_layout_splitk_partials");
}

} // namespace hpk
