// gemm_splitk.hip — K7 split-K: the 128^2-tile GEMM for small M, N and a
// long K (gradient-of-weights products, Gram matrices, tall-skinny A^T A).
//
// Every kernel in gemm.hip launches one workgroup per output tile, so
// A[256, 65536] x B[256, 65536]^T keeps 4 of 256 CUs busy. Here the grid is
// (tiles, S): blockIdx.y = s walks only the K-tiles gemm_splitk_ktiles()
// gives split s and writes its 128x128 partial to slice s of a workspace
// [S][M][N]; k_splitk_reduce, launched behind it on the same stream, folds
// the slices in ascending s. No atomics and no "last block reduces" ticket:
// the per-XCD L2s are not coherent with each other, the kernel boundary is,
// and a fixed summation order keeps the family's bitwise tests meaningful
// (the result is the same bits on every run). S == 1 writes C directly.
//
// The tile kernel is ONE body over an operand trait (bf16, fp8 e4m3, int8)
// in the double-buffered 8-wave structure of k_gemm_bf16_nt_db<2,4>: tile
// t+1's 16-byte global_load_lds DMAs are issued before tile t is waited
// for, a counted vmcnt retires exactly tile t, and the barriers are raw, so
// nothing drains the queue inside the loop. A split often has only a few
// K-tiles, and there the plain kernel's two vmcnt(0) barriers per K-step
// are the larger share of its time. Staging, LDS skews and the lane-linear
// LDS image are the family's (include/gemm_device.h); the operand row
// stride stays the full K while the loop runs from the split's first
// K-tile for the split's trip count.

#include "include/hpk.h"
#include "include/gemm_device.h"

#include <hip/hip_bf16.h>

#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace hpk {
namespace {

// Operand traits. CHUNK = elements in one 16-byte glds chunk, KSTEP = K of
// one MFMA; lane L's fragment is KSTEP/4 contiguous elements at
// k = (KSTEP/4) * (L>>4), row/col L&15 (the mappings of gemm.hip).
struct SkBf16 {
  using In = __hip_bfloat16;
  using Out = float;
  using Acc = f32x4;
  using Frag = bf16x8;
  static constexpr int CHUNK = 8, KSTEP = 32;
  static __device__ __forceinline__ long skew(long e) { return lds_skew(e); }
  static __device__ __forceinline__ long unskew(long y) {
    return lds_unskew(y);
  }
  static __device__ __forceinline__ Frag load(const In* p) {
    return *(const Frag*)p;
  }
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
struct SkFp8 {
  using In = unsigned char;
  using Out = float;
  using Acc = f32x4;
  using Frag = long; // 8 packed e4m3
  static constexpr int CHUNK = 16, KSTEP = 32;
  static __device__ __forceinline__ long skew(long e) { return lds_skew8(e); }
  static __device__ __forceinline__ long unskew(long y) {
    return lds_unskew8(y);
  }
  static __device__ __forceinline__ Frag load(const In* p) {
    return *(const Frag*)__builtin_assume_aligned(p, 8);
  }
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0);
  }
};
struct SkI8 {
  using In = signed char;
  using Out = int;
  using Acc = i32x4;
  using Frag = i32x4; // 16 packed int8
  static constexpr int CHUNK = 16, KSTEP = 64;
  static __device__ __forceinline__ long skew(long e) { return i8_skew(e); }
  static __device__ __forceinline__ long unskew(long y) {
    return i8_unskew(y);
  }
  static __device__ __forceinline__ Frag load(const In* p) {
    return *(const Frag*)__builtin_assume_aligned(p, 16);
  }
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
  }
};

// 8 waves as 2(M) x 4(N), 64x32 per wave. P is C when S == 1, else the
// workspace; this workgroup writes slice blockIdx.y of it. LDS: 2 buffers
// x (A|B) tile = 64 KiB for bf16, 32 KiB for the one-byte types.
template <class Tr>
__global__ __launch_bounds__(512) void k_gemm_splitk_nt(
    typename Tr::Out* __restrict__ P, const typename Tr::In* __restrict__ A,
    const typename Tr::In* __restrict__ B, int M, int N, int K, int S,
    int tiles_n, int nwg, int xcd_swizzle, int group) {
  using In = typename Tr::In;
  constexpr int WAVES_N = 4, THREADS = 512;
  constexpr int MREP = 4, NREP = 2;
  constexpr int WTM = 64, WTN = 32;
  __shared__ In lds[2 * 2 * TILE_HALF]; // 2 buffers x (A|B)

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

  constexpr long elems_per_issue = (long)THREADS * Tr::CHUNK;
  constexpr int ISSUES = TILE_HALF / (THREADS * Tr::CHUNK);
  static_assert(ISSUES >= 1, "tile too small for the staging plan");
  typename Tr::Acc acc[MREP][NREP] = {};

  // the row stride is the full K; only the start and the trip count are
  // the split's
  auto stage = [&](int buf, long k0) {
    In* dst = lds + (long)buf * 2 * TILE_HALF;
    for (int issue = 0; issue < ISSUES; ++issue) {
      long o_base =
          (long)issue * elems_per_issue + (long)wid * (64 * Tr::CHUNK);
      long o = Tr::unskew(o_base + (long)lane * Tr::CHUNK);
      int row = (int)(o / BK);
      int kk = (int)(o % BK);
      const In* ga = A + (brow + row) * (long)K + k0 + kk;
      const In* gb = B + (bcol + row) * (long)K + k0 + kk;
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
    for (int kk = 0; kk < BK; kk += Tr::KSTEP) {
      const int kfrag = kk + (Tr::KSTEP / 4) * (lane >> 4);
      typename Tr::Frag afrag[MREP], bfrag[NREP];
      for (int m = 0; m < MREP; ++m) {
        int row = wr * WTM + m * 16 + (lane & 15);
        afrag[m] = Tr::load(la + Tr::skew(row * BK + kfrag));
      }
      for (int n = 0; n < NREP; ++n) {
        int col = wc * WTN + n * 16 + (lane & 15);
        bfrag[n] = Tr::load(lb + Tr::skew(col * BK + kfrag));
      }
      for (int m = 0; m < MREP; ++m)
        for (int n = 0; n < NREP; ++n)
          acc[m][n] = Tr::mfma(afrag[m], bfrag[n], acc[m][n]);
    }
    // every wave done READING buf[cur] before the next iteration's
    // prefetch overwrites it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  // C/D mapping row = 4*(lane>>4)+r, col = lane&15, into slice s
  typename Tr::Out* out = P + (long)s * M * N;
  for (int m = 0; m < MREP; ++m)
    for (int n = 0; n < NREP; ++n) {
      long row0 = brow + wr * WTM + m * 16 + 4 * (lane >> 4);
      long col = bcol + wc * WTN + n * 16 + (lane & 15);
      for (int r = 0; r < 4; ++r)
        out[(row0 + r) * (long)N + col] = acc[m][n][r];
    }
}

// C[i] = ((P0[i] + P1[i]) + P2[i]) + ..., s ascending, on 16-byte vectors
// (V = f32x4 or i32x4); nvec = M * N / 4 per slice, a multiple of 4096, so
// there is no tail. Plain loads and stores: the tile kernel's stores are
// visible here because a kernel boundary lies between them, and plain
// loads are what that guarantee covers (nontemporal loads once summed a
// stale view of fresh data, docs/findings.md).
template <class V>
__global__ __launch_bounds__(256) void k_splitk_reduce(
    V* __restrict__ C, const V* __restrict__ P, long nvec, int S) {
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
    V v = P[i];
    int s = 1;
    // 8 slices' loads in flight, then their adds in order: a small M x N
    // gives this kernel few threads, so each has to overlap its own loads
    for (; s + 8 <= S; s += 8) {
      V p[8];
      for (int j = 0; j < 8; ++j) p[j] = P[(long)(s + j) * nvec + i];
      for (int j = 0; j < 8; ++j) v = v + p[j];
    }
    for (; s < S; ++s) v = v + P[(long)s * nvec + i];
    C[i] = v;
  }
}

// the fold's one launch site: nvec / 256 workgroups, grid-stride above
// kSplitKReduceMaxGrid
template <class V>
void launch_reduce(const char* label, void* C, const void* workspace,
                   long nvec, int S, hipStream_t stream) {
  long grid = nvec / 256;
  if (grid > kSplitKReduceMaxGrid) grid = kSplitKReduceMaxGrid;
  hipLaunchKernelGGL(k_splitk_reduce<V>, dim3((unsigned)grid), dim3(256), 0,
                     stream, (V*)C, (const V*)workspace, nvec, S);
  check_hip(hipGetLastError(), label);
}

template <class Tr, class V>
void launch_splitk(const char* kind, typename Tr::Out* C, const void* A,
                   const void* B, long M, long N, long K, int splits,
                   void* workspace, hipStream_t stream, int xcd_swizzle) {
  const std::string what = std::string("gemm_splitk_") + kind + "_nt";
  if (M <= 0 || N <= 0 || K <= 0 || M % BM != 0 || N % BN != 0 ||
      K % BK != 0)
    throw std::runtime_error(what +
                             " requires M,N % 128 == 0 and K % 64 == 0");
  if (splits < 1 || splits > K / BK || splits > 65535)
    throw std::runtime_error(what + " requires 1 <= splits <= K / 64 (" +
                             std::to_string(splits) + " splits, K = " +
                             std::to_string(K) + ")");
  if (splits > 1 && workspace == nullptr)
    throw std::runtime_error(what + " requires a workspace when splits > 1");
  if (splits > 1 && ((uintptr_t)workspace % 16 != 0 || (uintptr_t)C % 16 != 0))
    throw std::runtime_error(what + " requires C and the workspace on "
                                    "16-byte boundaries when splits > 1");
  // tile order: row-major unless HPK_GEMM_GROUP asks for bands (the grids
  // that split are smaller than the machine, so there is no band to gain)
  const char* genv = std::getenv("HPK_GEMM_GROUP");
  const int group = genv ? std::atoi(genv) : 1;
  const int tiles_n = (int)(N / BN);
  const int nwg = (int)(M / BM) * tiles_n;
  typename Tr::Out* out = splits == 1 ? C : (typename Tr::Out*)workspace;
  hipLaunchKernelGGL(k_gemm_splitk_nt<Tr>, dim3(nwg, splits), dim3(512), 0,
                     stream, out, (const typename Tr::In*)A,
                     (const typename Tr::In*)B, (int)M, (int)N, (int)K, splits,
                     tiles_n, nwg, xcd_swizzle, group);
  check_hip(hipGetLastError(), ("launch_" + what).c_str());
  if (splits == 1) return;
  const long nvec = M * N / 4;
  if constexpr (std::is_same<V, f32x4>::value)
    launch_splitk_reduce_f32(C, workspace, nvec, splits, stream);
  else
    launch_reduce<V>(("launch_" + what + "(reduce)").c_str(), C, workspace,
                     nvec, splits, stream);
}

// The tile kernel alone, for a caller that folds the slices itself
// (gemm_epilogue.hip: fold, bias and bf16 conversion in one pass). A
// template like launch_splitk, so that the kernels keep their order in the
// code object.
template <class Tr>
void launch_partials(const char* what, typename Tr::Out* workspace,
                     const void* A, const void* B, long M, long N, long K,
                     int splits, hipStream_t stream, int xcd_swizzle) {
  const std::string w = what;
  if (M <= 0 || N <= 0 || K <= 0 || M % BM != 0 || N % BN != 0 ||
      K % BK != 0)
    throw std::runtime_error(w + " requires M,N % 128 == 0 and K % 64 == 0");
  if (splits < 2 || splits > K / BK || splits > 65535)
    throw std::runtime_error(w + " requires 2 <= splits <= K / 64");
  if (workspace == nullptr || (uintptr_t)workspace % 16 != 0)
    throw std::runtime_error(w + " requires a workspace on a 16-byte "
                                 "boundary");
  const char* genv = std::getenv("HPK_GEMM_GROUP");
  const int group = genv ? std::atoi(genv) : 1;
  const int tiles_n = (int)(N / BN);
  const int nwg = (int)(M / BM) * tiles_n;
  hipLaunchKernelGGL(k_gemm_splitk_nt<Tr>, dim3(nwg, splits), dim3(512), 0,
                     stream, workspace, (const typename Tr::In*)A,
                     (const typename Tr::In*)B, (int)M, (int)N, (int)K, splits,
                     tiles_n, nwg, xcd_swizzle, group);
  check_hip(hipGetLastError(), ("launch_" + w).c_str());
}

} // namespace

int gemm_splitk_plan(long M, long N, long K, int n_cu) {
  if (M <= 0 || N <= 0 || K <= 0) return 1;
  const long tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  const long T = (K + BK - 1) / BK;
  if (tiles >= n_cu) return 1;
  long hi = T / kSplitKMinTiles;
  if (hi > kSplitKMaxSplits) hi = kSplitKMaxSplits;
  long want = n_cu / tiles;
  if (want > hi) want = hi;
  return want < 1 ? 1 : (int)want;
}

void launch_gemm_splitk_bf16_nt(float* C, const void* A, const void* B,
                                long M, long N, long K, int splits,
                                void* workspace, hipStream_t stream,
                                int xcd_swizzle) {
  launch_splitk<SkBf16, f32x4>("bf16", C, A, B, M, N, K, splits, workspace,
                               stream, xcd_swizzle);
}

// Stands here, behind the first use of the bf16 tile kernel, so that the
// kernels keep the order in the code object they had before the fold
// became a function of its own.
void launch_splitk_reduce_f32(float* C, const void* workspace, long nvec,
                              int S, hipStream_t stream) {
  if (C == nullptr || workspace == nullptr || nvec < 256 || nvec % 256 != 0 ||
      S < 2)
    throw std::runtime_error("splitk_reduce_f32 requires C, a workspace, "
                             "nvec % 256 == 0 and S >= 2");
  if ((uintptr_t)C % 16 != 0 || (uintptr_t)workspace % 16 != 0)
    throw std::runtime_error("splitk_reduce_f32 requires C and the workspace "
                             "on 16-byte boundaries");
  launch_reduce<f32x4>("launch_splitk_reduce_f32", C, workspace, nvec, S,
                       stream);
}

void launch_gemm_splitk_fp8_nt(float* C, const void* A, const void* B,
                               long M, long N, long K, int splits,
                               void* workspace, hipStream_t stream,
                               int xcd_swizzle) {
  launch_splitk<SkFp8, f32x4>("fp8", C, A, B, M, N, K, splits, workspace,
                              stream, xcd_swizzle);
}

void launch_gemm_splitk_i8_nt(int* C, const void* A, const void* B, long M,
                              long N, long K, int splits, void* workspace,
                              hipStream_t stream, int xcd_swizzle) {
  launch_splitk<SkI8, i32x4>("i8", C, A, B, M, N, K, splits, workspace,
                             stream, xcd_swizzle);
}

void launch_gemm_splitk_bf16_nt_partials(float* workspace, const void* A,
                                         const void* B, long M, long N, long K,
                                         int splits, hipStream_t stream,
                                         int xcd_swizzle) {
  launch_partials<SkBf16>("gemm_splitk_bf16_nt_partials", workspace, A, B, M,
                          N, K, splits, stream, xcd_swizzle);
}

} // namespace hpk
