// gemm_epilogue.hip — K7 with a bf16 output and a bias: the bf16 128^2-tile
// GEMM of all four operand layouts writing C[M,N] = bf16(acc + bias[n])
// itself, instead of an fp32 C that an elementwise kernel reads back, and
// the column sum that is the bias gradient.
//
// k_gemm_bf16_nt_out and k_gemm_bf16_lay_out<A_T, B_N> run the K loops of
// k_gemm_bf16_nt_db<2,4> (gemm.hip) and k_gemm_bf16_lay (gemm_layout.hip):
// include/gemm_bf16_nt_loop.inc and include/gemm_bf16_lay_loop.inc hold
// the one copy of each — staging, the counted vmcnt / lgkmcnt, the raw
// barriers, the MFMA operand order — so the accumulators are the parents'
// bit for bit. They are kernels of their own, not an epilogue switch
// inside the parents: that changes the register allocation of the kernels
// that exist (docs/findings.md #28).
//
// The epilogue (store_tile_bf16). In the C/D mapping a lane holds rows
// 4g .. 4g+3 (g = lane>>4) of ONE column, so the naive port has 16 lanes
// writing 2 bytes each: 32-byte row segments. Instead the tile goes through
// the LDS the K loop has finished with (its last barrier has every wave
// done reading): v_cvt_pk_bf16_f32 packs rows r and r+1 of the lane's
// column into one dword, one ds_write_b32 puts it into a [64 row pairs]
// [128 columns] image of dwords (32 KiB of the loop's 64 KiB, no LDS
// added), and after one barrier every thread reads 2 x 16 bytes = 4 columns
// x 2 rows each, separates the two rows with 8 bit operations and stores
// 16 bytes to each: 16 lanes write one whole 256-byte row of C. Per lane
// that is 16 LDS writes, 4 LDS reads and 4 global stores where the fp32
// epilogue has 32 global stores. Image, banks: gemm_out_lds_offset /
// gemm_out_read (include/hpk.h), docs/gemm.md "bf16 output and bias".
//
// ds_read_b64_tr_b16 needs EXEC all ones: no divergent branch and no early
// return anywhere; `bias != nullptr` is a scalar branch behind the K loop.
//
// splits > 1 launches the split-K tile kernels that exist (their partials
// are fp32 either way) and k_splitk_reduce_bf16 folds them in ascending s,
// adds the bias and converts: one pass where fold + add + cast were three.

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

// The epilogue of both GEMM kernels: acc is the 64x32 sub-tile of wave
// (wr, wc) in the C/D mapping row = 4*(lane>>4)+r, col = lane&15. Every
// wave must be done with `lds` (the K loop's last barrier).
__device__ __forceinline__ void store_tile_bf16(
    __hip_bfloat16* __restrict__ C, const float* __restrict__ bias,
    const f32x4 (&acc)[4][2], __hip_bfloat16* lds, long brow, long bcol,
    int N, int tid, int lane, int wr, int wc) {
  constexpr int MREP = 4, NREP = 2, WTM = 64, WTN = 32;
  char* img = (char*)lds;
  float bv[NREP] = {};
  if (bias != nullptr)
    for (int n = 0; n < NREP; ++n)
      bv[n] = bias[bcol + wc * WTN + n * 16 + (lane & 15)];
  for (int m = 0; m < MREP; ++m)
    for (int n = 0; n < NREP; ++n) {
      const int row = wr * WTM + m * 16 + 4 * (lane >> 4);
      const int col = wc * WTN + n * 16 + (lane & 15);
      f32x4 v = acc[m][n];
      if (bias != nullptr) v = v + bv[n]; // nullptr: no add at all
      for (int r = 0; r < 4; r += 2)
        *(lds_u32*)(img + gemm_out_lds_offset(row + r, col)) =
            pack_bf16(v[r], v[r + 1]);
    }
  __syncthreads();
  flush_tile(C, img, brow, bcol, N, tid);
}

// k_gemm_bf16_nt_db<2,4> (gemm.hip) with the bf16 epilogue: 8 waves as
// 2(M) x 4(N), 64x32 per wave, 2 buffers x (A|B) tile = 64 KiB LDS.
__global__ __launch_bounds__(512) void k_gemm_bf16_nt_out(
    __hip_bfloat16* __restrict__ C, const float* __restrict__ bias,
    const __hip_bfloat16* __restrict__ A, const __hip_bfloat16* __restrict__ B,
    int M, int N, int K, int tiles_n, int nwg, int xcd_swizzle, int group) {
  constexpr int WAVES_M = 2, WAVES_N = 4;
  constexpr int THREADS = WAVES_M * WAVES_N * 64;
  constexpr int MREP = BM / (WAVES_M * 16);
  constexpr int NREP = BN / (WAVES_N * 16);
  constexpr int WTM = BM / WAVES_M;
  constexpr int WTN = BN / WAVES_N;
  __shared__ __attribute__((aligned(16)))
  __hip_bfloat16 lds[2 * 2 * TILE_HALF]; // 2 buffers x (A|B)

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

#include "include/gemm_bf16_nt_loop.inc"

  store_tile_bf16(C, bias, acc, lds, brow, bcol, N, tid, lane, wr, wc);
}

// k_gemm_bf16_lay (gemm_layout.hip) with the bf16 epilogue. A_T: A is
// stored [K,M]; B_N: B is stored [K,N].
template <bool A_T, bool B_N>
__global__ __launch_bounds__(512) void k_gemm_bf16_lay_out(
    __hip_bfloat16* __restrict__ C, const float* __restrict__ bias,
    const __hip_bfloat16* __restrict__ A, const __hip_bfloat16* __restrict__ B,
    int M, int N, int K, int tiles_n, int nwg, int xcd_swizzle, int group) {
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

  store_tile_bf16(C, bias, acc, lds, brow, bcol, N, tid, lane, wr, wc);
}

// C[8i .. 8i+7] = bf16((((P0 + P1) + P2) + ...) + bias[n]), s ascending, the
// fold of k_splitk_reduce (gemm_splitk.hip) on two 16-byte vectors per
// lane; nvec8 = M * N / 8 per slice, a multiple of 2048, so there is no
// tail, and N % 8 == 0 keeps a lane's 8 outputs in one row. Plain loads:
// the kernel boundary publishes the partials, and plain loads are what
// that guarantee covers.
__global__ __launch_bounds__(256) void k_splitk_reduce_bf16(
    u32x4* __restrict__ C, const f32x4* __restrict__ P,
    const float* __restrict__ bias, long nvec8, int S, int N) {
  const long stride = (long)gridDim.x * 256;
  const long slice = 2 * nvec8; // 16-byte vectors per slice
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec8; i += stride) {
    f32x4 lo = P[2 * i], hi = P[2 * i + 1];
    int s = 1;
    for (; s + 8 <= S; s += 8) {
      f32x4 pl[8], ph[8];
      for (int j = 0; j < 8; ++j) {
        pl[j] = P[(long)(s + j) * slice + 2 * i];
        ph[j] = P[(long)(s + j) * slice + 2 * i + 1];
      }
      for (int j = 0; j < 8; ++j) {
        lo = lo + pl[j];
        hi = hi + ph[j];
      }
    }
    for (; s < S; ++s) {
      lo = lo + P[(long)s * slice + 2 * i];
      hi = hi + P[(long)s * slice + 2 * i + 1];
    }
    if (bias != nullptr) { // nullptr: no add at all
      const float* b = bias + (8 * i) % N;
      const f32x4 bl = {b[0], b[1], b[2], b[3]};
      const f32x4 bh = {b[4], b[5], b[6], b[7]};
      lo = lo + bl;
      hi = hi + bh;
    }
    const u32x4 out = {pack_bf16(lo[0], lo[1]), pack_bf16(lo[2], lo[3]),
                       pack_bf16(hi[0], hi[1]), pack_bf16(hi[2], hi[3])};
    C[i] = out;
  }
}

// partial[r][8g .. 8g+7] = sum of rows colsum_rows(M, R, r) of column group
// g (8 bf16 = one 16-byte load per row), ascending, in fp32; thread = one
// column group, blockIdx.y = r. 8 rows' loads are in flight before their
// adds, which stay in row order. 64-thread workgroups: a 1024-wide matrix
// has only 128 column groups, and the chunks, not the columns, fill the
// machine. Plain loads: in a backward pass x is what the kernel before
// this one wrote (findings.md on nontemporal loads of fresh data).
__global__ __launch_bounds__(64) void k_colsum_bf16(
    float* __restrict__ out, const u32x4* __restrict__ x, long M, int ngroups,
    long pitch, int R) {
  const int g = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (g >= ngroups) return;
  const int r = (int)blockIdx.y;
  const SplitKRange rows = colsum_rows(M, R, r);
  const u32x4* p = x + rows.first * ngroups + g;
  float acc[8] = {};
  auto add = [&](const u32x4& v) {
    for (int d = 0; d < 4; ++d) {
      acc[2 * d] += __builtin_bit_cast(float, v[d] << 16);
      acc[2 * d + 1] += __builtin_bit_cast(float, v[d] & 0xffff0000u);
    }
  };
  long i = 0;
  for (; i + 8 <= rows.count; i += 8) {
    u32x4 v[8];
    for (int j = 0; j < 8; ++j) v[j] = p[(i + j) * ngroups];
    for (int j = 0; j < 8; ++j) add(v[j]);
  }
  for (; i < rows.count; ++i) add(p[i * ngroups]);
  f32x4* o = (f32x4*)(out + (long)r * pitch + 8L * g);
  o[0] = f32x4{acc[0], acc[1], acc[2], acc[3]};
  o[1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
}

template <bool A_T, bool B_N>
void launch_lay_out(const char* label, void* C, const float* bias,
                    const void* A, const void* B, long M, long N, long K,
                    hipStream_t stream, int xcd_swizzle) {
  const int tiles_n = (int)(N / BN);
  const int nwg = (int)(M / BM) * tiles_n;
  hipLaunchKernelGGL((k_gemm_bf16_lay_out<A_T, B_N>), dim3(nwg), dim3(512), 0,
                     stream, (__hip_bfloat16*)C, bias,
                     (const __hip_bfloat16*)A, (const __hip_bfloat16*)B,
                     (int)M, (int)N, (int)K, tiles_n, nwg, xcd_swizzle,
                     gemm_tile_group());
  check_hip(hipGetLastError(), label);
}

} // namespace

void launch_gemm_bf16_epilogue(void* C, const void* A, const void* B,
                               const float* bias, long M, long N, long K,
                               const char* layout, int splits, void* workspace,
                               hipStream_t stream, int xcd_swizzle) {
  const GemmLayout lay = gemm_parse_layout("gemm_bf16_epilogue", layout, true);
  gemm_require_tile_shape("gemm_bf16_epilogue", M, N, K);
  if (splits < 1 || splits > K / BK || splits > 65535)
    throw std::runtime_error(
        "gemm_bf16_epilogue requires 1 <= splits <= K / 64 (" +
        std::to_string(splits) + " splits, K = " + std::to_string(K) + ")");
  if (C == nullptr || A == nullptr || B == nullptr)
    throw std::runtime_error("gemm_bf16_epilogue: null operand");
  if ((uintptr_t)A % 16 != 0 || (uintptr_t)B % 16 != 0 ||
      (uintptr_t)C % 16 != 0)
    throw std::runtime_error("gemm_bf16_epilogue requires A, B and C on "
                             "16-byte boundaries");
  if ((uintptr_t)bias % 4 != 0)
    throw std::runtime_error("gemm_bf16_epilogue requires the bias on a "
                             "4-byte boundary");
  if (splits > 1 && (workspace == nullptr || (uintptr_t)workspace % 16 != 0))
    throw std::runtime_error("gemm_bf16_epilogue requires a workspace on a "
                             "16-byte boundary when splits > 1");

  if (splits > 1) {
    const unsigned grid = gemm_launch_splitk_partials(
        (float*)workspace, A, B, M, N, K, layout, splits, stream, xcd_swizzle);
    hipLaunchKernelGGL(k_splitk_reduce_bf16, dim3(grid), dim3(256), 0, stream,
                       (u32x4*)C, (const f32x4*)workspace, bias, M * N / 8,
                       splits, (int)N);
    check_hip(hipGetLastError(), "launch_gemm_bf16_epilogue(reduce)");
    return;
  }
  if (!lay.a_t && !lay.b_n) {
    const int tiles_n = (int)(N / BN);
    const int nwg = (int)(M / BM) * tiles_n;
    hipLaunchKernelGGL(k_gemm_bf16_nt_out, dim3(nwg), dim3(512), 0, stream,
                       (__hip_bfloat16*)C, bias, (const __hip_bfloat16*)A,
                       (const __hip_bfloat16*)B, (int)M, (int)N, (int)K,
                       tiles_n, nwg, xcd_swizzle, gemm_tile_group());
    check_hip(hipGetLastError(), "launch_gemm_bf16_epilogue(nt)");
    return;
  }
  if (!lay.a_t)
    return launch_lay_out<false, true>("launch_gemm_bf16_epilogue(nn)", C,
                                       bias, A, B, M, N, K, stream,
                                       xcd_swizzle);
  if (lay.b_n)
    return launch_lay_out<true, true>("launch_gemm_bf16_epilogue(tn)", C, bias,
                                      A, B, M, N, K, stream, xcd_swizzle);
  return launch_lay_out<true, false>("launch_gemm_bf16_epilogue(tt)", C, bias,
                                     A, B, M, N, K, stream, xcd_swizzle);
}

int colsum_plan(long M, long N, int n_cu) {
  if (M <= 0 || N <= 0 || n_cu <= 0) return 1;
  const long blocks = ((N + 7) / 8 + 63) / 64; // workgroups per chunk
  long want = (long)n_cu * kColsumWavesPerCu / blocks;
  const long hi = M / kColsumMinRows;
  if (want > hi) want = hi;
  if (want > kColsumMaxChunks) want = kColsumMaxChunks;
  return want < 1 ? 1 : (int)want;
}

void launch_colsum_bf16(float* out, const void* x, long M, long N, int R,
                        void* workspace, hipStream_t stream) {
  if (M <= 0 || N <= 0 || N % 8 != 0 || N > INT32_MAX)
    throw std::runtime_error("colsum_bf16 requires M >= 1 and N % 8 == 0");
  if (R < 1 || R > M || R > 65535)
    throw std::runtime_error("colsum_bf16 requires 1 <= chunks <= min(M, "
                             "65535)");
  if (out == nullptr || x == nullptr || (uintptr_t)out % 16 != 0 ||
      (uintptr_t)x % 16 != 0)
    throw std::runtime_error("colsum_bf16 requires x and out on 16-byte "
                             "boundaries");
  if (R > 1 && (workspace == nullptr || (uintptr_t)workspace % 16 != 0))
    throw std::runtime_error("colsum_bf16 requires a workspace on a 16-byte "
                             "boundary when chunks > 1");
  const int ngroups = (int)(N / 8);
  const long pitch = colsum_pitch(N);
  float* dst = R == 1 ? out : (float*)workspace;
  hipLaunchKernelGGL(k_colsum_bf16, dim3((ngroups + 63) / 64, R), dim3(64), 0,
                     stream, dst, (const u32x4*)x, M, ngroups, pitch, R);
  check_hip(hipGetLastError(), "launch_colsum_bf16");
  if (R == 1) return;
  launch_splitk_reduce_f32(out, workspace, pitch / 4, R, stream);
}

} // namespace hpk
