// gemm_epilogue.hip — K7 with a bf16 output and a bias: the bf16 128^2-tile
// GEMM of all four operand layouts writing C[M,N] = bf16(acc + bias[n])
// itself, instead of an fp32 C that an elementwise kernel reads back, and
// the column sum that is the bias gradient.
//
// k_gemm_bf16_nt_out and k_gemm_bf16_lay_out<A_T, B_N> are the bodies of
// k_gemm_bf16_nt_db<2,4> (gemm.hip) and k_gemm_bf16_lay (gemm_layout.hip),
// pasted: staging, the counted vmcnt / lgkmcnt, the raw barriers, the
// hpk_tile_id preamble and the MFMA operand order are theirs, so the
// accumulators are theirs bit for bit. They are kernels of their own, not
// an epilogue switch inside the parents: folding GEMM bodies changes the
// register allocation of the kernels that exist (docs/findings.md #28).
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
#include "include/gemm_layout_device.h"

#include <hip/hip_bf16.h>

#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace hpk {
namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef unsigned __attribute__((may_alias)) lds_u32;
typedef u32x4 __attribute__((may_alias)) lds_u32x4;

// bf16(lo) | bf16(hi) << 16, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

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
  // 2 passes x 512 threads x (2 rows x 8 columns)
  for (int p = 0; p < 2; ++p) {
    const GemmOutRead r0 = gemm_out_read(tid, p, 0);
    const GemmOutRead r1 = gemm_out_read(tid, p, 1);
    const u32x4 q0 =
        *(const lds_u32x4*)(img + gemm_out_lds_offset(r0.row, r0.col));
    const u32x4 q1 =
        *(const lds_u32x4*)(img + gemm_out_lds_offset(r1.row, r1.col));
    const bool odd_first = (tid >> 3) & 1;
    const u32x4 ev = odd_first ? q1 : q0; // columns 8j .. 8j+3, both rows
    const u32x4 od = odd_first ? q0 : q1; // columns 8j+4 .. 8j+7
    const u32x4 top = {(ev[0] & 0xffffu) | (ev[1] << 16),
                       (ev[2] & 0xffffu) | (ev[3] << 16),
                       (od[0] & 0xffffu) | (od[1] << 16),
                       (od[2] & 0xffffu) | (od[3] << 16)};
    const u32x4 bot = {(ev[0] >> 16) | (ev[1] & 0xffff0000u),
                       (ev[2] >> 16) | (ev[3] & 0xffff0000u),
                       (od[0] >> 16) | (od[1] & 0xffff0000u),
                       (od[2] >> 16) | (od[3] & 0xffff0000u)};
    __hip_bfloat16* dst = C + (brow + r0.row) * (long)N + bcol + 8 * (tid & 15);
    *(u32x4*)dst = top;
    *(u32x4*)(dst + N) = bot;
  }
}

// The body of k_gemm_bf16_nt_db<2,4> (gemm.hip): 8 waves as 2(M) x 4(N),
// 64x32 per wave, 2 buffers x (A|B) tile = 64 KiB LDS.
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
    // prefetch overwrites it — and, behind the last tile, before the
    // epilogue's image does
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  store_tile_bf16(C, bias, acc, lds, brow, bcol, N, tid, lane, wr, wc);
}

// The body of k_gemm_bf16_lay (gemm_layout.hip). A_T: A is stored [K,M];
// B_N: B is stored [K,N].
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
    // prefetch overwrites it — and, behind the last tile, before the
    // epilogue's image does
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

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

int tile_group() {
  // tile order: row-major unless HPK_GEMM_GROUP asks for bands
  const char* genv = std::getenv("HPK_GEMM_GROUP");
  return genv ? std::atoi(genv) : 1;
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
                     tile_group());
  check_hip(hipGetLastError(), label);
}

} // namespace

void launch_gemm_bf16_epilogue(void* C, const void* A, const void* B,
                               const float* bias, long M, long N, long K,
                               const char* layout, int splits, void* workspace,
                               hipStream_t stream, int xcd_swizzle) {
  const std::string lay = layout ? layout : "";
  if (lay != "nt" && lay != "nn" && lay != "tn" && lay != "tt")
    throw std::invalid_argument("gemm_bf16_epilogue: unknown layout '" + lay +
                                "' (nt|nn|tn|tt)");
  if (M <= 0 || N <= 0 || K <= 0 || M % BM != 0 || N % BN != 0 ||
      K % BK != 0 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX)
    throw std::runtime_error("gemm_bf16_epilogue requires M,N % 128 == 0 and "
                             "K % 64 == 0");
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
    if (lay == "nt")
      launch_gemm_splitk_bf16_nt_partials((float*)workspace, A, B, M, N, K,
                                          splits, stream, xcd_swizzle);
    else
      launch_gemm_bf16_layout_splitk_partials((float*)workspace, A, B, M, N,
                                              K, lay.c_str(), splits, stream,
                                              xcd_swizzle);
    const long nvec8 = M * N / 8;
    long grid = nvec8 / 256;
    if (grid > kSplitKReduceMaxGrid) grid = kSplitKReduceMaxGrid;
    hipLaunchKernelGGL(k_splitk_reduce_bf16, dim3((unsigned)grid), dim3(256),
                       0, stream, (u32x4*)C, (const f32x4*)workspace, bias,
                       nvec8, splits, (int)N);
    check_hip(hipGetLastError(), "launch_gemm_bf16_epilogue(reduce)");
    return;
  }
  if (lay == "nt") {
    const int tiles_n = (int)(N / BN);
    const int nwg = (int)(M / BM) * tiles_n;
    hipLaunchKernelGGL(k_gemm_bf16_nt_out, dim3(nwg), dim3(512), 0, stream,
                       (__hip_bfloat16*)C, bias, (const __hip_bfloat16*)A,
                       (const __hip_bfloat16*)B, (int)M, (int)N, (int)K,
                       tiles_n, nwg, xcd_swizzle, tile_group());
    check_hip(hipGetLastError(), "launch_gemm_bf16_epilogue(nt)");
    return;
  }
  if (lay == "nn")
    return launch_lay_out<false, true>("launch_gemm_bf16_epilogue(nn)", C,
                                       bias, A, B, M, N, K, stream,
                                       xcd_swizzle);
  if (lay == "tn")
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
