// gemm_act.hip — K7 with an activation in the epilogue: the bf16 128^2-tile
// GEMM of all four operand layouts writing
//
//   forward   Y = bf16(act(z)), z = acc + bias[n] in fp32, and, when asked,
//             Z = bf16(z) beside it (what the GELU backward needs)
//   gradient  D = bf16(acc * act'(aux)), aux a bf16 [M,N] tensor (Z for
//             gelu, Y or Z for relu): dz = (dy W2) . act'(z) out of the GEMM
//             that forms dy W2
//
// for act = relu | gelu (tanh form). k_gemm_bf16_nt_act and
// k_gemm_bf16_lay_act<A_T, B_N> run the K loops of k_gemm_bf16_nt_out and
// k_gemm_bf16_lay_out (gemm_epilogue.hip): include/gemm_bf16_nt_loop.inc
// and include/gemm_bf16_lay_loop.inc hold the one copy of each — staging,
// the counted vmcnt / lgkmcnt, the raw barriers, the MFMA operand order —
// so the accumulators are theirs bit for bit. They are kernels of their
// own, not a switch inside the parents (docs/findings.md #28).
//
// Forward epilogue: the Y tile goes through the staged image of
// gemm_epilogue.hip (gemm_out_lds_offset / gemm_out_read, include/hpk.h) in
// the first 32 KiB of the loop's LDS, the Z tile through a second image in
// the other 32 KiB; one barrier, then whole 256-byte rows of each.
//
// Gradient epilogue: the store path run backwards for aux. Every thread
// loads 2 x 16 bytes of two rows (the addresses it would store to),
// interleaves them into row-pair dwords and writes the two 16-byte chunks
// gemm_out_read names into the second image; after a barrier a lane takes
// the dwords of ITS rows and column (the C/D mapping) with ds_read_b32 at
// gemm_out_lds_offset — the banks of the forward ds_write_b32, conflict
// free — multiplies in fp32 and stores through the first image. No 2-byte
// global load, no multiply after the rounding.
//
// GELU arithmetic (docs/gemm.md, "Activations", with the error bound):
//   t = z * fma(z^2, kc, k)      = -2u log2(e),  u = sqrt(2/pi)(z + 0.044715 z^3)
//   forward   s = rcp(1 + exp2(t)),  gelu = z * s
//   gradient  E = exp2(-|t|), R = rcp(1 + E): s = t >= 0 ? E R : R and
//             s (1 - s) = E R R (neither overflows nor cancels);
//             gelu' = fma(z c2 (1 + 0.134145 z^2), s (1 - s), s)
// exp2 and rcp are v_exp_f32 and v_rcp_f32. Selects are v_cndmask: there is
// no divergent branch (ds_read_b64_tr_b16 needs EXEC all ones); the
// epilogues branch on kernel arguments only.
//
// splits > 1 launches the split-K tile kernels that exist and
// k_splitk_reduce_bf16_act folds their fp32 partials in ascending s and
// applies the same two modes; it reads aux linearly.

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

constexpr int kImgBytes = BM * BN * 2; // one staged bf16 tile: 32 KiB

// constants of the tanh GELU, rounded once from double
constexpr double kSqrt2OverPi = 0.7978845608028654;
constexpr double kLog2E = 1.4426950408889634;
constexpr float kGeluK = (float)(-2.0 * kSqrt2OverPi * kLog2E);
constexpr float kGeluKc = (float)(-2.0 * kSqrt2OverPi * 0.044715 * kLog2E);
constexpr float kGeluC2 = (float)(2.0 * kSqrt2OverPi);
constexpr float kGeluC3 = 0.134145f; // 3 * 0.044715

// t = -2u log2(e): exp2(t) = exp(-2u)
__device__ __forceinline__ float gelu_t(float z) {
  const float z2 = z * z;
  return z * __builtin_fmaf(z2, kGeluKc, kGeluK);
}

template <int ACT>
__device__ __forceinline__ float act_fwd(float z) {
  if (ACT == kActRelu) // NaN stays NaN, -Inf and +-0 give 0
    return z > 0.f ? z : (z == z ? 0.f : z);
  const float e = __builtin_amdgcn_exp2f(gelu_t(z));
  const float s = __builtin_amdgcn_rcpf(1.f + e);
  return z * s;
}

// act'(z)
template <int ACT>
__device__ __forceinline__ float act_grad(float z) {
  if (ACT == kActRelu) return z > 0.f ? 1.f : 0.f;
  const float t = gelu_t(z);
  const float E = __builtin_amdgcn_exp2f(-__builtin_fabsf(t));
  const float R = __builtin_amdgcn_rcpf(1.f + E);
  const float ER = E * R;
  const float s = t >= 0.f ? ER : R;
  const float ss = ER * R; // s (1 - s)
  const float m = (z * kGeluC2) * __builtin_fmaf(z * z, kGeluC3, 1.f);
  return __builtin_fmaf(m, ss, s);
}

// Forward epilogue of both GEMM kernels: acc is the 64x32 sub-tile of wave
// (wr, wc) in the C/D mapping row = 4*(lane>>4)+r, col = lane&15. Every
// wave must be done with `lds` (the K loop's last barrier).
template <int ACT>
__device__ __forceinline__ void store_tile_act(
    __hip_bfloat16* __restrict__ Y, __hip_bfloat16* __restrict__ Z,
    const float* __restrict__ bias, const f32x4 (&acc)[4][2],
    __hip_bfloat16* lds, long brow, long bcol, int N, int tid, int lane,
    int wr, int wc) {
  constexpr int MREP = 4, NREP = 2, WTM = 64, WTN = 32;
  char* img = (char*)lds;
  char* zimg = img + kImgBytes;
  float bv[NREP] = {};
  if (bias != nullptr)
    for (int n = 0; n < NREP; ++n)
      bv[n] = bias[bcol + wc * WTN + n * 16 + (lane & 15)];
  for (int m = 0; m < MREP; ++m)
    for (int n = 0; n < NREP; ++n) {
      const int row = wr * WTM + m * 16 + 4 * (lane >> 4);
      const int col = wc * WTN + n * 16 + (lane & 15);
      f32x4 z = acc[m][n];
      if (bias != nullptr) z = z + bv[n]; // nullptr: no add at all
      for (int r = 0; r < 4; r += 2) {
        const int off = gemm_out_lds_offset(row + r, col);
        if (Z != nullptr)
          *(lds_u32*)(zimg + off) = pack_bf16(z[r], z[r + 1]);
        *(lds_u32*)(img + off) =
            pack_bf16(act_fwd<ACT>(z[r]), act_fwd<ACT>(z[r + 1]));
      }
    }
  __syncthreads();
  flush_tile(Y, img, brow, bcol, N, tid);
  if (Z != nullptr) flush_tile(Z, zimg, brow, bcol, N, tid);
}

// Gradient epilogue: D = bf16(acc * act'(aux)).
template <int ACT>
__device__ __forceinline__ void store_tile_act_grad(
    __hip_bfloat16* __restrict__ D, const __hip_bfloat16* __restrict__ aux,
    const f32x4 (&acc)[4][2], __hip_bfloat16* lds, long brow, long bcol,
    int N, int tid, int lane, int wr, int wc) {
  constexpr int MREP = 4, NREP = 2, WTM = 64, WTN = 32;
  char* img = (char*)lds;
  char* ximg = img + kImgBytes;
  // flush_tile backwards: the two rows x 8 columns this thread would store
  u32x4 top[2], bot[2];
  for (int p = 0; p < 2; ++p) {
    const GemmOutRead r0 = gemm_out_read(tid, p, 0);
    const __hip_bfloat16* src =
        aux + (brow + r0.row) * (long)N + bcol + 8 * (tid & 15);
    top[p] = *(const u32x4*)src;
    bot[p] = *(const u32x4*)(src + N);
  }
  for (int p = 0; p < 2; ++p) {
    const GemmOutRead r0 = gemm_out_read(tid, p, 0);
    const GemmOutRead r1 = gemm_out_read(tid, p, 1);
    const u32x4 t = top[p], b = bot[p];
    const u32x4 ev = {(t[0] & 0xffffu) | (b[0] << 16),
                      (t[0] >> 16) | (b[0] & 0xffff0000u),
                      (t[1] & 0xffffu) | (b[1] << 16),
                      (t[1] >> 16) | (b[1] & 0xffff0000u)};
    const u32x4 od = {(t[2] & 0xffffu) | (b[2] << 16),
                      (t[2] >> 16) | (b[2] & 0xffff0000u),
                      (t[3] & 0xffffu) | (b[3] << 16),
                      (t[3] >> 16) | (b[3] & 0xffff0000u)};
    const bool odd_first = (tid >> 3) & 1;
    *(lds_u32x4*)(ximg + gemm_out_lds_offset(r0.row, r0.col)) =
        odd_first ? od : ev;
    *(lds_u32x4*)(ximg + gemm_out_lds_offset(r1.row, r1.col)) =
        odd_first ? ev : od;
  }
  __syncthreads();
  for (int m = 0; m < MREP; ++m)
    for (int n = 0; n < NREP; ++n) {
      const int row = wr * WTM + m * 16 + 4 * (lane >> 4);
      const int col = wc * WTN + n * 16 + (lane & 15);
      const f32x4 v = acc[m][n];
      for (int r = 0; r < 4; r += 2) {
        const int off = gemm_out_lds_offset(row + r, col);
        const unsigned x = *(const lds_u32*)(ximg + off);
        *(lds_u32*)(img + off) =
            pack_bf16(v[r] * act_grad<ACT>(bf16_lo(x)),
                      v[r + 1] * act_grad<ACT>(bf16_hi(x)));
      }
    }
  __syncthreads();
  flush_tile(D, img, brow, bcol, N, tid);
}

template <int ACT, int MODE>
__device__ __forceinline__ void act_epilogue(
    __hip_bfloat16* __restrict__ C, __hip_bfloat16* __restrict__ aux,
    const float* __restrict__ bias, const f32x4 (&acc)[4][2],
    __hip_bfloat16* lds, long brow, long bcol, int N, int tid, int lane,
    int wr, int wc) {
  if (MODE == kActForward)
    store_tile_act<ACT>(C, aux, bias, acc, lds, brow, bcol, N, tid, lane, wr,
                        wc);
  else
    store_tile_act_grad<ACT>(C, aux, acc, lds, brow, bcol, N, tid, lane, wr,
                             wc);
}

// k_gemm_bf16_nt_out (gemm_epilogue.hip) with the activation epilogues: 8
// waves as 2(M) x 4(N), 64x32 per wave, 2 buffers x (A|B) tile = 64 KiB
// LDS. aux: forward, where Z goes (nullptr: not written); gradient, the
// tensor act' is taken of.
template <int ACT, int MODE>
__global__ __launch_bounds__(512) void k_gemm_bf16_nt_act(
    __hip_bfloat16* __restrict__ C, __hip_bfloat16* __restrict__ aux,
    const float* __restrict__ bias, const __hip_bfloat16* __restrict__ A,
    const __hip_bfloat16* __restrict__ B, int M, int N, int K, int tiles_n,
    int nwg, int xcd_swizzle, int group) {
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

  act_epilogue<ACT, MODE>(C, aux, bias, acc, lds, brow, bcol, N, tid, lane,
                          wr, wc);
}

// k_gemm_bf16_lay_out (gemm_epilogue.hip) with the activation epilogues.
// A_T: A is stored [K,M]; B_N: B is stored [K,N].
template <bool A_T, bool B_N, int ACT, int MODE>
__global__ __launch_bounds__(512) void k_gemm_bf16_lay_act(
    __hip_bfloat16* __restrict__ C, __hip_bfloat16* __restrict__ aux,
    const float* __restrict__ bias, const __hip_bfloat16* __restrict__ A,
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

  act_epilogue<ACT, MODE>(C, aux, bias, acc, lds, brow, bcol, N, tid, lane,
                          wr, wc);
}

// The fold of k_splitk_reduce_bf16 (gemm_epilogue.hip) with the two modes
// behind it. z[8i .. 8i+7] = (((P0 + P1) + P2) + ...) + bias[n], s
// ascending; forward: aux[i] = bf16(z) when aux is given, C[i] =
// bf16(act(z)); gradient: C[i] = bf16(fold * act'(aux[i])). nvec8 = M * N /
// 8 per slice, a multiple of 2048, so there is no tail, and N % 8 == 0 keeps
// a lane's 8 outputs in one row. Plain loads, as there.
template <int ACT, int MODE>
__global__ __launch_bounds__(256) void k_splitk_reduce_bf16_act(
    u32x4* __restrict__ C, u32x4* __restrict__ aux,
    const f32x4* __restrict__ P, const float* __restrict__ bias, long nvec8,
    int S, int N) {
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
    if (MODE == kActForward) {
      if (bias != nullptr) { // nullptr: no add at all
        const float* b = bias + (8 * i) % N;
        const f32x4 bl = {b[0], b[1], b[2], b[3]};
        const f32x4 bh = {b[4], b[5], b[6], b[7]};
        lo = lo + bl;
        hi = hi + bh;
      }
      if (aux != nullptr) {
        const u32x4 z = {pack_bf16(lo[0], lo[1]), pack_bf16(lo[2], lo[3]),
                         pack_bf16(hi[0], hi[1]), pack_bf16(hi[2], hi[3])};
        aux[i] = z;
      }
      for (int j = 0; j < 4; ++j) {
        lo[j] = act_fwd<ACT>(lo[j]);
        hi[j] = act_fwd<ACT>(hi[j]);
      }
    } else {
      const u32x4 x = aux[i];
      for (int d = 0; d < 2; ++d) {
        lo[2 * d] *= act_grad<ACT>(bf16_lo(x[d]));
        lo[2 * d + 1] *= act_grad<ACT>(bf16_hi(x[d]));
        hi[2 * d] *= act_grad<ACT>(bf16_lo(x[2 + d]));
        hi[2 * d + 1] *= act_grad<ACT>(bf16_hi(x[2 + d]));
      }
    }
    const u32x4 out = {pack_bf16(lo[0], lo[1]), pack_bf16(lo[2], lo[3]),
                       pack_bf16(hi[0], hi[1]), pack_bf16(hi[2], hi[3])};
    C[i] = out;
  }
}

struct ActArgs {
  void* C;
  void* aux;
  const float* bias;
  const void* A;
  const void* B;
  long M, N, K;
  int splits;
  void* workspace;
  hipStream_t stream;
  int xcd_swizzle;
};

template <int ACT, int MODE>
void launch_act(const std::string& lay, const ActArgs& a) {
  const int tiles_n = (int)(a.N / BN);
  const int nwg = (int)(a.M / BM) * tiles_n;
  if (a.splits > 1) {
    const unsigned grid = gemm_launch_splitk_partials(
        (float*)a.workspace, a.A, a.B, a.M, a.N, a.K, lay.c_str(), a.splits,
        a.stream, a.xcd_swizzle);
    hipLaunchKernelGGL((k_splitk_reduce_bf16_act<ACT, MODE>), dim3(grid),
                       dim3(256), 0, a.stream, (u32x4*)a.C, (u32x4*)a.aux,
                       (const f32x4*)a.workspace, a.bias, a.M * a.N / 8,
                       a.splits, (int)a.N);
    check_hip(hipGetLastError(), "launch_gemm_bf16_act(reduce)");
    return;
  }
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(nwg), dim3(512), 0, a.stream,
                       (__hip_bfloat16*)a.C, (__hip_bfloat16*)a.aux, a.bias,
                       (const __hip_bfloat16*)a.A, (const __hip_bfloat16*)a.B,
                       (int)a.M, (int)a.N, (int)a.K, tiles_n, nwg,
                       a.xcd_swizzle, gemm_tile_group());
    check_hip(hipGetLastError(), "launch_gemm_bf16_act");
  };
  if (lay == "nt") return go(k_gemm_bf16_nt_act<ACT, MODE>);
  if (lay == "nn") return go(k_gemm_bf16_lay_act<false, true, ACT, MODE>);
  if (lay == "tn") return go(k_gemm_bf16_lay_act<true, true, ACT, MODE>);
  return go(k_gemm_bf16_lay_act<true, false, ACT, MODE>);
}

} // namespace

void launch_gemm_bf16_act(void* C, void* aux, const void* A, const void* B,
                          const float* bias, long M, long N, long K,
                          const char* layout, int act, int mode, int splits,
                          void* workspace, hipStream_t stream,
                          int xcd_swizzle) {
  gemm_parse_layout("gemm_bf16_act", layout, true); // throws unless valid
  const std::string lay = layout;
  if (act != kActRelu && act != kActGelu)
    throw std::invalid_argument("gemm_bf16_act: unknown activation " +
                                std::to_string(act));
  if (mode != kActForward && mode != kActGrad)
    throw std::invalid_argument("gemm_bf16_act: unknown mode " +
                                std::to_string(mode));
  gemm_require_tile_shape("gemm_bf16_act", M, N, K);
  if (splits < 1 || splits > K / BK || splits > 65535)
    throw std::runtime_error(
        "gemm_bf16_act requires 1 <= splits <= K / 64 (" +
        std::to_string(splits) + " splits, K = " + std::to_string(K) + ")");
  if (C == nullptr || A == nullptr || B == nullptr)
    throw std::runtime_error("gemm_bf16_act: null operand");
  if ((uintptr_t)A % 16 != 0 || (uintptr_t)B % 16 != 0 ||
      (uintptr_t)C % 16 != 0 || (uintptr_t)aux % 16 != 0)
    throw std::runtime_error("gemm_bf16_act requires A, B, C and aux on "
                             "16-byte boundaries");
  if ((uintptr_t)bias % 4 != 0)
    throw std::runtime_error("gemm_bf16_act requires the bias on a 4-byte "
                             "boundary");
  if (mode == kActGrad && (aux == nullptr || bias != nullptr))
    throw std::runtime_error("gemm_bf16_act: the gradient mode takes an aux "
                             "tensor and no bias");
  if (splits > 1 && (workspace == nullptr || (uintptr_t)workspace % 16 != 0))
    throw std::runtime_error("gemm_bf16_act requires a workspace on a "
                             "16-byte boundary when splits > 1");

  const ActArgs a = {C, aux, bias, A, B, M, N, K, splits, workspace, stream,
                     xcd_swizzle};
  if (act == kActRelu) {
    if (mode == kActForward) return launch_act<kActRelu, kActForward>(lay, a);
    return launch_act<kActRelu, kActGrad>(lay, a);
  }
  if (mode == kActForward) return launch_act<kActGelu, kActForward>(lay, a);
  return launch_act<kActGelu, kActGrad>(lay, a);
}

} // namespace hpk
