// quant.hip — convert-to-MX (OCP MX v1.0 §6.3): fp32 / bf16 rows to the
// block-scaled operands the K7 MX GEMMs read (gemm.hip): e4m3 bytes or e2m1
// nibbles plus one e8m0 scale byte per 32 consecutive elements along K.
// The bit-exact contract is written down in docs/gemm.md §"MX quantize".
//
// A contiguous [rows, K] tensor with K % 32 == 0 is a flat run of
// rows*K/32 MX blocks, and so are both outputs, so the kernel never looks
// at rows or K: it streams blocks.
//
// Work shape. A quad (4 adjacent lanes) owns a tile of 4 consecutive MX
// blocks per grid-stride iteration. Every 16-byte load instruction has the
// quad read one contiguous 64 B of one block, so loads stay coalesced, and
// a block's 32 elements lie in the quad's registers: the block maximum is
// two DPP quad_perm steps, no LDS. After conversion lane i holds a quarter
// of each of the 4 blocks; a 4x4 in-quad transpose (DPP again) hands lane i
// the whole of block i, which it writes with 16-byte stores. All four lanes
// know all four scales after the reduction, so lane 0 stores the tile's 4
// scale bytes as one dword; only a ragged last tile stores bytes.

#include "include/hpk.h"

#include <stdexcept>
#include <string>

namespace hpk {

namespace {

constexpr int kBlock = 256; // 4 wave64 per workgroup
// Same threshold as the K2-K4 streaming kernels: from here on the input is
// far beyond cache scale and is read once, so loads and element stores carry
// the nontemporal hint.
constexpr size_t kNtMinBytes = 32u << 20;

typedef unsigned u32;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef short i16x2 __attribute__((ext_vector_type(2)));

constexpr int kQuadXor1 = 0xB1; // DPP quad_perm [1,0,3,2]
constexpr int kQuadXor2 = 0x4E; // DPP quad_perm [2,3,0,1]

template <int Ctrl> __device__ __forceinline__ u32 quad_swap(u32 v) {
  return (u32)__builtin_amdgcn_update_dpp(0, (int)v, Ctrl, 0xF, 0xF, false);
}

// In-quad 4x4 transpose: on entry lane i holds d[j] = its piece of block j;
// on return lane i holds d[k] = lane k's piece of block i. Two butterfly
// stages, each exchanging one register of a pair with the partner lane.
template <int Ctrl, int Bit>
__device__ __forceinline__ void transpose_stage(u32& lo, u32& hi, int lane) {
  const bool upper = lane & Bit;
  const u32 got = quad_swap<Ctrl>(upper ? lo : hi);
  if (upper) lo = got;
  else hi = got;
}

__device__ __forceinline__ void quad_transpose(u32 (&d)[4], int lane) {
  transpose_stage<kQuadXor1, 1>(d[0], d[1], lane);
  transpose_stage<kQuadXor1, 1>(d[2], d[3], lane);
  transpose_stage<kQuadXor2, 2>(d[0], d[2], lane);
  transpose_stage<kQuadXor2, 2>(d[1], d[3], lane);
}

// One element, fp32 bits in: exponent field 0 (zero, subnormal) becomes a
// signed zero; the rest is scaled by 2^shift (exact: v_ldexp_f32) and
// clamped to +-vmax so that the conversion saturates and never makes a NaN.
template <bool FP4>
__device__ __forceinline__ float scaled(u32 bits, int shift) {
  constexpr float vmax = FP4 ? 6.0f : 448.0f;
  if ((bits & 0x7F800000u) == 0) bits &= 0x80000000u;
  const float v = __builtin_ldexpf(__builtin_bit_cast(float, bits), shift);
  return __builtin_amdgcn_fmed3f(v, -vmax, vmax);
}

// 4 elements to 4 e4m3 bytes (element 0 in the low byte). The conversion
// instruction's own scale operand stays at 1.0: the scaling above is exact.
__device__ __forceinline__ u32 cvt4_fp8(float a, float b, float c, float d) {
  i16x2 r = {0, 0};
  r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, a, b, 1.0f, false);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, c, d, 1.0f, true);
  return __builtin_bit_cast(u32, r);
}

template <bool NT>
__device__ __forceinline__ u32x4 load16(const u32x4* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

template <bool NT>
__device__ __forceinline__ void store16(u32x4* p, u32x4 v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// <BF16, FP4, NT>: input element type, output element format, cache hint.
template <bool BF16, bool FP4, bool NT>
__global__ __launch_bounds__(kBlock) void k_quantize_mx(
    u32x4* __restrict__ q, unsigned char* __restrict__ scale,
    const u32x4* __restrict__ x, size_t nblocks) {
  constexpr int L = BF16 ? 1 : 2; // 16-byte loads per lane per MX block
  constexpr int emax = FP4 ? 2 : 8;
  const int lane = threadIdx.x & 3;
  const size_t ntiles = (nblocks + 3) / 4;
  const size_t stride = (size_t)gridDim.x * (kBlock / 4);
  // quad-uniform loop: all 4 lanes of a quad share `tile`, so the DPP
  // exchanges below only ever read active lanes
  for (size_t tile = ((size_t)blockIdx.x * kBlock + threadIdx.x) >> 2;
       tile < ntiles; tile += stride) {
    const size_t b0 = tile * 4;
    const int nb = nblocks - b0 < 4 ? (int)(nblocks - b0) : 4;

    // all loads first: 4 (bf16) or 8 (fp32) 16-byte loads in flight per lane
    u32x4 in[4][L];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int h = 0; h < L; ++h) {
        in[j][h] = u32x4{0, 0, 0, 0};
        if (j < nb) in[j][h] = load16<NT>(x + ((b0 + j) * L + h) * 4 + lane);
      }

    u32 sc[4];        // e8m0 byte of block j, the same in all 4 lanes
    u32 out[2][4];    // [.][j]: this lane's 1 or 2 output dwords of block j
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // this lane's 8 elements of block j as fp32 bits, in element order:
      // fp32: elements h*16 + lane*4 + c; bf16: elements lane*8 + 0..7
      u32 f[8];
      if constexpr (BF16) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          f[2 * c] = in[j][0][c] << 16;
          f[2 * c + 1] = in[j][0][c] & 0xFFFF0000u;
        }
      } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) f[c] = in[j][c / 4][c % 4];
      }

      // largest |element| of the block: the maximum of the sign-less bit
      // patterns carries the largest exponent field; Inf/NaN give 255
      u32 m = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const u32 a = f[c] & 0x7FFFFFFFu;
        m = a > m ? a : m;
      }
      u32 o = quad_swap<kQuadXor1>(m);
      m = o > m ? o : m;
      o = quad_swap<kQuadXor2>(m);
      m = o > m ? o : m;
      const int e = (int)(m >> 23);
      const int s = e == 255 ? 255 : (e > emax ? e - emax : 0);
      sc[j] = (u32)s;

      float v[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) v[c] = scaled<FP4>(f[c], 127 - s);

      if constexpr (FP4) {
        // 8 elements -> 4 bytes (fp32: bytes 0-1 from load 0, 2-3 from load
        // 1; bf16: 4 consecutive bytes)
        u32 w = 0;
        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v[0], v[1], 1.0f, 0);
        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v[2], v[3], 1.0f, 1);
        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v[4], v[5], 1.0f, 2);
        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v[6], v[7], 1.0f, 3);
        out[0][j] = w;
      } else {
        out[0][j] = cvt4_fp8(v[0], v[1], v[2], v[3]);
        out[1][j] = cvt4_fp8(v[4], v[5], v[6], v[7]);
      }
    }

    // scale bytes: one dword per full tile, bytes for a ragged last tile
    if (nb == 4) {
      if (lane == 0)
        ((u32*)scale)[tile] =
            sc[0] | (sc[1] << 8) | (sc[2] << 16) | (sc[3] << 24);
    } else if (lane < nb) {
      const u32 mine = lane == 0 ? sc[0] : lane == 1 ? sc[1] : sc[2];
      scale[b0 + lane] = (unsigned char)mine;
    }

    // lane i gathers block b0 + i: t[k] is lane k's piece of it
    quad_transpose(out[0], lane);
    if constexpr (!FP4) quad_transpose(out[1], lane);
    if (lane < nb) {
      const u32(&t0)[4] = out[0];
      [[maybe_unused]] const u32(&t1)[4] = out[1];
      if constexpr (FP4) {
        u32x4 r;
        if constexpr (BF16) {
          r = u32x4{t0[0], t0[1], t0[2], t0[3]};
        } else {
          // lane k sent (bytes of load 0) | (bytes of load 1) << 16; the
          // block's 16 bytes are the four low halves, then the four high
          r = u32x4{(t0[0] & 0xFFFFu) | (t0[1] << 16),
                    (t0[2] & 0xFFFFu) | (t0[3] << 16),
                    (t0[0] >> 16) | (t0[1] & 0xFFFF0000u),
                    (t0[2] >> 16) | (t0[3] & 0xFFFF0000u)};
        }
        store16<NT>(q + b0 + lane, r);
      } else {
        u32x4 r0, r1;
        if constexpr (BF16) {
          // lane k's two dwords are bytes k*8 .. k*8+7 of the block
          r0 = u32x4{t0[0], t1[0], t0[1], t1[1]};
          r1 = u32x4{t0[2], t1[2], t0[3], t1[3]};
        } else {
          // load h of lane k is bytes h*16 + k*4 .. +3 of the block
          r0 = u32x4{t0[0], t0[1], t0[2], t0[3]};
          r1 = u32x4{t1[0], t1[1], t1[2], t1[3]};
        }
        store16<NT>(q + (b0 + lane) * 2, r0);
        store16<NT>(q + (b0 + lane) * 2 + 1, r1);
      }
    }
  }
}

template <bool BF16, bool FP4>
void launch_variant(void* q, void* scale, const void* x, size_t nblocks,
                    hipStream_t stream) {
  const size_t threads = (nblocks + 3) / 4 * 4; // one quad per 4-block tile
  size_t grid = (threads + kBlock - 1) / kBlock;
  if (grid > kQuantMaxGrid) grid = kQuantMaxGrid;
  const bool nt = nblocks * 32 * (BF16 ? 2 : 4) >= kNtMinBytes;
  auto* kernel = nt ? k_quantize_mx<BF16, FP4, true>
                    : k_quantize_mx<BF16, FP4, false>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, (u32x4*)q,
                     (unsigned char*)scale, (const u32x4*)x, nblocks);
}

} // namespace

void launch_quantize_mx(void* q, void* scale, const void* x, int x_is_bf16,
                        int fmt, long rows, long K, hipStream_t stream) {
  if (fmt != kMxFp8 && fmt != kMxFp4)
    throw std::invalid_argument("launch_quantize_mx: fmt must be 0 (mxfp8) "
                                "or 1 (mxfp4), got " + std::to_string(fmt));
  if (rows < 1 || K < 32 || K % 32 != 0)
    throw std::invalid_argument("launch_quantize_mx: need rows >= 1 and K a "
                                "positive multiple of 32");
  if ((uintptr_t)x % 16 || (uintptr_t)q % 16 || (uintptr_t)scale % 4)
    throw std::invalid_argument("launch_quantize_mx: x and q must be 16-byte "
                                "aligned, scale 4-byte aligned");
  const size_t nblocks = (size_t)rows * (size_t)(K / 32);
  if (x_is_bf16) {
    if (fmt == kMxFp4) launch_variant<true, true>(q, scale, x, nblocks, stream);
    else launch_variant<true, false>(q, scale, x, nblocks, stream);
  } else {
    if (fmt == kMxFp4) launch_variant<false, true>(q, scale, x, nblocks, stream);
    else launch_variant<false, false>(q, scale, x, nblocks, stream);
  }
  check_hip(hipGetLastError(), "launch_quantize_mx");
}

} // namespace hpk
