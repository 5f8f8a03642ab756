// gemm_device.h — device helpers shared by the K7 GEMM translation units
// (gemm*.hip): vector typedefs, the bf16 pack and unpack, the 128^2-tile
// constants, the LDS skews, the tile order (hpk_group_remap, hpk_tile_id),
// the global_load_lds wrappers and the store of a staged bf16 tile
// (flush_tile). Everything sits in an anonymous namespace, so each
// translation unit gets its own internal copy, exactly as when these lived
// in the .hip files (every move left the device code identical:
// profiles/gemm_splitk.md, profiles/gemm_loop_fold.md). The K loops the
// kernels share are text, not functions: gemm_bf16_nt_loop.inc and
// gemm_bf16_lay_loop.inc.
#pragma once

#include "hpk.h"

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

namespace hpk {
namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(16))) int i32x16;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
// what a staged bf16 tile in LDS (an In[] array) is written and read as
typedef unsigned __attribute__((may_alias)) lds_u32;
typedef u32x4 __attribute__((may_alias)) lds_u32x4;

// bf16(lo) | bf16(hi) << 16, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
// the two halves of such a dword, widened (exact)
__device__ __forceinline__ float bf16_lo(unsigned d) {
  return __builtin_bit_cast(float, d << 16);
}
__device__ __forceinline__ float bf16_hi(unsigned d) {
  return __builtin_bit_cast(float, d & 0xffff0000u);
}

constexpr int BM = 128, BN = 128, BK = 64;

// one K-step's staging: A[128][64] + B[128][64] bf16 = 32 KiB
constexpr int TILE_HALF = BM * BK;            // elements per operand tile

// Cyclic-skew LDS layout: linear [128][64]-bf16 rows are 128 B, so
// ds_read_b128 fragment reads pile multiple lanes onto the same 4-dword
// bank window. gfx950's b128 lane groups are NOT contiguous 16-lane
// blocks — they mix rows AND kfrag halves (e.g. {0-3,12-15,20-27}:
// rows {0-3,12-15} at kfrag q and rows {4-11} at kfrag q+1,
// MI355X_MICROARCH.md LDS table) — so the shift must solve the mixed
// sets: rotating each row's K range by 16 elements per (row>>1)&3 class,
//   LDS(row, k) = (row, (k + 16*((row>>1)&3)) & 63)
// gives every row class an EVEN 4-dword window slot and the interleaved
// kfrag half the odd slots: all 16 lanes of each true lane group land on
// 16 distinct windows (verified by enumeration; a naive per-row-pair
// 8-element shift measured SQ_LDS_BANK_CONFLICT = 0.5x IDX_ACTIVE —
// 2-way residual — precisely because of the group mixing).
// The 16-element granule keeps every 16-B glds chunk and every 8-element
// fragment read contiguous, so the staging pre-applies the inverse on the
// GLOBAL source chunk address while the LDS write stays lane-linear (the
// global_load_lds requirement).
__device__ __forceinline__ long lds_skew(long e) { // tile elem -> LDS slot
  long row = e >> 6, k = e & 63;
  return (row << 6) | ((k + 16 * ((row >> 1) & 3)) & 63);
}
__device__ __forceinline__ long lds_unskew(long y) { // LDS slot -> tile elem
  long row = y >> 6, k = y & 63;
  return (row << 6) | ((k - 16 * ((row >> 1) & 3)) & 63);
}

// The fp8 and int8 skews of the same [128][64] image (one byte per
// element); their derivations stand at k_gemm_fp8_nt and k_gemm_i8_nt in
// gemm.hip.
__device__ __forceinline__ long lds_skew8(long e) { // tile elem -> LDS slot
  long row = e >> 6, k = e & 63;
  return (row << 6) | ((k + 16 * ((row >> 2) & 3)) & 63);
}
__device__ __forceinline__ long lds_unskew8(long y) {
  long row = y >> 6, k = y & 63;
  return (row << 6) | ((k - 16 * ((row >> 2) & 3)) & 63);
}
__device__ __forceinline__ long i8_skew(long e) {
  long row = e >> 6, k = e & 63;
  return (row << 6) | ((k + 32 * ((row >> 3) & 1)) & 63);
}
__device__ __forceinline__ long i8_unskew(long y) {
  long row = y >> 6, k = y & 63;
  return (row << 6) | ((k - 32 * ((row >> 3) & 1)) & 63);
}

// L2/MALL-aware grouped tile order (the CUTLASS threadblock-swizzle idea,
// re-derived for the 256 MiB MALL): remap the linear workgroup id so the
// ~256 CONCURRENTLY-resident workgroups cover a near-square super-block of
// output tiles — their A row-panels and B column-panels then stay resident
// in the LLC and each panel is streamed from HBM once per super-block
// instead of once per tile row. `group` = band width in N-tiles
// (HPK_GEMM_GROUP; <=1 keeps the row-major order). Bijective for any
// grid: the last band is simply narrower (gw < group).
__device__ __forceinline__ int hpk_group_remap(int wg, int tiles_n, int nwg,
                                               int group) {
  if (group <= 1) return wg;
  const int tiles_m = nwg / tiles_n;
  const int band = group * tiles_m;
  const int b = wg / band;
  const int within = wg - b * band;
  int gw = tiles_n - b * group;
  if (gw > group) gw = group;
  const int tm = within / gw;
  const int tn = b * group + within % gw;
  return tm * tiles_n + tn;
}

// This workgroup's output-tile index: optional bijective 8-XCD round-robin
// -> tile-linear remap, then the grouped order above. Tile row/col are
// id / tiles_n and id % tiles_n.
__device__ __forceinline__ int hpk_tile_id(int tiles_n, int nwg,
                                           int xcd_swizzle, int group) {
  int wg = (int)blockIdx.x;
  if (xcd_swizzle) {
    int q = nwg / 8, r = nwg % 8;
    int xcd = wg % 8, i = wg / 8;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + i;
  }
  return hpk_group_remap(wg, tiles_n, nwg, group);
}

// global_load_lds: each lane DMAs 16 B (4 B for the scale rows) from its
// OWN global address to (wave-uniform LDS base) + lane*size — so `l` is the
// WAVE chunk base and only `g` is per-lane; LDS images are lane-linear.
__device__ __forceinline__ void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)g,
      (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}
__device__ __forceinline__ void glds4(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)g,
      (__attribute__((address_space(3))) void*)l, 4, 0, 0);
}

// A staged bf16 tile (the image of gemm_out_lds_offset, hpk.h) from LDS at
// `img` to the 128x128 tile of `dst` at (brow, bcol), row stride ld (int or
// long): 2 passes x 512 threads x (2 rows x 8 columns), every thread two
// 16-byte LDS reads, 8 bit operations to separate the two rows and two
// 16-byte stores, so 16 lanes write one whole 256-byte row. Behind the
// barrier that completes the image.
template <typename Ld>
__device__ __forceinline__ void flush_tile(__hip_bfloat16* __restrict__ dst,
                                           const char* img, long brow,
                                           long bcol, Ld ld, int tid) {
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
    __hip_bfloat16* d =
        dst + (brow + r0.row) * (long)ld + bcol + 8 * (tid & 15);
    *(u32x4*)d = top;
    *(u32x4*)(d + ld) = bot;
  }
}

} // namespace
} // namespace hpk
