// gemm_layout_device.h — device helpers shared by the translation units of
// the nn/tn/tt operand layouts (gemm_layout.hip, gemm_layout_splitk.hip,
// gemm_epilogue.hip, gemm_act.hip, gemm_batched.hip) and used by their K
// loop, gemm_bf16_lay_loop.inc:
// the [64 k-rows][128 x] LDS image of an operand stored [K, X] (lay_key,
// lay_off) and its transposed reads (TrFrag, lay_issue, lay_take,
// lds_addr). Everything sits in an anonymous namespace, so each translation
// unit gets its own internal copy, exactly as when these lived at the top
// of gemm_layout.hip (the move left its device code identical:
// profiles/gemm_layout_splitk.md). Derivation: docs/gemm.md, "Operand
// layouts".
#pragma once

#include "gemm_device.h"

#include <cstdint>

namespace hpk {
namespace {

typedef __attribute__((ext_vector_type(4))) short bf16x4;

// Row key of the [64][128]-bf16 image: rows are 256 B = all 64 banks, so a
// row's number does not move its banks and the key alone must spread a
// read's 32 lanes. Those lanes touch rows q (0..3) of two blocks 8 rows
// apart, chunks c0 and c0+1: (row&3)<<2 separates q, (row>>2)&3 separates
// the two blocks (bit 1) and leaves bit 0 to the chunk pair.
__device__ __forceinline__ int lay_key(int row) {
  return ((row & 3) << 2) | ((row >> 2) & 3);
}
// byte offset, from the tile's base, of global 16-byte chunk ch (0..15) of
// row `row` (0..63) — and, the XOR being an involution, the global chunk
// that LDS slot ch of the row holds
__device__ __forceinline__ int lay_off(int row, int ch) {
  return 256 * row + 16 * (ch ^ lay_key(row));
}

// The 16x16x32 operand fragment of columns x0 .. x0+15, k-step kk, from a
// [64][128] image at `tile`: block 1 is rows kk+8g .. +3, block 2 rows
// kk+8g+4 .. +7 (g = lane>>4); lane 4q+p of the group supplies row q,
// columns x0+4p .. +3 — through lay_off, because the XOR may swap the two
// chunks of a 32-byte span.
//
// The reads are inline asm, not __builtin_amdgcn_ds_read_tr16_b64: in
// front of the builtin the compiler puts an s_waitcnt vmcnt(0) of its own
// (it cannot tell the read from the LDS DMAs in flight), which drains the
// prefetch the counted vmcnt is there to keep. The price: the compiler
// does not count these reads, so lay_issue only starts them and the
// kernel waits (lgkmcnt) itself before lay_take hands the registers on.
// LDS returns in order, so lgkmcnt(n) retires everything but the n most
// recent reads whatever the compiler has interleaved.
struct TrFrag {
  bf16x4 lo, hi; // k = kfrag + 0..3, + 4..7
};
__device__ __forceinline__ void lay_issue(TrFrag& f, unsigned tile, int x0,
                                          int kk, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int ch = (x0 >> 3) + (p >> 1);
  const int r1 = kk + 8 * g + q;
  const unsigned a1 = tile + lay_off(r1, ch) + 8 * (p & 1);
  const unsigned a2 = tile + lay_off(r1 + 4, ch) + 8 * (p & 1);
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f.lo) : "v"(a1) : "memory");
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f.hi) : "v"(a2) : "memory");
}
// after the wait: ties the registers to this point of the instruction
// stream, so no MFMA that uses them can move above the wait
__device__ __forceinline__ bf16x8 lay_take(TrFrag& f) {
  asm volatile("" : "+v"(f.lo), "+v"(f.hi));
  return __builtin_shufflevector(f.lo, f.hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
// byte address of a __shared__ object in the LDS address space
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(uintptr_t)(
      const __attribute__((address_space(3))) void*)p;
}

} // namespace
} // namespace hpk
