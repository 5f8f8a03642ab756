// gemm_host.h — host-side steps shared by the launchers of the bf16
// 128^2-tile GEMM family (gemm_layout.hip, gemm_layout_splitk.hip,
// gemm_epilogue.hip, gemm_act.hip, gemm_batched.hip): the tile order from
// the environment, the layout string, the whole-tiles check and the
// partials step of a split-K product with a fused reduce. Host only: it
// emits no device code. `who` names the calling launcher in every message.
#pragma once

#include "gemm_device.h"
#include "hpk.h"

#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace hpk {

// tile order: row-major unless HPK_GEMM_GROUP asks for bands
inline int gemm_tile_group() {
  const char* genv = std::getenv("HPK_GEMM_GROUP");
  return genv ? std::atoi(genv) : 1;
}

// A is stored [K,M] (transA), B is stored [K,N] (no transB)
struct GemmLayout {
  bool a_t, b_n;
};

// "nn" | "tn" | "tt", and "nt" where the caller has a kernel for it
inline GemmLayout gemm_parse_layout(const char* who, const char* layout,
                                    bool with_nt) {
  const std::string lay = layout ? layout : "";
  if (lay != "nn" && lay != "tn" && lay != "tt" && !(with_nt && lay == "nt"))
    throw std::invalid_argument(std::string(who) + ": unknown layout '" +
                                lay + "' (" + (with_nt ? "nt|" : "") +
                                "nn|tn|tt)");
  return {lay[0] == 't', lay[1] == 'n'};
}

// whole tiles, dimensions the kernels' int arguments hold, a grid that is
// an int
inline void gemm_require_tile_shape(const char* who, long M, long N, long K) {
  if (M <= 0 || N <= 0 || K <= 0 || M % BM != 0 || N % BN != 0 ||
      K % BK != 0 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX ||
      (M / BM) * (N / BN) > INT32_MAX)
    throw std::runtime_error(std::string(who) + " requires M,N % 128 == 0 "
                             "and K % 64 == 0");
}

// First half of a split-K product whose caller folds the slices with a
// reduce kernel of its own (bias, conversion, activation in the same pass):
// the tile kernels that exist write their fp32 partials to `workspace`, and
// the return value is the grid of that reduce kernel, 256 threads each over
// M * N / 8 items.
inline unsigned gemm_launch_splitk_partials(float* workspace, const void* A,
                                            const void* B, long M, long N,
                                            long K, const char* layout,
                                            int splits, hipStream_t stream,
                                            int xcd_swizzle) {
  if (std::string(layout) == "nt")
    launch_gemm_splitk_bf16_nt_partials(workspace, A, B, M, N, K, splits,
                                        stream, xcd_swizzle);
  else
    launch_gemm_bf16_layout_splitk_partials(workspace, A, B, M, N, K, layout,
                                            splits, stream, xcd_swizzle);
  long grid = M * N / 8 / 256;
  if (grid > kSplitKReduceMaxGrid) grid = kSplitKReduceMaxGrid;
  return (unsigned)grid;
}

} // namespace hpk
