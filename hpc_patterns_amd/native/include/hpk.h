// hpk.h — C++ API of the MI355X-native HPC-patterns core library.
//
// Brand-new CDNA4/HIP design with the capabilities of the reference suite
// (argonne-lcf/HPC-Patterns): hand-written gfx950 kernels (the reference's
// SYCL parallel_for / omp-target loops, see reference concurency/bench.hpp:7-31,
// allreduce-mpi-sycl.cpp:27-41), a multi-hipStream/hipGraph concurrency engine
// (reference bench_sycl.cpp:19-144 / bench_omp.cpp), xGMI topology discovery
// (reference p2p/topology.cpp, Level-Zero Sysman -> rocm_smi/HIP here), and
// HIP-IPC one-sided transport (reference MPI_Win/MPI_Put path,
// p2p/peer2pear.cpp:68-102).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace hpk {

// ---------------------------------------------------------------------------
// Error handling
// ---------------------------------------------------------------------------
void check_hip(hipError_t e, const char* what);

// ---------------------------------------------------------------------------
// Kernels (kernels.hip) — all launch asynchronously on `stream` unless noted.
// ---------------------------------------------------------------------------

// K1 "C" compute command: every work-item runs 64*tripcount dependent FMAs on
// registers and stores one float (reference bench.hpp:23-31 MAD_64 payload).
void launch_busy_wait(float* out, long tripcount, long globalsize,
                      hipStream_t stream);

// K1-MFMA variant: every wave runs `tripcount` chained
// v_mfma_f32_16x16x32_bf16 ops — lights up the matrix cores so concurrency
// profiles show MFMA utilisation. n_waves waves of 64 lanes.
void launch_busy_wait_mfma(float* out, long tripcount, long n_waves,
                           hipStream_t stream);

// K2 shader-copy: vectorized 16B grid-stride copy (the "shader blit" sibling
// of hipMemcpyAsync's SDMA path). Pointers may be in any HIP-visible space.
void launch_copy_kernel(void* dst, const void* src, size_t nbytes,
                        hipStream_t stream);
// Tunable variant for micro-benchmarking: unroll 1 or 4 (16 B vs 64 B per
// thread per iteration), or 5 = the nontemporal 16 B kernel; grid_cap = max
// workgroups.
void launch_copy_kernel_tuned(void* dst, const void* src, size_t nbytes,
                              hipStream_t stream, int unroll,
                              size_t grid_cap);

// K4 fills (reference Initialize kernel, allreduce-mpi-sycl.cpp:34-41).
void launch_fill_f32(float* dst, float value, size_t n, hipStream_t stream);
// dst[i] = (float)i — device-side iota payload generator (reference
// fill_randomly host shuffle, peer2pear.cpp:8-17; shuffling is done on host,
// the plain iota fill runs on device).
void launch_iota_f32(float* dst, size_t n, hipStream_t stream);

// K3 accumulate: dst[i] += src[i] (reference Accumulate,
// allreduce-mpi-sycl.cpp:27-31), vectorized float4 grid-stride.
void launch_acc_f32(float* dst, const float* src, size_t n, hipStream_t stream);
// nontemporal variant (read-once src / rmw-once dst, beyond-L3 sizes)
void launch_acc_f32_nt(float* dst, const float* src, size_t n,
                       hipStream_t stream);

// K7 (r2, beyond-parity showcase): LDS-tiled bf16 MFMA GEMM —
// C[M,N] (fp32) = A[M,K] x B[N,K]^T, both operands bf16 K-contiguous.
// Default for M,N % 256 / K % 128: the 256^2-tile 8-phase deep pipeline
// (v_mfma_f32_16x16x32_bf16, counted vmcnt, zero bank conflicts);
// otherwise the plain/db 128^2 kernels (HPK_GEMM_VARIANT /
// HPK_GEMM_WAVES select). Optional bijective XCD workgroup swizzle.
// Requires M,N % 128 == 0 and K % 64 == 0 (throws otherwise).
void launch_gemm_bf16_nt(float* C, const void* A, const void* B, long M,
                         long N, long K, hipStream_t stream,
                         int xcd_swizzle = 1);
// fp8 (OCP e4m3): 256-divisible shapes default to the 256^2 32x32x64
// scaled-MFMA kernel with hardcoded x1.0 scales (2.2 PF); otherwise the
// mfma_f32_16x16x32_fp8_fp8 family.
void launch_gemm_fp8_nt(float* C, const void* A, const void* B, long M,
                        long N, long K, hipStream_t stream,
                        int xcd_swizzle = 0);
// int8 GEMM (mfma_i32_16x16x64_i8, ~2x the bf16 rate, exact int32
// accumulation): C[M,N] int32 = A[M,K] x B[N,K]^T, int8 operands.
void launch_gemm_i8_nt(int* C, const void* A, const void* B, long M,
                       long N, long K, hipStream_t stream,
                       int xcd_swizzle = 0);
// Block-scaled MX-fp8 (mfma_scale_f32_16x16x128_f8f6f4, 2x the bf16
// rate): C = (A .* 2^(As-127)) x (B .* 2^(Bs-127))^T with one e8m0 scale
// byte per 32-element K-block (As: [M][K/32], Bs: [N][K/32], uint8).
// Requires M,N,K % 128 == 0.
void launch_gemm_mxfp8_nt(float* C, const void* A, const void* B,
                          const void* As, const void* Bs, long M, long N,
                          long K, hipStream_t stream, int xcd_swizzle = 0);
// Block-scaled MX-fp4 (e2m1, the 4x-bf16 rate class): A/B are
// nibble-PACKED uint8 [rows][K/2] (low nibble = even k), scales as for
// mxfp8. Operand/scale layout measured on hardware: diagonal (one OCP
// 32-block per lane, own-lane scale — scripts/probes/fp4_probe*).
void launch_gemm_mxfp4_nt(float* C, const void* A, const void* B,
                          const void* As, const void* Bs, long M, long N,
                          long K, hipStream_t stream, int xcd_swizzle = 0);
// Host-only: the name of the kernel the launcher for `kind`
// (bf16|fp8|i8|mxfp8|mxfp4) runs at this shape under the current HPK_*
// environment — bf16_plain8|plain4|db8|db4|8ph, fp8_plain|8ph|32,
// i8_plain|8ph|32, mxfp8_plain|32, mxfp4_w8|w4|db|32|32h. The launchers
// switch on the same decision; illegal shapes and unknown kinds throw.
const char* gemm_variant_name(const char* kind, long M, long N, long K);

// Split-K (gemm_splitk.hip): the 128^2-tile GEMM for small M, N and a long
// K. The grid is (tiles, splits): split s of a tile walks only its own
// K-tiles and writes a 128x128 partial to slice s of `workspace`
// ([splits][M][N], C's element type, 16-byte aligned); a second kernel on
// the same stream then folds the slices in ascending s,
//   C = ((P0 + P1) + P2) + ...,
// so the result is the same bits on every run. splits == 1 writes C
// directly: no workspace, no second kernel. Contract: docs/gemm.md.
//
// Which K-tiles (of T = K / 64) split s of S owns: T / S + (s < T % S)
// consecutive tiles from s * (T / S) + min(s, T % S). The kernel, the
// launchers and the tests all call this one function.
struct SplitKRange {
  long first, count;
};
__host__ __device__ inline SplitKRange gemm_splitk_ktiles(long T, int S,
                                                          int s) {
  const long q = T / S, r = T % S;
  return {s * q + (s < r ? s : r), q + (s < r ? 1 : 0)};
}
// The automatic split count (pure host; n_cu is the device's CU count).
// M, N are rounded up to 128 and K to 64; tiles = (M/128)*(N/128),
// T = K/64. 1 when tiles >= n_cu, else n_cu / tiles clamped to
// [1, min(T / kSplitKMinTiles, kSplitKMaxSplits)]. Both constants come from
// the sweep in profiles/gemm_splitk.md (scripts/gemm_splitk_sweep.py).
constexpr int kSplitKMinTiles = 8;
constexpr int kSplitKMaxSplits = 64;
int gemm_splitk_plan(long M, long N, long K, int n_cu);
// Workgroups of the fold kernel above which it walks grid-stride.
constexpr int kSplitKReduceMaxGrid = 1024;
// The fold alone, for fp32 partials: C[i] = ((P0[i] + P1[i]) + ...) over the
// S slices of `workspace` ([S][nvec] 16-byte vectors, nvec = M * N / 4), on
// `stream`, behind whatever wrote the slices there. The split-K launchers
// below and launch_gemm_bf16_layout_splitk share it. Throws
// std::runtime_error unless nvec % 256 == 0, S >= 2 and both pointers are
// non-null and on 16-byte boundaries.
void launch_splitk_reduce_f32(float* C, const void* workspace, long nvec,
                              int S, hipStream_t stream);
// Throw std::runtime_error unless M,N % 128 == 0, K % 64 == 0,
// 1 <= splits <= K / 64 and (splits == 1 or workspace != nullptr).
void launch_gemm_splitk_bf16_nt(float* C, const void* A, const void* B,
                                long M, long N, long K, int splits,
                                void* workspace, hipStream_t stream,
                                int xcd_swizzle = 0);
void launch_gemm_splitk_fp8_nt(float* C, const void* A, const void* B,
                               long M, long N, long K, int splits,
                               void* workspace, hipStream_t stream,
                               int xcd_swizzle = 0);
void launch_gemm_splitk_i8_nt(int* C, const void* A, const void* B, long M,
                              long N, long K, int splits, void* workspace,
                              hipStream_t stream, int xcd_swizzle = 0);

// Operand layouts (gemm_layout.hip): the bf16 128^2-tile GEMM for operands
// that are not K-contiguous. `layout` names transA then transB, row-major:
//   "nn": A [M,K], B [K,N]    "tn": A [K,M], B [K,N]    "tt": A [K,M], B [N,K]
// C [M,N] fp32. An operand stored [K, X] is staged by the same 16-byte
// DMAs and read from LDS with ds_read_b64_tr_b16; the result is the bits
// bf16_db8 gives on a materialised transpose. Contract: docs/gemm.md.
// Throws std::runtime_error unless M,N % 128 == 0, K % 64 == 0 and A, B
// start on 16-byte boundaries; std::invalid_argument on any other layout
// string, "nt" included (launch_gemm_bf16_nt owns it). Tile order:
// row-major unless HPK_GEMM_GROUP is set.
void launch_gemm_bf16_layout(float* C, const void* A, const void* B, long M,
                             long N, long K, const char* layout,
                             hipStream_t stream, int xcd_swizzle = 0);
// Split-K for the same three layouts (gemm_layout_splitk.hip), for the dW
// product of a linear layer: a small [M,N] output summed over a long K (the
// tokens). Grid (tiles, splits); split s walks the K-tiles
// gemm_splitk_ktiles(K / 64, splits, s) — for an operand stored [K, X]
// those are ROWS kbeg .. of the tensor — and writes its partial to slice s
// of `workspace` ([splits][M][N] fp32); launch_splitk_reduce_f32 folds the
// slices in ascending s. splits == 1 writes C directly: no workspace, no
// second kernel, and the bits of launch_gemm_bf16_layout. For every splits
// the result is the bits of launch_gemm_splitk_bf16_nt on materialised
// transposes. Throws as launch_gemm_bf16_layout does, and
// std::runtime_error unless 1 <= splits <= min(K / 64, 65535) and, when
// splits > 1, workspace is non-null and C and workspace are on 16-byte
// boundaries.
void launch_gemm_bf16_layout_splitk(float* C, const void* A, const void* B,
                                    long M, long N, long K,
                                    const char* layout, int splits,
                                    void* workspace, hipStream_t stream,
                                    int xcd_swizzle = 0);

// The split-K tile kernels alone (gemm_splitk.hip, gemm_layout_splitk.hip):
// split s writes its fp32 partial to slice s of `workspace` and nothing
// folds them — for launch_gemm_bf16_epilogue, whose fold also adds the bias
// and converts. Shapes and alignment as the launchers above; splits >= 2.
void launch_gemm_splitk_bf16_nt_partials(float* workspace, const void* A,
                                         const void* B, long M, long N, long K,
                                         int splits, hipStream_t stream,
                                         int xcd_swizzle = 0);
void launch_gemm_bf16_layout_splitk_partials(float* workspace, const void* A,
                                             const void* B, long M, long N,
                                             long K, const char* layout,
                                             int splits, hipStream_t stream,
                                             int xcd_swizzle = 0);

// bf16 output with bias (gemm_epilogue.hip): C[M,N] bf16 row-major =
// bf16(op(A) @ op(B) + bias[n]) for layout nt | nn | tn | tt (operands as
// stored, as above). The bodies are k_gemm_bf16_nt_db<2,4> and
// k_gemm_bf16_lay with another epilogue: one fp32 add of bias[n] (fp32 [N];
// nullptr = no add at all), one round-to-nearest-even conversion, the
// 128x128 bf16 tile staged through the K loop's LDS and written as whole
// 256-byte rows. The accumulators are those of bf16_db8, so the result is
// bf16(c32 + bias) of the fp32 kernels bit for bit. splits > 1: the
// existing split-K tile kernels write fp32 partials to `workspace`
// ([splits][M][N] fp32) and one fold kernel computes
// bf16((((P0 + P1) + P2) + ...) + bias[n]). Contract: docs/gemm.md, "bf16
// output and bias". Throws std::invalid_argument on an unknown layout,
// std::runtime_error unless M,N % 128 == 0, K % 64 == 0,
// 1 <= splits <= min(K / 64, 65535), A, B, C (and the workspace when
// splits > 1) on 16-byte boundaries.
void launch_gemm_bf16_epilogue(void* C, const void* A, const void* B,
                               const float* bias, long M, long N, long K,
                               const char* layout, int splits, void* workspace,
                               hipStream_t stream, int xcd_swizzle = 0);
// Byte offset, in the staged 128x128 bf16 tile (32 KiB), of element
// (row, col): rows 2p and 2p+1 of a column share a dword (one
// v_cvt_pk_bf16_f32 result, one ds_write_b32), a row pair is 512 bytes, and
// the 16-byte chunk (4 columns) index is XORed with 4 * ((p >> 1) & 1) so
// that the two 16-lane halves of a write land on different banks. The
// kernel, and the bank enumeration in tests/test_gemm_epilogue_logic.py,
// call this function.
__host__ __device__ inline int gemm_out_lds_offset(int row, int col) {
  const int p = row >> 1;
  const int chunk = (col >> 2) ^ (((p >> 1) & 1) << 2);
  return 512 * p + 16 * chunk + 4 * (col & 3) + 2 * (row & 1);
}
// Tile (row, col) of the first element of 16-byte LDS read i (0 | 1) of
// thread t (0..511) in pass p (0 | 1) of the store loop: the thread owns
// columns 8 * (t & 15) .. +7 of rows `row` and `row + 1`; lanes 8..15 of a
// row take their odd chunk first, so 16 lanes cover all 16 bank windows.
struct GemmOutRead {
  int row, col;
};
__host__ __device__ inline GemmOutRead gemm_out_read(int t, int p, int i) {
  return {2 * (32 * p + (t >> 4)), 4 * (2 * (t & 15) + (i ^ ((t >> 3) & 1)))};
}

// Activation epilogues (gemm_act.hip): the kernels above with relu or the
// tanh-form gelu behind the accumulators, layout nt | nn | tn | tt.
//   kActForward: z = acc + bias[n] in fp32 (nullptr = no add), C[M,N] =
//     bf16(act(z)); aux, when non-null, receives bf16(z) [M,N] — bit for bit
//     what launch_gemm_bf16_epilogue writes.
//   kActGrad: C[M,N] = bf16(acc * act'(aux)), aux a bf16 [M,N] tensor (the
//     forward's z for gelu, its output or z for relu: act' = aux > 0); one
//     fp32 multiply before the one rounding. No bias.
// splits > 1: the split-K tile kernels write fp32 partials to `workspace`
// ([splits][M][N] fp32) and one fold kernel applies the same mode. The
// arithmetic, its error bound and the special values: docs/gemm.md,
// "Activations". Throws as launch_gemm_bf16_epilogue does (aux too must be
// on a 16-byte boundary); std::invalid_argument on an unknown activation
// or mode; std::runtime_error when kActGrad comes without aux or with a
// bias.
enum GemmAct { kActRelu = 0, kActGelu = 1 };
enum GemmActMode { kActForward = 0, kActGrad = 1 };
void launch_gemm_bf16_act(void* C, void* aux, const void* A, const void* B,
                          const float* bias, long M, long N, long K,
                          const char* layout, int act, int mode, int splits,
                          void* workspace, hipStream_t stream,
                          int xcd_swizzle = 0);

// Batched and strided operands (gemm_batched.hip): C_b[M,N] = alpha *
// op(A_b) @ op(B_b) for b = 0 .. batch-1, bf16 operands in layout nt | nn |
// tn | tt as stored (as above), C fp32 or bf16 (c_is_bf16). Each of A, B, C
// has a row stride ld and a batch stride bs, both in elements: a
// K-contiguous operand is read at P + b*bs + row*ld + k, an operand stored
// [K, X] at P + b*bs + k*ld + x, C_b[i][j] is written at C + b*bsC + i*ldc
// + j. The grid is (tiles, batch). The bodies are k_gemm_bf16_nt_db<2,4>
// and k_gemm_bf16_lay, so with alpha == 1 an fp32 C holds their bits; the
// epilogue is one fp32 multiply by alpha (always executed) and, for a bf16
// C, one round-to-nearest-even conversion behind it and the staged
// whole-row store of launch_gemm_bf16_epilogue. No bias, activation or
// split-K. Contract: docs/gemm.md, "Batched and strided operands". Throws
// std::invalid_argument on an unknown layout, std::runtime_error unless
//   M,N % 128 == 0, K % 64 == 0, 1 <= batch <= kGemmBatchedMaxBatch;
//   A and B on 16-byte boundaries, lda, ldb, bsA, bsB % 8 == 0, lda and ldb
//   at least the stored row length, bsA, bsB >= 0 (0 broadcasts the
//   operand);
//   gemm_batched_c_disjoint(batch, M, N, ldc, bsC);
//   a bf16 C on a 16-byte boundary with ldc, bsC % 8 == 0.
// With batch == 1 the three batch strides are ignored.
constexpr long kGemmBatchedMaxBatch = 65535; // gridDim.y
// ldc >= N and the batches' C images pairwise disjoint, in one of the two
// forms the launcher takes: batch-major (an image ends before the next
// begins) or interleaved inside a row (the batches are column blocks of one
// wide row). Pure host function; tests/test_gemm_batched_logic.py checks it
// against the enumerated address sets.
inline bool gemm_batched_c_disjoint(long batch, long M, long N, long ldc,
                                    long bsC) {
  if (batch < 1 || M < 1 || N < 1 || ldc < N) return false;
  if (batch == 1) return true;
  if (bsC >= (M - 1) * ldc + N) return true;
  return bsC >= N && ldc >= (batch - 1) * bsC + N;
}
void launch_gemm_bf16_batched(void* C, int c_is_bf16, const void* A,
                              const void* B, long M, long N, long K,
                              long batch, long lda, long bsA, long ldb,
                              long bsB, long ldc, long bsC, const char* layout,
                              float alpha, hipStream_t stream,
                              int xcd_swizzle = 0);

// Column sums of a bf16 matrix (gemm_epilogue.hip): out[n] = sum_m x[m,n],
// the bias gradient of a linear layer. x [M,N] bf16 contiguous, N % 8 == 0,
// 16-byte aligned; out fp32. Row chunk r of R sums rows colsum_rows(M, R, r)
// in ascending order in fp32; R == 1 writes `out`, else chunk r writes
// workspace[r * colsum_pitch(N) ..] and launch_splitk_reduce_f32 folds the
// R rows in ascending r into `out`, which then must hold colsum_pitch(N)
// floats (only the first N mean anything). Same bits on every run for the
// same (M, N, R). Throws std::runtime_error unless 1 <= R <= min(M, 65535),
// N % 8 == 0, x and out (and the workspace) on 16-byte boundaries.
__host__ __device__ inline SplitKRange colsum_rows(long M, int R, int r) {
  return gemm_splitk_ktiles(M, R, r);
}
inline long colsum_pitch(long N) { return (N + 1023) / 1024 * 1024; }
// Row chunks the front door uses (pure host): enough 64-thread workgroups
// for kColsumWavesPerCu waves per compute unit, at least kColsumMinRows
// rows per chunk, at most kColsumMaxChunks chunks.
constexpr int kColsumWavesPerCu = 16;
constexpr int kColsumMinRows = 32;
constexpr int kColsumMaxChunks = 256;
int colsum_plan(long M, long N, int n_cu);
void launch_colsum_bf16(float* out, const void* x, long M, long N, int R,
                        void* workspace, hipStream_t stream);

// MX quantize (quant.hip): the convert-to-MX step that makes the two MX
// GEMMs' operands from real data. x is [rows][K] contiguous fp32 (or bf16
// when x_is_bf16), K % 32 == 0; every 32 consecutive elements along K get
// one e8m0 scale byte (scale: uint8 [rows][K/32]) and are rounded to
// nearest-even, saturating, into q: fmt kMxFp8 -> e4m3 bytes [rows][K],
// fmt kMxFp4 -> e2m1 nibbles [rows][K/2], low nibble = even k. Bit-exact
// contract: docs/gemm.md. x and q 16-byte aligned, scale 4-byte aligned
// (throws otherwise). Grid-stride above kQuantMaxGrid workgroups.
enum { kMxFp8 = 0, kMxFp4 = 1 };
// 8 resident 256-thread blocks per CU. Measured at 1 GiB (profiles/
// membench_quantize.log): caps of 32768 and up run 6-13% faster, but then
// the grid-stride pass only starts beyond 1 GiB of fp32 input, out of reach
// of a quick test; 2048 keeps it testable at 64 MiB.
constexpr size_t kQuantMaxGrid = 2048;
void launch_quantize_mx(void* q, void* scale, const void* x, int x_is_bf16,
                        int fmt, long rows, long K, hipStream_t stream);

// Exact double-precision sum of n floats. Synchronizes `stream`.
// Replaces the reference's O(N log N) host sort+sum checksum
// (peer2pear.cpp:56-63) with an order-independent exact device reduction.
double reduce_sum_f32(const float* src, size_t n, hipStream_t stream);

// int32 twins (the reference instantiates miniapps for float AND int).
void launch_fill_i32(int* dst, int value, size_t n, hipStream_t stream);
void launch_acc_i32(int* dst, const int* src, size_t n, hipStream_t stream);
long long reduce_sum_i32(const int* src, size_t n, hipStream_t stream);

// Typed spellings for C++ callers templated on float|int (the miniapps).
// The _f32/_i32 names stay the bindings' entry points.
inline void launch_fill(float* d, float v, size_t n, hipStream_t s) {
  launch_fill_f32(d, v, n, s);
}
inline void launch_fill(int* d, int v, size_t n, hipStream_t s) {
  launch_fill_i32(d, v, n, s);
}
inline void launch_acc(float* d, const float* src, size_t n, hipStream_t s) {
  launch_acc_f32(d, src, n, s);
}
inline void launch_acc(int* d, const int* src, size_t n, hipStream_t s) {
  launch_acc_i32(d, src, n, s);
}
inline double reduce_sum(const float* p, size_t n, hipStream_t s) {
  return reduce_sum_f32(p, n, s);
}
inline double reduce_sum(const int* p, size_t n, hipStream_t s) {
  return (double)reduce_sum_i32(p, n, s);
}

// ---------------------------------------------------------------------------
// Concurrency engine (conc.hip) — reference bench<T>() ABI, bench.hpp:37-40.
// ---------------------------------------------------------------------------

// Modes:
//   serial       — one stream, synchronize after every command (baseline)
//   in_order     — N hipStreams (default: one per command), round-robin
//   host_threads — one std::thread + stream per command (reference
//                  bench_omp.cpp host_threads mode)
//   graph        — all commands as independent nodes of one hipGraph; the
//                  HIP analog of a SYCL out-of-order queue
//   out_of_order — alias of graph (HIP streams are strictly in-order; the
//                  graph scheduler is the runtime-managed concurrency path)
//   graph_explicit — same graph semantics but built with explicit node-API
//                  calls (hipGraphAddMemcpyNode1D / child-graph kernel
//                  nodes, all independent roots) instead of stream capture
//   nowait       — alias of in_order (reference bench_omp.cpp nowait mode)
extern const std::string allowed_modes;
bool mode_is_allowed(const std::string& mode);

// copy-engine selection for A2B commands (the reference's copy-engine env
// knobs as a first-class CLI switch):
//   auto   -> hipMemcpyAsync (runtime picks SDMA or blit)
//   shader -> hand-written K2 copy kernel (CU path)
//   sdma   -> explicit hsa_amd_memory_async_copy_on_engine (DMA path)
enum CopyEngine { kCopyEngineAuto = 0, kCopyEngineShader = 1,
                  kCopyEngineSdma = 2 };

struct ConcResult {
  long total_us = 0;                  // min over repetitions
  std::vector<long> per_cmd_us;       // serial mode: min per-command wall time
  std::vector<double> per_cmd_dev_ms; // hipEvent device time (profiling only)
  // unmeasured per-command entries are -1 (e.g. per_cmd_us outside serial
  // mode, per_cmd_dev_ms without --enable_profiling)
};

// commands: "C" or "A2B"/"AB" with A,B in {M,D,H,S} =
// malloc/hipMalloc/hipHostMalloc/hipMallocManaged (reference
// bench_sycl.cpp:55-72 letter DSL).
// params keys: tripcount_C, globalsize_C, globalsize_<CMD> (floats).
ConcResult conc_bench(const std::string& mode,
                      const std::vector<std::string>& commands,
                      const std::map<std::string, size_t>& params,
                      bool enable_profiling, int n_queues, int n_repetitions,
                      bool verbose, int copy_engine);

// ---------------------------------------------------------------------------
// Topology (topo.hip) — xGMI link discovery (reference p2p/topology.cpp).
// ---------------------------------------------------------------------------

struct LinkInfo {
  int p2p_accessible = 0; // hipDeviceCanAccessPeer
  int link_type = -1;     // hipExtGetLinkTypeAndHopCount type (2 == xGMI)
  int hops = -1;
  long min_bw_mbps = -1;  // rocm_smi min/max link bandwidth (if available)
  long max_bw_mbps = -1;
  long weight = -1;       // rocm_smi link weight (if available)
};

int device_count();
// NxN matrix; [i][i] is zero-initialized LinkInfo.
std::vector<std::vector<LinkInfo>> link_matrix();

// XCD compute-partition (SPX/DPX/CPX...) and memory-partition (NPS*) mode
// per device — the MI355X analog of the reference's tile-fission awareness.
struct PartitionInfo {
  std::string compute; // e.g. "SPX", "CPX"; empty if unavailable
  std::string memory;  // e.g. "NPS1"; empty if unavailable
};
std::vector<PartitionInfo> partition_info();
// Connected components under direct-P2P reachability (the reference's
// "connectivity planes", topology.cpp:76-89). MI355X nodes are fully
// connected, so this is usually one plane — the interesting data is the
// per-pair link table above.
std::vector<std::vector<int>> p2p_planes();

// ---------------------------------------------------------------------------
// IPC one-sided transport (ipc.hip) — reference MPI_Win/MPI_Put analog.
// ---------------------------------------------------------------------------

// 64-byte opaque handle for a hipMalloc'd region, exchangeable between
// processes (dmabuf IPC; requires HSA_ENABLE_IPC_MODE_LEGACY=0).
std::vector<uint8_t> ipc_get_handle(void* dptr);
void* ipc_open_handle(const std::vector<uint8_t>& handle);
void ipc_close_handle(void* dptr);

// ---------------------------------------------------------------------------
// Explicit SDMA-engine copies (sdma.hip) — hsa_amd_memory_async_copy[_on_
// engine]: copies placed on a named DMA engine, bypassing rocclr's
// blit-fallback heuristics (the reference's copy-engine selection knobs,
// done natively).
// ---------------------------------------------------------------------------
int sdma_num_engines(int device);
// Pipelined pageable<->device copy through pinned double-buffer staging on
// a named SDMA engine (blocking call; run it on its own thread to overlap
// with other commands). h2d: src pageable -> dst device; else reverse.
void staged_copy(void* dst, const void* src, size_t nbytes, int device,
                 int engine_index, bool h2d);
// engines usable for src_device -> dst_device peer copies (xGMI SDMA).
int sdma_num_engines_pair(int dst_device, int src_device);
// engine_index < 0 lets ROCr pick. Returns a handle; copy completes when
// sdma_wait(handle) returns (handle is consumed).
void* sdma_copy_begin(void* dst, const void* src, size_t nbytes, int device,
                      int engine_index);
void sdma_wait(void* handle);

// ---------------------------------------------------------------------------
// Step plan (step.hip) — the flagship step's four local commands behind one
// submit and one join. Everything that does not change from step to step
// (owning agents, engine ids, completion signals) is resolved once at
// construction, so submit() puts both PCIe copies on their engines back to
// back with no lookup, allocation or status query in between, and only then
// launches the two kernels: the copy pair is the step's critical path.
// Not thread-safe: one thread drives a plan.
// ---------------------------------------------------------------------------
struct StepCopy {
  void* dst = nullptr;
  const void* src = nullptr;
  size_t nbytes = 0;
};

// Below this H2D size the plan does not choose a push fraction by itself:
// waking the workers costs about what 2 % of the copy would save.
constexpr size_t kStepPushMinBytes = size_t(16) << 20;
// Push workers when HPK_STEP_PUSH_THREADS is not set: the smallest count at
// which the measured push rate stops rising (profiles/flagship_host_push.md).
constexpr int kStepPushDefaultThreads = 8;

// Host push (step.hip, include/push_pool.h). An engine-driven H2D is a
// stream of device reads whose requests travel host-bound, next to the D2H
// payload; bytes that the host stores straight into device memory (posted
// writes through the PCIe BAR) need none. The plan can therefore give the
// tail [head, nbytes) of its H2D copy to a pool of host threads and leave
// the head on the engine. Where the head ends and which thread stores what:
struct StepPushSplit {
  size_t head = 0;                               // engine copies [0, head)
  std::vector<std::pair<size_t, size_t>> ranges; // [begin, end) per thread
};
// Pure host function. head = (1 - g) * nbytes rounded down to 4 KiB; the
// ranges tile [head, nbytes) in order, each beginning on a 64-byte line and
// only the last non-empty one ending off a line; threads left without a
// line get an empty range. g <= 0: head == nbytes; g >= 1: head == 0.
StepPushSplit step_push_ranges(size_t nbytes, double g, int nthreads);

class StepPlan {
 public:
  // Construct with the device idle (the engine status query reports only
  // idle engines). Throws if the H2D and D2H copies do not resolve to two
  // distinct host SDMA engines. time_copies turns on ROCr's async-copy
  // profiling for the life of the plan and records the workers' times
  // (diagnostic; off in normal use).
  //
  // push_fraction is g, the share of H2D that host threads store:
  //   < 0  (default) — HPK_STEP_PUSH if set (0 = off, else the fraction);
  //        otherwise chosen once, here, from three times measured on the
  //        plan's own buffers (engine H2D alone, engine D2H alone, a pushed
  //        slice of up to 32 MiB) — which runs both copies once — and only
  //        for an H2D of kStepPushMinBytes or more;
  //   >= 0 — that fraction (1.0 pushes everything; for tests).
  // Whatever was asked, g is 0 when the CPU agent nearest the device is not
  // granted access to the H2D destination or the device reports no HDP
  // flush register. Thread count: HPK_STEP_PUSH_THREADS, 1..8.
  StepPlan(int device, StepCopy h2d, StepCopy d2h, StepCopy d2d,
           float* busy_out, long busy_globalsize, hipStream_t busy_stream,
           hipStream_t copy_stream, bool time_copies = false,
           double push_fraction = -1.0);
  ~StepPlan();
  StepPlan(const StepPlan&) = delete;
  StepPlan& operator=(const StepPlan&) = delete;

  // Wakes the push workers, then H2D head, D2H (engines), then busy-wait
  // and shader-copy kernels (streams). Throws if the previous submission was
  // not joined; that submission stays joinable.
  void submit(long tripcount);
  // Waits for the workers and flushes the HDP so the device sees what they
  // stored, waits for both copies, then synchronizes both kernel streams.
  // Returns at once when nothing is pending.
  void join();
  // join() if pending, then end the workers and destroy the signals.
  // Idempotent.
  void close();
  bool pending() const;

  // (start_ns, end_ns) of every engine copy joined so far, H2D then D2H
  // per submission, on the hsa_timestamp_ns() clock; (0, 0) for an H2D
  // that was pushed whole. Empty unless time_copies was set.
  const std::vector<std::pair<uint64_t, uint64_t>>& copy_times() const;
  void clear_copy_times();

  // What the plan chose.
  double push_fraction() const; // tail bytes / H2D bytes after rounding
  int push_threads() const;     // 0 when nothing is pushed
  bool push_access() const;     // CPU access granted and HDP flush present
  // Last joined step, time_copies only, else zeros: submit() entry to the
  // first worker's first store, and to the last worker's fence, in ns.
  std::pair<uint64_t, uint64_t> push_times() const;

  // Measurements behind profiles/flagship_host_push.md, on this plan's
  // buffers, copies only (no kernels): BAR access, push rate for 1/2/4/8
  // threads at 32 and 128 MiB, and the D2H engine time alone, next to the
  // engine H2D, next to a push of all of H2D and next to each g-split.
  // (name, value) rows; times in us, rates in GB/s. Nothing may be pending.
  std::vector<std::pair<std::string, double>> push_probe(int reps = 5);

 private:
  struct Impl;
  Impl* impl_;
};

// HSA system timestamp in ns — the clock StepPlan::copy_times() is on.
uint64_t hsa_timestamp_ns();

// ---------------------------------------------------------------------------
// Tracing (trace.hip) — roctx ranges for rocprofv3 --marker-trace.
// ---------------------------------------------------------------------------
void trace_push(const char* name);
void trace_pop();
void trace_mark(const char* name);

void enable_peer_access(int peer_device);
void memcpy_peer_async(void* dst, int dst_dev, const void* src, int src_dev,
                       size_t nbytes, hipStream_t stream);

} // namespace hpk
