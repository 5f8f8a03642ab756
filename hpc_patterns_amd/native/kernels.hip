// kernels.hip — hand-written gfx950 (CDNA4) kernels for the pattern suite.
//
// These are the MI355X-native equivalents of the reference's device-code
// sites: the SYCL busy_wait parallel_for
// (reference concurency/bench_sycl.cpp:92-97 + bench.hpp:23-31), the A2B copy
// (bench_sycl.cpp:100), Accumulate / Initialize
// (allreduce-mpi-sycl.cpp:27-41), and the checksum payload
// (peer2pear.cpp:8-17). All kernels use 256-thread blocks (4 wave64) and
// grid-stride loops sized well past the 256 CUs / 8 XCDs.

#include "include/hpk.h"

#include <cstdio>
#include <stdexcept>
#include <string>

namespace hpk {

void check_hip(hipError_t e, const char* what) {
  if (e != hipSuccess) {
    throw std::runtime_error(std::string("HIP error in ") + what + ": " +
                             hipGetErrorString(e));
  }
}

namespace {

constexpr int kBlock = 256; // 4 wave64 per workgroup
// Streaming grid cap: 256 CUs want >> 256 workgroups in flight. Measured on
// MI355X (profiles/membench_1gpu_r3.log): 1 GiB copy at cap 65536 runs
// 2.60 TB/s payload vs 2.32 at 16384 — fewer grid-stride iterations per
// thread wins for pure streaming.
constexpr size_t kMaxGrid = 65536;
// Large copies, fills and accumulates (>= kNtMinBytes, far beyond cache
// scale) take the nontemporal kernels at a kNtMaxGrid-block grid: measured
// 3.02 TB/s payload vs 2.60 for the plain copy kernel at 1 GiB (96% of the
// 6.3 TB/s achievable HBM rate; membench r12). Smaller sizes keep the plain
// kernels (NT hints only pay beyond cache scale).
constexpr size_t kNtMinBytes = 32u << 20;
constexpr size_t kNtMaxGrid = 131072;

inline size_t stream_grid(size_t n_items) {
  size_t blocks = (n_items + kBlock - 1) / kBlock;
  if (blocks == 0) blocks = 1;
  if (blocks > kMaxGrid) blocks = kMaxGrid;
  return blocks;
}

// --------------------------------------------------------------------------
// K1: busy-wait FMA chain. Each work-item performs 64*tripcount dependent
// v_fma_f32 ops on registers and stores one float. The dependency chain makes
// the kernel's duration linear in tripcount (the property the autotuner's
// linear regression relies on) and independent of memory traffic.
// --------------------------------------------------------------------------
__global__ void k_busy_wait(float* __restrict__ out, long tripcount,
                            long globalsize) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < globalsize; i += stride) {
    float x = 1.0f + (float)i * 1e-9f;
    const float y = 1.000001f;
    for (long t = 0; t < tripcount; ++t) {
#pragma unroll
      for (int k = 0; k < 64; ++k) {
        x = __builtin_fmaf(y, x, y); // dependent chain: not foldable
      }
    }
    out[i] = x;
  }
}

// --------------------------------------------------------------------------
// K1-MFMA: matrix-core busy loop. Each wave chains `tripcount`
// v_mfma_f32_16x16x32_bf16 instructions through one accumulator, so the
// kernel occupies the MFMA pipe (visible as MfmaUtil in rocprof PMC runs)
// while doing no memory traffic.
// --------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

__global__ void k_busy_wait_mfma(float* __restrict__ out, long tripcount) {
  // Arbitrary nonzero fragments; value is irrelevant, occupancy of the MFMA
  // pipe is the payload.
  short seed = (short)(threadIdx.x + 1);
  bf16x8_t a = {seed, seed, seed, seed, seed, seed, seed, seed};
  bf16x8_t b = {1, 2, 3, 4, 5, 6, 7, 8};
  // Two independent accumulators: the 16x16x32 MFMA's dependent-accumulator
  // latency exceeds its issue interval, so a single chain leaves the pipe
  // under-issued (measured 1.63 PF with one chain at 2 waves/SIMD).
  f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f};
  f32x4_t acc1 = {0.f, 0.f, 0.f, 0.f};
  for (long t = 0; t < tripcount; t += 2) {
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc1, 0, 0, 0);
  }
  // One store per thread keeps the accumulators alive without noise.
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] =
      (acc0[0] + acc1[0]) * 1e-30f; // scaled to avoid overflow for readers
}

// --------------------------------------------------------------------------
// Streaming kernels: one grid-stride loop, and copy / fill / accumulate as
// <T, W> templates (element type, items of W = 1 or 4 elements) with one
// nontemporal sibling each.
// --------------------------------------------------------------------------
// `block` is a default argument so that blockDim.x is read in the calling
// kernel: read inside a __device__ function it compiles to the
// partial-last-workgroup form (a select plus a dependent global load in
// every kernel's preamble) instead of one scalar load.
template <class F>
__device__ __forceinline__ void for_each_item(size_t n, F f,
                                              size_t block = blockDim.x) {
  size_t i = (size_t)blockIdx.x * block + threadIdx.x;
  size_t stride = (size_t)gridDim.x * block;
  for (; i < n; i += stride) f(i);
}

// <T, W>: items of W elements of T — T itself, or HIP's float4 / int4 /
// uint4. The nontemporal siblings tell the cache hierarchy not to retain
// lines, a win for data far beyond L3 that is touched once; the builtins
// want the compiler's own vector type, hence vec4<T>.
template <class T, int W> struct item { typedef T type; };
template <class T> struct item<T, 4> { typedef HIP_vector_type<T, 4> type; };
template <class T, int W> using item_t = typename item<T, W>::type;
template <class T> using vec4 = T __attribute__((ext_vector_type(4)));

// K2: shader copy, 16 B per lane per iteration (1 KiB per wave-instruction)
// as <unsigned, 4>, bytes as <unsigned char, 1> for the tail and misaligned
// pointers. The SDMA sibling is plain hipMemcpyAsync; this kernel measures
// the shader-blit path and doubles as a D2D bandwidth workload.
template <class T, int W>
__global__ void k_copy(const item_t<T, W>* __restrict__ src,
                       item_t<T, W>* __restrict__ dst, size_t n) {
  for_each_item(n, [=](size_t i) { dst[i] = src[i]; });
}

__global__ void k_copy_nt(const uint4* __restrict__ src,
                          uint4* __restrict__ dst, size_t n16) {
  const vec4<unsigned>* s = (const vec4<unsigned>*)src;
  vec4<unsigned>* d = (vec4<unsigned>*)dst;
  for_each_item(n16, [=](size_t i) {
    vec4<unsigned> v = __builtin_nontemporal_load(s + i);
    __builtin_nontemporal_store(v, d + i);
  });
}

// 4x-unrolled variant: 64 B per thread per iteration, 4 loads in flight
// before the first store — deeper MLP for the HBM path at large sizes.
__global__ void k_copy_b16x4(const uint4* __restrict__ src,
                             uint4* __restrict__ dst, size_t n16) {
  size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n16; i += 4 * stride) {
    uint4 a = src[i];
    uint4 b = src[i + stride];
    uint4 c = src[i + 2 * stride];
    uint4 d = src[i + 3 * stride];
    dst[i] = a;
    dst[i + stride] = b;
    dst[i + 2 * stride] = c;
    dst[i + 3 * stride] = d;
  }
  for (; i < n16; i += stride) dst[i] = src[i];
}

// K4: fills (reference Initialize) and iota payload.
template <class T, int W>
__global__ void k_fill(item_t<T, W>* __restrict__ dst, T v, size_t n) {
  item_t<T, W> val;
  if constexpr (W == 4) val = item_t<T, 4>(v, v, v, v);
  else val = v;
  for_each_item(n, [=](size_t i) { dst[i] = val; });
}

__global__ void k_fill_nt(float4* __restrict__ dst, float v, size_t n4) {
  vec4<float>* d = (vec4<float>*)dst;
  vec4<float> val = {v, v, v, v};
  for_each_item(n4, [=](size_t i) { __builtin_nontemporal_store(val, d + i); });
}

__global__ void k_iota_f32(float* __restrict__ dst, size_t n) {
  for_each_item(n, [=](size_t i) { dst[i] = (float)i; });
}

// K3: accumulate dst[i] += src[i] (the ring-allreduce reduction kernel).
template <class T, int W>
__global__ void k_acc(item_t<T, W>* __restrict__ dst,
                      const item_t<T, W>* __restrict__ src, size_t n) {
  for_each_item(n, [=](size_t i) {
    if constexpr (W == 4) {
      item_t<T, 4> d = dst[i];
      item_t<T, 4> s = src[i];
      d.x += s.x;
      d.y += s.y;
      d.z += s.z;
      d.w += s.w;
      dst[i] = d;
    } else {
      dst[i] += src[i];
    }
  });
}

// NT variant: src is read once (never re-read) -> nontemporal load; dst is
// read-modify-write with an NT store (the line won't be revisited either).
__global__ void k_acc_nt(float4* __restrict__ dst,
                         const float4* __restrict__ src, size_t n4) {
  const vec4<float>* s = (const vec4<float>*)src;
  vec4<float>* d = (vec4<float>*)dst;
  for_each_item(n4, [=](size_t i) {
    vec4<float> a = __builtin_nontemporal_load(d + i);
    vec4<float> b = __builtin_nontemporal_load(s + i);
    __builtin_nontemporal_store(a + b, d + i);
  });
}

// --------------------------------------------------------------------------
// Exact checksums: one partial sum per block (wave64 shuffle reduction,
// then LDS across the block's 4 waves), host-side final sum of <=4096
// partials.
// --------------------------------------------------------------------------
template <class Acc>
__device__ __forceinline__ void block_sum(Acc s, Acc* __restrict__ partial) {
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  __shared__ Acc wsum[kBlock / 64];
  int lane = threadIdx.x & 63;
  int wave = threadIdx.x >> 6;
  if (lane == 0) wsum[wave] = s;
  __syncthreads();
  if (wave == 0) {
    Acc b = (lane < kBlock / 64) ? wsum[lane] : Acc(0);
    for (int off = 32; off > 0; off >>= 1) b += __shfl_down(b, off, 64);
    if (lane == 0) partial[blockIdx.x] = b;
  }
}

__global__ void k_reduce_partial_i32(const int* __restrict__ src, size_t n,
                                     long long* __restrict__ partial) {
  long long s = 0;
  for_each_item(n, [&](size_t i) { s += src[i]; });
  block_sum(s, partial);
}

__global__ void k_reduce_partial_f32(const float* __restrict__ src, size_t n,
                                     double* __restrict__ partial) {
  // float4 loads + 4 independent f64 accumulators: breaks the serial f64-add
  // dependency chain that capped the first version at 2.2 TB/s read.
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  size_t n4 = n / 4;
  if (((uintptr_t)src % 16) == 0) {
    // PLAIN loads on purpose: this kernel is the suite's checksum oracle.
    // An NT-load variant read a stale/partial view of freshly-copied data
    // once on gfx950 (p2p checksum exactly half, r24) — verification must
    // not depend on cache-hint semantics.
    const float4* src4 = (const float4*)src;
    for_each_item(n4, [&](size_t i) {
      float4 v = src4[i];
      s0 += (double)v.x;
      s1 += (double)v.y;
      s2 += (double)v.z;
      s3 += (double)v.w;
    });
    // tail elements by block 0 / thread 0..3
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4)
      s0 += (double)src[n4 * 4 + threadIdx.x];
  } else {
    for_each_item(n, [&](size_t i) { s0 += (double)src[i]; });
  }
  block_sum((s0 + s1) + (s2 + s3), partial);
}

// --------------------------------------------------------------------------
// Launch shapes, each decided once.
// --------------------------------------------------------------------------
template <class... P>
bool aligned16(const P*... p) {
  return (((uintptr_t)p % 16 == 0) && ...);
}

size_t nt_grid(size_t n_items) {
  size_t blocks = (n_items + kBlock - 1) / kBlock;
  return blocks > kNtMaxGrid ? kNtMaxGrid : blocks;
}

// Fill and accumulate, both element types, decide their shape here. All
// pointers 16-byte aligned and n >= 4: the 4-wide kernel over n4 = n/4
// items, then the scalar kernel over the 1-3 leftover elements in one
// 64-thread block. Otherwise n4 == 0 and the scalar kernel takes all n.
struct Vec4Shape {
  size_t n4;                    // 4-wide items; 0 = no 4-wide launch
  size_t first, count;          // the scalar kernel's elements
  unsigned grid, block;         // the scalar kernel's launch
  bool scalar() const { return n4 == 0 || count; }
};

Vec4Shape vec4_shape(bool aligned, size_t n) {
  if (aligned && n >= 4) return {n / 4, n / 4 * 4, n % 4, 1, 64};
  return {0, 0, n, (unsigned)stream_grid(n), kBlock};
}

// `vec` is the 4-wide kernel and `vec_grid` its grid rule: the plain
// template with stream_grid, or the nontemporal sibling with nt_grid. The
// scalar kernel is always the plain one, the nontemporal tail included.
template <class T>
void fill_impl(void (*vec)(item_t<T, 4>*, T, size_t),
               size_t (*vec_grid)(size_t), T* dst, T value, size_t n,
               hipStream_t stream) {
  const Vec4Shape sh = vec4_shape(aligned16(dst), n);
  if (sh.n4)
    hipLaunchKernelGGL(vec, dim3(vec_grid(sh.n4)), dim3(kBlock), 0, stream,
                       (item_t<T, 4>*)dst, value, sh.n4);
  if (sh.scalar())
    hipLaunchKernelGGL((k_fill<T, 1>), dim3(sh.grid), dim3(sh.block), 0,
                       stream, dst + sh.first, value, sh.count);
}

template <class T>
void acc_impl(void (*vec)(item_t<T, 4>*, const item_t<T, 4>*, size_t),
              size_t (*vec_grid)(size_t), T* dst, const T* src, size_t n,
              hipStream_t stream) {
  const Vec4Shape sh = vec4_shape(aligned16(dst, src), n);
  if (sh.n4)
    hipLaunchKernelGGL(vec, dim3(vec_grid(sh.n4)), dim3(kBlock), 0, stream,
                       (item_t<T, 4>*)dst, (const item_t<T, 4>*)src, sh.n4);
  if (sh.scalar())
    hipLaunchKernelGGL((k_acc<T, 1>), dim3(sh.grid), dim3(sh.block), 0, stream,
                       dst + sh.first, src + sh.first, sh.count);
}

// Copy's 1-15 leftover bytes after n16 16-byte items: one 256-thread block.
void launch_copy_tail(void* dst, const void* src, size_t n16, size_t tail,
                      hipStream_t stream) {
  hipLaunchKernelGGL((k_copy<unsigned char, 1>), dim3(1), dim3(kBlock), 0,
                     stream, (const unsigned char*)src + n16 * 16,
                     (unsigned char*)dst + n16 * 16, tail);
}

// Host half of both exact reductions: device-wide pre-sync, one partial per
// block in a stream-ordered scratch buffer, D2H, stream sync, host sum.
template <class T, class Acc>
Acc reduce_sum_impl(void (*kernel)(const T*, size_t, Acc*), const char* name,
                    const T* src, size_t n, hipStream_t stream) {
  auto check = [&](hipError_t e, const char* step) {
    if (e != hipSuccess) check_hip(e, (std::string(name) + " " + step).c_str());
  };
  // This is the suite's checksum oracle: device-wide sync first. Measured
  // on ROCm 7.2 (profiles/p2p_fail_r37.log): a kernel launched on another
  // stream immediately after hipStreamSynchronize() of the producing
  // stream intermittently (~1/25) read a partially-visible buffer; the
  // data was correct after hipDeviceSynchronize(). Verification must not
  // depend on cross-stream visibility timing.
  check(hipDeviceSynchronize(), "pre-sync");
  constexpr size_t kRedBlocks = 4096;
  size_t blocks = (n + (size_t)kBlock * 8 - 1) / ((size_t)kBlock * 8);
  if (blocks == 0) blocks = 1;
  if (blocks > kRedBlocks) blocks = kRedBlocks;

  Acc* d_partial = nullptr;
  check(hipMallocAsync((void**)&d_partial, blocks * sizeof(Acc), stream),
        "hipMallocAsync");
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, stream, src, n,
                     d_partial);
  check(hipGetLastError(), "kernel");

  std::vector<Acc> h(blocks);
  check(hipMemcpyAsync(h.data(), d_partial, blocks * sizeof(Acc),
                       hipMemcpyDeviceToHost, stream),
        "D2H");
  check(hipFreeAsync(d_partial, stream), "hipFreeAsync");
  check(hipStreamSynchronize(stream), "sync");

  Acc s = 0;
  for (Acc v : h) s += v;
  return s;
}

} // namespace

void launch_busy_wait(float* out, long tripcount, long globalsize,
                      hipStream_t stream) {
  size_t grid = stream_grid((size_t)globalsize);
  hipLaunchKernelGGL(k_busy_wait, dim3(grid), dim3(kBlock), 0, stream, out,
                     tripcount, globalsize);
  check_hip(hipGetLastError(), "launch_busy_wait");
}

void launch_busy_wait_mfma(float* out, long tripcount, long n_waves,
                           hipStream_t stream) {
  if (n_waves < 1) n_waves = 1;
  size_t blocks = ((size_t)n_waves * 64 + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_busy_wait_mfma, dim3(blocks), dim3(kBlock), 0, stream,
                     out, tripcount);
  check_hip(hipGetLastError(), "launch_busy_wait_mfma");
}

void launch_copy_kernel_tuned(void* dst, const void* src, size_t nbytes,
                              hipStream_t stream, int unroll,
                              size_t grid_cap) {
  if (!aligned16(dst, src)) {
    launch_copy_kernel(dst, src, nbytes, stream);
    return;
  }
  size_t n16 = nbytes / 16;
  size_t tail = nbytes - n16 * 16;
  // the caller's cap, not kMaxGrid; the body launches even when n16 == 0
  size_t blocks = (n16 + kBlock - 1) / kBlock;
  if (blocks == 0) blocks = 1;
  if (blocks > grid_cap) blocks = grid_cap;
  auto* body = unroll == 5   ? k_copy_nt // nontemporal streaming variant
               : unroll >= 4 ? k_copy_b16x4
                             : k_copy<unsigned, 4>;
  hipLaunchKernelGGL(body, dim3(blocks), dim3(kBlock), 0, stream,
                     (const uint4*)src, (uint4*)dst, n16);
  if (tail) launch_copy_tail(dst, src, n16, tail, stream);
  check_hip(hipGetLastError(), "launch_copy_kernel_tuned");
}

void launch_copy_kernel(void* dst, const void* src, size_t nbytes,
                        hipStream_t stream) {
  if (aligned16(dst, src)) {
    size_t n16 = nbytes / 16;
    size_t tail = nbytes - n16 * 16;
    if (n16) {
      const bool nt = nbytes >= kNtMinBytes;
      auto* body = nt ? k_copy_nt : k_copy<unsigned, 4>;
      hipLaunchKernelGGL(body, dim3(nt ? nt_grid(n16) : stream_grid(n16)),
                         dim3(kBlock), 0, stream, (const uint4*)src,
                         (uint4*)dst, n16);
    }
    if (tail) launch_copy_tail(dst, src, n16, tail, stream);
  } else {
    hipLaunchKernelGGL((k_copy<unsigned char, 1>),
                       dim3(stream_grid(nbytes)), dim3(kBlock), 0, stream,
                       (const unsigned char*)src, (unsigned char*)dst, nbytes);
  }
  check_hip(hipGetLastError(), "launch_copy_kernel");
}

void launch_fill_f32(float* dst, float value, size_t n, hipStream_t stream) {
  if (n * 4 >= kNtMinBytes)
    fill_impl(k_fill_nt, nt_grid, dst, value, n, stream);
  else
    fill_impl(k_fill<float, 4>, stream_grid, dst, value, n, stream);
  check_hip(hipGetLastError(), "launch_fill_f32");
}

void launch_iota_f32(float* dst, size_t n, hipStream_t stream) {
  hipLaunchKernelGGL(k_iota_f32, dim3(stream_grid(n)), dim3(kBlock), 0, stream,
                     dst, n);
  check_hip(hipGetLastError(), "launch_iota_f32");
}

void launch_acc_f32(float* dst, const float* src, size_t n, hipStream_t stream) {
  // beyond-L3 sizes: nontemporal variant (5.87 vs 5.11 TB/s at 1 GiB,
  // membench r22) — the ring-allreduce accumulate hot path
  if (aligned16(dst, src) && n * 4 >= kNtMinBytes) {
    launch_acc_f32_nt(dst, src, n, stream);
    return;
  }
  acc_impl(k_acc<float, 4>, stream_grid, dst, src, n, stream);
  check_hip(hipGetLastError(), "launch_acc_f32");
}

void launch_acc_f32_nt(float* dst, const float* src, size_t n,
                       hipStream_t stream) {
  if (!aligned16(dst, src) || n < 4) {
    launch_acc_f32(dst, src, n, stream);
    return;
  }
  acc_impl(k_acc_nt, nt_grid, dst, src, n, stream);
  check_hip(hipGetLastError(), "launch_acc_f32_nt");
}

// int32 twins (the reference instantiates its miniapps for float AND int
// via -DAPP_DATA_TYPE, mpi-sycl/CMakeLists.txt:4-5). No nontemporal path.
void launch_fill_i32(int* dst, int value, size_t n, hipStream_t stream) {
  fill_impl(k_fill<int, 4>, stream_grid, dst, value, n, stream);
  check_hip(hipGetLastError(), "launch_fill_i32");
}

void launch_acc_i32(int* dst, const int* src, size_t n, hipStream_t stream) {
  acc_impl(k_acc<int, 4>, stream_grid, dst, src, n, stream);
  check_hip(hipGetLastError(), "launch_acc_i32");
}

long long reduce_sum_i32(const int* src, size_t n, hipStream_t stream) {
  return reduce_sum_impl(k_reduce_partial_i32, "reduce_sum_i32", src, n,
                         stream);
}

double reduce_sum_f32(const float* src, size_t n, hipStream_t stream) {
  return reduce_sum_impl(k_reduce_partial_f32, "reduce_sum_f32", src, n,
                         stream);
}

} // namespace hpk
