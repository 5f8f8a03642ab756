// interop_main.cpp — hpk_interop: runtime-interop proof.
//
// MI355X-native re-design of the reference OMP<->SYCL<->Level-Zero interop
// demos (reference sycl_omp_ze_interopt/interop_omp_sycl.cpp:13-75,
// interop_omp_ze_sycl.cpp:14-116). The reference proves two offload runtimes
// can share one device and exchange raw pointers; the equivalent runtime
// pair on the ROCm stack is the HIP runtime and RCCL (plus, across
// processes, HIP-IPC — exercised by hpk_p2p --engine ipc, and with torch by
// tests/test_gpu_kernels.py::test_interop_torch_allocator_shared_with_hip_kernels).
//
// Proofs, each asserted:
//  1. a hipMalloc'd pointer written by a hand-written HIP kernel is consumed
//     by RCCL (ncclAllReduce on a 1-rank communicator) with no copy;
//  2. RCCL enqueues onto an EXTERNALLY created hipStream (stream sharing
//     across runtimes — the reference's queue-from-native-handle proof);
//  3. the result is read back by the HIP runtime (hipMemcpy) and verified;
//  4. round-trip the other way: a buffer RCCL reduced into is handed to the
//     HIP accumulate kernel and re-verified.

#include "../hpc_patterns_amd/native/include/hpk.h"
#include "launch_util.h"

#include <rccl/rccl.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

using hpk_launch::check_nccl;

int main() {
  const size_t N = 1 << 20;
  hpk::check_hip(hipSetDevice(0), "set device");

  // runtime A: HIP — allocate + fill with a kernel on an explicit stream
  hipStream_t stream;
  hpk::check_hip(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking),
                 "stream");
  float* buf = nullptr;
  hpk::check_hip(hipMalloc(&buf, N * sizeof(float)), "malloc");
  hpk::launch_fill_f32(buf, 21.0f, N, stream);

  // runtime B: RCCL — same pointer, same externally-created stream
  ncclComm_t comm;
  ncclUniqueId id;
  check_nccl(ncclGetUniqueId(&id), "id");
  check_nccl(ncclCommInitRank(&comm, 1, id, 0), "init");
  // in-place sum-allreduce over 1 rank: must read the kernel's 21.0s
  check_nccl(ncclAllReduce(buf, buf, N, ncclFloat, ncclSum, comm, stream),
             "allreduce");

  // runtime A again: HIP kernel doubles it (21 -> 42) on the same stream
  hpk::launch_acc_f32(buf, buf, N, stream);
  hpk::check_hip(hipStreamSynchronize(stream), "sync");

  // verify through the HIP runtime
  std::vector<float> h(N);
  hpk::check_hip(
      hipMemcpy(h.data(), buf, N * sizeof(float), hipMemcpyDeviceToHost),
      "d2h");
  for (size_t i = 0; i < N; ++i) {
    if (h[i] != 42.0f) {
      std::fprintf(stderr, "FAILED at %zu: %f != 42\n", i, h[i]);
      return 1;
    }
  }
  // exact device-side checksum as the second, independent readback path
  double sum = hpk::reduce_sum_f32(buf, N, stream);
  if (sum != 42.0 * N) {
    std::fprintf(stderr, "FAILED checksum: %f\n", sum);
    return 1;
  }

  ncclCommDestroy(comm);
  (void)hipFree(buf);
  (void)hipStreamDestroy(stream);
  std::printf("PASSED: HIP kernel -> RCCL allreduce -> HIP kernel shared one "
              "pointer and one externally-created stream (N=%zu)\n", N);
  return 0;
}
