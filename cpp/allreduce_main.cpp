// allreduce_main.cpp — hpk_allreduce: device-buffer all-reduce miniapp.
//
// MI355X-native re-design of the reference GPU-aware-MPI ring-allreduce
// miniapps (reference aurora.mpich.miniapps/src/allreduce/mpi-sycl/
// allreduce-mpi-sycl.cpp:88-215 and the two OMP variants). The reference's
// three comparisons (hand ring over blocking MPI_Send/Recv vs native
// MPI_Allreduce) become, on MI355X:
//   --algo ring     hand ring over RCCL ncclSend/ncclRecv pt2pt + the
//                   hand-written HIP Accumulate kernel (K3) between steps —
//                   the reference's SendRecvRing+Accumulate pattern
//                   (allreduce-mpi-sycl.cpp:44-59,173-182)
//   --algo pipeline chunked ring: send/recv and Accumulate overlapped on two
//                   hipStreams (the tuned variant the reference leaves as an
//                   exercise — SURVEY.md §7.4)
//   --algo rccl     native ncclAllReduce over xGMI (the reference's
//                   MPI_Allreduce path, allreduce-mpi-sycl.cpp:62-67)
//
// Launcher model: no MPI exists on this stack; the binary self-launches
// one process per GPU (fork), sharing the ncclUniqueId through pre-fork
// memory — the MI355X-native "mpirun -np N" for a single node.
//
// Verification is the reference's analytic oracle: VA=rank everywhere, so
// after all-reduce every element must equal size*(size-1)/2
// (allreduce-mpi-sycl.cpp:192-204) — checked with an exact device-side
// double reduction instead of an O(N) host scan.
//
// CLI (reference getopt surface, allreduce-mpi-sycl.cpp:106-131, extended):
//   -p <P>     2^P elements (default 25 -> 128 MiB float)
//   -D|-H|-S   allocator: hipMalloc | hipHostMalloc | hipMallocManaged
//   -a         native ncclAllReduce (same as --algo rccl)
//   -n <N>     number of ranks (default: visible device count)
//   -i <iters> timed iterations (default 10, min-time reported)
//   -c <K>     pipeline chunk count (default 8; pipeline algo only)
//   -t <T>     dtype: float (default) | int — the reference's two
//              -DAPP_DATA_TYPE instantiations as a runtime switch
//   --algo ring|pipeline|rccl

#include "../hpc_patterns_amd/native/include/hpk.h"
#include "../hpc_patterns_amd/native/include/rccl_datatype.h"
#include "launch_util.h"
#include "miniapp_util.h"

#include <rccl/rccl.h>
#include <sys/mman.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

using hpk_app::alloc_buf;
using hpk_app::now_s;
using hpk_launch::check_nccl;

struct Config {
  int p = 25;
  char alloc = 'D';
  std::string algo = "ring";
  std::string dtype = "float"; // float | int (reference -DAPP_DATA_TYPE pair)
  std::string transport = "nccl"; // nccl | ipc (ring exchange transport)
  int nranks = -1;
  int iters = 10;
  int chunks = 8;
};

// Ring exchange transports. The ring ALGORITHM below is transport-agnostic;
// these provide one step's neighbour exchange:
//   NcclRing — grouped ncclSend/ncclRecv, fully async on `stream` (the RCCL
//              pt2pt path; no odd/even ordering dance — that deadlock-
//              avoidance trick is an MPI-blocking-call artifact, reference
//              allreduce-mpi-sycl.cpp:50-58)
//   IpcRing  — one-sided put into the RIGHT neighbour's recv buffer through
//              a hipIpc mapping + shared-memory fence. RCCL refuses two
//              ranks on one device, so this is what lets the ring run
//              oversubscribed (size>=2 on a 1-GPU box) under ctest, the way
//              the reference's `mpirun -np 4` oversubscribed tiles
//              (CMakeLists.txt:45-50).
template <typename T>
struct NcclRing {
  ncclComm_t comm;
  int right, left;
  void sendrecv(T* send, T* recv, size_t n, hipStream_t stream) {
    const ncclDataType_t dt = hpk::get_rccl_datatype<T>();
    check_nccl(ncclGroupStart(), "group start");
    check_nccl(ncclSend(send, n, dt, right, comm, stream), "send");
    check_nccl(ncclRecv(recv, n, dt, left, comm, stream), "recv");
    check_nccl(ncclGroupEnd(), "group end");
  }
};

constexpr int kMaxArRanks = 16;

struct ArIpcShared {
  hpk_launch::SharedBarrier bar;
  // each rank exports BOTH ring buffers (va/vb swap identity every step,
  // all ranks in lockstep, so buffer index i on my side pairs with buffer
  // index i on every neighbour)
  uint8_t handle[kMaxArRanks][2][sizeof(hipIpcMemHandle_t)];
  double dt[kMaxArRanks]; // wall-time MAX-reduction without a communicator
};

template <typename T>
struct IpcRing {
  T* alloc0 = nullptr; // my two exchange buffers (allocation identity)
  T* alloc1 = nullptr;
  void* right_buf[2] = {nullptr, nullptr}; // right neighbour's, IPC-mapped
  bool same_dev = false;
  ArIpcShared* sh = nullptr;
  bool ok = true;

  void setup(int rank, int size, int ndev, ArIpcShared* shared, T* a0, T* a1) {
    sh = shared;
    alloc0 = a0;
    alloc1 = a1;
    int right = (rank + 1) % size;
    same_dev = (rank % ndev) == (right % ndev);
    auto h0 = hpk::ipc_get_handle(a0);
    auto h1 = hpk::ipc_get_handle(a1);
    std::memcpy(sh->handle[rank][0], h0.data(), h0.size());
    std::memcpy(sh->handle[rank][1], h1.data(), h1.size());
    ok = sh->bar.wait();
    if (!ok) return;
    for (int i = 0; i < 2; ++i) {
      std::vector<uint8_t> hv(sh->handle[right][i],
                              sh->handle[right][i] + sizeof(hipIpcMemHandle_t));
      right_buf[i] = hpk::ipc_open_handle(hv);
    }
  }

  void sendrecv(T* send, T* recv, size_t n, hipStream_t stream) {
    if (!ok) return; // a fence already timed out (lost sibling) — stop
                     // issuing puts; the worker reports the failure
    // my recv allocation index == right's recv allocation index (lockstep)
    int idx = (recv == alloc1) ? 1 : 0;
    void* dst = right_buf[idx];
    // same-device put: hand-written copy kernel (release-semantics
    // completion, robust against the same-device SDMA visibility artifact);
    // cross-device: SDMA over xGMI
    if (same_dev)
      hpk::launch_copy_kernel(dst, send, n * sizeof(T), stream);
    else
      hpk::check_hip(hipMemcpyAsync(dst, send, n * sizeof(T),
                                    hipMemcpyDeviceToDevice, stream),
                     "ipc ring put");
    hpk::check_hip(hipStreamSynchronize(stream), "ipc ring sync");
    ok = ok && sh->bar.wait(); // fence: every put landed -> recv is valid
  }

  void teardown() {
    for (int i = 0; i < 2; ++i)
      if (right_buf[i]) hpk::ipc_close_handle(right_buf[i]);
  }
};

// Hand ring all-reduce, the reference SendRecvRing pattern: (size-1) steps of
// [exchange full buffer with ring neighbours] + [VC += recv]. Buffers VA
// (send payload, swapped with VB each step), VB (recv), VC (accumulator).
template <typename T, typename Ring>
double run_ring(Ring& ring, hipStream_t stream, T* va, T* vb,
                T* vc, size_t n, int size, int* steps_out = nullptr) {
  double t0 = now_s();
  int steps = 0;
  hpk::launch_acc(vc, va, n, stream); // VC += own VA (VC starts at 0)
  for (int step = 0; step < size - 1; ++step) {
    ring.sendrecv(va, vb, n, stream);
    hpk::launch_acc(vc, vb, n, stream);
    std::swap(va, vb);
    ++steps;
  }
  hpk::check_hip(hipStreamSynchronize(stream), "ring sync");
  if (steps_out) *steps_out = steps;
  return now_s() - t0;
}

// Chunked pipelined ring: split the buffer into K chunks; while chunk c is
// being accumulated on the compute stream, chunk c+1 is already in flight on
// the comm stream. Overlaps xGMI transfer with the HIP Accumulate kernel.
template <typename T>
double run_pipeline(ncclComm_t comm, hipStream_t comm_stream,
                    hipStream_t comp_stream, T* va, T* vb, T* vc,
                    size_t n, int rank, int size, int chunks) {
  const ncclDataType_t dt = hpk::get_rccl_datatype<T>();
  int right = (rank + 1) % size;
  int left = (rank - 1 + size) % size;
  size_t chunk = (n + chunks - 1) / chunks;
  std::vector<hipEvent_t> done((size_t)chunks);
  for (auto& e : done)
    hpk::check_hip(hipEventCreateWithFlags(&e, hipEventDisableTiming), "ev");

  double t0 = now_s();
  hpk::launch_acc(vc, va, n, comp_stream);
  for (int step = 0; step < size - 1; ++step) {
    // launch all chunk exchanges; accumulate each chunk as soon as it lands
    for (int c = 0; c < chunks; ++c) {
      size_t off = (size_t)c * chunk;
      if (off >= n) break;
      size_t len = std::min(chunk, n - off);
      check_nccl(ncclGroupStart(), "group start");
      check_nccl(ncclSend(va + off, len, dt, right, comm, comm_stream),
                 "send");
      check_nccl(ncclRecv(vb + off, len, dt, left, comm, comm_stream),
                 "recv");
      check_nccl(ncclGroupEnd(), "group end");
      hpk::check_hip(hipEventRecord(done[c], comm_stream), "record");
      hpk::check_hip(hipStreamWaitEvent(comp_stream, done[c], 0), "wait");
      hpk::launch_acc(vc + off, vb + off, len, comp_stream);
    }
    // comm of next step must not overwrite vb before accumulate read it:
    // swap uses distinct buffers, but step s+1 recv into (old) va after
    // compute consumed it -> order via event from comp_stream.
    hipEvent_t barrier_ev = done[0];
    hpk::check_hip(hipEventRecord(barrier_ev, comp_stream), "step ev");
    hpk::check_hip(hipStreamWaitEvent(comm_stream, barrier_ev, 0), "step wait");
    std::swap(va, vb);
  }
  hpk::check_hip(hipStreamSynchronize(comp_stream), "pipeline sync");
  hpk::check_hip(hipStreamSynchronize(comm_stream), "pipeline sync comm");
  double elapsed = now_s() - t0;
  for (auto& e : done) (void)hipEventDestroy(e);
  return elapsed;
}

template <typename T>
int worker(int rank, int size, int ndev, hpk_launch::SharedBootstrap* sh,
           ArIpcShared* ipc_sh, const Config& cfg) {
  const bool use_ipc = (cfg.transport == "ipc");
  int dev = rank % ndev;
  hpk::check_hip(hipSetDevice(dev), "hipSetDevice");
  ncclComm_t comm = nullptr;
  if (!use_ipc) {
    ncclUniqueId id;
    hpk_launch::bootstrap_id(sh, rank, &id);
    check_nccl(ncclCommInitRank(&comm, size, id, rank), "ncclCommInitRank");
  }

  size_t n = 1ull << cfg.p;
  size_t bytes = n * sizeof(T);
  T* va = (T*)alloc_buf(cfg.alloc, bytes);
  T* vb = (T*)alloc_buf(cfg.alloc, bytes);
  T* vc = (T*)alloc_buf(cfg.alloc, bytes);

  hipStream_t stream, comp_stream;
  hpk::check_hip(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "s");
  hpk::check_hip(hipStreamCreateWithFlags(&comp_stream, hipStreamNonBlocking),
                 "s2");

  int right = (rank + 1) % size;
  int left = (rank - 1 + size) % size;
  NcclRing<T> nring{comm, right, left};
  IpcRing<T> iring;
  if (use_ipc) {
    iring.setup(rank, size, ndev, ipc_sh, va, vb);
    if (!iring.ok) return 3;
  }

  double best = 1e30;
  int ring_steps = 0;
  for (int it = 0; it < cfg.iters; ++it) {
    // (re)initialize: VA = rank, VB = -1, VC = 0 (reference Initialize)
    hpk::launch_fill(va, (T)rank, n, stream);
    hpk::launch_fill(vb, (T)-1, n, stream);
    hpk::launch_fill(vc, (T)0, n, stream);
    hpk::check_hip(hipStreamSynchronize(stream), "init sync");
    // ipc transport: nobody may put into my freshly-filled recv buffer
    // before the fill above completed everywhere
    if (use_ipc && !ipc_sh->bar.wait()) return 3;

    double dt;
    if (cfg.algo == "rccl") {
      double t0 = now_s();
      check_nccl(ncclAllReduce(va, vc, n, hpk::get_rccl_datatype<T>(),
                               ncclSum, comm, stream),
                 "ncclAllReduce");
      hpk::check_hip(hipStreamSynchronize(stream), "allreduce sync");
      dt = now_s() - t0;
    } else if (cfg.algo == "pipeline") {
      dt = run_pipeline(comm, stream, comp_stream, va, vb, vc, n, rank, size,
                        cfg.chunks);
    } else if (use_ipc) {
      dt = run_ring(iring, stream, va, vb, vc, n, size, &ring_steps);
      if (!iring.ok) return 3;
    } else {
      dt = run_ring(nring, stream, va, vb, vc, n, size, &ring_steps);
    }
    best = std::min(best, dt);
  }

  // max over ranks (reference MPI_Allreduce MAX of wall time)
  double max_time = best;
  if (use_ipc) {
    ipc_sh->dt[rank] = best;
    if (!ipc_sh->bar.wait()) return 3;
    for (int r = 0; r < size; ++r) max_time = std::max(max_time, ipc_sh->dt[r]);
  } else {
    double* d_time = nullptr;
    hpk::check_hip(hipMalloc(&d_time, sizeof(double)), "time buf");
    hpk::check_hip(hipMemcpy(d_time, &best, sizeof(double),
                             hipMemcpyHostToDevice), "time h2d");
    check_nccl(ncclAllReduce(d_time, d_time, 1, ncclDouble, ncclMax, comm,
                             stream), "time max");
    hpk::check_hip(hipStreamSynchronize(stream), "time sync");
    hpk::check_hip(hipMemcpy(&max_time, d_time, sizeof(double),
                             hipMemcpyDeviceToHost), "time d2h");
    (void)hipFree(d_time);
  }

  bool pass = hpk_app::allreduce_verdict(hpk::reduce_sum(vc, n, stream), n,
                                         size, rank);

  if (rank == 0) {
    double busbw = hpk_app::allreduce_busbw(bytes, size, max_time);
    std::printf("# algo=%s transport=%s dtype=%s ranks=%d elems=2^%d alloc=%c "
                "steps=%d time=%.6fs busbw=%.2f GB/s\n",
                cfg.algo.c_str(), cfg.transport.c_str(), cfg.dtype.c_str(),
                size, cfg.p, cfg.alloc, ring_steps, max_time, busbw);
    if (sh) sh->result = max_time;
  }

  if (use_ipc) iring.teardown();
  if (comm) ncclCommDestroy(comm);
  return pass ? 0 : 2;
}

} // namespace

int main(int argc, char* argv[]) {
  Config cfg;
  for (int i = 1; i < argc; ++i) {
    std::string s = argv[i];
    auto next = [&] { return hpk_app::next_arg(i, argc, argv); };
    if (s == "--probe-ndev") {  // launch_util.h re-exec probe
      std::printf("%d\n", hpk::device_count());
      return 0;
    } else if (s == "-p") cfg.p = std::atoi(next());
    else if (s == "-D") cfg.alloc = 'D';
    else if (s == "-H") cfg.alloc = 'H';
    else if (s == "-S") cfg.alloc = 'S';
    else if (s == "-a") cfg.algo = "rccl";
    else if (s == "-n") cfg.nranks = std::atoi(next());
    else if (s == "-i") cfg.iters = std::atoi(next());
    else if (s == "-c") cfg.chunks = std::atoi(next());
    else if (s == "--algo") cfg.algo = next();
    else if (s == "-t" || s == "--dtype") cfg.dtype = next();
    else if (s == "--transport") cfg.transport = next();
    else {
      std::printf(
          "Usage: %s [-p P] [-D|-H|-S] [-a] [-n ranks] [-i iters] [-c chunks] "
          "[--algo ring|pipeline|rccl] [--transport nccl|ipc]\n", argv[0]);
      return s == "-h" || s == "--help" ? 0 : 1;
    }
  }
  if (cfg.algo != "ring" && cfg.algo != "pipeline" && cfg.algo != "rccl") {
    std::fprintf(stderr, "unknown algo '%s'\n", cfg.algo.c_str());
    return 1;
  }
  if (cfg.transport != "nccl" && cfg.transport != "ipc") {
    std::fprintf(stderr, "unknown transport '%s'\n", cfg.transport.c_str());
    return 1;
  }
  if (cfg.transport == "ipc") {
    if (cfg.algo != "ring") {
      std::fprintf(stderr, "--transport ipc supports --algo ring only "
                   "(the pipeline/collective paths are RCCL)\n");
      return 1;
    }
    if (cfg.alloc != 'D') {
      std::fprintf(stderr, "--transport ipc requires -D (hipIpc shares "
                   "hipMalloc memory only)\n");
      return 1;
    }
  }

  // Parent stays HIP-free (launch_util.h invariant): probe device count by
  // re-exec, bootstrap the ncclUniqueId inside rank 0 after fork.
  int ndev = hpk_launch::probe_device_count(argv[0]);
  if (ndev == 0) {
    std::fprintf(stderr, "no HIP devices\n");
    return 1;
  }
  int size = cfg.nranks > 0 ? cfg.nranks : ndev;
  if (cfg.transport == "ipc") {
    // ipc transport oversubscribes freely: many ranks per GPU is exactly
    // its purpose (multi-rank ring exchange under ctest on a 1-GPU lease)
    if (size < 2) size = 2;
    if (size > kMaxArRanks) size = kMaxArRanks;
  } else if (size > ndev) {
    // RCCL refuses two ranks on one device; clamp with a notice and point
    // at the transport that CAN oversubscribe.
    std::fprintf(stderr, "# clamping ranks %d -> %d (one rank per GPU; "
                 "use --transport ipc to oversubscribe)\n", size, ndev);
    size = ndev;
  }

  hpk_launch::SharedBootstrap* sh = hpk_launch::map_shared();
  ArIpcShared* ipc_sh = nullptr;
  if (cfg.transport == "ipc") {
    ipc_sh = hpk_launch::map_shared_struct<ArIpcShared>();
    if (!ipc_sh) {
      std::fprintf(stderr, "shared map failed\n");
      return 1;
    }
    ipc_sh->bar.size = size;
  }
  return hpk_launch::fork_workers(size, [&](int rank) {
    return cfg.dtype == "int"
               ? worker<int>(rank, size, ndev, sh, ipc_sh, cfg)
               : worker<float>(rank, size, ndev, sh, ipc_sh, cfg);
  });
}
