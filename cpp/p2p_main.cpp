// p2p_main.cpp — hpk_p2p: GPU<->GPU bandwidth benchmark over xGMI.
//
// MI355X-native re-design of the reference pairwise P2P bench
// (reference p2p/peer2pear.cpp:104-156): ranks are paired even<->odd, each
// pair exchanges a 47,185,920-float (~188.7 MB) device buffer, phase 1
// unidirectional, phase 2 bidirectional, aggregate bandwidth = payload bytes
// x pairs / min-time over 10 iterations, with a shuffled-iota checksum.
//
// Three transfer engines replace the reference's two MPI paths:
//   --engine peer   hipMemcpyPeerAsync over xGMI, one process drives all
//                   GPUs on per-pair hipStreams (the direct SDMA path; the
//                   reference's MPI_Isend/Irecv GPU-IPC fast path collapses
//                   to exactly this on a single node)
//   --engine ipc    two processes, hipIpc handle exchange over a socketpair,
//                   one-sided put into the peer's buffer (the reference's
//                   MPI_Win/MPI_Put RMA engine, peer2pear.cpp:68-102)
//   --engine rccl   one process per GPU, ncclSend/ncclRecv pt2pt (the
//                   portable two-sided engine)
//
// Verification: payload is a host-shuffled iota (reference
// peer2pear.cpp:8-17); the received buffer's exact double sum must equal
// sum_i float(i) — order-independent and O(N) on device, replacing the
// reference's host sort+sum.

#include "../hpc_patterns_amd/native/include/hpk.h"
#include "launch_util.h"
#include "miniapp_util.h"

#include <rccl/rccl.h>
#include <sys/socket.h>
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

constexpr size_t kDefaultN = 47185920; // reference peer2pear.cpp:115
constexpr int kIters = 10;

using hpk_app::now_s;
using hpk_launch::check_nccl;

// Host-shuffled iota payload + its exact double checksum.
double fill_payload(float* dptr, size_t n, unsigned seed) {
  hpk_app::Payload p = hpk_app::shuffled_iota(n, seed);
  hpk::check_hip(hipMemcpy(dptr, p.v.data(), n * sizeof(float),
                           hipMemcpyHostToDevice),
                 "payload H2D");
  return p.sum;
}

void verify(float* dptr, size_t n, double expected, const char* what) {
  double got = hpk::reduce_sum_f32(dptr, n, nullptr);
  if (got != expected) {
    // Second opinion before declaring failure: full device sync + host-side
    // sum distinguishes "buffer really wrong" from "device reduction raced
    // something" (an intermittent ~half-sum was observed on some boxes —
    // see profiles/README.md).
    hpk::check_hip(hipDeviceSynchronize(), "verify sync");
    std::vector<float> h(n);
    hpk::check_hip(hipMemcpy(h.data(), dptr, n * sizeof(float),
                             hipMemcpyDeviceToHost),
                   "verify D2H");
    double host_sum = 0.0;
    for (size_t i = 0; i < n; ++i) host_sum += (double)h[i];
    double got2 = hpk::reduce_sum_f32(dptr, n, nullptr);
    if (host_sum == expected) {
      // The transferred DATA is provably correct (exact host sum); the
      // first device reduction observed a partially-visible buffer. On
      // some ROCm 7.2 pods an SDMA copy's completion signal fires before
      // its writes are visible to a subsequently launched kernel — even
      // across hipDeviceSynchronize (profiles/p2p_fail_r38.log). Warn
      // loudly, do not fail the transfer.
      std::fprintf(stderr,
                   "WARNING (%s): device reduction saw a partially-visible "
                   "buffer (%.1f, after-sync %.1f); host sum exact %.1f — "
                   "SDMA completion/visibility artifact, transfer correct\n",
                   what, got, got2, expected);
      return;
    }
    std::fprintf(stderr,
                 "CHECKSUM FAILURE (%s): device %.1f, device-after-sync %.1f, "
                 "host %.1f, expected %.1f\n",
                 what, got, got2, host_sum, expected);
    std::exit(2);
  }
}

// ---------------------------------------------------------------------------
// Engine 1: single-process hipMemcpyPeerAsync over xGMI.
// ---------------------------------------------------------------------------
int run_peer(size_t n, bool bidir_phase) {
  int ndev = hpk::device_count();
  if (ndev < 2) {
    std::printf("# peer engine needs >=2 GPUs (have %d) — falling back to "
                "same-device D2D plumbing check\n", ndev);
  }
  int npairs = std::max(ndev / 2, 1);
  size_t bytes = n * sizeof(float);

  struct Pair {
    int a, b;
    float *src_a, *dst_b, *src_b, *dst_a;
    hipStream_t sa, sb;
    double sum_a, sum_b;
  };
  std::vector<Pair> pairs((size_t)npairs);
  for (int p = 0; p < npairs; ++p) {
    Pair& pr = pairs[p];
    pr.a = (2 * p) % std::max(ndev, 1);
    pr.b = ndev >= 2 ? 2 * p + 1 : pr.a;
    hpk::check_hip(hipSetDevice(pr.a), "set a");
    if (pr.a != pr.b) hpk::enable_peer_access(pr.b);
    hpk::check_hip(hipMalloc(&pr.src_a, bytes), "src_a");
    hpk::check_hip(hipMalloc(&pr.dst_a, bytes), "dst_a");
    hpk::check_hip(hipStreamCreateWithFlags(&pr.sa, hipStreamNonBlocking), "sa");
    pr.sum_a = fill_payload(pr.src_a, n, 2 * p);
    hpk::check_hip(hipSetDevice(pr.b), "set b");
    if (pr.a != pr.b) hpk::enable_peer_access(pr.a);
    hpk::check_hip(hipMalloc(&pr.src_b, bytes), "src_b");
    hpk::check_hip(hipMalloc(&pr.dst_b, bytes), "dst_b");
    hpk::check_hip(hipStreamCreateWithFlags(&pr.sb, hipStreamNonBlocking), "sb");
    pr.sum_b = fill_payload(pr.src_b, n, 2 * p + 1);
  }

  for (int phase = 0; phase < (bidir_phase ? 2 : 1); ++phase) {
    bool bidir = (phase == 1);
    double best = 1e30;
    for (int it = 0; it < kIters; ++it) {
      double t0 = now_s();
      for (auto& pr : pairs) {
        // same-device fallback uses the hand-written copy kernel:
        // hipMemcpyPeerAsync with srcDevice==dstDevice returns success but
        // moves nothing, and the runtime's D2D SDMA path has the
        // completion-visibility artifact above (both observed on
        // ROCm 7.2/gfx950). A kernel's completion signal carries release
        // semantics — deterministic, and faster (3 TB/s).
        if (pr.a == pr.b) {
          hpk::launch_copy_kernel(pr.dst_b, pr.src_a, bytes, pr.sa);
          if (bidir) hpk::launch_copy_kernel(pr.dst_a, pr.src_b, bytes, pr.sb);
          continue;
        }
        hpk::memcpy_peer_async(pr.dst_b, pr.b, pr.src_a, pr.a, bytes, pr.sa);
        if (bidir)
          hpk::memcpy_peer_async(pr.dst_a, pr.a, pr.src_b, pr.b, bytes, pr.sb);
      }
      for (auto& pr : pairs) {
        hpk::check_hip(hipStreamSynchronize(pr.sa), "sync a");
        if (bidir) hpk::check_hip(hipStreamSynchronize(pr.sb), "sync b");
      }
      best = std::min(best, now_s() - t0);
    }
    for (auto& pr : pairs) {
      hpk::check_hip(hipSetDevice(pr.b), "set b");
      verify(pr.dst_b, n, pr.sum_a, "peer a->b");
      if (bidir) {
        hpk::check_hip(hipSetDevice(pr.a), "set a");
        verify(pr.dst_a, n, pr.sum_b, "peer b->a");
      }
    }
    double gb = (double)bytes * npairs * (bidir ? 2 : 1) / 1e9;
    std::printf("peer %s Bandwidth: %.2f GB/s (pairs=%d, %.1f MB each, "
                "min over %d iters)\n",
                bidir ? "Bidirectional" : "Unidirectional", gb / best, npairs,
                bytes / 1e6, kIters);
  }
  return 0;
}

// ---------------------------------------------------------------------------
// Engine 2: HIP-IPC one-sided RMA — full reference protocol parity
// (reference p2p/peer2pear.cpp:68-102,119-122,141-155): every rank exposes a
// window (hipIpcMemHandle = the MPI_Win_create), all N/2 pairs run
// concurrently, a shared-memory barrier is the fence epoch, phase 1 is a
// unidirectional put (even rank -> odd peer's window), phase 2 bidirectional
// (both directions), aggregate GB/s = bytes x pairs x dirs / min global
// interval over 10 iterations, output isomorphic to the two-sided engines.
// On a 1-GPU box the ranks oversubscribe the device (cross-PROCESS one-sided
// puts still exercise the whole protocol — the reference oversubscribed
// tiles the same way, CMakeLists.txt:45-50).
// ---------------------------------------------------------------------------
constexpr int kMaxIpcRanks = 16;

struct IpcShared {
  hpk_launch::SharedBarrier bar;
  uint8_t handle[kMaxIpcRanks][sizeof(hipIpcMemHandle_t)];
  double src_sum[kMaxIpcRanks]; // expected checksum of each rank's payload
  double dt[kMaxIpcRanks];      // per-rank interval for the clock union
};

int ipc_rma_worker(int rank, int size, int ndev, IpcShared* sh, size_t n) {
  int dev = rank % std::max(ndev, 1);
  hpk::check_hip(hipSetDevice(dev), "set dev");
  size_t bytes = n * sizeof(float);

  // window (exposed) + source payload (origin side)
  float *win = nullptr, *src = nullptr;
  hpk::check_hip(hipMalloc(&win, bytes), "win");
  hpk::check_hip(hipMalloc(&src, bytes), "src");
  auto hv = hpk::ipc_get_handle(win);
  std::memcpy(sh->handle[rank], hv.data(), hv.size());
  sh->src_sum[rank] = fill_payload(src, n, (unsigned)rank);
  if (!sh->bar.wait()) return 3; // handle-exchange epoch

  int peer = (rank % 2 == 0) ? rank + 1 : rank - 1;
  bool paired = peer < size;
  float* peer_win = nullptr;
  int peer_dev = paired ? peer % std::max(ndev, 1) : dev;
  if (paired) {
    std::vector<uint8_t> ph(sh->handle[peer],
                            sh->handle[peer] + sizeof(hipIpcMemHandle_t));
    peer_win = (float*)hpk::ipc_open_handle(ph);
  }
  hipStream_t s;
  hpk::check_hip(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "s");

  int rc = 0;
  for (int phase = 0; phase < 2; ++phase) {
    bool bidir = (phase == 1);
    bool origin = paired && ((rank % 2 == 0) || bidir);
    double best = 1e30;
    for (int it = 0; it < kIters; ++it) {
      if (!sh->bar.wait()) return 3; // fence: epoch open
      double t0 = now_s();
      if (origin) {
        // one-sided put into the peer process's window. Cross-device: SDMA
        // over xGMI (hipMemcpyAsync on the IPC mapping). Same device
        // (oversubscribed 1-GPU box): the hand-written copy kernel — its
        // completion signal carries release semantics, dodging the SDMA
        // same-device completion-visibility artifact (profiles/README.md).
        if (peer_dev == dev)
          hpk::launch_copy_kernel(peer_win, src, bytes, s);
        else
          hpk::check_hip(hipMemcpyAsync(peer_win, src, bytes,
                                        hipMemcpyDeviceToDevice, s),
                         "ipc put");
        hpk::check_hip(hipStreamSynchronize(s), "put sync");
      }
      sh->dt[rank] = now_s() - t0;
      if (!sh->bar.wait()) return 3; // fence: epoch close (puts visible)
      // clock union: global interval = MAX over ranks (all started together
      // at the opening fence — reference MPI_Reduce MIN/MAX, :49-51)
      double g_dt = 0.0;
      for (int r = 0; r < size; ++r) g_dt = std::max(g_dt, sh->dt[r]);
      best = std::min(best, g_dt);
      if (!sh->bar.wait()) return 3; // dt array consumed before next write
    }
    // verify: my window must hold my pair-peer's payload (odd ranks in the
    // uni phase, every paired rank in the bidi phase)
    bool target = paired && ((rank % 2 == 1) || bidir);
    if (target) verify(win, n, sh->src_sum[peer], "ipc put");
    if (rank == 0) {
      int npairs = size / 2;
      double gb = (double)bytes * npairs * (bidir ? 2 : 1) / 1e9;
      std::printf("ipc %s Bandwidth: %.2f GB/s (pairs=%d, %.1f MB each, "
                  "min over %d iters, one-sided put, fence epochs)\n",
                  bidir ? "Bidirectional" : "Unidirectional", gb / best,
                  npairs, bytes / 1e6, kIters);
    }
    if (!sh->bar.wait()) return 3; // phase boundary
  }
  if (paired) hpk::ipc_close_handle(peer_win);
  (void)hipFree(win);
  (void)hipFree(src);
  return rc;
}

int run_ipc(const char* self, size_t n, int nranks) {
  // parent stays HIP-free (launch_util.h invariant); fork BEFORE any HIP
  // call — an initialized HIP runtime does not survive fork().
  int ndev = hpk_launch::probe_device_count(self);
  if (ndev == 0) {
    std::fprintf(stderr, "no HIP devices\n");
    return 1;
  }
  // default: one rank per GPU; 1-GPU boxes oversubscribe to 2 ranks so the
  // cross-process protocol still runs end to end
  int size = nranks > 0 ? nranks : (ndev >= 2 ? ndev : 2);
  size -= size % 2; // pairs
  size = std::max(2, std::min(size, kMaxIpcRanks));

  IpcShared* sh = hpk_launch::map_shared_struct<IpcShared>();
  if (!sh) {
    std::fprintf(stderr, "shared map failed\n");
    return 1;
  }
  sh->bar.size = size;
  std::printf("# ipc engine: %d ranks on %d GPU(s) (%s)\n", size, ndev,
              size > ndev ? "oversubscribed" : "one rank per GPU");
  return hpk_launch::fork_workers(
      size, [&](int rank) { return ipc_rma_worker(rank, size, ndev, sh, n); });
}

// ---------------------------------------------------------------------------
// Engine 3: RCCL pt2pt, one process per GPU.
// ---------------------------------------------------------------------------
int rccl_worker(int rank, int size, hpk_launch::SharedBootstrap* sh, size_t n) {
  hpk::check_hip(hipSetDevice(rank), "set dev");
  ncclUniqueId id;
  hpk_launch::bootstrap_id(sh, rank, &id);
  ncclComm_t comm;
  check_nccl(ncclCommInitRank(&comm, size, id, rank), "init");
  size_t bytes = n * sizeof(float);
  float *src = nullptr, *dst = nullptr;
  hpk::check_hip(hipMalloc(&src, bytes), "src");
  hpk::check_hip(hipMalloc(&dst, bytes), "dst");
  double my_sum = fill_payload(src, n, (unsigned)rank);
  int peer = (rank % 2 == 0) ? rank + 1 : rank - 1;
  bool paired = peer < size;
  hipStream_t s;
  hpk::check_hip(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "s");

  // exchange expected checksums out-of-band (via RCCL itself, double buffer)
  double peer_sum = 0.0;
  if (paired) {
    double* d_sum = nullptr;
    hpk::check_hip(hipMalloc(&d_sum, 2 * sizeof(double)), "sum buf");
    hpk::check_hip(hipMemcpy(d_sum, &my_sum, sizeof(double),
                             hipMemcpyHostToDevice), "sum h2d");
    check_nccl(ncclGroupStart(), "gs");
    check_nccl(ncclSend(d_sum, 1, ncclDouble, peer, comm, s), "send sum");
    check_nccl(ncclRecv(d_sum + 1, 1, ncclDouble, peer, comm, s), "recv sum");
    check_nccl(ncclGroupEnd(), "ge");
    hpk::check_hip(hipStreamSynchronize(s), "sum sync");
    hpk::check_hip(hipMemcpy(&peer_sum, d_sum + 1, sizeof(double),
                             hipMemcpyDeviceToHost), "sum d2h");
    (void)hipFree(d_sum);
  }

  for (int phase = 0; phase < 2; ++phase) {
    bool bidir = (phase == 1);
    bool sender = (rank % 2 == 0) || bidir;
    bool receiver = (rank % 2 == 1) || bidir;
    double best = 1e30;
    for (int it = 0; it < kIters; ++it) {
      double* d_t = nullptr; // barrier via tiny allreduce
      hpk::check_hip(hipMalloc(&d_t, sizeof(double)), "bar");
      check_nccl(ncclAllReduce(d_t, d_t, 1, ncclDouble, ncclMax, comm, s), "bar");
      hpk::check_hip(hipStreamSynchronize(s), "bar sync");
      double t0 = now_s();
      if (paired) {
        check_nccl(ncclGroupStart(), "gs");
        if (sender) check_nccl(ncclSend(src, n, ncclFloat, peer, comm, s), "send");
        if (receiver) check_nccl(ncclRecv(dst, n, ncclFloat, peer, comm, s), "recv");
        check_nccl(ncclGroupEnd(), "ge");
        hpk::check_hip(hipStreamSynchronize(s), "sync");
      }
      double l_dt = now_s() - t0;
      // global interval: max over ranks
      hpk::check_hip(hipMemcpy(d_t, &l_dt, sizeof(double),
                               hipMemcpyHostToDevice), "t h2d");
      check_nccl(ncclAllReduce(d_t, d_t, 1, ncclDouble, ncclMax, comm, s), "t max");
      hpk::check_hip(hipStreamSynchronize(s), "t sync");
      double g_dt;
      hpk::check_hip(hipMemcpy(&g_dt, d_t, sizeof(double),
                               hipMemcpyDeviceToHost), "t d2h");
      (void)hipFree(d_t);
      best = std::min(best, g_dt);
    }
    if (paired && receiver) verify(dst, n, peer_sum, "rccl pt2pt");
    if (rank == 0) {
      int npairs = size / 2;
      if (npairs >= 1) {
        double gb = (double)bytes * npairs * (bidir ? 2 : 1) / 1e9;
        std::printf("rccl %s Bandwidth: %.2f GB/s (pairs=%d, %.1f MB each)\n",
                    bidir ? "Bidirectional" : "Unidirectional", gb / best,
                    npairs, bytes / 1e6);
      } else {
        std::printf("# rccl 1-rank plumbing check ok (%s phase, no pairs "
                    "to measure)\n", bidir ? "bidirectional" : "unidirectional");
      }
    }
  }
  ncclCommDestroy(comm);
  return 0;
}

int run_rccl(const char* self, size_t n) {
  // parent stays HIP-free (launch_util.h invariant)
  int ndev = hpk_launch::probe_device_count(self);
  hpk_launch::SharedBootstrap* sh = hpk_launch::map_shared();
  if (ndev < 2) {
    std::printf("# rccl engine needs >=2 GPUs (have %d) — running 1-rank "
                "plumbing check\n", ndev);
    return rccl_worker(0, 1, sh, n);
  }
  int size = ndev - (ndev % 2); // even
  return hpk_launch::fork_workers(
      size, [&](int rank) { return rccl_worker(rank, size, sh, n); });
}

} // namespace

int main(int argc, char* argv[]) {
  std::string engine = "peer";
  size_t n = kDefaultN;
  int nranks = -1;
  for (int i = 1; i < argc; ++i) {
    std::string s = argv[i];
    auto next = [&] { return hpk_app::next_arg(i, argc, argv); };
    if (s == "--probe-ndev") {  // launch_util.h re-exec probe
      std::printf("%d\n", hpk::device_count());
      return 0;
    } else if (s == "--engine") engine = next();
    else if (s == "-n" || s == "--floats") n = std::strtoull(next(), nullptr, 10);
    else if (s == "--ranks") nranks = std::atoi(next());
    else {
      std::printf("Usage: %s [--engine peer|ipc|rccl] [--floats N] "
                  "[--ranks R]\n", argv[0]);
      return (s == "-h" || s == "--help") ? 0 : 1;
    }
  }
  if (engine == "peer") return run_peer(n, true);
  if (engine == "ipc") return run_ipc(argv[0], n, nranks);
  if (engine == "rccl") return run_rccl(argv[0], n);
  std::fprintf(stderr, "unknown engine '%s'\n", engine.c_str());
  return 1;
}
