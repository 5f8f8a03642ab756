// miniapp_util.h — host-side helpers the miniapps share: wall clock,
// argument fetcher, the M|D|H|S allocator letters, the shuffled-iota
// payload and the all-reduce verdict. Neither RCCL nor MPI is included.
#pragma once

#include "../hpc_patterns_amd/native/include/hpk.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

namespace hpk_app {

inline double now_s() {
  return std::chrono::duration<double>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

// The value that follows option argv[i]; advances i.
inline const char* next_arg(int& i, int argc, char* argv[]) {
  if (++i >= argc) { std::fprintf(stderr, "missing value\n"); std::exit(1); }
  return argv[i];
}

// Allocator letters: M malloc, D hipMalloc, H hipHostMalloc (pinned),
// S hipMallocManaged. malloc failure returns nullptr; HIP failures throw.
inline void* alloc_buf(char kind, size_t bytes) {
  void* p = nullptr;
  switch (kind) {
    case 'M': p = std::malloc(bytes); break;
    case 'D': hpk::check_hip(hipMalloc(&p, bytes), "hipMalloc"); break;
    case 'H':
      hpk::check_hip(hipHostMalloc(&p, bytes, hipHostMallocDefault),
                     "hipHostMalloc");
      break;
    case 'S':
      hpk::check_hip(hipMallocManaged(&p, bytes, hipMemAttachGlobal),
                     "hipMallocManaged");
      break;
    default: std::abort();
  }
  return p;
}

inline void free_buf(char kind, void* p) {
  if (!p) return;
  if (kind == 'M') std::free(p);
  else if (kind == 'H') (void)hipHostFree(p);
  else (void)hipFree(p);
}

// Host-shuffled iota payload (reference peer2pear.cpp:8-17) and its exact
// double checksum. The seed defines the payload: the generator, shuffle and
// summation order must not change.
struct Payload {
  std::vector<float> v;
  double sum;
};

inline Payload shuffled_iota(size_t n, unsigned seed) {
  Payload p{std::vector<float>(n), 0.0};
  std::iota(p.v.begin(), p.v.end(), 0.f);
  std::minstd_rand g(seed);
  std::shuffle(p.v.begin(), p.v.end(), g);
  for (size_t i = 0; i < n; ++i) p.sum += (double)p.v[i];
  return p;
}

// All-reduce analytic oracle: VA=rank everywhere, so every element must be
// size*(size-1)/2 (reference allreduce-mpi-sycl.cpp:192-204). Prints the
// rank's verdict line; returns whether it passed.
inline bool allreduce_verdict(double got, size_t n, int size, int rank) {
  double expected = (double)n * ((double)size * (size - 1) / 2.0);
  bool pass = std::abs(got - expected) < 1e-6 * std::max(1.0, expected);
  std::printf("%s rank %d (sum %.1f, expected %.1f)\n",
              pass ? "Passed" : "FAILED", rank, got, expected);
  return pass;
}

// Bus bandwidth convention: a ring moves 2(size-1)/size * bytes per rank.
inline double allreduce_busbw(size_t bytes, int size, double seconds) {
  double gb = (double)bytes / 1e9;
  return size > 1 ? 2.0 * (size - 1) / size * gb / seconds : gb / seconds;
}

} // namespace hpk_app
