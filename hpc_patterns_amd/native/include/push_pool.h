// push_pool.h — library-internal, host-only: the worker pool that stores the
// tail of StepPlan's H2D copy straight into device memory, and the function
// that cuts the copy into an engine head and per-thread tail ranges.
// No HIP or HSA in here, so cpp/push_pool_main.cpp can build it with the
// plain host compiler (and -fsanitize=thread) and push into host memory.
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace hpk {

struct PushRange {
  size_t begin = 0, end = 0; // byte offsets into the copy, [begin, end)
};

struct PushSplit {
  size_t head = 0;               // the engine copies [0, head)
  std::vector<PushRange> ranges; // nthreads entries tiling [head, nbytes)
};

constexpr size_t kPushLine = 64;    // one write-combine buffer
constexpr size_t kPushSplitAlign = 4096;
constexpr int kPushMaxThreads = 8;

// The engine keeps [0, head), head = (1 - g) * nbytes rounded DOWN to 4 KiB
// (so the tail also takes whatever nbytes has beyond a 4 KiB multiple); the
// tail is dealt out in whole 64-byte lines, as evenly as they divide, to
// nthreads ranges in order. Every range begins on a line; only the last
// non-empty one may end off a line, at nbytes. Threads left without a line
// get an empty range at nbytes. g <= 0 gives head == nbytes and all ranges
// empty; g >= 1 gives head == 0.
inline PushSplit step_push_ranges_impl(size_t nbytes, double g, int nthreads) {
  PushSplit s;
  if (nthreads < 1) nthreads = 1;
  if (!(g > 0.0)) g = 0.0; // also NaN
  if (g > 1.0) g = 1.0;
  size_t tail_want = (size_t)((double)nbytes * g + 0.5);
  if (tail_want > nbytes) tail_want = nbytes;
  s.head = g > 0.0 ? (nbytes - tail_want) / kPushSplitAlign * kPushSplitAlign
                   : nbytes;
  size_t lines = (nbytes - s.head + kPushLine - 1) / kPushLine;
  size_t per = lines / (size_t)nthreads, extra = lines % (size_t)nthreads;
  size_t line = 0;
  s.ranges.resize((size_t)nthreads);
  for (int t = 0; t < nthreads; ++t) {
    size_t n = per + ((size_t)t < extra ? 1 : 0);
    size_t b = s.head + line * kPushLine, e = b + n * kPushLine;
    s.ranges[(size_t)t].begin = b < nbytes ? b : nbytes;
    s.ranges[(size_t)t].end = e < nbytes ? e : nbytes;
    line += n;
  }
  return s;
}

// dst[0, n) = src[0, n) with nontemporal 64-byte stores on every whole
// dst-aligned line (four 16-byte stores fill one write-combine buffer, which
// leaves as one 64-byte write), plain stores on the ragged ends, and a store
// fence so that everything has left the core when this returns.
inline void push_copy(void* dst, const void* src, size_t n) {
  char* d = static_cast<char*>(dst);
  const char* s = static_cast<const char*>(src);
#if defined(__x86_64__)
  size_t lead = (kPushLine - (reinterpret_cast<uintptr_t>(d) % kPushLine)) %
                kPushLine;
  if (lead > n) lead = n;
  std::memcpy(d, s, lead);
  d += lead, s += lead, n -= lead;
  for (; n >= kPushLine; d += kPushLine, s += kPushLine, n -= kPushLine) {
    __m128i a = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s));
    __m128i b = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + 16));
    __m128i c = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + 32));
    __m128i e = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + 48));
    _mm_stream_si128(reinterpret_cast<__m128i*>(d), a);
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + 16), b);
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + 32), c);
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + 48), e);
  }
  std::memcpy(d, s, n);
  _mm_sfence();
#else
  std::memcpy(d, s, n);
  std::atomic_thread_fence(std::memory_order_seq_cst);
#endif
}

inline void push_cpu_relax() {
#if defined(__x86_64__)
  _mm_pause();
#endif
}

// Workers created once, parked on a generation counter. One thread drives
// the pool: kick() hands every worker its range, wait() returns when all of
// them have fenced their stores. Between kicks a worker spins for spin_ns
// (the caller sizes that to about one step, so a steady run of steps never
// pays a wake-up), then sleeps on a condition variable.
class PushPool {
 public:
  struct Stat {
    uint64_t first_store_ns = 0; // steady clock; 0 when the range was empty
    uint64_t done_ns = 0;
  };

  PushPool(int nthreads, uint64_t spin_ns)
      : n_(nthreads < 1 ? 1
                        : nthreads > kPushMaxThreads ? kPushMaxThreads
                                                     : nthreads),
        spin_ns_(spin_ns), stats_((size_t)n_) {
    threads_.reserve((size_t)n_);
    for (int t = 0; t < n_; ++t) threads_.emplace_back([this, t] { run(t); });
  }
  ~PushPool() { stop(); }
  PushPool(const PushPool&) = delete;
  PushPool& operator=(const PushPool&) = delete;

  int size() const { return n_; }
  void set_spin_ns(uint64_t ns) { spin_ns_.store(ns, std::memory_order_relaxed); }

  static uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
  }

  // ranges.size() <= size(); workers beyond it get nothing. The previous
  // kick must have been waited for.
  void kick(void* dst, const void* src, const std::vector<PushRange>& ranges,
            bool record) {
    dst_ = static_cast<char*>(dst);
    src_ = static_cast<const char*>(src);
    ranges_ = ranges;
    ranges_.resize((size_t)n_);
    record_ = record;
    remaining_.store(n_, std::memory_order_relaxed);
    in_flight_ = true;
    {
      // under the lock, so a worker between its last look at the counter
      // and its sleep cannot miss the change
      std::lock_guard<std::mutex> lk(m_);
      gen_.fetch_add(1, std::memory_order_release);
    }
    if (sleepers_.load(std::memory_order_acquire) > 0) cv_.notify_all();
  }

  void wait() {
    if (!in_flight_) return;
    uint64_t spin = spin_ns_.load(std::memory_order_relaxed);
    uint64_t t0 = now_ns();
    int polls = 0;
    while (remaining_.load(std::memory_order_acquire) != 0) {
      push_cpu_relax();
      if (++polls == 256) {
        polls = 0;
        if (now_ns() - t0 > spin) {
          std::unique_lock<std::mutex> lk(m_);
          done_cv_.wait(lk, [this] {
            return remaining_.load(std::memory_order_acquire) == 0;
          });
        }
      }
    }
    in_flight_ = false;
  }

  // valid after wait() for a kick with record set
  const std::vector<Stat>& stats() const { return stats_; }

  // wait(), then end and join the workers. Idempotent.
  void stop() {
    if (threads_.empty()) return;
    wait();
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_.store(true, std::memory_order_release);
      gen_.fetch_add(1, std::memory_order_release);
    }
    cv_.notify_all();
    for (auto& t : threads_) t.join();
    threads_.clear();
  }

 private:
  void run(int t) {
    uint64_t seen = 0;
    for (;;) {
      uint64_t spin = spin_ns_.load(std::memory_order_relaxed);
      uint64_t t0 = now_ns();
      int polls = 0;
      while (gen_.load(std::memory_order_acquire) == seen) {
        push_cpu_relax();
        if (++polls == 256) {
          polls = 0;
          if (now_ns() - t0 > spin) {
            std::unique_lock<std::mutex> lk(m_);
            sleepers_.fetch_add(1, std::memory_order_acq_rel);
            cv_.wait(lk, [&] {
              return gen_.load(std::memory_order_acquire) != seen;
            });
            sleepers_.fetch_sub(1, std::memory_order_acq_rel);
          }
        }
      }
      seen = gen_.load(std::memory_order_acquire);
      if (stop_.load(std::memory_order_acquire)) return;

      PushRange r = ranges_[(size_t)t];
      Stat st;
      if (r.end > r.begin) {
        if (record_) st.first_store_ns = now_ns();
        push_copy(dst_ + r.begin, src_ + r.begin, r.end - r.begin);
      }
      if (record_) {
        st.done_ns = now_ns();
        stats_[(size_t)t] = st;
      }
      if (remaining_.fetch_sub(1, std::memory_order_acq_rel) == 1) {
        // the driver may already be asleep in wait()
        std::lock_guard<std::mutex> lk(m_);
        done_cv_.notify_all();
      }
    }
  }

  const int n_;
  std::atomic<uint64_t> spin_ns_;
  std::vector<std::thread> threads_;
  std::vector<Stat> stats_;
  std::mutex m_;
  std::condition_variable cv_, done_cv_;
  std::atomic<uint64_t> gen_{0};
  std::atomic<int> remaining_{0};
  std::atomic<int> sleepers_{0};
  std::atomic<bool> stop_{false};
  bool in_flight_ = false;
  // written by kick() before the generation changes, read by workers after
  char* dst_ = nullptr;
  const char* src_ = nullptr;
  std::vector<PushRange> ranges_;
  bool record_ = false;
};

} // namespace hpk
