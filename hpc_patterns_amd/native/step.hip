// step.hip — StepPlan: submit and join the flagship step's four local
// commands from native code.
//
// Why this exists: the 1-GPU flagship step is bound by the PCIe copy pair
// (H2D + D2H on the two host SDMA engines), and every microsecond between
// the last byte of one step's pair and the first byte of the next is link
// idle time added straight to the step. Going through sdma_copy_begin /
// sdma_wait per copy put two pointer lookups, a signal create/destroy, an
// engine status query and an interrupt wake-up on that path, and started
// the two directions one whole call apart. None of those inputs change from
// step to step, so the plan resolves them once and keeps the per-step path
// to: two signal stores, two copy submissions, two kernel launches.
//
// Host push: the pair itself is lopsided. An engine H2D is a stream of
// device reads, and every read request travels host-bound next to the D2H
// payload, so D2H runs slower while H2D is in flight and the device-bound
// direction idles at the end of the pair. The plan can move the tail of H2D
// with host threads instead (nontemporal stores through the PCIe BAR: posted
// writes, no requests), which unloads the host-bound direction. How much it
// pushes is chosen once from measured times; see choose_push_fraction().

#include "include/hpk.h"
#include "include/push_pool.h"
#include "include/sdma_route.h"

#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <stdexcept>

#include <fcntl.h>
#include <unistd.h>

namespace hpk {

namespace {

uint64_t timestamp_frequency() {
  static uint64_t hz = [] {
    (void)hipFree(nullptr); // ROCr is live once HIP is
    uint64_t f = 0;
    detail::check_hsa(
        hsa_system_get_info(HSA_SYSTEM_INFO_TIMESTAMP_FREQUENCY, &f),
        "hsa_system_get_info(TIMESTAMP_FREQUENCY)");
    if (f == 0) throw std::runtime_error("HSA timestamp frequency is 0");
    return f;
  }();
  return hz;
}

uint64_t ticks_to_ns(uint64_t ticks) {
  uint64_t hz = timestamp_frequency();
  return (ticks / hz) * 1000000000ull + (ticks % hz) * 1000000000ull / hz;
}

// ROCr's async-copy profiling is one process-wide switch; plans that asked
// for copy timing share it by count. Single-threaded like the plans.
int g_copy_profiling_users = 0;

struct CopyProfiling { // on for a scope (calibration, probe)
  CopyProfiling() {
    if (g_copy_profiling_users == 0)
      detail::check_hsa(hsa_amd_profiling_async_copy_enable(true),
                        "hsa_amd_profiling_async_copy_enable");
    ++g_copy_profiling_users;
  }
  ~CopyProfiling() {
    if (--g_copy_profiling_users == 0)
      hsa_amd_profiling_async_copy_enable(false);
  }
};

// The account the push fraction is chosen by (docs/findings.md). With
// Th, Td the engine times of H2D and D2H alone and R the push rate:
//   host-bound direction   Td + kReadRequestShare * (1 - g) * Th
//   device-bound direction (1 - g) * Th + kPushedByteCost * g * Th
//   pushing threads        g * bytes / R
// The pair takes the largest of the three.
// Both measured at 256 MiB per direction with 10-50 % pushed
// (profiles/flagship_host_push.md): D2H stretches by 0.12-0.13 of the engine
// H2D time next to it (0.17 with nothing pushed, so the predicted gain is on
// the low side), and a pushed byte costs the device-bound direction 1.33
// engine bytes (8 threads push 41 GB/s alone against the engine's 57).
constexpr double kReadRequestShare = 0.125;
constexpr double kPushedByteCost = 1.33;
constexpr double kPushMaxFraction = 0.5;
constexpr double kPushMinGain = 0.02;

double pair_model(double g, double th, double td, double push_s_per_byte,
                  double nbytes) {
  double hb = td + kReadRequestShare * (1.0 - g) * th;
  double db = (1.0 - g) * th + kPushedByteCost * g * th;
  double pt = g * nbytes * push_s_per_byte;
  return std::max(hb, std::max(db, pt));
}

// g in [0, 0.5] with the shortest predicted pair; 0 when that is less than
// 2 % shorter than the pair without a push.
double choose_push_fraction(double th, double td, double push_s_per_byte,
                            double nbytes) {
  double base = pair_model(0.0, th, td, push_s_per_byte, nbytes);
  double best = base, best_g = 0.0;
  for (int i = 1; i <= 64; ++i) {
    double g = kPushMaxFraction * i / 64.0;
    double t = pair_model(g, th, td, push_s_per_byte, nbytes);
    if (t < best) best = t, best_g = g;
  }
  return (base - best) < kPushMinGain * base ? 0.0 : best_g;
}

double median(std::vector<double> v) {
  if (v.empty()) return 0.0;
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

// Whether [p, p + 1) is mapped into this process, asked of the kernel (a
// pipe write from an unmapped address fails with EFAULT) so that a refused
// mapping shows up here and not as a fault in a worker.
bool cpu_can_read(const void* p) {
  int fd[2];
  if (pipe2(fd, O_CLOEXEC | O_NONBLOCK) != 0) return false;
  ssize_t n = write(fd[1], p, 1);
  ::close(fd[0]);
  ::close(fd[1]);
  return n == 1;
}

} // namespace

uint64_t hsa_timestamp_ns() {
  uint64_t hz = timestamp_frequency(); // also makes sure ROCr is up
  (void)hz;
  uint64_t t = 0;
  detail::check_hsa(hsa_system_get_info(HSA_SYSTEM_INFO_TIMESTAMP, &t),
                    "hsa_system_get_info(TIMESTAMP)");
  return ticks_to_ns(t);
}

StepPushSplit step_push_ranges(size_t nbytes, double g, int nthreads) {
  PushSplit s = hpk::step_push_ranges_impl(nbytes, g, nthreads);
  StepPushSplit out;
  out.head = s.head;
  for (const PushRange& r : s.ranges) out.ranges.emplace_back(r.begin, r.end);
  return out;
}

struct StepPlan::Impl {
  StepCopy h2d, d2h, d2d;
  detail::SdmaRoute h2d_route, d2h_route;
  float* busy_out = nullptr;
  long busy_globalsize = 0;
  hipStream_t busy_stream = nullptr, copy_stream = nullptr;
  hsa_signal_t sig[2] = {{0}, {0}}; // [0] H2D, [1] D2H
  bool have_signals = false;
  bool pending = false;
  bool time_copies = false;
  bool blocked_wait = false;
  uint64_t spin_ticks = 0;
  std::vector<std::pair<uint64_t, uint64_t>> times;

  // host push
  int access_pool = -1;      // hsa_amd_memory_pool_access_t of the CPU agent
  std::vector<std::pair<uint32_t, int>> pool_access; // (flags, access)
  bool access_resolved = false;
  bool access_granted = false, mapping_ok = false;
  volatile uint32_t* hdp_flush = nullptr;
  bool push_ok = false;      // all of the above
  int nthreads = 0;          // configured worker count
  PushSplit split;           // head == h2d.nbytes and no ranges: no push
  bool pushing = false;      // split.head < h2d.nbytes
  std::unique_ptr<PushPool> pool;
  uint64_t submit_ns = 0;
  std::pair<uint64_t, uint64_t> last_push{0, 0};

  // Wait policy: bounded ACTIVE wait, then BLOCKED. Measured on MI355X at
  // the default step (30 steps each, profiles/flagship_link_idle.md): from
  // the last copy byte to join() returning takes 34 us with the active wait
  // against 68 us with the blocked one (interrupt wake-up), and the link
  // idles 47 us against 90 us between steps. The spin is bounded (50 ms,
  // ~9x the 256 MiB pair) so a stalled link does not pin a CPU forever.
  // HPK_STEP_WAIT=blocked selects the blocked wait from the start.
  void wait_signal(hsa_signal_t s) const {
    if (!blocked_wait &&
        hsa_signal_wait_scacquire(s, HSA_SIGNAL_CONDITION_LT, 1, spin_ticks,
                                  HSA_WAIT_STATE_ACTIVE) < 1)
      return;
    while (hsa_signal_wait_scacquire(s, HSA_SIGNAL_CONDITION_LT, 1,
                                     UINT64_MAX, HSA_WAIT_STATE_BLOCKED) >= 1) {
    }
  }

  hsa_status_t issue(const StepCopy& c, size_t nbytes,
                     const detail::SdmaRoute& r, hsa_signal_t s) const {
    return hsa_amd_memory_async_copy_on_engine(
        c.dst, r.dst_agent, c.src, r.src_agent, nbytes, 0, nullptr, s,
        (hsa_amd_sdma_engine_id_t)r.engine, /*force_copy_on_sdma=*/true);
  }

  // The route the runtime takes for its own direct host writes to device
  // memory: they sit in the HDP until its flush register is written; the
  // read back makes sure the write has reached the device.
  void flush_hdp() const {
    *hdp_flush = 1u;
    (void)*hdp_flush;
  }

  // (a) of the probe, and the gate for any push: ask for CPU access to the
  // H2D destination and find the HDP flush register. "No" is an answer.
  void resolve_push_access() {
    access_resolved = true;
    hsa_agent_t gpu = h2d_route.dst_agent, cpu{};
    if (hsa_agent_get_info(gpu,
                           (hsa_agent_info_t)HSA_AMD_AGENT_INFO_NEAREST_CPU,
                           &cpu) != HSA_STATUS_SUCCESS)
      return;
    hsa_device_type_t type;
    if (hsa_agent_get_info(cpu, HSA_AGENT_INFO_DEVICE, &type) !=
            HSA_STATUS_SUCCESS ||
        type != HSA_DEVICE_TYPE_CPU)
      return;

    hsa_amd_pointer_info_t info;
    info.size = sizeof(info);
    uint32_t n_acc = 0;
    hsa_agent_t* acc = nullptr;
    if (hsa_amd_pointer_info(h2d.dst, &info, std::malloc, &n_acc, &acc) !=
        HSA_STATUS_SUCCESS)
      return;
    std::vector<hsa_agent_t> agents(acc, acc + n_acc);
    std::free(acc);
    if (info.type != HSA_EXT_POINTER_TYPE_HSA ||
        info.agentOwner.handle != gpu.handle)
      return;
    const char* base = static_cast<const char*>(info.agentBaseAddress);
    const char* dst = static_cast<const char*>(h2d.dst);
    if (dst < base || dst + h2d.nbytes > base + info.sizeInBytes) return;

    // The CPU agent's access to the pool the buffer came from: the owner's
    // global pool with the allocation's own flags (coarse-grained for
    // hipMalloc). Every global pool's answer is kept for the probe.
    struct Ctx {
      hsa_agent_t cpu;
      uint32_t want_flags;
      int access;
      std::vector<std::pair<uint32_t, int>>* pools;
    } ctx{cpu, info.global_flags, -1, &pool_access};
    pool_access.clear();
    hsa_amd_agent_iterate_memory_pools(
        gpu,
        [](hsa_amd_memory_pool_t pool, void* data) -> hsa_status_t {
          auto* c = static_cast<Ctx*>(data);
          hsa_amd_segment_t seg;
          if (hsa_amd_memory_pool_get_info(pool, HSA_AMD_MEMORY_POOL_INFO_SEGMENT,
                                           &seg) != HSA_STATUS_SUCCESS ||
              seg != HSA_AMD_SEGMENT_GLOBAL)
            return HSA_STATUS_SUCCESS;
          uint32_t flags = 0;
          hsa_amd_memory_pool_get_info(pool, HSA_AMD_MEMORY_POOL_INFO_GLOBAL_FLAGS,
                                       &flags);
          hsa_amd_memory_pool_access_t a = HSA_AMD_MEMORY_POOL_ACCESS_NEVER_ALLOWED;
          if (hsa_amd_agent_memory_pool_get_info(
                  c->cpu, pool, HSA_AMD_AGENT_MEMORY_POOL_INFO_ACCESS, &a) !=
              HSA_STATUS_SUCCESS)
            a = HSA_AMD_MEMORY_POOL_ACCESS_NEVER_ALLOWED;
          c->pools->emplace_back(flags, (int)a);
          const uint32_t grain = HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_FINE_GRAINED |
                                 HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_COARSE_GRAINED |
                                 HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_EXTENDED_SCOPE_FINE_GRAINED;
          if ((flags & grain) == (c->want_flags & grain)) c->access = (int)a;
          return HSA_STATUS_SUCCESS;
        },
        &ctx);
    access_pool = ctx.access;

    // The other three facts are taken whatever the pool said, so the probe
    // can show all of them; the push needs every one.
    // allow_access replaces the list of agents with access, so keep those
    // that have it
    bool listed = false;
    for (hsa_agent_t a : agents) listed = listed || a.handle == cpu.handle;
    if (!listed) agents.push_back(cpu);
    access_granted =
        hsa_amd_agents_allow_access((uint32_t)agents.size(), agents.data(),
                                    nullptr, info.agentBaseAddress) ==
        HSA_STATUS_SUCCESS;
    mapping_ok = cpu_can_read(dst) && cpu_can_read(dst + h2d.nbytes - 1);

    hsa_amd_hdp_flush_t hdp{nullptr, nullptr};
    if (hsa_agent_get_info(gpu, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_HDP_FLUSH,
                           &hdp) == HSA_STATUS_SUCCESS &&
        hdp.HDP_MEM_FLUSH_CNTL && cpu_can_read(hdp.HDP_MEM_FLUSH_CNTL))
      hdp_flush = hdp.HDP_MEM_FLUSH_CNTL;
    if (access_pool <= (int)HSA_AMD_MEMORY_POOL_ACCESS_NEVER_ALLOWED ||
        !access_granted || !mapping_ok || !hdp_flush)
      return;
    push_ok = true;
  }

  // One round of copies without kernels, for calibration and the probe.
  // Any of: engine H2D of [0, head), pushed ranges, engine D2H. Engine
  // times need CopyProfiling alive; all in seconds, 0 for a part left out.
  struct Round {
    double h2d = 0, d2h = 0, push = 0, wake = 0, wall = 0;
  };
  Round run_round(PushPool* workers, size_t head,
                  const std::vector<PushRange>* ranges, bool with_d2h) {
    Round r;
    bool eng_h2d = head > 0;
    hsa_signal_store_relaxed(sig[0], eng_h2d ? 1 : 0);
    hsa_signal_store_relaxed(sig[1], with_d2h ? 1 : 0);
    uint64_t t0 = PushPool::now_ns();
    if (workers && ranges) workers->kick(h2d.dst, h2d.src, *ranges, true);
    hsa_status_t s0 = HSA_STATUS_SUCCESS, s1 = HSA_STATUS_SUCCESS;
    if (eng_h2d) s0 = issue(h2d, head, h2d_route, sig[0]);
    if (s0 != HSA_STATUS_SUCCESS) hsa_signal_store_relaxed(sig[0], 0);
    if (with_d2h && s0 == HSA_STATUS_SUCCESS)
      s1 = issue(d2h, d2h.nbytes, d2h_route, sig[1]);
    if (s1 != HSA_STATUS_SUCCESS || s0 != HSA_STATUS_SUCCESS)
      hsa_signal_store_relaxed(sig[1], 0);
    if (workers && ranges) {
      workers->wait();
      flush_hdp();
    }
    wait_signal(sig[0]);
    wait_signal(sig[1]);
    r.wall = (PushPool::now_ns() - t0) * 1e-9;
    detail::check_hsa(s0, "hsa_amd_memory_async_copy_on_engine(H2D)");
    detail::check_hsa(s1, "hsa_amd_memory_async_copy_on_engine(D2H)");
    if (hsa_signal_load_relaxed(sig[0]) < 0 ||
        hsa_signal_load_relaxed(sig[1]) < 0)
      throw std::runtime_error("StepPlan: an engine copy completed with error");
    hsa_amd_profiling_async_copy_time_t t{};
    if (eng_h2d &&
        hsa_amd_profiling_get_async_copy_time(sig[0], &t) == HSA_STATUS_SUCCESS)
      r.h2d = ticks_to_ns(t.end - t.start) * 1e-9;
    if (with_d2h &&
        hsa_amd_profiling_get_async_copy_time(sig[1], &t) == HSA_STATUS_SUCCESS)
      r.d2h = ticks_to_ns(t.end - t.start) * 1e-9;
    if (workers && ranges) {
      uint64_t first = 0, done = 0;
      for (const PushPool::Stat& st : workers->stats()) {
        if (!st.first_store_ns) continue;
        if (!first || st.first_store_ns < first) first = st.first_store_ns;
        done = std::max(done, st.done_ns);
      }
      if (first) r.wake = (first - t0) * 1e-9, r.push = (done - t0) * 1e-9;
    }
    return r;
  }

  void set_split(double g) {
    split = step_push_ranges_impl(h2d.nbytes, g, nthreads);
    pushing = split.head < h2d.nbytes;
  }

  // g from three times measured here, with the device idle: legitimate to
  // do once because buffers, link and host stay what they are from step to
  // step in real use, too.
  double calibrate_push_fraction() {
    CopyProfiling prof;
    size_t slice = std::min(h2d.nbytes, size_t(32) << 20);
    PushSplit probe = step_push_ranges_impl(
        h2d.nbytes, (double)slice / (double)h2d.nbytes, nthreads);
    double th = 0, td = 0, tp = 0;
    for (int i = 0; i < 2; ++i) { // first round touches the buffers
      th = run_round(nullptr, h2d.nbytes, nullptr, false).h2d;
      td = run_round(nullptr, 0, nullptr, true).d2h;
      tp = run_round(pool.get(), 0, &probe.ranges, false).push;
    }
    if (th <= 0 || td <= 0 || tp <= 0) return 0.0;
    double pushed = (double)(h2d.nbytes - probe.head);
    return choose_push_fraction(th, td, tp / pushed, (double)h2d.nbytes);
  }
};

StepPlan::StepPlan(int device, StepCopy h2d, StepCopy d2h, StepCopy d2d,
                   float* busy_out, long busy_globalsize,
                   hipStream_t busy_stream, hipStream_t copy_stream,
                   bool time_copies, double push_fraction)
    : impl_(new Impl) {
  Impl& p = *impl_;
  try {
    if (!h2d.dst || !h2d.src || !d2h.dst || !d2h.src || !h2d.nbytes ||
        !d2h.nbytes)
      throw std::runtime_error("StepPlan: empty H2D/D2H copy");
    if (d2d.nbytes && (!d2d.dst || !d2d.src))
      throw std::runtime_error("StepPlan: null D2D pointer");
    if (busy_globalsize > 0 && !busy_out)
      throw std::runtime_error("StepPlan: null busy-wait buffer");
    p.h2d = h2d;
    p.d2h = d2h;
    p.d2d = d2d;
    p.busy_out = busy_out;
    p.busy_globalsize = busy_globalsize;
    p.busy_stream = busy_stream;
    p.copy_stream = copy_stream;

    // same rule as the per-call path: H2D = first engine of gpu<-cpu,
    // D2H = second engine of cpu<-gpu — but asked once, with the device idle
    p.h2d_route = detail::sdma_resolve(h2d.dst, h2d.src, device, 0);
    p.d2h_route = detail::sdma_resolve(d2h.dst, d2h.src, device, 1);
    if (p.h2d_route.engine == 0 || p.d2h_route.engine == 0 ||
        p.h2d_route.engine == p.d2h_route.engine)
      throw std::runtime_error(
          "StepPlan: fewer than two host SDMA engines resolved");

    const char* w = std::getenv("HPK_STEP_WAIT");
    p.blocked_wait = w && std::strcmp(w, "blocked") == 0;
    p.spin_ticks = timestamp_frequency() / 20; // 50 ms

    detail::check_hsa(hsa_signal_create(0, 0, nullptr, &p.sig[0]),
                      "hsa_signal_create");
    hsa_status_t s = hsa_signal_create(0, 0, nullptr, &p.sig[1]);
    if (s != HSA_STATUS_SUCCESS) {
      hsa_signal_destroy(p.sig[0]);
      detail::check_hsa(s, "hsa_signal_create");
    }
    p.have_signals = true;

    // ---- host push: how much, by how many threads ----
    // Thread count from the probe table (profiles/flagship_host_push.md),
    // never from the number of CPUs the host happens to have.
    p.nthreads = kStepPushDefaultThreads;
    if (const char* e = std::getenv("HPK_STEP_PUSH_THREADS")) {
      int n = std::atoi(e);
      if (n >= 1) p.nthreads = std::min(n, kPushMaxThreads);
    }
    double want = push_fraction; // < 0: not fixed by the caller
    if (want < 0.0) {
      const char* e = std::getenv("HPK_STEP_PUSH");
      if (e && *e) {
        char* end = nullptr;
        double v = std::strtod(e, &end);
        if (end == e || v < 0.0 || v > 1.0)
          throw std::runtime_error(
              "StepPlan: HPK_STEP_PUSH must be a fraction in [0, 1]");
        want = v;
      } else if (h2d.nbytes < kStepPushMinBytes) {
        want = 0.0;
      }
    }
    p.set_split(0.0);
    if (want != 0.0) {
      p.resolve_push_access();
      if (p.push_ok) {
        // spin for about a step before sleeping: 2x an engine copy of the
        // larger payload at the ~50 GB/s the link gives one direction
        uint64_t spin_ns = std::max<uint64_t>(
            200000, std::max(h2d.nbytes, d2h.nbytes) / 25);
        p.pool.reset(new PushPool(p.nthreads, spin_ns));
        if (want < 0.0) want = p.calibrate_push_fraction();
        p.set_split(want);
        if (!p.pushing) p.pool.reset();
      }
    }

    if (time_copies) {
      if (g_copy_profiling_users == 0)
        detail::check_hsa(hsa_amd_profiling_async_copy_enable(true),
                          "hsa_amd_profiling_async_copy_enable");
      ++g_copy_profiling_users;
      p.time_copies = true;
    }
  } catch (...) {
    p.pool.reset();
    if (p.have_signals) {
      hsa_signal_destroy(p.sig[0]);
      hsa_signal_destroy(p.sig[1]);
    }
    delete impl_;
    impl_ = nullptr;
    throw;
  }
}

StepPlan::~StepPlan() {
  try {
    close();
  } catch (...) { // a destructor reports nothing; the signals are gone
  }
  delete impl_;
}

bool StepPlan::pending() const { return impl_->pending; }

void StepPlan::submit(long tripcount) {
  Impl& p = *impl_;
  if (!p.have_signals) throw std::runtime_error("StepPlan: submit after close");
  // re-arming a signal that a copy in flight still decrements would lose
  // that copy's completion
  if (p.pending)
    throw std::runtime_error(
        "StepPlan: submit with the previous submission not joined");

  // workers first: they need no engine, and their stores are the part of
  // H2D that starts latest after a wake-up
  if (p.pushing) {
    if (p.time_copies) p.submit_ns = PushPool::now_ns();
    p.pool->kick(p.h2d.dst, p.h2d.src, p.split.ranges, p.time_copies);
  }
  bool eng_h2d = p.split.head > 0;
  hsa_signal_store_relaxed(p.sig[0], eng_h2d ? 1 : 0);
  hsa_signal_store_relaxed(p.sig[1], 1);
  hsa_status_t s0 = HSA_STATUS_SUCCESS;
  if (eng_h2d) s0 = p.issue(p.h2d, p.split.head, p.h2d_route, p.sig[0]);
  if (s0 != HSA_STATUS_SUCCESS) { // no engine copy in flight
    hsa_signal_store_relaxed(p.sig[0], 0);
    hsa_signal_store_relaxed(p.sig[1], 0);
    if (p.pushing) p.pool->wait();
    detail::check_hsa(s0, "hsa_amd_memory_async_copy_on_engine(H2D)");
  }
  hsa_status_t s1 = p.issue(p.d2h, p.d2h.nbytes, p.d2h_route, p.sig[1]);
  if (s1 != HSA_STATUS_SUCCESS) { // H2D is in flight: drain it, then report
    hsa_signal_store_relaxed(p.sig[1], 0);
    if (p.pushing) p.pool->wait();
    p.wait_signal(p.sig[0]);
    detail::check_hsa(s1, "hsa_amd_memory_async_copy_on_engine(D2H)");
  }
  p.pending = true; // from here on a throw leaves the plan joinable

  if (p.busy_globalsize > 0)
    launch_busy_wait(p.busy_out, tripcount, p.busy_globalsize, p.busy_stream);
  if (p.d2d.nbytes)
    launch_copy_kernel(p.d2d.dst, p.d2d.src, p.d2d.nbytes, p.copy_stream);
}

void StepPlan::join() {
  Impl& p = *impl_;
  if (!p.pending) return;
  if (p.pushing) {
    p.pool->wait();
    p.flush_hdp();
  }
  p.wait_signal(p.sig[0]);
  p.wait_signal(p.sig[1]);
  // neither signal is referenced by a copy any more
  p.pending = false;
  bool copy_failed = hsa_signal_load_relaxed(p.sig[0]) < 0 ||
                     hsa_signal_load_relaxed(p.sig[1]) < 0;
  check_hip(hipStreamSynchronize(p.busy_stream), "hipStreamSynchronize(busy)");
  if (p.copy_stream != p.busy_stream)
    check_hip(hipStreamSynchronize(p.copy_stream),
              "hipStreamSynchronize(copy)");
  if (copy_failed)
    throw std::runtime_error("StepPlan: an engine copy completed with error");
  if (p.time_copies) {
    for (int i = 0; i < 2; ++i) {
      if (i == 0 && p.split.head == 0) { // pushed whole: no engine copy
        p.times.emplace_back(0, 0);
        continue;
      }
      hsa_amd_profiling_async_copy_time_t t{};
      detail::check_hsa(hsa_amd_profiling_get_async_copy_time(p.sig[i], &t),
                        "hsa_amd_profiling_get_async_copy_time");
      p.times.emplace_back(ticks_to_ns(t.start), ticks_to_ns(t.end));
    }
    if (p.pushing) {
      uint64_t first = 0, done = 0;
      for (const PushPool::Stat& st : p.pool->stats()) {
        if (!st.first_store_ns) continue;
        if (!first || st.first_store_ns < first) first = st.first_store_ns;
        done = std::max(done, st.done_ns);
      }
      p.last_push = {first > p.submit_ns ? first - p.submit_ns : 0,
                     done > p.submit_ns ? done - p.submit_ns : 0};
    }
  }
}

void StepPlan::close() {
  Impl& p = *impl_;
  if (!p.have_signals) return;
  // Wait out the copies whatever else happens: a signal that a copy still
  // references must not be destroyed.
  std::exception_ptr err;
  try {
    join();
  } catch (...) {
    err = std::current_exception();
  }
  if (p.pool) { // join() above has waited for the workers
    p.pool->stop();
    p.pool.reset();
    p.pushing = false;
  }
  hsa_signal_destroy(p.sig[0]);
  hsa_signal_destroy(p.sig[1]);
  p.have_signals = false;
  if (p.time_copies) {
    p.time_copies = false;
    if (--g_copy_profiling_users == 0)
      hsa_amd_profiling_async_copy_enable(false);
  }
  if (err) std::rethrow_exception(err);
}

const std::vector<std::pair<uint64_t, uint64_t>>& StepPlan::copy_times()
    const {
  return impl_->times;
}

void StepPlan::clear_copy_times() { impl_->times.clear(); }

double StepPlan::push_fraction() const {
  const Impl& p = *impl_;
  return (double)(p.h2d.nbytes - p.split.head) / (double)p.h2d.nbytes;
}

int StepPlan::push_threads() const {
  const Impl& p = *impl_;
  return p.split.head < p.h2d.nbytes ? p.nthreads : 0;
}

bool StepPlan::push_access() const { return impl_->push_ok; }

std::pair<uint64_t, uint64_t> StepPlan::push_times() const {
  return impl_->last_push;
}

std::vector<std::pair<std::string, double>> StepPlan::push_probe(int reps) {
  Impl& p = *impl_;
  if (!p.have_signals) throw std::runtime_error("StepPlan: probe after close");
  if (p.pending) throw std::runtime_error("StepPlan: probe with a step pending");
  if (reps < 1) reps = 1;
  std::vector<std::pair<std::string, double>> rows;
  auto row = [&](const std::string& k, double v) { rows.emplace_back(k, v); };

  // (a)
  if (!p.access_resolved) p.resolve_push_access();
  for (const auto& pa : p.pool_access)
    row("access_pool_info.flags_" + std::to_string(pa.first), pa.second);
  row("access_pool_info", p.access_pool);
  row("access_granted", p.access_granted);
  row("mapping_ok", p.mapping_ok);
  row("hdp_flush_present", p.hdp_flush != nullptr);
  row("bar_access", p.push_ok);

  CopyProfiling prof;
  const size_t nb = p.h2d.nbytes;
  auto med = [&](auto&& fn) { // median of each field over reps, 1 warm-up
    std::vector<double> h, d, pu, wk, wa;
    for (int i = 0; i <= reps; ++i) {
      Impl::Round r = fn();
      if (i == 0) continue;
      h.push_back(r.h2d), d.push_back(r.d2h), pu.push_back(r.push);
      wk.push_back(r.wake), wa.push_back(r.wall);
    }
    Impl::Round m;
    m.h2d = median(h), m.d2h = median(d), m.push = median(pu);
    m.wake = median(wk), m.wall = median(wa);
    return m;
  };
  auto emit = [&](const std::string& name, const Impl::Round& m) {
    row(name + ".h2d_engine_us", m.h2d * 1e6);
    row(name + ".d2h_engine_us", m.d2h * 1e6);
    row(name + ".push_done_us", m.push * 1e6);
    row(name + ".push_wake_us", m.wake * 1e6);
    row(name + ".wall_us", m.wall * 1e6);
  };

  // (c) engine only
  emit("h2d_alone", med([&] { return p.run_round(nullptr, nb, nullptr, false); }));
  emit("d2h_alone", med([&] { return p.run_round(nullptr, 0, nullptr, true); }));
  emit("engine_pair", med([&] { return p.run_round(nullptr, nb, nullptr, true); }));
  if (!p.push_ok) return rows;

  // (b) push rate
  uint64_t spin_ns = 20000000; // keep the workers awake between rounds
  for (int nt : {1, 2, 4, 8}) {
    PushPool workers(nt, spin_ns);
    for (size_t mib : {size_t(32), size_t(128)}) {
      size_t bytes = mib << 20;
      if (bytes > nb) continue;
      PushSplit s = step_push_ranges_impl(nb, (double)bytes / (double)nb, nt);
      Impl::Round m =
          med([&] { return p.run_round(&workers, 0, &s.ranges, false); });
      row("push_GBps." + std::to_string(nt) + "t." + std::to_string(mib) +
              "MiB",
          (double)(nb - s.head) / m.push * 1e-9);
    }
  }

  // (c) under push, with the plan's thread count
  PushPool workers(p.nthreads, spin_ns);
  row("split_threads", p.nthreads);
  {
    PushSplit s = step_push_ranges_impl(nb, 1.0, p.nthreads);
    emit("push_all_pair",
         med([&] { return p.run_round(&workers, 0, &s.ranges, true); }));
  }
  for (int pct : {10, 20, 30, 40, 50}) {
    PushSplit s = step_push_ranges_impl(nb, pct / 100.0, p.nthreads);
    emit("split_pair.g" + std::to_string(pct),
         med([&] { return p.run_round(&workers, s.head, &s.ranges, true); }));
  }
  row("plan_push_fraction", push_fraction());
  return rows;
}

} // namespace hpk
