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

#include "include/hpk.h"
#include "include/sdma_route.h"

#include <cstdlib>
#include <cstring>
#include <exception>
#include <stdexcept>

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

} // namespace

uint64_t hsa_timestamp_ns() {
  uint64_t hz = timestamp_frequency(); // also makes sure ROCr is up
  (void)hz;
  uint64_t t = 0;
  detail::check_hsa(hsa_system_get_info(HSA_SYSTEM_INFO_TIMESTAMP, &t),
                    "hsa_system_get_info(TIMESTAMP)");
  return ticks_to_ns(t);
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

  hsa_status_t issue(const StepCopy& c, const detail::SdmaRoute& r,
                     hsa_signal_t s) const {
    return hsa_amd_memory_async_copy_on_engine(
        c.dst, r.dst_agent, c.src, r.src_agent, c.nbytes, 0, nullptr, s,
        (hsa_amd_sdma_engine_id_t)r.engine, /*force_copy_on_sdma=*/true);
  }
};

StepPlan::StepPlan(int device, StepCopy h2d, StepCopy d2h, StepCopy d2d,
                   float* busy_out, long busy_globalsize,
                   hipStream_t busy_stream, hipStream_t copy_stream,
                   bool time_copies)
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

    if (time_copies) {
      if (g_copy_profiling_users == 0)
        detail::check_hsa(hsa_amd_profiling_async_copy_enable(true),
                          "hsa_amd_profiling_async_copy_enable");
      ++g_copy_profiling_users;
      p.time_copies = true;
    }
  } catch (...) {
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

  hsa_signal_store_relaxed(p.sig[0], 1);
  hsa_signal_store_relaxed(p.sig[1], 1);
  hsa_status_t s0 = p.issue(p.h2d, p.h2d_route, p.sig[0]);
  if (s0 != HSA_STATUS_SUCCESS) { // nothing in flight
    hsa_signal_store_relaxed(p.sig[0], 0);
    hsa_signal_store_relaxed(p.sig[1], 0);
    detail::check_hsa(s0, "hsa_amd_memory_async_copy_on_engine(H2D)");
  }
  hsa_status_t s1 = p.issue(p.d2h, p.d2h_route, p.sig[1]);
  if (s1 != HSA_STATUS_SUCCESS) { // H2D is in flight: drain it, then report
    hsa_signal_store_relaxed(p.sig[1], 0);
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
      hsa_amd_profiling_async_copy_time_t t{};
      detail::check_hsa(hsa_amd_profiling_get_async_copy_time(p.sig[i], &t),
                        "hsa_amd_profiling_get_async_copy_time");
      p.times.emplace_back(ticks_to_ns(t.start), ticks_to_ns(t.end));
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

} // namespace hpk
