// push_pool_main.cpp — StepPlan's push workers on their own, storing into
// ordinary host memory: no GPU, no HIP. Built by the plain host compiler
// (`make bin/hpk_push_pool`), and with ThreadSanitizer by `make tsan-push`.
//
// Checks, for every split the plan can ask for: each byte of the tail ends
// up in dst exactly as in src, nothing outside the tail is written, rounds
// with fresh payloads never show the round before, a pool that went to
// sleep wakes up, and stop() with a kick in flight joins the workers.
// Exit status 0 and "push_pool OK" on success.

#include "../hpc_patterns_amd/native/include/push_pool.h"

#include <cstdio>
#include <cstdlib>

namespace {

int failures = 0;

void expect(bool ok, const char* what, size_t nbytes, double g, int nt) {
  if (ok) return;
  ++failures;
  std::fprintf(stderr, "FAIL %s: nbytes=%zu g=%g threads=%d\n", what, nbytes, g,
               nt);
}

void check_split(size_t nbytes, double g, int nt) {
  hpk::PushSplit s = hpk::step_push_ranges_impl(nbytes, g, nt);
  expect((s.head <= nbytes && s.head % hpk::kPushSplitAlign == 0) ||
             s.head == nbytes,
         "head", nbytes, g, nt);
  expect((int)s.ranges.size() == nt, "range count", nbytes, g, nt);
  size_t at = s.head;
  for (const hpk::PushRange& r : s.ranges) {
    expect(r.begin == at || (r.begin == r.end && r.begin == nbytes), "tiling",
           nbytes, g, nt);
    expect(r.begin == r.end || r.begin % hpk::kPushLine == 0, "begin aligned",
           nbytes, g, nt);
    expect(r.end % hpk::kPushLine == 0 || r.end == nbytes, "end aligned",
           nbytes, g, nt);
    if (r.end > r.begin) at = r.end;
  }
  expect(at == nbytes, "coverage", nbytes, g, nt);
}

void check_rounds(hpk::PushPool& pool, size_t nbytes, double g, int rounds) {
  const int nt = pool.size();
  hpk::PushSplit s = hpk::step_push_ranges_impl(nbytes, g, nt);
  // 64 guard bytes either side, and dst off a line so the ragged-lead path
  // of push_copy runs for odd sizes
  std::vector<unsigned char> src(nbytes), buf(nbytes + 128, 0xEE);
  unsigned char* dst = buf.data() + 64;
  for (int rnd = 0; rnd < rounds; ++rnd) {
    for (size_t i = 0; i < nbytes; ++i)
      src[i] = (unsigned char)((i * 131 + (size_t)rnd * 17 + 1) & 0xFF);
    for (size_t i = 0; i < s.head; ++i) dst[i] = 0xAB; // the engine's share
    pool.kick(dst, src.data(), s.ranges, true);
    pool.wait();
    bool ok = true;
    for (size_t i = 0; i < s.head; ++i) ok = ok && dst[i] == 0xAB;
    for (size_t i = s.head; i < nbytes; ++i) ok = ok && dst[i] == src[i];
    for (size_t i = 0; i < 64; ++i)
      ok = ok && buf[i] == 0xEE && buf[64 + nbytes + i] == 0xEE;
    expect(ok, "round payload", nbytes, g, nt);
  }
}

} // namespace

int main() {
  const size_t sizes[] = {0, 1, 63, 64, 4096, 4096 + 68, (size_t(1) << 20) + 68};
  const double fractions[] = {0.0, 0.01, 0.25, 0.5, 1.0};
  for (int nt : {1, 3, 8}) {
    hpk::PushPool pool(nt, /*spin_ns=*/200000);
    for (size_t nbytes : sizes)
      for (double g : fractions) {
        check_split(nbytes, g, nt);
        check_rounds(pool, nbytes, g, 3);
      }
    // let the workers fall asleep, then wake them
    std::this_thread::sleep_for(std::chrono::milliseconds(2));
    check_rounds(pool, (size_t(1) << 20) + 68, 0.5, 2);
    // stop() with a kick in flight
    std::vector<unsigned char> src(size_t(4) << 20, 0x5A), dst(src.size(), 0);
    hpk::PushSplit s = hpk::step_push_ranges_impl(src.size(), 1.0, nt);
    pool.kick(dst.data(), src.data(), s.ranges, false);
    pool.stop();
    expect(dst == src, "stop joins the kick in flight", src.size(), 1.0, nt);
    pool.stop(); // idempotent
  }
  if (failures) {
    std::fprintf(stderr, "push_pool: %d failure(s)\n", failures);
    return 1;
  }
  std::puts("push_pool OK");
  return 0;
}
