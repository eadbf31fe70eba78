// TEST INFRASTRUCTURE (CPU only): the host stand-in for the draw launcher (aeonflux_amd/csrc/kernels.hip k_draw), which
// tests/hostsim/fake_hip.cpp does not have: the engine's host sources reach it through a weak reference (plans.cpp run_draws), and only
// the host simulations of the *_rng doors link this file.  It draws nothing - every row it is given is filled with 0xD7 - but it keeps
// what a test needs to see where a call's seed went: how many rows it filled, whether every job came with the 40 staged bytes the test
// announced (fake_draw_expect), and the list of the ranges of fake device memory its jobs read a seed from or wrote rows to, which
// fake_draw_seed_left() searches for those bytes after the call, range by range (never the memory between two ranges: they may lie in
// different lanes' staging areas).  A range whose allocation has been released since (a staging area regrown between two slices) is
// not read but counted (fake_draw_ranges_gone; known only to an AddressSanitizer build, which is what the simulations are).
// What the search cannot see: the pinned host image the seed was uploaded from, which the jobs never point at - that copy is wiped by
// afx::Session::wipe_seeds, under the sanitizer's eyes but not under this file's.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>
#include "../../aeonflux_amd/csrc/plan.h"
#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#endif

static std::mutex mu;
static uint8_t expect40[40];
static uint64_t jobs_seen = 0, jobs_with_seed = 0, ranges_gone = 0;
static std::vector<std::pair<const uint8_t*, size_t>> touched;

static void touch(const uint8_t* a, size_t n) {
  const std::pair<const uint8_t*, size_t> r(a, n);
  if (std::find(touched.begin(), touched.end(), r) == touched.end()) touched.push_back(r);
}
static bool still_there(const uint8_t* a, size_t n) {
#if defined(__SANITIZE_ADDRESS__)
  return __asan_region_is_poisoned(const_cast<uint8_t*>(a), n) == nullptr;
#else
  (void)a; (void)n;
  return true;
#endif
}
extern "C" void fake_draw_expect(const uint8_t* seed40) {
  std::lock_guard<std::mutex> lk(mu);
  memcpy(expect40, seed40, 40);
  jobs_seen = jobs_with_seed = ranges_gone = 0;
  touched.clear();
}
extern "C" uint64_t fake_draw_jobs(int with_seed) { std::lock_guard<std::mutex> lk(mu); return with_seed ? jobs_with_seed : jobs_seen; }
// how often the 32 seed bytes occur in the ranges the draws touched since fake_draw_expect
extern "C" uint64_t fake_draw_seed_left(void) {
  std::lock_guard<std::mutex> lk(mu);
  uint64_t found = 0;
  ranges_gone = 0;
  for (const auto& r : touched) {
    if (!still_there(r.first, r.second)) { ranges_gone++; continue; }
    for (size_t k = 0; k + 32 <= r.second; k++) found += memcmp(r.first + k, expect40, 32) == 0;
  }
  return found;
}
// how many of those ranges the last fake_draw_seed_left() could not read any more
extern "C" uint64_t fake_draw_ranges_gone(void) { std::lock_guard<std::mutex> lk(mu); return ranges_gone; }

hipError_t afxk_draw(hipStream_t, const afx_draw_job* jobs, uint32_t njobs, uint32_t max_count) {
  std::lock_guard<std::mutex> lk(mu);
  for (uint32_t r = 0; r < njobs; r++) {
    const afx_draw_job& j = jobs[r];
    if (!j.seed || !j.dst || j.count == 0 || j.count > max_count || ((uintptr_t)j.seed & 7u) || ((uintptr_t)j.dst & 15u)) return hipErrorInvalidValue;
    const size_t len = (size_t)j.count * AFX_DRAW_LEN(j.label);
    jobs_seen++;
    jobs_with_seed += memcmp(j.seed, expect40, 40) == 0;
    memset(j.dst, 0xD7, len);
    touch(j.seed, 40);
    touch(j.dst, len);
  }
  return hipSuccess;
}
