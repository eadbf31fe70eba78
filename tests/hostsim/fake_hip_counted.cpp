// TEST INFRASTRUCTURE (CPU only): the fake HIP runtime of fake_hip.cpp, unchanged, with two of its entry points counted - what
// tests/hostsim/batch_array_doors.cpp reads to see that a refused call did no device work.  A program links this file INSTEAD of
// fake_hip.cpp: it compiles that file's text with the two definitions under other names and puts counting wrappers in their place.
//   afx_fake_count("copies" | "finishes", reset): asynchronous copies (every upload and fetch) / finishing launches (one per plan) so far
#include <hip/hip_runtime_api.h>
#include <string.h>
#include <atomic>
#include "../../aeonflux_amd/csrc/kernels.h"

#define hipMemcpyAsync fake_uncounted_hipMemcpyAsync
#define afxk_finish fake_uncounted_afxk_finish
#include "fake_hip.cpp"
#undef hipMemcpyAsync
#undef afxk_finish

static std::atomic<unsigned long long> g_copies{ 0 }, g_finishes{ 0 };
extern "C" unsigned long long afx_fake_count(const char* what, int reset) {
  std::atomic<unsigned long long>& c = !strcmp(what, "copies") ? g_copies : g_finishes;
  return reset ? c.exchange(0) : c.load();
}
extern "C" hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind k, hipStream_t st) {
  g_copies++;
  return fake_uncounted_hipMemcpyAsync(d, s, n, k, st);
}
hipError_t afxk_finish(hipStream_t s, const afx_finish_job* jobs, uint32_t njobs, const afx_row* rows, uint32_t max_count) {
  g_finishes++;
  return fake_uncounted_afxk_finish(s, jobs, njobs, rows, max_count);
}
