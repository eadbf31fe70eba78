// Host stand-ins for the two launchers of the spent-tag set (aeonflux_amd/csrc/tagset.cuh afxk_tagset_spend, afxk_tagset_contains),
// which tests/hostsim/fake_hip.cpp does not have: tagset.cpp reaches them through weak references, and only the host simulation of
// tests/test_hostsim_tagset.py links this file.  UNLIKE the other stand-ins these compute: they run the REAL lane bodies of tagset.cuh's
// host branch (tagset_claim_item, tagset_resolve_item, tagset_contains_item), item by item in a seeded shuffled order - the claim
// items, then the resolve items, then the size word, as the two launches on a stream do - on whatever pointers tagset.cpp hands them.
// So a whole afx_tagset_* call can be compared with a std::set loop, and a scratch layout that overlaps or overruns shows as a wrong
// answer or under ASan ("device" memory is the fake runtime's calloc).  Like k_tagset_claim and its siblings, an item does nothing once
// the table's error word is set.
//
// Knobs for the driver (fake_tagset_set):
//   "fail_next"   the next launcher call returns hipErrorLaunchFailure and runs nothing
//   "error_next"  the next launcher call sets the table's error word before its items run (what a probe over a full table does)
// fake_tagset_launches(which): launcher calls so far, 0 = spend, 1 = contains.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <vector>
#include "../../aeonflux_amd/csrc/tagset.cuh"
#include "../../aeonflux_amd/csrc/kernels.h"

static int g_fail_next = 0, g_error_next = 0;
static uint64_t g_launches[2] = { 0, 0 };
extern "C" void fake_tagset_set(const char* what, int v) {
  if (!strcmp(what, "fail_next")) g_fail_next = v;
  else if (!strcmp(what, "error_next")) g_error_next = v;
}
extern "C" uint64_t fake_tagset_launches(int which) { return g_launches[which]; }

static std::vector<uint32_t> shuffled(uint32_t count, uint64_t phase) {
  std::vector<uint32_t> o(count);
  for (uint32_t i = 0; i < count; i++) o[i] = i;
  std::mt19937_64 g(0x7a675e7ull + 1000003ull * (g_launches[0] + g_launches[1]) + phase);
  std::shuffle(o.begin(), o.end(), g);
  return o;
}
// what every launcher call starts with; true: the call goes on
static bool begin(const afx_tagset_table* t, int which, hipError_t* rc) {
  g_launches[which]++;
  if (g_fail_next > 0) { g_fail_next--; *rc = hipErrorLaunchFailure; return false; }
  if (g_error_next > 0) { g_error_next--; t->words[1] |= 1ull; }
  return true;
}

hipError_t afxk_tagset_spend(hipStream_t, const afx_tagset_table* t, const uint8_t* T, const uint8_t* status_in, uint32_t count, uint32_t* slot_of, uint8_t* seen_out) {
  if (count == 0) return hipSuccess;
  if (!t || !T || !slot_of || !seen_out || ((uintptr_t)T & 15u) || ((uintptr_t)slot_of & 3u)) return hipErrorInvalidValue;
  hipError_t rc = hipSuccess;
  if (!begin(t, 0, &rc)) return rc;
  for (uint32_t i : shuffled(count, 1))
    if (t->words[1] == 0) tagset_claim_item(*t, T, status_in, count, i, slot_of);
  unsigned long long inserted = 0;
  for (uint32_t i : shuffled(count, 2))
    if (t->words[1] == 0 && tagset_resolve_item(*t, T, i, slot_of, seen_out)) inserted++;
  TS_ADD(&t->words[0], inserted);
  return hipSuccess;
}
hipError_t afxk_tagset_contains(hipStream_t, const afx_tagset_table* t, const uint8_t* T, uint32_t count, uint8_t* seen_out) {
  if (count == 0) return hipSuccess;
  if (!t || !T || !seen_out || ((uintptr_t)T & 15u)) return hipErrorInvalidValue;
  hipError_t rc = hipSuccess;
  if (!begin(t, 1, &rc)) return rc;
  for (uint32_t i : shuffled(count, 3))
    if (t->words[1] == 0) tagset_contains_item(*t, T, i, seen_out);
  return hipSuccess;
}
