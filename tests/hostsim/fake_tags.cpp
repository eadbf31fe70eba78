// Host stand-ins for the three launchers of the presentation tags (aeonflux_amd/csrc/tags.cuh), which tests/hostsim/fake_hip.cpp does
// not have: the engine's host sources reach them through weak references, and only the host simulation of
// tests/test_hostsim_tagged.py links this file.  Like the other stubs they do not do the kernels' arithmetic
// (tests/test_scinv_on_host.py runs the inversion itself on the host): they touch the first and last byte of every array they are
// given, so that ASan sees a pointer the caller got wrong, fill their outputs with something recognisable, and count their launches.
//   afxk_sc_invert        out rows = the scalar 1
//   afxk_tag_broadcast    the kernel's own work: a copy of the 32 bytes into every cell; the bytes it was given are kept
//                         (fake_tags_last_broadcast): what the lane's buffer held as H when the cells were made
//   afxk_tag_scope_check  NOT a ristretto255 decoding: ok = the 32 bytes are a canonical, non-negative field element (below 2^255 - 19,
//                         lowest bit clear) - the first two of the decoding's three conditions, enough to tell 32 bytes of 0xff from a
//                         generator's encoding
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>

static volatile uint8_t sink;
static uint64_t seen[3] = { 0, 0, 0 };
static uint64_t inverted_items = 0;
extern "C" uint64_t fake_tags_launches(int which, int reset) { const uint64_t m = seen[which]; if (reset) seen[which] = 0; return m; }
extern "C" uint64_t fake_tags_inverted_items(void) { return inverted_items; }
static uint8_t last_broadcast[32];
extern "C" void fake_tags_last_broadcast(uint8_t out[32]) { memcpy(out, last_broadcast, 32); }
static void touch(const uint8_t* p, size_t bytes) { if (p && bytes) { sink = p[0]; sink = p[bytes - 1]; } }

hipError_t afxk_sc_invert(hipStream_t, const uint8_t* a, const uint8_t* b, uint8_t* out, uint32_t count) {
  if (count == 0) return hipSuccess;
  if (!a || !b || !out || ((uintptr_t)out & 15u)) return hipErrorInvalidValue;
  seen[0]++;
  inverted_items += count;
  touch(a, 32 * (size_t)count);
  touch(b, 32 * (size_t)count);
  memset(out, 0, 32 * (size_t)count);
  for (uint32_t i = 0; i < count; i++) out[32 * (size_t)i] = 1;
  return hipSuccess;
}
hipError_t afxk_tag_broadcast(hipStream_t, const uint8_t* enc, uint8_t* rows, uint32_t count) {
  if (count == 0) return hipSuccess;
  if (!enc || !rows || ((uintptr_t)enc & 15u) || ((uintptr_t)rows & 15u)) return hipErrorInvalidValue;
  seen[1]++;
  memcpy(last_broadcast, enc, 32);
  for (uint32_t i = 0; i < count; i++) memcpy(rows + 32 * (size_t)i, enc, 32);
  return hipSuccess;
}
hipError_t afxk_tag_scope_check(hipStream_t, const uint8_t* enc, uint8_t* ok) {
  if (!enc || !ok) return hipErrorInvalidValue;
  seen[2]++;
  static const uint8_t P[32] = { 0xed, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff,
                                 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0x7f };
  bool below = false;
  for (int i = 31; i >= 0; i--)
    if (enc[i] != P[i]) { below = enc[i] < P[i]; break; }
  ok[0] = (below && !(enc[0] & 1u)) ? 1 : 0;
  return hipSuccess;
}
