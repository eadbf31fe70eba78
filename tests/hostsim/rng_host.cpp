// The device draw (aeonflux_amd/csrc/keccak.cuh shake256_draw, what k_draw runs per lane) compiled for the host, so that the CPU
// test-suite checks it against hashlib's SHAKE256 without a GPU (tests/test_device_rng_on_host.py).  Test infrastructure only.
#include <stdint.h>
#include <string.h>
#include "../../aeonflux_amd/csrc/keccak.cuh"
#include "../../aeonflux_amd/csrc/plan.h"

extern "C" {
// out = draw(seed, stream, index, label): AFX_DRAW_LEN(label) bytes; returns that length
uint32_t rng_host_draw(uint8_t* out, const uint8_t seed[32], uint64_t stream, uint64_t index, uint32_t label) {
  uint8_t staged[40];   // seed || u64le(stream), as the engine stages it
  memcpy(staged, seed, 32);
  for (int b = 0; b < 8; b++) staged[32 + b] = (uint8_t)(stream >> (8 * b));
  uint64_t ss[5], d[8];
  for (int k = 0; k < 5; k++) {
    ss[k] = 0;
    for (int b = 0; b < 8; b++) ss[k] |= (uint64_t)staged[8 * k + b] << (8 * b);
  }
  shake256_draw(d, ss, index, label);
  const uint32_t len = AFX_DRAW_LEN(label);
  for (uint32_t b = 0; b < len; b++) out[b] = (uint8_t)(d[b / 8] >> (8 * (b % 8)));
  return len;
}
}
