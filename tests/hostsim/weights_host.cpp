// The weight draw of a batchable verification (aeonflux_amd/csrc/keccak.cuh shake256_draw_words, what k_batch_weights runs per lane)
// compiled for the host, so that the CPU test-suite checks it against hashlib's SHAKE256 without a GPU
// (tests/test_batchable_weights_on_host.py).  Test infrastructure only.
#include <stdint.h>
#include <string.h>
#include "../../aeonflux_amd/csrc/keccak.cuh"
#include "../../aeonflux_amd/csrc/plan.h"

extern "C" {
// out = the n_weights 16-byte weights of item `index`, in order
void weights_host_draw(uint8_t* out, const uint8_t seed[32], uint64_t stream, uint64_t index, uint32_t label, uint32_t n_weights) {
  uint8_t staged[40];   // seed || u64le(stream), as the engine stages it
  memcpy(staged, seed, 32);
  for (int b = 0; b < 8; b++) staged[32 + b] = (uint8_t)(stream >> (8 * b));
  uint64_t ss[5];
  for (int k = 0; k < 5; k++) {
    ss[k] = 0;
    for (int b = 0; b < 8; b++) ss[k] |= (uint64_t)staged[8 * k + b] << (8 * b);
  }
  shake256_draw_words(ss, index, label, 2 * n_weights, [&](uint32_t k, uint64_t word) {
    for (int b = 0; b < 8; b++) out[(size_t)(k >> 1) * AFX_WEIGHT_BYTES + 8 * (k & 1) + b] = (uint8_t)(word >> (8 * b));
  });
}
}
