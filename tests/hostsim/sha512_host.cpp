// SHA-512 and encode_to_group's candidate writer (aeonflux_amd/csrc/sha512.cuh, what k_sha512 and k_encode_to_group run per lane)
// compiled for the host, so that the CPU test-suite checks them against hashlib without a GPU (tests/test_sha512_on_host.py).
// Test infrastructure only.
#include <stdint.h>
#include <string.h>
#include "../../aeonflux_amd/csrc/sha512.cuh"

extern "C" {
// out = SHA-512(msg[0 .. len)); aligned != 0: the dword path (msg must then be 4-byte aligned)
void sha512_host(uint8_t out[64], const uint8_t* msg, uint32_t len, int aligned) {
  uint64_t h[8];
  if (aligned) sha512_words<true>(h, msg, len);
  else sha512_words<false>(h, msg, len);
  uint32_t d[16];
  sha512_digest_dwords(d, h);
  for (int i = 0; i < 16; i++)
    for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(d[i] >> (8 * b));
}
// out = candidate `ctr` of the 30-byte message
void candidate_host(uint8_t out[32], const uint8_t msg[30], uint32_t ctr) {
  uint8_t padded[32] = { 0 };
  memcpy(padded, msg, 30);
  padded[30] = 0xa5; padded[31] = 0x5a;   // the writer must ignore these
  uint32_t mw[8], w[8];
  for (int i = 0; i < 8; i++) mw[i] = (uint32_t)padded[4 * i] | ((uint32_t)padded[4 * i + 1] << 8) | ((uint32_t)padded[4 * i + 2] << 16) | ((uint32_t)padded[4 * i + 3] << 24);
  encode_candidate(w, mw, ctr);
  for (int i = 0; i < 8; i++)
    for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(w[i] >> (8 * b));
}
}
