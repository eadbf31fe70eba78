// The scalar inversion of the presentation tags (aeonflux_amd/csrc/tags.cuh sc_invert, tag_sum and tag_inverse_row: the very statements
// k_sc_invert runs per lane) compiled for the host, so that the CPU test-suite checks them against Python integers without a GPU
// (tests/test_scinv_on_host.py).  Test infrastructure only.
#include <stdint.h>
#include <string.h>
#include "../../aeonflux_amd/csrc/tags.cuh"

extern "C" {
// out = a^(l - 2) mod l, 32 bytes little-endian, for a canonical a
void scinv_host_invert(uint8_t out[32], const uint8_t a[32]) {
  sc x;
  memcpy(x.v, a, 32);
  const sc r = sc_invert(x);
  memcpy(out, r.v, 32);
}
// out = one item's row of k_sc_invert: (a + b)^-1 mod l, or l where a + b == 0 (mod l)
void scinv_host_row(uint8_t out[32], const uint8_t a[32], const uint8_t b[32]) {
  sc x, y;
  memcpy(x.v, a, 32);
  memcpy(y.v, b, 32);
  const sc r = tag_inverse_row(x, y);
  memcpy(out, r.v, 32);
}
}
