// TEST INFRASTRUCTURE (CPU only): the host stand-in for the one kernel launcher the serialized issuance path adds
// (kernels.hip k_soa_to_aos), linked beside fake_hip.cpp by tests/test_request_wire_fuzz.py.  Like the fake afxk_aos_to_soa it
// moves the bytes for real: rows [row][count][32] -> records of `cells` cells, zeros for an item whose status byte is not 0.
#include <string.h>
#include "../../aeonflux_amd/csrc/kernels.h"

hipError_t afxk_soa_to_aos(hipStream_t, const uint8_t* soa, uint8_t* rec, const uint32_t* m, const uint8_t* status, uint32_t cells, uint32_t n) {
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t c = 0; c < cells; c++) {
      uint8_t* dst = rec + ((size_t)i * cells + c) * 32;
      if (status && status[i]) memset(dst, 0, 32);
      else memcpy(dst, soa + ((size_t)m[c] * n + i) * 32, 32);
    }
  return hipSuccess;
}
