// One coefficient of the batchable verification's weighted sum (aeonflux_amd/csrc/batchable.cuh coef_item and coef_mac: the very
// statements k_coef runs per lane) compiled for the host, so that the CPU test-suite checks them against Python integers without a GPU
// (tests/test_batchable_coef_on_host.py).  Test infrastructure only.
#include <stdint.h>
#include <string.h>
#include "../../aeonflux_amd/csrc/batchable.cuh"

static_assert(sizeof(afx_coef_triple) == 8, "the test passes triples as four 16-bit words");

extern "C" {
// out = the job's coefficient of `item`, 32 bytes little-endian.  weights: what afx_coef_job.weights points at ([n_weights][stride][16],
// already offset to the pass's first item); triples: n_triples x (weight, operand, negate, 0); operands: pointers to [count][32] arrays
void coef_host_item(uint8_t out[32], const uint8_t* weights, uint64_t stride, const uint16_t* triples, uint32_t n_triples,
                    const uint8_t* const* operands, uint32_t item) {
  afx_coef_job job;
  memset(&job, 0, sizeof job);
  job.weights = weights;
  job.triples = reinterpret_cast<const afx_coef_triple*>(triples);
  job.operands = operands;
  job.stride = stride;
  job.n_triples = n_triples;
  const sc r = coef_item(job, item);
  memcpy(out, r.v, 32);
}
}
