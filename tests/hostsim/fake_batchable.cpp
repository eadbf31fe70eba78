// Host stand-ins for the two launchers of the batchable verification's coefficient stage (aeonflux_amd/csrc/batchable.cuh), which
// tests/hostsim/fake_hip.cpp does not have: the engine's eight host sources reach them through weak references, and only the
// host simulation of tests/test_hostsim_batchable.py links this file.  Like the other stubs they compute nothing; they touch the
// first and last byte of every array a job names for its pass, so that ASan sees a pointer the plan got wrong.  The one thing they keep
// is the length of the longest coefficient job seen (fake_coef_most_triples), which tests/test_batchable_coef_on_host.py runs for real.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "../../aeonflux_amd/csrc/plan.h"

static volatile uint8_t sink;
static uint32_t most_triples = 0;
extern "C" uint32_t fake_coef_most_triples(int reset) { const uint32_t m = most_triples; if (reset) most_triples = 0; return m; }
static void touch(const uint8_t* p, size_t bytes) { if (p && bytes) { sink = p[0]; sink = p[bytes - 1]; } }

hipError_t afxk_batch_weights(hipStream_t, const uint8_t* seed, uint64_t, uint32_t label, uint32_t n_weights, uint32_t count, uint8_t* weights) {
  if (!seed || !weights || label != 64u) return hipErrorInvalidValue;
  touch(seed, 40);
  for (size_t i = 0; i < (size_t)n_weights * count * AFX_WEIGHT_BYTES; i++) weights[i] = (uint8_t)(i * 151u + 7u);
  return hipSuccess;
}
hipError_t afxk_coef(hipStream_t, const afx_coef_job* jobs, uint32_t njobs, const afx_row* rows, const afx_pass* passes, uint32_t max_count) {
  for (uint32_t r = 0; r < njobs; r++) {
    const afx_coef_job& j = rows ? *(const afx_coef_job*)((const uint8_t*)jobs + rows[r].job_off) : jobs[r];
    const afx_pass& P = passes[rows ? rows[r].pass : 0];
    if (P.count == 0 || P.count > max_count || !j.out || !j.weights || !j.triples || j.n_triples == 0 || j.stride < P.count) return hipErrorInvalidValue;
    if (j.n_triples > most_triples) most_triples = j.n_triples;
    for (uint32_t t = 0; t < j.n_triples; t++) {
      const afx_coef_triple& tr = j.triples[t];
      touch(j.weights + (size_t)tr.weight * j.stride * AFX_WEIGHT_BYTES, (size_t)P.count * AFX_WEIGHT_BYTES);
      if (tr.operand != AFX_COEF_ONE) touch(j.operands[tr.operand], 32 * (size_t)P.count);
      if (tr.negate > 1 || tr.pad) return hipErrorInvalidValue;
    }
    j.out[0] = 1; j.out[32 * (size_t)P.count - 1] = 0;
  }
  return hipSuccess;
}
