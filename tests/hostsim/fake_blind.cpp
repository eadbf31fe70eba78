// Host stand-in for the output-masking launcher (aeonflux_amd/csrc/kernels.hip k_mask_rows), which tests/hostsim/fake_hip.cpp does not
// have: the engine's host sources reach it through a weak reference, and only the host simulation of tests/test_hostsim_blind.py links
// this file.  Unlike the other stubs it does the kernel's work - the simulation's statuses follow the fake kernels' bad words, and a
// failed item's rows must read zero there too - and it counts the rows it was given (fake_mask_rows_seen).
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>
#include "../../aeonflux_amd/csrc/plan.h"

static uint64_t rows_seen = 0;
extern "C" uint64_t fake_mask_rows_seen(int reset) { const uint64_t m = rows_seen; if (reset) rows_seen = 0; return m; }

hipError_t afxk_mask_rows(hipStream_t, const afx_mask_job* jobs, uint32_t njobs, const afx_row* rows, const afx_pass* passes, uint32_t max_count) {
  for (uint32_t r = 0; r < njobs; r++) {
    const afx_mask_job& j = rows ? *(const afx_mask_job*)((const uint8_t*)jobs + rows[r].job_off) : jobs[r];
    const afx_pass& P = passes[rows ? rows[r].pass : 0];
    if (P.count == 0 || P.count > max_count || !j.p || !P.bad || ((uintptr_t)j.p & 15u)) return hipErrorInvalidValue;
    rows_seen++;
    for (uint32_t i = 0; i < P.count; i++) {
      volatile uint8_t first = j.p[32 * (size_t)i], last = j.p[32 * (size_t)i + 31];   // every cell is the pass's to touch
      (void)first; (void)last;
      if (P.bad[i]) memset(j.p + 32 * (size_t)i, 0, 32);
    }
  }
  return hipSuccess;
}
