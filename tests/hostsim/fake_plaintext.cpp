// Host stand-ins for the three launchers of the plaintext path (aeonflux_amd/csrc/sha512.cuh; kernels.hip k_sha512,
// k_encode_to_group), which tests/hostsim/fake_hip.cpp does not have: the engine's host sources reach them through weak references,
// and only the host simulation of tests/test_hostsim_plaintext.py links this file.  Like the other stubs they compute nothing; they
// touch the first and last byte of every array a job names for its pass, so that ASan sees a pointer the plan got wrong, and count
// their launches (fake_plaintext_launches).
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "../../aeonflux_amd/csrc/plan.h"

static volatile uint8_t sink;
static uint32_t launches[3];
extern "C" uint32_t fake_plaintext_launches(int which, int reset) { const uint32_t m = launches[which]; if (reset) launches[which] = 0; return m; }
static void touch(const uint8_t* p, size_t bytes) { if (p && bytes) { sink = p[0]; sink = p[bytes - 1]; } }
static void mark(uint8_t* p, size_t bytes) { if (p && bytes) { p[0] = 0; p[bytes - 1] = 0; } }

static hipError_t hash_job(const afx_sha512_job& j, size_t count) {
  if (!j.src || !j.out || j.len > 1024 || j.pad || (j.stride && j.offset + j.len > j.stride)) return hipErrorInvalidValue;
  if (((uintptr_t)j.out & 15) != 0) return hipErrorInvalidValue;
  if (j.len) touch(j.src + j.offset, (count - 1) * (size_t)j.stride + j.len);
  mark(j.out, 64 * count);
  mark(j.copy, (size_t)j.len * count);
  return hipSuccess;
}
hipError_t afxk_sha512_jobs(hipStream_t, const afx_sha512_job* jobs, uint32_t njobs, const afx_row* rows, const afx_pass* passes, uint32_t max_count) {
  launches[0]++;
  for (uint32_t r = 0; r < njobs; r++) {
    const afx_sha512_job& j = rows ? *(const afx_sha512_job*)((const uint8_t*)jobs + rows[r].job_off) : jobs[r];
    const afx_pass& P = passes[rows ? rows[r].pass : 0];
    if (P.count == 0 || P.count > max_count) return hipErrorInvalidValue;
    const hipError_t e = hash_job(j, P.count);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
hipError_t afxk_sha512(hipStream_t, const uint8_t* src, uint32_t stride, uint32_t offset, uint32_t len, uint8_t* out, uint32_t count) {
  launches[1]++;
  if (!count) return hipSuccess;
  const afx_sha512_job j = { src, out, nullptr, stride, offset, len, 0 };
  return hash_job(j, count);
}
hipError_t afxk_encode_to_group(hipStream_t, const afx_encode_job* jobs, uint32_t njobs, const afx_row* rows, const afx_pass* passes, uint32_t max_count) {
  launches[2]++;
  for (uint32_t r = 0; r < njobs; r++) {
    const afx_encode_job& j = rows ? *(const afx_encode_job*)((const uint8_t*)jobs + rows[r].job_off) : jobs[r];
    const afx_pass& P = passes[rows ? rows[r].pass : 0];
    if (P.count == 0 || P.count > max_count || !j.msgs || !j.M1 || !P.bad) return hipErrorInvalidValue;
    if (((uintptr_t)j.M1 & 15) != 0 || ((uintptr_t)j.counters & 3) != 0) return hipErrorInvalidValue;
    touch(j.msgs, 30 * (size_t)P.count);
    touch((const uint8_t*)P.bad, 4 * (size_t)P.count);
    mark(j.M1, 32 * (size_t)P.count);
    mark((uint8_t*)j.counters, 4 * (size_t)P.count);
    mark(j.zero_a, 32 * (size_t)P.count);
    mark(j.zero_b, 32 * (size_t)P.count);
  }
  return hipSuccess;
}
