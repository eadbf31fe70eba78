// Host stand-ins for the four launchers of the whole-message calls (aeonflux_amd/csrc/messages.cuh: k_encode_at, k_msg_gather,
// k_msg_expand, k_msg_status), which tests/hostsim/fake_hip.cpp does not have: the engine's host sources reach them through weak
// references, and only the host simulation of tests/test_launch_kinds_host.py links this file.  Like the other stubs they compute
// nothing; they touch the first and last byte of every array a job names, so that a pointer the plan got wrong is read, and count
// their launches (fake_messages_launches).
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "../../aeonflux_amd/csrc/plan.h"

static volatile uint8_t sink;
static uint32_t launches[4];
extern "C" uint32_t fake_messages_launches(int which, int reset) { const uint32_t m = launches[which]; if (reset) launches[which] = 0; return m; }
static void touch(const void* q, size_t bytes) { const uint8_t* p = (const uint8_t*)q; if (p && bytes) { sink = p[0]; sink = p[bytes - 1]; } }
static void mark(void* q, size_t bytes) { uint8_t* p = (uint8_t*)q; if (p && bytes) { p[0] = 0; p[bytes - 1] = 0; } }

hipError_t afxk_encode_at(hipStream_t, const afx_encode_at_job* jobs, uint32_t njobs, const afx_row* rows, const afx_pass* passes, uint32_t max_count) {
  launches[0]++;
  for (uint32_t r = 0; r < njobs; r++) {
    const afx_encode_at_job& j = rows ? *(const afx_encode_at_job*)((const uint8_t*)jobs + rows[r].job_off) : jobs[r];
    const afx_pass& P = passes[rows ? rows[r].pass : 0];
    if (P.count == 0 || P.count > max_count || !j.msgs || !j.counters_in || !j.M1 || !P.bad) return hipErrorInvalidValue;
    if (((uintptr_t)j.M1 & 15) != 0 || ((uintptr_t)j.counters_in & 3) != 0) return hipErrorInvalidValue;
    touch(j.msgs, 30 * (size_t)P.count);
    touch(j.counters_in, 4 * (size_t)P.count);
    touch(P.bad, 4 * (size_t)P.count);
    mark(j.M1, 32 * (size_t)P.count);
    mark(j.zero_a, 32 * (size_t)P.count);
    mark(j.zero_b, 32 * (size_t)P.count);
  }
  return hipSuccess;
}
// the chunk table as the kernels read it: chunk_first[0 .. count], nondecreasing, chunk_first[count] = n_chunks
static bool table_ok(const uint32_t* chunk_first, uint32_t count, uint32_t n_chunks) {
  if (!chunk_first) return false;
  touch(chunk_first, 4 * ((size_t)count + 1));
  for (uint32_t i = 0; i < count; i++) if (chunk_first[i] > chunk_first[i + 1]) return false;
  return chunk_first[count] == n_chunks;
}
hipError_t afxk_msg_gather(hipStream_t, const afx_gather_job* job) {
  launches[1]++;
  if (!job->n_chunks) return hipSuccess;
  if (!job->blob || !job->offsets || !job->rows || !table_ok(job->chunk_first, job->count, job->n_chunks)) return hipErrorInvalidValue;
  touch(job->offsets, 8 * ((size_t)job->count + 1));
  if (job->offsets[0] < job->bias || job->offsets[job->count] < job->offsets[0]) return hipErrorInvalidValue;
  touch(job->blob + (job->offsets[0] - job->bias), job->offsets[job->count] - job->offsets[0]);
  mark(job->rows, 30 * (size_t)job->n_chunks);
  return hipSuccess;
}
hipError_t afxk_msg_expand(hipStream_t, const afx_expand_job* job) {
  launches[2]++;
  if (!job->n_chunks || !job->n_rows) return hipSuccess;
  if (job->n_rows > AFX_EXPAND_MAX || !table_ok(job->chunk_first, job->count, job->n_chunks)) return hipErrorInvalidValue;
  for (uint32_t k = 0; k < job->n_rows; k++) {
    if (!job->src[k] || !job->dst[k] || (((uintptr_t)job->src[k] | (uintptr_t)job->dst[k]) & 15) != 0) return hipErrorInvalidValue;
    touch(job->src[k], 32 * (size_t)job->count);
    mark(job->dst[k], 32 * (size_t)job->n_chunks);
  }
  return hipSuccess;
}
hipError_t afxk_msg_status(hipStream_t, const afx_msgstat_job* job) {
  launches[3]++;
  if (!job->n_chunks && !job->count) return hipSuccess;
  if (!job->status || job->n_keys > AFX_EXPAND_MAX) return hipErrorInvalidValue;
  for (uint32_t k = 0; k < job->n_keys; k++) {
    if (!job->keys[k]) return hipErrorInvalidValue;
    touch(job->keys[k], 32 * (size_t)job->count);
  }
  mark(job->status, job->count);
  if (!job->n_chunks) return hipSuccess;
  if (!job->chunk_status[0] || !table_ok(job->chunk_first, job->count, job->n_chunks)) return hipErrorInvalidValue;
  touch(job->chunk_status[0], job->n_chunks);
  touch(job->chunk_status[1], job->n_chunks);
  mark(job->rows32[0], 32 * (size_t)job->n_chunks);
  mark(job->rows32[1], 32 * (size_t)job->n_chunks);
  mark(job->rows30, 30 * (size_t)job->n_chunks);
  mark(job->words, 4 * (size_t)job->n_chunks);
  return hipSuccess;
}
