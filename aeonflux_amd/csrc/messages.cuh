// Whole messages (include/aeonflux_gpu.h "whole messages"; plan.h afx_gather_job ..): the kernels between a batch of byte strings of
// any length and the 30-byte chunk rows the plaintext, encryption and decryption plans run on, and k_encode_at, the candidate at a
// known counter.  Included by kernels.hip behind k_encode_to_group (load_msg30, encode_candidate, enc_store, row_job).
//   Plaintext::from_slice            src/symmetric.rs:118-133 (chunks(30), the last one zero-padded)
//   impl From<&RistrettoPoint>       src/symmetric.rs:152-161
//   "shortcut if counter is known"   src/encoding.rs:54
#pragma once

// The message of chunk c: the i with chunk_first[i] <= c < chunk_first[i + 1] (empty messages repeat an entry and are skipped).
// chunk_first[0] = 0 <= c < n_chunks = chunk_first[count]; every index read lies in [0, count] whatever the table holds.  The
// lengths are public, and the lanes of a wave walk almost the same path: the loads hit the same few cache lines.
AFX_DEV uint32_t chunk_message(const uint32_t* __restrict__ chunk_first, uint32_t count, uint32_t c) {
  uint32_t lo = 0, hi = count;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (chunk_first[mid] <= c) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(AFX_BLOCK) k_msg_gather(const afx_gather_job job) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= job.n_chunks) return;
  const uint32_t i = chunk_message(job.chunk_first, job.count, c);
  const uint64_t at = job.offsets[i] + 30ull * (c - job.chunk_first[i]), end = job.offsets[i + 1];
  const uint32_t n = at >= end ? 0u : (end - at < 30 ? (uint32_t)(end - at) : 30u);
  const uint8_t* __restrict__ src = job.blob + (at - job.bias);
  uint8_t* __restrict__ dst = job.rows + 30ull * c;
#pragma unroll
  for (uint32_t b = 0; b < 30; b++) dst[b] = b < n ? src[b] : (uint8_t)0;
}

__global__ void __launch_bounds__(AFX_BLOCK) k_msg_expand(const afx_expand_job job) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= job.n_chunks) return;
  const uint32_t i = chunk_message(job.chunk_first, job.count, c);
#pragma unroll
  for (uint32_t k = 0; k < AFX_EXPAND_MAX; k++) {
    if (k >= job.n_rows) break;   // (uniform)
    const uint4* s = reinterpret_cast<const uint4*>(job.src[k] + 32ull * i);
    uint4* d = reinterpret_cast<uint4*>(job.dst[k] + 32ull * c);
    const uint4 a = s[0], b = s[1];
    d[0] = a;
    d[1] = b;
  }
}

__global__ void __launch_bounds__(AFX_BLOCK) k_msg_status(const afx_msgstat_job job) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (job.phase == 0) {   // (uniform)
    if (c < job.count) {
      bool bad_key = false;
#pragma unroll
      for (uint32_t k = 0; k < AFX_EXPAND_MAX; k++)
        if (k < job.n_keys && !sc_is_canonical(sc_load_item(job.keys[k], 32, c))) bad_key = true;
      if (bad_key) job.status[c] = (uint8_t)job.fail_code;
    }
    if (c < job.n_chunks && (job.chunk_status[0][c] | (job.chunk_status[1] ? job.chunk_status[1][c] : (uint8_t)0)) != 0)
      job.status[chunk_message(job.chunk_first, job.count, c)] = (uint8_t)job.fail_code;
    return;
  }
  if (c >= job.n_chunks) return;
  if (job.status[chunk_message(job.chunk_first, job.count, c)] == 0) return;
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int k = 0; k < 2; k++)
    if (job.rows32[k]) {
      uint4* cell = reinterpret_cast<uint4*>(job.rows32[k] + 32ull * c);
      cell[0] = z;
      cell[1] = z;
    }
  if (job.rows30) {   // rows of 30 bytes are 2-byte aligned at best
    uint8_t* r = job.rows30 + 30ull * c;
#pragma unroll
    for (int b = 0; b < 30; b++) r[b] = 0;
  }
  if (job.words) job.words[c] = 0u;
}

// encode_to_group at a counter the caller kept (k_encode_to_group's body for one candidate): the message is read again for the
// candidate that is written out, as there, so that nothing but the decoding's own values lives across the square-root chain.
__global__ void __launch_bounds__(AFX_BLOCK, 2) k_encode_at(const afx_encode_at_job* __restrict__ jobs, const afx_row* __restrict__ rows, const afx_pass* __restrict__ passes) {
  const afx_encode_at_job job = *row_job(jobs, rows);
  const afx_pass pass = passes[row_pass_index(rows)];
  const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= pass.count) return;
  const uint8_t* m = job.msgs + 30ull * item;
  const uint32_t ctr = job.counters_in[item];
  bool ok;
  {
    uint32_t mw[8], w[8];
    load_msg30(mw, m);
    encode_candidate(w, mw, ctr & 8191u);
    ge_p3 P;
    ok = ristretto_decode(P, w);
  }
  ok = ok && ctr < 128u * 64u;
  uint32_t w[8];
  if (ok) {
    uint32_t mw[8];
    load_msg30(mw, m);
    encode_candidate(w, mw, ctr);
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = 0;
    atomicOr(&pass.bad[item], AFX_BAD_DECODE);
    if (job.zero_a) enc_store(job.zero_a, item, w);
    if (job.zero_b) enc_store(job.zero_b, item, w);
  }
  enc_store(job.M1, item, w);
}

hipError_t afxk_msg_gather(hipStream_t s, const afx_gather_job* job) {
  if (!job->n_chunks) return hipSuccess;
  hipLaunchKernelGGL(k_msg_gather, dim3((job->n_chunks + AFX_BLOCK - 1) / AFX_BLOCK), dim3(AFX_BLOCK), 0, s, *job);
  return hipGetLastError();
}
hipError_t afxk_msg_expand(hipStream_t s, const afx_expand_job* job) {
  if (!job->n_chunks || !job->n_rows) return hipSuccess;
  hipLaunchKernelGGL(k_msg_expand, dim3((job->n_chunks + AFX_BLOCK - 1) / AFX_BLOCK), dim3(AFX_BLOCK), 0, s, *job);
  return hipGetLastError();
}
// both phases, in stream order (the caller has zeroed job->status in front)
hipError_t afxk_msg_status(hipStream_t s, const afx_msgstat_job* job) {
  afx_msgstat_job j = *job;
  const uint32_t lanes0 = j.n_chunks > j.count ? j.n_chunks : j.count;
  if (!lanes0) return hipSuccess;
  j.phase = 0;
  hipLaunchKernelGGL(k_msg_status, dim3((lanes0 + AFX_BLOCK - 1) / AFX_BLOCK), dim3(AFX_BLOCK), 0, s, j);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !j.n_chunks) return e;
  j.phase = 1;
  hipLaunchKernelGGL(k_msg_status, dim3((j.n_chunks + AFX_BLOCK - 1) / AFX_BLOCK), dim3(AFX_BLOCK), 0, s, j);
  return hipGetLastError();
}
hipError_t afxk_encode_at(hipStream_t s, const afx_encode_at_job* jobs, uint32_t njobs, const afx_row* rows, const afx_pass* passes, uint32_t max_count) {
  hipLaunchKernelGGL(k_encode_at, grid_for(max_count, njobs), dim3(block_for(max_count)), 0, s, jobs, rows, passes);
  return hipGetLastError();
}
