// Kernels of the batchable presentation proofs (include/aeonflux_gpu.h "Batchable presentation proofs"): the verifier checks all the
// constraints of a presentation's proofs with ONE weighted sum per item,
//     sum_j rho_j * ( sum_s resp_s * P_(j,s) - c * LHS_j - R_j ) == identity,
// and these two kernels make its scalars: k_batch_weights draws the 128-bit rho_j of every (item, proof, constraint) once, k_coef
// folds them with the responses and challenges into one coefficient per distinct base (plan.h afx_coef_job).  The sum itself runs
// on the multiscalar kernels of kernels.hip, which includes this file at its end (one code object per library).
//
// Neither kernel uses LDS or scratch: every array below is indexed by unrolled loops only (tests/test_kernel_isa_batchable.py).
//
// The arithmetic of one coefficient (coef_mac, coef_item) is plain C++ on sc.cuh and plan.h: tests/hostsim/coef_host.cpp compiles these
// very statements for the host and compares them with Python integers.  The kernels and their launchers need the HIP compiler.
#pragma once
#include <hip/hip_runtime.h>
#include "sc.cuh"
#include "plan.h"

// acc (13 limbs) += rho (4 limbs) * x (8 limbs)
AFX_DEV void coef_mac(uint32_t acc[13], const uint32_t rho[4], const uint32_t x[8]) {
  uint32_t p[12];
  mp_mul<4, 8>(p, rho, x);
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 13; i++) {
    c += (uint64_t)acc[i] + (i < 12 ? p[i] : 0u);
    acc[i] = (uint32_t)c;
    c >>= 32;
  }
}

// One output scalar of one item (plan.h afx_coef_job).  Positive and negative triples are summed apart as plain integers (a product
// has 384 bits, a sum of 2^16 of them 400: 13 limbs), each sum is reduced once, and the output is their difference mod l: three
// reductions per output whatever the number of triples.
AFX_DEV sc coef_item(const afx_coef_job& job, uint32_t item) {
  uint32_t pos[13], neg[13];
#pragma unroll
  for (int i = 0; i < 13; i++) pos[i] = neg[i] = 0;
#pragma unroll 1
  for (uint32_t t = 0; t < job.n_triples; t++) {
    const afx_coef_triple tr = job.triples[t];
    const uint4 r = *reinterpret_cast<const uint4*>(job.weights + ((uint64_t)tr.weight * job.stride + item) * AFX_WEIGHT_BYTES);
    const uint32_t rho[4] = { r.x, r.y, r.z, r.w };
    uint32_t x[8] = { 1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
    if (tr.operand != AFX_COEF_ONE) {
      const sc v = sc_load(job.operands[tr.operand] + (uint64_t)item * 32);   // (a caller's array: 4-byte aligned is all it promises)
#pragma unroll
      for (int i = 0; i < 8; i++) x[i] = v.v[i];
    }
    if (tr.negate) coef_mac(neg, rho, x);
    else coef_mac(pos, rho, x);
  }
  uint32_t wide[16];
#pragma unroll
  for (int i = 0; i < 16; i++) wide[i] = i < 13 ? pos[i] : 0u;
  const sc p = sc_reduce512(wide);
#pragma unroll
  for (int i = 0; i < 16; i++) wide[i] = i < 13 ? neg[i] : 0u;
  const sc n = sc_reduce512(wide);
  // p + (l - n) < 2 l
  uint64_t c = 0;
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)SC_L[i] - n.v[i] - borrow;
    borrow = (uint32_t)(d >> 63);
    c += (uint64_t)p.v[i] + (uint32_t)d;
    wide[i] = (uint32_t)c;
    c >>= 32;
  }
  wide[8] = (uint32_t)c;
#pragma unroll
  for (int i = 9; i < 16; i++) wide[i] = 0;
  return sc_reduce512(wide);
}

#if defined(__HIPCC__)
#include "keccak.cuh"
#include "kernels.h"

// One lane per item: the item's weights are the first 16 * n_weights bytes of draw(seed, stream, index0 + item, label) - SHAKE256
// squeezed over as many blocks of its 136-byte rate as that takes - written as weights[w][item] (16 bytes each, 8-byte stores: a
// weight can straddle two blocks).  `seed`: the 40 staged bytes seed || u64le(stream), 8-byte aligned.
__global__ void __launch_bounds__(AFX_BLOCK) k_batch_weights(const uint8_t* __restrict__ seed, uint64_t index0, uint32_t label, uint32_t n_weights,
                                                             uint32_t count, uint8_t* __restrict__ weights) {
  const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= count) return;
  const uint2* sp = reinterpret_cast<const uint2*>(seed);
  uint64_t ss[5];
#pragma unroll
  for (int k = 0; k < 5; k++) { const uint2 v = sp[k]; ss[k] = (uint64_t)v.x | ((uint64_t)v.y << 32); }
  // 64-bit word k of the draw is half (k & 1) of weight k >> 1
  shake256_draw_words(ss, index0 + item, label, 2 * n_weights, [&](uint32_t k, uint64_t word) {
    uint2* dst = reinterpret_cast<uint2*>(weights + ((uint64_t)(k >> 1) * count + item) * AFX_WEIGHT_BYTES + 8 * (k & 1));
    *dst = make_uint2((uint32_t)word, (uint32_t)(word >> 32));
  });
}

// One grid row per output scalar, one lane per item (plan.h afx_coef_job)
__global__ void __launch_bounds__(AFX_BLOCK) k_coef(const afx_coef_job* __restrict__ jobs, const afx_row* __restrict__ rows, const afx_pass* __restrict__ passes) {
  const afx_coef_job job = *row_job(jobs, rows);
  const uint32_t count = passes[row_pass_index(rows)].count;   // wave-uniform: scalar loads
  const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= count) return;
  const sc out = coef_item(job, item);
  uint4* dst = reinterpret_cast<uint4*>(job.out + (uint64_t)item * 32);
  dst[0] = make_uint4(out.v[0], out.v[1], out.v[2], out.v[3]);
  dst[1] = make_uint4(out.v[4], out.v[5], out.v[6], out.v[7]);
}

hipError_t afxk_batch_weights(hipStream_t s, const uint8_t* seed, uint64_t index0, uint32_t label, uint32_t n_weights, uint32_t count, uint8_t* weights) {
  if (count == 0 || n_weights == 0) return hipSuccess;
  hipLaunchKernelGGL(k_batch_weights, dim3((count + AFX_BLOCK - 1) / AFX_BLOCK), dim3(AFX_BLOCK), 0, s, seed, index0, label, n_weights, count, weights);
  return hipGetLastError();
}
hipError_t afxk_coef(hipStream_t s, const afx_coef_job* jobs, uint32_t njobs, const afx_row* rows, const afx_pass* passes, uint32_t max_count) {
  if (njobs == 0 || max_count == 0) return hipSuccess;
  const uint32_t block = block_for(max_count);
  hipLaunchKernelGGL(k_coef, dim3((max_count + block - 1) / block, njobs), dim3(block), 0, s, jobs, rows, passes);
  return hipGetLastError();
}
#endif   // __HIPCC__
