// Kernels of the presentation tags (include/aeonflux_gpu.h "Presentation tags"): a tagged show carries T = (m + n)^-1 * H for a hidden
// scalar attribute m, a public per-item counter n and a per-call scope generator H.  The one computation the rest of the engine
// cannot do is the inverse mod l: k_sc_invert makes it, one lane per item, ONCE per call and in front of the call's passes (the way
// k_batch_weights runs, statements.cpp draw_weights); the passes read its output rows as ordinary per-item scalars.
// k_tag_broadcast writes the call's H into one 32-byte cell per item, so that the plans decode it like any per-item encoding.
//
// The inversion is Fermat's, s^(l - 2), by square-and-multiply over the bits of the PUBLIC exponent: the branch on an exponent bit is
// wave-uniform, the instruction stream and every address are the same for every s (s is secret-derived), and no array is indexed by a
// runtime value, so nothing goes to scratch (tests/test_kernel_isa_tags.py).  The loop stays rolled: sc_mul is inlined twice, not 300
// times.
//
// The arithmetic (tag_sum, sc_invert, tag_inverse_row) is plain C++ on sc.cuh: tests/hostsim/scinv_host.cpp compiles these very
// statements for the host and compares them with Python integers.  The kernels and their launchers need the HIP compiler.
#pragma once
#include <hip/hip_runtime.h>
#include "sc.cuh"
#include "plan.h"

// l - 2, little-endian words: bit 252 and 72 of the 125 bits below it are set
__device__ __constant__ const uint32_t SC_L_MINUS_2[8] = { 0x5cf5d3ebu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0u, 0u, 0u, 0x10000000u };

// a^(l - 2) mod l: the inverse of a canonical a != 0, and 0 for a == 0.  252 squarings and one product per set bit below the top one.
AFX_DEV sc sc_invert(const sc& a) {
  sc r = a;   // bit 252
#pragma unroll 1
  for (int bit = 251; bit >= 0; bit--) {
    r = sc_mul(r, r);
    if ((SC_L_MINUS_2[bit >> 5] >> (bit & 31)) & 1u) r = sc_mul(r, a);
  }
  return r;
}

// a + b mod l for any two 256-bit values (the sum has 257 bits; one reduction)
AFX_DEV sc tag_sum(const sc& a, const sc& b) {
  uint32_t wide[16];
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)a.v[i] + b.v[i];
    wide[i] = (uint32_t)c;
    c >>= 32;
  }
  wide[8] = (uint32_t)c;
#pragma unroll
  for (int i = 9; i < 16; i++) wide[i] = 0;
  return sc_reduce512(wide);
}

// One item's output row: (a + b)^-1 mod l, or l itself when a + b == 0 (mod l) - the smallest value that is no canonical scalar: the
// pass's canonicity test of the row (an afx_sccheck_job) fails the item, no second flag array is needed, and a chain that still runs
// on the row reads a 253-bit value like any other.  The same instructions either way (the inverse of 0 comes out as 0).
AFX_DEV sc tag_inverse_row(const sc& a, const sc& b) {
  const sc s = tag_sum(a, b);
  sc r = sc_invert(s);
  uint32_t nz = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) nz |= s.v[i];
  const uint32_t none = nz ? 0u : 0xffffffffu;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] |= none & SC_L[i];
  return r;
}

#if defined(__HIPCC__)
#include "ge.cuh"
#include "kernels.h"

// One lane per item: out[item] = tag_inverse_row(a[item], b[item]); all three [count][32], out 16-byte aligned
__global__ void __launch_bounds__(AFX_BLOCK) k_sc_invert(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint8_t* __restrict__ out, uint32_t count) {
  const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= count) return;
  const sc r = tag_inverse_row(sc_load(a + (uint64_t)item * 32), sc_load(b + (uint64_t)item * 32));
  uint4* dst = reinterpret_cast<uint4*>(out + (uint64_t)item * 32);
  dst[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
  dst[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
}

// One lane per item: rows[item] = the 32 bytes at `enc` (both 16-byte aligned)
__global__ void __launch_bounds__(AFX_BLOCK) k_tag_broadcast(const uint8_t* __restrict__ enc, uint8_t* __restrict__ rows, uint32_t count) {
  const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= count) return;
  const uint4* src = reinterpret_cast<const uint4*>(enc);
  uint4* dst = reinterpret_cast<uint4*>(rows + (uint64_t)item * 32);
  dst[0] = src[0];
  dst[1] = src[1];
}

// One lane: ok[0] = 1 when the 32 bytes at `enc` (4-byte aligned) decode to a ristretto255 point - the test k_decode runs - else 0
__global__ void k_tag_scope_check(const uint8_t* __restrict__ enc, uint8_t* __restrict__ ok) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t* q = reinterpret_cast<const uint32_t*>(enc);
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = q[i];
  ge_p3 P;
  ok[0] = ristretto_decode(P, w) ? 1 : 0;
}

hipError_t afxk_tag_scope_check(hipStream_t s, const uint8_t* enc, uint8_t* ok) {
  hipLaunchKernelGGL(k_tag_scope_check, dim3(1), dim3(64), 0, s, enc, ok);
  return hipGetLastError();
}
hipError_t afxk_sc_invert(hipStream_t s, const uint8_t* a, const uint8_t* b, uint8_t* out, uint32_t count) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sc_invert, dim3((count + AFX_BLOCK - 1) / AFX_BLOCK), dim3(AFX_BLOCK), 0, s, a, b, out, count);
  return hipGetLastError();
}
hipError_t afxk_tag_broadcast(hipStream_t s, const uint8_t* enc, uint8_t* rows, uint32_t count) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_tag_broadcast, dim3((count + AFX_BLOCK - 1) / AFX_BLOCK), dim3(AFX_BLOCK), 0, s, enc, rows, count);
  return hipGetLastError();
}
#endif   // __HIPCC__
