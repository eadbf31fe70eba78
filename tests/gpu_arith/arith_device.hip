// The device twin of tests/hostsim/arith_host.cpp: the engine's arithmetic headers (fe.cuh, fe10.cuh, ge.cuh, sc.cuh) compiled
// by hipcc for gfx950 with the flags of the product's kernels.o, AFX_PIN live, and fed chosen limbs - one case of
// tests/arith_cases.py per lane (the case bodies: arith_cases.cuh, shared with the host build).  tests/test_gpu_device_arith.py
// compares what comes back with Python integers, pyref and the oracle, and limb for limb with the bounds-checked host build.
// Test infrastructure only: nothing in the product links this file.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../aeonflux_amd/csrc/ge.cuh"
#include "../../aeonflux_amd/csrc/sc.cuh"
#include "../../aeonflux_amd/csrc/plan.h"
#include "arith_cases.cuh"

// lane = case: NI words in, NO words out, case-major
#define AC_KERNEL(name, body, NI, NO)                                                                                \
  __global__ void __launch_bounds__(AFX_BLOCK) name(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) { \
    const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;                                                     \
    if (item >= n) return;                                                                                           \
    uint32_t a[NI], o[NO];                                                                                           \
    for (int i = 0; i < NI; i++) a[i] = in[(size_t)item * NI + i];                                                   \
    body(a, o);                                                                                                      \
    for (int i = 0; i < NO; i++) out[(size_t)item * NO + i] = o[i];                                                  \
  }

AC_KERNEL(k_fe_limbs, case_fe_limbs, AC_FE_LIMBS_IN, AC_FE_LIMBS_OUT)
AC_KERNEL(k_fe10_limbs, case_fe10_limbs, AC_FE10_LIMBS_IN, AC_FE10_LIMBS_OUT)
AC_KERNEL(k_fe_bytes, case_fe_bytes, AC_FE_BYTES_IN, AC_FE_BYTES_OUT)
AC_KERNEL(k_sqrt_ratio, case_sqrt_ratio, AC_SQRT_RATIO_IN, AC_SQRT_RATIO_OUT)
AC_KERNEL(k_elligator, case_elligator, AC_ELLIGATOR_IN, AC_ELLIGATOR_OUT)
AC_KERNEL(k_decode_encode, case_decode_encode, AC_DECODE_ENCODE_IN, AC_DECODE_ENCODE_OUT)
AC_KERNEL(k_point_ops, case_point_ops, AC_POINT_OPS_IN, AC_POINT_OPS_OUT)
AC_KERNEL(k_scalar, case_scalar, AC_SCALAR_IN, AC_SCALAR_OUT)

// allocate, copy in, launch once, synchronise, copy out, free; the first HIP error is what comes back (0 = success)
typedef void (*ac_kernel)(const uint32_t*, uint32_t*, uint32_t);
static int ac_run(ac_kernel k, const uint32_t* in, uint32_t* out, uint32_t n, uint32_t ni, uint32_t no) {
  if (n == 0) return 0;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_in, (size_t)n * ni * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&d_out, (size_t)n * no * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpy(d_in, in, (size_t)n * ni * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0, (size_t)n * no * sizeof(uint32_t));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k, dim3((n + AFX_BLOCK - 1) / AFX_BLOCK), dim3(AFX_BLOCK), 0, 0, d_in, d_out, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)n * no * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return (int)e;
}

extern "C" {
int arith_dev_block(void) { return AFX_BLOCK; }
int arith_dev_fe_limbs(const uint32_t* in, uint32_t* out, uint32_t n) { return ac_run(k_fe_limbs, in, out, n, AC_FE_LIMBS_IN, AC_FE_LIMBS_OUT); }
int arith_dev_fe10_limbs(const uint32_t* in, uint32_t* out, uint32_t n) { return ac_run(k_fe10_limbs, in, out, n, AC_FE10_LIMBS_IN, AC_FE10_LIMBS_OUT); }
int arith_dev_fe_bytes(const uint32_t* in, uint32_t* out, uint32_t n) { return ac_run(k_fe_bytes, in, out, n, AC_FE_BYTES_IN, AC_FE_BYTES_OUT); }
int arith_dev_sqrt_ratio(const uint32_t* in, uint32_t* out, uint32_t n) { return ac_run(k_sqrt_ratio, in, out, n, AC_SQRT_RATIO_IN, AC_SQRT_RATIO_OUT); }
int arith_dev_elligator(const uint32_t* in, uint32_t* out, uint32_t n) { return ac_run(k_elligator, in, out, n, AC_ELLIGATOR_IN, AC_ELLIGATOR_OUT); }
int arith_dev_decode_encode(const uint32_t* in, uint32_t* out, uint32_t n) { return ac_run(k_decode_encode, in, out, n, AC_DECODE_ENCODE_IN, AC_DECODE_ENCODE_OUT); }
int arith_dev_point_ops(const uint32_t* in, uint32_t* out, uint32_t n) { return ac_run(k_point_ops, in, out, n, AC_POINT_OPS_IN, AC_POINT_OPS_OUT); }
int arith_dev_scalar(const uint32_t* in, uint32_t* out, uint32_t n) { return ac_run(k_scalar, in, out, n, AC_SCALAR_IN, AC_SCALAR_OUT); }
// words per case of every kind, in the order of tests/arith_cases.py KINDS
void arith_dev_words(uint32_t out[16]) {
  const uint32_t v[16] = { AC_FE_LIMBS_IN, AC_FE_LIMBS_OUT, AC_FE10_LIMBS_IN, AC_FE10_LIMBS_OUT, AC_FE_BYTES_IN, AC_FE_BYTES_OUT,
                           AC_SQRT_RATIO_IN, AC_SQRT_RATIO_OUT, AC_ELLIGATOR_IN, AC_ELLIGATOR_OUT, AC_DECODE_ENCODE_IN, AC_DECODE_ENCODE_OUT,
                           AC_POINT_OPS_IN, AC_POINT_OPS_OUT, AC_SCALAR_IN, AC_SCALAR_OUT };
  for (int i = 0; i < 16; i++) out[i] = v[i];
}
}  // extern "C"
