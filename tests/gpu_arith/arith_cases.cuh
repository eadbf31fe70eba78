// One case of tests/arith_cases.py per call: words in, words out.  The SAME bodies are compiled twice - by g++ into
// tests/hostsim/arith_host.cpp (every product under the bounds checker, AFX_PIN empty) and by hipcc into
// tests/gpu_arith/arith_device.hip (one case per lane, the product's flags) - so that the two builds of fe.cuh / fe10.cuh /
// ge.cuh / sc.cuh can be compared limb for limb.  Test infrastructure only: nothing in the product includes this file.
// Include after ge.cuh and sc.cuh.  No printf, no assert: a case only computes.
#pragma once

// words per case, in and out (tests/arith_cases.py KINDS holds the same numbers and the tests compare them)
#define AC_FE_LIMBS_IN 28
#define AC_FE_LIMBS_OUT 93
#define AC_FE10_LIMBS_IN 21
#define AC_FE10_LIMBS_OUT 54
#define AC_FE_BYTES_IN 16
#define AC_FE_BYTES_OUT 40
#define AC_SQRT_RATIO_IN 16
#define AC_SQRT_RATIO_OUT 9
#define AC_ELLIGATOR_IN 8
#define AC_ELLIGATOR_OUT 8
#define AC_DECODE_ENCODE_IN 8
#define AC_DECODE_ENCODE_OUT 9
#define AC_POINT_OPS_IN 16
#define AC_POINT_OPS_N 15
#define AC_POINT_OPS_OUT (1 + 8 * AC_POINT_OPS_N)
#define AC_SCALAR_IN 48
#define AC_SCALAR_OUT 41

AFX_DEV fe ac_get_fe(const uint32_t* in) {
  fe r;
#pragma unroll
  for (int i = 0; i < AFX_FE_LIMBS; i++) r.v[i] = (int32_t)in[i];
  return r;
}
AFX_DEV void ac_put_fe(uint32_t* out, const fe& f) {
#pragma unroll
  for (int i = 0; i < AFX_FE_LIMBS; i++) out[i] = (uint32_t)f.v[i];
}
AFX_DEV fe10 ac_get_fe10(const uint32_t* in) {
  fe10 r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = (int32_t)in[i];
  return r;
}
AFX_DEV void ac_put_fe10(uint32_t* out, const fe10& f) {
#pragma unroll
  for (int i = 0; i < 10; i++) out[i] = (uint32_t)f.v[i];
}
AFX_DEV sc ac_get_sc(const uint32_t* in) {
  sc r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = in[i];
  return r;
}
AFX_DEV void ac_put_sc(uint32_t* out, const sc& s) {
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = s.v[i];
}

// in: f[9], fs[9], g[9], which.  which & 1: f * g, centred and raw; & 2: fs^2, centred and raw, and fs itself; & 4: f itself.
// out: limbs of fe_mul, fe_mul_raw, fe_sq, fe_sq_raw, fe_carry(f) (5 x 9), then the canonical bytes of those four results, of f
// and of fs (6 x 8).  What is not asked for stays zero: a case beyond the discipline of a product (the int32-wide operands of
// the encoding test) never reaches one.
AFX_DEV void case_fe_limbs(const uint32_t* in, uint32_t* out) {
  const fe f = ac_get_fe(in), fs = ac_get_fe(in + 9), g = ac_get_fe(in + 18);
  const uint32_t which = in[27];
#pragma unroll
  for (int i = 0; i < AC_FE_LIMBS_OUT; i++) out[i] = 0;
  if (which & 1u) {
    const fe c = fe_mul(f, g), r = fe_mul_raw(f, g);
    ac_put_fe(out, c); fe_tobytes(out + 45, c);
    ac_put_fe(out + 9, r); fe_tobytes(out + 53, r);
  }
  if (which & 2u) {
    const fe c = fe_sq(fs), r = fe_sq_raw(fs);
    ac_put_fe(out + 18, c); fe_tobytes(out + 61, c);
    ac_put_fe(out + 27, r); fe_tobytes(out + 69, r);
    fe_tobytes(out + 85, fs);
  }
  if (which & 4u) {
    ac_put_fe(out + 36, fe_carry(f));
    fe_tobytes(out + 77, f);
  }
}

// in: f[10], g[10], which.  which & 1: fe10_mul_raw(f, g) and fe10_sq_raw(f); & 4: fe10_carry(f) and fe10_tobytes(f).
// out: limbs of the product, the squaring, the carry (3 x 10), then the canonical bytes of the product, the squaring and f.
AFX_DEV void case_fe10_limbs(const uint32_t* in, uint32_t* out) {
  const fe10 f = ac_get_fe10(in), g = ac_get_fe10(in + 10);
  const uint32_t which = in[20];
#pragma unroll
  for (int i = 0; i < AC_FE10_LIMBS_OUT; i++) out[i] = 0;
  if (which & 1u) {
    const fe10 m = fe10_mul_raw(f, g), s = fe10_sq_raw(f);
    ac_put_fe10(out, m); fe10_tobytes(out + 30, m);
    ac_put_fe10(out + 10, s); fe10_tobytes(out + 38, s);
  }
  if (which & 4u) {
    ac_put_fe10(out + 20, fe10_carry(f));
    fe10_tobytes(out + 46, f);
  }
}

// in: a[8], b[8] (32-byte encodings, bit 255 ignored).  out: canonical bytes of a * b, a^2, 1 / a, a^((p-5)/8), and a taken
// through fe10_frombytes -> fe10_tobytes.
AFX_DEV void case_fe_bytes(const uint32_t* in, uint32_t* out) {
  const fe x = fe_frombytes(in), y = fe_frombytes(in + 8);
  fe_tobytes(out, fe_mul(x, y));
  fe_tobytes(out + 8, fe_sq(x));
  fe_tobytes(out + 16, fe_invert(x));
  fe_tobytes(out + 24, fe_pow22523(x));
  fe10_tobytes(out + 32, fe10_frombytes(in));
}

// in: u[8], v[8].  out: was_square, then the canonical bytes of the root fe_sqrt_ratio_i returns.
AFX_DEV void case_sqrt_ratio(const uint32_t* in, uint32_t* out) {
  fe r;
  const bool sq = fe_sqrt_ratio_i(r, fe_frombytes(in), fe_frombytes(in + 8));
  out[0] = sq ? 1u : 0u;
  fe_tobytes(out + 1, r);
}

// in: r0[8].  out: the encoding of MAP(r0).
AFX_DEV void case_elligator(const uint32_t* in, uint32_t* out) { ristretto_encode(out, ristretto_elligator(fe_frombytes(in))); }

// in: an encoding.  out: 1 and the encoding of the decoded point, or 0 and zeros.
AFX_DEV void case_decode_encode(const uint32_t* in, uint32_t* out) {
  ge_p3 P;
  const bool ok = ristretto_decode(P, in);
  out[0] = ok ? 1u : 0u;
#pragma unroll
  for (int i = 0; i < 8; i++) out[1 + i] = 0;
  if (ok) ristretto_encode(out + 1, P);
}

// in: encodings of P and Q.  out: 1 if both decode (else 0 and zeros), then the encodings of
//   0 P + Q          1 P - Q          2 ge_double(P)   3 P + P through ge_add        4 P - P
//   5 P + identity   6 identity + P   7 identity + identity   8 ge_double(identity)
//   9 ge_madd(P, niels identity)      10 the same with neg    11 ge_madd(P, niels(Q))   12 the same with neg (P - Q)
//   13 ge_neg(identity)               14 ge_neg(P)
AFX_DEV void case_point_ops(const uint32_t* in, uint32_t* out) {
  ge_p3 P, Q;
  const bool ok = ristretto_decode(P, in) & ristretto_decode(Q, in + 8);
  out[0] = ok ? 1u : 0u;
#pragma unroll 1
  for (int i = 1; i < AC_POINT_OPS_OUT; i++) out[i] = 0;
  if (!ok) return;
  const ge_p3 I = ge_identity();
  const ge_niels nid = ge_niels_identity(), nq = ge_niels_from_affine(Q.X, Q.Y);   // a decoded point has Z = 1
  ge_p3 r[AC_POINT_OPS_N];
  r[0] = ge_add(P, Q); r[1] = ge_sub(P, Q); r[2] = ge_double(P); r[3] = ge_add(P, P); r[4] = ge_sub(P, P);
  r[5] = ge_add(P, I); r[6] = ge_add(I, P); r[7] = ge_add(I, I); r[8] = ge_double(I);
  r[9] = ge_p1p1_to_p3(ge_madd(P, nid, false)); r[10] = ge_p1p1_to_p3(ge_madd(P, nid, true));
  r[11] = ge_p1p1_to_p3(ge_madd(P, nq, false)); r[12] = ge_p1p1_to_p3(ge_madd(P, nq, true));
  r[13] = ge_neg(I); r[14] = ge_neg(P);
#pragma unroll 1
  for (int k = 0; k < AC_POINT_OPS_N; k++) ristretto_encode(out + 1 + 8 * k, r[k]);   // one encoder, not fifteen copies
}

// in: wide[16], a[8] (any 256-bit value), x[8], b[8], c[8] (canonical).  out: wide mod l, x * b + c, -x, x / 2, 2 x, and whether
// a is canonical.
AFX_DEV void case_scalar(const uint32_t* in, uint32_t* out) {
  const sc x = ac_get_sc(in + 24);
  ac_put_sc(out, sc_reduce512(in));
  ac_put_sc(out + 8, sc_muladd(x, ac_get_sc(in + 32), ac_get_sc(in + 40)));
  ac_put_sc(out + 16, sc_neg(x));
  ac_put_sc(out + 24, sc_half(x));
  ac_put_sc(out + 32, sc_dbl(x));
  out[40] = sc_is_canonical(ac_get_sc(in + 16)) ? 1u : 0u;
}
