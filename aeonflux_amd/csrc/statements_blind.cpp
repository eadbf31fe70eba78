// Blind issuance in batch form (include/aeonflux_gpu.h, "Blind issuance"): the user's request (ElGamal ciphertexts of the hidden
// attributes under a one-time key + a proof that they are well formed), the issuer's MAC on the ciphertexts with its proof, and the
// user's verification and decryption of V.  The crate names this half and leaves it unimplemented (src/user.rs:86-128); the
// statements are built from the machinery of statements_prove.cpp - SchnorrBuilder, the issuance proof's allocations, Messages::
// from_attributes - as launch lists:
//   request   reductions (r_j) -> D, A_j, B_j (fixed-base chains: B_j = (r_j*d)*G + M_i) -> the request proof
//   issue     the request's verification, t, U, r' -> S1, S2 (the key's terms on the per-item A_i, B_i run as they do for y_i*M_i in
//             Amac::tag) -> the blind issuance proof
//   unblind   the issuance proof's verification, d*S1 -> V = S2 - d*S1
// Every call ends with the output masking (Assembler::mask, k_mask_rows) in front of k_finish: a failed item's output rows are zeros.
// A plan has ONE secret setting: the verification inside issue and unblind runs under its plan's prover-side setting.
#include "statements.hpp"

namespace {
constexpr const char* TRANSCRIPT = "2019/1416 anonymous credential";
constexpr const char* REQUEST_LABEL = "2019/1416 blind request proof";
constexpr const char* ISSUANCE_LABEL = "2019/1416 blind issuance proof";

bool is_scalar_kind(uint8_t k) { return k == AFX_ATTR_PUBLIC_SCALAR || k == AFX_ATTR_SECRET_SCALAR; }
bool is_hidden_kind(uint8_t k) { return k == AFX_ATTR_SECRET_SCALAR || k == AFX_ATTR_SECRET_POINT; }
afx_scalarop_job mk_scalarop(const uint8_t* a, uint32_t as_, const uint8_t* b, uint32_t bs, const uint8_t* c, uint32_t cs, bool neg, uint8_t* out) {
  afx_scalarop_job o;
  memset(&o, 0, sizeof o);
  o.a = a; o.a_stride = as_; o.b = b; o.b_stride = bs; o.c = c; o.c_stride = cs; o.negate = neg ? 1u : 0u; o.out = out;
  return o;
}
afx_msm_job mk_job(const std::vector<afx_msm_term>& terms, const int32_t* addend, int32_t* out_var, uint8_t* out_enc, bool reject_identity) {
  afx_msm_job j;
  memset(&j, 0, sizeof j);
  set_terms(j, terms);
  j.addend = addend;
  j.out_var = out_var;
  j.out_enc = out_enc;
  j.reject_identity = reject_identity ? 1u : 0u;
  return j;
}
ScalarVar sv_item(const uint8_t* dev) { ScalarVar s; s.dev = dev; s.stride = 32; return s; }
ScalarVar sv_uniform(const uint8_t* dev, const Enc& host) { ScalarVar s; s.dev = dev; s.stride = 0; s.host = host; return s; }

// the hidden positions of a layout: H in increasing order, h = |H|, hs scalars among them
struct Layout {
  uint32_t n = 0, h = 0, hs = 0;
  uint8_t kinds[AFX_MAX_ATTRIBUTES];
  uint32_t H[AFX_MAX_ATTRIBUTES];
  int32_t slot[AFX_MAX_ATTRIBUTES];   // position -> its index in H, or -1
  bool bad_kind = false;
  explicit Layout(const afx_attributes_soa& a) {
    memset(kinds, 0, sizeof kinds);
    n = a.n_attributes;
    for (uint32_t i = 0; i < AFX_MAX_ATTRIBUTES; i++) slot[i] = -1;
    for (uint32_t i = 0; i < n && i < AFX_MAX_ATTRIBUTES; i++) {
      kinds[i] = a.kinds[i];
      bad_kind |= kinds[i] > AFX_ATTR_SECRET_POINT;
      if (!is_hidden_kind(kinds[i])) continue;
      slot[i] = (int32_t)h;
      H[h++] = i;
      hs += kinds[i] == AFX_ATTR_SECRET_SCALAR;
    }
  }
  uint32_t request_responses() const { return 1 + h + hs; }
  bool hidden_scalar(uint32_t j) const { return kinds[H[j]] == AFX_ATTR_SECRET_SCALAR; }
  bool fits(const afx_ctx* c) const { return n == c->n && !bad_kind; }   // Amac::tag's length test (amacs.rs:285-287) and the kinds the engine knows
  uint32_t revealed() const { return (n < AFX_MAX_ATTRIBUTES ? n : AFX_MAX_ATTRIBUTES) - h; }
};
PlanKey blind_key(const afx_ctx* c, const char* statement, const Layout& L, uint32_t nr_request, uint32_t nr_issuance) {
  struct { uint32_t n, nr_request, nr_issuance; uint8_t kinds[AFX_MAX_ATTRIBUTES]; } kd;
  memset(&kd, 0, sizeof kd);
  kd.n = L.n; kd.nr_request = nr_request; kd.nr_issuance = nr_issuance; memcpy(kd.kinds, L.kinds, sizeof kd.kinds);
  return plan_key(statement, &kd, sizeof kd, mode_flags(c));
}

// ---- the request proof: allocation order and constraints, shared by prover and verifier ----
struct RequestVars {
  ScalarVar d, r[AFX_MAX_ATTRIBUTES], m[AFX_MAX_ATTRIBUTES];   // r, m by index in H
  PointVar D, A[AFX_MAX_ATTRIBUTES], B[AFX_MAX_ATTRIBUTES];
};
void request_statement(SchnorrBuilder& b, afx_ctx* c, const Layout& L, const RequestVars& v) {
  int r[AFX_MAX_ATTRIBUTES], m[AFX_MAX_ATTRIBUTES], A[AFX_MAX_ATTRIBUTES], B[AFX_MAX_ATTRIBUTES], G_m[AFX_MAX_ATTRIBUTES];
  const int d = b.allocate_scalar("d", v.d);
  for (uint32_t j = 0; j < L.h; j++) {
    r[j] = b.allocate_scalar("r", v.r[j]);
    if (L.hidden_scalar(j)) m[j] = b.allocate_scalar("m", v.m[j]);
  }
  const int G = b.allocate_point("G", PointVar::Const(c->id_G()));
  const int D = b.allocate_point("D", v.D);
  for (uint32_t j = 0; j < L.h; j++) {
    A[j] = b.allocate_point("A", v.A[j]);
    B[j] = b.allocate_point("B", v.B[j]);   // a hidden point's B is only bound into the challenge
    if (L.hidden_scalar(j)) G_m[j] = b.allocate_point("G_m", PointVar::Const(c->id_Gm(L.H[j])));
  }
  b.constrain(D, { { d, G } });
  for (uint32_t j = 0; j < L.h; j++) {
    b.constrain(A[j], { { r[j], G } });
    if (L.hidden_scalar(j)) b.constrain(B[j], { { r[j], D }, { m[j], G_m[j] } });
  }
}

// D, A_j, B_j of a received request, decoded (an identity encoding fails the item: they are allocated into transcripts)
struct RequestPoints { int32_t* D; int32_t* A[AFX_MAX_ATTRIBUTES]; int32_t* B[AFX_MAX_ATTRIBUTES]; };
RequestPoints decode_request(Assembler& as, const Layout& L, const afx_blind_request_soa& q, size_t count, size_t off, std::vector<afx_decode_job>& decode) {
  auto row = [&](const uint8_t* base, size_t k) { return base + (k * count + off) * 32; };
  RequestPoints P;
  memset(&P, 0, sizeof P);
  P.D = as.new_var();
  decode.push_back({ row(q.D, 0), P.D, 1u });
  for (uint32_t j = 0; j < L.h; j++) {
    P.A[j] = as.new_var(); P.B[j] = as.new_var();
    decode.push_back({ row(q.A, j), P.A[j], 1u });
    decode.push_back({ row(q.B, j), P.B[j], 1u });
  }
  return P;
}
// the request as a zkp Verifier verifies it: its jobs join the caller's lists (the chains read decoded points only)
RequestPoints add_request_verify(Assembler& as, const Layout& L, const afx_blind_request_soa& q, size_t count, size_t off, JobSets& js, std::vector<afx_msm_job>& msm) {
  auto row = [&](const uint8_t* base, size_t k) { return base + (k * count + off) * 32; };
  js.sccheck.push_back({ row(q.challenge, 0) });
  for (uint32_t k = 0; k < L.request_responses(); k++) js.sccheck.push_back({ row(q.responses, k) });
  const RequestPoints P = decode_request(as, L, q, count, off, js.decode);
  RequestVars v;
  uint32_t k = 0;
  v.d = sv_item(row(q.responses, k++));
  for (uint32_t j = 0; j < L.h; j++) {
    v.r[j] = sv_item(row(q.responses, k++));
    if (L.hidden_scalar(j)) v.m[j] = sv_item(row(q.responses, k++));
  }
  v.D = PointVar::Var(P.D, row(q.D, 0));
  for (uint32_t j = 0; j < L.h; j++) { v.A[j] = PointVar::Var(P.A[j], row(q.A, j)); v.B[j] = PointVar::Var(P.B[j], row(q.B, j)); }
  SchnorrBuilder b(as, TRANSCRIPT, REQUEST_LABEL);
  request_statement(b, as.ctx, L, v);
  b.verify_compact(row(q.challenge, 0), 0, count, off, msm, js.hash, &js.scalarop);
  return P;
}

// M_i of the revealed positions (Messages::from_attributes, src/amacs.rs:225-243); the rows of hidden positions are not touched
void revealed_messages(Assembler& as, const Layout& L, const uint8_t* values, size_t count, size_t off, bool reject_identity, JobSets& js,
                       std::vector<afx_msm_job>& msm, PointVar M[AFX_MAX_ATTRIBUTES]) {
  afx_ctx* c = as.ctx;
  for (uint32_t i = 0; i < L.n; i++) {
    if (L.slot[i] >= 0) continue;
    const uint8_t* val = values + (i * count + off) * 32;
    if (is_scalar_kind(L.kinds[i])) {
      js.sccheck.push_back({ val });
      uint8_t* e = as.new_enc();
      msm.push_back(mk_job({ mk_term(val, 32, nullptr, (int32_t)c->id_Gm(i), false) }, nullptr, nullptr, e, reject_identity));
      M[i] = PointVar::Var(nullptr, e);
      M[i].has_alt = true; M[i].alt_gen = c->id_Gm(i); M[i].alt_scalar = val;   // M_i = m_i * G_m_i: its terms run on the generator
    } else {
      int32_t* v = as.new_var();
      js.decode.push_back({ val, v, reject_identity ? 1u : 0u });
      M[i] = PointVar::Var(v, val);
    }
  }
}

// ---- the blind issuance proof ----
struct IssuanceVars {
  ScalarVar w, wp, x0, x1, y[AFX_MAX_ATTRIBUTES], one, rp;
  PointVar U, tU, D, S1, S2, A[AFX_MAX_ATTRIBUTES], B[AFX_MAX_ATTRIBUTES] /* by index in H */, M[AFX_MAX_ATTRIBUTES] /* by position */;
};
void issuance_statement(SchnorrBuilder& b, afx_ctx* c, const Layout& L, const IssuanceVars& iv) {
  const uint32_t n = c->n, g = c->g;
  const int w = b.allocate_scalar("w", iv.w);
  const int w_prime = b.allocate_scalar("w'", iv.wp);
  const int x_0 = b.allocate_scalar("x_0", iv.x0);
  const int x_1 = b.allocate_scalar("x_1", iv.x1);
  int y[AFX_MAX_ATTRIBUTES];
  for (uint32_t i = 0; i < n; i++) y[i] = b.allocate_scalar("y", iv.y[i]);
  const int one = b.allocate_scalar("1", iv.one);
  const int rp = b.allocate_scalar("r'", iv.rp);
  const int G_V = b.allocate_point("G_V", PointVar::Const(c->id_GV()));
  const int G_w = b.allocate_point("G_w", PointVar::Const(c->id_Gw()));
  const int G_w_prime = b.allocate_point("G_w_prime", PointVar::Const(c->id_Gwp()));
  const int neg_G_x_0 = b.allocate_point("-G_x_0", PointVar::Const(c->id_Gx0(), true));
  const int neg_G_x_1 = b.allocate_point("-G_x_1", PointVar::Const(c->id_Gx1(), true));
  int neg_G_y[AFX_MAX_ATTRIBUTES];
  for (uint32_t i = 0; i < g; i++) neg_G_y[i] = b.allocate_point("-G_y", PointVar::Const(c->id_Gy(i), true));
  const int C_W = b.allocate_point("C_W", PointVar::Const(c->id_CW()));
  const int I = b.allocate_point("I", PointVar::Const(c->id_I()));
  const int U = b.allocate_point("U", iv.U);
  const int tU = b.allocate_point("tU", iv.tU);   // (the issuance proof's V is not allocated)
  const int G = b.allocate_point("G", PointVar::Const(c->id_G()));
  const int D = b.allocate_point("D", iv.D);
  const int S1 = b.allocate_point("S1", iv.S1);
  const int S2 = b.allocate_point("S2", iv.S2);
  int A[AFX_MAX_ATTRIBUTES], last[AFX_MAX_ATTRIBUTES];   // last: B_i of a hidden position, M_i of a revealed one
  for (uint32_t i = 0; i < n; i++) {
    if (L.slot[i] >= 0) {
      A[i] = b.allocate_point("A", iv.A[L.slot[i]]);
      last[i] = b.allocate_point("B", iv.B[L.slot[i]]);
    } else {
      last[i] = b.allocate_point("M", iv.M[i]);
    }
  }
  b.constrain(C_W, { { w, G_w }, { w_prime, G_w_prime } });
  std::vector<std::pair<int, int>> rhs = { { one, G_V }, { x_0, neg_G_x_0 }, { x_1, neg_G_x_1 } };
  for (uint32_t i = 0; i < n; i++) rhs.push_back({ y[i], neg_G_y[i] });
  b.constrain(I, rhs);
  rhs = { { rp, G } };
  for (uint32_t j = 0; j < L.h; j++) rhs.push_back({ y[L.H[j]], A[L.H[j]] });
  b.constrain(S1, rhs);
  rhs = { { w, G_w }, { x_0, U }, { x_1, tU }, { rp, D } };
  for (uint32_t i = 0; i < n; i++) rhs.push_back({ y[i], last[i] });
  b.constrain(S2, rhs);
}

// every statement fails: the bad words are filled by the plan's opening launch, the masking zeroes the outputs
void fail_every_item(Assembler& as, const std::vector<uint8_t*>& outs, uint8_t* status_dev, uint8_t code) {
  as.fail_all = true;
  as.mask(outs);
  as.finish(status_dev, code);
}
void rows_of(std::vector<uint8_t*>& v, uint8_t* base, size_t rows, size_t count, size_t off) {
  for (size_t k = 0; base && k < rows; k++) v.push_back(base + (k * count + off) * 32);
}
}  // namespace

// ------------------------------------------------------------------------------------------------
// the user's request
// ------------------------------------------------------------------------------------------------
extern "C" int afx_blind_request_dev(afx_ctx* ctx, const afx_attributes_soa* attrs, const uint8_t* d, const afx_blind_request_randomness* rnd, size_t count,
                                     const afx_blind_request_soa* out, uint8_t* status_dev) try {
  CtxLock lock__(ctx);
  if (!ctx || !attrs || !rnd || !out || !status_dev) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  const afx_attributes_soa a = *attrs;
  const afx_blind_request_randomness r = *rnd;
  const afx_blind_request_soa o = *out;
  const Layout L(a);
  if (L.fits(ctx) && (!a.values || !d || !r.rng_seed || !o.D || !o.challenge || !o.responses || (L.h && (!r.r_wide || !o.A || !o.B)))) {
    set_error("null batch array");
    return AFX_E_BAD_ARGS;
  }
  return run_chunked(ctx, count, [&](Assembler& as, size_t off, uint32_t) {
    afx_ctx* c = as.ctx;
    as.secret_scalars = true;   // d, r_j, the hidden values, the proof's blindings: afx_ctx_set_secret_independent_addressing
    auto row = [&](const uint8_t* base, size_t k) { return base + (k * count + off) * 32; };
    auto orow = [&](uint8_t* base, size_t k) { return base + (k * count + off) * 32; };
    std::vector<uint8_t*> outs;
    rows_of(outs, o.D, 1, count, off); rows_of(outs, o.A, L.h, count, off); rows_of(outs, o.B, L.h, count, off);
    rows_of(outs, o.challenge, 1, count, off); rows_of(outs, o.responses, L.request_responses(), count, off);
    if (!L.fits(c)) { fail_every_item(as, outs, status_dev + off, AFX_ST_MAC_CREATION); return; }
    JobSets js;
    std::vector<afx_msm_job> msm1;
    std::vector<afx_scalarop_job> sc1;
    js.sccheck.push_back({ row(d, 0) });
    // every position's value is checked; only the hidden ones enter the request
    const int32_t* v_M[AFX_MAX_ATTRIBUTES] = { nullptr };
    for (uint32_t i = 0; i < L.n; i++) {
      if (is_scalar_kind(L.kinds[i])) js.sccheck.push_back({ row(a.values, i) });
      else {
        int32_t* v = L.slot[i] >= 0 ? as.new_var() : nullptr;
        js.decode.push_back({ row(a.values, i), v, 0u });
        v_M[i] = v;
      }
    }
    // r_j and r_j*d, in one piece: zeroed at the end
    uint8_t* sec = L.h ? as.new_rows(2 * (size_t)L.h) : nullptr;
    auto r_of = [&](uint32_t j) { return sec + 32 * (size_t)as.count * j; };
    auto rd_of = [&](uint32_t j) { return sec + 32 * (size_t)as.count * (L.h + j); };
    int32_t* v_D = as.new_var();
    msm1.push_back(mk_job({ mk_term(row(d, 0), 32, nullptr, (int32_t)c->id_G(), false) }, nullptr, v_D, orow(o.D, 0), true));   // D = d*G: an output, and r's base in the proof
    RequestVars v;
    v.d = sv_item(row(d, 0));
    v.D = PointVar::Var(v_D, orow(o.D, 0));
    v.D.parts.push_back({ row(d, 0), 32, false, nullptr, (int32_t)c->id_G() });   // (a segmenting pass multiplies by G instead: SchnorrBuilder::prove_compact)
    for (uint32_t j = 0; j < L.h; j++) {
      const uint32_t i = L.H[j];
      as.reduce_wide(r.r_wide + ((size_t)j * count + off) * 64, r_of(j));
      sc1.push_back(mk_scalarop(r_of(j), 32, row(d, 0), 32, nullptr, 0, false, rd_of(j)));
      msm1.push_back(mk_job({ mk_term(r_of(j), 32, nullptr, (int32_t)c->id_G(), false) }, nullptr, nullptr, orow(o.A, j), true));
      // B_j = r_j*D + M_i = (r_j*d)*G + M_i: no chain waits for D
      if (L.hidden_scalar(j))
        msm1.push_back(mk_job({ mk_term(rd_of(j), 32, nullptr, (int32_t)c->id_G(), false), mk_term(row(a.values, i), 32, nullptr, (int32_t)c->id_Gm(i), false) },
                              nullptr, nullptr, orow(o.B, j), true));
      else
        msm1.push_back(mk_job({ mk_term(rd_of(j), 32, nullptr, (int32_t)c->id_G(), false) }, v_M[i], nullptr, orow(o.B, j), true));
      v.r[j] = sv_item(r_of(j));
      if (L.hidden_scalar(j)) v.m[j] = sv_item(row(a.values, i));
      v.A[j] = PointVar::Var(nullptr, orow(o.A, j));   // left-hand sides only: the prover needs their encodings
      v.B[j] = PointVar::Var(nullptr, orow(o.B, j));
    }
    SchnorrBuilder p(as, TRANSCRIPT, REQUEST_LABEL);
    request_statement(p, c, L, v);
    std::vector<afx_hash_program> rng_hash, chal_hash;
    std::vector<afx_msm_job> commit;
    std::vector<afx_scalarop_job> resp, blind_products;
    p.prove_compact(r.rng_seed + off * 32, orow(o.challenge, 0), orow(o.responses, 0), 32 * count, rng_hash, commit, chal_hash, resp, &blind_products);
    as.sccheck(js.sccheck);
    as.decode(js.decode);
    as.scalarop(sc1);
    as.msm(msm1);
    as.hash(rng_hash);
    as.scalarop(blind_products);
    as.msm(commit);
    as.hash(chal_hash);
    as.scalarop(resp);
    if (sec) as.wipe(sec, 64 * (size_t)L.h);
    as.mask(outs);
    as.finish(status_dev + off, AFX_ST_MAC_CREATION);
  }, blind_key(ctx, "blind_request", L, 0, 0));
} catch (...) { return afx::exception_rc(); }

// ------------------------------------------------------------------------------------------------
// the request's verification alone
// ------------------------------------------------------------------------------------------------
extern "C" int afx_verify_blind_requests_dev(afx_ctx* ctx, const afx_attributes_soa* attrs, const afx_blind_request_soa* requests, uint32_t n_responses,
                                             size_t count, uint8_t* status_dev) try {
  CtxLock lock__(ctx);
  if (!ctx || !attrs || !requests || !status_dev) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  const afx_blind_request_soa q = *requests;
  const Layout L(*attrs);
  const bool shape_ok = L.fits(ctx) && n_responses == L.request_responses();
  if (shape_ok && (!q.D || !q.challenge || !q.responses || (L.h && (!q.A || !q.B)))) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
  const PlanKey key__ = ctx->trace ? PlanKey() : blind_key(ctx, "verify_blind_requests", L, n_responses, 0);
  return run_chunked(ctx, count, [&](Assembler& as, size_t off, uint32_t) {
    JobSets js;
    if (!shape_ok) { as.fail_all = true; emit(as, js, status_dev + off, AFX_ST_VERIFICATION_FAILURE); return; }
    add_request_verify(as, L, q, count, off, js, js.msm1);
    emit(as, js, status_dev + off, AFX_ST_VERIFICATION_FAILURE);
  }, key__);
} catch (...) { return afx::exception_rc(); }

// ------------------------------------------------------------------------------------------------
// the issuer
// ------------------------------------------------------------------------------------------------
extern "C" int afx_issue_blind_dev(afx_ctx* ctx, const afx_attributes_soa* attrs, const afx_blind_request_soa* requests, uint32_t request_n_responses,
                                   const afx_blind_issue_randomness* rnd, size_t count, const afx_blind_issuance_soa* out, uint8_t* status_dev) try {
  CtxLock lock__(ctx);
  if (!ctx || !attrs || !requests || !rnd || !out || !status_dev) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (!ctx->has_key) { set_error("blind issuance needs the issuer key"); return AFX_E_NO_KEY; }
  if (count == 0) return AFX_OK;
  const afx_attributes_soa a = *attrs;
  const afx_blind_request_soa q = *requests;
  const afx_blind_issue_randomness r = *rnd;
  const afx_blind_issuance_soa o = *out;
  const Layout L(a);
  const bool nr_ok = request_n_responses == L.request_responses();
  if (L.fits(ctx) && nr_ok &&
      ((L.revealed() && !a.values) || !q.D || !q.challenge || !q.responses || (L.h && (!q.A || !q.B)) || !r.t_wide || !r.U_wide || !r.rprime_wide || !r.rng_seed ||
       !o.t || !o.U || !o.S1 || !o.S2 || !o.challenge || !o.responses)) {
    set_error("null batch array");
    return AFX_E_BAD_ARGS;
  }
  const PlanKey key__ = ctx->trace ? PlanKey() : blind_key(ctx, "issue_blind", L, request_n_responses, 0);
  return run_chunked(ctx, count, [&](Assembler& as, size_t off, uint32_t) {
    afx_ctx* c = as.ctx;
    // the key, t, r', the proof's blindings: afx_ctx_set_secret_independent_addressing.  The request's (public) verification shares the setting.
    as.secret_scalars = true;
    const uint32_t n = c->n;
    auto row = [&](const uint8_t* base, size_t k) { return base + (k * count + off) * 32; };
    auto orow = [&](uint8_t* base, size_t k) { return base + (k * count + off) * 32; };
    std::vector<uint8_t*> outs;
    for (uint8_t* p : { o.t, o.U, o.S1, o.S2, o.challenge }) rows_of(outs, p, 1, count, off);
    rows_of(outs, o.responses, (size_t)n + 6, count, off);
    // Amac::tag: attributes.len() != NUMBER_OF_ATTRIBUTES -> MacCreation (amacs.rs:285-287), as afx_issue; a wrong response count: zkp rejects
    if (!L.fits(c)) { fail_every_item(as, outs, status_dev + off, AFX_ST_MAC_CREATION); return; }
    if (!nr_ok) { fail_every_item(as, outs, status_dev + off, AFX_ST_VERIFICATION_FAILURE); return; }
    JobSets js;
    std::vector<afx_msm_job> msm1;
    std::vector<afx_scalarop_job> sc1;
    const RequestPoints P = add_request_verify(as, L, q, count, off, js, msm1);
    // t = Scalar::random, U = RistrettoPoint::random (amacs.rs:289-290), r'
    uint32_t n_ym = 0;
    for (uint32_t i = 0; i < n; i++) n_ym += L.slot[i] < 0 && is_scalar_kind(L.kinds[i]);
    uint8_t* sec = as.new_rows(2 + (size_t)n_ym);   // r', x0 + x1*t, y_i*m_i: zeroed at the end
    uint8_t *rp = sec, *k_xt = sec + 32 * (size_t)as.count;
    int32_t* v_U = as.new_var();
    as.reduce_wide(r.t_wide + off * 64, orow(o.t, 0));
    as.reduce_wide(r.rprime_wide + off * 64, rp);
    as.from_uniform(r.U_wide + off * 64, orow(o.U, 0), v_U);
    IssuanceVars iv;
    revealed_messages(as, L, a.values, count, off, false, js, msm1, iv.M);
    // S1 = r'*G + sum_H y_i*A_i;  S2 = r'*D + W + (x0 + x1*t)*U + sum_{revealed} y_i*M_i + sum_H y_i*B_i
    sc1.push_back(mk_scalarop(c->key_x1(), 0, orow(o.t, 0), 32, c->key_x0(), 0, false, k_xt));
    std::vector<afx_msm_term> s1 = { mk_term(rp, 32, nullptr, (int32_t)c->id_G(), false) };
    std::vector<afx_msm_term> s2 = { mk_term(rp, 32, P.D, -1, false), mk_term(k_xt, 32, v_U, -1, false) };
    uint32_t k_ym = 0;
    for (uint32_t i = 0; i < n; i++) {
      if (L.slot[i] >= 0) {
        s1.push_back(mk_term(c->key_y(i), 0, P.A[L.slot[i]], -1, false));
        s2.push_back(mk_term(c->key_y(i), 0, P.B[L.slot[i]], -1, false));
      } else if (is_scalar_kind(L.kinds[i])) {
        uint8_t* ym = sec + 32 * (size_t)as.count * (2 + k_ym++);
        sc1.push_back(mk_scalarop(c->key_y(i), 0, row(a.values, i), 32, nullptr, 0, false, ym));
        s2.push_back(mk_term(ym, 32, nullptr, (int32_t)c->id_Gm(i), false));
      } else {
        s2.push_back(mk_term(c->key_y(i), 0, iv.M[i].var, -1, false));
      }
    }
    s2.push_back(mk_term(c->const_one(), 0, nullptr, (int32_t)c->id_W(), false));
    int32_t* v_tU = as.new_var();
    uint8_t* e_tU = as.new_enc();
    msm1.push_back(mk_job(s1, nullptr, nullptr, orow(o.S1, 0), false));
    msm1.push_back(mk_job(s2, nullptr, nullptr, orow(o.S2, 0), false));
    afx_msm_job tu = mk_job({ mk_term(orow(o.t, 0), 32, v_U, -1, false) }, nullptr, v_tU, e_tU, false);   // t*U: hashed, and x_1's base
    tu.leave_half = 1;
    msm1.push_back(tu);
    Enc one{};
    one[0] = 1;
    iv.w = sv_uniform(c->key_w(), c->host_key[0]); iv.wp = sv_uniform(c->key_wp(), c->host_key[1]);
    iv.x0 = sv_uniform(c->key_x0(), c->host_key[2]); iv.x1 = sv_uniform(c->key_x1(), c->host_key[3]);
    for (uint32_t i = 0; i < n; i++) iv.y[i] = sv_uniform(c->key_y(i), c->host_key[4 + i]);
    iv.one = sv_uniform(c->const_one(), one);
    iv.rp = sv_item(rp);
    iv.U = PointVar::Var(v_U, orow(o.U, 0));
    iv.tU = PointVar::Var(v_tU, e_tU);
    iv.tU.parts.push_back({ orow(o.t, 0), 32, false, v_U, -1 });   // tU = t * U
    iv.D = PointVar::Var(P.D, row(q.D, 0));
    iv.S1 = PointVar::Var(nullptr, orow(o.S1, 0));   // left-hand sides only
    iv.S2 = PointVar::Var(nullptr, orow(o.S2, 0));
    for (uint32_t j = 0; j < L.h; j++) { iv.A[j] = PointVar::Var(P.A[j], row(q.A, j)); iv.B[j] = PointVar::Var(P.B[j], row(q.B, j)); }
    SchnorrBuilder p(as, TRANSCRIPT, ISSUANCE_LABEL);
    issuance_statement(p, c, L, iv);
    std::vector<afx_hash_program> rng_hash, chal_hash;
    std::vector<afx_msm_job> commit;
    std::vector<afx_scalarop_job> resp, blind_products;
    p.prove_compact(r.rng_seed + off * 32, orow(o.challenge, 0), orow(o.responses, 0), 32 * count, rng_hash, commit, chal_hash, resp, &blind_products);
    as.sccheck(js.sccheck);
    as.decode(js.decode);
    as.scalarop(js.scalarop);
    as.scalarop(sc1);
    as.msm(msm1);
    rng_hash.insert(rng_hash.end(), js.hash.begin(), js.hash.end());   // the request's challenge beside the proof's blindings
    as.hash(rng_hash);
    as.scalarop(blind_products);
    as.msm(commit);
    as.hash(chal_hash);
    as.scalarop(resp);
    as.wipe(sec, 32 * (2 + (size_t)n_ym));
    as.mask(outs);
    as.finish(status_dev + off, AFX_ST_VERIFICATION_FAILURE);
  }, key__);
} catch (...) { return afx::exception_rc(); }

// ------------------------------------------------------------------------------------------------
// the user's verification and decryption
// ------------------------------------------------------------------------------------------------
extern "C" int afx_unblind_issuances_dev(afx_ctx* ctx, const afx_attributes_soa* attrs, const uint8_t* d, const afx_blind_request_soa* requests,
                                         const afx_blind_issuance_soa* issuances, uint32_t n_responses, size_t count, uint8_t* V, uint8_t* status_dev) try {
  CtxLock lock__(ctx);
  if (!ctx || !attrs || !requests || !issuances || !V || !status_dev) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  const afx_attributes_soa a = *attrs;
  const afx_blind_request_soa q = *requests;
  const afx_blind_issuance_soa s = *issuances;
  const Layout L(a);
  const bool shape_ok = L.fits(ctx) && n_responses == ctx->n + 6;
  if (shape_ok && ((L.revealed() && !a.values) || !d || !q.D || (L.h && (!q.A || !q.B)) || !s.t || !s.U || !s.S1 || !s.S2 || !s.challenge || !s.responses)) {
    set_error("null batch array");
    return AFX_E_BAD_ARGS;
  }
  const PlanKey key__ = ctx->trace ? PlanKey() : blind_key(ctx, "unblind_issuances", L, 0, n_responses);
  return run_chunked(ctx, count, [&](Assembler& as, size_t off, uint32_t) {
    afx_ctx* c = as.ctx;
    as.secret_scalars = true;   // d in d*S1; the issuance proof's (public) verification shares the setting
    const uint32_t n = c->n;
    auto row = [&](const uint8_t* base, size_t k) { return base + (k * count + off) * 32; };
    std::vector<uint8_t*> outs = { V + off * 32 };
    if (!shape_ok) { fail_every_item(as, outs, status_dev + off, AFX_ST_VERIFICATION_FAILURE); return; }
    JobSets js;
    js.sccheck.push_back({ row(d, 0) });
    js.sccheck.push_back({ row(s.t, 0) });
    js.sccheck.push_back({ row(s.challenge, 0) });
    for (uint32_t k = 0; k < n_responses; k++) js.sccheck.push_back({ row(s.responses, k) });
    const RequestPoints P = decode_request(as, L, q, count, off, js.decode);
    int32_t *v_U = as.new_var(), *v_S1 = as.new_var(), *v_S2 = as.new_var(), *v_tU = as.new_var(), *v_dS1 = as.new_var();
    uint8_t* e_tU = as.new_enc();
    js.decode.push_back({ row(s.U, 0), v_U, 1u });
    js.decode.push_back({ row(s.S1, 0), v_S1, 1u });
    js.decode.push_back({ row(s.S2, 0), v_S2, 1u });
    IssuanceVars iv;
    revealed_messages(as, L, a.values, count, off, true, js, js.msm1, iv.M);
    js.msm1.push_back(mk_job({ mk_term(row(s.t, 0), 32, v_U, -1, false) }, nullptr, v_tU, e_tU, true));   // tU, recomputed
    js.msm1.push_back(mk_job({ mk_term(row(d, 0), 32, v_S1, -1, false) }, nullptr, v_dS1, nullptr, false));   // d*S1
    uint32_t k = 0;
    iv.w = sv_item(row(s.responses, k++)); iv.wp = sv_item(row(s.responses, k++)); iv.x0 = sv_item(row(s.responses, k++)); iv.x1 = sv_item(row(s.responses, k++));
    for (uint32_t i = 0; i < n; i++) iv.y[i] = sv_item(row(s.responses, k++));
    iv.one = sv_item(row(s.responses, k++));
    iv.rp = sv_item(row(s.responses, k++));
    iv.U = PointVar::Var(v_U, row(s.U, 0));
    iv.tU = PointVar::Var(v_tU, e_tU);
    iv.D = PointVar::Var(P.D, row(q.D, 0));
    iv.S1 = PointVar::Var(v_S1, row(s.S1, 0));
    iv.S2 = PointVar::Var(v_S2, row(s.S2, 0));
    for (uint32_t j = 0; j < L.h; j++) { iv.A[j] = PointVar::Var(P.A[j], row(q.A, j)); iv.B[j] = PointVar::Var(P.B[j], row(q.B, j)); }
    SchnorrBuilder v(as, TRANSCRIPT, ISSUANCE_LABEL);
    issuance_statement(v, c, L, iv);
    v.verify_compact(row(s.challenge, 0), 0, count, off, js.msm2, js.hash, &js.scalarop);
    const afx_pointop_job vj = { v_S2, v_dS1, nullptr, +1, -1, nullptr, V + off * 32, 0 };   // V = S2 - d*S1
    js.pointop.push_back(vj);
    as.sccheck(js.sccheck);
    as.decode(js.decode);
    as.scalarop(js.scalarop);
    as.msm(js.msm1);
    as.msm(js.msm2);
    as.pointop(js.pointop);
    as.hash(js.hash);
    as.mask(outs);
    as.wipe(v_dS1, sizeof(int32_t) * AFX_VAR_DWORDS);   // d*S1: its one reader, the subtraction, has run
    as.finish(status_dev + off, AFX_ST_VERIFICATION_FAILURE);
  }, key__);
} catch (...) { return afx::exception_rc(); }

// ------------------------------------------------------------------------------------------------
// host-pointer forms: the call's arrays staged in one piece, the *_dev form, the results fetched.  A shape every item fails on is
// answered here (its arrays' extents are the caller's own arithmetic on a layout the context does not have).
// ------------------------------------------------------------------------------------------------
namespace {
void zero_host(uint8_t* p, size_t rows, size_t count) { if (p && rows) memset(p, 0, rows * count * 32); }
}  // namespace

extern "C" int afx_blind_request(afx_ctx* ctx, const afx_attributes_soa* attrs, const uint8_t* d, const afx_blind_request_randomness* rnd, size_t count,
                                 const afx_blind_request_soa* out, uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !attrs || !rnd || !out || !status) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  const Layout L(*attrs);
  if (!L.fits(ctx)) {
    memset(status, AFX_ST_MAC_CREATION, count);
    zero_host(out->D, 1, count); zero_host(out->A, L.h, count); zero_host(out->B, L.h, count); zero_host(out->challenge, 1, count);
    zero_host(out->responses, L.request_responses(), count);
    return AFX_OK;
  }
  if (!attrs->values || !d || !rnd->rng_seed || !out->D || !out->challenge || !out->responses || (L.h && (!rnd->r_wide || !out->A || !out->B))) {
    set_error("null batch array");
    return AFX_E_BAD_ARGS;
  }
  AFX_HIP(hipSetDevice(ctx->device));
  HostCall hc(ctx, count, 0);
  const size_t o_val = hc.in(attrs->values, L.n), o_d = hc.in(d, 1), o_rw = hc.in(rnd->r_wide, L.h, 64), o_seed = hc.in(rnd->rng_seed, 1);
  const size_t o_D = hc.res(out->D, 1), o_A = hc.res(out->A, L.h), o_B = hc.res(out->B, L.h), o_ch = hc.res(out->challenge, 1),
               o_rs = hc.res(out->responses, L.request_responses()), o_st = hc.res(status, 1, 1);
  int rc = hc.st.upload();
  if (rc) return rc;
  afx_attributes_soa da = *attrs;
  da.values = hc.st.dev(o_val);
  const afx_blind_request_randomness dr = { hc.st.dev(o_rw), hc.st.dev(o_seed) };
  const afx_blind_request_soa dout = { hc.st.dev(o_D), hc.st.dev(o_A), hc.st.dev(o_B), hc.st.dev(o_ch), hc.st.dev(o_rs) };
  if ((rc = afx_blind_request_dev(ctx, &da, hc.st.dev(o_d), &dr, count, &dout, hc.st.dev(o_st)))) return rc;
  return hc.fetch();
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_verify_blind_requests(afx_ctx* ctx, const afx_attributes_soa* attrs, const afx_blind_request_soa* requests, uint32_t n_responses, size_t count,
                                         uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !attrs || !requests || !status) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  const Layout L(*attrs);
  if (!L.fits(ctx) || n_responses != L.request_responses()) { memset(status, AFX_ST_VERIFICATION_FAILURE, count); return AFX_OK; }
  const afx_blind_request_soa& q = *requests;
  if (!q.D || !q.challenge || !q.responses || (L.h && (!q.A || !q.B))) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
  AFX_HIP(hipSetDevice(ctx->device));
  HostCall hc(ctx, count, 0);
  const size_t o_D = hc.in(q.D, 1), o_A = hc.in(q.A, L.h), o_B = hc.in(q.B, L.h), o_ch = hc.in(q.challenge, 1), o_rs = hc.in(q.responses, n_responses),
               o_st = hc.res(status, 1, 1);
  int rc = hc.st.upload();
  if (rc) return rc;
  afx_attributes_soa da = *attrs;
  da.values = nullptr;
  const afx_blind_request_soa dq = { hc.st.dev(o_D), hc.st.dev(o_A), hc.st.dev(o_B), hc.st.dev(o_ch), hc.st.dev(o_rs) };
  if ((rc = afx_verify_blind_requests_dev(ctx, &da, &dq, n_responses, count, hc.st.dev(o_st)))) return rc;
  return hc.fetch();
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_issue_blind(afx_ctx* ctx, const afx_attributes_soa* attrs, const afx_blind_request_soa* requests, uint32_t request_n_responses,
                               const afx_blind_issue_randomness* rnd, size_t count, const afx_blind_issuance_soa* out, uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !attrs || !requests || !rnd || !out || !status) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (!ctx->has_key) { set_error("blind issuance needs the issuer key"); return AFX_E_NO_KEY; }
  if (count == 0) return AFX_OK;
  const Layout L(*attrs);
  if (!L.fits(ctx) || request_n_responses != L.request_responses()) {
    memset(status, L.fits(ctx) ? AFX_ST_VERIFICATION_FAILURE : AFX_ST_MAC_CREATION, count);
    for (uint8_t* p : { out->t, out->U, out->S1, out->S2, out->challenge }) zero_host(p, 1, count);
    zero_host(out->responses, (size_t)ctx->n + 6, count);
    return AFX_OK;
  }
  const afx_blind_request_soa& q = *requests;
  if ((L.revealed() && !attrs->values) || !q.D || !q.challenge || !q.responses || (L.h && (!q.A || !q.B)) || !rnd->t_wide || !rnd->U_wide || !rnd->rprime_wide ||
      !rnd->rng_seed || !out->t || !out->U || !out->S1 || !out->S2 || !out->challenge || !out->responses) {
    set_error("null batch array");
    return AFX_E_BAD_ARGS;
  }
  AFX_HIP(hipSetDevice(ctx->device));
  const uint32_t nr = ctx->n + 6;
  HostCall hc(ctx, count, 0);
  // the rows of hidden positions stay on the host: the issuer's plan never reads them (zeros stand in their place)
  std::vector<size_t> o_val(L.n);
  const size_t val_block = hc.st.reserve((size_t)L.n * count * 32);
  for (uint32_t i = 0; i < L.n; i++) o_val[i] = val_block + (size_t)i * count * 32;
  const size_t o_D = hc.in(q.D, 1), o_A = hc.in(q.A, L.h), o_B = hc.in(q.B, L.h), o_ch = hc.in(q.challenge, 1), o_rs = hc.in(q.responses, request_n_responses),
               o_tw = hc.in(rnd->t_wide, 1, 64), o_uw = hc.in(rnd->U_wide, 1, 64), o_rw = hc.in(rnd->rprime_wide, 1, 64), o_seed = hc.in(rnd->rng_seed, 1);
  const size_t r_t = hc.res(out->t, 1), r_U = hc.res(out->U, 1), r_S1 = hc.res(out->S1, 1), r_S2 = hc.res(out->S2, 1), r_ch = hc.res(out->challenge, 1),
               r_rs = hc.res(out->responses, nr), o_st = hc.res(status, 1, 1);
  int rc = hc.st.upload();
  if (rc) return rc;
  for (uint32_t i = 0; i < L.n; i++)
    if (L.slot[i] < 0) AFX_HIP(hipMemcpyAsync(hc.st.dev(o_val[i]), attrs->values + (size_t)i * count * 32, count * 32, hipMemcpyHostToDevice, hc.st.stream()));
  afx_attributes_soa da = *attrs;
  da.values = hc.st.dev(val_block);
  const afx_blind_request_soa dq = { hc.st.dev(o_D), hc.st.dev(o_A), hc.st.dev(o_B), hc.st.dev(o_ch), hc.st.dev(o_rs) };
  const afx_blind_issue_randomness dr = { hc.st.dev(o_tw), hc.st.dev(o_uw), hc.st.dev(o_rw), hc.st.dev(o_seed) };
  const afx_blind_issuance_soa dout = { hc.st.dev(r_t), hc.st.dev(r_U), hc.st.dev(r_S1), hc.st.dev(r_S2), hc.st.dev(r_ch), hc.st.dev(r_rs) };
  if ((rc = afx_issue_blind_dev(ctx, &da, &dq, request_n_responses, &dr, count, &dout, hc.st.dev(o_st)))) return rc;
  return hc.fetch();
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_unblind_issuances(afx_ctx* ctx, const afx_attributes_soa* attrs, const uint8_t* d, const afx_blind_request_soa* requests,
                                     const afx_blind_issuance_soa* issuances, uint32_t n_responses, size_t count, uint8_t* V, uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !attrs || !requests || !issuances || !V || !status) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  const Layout L(*attrs);
  if (!L.fits(ctx) || n_responses != ctx->n + 6) { memset(status, AFX_ST_VERIFICATION_FAILURE, count); zero_host(V, 1, count); return AFX_OK; }
  const afx_blind_request_soa& q = *requests;
  const afx_blind_issuance_soa& s = *issuances;
  if ((L.revealed() && !attrs->values) || !d || !q.D || (L.h && (!q.A || !q.B)) || !s.t || !s.U || !s.S1 || !s.S2 || !s.challenge || !s.responses) {
    set_error("null batch array");
    return AFX_E_BAD_ARGS;
  }
  AFX_HIP(hipSetDevice(ctx->device));
  HostCall hc(ctx, count, 0);
  const size_t o_val = hc.in(attrs->values, L.n), o_d = hc.in(d, 1), o_D = hc.in(q.D, 1), o_A = hc.in(q.A, L.h), o_B = hc.in(q.B, L.h), o_t = hc.in(s.t, 1),
               o_U = hc.in(s.U, 1), o_S1 = hc.in(s.S1, 1), o_S2 = hc.in(s.S2, 1), o_ch = hc.in(s.challenge, 1), o_rs = hc.in(s.responses, n_responses);
  const size_t r_V = hc.res(V, 1), o_st = hc.res(status, 1, 1);
  int rc = hc.st.upload();
  if (rc) return rc;
  afx_attributes_soa da = *attrs;
  da.values = attrs->values ? hc.st.dev(o_val) : nullptr;
  const afx_blind_request_soa dq = { hc.st.dev(o_D), hc.st.dev(o_A), hc.st.dev(o_B), nullptr, nullptr };
  const afx_blind_issuance_soa di = { hc.st.dev(o_t), hc.st.dev(o_U), hc.st.dev(o_S1), hc.st.dev(o_S2), hc.st.dev(o_ch), hc.st.dev(o_rs) };
  if ((rc = afx_unblind_issuances_dev(ctx, &da, hc.st.dev(o_d), &dq, &di, n_responses, count, hc.st.dev(r_V), hc.st.dev(o_st)))) return rc;
  return hc.fetch();
} catch (...) { return afx::exception_rc(); }
