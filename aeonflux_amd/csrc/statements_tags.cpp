// Presentation tags (include/aeonflux_gpu.h "Presentation tags"): a show that also carries T = (m + n)^-1 * H for a hidden scalar
// attribute m, a public counter n and a scope generator H, with a proof that T was made from the attribute the MAC covers; the
// issuer's verification of both; the tag proofs alone.  The crate has no counterpart.
//
// This file holds the entry points and what runs in front of the passes: the scope generator goes to the lane's tag buffer (a lane that
// holds this H already copies nothing and waits for nothing), is tested once (k_tag_scope_check; a repeated H is remembered) and
// written into one cell per item (k_tag_broadcast), and a show's (m + n)^-1 rows are made by ONE k_sc_invert launch (tags.cuh) - the way
// the batchable verifier's weights are drawn before its passes.  The plans are the show and verify plans themselves with one more
// argument (statements_prove.cpp show_dev_impl, statements.cpp add_tagproof_verify).
// Where the cells and rows lie: a _dev call's in the lane's tag buffer; a host-pointer call's in scratch of its own staging, so that
// its plan names only addresses the relocation knows and small calls keep their plans (run_chunked keeps no plan of a _dev call).
#include "statements.hpp"
#include "batch_arrays.hpp"

namespace {
// H -> the lane's buffer; H_rows[i] = H for i < count; inv[i] = (m[i] + n[i])^-1 when m_dev is given.  Refuses an H that is the identity
// encoding or does not decode, before anything is written to the caller's arrays.  H_dst / inv_dst: where the cells and rows go
// ([count][32] device scratch of the caller's), or null: behind H in the lane's buffer.  stream_out: the stream it all ran on.
int tag_rows(afx_ctx* ctx, const uint8_t* H, const uint8_t* m_dev, const uint8_t* n_dev, size_t count, uint8_t* H_dst, uint8_t* inv_dst, const uint8_t** H_rows,
             uint8_t** inv, hipStream_t* stream_out = nullptr) {
  if (!afxk_tag_broadcast || !afxk_sc_invert || !afxk_tag_scope_check) { set_error("presentation tags: no k_sc_invert launcher in this build"); return AFX_E_NO_DEVICE; }
  if (count > 0xffffffffull) { set_error("too many items in one call"); return AFX_E_BAD_ARGS; }
  bool nz = false;
  for (int i = 0; i < 32; i++) nz |= H[i] != 0;
  if (!nz) { set_error("the scope generator is the identity encoding"); return AFX_E_BAD_ARGS; }
  AFX_HIP(hipSetDevice(ctx->device));
  afx::Session* ses = (ctx->session && !ctx->session->paused) ? ctx->session : nullptr;
  const int lane = ses ? ses->lane : (ctx->force_lane >= 0 ? ctx->force_lane : (ctx->pipelining ? (int)(ctx->lane_next & 1u) : 0));   // run_chunked's choice
  afx_ctx::Lane& L = ctx->lane[lane];
  if (stream_out) *stream_out = L.stream;
  // (a buffer that grows is a NEW buffer - zeroed, freed, allocated again, possibly at the old address: what it held is gone)
  const size_t cap_before = L.tags.cap;
  int rc = L.tags.ensure(256 + (H_dst ? 0 : 32 * count) + (inv_dst || !m_dev ? 0 : 32 * count));
  if (rc || L.tags.cap != cap_before) L.tags_H_valid = false;
  if (rc) return rc;
  if (!L.tags_pin) AFX_HIP(hipHostMalloc(&L.tags_pin, 64, hipHostMallocDefault));
  if (!L.tags_copied) AFX_HIP(hipEventCreateWithFlags(&L.tags_copied, hipEventDisableTiming));
  uint8_t* pin = (uint8_t*)L.tags_pin;
  uint8_t* d_H = (uint8_t*)L.tags.p;
  const bool known = ctx->tag_scope_known && memcmp(ctx->tag_scope_checked.data(), H, 32) == 0;
  // the lane's buffer holds this very H from an earlier call (and the buffer has not been replaced since): nothing to copy, nothing to
  // wait for - back-to-back _dev calls of one scope queue up behind each other
  const bool resident = known && L.tags_H_valid && memcmp(L.tags_H.data(), H, 32) == 0;
  if (!resident) {
    L.tags_H_valid = false;
    memcpy(pin, H, 32);
    pin[32] = 0;
    AFX_HIP(hipMemcpyAsync(d_H, pin, 32, hipMemcpyHostToDevice, L.stream));
  }
  if (!resident && !known) {
    // one decoding of H, its verdict back: the only round trip of a tagged call, and only for an H the context has not just seen
    AFX_HIP(afxk_tag_scope_check(L.stream, d_H, d_H + 32));
    AFX_HIP(hipMemcpyAsync(pin + 32, d_H + 32, 1, hipMemcpyDeviceToHost, L.stream));
    AFX_HIP(hipStreamSynchronize(L.stream));
    if (pin[32] != 1) { set_error("the scope generator does not decode"); return AFX_E_BAD_ARGS; }
    memcpy(ctx->tag_scope_checked.data(), H, 32);
    ctx->tag_scope_known = true;
  } else if (!resident) {
    AFX_HIP(hipEventRecord(L.tags_copied, L.stream));
    AFX_HIP(hipEventSynchronize(L.tags_copied));   // the pinned image is free for the next call
  }
  if (!resident) { memcpy(L.tags_H.data(), H, 32); L.tags_H_valid = true; }
  uint8_t* const cells = H_dst ? H_dst : d_H + 256;
  uint8_t* const rows = inv_dst ? inv_dst : cells == H_dst ? d_H + 256 : d_H + 256 + 32 * count;
  AFX_HIP(afxk_tag_broadcast(L.stream, d_H, cells, (uint32_t)count));
  if (m_dev) {
    afx_ctx::TimedLaunch tl = { (int)afx::T_SC_INVERT, nullptr, nullptr };   // afx_ctx_get_timing "k_sc_invert"
    if (ctx->timing) {
      for (hipEvent_t* e : { &tl.start, &tl.stop }) {
        if (ctx->event_pool.empty()) AFX_HIP(hipEventCreate(e));
        else { *e = ctx->event_pool.back(); ctx->event_pool.pop_back(); }
      }
      AFX_HIP(hipEventRecord(tl.start, L.stream));
    }
    AFX_HIP(afxk_sc_invert(L.stream, m_dev, n_dev, rows, (uint32_t)count));
    if (ctx->timing) {
      AFX_HIP(hipEventRecord(tl.stop, L.stream));
      ctx->timed.push_back(tl);
    }
  }
  *H_rows = cells;
  if (inv) *inv = rows;
  return AFX_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// H = RistrettoPoint::hash_from_bytes::<Sha512>(scope): the SHA-512 and Elligator plans at count 1
// ------------------------------------------------------------------------------------------------
extern "C" int afx_tag_scope_generator(afx_ctx* ctx, const uint8_t* scope, size_t scope_len, uint8_t out[32]) try {
  if (!ctx || !out || (scope_len && !scope)) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (scope_len > 1024) { set_error("scope longer than 1024 bytes"); return AFX_E_BAD_ARGS; }
  uint8_t wide[64];
  const uint8_t none = 0;
  int rc = afx_sha512(ctx, scope_len ? scope : &none, scope_len, 1, wide);
  if (rc) return rc;
  return afx_points_from_uniform_bytes(ctx, wide, 1, out);
} catch (...) { return afx::exception_rc(); }

// ------------------------------------------------------------------------------------------------
// show
// ------------------------------------------------------------------------------------------------
// H_dst, inv_dst: scratch of a host-pointer call's staging for the cells of H and the inverse rows, or null (the lane's buffer)
static int show_tagged_dev_impl(afx_ctx* ctx, const afx_credentials_soa* creds, const afx_keypairs_soa* keypairs, const afx_show_randomness* rnd,
                                const afx_tag_statement* tag, const uint8_t* nonce, const uint8_t* tag_seed, size_t count, const afx_presentation_out* out,
                                const afx_tags_out* tags_out, afx_shape* shape_out, uint8_t* status_dev, uint8_t* H_dst, uint8_t* inv_dst) {
  CtxLock lock__(ctx);
  if (!ctx || !creds || !rnd || !tag || !out || !tags_out || !shape_out || !status_dev || !tag->scope_generator) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  TagShow ts;
  memset(&ts, 0, sizeof ts);
  ts.position = tag->position;
  if (count == 0) return show_dev_impl(ctx, creds, keypairs, rnd, 0, out, nullptr, shape_out, status_dev, &ts);   // the position's kind is still tested, the shape reported
  if (ts.position >= creds->n_attributes || ts.position >= AFX_MAX_ATTRIBUTES || creds->kinds[ts.position] != AFX_ATTR_SECRET_SCALAR) {
    set_error("a tag needs the position of a hidden scalar attribute");
    return AFX_E_BAD_ARGS;
  }
  if (!creds->values || !nonce || !tag_seed || any_null(*tags_out, Dims())) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
  hipStream_t stream = nullptr;
  int rc = tag_rows(ctx, tag->scope_generator, creds->values + (size_t)ts.position * count * 32, nonce, count, H_dst, inv_dst, &ts.H_rows, &ts.inv, &stream);
  if (rc) return rc;
  ts.nonce = nonce; ts.seed = tag_seed;
  ts.T = tags_out->T; ts.challenge = tags_out->challenge; ts.responses = tags_out->responses;
  try {
    rc = show_dev_impl(ctx, creds, keypairs, rnd, count, out, nullptr, shape_out, status_dev, &ts);
  } catch (...) { rc = afx::exception_rc(); }
  // a call that ends before its plan ran (a null array, a plan that could not be placed) has still made the inverse rows: zeroed here, in
  // stream order, as the plan would have
  if (rc) (void)hipMemsetAsync(ts.inv, 0, 32 * count, stream);
  return rc;
}
extern "C" int afx_show_tagged_dev(afx_ctx* ctx, const afx_credentials_soa* creds, const afx_keypairs_soa* keypairs, const afx_show_randomness* rnd,
                                   const afx_tag_statement* tag, const uint8_t* nonce, const uint8_t* tag_seed, size_t count, const afx_presentation_out* out,
                                   const afx_tags_out* tags_out, afx_shape* shape_out, uint8_t* status_dev) try {
  return show_tagged_dev_impl(ctx, creds, keypairs, rnd, tag, nonce, tag_seed, count, out, tags_out, shape_out, status_dev, nullptr, nullptr);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_show_tagged(afx_ctx* ctx, const afx_credentials_soa* creds, const afx_keypairs_soa* keypairs, const afx_show_randomness* rnd,
                               const afx_tag_statement* tag, const uint8_t* nonce, const uint8_t* tag_seed, size_t count, const afx_presentation_out* out,
                               const afx_tags_out* tags_out, afx_shape* shape_out, uint8_t* status) try {
  CtxLock lock__(ctx);   // (a tagged call takes the context in turn: it joins no collecting session)
  if (!ctx || !creds || !rnd || !tag || !out || !tags_out || !shape_out || !status || !tag->scope_generator) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return afx_show_tagged_dev(ctx, creds, keypairs, rnd, tag, nonce, tag_seed, 0, out, tags_out, shape_out, status);
  const uint32_t na = creds->n_attributes;
  if (na == 0 || na > ctx->n) { set_error("credential attribute count does not fit the system parameters"); return AFX_E_BAD_ARGS; }
  const Dims dm = dims_of(*creds);
  if (any_null(*creds, dm) || any_null(*rnd, dm) || any_null(*out, outputs(dm)) || (dm.proofs && !out->enc) || !nonce || !tag_seed || any_null(*tags_out, dm)) {
    set_error("null batch array");
    return AFX_E_BAD_ARGS;
  }
  const bool kp = keypairs && dm.proofs;
  if (kp && any_null(*keypairs, dm)) { set_error("null keypair array"); return AFX_E_BAD_ARGS; }
  if (any_null_with_proofs(*out, outputs(dm))) { set_error("null batch array"); return AFX_E_BAD_ARGS; }   // (the proofs' arrays)
  AFX_HIP(hipSetDevice(ctx->device));
  HostCall hc(ctx, count, 14);   // (a staging layout of its own: part of the plan-cache key)
  auto in = [&](const uint8_t* p, size_t rows, size_t elem) { const size_t o = hc.in(p, rows, elem); return p ? o : NO_ARRAY; };
  auto res = [&](uint8_t* dst, size_t rows, size_t elem) { const size_t o = hc.res(dst, dst ? rows : 0, elem); return dst ? o : NO_ARRAY; };   // (attr_values may be absent)
  const Offsets<afx_credentials_soa> oc = stage(*creds, dm, in);
  const Offsets<afx_show_randomness> orn = stage(*rnd, dm, in);
  const size_t o_n = hc.in(nonce, 1), o_ts = hc.in(tag_seed, 1);
  Offsets<afx_keypairs_soa> ok;
  if (kp) stage(ok, *keypairs, dm, in);
  const Offsets<afx_presentation_out> om = stage(*out, dm, res);
  const Offsets<afx_tags_out> ot = stage(*tags_out, dm, res);
  const size_t o_st = hc.res(status, 1, 1);
  std::vector<Offsets<afx_encproof_out>> oe(dm.proofs);
  for (uint32_t e = 0; e < dm.proofs; e++) stage(oe[e], out->enc[e], dm, res);
  const size_t o_H = hc.st.reserve(32 * count), o_inv = hc.st.reserve(32 * count);   // the cells of H, the inverse rows
  int rc = hc.st.upload();
  if (rc) return rc;
  Stager& st = hc.st;
  const afx_credentials_soa dc = on_device(st, oc, *creds);
  const afx_keypairs_soa dk = on_device(st, ok);
  const afx_show_randomness dr = on_device(st, orn);
  const std::vector<afx_encproof_out> de = on_device(st, oe);
  afx_presentation_out dout = on_device(st, om);
  dout.enc = de.data();
  const afx_tags_out dto = on_device(st, ot);
  if ((rc = show_tagged_dev_impl(ctx, &dc, kp ? &dk : nullptr, &dr, tag, st.dev(o_n), st.dev(o_ts), count, &dout, &dto, shape_out, st.dev(o_st), st.dev(o_H), st.dev(o_inv))))
    return rc;
  return hc.fetch();
} catch (...) { return afx::exception_rc(); }

// ------------------------------------------------------------------------------------------------
// verify
// ------------------------------------------------------------------------------------------------
static int verify_presentations_tagged_dev_impl(afx_ctx* ctx, const afx_shape* shape, const afx_presentation_soa* batch, const afx_tag_statement* tag,
                                               const afx_tags_soa* tags, size_t count, uint8_t* status_dev, uint8_t* H_dst) {
  CtxLock lock__(ctx);
  if (!ctx || !shape || !batch || !tag || !tags || !status_dev || !tag->scope_generator) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (!ctx->has_key) { set_error("Issuer::verify needs the issuer key"); return AFX_E_NO_KEY; }
  if (count == 0) return AFX_OK;
  TagVerify tv;
  memset(&tv, 0, sizeof tv);
  tv.position = tag->position;
  if (tagged_shape_ok(ctx, *shape, tv.position)) {   // (otherwise every item fails and no tag array is read)
    if (any_null(*tags, Dims())) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
    tv.nonce = tags->nonce; tv.T = tags->T; tv.challenge = tags->challenge; tv.responses = tags->responses;
  }
  const int rc = tag_rows(ctx, tag->scope_generator, nullptr, nullptr, count, H_dst, nullptr, &tv.H_rows, nullptr);
  if (rc) return rc;
  return verify_presentations_dev_impl(ctx, shape, batch, count, status_dev, &tv);
}
extern "C" int afx_verify_presentations_tagged_dev(afx_ctx* ctx, const afx_shape* shape, const afx_presentation_soa* batch, const afx_tag_statement* tag,
                                                   const afx_tags_soa* tags, size_t count, uint8_t* status_dev) try {
  return verify_presentations_tagged_dev_impl(ctx, shape, batch, tag, tags, count, status_dev, nullptr);
} catch (...) { return afx::exception_rc(); }

static int verify_tag_proofs_dev_impl2(afx_ctx* ctx, const afx_tag_statement* tag, const uint8_t* C_y_p, const afx_tags_soa* tags, size_t count, uint8_t* status_dev,
                                      uint8_t* H_dst) {
  CtxLock lock__(ctx);
  if (!ctx || !tag || !tags || !status_dev || !tag->scope_generator) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  TagVerify tv;
  memset(&tv, 0, sizeof tv);
  tv.position = tag->position;
  if (tv.position < ctx->n) {
    if (!C_y_p || any_null(*tags, Dims())) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
    tv.nonce = tags->nonce; tv.T = tags->T; tv.challenge = tags->challenge; tv.responses = tags->responses;
  }
  const int rc = tag_rows(ctx, tag->scope_generator, nullptr, nullptr, count, H_dst, nullptr, &tv.H_rows, nullptr);
  if (rc) return rc;
  return verify_tag_proofs_dev_impl(ctx, tv, C_y_p, count, status_dev);
}
extern "C" int afx_verify_tag_proofs_dev(afx_ctx* ctx, const afx_tag_statement* tag, const uint8_t* C_y_p, const afx_tags_soa* tags, size_t count,
                                         uint8_t* status_dev) try {
  return verify_tag_proofs_dev_impl2(ctx, tag, C_y_p, tags, count, status_dev, nullptr);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_verify_tag_proofs(afx_ctx* ctx, const afx_tag_statement* tag, const uint8_t* C_y_p, const afx_tags_soa* tags, size_t count, uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !tag || !tags || !status || !tag->scope_generator) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  AFX_HIP(hipSetDevice(ctx->device));
  if (tag->position >= ctx->n) {   // every item fails and no array is read; a bad H is refused all the same, as everywhere
    const uint8_t* none = nullptr;
    const int rc0 = tag_rows(ctx, tag->scope_generator, nullptr, nullptr, 0, nullptr, nullptr, &none, nullptr);
    if (rc0) return rc0;
    memset(status, AFX_ST_VERIFICATION_FAILURE, count);
    return AFX_OK;
  }
  if (!C_y_p || any_null(*tags, Dims())) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
  HostCall hc(ctx, count, 14);   // (a staging layout of its own: part of the plan-cache key)
  const size_t o_cy = hc.in(C_y_p, 1), o_n = hc.in(tags->nonce, 1), o_T = hc.in(tags->T, 1), o_ch = hc.in(tags->challenge, 1), o_rs = hc.in(tags->responses, 2),
               o_st = hc.res(status, 1, 1);
  const size_t o_H = hc.st.reserve(32 * count);   // the cells of H
  int rc = hc.st.upload();
  if (rc) return rc;
  const afx_tags_soa dt = { hc.st.dev(o_n), hc.st.dev(o_T), hc.st.dev(o_ch), hc.st.dev(o_rs) };
  if ((rc = verify_tag_proofs_dev_impl2(ctx, tag, hc.st.dev(o_cy), &dt, count, hc.st.dev(o_st), hc.st.dev(o_H)))) return rc;
  return hc.fetch();
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_verify_presentations_tagged(afx_ctx* ctx, const afx_shape* shape, const afx_presentation_soa* b, const afx_tag_statement* tag,
                                               const afx_tags_soa* tags, size_t count, uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !shape || !b || !tag || !tags || !status || !tag->scope_generator) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  AFX_HIP(hipSetDevice(ctx->device));
  if (!ctx->has_key) { set_error("Issuer::verify needs the issuer key"); return AFX_E_NO_KEY; }
  // a shape every item fails on says nothing reliable about the arrays' extents: answer without reading them
  // (a bad H is refused all the same, as everywhere)
  if (!afx_batchable_main_commitments(ctx, shape) || !tagged_shape_ok(ctx, *shape, tag->position)) {
    const uint8_t* none = nullptr;
    const int rc0 = tag_rows(ctx, tag->scope_generator, nullptr, nullptr, 0, nullptr, nullptr, &none, nullptr);
    if (rc0) return rc0;
    memset(status, AFX_ST_VERIFICATION_FAILURE, count);
    return AFX_OK;
  }
  const Dims dm = dims_of(*shape);
  if (any_null_with_proofs(*b, dm) || any_null(*tags, dm)) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
  HostCall hc(ctx, count, 14);   // (a staging layout of its own: part of the plan-cache key)
  auto in = [&](const uint8_t* p, size_t rows, size_t elem) { const size_t o = hc.in(p, rows, elem); return p ? o : NO_ARRAY; };
  const Offsets<afx_presentation_soa> om = stage(*b, dm, in);
  const Offsets<afx_tags_soa> ot = stage(*tags, dm, in);
  std::vector<Offsets<afx_encproof_soa>> oe(dm.proofs);
  for (uint32_t e = 0; e < dm.proofs; e++) stage(oe[e], b->enc[e], dm, in);
  const size_t o_st = hc.res(status, 1, 1);
  const size_t o_H = hc.st.reserve(32 * count);   // the cells of H
  int rc = hc.st.upload();
  if (rc) return rc;
  Stager& st = hc.st;
  const std::vector<afx_encproof_soa> de = on_device(st, oe);
  afx_presentation_soa d = on_device(st, om);
  d.enc = de.data();
  const afx_tags_soa dt = on_device(st, ot);
  if ((rc = verify_presentations_tagged_dev_impl(ctx, shape, &d, tag, &dt, count, st.dev(o_st), st.dev(o_H)))) return rc;
  return hc.fetch();
} catch (...) { return afx::exception_rc(); }
