// Issuer::issue over serialized requests (include/aeonflux_gpu.h "AFXR" v1, afx_issue_wire): request bytes in, AFXI response bytes
// out.  /root/reference/src/issuer.rs:111-124 takes one CredentialRequest; the crate serialises none (src/user.rs:137-139), so AFXR is
// the engine's own, in the style of AFXP / AFXI.  The request records are transposed to struct-of-arrays on the GPU (k_aos_to_soa),
// afx_issue_dev writes its outputs into the rows in front of the attribute values, and k_soa_to_aos turns the whole region back into
// AFXI records - zeros for an item that failed - which come back in one fetch.  Only bytes move on the host.
// Splitting the stream, merging its sections by layout, the answers' headers and the group form are request_stream.hpp's, shared with
// wire_blind.cpp; the AFXR header is an entry of wire_formats.hpp's table and the two transpositions are records.hpp's.  This file says
// what an AFXR door is (request_door) and what it stages and launches (issue_records), and holds the format's C functions.
#include <string>
#include <vector>
#include "records.hpp"
#include "request_stream.hpp"

namespace {

int issue_records(afx_ctx* ctx, const Batch& B, size_t first, size_t n);
// The AFXR door (request_stream.hpp): a request record holds the attribute values only, an AFXI record is t | U | V | challenge |
// responses[ctx n + 5] | values[n], and a request takes t_wide, U_wide and rng_seed.  rnd == null: every column null (the _rng forms).
Door request_door(const afx_issue_randomness* rnd) {
  Door d = {};
  d.in = &FORMATS[AFXR]; d.out = &FORMATS[AFXI];   // (an AFXR request carries no proof: its sections' nrq is 0)
  d.cells_in = [](uint32_t n, uint32_t, uint32_t) { return n; };
  d.cells_out = [](uint32_t n, uint32_t ctx_n) { return 4 + (ctx_n + 5) + n; };
  d.n_responses = [](uint32_t ctx_n) { return ctx_n + 5; };
  d.rnd[0] = { rnd ? rnd->t_wide : nullptr, 64 }; d.rnd[1] = { rnd ? rnd->U_wide : nullptr, 64 }; d.rnd[2] = { rnd ? rnd->rng_seed : nullptr, 32 };
  d.n_rnd = 3;
  d.rnd_for_any_stream = false;   // (a stream with nothing for the GPU reads no randomness)
  d.foreign_status = AFX_ST_MAC_CREATION;
  d.issue = true;
  d.needs_key = "Issuer::issue needs the issuer key";
  d.collected = true;   // as afx_issue_mixed runs its groups: the collector, or a session of the request's own
  d.run = issue_records;
  return d;
}

// Items [first, first + n) of a batch.  Per pass, one region of scratch holds the rows t | U | V | challenge | responses[nr] | values[n]:
// k_aos_to_soa fills the values (after the upload; under a Session: the session's `pre`), afx_issue_dev the rows in front of them, and
// k_soa_to_aos copies the region out as AFXI records (right after the plan, or the session's `post`), fetched in one piece.
int issue_records(afx_ctx* ctx, const Batch& B, size_t first, size_t n) {
  CtxLock lock__(ctx, true);
  if (n == 0) return AFX_OK;
  AFX_HIP(hipSetDevice(ctx->device));
  if (!ctx->has_key) { set_error("Issuer::issue needs the issuer key"); return AFX_E_NO_KEY; }
  if (B.n != ctx->n) { set_error("internal: request layout of another context"); return AFX_E_BAD_ARGS; }
  const uint32_t na = B.n, nr = ctx->n + 5, cells = 4 + nr + na;
  // a request record holds the values only; an AFXI record is the region's rows in order
  const std::vector<uint32_t> map_in = identity_map(na, 4 + nr), map_out = identity_map(cells);
  struct { uint32_t n; uint8_t kinds[AFX_MAX_ATTRIBUTES]; } jd;   // what makes two calls one pass (statements.hpp host_pipe)
  memset(&jd, 0, sizeof jd);
  jd.n = na; memcpy(jd.kinds, B.kinds, AFX_MAX_ATTRIBUTES);
  const PlanKey jkey = plan_key(B.seed40 ? "IWR" : "IW", &jd, sizeof jd, mode_flags(ctx));
  const size_t total = B.count;
  return host_pipe(ctx, n, [&](Stager& st, size_t off, size_t sn) -> int {
    const size_t f0 = first + off;
    st.layout_tag = B.seed40 ? 4 : 2;
    const size_t dn = st.dev_items(sn);
    const size_t o_rec = st.add_rows(B.rec, 1, (size_t)na * 32, total, f0, sn, dn), o_min = st.add((const uint8_t*)map_in.data(), 4 * (size_t)na),
                 o_mout = st.add((const uint8_t*)map_out.data(), 4 * (size_t)cells);
    size_t o_tw, o_uw, o_seed;
    if (B.seed40) {   // drawn on the device after the upload, into the rows k_reduce_wide, k_from_uniform and k_hash read
      const size_t s_at = st.add_seed(B.seed40, dn);
      o_tw = st.add_drawn(s_at, AFX_DRAW_T_WIDE, 1, B.draws, f0, sn, dn);
      o_uw = st.add_drawn(s_at, AFX_DRAW_U_WIDE, 1, B.draws, f0, sn, dn);
      o_seed = st.add_drawn(s_at, AFX_DRAW_ISSUE_SEED, 1, B.draws, f0, sn, dn);
    } else {
      o_tw = st.add_rows(B.rnd[0], 1, 64, total, f0, sn, dn);
      o_uw = st.add_rows(B.rnd[1], 1, 64, total, f0, sn, dn);
      o_seed = st.add_rows(B.rnd[2], 1, 32, total, f0, sn, dn);
    }
    const size_t o_soa = st.reserve(dn * cells * 32), o_out = st.add_rows(nullptr, 1, (size_t)cells * 32, total, f0, sn, dn), o_st = st.add(nullptr, dn);
    st.plan_fetch(B.out, o_out, 1, (size_t)cells * 32, total, f0, sn, dn);
    st.plan_fetch(B.status, o_st, 1, 1, total, f0, sn, dn);
    int rc = st.upload();
    if (rc) return rc;
    if ((rc = transpose_in(st, o_rec, o_soa, o_min, na, dn))) return rc;
    uint8_t* soa_d = st.dev(o_soa);
    auto rowp = [&](uint32_t r) { return soa_d + (size_t)r * dn * 32; };
    afx_attributes_soa da;
    memset(&da, 0, sizeof da);
    da.n_attributes = na; memcpy(da.kinds, B.kinds, AFX_MAX_ATTRIBUTES);
    da.values = rowp(4 + nr);
    const afx_issue_randomness dr = { st.dev(o_tw), st.dev(o_uw), st.dev(o_seed) };
    const afx_issuance_soa dout = { rowp(0), rowp(1), rowp(2), rowp(3), rowp(4) };
    if ((rc = afx_issue_dev(ctx, &da, &dr, dn, &dout, st.dev(o_st)))) return rc;
    if ((rc = transpose_out(st, o_soa, o_out, o_mout, o_st, cells, dn))) return rc;
    return st.fetch_all();
  }, jkey);
}

}  // namespace

// ---- the AFXR format (wire_formats.hpp): host only, bytes only ----
extern "C" size_t afx_request_wire_header_bytes(uint32_t n_attributes) { return header_bytes(FORMATS[AFXR], n_attributes); }

extern "C" int afx_request_wire_parse(const uint8_t* blob, size_t len, uint32_t* n_out, uint8_t kinds_out[AFX_MAX_ATTRIBUTES], size_t* count_out,
                                      size_t* records_offset_out) try {
  uint32_t no_responses;
  return parse_layout(FORMATS[AFXR], blob, len, n_out, kinds_out, &no_responses, count_out, records_offset_out);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_request_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out) try {
  return section_bytes(FORMATS[AFXR], blob, len, section_len_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_request_wire_pack(const afx_attributes_soa* requests, size_t count, uint8_t* blob, size_t blob_cap, size_t* len_out) try {
  if (!requests || !len_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  const uint32_t n = requests->n_attributes;
  const size_t hdr = afx_request_wire_header_bytes(n);
  if (hdr == 0 || count > 0xffffffffu) { set_error("layout out of range"); return AFX_E_BAD_ARGS; }
  const size_t len = hdr + count * n * 32;
  *len_out = len;
  if (!blob) return AFX_OK;   // size query
  if (blob_cap < len) { set_error("blob buffer too small"); return AFX_E_BAD_ARGS; }
  if (count && n && !requests->values) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
  for (uint32_t i = 0; i < n; i++)
    if (requests->kinds[i] > AFX_ATTR_SECRET_POINT) { set_error("attribute kind out of range"); return AFX_E_BAD_ARGS; }
  write_header(FORMATS[AFXR], blob, count, n, n, 0, requests->kinds);
  uint8_t* rec = blob + hdr;
  for (size_t i = 0; i < count; i++)
    for (uint32_t c = 0; c < n; c++, rec += 32) memcpy(rec, requests->values + ((size_t)c * count + i) * 32, 32);
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }

// ---- the doors (request_stream.hpp) ----
extern "C" int afx_issue_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_issue_randomness* rnd, uint8_t* out, size_t out_cap, size_t* out_len,
                              uint8_t* status, size_t status_cap, size_t* count_out) try {
  return door(ctx, request_door(rnd), blob, len, nullptr, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_issue_wire_rng(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_device_rng* rng, uint8_t* out, size_t out_cap,
                                  size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  if (!rng) { set_error("null device rng"); return AFX_E_BAD_ARGS; }
  DrawSeed seed;
  int rc = out ? seed.init(rng) : AFX_OK;   // (the size query draws nothing)
  if (rc) return rc;
  return door(ctx, request_door(nullptr), blob, len, seed.b, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

// The same stream over a group's devices (request_stream.hpp group_door): a small stream goes whole to ONE member, the next in turn; a
// larger one has every batch split over the members.
extern "C" int afx_group_issue_wire(afx_group* group, const uint8_t* blob, size_t len, const afx_issue_randomness* rnd, uint8_t* out, size_t out_cap,
                                    size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  return group_door(group, request_door(rnd), blob, len, nullptr, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_group_issue_wire_rng(afx_group* group, const uint8_t* blob, size_t len, const afx_device_rng* rng, uint8_t* out, size_t out_cap,
                                        size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  if (!rng) { set_error("null device rng"); return AFX_E_BAD_ARGS; }
  DrawSeed seed;   // one seed for the whole group call: every member indexes by the request's ordinal in the stream
  int rc = out ? seed.init(rng) : AFX_OK;
  if (rc) return rc;
  return group_door(group, request_door(nullptr), blob, len, seed.b, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

// Device draws straight into a host array (include/aeonflux_gpu.h afx_rng_expand): k_draw into an output row of the staging area,
// fetched like any result; large counts go through the two lanes in slices.
static_assert(sizeof(size_t) == sizeof(uint64_t), "afx_rng_expand takes a 64-bit index as size_t");
extern "C" int afx_rng_expand(afx_ctx* ctx, const afx_device_rng* rng, uint32_t label, size_t first, size_t count, uint8_t* out) try {
  if (!ctx || !rng || (!out && count)) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (label > AFX_DRAW_ENC_SEED(AFX_MAX_ATTRIBUTES - 1)) { set_error("draw label out of range"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  DrawSeed seed;
  int rc = seed.init(rng);
  if (rc) return rc;
  CtxLock lock__(ctx);
  AFX_HIP(hipSetDevice(ctx->device));
  const size_t len = AFX_DRAW_BYTES(label);
  return host_pipe(ctx, count, [&](Stager& st, size_t off, size_t sn) -> int {
    const size_t dn = st.dev_items(sn);
    const size_t s_at = st.add_seed(seed.b, dn), o_out = st.add_rows(nullptr, 1, len, count, off, sn, dn);
    st.draw(s_at, o_out, label, first + off, sn);
    st.plan_fetch(out, o_out, 1, len, count, off, sn, dn);
    const int r = st.upload();
    return r ? r : st.fetch_all();
  });
} catch (...) { return afx::exception_rc(); }
