// The issuer's side of blind issuance on bytes (include/aeonflux_gpu.h "Blind issuance on bytes"): AFXQ request sections in, AFXJ
// issuance sections out, and the request's verification alone over the same sections.  The doors are request_stream.hpp's, as
// wire_issue.cpp's are; the two headers are entries of wire_formats.hpp's table, whose C functions stand here; the transpositions and
// their cell maps are records.hpp's (this file says what an AFXQ door is: blind_door, and what it stages and launches: run_records): the records of
// one layout are transposed to struct-of-arrays rows on the GPU (k_aos_to_soa), afx_issue_blind_dev runs on those rows and writes its
// outputs into further rows of the same region, and k_soa_to_aos turns those into AFXJ records - zeros for an item that failed - which
// come back in one fetch.  Only bytes move on the host.  The explicit form takes its four draws per request from host arrays, the
// _rng form has k_draw write them into the rows the plan reads (labels AFX_DRAW_BLIND_*).
// A call takes the context in turn and stages slice after slice on the two lanes (host_pipe); it never hands a small call to the
// collector of other threads' calls: blind issuance plans are not laid out for shared item slots.
#include <string>
#include <vector>
#include "records.hpp"
#include "request_stream.hpp"

namespace {

// Items [first, first + n) of a batch.  Per pass, one region of scratch holds the rows
//   D | A[h] | B[h] | challenge | responses[1 + h + hs] | values[n] | t | U | S1 | S2 | challenge | responses[n + 6]
// k_aos_to_soa fills the request rows and the value rows of the revealed positions (the rows of hidden positions are part of the
// region and are never read), afx_issue_blind_dev reads those and writes the rows behind them, and k_soa_to_aos copies the last
// n + 11 rows out as AFXJ records, fetched in one piece.  B.out == null: afx_verify_blind_requests_dev on the request rows, statuses
// only.  Two transposition launches per pass beyond the plan (one for the verification alone).
int run_records(afx_ctx* ctx, const Batch& B, size_t first, size_t n) {
  CtxLock lock__(ctx);   // the context in turn: no session of the collector collects or is in flight from here on
  if (n == 0) return AFX_OK;
  AFX_HIP(hipSetDevice(ctx->device));
  const bool issue = B.out != nullptr;
  if (issue && !ctx->has_key) { set_error("blind issuance needs the issuer key"); return AFX_E_NO_KEY; }
  if (B.n != ctx->n) { set_error("internal: request layout of another context"); return AFX_E_BAD_ARGS; }
  const uint32_t na = B.n, h = B.h, rq = 3 + 3 * h + B.hs, cells_in = B.cells_in, out_cells = issue ? na + 11 : 0, rows = rq + na + out_cells;
  // D, A, B, challenge, responses: the record's order is the rows' order; a revealed value lands on the row of its position
  const std::vector<uint32_t> map_in = blind_request_map(B.kinds, na, rq, 0, rq);
  const std::vector<uint32_t> map_out = issue ? identity_map(out_cells, rq + na) : std::vector<uint32_t>(1);   // (the verification alone stages one unused word)
  if (map_in.size() != cells_in) { set_error("internal: AFXQ cell map"); return AFX_E_BAD_ARGS; }
  const size_t total = B.count;
  return host_pipe(ctx, n, [&](Stager& st, size_t off, size_t sn) -> int {
    if (st.ses || st.app) { set_error("internal: a blind wire call inside a collected session"); return AFX_E_BAD_ARGS; }
    const size_t f0 = first + off;
    st.layout_tag = !issue ? 8 : B.seed40 ? 7 : 6;
    const size_t dn = st.dev_items(sn);
    const size_t o_rec = st.add_rows(B.rec, 1, (size_t)cells_in * 32, total, f0, sn, dn), o_min = st.add((const uint8_t*)map_in.data(), 4 * (size_t)cells_in),
                 o_mout = st.add((const uint8_t*)map_out.data(), 4 * map_out.size());
    size_t o_tw = 0, o_uw = 0, o_rw = 0, o_seed = 0;
    if (issue && B.seed40) {   // drawn on the device after the upload, into the rows k_reduce_wide, k_from_uniform and k_hash read
      const size_t s_at = st.add_seed(B.seed40, dn);
      o_tw = st.add_drawn(s_at, AFX_DRAW_BLIND_T_WIDE, 1, B.draws, f0, sn, dn);
      o_uw = st.add_drawn(s_at, AFX_DRAW_BLIND_U_WIDE, 1, B.draws, f0, sn, dn);
      o_rw = st.add_drawn(s_at, AFX_DRAW_BLIND_RPRIME_WIDE, 1, B.draws, f0, sn, dn);
      o_seed = st.add_drawn(s_at, AFX_DRAW_BLIND_ISSUE_SEED, 1, B.draws, f0, sn, dn);
    } else if (issue) {
      o_tw = st.add_rows(B.rnd[0], 1, 64, total, f0, sn, dn);
      o_uw = st.add_rows(B.rnd[1], 1, 64, total, f0, sn, dn);
      o_rw = st.add_rows(B.rnd[2], 1, 64, total, f0, sn, dn);
      o_seed = st.add_rows(B.rnd[3], 1, 32, total, f0, sn, dn);
    }
    const size_t o_soa = st.reserve(dn * rows * 32);
    const size_t o_out = issue ? st.add_rows(nullptr, 1, (size_t)out_cells * 32, total, f0, sn, dn) : 0, o_st = st.add(nullptr, dn);
    if (issue) st.plan_fetch(B.out, o_out, 1, (size_t)out_cells * 32, total, f0, sn, dn);
    st.plan_fetch(B.status, o_st, 1, 1, total, f0, sn, dn);
    int rc = st.upload();
    if (rc) return rc;
    uint8_t* soa_d = st.dev(o_soa);
    if ((rc = transpose_in(st, o_rec, o_soa, o_min, cells_in, dn))) return rc;   // (never in a session: at once)
    auto rowp = [&](uint32_t r) { return soa_d + (size_t)r * dn * 32; };
    afx_attributes_soa da;
    memset(&da, 0, sizeof da);
    da.n_attributes = na; memcpy(da.kinds, B.kinds, AFX_MAX_ATTRIBUTES);
    da.values = rowp(rq);
    const afx_blind_request_soa dq = { rowp(0), rowp(1), rowp(1 + h), rowp(1 + 2 * h), rowp(2 + 2 * h) };
    if (!issue) {
      if ((rc = afx_verify_blind_requests_dev(ctx, &da, &dq, B.nrq, dn, st.dev(o_st)))) return rc;
      return st.fetch_all();
    }
    const uint32_t o0 = rq + na;
    const afx_blind_issue_randomness dr = { st.dev(o_tw), st.dev(o_uw), st.dev(o_rw), st.dev(o_seed) };
    const afx_blind_issuance_soa dout = { rowp(o0), rowp(o0 + 1), rowp(o0 + 2), rowp(o0 + 3), rowp(o0 + 4), rowp(o0 + 5) };
    if ((rc = afx_issue_blind_dev(ctx, &da, &dq, B.nrq, &dr, dn, &dout, st.dev(o_st)))) return rc;
    if ((rc = transpose_out(st, o_soa, o_out, o_mout, o_st, out_cells, dn))) return rc;
    return st.fetch_all();
  }, PlanKey(), true);   // never collected: a small call too runs its slices itself
}

// The AFXQ door (request_stream.hpp): a request record is D | A[h] | B[h] | challenge | responses[1 + h + hs] | the revealed values, an
// AFXJ record is t | U | S1 | S2 | challenge | responses[ctx n + 6], and a request takes t_wide, U_wide, rprime_wide and rng_seed.
// rnd == null: every column null (the _rng form, and the verification alone).  issue == false: afx_verify_blind_requests_wire.
// Several batches run one after another: run_records never hands a call to the collector.
Door blind_door(const afx_blind_issue_randomness* rnd, bool issue) {
  Door d = {};
  d.in = &FORMATS[AFXQ]; d.out = &FORMATS[AFXJ];
  d.cells_in = [](uint32_t n, uint32_t h, uint32_t hs) { return 3 + 2 * h + hs + n; };
  d.cells_out = [](uint32_t, uint32_t ctx_n) { return ctx_n + 11; };
  d.n_responses = [](uint32_t ctx_n) { return ctx_n + 6; };
  d.rnd[0] = { rnd ? rnd->t_wide : nullptr, 64 }; d.rnd[1] = { rnd ? rnd->U_wide : nullptr, 64 };
  d.rnd[2] = { rnd ? rnd->rprime_wide : nullptr, 64 }; d.rnd[3] = { rnd ? rnd->rng_seed : nullptr, 32 };
  d.n_rnd = 4;
  d.rnd_for_any_stream = true;
  d.foreign_status = issue ? AFX_ST_MAC_CREATION : AFX_ST_VERIFICATION_FAILURE;   // afx_issue_blind (amacs.rs:285-287), afx_verify_blind_requests
  d.issue = issue;
  d.needs_key = "blind issuance needs the issuer key";
  d.collected = false;
  d.run = run_records;
  return d;
}

}  // namespace

// ---- the two formats: host only, bytes only ----
extern "C" size_t afx_blind_request_wire_header_bytes(uint32_t n_attributes) { return header_bytes(FORMATS[AFXQ], n_attributes); }
extern "C" size_t afx_blind_issuance_wire_header_bytes(uint32_t n_attributes) { return header_bytes(FORMATS[AFXJ], n_attributes); }

extern "C" int afx_blind_request_wire_parse(const uint8_t* blob, size_t len, uint32_t* n_attributes_out, uint8_t kinds_out[AFX_MAX_ATTRIBUTES],
                                            uint32_t* n_responses_out, size_t* count_out, size_t* records_offset_out) try {
  return parse_layout(FORMATS[AFXQ], blob, len, n_attributes_out, kinds_out, n_responses_out, count_out, records_offset_out);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_blind_issuance_wire_parse(const uint8_t* blob, size_t len, uint32_t* n_attributes_out, uint8_t kinds_out[AFX_MAX_ATTRIBUTES],
                                             uint32_t* n_responses_out, size_t* count_out, size_t* records_offset_out) try {
  return parse_layout(FORMATS[AFXJ], blob, len, n_attributes_out, kinds_out, n_responses_out, count_out, records_offset_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_blind_request_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out) try {
  return section_bytes(FORMATS[AFXQ], blob, len, section_len_out);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_blind_issuance_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out) try {
  return section_bytes(FORMATS[AFXJ], blob, len, section_len_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_blind_request_wire_pack(const afx_attributes_soa* attrs, const afx_blind_request_soa* requests, size_t count, uint8_t* blob, size_t blob_cap,
                                           size_t* len_out) try {
  if (!attrs || !requests || !len_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  const uint32_t n = attrs->n_attributes;
  const size_t hdr = header_bytes(FORMATS[AFXQ], n);
  if (hdr == 0 || count > 0xffffffffu) { set_error("layout out of range"); return AFX_E_BAD_ARGS; }
  for (uint32_t i = 0; i < n; i++)
    if (attrs->kinds[i] > AFX_ATTR_SECRET_POINT) { set_error("attribute kind out of range"); return AFX_E_BAD_ARGS; }
  const Hidden hd = hidden_of(attrs->kinds, n);
  const uint32_t h = hd.h, nr = 1 + hd.h + hd.hs, cells = 3 + 2 * hd.h + hd.hs + n;
  const size_t len = hdr + count * cells * 32;
  *len_out = len;
  if (!blob) return AFX_OK;   // size query
  if (blob_cap < len) { set_error("blob buffer too small"); return AFX_E_BAD_ARGS; }
  const afx_blind_request_soa& q = *requests;
  if (count && (!q.D || !q.challenge || !q.responses || (h && (!q.A || !q.B)) || (n > h && !attrs->values))) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
  write_header(FORMATS[AFXQ], blob, count, cells, n, nr, attrs->kinds);
  uint8_t* rec = blob + hdr;
  auto put = [&](const uint8_t* base, size_t row, size_t i) { memcpy(rec, base + (row * count + i) * 32, 32); rec += 32; };
  for (size_t i = 0; i < count; i++) {
    put(q.D, 0, i);
    for (uint32_t j = 0; j < h; j++) put(q.A, j, i);
    for (uint32_t j = 0; j < h; j++) put(q.B, j, i);
    put(q.challenge, 0, i);
    for (uint32_t k = 0; k < nr; k++) put(q.responses, k, i);
    for (uint32_t p = 0; p < n; p++)
      if (!is_hidden_kind(attrs->kinds[p])) put(attrs->values, p, i);   // (the value rows of hidden positions are not read)
  }
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_blind_issuance_wire_pack(const afx_attributes_soa* attrs, const afx_blind_issuance_soa* issuances, uint32_t n_responses, size_t count,
                                            uint8_t* blob, size_t blob_cap, size_t* len_out) try {
  if (!attrs || !issuances || !len_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  const uint32_t n = attrs->n_attributes;
  const size_t hdr = header_bytes(FORMATS[AFXJ], n);
  if (hdr == 0 || count > 0xffffffffu || n_responses > AFX_MAX_ATTRIBUTES + 6) { set_error("layout out of range"); return AFX_E_BAD_ARGS; }
  for (uint32_t i = 0; i < n; i++)
    if (attrs->kinds[i] > AFX_ATTR_SECRET_POINT) { set_error("attribute kind out of range"); return AFX_E_BAD_ARGS; }
  const uint32_t cells = 5 + n_responses;
  const size_t len = hdr + count * cells * 32;
  *len_out = len;
  if (!blob) return AFX_OK;   // size query
  if (blob_cap < len) { set_error("blob buffer too small"); return AFX_E_BAD_ARGS; }
  const afx_blind_issuance_soa& s = *issuances;
  if (count && (!s.t || !s.U || !s.S1 || !s.S2 || !s.challenge || (n_responses && !s.responses))) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
  write_header(FORMATS[AFXJ], blob, count, cells, n, n_responses, attrs->kinds);
  uint8_t* rec = blob + hdr;
  auto put = [&](const uint8_t* base, size_t row, size_t i) { memcpy(rec, base + (row * count + i) * 32, 32); rec += 32; };
  for (size_t i = 0; i < count; i++) {
    put(s.t, 0, i); put(s.U, 0, i); put(s.S1, 0, i); put(s.S2, 0, i); put(s.challenge, 0, i);
    for (uint32_t k = 0; k < n_responses; k++) put(s.responses, k, i);
  }
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }

// ---- the doors (request_stream.hpp) ----
extern "C" int afx_issue_blind_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_blind_issue_randomness* rnd, uint8_t* out, size_t out_cap,
                                    size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  return door(ctx, blind_door(rnd, true), blob, len, nullptr, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_group_issue_blind_wire(afx_group* group, const uint8_t* blob, size_t len, const afx_blind_issue_randomness* rnd, uint8_t* out, size_t out_cap,
                                          size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  return group_door(group, blind_door(rnd, true), blob, len, nullptr, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_verify_blind_requests_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  return door(ctx, blind_door(nullptr, false), blob, len, nullptr, nullptr, 0, nullptr, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_issue_blind_wire_rng(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_device_rng* rng, uint8_t* out, size_t out_cap, size_t* out_len,
                                        uint8_t* status, size_t status_cap, size_t* count_out) try {
  if (!rng) { set_error("null device rng"); return AFX_E_BAD_ARGS; }
  DrawSeed seed;
  const int rc = out ? seed.init(rng) : AFX_OK;   // (the size query draws nothing)
  if (rc) return rc;
  return door(ctx, blind_door(nullptr, true), blob, len, seed.b, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_group_issue_blind_wire_rng(afx_group* group, const uint8_t* blob, size_t len, const afx_device_rng* rng, uint8_t* out, size_t out_cap,
                                              size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  if (!rng) { set_error("null device rng"); return AFX_E_BAD_ARGS; }
  DrawSeed seed;   // one seed for the whole group call: every member indexes by the request's ordinal in the stream
  const int rc = out ? seed.init(rng) : AFX_OK;
  if (rc) return rc;
  return group_door(group, blind_door(nullptr, true), blob, len, seed.b, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }
