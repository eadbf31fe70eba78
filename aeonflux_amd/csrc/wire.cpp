// The two formats every build of the engine speaks (include/aeonflux_gpu.h "wire format"): AFXP presentation batches and AFXI issuance
// batches.  Their header functions (thin wrappers over wire_formats.hpp's table), the packers that write a batch from the
// struct-of-arrays a prover call returns, and the two verifications on records: the records are transposed to struct-of-arrays rows on
// the GPU (records.hpp) and verified by the *_dev calls.  Only bytes move on the host - the reference defines no serialisation for
// these messages (/root/reference/src/nizk/presentation.rs:117-127, src/issuer.rs:42-45).  The other formats' wrappers stand with
// their doors (wire_issue.cpp, wire_batchable.cpp, wire_blind.cpp).
#include <string.h>
#include "wire_formats.hpp"
#include "records.hpp"
#include "batch_arrays.hpp"

// ---- Presentation batches ("AFXP" v1) ------------------------------------------------------------
extern "C" uint32_t afx_wire_cells_per_record(const afx_shape* sh) { return sh && shape_ok(*sh) ? presentation_cells(*sh, 1, 14) : 0; }
extern "C" size_t afx_wire_header_bytes(const afx_shape* sh) {
  return sh && shape_ok(*sh) ? header_bytes(FORMATS[AFXP], sh->n_attributes, sh->n_hidden_scalars, sh->n_enc_proofs) : 0;
}
extern "C" int afx_wire_parse(const uint8_t* blob, size_t len, afx_shape* shape_out, size_t* count_out, size_t* records_offset_out) try {
  if (!blob || !shape_out || !count_out || !records_offset_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  Header H;
  const int rc = read_header(FORMATS[AFXP], blob, len, H);
  if (rc) return rc;
  *shape_out = shape_of(H);
  *count_out = H.count;
  *records_offset_out = H.hdr;
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out) try {
  return section_bytes(FORMATS[AFXP], blob, len, section_len_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_wire_pack_presentations(const afx_shape* shape, const afx_presentation_soa* batch, size_t count, uint8_t* blob, size_t blob_cap,
                                           size_t* len_out) try {
  if (!shape || !batch || !len_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  const size_t hdr = afx_wire_header_bytes(shape);
  const uint32_t cells = afx_wire_cells_per_record(shape);
  if (hdr == 0 || cells == 0 || count > 0xffffffffu) { set_error("shape out of range"); return AFX_E_BAD_ARGS; }
  const size_t len = hdr + count * cells * 32;
  *len_out = len;
  if (!blob) return AFX_OK;   // size query
  if (blob_cap < len) { set_error("blob buffer too small"); return AFX_E_BAD_ARGS; }
  const afx_shape& sh = *shape;
  const afx_presentation_soa& b = *batch;
  const Dims dm = dims_of(sh);
  if (count && any_null_with_proofs(b, dm)) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
  write_header(FORMATS[AFXP], blob, sh, count, cells);
  if (!count) return AFX_OK;   // (no record: no array is looked at)
  // the record's cells, in order: where each comes from in the struct-of-arrays ([row][count][32])
  std::vector<const uint8_t*> col;
  auto cell = [&](const uint8_t* base, uint32_t r) { col.push_back(base + (size_t)r * count * 32); };
  each_cell(b, dm, cell);
  for (uint32_t e = 0; e < sh.n_enc_proofs; e++) each_cell(b.enc[e], dm, cell);
  if (col.size() != cells) { set_error("internal: wire cell list"); return AFX_E_BAD_ARGS; }
  uint8_t* rec = blob + hdr;
  for (size_t i = 0; i < count; i++)
    for (uint32_t c = 0; c < cells; c++, rec += 32) memcpy(rec, col[c] + i * 32, 32);
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }

// records [first, first + n) of a parsed AFXP batch; status is the whole batch's array (element first + i answers record first + i)
static int verify_wire_records(afx_ctx* ctx, const afx_shape& sh, const uint8_t* records, size_t count, size_t first, size_t n, uint8_t* status) {
  if (n == 0) return AFX_OK;
  AFX_HIP(hipSetDevice(ctx->device));
  const uint32_t cells = afx_wire_cells_per_record(&sh);
  // SoA rows: challenge | responses | C_x_0 C_x_1 C_V | C_y[n] | attr_values[n] (secret rows stay unused) | enc proofs
  const uint32_t na = sh.n_attributes;
  const uint32_t row_resp = 1, row_cx = row_resp + sh.n_responses, row_cy = row_cx + 3, row_av = row_cy + na, row_enc = row_av + na;
  const uint32_t rows = row_enc + 14 * sh.n_enc_proofs;
  const std::vector<uint32_t> map = presentation_map(sh, 1, 14, row_av, row_enc);
  if (map.size() != cells) { set_error("internal: wire cell map"); return AFX_E_BAD_ARGS; }
  // records are contiguous: a slice of the batch is a byte range of the blob; slices alternate between the two lanes like
  // those of the column-array calls (statements.hpp host_pipe), each transposed on the GPU into its own SoA scratch
  const afx_shape jsh = canonical_shape(sh);
  const PlanKey jkey = plan_key("VW", &jsh, sizeof jsh, mode_flags(ctx));
  return host_pipe(ctx, n, [&](Stager& st, size_t off, size_t sn) -> int {
    const size_t f0 = first + off;
    st.layout_tag = 1;
    const size_t dn = st.dev_items(sn);
    const size_t o_rec = st.add_rows(records, 1, (size_t)cells * 32, count, f0, sn, dn), o_map = st.add((const uint8_t*)map.data(), 4 * (size_t)cells),
                 o_soa = st.reserve(dn * rows * 32), o_st = st.add(nullptr, dn);
    st.plan_fetch(status, o_st, 1, 1, count, f0, sn, dn);
    int rc2 = st.upload();
    if (rc2) return rc2;
    if ((rc2 = transpose_in(st, o_rec, o_soa, o_map, cells, dn))) return rc2;
    auto rowp = [&](uint32_t r) { return (const uint8_t*)st.dev(o_soa) + (size_t)r * dn * 32; };
    const Dims dm = dims_of(sh);
    afx_presentation_soa d;
    view_rows(d, dm, rowp, 0);
    std::vector<afx_encproof_soa> encs(sh.n_enc_proofs);
    for (uint32_t e = 0; e < sh.n_enc_proofs; e++) view_rows(encs[e], dm, rowp, row_enc + ENC_ROWS * e);
    d.enc = encs.data();
    if ((rc2 = afx_verify_presentations_dev(ctx, &sh, &d, dn, st.dev(o_st)))) return rc2;
    return st.fetch_all();
  }, jkey);
}
extern "C" int afx_verify_presentations_wire_range(afx_ctx* ctx, const uint8_t* blob, size_t len, size_t first, size_t n, uint8_t* status, size_t status_cap,
                                                   size_t* count_out) try {
  CtxLock lock__(ctx, true);
  if (!ctx || !status || !count_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  afx_shape sh;
  size_t count = 0, off = 0;
  int rc = afx_wire_parse(blob, len, &sh, &count, &off);
  if (rc) return rc;
  *count_out = count;
  if (first > count || n > count - first) { set_error("range outside the batch"); return AFX_E_BAD_ARGS; }
  if (n == 0) return AFX_OK;
  if (status_cap < count) { set_error("status buffer too small"); return AFX_E_BAD_ARGS; }
  if (count > 0xffffffffu / 64) { set_error("batch too large for one call"); return AFX_E_BAD_ARGS; }
  if (!ctx->has_key) { set_error("Issuer::verify needs the issuer key"); return AFX_E_NO_KEY; }
  return verify_wire_records(ctx, sh, blob + off, count, first, n, status);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_verify_presentations_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  if (!count_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  size_t count = 0, hdr = 0;
  afx_shape sh;
  int rc = afx_wire_parse(blob, len, &sh, &count, &hdr);
  if (rc) return rc;
  *count_out = count;
  return afx_verify_presentations_wire_range(ctx, blob, len, 0, count, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

// ---- CredentialIssuance batches ("AFXI" v1) -----------------------------------------------------
extern "C" size_t afx_issuance_wire_header_bytes(uint32_t n_attributes) { return header_bytes(FORMATS[AFXI], n_attributes); }
extern "C" int afx_issuance_wire_parse(const uint8_t* blob, size_t len, uint32_t* n_out, uint8_t kinds_out[AFX_MAX_ATTRIBUTES], uint32_t* nr_out,
                                       size_t* count_out, size_t* records_offset_out) try {
  return parse_layout(FORMATS[AFXI], blob, len, n_out, kinds_out, nr_out, count_out, records_offset_out);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_issuance_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out) try {
  return section_bytes(FORMATS[AFXI], blob, len, section_len_out);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_issuance_wire_pack(const afx_attributes_soa* attrs, const afx_issuance_soa* issuances, uint32_t n_responses, size_t count,
                                      uint8_t* blob, size_t blob_cap, size_t* len_out) try {
  if (!attrs || !issuances || !len_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  const uint32_t n = attrs->n_attributes;
  const size_t hdr = afx_issuance_wire_header_bytes(n);
  if (hdr == 0 || n_responses > AFX_MAX_ATTRIBUTES + 5 || count > 0xffffffffu) { set_error("layout out of range"); return AFX_E_BAD_ARGS; }
  const uint32_t cells = 4 + n_responses + n;
  const size_t len = hdr + count * cells * 32;
  *len_out = len;
  if (!blob) return AFX_OK;   // size query
  if (blob_cap < len) { set_error("blob buffer too small"); return AFX_E_BAD_ARGS; }
  const afx_issuance_soa& s = *issuances;
  if (count && (!s.t || !s.U || !s.V || !s.challenge || (n_responses && !s.responses) || (n && !attrs->values))) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
  for (uint32_t i = 0; i < n; i++)
    if (attrs->kinds[i] > AFX_ATTR_SECRET_POINT) { set_error("attribute kind out of range"); return AFX_E_BAD_ARGS; }
  write_header(FORMATS[AFXI], blob, count, cells, n, n_responses, attrs->kinds);
  std::vector<const uint8_t*> col = { s.t, s.U, s.V, s.challenge };
  for (uint32_t r = 0; r < n_responses; r++) col.push_back(s.responses + (size_t)r * count * 32);
  for (uint32_t i = 0; i < n; i++) col.push_back(attrs->values + (size_t)i * count * 32);
  uint8_t* rec = blob + hdr;
  for (size_t i = 0; i < count; i++)
    for (uint32_t c = 0; c < cells; c++, rec += 32) memcpy(rec, col[c] + i * 32, 32);
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }

// Items [first, first + n) of the AFXI records of one layout (statements.hpp IssuanceRecords): the one staging of both front ends
int verify_records(afx_ctx* ctx, const IssuanceRecords& B, size_t first, size_t n) {
  CtxLock lock__(ctx, true);
  if (n == 0) return AFX_OK;
  AFX_HIP(hipSetDevice(ctx->device));
  const uint32_t na = B.n, nr = B.nr, cells = 4 + nr + na;
  const std::vector<uint32_t> map = identity_map(cells);   // SoA rows in record order: t U V challenge responses[] values[]
  struct { uint32_t n, nr; uint8_t kinds[AFX_MAX_ATTRIBUTES]; } jd;
  memset(&jd, 0, sizeof jd);
  jd.n = na; jd.nr = nr; memcpy(jd.kinds, B.kinds, AFX_MAX_ATTRIBUTES);
  const PlanKey jkey = plan_key("VIW", &jd, sizeof jd, mode_flags(ctx));
  const size_t total = B.count;
  return host_pipe(ctx, n, [&](Stager& st, size_t off, size_t sn) -> int {
    const size_t f0 = first + off;
    st.layout_tag = 1;
    const size_t dn = st.dev_items(sn);
    // (one section: its records as they lie; several: the same region, filled section by section)
    const size_t o_rec = B.rec ? st.add_rows(B.rec, 1, (size_t)cells * 32, total, f0, sn, dn)
                               : st.add_rows_pieces(*B.pieces, (size_t)cells * 32, total, f0, sn, dn),
                 o_map = st.add((const uint8_t*)map.data(), 4 * (size_t)cells),
                 o_soa = st.reserve(dn * cells * 32), o_st = st.add(nullptr, dn);
    st.plan_fetch(B.status, o_st, 1, 1, total, f0, sn, dn);
    int rc = st.upload();
    if (rc) return rc;
    if ((rc = transpose_in(st, o_rec, o_soa, o_map, cells, dn))) return rc;
    auto rowp = [&](uint32_t r) { return st.dev(o_soa) + (size_t)r * dn * 32; };
    afx_attributes_soa as;
    memset(&as, 0, sizeof as);
    as.n_attributes = na; memcpy(as.kinds, B.kinds, AFX_MAX_ATTRIBUTES);
    as.values = rowp(4 + nr);
    const afx_issuance_soa iss = { rowp(0), rowp(1), rowp(2), rowp(3), rowp(4) };
    if ((rc = afx_verify_issuances_dev(ctx, &as, &iss, nr, dn, st.dev(o_st)))) return rc;
    return st.fetch_all();
  }, jkey);
}
// one section: a batch in one piece.  (A layout every item fails on still goes to afx_verify_issuances_dev here; the stream's entry
// point, wire_user.cpp, answers it without a launch.)
extern "C" int afx_verify_issuances_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  if (!ctx || !status || !count_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  IssuanceRecords B;
  size_t off = 0;
  int rc = afx_issuance_wire_parse(blob, len, &B.n, B.kinds, &B.nr, &B.count, &off);
  if (rc) return rc;
  *count_out = B.count;
  if (B.count == 0) return AFX_OK;
  if (status_cap < B.count) { set_error("status buffer too small"); return AFX_E_BAD_ARGS; }
  if (B.count > 0xffffffffu / 64) { set_error("batch too large for one call"); return AFX_E_BAD_ARGS; }
  B.rec = blob + off;
  B.status = status;
  return verify_records(ctx, B, 0, B.count);   // (which takes the context: nothing above reads it)
} catch (...) { return afx::exception_rc(); }
