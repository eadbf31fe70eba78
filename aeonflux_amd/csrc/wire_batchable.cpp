// Batchable presentations on bytes (include/aeonflux_gpu.h "AFXB"): the format's C functions (thin wrappers over wire_formats.hpp's
// table) and the packer (host, bytes only) and the
// two doors - afx_verify_presentations_batchable_wire (AFXB sections in, statuses out) and afx_show_batchable_wire (credentials in,
// one AFXB section per group out).  Records are transposed on the GPU by the kernels the AFXP doors use (k_aos_to_soa,
// k_soa_to_aos, through records.hpp); the arithmetic is afx_verify_presentations_batchable_dev / afx_show_batchable_dev.  A batchable call takes the
// context in turn: the groups of a request run one after the other, none is collected with other threads' calls.
#include <string.h>
#include <map>
#include "records.hpp"
#include "wire_formats.hpp"
#include "batch_arrays.hpp"

namespace {
// Rows of the struct-of-arrays scratch both doors use, in record order but for the revealed values:
//   R[n_main] | responses[nr] | C_x_0 C_x_1 C_V | C_y[na] | per proof of encryption: R[5] and the proof's rows but its challenge
constexpr uint32_t PER_PROOF_ROWS = CM_ENC_ROWS + ENC_ROWS - 1;   // 18
struct Rows {
  uint32_t resp, enc, end;
  Rows(const afx_shape& sh, uint32_t n_main) : resp(n_main), enc(resp + sh.n_responses + 3 + sh.n_attributes), end(enc + PER_PROOF_ROWS * sh.n_enc_proofs) {}
};
}  // namespace

// ---- the AFXB format (wire_formats.hpp): host only, bytes only ----
extern "C" size_t afx_batchable_wire_header_bytes(const afx_shape* sh) {
  return sh && shape_ok(*sh) ? header_bytes(FORMATS[AFXB], sh->n_attributes, sh->n_hidden_scalars, sh->n_enc_proofs) : 0;
}
extern "C" uint32_t afx_batchable_wire_cells_per_record(const afx_shape* sh, uint32_t n_main_commitments) {
  return sh && shape_ok(*sh) && n_main_ok(*sh, n_main_commitments) ? presentation_cells(*sh, n_main_commitments, 18) : 0;
}
extern "C" int afx_batchable_wire_parse(const uint8_t* blob, size_t len, afx_shape* shape_out, uint32_t* n_main_out, size_t* count_out, size_t* records_offset_out) try {
  if (!blob || !shape_out || !n_main_out || !count_out || !records_offset_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  Header H;
  const int rc = read_header(FORMATS[AFXB], blob, len, H);
  if (rc) return rc;
  *shape_out = shape_of(H); *n_main_out = H.n_main; *count_out = H.count; *records_offset_out = H.hdr;
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }
// the length of the section that starts at blob (its header names it); the section itself is checked by afx_batchable_wire_parse
extern "C" int afx_batchable_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out) try {
  return section_bytes(FORMATS[AFXB], blob, len, section_len_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_batchable_wire_pack(const afx_shape* shape, const afx_presentation_soa* batch, const afx_commitments_soa* cm, uint32_t n_main, size_t count,
                                       uint8_t* blob, size_t blob_cap, size_t* len_out) try {
  if (!shape || !batch || !cm || !len_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  const size_t hdr = afx_batchable_wire_header_bytes(shape);
  const uint32_t cells = afx_batchable_wire_cells_per_record(shape, n_main);
  if (hdr == 0 || cells == 0 || count > 0xffffffffu) { set_error("shape or n_main_commitments out of range"); return AFX_E_BAD_ARGS; }
  const size_t len = hdr + count * cells * 32;
  *len_out = len;
  if (!blob) return AFX_OK;   // size query
  if (blob_cap < len) { set_error("blob buffer too small"); return AFX_E_BAD_ARGS; }
  const afx_shape& sh = *shape;
  const afx_presentation_soa& b = *batch;
  const Dims dm = dims_of(sh);
  if (count && batchable_any_null(b, *cm, dm)) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
  write_header(FORMATS[AFXB], blob, sh, count, cells, n_main);
  if (!count) return AFX_OK;   // (no record: no array is looked at)
  std::vector<const uint8_t*> col;
  auto cell = [&](const uint8_t* base, uint32_t r) { col.push_back(base + (size_t)r * count * 32); };
  for (uint32_t r = 0; r < n_main; r++) cell(cm->main, r);
  each_cell(b, dm, cell, NO_CHALLENGE);
  for (uint32_t e = 0; e < sh.n_enc_proofs; e++) {
    for (uint32_t r = 0; r < CM_ENC_ROWS; r++) cell(cm->enc[e], r);
    each_cell(b.enc[e], dm, cell, NO_CHALLENGE);
  }
  if (col.size() != cells) { set_error("internal: wire cell list"); return AFX_E_BAD_ARGS; }
  uint8_t* rec = blob + hdr;
  for (size_t i = 0; i < count; i++)
    for (uint32_t c = 0; c < cells; c++, rec += 32) memcpy(rec, col[c] + i * 32, 32);
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }

// ------------------------------------------------------------------------------------------------
// the verifier's door
// ------------------------------------------------------------------------------------------------
namespace {
struct VSection { size_t first, n; const uint8_t* rec; };             // items [first, first + n) of the stream
struct VGroup { afx_shape sh; uint32_t n_main, cells; std::vector<VSection> secs; size_t total = 0; };

// one merged group: its sections' records gathered into one staged array, transposed, verified as one column call
int verify_group(afx_ctx* ctx, const VGroup& G, const afx_device_rng& rng, uint8_t* status) {
  AFX_HIP(hipSetDevice(ctx->device));
  const uint32_t expect = afx_batchable_main_commitments(ctx, &G.sh);
  if (expect == 0) {   // a shape every item fails on: answered without reading a record
    for (const VSection& s : G.secs) memset(status + s.first, AFX_ST_VERIFICATION_FAILURE, s.n);
    return AFX_OK;
  }
  const afx_shape& sh = G.sh;
  const Rows R(sh, G.n_main);
  const uint32_t values_row = R.end, rows = values_row + sh.n_attributes;
  const std::vector<uint32_t> map = presentation_map(sh, R.resp, PER_PROOF_ROWS, values_row, R.enc);
  if (map.size() != G.cells) { set_error("internal: AFXB cell map"); return AFX_E_BAD_ARGS; }
  const size_t n = G.total;
  std::vector<Stager::Piece> pieces;
  size_t at = 0;
  for (const VSection& s : G.secs) { pieces.push_back({ at, s.n, s.rec }); at += s.n; }
  Stager st(ctx);
  const size_t o_rec = st.add_rows_pieces(pieces, (size_t)G.cells * 32, n, 0, n, n), o_map = st.add((const uint8_t*)map.data(), 4 * map.size()),
               o_soa = st.reserve(n * rows * 32), o_st = st.add(nullptr, n);
  int rc = st.upload();
  if (rc) return rc;
  if ((rc = transpose_in(st, o_rec, o_soa, o_map, G.cells, n))) return rc;   // (a Stager of the call's own: at once)
  auto rowp = [&](uint32_t r) { return st.dev(o_soa) + (size_t)r * n * 32; };
  const Dims dm = dims_of(sh);
  std::vector<afx_encproof_soa> encs(sh.n_enc_proofs);
  std::vector<uint8_t*> cenc(sh.n_enc_proofs);
  for (uint32_t e = 0; e < sh.n_enc_proofs; e++) {
    const uint32_t r = R.enc + PER_PROOF_ROWS * e;
    cenc[e] = rowp(r);
    encs[e].challenge = nullptr;
    view_rows(encs[e], dm, rowp, r + CM_ENC_ROWS, NO_CHALLENGE);
  }
  afx_presentation_soa d = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rowp(values_row), encs.data() };
  view_rows(d, dm, rowp, R.resp, NO_CHALLENGE, NO_VALUES);
  const afx_commitments_soa dcm = { rowp(0), cenc.data() };
  if ((rc = afx_verify_presentations_batchable_dev(ctx, &sh, &d, &dcm, &rng, n, st.dev(o_st)))) return rc;
  std::vector<uint8_t> got(n);
  AFX_HIP(hipMemcpyAsync(got.data(), st.dev(o_st), n, hipMemcpyDeviceToHost, st.stream()));
  AFX_HIP(hipStreamSynchronize(st.stream()));
  at = 0;
  for (const VSection& s : G.secs) { memcpy(status + s.first, got.data() + at, s.n); at += s.n; }
  return AFX_OK;
}
}  // namespace

extern "C" int afx_verify_presentations_batchable_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_device_rng* weights, uint8_t* status,
                                                       size_t status_cap, size_t* count_out) try {
  CtxLock lock__(ctx);
  if (!ctx || !blob || !count_out || (!status && status_cap)) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  // every section is parsed before anything runs: a malformed one anywhere fails the call with nothing written
  std::vector<VGroup> groups;
  std::map<std::string, size_t> by_shape;
  size_t off = 0, total = 0;
  while (off < len) {
    Header H;
    const int rc = read_section(FORMATS[AFXB], blob + off, len - off, H);
    if (rc) { set_error("section at byte " + std::to_string(off) + ": " + afx_last_error()); return rc; }
    const afx_shape sh = shape_of(H);
    const uint32_t n_main = H.n_main;
    const size_t sl = H.section, cnt = H.count, rec = H.hdr;
    const uint32_t expect = afx_batchable_main_commitments(ctx, &sh);
    if (expect && expect != n_main) { set_error("section at byte " + std::to_string(off) + ": n_main_commitments is not what this context verifies for the shape"); return AFX_E_BAD_ARGS; }
    const afx_shape csh = canonical_shape(sh);
    std::string key((const char*)&csh, sizeof csh);
    key.append((const char*)&n_main, sizeof n_main);
    auto it = by_shape.find(key);
    if (it == by_shape.end()) {
      it = by_shape.emplace(key, groups.size()).first;
      VGroup g;
      g.sh = sh; g.n_main = n_main; g.cells = afx_batchable_wire_cells_per_record(&sh, n_main);
      groups.push_back(g);
    }
    if (cnt) { groups[it->second].secs.push_back({ total, cnt, blob + off + rec }); groups[it->second].total += cnt; }
    total += cnt;
    off += sl;
  }
  *count_out = total;
  if (total == 0) return AFX_OK;
  if (status_cap < total) { set_error("status buffer too small"); return AFX_E_BAD_ARGS; }
  if (total > 0xffffffffu / 64) { set_error("stream too large for one call"); return AFX_E_BAD_ARGS; }
  if (!ctx->has_key) { set_error("Issuer::verify needs the issuer key"); return AFX_E_NO_KEY; }
  // one seed for the call (the caller's, or the library's own); every merged group draws under its own stream number
  uint8_t seed[32];
  afx_device_rng base = { nullptr, 0 };
  if (weights) base = *weights;
  if (!base.seed) {
    DrawSeed own;
    const afx_device_rng none = { nullptr, base.stream };
    int rc = own.init(&none);
    if (rc) return rc;
    memcpy(seed, own.b, 32);
    base.seed = seed;
  }
  int rc = AFX_OK;
  for (size_t g = 0; g < groups.size() && !rc; g++) {
    if (!groups[g].total) continue;
    const afx_device_rng rng = { base.seed, base.stream + g };
    rc = verify_group(ctx, groups[g], rng, status);
  }
  afx::afx_wipe(seed, sizeof seed);
  return rc;
} catch (...) { return afx::exception_rc(); }

// ------------------------------------------------------------------------------------------------
// the user's door
// ------------------------------------------------------------------------------------------------
namespace {
afx_shape shape_of_credentials(const afx_credentials_soa& cr) {
  afx_shape sh;
  memset(&sh, 0, sizeof sh);
  sh.n_attributes = cr.n_attributes;
  uint32_t hs = 0, nsp = 0;
  for (uint32_t i = 0; i < cr.n_attributes; i++) {
    switch (cr.kinds[i]) {
      case AFX_ATTR_PUBLIC_SCALAR: sh.kinds[i] = AFX_ENC_PUBLIC_SCALAR; break;
      case AFX_ATTR_SECRET_SCALAR: sh.kinds[i] = AFX_ENC_SECRET_SCALAR; sh.hidden_scalar_indices[hs++] = (uint16_t)i; break;
      case AFX_ATTR_SECRET_POINT: sh.kinds[i] = AFX_ENC_SECRET_POINT; sh.enc_indices[nsp++] = (uint16_t)i; break;
      default: sh.kinds[i] = AFX_ENC_PUBLIC_POINT; break;
    }
  }
  sh.n_hidden_scalars = hs; sh.n_responses = 3 + hs; sh.n_enc_proofs = nsp;
  return sh;
}
struct BJob { afx_shape sh; uint32_t n_main = 0, cells = 0; size_t out_off = 0, hdr = 0; bool no_key = false; };

// one group: afx_show_batchable_dev writes into the rows of a scratch region, the credential's value rows are staged right behind it
// (a revealed value's cell reads its value row), k_soa_to_aos makes the records (failed items zeroed), fetched in one piece
int show_group(afx_ctx* ctx, const afx_show_group& G, const BJob& J, uint8_t* rec_out, uint8_t* status) {
  AFX_HIP(hipSetDevice(ctx->device));
  const afx_credentials_soa& cr = G.creds;
  const afx_shape& sh = J.sh;
  const size_t n = G.count;
  const uint32_t nsp = sh.n_enc_proofs;
  const bool kp = G.keypairs && nsp;
  const Rows R(sh, J.n_main);
  const uint32_t chal = R.end, values_row = (chal + 1 + nsp + 7) & ~7u;   // the compact challenges (written, not sent), then pad: values_row * n * 32 is a multiple of 256
  const std::vector<uint32_t> map = presentation_map(sh, R.resp, PER_PROOF_ROWS, values_row, R.enc);
  if (map.size() != J.cells) { set_error("internal: AFXB show cell map"); return AFX_E_BAD_ARGS; }
  Stager st(ctx);
  const Dims dm = dims_of(cr);
  auto in = [&](const uint8_t* p, size_t k, size_t elem) { return p ? st.add(p, k * n * elem) : NO_ARRAY; };   // (an array the layout does not read: nothing staged)
  const size_t o_soa = st.reserve(n * values_row * 32);
  Offsets<afx_credentials_soa> oc;
  stage(oc, cr, dm, in, 0, 1);   // the value rows, right behind the scratch
  const size_t o_map = st.add((const uint8_t*)map.data(), 4 * map.size());
  stage(oc, cr, dm, in, 1);
  const Offsets<afx_show_randomness> orn = stage(G.rnd, dm, in);
  Offsets<afx_keypairs_soa> ok;
  if (kp) stage(ok, *G.keypairs, dm, in);
  const size_t o_out = st.add(nullptr, n * J.cells * 32), o_st = st.add(nullptr, n);
  int rc = st.upload();
  if (rc) return rc;
  uint8_t* soa_d = st.dev(o_soa);
  if (st.dev(oc.at[0]) != soa_d + (size_t)values_row * n * 32) { set_error("internal: value rows are not behind the show scratch"); return AFX_E_BAD_ARGS; }
  auto rowp = [&](uint32_t r) { return soa_d + (size_t)r * n * 32; };
  const afx_credentials_soa dc = on_device(st, oc, cr);
  const afx_keypairs_soa dk = on_device(st, ok);
  const afx_show_randomness dr = on_device(st, orn);
  std::vector<afx_encproof_out> de(nsp);
  std::vector<uint8_t*> ce(nsp);
  for (uint32_t e = 0; e < nsp; e++) {
    const uint32_t r = R.enc + PER_PROOF_ROWS * e;
    ce[e] = rowp(r);
    de[e].challenge = rowp(chal + 1 + e);
    view_rows(de[e], dm, rowp, r + CM_ENC_ROWS, NO_CHALLENGE);
  }
  afx_presentation_out dout = { rowp(chal), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nsp ? de.data() : nullptr };
  view_rows(dout, dm, rowp, R.resp, NO_CHALLENGE, NO_VALUES);
  const afx_commitments_soa dcm = { rowp(0), ce.data() };
  afx_shape shape_dev;
  if ((rc = afx_show_batchable_dev(ctx, &dc, kp ? &dk : nullptr, &dr, n, &dout, &dcm, &shape_dev, st.dev(o_st)))) return rc;
  if ((rc = transpose_out(st, o_soa, o_out, o_map, o_st, J.cells, n))) return rc;   // (a Stager of the call's own: at once)
  AFX_HIP(hipMemcpyAsync(rec_out, st.dev(o_out), n * J.cells * 32, hipMemcpyDeviceToHost, st.stream()));
  AFX_HIP(hipMemcpyAsync(status, st.dev(o_st), n, hipMemcpyDeviceToHost, st.stream()));
  AFX_HIP(hipStreamSynchronize(st.stream()));
  return AFX_OK;
}
}  // namespace

extern "C" int afx_show_batchable_wire(afx_ctx* ctx, afx_show_group* groups, size_t n_groups, uint8_t* out, size_t out_cap, size_t* out_len, uint8_t* status,
                                       size_t status_len) try {
  CtxLock lock__(ctx);
  if (!ctx || !out_len || (!groups && n_groups)) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  std::vector<BJob> jobs(n_groups);
  size_t total_len = 0, items = 0;
  for (size_t gi = 0; gi < n_groups; gi++) {
    const afx_show_group& G = groups[gi];
    const afx_credentials_soa& cr = G.creds;
    BJob& J = jobs[gi];
    auto bad = [&](const char* why) { set_error("group " + std::to_string(gi) + ": " + why); return AFX_E_BAD_ARGS; };
    if (cr.n_attributes == 0 || cr.n_attributes > ctx->n) return bad("credential attribute count does not fit the system parameters");
    for (uint32_t i = 0; i < cr.n_attributes; i++)
      if (cr.kinds[i] > AFX_ATTR_SECRET_POINT) return bad("unknown attribute kind");
    if (G.count > 0xffffffffu / 64) return bad("too many credentials in one group");
    J.sh = shape_of_credentials(cr);
    J.n_main = afx_batchable_main_commitments(ctx, &J.sh);
    if (!J.n_main) return bad("this shape has no batchable form (every presentation of it is rejected)");
    J.cells = afx_batchable_wire_cells_per_record(&J.sh, J.n_main);
    J.hdr = afx_batchable_wire_header_bytes(&J.sh);
    const uint32_t nsp = J.sh.n_enc_proofs;
    J.no_key = nsp && !G.keypairs;
    if (out && G.count) {
      if (!cr.values || !cr.t || !cr.U || !cr.V || !G.rnd.z_wide || !G.rnd.rng_seed || (nsp && (!G.rnd.enc_seeds || !cr.M2 || !cr.m3))) return bad("null batch array");
      if (G.keypairs && nsp && (!G.keypairs->a || !G.keypairs->a0 || !G.keypairs->a1 || !G.keypairs->pk)) return bad("null keypair array");
    }
    J.out_off = total_len;
    total_len += J.hdr + G.count * J.cells * 32;
    items += G.count;
  }
  *out_len = total_len;
  if (out) {
    if (out_cap < total_len) { set_error("output buffer too small"); return AFX_E_BAD_ARGS; }
    if (!status && status_len) { set_error("null argument"); return AFX_E_BAD_ARGS; }
    // positions given: each < status_len and used once over all groups; not given: contiguous after the groups before
    std::vector<uint8_t> used(status_len, 0);
    size_t next = 0;
    for (size_t g = 0; g < n_groups; g++) {
      for (size_t i = 0; i < groups[g].count; i++) {
        const uint64_t p = groups[g].positions ? groups[g].positions[i] : (uint64_t)(next + i);
        if (p >= status_len) { set_error("group " + std::to_string(g) + ": position outside the status array"); return AFX_E_BAD_ARGS; }
        if (used[p]) { set_error("group " + std::to_string(g) + ": a status position is used twice"); return AFX_E_BAD_ARGS; }
        used[p] = 1;
      }
      next += groups[g].count;
    }
  }
  for (size_t g = 0; g < n_groups; g++) groups[g].shape_out = jobs[g].sh;
  if (!out) return AFX_OK;   // size query: shapes and length only
  size_t next = 0;
  for (size_t g = 0; g < n_groups; g++) {
    const afx_show_group& G = groups[g];
    const BJob& J = jobs[g];
    const size_t count = G.count;
    uint8_t* h = out + J.out_off;
    write_header(FORMATS[AFXB], h, J.sh, count, J.cells, J.n_main);
    std::vector<uint8_t> st_buf(count, AFX_ST_VERIFICATION_FAILURE);
    if (J.no_key) {   // CredentialError::NoSymmetricKey, as afx_show answers it: zero records
      memset(h + J.hdr, 0, count * J.cells * 32);
      memset(st_buf.data(), AFX_ST_NO_SYMMETRIC_KEY, count);
    } else if (count) {
      const int rc = show_group(ctx, G, J, h + J.hdr, st_buf.data());
      if (rc) return rc;
    }
    for (size_t i = 0; i < count; i++) status[G.positions ? G.positions[i] : next + i] = st_buf[i];
    next += count;
  }
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }
