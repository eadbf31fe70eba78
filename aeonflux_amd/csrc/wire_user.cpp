// The user side of the protocol on bytes (include/aeonflux_gpu.h afx_verify_issuances_mixed_wire, afx_show_wire).
//  - CredentialIssuance::verify (the crate's src/issuer.rs:48-57) over a stream of AFXI sections, as afx_issue_wire writes them:
//    sections of one layout are merged wherever they stand (and staged from where they lie), the records are transposed to
//    struct-of-arrays on the GPU and verified by the function that verifies afx_verify_issuances_wire's one section (wire.cpp
//    verify_records; the AFXI format's C functions stand there too).
//  - AnonymousCredential::show (src/credential.rs:37-46) straight into AFXP sections: afx_show_dev writes its outputs into the rows of
//    one scratch region per pass, the revealed attribute values are read from the credential's own value rows, and k_soa_to_aos turns
//    the region into AFXP records - zeros for an item that failed - which come back in one fetch.
// Only bytes move on the host.  The scheduling is afx_issue_wire's (doors.hpp run_batches, on_members): small batches share one set of launches, small
// calls are collected with other threads' calls, large ones go through the two lanes in slices, and a group splits every batch.
#include <map>
#include <string>
#include <vector>
#include "records.hpp"
#include "wire_formats.hpp"
#include "batch_arrays.hpp"

namespace {

// ---- CredentialIssuance::verify over AFXI streams -------------------------------------------------------------------------------

struct ISection {
  size_t off, hdr, count, first;   // bytes, header bytes, items, index of its first item in the stream
  uint32_t n, nr;
  uint8_t kinds[AFX_MAX_ATTRIBUTES];
};
// The issuances of one (n_attributes, n_responses, kinds), merged over the sections that carry it: their records stay where they lie
// in the caller's blob (staged piece by piece); the statuses go to the caller's array when ONE section carries the layout, else to a
// buffer of the batch's own, scattered afterwards.
struct IBatch : IssuanceRecords {      // (statements.hpp: the layout, where the records lie, where the statuses go)
  std::vector<size_t> secs;
  std::vector<Stager::Piece> in_pieces;   // the records of several sections, where they lie in the caller's blob
  bool fails = false;                  // a layout every item fails on (afx_verify_issuances_dev's fail_all): answered here
  std::vector<uint8_t> st_buf;
};
struct IStream {
  std::vector<ISection> secs;
  std::vector<IBatch> batches;   // in order of first appearance
  size_t total = 0;
};

// Splits the stream into sections (every one parsed in full: a malformed one anywhere fails the call before anything runs) and merges
// the sections of one layout.
int parse_issuances(const uint8_t* blob, size_t len, uint32_t ctx_n, IStream& S) {
  if (!blob && len) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  std::map<std::string, size_t> by_layout;
  for (size_t off = 0; off < len;) {
    Header H;
    const int rc = read_section(FORMATS[AFXI], blob + off, len - off, H);
    if (rc) { set_error("section at byte " + std::to_string(off) + ": " + afx_last_error()); return rc; }
    const size_t cnt = H.count;
    ISection s;
    s.off = off; s.hdr = H.hdr; s.count = cnt; s.first = S.total;
    s.n = H.n; s.nr = H.nr;
    memset(s.kinds, 0, sizeof s.kinds);
    memcpy(s.kinds, H.kinds, H.n);
    S.total += cnt;   // (< len / 32)
    if (cnt) {
      std::string key((const char*)&s.nr, sizeof s.nr);
      key.append((const char*)s.kinds, s.n);   // (n is the key's length - 4)
      auto it = by_layout.find(key);
      if (it == by_layout.end()) {
        it = by_layout.emplace(key, S.batches.size()).first;
        S.batches.emplace_back();
        IBatch& B = S.batches.back();
        B.n = s.n; B.nr = s.nr;
        memcpy(B.kinds, s.kinds, AFX_MAX_ATTRIBUTES);
        // more attributes than generators, or a response count the statement does not have: every item fails (statements_prove.cpp
        // afx_verify_issuances_dev), without a launch
        B.fails = s.n > ctx_n || s.nr != ctx_n + 5;
      }
      S.batches[it->second].secs.push_back(S.secs.size());
      S.batches[it->second].count += cnt;
    }
    S.secs.push_back(s);
    off += H.section;
  }
  return AFX_OK;
}

int check_issuances(const IStream& S, const uint8_t* status, size_t status_cap) {
  if (status_cap < S.total || (!status && S.total)) { set_error("status buffer too small"); return AFX_E_BAD_ARGS; }
  for (const IBatch& B : S.batches)
    if (!B.fails && B.count > 0xffffffffu / 64) { set_error("too many issuances of one layout"); return AFX_E_BAD_ARGS; }
  return AFX_OK;
}

// every batch's records (where they lie in the blob) and statuses; the batches nothing is launched for are answered here
void prepare_issuances(IStream& S, const uint8_t* blob, uint8_t* status) {
  for (IBatch& B : S.batches) {
    if (B.fails) {
      for (size_t k : B.secs) memset(status + S.secs[k].first, AFX_ST_VERIFICATION_FAILURE, S.secs[k].count);
      continue;
    }
    size_t at = 0;
    for (size_t k : B.secs) {
      const ISection& s = S.secs[k];
      B.in_pieces.push_back({ at, s.count, blob + s.off + s.hdr });
      at += s.count;
    }
    if (B.secs.size() == 1) { B.rec = B.in_pieces[0].src; B.status = status + S.secs[B.secs[0]].first; }
    else {   // (the batch points into itself: S.batches neither grows nor moves from here on)
      B.pieces = &B.in_pieces;
      B.st_buf.assign(B.count, AFX_ST_VERIFICATION_FAILURE);
      B.status = B.st_buf.data();
    }
  }
}
void scatter_issuances(const IStream& S, uint8_t* status) {
  for (const IBatch& B : S.batches) {
    if (B.fails || B.secs.size() == 1) continue;
    size_t at = 0;
    for (size_t k : B.secs) {
      const ISection& s = S.secs[k];
      memcpy(status + s.first, B.status + at, s.count);
      at += s.count;
    }
  }
}

std::vector<size_t> launch_counts(const IStream& S) {
  std::vector<size_t> c(S.batches.size(), 0);
  for (size_t b = 0; b < S.batches.size(); b++) c[b] = S.batches[b].fails ? 0 : S.batches[b].count;
  return c;
}

// ---- AnonymousCredential::show into AFXP ----------------------------------------------------------------------------------------

// the presentation shape afx_show gives a credential layout (statements_prove.cpp afx_show_dev; presentation.rs:293-320)
afx_shape shape_of(const afx_credentials_soa& cr) {
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
  sh.n_hidden_scalars = hs;
  sh.n_responses = 3 + hs;
  sh.n_enc_proofs = nsp;
  return sh;
}

// One afx_show_group as one AFXP section of the output.
struct SJob {
  const afx_show_group* g = nullptr;
  afx_shape sh;
  uint32_t cells = 0;
  size_t out_off = 0, hdr = 0;
  bool no_key = false;                 // SECRET_POINT attributes and no keypairs: NoSymmetricKey for every item, nothing launched
  uint64_t index0 = 0;                 // draw index of the group's first item (afx_show_wire_rng): the counts of the groups before it
  uint8_t* rec = nullptr;              // out + out_off + hdr: [count][cells][32]
  uint8_t* status = nullptr;           // the caller's contiguous range, or st_buf (positions given)
  std::vector<uint8_t> st_buf;
};
struct SPlan {
  std::vector<SJob> jobs;
  size_t out_len = 0, items = 0;
};

// The groups' sections and their length; every group whose layout afx_show refuses fails the call.  `arrays`: the full call also
// checks the arrays afx_show would read (the size query reads none).
// `drawn`: the randomness is drawn on the device (afx_show_wire_rng): the groups' rnd is not read.
int plan_show(afx_ctx* ctx, const afx_show_group* groups, size_t n_groups, bool arrays, SPlan& P, bool drawn = false) {
  if (!groups && n_groups) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  P.jobs.resize(n_groups);
  for (size_t gi = 0; gi < n_groups; gi++) {
    const afx_show_group& G = groups[gi];
    SJob& J = P.jobs[gi];
    J.g = &G;
    const afx_credentials_soa& cr = G.creds;
    auto bad = [&](const char* why) { set_error("group " + std::to_string(gi) + ": " + why); return AFX_E_BAD_ARGS; };
    if (cr.n_attributes == 0 || cr.n_attributes > ctx->n) return bad("credential attribute count does not fit the system parameters");
    for (uint32_t i = 0; i < cr.n_attributes; i++)
      if (cr.kinds[i] > AFX_ATTR_SECRET_POINT) return bad("unknown attribute kind");
    if (G.count > 0xffffffffu / 64) return bad("too many credentials in one group");
    J.sh = shape_of(cr);
    J.cells = afx_wire_cells_per_record(&J.sh);
    J.hdr = afx_wire_header_bytes(&J.sh);
    const uint32_t nsp = J.sh.n_enc_proofs;
    J.no_key = nsp && !G.keypairs;
    if (arrays && G.count) {   // (afx_show_range's checks)
      if (!cr.values || !cr.t || !cr.U || !cr.V || (!drawn && (!G.rnd.z_wide || !G.rnd.rng_seed)) || (nsp && ((!drawn && !G.rnd.enc_seeds) || !cr.M2 || !cr.m3)))
        return bad("null batch array");
      if (G.keypairs && nsp && (!G.keypairs->a || !G.keypairs->a0 || !G.keypairs->a1 || !G.keypairs->pk)) return bad("null keypair array");
    }
    J.out_off = P.out_len;
    P.out_len += J.hdr + G.count * J.cells * 32;   // (< 2^26 * 2^10 * 2^5 per group)
    J.index0 = P.items;
    P.items += G.count;
  }
  return AFX_OK;
}

// positions given: each < status_len and used once over all groups; not given: contiguous after the groups before (mixed.cpp)
int check_positions(const afx_show_group* groups, size_t n_groups, size_t status_len) {
  std::vector<uint8_t> used(status_len, 0);
  size_t next = 0;
  for (size_t g = 0; g < n_groups; g++) {
    const afx_show_group& grp = groups[g];
    for (size_t i = 0; i < grp.count; i++) {
      const uint64_t p = grp.positions ? grp.positions[i] : (uint64_t)(next + i);
      if (p >= status_len) { set_error("group " + std::to_string(g) + ": position outside the status array"); return AFX_E_BAD_ARGS; }
      if (used[p]) { set_error("group " + std::to_string(g) + ": a status position is used twice"); return AFX_E_BAD_ARGS; }
      used[p] = 1;
    }
    next += grp.count;
  }
  return AFX_OK;
}

// headers, the sections nothing is launched for, and where every group's statuses go
void prepare_show(SPlan& P, uint8_t* out, uint8_t* status) {
  size_t next = 0;
  for (SJob& J : P.jobs) {
    const afx_shape& sh = J.sh;
    const size_t count = J.g->count;
    uint8_t* h = out + J.out_off;
    write_header(FORMATS[AFXP], h, sh, count, J.cells);
    J.rec = h + J.hdr;
    if (J.g->positions) { J.st_buf.assign(count, AFX_ST_VERIFICATION_FAILURE); J.status = J.st_buf.data(); }
    else J.status = status + next;
    next += count;
    if (J.no_key) {   // CredentialError::NoSymmetricKey (presentation.rs:150-157), as afx_show answers it
      memset(J.rec, 0, count * J.cells * 32);
      memset(J.status, AFX_ST_NO_SYMMETRIC_KEY, count);
    }
  }
}
void scatter_show(const SPlan& P, uint8_t* status) {
  for (const SJob& J : P.jobs)
    if (J.g->positions)
      for (size_t i = 0; i < J.g->count; i++) status[J.g->positions[i]] = J.st_buf[i];
}
std::vector<size_t> launch_counts(const SPlan& P) {
  std::vector<size_t> c(P.jobs.size(), 0);
  for (size_t b = 0; b < P.jobs.size(); b++) c[b] = P.jobs[b].no_key ? 0 : P.jobs[b].g->count;
  return c;
}

// Items [first, first + n) of a group.  Per pass, one region of scratch holds the rows
//   challenge | responses[3 + hs] | C_x_0 C_x_1 C_V | C_y[n] | 14 per proof of encryption | (pad to a multiple of 8 rows)
// and the credential's value rows are staged right behind it, so that a revealed value's cell maps to its value row directly.
// afx_show_dev fills the rows; k_soa_to_aos copies the region out as AFXP records (right after the plan, or the session's `post`),
// fetched in one piece.
// seed40: the call's staged seed || stream (afx_show_wire_rng): z_wide, rng_seed and enc_seeds are drawn on the device at the items'
// ordinals (J.index0 + i), into the rows afx_show_dev reads
int show_records(afx_ctx* ctx, const SJob& J, size_t first, size_t n, const uint8_t* seed40 = nullptr) {
  CtxLock lock__(ctx, true);
  if (n == 0) return AFX_OK;
  AFX_HIP(hipSetDevice(ctx->device));
  const afx_show_group& G = *J.g;
  const afx_credentials_soa& cr = G.creds;
  const afx_shape& sh = J.sh;
  const uint32_t na = sh.n_attributes, nr = sh.n_responses, nsp = sh.n_enc_proofs, cells = J.cells;
  const bool kp = G.keypairs && nsp;
  const Dims dm = dims_of(cr);
  const uint32_t r_enc = 1 + nr + 3 + na, rows = r_enc + ENC_ROWS * nsp, r_val = (rows + 7) & ~7u;   // (r_val * dn * 32: a multiple of 256)
  const std::vector<uint32_t> map = presentation_map(sh, 1, 14, r_val, r_enc);
  if (map.size() != cells) { set_error("internal: show wire cell map"); return AFX_E_BAD_ARGS; }
  struct { uint32_t n; uint8_t kinds[AFX_MAX_ATTRIBUTES]; } jd;   // what makes two calls one pass (statements.hpp host_pipe)
  memset(&jd, 0, sizeof jd);
  jd.n = na; memcpy(jd.kinds, cr.kinds, na);
  const PlanKey jkey = plan_key(seed40 ? "SWR" : "SW", &jd, sizeof jd, mode_flags(ctx) | (kp ? (uint64_t)1 << 63 : 0));
  const std::vector<Stager::DrawPiece> draws = { { 0, (size_t)G.count, J.index0 } };
  const size_t total = G.count;
  return host_pipe(ctx, n, [&](Stager& st, size_t off, size_t sn) -> int {
    const size_t f0 = first + off;
    st.layout_tag = seed40 ? 5 : 3;
    const size_t dn = st.dev_items(sn);
    auto in = [&](const uint8_t* p, size_t k, size_t elem) { return p ? st.add_rows(p, k, elem, total, f0, sn, dn) : NO_ARRAY; };   // (an array the layout does not read: nothing staged)
    const size_t o_soa = st.reserve(dn * r_val * 32);
    Offsets<afx_credentials_soa> oc;
    stage(oc, cr, dm, in, 0, 1);   // the value rows, right behind the scratch
    const size_t o_map = st.add((const uint8_t*)map.data(), 4 * (size_t)cells);
    stage(oc, cr, dm, in, 1);
    Offsets<afx_show_randomness> orn;
    if (seed40) {
      const size_t s_at = st.add_seed(seed40, dn);
      orn.at[0] = st.add_drawn(s_at, AFX_DRAW_Z_WIDE, 1, draws, f0, sn, dn);
      orn.at[1] = st.add_drawn(s_at, AFX_DRAW_SHOW_SEED, 1, draws, f0, sn, dn);
      if (nsp) orn.at[2] = st.add_drawn(s_at, AFX_DRAW_ENC_SEED(0), nsp, draws, f0, sn, dn);
    } else {
      stage(orn, G.rnd, dm, in);
    }
    Offsets<afx_keypairs_soa> ok;
    if (kp) stage(ok, *G.keypairs, dm, in);
    const size_t o_out = st.add_rows(nullptr, 1, (size_t)cells * 32, total, f0, sn, dn), o_st = st.add(nullptr, dn);
    st.plan_fetch(J.rec, o_out, 1, (size_t)cells * 32, total, f0, sn, dn);
    st.plan_fetch(J.status, o_st, 1, 1, total, f0, sn, dn);
    int rc = st.upload();
    if (rc) return rc;
    uint8_t* soa_d = st.dev(o_soa);
    if (st.dev(oc.at[0]) != soa_d + (size_t)r_val * dn * 32) { set_error("internal: value rows are not behind the show scratch"); return AFX_E_BAD_ARGS; }
    auto rowp = [&](uint32_t r) { return soa_d + (size_t)r * dn * 32; };
    const afx_credentials_soa dc = on_device(st, oc, cr);
    const afx_keypairs_soa dk = on_device(st, ok);
    const afx_show_randomness dr = on_device(st, orn);
    std::vector<afx_encproof_out> de(nsp);
    for (uint32_t e = 0; e < nsp; e++) view_rows(de[e], dm, rowp, r_enc + ENC_ROWS * e);
    // (attr_values == null: the revealed values are not copied - their cells read the value rows)
    afx_presentation_out dout = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nsp ? de.data() : nullptr };
    view_rows(dout, dm, rowp, 0, 0, NO_VALUES);
    afx_shape shape_dev;
    if ((rc = afx_show_dev(ctx, &dc, kp ? &dk : nullptr, &dr, dn, &dout, &shape_dev, st.dev(o_st)))) return rc;
    if ((rc = transpose_out(st, o_soa, o_out, o_map, o_st, cells, dn))) return rc;
    return st.fetch_all();
  }, jkey);
}

// a parsed stream (parse_issuances with this context's n) on one context
int verify_stream(afx_ctx* ctx, IStream& S, const uint8_t* blob, uint8_t* status, size_t status_cap) {
  int rc = check_issuances(S, status, status_cap);
  if (rc) return rc;
  prepare_issuances(S, blob, status);
  if ((rc = run_batches(ctx, launch_counts(S), [&](size_t b) { return verify_records(ctx, S.batches[b], 0, S.batches[b].count); }))) return rc;
  scatter_issuances(S, status);
  return AFX_OK;
}
}  // namespace

extern "C" int afx_verify_issuances_mixed_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  if (!ctx || !count_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  IStream S;
  const int rc = parse_issuances(blob, len, ctx->n, S);
  if (rc) return rc;
  *count_out = S.total;
  return verify_stream(ctx, S, blob, status, status_cap);
} catch (...) { return afx::exception_rc(); }

// The same stream over a group's devices.  A stream of at most afx_ctx_set_small_batch_items issuances (member 0's) goes whole to ONE
// member, the next in turn; a larger one has every batch split over the members (afx_shard_bounds), one host thread per member.
extern "C" int afx_group_verify_issuances_mixed_wire(afx_group* group, const uint8_t* blob, size_t len, uint8_t* status, size_t status_cap,
                                                     size_t* count_out) try {
  if (!group || !count_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  const uint32_t m = afx_group_size(group);
  if (m == 0) { set_error("empty group"); return AFX_E_BAD_ARGS; }
  afx_ctx* c0 = afx_group_member(group, 0);
  const uint32_t small = afx_group_small_batch_items(group);
  IStream S;   // parsed once, for whichever path (the members share the parameters, so member 0's n is every member's)
  int rc = parse_issuances(blob, len, c0->n, S);
  if (rc) return rc;
  *count_out = S.total;
  if (m == 1 || (small && S.total <= small)) {
    const uint32_t k = afx_group_pick_small(group);
    GroupPin pin(group, k, true);
    rc = verify_stream(afx_group_member(group, k), S, blob, status, status_cap);
    if (rc && m > 1) { const std::string why = afx_last_error(); set_error("member " + std::to_string(k) + ": " + why); }
    return rc;
  }
  if ((rc = check_issuances(S, status, status_cap))) return rc;
  prepare_issuances(S, blob, status);
  rc = on_members(group, m, [&](afx_ctx* c, uint32_t k) -> int {
    for (const IBatch& B : S.batches) {
      if (B.fails) continue;
      size_t first = 0, n = 0;
      afx_shard_bounds(B.count, m, k, &first, &n);
      if (n) { const int r = verify_records(c, B, first, n); if (r) return r; }
    }
    return AFX_OK;
  });
  if (rc) return rc;
  scatter_issuances(S, status);
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }

namespace {
// afx_show_wire (seed40 == null) and afx_show_wire_rng (seed40: the staged seed || stream; the groups' rnd is not read)
int show_wire(afx_ctx* ctx, afx_show_group* groups, size_t n_groups, const uint8_t* seed40, uint8_t* out, size_t out_cap, size_t* out_len,
              uint8_t* status, size_t status_len) {
  if (!ctx || !out_len) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  SPlan P;
  int rc = plan_show(ctx, groups, n_groups, out != nullptr, P, seed40 != nullptr);
  if (rc) return rc;
  *out_len = P.out_len;
  if (out) {
    if (out_cap < P.out_len) { set_error("output buffer too small"); return AFX_E_BAD_ARGS; }
    if (!status && status_len) { set_error("null argument"); return AFX_E_BAD_ARGS; }
    if ((rc = check_positions(groups, n_groups, status_len))) return rc;
  }
  for (size_t g = 0; g < n_groups; g++) groups[g].shape_out = P.jobs[g].sh;
  if (!out) return AFX_OK;   // size query: shapes and length only
  prepare_show(P, out, status);
  if ((rc = run_batches(ctx, launch_counts(P), [&](size_t b) { return show_records(ctx, P.jobs[b], 0, P.jobs[b].g->count, seed40); }))) return rc;
  scatter_show(P, status);
  return AFX_OK;
}
int group_show_wire(afx_group* group, afx_show_group* groups, size_t n_groups, const uint8_t* seed40, uint8_t* out, size_t out_cap,
                    size_t* out_len, uint8_t* status, size_t status_len);
}  // namespace

extern "C" int afx_show_wire(afx_ctx* ctx, afx_show_group* groups, size_t n_groups, uint8_t* out, size_t out_cap, size_t* out_len, uint8_t* status,
                             size_t status_len) try {
  return show_wire(ctx, groups, n_groups, nullptr, out, out_cap, out_len, status, status_len);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_show_wire_rng(afx_ctx* ctx, afx_show_group* groups, size_t n_groups, const afx_device_rng* rng, uint8_t* out, size_t out_cap,
                                 size_t* out_len, uint8_t* status, size_t status_len) try {
  if (!rng) { set_error("null device rng"); return AFX_E_BAD_ARGS; }
  DrawSeed seed;
  int rc = out ? seed.init(rng) : AFX_OK;   // (the size query draws nothing)
  if (rc) return rc;
  return show_wire(ctx, groups, n_groups, seed.b, out, out_cap, out_len, status, status_len);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_group_show_wire_rng(afx_group* group, afx_show_group* groups, size_t n_groups, const afx_device_rng* rng, uint8_t* out,
                                       size_t out_cap, size_t* out_len, uint8_t* status, size_t status_len) try {
  if (!rng) { set_error("null device rng"); return AFX_E_BAD_ARGS; }
  DrawSeed seed;   // one seed for the whole group call: every member indexes by the credential's ordinal over the groups
  int rc = out ? seed.init(rng) : AFX_OK;
  if (rc) return rc;
  return group_show_wire(group, groups, n_groups, seed.b, out, out_cap, out_len, status, status_len);
} catch (...) { return afx::exception_rc(); }

// ... over a group's devices: every group split over the members, each writing its own record range of `out`; a request of at most
// afx_ctx_set_small_batch_items credentials goes whole to one member, in turn.
extern "C" int afx_group_show_wire(afx_group* group, afx_show_group* groups, size_t n_groups, uint8_t* out, size_t out_cap, size_t* out_len,
                                   uint8_t* status, size_t status_len) try {
  return group_show_wire(group, groups, n_groups, nullptr, out, out_cap, out_len, status, status_len);
} catch (...) { return afx::exception_rc(); }

namespace {
int group_show_wire(afx_group* group, afx_show_group* groups, size_t n_groups, const uint8_t* seed40, uint8_t* out, size_t out_cap,
                    size_t* out_len, uint8_t* status, size_t status_len) {
  if (!group || !out_len) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  const uint32_t m = afx_group_size(group);
  if (m == 0) { set_error("empty group"); return AFX_E_BAD_ARGS; }
  afx_ctx* c0 = afx_group_member(group, 0);
  const uint32_t small = afx_group_small_batch_items(group);
  SPlan P;
  int rc = plan_show(c0, groups, n_groups, out != nullptr, P, seed40 != nullptr);
  if (rc) return rc;
  if (!out || m == 1 || (small && P.items <= small)) {
    const uint32_t k = out ? afx_group_pick_small(group) : 0;
    GroupPin pin(group, k, true);
    rc = show_wire(afx_group_member(group, k), groups, n_groups, seed40, out, out_cap, out_len, status, status_len);
    if (rc && m > 1) { const std::string why = afx_last_error(); set_error("member " + std::to_string(k) + ": " + why); }
    return rc;
  }
  *out_len = P.out_len;
  if (out_cap < P.out_len) { set_error("output buffer too small"); return AFX_E_BAD_ARGS; }
  if (!status && status_len) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if ((rc = check_positions(groups, n_groups, status_len))) return rc;
  for (size_t g = 0; g < n_groups; g++) groups[g].shape_out = P.jobs[g].sh;
  prepare_show(P, out, status);
  rc = on_members(group, m, [&](afx_ctx* c, uint32_t k) -> int {
    for (const SJob& J : P.jobs) {
      if (J.no_key) continue;
      size_t first = 0, n = 0;
      afx_shard_bounds(J.g->count, m, k, &first, &n);
      if (n) { const int r = show_records(c, J, first, n, seed40); if (r) return r; }
    }
    return AFX_OK;
  });
  if (rc) return rc;
  scatter_show(P, status);
  return AFX_OK;
}
}  // namespace
