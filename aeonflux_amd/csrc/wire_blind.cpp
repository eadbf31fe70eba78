// The issuer's side of blind issuance on bytes (include/aeonflux_gpu.h "Blind issuance on bytes"): AFXQ request sections in, AFXJ
// issuance sections out, and the request's verification alone over the same sections.  The doors follow wire_issue.cpp: the records of
// one layout are transposed to struct-of-arrays rows on the GPU (k_aos_to_soa), afx_issue_blind_dev runs on those rows and writes its
// outputs into further rows of the same region, and k_soa_to_aos turns those into AFXJ records - zeros for an item that failed - which
// come back in one fetch.  Only bytes move on the host.  The explicit form takes its four draws per request from host arrays, the
// _rng form has k_draw write them into the rows the plan reads (labels AFX_DRAW_BLIND_*).
// A call takes the context in turn and stages slice after slice on the two lanes (host_pipe); it never hands a small call to the
// collector of other threads' calls: blind issuance plans are not laid out for shared item slots.
#include <atomic>
#include <map>
#include <string>
#include <system_error>
#include <thread>
#include <vector>
#include "kernels.h"
#include "statements.hpp"

namespace {

uint32_t rd32(const uint8_t* b) { return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24); }
void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
bool is_hidden_kind(uint8_t k) { return k == AFX_ATTR_SECRET_SCALAR || k == AFX_ATTR_SECRET_POINT; }

// h and hs of a layout (kinds already checked to be in range)
struct Hidden { uint32_t h = 0, hs = 0; };
Hidden hidden_of(const uint8_t* kinds, uint32_t n) {
  Hidden r;
  for (uint32_t i = 0; i < n; i++) {
    r.h += is_hidden_kind(kinds[i]);
    r.hs += kinds[i] == AFX_ATTR_SECRET_SCALAR;
  }
  return r;
}
size_t header_bytes(uint32_t n) { return n > AFX_MAX_ATTRIBUTES ? 0 : (24 + (size_t)n + 31) & ~size_t(31); }
void write_header(uint8_t* h, const char* magic, size_t hdr, size_t count, uint32_t cells, uint32_t n, uint32_t nr, const uint8_t* kinds) {
  memset(h, 0, hdr);
  memcpy(h, magic, 4);
  wr32(h + 4, 1); wr32(h + 8, (uint32_t)count); wr32(h + 12, cells); wr32(h + 16, n); wr32(h + 20, nr);
  memcpy(h + 24, kinds, n);
}

// The header both formats share: magic | version | count | cells_per_record | n_attributes | n_responses | kinds | padding.
struct Header { uint32_t count, cells, n, nr; size_t hdr; };
int read_header(const uint8_t* blob, size_t len, const char* magic, Header& H) {
  if (len < 24 || memcmp(blob, magic, 4) != 0 || rd32(blob + 4) != 1) { set_error(std::string("not an ") + magic + " v1 section"); return AFX_E_BAD_ARGS; }
  H.count = rd32(blob + 8); H.cells = rd32(blob + 12); H.n = rd32(blob + 16); H.nr = rd32(blob + 20);
  if (H.n > AFX_MAX_ATTRIBUTES) { set_error("n_attributes out of range"); return AFX_E_BAD_ARGS; }
  H.hdr = header_bytes(H.n);
  if (len < H.hdr) { set_error("truncated header"); return AFX_E_BAD_ARGS; }
  for (uint32_t i = 0; i < H.n; i++)
    if (blob[24 + i] > AFX_ATTR_SECRET_POINT) { set_error("attribute kind out of range"); return AFX_E_BAD_ARGS; }
  for (size_t k = 24 + (size_t)H.n; k < H.hdr; k++)   // (the padding is part of the format: a section that parses packs to the same bytes)
    if (blob[k]) { set_error("header padding is not zero"); return AFX_E_BAD_ARGS; }
  return AFX_OK;
}
// what each format adds: the response count and the cell count that go with the kinds
int check_request_header(const uint8_t* blob, const Header& H) {
  const Hidden hd = hidden_of(blob + 24, H.n);
  if (H.nr != 1 + hd.h + hd.hs) { set_error("n_responses does not match the kinds"); return AFX_E_BAD_ARGS; }
  if (H.cells != 3 + 2 * hd.h + hd.hs + H.n) { set_error("cells_per_record does not match the layout"); return AFX_E_BAD_ARGS; }
  return AFX_OK;
}
int check_issuance_header(const Header& H) {
  if (H.nr > AFX_MAX_ATTRIBUTES + 6) { set_error("n_responses out of range"); return AFX_E_BAD_ARGS; }
  if (H.cells != 5 + H.nr) { set_error("cells_per_record does not match the layout"); return AFX_E_BAD_ARGS; }
  return AFX_OK;
}
int parse_section(const uint8_t* blob, size_t len, bool request, uint32_t* n_out, uint8_t* kinds_out, uint32_t* nr_out, size_t* count_out, size_t* rec_out) {
  if (!blob || !n_out || !kinds_out || !nr_out || !count_out || !rec_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  Header H;
  int rc = read_header(blob, len, request ? "AFXQ" : "AFXJ", H);
  if (!rc) rc = request ? check_request_header(blob, H) : check_issuance_header(H);
  if (rc) return rc;
  if (len - H.hdr != (size_t)H.count * H.cells * 32) { set_error("record area length"); return AFX_E_BAD_ARGS; }   // (count * cells * 32 < 2^45)
  memset(kinds_out, 0, AFX_MAX_ATTRIBUTES);
  memcpy(kinds_out, blob + 24, H.n);
  *n_out = H.n; *nr_out = H.nr; *count_out = H.count; *rec_out = H.hdr;
  return AFX_OK;
}
int section_bytes(const uint8_t* blob, size_t len, bool request, size_t* section_len_out) {
  if (!blob || !section_len_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  Header H;
  int rc = read_header(blob, len, request ? "AFXQ" : "AFXJ", H);
  if (!rc) rc = request ? check_request_header(blob, H) : check_issuance_header(H);
  if (rc) return rc;
  const uint64_t total = (uint64_t)H.hdr + (uint64_t)H.count * H.cells * 32;   // (< 2^46)
  if (total > len) { set_error("section runs past the end of the blob"); return AFX_E_BAD_ARGS; }
  *section_len_out = (size_t)total;
  return AFX_OK;
}

// One AFXQ section of a request stream and where its AFXJ answer goes in `out`.
struct Section {
  size_t off, hdr, count, first;   // in the request stream: bytes, header bytes, items, index of its first item in the stream
  size_t out_off, out_hdr;         // in the response stream
  uint32_t n, nrq;
  uint8_t kinds[AFX_MAX_ATTRIBUTES];
};
// The items of one layout that go to the GPU, merged over the sections that carry it: where its records, randomness and results lie
// (the caller's arrays when ONE section carries it, else copies made here and scattered afterwards).
struct Batch {
  std::vector<size_t> secs;
  size_t count = 0;
  uint32_t n = 0, nrq = 0, h = 0, hs = 0;
  uint8_t kinds[AFX_MAX_ATTRIBUTES];
  const uint8_t* rec = nullptr;                                   // [count][cells_in][32]
  const uint8_t *t_wide = nullptr, *U_wide = nullptr, *rp_wide = nullptr, *seed = nullptr;
  uint8_t* out = nullptr;                                         // [count][ctx n + 11][32] (null: the verification alone)
  uint8_t* status = nullptr;                                      // [count]
  std::vector<uint8_t> rec_buf, rnd_buf, out_buf, st_buf;
  const uint8_t* seed40 = nullptr;                                // the _rng form: the call's staged seed || stream
  std::vector<Stager::DrawPiece> draws;                           // per section: its items in the batch and the stream index of its first
  uint32_t cells_in() const { return 3 + 2 * h + hs + n; }
};
struct Stream {
  std::vector<Section> secs;
  std::vector<Batch> batches;   // in order of first appearance
  size_t total = 0, out_len = 0;
};

// Splits the stream into sections (every one parsed in full: a malformed one anywhere fails the call before anything runs) and merges
// the sections the GPU works on - n == the context's n, n != 0 - by layout.
int parse_stream(const uint8_t* blob, size_t len, uint32_t ctx_n, Stream& S) {
  if (!blob && len) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  const size_t out_cells = (size_t)ctx_n + 11;
  std::map<std::string, size_t> by_layout;
  for (size_t off = 0; off < len;) {
    size_t sl = 0, cnt = 0, rec = 0;
    Section s;
    int rc = section_bytes(blob + off, len - off, true, &sl);
    if (!rc) rc = parse_section(blob + off, sl, true, &s.n, s.kinds, &s.nrq, &cnt, &rec);
    if (rc) { set_error("section at byte " + std::to_string(off) + ": " + afx_last_error()); return rc; }
    s.off = off; s.hdr = rec; s.count = cnt; s.first = S.total;
    s.out_off = S.out_len;
    s.out_hdr = header_bytes(s.n);
    const size_t out_bytes = s.out_hdr + cnt * out_cells * 32;   // (< 2^32 * 2^6 * 2^5)
    if (__builtin_add_overflow(S.out_len, out_bytes, &S.out_len) || __builtin_add_overflow(S.total, cnt, &S.total)) {
      set_error("request stream too large");
      return AFX_E_BAD_ARGS;
    }
    if (s.n == ctx_n && s.n != 0 && cnt) {
      const std::string key((const char*)s.kinds, s.n);
      auto it = by_layout.find(key);
      if (it == by_layout.end()) {
        it = by_layout.emplace(key, S.batches.size()).first;
        S.batches.emplace_back();
        Batch& B = S.batches.back();
        const Hidden hd = hidden_of(s.kinds, s.n);
        B.n = s.n; B.nrq = s.nrq; B.h = hd.h; B.hs = hd.hs;
        memcpy(B.kinds, s.kinds, AFX_MAX_ATTRIBUTES);
      }
      S.batches[it->second].secs.push_back(S.secs.size());
      S.batches[it->second].count += cnt;
    }
    S.secs.push_back(s);
    off += sl;
  }
  return AFX_OK;
}

bool all_there(const afx_blind_issue_randomness* r) { return r && r->t_wide && r->U_wide && r->rprime_wide && r->rng_seed; }

// What must hold before anything is written or launched (the size query has returned before this).  issue == false: the
// verification alone, which writes statuses only and needs neither randomness nor the key.
int check_call(afx_ctx* ctx, const Stream& S, bool issue, const afx_blind_issue_randomness* rnd, const uint8_t* seed40, size_t out_cap, const uint8_t* status,
               size_t status_cap) {
  if (issue && out_cap < S.out_len) { set_error("output buffer too small"); return AFX_E_BAD_ARGS; }
  if (status_cap < S.total || (!status && S.total)) { set_error("status buffer too small"); return AFX_E_BAD_ARGS; }
  if (issue && !seed40 && !all_there(rnd)) { set_error("null randomness array"); return AFX_E_BAD_ARGS; }
  for (const Batch& B : S.batches)
    if (B.count > 0xffffffffu / 64) { set_error("too many requests of one layout"); return AFX_E_BAD_ARGS; }
  if (issue && !ctx->has_key) { set_error("blind issuance needs the issuer key"); return AFX_E_NO_KEY; }
  return AFX_OK;
}

// Every section's AFXJ header; the sections the GPU does not see (n != the context's n, or n == 0) get records of zeros and their
// statuses here: what afx_issue_blind (MacCreation, amacs.rs:285-287) and afx_verify_blind_requests answer a layout that does not fit.
// Then every batch's arrays: the caller's own, or gathered copies.
void prepare(Stream& S, const uint8_t* blob, bool issue, const afx_blind_issue_randomness* rnd, const uint8_t* seed40, uint32_t ctx_n, uint8_t* out, uint8_t* status) {
  const uint32_t nr = ctx_n + 6, out_cells = 5 + nr;
  for (const Section& s : S.secs) {
    const bool on_gpu = s.n == ctx_n && s.n != 0;
    if (issue) {
      uint8_t* h = out + s.out_off;
      write_header(h, "AFXJ", s.out_hdr, s.count, out_cells, s.n, nr, s.kinds);
      if (!on_gpu) memset(h + s.out_hdr, 0, s.count * out_cells * 32);
    }
    if (!on_gpu) memset(status + s.first, issue ? AFX_ST_MAC_CREATION : AFX_ST_VERIFICATION_FAILURE, s.count);
  }
  for (Batch& B : S.batches) {
    const size_t rb = (size_t)B.cells_in() * 32, ob = (size_t)out_cells * 32;
    if (seed40) {   // (no rnd_buf: the draws land in the staged rows themselves)
      B.seed40 = seed40;
      size_t at = 0;
      for (size_t k : B.secs) { B.draws.push_back({ at, S.secs[k].count, (uint64_t)S.secs[k].first }); at += S.secs[k].count; }
    }
    const bool host_rnd = issue && !seed40;
    if (B.secs.size() == 1) {
      const Section& s = S.secs[B.secs[0]];
      B.rec = blob + s.off + s.hdr;
      if (host_rnd) {
        B.t_wide = rnd->t_wide + s.first * 64; B.U_wide = rnd->U_wide + s.first * 64; B.rp_wide = rnd->rprime_wide + s.first * 64;
        B.seed = rnd->rng_seed + s.first * 32;
      }
      if (issue) B.out = out + s.out_off + s.out_hdr;
      B.status = status + s.first;
      continue;
    }
    B.rec_buf.resize(B.count * rb);
    if (host_rnd) B.rnd_buf.resize(B.count * 224);
    if (issue) B.out_buf.assign(B.count * ob, 0);
    B.st_buf.assign(B.count, issue ? AFX_ST_MAC_CREATION : AFX_ST_VERIFICATION_FAILURE);
    uint8_t *tw = nullptr, *uw = nullptr, *rw = nullptr, *sd = nullptr;   // (rnd_buf is empty without host randomness: no offsets from its null data())
    if (host_rnd) { tw = B.rnd_buf.data(); uw = tw + B.count * 64; rw = uw + B.count * 64; sd = rw + B.count * 64; }
    size_t at = 0;
    for (size_t k : B.secs) {
      const Section& s = S.secs[k];
      memcpy(B.rec_buf.data() + at * rb, blob + s.off + s.hdr, s.count * rb);
      if (host_rnd) {
        memcpy(tw + at * 64, rnd->t_wide + s.first * 64, s.count * 64);
        memcpy(uw + at * 64, rnd->U_wide + s.first * 64, s.count * 64);
        memcpy(rw + at * 64, rnd->rprime_wide + s.first * 64, s.count * 64);
        memcpy(sd + at * 32, rnd->rng_seed + s.first * 32, s.count * 32);
      }
      at += s.count;
    }
    B.rec = B.rec_buf.data();
    if (host_rnd) { B.t_wide = tw; B.U_wide = uw; B.rp_wide = rw; B.seed = sd; }
    if (issue) B.out = B.out_buf.data();
    B.status = B.st_buf.data();
  }
}
// results of the batches that were gathered go back to their sections; the gathered randomness is wiped
void scatter(Stream& S, bool issue, uint32_t ctx_n, uint8_t* out, uint8_t* status) {
  const size_t ob = (size_t)(ctx_n + 11) * 32;
  for (Batch& B : S.batches) {
    if (!B.rnd_buf.empty()) afx::afx_wipe(B.rnd_buf.data(), B.rnd_buf.size());
    if (B.secs.size() == 1) continue;
    size_t at = 0;
    for (size_t k : B.secs) {
      const Section& s = S.secs[k];
      if (issue) memcpy(out + s.out_off + s.out_hdr, B.out + at * ob, s.count * ob);
      memcpy(status + s.first, B.status + at, s.count);
      at += s.count;
    }
  }
}

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
  const uint32_t na = B.n, h = B.h, rq = 3 + 3 * h + B.hs, cells_in = B.cells_in(), out_cells = issue ? na + 11 : 0, rows = rq + na + out_cells;
  std::vector<uint32_t> map_in(cells_in), map_out(out_cells ? out_cells : 1);
  for (uint32_t c = 0; c < rq; c++) map_in[c] = c;   // D, A, B, challenge, responses: the record's order is the rows' order
  for (uint32_t i = 0, c = rq; i < na; i++)
    if (!is_hidden_kind(B.kinds[i])) map_in[c++] = rq + i;   // a revealed value lands on the row of its position
  for (uint32_t c = 0; c < out_cells; c++) map_out[c] = rq + na + c;
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
      o_tw = st.add_rows(B.t_wide, 1, 64, total, f0, sn, dn);
      o_uw = st.add_rows(B.U_wide, 1, 64, total, f0, sn, dn);
      o_rw = st.add_rows(B.rp_wide, 1, 64, total, f0, sn, dn);
      o_seed = st.add_rows(B.seed, 1, 32, total, f0, sn, dn);
    }
    const size_t o_soa = st.reserve(dn * rows * 32);
    const size_t o_out = issue ? st.add_rows(nullptr, 1, (size_t)out_cells * 32, total, f0, sn, dn) : 0, o_st = st.add(nullptr, dn);
    if (issue) st.plan_fetch(B.out, o_out, 1, (size_t)out_cells * 32, total, f0, sn, dn);
    st.plan_fetch(B.status, o_st, 1, 1, total, f0, sn, dn);
    int rc = st.upload();
    if (rc) return rc;
    hipStream_t strm = st.stream();
    uint8_t* soa_d = st.dev(o_soa);
    AFX_HIP(afxk_aos_to_soa(strm, st.dev(o_rec), soa_d, (const uint32_t*)st.dev(o_min), cells_in, (uint32_t)dn));
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
    AFX_HIP(afxk_soa_to_aos(strm, soa_d, st.dev(o_out), (const uint32_t*)st.dev(o_mout), st.dev(o_st), out_cells, (uint32_t)dn));
    return st.fetch_all();
  }, PlanKey(), true);   // never collected: a small call too runs its slices itself
}

// may small calls of a group go to any member (the members' settings alike, as group.cpp run_members requires)?
bool members_alike(afx_group* g, uint32_t m) {
  struct Set { uint32_t sb, chunk; bool strict, fixed, timing, trace; int secret; };
  auto of = [](afx_ctx* c) { std::lock_guard<std::mutex> l(c->settings_mu); return Set{ c->small_batch_items, c->chunk_items, c->strict, c->fixed_key_schedule, c->timing, c->trace != nullptr, c->secret_mode }; };
  const Set s0 = of(afx_group_member(g, 0));
  if (s0.trace) return false;
  for (uint32_t k = 1; k < m; k++) {
    const Set s = of(afx_group_member(g, k));
    if (s.sb != s0.sb || s.chunk != s0.chunk || s.strict != s0.strict || s.fixed != s0.fixed || s.timing != s0.timing || s.secret != s0.secret || s.trace) return false;
  }
  return true;
}
std::atomic<uint32_t> g_next_small{ 0 };

// A parsed stream (parse_stream with this context's n) on one context: afx_issue_blind_wire (seed40 == null), afx_issue_blind_wire_rng
// (seed40: the staged seed || stream; rnd is not read) and, with issue == false, afx_verify_blind_requests_wire (out, rnd and seed40
// are not used)
int run_door(afx_ctx* ctx, Stream& S, bool issue, const uint8_t* blob, const afx_blind_issue_randomness* rnd, const uint8_t* seed40, uint8_t* out, size_t out_cap,
             size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) {
  int rc = AFX_OK;
  if (issue) *out_len = S.out_len;
  *count_out = S.total;
  if (issue && !out) return AFX_OK;   // size query: headers only
  if ((rc = check_call(ctx, S, issue, rnd, seed40, out_cap, status, status_cap))) return rc;
  prepare(S, blob, issue, rnd, seed40, ctx->n, out, status);
  for (size_t b = 0; b < S.batches.size() && !rc; b++) {
    rc = run_records(ctx, S.batches[b], 0, S.batches[b].count);
    if (rc && S.batches.size() > 1) { const std::string why = afx_last_error(); set_error("layout " + std::to_string(b) + ": " + why); }
  }
  scatter(S, issue, ctx->n, out, status);   // (after a failure too: the gathered randomness is wiped there)
  return rc;
}
int door(afx_ctx* ctx, bool issue, const uint8_t* blob, size_t len, const afx_blind_issue_randomness* rnd, const uint8_t* seed40, uint8_t* out, size_t out_cap,
         size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) {
  if (!ctx || (issue && !out_len) || !count_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  Stream S;
  const int rc = parse_stream(blob, len, ctx->n, S);
  return rc ? rc : run_door(ctx, S, issue, blob, rnd, seed40, out, out_cap, out_len, status, status_cap, count_out);
}

// The same stream over a group's devices.  A stream of at most afx_ctx_set_small_batch_items requests (member 0's) goes whole to ONE
// member, the next in turn; a larger one has every batch split over the members (afx_shard_bounds), one host thread per member, each
// writing its own record range of `out`.  The headers and the MacCreation sections are written once, here.
int group_door(afx_group* group, const uint8_t* blob, size_t len, const afx_blind_issue_randomness* rnd, const uint8_t* seed40, uint8_t* out, size_t out_cap,
               size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) {
  if (!group || !out_len || !count_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  const uint32_t m = afx_group_size(group);
  if (m == 0) { set_error("empty group"); return AFX_E_BAD_ARGS; }
  afx_ctx* c0 = afx_group_member(group, 0);
  const uint32_t small = afx_group_small_batch_items(group);
  Stream S;   // parsed once, for whichever path (the members share the parameters, so member 0's n is every member's)
  int rc = parse_stream(blob, len, c0->n, S);
  if (rc) return rc;
  if (m == 1 || (small && len && S.total <= small)) {
    const uint32_t k = m == 1 ? 0 : members_alike(group, m) ? g_next_small.fetch_add(1, std::memory_order_relaxed) % m : 0;
    GroupPin pin(group, k, true);
    rc = run_door(afx_group_member(group, k), S, true, blob, rnd, seed40, out, out_cap, out_len, status, status_cap, count_out);
    if (rc && m > 1) { const std::string why = afx_last_error(); set_error("member " + std::to_string(k) + ": " + why); }
    return rc;
  }
  *out_len = S.out_len;
  *count_out = S.total;
  if (!out) return AFX_OK;
  if ((rc = check_call(c0, S, true, rnd, seed40, out_cap, status, status_cap))) return rc;
  prepare(S, blob, true, rnd, seed40, c0->n, out, status);
  std::vector<int> rcs(m, AFX_OK);
  std::vector<std::string> errs(m);
  auto body = [&](uint32_t k) {
    GroupPin pin(group, k, k == 0);   // the member's thread on its device's NUMA node (member 0: the caller's thread, restored)
    afx_ctx* c = afx_group_member(group, k);
    try {
      for (const Batch& B : S.batches) {
        size_t first = 0, n = 0;
        afx_shard_bounds(B.count, m, k, &first, &n);
        if (n && (rcs[k] = run_records(c, B, first, n))) { errs[k] = afx_last_error(); return; }   // (the error string is per thread)
      }
    } catch (...) { rcs[k] = afx::exception_rc(); errs[k] = afx_last_error(); }
  };
  std::vector<std::thread> threads;
  for (uint32_t k = 1; k < m; k++) {
    try { threads.emplace_back(body, k); } catch (const std::system_error&) { body(k); }
  }
  body(0);
  for (std::thread& t : threads) t.join();
  scatter(S, true, c0->n, out, status);
  for (uint32_t k = 0; k < m; k++)
    if (rcs[k]) { set_error("member " + std::to_string(k) + ": " + errs[k]); return rcs[k]; }
  return AFX_OK;
}

}  // namespace

// ---- the two formats: host only, bytes only ----
extern "C" size_t afx_blind_request_wire_header_bytes(uint32_t n_attributes) { return header_bytes(n_attributes); }
extern "C" size_t afx_blind_issuance_wire_header_bytes(uint32_t n_attributes) { return header_bytes(n_attributes); }

extern "C" int afx_blind_request_wire_parse(const uint8_t* blob, size_t len, uint32_t* n_attributes_out, uint8_t kinds_out[AFX_MAX_ATTRIBUTES],
                                            uint32_t* n_responses_out, size_t* count_out, size_t* records_offset_out) try {
  return parse_section(blob, len, true, n_attributes_out, kinds_out, n_responses_out, count_out, records_offset_out);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_blind_issuance_wire_parse(const uint8_t* blob, size_t len, uint32_t* n_attributes_out, uint8_t kinds_out[AFX_MAX_ATTRIBUTES],
                                             uint32_t* n_responses_out, size_t* count_out, size_t* records_offset_out) try {
  return parse_section(blob, len, false, n_attributes_out, kinds_out, n_responses_out, count_out, records_offset_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_blind_request_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out) try {
  return section_bytes(blob, len, true, section_len_out);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_blind_issuance_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out) try {
  return section_bytes(blob, len, false, section_len_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_blind_request_wire_pack(const afx_attributes_soa* attrs, const afx_blind_request_soa* requests, size_t count, uint8_t* blob, size_t blob_cap,
                                           size_t* len_out) try {
  if (!attrs || !requests || !len_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  const uint32_t n = attrs->n_attributes;
  const size_t hdr = header_bytes(n);
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
  write_header(blob, "AFXQ", hdr, count, cells, n, nr, attrs->kinds);
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
  const size_t hdr = header_bytes(n);
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
  write_header(blob, "AFXJ", hdr, count, cells, n, n_responses, attrs->kinds);
  uint8_t* rec = blob + hdr;
  auto put = [&](const uint8_t* base, size_t row, size_t i) { memcpy(rec, base + (row * count + i) * 32, 32); rec += 32; };
  for (size_t i = 0; i < count; i++) {
    put(s.t, 0, i); put(s.U, 0, i); put(s.S1, 0, i); put(s.S2, 0, i); put(s.challenge, 0, i);
    for (uint32_t k = 0; k < n_responses; k++) put(s.responses, k, i);
  }
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }

// ---- the doors ----
extern "C" int afx_issue_blind_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_blind_issue_randomness* rnd, uint8_t* out, size_t out_cap,
                                    size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  return door(ctx, true, blob, len, rnd, nullptr, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_group_issue_blind_wire(afx_group* group, const uint8_t* blob, size_t len, const afx_blind_issue_randomness* rnd, uint8_t* out, size_t out_cap,
                                          size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  return group_door(group, blob, len, rnd, nullptr, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_verify_blind_requests_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  return door(ctx, false, blob, len, nullptr, nullptr, nullptr, 0, nullptr, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_issue_blind_wire_rng(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_device_rng* rng, uint8_t* out, size_t out_cap, size_t* out_len,
                                        uint8_t* status, size_t status_cap, size_t* count_out) try {
  if (!rng) { set_error("null device rng"); return AFX_E_BAD_ARGS; }
  DrawSeed seed;
  const int rc = out ? seed.init(rng) : AFX_OK;   // (the size query draws nothing)
  if (rc) return rc;
  return door(ctx, true, blob, len, nullptr, seed.b, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_group_issue_blind_wire_rng(afx_group* group, const uint8_t* blob, size_t len, const afx_device_rng* rng, uint8_t* out, size_t out_cap,
                                              size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  if (!rng) { set_error("null device rng"); return AFX_E_BAD_ARGS; }
  DrawSeed seed;   // one seed for the whole group call: every member indexes by the request's ordinal in the stream
  const int rc = out ? seed.init(rng) : AFX_OK;
  if (rc) return rc;
  return group_door(group, blob, len, nullptr, seed.b, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }
