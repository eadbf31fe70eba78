// The user's side of blind issuance on bytes (include/aeonflux_gpu.h "Blind issuance on bytes: the user's doors"): attribute columns in,
// AFXQ request sections out (afx_blind_request_wire), and AFXJ issuance sections in, the credential's t, U, V out
// (afx_unblind_issuances_wire), each with its _rng form - d, r_wide and rng_seed drawn on the device (labels AFX_DRAW_BLINDREQ_*),
// d re-derived by the unblinding call from the same seed - and its form over a group's devices.  Only bytes move on the host: per
// slice the request door has afx_blind_request_dev write D, A, B, the challenge and the responses into rows behind the staged value
// rows and k_soa_to_aos make the records of them; the unblinding door transposes both record streams into one row region
// (k_aos_to_soa), runs afx_unblind_issuances_dev on it and copies t, U and V out through k_soa_to_aos, which zeroes a failed item.
// Like wire_blind.cpp's doors a call takes the context in turn and stages slice after slice on the two lanes (host_pipe); it is never
// handed to the collector of other threads' calls.  The two formats are entries of wire_formats.hpp's table; the cell maps are records.hpp's
// (the launches here stay where they are: they interleave with k_reduce_wide and the wipes).
#include <map>
#include <string>
#include <vector>
#include "records.hpp"
#include "request_stream.hpp"

namespace {

// one context, or the members of a group
struct Where {
  afx_ctx* ctx = nullptr;
  afx_group* group = nullptr;
  afx_ctx* first() const { return group ? (afx_group_size(group) ? afx_group_member(group, 0) : nullptr) : ctx; }
};
int check_where(const Where& w) {
  if (!w.ctx && !w.group) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (w.group && afx_group_size(w.group) == 0) { set_error("empty group"); return AFX_E_BAD_ARGS; }
  return AFX_OK;
}
// run(context, b, first, n) over the items of every batch b: on one context batch after batch; over a group as every group door goes
// (doors.hpp): a stream of at most afx_ctx_set_small_batch_items items whole on one member, else every batch split over the members
template <class Run>
int spread(const Where& w, size_t total, const std::vector<size_t>& counts, Run&& run) {
  auto whole = [&](afx_ctx* c) -> int {
    for (size_t b = 0; b < counts.size(); b++)
      if (counts[b]) { const int rc = run(c, b, size_t(0), counts[b]); if (rc) return rc; }
    return AFX_OK;
  };
  if (!w.group) return whole(w.ctx);
  const uint32_t m = afx_group_size(w.group), small = afx_group_small_batch_items(w.group);
  if (m == 1 || (small && total <= small)) return on_one_member(w.group, m, whole);
  return shard_over_members(w.group, m, counts, run);
}
// rows that held d or d_wide: zeros in stream order, whatever became of the launches in front (the first failure is what the call returns)
int wipe_rows(hipStream_t s, int rc, std::initializer_list<std::pair<uint8_t*, size_t>> rows) {
  for (const auto& r : rows) {
    const hipError_t e = r.second ? hipMemsetAsync(r.first, 0, r.second, s) : hipSuccess;
    if (e != hipSuccess && !rc) { set_error(std::string("hipMemsetAsync: ") + hipGetErrorString(e)); rc = AFX_E_HIP; }
  }
  return rc;
}

// ------------------------------------------------------------------------------------------------
// afx_blind_request_wire
// ------------------------------------------------------------------------------------------------
// One group of the call and the AFXQ section it becomes.  n: what the section's header says - the group's n_attributes, or 0 kinds
// for a group of none or of more than AFX_MAX_ATTRIBUTES.
struct ReqGroup {
  const afx_blind_request_group* g = nullptr;
  uint32_t n = 0, h = 0, hs = 0, cells = 3, nr = 1;
  uint8_t kinds[AFX_MAX_ATTRIBUTES];
  bool on_gpu = false;             // the context's layout: everything else is zero records and AFX_ST_MAC_CREATION, written on the host
  size_t count = 0, first = 0;     // items, and the stream index of the first
  size_t out_off = 0, hdr = 0;
  uint8_t* rec = nullptr;          // [count][cells][32]
  uint8_t* status = nullptr;       // [count]
  uint8_t* d_out = nullptr;        // [count] Sc, or null
  const uint8_t* seed40 = nullptr; // the _rng form: d, r_wide and rng_seed are drawn, the group's own are not read
};
struct ReqPlan {
  std::vector<ReqGroup> groups;
  size_t total = 0, out_len = 0;
};
int plan_request(uint32_t ctx_n, const afx_blind_request_group* groups, size_t n_groups, ReqPlan& P) {
  if (!groups && n_groups) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  for (size_t k = 0; k < n_groups; k++) {
    const afx_attributes_soa& a = groups[k].attrs;
    ReqGroup G;
    G.g = &groups[k];
    memset(G.kinds, 0, sizeof G.kinds);
    for (uint32_t i = 0; i < a.n_attributes && i < AFX_MAX_ATTRIBUTES; i++)
      if (a.kinds[i] > AFX_ATTR_SECRET_POINT) { set_error("group " + std::to_string(k) + ": attribute kind out of range"); return AFX_E_BAD_ARGS; }   // no AFXQ header carries it
    G.n = a.n_attributes > AFX_MAX_ATTRIBUTES ? 0 : a.n_attributes;
    memcpy(G.kinds, a.kinds, G.n);
    const Hidden hd = hidden_of(G.kinds, G.n);
    G.h = hd.h; G.hs = hd.hs; G.cells = 3 + 2 * hd.h + hd.hs + G.n; G.nr = 1 + hd.h + hd.hs;
    G.on_gpu = a.n_attributes == ctx_n && a.n_attributes != 0 && a.n_attributes <= AFX_MAX_ATTRIBUTES;
    G.count = groups[k].count;
    if (G.count > 0xffffffffu / 64) { set_error("too many requests in one group"); return AFX_E_BAD_ARGS; }
    G.first = P.total;
    G.out_off = P.out_len;
    G.hdr = header_bytes(FORMATS[AFXQ], G.n);
    const size_t bytes = G.hdr + G.count * G.cells * 32;   // (< 2^26 * 2^8 * 2^5)
    if (__builtin_add_overflow(P.out_len, bytes, &P.out_len) || __builtin_add_overflow(P.total, G.count, &P.total)) {
      set_error("request stream too large");
      return AFX_E_BAD_ARGS;
    }
    P.groups.push_back(G);
  }
  return AFX_OK;
}

// Items [first, first + n) of a group.  Per pass the staging area holds the rows
//   values[n] | D | A[h] | B[h] | challenge | responses[1 + h + hs]
// in one piece: the value rows come from the host (all positions: the plan checks every one), afx_blind_request_dev writes the rows
// behind them, and k_soa_to_aos makes the records of those and of the revealed positions' value rows - zeros for an item that failed -
// which come back in one fetch.  The pass runs on a multiple of 8 items, so that the two parts of the region meet (rows of 256 bytes'
// multiples); the lanes beyond the slice work on zeros and nothing of them is fetched.
int run_request(afx_ctx* ctx, const ReqGroup& G, size_t first, size_t n) {
  CtxLock lock__(ctx);   // the context in turn: no session of the collector collects or is in flight from here on
  if (n == 0) return AFX_OK;
  AFX_HIP(hipSetDevice(ctx->device));
  if (G.n != ctx->n) { set_error("internal: request layout of another context"); return AFX_E_BAD_ARGS; }
  const uint32_t na = G.n, h = G.h, rq = 3 + 3 * h + G.hs, cells = G.cells;
  // D, A, B, challenge, responses: the rows' order is the record's; the value rows lie in front of them
  const std::vector<uint32_t> map = blind_request_map(G.kinds, na, rq, na, 0);
  if (map.size() != cells) { set_error("internal: AFXQ cell map"); return AFX_E_BAD_ARGS; }
  const uint32_t one_cell = 0;
  const afx_blind_request_group& g = *G.g;
  const size_t total = G.count;
  const std::vector<Stager::DrawPiece> draws = { { 0, total, (uint64_t)G.first } };
  return host_pipe(ctx, n, [&](Stager& st, size_t off, size_t sn) -> int {
    if (st.ses || st.app) { set_error("internal: a blind wire call inside a collected session"); return AFX_E_BAD_ARGS; }
    const size_t f0 = first + off;
    const bool drawn = G.seed40 != nullptr;
    const bool want_d = drawn && G.d_out != nullptr;   // d leaves its scratch row only for a caller that asked for it
    st.layout_tag = want_d ? 13 : drawn ? 10 : 9;
    const size_t dn = (st.dev_items(sn) + 7) & ~size_t(7);
    const size_t o_val = st.add_rows(g.attrs.values, na, 32, total, f0, sn, dn), o_req = st.reserve(dn * rq * 32);
    if (o_req != o_val + dn * na * 32) { set_error("internal: the request rows do not follow the value rows"); return AFX_E_BAD_ARGS; }
    const size_t o_map = st.add((const uint8_t*)map.data(), 4 * (size_t)cells), o_one = st.add((const uint8_t*)&one_cell, 4);
    size_t o_d = 0, o_dw = 0, o_rw = 0, o_seed = 0;
    if (drawn) {   // drawn on the device after the upload, into the rows k_reduce_wide and the plan read
      const size_t s_at = st.add_seed(G.seed40, dn);
      o_dw = st.add_drawn(s_at, AFX_DRAW_BLINDREQ_D_WIDE, 1, draws, f0, sn, dn);
      o_d = st.reserve(dn * 32);
      o_rw = h ? st.add_drawn(s_at, AFX_DRAW_BLINDREQ_R_WIDE(0), h, draws, f0, sn, dn) : st.reserve(0);
      o_seed = st.add_drawn(s_at, AFX_DRAW_BLINDREQ_SEED, 1, draws, f0, sn, dn);
    } else {
      o_d = st.add_rows(g.d, 1, 32, total, f0, sn, dn);
      o_rw = h ? st.add_rows(g.rnd.r_wide, h, 64, total, f0, sn, dn) : st.reserve(0);
      o_seed = st.add_rows(g.rnd.rng_seed, 1, 32, total, f0, sn, dn);
    }
    const size_t o_out = st.add_rows(nullptr, 1, (size_t)cells * 32, total, f0, sn, dn), o_st = st.add(nullptr, dn);
    const size_t o_dout = want_d ? st.add_rows(nullptr, 1, 32, total, f0, sn, dn) : 0;
    st.plan_fetch(G.rec, o_out, 1, (size_t)cells * 32, total, f0, sn, dn);
    st.plan_fetch(G.status, o_st, 1, 1, total, f0, sn, dn);
    if (want_d) st.plan_fetch(G.d_out, o_dout, 1, 32, total, f0, sn, dn);
    int rc = st.upload();
    if (rc) return rc;
    hipStream_t strm = st.stream();
    uint8_t* soa_d = st.dev(o_val);
    auto rowp = [&](uint32_t r) { return soa_d + (size_t)r * dn * 32; };
    afx_attributes_soa da;
    memset(&da, 0, sizeof da);
    da.n_attributes = na; memcpy(da.kinds, G.kinds, AFX_MAX_ATTRIBUTES);
    da.values = soa_d;
    const afx_blind_request_randomness dr = { st.dev(o_rw), st.dev(o_seed) };
    const afx_blind_request_soa dout = { rowp(na), rowp(na + 1), rowp(na + 1 + h), rowp(na + 1 + 2 * h), rowp(na + 2 + 2 * h) };
    auto launch = [&]() -> int {
      if (drawn) AFX_HIP(afxk_reduce_wide(strm, st.dev(o_dw), st.dev(o_d), (uint32_t)dn));   // d = from_bytes_mod_order_wide(d_wide)
      const int r = afx_blind_request_dev(ctx, &da, st.dev(o_d), &dr, dn, &dout, st.dev(o_st));
      if (r) return r;
      AFX_HIP(afxk_soa_to_aos(strm, soa_d, st.dev(o_out), (const uint32_t*)st.dev(o_map), st.dev(o_st), cells, (uint32_t)dn));
      if (want_d) AFX_HIP(afxk_soa_to_aos(strm, st.dev(o_d), st.dev(o_dout), (const uint32_t*)st.dev(o_one), st.dev(o_st), 1, (uint32_t)dn));   // d, zeros for a failed item
      return AFX_OK;
    };
    rc = launch();
    if (drawn) rc = wipe_rows(strm, rc, { { st.dev(o_dw), dn * 64 }, { st.dev(o_d), dn * 32 } });
    if (!rc) rc = st.fetch_all();
    // the staged copy of d_out goes too, behind the copy that fetches it (a failed slice fetches nothing): what is left of d is the caller's own
    if (want_d) rc = wipe_rows(strm, rc, { { st.dev(o_dout), dn * 32 } });
    return rc;
  }, PlanKey(), true);   // never collected: a small call too runs its slices itself
}

int request_wire(const Where& w, const afx_blind_request_group* groups, size_t n_groups, const uint8_t* seed40, uint8_t* d_out, uint8_t* out, size_t out_cap,
                 size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) {
  int rc = check_where(w);
  if (rc) return rc;
  if (!out_len || !count_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  ReqPlan P;
  if ((rc = plan_request(w.first()->n, groups, n_groups, P))) return rc;
  *out_len = P.out_len;
  *count_out = P.total;
  if (!out) return AFX_OK;   // size query: from the kinds and the counts
  if (out_cap < P.out_len) { set_error("output buffer too small"); return AFX_E_BAD_ARGS; }
  if (status_cap < P.total || (!status && P.total)) { set_error("status buffer too small"); return AFX_E_BAD_ARGS; }
  for (const ReqGroup& G : P.groups) {
    const afx_blind_request_group& g = *G.g;
    if (!G.count) continue;
    if ((G.n && !g.attrs.values) || (!seed40 && (!g.d || !g.rnd.rng_seed || (G.h && !g.rnd.r_wide)))) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
  }
  std::vector<size_t> counts;
  for (ReqGroup& G : P.groups) {
    uint8_t* hd = out + G.out_off;
    write_header(FORMATS[AFXQ], hd, G.count, G.cells, G.n, G.nr, G.kinds);
    G.rec = hd + G.hdr;
    G.status = status + G.first;
    G.d_out = d_out ? d_out + G.first * 32 : nullptr;
    G.seed40 = seed40;
    if (!G.on_gpu) {   // a layout the context does not serve (amacs.rs:285-287, as afx_blind_request answers it)
      memset(G.rec, 0, G.count * G.cells * 32);
      memset(G.status, AFX_ST_MAC_CREATION, G.count);
      if (G.d_out) memset(G.d_out, 0, G.count * 32);
    }
    counts.push_back(G.on_gpu ? G.count : 0);
  }
  return spread(w, P.total, counts, [&](afx_ctx* c, size_t b, size_t first, size_t n) { return run_request(c, P.groups[b], first, n); });
}
int request_wire_rng(const Where& w, const afx_blind_request_group* groups, size_t n_groups, const afx_device_rng* rng, uint8_t* d_out, uint8_t* out, size_t out_cap,
                     size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) {
  if (!rng) { set_error("null device rng"); return AFX_E_BAD_ARGS; }
  if (out && !d_out && !rng->seed) { set_error("a seed from getrandom and no d_out: the requests could never be unblinded"); return AFX_E_BAD_ARGS; }
  DrawSeed seed;   // one seed for the whole call, a group call too: a draw depends on the item's index in the stream only
  const int rc = out ? seed.init(rng) : AFX_OK;   // (the size query draws nothing)
  if (rc) return rc;
  return request_wire(w, groups, n_groups, seed.b, d_out, out, out_cap, out_len, status, status_cap, count_out);
}

// ------------------------------------------------------------------------------------------------
// afx_unblind_issuances_wire
// ------------------------------------------------------------------------------------------------
// An AFXJ section and the AFXQ section it answers
struct Pair {
  size_t q_rec = 0, j_rec = 0;   // where the records start in the two streams
  size_t count = 0, first = 0;
  uint32_t n = 0, nrj = 0;
  uint8_t kinds[AFX_MAX_ATTRIBUTES];
};
// The pairs of one layout, merged: where their records, d and results lie (the caller's arrays when ONE pair carries the layout, else
// copies made here and scattered afterwards)
struct UBatch {
  std::vector<size_t> pairs;
  size_t count = 0;
  uint32_t n = 0, h = 0, hs = 0, cells_q = 0, cells_j = 0;
  uint8_t kinds[AFX_MAX_ATTRIBUTES];
  const uint8_t *recq = nullptr, *recj = nullptr, *d = nullptr;
  uint8_t *t = nullptr, *U = nullptr, *V = nullptr, *status = nullptr;
  std::vector<uint8_t> q_buf, j_buf, d_buf, out_buf, st_buf;
  const uint8_t* seed40 = nullptr;   // the _rng form: d is drawn again at the items' stream indices
  std::vector<Stager::DrawPiece> draws;
};
struct UStream {
  std::vector<Pair> pairs;
  std::vector<UBatch> batches;   // in order of first appearance
  size_t total = 0;
};
bool on_gpu(const Pair& p, uint32_t ctx_n) { return p.n == ctx_n && p.n != 0 && p.nrj == ctx_n + 6; }

// both streams, section by section, every one parsed in full before anything runs
int parse_pairs(const uint8_t* iss, size_t iss_len, const uint8_t* req, size_t req_len, uint32_t ctx_n, UStream& S) {
  if ((!iss && iss_len) || (!req && req_len)) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  std::map<std::string, size_t> by_layout;
  size_t jo = 0, qo = 0;
  while (jo < iss_len || qo < req_len) {
    const std::string at = "section " + std::to_string(S.pairs.size()) + ": ";
    if (jo >= iss_len || qo >= req_len) { set_error("the issuance stream and the request stream differ in their section counts"); return AFX_E_BAD_ARGS; }
    Header J, Q;
    int rc = read_section(FORMATS[AFXJ], iss + jo, iss_len - jo, J);
    if (rc) { set_error(at + "issuance: " + afx_last_error()); return rc; }
    if ((rc = read_section(FORMATS[AFXQ], req + qo, req_len - qo, Q))) { set_error(at + "request: " + afx_last_error()); return rc; }
    if (J.count != Q.count || J.n != Q.n || memcmp(J.kinds, Q.kinds, J.n) != 0) { set_error(at + "the issuance section does not answer the request section (count, n_attributes or kinds)"); return AFX_E_BAD_ARGS; }
    const size_t jc = J.count, jl = J.section, ql = Q.section;
    Pair p;
    p.q_rec = qo + Q.hdr; p.j_rec = jo + J.hdr; p.count = jc; p.first = S.total; p.n = J.n; p.nrj = J.nr;
    memset(p.kinds, 0, sizeof p.kinds);
    memcpy(p.kinds, J.kinds, J.n);
    if (__builtin_add_overflow(S.total, jc, &S.total)) { set_error("issuance stream too large"); return AFX_E_BAD_ARGS; }
    if (on_gpu(p, ctx_n) && jc) {
      const std::string key((const char*)p.kinds, p.n);
      auto it = by_layout.find(key);
      if (it == by_layout.end()) {
        it = by_layout.emplace(key, S.batches.size()).first;
        S.batches.emplace_back();
        UBatch& B = S.batches.back();
        const Hidden hd = hidden_of(p.kinds, p.n);
        B.n = p.n; B.h = hd.h; B.hs = hd.hs; B.cells_q = 3 + 2 * hd.h + hd.hs + p.n; B.cells_j = 5 + p.nrj;
        memcpy(B.kinds, p.kinds, AFX_MAX_ATTRIBUTES);
      }
      S.batches[it->second].pairs.push_back(S.pairs.size());
      S.batches[it->second].count += jc;
    }
    S.pairs.push_back(p);
    jo += jl; qo += ql;
  }
  for (const UBatch& B : S.batches)
    if (B.count > 0xffffffffu / 64) { set_error("too many issuances of one layout"); return AFX_E_BAD_ARGS; }
  return AFX_OK;
}

// Items [first, first + n) of a batch.  Per pass one region of scratch holds the rows
//   D | A[h] | B[h] | challenge | responses[1 + h + hs] | values[n] | t | U | S1 | S2 | challenge | responses[n + 6] | V   (| d, the _rng form)
// k_aos_to_soa fills the issuance rows and then the request rows and the value rows of the revealed positions (the rows of hidden
// positions are part of the region and are never read), afx_unblind_issuances_dev reads those and writes V, and k_soa_to_aos copies t,
// U and V out, a row each - zeros for an item that failed.  Five transposition launches per pass beyond the plan.
int run_unblind(afx_ctx* ctx, const UBatch& B, size_t first, size_t n) {
  CtxLock lock__(ctx);   // the context in turn
  if (n == 0) return AFX_OK;
  AFX_HIP(hipSetDevice(ctx->device));
  if (B.n != ctx->n) { set_error("internal: issuance layout of another context"); return AFX_E_BAD_ARGS; }
  const uint32_t na = B.n, h = B.h, rq = 3 + 3 * h + B.hs, j0 = rq + na, v_row = j0 + na + 11, d_row = v_row + 1;
  const bool drawn = B.seed40 != nullptr;
  const uint32_t rows = d_row + (drawn ? 1 : 0);
  // (a revealed value lands on the row of its position)
  const std::vector<uint32_t> map_q = blind_request_map(B.kinds, na, rq, 0, rq), map_j = identity_map(B.cells_j, j0);
  if (map_q.size() != B.cells_q) { set_error("internal: AFXQ cell map"); return AFX_E_BAD_ARGS; }
  const uint32_t map_o[3] = { j0, j0 + 1, v_row };
  const size_t total = B.count;
  return host_pipe(ctx, n, [&](Stager& st, size_t off, size_t sn) -> int {
    if (st.ses || st.app) { set_error("internal: a blind wire call inside a collected session"); return AFX_E_BAD_ARGS; }
    const size_t f0 = first + off;
    st.layout_tag = drawn ? 12 : 11;
    const size_t dn = st.dev_items(sn);
    const size_t o_j = st.add_rows(B.recj, 1, (size_t)B.cells_j * 32, total, f0, sn, dn), o_q = st.add_rows(B.recq, 1, (size_t)B.cells_q * 32, total, f0, sn, dn);
    const size_t o_mj = st.add((const uint8_t*)map_j.data(), 4 * map_j.size()), o_mq = st.add((const uint8_t*)map_q.data(), 4 * map_q.size()),
                 o_mo = st.add((const uint8_t*)map_o, sizeof map_o);
    size_t o_d = 0, o_dw = 0;
    if (drawn) o_dw = st.add_drawn(st.add_seed(B.seed40, dn), AFX_DRAW_BLINDREQ_D_WIDE, 1, B.draws, f0, sn, dn);
    else o_d = st.add_rows(B.d, 1, 32, total, f0, sn, dn);
    const size_t o_soa = st.reserve(dn * rows * 32);
    const size_t o_t = st.add_rows(nullptr, 1, 32, total, f0, sn, dn), o_U = st.add_rows(nullptr, 1, 32, total, f0, sn, dn),
                 o_V = st.add_rows(nullptr, 1, 32, total, f0, sn, dn), o_st = st.add(nullptr, dn);
    st.plan_fetch(B.t, o_t, 1, 32, total, f0, sn, dn);
    st.plan_fetch(B.U, o_U, 1, 32, total, f0, sn, dn);
    st.plan_fetch(B.V, o_V, 1, 32, total, f0, sn, dn);
    st.plan_fetch(B.status, o_st, 1, 1, total, f0, sn, dn);
    int rc = st.upload();
    if (rc) return rc;
    hipStream_t strm = st.stream();
    uint8_t* soa_d = st.dev(o_soa);
    auto rowp = [&](uint32_t r) { return soa_d + (size_t)r * dn * 32; };
    uint8_t* d_dev = drawn ? rowp(d_row) : st.dev(o_d);
    afx_attributes_soa da;
    memset(&da, 0, sizeof da);
    da.n_attributes = na; memcpy(da.kinds, B.kinds, AFX_MAX_ATTRIBUTES);
    da.values = rowp(rq);
    const afx_blind_request_soa dq = { rowp(0), rowp(1), rowp(1 + h), nullptr, nullptr };   // the user's own D, A, B
    const afx_blind_issuance_soa di = { rowp(j0), rowp(j0 + 1), rowp(j0 + 2), rowp(j0 + 3), rowp(j0 + 4), rowp(j0 + 5) };
    auto launch = [&]() -> int {
      AFX_HIP(afxk_aos_to_soa(strm, st.dev(o_j), soa_d, (const uint32_t*)st.dev(o_mj), B.cells_j, (uint32_t)dn));
      AFX_HIP(afxk_aos_to_soa(strm, st.dev(o_q), soa_d, (const uint32_t*)st.dev(o_mq), B.cells_q, (uint32_t)dn));
      if (drawn) AFX_HIP(afxk_reduce_wide(strm, st.dev(o_dw), d_dev, (uint32_t)dn));
      const int r = afx_unblind_issuances_dev(ctx, &da, d_dev, &dq, &di, na + 6, dn, rowp(v_row), st.dev(o_st));
      if (r) return r;
      const uint32_t* mo = (const uint32_t*)st.dev(o_mo);
      AFX_HIP(afxk_soa_to_aos(strm, soa_d, st.dev(o_t), mo, st.dev(o_st), 1, (uint32_t)dn));
      AFX_HIP(afxk_soa_to_aos(strm, soa_d, st.dev(o_U), mo + 1, st.dev(o_st), 1, (uint32_t)dn));
      AFX_HIP(afxk_soa_to_aos(strm, soa_d, st.dev(o_V), mo + 2, st.dev(o_st), 1, (uint32_t)dn));
      return AFX_OK;
    };
    rc = launch();
    if (drawn) rc = wipe_rows(strm, rc, { { st.dev(o_dw), dn * 64 }, { d_dev, dn * 32 } });
    return rc ? rc : st.fetch_all();
  }, PlanKey(), true);   // never collected
}

int unblind_wire(const Where& w, const uint8_t* iss, size_t iss_len, const uint8_t* req, size_t req_len, const uint8_t* d, const uint8_t* seed40,
                 const afx_credential_out* out, uint8_t* status, size_t status_cap, size_t* count_out) {
  int rc = check_where(w);
  if (rc) return rc;
  if (!out || !count_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  const uint32_t ctx_n = w.first()->n;
  UStream S;
  if ((rc = parse_pairs(iss, iss_len, req, req_len, ctx_n, S))) return rc;
  if (status_cap < S.total || (!status && S.total)) { set_error("status buffer too small"); return AFX_E_BAD_ARGS; }
  if (S.total && (!out->t || !out->U || !out->V || (!seed40 && !d))) { set_error("null batch array"); return AFX_E_BAD_ARGS; }
  *count_out = S.total;
  const afx_credential_out o = *out;
  for (const Pair& p : S.pairs)
    if (!on_gpu(p, ctx_n)) {   // answered on the host, as afx_unblind_issuances answers a layout or a response count that does not fit
      memset(status + p.first, AFX_ST_VERIFICATION_FAILURE, p.count);
      for (uint8_t* col : { o.t, o.U, o.V }) memset(col + p.first * 32, 0, p.count * 32);
    }
  std::vector<size_t> counts;
  for (UBatch& B : S.batches) {
    counts.push_back(B.count);
    const size_t qb = (size_t)B.cells_q * 32, jb = (size_t)B.cells_j * 32;
    B.seed40 = seed40;
    if (seed40) {
      size_t at = 0;
      for (size_t k : B.pairs) { B.draws.push_back({ at, S.pairs[k].count, (uint64_t)S.pairs[k].first }); at += S.pairs[k].count; }
    }
    if (B.pairs.size() == 1) {
      const Pair& p = S.pairs[B.pairs[0]];
      B.recq = req + p.q_rec; B.recj = iss + p.j_rec;
      B.d = seed40 ? nullptr : d + p.first * 32;
      B.t = o.t + p.first * 32; B.U = o.U + p.first * 32; B.V = o.V + p.first * 32; B.status = status + p.first;
      continue;
    }
    B.q_buf.resize(B.count * qb); B.j_buf.resize(B.count * jb);
    if (!seed40) B.d_buf.resize(B.count * 32);
    B.out_buf.assign(3 * B.count * 32, 0);
    B.st_buf.assign(B.count, AFX_ST_VERIFICATION_FAILURE);
    size_t at = 0;
    for (size_t k : B.pairs) {
      const Pair& p = S.pairs[k];
      memcpy(B.q_buf.data() + at * qb, req + p.q_rec, p.count * qb);
      memcpy(B.j_buf.data() + at * jb, iss + p.j_rec, p.count * jb);
      if (!seed40) memcpy(B.d_buf.data() + at * 32, d + p.first * 32, p.count * 32);
      at += p.count;
    }
    B.recq = B.q_buf.data(); B.recj = B.j_buf.data();
    B.d = seed40 ? nullptr : B.d_buf.data();
    B.t = B.out_buf.data(); B.U = B.t + B.count * 32; B.V = B.U + B.count * 32; B.status = B.st_buf.data();
  }
  rc = spread(w, S.total, counts, [&](afx_ctx* c, size_t b, size_t first, size_t n) { return run_unblind(c, S.batches[b], first, n); });
  for (UBatch& B : S.batches) {   // (after a failure too: the gathered d is wiped here)
    if (!B.d_buf.empty()) afx::afx_wipe(B.d_buf.data(), B.d_buf.size());
    if (B.pairs.size() == 1) continue;
    size_t at = 0;
    for (size_t k : B.pairs) {
      const Pair& p = S.pairs[k];
      memcpy(o.t + p.first * 32, B.t + at * 32, p.count * 32);
      memcpy(o.U + p.first * 32, B.U + at * 32, p.count * 32);
      memcpy(o.V + p.first * 32, B.V + at * 32, p.count * 32);
      memcpy(status + p.first, B.status + at, p.count);
      at += p.count;
    }
  }
  return rc;
}
int unblind_wire_rng(const Where& w, const uint8_t* iss, size_t iss_len, const uint8_t* req, size_t req_len, const afx_device_rng* rng, const afx_credential_out* out,
                     uint8_t* status, size_t status_cap, size_t* count_out) {
  if (!rng || !rng->seed) { set_error("unblinding needs the seed the requests were drawn from"); return AFX_E_BAD_ARGS; }
  DrawSeed seed;
  const int rc = seed.init(rng);
  if (rc) return rc;
  return unblind_wire(w, iss, iss_len, req, req_len, nullptr, seed.b, out, status, status_cap, count_out);
}

Where on_ctx(afx_ctx* c) { Where w; w.ctx = c; return w; }
Where on_group(afx_group* g) { Where w; w.group = g; return w; }

}  // namespace

extern "C" int afx_blind_request_wire(afx_ctx* ctx, const afx_blind_request_group* groups, size_t n_groups, uint8_t* out, size_t out_cap, size_t* out_len,
                                      uint8_t* status, size_t status_cap, size_t* count_out) try {
  return request_wire(on_ctx(ctx), groups, n_groups, nullptr, nullptr, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_group_blind_request_wire(afx_group* group, const afx_blind_request_group* groups, size_t n_groups, uint8_t* out, size_t out_cap, size_t* out_len,
                                            uint8_t* status, size_t status_cap, size_t* count_out) try {
  return request_wire(on_group(group), groups, n_groups, nullptr, nullptr, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_blind_request_wire_rng(afx_ctx* ctx, const afx_blind_request_group* groups, size_t n_groups, const afx_device_rng* rng, uint8_t* d_out, uint8_t* out,
                                          size_t out_cap, size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  return request_wire_rng(on_ctx(ctx), groups, n_groups, rng, d_out, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_group_blind_request_wire_rng(afx_group* group, const afx_blind_request_group* groups, size_t n_groups, const afx_device_rng* rng, uint8_t* d_out,
                                                uint8_t* out, size_t out_cap, size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  return request_wire_rng(on_group(group), groups, n_groups, rng, d_out, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_unblind_issuances_wire(afx_ctx* ctx, const uint8_t* issuances, size_t issuances_len, const uint8_t* requests, size_t requests_len, const uint8_t* d,
                                          const afx_credential_out* out, uint8_t* status, size_t status_cap, size_t* count_out) try {
  return unblind_wire(on_ctx(ctx), issuances, issuances_len, requests, requests_len, d, nullptr, out, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_group_unblind_issuances_wire(afx_group* group, const uint8_t* issuances, size_t issuances_len, const uint8_t* requests, size_t requests_len,
                                                const uint8_t* d, const afx_credential_out* out, uint8_t* status, size_t status_cap, size_t* count_out) try {
  return unblind_wire(on_group(group), issuances, issuances_len, requests, requests_len, d, nullptr, out, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_unblind_issuances_wire_rng(afx_ctx* ctx, const uint8_t* issuances, size_t issuances_len, const uint8_t* requests, size_t requests_len,
                                              const afx_device_rng* rng, const afx_credential_out* out, uint8_t* status, size_t status_cap, size_t* count_out) try {
  return unblind_wire_rng(on_ctx(ctx), issuances, issuances_len, requests, requests_len, rng, out, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_group_unblind_issuances_wire_rng(afx_group* group, const uint8_t* issuances, size_t issuances_len, const uint8_t* requests, size_t requests_len,
                                                    const afx_device_rng* rng, const afx_credential_out* out, uint8_t* status, size_t status_cap,
                                                    size_t* count_out) try {
  return unblind_wire_rng(on_group(group), issuances, issuances_len, requests, requests_len, rng, out, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }
