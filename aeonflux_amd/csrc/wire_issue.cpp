// Issuer::issue over serialized requests (include/aeonflux_gpu.h "AFXR" v1, afx_issue_wire): request bytes in, AFXI response bytes
// out.  /root/reference/src/issuer.rs:111-124 takes one CredentialRequest; the crate serialises none (src/user.rs:137-139), so AFXR is
// the engine's own, in the style of AFXP / AFXI.  The request records are transposed to struct-of-arrays on the GPU (k_aos_to_soa),
// afx_issue_dev writes its outputs into the rows in front of the attribute values, and k_soa_to_aos turns the whole region back into
// AFXI records - zeros for an item that failed - which come back in one fetch.  Only bytes move on the host.
#include <atomic>
#include <map>
#include <memory>
#include <string>
#include <system_error>
#include <thread>
#include <vector>
#include "kernels.h"
#include "statements.hpp"

namespace {

uint32_t rd32(const uint8_t* b) { return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24); }
void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// One AFXR section of a request stream and where its AFXI answer goes in `out`.
struct Section {
  size_t off, hdr, count, first;   // in the request stream: bytes, header bytes, items, index of its first item in the stream
  size_t out_off, out_hdr;         // in the response stream
  uint32_t n;
  uint8_t kinds[AFX_MAX_ATTRIBUTES];
};
// The items of one attribute layout that go to the GPU, merged over the sections that carry it: where its records, randomness and
// results lie (the caller's arrays when ONE section carries it, else copies made here and scattered afterwards).
struct Batch {
  std::vector<size_t> secs;
  size_t count = 0;
  uint32_t n = 0;
  uint8_t kinds[AFX_MAX_ATTRIBUTES];
  const uint8_t* rec = nullptr;                                   // [count][n][32]
  const uint8_t *t_wide = nullptr, *U_wide = nullptr, *seed = nullptr;
  uint8_t* out = nullptr;                                         // [count][4 + nr + n][32]
  uint8_t* status = nullptr;                                      // [count]
  std::vector<uint8_t> rec_buf, rnd_buf, out_buf, st_buf;
  // device-drawn randomness (afx_issue_wire_rng): the call's staged seed || stream, and per section the batch items it holds and the
  // stream index of its first (the draws of a request depend on its index in the stream only)
  const uint8_t* seed40 = nullptr;
  std::vector<Stager::DrawPiece> draws;
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
  const size_t nr = (size_t)ctx_n + 5;
  std::map<std::string, size_t> by_layout;
  for (size_t off = 0; off < len;) {
    size_t sl = 0, cnt = 0, rec = 0;
    Section s;
    int rc = afx_request_wire_section_bytes(blob + off, len - off, &sl);
    if (!rc) rc = afx_request_wire_parse(blob + off, sl, &s.n, s.kinds, &cnt, &rec);
    if (rc) { set_error("section at byte " + std::to_string(off) + ": " + afx_last_error()); return rc; }
    s.off = off; s.hdr = rec; s.count = cnt; s.first = S.total;
    s.out_off = S.out_len;
    s.out_hdr = afx_issuance_wire_header_bytes(s.n);
    const size_t out_bytes = s.out_hdr + cnt * (4 + nr + s.n) * 32;   // (< 2^32 * 2^7 * 2^5)
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
        S.batches.back().n = s.n;
        memcpy(S.batches.back().kinds, s.kinds, AFX_MAX_ATTRIBUTES);
      }
      S.batches[it->second].secs.push_back(S.secs.size());
      S.batches[it->second].count += cnt;
    }
    S.secs.push_back(s);
    off += sl;
  }
  return AFX_OK;
}

// What must hold before anything is written or launched (the size query has returned before this).
// seed40: the randomness is drawn on the device (rnd is not read)
int check_call(afx_ctx* ctx, const Stream& S, const afx_issue_randomness* rnd, const uint8_t* seed40, size_t out_cap, const uint8_t* status,
               size_t status_cap) {
  if (out_cap < S.out_len) { set_error("output buffer too small"); return AFX_E_BAD_ARGS; }
  if (status_cap < S.total || (!status && S.total)) { set_error("status buffer too small"); return AFX_E_BAD_ARGS; }
  if (!S.batches.empty() && !seed40 && (!rnd || !rnd->t_wide || !rnd->U_wide || !rnd->rng_seed)) { set_error("null randomness array"); return AFX_E_BAD_ARGS; }
  for (const Batch& B : S.batches)
    if (B.count > 0xffffffffu / 64) { set_error("too many requests of one layout"); return AFX_E_BAD_ARGS; }
  if (!ctx->has_key) { set_error("Issuer::issue needs the issuer key"); return AFX_E_NO_KEY; }
  return AFX_OK;
}

// Every section's AFXI header; the sections the GPU does not see (n != the context's n, or n == 0: MacCreation, amacs.rs:285-287)
// get records of zeros and their statuses here.  Then every batch's arrays: the caller's own, or gathered copies.
void prepare(Stream& S, const uint8_t* blob, const afx_issue_randomness* rnd, const uint8_t* seed40, uint32_t ctx_n, uint8_t* out, uint8_t* status) {
  const uint32_t nr = ctx_n + 5;
  for (const Section& s : S.secs) {
    uint8_t* h = out + s.out_off;
    memset(h, 0, s.out_hdr);
    memcpy(h, "AFXI", 4);
    wr32(h + 4, 1); wr32(h + 8, (uint32_t)s.count); wr32(h + 12, 4 + nr + s.n); wr32(h + 16, s.n); wr32(h + 20, nr);
    memcpy(h + 24, s.kinds, s.n);
    if (!(s.n == ctx_n && s.n != 0)) {
      memset(h + s.out_hdr, 0, s.count * (4 + nr + s.n) * 32);
      memset(status + s.first, AFX_ST_MAC_CREATION, s.count);
    }
  }
  for (Batch& B : S.batches) {
    const size_t rb = (size_t)B.n * 32, ob = (size_t)(4 + nr + B.n) * 32;
    if (seed40) {   // (no rnd_buf: the draws land in the staged rows themselves)
      B.seed40 = seed40;
      size_t at = 0;
      for (size_t k : B.secs) { B.draws.push_back({ at, S.secs[k].count, (uint64_t)S.secs[k].first }); at += S.secs[k].count; }
    }
    if (B.secs.size() == 1) {
      const Section& s = S.secs[B.secs[0]];
      B.rec = blob + s.off + s.hdr;
      if (!seed40) { B.t_wide = rnd->t_wide + s.first * 64; B.U_wide = rnd->U_wide + s.first * 64; B.seed = rnd->rng_seed + s.first * 32; }
      B.out = out + s.out_off + s.out_hdr;
      B.status = status + s.first;
      continue;
    }
    B.rec_buf.resize(B.count * rb);
    if (!seed40) B.rnd_buf.resize(B.count * 160);
    B.out_buf.assign(B.count * ob, 0);
    B.st_buf.assign(B.count, AFX_ST_MAC_CREATION);
    uint8_t *tw = B.rnd_buf.data(), *uw = tw + B.count * 64, *sd = uw + B.count * 64;
    size_t at = 0;
    for (size_t k : B.secs) {
      const Section& s = S.secs[k];
      memcpy(B.rec_buf.data() + at * rb, blob + s.off + s.hdr, s.count * rb);
      if (!seed40) {
        memcpy(tw + at * 64, rnd->t_wide + s.first * 64, s.count * 64);
        memcpy(uw + at * 64, rnd->U_wide + s.first * 64, s.count * 64);
        memcpy(sd + at * 32, rnd->rng_seed + s.first * 32, s.count * 32);
      }
      at += s.count;
    }
    B.rec = B.rec_buf.data();
    if (!seed40) { B.t_wide = tw; B.U_wide = uw; B.seed = sd; }
    B.out = B.out_buf.data(); B.status = B.st_buf.data();
  }
}
// results of the batches that were gathered go back to their sections
void scatter(const Stream& S, uint32_t ctx_n, uint8_t* out, uint8_t* status) {
  const uint32_t nr = ctx_n + 5;
  for (const Batch& B : S.batches) {
    if (B.secs.size() == 1) continue;
    const size_t ob = (size_t)(4 + nr + B.n) * 32;
    size_t at = 0;
    for (size_t k : B.secs) {
      const Section& s = S.secs[k];
      memcpy(out + s.out_off + s.out_hdr, B.out + at * ob, s.count * ob);
      memcpy(status + s.first, B.status + at, s.count);
      at += s.count;
    }
  }
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
  std::vector<uint32_t> map_in(na), map_out(cells);
  for (uint32_t c = 0; c < na; c++) map_in[c] = 4 + nr + c;   // a request record holds the values only
  for (uint32_t c = 0; c < cells; c++) map_out[c] = c;         // an AFXI record is the region's rows in order
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
      o_tw = st.add_rows(B.t_wide, 1, 64, total, f0, sn, dn);
      o_uw = st.add_rows(B.U_wide, 1, 64, total, f0, sn, dn);
      o_seed = st.add_rows(B.seed, 1, 32, total, f0, sn, dn);
    }
    const size_t o_soa = st.reserve(dn * cells * 32), o_out = st.add_rows(nullptr, 1, (size_t)cells * 32, total, f0, sn, dn), o_st = st.add(nullptr, dn);
    st.plan_fetch(B.out, o_out, 1, (size_t)cells * 32, total, f0, sn, dn);
    st.plan_fetch(B.status, o_st, 1, 1, total, f0, sn, dn);
    int rc = st.upload();
    if (rc) return rc;
    // (a call that took item slots of an earlier call's pass: that call's two transpositions cover them)
    hipStream_t strm = st.stream();
    uint8_t* soa_d = st.dev(o_soa);
    const uint32_t dn_ = (uint32_t)dn;
    if (!st.app) {
      const uint8_t* rec_d = st.dev(o_rec);
      const uint32_t* map_d = (const uint32_t*)st.dev(o_min);
      auto transpose = [=]() -> int { AFX_HIP(afxk_aos_to_soa(strm, rec_d, soa_d, map_d, na, dn_)); return AFX_OK; };
      if (st.ses) st.ses->pre.push_back(transpose);
      else if ((rc = transpose())) return rc;
    }
    auto rowp = [&](uint32_t r) { return soa_d + (size_t)r * dn * 32; };
    afx_attributes_soa da;
    memset(&da, 0, sizeof da);
    da.n_attributes = na; memcpy(da.kinds, B.kinds, AFX_MAX_ATTRIBUTES);
    da.values = rowp(4 + nr);
    const afx_issue_randomness dr = { st.dev(o_tw), st.dev(o_uw), st.dev(o_seed) };
    const afx_issuance_soa dout = { rowp(0), rowp(1), rowp(2), rowp(3), rowp(4) };
    if ((rc = afx_issue_dev(ctx, &da, &dr, dn, &dout, st.dev(o_st)))) return rc;
    if (!st.app) {
      uint8_t* out_d = st.dev(o_out);
      const uint32_t* map_d = (const uint32_t*)st.dev(o_mout);
      const uint8_t* st_d = st.dev(o_st);
      auto transpose = [=]() -> int { AFX_HIP(afxk_soa_to_aos(strm, soa_d, out_d, map_d, st_d, cells, dn_)); return AFX_OK; };
      if (st.ses) st.ses->post.push_back(transpose);
      else if ((rc = transpose())) return rc;
    }
    return st.fetch_all();
  }, jkey);
}

// does a request of several batches on this context leave its small batches with the collector's sessions (plans.cpp; as mixed.cpp)?
bool joins_the_collector(afx_ctx* ctx) {
  CtxLock probe(ctx, true);
  return ctx->lock_depth == 1 && ctx->co.enabled && ctx->co.max_items && ctx->small_batch_items && !ctx->trace && !ctx->pipelining && !ctx->session;
}

// Every batch of the stream on one context, as afx_issue_mixed runs its groups (mixed.cpp run_groups): with the collector on, the small
// batches join the collecting session; otherwise they are assembled into ONE set of launches of the request's own; a large batch runs
// by itself, in between.
int run_batches(afx_ctx* ctx, Stream& S) {
  if (S.batches.empty()) return AFX_OK;
  if (S.batches.size() == 1) return issue_records(ctx, S.batches[0], 0, S.batches[0].count);
  int rc = AFX_OK;
  afx::Deferred deferred;
  std::unique_ptr<afx::DeferScope> defer;
  std::unique_ptr<CtxLock> lock;
  std::unique_ptr<afx::Session> ses;
  const bool join = joins_the_collector(ctx);
  if (join) defer.reset(new afx::DeferScope(&deferred));
  else lock.reset(new CtxLock(ctx));   // the session owns the context until its last flush
  if (lock && ctx->small_batch_items && !ctx->trace && !ctx->session) {
    ses.reset(new afx::Session(ctx));
    if ((rc = ses->ensure_images(0, 0))) return rc;
    uint64_t width = 0;   // as in mixed.cpp run_groups
    for (const Batch& B : S.batches)
      if (B.count <= ctx->small_batch_items) width += (B.count + 63) / 64;
    ctx->merge_class = afx_ctx::merge_class_of(width);
  }
  struct WidthReset { afx_ctx* c; ~WidthReset() { if (c) c->merge_class = 0; } } width_reset = { ses ? ctx : nullptr };
  try {   // (an exception must not pass the drain below: other threads' calls may sit in a session only this thread launches)
    for (size_t b = 0; b < S.batches.size() && !rc; b++) {
      const Batch& B = S.batches[b];
      const bool collect = ses && B.count <= ctx->small_batch_items;
      if (ses && !collect) {
        if ((rc = ses->flush())) break;
        ses->paused = true;
      }
      rc = issue_records(ctx, B, 0, B.count);
      if (ses) ses->paused = false;
      if (rc) set_error("layout " + std::to_string(b) + ": " + afx_last_error());
    }
  } catch (...) {
    if (!join) throw;
    rc = afx::exception_rc();
  }
  if (ses) {
    if (rc) ses->drop();
    else rc = ses->flush();
    ses.reset();
  }
  if (join) {
    CtxLock lk(ctx, true);
    const int rc2 = afx::drain_deferred(ctx, deferred);   // (also after a failure: the staged rows point into this request's buffers)
    if (!rc) rc = rc2;
    defer.reset();
  }
  return rc;
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

}  // namespace

extern "C" size_t afx_request_wire_header_bytes(uint32_t n_attributes) {
  if (n_attributes > AFX_MAX_ATTRIBUTES) return 0;
  return (20 + (size_t)n_attributes + 31) & ~size_t(31);
}

extern "C" int afx_request_wire_parse(const uint8_t* blob, size_t len, uint32_t* n_out, uint8_t kinds_out[AFX_MAX_ATTRIBUTES], size_t* count_out,
                                      size_t* records_offset_out) try {
  if (!blob || !n_out || !kinds_out || !count_out || !records_offset_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (len < 20 || memcmp(blob, "AFXR", 4) != 0 || rd32(blob + 4) != 1) { set_error("not an AFXR v1 batch"); return AFX_E_BAD_ARGS; }
  const uint32_t count = rd32(blob + 8), cells = rd32(blob + 12), n = rd32(blob + 16);
  if (n > AFX_MAX_ATTRIBUTES) { set_error("n_attributes out of range"); return AFX_E_BAD_ARGS; }
  const size_t hdr = afx_request_wire_header_bytes(n);
  if (len < hdr) { set_error("truncated header"); return AFX_E_BAD_ARGS; }
  for (uint32_t i = 0; i < n; i++)
    if (blob[20 + i] > AFX_ATTR_SECRET_POINT) { set_error("attribute kind out of range"); return AFX_E_BAD_ARGS; }
  if (cells != n) { set_error("cells_per_record does not match the layout"); return AFX_E_BAD_ARGS; }
  if (len - hdr != (size_t)count * n * 32) { set_error("record area length"); return AFX_E_BAD_ARGS; }   // (count * n * 32 < 2^42)
  memset(kinds_out, 0, AFX_MAX_ATTRIBUTES);
  memcpy(kinds_out, blob + 20, n);
  *n_out = n; *count_out = count; *records_offset_out = hdr;
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_request_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out) try {
  if (!blob || !section_len_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (len < 20 || memcmp(blob, "AFXR", 4) != 0 || rd32(blob + 4) != 1) { set_error("not an AFXR v1 section"); return AFX_E_BAD_ARGS; }
  const uint64_t count = rd32(blob + 8), cells = rd32(blob + 12);
  const uint32_t n = rd32(blob + 16);
  if (n > AFX_MAX_ATTRIBUTES || cells != n) { set_error("layout field out of range"); return AFX_E_BAD_ARGS; }
  const uint64_t total = (uint64_t)afx_request_wire_header_bytes(n) + count * cells * 32;   // (< 2^42)
  if (total > len) { set_error("section runs past the end of the blob"); return AFX_E_BAD_ARGS; }
  *section_len_out = (size_t)total;
  return AFX_OK;
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
  memset(blob, 0, hdr);
  memcpy(blob, "AFXR", 4);
  wr32(blob + 4, 1); wr32(blob + 8, (uint32_t)count); wr32(blob + 12, n); wr32(blob + 16, n);
  memcpy(blob + 20, requests->kinds, n);
  uint8_t* rec = blob + hdr;
  for (size_t i = 0; i < count; i++)
    for (uint32_t c = 0; c < n; c++, rec += 32) memcpy(rec, requests->values + ((size_t)c * count + i) * 32, 32);
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }

namespace {
// afx_issue_wire (seed40 == null) and afx_issue_wire_rng (seed40: the staged seed || stream; rnd is not read)
int issue_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_issue_randomness* rnd, const uint8_t* seed40, uint8_t* out, size_t out_cap,
               size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) {
  if (!ctx || !out_len || !count_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  Stream S;
  int rc = parse_stream(blob, len, ctx->n, S);
  if (rc) return rc;
  *out_len = S.out_len;
  *count_out = S.total;
  if (!out) return AFX_OK;   // size query: headers only
  if ((rc = check_call(ctx, S, rnd, seed40, out_cap, status, status_cap))) return rc;
  prepare(S, blob, rnd, seed40, ctx->n, out, status);
  if ((rc = run_batches(ctx, S))) return rc;
  scatter(S, ctx->n, out, status);
  return AFX_OK;
}
int group_issue_wire(afx_group* group, const uint8_t* blob, size_t len, const afx_issue_randomness* rnd, const uint8_t* seed40, uint8_t* out,
                     size_t out_cap, size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out);
}  // namespace

extern "C" int afx_issue_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_issue_randomness* rnd, uint8_t* out, size_t out_cap, size_t* out_len,
                              uint8_t* status, size_t status_cap, size_t* count_out) try {
  return issue_wire(ctx, blob, len, rnd, nullptr, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_issue_wire_rng(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_device_rng* rng, uint8_t* out, size_t out_cap,
                                  size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  if (!rng) { set_error("null device rng"); return AFX_E_BAD_ARGS; }
  DrawSeed seed;
  int rc = out ? seed.init(rng) : AFX_OK;   // (the size query draws nothing)
  if (rc) return rc;
  return issue_wire(ctx, blob, len, nullptr, seed.b, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_group_issue_wire_rng(afx_group* group, const uint8_t* blob, size_t len, const afx_device_rng* rng, uint8_t* out, size_t out_cap,
                                        size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  if (!rng) { set_error("null device rng"); return AFX_E_BAD_ARGS; }
  DrawSeed seed;   // one seed for the whole group call: every member indexes by the request's ordinal in the stream
  int rc = out ? seed.init(rng) : AFX_OK;
  if (rc) return rc;
  return group_issue_wire(group, blob, len, nullptr, seed.b, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

// The same stream over a group's devices.  A stream of at most afx_ctx_set_small_batch_items requests (member 0's) goes whole to ONE
// member, the next in turn; a larger one has every batch split over the members (afx_shard_bounds), one host thread per member, each
// writing its own record range of `out`.  The headers and the MacCreation sections are written once, here.
extern "C" int afx_group_issue_wire(afx_group* group, const uint8_t* blob, size_t len, const afx_issue_randomness* rnd, uint8_t* out, size_t out_cap,
                                    size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) try {
  return group_issue_wire(group, blob, len, rnd, nullptr, out, out_cap, out_len, status, status_cap, count_out);
} catch (...) { return afx::exception_rc(); }

namespace {
int group_issue_wire(afx_group* group, const uint8_t* blob, size_t len, const afx_issue_randomness* rnd, const uint8_t* seed40, uint8_t* out,
                     size_t out_cap, size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out) {
  if (!group || !out_len || !count_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  const uint32_t m = afx_group_size(group);
  if (m == 0) { set_error("empty group"); return AFX_E_BAD_ARGS; }
  afx_ctx* c0 = afx_group_member(group, 0);
  const uint32_t small = afx_group_small_batch_items(group);
  if (m == 1 || (small && len && [&] { Stream T; return !parse_stream(blob, len, c0->n, T) && T.total <= small; }())) {
    const uint32_t k = m == 1 ? 0 : members_alike(group, m) ? g_next_small.fetch_add(1, std::memory_order_relaxed) % m : 0;
    GroupPin pin(group, k, true);
    const int rc = issue_wire(afx_group_member(group, k), blob, len, rnd, seed40, out, out_cap, out_len, status, status_cap, count_out);
    if (rc && m > 1) { const std::string why = afx_last_error(); set_error("member " + std::to_string(k) + ": " + why); }
    return rc;
  }
  Stream S;
  int rc = parse_stream(blob, len, c0->n, S);
  if (rc) return rc;
  *out_len = S.out_len;
  *count_out = S.total;
  if (!out) return AFX_OK;
  if ((rc = check_call(c0, S, rnd, seed40, out_cap, status, status_cap))) return rc;
  prepare(S, blob, rnd, seed40, c0->n, out, status);
  std::vector<int> rcs(m, AFX_OK);
  std::vector<std::string> errs(m);
  auto body = [&](uint32_t k) {
    GroupPin pin(group, k, k == 0);   // the member's thread on its device's NUMA node (member 0: the caller's thread, restored)
    afx_ctx* c = afx_group_member(group, k);
    for (const Batch& B : S.batches) {
      size_t first = 0, n = 0;
      afx_shard_bounds(B.count, m, k, &first, &n);
      if (n && (rcs[k] = issue_records(c, B, first, n))) { errs[k] = afx_last_error(); return; }   // (the error string is per thread)
    }
  };
  std::vector<std::thread> threads;
  for (uint32_t k = 1; k < m; k++) {
    try { threads.emplace_back(body, k); } catch (const std::system_error&) { body(k); }
  }
  body(0);
  for (std::thread& t : threads) t.join();
  for (uint32_t k = 0; k < m; k++)
    if (rcs[k]) { set_error("member " + std::to_string(k) + ": " + errs[k]); return rcs[k]; }
  scatter(S, c0->n, out, status);
  return AFX_OK;
}
}  // namespace

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
