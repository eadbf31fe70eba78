// The request-stream layer of the two issuer doors (wire_issue.cpp: AFXR requests in, AFXI issuances out; wire_blind.cpp: AFXQ in, AFXJ
// out): a stream of request sections is split, the sections the GPU works on are merged by layout into batches, every section's
// answer gets its header, the batches run - on one context or split over a group's members - and what was gathered goes back to its
// sections.  The two doors differ in data only: a Door says what a format's sections look like, how large its records are, which
// randomness a request takes and which function runs a batch's items.  Only bytes move here; what is staged and launched is the
// doors' own (issue_records, run_records), and what a header looks like is wire_formats.hpp's.
#pragma once
#include <map>
#include "wire_formats.hpp"

namespace {   // (every source file its own copy, as before: nothing here is exported from the library)

// One request section of a stream and where its answer goes in `out`.
struct Section {
  size_t off, hdr, count, first;   // in the request stream: bytes, header bytes, items, index of its first item in the stream
  size_t out_off, out_hdr;         // in the response stream
  uint32_t n, nrq;                 // (nrq: the request's own response count; 0 where the format has none)
  uint8_t kinds[AFX_MAX_ATTRIBUTES];
};
// The items of one layout that go to the GPU, merged over the sections that carry it: where its records, randomness and results lie
// (the caller's arrays when ONE section carries it, else copies made here and scattered afterwards).
struct Batch {
  static constexpr uint32_t MAX_RND = 4;
  std::vector<size_t> secs;
  size_t count = 0;
  uint32_t n = 0, nrq = 0, h = 0, hs = 0, cells_in = 0;
  uint8_t kinds[AFX_MAX_ATTRIBUTES];
  const uint8_t* rec = nullptr;                                   // [count][cells_in][32]
  const uint8_t* rnd[MAX_RND] = { nullptr, nullptr, nullptr, nullptr };   // the door's randomness columns, [count][bytes per item] each
  uint8_t* out = nullptr;                                         // [count][cells of an output record][32] (null: the verification alone)
  uint8_t* status = nullptr;                                      // [count]
  std::vector<uint8_t> rec_buf, rnd_buf, out_buf, st_buf;
  // device-drawn randomness (the _rng forms): the call's staged seed || stream, and per section the batch items it holds and the
  // stream index of its first (the draws of a request depend on its index in the stream only)
  const uint8_t* seed40 = nullptr;
  std::vector<Stager::DrawPiece> draws;
};
struct Stream {
  std::vector<Section> secs;
  std::vector<Batch> batches;   // in order of first appearance
  size_t total = 0, out_len = 0;
};

// What tells one door from the other.
struct Door {
  const Format *in, *out;                                         // (wire_formats.hpp) AFXR in, AFXI out; or AFXQ in, AFXJ out
  uint32_t (*cells_in)(uint32_t n, uint32_t h, uint32_t hs);      // cells of a request record of a layout
  uint32_t (*cells_out)(uint32_t n, uint32_t ctx_n);              // cells of an answer record to a section of n attributes
  uint32_t (*n_responses)(uint32_t ctx_n);                        // of the answer's proof
  // the randomness of a request, one host array per column in stream order (null arrays: drawn on the device, or none needed)
  struct Column { const uint8_t* host; size_t bytes; } rnd[Batch::MAX_RND];
  uint32_t n_rnd;
  bool rnd_for_any_stream;      // a null host array is refused even where no section would read it
  uint8_t foreign_status;       // what a request of a layout the context does not issue gets (n != the context's n, or n == 0)
  bool issue;                   // false: the requests' verification alone - statuses only, neither randomness nor the key
  const char* needs_key;        // the error of an issuing call on a context without the issuer key
  bool collected;               // several batches: through run_batches (the collector, or a session of the request's own), or one after
                                // another, never collected
  int (*run)(afx_ctx* ctx, const Batch& B, size_t first, size_t n);   // items [first, first + n) of a batch on a context
};

// Splits the stream into sections (every one parsed in full: a malformed one anywhere fails the call before anything runs) and merges
// the sections the GPU works on - n == the context's n, n != 0 - by layout.
inline int parse_stream(const Door& d, const uint8_t* blob, size_t len, uint32_t ctx_n, Stream& S) {
  if (!blob && len) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  std::map<std::string, size_t> by_layout;
  for (size_t off = 0; off < len;) {
    Header H;
    const int rc = read_section(*d.in, blob + off, len - off, H);
    if (rc) { set_error("section at byte " + std::to_string(off) + ": " + afx_last_error()); return rc; }
    const size_t cnt = H.count;
    Section s;
    s.off = off; s.hdr = H.hdr; s.count = cnt; s.first = S.total;
    s.n = H.n; s.nrq = H.nr;
    memset(s.kinds, 0, sizeof s.kinds);
    memcpy(s.kinds, H.kinds, H.n);
    s.out_off = S.out_len;
    s.out_hdr = header_bytes(*d.out, s.n);
    const size_t out_bytes = s.out_hdr + cnt * d.cells_out(s.n, ctx_n) * 32;   // (< 2^32 * 2^7 * 2^5)
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
        B.n = s.n; B.nrq = s.nrq; B.h = hd.h; B.hs = hd.hs; B.cells_in = d.cells_in(s.n, hd.h, hd.hs);
        memcpy(B.kinds, s.kinds, AFX_MAX_ATTRIBUTES);
      }
      S.batches[it->second].secs.push_back(S.secs.size());
      S.batches[it->second].count += cnt;
    }
    S.secs.push_back(s);
    off += H.section;
  }
  return AFX_OK;
}

// What must hold before anything is written or launched (the size query has returned before this).
// seed40: the randomness is drawn on the device (the door's host arrays are not read)
inline int check_call(afx_ctx* ctx, const Door& d, const Stream& S, const uint8_t* seed40, size_t out_cap, const uint8_t* status, size_t status_cap) {
  if (d.issue && out_cap < S.out_len) { set_error("output buffer too small"); return AFX_E_BAD_ARGS; }
  if (status_cap < S.total || (!status && S.total)) { set_error("status buffer too small"); return AFX_E_BAD_ARGS; }
  if (d.issue && !seed40 && (d.rnd_for_any_stream || !S.batches.empty()))
    for (uint32_t c = 0; c < d.n_rnd; c++)
      if (!d.rnd[c].host) { set_error("null randomness array"); return AFX_E_BAD_ARGS; }
  for (const Batch& B : S.batches)
    if (B.count > 0xffffffffu / 64) { set_error("too many requests of one layout"); return AFX_E_BAD_ARGS; }
  if (d.issue && !ctx->has_key) { set_error(d.needs_key); return AFX_E_NO_KEY; }
  return AFX_OK;
}

// Every section's answer header; the sections the GPU does not see (n != the context's n, or n == 0: MacCreation, amacs.rs:285-287)
// get records of zeros and their statuses here.  Then every batch's arrays: the caller's own, or gathered copies.
inline void prepare(Stream& S, const Door& d, const uint8_t* blob, const uint8_t* seed40, uint32_t ctx_n, uint8_t* out, uint8_t* status) {
  const uint32_t nr = d.n_responses(ctx_n);
  for (const Section& s : S.secs) {
    const bool on_gpu = s.n == ctx_n && s.n != 0;
    if (d.issue) {
      const uint32_t out_cells = d.cells_out(s.n, ctx_n);
      uint8_t* h = out + s.out_off;
      write_header(*d.out, h, s.count, out_cells, s.n, nr, s.kinds);
      if (!on_gpu) memset(h + s.out_hdr, 0, s.count * out_cells * 32);
    }
    if (!on_gpu) memset(status + s.first, d.foreign_status, s.count);
  }
  const bool host_rnd = d.issue && !seed40;
  size_t rnd_bytes = 0;   // of one request, over the columns
  for (uint32_t c = 0; c < d.n_rnd; c++) rnd_bytes += d.rnd[c].bytes;
  for (Batch& B : S.batches) {
    const size_t rb = (size_t)B.cells_in * 32, ob = (size_t)d.cells_out(B.n, ctx_n) * 32;
    if (seed40) {   // (no rnd_buf: the draws land in the staged rows themselves)
      B.seed40 = seed40;
      size_t at = 0;
      for (size_t k : B.secs) { B.draws.push_back({ at, S.secs[k].count, (uint64_t)S.secs[k].first }); at += S.secs[k].count; }
    }
    if (B.secs.size() == 1) {
      const Section& s = S.secs[B.secs[0]];
      B.rec = blob + s.off + s.hdr;
      if (host_rnd)
        for (uint32_t c = 0; c < d.n_rnd; c++) B.rnd[c] = d.rnd[c].host + s.first * d.rnd[c].bytes;
      if (d.issue) B.out = out + s.out_off + s.out_hdr;
      B.status = status + s.first;
      continue;
    }
    B.rec_buf.resize(B.count * rb);
    if (d.issue) B.out_buf.assign(B.count * ob, 0);
    B.st_buf.assign(B.count, d.foreign_status);
    uint8_t* col[Batch::MAX_RND] = { nullptr, nullptr, nullptr, nullptr };   // (rnd_buf is empty without host randomness: no offsets from its null data())
    if (host_rnd) {
      B.rnd_buf.resize(B.count * rnd_bytes);
      uint8_t* p = B.rnd_buf.data();
      for (uint32_t c = 0; c < d.n_rnd; c++) { col[c] = p; p += B.count * d.rnd[c].bytes; }
    }
    size_t at = 0;
    for (size_t k : B.secs) {
      const Section& s = S.secs[k];
      memcpy(B.rec_buf.data() + at * rb, blob + s.off + s.hdr, s.count * rb);
      if (host_rnd)
        for (uint32_t c = 0; c < d.n_rnd; c++) memcpy(col[c] + at * d.rnd[c].bytes, d.rnd[c].host + s.first * d.rnd[c].bytes, s.count * d.rnd[c].bytes);
      at += s.count;
    }
    B.rec = B.rec_buf.data();
    for (uint32_t c = 0; c < d.n_rnd; c++) B.rnd[c] = col[c];
    if (d.issue) B.out = B.out_buf.data();
    B.status = B.st_buf.data();
  }
}
// results of the batches that were gathered go back to their sections; the gathered randomness is wiped
inline void scatter(Stream& S, const Door& d, uint32_t ctx_n, uint8_t* out, uint8_t* status) {
  for (Batch& B : S.batches) {
    if (!B.rnd_buf.empty()) afx::afx_wipe(B.rnd_buf.data(), B.rnd_buf.size());
    if (B.secs.size() == 1) continue;
    const size_t ob = (size_t)d.cells_out(B.n, ctx_n) * 32;
    size_t at = 0;
    for (size_t k : B.secs) {
      const Section& s = S.secs[k];
      if (d.issue) memcpy(out + s.out_off + s.out_hdr, B.out + at * ob, s.count * ob);
      memcpy(status + s.first, B.status + at, s.count);
      at += s.count;
    }
  }
}

// A parsed stream (parse_stream with this context's n) on one context.  seed40 == null: the door's host randomness; seed40: the _rng
// form's staged seed || stream.  A door that only verifies uses neither, nor out, out_cap and out_len.
inline int run_door(afx_ctx* ctx, const Door& d, Stream& S, const uint8_t* blob, const uint8_t* seed40, uint8_t* out, size_t out_cap, size_t* out_len,
                    uint8_t* status, size_t status_cap, size_t* count_out) {
  int rc = AFX_OK;
  if (d.issue) *out_len = S.out_len;
  *count_out = S.total;
  if (d.issue && !out) return AFX_OK;   // size query: headers only
  if ((rc = check_call(ctx, d, S, seed40, out_cap, status, status_cap))) return rc;
  prepare(S, d, blob, seed40, ctx->n, out, status);
  if (d.collected) {
    std::vector<size_t> counts;
    for (const Batch& B : S.batches) counts.push_back(B.count);
    rc = run_batches(ctx, counts, [&](size_t b) { return d.run(ctx, S.batches[b], 0, S.batches[b].count); }, "layout");
  } else {
    for (size_t b = 0; b < S.batches.size() && !rc; b++) {
      rc = d.run(ctx, S.batches[b], 0, S.batches[b].count);
      if (rc && S.batches.size() > 1) { const std::string why = afx_last_error(); set_error("layout " + std::to_string(b) + ": " + why); }
    }
  }
  scatter(S, d, ctx->n, out, status);   // (after a failure too: the gathered randomness is wiped there)
  return rc;
}
inline int door(afx_ctx* ctx, const Door& d, const uint8_t* blob, size_t len, const uint8_t* seed40, uint8_t* out, size_t out_cap, size_t* out_len,
                uint8_t* status, size_t status_cap, size_t* count_out) {
  if (!ctx || (d.issue && !out_len) || !count_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  Stream S;
  const int rc = parse_stream(d, blob, len, ctx->n, S);
  return rc ? rc : run_door(ctx, d, S, blob, seed40, out, out_cap, out_len, status, status_cap, count_out);
}

// The same stream over a group's devices.  A stream of at most afx_ctx_set_small_batch_items requests (member 0's) goes whole to ONE
// member, the next in turn; a larger one has every batch split over the members (afx_shard_bounds), one host thread per member, each
// writing its own record range of `out`.  The headers and the MacCreation sections are written once, here.
inline int group_door(afx_group* group, const Door& d, const uint8_t* blob, size_t len, const uint8_t* seed40, uint8_t* out, size_t out_cap, size_t* out_len,
                      uint8_t* status, size_t status_cap, size_t* count_out) {
  if (!group || !out_len || !count_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  const uint32_t m = afx_group_size(group);
  if (m == 0) { set_error("empty group"); return AFX_E_BAD_ARGS; }
  afx_ctx* c0 = afx_group_member(group, 0);
  const uint32_t small = afx_group_small_batch_items(group);
  Stream S;   // parsed once, for whichever path (the members share the parameters, so member 0's n is every member's)
  int rc = parse_stream(d, blob, len, c0->n, S);
  if (rc) return rc;
  if (m == 1 || (small && len && S.total <= small)) {
    return on_one_member(group, m, [&](afx_ctx* c) { return run_door(c, d, S, blob, seed40, out, out_cap, out_len, status, status_cap, count_out); });
  }
  *out_len = S.out_len;
  *count_out = S.total;
  if (!out) return AFX_OK;
  if ((rc = check_call(c0, d, S, seed40, out_cap, status, status_cap))) return rc;
  prepare(S, d, blob, seed40, c0->n, out, status);
  std::vector<size_t> counts;
  for (const Batch& B : S.batches) counts.push_back(B.count);
  rc = shard_over_members(group, m, counts, [&](afx_ctx* c, size_t b, size_t first, size_t n) { return d.run(c, S.batches[b], first, n); });
  scatter(S, d, c0->n, out, status);
  return rc;
}

}  // namespace
