// TEST INFRASTRUCTURE (CPU only): the doors of blind issuance on bytes (aeonflux_amd/csrc/wire_blind.cpp) on the engine's host half.
// tests/test_hostsim_blind_wire.py links this file with the engine's host sources, statements_blind.cpp, wire_blind.cpp, the fake HIP
// runtime and the stand-ins for the masking, record-writing and draw launchers under AddressSanitizer + UBSan and runs it with
// AFX_PLAN_SELFCHECK=1.
//   blind_wire_doors <dir>
// <dir> holds params.bin, key.bin and ip.bin of an issuer of 4 attributes, written by the test.  The requests are all zeros, so every
// item fails: what is checked is sizes, headers, what an argument error leaves untouched, zero records, and where the _rng form's seed
// goes.  Prints "blind wire doors ok" and exits 0, or says which check failed and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <utility>
#include <vector>
#include "../../include/aeonflux_gpu.h"

extern "C" void fake_draw_expect(const uint8_t* seed40);
extern "C" uint64_t fake_draw_jobs(int with_seed);
extern "C" uint64_t fake_draw_seed_left(void);
extern "C" uint64_t fake_draw_ranges_gone(void);

typedef std::vector<uint8_t> Bytes;
typedef std::vector<uint8_t> Kinds;

#define CHECK(cond)                                                                                       \
  do {                                                                                                    \
    if (!(cond)) {                                                                                        \
      fprintf(stderr, "%s:%d: check failed: %s (last error: %s)\n", __FILE__, __LINE__, #cond, afx_last_error()); \
      exit(1);                                                                                            \
    }                                                                                                     \
  } while (0)

static Bytes rd(const std::string& p) {
  FILE* f = fopen(p.c_str(), "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", p.c_str()); exit(2); }
  Bytes v;
  uint8_t buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}
static void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
static bool all_are(const Bytes& b, uint8_t v) {
  for (uint8_t x : b)
    if (x != v) return false;
  return true;
}

// one AFXQ section of `count` all-zero requests, from the library's own packer
static Bytes section(const Kinds& kinds, size_t count) {
  uint32_t h = 0, hs = 0;
  for (uint8_t k : kinds) { h += k == AFX_ATTR_SECRET_SCALAR || k == AFX_ATTR_SECRET_POINT; hs += k == AFX_ATTR_SECRET_SCALAR; }
  const size_t rows = kinds.size() > 1 + h + hs ? kinds.size() : 1 + h + hs;
  Bytes zeros(rows * count * 32 + 1, 0);
  afx_attributes_soa a;
  memset(&a, 0, sizeof a);
  a.n_attributes = (uint32_t)kinds.size();
  memcpy(a.kinds, kinds.data(), kinds.size());
  a.values = zeros.data();
  afx_blind_request_soa q = { zeros.data(), zeros.data(), zeros.data(), zeros.data(), zeros.data() };
  size_t len = 0;
  CHECK(afx_blind_request_wire_pack(&a, &q, count, nullptr, 0, &len) == AFX_OK);
  CHECK(len == 32 + count * (3 + 2 * h + hs + kinds.size()) * 32);
  Bytes blob(len);
  CHECK(afx_blind_request_wire_pack(&a, &q, count, blob.data(), blob.size(), &len) == AFX_OK && len == blob.size());
  return blob;
}

static const uint32_t N = 4;
static const size_t OUT_REC = (N + 11) * 32;
typedef std::vector<std::pair<Kinds, size_t>> Parts;

// well-formed AFXJ headers echoing the request sections, zero records, a failing status per request
static void check_answer(const char* what, const Parts& parts, const Bytes& out, const Bytes& status, size_t out_len, size_t cnt, size_t want_len, size_t total) {
  if (out_len != want_len || cnt != total) { fprintf(stderr, "%s: out_len %zu count %zu\n", what, out_len, cnt); exit(1); }
  size_t off = 0, first = 0;
  for (const auto& part : parts) {
    const Kinds& kinds = part.first;
    const size_t c = part.second, size = 32 + c * OUT_REC;
    uint8_t want[32];
    memset(want, 0, sizeof want);
    memcpy(want, "AFXJ", 4);
    wr32(want + 4, 1); wr32(want + 8, (uint32_t)c); wr32(want + 12, N + 11); wr32(want + 16, (uint32_t)kinds.size()); wr32(want + 20, N + 6);
    memcpy(want + 24, kinds.data(), kinds.size());
    bool ok = memcmp(&out[off], want, 32) == 0;
    size_t sl = 0;
    ok = ok && afx_blind_issuance_wire_section_bytes(&out[off], out.size() - off, &sl) == AFX_OK && sl == size;
    for (size_t k = 32; ok && k < size; k++) ok = out[off + k] == 0;   // nothing is released for a request that was not accepted
    for (size_t i = 0; ok && i < c; i++) ok = status[first + i] != 0 && (kinds.size() == N || status[first + i] == AFX_ST_MAC_CREATION);
    if (!ok) { fprintf(stderr, "%s: the answer to the section at item %zu (last error: %s)\n", what, first, afx_last_error()); exit(1); }
    off += size;
    first += c;
  }
  CHECK(off == want_len);
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: blind_wire_doors <dir>\n"); return 2; }
  const std::string dir = argv[1];
  const Bytes params = rd(dir + "/params.bin"), key = rd(dir + "/key.bin"), ip = rd(dir + "/ip.bin");
  CHECK(ip.size() == 64);
  afx_ctx *issuer = nullptr, *user = nullptr;
  CHECK(afx_ctx_create(&issuer, 0, params.data(), params.size(), key.data(), key.size(), ip.data()) == AFX_OK);
  CHECK(afx_ctx_create(&user, 0, params.data(), params.size(), nullptr, 0, ip.data()) == AFX_OK);
  CHECK(afx_ctx_n_attributes(issuer) == N);

  const Kinds A = { 4, 2, 3, 1 }, B = { 0, 1, 4, 2 }, W = { 0, 2 };
  const Parts parts = { { A, 3 }, { B, 2 }, { W, 2 }, { A, 2 } };   // two layouts of the context's n (the first in two sections) and one of another n
  Bytes stream;
  size_t total = 0, want_len = 0;
  for (const auto& p : parts) {
    const Bytes s = section(p.first, p.second);
    stream.insert(stream.end(), s.begin(), s.end());
    total += p.second;
    want_len += 32 + p.second * OUT_REC;
  }
  const Bytes last = section(A, 2);

  // ---- the size query: lengths from the headers and the context's n, no randomness, nothing staged (and no key needed) ----
  size_t out_len = 0, cnt = 0;
  for (afx_ctx* c : { issuer, user }) {
    out_len = cnt = 0;
    CHECK(afx_issue_blind_wire(c, stream.data(), stream.size(), nullptr, nullptr, 0, &out_len, nullptr, 0, &cnt) == AFX_OK);
    CHECK(out_len == want_len && cnt == total);
  }
  {
    const afx_device_rng q = { nullptr, 3 };
    out_len = cnt = 0;
    CHECK(afx_issue_blind_wire_rng(issuer, stream.data(), stream.size(), &q, nullptr, 0, &out_len, nullptr, 0, &cnt) == AFX_OK);
    CHECK(out_len == want_len && cnt == total);
    out_len = cnt = 7;
    CHECK(afx_issue_blind_wire(issuer, stream.data(), 0, nullptr, nullptr, 0, &out_len, nullptr, 0, &cnt) == AFX_OK && out_len == 0 && cnt == 0);
  }

  // ---- argument errors: the code, and not a byte of out or status written ----
  Bytes tw(total * 64, 0), uw(total * 64, 0), rw(total * 64, 0), sd(total * 32, 0);
  const afx_blind_issue_randomness rnd = { tw.data(), uw.data(), rw.data(), sd.data() };
  Bytes out(want_len, 0xEE), status(total, 0xEE);
  uint8_t seed40[40];
  for (int k = 0; k < 32; k++) seed40[k] = (uint8_t)(101 + k);
  const uint64_t stream_no = 9;
  for (int k = 0; k < 8; k++) seed40[32 + k] = (uint8_t)(stream_no >> (8 * k));
  const afx_device_rng rng = { seed40, stream_no };

  struct Args {
    afx_ctx* ctx; const Bytes* blob; size_t len; bool null_r; const afx_blind_issue_randomness* r; size_t cap, scap; bool null_status;
  };
  const Args good = { issuer, &stream, stream.size(), false, &rnd, want_len, total, false };
  auto call = [&](bool drawn, const Args& a) {
    uint8_t* st = a.null_status ? nullptr : status.data();
    if (drawn) return afx_issue_blind_wire_rng(a.ctx, a.blob->data(), a.len, a.null_r ? nullptr : &rng, out.data(), a.cap, &out_len, st, a.scap, &cnt);
    return afx_issue_blind_wire(a.ctx, a.blob->data(), a.len, a.null_r ? nullptr : a.r, out.data(), a.cap, &out_len, st, a.scap, &cnt);
  };
  Bytes truncated(stream.begin(), stream.end() - 1), trailing = stream, bad_kind = stream;
  trailing.insert(trailing.end(), { 'A', 'F', 'X', 'Q' });
  bad_kind[stream.size() - last.size() + 24] = 7;
  for (int drawn = 0; drawn < 2; drawn++) {
    std::vector<std::pair<Args, int>> table;
    auto add = [&](Args a, int want) { table.push_back({ a, want }); };
    { Args a = good; a.cap = want_len - 1; add(a, AFX_E_BAD_ARGS); }
    { Args a = good; a.scap = total - 1; add(a, AFX_E_BAD_ARGS); }
    { Args a = good; a.null_status = true; add(a, AFX_E_BAD_ARGS); }
    { Args a = good; a.null_r = true; add(a, AFX_E_BAD_ARGS); }
    { Args a = good; a.ctx = nullptr; add(a, AFX_E_BAD_ARGS); }
    { Args a = good; a.ctx = user; add(a, AFX_E_NO_KEY); }
    { Args a = good; a.blob = &truncated; a.len = truncated.size(); add(a, AFX_E_BAD_ARGS); }   // a malformed LAST section: nothing of the sections before it is answered
    { Args a = good; a.blob = &trailing; a.len = trailing.size(); add(a, AFX_E_BAD_ARGS); }
    { Args a = good; a.blob = &bad_kind; a.len = bad_kind.size(); add(a, AFX_E_BAD_ARGS); }
    afx_blind_issue_randomness holes[4] = { rnd, rnd, rnd, rnd };
    holes[0].t_wide = nullptr; holes[1].U_wide = nullptr; holes[2].rprime_wide = nullptr; holes[3].rng_seed = nullptr;
    if (!drawn)
      for (int k = 0; k < 4; k++) { Args a = good; a.r = &holes[k]; add(a, AFX_E_BAD_ARGS); }
    for (size_t k = 0; k < table.size(); k++) {
      const int got = call(drawn != 0, table[k].first);
      if (got != table[k].second || !all_are(out, 0xEE) || !all_are(status, 0xEE)) {
        fprintf(stderr, "argument error %zu of the %s door: returned %d, expected %d; out untouched %d, status untouched %d\n", k, drawn ? "_rng" : "explicit", got,
                table[k].second, (int)all_are(out, 0xEE), (int)all_are(status, 0xEE));
        return 1;
      }
    }
  }
  CHECK(afx_issue_blind_wire(issuer, stream.data(), stream.size(), &rnd, out.data(), want_len, nullptr, status.data(), total, &cnt) == AFX_E_BAD_ARGS);
  CHECK(all_are(out, 0xEE) && all_are(status, 0xEE));
  {   // a NULL randomness array is refused even where no section would use it: a stream of one section of another n
    const Bytes other = section(W, 2);
    CHECK(afx_issue_blind_wire(issuer, other.data(), other.size(), nullptr, out.data(), want_len, &out_len, status.data(), total, &cnt) == AFX_E_BAD_ARGS);
    CHECK(all_are(out, 0xEE) && all_are(status, 0xEE));
    CHECK(afx_issue_blind_wire(issuer, other.data(), other.size(), &rnd, out.data(), want_len, &out_len, status.data(), total, &cnt) == AFX_OK);
    CHECK(out_len == 32 + 2 * OUT_REC && cnt == 2 && status[0] == AFX_ST_MAC_CREATION && status[1] == AFX_ST_MAC_CREATION && status[2] == 0xEE);
    out.assign(want_len, 0xEE); status.assign(total, 0xEE);
  }
  Bytes vst(total, 0xEE);
  CHECK(afx_verify_blind_requests_wire(user, stream.data(), stream.size(), vst.data(), total - 1, &cnt) == AFX_E_BAD_ARGS);
  CHECK(afx_verify_blind_requests_wire(user, stream.data(), stream.size() - 1, vst.data(), total, &cnt) == AFX_E_BAD_ARGS);
  CHECK(all_are(vst, 0xEE));

  // ---- the full calls ----
  for (uint32_t small : { 4096u, 0u }) {   // the latency plan (padded passes, kept plans) and the plan of large passes
    CHECK(afx_ctx_set_small_batch_items(issuer, small) == AFX_OK && afx_ctx_set_small_batch_items(user, small) == AFX_OK);
    for (int round = 0; round < 2; round++) {   // (the second round reuses the kept plans: the self-check compares each with a fresh one)
      out.assign(want_len, 0xEE); status.assign(total, 0xEE);
      CHECK(call(false, good) == AFX_OK);
      check_answer("explicit", parts, out, status, out_len, cnt, want_len, total);
      out.assign(want_len, 0xEE); status.assign(total, 0xEE);
      fake_draw_expect(seed40);
      CHECK(call(true, good) == AFX_OK);
      check_answer("drawn", parts, out, status, out_len, cnt, want_len, total);
      // two layouts on the GPU, four draws each per section that carries them; every job came with this call's seed || stream ...
      CHECK(fake_draw_jobs(0) == 4 * 3 && fake_draw_jobs(1) == 4 * 3);
      // ... and no copy of the seed is left where the draws read it or wrote (every one of those ranges still there to be read)
      CHECK(fake_draw_seed_left() == 0);
      CHECK(fake_draw_ranges_gone() == 0);
    }
    vst.assign(total, 0xEE);
    CHECK(afx_verify_blind_requests_wire(user, stream.data(), stream.size(), vst.data(), total, &cnt) == AFX_OK);
    CHECK(cnt == total);
    for (size_t i = 0; i < total; i++) CHECK(vst[i] != 0);
    CHECK(vst[5] == AFX_ST_VERIFICATION_FAILURE && vst[6] == AFX_ST_VERIFICATION_FAILURE);
  }

  // ---- three slices of one merged batch (256 is the smallest pass afx_ctx_set_chunk_items takes): 600 requests in two sections ----
  CHECK(afx_ctx_set_small_batch_items(issuer, 4096) == AFX_OK);
  CHECK(afx_ctx_set_chunk_items(issuer, 256) == AFX_OK);
  {
    const Bytes half = section(A, 300);
    Bytes big = half;
    big.insert(big.end(), half.begin(), half.end());
    Bytes btw(600 * 64, 0), buw(600 * 64, 0), brw(600 * 64, 0), bsd(600 * 32, 0);
    const afx_blind_issue_randomness brnd = { btw.data(), buw.data(), brw.data(), bsd.data() };
    const size_t sec_len = 32 + 300 * OUT_REC;
    const Parts two = { { A, 300 }, { A, 300 } };
    for (int drawn = 0; drawn < 2; drawn++) {
      Bytes bout(2 * sec_len, 0xEE), bst(600, 0xEE);
      const int rc = drawn ? afx_issue_blind_wire_rng(issuer, big.data(), big.size(), &rng, bout.data(), bout.size(), &out_len, bst.data(), 600, &cnt)
                           : afx_issue_blind_wire(issuer, big.data(), big.size(), &brnd, bout.data(), bout.size(), &out_len, bst.data(), 600, &cnt);
      CHECK(rc == AFX_OK);
      check_answer(drawn ? "slices, drawn" : "slices, explicit", two, bout, bst, out_len, cnt, 2 * sec_len, 600);
    }
  }
  CHECK(afx_ctx_set_chunk_items(issuer, 0) == AFX_OK);

  // ---- a group of two members on the fake device: the small path and the split path ----
  {
    const int devices[2] = { 0, 0 };
    afx_group* g = nullptr;
    CHECK(afx_group_create(&g, devices, 2, params.data(), params.size(), key.data(), key.size(), ip.data()) == AFX_OK);
    for (uint32_t small : { 4096u, 2u }) {   // 9 requests: whole to one member, then every batch split over the two
      for (uint32_t k = 0; k < 2; k++) CHECK(afx_ctx_set_small_batch_items(afx_group_member(g, k), small) == AFX_OK);
      for (int drawn = 0; drawn < 2; drawn++) {
        auto gcall = [&](size_t cap) {
          return drawn ? afx_group_issue_blind_wire_rng(g, stream.data(), stream.size(), &rng, out.data(), cap, &out_len, status.data(), total, &cnt)
                       : afx_group_issue_blind_wire(g, stream.data(), stream.size(), &rnd, out.data(), cap, &out_len, status.data(), total, &cnt);
        };
        out.assign(want_len, 0xEE); status.assign(total, 0xEE);
        CHECK(gcall(want_len) == AFX_OK);
        check_answer("group", parts, out, status, out_len, cnt, want_len, total);
        out.assign(want_len, 0xEE); status.assign(total, 0xEE);
        CHECK(gcall(want_len - 1) == AFX_E_BAD_ARGS);
        CHECK(all_are(out, 0xEE) && all_are(status, 0xEE));
      }
    }
    afx_group_destroy(g);
  }
  afx_ctx_destroy(issuer);
  afx_ctx_destroy(user);
  printf("blind wire doors ok\n");
  return 0;
}
