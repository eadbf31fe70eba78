// TEST INFRASTRUCTURE (CPU only): the doors of issuance on bytes (aeonflux_amd/csrc/wire_issue.cpp: afx_issue_wire, afx_issue_wire_rng and
// their group forms) and the verification of what they write (wire_user.cpp: afx_verify_issuances_mixed_wire and its group form) on the
// engine's host half.  tests/test_hostsim_request_wire.py links this file with the engine's host sources, wire_issue.cpp, wire_user.cpp,
// the fake HIP runtime and the stand-ins for the record-writing and draw launchers under AddressSanitizer + UBSan and runs it with
// AFX_PLAN_SELFCHECK=1.
//   request_wire_doors <dir>
// <dir> holds params.bin, key.bin and ip.bin of an issuer of 4 attributes, written by the test.
// The stream has five AFXR sections - layout A x 3, layout B x 2, a layout of n = 2 x 2, layout A x 2, layout A x 0 - so two batches go
// to the device, one of them gathered over two sections, and one section is answered on the host (MacCreation).  Nothing is computed
// on the fake device, but its two transpositions move bytes for real and its `echo` knob makes an item's status the first byte of the
// item's first scalar row: every scalar attribute value starts with the status its request is to get, and an accepted request's value
// cells must come back in its own AFXI record.  That pins which request lands where through gathering, scattering and a group's split.
// Prints "request wire doors ok" and exits 0, or says which check failed and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/aeonflux_gpu.h"

extern "C" void afx_fake_set(const char* what, int v);
extern "C" void fake_draw_expect(const uint8_t* seed40);
extern "C" uint64_t fake_draw_jobs(int with_seed);

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
static bool is_scalar(uint8_t k) { return k == AFX_ATTR_PUBLIC_SCALAR || k == AFX_ATTR_SECRET_SCALAR; }

static const uint32_t N = 4, NR = N + 5;
struct Part { Kinds kinds; size_t count; };

// the status the echoing fake gives stream item g of a section the device sees: every third request is refused
static uint8_t want_status(size_t g) { return g % 3 == 1 ? (uint8_t)(0x40 + g) : 0; }
// cell c of request g: a scalar value starts with the request's status; every value names its request and its cell
static void value_of(uint8_t v[32], const Kinds& kinds, size_t g, uint32_t c) {
  for (int k = 0; k < 32; k++) v[k] = (uint8_t)(g * 31 + c * 7 + k + 1);
  v[0] = is_scalar(kinds[c]) ? want_status(g) : (uint8_t)(0x80 + g);
  v[1] = (uint8_t)g; v[2] = (uint8_t)c;
}
// one AFXR section from the library's own packer: requests g0 .. g0 + count - 1 of the stream
static Bytes section(const Part& p, size_t g0) {
  const uint32_t n = (uint32_t)p.kinds.size();
  Bytes soa((size_t)n * p.count * 32 + 1, 0);
  for (uint32_t c = 0; c < n; c++)
    for (size_t i = 0; i < p.count; i++) value_of(&soa[((size_t)c * p.count + i) * 32], p.kinds, g0 + i, c);
  afx_attributes_soa a;
  memset(&a, 0, sizeof a);
  a.n_attributes = n;
  memcpy(a.kinds, p.kinds.data(), n);
  a.values = soa.data();
  size_t len = 0;
  CHECK(afx_request_wire_pack(&a, p.count, nullptr, 0, &len) == AFX_OK);
  CHECK(len == afx_request_wire_header_bytes(n) + p.count * n * 32);
  Bytes blob(len);
  CHECK(afx_request_wire_pack(&a, p.count, blob.data(), blob.size(), &len) == AFX_OK && len == blob.size());
  return blob;
}

static size_t out_bytes(const Part& p) { return 32 + p.count * (4 + NR + p.kinds.size()) * 32; }

// Every AFXI header; a section of another n: zero records and MacCreation; a section the device saw: with `echo` the statuses the
// requests ask for, zero records for the refused ones and the accepted ones' own values in their value cells - without it (the fake
// fails every item) only zero records and failing statuses.
static void check_answer(const char* what, const std::vector<Part>& parts, bool echo, const Bytes& out, const Bytes& status, size_t out_len, size_t cnt, size_t want_len,
                         size_t total) {
  if (out_len != want_len || cnt != total) { fprintf(stderr, "%s: out_len %zu count %zu\n", what, out_len, cnt); exit(1); }
  size_t off = 0, first = 0;
  for (const Part& part : parts) {
    const Kinds& kinds = part.kinds;
    const uint32_t n = (uint32_t)kinds.size(), cells = 4 + NR + n;
    const size_t c = part.count, size = out_bytes(part);
    uint8_t want[32];
    memset(want, 0, sizeof want);
    memcpy(want, "AFXI", 4);
    wr32(want + 4, 1); wr32(want + 8, (uint32_t)c); wr32(want + 12, cells); wr32(want + 16, n); wr32(want + 20, NR);
    memcpy(want + 24, kinds.data(), n);
    bool ok = memcmp(&out[off], want, 32) == 0;
    size_t sl = 0;
    ok = ok && afx_issuance_wire_section_bytes(&out[off], out.size() - off, &sl) == AFX_OK && sl == size;
    for (size_t i = 0; ok && i < c; i++) {
      const uint8_t* rec = &out[off + 32 + i * cells * 32];
      const size_t g = first + i;
      const uint8_t st = n != N ? AFX_ST_MAC_CREATION : echo ? want_status(g) : status[g];
      ok = status[g] == st && (echo || n != N || st != 0);
      if (st != 0) {
        for (size_t k = 0; ok && k < (size_t)cells * 32; k++) ok = rec[k] == 0;   // nothing is released for a request that was not accepted
      } else {
        for (uint32_t a = 0; ok && a < n; a++) {
          uint8_t v[32];
          value_of(v, kinds, g, a);
          ok = memcmp(rec + (size_t)(4 + NR + a) * 32, v, 32) == 0;
        }
      }
    }
    if (!ok) { fprintf(stderr, "%s: the answer to the section at item %zu (last error: %s)\n", what, first, afx_last_error()); exit(1); }
    off += size;
    first += c;
  }
  CHECK(off == want_len);
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: request_wire_doors <dir>\n"); return 2; }
  const std::string dir = argv[1];
  const Bytes params = rd(dir + "/params.bin"), key = rd(dir + "/key.bin"), ip = rd(dir + "/ip.bin");
  CHECK(ip.size() == 64);
  afx_ctx* issuer = nullptr;
  CHECK(afx_ctx_create(&issuer, 0, params.data(), params.size(), key.data(), key.size(), ip.data()) == AFX_OK);
  CHECK(afx_ctx_n_attributes(issuer) == N);
  const int devices[2] = { 0, 0 };
  afx_group* group = nullptr;
  CHECK(afx_group_create(&group, devices, 2, params.data(), params.size(), key.data(), key.size(), ip.data()) == AFX_OK);

  const Kinds A = { 1, 0, 2, 3 }, B = { 2, 0, 4, 1 }, W = { 0, 2 };
  const std::vector<Part> parts = { { A, 3 }, { B, 2 }, { W, 2 }, { A, 2 }, { A, 0 } };
  Bytes stream;
  std::vector<size_t> sec_off;
  size_t total = 0, want_len = 0;
  for (const Part& p : parts) {
    const Bytes s = section(p, total);
    sec_off.push_back(stream.size());
    stream.insert(stream.end(), s.begin(), s.end());
    total += p.count;
    want_len += out_bytes(p);
  }
  CHECK(total == 9);

  Bytes tw(total * 64), uw(total * 64), sd(total * 32);
  for (size_t k = 0; k < tw.size(); k++) { tw[k] = (uint8_t)(k * 13 + 5); uw[k] = (uint8_t)(k * 11 + 3); }
  for (size_t k = 0; k < sd.size(); k++) sd[k] = (uint8_t)(k * 7 + 1);
  const afx_issue_randomness rnd = { tw.data(), uw.data(), sd.data() };
  uint8_t seed40[40];
  for (int k = 0; k < 32; k++) seed40[k] = (uint8_t)(77 + k);
  const uint64_t stream_no = 5;
  for (int k = 0; k < 8; k++) seed40[32 + k] = (uint8_t)(stream_no >> (8 * k));
  const afx_device_rng rng = { seed40, stream_no };

  Bytes out(want_len, 0xEE), status(total, 0xEE);
  size_t out_len = 0, cnt = 0;
  // door 0, 1: afx_issue_wire, afx_issue_wire_rng; 2, 3: their group forms
  auto call = [&](int door, const Bytes& blob, uint8_t* o, size_t cap, uint8_t* st, size_t scap) {
    switch (door) {
      case 0: return afx_issue_wire(issuer, blob.data(), blob.size(), &rnd, o, cap, &out_len, st, scap, &cnt);
      case 1: return afx_issue_wire_rng(issuer, blob.data(), blob.size(), &rng, o, cap, &out_len, st, scap, &cnt);
      case 2: return afx_group_issue_wire(group, blob.data(), blob.size(), &rnd, o, cap, &out_len, st, scap, &cnt);
      default: return afx_group_issue_wire_rng(group, blob.data(), blob.size(), &rng, o, cap, &out_len, st, scap, &cnt);
    }
  };
  auto set_group_small = [&](uint32_t small) {
    for (uint32_t k = 0; k < 2; k++) CHECK(afx_ctx_set_small_batch_items(afx_group_member(group, k), small) == AFX_OK);
  };
  Bytes damaged = stream;   // the third section's n no longer matches its cells_per_record
  damaged[sec_off[2] + 16] ^= 1;

  static const char* const NAMES[4] = { "afx_issue_wire", "afx_issue_wire_rng", "afx_group_issue_wire", "afx_group_issue_wire_rng" };
  // small_batch_items of the group's members: above the stream's 9 requests (one member takes the call), then 0 (split over the two)
  for (uint32_t small : { 4096u, 0u }) {
    set_group_small(small);
    for (int door = 0; door < 4; door++) {
      // ---- the size query: lengths from the headers and the context's n, and nothing drawn ----
      fake_draw_expect(seed40);
      out_len = cnt = 7;
      CHECK(call(door, stream, nullptr, 0, nullptr, 0) == AFX_OK);
      CHECK(out_len == want_len && cnt == total);
      CHECK(fake_draw_jobs(0) == 0);
      // ---- argument errors: the code, and not a byte of out or status written ----
      out.assign(want_len, 0xEE); status.assign(total, 0xEE);
      CHECK(call(door, stream, out.data(), want_len - 1, status.data(), total) == AFX_E_BAD_ARGS);
      CHECK(call(door, stream, out.data(), want_len, status.data(), total - 1) == AFX_E_BAD_ARGS);
      CHECK(call(door, damaged, out.data(), want_len, status.data(), total) == AFX_E_BAD_ARGS);
      if (!all_are(out, 0xEE) || !all_are(status, 0xEE)) { fprintf(stderr, "%s: a refused call wrote to out or status\n", NAMES[door]); return 1; }
    }
  }

  // ---- the full calls: the group's bytes and statuses are the one context's ----
  // The one context runs its two batches with the collector's session (the default), in a session of the request's own (the collector
  // off) and one after the other (no latency plan); the group with one member taking the call and with every batch split.
  Bytes single_out[2][2], single_st[2][2];   // [echo][drawn]
  for (int echo = 0; echo < 2; echo++) {
    afx_fake_set("echo", echo);
    for (int mode = 0; mode < 3; mode++) {
      CHECK(afx_ctx_set_coalescing(issuer, mode == 0 ? 200 : 0, mode == 0 ? 4096 : 0) == AFX_OK);
      CHECK(afx_ctx_set_small_batch_items(issuer, mode == 2 ? 0 : 512) == AFX_OK);
      for (int drawn = 0; drawn < 2; drawn++) {
        out.assign(want_len, 0xEE); status.assign(total, 0xEE);
        fake_draw_expect(seed40);
        CHECK(call(drawn, stream, out.data(), want_len, status.data(), total) == AFX_OK);
        check_answer(NAMES[drawn], parts, echo != 0, out, status, out_len, cnt, want_len, total);
        // two layouts on the device, three draws each per section that carries them, every job with this call's seed || stream
        if (drawn) CHECK(fake_draw_jobs(0) == 3 * 3 && fake_draw_jobs(1) == 3 * 3);
        else CHECK(fake_draw_jobs(0) == 0);
        if (mode == 0) { single_out[echo][drawn] = out; single_st[echo][drawn] = status; }
        else if (!echo) CHECK(out == single_out[0][drawn]);   // (every record is zeros here: the whole stream can be compared)
        CHECK(status == single_st[echo][drawn]);
      }
    }
    for (uint32_t small : { 4096u, 0u }) {
      set_group_small(small);
      for (int round = 0; round < 2; round++)   // (the small path: a member each, in turn)
        for (int drawn = 0; drawn < 2; drawn++) {
          out.assign(want_len, 0xEE); status.assign(total, 0xEE);
          fake_draw_expect(seed40);
          CHECK(call(2 + drawn, stream, out.data(), want_len, status.data(), total) == AFX_OK);
          check_answer(NAMES[2 + drawn], parts, echo != 0, out, status, out_len, cnt, want_len, total);
          CHECK(fake_draw_jobs(0) == fake_draw_jobs(1) && (fake_draw_jobs(0) != 0) == (drawn != 0));
          if (!echo) CHECK(out == single_out[0][drawn]);
          CHECK(status == single_st[echo][drawn]);
        }
    }
  }

  // ---- the AFXI stream back through the verification.  The fake device's verification of an issuance fails whole before any check is
  // laid out (its negated generators encode as zeros), so the echo does not reach it: every path must give every issuance the same
  // failing status, and leave nothing unanswered. ----
  const Bytes& issued = single_out[1][0];
  Bytes vst(total, 0xEE), vsingle;
  CHECK(afx_verify_issuances_mixed_wire(issuer, issued.data(), issued.size(), vst.data(), total - 1, &cnt) == AFX_E_BAD_ARGS);
  CHECK(all_are(vst, 0xEE));
  for (int mode = 0; mode < 3; mode++) {
    CHECK(afx_ctx_set_coalescing(issuer, mode == 0 ? 200 : 0, mode == 0 ? 4096 : 0) == AFX_OK);
    CHECK(afx_ctx_set_small_batch_items(issuer, mode == 2 ? 0 : 512) == AFX_OK);
    vst.assign(total, 0xEE); cnt = 0;
    CHECK(afx_verify_issuances_mixed_wire(issuer, issued.data(), issued.size(), vst.data(), total, &cnt) == AFX_OK && cnt == total);
    for (size_t g = 0; g < total; g++) CHECK(vst[g] != AFX_ST_OK && vst[g] != 0xEE);
    if (mode == 0) vsingle = vst;
    CHECK(vst == vsingle);
  }
  for (uint32_t small : { 4096u, 0u }) {
    set_group_small(small);
    for (int round = 0; round < 2; round++) {
      vst.assign(total, 0xEE); cnt = 0;
      CHECK(afx_group_verify_issuances_mixed_wire(group, issued.data(), issued.size(), vst.data(), total, &cnt) == AFX_OK && cnt == total);
      CHECK(vst == vsingle);
    }
    vst.assign(total, 0xEE);
    CHECK(afx_group_verify_issuances_mixed_wire(group, issued.data(), issued.size(), vst.data(), total - 1, &cnt) == AFX_E_BAD_ARGS);
    CHECK(afx_group_verify_issuances_mixed_wire(group, issued.data(), issued.size() - 1, vst.data(), total, &cnt) == AFX_E_BAD_ARGS);
    CHECK(all_are(vst, 0xEE));
  }
  afx_fake_set("echo", 0);
  afx_group_destroy(group);
  afx_ctx_destroy(issuer);
  printf("request wire doors ok\n");
  return 0;
}
