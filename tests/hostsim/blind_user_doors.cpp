// TEST INFRASTRUCTURE (CPU only): the user's doors of blind issuance on bytes (aeonflux_amd/csrc/wire_blind_user.cpp) on the engine's
// host half.  tests/test_hostsim_blind_user_wire.py links this file with the engine's host sources, statements_blind.cpp, wire_blind.cpp,
// wire_blind_user.cpp, the fake HIP runtime and the stand-ins for the masking, record-writing and draw launchers under AddressSanitizer
// + UBSan and runs it with AFX_PLAN_SELFCHECK=1.
//   blind_user_doors <dir>
// <dir> holds params.bin, key.bin and ip.bin of an issuer of 4 attributes, written by the test.  Every input is zeros, so every item
// fails: what is checked is sizes, headers, what an argument error leaves untouched, zero records and zero t, U, V, slices, the group's
// two paths, and where the _rng forms' seed, d_wide rows and d rows go.  The stand-in for k_reduce_wide in fake_hip.cpp writes nothing, so
// the program is linked with --wrap for that launcher and for the record-writing one (their mangled names: WRAP_* below, which the test
// passes to the linker): reduce_wide here fills the row it is given - the d row - with 0xD5 and remembers it, soa_to_aos notes every
// call that reads such a row (the copy of d into an output row, which only a caller that gave d_out may get) and where it wrote.
// After a call every remembered row must read zero.
// Prints "blind user doors ok" and exits 0, or says which check failed and exits 1.
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

// ---- the wrapped launchers (ld --wrap: every call of the engine's goes through these; __real_ is the stand-in of tests/hostsim) ----
#include <hip/hip_runtime_api.h>
#include <mutex>
#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#endif
#define WRAP_REDUCE_WIDE _Z16afxk_reduce_wideP12ihipStream_tPKhPhj
#define WRAP_SOA_TO_AOS _Z15afxk_soa_to_aosP12ihipStream_tPKhPhPKjS2_jj
#define GLUE2(a, b) a##b
#define GLUE(a, b) GLUE2(a, b)
extern "C" hipError_t GLUE(__real_, WRAP_REDUCE_WIDE)(hipStream_t, const uint8_t*, uint8_t*, uint32_t);
extern "C" hipError_t GLUE(__real_, WRAP_SOA_TO_AOS)(hipStream_t, const uint8_t*, uint8_t*, const uint32_t*, const uint8_t*, uint32_t, uint32_t);
static std::mutex watch_mu;
static std::vector<std::pair<const uint8_t*, size_t>> d_rows, d_copies;   // rows reduce_wide "wrote" d into; output rows a copy of such a row went to
static uint64_t reduce_calls = 0;
extern "C" hipError_t GLUE(__wrap_, WRAP_REDUCE_WIDE)(hipStream_t s, const uint8_t* wide, uint8_t* out, uint32_t count) {
  {
    std::lock_guard<std::mutex> lk(watch_mu);
    reduce_calls++;
    memset(out, 0xD5, (size_t)count * 32);   // "d"
    d_rows.push_back({ out, (size_t)count * 32 });
  }
  return GLUE(__real_, WRAP_REDUCE_WIDE)(s, wide, out, count);
}
extern "C" hipError_t GLUE(__wrap_, WRAP_SOA_TO_AOS)(hipStream_t s, const uint8_t* soa, uint8_t* rec, const uint32_t* m, const uint8_t* status, uint32_t cells, uint32_t n) {
  {
    std::lock_guard<std::mutex> lk(watch_mu);
    for (const auto& r : d_rows)
      if (cells == 1 && soa + (size_t)m[0] * n * 32 == r.first) { d_copies.push_back({ rec, (size_t)n * 32 }); break; }   // (slices reuse a lane's rows: one note per call)
  }
  return GLUE(__real_, WRAP_SOA_TO_AOS)(s, soa, rec, m, status, cells, n);
}
static void watch_reset() { std::lock_guard<std::mutex> lk(watch_mu); d_rows.clear(); d_copies.clear(); reduce_calls = 0; }
// how many of the remembered ranges can still be read (a staging area regrown since is gone), and whether all of those read zero
static bool all_zero(const std::vector<std::pair<const uint8_t*, size_t>>& ranges, size_t* readable) {
  bool zero = true;
  *readable = 0;
  for (const auto& r : ranges) {
#if defined(__SANITIZE_ADDRESS__)
    if (__asan_region_is_poisoned(const_cast<uint8_t*>(r.first), r.second)) continue;
#endif
    ++*readable;
    for (size_t k = 0; k < r.second; k++) zero = zero && r.first[k] == 0;
  }
  return zero;
}
// after an _rng call: d was made (`slices` reductions), every d row is zeros again, and d was copied to an output row - itself zeroed
// behind the fetch - exactly when the caller asked for it
static void check_d_rows(const char* what, size_t slices, bool copied) {
  std::lock_guard<std::mutex> lk(watch_mu);
  size_t rows = 0, copies = 0;
  const bool rows_zero = all_zero(d_rows, &rows), copies_zero = all_zero(d_copies, &copies);
  if (reduce_calls != slices || d_rows.size() != slices || rows == 0 || !rows_zero || d_copies.size() != (copied ? slices : 0) || !copies_zero || (copied && copies == 0)) {
    fprintf(stderr, "%s: %llu reductions (expected %zu), %zu d rows readable, all zero %d; %zu copies of d to an output row (expected %zu), all zero %d\n", what,
            (unsigned long long)reduce_calls, slices, rows, (int)rows_zero, d_copies.size(), copied ? slices : (size_t)0, (int)copies_zero);
    exit(1);
  }
}

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
static void layout(const Kinds& kinds, uint32_t& h, uint32_t& hs) {
  h = hs = 0;
  for (uint8_t k : kinds) { h += k == AFX_ATTR_SECRET_SCALAR || k == AFX_ATTR_SECRET_POINT; hs += k == AFX_ATTR_SECRET_SCALAR; }
}

static const uint32_t N = 4;
typedef std::vector<std::pair<Kinds, size_t>> Parts;

// the groups of a request call over all-zero columns (one zero buffer serves every array)
struct Groups {
  std::vector<afx_blind_request_group> g;
  Bytes zeros;
  Groups(const Parts& parts, uint32_t n_of_last = 0) {
    size_t most = 1;
    for (const auto& p : parts) most = p.second > most ? p.second : most;
    zeros.assign(AFX_MAX_ATTRIBUTES * most * 64, 0);
    for (const auto& p : parts) {
      afx_blind_request_group x;
      memset(&x, 0, sizeof x);
      x.attrs.n_attributes = (uint32_t)p.first.size();
      if (!p.first.empty()) memcpy(x.attrs.kinds, p.first.data(), p.first.size());
      x.attrs.values = zeros.data();
      x.d = zeros.data();
      x.rnd.r_wide = zeros.data();
      x.rnd.rng_seed = zeros.data();
      x.count = p.second;
      g.push_back(x);
    }
    if (n_of_last) g.back().attrs.n_attributes = n_of_last;   // (a layout of more positions than a header has room for)
  }
};
// what the section of a group must be: (header n, cells, n_responses)
static size_t section_size(const Kinds& kinds, size_t count, bool no_kinds) {
  uint32_t h, hs;
  layout(no_kinds ? Kinds() : kinds, h, hs);
  const size_t n = no_kinds ? 0 : kinds.size();
  return ((24 + n + 31) & ~size_t(31)) + count * (3 + 2 * h + hs + n) * 32;
}
// well-formed AFXQ headers, zero records, a failing status per item (AFX_ST_MAC_CREATION where the context does not serve the layout)
static void check_requests(const char* what, const Parts& parts, size_t zero_kind_from, const Bytes& out, const Bytes& status, size_t out_len, size_t cnt) {
  size_t off = 0, first = 0;
  for (size_t k = 0; k < parts.size(); k++) {
    const bool no_kinds = k >= zero_kind_from;
    const Kinds kinds = no_kinds ? Kinds() : parts[k].first;
    uint32_t h, hs;
    layout(kinds, h, hs);
    const size_t c = parts[k].second, hdr = (24 + kinds.size() + 31) & ~size_t(31), size = section_size(parts[k].first, c, no_kinds);
    Bytes want(hdr, 0);
    memcpy(want.data(), "AFXQ", 4);
    wr32(&want[4], 1); wr32(&want[8], (uint32_t)c); wr32(&want[12], (uint32_t)(3 + 2 * h + hs + kinds.size())); wr32(&want[16], (uint32_t)kinds.size()); wr32(&want[20], 1 + h + hs);
    if (!kinds.empty()) memcpy(&want[24], kinds.data(), kinds.size());
    bool ok = off + size <= out.size() && memcmp(&out[off], want.data(), hdr) == 0;
    size_t sl = 0;
    ok = ok && afx_blind_request_wire_section_bytes(&out[off], out.size() - off, &sl) == AFX_OK && sl == size;
    for (size_t b = hdr; ok && b < size; b++) ok = out[off + b] == 0;
    const bool served = !no_kinds && kinds.size() == N;
    for (size_t i = 0; ok && i < c; i++) ok = status[first + i] != 0 && (served || status[first + i] == AFX_ST_MAC_CREATION);
    if (!ok) { fprintf(stderr, "%s: the section of group %zu (last error: %s)\n", what, k, afx_last_error()); exit(1); }
    off += size;
    first += c;
  }
  if (off != out_len || first != cnt) { fprintf(stderr, "%s: out_len %zu count %zu, expected %zu and %zu\n", what, out_len, cnt, off, first); exit(1); }
}

// all-zero AFXQ and AFXJ sections from the library's own packers
static Bytes request_section(const Kinds& kinds, size_t count) {
  Bytes zeros((AFX_MAX_ATTRIBUTES + 8) * count * 32 + 1, 0);
  afx_attributes_soa a;
  memset(&a, 0, sizeof a);
  a.n_attributes = (uint32_t)kinds.size();
  memcpy(a.kinds, kinds.data(), kinds.size());
  a.values = zeros.data();
  afx_blind_request_soa q = { zeros.data(), zeros.data(), zeros.data(), zeros.data(), zeros.data() };
  size_t len = 0;
  CHECK(afx_blind_request_wire_pack(&a, &q, count, nullptr, 0, &len) == AFX_OK);
  Bytes blob(len);
  CHECK(afx_blind_request_wire_pack(&a, &q, count, blob.data(), blob.size(), &len) == AFX_OK && len == blob.size());
  return blob;
}
static Bytes issuance_section(const Kinds& kinds, size_t count, uint32_t nr = N + 6) {
  Bytes zeros((size_t)(nr + 1) * count * 32 + 1, 0);
  afx_attributes_soa a;
  memset(&a, 0, sizeof a);
  a.n_attributes = (uint32_t)kinds.size();
  memcpy(a.kinds, kinds.data(), kinds.size());
  afx_blind_issuance_soa s = { zeros.data(), zeros.data(), zeros.data(), zeros.data(), zeros.data(), zeros.data() };
  size_t len = 0;
  CHECK(afx_blind_issuance_wire_pack(&a, &s, nr, count, nullptr, 0, &len) == AFX_OK);
  Bytes blob(len);
  CHECK(afx_blind_issuance_wire_pack(&a, &s, nr, count, blob.data(), blob.size(), &len) == AFX_OK && len == blob.size());
  return blob;
}
static void append(Bytes& to, const Bytes& s) { to.insert(to.end(), s.begin(), s.end()); }

// t, U, V and the statuses of an unblinding call over `total` items, pre-filled so that what a call leaves alone shows
struct Cred {
  Bytes t, U, V, status;
  afx_credential_out out;
  explicit Cred(size_t total) : t(total * 32, 0xEE), U(total * 32, 0xEE), V(total * 32, 0xEE), status(total, 0xEE) { out = { t.data(), U.data(), V.data() }; }
  bool untouched() const { return all_are(t, 0xEE) && all_are(U, 0xEE) && all_are(V, 0xEE) && all_are(status, 0xEE); }
  bool all_failed() const {
    for (uint8_t s : status)
      if (s == 0 || s == 0xEE) return false;
    return all_are(t, 0) && all_are(U, 0) && all_are(V, 0);
  }
};

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: blind_user_doors <dir>\n"); return 2; }
  const std::string dir = argv[1];
  const Bytes params = rd(dir + "/params.bin"), key = rd(dir + "/key.bin"), ip = rd(dir + "/ip.bin");
  CHECK(ip.size() == 64);
  afx_ctx* user = nullptr;
  CHECK(afx_ctx_create(&user, 0, params.data(), params.size(), nullptr, 0, ip.data()) == AFX_OK);   // the user's doors need no key
  CHECK(afx_ctx_n_attributes(user) == N);

  uint8_t seed40[40], d7[40];
  for (int k = 0; k < 32; k++) { seed40[k] = (uint8_t)(101 + k); d7[k] = 0xD7; }   // (0xD7: what the fake k_draw fills a row with)
  const uint64_t stream_no = 9;
  for (int k = 0; k < 8; k++) seed40[32 + k] = d7[32 + k] = (uint8_t)(stream_no >> (8 * k));
  const afx_device_rng rng = { seed40, stream_no }, rng_d7 = { d7, stream_no }, rng_os = { nullptr, stream_no };

  const Kinds A = { 4, 2, 3, 1 }, B = { 0, 1, 4, 2 }, W = { 0, 2 }, P = { 0, 2, 0, 3 };
  size_t out_len = 0, cnt = 0;

  // ================= afx_blind_request_wire =================
  // two layouts of the context's n (the first in two groups), one of another n, one of no attributes and one of more than a header holds
  const Parts parts = { { A, 3 }, { B, 2 }, { W, 2 }, { A, 2 }, { Kinds(), 1 }, { A, 1 } };
  Groups G(parts, AFX_MAX_ATTRIBUTES + 3);
  const size_t zero_kind_from = 4, n_groups = parts.size();
  size_t total = 0, want_len = 0;
  for (size_t k = 0; k < parts.size(); k++) { total += parts[k].second; want_len += section_size(parts[k].first, parts[k].second, k >= zero_kind_from); }
  CHECK(afx_blind_request_wire_header_bytes(0) == 32);

  {   // the size query: from the kinds and the counts, no arrays
    std::vector<afx_blind_request_group> bare = G.g;
    for (auto& x : bare) { x.attrs.values = nullptr; x.d = nullptr; x.rnd.r_wide = nullptr; x.rnd.rng_seed = nullptr; }
    CHECK(afx_blind_request_wire(user, bare.data(), n_groups, nullptr, 0, &out_len, nullptr, 0, &cnt) == AFX_OK && out_len == want_len && cnt == total);
    out_len = cnt = 7;
    CHECK(afx_blind_request_wire_rng(user, bare.data(), n_groups, &rng_os, nullptr, nullptr, 0, &out_len, nullptr, 0, &cnt) == AFX_OK && out_len == want_len && cnt == total);
    CHECK(afx_blind_request_wire(user, nullptr, 0, nullptr, 0, &out_len, nullptr, 0, &cnt) == AFX_OK && out_len == 0 && cnt == 0);
  }

  Bytes out(want_len, 0xEE), status(total, 0xEE), d_out(total * 32, 0xEE);
  struct RArgs { afx_ctx* ctx; const std::vector<afx_blind_request_group>* g; size_t cap, scap; bool null_status, null_rng, null_d_out; const afx_device_rng* rng; };
  const RArgs rgood = { user, &G.g, want_len, total, false, false, false, &rng };
  auto rcall = [&](bool drawn, const RArgs& a) {
    uint8_t* st = a.null_status ? nullptr : status.data();
    if (drawn)
      return afx_blind_request_wire_rng(a.ctx, a.g->data(), a.g->size(), a.null_rng ? nullptr : a.rng, a.null_d_out ? nullptr : d_out.data(), out.data(), a.cap, &out_len, st, a.scap, &cnt);
    return afx_blind_request_wire(a.ctx, a.g->data(), a.g->size(), out.data(), a.cap, &out_len, st, a.scap, &cnt);
  };
  // ---- argument errors: the code, and not a byte of out, status or d_out written ----
  std::vector<afx_blind_request_group> bad_kind = G.g, bad_kind0 = G.g, no_values = G.g, no_d = G.g, no_seed = G.g, no_rw = G.g;
  bad_kind[3].attrs.kinds[2] = 5;
  { afx_blind_request_group z = G.g[0]; z.count = 0; z.attrs.kinds[0] = 5; bad_kind0.push_back(z); }   // the layout of a group of count 0 is checked too
  no_values[1].attrs.values = nullptr; no_d[0].d = nullptr; no_seed[3].rnd.rng_seed = nullptr; no_rw[1].rnd.r_wide = nullptr;
  for (int drawn = 0; drawn < 2; drawn++) {
    std::vector<RArgs> table;
    { RArgs a = rgood; a.cap = want_len - 1; table.push_back(a); }
    { RArgs a = rgood; a.scap = total - 1; table.push_back(a); }
    { RArgs a = rgood; a.null_status = true; table.push_back(a); }
    { RArgs a = rgood; a.ctx = nullptr; table.push_back(a); }
    { RArgs a = rgood; a.g = &bad_kind; table.push_back(a); }
    { RArgs a = rgood; a.g = &bad_kind0; table.push_back(a); }
    { RArgs a = rgood; a.g = &no_values; table.push_back(a); }
    if (!drawn)
      for (const auto* g : { &no_d, &no_seed, &no_rw }) { RArgs a = rgood; a.g = g; table.push_back(a); }
    if (drawn) {
      { RArgs a = rgood; a.null_rng = true; table.push_back(a); }
      { RArgs a = rgood; a.rng = &rng_os; a.null_d_out = true; table.push_back(a); }   // a seed nobody keeps and no d: the requests could never be unblinded
    }
    for (size_t k = 0; k < table.size(); k++) {
      const int got = rcall(drawn != 0, table[k]);
      if (got != AFX_E_BAD_ARGS || !all_are(out, 0xEE) || !all_are(status, 0xEE) || !all_are(d_out, 0xEE)) {
        fprintf(stderr, "argument error %zu of the %s request door: returned %d; out untouched %d, status %d, d_out %d\n", k, drawn ? "_rng" : "explicit", got,
                (int)all_are(out, 0xEE), (int)all_are(status, 0xEE), (int)all_are(d_out, 0xEE));
        return 1;
      }
    }
  }
  CHECK(afx_blind_request_wire(user, G.g.data(), n_groups, out.data(), want_len, nullptr, status.data(), total, &cnt) == AFX_E_BAD_ARGS && all_are(out, 0xEE));
  // (the size query reports a kind no header can carry as well)
  CHECK(afx_blind_request_wire(user, bad_kind.data(), n_groups, nullptr, 0, &out_len, nullptr, 0, &cnt) == AFX_E_BAD_ARGS);

  // ---- the full calls ----
  for (uint32_t small : { 4096u, 0u }) {   // the latency plan (padded passes, kept plans) and the plan of large passes
    CHECK(afx_ctx_set_small_batch_items(user, small) == AFX_OK);
    for (int round = 0; round < 2; round++) {   // (the second round reuses the kept plans: the self-check compares each with a fresh one)
      out.assign(want_len, 0xEE); status.assign(total, 0xEE);
      CHECK(rcall(false, rgood) == AFX_OK);
      check_requests("explicit", parts, zero_kind_from, out, status, out_len, cnt);
      out.assign(want_len, 0xEE); status.assign(total, 0xEE); d_out.assign(total * 32, 0xEE);
      fake_draw_expect(seed40);
      watch_reset();
      CHECK(rcall(true, rgood) == AFX_OK);
      check_requests("drawn", parts, zero_kind_from, out, status, out_len, cnt);
      check_d_rows("drawn", 3, true);   // three groups on the GPU, a slice each
      CHECK(all_are(d_out, 0));   // every item failed: no d is handed out
      // three groups on the GPU, each with d_wide, two r_wide rows and rng_seed; every job came with this call's seed || stream ...
      CHECK(fake_draw_jobs(0) == 3 * 4 && fake_draw_jobs(1) == 3 * 4);
      // ... and no copy of the seed is left where the draws read it or wrote
      CHECK(fake_draw_seed_left() == 0);
      CHECK(fake_draw_ranges_gone() == 0);
      watch_reset();
      { RArgs a = rgood; a.null_d_out = true; out.assign(want_len, 0xEE); status.assign(total, 0xEE); CHECK(rcall(true, a) == AFX_OK); }   // a seed the caller keeps: d_out may be NULL
      check_d_rows("drawn, no d_out", 3, false);   // ... and then d never leaves its scratch row
      check_requests("drawn, no d_out", parts, zero_kind_from, out, status, out_len, cnt);
    }
  }
  CHECK(afx_ctx_set_small_batch_items(user, 4096) == AFX_OK);
  {
    // the d_wide rows are zeros when the call returns: with a seed of 0xD7 bytes a row the fake draw filled reads like the seed, and of
    // the rows this call draws - d_wide [3][64] and rng_seed [3][32] of a layout that hides nothing - only the 96 bytes of rng_seed are
    // left to be found (96 - 31 places)
    const Parts plain = { { P, 3 } };
    Groups GP(plain);
    const size_t len = section_size(P, 3, false);
    Bytes o(len, 0xEE), s(3, 0xEE), dd(96, 0xEE);
    fake_draw_expect(d7);
    CHECK(afx_blind_request_wire_rng(user, GP.g.data(), 1, &rng_d7, dd.data(), o.data(), len, &out_len, s.data(), 3, &cnt) == AFX_OK);
    check_requests("drawn, 0xD7", plain, 1, o, s, out_len, cnt);
    CHECK(fake_draw_jobs(0) == 2 && fake_draw_jobs(1) == 2);
    CHECK(fake_draw_seed_left() == 96 - 31);
    CHECK(fake_draw_ranges_gone() == 0);
  }

  // ================= afx_unblind_issuances_wire =================
  const Parts uparts = { { A, 3 }, { B, 2 }, { W, 2 }, { A, 2 } };
  Bytes qs, js;
  size_t utotal = 0;
  for (const auto& p : uparts) { append(qs, request_section(p.first, p.second)); append(js, issuance_section(p.first, p.second)); utotal += p.second; }
  Bytes dz(utotal * 32 + 32, 0);
  {
    struct UArgs { afx_ctx* ctx; const Bytes* j; const Bytes* q; bool null_d, null_out, null_status; size_t scap; const afx_device_rng* rng; };
    Cred C(utotal);
    const UArgs ugood = { user, &js, &qs, false, false, false, utotal, &rng };
    auto ucall = [&](bool drawn, const UArgs& a) {
      uint8_t* st = a.null_status ? nullptr : C.status.data();
      const afx_credential_out* o = a.null_out ? nullptr : &C.out;
      if (drawn) return afx_unblind_issuances_wire_rng(a.ctx, a.j->data(), a.j->size(), a.q->data(), a.q->size(), a.rng, o, st, a.scap, &cnt);
      return afx_unblind_issuances_wire(a.ctx, a.j->data(), a.j->size(), a.q->data(), a.q->size(), a.null_d ? nullptr : dz.data(), o, st, a.scap, &cnt);
    };
    // ---- argument errors ----
    const Bytes last_j = issuance_section(A, 2), last_q = request_section(A, 2);
    Bytes fewer_j(js.begin(), js.end() - last_j.size()), fewer_q(qs.begin(), qs.end() - last_q.size()), truncated(js.begin(), js.end() - 1), other_count = fewer_j,
          other_kind = fewer_j, trailing = js, bad_q = qs;
    append(other_count, issuance_section(A, 1));
    { Kinds A2 = A; A2[1] = 0; append(other_kind, issuance_section(A2, 2)); }
    trailing.insert(trailing.end(), { 'A', 'F', 'X', 'J' });
    bad_q[4] = 2;   // a version no parser knows, in the first request section
    for (int drawn = 0; drawn < 2; drawn++) {
      std::vector<UArgs> table;
      { UArgs a = ugood; a.j = &fewer_j; table.push_back(a); }      // the section counts differ, either way
      { UArgs a = ugood; a.q = &fewer_q; table.push_back(a); }
      { UArgs a = ugood; a.j = &other_count; table.push_back(a); }  // a pair that differs in count
      { UArgs a = ugood; a.j = &other_kind; table.push_back(a); }   // ... in one kind
      { UArgs a = ugood; a.j = &truncated; table.push_back(a); }
      { UArgs a = ugood; a.j = &trailing; table.push_back(a); }
      { UArgs a = ugood; a.q = &bad_q; table.push_back(a); }
      { UArgs a = ugood; a.scap = utotal - 1; table.push_back(a); }
      { UArgs a = ugood; a.null_status = true; table.push_back(a); }
      { UArgs a = ugood; a.null_out = true; table.push_back(a); }
      { UArgs a = ugood; a.ctx = nullptr; table.push_back(a); }
      if (!drawn) { UArgs a = ugood; a.null_d = true; table.push_back(a); }
      if (drawn) {
        { UArgs a = ugood; a.rng = nullptr; table.push_back(a); }
        { UArgs a = ugood; a.rng = &rng_os; table.push_back(a); }   // no seed: nothing to derive d from
      }
      for (size_t k = 0; k < table.size(); k++) {
        const int got = ucall(drawn != 0, table[k]);
        if (got != AFX_E_BAD_ARGS || !C.untouched()) {
          fprintf(stderr, "argument error %zu of the %s unblinding door: returned %d; outputs untouched %d\n", k, drawn ? "_rng" : "explicit", got, (int)C.untouched());
          return 1;
        }
      }
    }
    // ---- the full calls ----
    for (uint32_t small : { 4096u, 0u }) {
      CHECK(afx_ctx_set_small_batch_items(user, small) == AFX_OK);
      for (int round = 0; round < 2; round++) {
        Cred E(utotal);
        cnt = 0;
        CHECK(afx_unblind_issuances_wire(user, js.data(), js.size(), qs.data(), qs.size(), dz.data(), &E.out, E.status.data(), utotal, &cnt) == AFX_OK && cnt == utotal);
        CHECK(E.all_failed() && E.status[5] == AFX_ST_VERIFICATION_FAILURE && E.status[6] == AFX_ST_VERIFICATION_FAILURE);
        Cred D(utotal);
        cnt = 0;
        fake_draw_expect(seed40);
        watch_reset();
        CHECK(afx_unblind_issuances_wire_rng(user, js.data(), js.size(), qs.data(), qs.size(), &rng, &D.out, D.status.data(), utotal, &cnt) == AFX_OK && cnt == utotal);
        check_d_rows("unblinding, drawn", 2, false);   // two merged batches, a slice each
        CHECK(D.all_failed() && D.status[5] == AFX_ST_VERIFICATION_FAILURE);
        // two merged batches, one of them in two sections: a d_wide draw per section that carries a batch's items
        CHECK(fake_draw_jobs(0) == 3 && fake_draw_jobs(1) == 3);
        CHECK(fake_draw_seed_left() == 0);
        CHECK(fake_draw_ranges_gone() == 0);
      }
    }
    CHECK(afx_ctx_set_small_batch_items(user, 4096) == AFX_OK);
    {   // d_wide is the only row this door draws: with the seed of 0xD7 bytes nothing that reads like it may be left
      Cred D(utotal);
      fake_draw_expect(d7);
      CHECK(afx_unblind_issuances_wire_rng(user, js.data(), js.size(), qs.data(), qs.size(), &rng_d7, &D.out, D.status.data(), utotal, &cnt) == AFX_OK);
      CHECK(D.all_failed() && fake_draw_jobs(1) == 3);
      CHECK(fake_draw_seed_left() == 0);
      CHECK(fake_draw_ranges_gone() == 0);
    }
    {   // a response count that is not the context's n + 6 fails its section on the host; an empty pair of streams is no item
      Bytes j2 = issuance_section(A, 2, N + 5), q2 = request_section(A, 2);
      Cred E(3);
      CHECK(afx_unblind_issuances_wire(user, j2.data(), j2.size(), q2.data(), q2.size(), dz.data(), &E.out, E.status.data(), 3, &cnt) == AFX_OK && cnt == 2);
      CHECK(E.status[0] == AFX_ST_VERIFICATION_FAILURE && E.status[1] == AFX_ST_VERIFICATION_FAILURE && E.status[2] == 0xEE && E.t[63] == 0 && E.t[64] == 0xEE && E.V[0] == 0);
      cnt = 7;
      CHECK(afx_unblind_issuances_wire(user, nullptr, 0, nullptr, 0, nullptr, &E.out, nullptr, 0, &cnt) == AFX_OK && cnt == 0);
    }
  }

  // ---- slices (256 is the smallest pass afx_ctx_set_chunk_items takes): 300 items make two, 600 in two sections of one layout three ----
  CHECK(afx_ctx_set_chunk_items(user, 256) == AFX_OK);
  for (int two = 0; two < 2; two++) {
    const Parts sp = two ? Parts{ { A, 300 }, { A, 300 } } : Parts{ { A, 300 } };
    const size_t items = two ? 600 : 300;
    Groups GS(sp);
    size_t len = 0;
    Bytes sq, sj;
    for (const auto& p : sp) { len += section_size(p.first, p.second, false); append(sq, request_section(p.first, p.second)); append(sj, issuance_section(p.first, p.second)); }
    Bytes dzs(items * 32, 0);
    for (int drawn = 0; drawn < 2; drawn++) {
      Bytes o(len, 0xEE), s(items, 0xEE), dd(items * 32, 0xEE);
      const int rc = drawn ? afx_blind_request_wire_rng(user, GS.g.data(), sp.size(), &rng, dd.data(), o.data(), len, &out_len, s.data(), items, &cnt)
                           : afx_blind_request_wire(user, GS.g.data(), sp.size(), o.data(), len, &out_len, s.data(), items, &cnt);
      CHECK(rc == AFX_OK);
      check_requests(drawn ? "slices, drawn" : "slices, explicit", sp, sp.size(), o, s, out_len, cnt);
      CHECK(!drawn || all_are(dd, 0));
      Cred E(items);
      const int rc2 = drawn ? afx_unblind_issuances_wire_rng(user, sj.data(), sj.size(), sq.data(), sq.size(), &rng, &E.out, E.status.data(), items, &cnt)
                            : afx_unblind_issuances_wire(user, sj.data(), sj.size(), sq.data(), sq.size(), dzs.data(), &E.out, E.status.data(), items, &cnt);
      CHECK(rc2 == AFX_OK && cnt == items && E.all_failed());
    }
  }
  CHECK(afx_ctx_set_chunk_items(user, 0) == AFX_OK);

  // ---- a group of two members on the fake device: the small path and the split path ----
  {
    const int devices[2] = { 0, 0 };
    afx_group* g = nullptr;
    CHECK(afx_group_create(&g, devices, 2, params.data(), params.size(), key.data(), key.size(), ip.data()) == AFX_OK);
    for (uint32_t small : { 4096u, 2u }) {   // whole to one member, then every group or batch split over the two
      for (uint32_t k = 0; k < 2; k++) CHECK(afx_ctx_set_small_batch_items(afx_group_member(g, k), small) == AFX_OK);
      for (int drawn = 0; drawn < 2; drawn++) {
        auto gcall = [&](size_t cap) {
          return drawn ? afx_group_blind_request_wire_rng(g, G.g.data(), n_groups, &rng, d_out.data(), out.data(), cap, &out_len, status.data(), total, &cnt)
                       : afx_group_blind_request_wire(g, G.g.data(), n_groups, out.data(), cap, &out_len, status.data(), total, &cnt);
        };
        out.assign(want_len, 0xEE); status.assign(total, 0xEE); d_out.assign(total * 32, 0xEE);
        CHECK(gcall(want_len) == AFX_OK);
        check_requests("group", parts, zero_kind_from, out, status, out_len, cnt);
        CHECK(!drawn || all_are(d_out, 0));
        out.assign(want_len, 0xEE); status.assign(total, 0xEE); d_out.assign(total * 32, 0xEE);
        CHECK(gcall(want_len - 1) == AFX_E_BAD_ARGS);
        CHECK(all_are(out, 0xEE) && all_are(status, 0xEE) && all_are(d_out, 0xEE));
        Cred E(utotal);
        const int rc = drawn ? afx_group_unblind_issuances_wire_rng(g, js.data(), js.size(), qs.data(), qs.size(), &rng, &E.out, E.status.data(), utotal, &cnt)
                             : afx_group_unblind_issuances_wire(g, js.data(), js.size(), qs.data(), qs.size(), dz.data(), &E.out, E.status.data(), utotal, &cnt);
        CHECK(rc == AFX_OK && cnt == utotal && E.all_failed() && E.status[5] == AFX_ST_VERIFICATION_FAILURE);
        Cred F(utotal);
        const int rc2 = drawn ? afx_group_unblind_issuances_wire_rng(g, js.data(), js.size(), qs.data(), qs.size(), &rng, &F.out, F.status.data(), utotal - 1, &cnt)
                              : afx_group_unblind_issuances_wire(g, js.data(), js.size(), qs.data(), qs.size(), dz.data(), &F.out, F.status.data(), utotal - 1, &cnt);
        CHECK(rc2 == AFX_E_BAD_ARGS && F.untouched());
      }
    }
    afx_group_destroy(g);
  }
  afx_ctx_destroy(user);
  printf("blind user doors ok\n");
  return 0;
}
