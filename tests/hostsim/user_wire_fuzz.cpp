// TEST INFRASTRUCTURE (CPU only): mutation fuzzer for the user side on bytes - afx_issuance_wire_section_bytes,
// afx_verify_issuances_mixed_wire and afx_show_wire - linked with the engine's host sources, wire_issue.cpp, wire_user.cpp and the fake
// HIP runtime (fake_hip.cpp, fake_wire_issue.cpp) under AddressSanitizer + UBSan by tests/test_user_wire_fuzz.py.
//   user_wire_fuzz <dir> <mutations>
// <dir> holds params.bin and ip.bin (n = 4; a user context: no key) and the valid AFXI streams a.afxi (one section of the context's
// layout), b.afxi (another layout), m.afxi (n = 3), z.afxi (count 0) and mixed.afxi (several sections) written by the test.  Every
// mutated stream goes through the section measure and the stream verification in EXACT-size heap buffers (an over-read of one byte
// lands in a red zone), with a status buffer of the reported size and one byte short; then afx_show_wire gets size queries of every
// layout, full calls and damaged positions.  Every call must return AFX_OK or AFX_E_BAD_ARGS.
// Before any of that, on a context of its own: afx_verify_issuances_wire and afx_verify_issuances_mixed_wire stage one section alike -
// the plan the first call assembles serves the second call and the stream's (shared_plan_cache).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/aeonflux_gpu.h"

typedef std::vector<uint8_t> Bytes;
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
static uint64_t rng_state = 0x20261016ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static afx_ctx* ctx;
static unsigned long long calls = 0, accepted = 0;

static void fail(const char* which, int rc, const uint8_t* p, size_t n) {
  fprintf(stderr, "%s returned %d (%s) on %zu bytes starting", which, rc, afx_last_error(), n);
  for (size_t k = 0; k < n && k < 48; k++) fprintf(stderr, " %02x", p[k]);
  fprintf(stderr, "\n");
  exit(1);
}
static void hit(const Bytes& b) {
  const size_t n = b.size();
  uint8_t* p = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(p, b.data(), n);
  size_t sl = 0, cnt = 0;
  int rc = afx_issuance_wire_section_bytes(p, n, &sl);
  if (rc != AFX_OK && rc != AFX_E_BAD_ARGS) fail("section_bytes", rc, p, n);
  if (rc == AFX_OK && (sl > n || sl < 24)) { fprintf(stderr, "section of %zu bytes in a %zu-byte blob\n", sl, n); exit(1); }
  // a status buffer of the item count the stream claims (bounded), and one byte short of it, which must be refused untouched
  rc = afx_verify_issuances_mixed_wire(ctx, p, n, nullptr, 0, &cnt);
  if (rc != AFX_OK && rc != AFX_E_BAD_ARGS) fail("verify_issuances_mixed_wire (no status)", rc, p, n);
  if (rc == AFX_E_BAD_ARGS && cnt > 0 && cnt <= (size_t(1) << 16)) {
    uint8_t* st = (uint8_t*)malloc(cnt);
    memset(st, 0xEE, cnt);
    rc = afx_verify_issuances_mixed_wire(ctx, p, n, st, cnt - 1, &cnt);
    if (rc != AFX_E_BAD_ARGS) fail("verify_issuances_mixed_wire (short status)", rc, p, n);
    for (size_t i = 0; i + 1 < cnt; i++)
      if (st[i] != 0xEE) { fprintf(stderr, "a refused call wrote a status\n"); exit(1); }
    rc = afx_verify_issuances_mixed_wire(ctx, p, n, st, cnt, &cnt);
    if (rc != AFX_OK && rc != AFX_E_BAD_ARGS) fail("verify_issuances_mixed_wire", rc, p, n);
    accepted += rc == AFX_OK;
    free(st);
  } else if (rc == AFX_OK) {
    accepted++;   // (an empty stream)
  }
  free(p);
  calls++;
}
static void put32(Bytes& b, size_t at, uint32_t v) { for (int k = 0; k < 4 && at + k < b.size(); k++) b[at + k] = (uint8_t)(v >> (8 * k)); }

// ---- afx_show_wire -------------------------------------------------------------------------------------------------------------
struct ShowData {   // random bytes in every array a group of `count` credentials of n attributes reads (the fake runtime computes nothing)
  Bytes values, M2, m3, t, U, V, z, seed, es, a, a0, a1, pk;
  afx_keypairs_soa kp;
  ShowData(size_t n, size_t count, size_t nsp) {
    auto fill = [](Bytes& b, size_t len) { b.resize(len ? len : 1); for (uint8_t& x : b) x = (uint8_t)rnd(); };
    fill(values, n * count * 32); fill(M2, n * count * 32); fill(m3, n * count * 32);
    fill(t, count * 32); fill(U, count * 32); fill(V, count * 32); fill(z, count * 64); fill(seed, count * 32); fill(es, nsp * count * 32);
    fill(a, count * 32); fill(a0, count * 32); fill(a1, count * 32); fill(pk, count * 32);
    kp = { a.data(), a0.data(), a1.data(), pk.data() };
  }
  afx_show_group group(const uint8_t* kinds, uint32_t n, size_t count, bool keys) {
    afx_show_group g;
    memset(&g, 0, sizeof g);   // (`out` is not read: left zeroed)
    g.creds.n_attributes = n;
    memcpy(g.creds.kinds, kinds, n < AFX_MAX_ATTRIBUTES ? n : AFX_MAX_ATTRIBUTES);
    g.creds.values = values.data(); g.creds.M2 = M2.data(); g.creds.m3 = m3.data(); g.creds.t = t.data(); g.creds.U = U.data(); g.creds.V = V.data();
    g.keypairs = keys ? &kp : nullptr;
    g.rnd = { z.data(), seed.data(), es.data() };
    g.count = count;
    return g;
  }
};

static void show_cases(unsigned long long target, unsigned long long& m) {
  static const uint8_t L0[4] = { 1, 0, 2, 4 }, L1[4] = { 3, 3, 1, 1 }, L2[2] = { 4, 4 }, L3[1] = { 2 }, BADK[4] = { 1, 5, 0, 0 };
  ShowData d4(4, 40, 1), d2(2, 40, 2), d1(1, 40, 0);
  size_t len = 0;
  // size queries: every layout afx_show takes, and the ones it refuses (n = 0, n above the context's, a kind out of range)
  for (uint32_t n = 0; n <= 6; n++)
    for (int k = 0; k < 6; k++) {
      uint8_t kinds[AFX_MAX_ATTRIBUTES] = { 0 };
      for (uint32_t i = 0; i < n; i++) kinds[i] = (uint8_t)((k + i) % 6);
      afx_show_group g = d4.group(kinds, n, 3, true);
      g.rnd = { nullptr, nullptr, nullptr };   // (the size query reads no arrays)
      const int rc = afx_show_wire(ctx, &g, 1, nullptr, 0, &len, nullptr, 0);
      bool layout_ok = n >= 1 && n <= 4;
      for (uint32_t i = 0; i < n; i++) layout_ok &= kinds[i] <= AFX_ATTR_SECRET_POINT;
      if (rc != (layout_ok ? AFX_OK : AFX_E_BAD_ARGS)) fail("show_wire size query", rc, kinds, n);
      m++;
    }
  afx_show_group bad = d4.group(BADK, 4, 3, true);
  if (afx_show_wire(ctx, &bad, 1, nullptr, 0, &len, nullptr, 0) != AFX_E_BAD_ARGS) { fprintf(stderr, "a kind out of range was accepted\n"); exit(1); }
  // full calls: several groups (one without keypairs, one of count 0), positions permuted, given and damaged, buffers exact and short
  while (m < target) {
    const size_t c0 = 1 + rnd() % 20, c1 = rnd() % 6, c2 = 1 + rnd() % 4, c3 = 1 + rnd() % 3;
    afx_show_group g[4] = { d4.group(L0, 4, c0, true), d4.group(L1, 4, c1, true), d2.group(L2, 2, c2, (rnd() & 1) != 0), d1.group(L3, 1, c3, false) };
    const size_t total = c0 + c1 + c2 + c3;
    std::vector<uint64_t> perm(total);
    for (size_t i = 0; i < total; i++) perm[i] = i;
    for (size_t i = total; i > 1; i--) std::swap(perm[i - 1], perm[rnd() % i]);
    const unsigned how = (unsigned)(rnd() % 8);
    size_t at = 0;
    for (int k = 0; k < 4; k++) { if (how & 1) g[k].positions = perm.data() + at; at += g[k].count; }
    std::vector<uint64_t> damaged;
    if (how == 3 || how == 5) {   // a position out of range or used twice
      damaged = perm;
      damaged[rnd() % total] = how == 3 ? total + (rnd() % 3) : damaged[(rnd() % total)];
      at = 0;
      for (int k = 0; k < 4; k++) { g[k].positions = damaged.data() + at; at += g[k].count; }
    }
    const size_t ng = 1 + rnd() % 4;
    size_t need = 0;
    int rc = afx_show_wire(ctx, g, ng, nullptr, 0, &need, nullptr, 0);
    if (rc != AFX_OK) fail("show_wire size query of valid groups", rc, nullptr, 0);
    size_t items = 0;
    for (size_t k = 0; k < ng; k++) items += g[k].count;
    const bool short_out = rnd() % 6 == 0, short_st = rnd() % 6 == 0;
    const size_t cap = short_out ? need - 1 : need, slen = g[0].positions ? (short_st ? total - 1 : total) : (short_st ? items - 1 : items);
    uint8_t* out = (uint8_t*)malloc(cap);
    uint8_t* st = (uint8_t*)malloc(slen ? slen : 1);
    memset(out, 0xEE, cap);
    memset(st, 0xEE, slen ? slen : 1);
    rc = afx_show_wire(ctx, g, ng, out, cap, &len, st, slen);
    if (rc != AFX_OK && rc != AFX_E_BAD_ARGS) fail("show_wire", rc, nullptr, 0);
    if (rc == AFX_OK && (short_out || len != need)) { fprintf(stderr, "show_wire accepted a short output buffer\n"); exit(1); }
    if (rc != AFX_OK) {
      for (size_t i = 0; i < cap; i++) if (out[i] != 0xEE) { fprintf(stderr, "a refused show_wire wrote output\n"); exit(1); }
      for (size_t i = 0; i < slen; i++) if (st[i] != 0xEE) { fprintf(stderr, "a refused show_wire wrote a status\n"); exit(1); }
    } else if (memcmp(out, "AFXP", 4) != 0) {
      fprintf(stderr, "show_wire output does not start with a section\n");
      exit(1);
    }
    accepted += rc == AFX_OK;
    free(out);
    free(st);
    calls++;
    m++;
  }
}

// One 3-item AFXI section of 2 attributes (n_responses = the context's n + 5: a layout the stream verifies on the device) through
// afx_verify_issuances_wire twice, then through afx_verify_issuances_mixed_wire: the second and the third call take the first call's
// plans from the cache - hits and not one miss - because both entry points stage the section in one function (wire.cpp verify_records).
static void shared_plan_cache(const Bytes& params, const Bytes& ip) {
  afx_ctx* c = nullptr;
  if (afx_ctx_create(&c, 0, params.data(), params.size(), nullptr, 0, ip.data())) { fprintf(stderr, "ctx: %s\n", afx_last_error()); exit(2); }
  afx_ctx_set_coalescing(c, 0, 0);
  const size_t count = 3;
  const uint32_t n = 2, nr = afx_ctx_n_attributes(c) + 5;
  afx_attributes_soa at;
  memset(&at, 0, sizeof at);
  at.n_attributes = n; at.kinds[0] = AFX_ATTR_PUBLIC_SCALAR; at.kinds[1] = AFX_ATTR_PUBLIC_POINT;
  Bytes values(n * count * 32), t(count * 32), U(count * 32), V(count * 32), ch(count * 32), resp(nr * count * 32);
  for (Bytes* b : { &values, &t, &U, &V, &ch, &resp }) for (uint8_t& x : *b) x = (uint8_t)rnd();
  at.values = values.data();
  const afx_issuance_soa iss = { t.data(), U.data(), V.data(), ch.data(), resp.data() };
  size_t len = 0;
  if (afx_issuance_wire_pack(&at, &iss, nr, count, nullptr, 0, &len)) { fprintf(stderr, "pack: %s\n", afx_last_error()); exit(1); }
  Bytes blob(len);
  if (afx_issuance_wire_pack(&at, &iss, nr, count, blob.data(), blob.size(), &len)) { fprintf(stderr, "pack: %s\n", afx_last_error()); exit(1); }
  afx_plan_cache_stats s[4];
  uint8_t st[3];
  size_t cnt = 0;
  afx_ctx_get_plan_cache_stats(c, &s[0]);
  for (int k = 1; k <= 3; k++) {
    const int rc = k < 3 ? afx_verify_issuances_wire(c, blob.data(), blob.size(), st, sizeof st, &cnt) : afx_verify_issuances_mixed_wire(c, blob.data(), blob.size(), st, sizeof st, &cnt);
    if (rc || cnt != count) { fprintf(stderr, "shared plan cache: call %d returned %d (%s), %zu items\n", k, rc, afx_last_error(), cnt); exit(1); }
    afx_ctx_get_plan_cache_stats(c, &s[k]);
  }
  fprintf(stderr, "shared plan cache: hits %llu %llu %llu %llu, misses %llu %llu %llu %llu\n", (unsigned long long)s[0].hits, (unsigned long long)s[1].hits,
          (unsigned long long)s[2].hits, (unsigned long long)s[3].hits, (unsigned long long)s[0].misses, (unsigned long long)s[1].misses,
          (unsigned long long)s[2].misses, (unsigned long long)s[3].misses);
  if (s[1].misses <= s[0].misses) { fprintf(stderr, "shared plan cache: the first call assembled nothing\n"); exit(1); }
  for (int k = 2; k <= 3; k++)
    if (s[k].hits <= s[k - 1].hits || s[k].misses != s[k - 1].misses) { fprintf(stderr, "shared plan cache: call %d did not run on the first call's plans\n", k); exit(1); }
  afx_ctx_destroy(c);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string dir = argv[1];
  const unsigned long long target = strtoull(argv[2], nullptr, 10);
  const Bytes params = rd(dir + "/params.bin"), ip = rd(dir + "/ip.bin");
  if (afx_ctx_create(&ctx, 0, params.data(), params.size(), nullptr, 0, ip.data())) { fprintf(stderr, "ctx: %s\n", afx_last_error()); return 2; }
  afx_ctx_set_coalescing(ctx, 0, 0);   // (one thread: nothing to collect)
  shared_plan_cache(params, ip);
  const Bytes A = rd(dir + "/a.afxi"), B = rd(dir + "/b.afxi"), M3 = rd(dir + "/m.afxi"), Z = rd(dir + "/z.afxi"), X = rd(dir + "/mixed.afxi");
  const std::vector<Bytes> seeds = { A, B, M3, Z, X };
  for (const Bytes& g : seeds) hit(g);
  hit(Bytes());
  if (accepted != seeds.size() + 1) { fprintf(stderr, "a valid stream was refused: %s\n", afx_last_error()); return 1; }
  static const uint32_t EDGE[] = { 0, 1, 2, 3, 4, 5, 9, 13, 17, 31, 32, 33, 37, 38, 255, 256, 65535, 65536, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu, 0x04000000u };
  unsigned long long m = 0;
  // (1) every header word of every stream gets every edge value; (2) truncation at every byte
  for (const Bytes& g : seeds) {
    const size_t words = g.size() / 4 < 16 ? g.size() / 4 : 16;
    for (size_t w = 0; w < words; w++)
      for (uint32_t v : EDGE) { Bytes b = g; put32(b, 4 * w, v); hit(b); m++; }
    for (size_t cut = 0; cut <= g.size(); cut++) { hit(Bytes(g.begin(), g.begin() + cut)); m++; }
  }
  // (3) the second section's header inside the mixed stream, and splices of whole and cut sections
  for (size_t w = 0; w < 8; w++)
    for (uint32_t v : EDGE) { Bytes b = X; put32(b, A.size() + 4 * w, v); hit(b); m++; }
  const std::vector<Bytes> parts = { A, B, Z, M3, Bytes(A.begin(), A.begin() + A.size() / 2), Bytes(B.begin(), B.begin() + 40), Bytes({ 'A', 'F', 'X', 'I' }),
                                     [] { Bytes x(32, 0); memcpy(x.data(), "AFXP", 4); x[4] = 1; return x; }() };
  for (const Bytes& x : parts)
    for (const Bytes& y : parts) { Bytes b = x; b.insert(b.end(), y.begin(), y.end()); hit(b); m++; }
  // (4) random damage: bit flips in the first 96 bytes, now and then a truncation, a field copied from elsewhere, a section appended
  const unsigned long long stream_target = m + target;
  while (m < stream_target) {
    Bytes b = seeds[rnd() % seeds.size()];
    const size_t span = b.size() < 96 ? b.size() : 96;
    for (int k = 1 + (int)(rnd() % 3); k > 0 && span; k--) { const size_t bit = rnd() % (8 * span); b[bit >> 3] ^= (uint8_t)(1u << (bit & 7)); }
    const unsigned r = (unsigned)(rnd() % 100);
    if (r < 15) b.resize(rnd() % (b.size() + 1));
    else if (r < 25 && b.size() > 8) { const size_t a = rnd() % (b.size() - 4), c = rnd() % (b.size() - 4); memmove(&b[a], &b[c], 4); }
    else if (r < 35) { const Bytes& s = seeds[rnd() % seeds.size()]; b.insert(b.end(), s.begin(), s.end()); }
    hit(b); m++;
  }
  const unsigned long long streams = m, stream_accepted = accepted;
  accepted = 0;
  unsigned long long shows = 0;
  show_cases(target / 4 + 40, shows);
  afx_ctx_destroy(ctx);
  printf("user wire fuzz ok: %llu streams (%llu accepted), %llu show_wire cases (%llu full calls accepted), %llu calls\n", streams, stream_accepted, shows,
         accepted, calls);
  return 0;
}
