// TEST INFRASTRUCTURE (CPU only): mutation fuzzer for the host-only entry points that take blind request bytes (AFXQ v1) and blind
// issuance bytes (AFXJ v1), linked with the engine's host sources, statements_blind.cpp, wire_blind.cpp and the fake HIP runtime under
// AddressSanitizer + UBSan by tests/test_blind_wire_fuzz.py.
//   blind_wire_fuzz <dir> <mutations>
// <dir> holds valid streams written by the test from the Python packers: q_a.bin, q_b.bin, q_z.bin (AFXQ sections of two layouts and
// of n = 0), j_a.bin, j_b.bin (AFXJ sections) and mixed.bin (sections of both formats back to back).  Every mutated stream goes
// through both parsers and both section walkers in an EXACT-size heap buffer (an over-read of one byte lands in a red zone); every call
// must return AFX_OK or AFX_E_BAD_ARGS, a walker must never report a section longer than the buffer, and every section a parser
// accepts is transposed to columns and packed again: the packer must write the very bytes that were parsed.
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
static uint64_t rng_state = 0x20191416ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static unsigned long long calls = 0, accepted_q = 0, accepted_j = 0, walked = 0;

static void fail(const char* what, int rc, const uint8_t* p, size_t n) {
  fprintf(stderr, "%s: %d (%s) on a %zu-byte stream starting", what, rc, afx_last_error(), n);
  for (size_t k = 0; k < n && k < 48; k++) fprintf(stderr, " %02x", p[k]);
  fprintf(stderr, "\n");
  exit(1);
}
static bool hidden(uint8_t k) { return k == AFX_ATTR_SECRET_SCALAR || k == AFX_ATTR_SECRET_POINT; }

// records [count][cells][32] at p + off -> rows [cells][count][32]
static Bytes columns(const uint8_t* rec, size_t count, size_t cells) {
  Bytes soa(count * cells * 32 + 1);
  for (size_t i = 0; i < count; i++)
    for (size_t c = 0; c < cells; c++) memcpy(&soa[(c * count + i) * 32], rec + (i * cells + c) * 32, 32);
  return soa;
}
static void repack_request(const uint8_t* p, size_t n, uint32_t na, const uint8_t* kinds, uint32_t nr, size_t count, size_t off) {
  uint32_t h = 0;
  for (uint32_t i = 0; i < na; i++) h += hidden(kinds[i]);
  const size_t cells = 2 + 2 * (size_t)h + nr + (na - h);
  if ((n - off) != count * cells * 32) fail("AFXQ parse accepted a record area of another length", 0, p, n);
  if (count > (size_t(1) << 16)) return;   // (a count no seed stream has: its length could not have matched)
  Bytes soa = columns(p + off, count, cells);
  uint8_t* row = soa.data();
  auto rows = [&](size_t k) { uint8_t* r = row; row += k * count * 32; return r; };
  afx_blind_request_soa q;
  q.D = rows(1); q.A = rows(h); q.B = rows(h); q.challenge = rows(1); q.responses = rows(nr);
  Bytes values((size_t)na * count * 32 + 1, 0xA5);   // the rows of hidden positions: bytes the packer must not read into the blob
  for (uint32_t i = 0; i < na; i++)
    if (!hidden(kinds[i])) memcpy(&values[(size_t)i * count * 32], rows(1), count * 32);
  afx_attributes_soa a;
  memset(&a, 0, sizeof a);
  a.n_attributes = na; memcpy(a.kinds, kinds, na); a.values = values.data();
  size_t len = 0;
  int rc = afx_blind_request_wire_pack(&a, &q, count, nullptr, 0, &len);
  if (rc || len != n) fail("AFXQ size query after an accepted parse", rc, p, n);
  uint8_t* out = (uint8_t*)malloc(len ? len : 1);
  rc = afx_blind_request_wire_pack(&a, &q, count, out, len, &len);
  if (rc || memcmp(out, p, n) != 0) fail("an accepted AFXQ section does not re-pack to itself", rc, p, n);
  free(out);
}
static void repack_issuance(const uint8_t* p, size_t n, uint32_t na, const uint8_t* kinds, uint32_t nr, size_t count, size_t off) {
  const size_t cells = 5 + (size_t)nr;
  if ((n - off) != count * cells * 32) fail("AFXJ parse accepted a record area of another length", 0, p, n);
  if (count > (size_t(1) << 16)) return;
  Bytes soa = columns(p + off, count, cells);
  uint8_t* row = soa.data();
  auto rows = [&](size_t k) { uint8_t* r = row; row += k * count * 32; return r; };
  afx_blind_issuance_soa s;
  s.t = rows(1); s.U = rows(1); s.S1 = rows(1); s.S2 = rows(1); s.challenge = rows(1); s.responses = rows(nr);
  afx_attributes_soa a;
  memset(&a, 0, sizeof a);
  a.n_attributes = na; memcpy(a.kinds, kinds, na);
  size_t len = 0;
  int rc = afx_blind_issuance_wire_pack(&a, &s, nr, count, nullptr, 0, &len);
  if (rc || len != n) fail("AFXJ size query after an accepted parse", rc, p, n);
  uint8_t* out = (uint8_t*)malloc(len ? len : 1);
  rc = afx_blind_issuance_wire_pack(&a, &s, nr, count, out, len, &len);
  if (rc || memcmp(out, p, n) != 0) fail("an accepted AFXJ section does not re-pack to itself", rc, p, n);
  free(out);
}

static void hit(const Bytes& b) {
  const size_t n = b.size();
  uint8_t* p = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(p, b.data(), n);
  size_t cnt = 0, off = 0, sl = 0;
  uint32_t na = 0, nr = 0;
  uint8_t kinds[AFX_MAX_ATTRIBUTES];
  int rc = afx_blind_request_wire_parse(p, n, &na, kinds, &nr, &cnt, &off);
  if (rc != AFX_OK && rc != AFX_E_BAD_ARGS) fail("afx_blind_request_wire_parse", rc, p, n);
  if (rc == AFX_OK) { accepted_q++; repack_request(p, n, na, kinds, nr, cnt, off); }
  rc = afx_blind_issuance_wire_parse(p, n, &na, kinds, &nr, &cnt, &off);
  if (rc != AFX_OK && rc != AFX_E_BAD_ARGS) fail("afx_blind_issuance_wire_parse", rc, p, n);
  if (rc == AFX_OK) { accepted_j++; repack_issuance(p, n, na, kinds, nr, cnt, off); }
  // the walkers, section after section over the whole stream, whichever format each section has
  for (size_t at = 0; at < n;) {
    const int rq = afx_blind_request_wire_section_bytes(p + at, n - at, &sl);
    if (rq != AFX_OK && rq != AFX_E_BAD_ARGS) fail("afx_blind_request_wire_section_bytes", rq, p, n);
    int rj = AFX_E_BAD_ARGS;
    if (rq != AFX_OK) {
      rj = afx_blind_issuance_wire_section_bytes(p + at, n - at, &sl);
      if (rj != AFX_OK && rj != AFX_E_BAD_ARGS) fail("afx_blind_issuance_wire_section_bytes", rj, p, n);
    }
    if (rq != AFX_OK && rj != AFX_OK) break;
    if (sl == 0 || sl > n - at) fail("a walker reported a section that does not fit", 0, p, n);
    // what a walker passes, the parser of its format accepts
    const int rp = rq == AFX_OK ? afx_blind_request_wire_parse(p + at, sl, &na, kinds, &nr, &cnt, &off) : afx_blind_issuance_wire_parse(p + at, sl, &na, kinds, &nr, &cnt, &off);
    if (rp != AFX_OK) fail("a walked section does not parse", rp, p + at, sl);
    walked++;
    at += sl;
  }
  free(p);
  calls++;
}
static void put32(Bytes& b, size_t at, uint32_t v) { for (int k = 0; k < 4 && at + k < b.size(); k++) b[at + k] = (uint8_t)(v >> (8 * k)); }

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string dir = argv[1];
  const unsigned long long target = strtoull(argv[2], nullptr, 10);
  const Bytes QA = rd(dir + "/q_a.bin"), QB = rd(dir + "/q_b.bin"), QZ = rd(dir + "/q_z.bin"), JA = rd(dir + "/j_a.bin"), JB = rd(dir + "/j_b.bin"), M = rd(dir + "/mixed.bin");
  const std::vector<Bytes> seeds = { QA, QB, QZ, JA, JB, M };
  for (const Bytes& g : seeds) hit(g);
  if (accepted_q != 3 || accepted_j != 2 || walked < 5 + 4) { fprintf(stderr, "a valid stream was refused: %llu %llu %llu %s\n", accepted_q, accepted_j, walked, afx_last_error()); return 1; }
  static const uint32_t EDGE[] = { 0, 1, 2, 3, 4, 5, 6, 31, 32, 33, 38, 39, 255, 256, 65535, 65536, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu, 0x04000000u, 0x08000001u };
  unsigned long long m = 0;
  // (1) every header word of every stream gets every edge value; (2) truncations at every 32-byte boundary and one byte either side
  for (const Bytes& g : seeds) {
    const size_t words = g.size() / 4 < 16 ? g.size() / 4 : 16;
    for (size_t w = 0; w < words; w++)
      for (uint32_t v : EDGE) { Bytes b = g; put32(b, 4 * w, v); hit(b); m++; }
    for (size_t cut = 0; cut <= g.size(); cut += 32)
      for (int d = -1; d <= 1; d++) {
        const long long at = (long long)cut + d;
        if (at < 0 || at > (long long)g.size()) continue;
        hit(Bytes(g.begin(), g.begin() + at)); m++;
      }
  }
  // (3) the second section's header inside the mixed stream, and splices: sections dropped, doubled, swapped, cut in the middle
  for (size_t w = 0; w < 8; w++)
    for (uint32_t v : EDGE) { Bytes b = M; put32(b, QA.size() + 4 * w, v); hit(b); m++; }
  const std::vector<Bytes> parts = { QA, JA, QZ, JB, Bytes(QA.begin(), QA.begin() + QA.size() / 2), Bytes(JB.begin(), JB.begin() + 40), Bytes({ 'A', 'F', 'X', 'Q' }),
                                     [] { Bytes x(32, 0); memcpy(x.data(), "AFXJ", 4); x[4] = 1; return x; }() };
  for (const Bytes& x : parts)
    for (const Bytes& y : parts) {
      Bytes b = x; b.insert(b.end(), y.begin(), y.end()); hit(b); m++;
      for (size_t k = 0; k < parts.size(); k += 2) { Bytes c = b; c.insert(c.end(), parts[k].begin(), parts[k].end()); hit(c); m++; }
    }
  // (4) random damage until the target: a few bit flips in the first 96 bytes (header + the start of the records), now and then a
  // random truncation, a field copied from elsewhere in the stream, the other format's magic, or a section appended again
  while (m < target) {
    Bytes b = seeds[rnd() % seeds.size()];
    const size_t span = b.size() < 96 ? b.size() : 96;
    for (int k = 1 + (int)(rnd() % 3); k > 0; k--) { const size_t bit = rnd() % (8 * span); b[bit >> 3] ^= (uint8_t)(1u << (bit & 7)); }
    const unsigned r = (unsigned)(rnd() % 100);
    if (r < 15) b.resize(rnd() % (b.size() + 1));
    else if (r < 25 && b.size() > 8) { const size_t a = rnd() % (b.size() - 4), c = rnd() % (b.size() - 4); memmove(&b[a], &b[c], 4); }
    else if (r < 35) { const Bytes& s = seeds[rnd() % seeds.size()]; b.insert(b.end(), s.begin(), s.end()); }
    else if (r < 40 && b.size() > 4) b[3] = b[3] == 'Q' ? 'J' : 'Q';
    hit(b); m++;
  }
  printf("blind wire fuzz ok: %llu mutated streams, %llu x 4 entry-point calls, %llu AFXQ and %llu AFXJ sections re-packed, %llu sections walked\n", m, calls,
         accepted_q, accepted_j, walked);
  return 0;
}
