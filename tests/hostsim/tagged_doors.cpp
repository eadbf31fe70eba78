// TEST INFRASTRUCTURE (CPU only): the calls of the presentation tags (aeonflux_amd/csrc/statements_tags.cpp and the tagged plans of
// statements_prove.cpp / statements.cpp) on the engine's host half.  tests/test_hostsim_tagged.py links this file with the engine's host
// sources, statements_tags.cpp, the fake HIP runtime and the stand-ins for the masking and tag launchers under AddressSanitizer + UBSan
// and runs it with AFX_PLAN_SELFCHECK=1.
//   tagged_doors <dir>
// <dir> holds params.bin, key.bin and ip.bin of an issuer of 4 attributes, written by the test.  The fake kernels compute nothing, so no
// status is looked at: what is checked is argument errors and what they leave untouched, count 0, a two-pass call, that the inversion
// runs once per call, the job counts a tag adds to a verification plan, and that untagged plans count what they counted before.
// Prints "tagged doors ok" and exits 0, or says which check failed and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/aeonflux_gpu.h"

extern "C" uint64_t fake_tags_launches(int which, int reset);
extern "C" uint64_t fake_tags_inverted_items(void);
extern "C" void fake_tags_last_broadcast(uint8_t out[32]);

typedef std::vector<uint8_t> Bytes;

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
static bool all_are(const Bytes& b, uint8_t v) {
  for (uint8_t x : b)
    if (x != v) return false;
  return true;
}

static const uint32_t N = 4;
static const size_t MAXC = 300;
static const uint8_t KINDS[N] = { AFX_ATTR_SECRET_SCALAR, AFX_ATTR_PUBLIC_SCALAR, AFX_ATTR_PUBLIC_POINT, AFX_ATTR_SECRET_POINT };
static const uint8_t MARK = 0xAB;

// every array of a tagged show and of its verification, sized for MAXC items; outputs carry MARK until something writes them
struct Arrays {
  Bytes in = Bytes(N * MAXC * 64, 0);                // any input: zeros
  Bytes out[24];
  Bytes status = Bytes(MAXC, MARK);
  afx_credentials_soa creds;
  afx_keypairs_soa kp;
  afx_show_randomness rnd;
  afx_encproof_out eo;
  afx_presentation_out po;
  afx_tags_out to;
  afx_encproof_soa es;
  afx_presentation_soa ps;
  afx_tags_soa ts;
  Arrays() {
    for (Bytes& b : out) b.assign(N * MAXC * 32 * 2, MARK);
    memset(&creds, 0, sizeof creds);
    creds.n_attributes = N;
    memcpy(creds.kinds, KINDS, N);
    creds.values = creds.M2 = creds.m3 = creds.t = creds.U = creds.V = in.data();
    kp = { in.data(), in.data(), in.data(), in.data() };
    rnd = { in.data(), in.data(), in.data() };
    eo = { out[0].data(), out[1].data(), out[2].data(), out[3].data(), out[4].data(), out[5].data(), out[6].data(), out[7].data(), out[8].data() };
    po = { out[9].data(), out[10].data(), out[11].data(), out[12].data(), out[13].data(), out[14].data(), out[15].data(), &eo };
    to = { out[16].data(), out[17].data(), out[18].data() };
    es = { out[0].data(), out[1].data(), out[2].data(), out[3].data(), out[4].data(), out[5].data(), out[6].data(), out[7].data(), out[8].data() };
    ps = { out[9].data(), out[10].data(), out[11].data(), out[12].data(), out[13].data(), out[14].data(), out[15].data(), &es };
    ts = { in.data(), out[16].data(), out[17].data(), out[18].data() };
  }
  bool untouched() const {
    for (const Bytes& b : out)
      if (!all_are(b, MARK)) return false;
    return all_are(status, MARK);
  }
};

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: tagged_doors <dir>\n"); return 2; }
  const std::string dir = argv[1];
  const Bytes params = rd(dir + "/params.bin"), key = rd(dir + "/key.bin"), ip = rd(dir + "/ip.bin");
  CHECK(ip.size() == 64);
  afx_ctx *issuer = nullptr, *user = nullptr;
  CHECK(afx_ctx_create(&issuer, 0, params.data(), params.size(), key.data(), key.size(), ip.data()) == AFX_OK);
  CHECK(afx_ctx_create(&user, 0, params.data(), params.size(), nullptr, 0, ip.data()) == AFX_OK);
  CHECK(afx_ctx_n_attributes(issuer) == N);

  Arrays A;
  uint8_t H[32], zeroH[32], ffH[32];
  memcpy(H, params.data() + 4, 32);   // SystemParameters.G: an encoding that decodes
  memset(zeroH, 0, 32);
  memset(ffH, 0xff, 32);
  afx_tag_statement tag = { 0, H };
  afx_shape shape, shape0;
  memset(&shape, 0, sizeof shape);
  uint8_t* const st = A.status.data();
  const uint8_t *nonce = A.in.data(), *seed = A.in.data();

  // ---- null arguments ----
  CHECK(afx_show_tagged(nullptr, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, 4, &A.po, &A.to, &shape, st) == AFX_E_BAD_ARGS);
  CHECK(afx_show_tagged(user, nullptr, &A.kp, &A.rnd, &tag, nonce, seed, 4, &A.po, &A.to, &shape, st) == AFX_E_BAD_ARGS);
  CHECK(afx_show_tagged(user, &A.creds, &A.kp, nullptr, &tag, nonce, seed, 4, &A.po, &A.to, &shape, st) == AFX_E_BAD_ARGS);
  CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, nullptr, nonce, seed, 4, &A.po, &A.to, &shape, st) == AFX_E_BAD_ARGS);
  CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &tag, nullptr, seed, 4, &A.po, &A.to, &shape, st) == AFX_E_BAD_ARGS);
  CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, nullptr, 4, &A.po, &A.to, &shape, st) == AFX_E_BAD_ARGS);
  CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, 4, nullptr, &A.to, &shape, st) == AFX_E_BAD_ARGS);
  CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, 4, &A.po, nullptr, &shape, st) == AFX_E_BAD_ARGS);
  CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, 4, &A.po, &A.to, nullptr, st) == AFX_E_BAD_ARGS);
  CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, 4, &A.po, &A.to, &shape, nullptr) == AFX_E_BAD_ARGS);
  {
    afx_tag_statement no_scope = { 0, nullptr };
    CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &no_scope, nonce, seed, 4, &A.po, &A.to, &shape, st) == AFX_E_BAD_ARGS);
    CHECK(afx_verify_presentations_tagged(issuer, &shape, &A.ps, &no_scope, &A.ts, 4, st) == AFX_E_BAD_ARGS);
    CHECK(afx_verify_tag_proofs(user, &no_scope, A.in.data(), &A.ts, 4, st) == AFX_E_BAD_ARGS);
    afx_tags_out no_T = A.to;
    no_T.T = nullptr;
    CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, 4, &A.po, &no_T, &shape, st) == AFX_E_BAD_ARGS);
    CHECK(afx_show_tagged_dev(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, 4, &A.po, &no_T, &shape, st) == AFX_E_BAD_ARGS);
  }
  CHECK(afx_verify_presentations_tagged(issuer, nullptr, &A.ps, &tag, &A.ts, 4, st) == AFX_E_BAD_ARGS);
  CHECK(afx_verify_presentations_tagged(issuer, &shape, &A.ps, &tag, nullptr, 4, st) == AFX_E_BAD_ARGS);
  CHECK(afx_verify_tag_proofs(user, nullptr, A.in.data(), &A.ts, 4, st) == AFX_E_BAD_ARGS);
  CHECK(afx_verify_tag_proofs(user, &tag, A.in.data(), &A.ts, 4, nullptr) == AFX_E_BAD_ARGS);
  CHECK(afx_verify_tag_proofs(user, &tag, nullptr, &A.ts, 4, st) == AFX_E_BAD_ARGS);
  {
    uint8_t out32[32];
    Bytes scope(1025, 7);
    CHECK(afx_tag_scope_generator(nullptr, scope.data(), 4, out32) == AFX_E_BAD_ARGS);
    CHECK(afx_tag_scope_generator(user, scope.data(), 4, nullptr) == AFX_E_BAD_ARGS);
    CHECK(afx_tag_scope_generator(user, nullptr, 4, out32) == AFX_E_BAD_ARGS);
    CHECK(afx_tag_scope_generator(user, scope.data(), 1025, out32) == AFX_E_BAD_ARGS);
  }
  CHECK(A.untouched());

  // ---- a position that is no hidden scalar of the credentials ----
  for (uint32_t p : { 1u, 2u, 3u, 4u, 64u, 0xffffffffu }) {
    afx_tag_statement bad = { p, H };
    CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &bad, nonce, seed, 4, &A.po, &A.to, &shape, st) == AFX_E_BAD_ARGS);
    CHECK(afx_show_tagged_dev(user, &A.creds, &A.kp, &A.rnd, &bad, nonce, seed, 4, &A.po, &A.to, &shape, st) == AFX_E_BAD_ARGS);
    CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &bad, nonce, seed, 0, &A.po, &A.to, &shape, st) == AFX_E_BAD_ARGS);
  }
  CHECK(A.untouched() && fake_tags_launches(0, 0) == 0 && fake_tags_launches(1, 0) == 0);

  // ---- count 0: nothing runs, the shape is reported ----
  memset(&shape0, 0xEE, sizeof shape0);
  CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, 0, &A.po, &A.to, &shape0, st) == AFX_OK);
  CHECK(shape0.n_attributes == N && shape0.n_hidden_scalars == 1 && shape0.n_enc_proofs == 1 && shape0.kinds[0] == AFX_ENC_SECRET_SCALAR);
  CHECK(afx_show_tagged_dev(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, 0, &A.po, &A.to, &shape, st) == AFX_OK);
  CHECK(memcmp(&shape, &shape0, sizeof shape) == 0);
  CHECK(afx_verify_presentations_tagged(issuer, &shape, &A.ps, &tag, &A.ts, 0, st) == AFX_OK);
  CHECK(afx_verify_presentations_tagged_dev(issuer, &shape, &A.ps, &tag, &A.ts, 0, st) == AFX_OK);
  CHECK(afx_verify_tag_proofs(user, &tag, A.in.data(), &A.ts, 0, st) == AFX_OK);
  CHECK(afx_verify_tag_proofs_dev(user, &tag, A.in.data(), &A.ts, 0, st) == AFX_OK);
  CHECK(A.untouched() && fake_tags_launches(0, 0) == 0 && fake_tags_launches(1, 0) == 0 && fake_tags_launches(2, 0) == 0);

  // ---- a scope generator that is the identity encoding or does not decode: refused, nothing written ----
  for (const uint8_t* bad_H : { (const uint8_t*)zeroH, (const uint8_t*)ffH }) {
    afx_tag_statement bad = { 0, bad_H };
    CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &bad, nonce, seed, 4, &A.po, &A.to, &shape, st) == AFX_E_BAD_ARGS);
    CHECK(afx_verify_presentations_tagged(issuer, &shape, &A.ps, &bad, &A.ts, 4, st) == AFX_E_BAD_ARGS);
    CHECK(afx_verify_tag_proofs(user, &bad, A.in.data(), &A.ts, 4, st) == AFX_E_BAD_ARGS);
    CHECK(A.untouched());
  }
  CHECK(fake_tags_launches(0, 0) == 0 && fake_tags_launches(1, 0) == 0);
  CHECK(fake_tags_launches(2, 1) == 3);   // the three calls that brought 32 bytes of 0xff asked the device; a zero H is refused before that
  CHECK(afx_verify_presentations_tagged(user, &shape, &A.ps, &tag, &A.ts, 4, st) == AFX_E_NO_KEY && A.untouched());

  // ---- small host-pointer calls keep their plans (keys of their own, with the position): the second call of a size reuses the first's,
  // and under AFX_PLAN_SELFCHECK a reused plan must equal a freshly assembled one byte for byte ----
  {
    afx_plan_cache_stats u0, u1, i0, i1;
    CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, 5, &A.po, &A.to, &shape0, st) == AFX_OK);
    CHECK(afx_verify_presentations_tagged(issuer, &shape, &A.ps, &tag, &A.ts, 5, st) == AFX_OK);
    CHECK(afx_verify_tag_proofs(issuer, &tag, A.out[14].data(), &A.ts, 5, st) == AFX_OK);
    CHECK(afx_ctx_get_plan_cache_stats(user, &u0) == AFX_OK && afx_ctx_get_plan_cache_stats(issuer, &i0) == AFX_OK);
    CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, 5, &A.po, &A.to, &shape0, st) == AFX_OK);   // the same size: the same entry
    CHECK(afx_verify_presentations_tagged(issuer, &shape, &A.ps, &tag, &A.ts, 5, st) == AFX_OK);
    CHECK(afx_verify_tag_proofs(issuer, &tag, A.out[14].data(), &A.ts, 5, st) == AFX_OK);
    CHECK(afx_ctx_get_plan_cache_stats(user, &u1) == AFX_OK && afx_ctx_get_plan_cache_stats(issuer, &i1) == AFX_OK);
    CHECK(u1.hits == u0.hits + 1 && u1.misses == u0.misses && i1.hits == i0.hits + 2 && i1.misses == i0.misses);
    // the _dev forms leave no plan behind (their cells of H lie in the lane's buffer, which no relocation knows)
    CHECK(afx_show_tagged_dev(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, 7, &A.po, &A.to, &shape0, st) == AFX_OK);
    CHECK(afx_verify_presentations_tagged_dev(issuer, &shape, &A.ps, &tag, &A.ts, 5, st) == AFX_OK);
    CHECK(afx_ctx_get_plan_cache_stats(user, &u0) == AFX_OK && afx_ctx_get_plan_cache_stats(issuer, &i0) == AFX_OK);
    CHECK(u0.entries == u1.entries && i0.entries == i1.entries && u0.hits == u1.hits && i0.hits == i1.hits);
    (void)fake_tags_launches(0, 1); (void)fake_tags_launches(1, 1); (void)fake_tags_launches(2, 1);
    memset(st, MARK, MAXC);
    for (Bytes& b : A.out) b.assign(b.size(), MARK);
  }

  // ---- untagged plans, before anything tagged has run at their size: what they count ----
  afx_plan_stats show_before, verify_before, show_after, verify_after, tagged;
  CHECK(afx_ctx_set_small_batch_items(issuer, 0) == AFX_OK && afx_ctx_set_small_batch_items(user, 0) == AFX_OK);   // the plan of large passes at any count
  CHECK(afx_show(user, &A.creds, &A.kp, &A.rnd, MAXC, &A.po, &shape0, st) == AFX_OK && afx_ctx_get_plan_stats(user, &show_before) == AFX_OK);
  CHECK(memcmp(&shape, &shape0, sizeof shape) == 0);
  CHECK(afx_verify_presentations(issuer, &shape, &A.ps, MAXC, st) == AFX_OK && afx_ctx_get_plan_stats(issuer, &verify_before) == AFX_OK);

  // ---- a call of two passes: 300 items at 256 per pass; the inversion runs ONCE, in front of them ----
  CHECK(afx_ctx_set_chunk_items(user, 256) == AFX_OK && afx_ctx_set_chunk_items(issuer, 256) == AFX_OK);
  CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, MAXC, &A.po, &A.to, &shape0, st) == AFX_OK);
  CHECK(memcmp(&shape, &shape0, sizeof shape) == 0);
  CHECK(fake_tags_launches(0, 1) == 1 && fake_tags_launches(1, 1) == 1 && fake_tags_launches(2, 1) == 0);   // (the same H as before: remembered)
  CHECK(afx_verify_presentations_tagged(issuer, &shape, &A.ps, &tag, &A.ts, MAXC, st) == AFX_OK);
  CHECK(afx_ctx_get_plan_stats(issuer, &tagged) == AFX_OK);
  CHECK(fake_tags_launches(0, 1) == 0 && fake_tags_launches(1, 1) == 1 && fake_tags_launches(2, 1) == 0);
  CHECK(afx_verify_tag_proofs(issuer, &tag, A.out[14].data(), &A.ts, MAXC, st) == AFX_OK);
  CHECK(fake_tags_launches(1, 1) == 1 && fake_tags_launches(2, 1) == 0);
  {
    // another H: tested once by the context that meets it, then remembered; a bad H is refused by the calls every item fails in, too
    uint8_t H2[32];
    memcpy(H2, params.data() + 4 + 32, 32);   // G_w
    afx_tag_statement tag2 = { 0, H2 }, far_bad = { N, ffH }, far_zero = { N, zeroH }, other_bad = { 1, ffH };
    afx_tags_soa none = { nullptr, nullptr, nullptr, nullptr };
    CHECK(afx_verify_tag_proofs(issuer, &tag2, A.out[14].data(), &A.ts, 9, st) == AFX_OK && fake_tags_launches(2, 1) == 1);
    CHECK(afx_verify_tag_proofs(issuer, &tag2, A.out[14].data(), &A.ts, 9, st) == AFX_OK && fake_tags_launches(2, 1) == 0);
    CHECK(afx_verify_tag_proofs(issuer, &far_bad, nullptr, &none, 9, st) == AFX_E_BAD_ARGS);
    CHECK(afx_verify_tag_proofs(issuer, &far_zero, nullptr, &none, 9, st) == AFX_E_BAD_ARGS);
    CHECK(afx_verify_tag_proofs_dev(issuer, &far_bad, nullptr, &none, 9, st) == AFX_E_BAD_ARGS);
    CHECK(afx_verify_presentations_tagged(issuer, &shape, &A.ps, &other_bad, &none, 9, st) == AFX_E_BAD_ARGS);
    (void)fake_tags_launches(1, 1); (void)fake_tags_launches(2, 1);
  }
  CHECK(afx_show_tagged_dev(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, MAXC, &A.po, &A.to, &shape0, st) == AFX_OK);
  CHECK(afx_verify_presentations_tagged_dev(issuer, &shape, &A.ps, &tag, &A.ts, MAXC, st) == AFX_OK);
  CHECK(afx_verify_tag_proofs_dev(user, &tag, A.out[14].data(), &A.ts, MAXC, st) == AFX_OK);
  CHECK(afx_ctx_set_chunk_items(user, 0) == AFX_OK && afx_ctx_set_chunk_items(issuer, 0) == AFX_OK);
  // one pass, and the shape every item fails on: a position that is no hidden scalar of the SHAPE reads no tag array
  CHECK(afx_show_tagged(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, 70, &A.po, &A.to, &shape0, st) == AFX_OK);
  {
    afx_tag_statement other = { 1, H };
    afx_tags_soa none = { nullptr, nullptr, nullptr, nullptr };
    memset(st, MARK, MAXC);
    CHECK(afx_verify_presentations_tagged(issuer, &shape, &A.ps, &other, &none, 70, st) == AFX_OK);
    for (size_t i = 0; i < 70; i++) CHECK(st[i] == AFX_ST_VERIFICATION_FAILURE);
    afx_tag_statement far = { N, H };
    CHECK(afx_verify_tag_proofs(user, &far, nullptr, &none, 70, st) == AFX_OK);
    for (size_t i = 0; i < 70; i++) CHECK(st[i] == AFX_ST_VERIFICATION_FAILURE);
  }

  // ---- a call that needs a larger tag buffer: the buffer is REPLACED (zeroed, freed, allocated again - the fake runtime hands out zeroed
  // memory, a real one possibly the old address), so the H the lane remembered is gone with it and must be copied again, although the
  // scope is the one the lane has just served.  What the broadcast is given as H says whether it was. ----
  {
    const size_t BIG = 40000;                       // 32 bytes a cell: past the buffer's first megabyte
    Bytes zeros(2 * BIG * 32, 0), big_status(BIG, MARK);
    const afx_tags_soa big = { zeros.data(), zeros.data(), zeros.data(), zeros.data() };
    uint8_t got[32];
    CHECK(afx_verify_tag_proofs_dev(user, &tag, zeros.data(), &big, 8, big_status.data()) == AFX_OK);        // the small buffer holds H
    fake_tags_last_broadcast(got);
    CHECK(memcmp(got, H, 32) == 0);
    CHECK(afx_verify_tag_proofs_dev(user, &tag, zeros.data(), &big, 8, big_status.data()) == AFX_OK);        // resident: nothing copied
    fake_tags_last_broadcast(got);
    CHECK(memcmp(got, H, 32) == 0);
    CHECK(afx_verify_tag_proofs_dev(user, &tag, zeros.data(), &big, BIG, big_status.data()) == AFX_OK);      // the buffer grows
    fake_tags_last_broadcast(got);
    CHECK(memcmp(got, H, 32) == 0);
    CHECK(afx_show_tagged_dev(user, &A.creds, &A.kp, &A.rnd, &tag, nonce, seed, 9, &A.po, &A.to, &shape0, st) == AFX_OK);   // and stays
    fake_tags_last_broadcast(got);
    CHECK(memcmp(got, H, 32) == 0);
    (void)fake_tags_launches(0, 1); (void)fake_tags_launches(1, 1); (void)fake_tags_launches(2, 1);
  }

  // ---- what a tag adds to a verification plan: the fixed-base job that makes C' and exactly two chains ----
  CHECK(tagged.msm_jobs == verify_before.msm_jobs + 3);
  CHECK(tagged.doublings == verify_before.doublings + 2 * 252);
  CHECK(tagged.encodings == verify_before.encodings + 3 && tagged.decodings == verify_before.decodings + 2);
  CHECK(tagged.keccak_permutations > verify_before.keccak_permutations && tagged.secret_terms == verify_before.secret_terms);

  // ---- untagged plans after the tagged calls count exactly what they counted before ----
  CHECK(afx_show(user, &A.creds, &A.kp, &A.rnd, MAXC, &A.po, &shape0, st) == AFX_OK && afx_ctx_get_plan_stats(user, &show_after) == AFX_OK);
  CHECK(afx_verify_presentations(issuer, &shape, &A.ps, MAXC, st) == AFX_OK && afx_ctx_get_plan_stats(issuer, &verify_after) == AFX_OK);
  CHECK(memcmp(&show_before, &show_after, sizeof show_before) == 0 && memcmp(&verify_before, &verify_after, sizeof verify_before) == 0);

  afx_ctx_destroy(user);
  afx_ctx_destroy(issuer);
  printf("tagged doors ok\n");
  return 0;
}
