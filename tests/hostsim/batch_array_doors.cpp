// TEST INFRASTRUCTURE (CPU only): every door that takes the column structs of a presentation, swept array by array from the table that
// describes them (aeonflux_amd/csrc/batch_arrays.hpp).  tests/test_hostsim_batch_arrays.py links this file with the engine's host
// sources, the fake HIP runtime and the stand-in launchers under AddressSanitizer + UBSan and runs it with AFX_PLAN_SELFCHECK=1.
//   batch_array_doors <dir>
// <dir> holds params.bin, key.bin and ip.bin of an issuer of 4 attributes, written by the test.  For three layouts at 3 items and every
// door: the untouched call is AFX_OK; with any ONE array the description says the shape reads set to null it is AFX_E_BAD_ARGS, no plan
// is launched, a host-pointer door copies nothing, and the caller's status bytes stay as they were.  An array added to a table is
// swept without a change here.  Then the converse (an array the shape does not read may be null) and the two packers cell by cell,
// the expectation written out from the format comments of wire.cpp / wire_batchable.cpp, not from the table.
// Prints "batch array doors ok" and exits 0, or says which check failed and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <functional>
#include <list>
#include <string>
#include <vector>
#include "../../aeonflux_amd/csrc/batch_arrays.hpp"

extern "C" unsigned long long afx_fake_count(const char* what, int reset);

typedef std::vector<uint8_t> Bytes;

#define CHECK(cond)                                                                                       \
  do {                                                                                                    \
    if (!(cond)) {                                                                                        \
      fprintf(stderr, "%s:%d: [%s] check failed: %s (last error: %s)\n", __FILE__, __LINE__, g_where.c_str(), #cond, afx_last_error()); \
      exit(1);                                                                                            \
    }                                                                                                     \
  } while (0)
static std::string g_where;

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

static const uint32_t N = 4;
static const size_t COUNT = 3, MAX_ROWS = 8;
static const uint8_t MARK = 0xAB;
static uint8_t g_status[COUNT];
static size_t g_swept = 0;

// one buffer per array, every 32-byte cell (array, row, item) with a pattern of its own
static std::list<Bytes> g_store;
static uint8_t g_next_id = 1;
static uint8_t* new_array() {
  g_store.emplace_back(MAX_ROWS * COUNT * 64);
  Bytes& b = g_store.back();
  for (size_t cell = 0; cell < b.size() / 32; cell++)
    for (size_t j = 0; j < 32; j++) b[cell * 32 + j] = (uint8_t)(j < 2 ? (j ? cell : g_next_id) : g_next_id * 29 + cell * 7 + j);
  g_next_id++;
  return b.data();
}
template <class S> static void fill(S& s) {
  for (size_t k = 0; k < Described<S>::n; k++) array_at(s, Described<S>::cols[k]) = new_array();
}

// `call` with each array of `s` that the shape reads set to null in turn
enum Door { HOST, DEV, PACKER };
template <class S> static void sweep(const char* what, S& s, const Dims& d, Door door, const std::function<int()>& call, size_t from = 0) {
  for (size_t k = from; k < Described<S>::n; k++) {
    const Col& c = Described<S>::cols[k];
    if (!c.read(d)) continue;
    g_where = std::string(what) + ", a struct of " + std::to_string(Described<S>::n) + " arrays, array " + std::to_string(k);
    const ptr_of<S> kept = array_at(s, c);
    array_at(s, c) = nullptr;
    memset(g_status, MARK, COUNT);
    (void)afx_fake_count("copies", 1);
    (void)afx_fake_count("finishes", 1);
    CHECK(call() == AFX_E_BAD_ARGS);
    CHECK(afx_fake_count("finishes", 1) == 0);
    if (door == HOST) CHECK(afx_fake_count("copies", 1) == 0);
    for (size_t i = 0; i < COUNT; i++) CHECK(g_status[i] == MARK);
    array_at(s, c) = kept;
    g_swept++;
  }
  g_where = what;
  CHECK(call() == AFX_OK);
}
// ... and a plain pointer (enc, a commitment array)
template <class P> static void sweep_pointer(const char* what, P& p, Door door, const std::function<int()>& call) {
  g_where = what;
  const P kept = p;
  p = nullptr;
  memset(g_status, MARK, COUNT);
  (void)afx_fake_count("copies", 1);
  (void)afx_fake_count("finishes", 1);
  CHECK(call() == AFX_E_BAD_ARGS);
  CHECK(afx_fake_count("finishes", 1) == 0);
  if (door == HOST) CHECK(afx_fake_count("copies", 1) == 0);
  for (size_t i = 0; i < COUNT; i++) CHECK(g_status[i] == MARK);
  p = kept;
  g_swept++;
  CHECK(call() == AFX_OK);
}

struct Layout {
  afx_credentials_soa creds;
  afx_keypairs_soa kp;
  afx_show_randomness rnd;
  std::vector<afx_encproof_out> eo;
  afx_presentation_out po;
  afx_tags_out to;
  std::vector<afx_encproof_soa> es;
  afx_presentation_soa ps;
  afx_tags_soa ts;
  std::vector<uint8_t*> ce;
  afx_commitments_soa cm;
  afx_shape shape;
  Dims d;
  uint32_t tag_position = 0;
  explicit Layout(afx_ctx* user, const uint8_t kinds[N]) {
    memset(&creds, 0, sizeof creds);
    creds.n_attributes = N;
    memcpy(creds.kinds, kinds, N);
    for (uint32_t i = 0; i < N; i++) if (kinds[i] == AFX_ATTR_SECRET_SCALAR) tag_position = i;
    fill(creds); fill(kp); fill(rnd); fill(po); fill(to); fill(ps); fill(ts);
    d = dims_of(creds);
    eo.resize(d.proofs); es.resize(d.proofs); ce.resize(d.proofs);
    for (uint32_t e = 0; e < d.proofs; e++) { fill(eo[e]); fill(es[e]); ce[e] = new_array(); }
    po.enc = d.proofs ? eo.data() : nullptr;
    ps.enc = d.proofs ? es.data() : nullptr;
    cm.main = new_array();
    cm.enc = d.proofs ? ce.data() : nullptr;
    CHECK(afx_show_dev(user, &creds, &kp, &rnd, 0, &po, &shape, g_status) == AFX_OK);   // (count 0: only the shape is reported)
    const Dims ds = dims_of(shape);
    CHECK(ds.attributes == d.attributes && ds.responses == d.responses && ds.proofs == d.proofs && ds.revealed == d.revealed);
  }
};

static void doors_of(afx_ctx* issuer, afx_ctx* user, Layout& L, const uint8_t* H) {
  const Dims d = L.d;
  uint8_t* const st = g_status;
  afx_tag_statement tag = { L.tag_position, H };
  const uint8_t* nonce = L.ts.nonce;
  const uint8_t* seed = L.rnd.rng_seed;
  afx_shape so;
  afx_device_rng rng = { seed, 0 };
  const uint32_t n_main = afx_batchable_main_commitments(issuer, &L.shape);
  CHECK(n_main >= 2 && n_main <= MAX_ROWS);
  Bytes blob(64 + COUNT * 128 * 32 + 4096);
  size_t len = 0;

  // ---- the verifier's doors ----
  struct V { const char* name; Door door; size_t from; std::function<int()> call; };
  const V verifiers[] = {
    { "afx_verify_presentations", HOST, 0, [&] { return afx_verify_presentations(issuer, &L.shape, &L.ps, COUNT, st); } },
    { "afx_verify_presentations_range", HOST, 0, [&] { return afx_verify_presentations_range(issuer, &L.shape, &L.ps, COUNT, 0, COUNT, st); } },
    { "afx_verify_presentations_dev", DEV, 0, [&] { return afx_verify_presentations_dev(issuer, &L.shape, &L.ps, COUNT, st); } },
    { "afx_verify_presentations_tagged", HOST, 0, [&] { return afx_verify_presentations_tagged(issuer, &L.shape, &L.ps, &tag, &L.ts, COUNT, st); } },
    { "afx_verify_presentations_tagged_dev", DEV, 0, [&] { return afx_verify_presentations_tagged_dev(issuer, &L.shape, &L.ps, &tag, &L.ts, COUNT, st); } },
    { "afx_verify_presentations_batchable", HOST, NO_CHALLENGE, [&] { return afx_verify_presentations_batchable(issuer, &L.shape, &L.ps, &L.cm, &rng, COUNT, st); } },
    { "afx_verify_presentations_batchable_dev", DEV, NO_CHALLENGE, [&] { return afx_verify_presentations_batchable_dev(issuer, &L.shape, &L.ps, &L.cm, &rng, COUNT, st); } },
    { "afx_wire_pack_presentations", PACKER, 0, [&] { return afx_wire_pack_presentations(&L.shape, &L.ps, COUNT, blob.data(), blob.size(), &len); } },
    { "afx_batchable_wire_pack", PACKER, NO_CHALLENGE, [&] { return afx_batchable_wire_pack(&L.shape, &L.ps, &L.cm, n_main, COUNT, blob.data(), blob.size(), &len); } },
  };
  for (const V& v : verifiers) {
    sweep(v.name, L.ps, d, v.door, v.call, v.from);
    for (uint32_t e = 0; e < d.proofs; e++) sweep(v.name, L.es[e], d, v.door, v.call, v.from);
    if (d.proofs) sweep_pointer(v.name, L.ps.enc, v.door, v.call);
    if (strstr(v.name, "tagged")) sweep(v.name, L.ts, d, v.door, v.call);
    if (strstr(v.name, "batchable")) {
      sweep_pointer(v.name, L.cm.main, v.door, v.call);
      for (uint32_t e = 0; e < d.proofs; e++) sweep_pointer(v.name, L.ce[e], v.door, v.call);
      if (d.proofs) sweep_pointer(v.name, L.cm.enc, v.door, v.call);
    }
  }
  {
    afx_encproof_soa one;
    fill(one);
    sweep("afx_verify_encryption_proofs", one, d, HOST, [&] { return afx_verify_encryption_proofs(issuer, 3, &one, COUNT, st); });
    sweep("afx_verify_encryption_proofs_dev", one, d, DEV, [&] { return afx_verify_encryption_proofs_dev(issuer, 3, &one, COUNT, st); });
    // an index the parameters do not have: every item fails, no array is read
    afx_encproof_soa none;
    memset(&none, 0, sizeof none);
    g_where = "afx_verify_encryption_proofs, index >= n";
    CHECK(afx_verify_encryption_proofs_dev(issuer, N, &none, COUNT, st) == AFX_OK);
  }

  // ---- the prover's doors: inputs (keypairs present) and outputs ----
  struct S { const char* name; std::function<int()> call; };
  const S shows[] = {
    { "afx_show", [&] { return afx_show(user, &L.creds, &L.kp, &L.rnd, COUNT, &L.po, &so, st); } },
    { "afx_show_batchable", [&] { return afx_show_batchable(user, &L.creds, &L.kp, &L.rnd, COUNT, &L.po, &L.cm, &so, st); } },
    { "afx_show_tagged", [&] { return afx_show_tagged(user, &L.creds, &L.kp, &L.rnd, &tag, nonce, seed, COUNT, &L.po, &L.to, &so, st); } },
  };
  for (const S& s : shows) {
    sweep(s.name, L.creds, d, HOST, s.call);
    sweep(s.name, L.rnd, d, HOST, s.call);
    if (d.proofs) sweep(s.name, L.kp, d, HOST, s.call);
    sweep(s.name, L.po, outputs(d), HOST, s.call);
    for (uint32_t e = 0; e < d.proofs; e++) sweep(s.name, L.eo[e], d, HOST, s.call);
    if (d.proofs) sweep_pointer(s.name, L.po.enc, HOST, s.call);
    if (strstr(s.name, "tagged")) sweep(s.name, L.to, d, HOST, s.call);
    if (strstr(s.name, "batchable")) {
      sweep_pointer(s.name, L.cm.main, HOST, s.call);
      for (uint32_t e = 0; e < d.proofs; e++) sweep_pointer(s.name, L.ce[e], HOST, s.call);
    }
    // an output's attr_values is the caller's choice
    g_where = std::string(s.name) + ", no attr_values";
    uint8_t* const av = L.po.attr_values;
    L.po.attr_values = nullptr;
    CHECK(s.call() == AFX_OK);
    L.po.attr_values = av;
  }
}

// what a record must hold, written out from the format comments: AFXP (wire.cpp, include/aeonflux_gpu.h "wire format")
//   challenge | responses[n_responses] | C_x_0 | C_x_1 | C_V | C_y[n_attributes] | value of every revealed attribute, in position order
//   | per proof of encryption: challenge | responses[6] | pk | E1 | E2 | C_y_1 | C_y_2 | C_y_3 | C_y_2'
// and AFXB (wire_batchable.cpp): the same with R[n_main] in the main challenge's place and R[5] in each proof's
struct Cell { const uint8_t* array; uint32_t row; };
static std::vector<Cell> expected_cells(const Layout& L, bool batchable, uint32_t n_main) {
  std::vector<Cell> c;
  auto rows = [&](const uint8_t* a, uint32_t k) { for (uint32_t r = 0; r < k; r++) c.push_back({ a, r }); };
  const afx_shape& sh = L.shape;
  if (batchable) rows(L.cm.main, n_main); else rows(L.ps.challenge, 1);
  rows(L.ps.responses, sh.n_responses); rows(L.ps.C_x_0, 1); rows(L.ps.C_x_1, 1); rows(L.ps.C_V, 1); rows(L.ps.C_y, sh.n_attributes);
  for (uint32_t i = 0; i < sh.n_attributes; i++)
    if (sh.kinds[i] == AFX_ENC_PUBLIC_SCALAR || sh.kinds[i] == AFX_ENC_PUBLIC_POINT) c.push_back({ L.ps.attr_values, i });
  for (uint32_t e = 0; e < sh.n_enc_proofs; e++) {
    const afx_encproof_soa& q = L.es[e];
    if (batchable) rows(L.ce[e], 5); else rows(q.challenge, 1);
    rows(q.responses, 6); rows(q.pk, 1); rows(q.E1, 1); rows(q.E2, 1); rows(q.C_y_1, 1); rows(q.C_y_2, 1); rows(q.C_y_3, 1); rows(q.C_y_2p, 1);
  }
  return c;
}
static void round_trip(afx_ctx* issuer, const Layout& L) {
  for (int batchable = 0; batchable < 2; batchable++) {
    g_where = batchable ? "AFXB round trip" : "AFXP round trip";
    const uint32_t n_main = afx_batchable_main_commitments(issuer, &L.shape);
    const std::vector<Cell> want = expected_cells(L, batchable, n_main);
    const size_t hdr = batchable ? afx_batchable_wire_header_bytes(&L.shape) : afx_wire_header_bytes(&L.shape);
    const uint32_t cells = batchable ? afx_batchable_wire_cells_per_record(&L.shape, n_main) : afx_wire_cells_per_record(&L.shape);
    CHECK(hdr && cells == want.size());
    Bytes blob(hdr + COUNT * cells * 32, MARK);
    size_t len = 0;
    if (batchable) CHECK(afx_batchable_wire_pack(&L.shape, &L.ps, &L.cm, n_main, COUNT, blob.data(), blob.size(), &len) == AFX_OK);
    else CHECK(afx_wire_pack_presentations(&L.shape, &L.ps, COUNT, blob.data(), blob.size(), &len) == AFX_OK);
    CHECK(len == blob.size());
    for (size_t i = 0; i < COUNT; i++)
      for (uint32_t k = 0; k < cells; k++)
        CHECK(memcmp(blob.data() + hdr + (i * cells + k) * 32, want[k].array + ((size_t)want[k].row * COUNT + i) * 32, 32) == 0);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: batch_array_doors <dir>\n"); return 2; }
  const std::string dir = argv[1];
  const Bytes params = rd(dir + "/params.bin"), key = rd(dir + "/key.bin"), ip = rd(dir + "/ip.bin");
  afx_ctx *issuer = nullptr, *user = nullptr;
  CHECK(afx_ctx_create(&issuer, 0, params.data(), params.size(), key.data(), key.size(), ip.data()) == AFX_OK);
  CHECK(afx_ctx_create(&user, 0, params.data(), params.size(), nullptr, 0, ip.data()) == AFX_OK);
  CHECK(afx_ctx_n_attributes(issuer) == N);
  uint8_t H[32];
  memcpy(H, params.data() + 4, 32);   // SystemParameters.G: an encoding that decodes

  // one of each kind; no hidden group element (enc null); two hidden group elements
  const uint8_t KINDS[3][N] = { { AFX_ATTR_PUBLIC_SCALAR, AFX_ATTR_PUBLIC_POINT, AFX_ATTR_SECRET_SCALAR, AFX_ATTR_SECRET_POINT },
                                { AFX_ATTR_PUBLIC_SCALAR, AFX_ATTR_PUBLIC_POINT, AFX_ATTR_SECRET_SCALAR, AFX_ATTR_SECRET_SCALAR },
                                { AFX_ATTR_PUBLIC_SCALAR, AFX_ATTR_SECRET_SCALAR, AFX_ATTR_SECRET_POINT, AFX_ATTR_SECRET_POINT } };
  for (int l = 0; l < 3; l++) {
    Layout L(user, KINDS[l]);
    CHECK(L.d.proofs == (l == 0 ? 1u : l == 1 ? 0u : 2u) && (L.ps.enc == nullptr) == (l == 1));
    const size_t before = g_swept;
    doors_of(issuer, user, L, H);
    CHECK(g_swept - before > 50);
    if (l != 1) round_trip(issuer, L);
    if (l == 1) {
      // keypairs are read only with a hidden group element: absent, or a struct of null arrays
      afx_shape so;
      afx_keypairs_soa none = { nullptr, nullptr, nullptr, nullptr };
      g_where = "keypairs without a hidden group element";
      CHECK(afx_show(user, &L.creds, nullptr, &L.rnd, COUNT, &L.po, &so, g_status) == AFX_OK);
      CHECK(afx_show(user, &L.creds, &none, &L.rnd, COUNT, &L.po, &so, g_status) == AFX_OK);
    }
  }
  {
    // nothing revealed: attr_values may be null at every verifier's door and both packers
    const uint8_t hidden[N] = { AFX_ATTR_SECRET_SCALAR, AFX_ATTR_SECRET_SCALAR, AFX_ATTR_SECRET_SCALAR, AFX_ATTR_SECRET_POINT };
    Layout L(user, hidden);
    g_where = "attr_values with nothing revealed";
    CHECK(L.d.revealed == 0);
    L.ps.attr_values = nullptr;
    afx_tag_statement tag = { L.tag_position, H };
    afx_device_rng rng = { L.rnd.rng_seed, 0 };
    const uint32_t n_main = afx_batchable_main_commitments(issuer, &L.shape);
    Bytes blob(1 << 16);
    size_t len = 0;
    CHECK(afx_verify_presentations(issuer, &L.shape, &L.ps, COUNT, g_status) == AFX_OK);
    CHECK(afx_verify_presentations_dev(issuer, &L.shape, &L.ps, COUNT, g_status) == AFX_OK);
    CHECK(afx_verify_presentations_tagged(issuer, &L.shape, &L.ps, &tag, &L.ts, COUNT, g_status) == AFX_OK);
    CHECK(afx_verify_presentations_batchable(issuer, &L.shape, &L.ps, &L.cm, &rng, COUNT, g_status) == AFX_OK);
    CHECK(afx_wire_pack_presentations(&L.shape, &L.ps, COUNT, blob.data(), blob.size(), &len) == AFX_OK);
    CHECK(afx_batchable_wire_pack(&L.shape, &L.ps, &L.cm, n_main, COUNT, blob.data(), blob.size(), &len) == AFX_OK);
    // C_y and responses at zero rows, enc at zero proofs: the packers read none of them
    afx_shape empty;
    memset(&empty, 0, sizeof empty);
    afx_presentation_soa bare = L.ps;
    bare.C_y = bare.responses = nullptr;
    bare.enc = nullptr;
    g_where = "C_y / responses at zero rows";
    CHECK(afx_wire_pack_presentations(&empty, &bare, COUNT, blob.data(), blob.size(), &len) == AFX_OK);
  }
  afx_ctx_destroy(user);
  afx_ctx_destroy(issuer);
  printf("batch array doors ok (%zu null arrays swept)\n", g_swept);
  return 0;
}
