// TEST INFRASTRUCTURE (CPU only): the host half of the spent-tag set (aeonflux_amd/csrc/tagset.cpp) - the bound arithmetic and
// AFX_E_FULL, the refresh from the table's two words, the scratch layout of the host-pointer forms, the order of calls over the two
// pipelining lanes, and the `broken` state, which no GPU test can reach without provoking a fault.  tests/test_hostsim_tagset.py links
// this file with the engine's host sources, tagset.cpp, the fake HIP runtime and tests/hostsim/fake_tagset.cpp under AddressSanitizer
// and UBSan.  The stand-in launchers run the real lane bodies, so whole calls are compared with a std::set loop here.
//   tagset_doors <dir> SCENARIO...
// <dir> holds params.bin and ip.bin of any issuer, written by the test; a SCENARIO is the text tests/hostsim/tagset_host.cpp reads
// (set / call / contains).  Every scenario runs through afx_tagset_spend and afx_tagset_contains on one set and through the _dev forms
// on another, under both pipelining settings; the answers of the first run are printed ("seen <digits>" per call, "has <digits>" per
// lookup) for the test to compare with its own model.  Prints "tagset doors ok" and exits 0, or says which check failed and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fstream>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>
#include "../../include/aeonflux_gpu.h"

extern "C" void fake_tagset_set(const char* what, int v);
extern "C" uint64_t fake_tagset_launches(int which);

typedef std::vector<uint8_t> Bytes;
typedef std::vector<Bytes> Tags;

#define CHECK(cond)                                                                                       \
  do {                                                                                                    \
    if (!(cond)) {                                                                                        \
      fprintf(stderr, "%s:%d: check failed: %s (last error: %s)\n", __FILE__, __LINE__, #cond, afx_last_error()); \
      exit(1);                                                                                            \
    }                                                                                                     \
  } while (0)

static const uint8_t MARK = 0xEE;

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
static bool unhex(const std::string& h, uint8_t* out, size_t n) {
  if (h.size() != 2 * n) return false;
  for (size_t i = 0; i < n; i++) {
    unsigned v = 0;
    if (sscanf(h.c_str() + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}
// tag number k of a family: any 32 bytes do
static Bytes tag(uint8_t family, uint32_t k) {
  Bytes t(32, family);
  memcpy(t.data(), &k, 4);
  return t;
}
static Tags tags(uint8_t family, uint32_t first, uint32_t count) {
  Tags v;
  for (uint32_t k = 0; k < count; k++) v.push_back(tag(family, first + k));
  return v;
}
static uint8_t SALT[32];

// the loop of the header
struct Model {
  std::set<Bytes> in;
  Bytes spend(const Tags& T, const Bytes* status) {
    Bytes seen;
    for (size_t i = 0; i < T.size(); i++) {
      if (status && (*status)[i] != 0) seen.push_back(AFX_TAG_SKIPPED);
      else if (in.count(T[i])) seen.push_back(AFX_TAG_SPENT);
      else { seen.push_back(AFX_TAG_FRESH); in.insert(T[i]); }
    }
    return seen;
  }
  Bytes contains(const Tags& T) const {
    Bytes seen;
    for (const Bytes& t : T) seen.push_back(in.count(t) ? 1 : 0);
    return seen;
  }
};

// The arrays of one call, each a heap block of exactly its size (the rows 16-byte aligned, as the _dev forms require): on the fake
// runtime "device" pointers are host memory, so the same blocks serve both forms.
struct Call {
  size_t count;
  uint8_t* T;
  std::unique_ptr<uint8_t[]> status, seen;
  Call(const Tags& t, const Bytes* st) : count(t.size()), T((uint8_t*)aligned_alloc(16, 32 * (t.size() ? t.size() : 1))), status(st ? new uint8_t[count] : nullptr), seen(new uint8_t[count]) {
    for (size_t i = 0; i < count; i++) memcpy(T + 32 * i, t[i].data(), 32);
    if (st) memcpy(status.get(), st->data(), count);
    memset(seen.get(), MARK, count);
  }
  ~Call() { free(T); }
  Bytes answers() const { return Bytes(seen.get(), seen.get() + count); }
  bool untouched() const { return answers() == Bytes(count, MARK); }
};

enum Form { HOST, DEV };
static afx_ctx* ctx = nullptr;

static int spend_rc(afx_tagset* s, Form f, Call& c) {
  return f == HOST ? afx_tagset_spend(s, c.T, c.status.get(), c.count, c.seen.get()) : afx_tagset_spend_dev(s, c.T, c.status.get(), c.count, c.seen.get());
}
static int contains_rc(afx_tagset* s, Form f, Call& c) {
  return f == HOST ? afx_tagset_contains(s, c.T, c.count, c.seen.get()) : afx_tagset_contains_dev(s, c.T, c.count, c.seen.get());
}
// one call that must succeed and answer as the model does
static Bytes spend(afx_tagset* s, Form f, Model& m, const Tags& t, const Bytes* status = nullptr) {
  Call c(t, status);
  CHECK(spend_rc(s, f, c) == AFX_OK);
  if (f == DEV) CHECK(afx_ctx_synchronize(ctx) == AFX_OK);
  const Bytes want = m.spend(t, status);
  CHECK(c.answers() == want);
  return want;
}
static Bytes contains(afx_tagset* s, Form f, const Model& m, const Tags& t) {
  Call c(t, nullptr);
  CHECK(contains_rc(s, f, c) == AFX_OK);
  if (f == DEV) CHECK(afx_ctx_synchronize(ctx) == AFX_OK);
  const Bytes want = m.contains(t);
  CHECK(c.answers() == want);
  return want;
}
static void size_is(afx_tagset* s, uint64_t size, uint64_t capacity) {
  uint64_t n = ~0ull, cap = ~0ull;
  CHECK(afx_tagset_size(s, &n, &cap) == AFX_OK);
  CHECK(n == size && cap == capacity);
}
static afx_tagset* make(size_t capacity) {
  afx_tagset* s = nullptr;
  CHECK(afx_tagset_create(ctx, capacity, SALT, &s) == AFX_OK && s);
  return s;
}

struct Op {
  bool is_spend;
  Tags T;
  Bytes status;
  bool any_status;
};
static void scenario(const char* path, bool print) {
  std::ifstream in(path);
  CHECK(in.good());
  uint64_t capacity = 0;
  uint8_t salt[32];
  std::vector<Op> ops;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string word;
    if (!(ls >> word)) continue;
    if (word == "set") {
      std::string salt_hex;
      CHECK((ls >> capacity >> salt_hex) && unhex(salt_hex, salt, 32));
      continue;
    }
    CHECK(word == "call" || word == "contains");
    Op op;
    op.is_spend = word == "call";
    op.any_status = false;
    size_t count = 0;
    CHECK(!!(ls >> count));
    for (size_t i = 0; i < count; i++) {
      std::string th;
      unsigned st = 0;
      CHECK(!!std::getline(in, line));
      std::istringstream is(line);
      Bytes t(32);
      CHECK((is >> th) && unhex(th, t.data(), 32) && (!op.is_spend || (is >> st)));
      op.T.push_back(t);
      op.status.push_back((uint8_t)st);
      op.any_status |= st != 0;
    }
    ops.push_back(op);
  }
  CHECK(capacity != 0);
  for (Form f : { HOST, DEV }) {
    afx_tagset* s = nullptr;
    CHECK(afx_tagset_create(ctx, capacity, salt, &s) == AFX_OK);
    size_is(s, 0, capacity);
    Model m;
    for (const Op& op : ops) {
      const Bytes got = op.is_spend ? spend(s, f, m, op.T, op.any_status ? &op.status : nullptr) : contains(s, f, m, op.T);   // (no status at all where none is set: the null form)
      if (print && f == HOST) {
        std::string digits;
        for (uint8_t b : got) digits += (char)('0' + b);
        printf("%s %s\n", op.is_spend ? "seen" : "has", digits.c_str());
      }
    }
    size_is(s, m.in.size(), capacity);
    const Tags all(m.in.begin(), m.in.end());
    contains(s, f == HOST ? DEV : HOST, m, all);                            // ... and the other form reads the same table
    afx_tagset_destroy(s);
  }
}

// _dev calls count towards the bound until the size is read; a refused call touches nothing
static void the_bound() {
  for (Form f : { DEV, HOST }) {
    afx_tagset* s = make(64);
    Model m;
    const Tags first = tags(1, 0, 40), replay = tags(1, 0, 20), fresh5 = tags(2, 0, 5), fresh24 = tags(3, 0, 24);
    spend(s, f, m, first);
    spend(s, f, m, replay);                                                 // the set still holds 40; after _dev calls the bound says 60
    if (f == DEV) {
      const uint64_t launches = fake_tagset_launches(0);
      Call c(fresh5, nullptr);
      CHECK(spend_rc(s, DEV, c) == AFX_E_FULL && afx_last_error()[0]);
      CHECK(c.untouched() && fake_tagset_launches(0) == launches);
      Call h(fresh5, nullptr);                                              // the host form asks the same bound
      CHECK(spend_rc(s, HOST, h) == AFX_E_FULL && h.untouched());
      contains(s, DEV, m, fresh5);                                          // none of them went in
      size_is(s, 40, 64);                                                   // ... and the bound is exact again
    }
    spend(s, f, m, fresh24);                                                // 40 + 24: exactly the capacity
    size_is(s, 64, 64);
    for (const Tags& one : { tags(4, 0, 1), tags(1, 0, 1) }) {              // one more, new or not
      Call c(one, nullptr);
      CHECK(spend_rc(s, f, c) == AFX_E_FULL && c.untouched());
    }
    size_is(s, 64, 64);
    afx_tagset_destroy(s);
  }
  // skipped items count too, and a call of capacity + 1 is refused on an empty set
  afx_tagset* s = make(8);
  Model m;
  const Bytes skip_all(9, 1);
  Call c(tags(5, 0, 9), &skip_all);
  CHECK(spend_rc(s, HOST, c) == AFX_E_FULL && spend_rc(s, DEV, c) == AFX_E_FULL && c.untouched());
  const Bytes skip8(8, 7);
  spend(s, DEV, m, tags(5, 0, 8), &skip8);                                  // nothing inserted, the bound says 8 all the same
  Call one(tags(5, 0, 1), nullptr);
  CHECK(spend_rc(s, DEV, one) == AFX_E_FULL && one.untouched());
  size_is(s, 0, 8);
  spend(s, DEV, m, tags(5, 0, 8));
  size_is(s, 8, 8);
  afx_tagset_destroy(s);
}

static void arguments() {
  afx_tagset* s = (afx_tagset*)(uintptr_t)0x10;
  for (size_t capacity : { (size_t)0, ((size_t)1 << 30) + 1 }) {
    s = (afx_tagset*)(uintptr_t)0x10;
    CHECK(afx_tagset_create(ctx, capacity, SALT, &s) == AFX_E_BAD_ARGS && s == nullptr && afx_last_error()[0]);
  }
  CHECK(afx_tagset_create(nullptr, 64, SALT, &s) == AFX_E_BAD_ARGS);
  CHECK(afx_tagset_create(ctx, 64, SALT, nullptr) == AFX_E_BAD_ARGS);
  s = make(64);
  Model m;
  Call c(tags(6, 0, 4), nullptr);
  const uint64_t l0 = fake_tagset_launches(0), l1 = fake_tagset_launches(1);
  // a null set, null rows, null answers
  CHECK(afx_tagset_size(nullptr, nullptr, nullptr) == AFX_E_BAD_ARGS);
  CHECK(afx_tagset_spend(nullptr, c.T, nullptr, 4, c.seen.get()) == AFX_E_BAD_ARGS && afx_tagset_spend_dev(nullptr, c.T, nullptr, 4, c.seen.get()) == AFX_E_BAD_ARGS);
  CHECK(afx_tagset_contains(nullptr, c.T, 4, c.seen.get()) == AFX_E_BAD_ARGS && afx_tagset_contains_dev(nullptr, c.T, 4, c.seen.get()) == AFX_E_BAD_ARGS);
  CHECK(afx_tagset_spend(s, nullptr, nullptr, 4, c.seen.get()) == AFX_E_BAD_ARGS && afx_tagset_spend_dev(s, nullptr, nullptr, 4, c.seen.get()) == AFX_E_BAD_ARGS);
  CHECK(afx_tagset_contains(s, nullptr, 4, c.seen.get()) == AFX_E_BAD_ARGS && afx_tagset_contains_dev(s, nullptr, 4, c.seen.get()) == AFX_E_BAD_ARGS);
  CHECK(afx_tagset_spend(s, c.T, nullptr, 4, nullptr) == AFX_E_BAD_ARGS && afx_tagset_spend_dev(s, c.T, nullptr, 4, nullptr) == AFX_E_BAD_ARGS);
  CHECK(afx_tagset_contains(s, c.T, 4, nullptr) == AFX_E_BAD_ARGS && afx_tagset_contains_dev(s, c.T, 4, nullptr) == AFX_E_BAD_ARGS);
  // _dev rows that are not 16-byte aligned: refused, not read
  for (size_t off : { (size_t)1, (size_t)4, (size_t)8 }) {
    CHECK(afx_tagset_spend_dev(s, c.T + off, nullptr, 1, c.seen.get()) == AFX_E_BAD_ARGS);
    CHECK(afx_tagset_contains_dev(s, c.T + off, 1, c.seen.get()) == AFX_E_BAD_ARGS);
  }
  // more items than there are item numbers below the table's marks (nothing is read: the rows are 4 items long)
  for (size_t count : { (size_t)0xfffffffeull, (size_t)0xffffffffull, (size_t)1 << 32, ~(size_t)0 }) {
    CHECK(afx_tagset_spend(s, c.T, nullptr, count, c.seen.get()) == AFX_E_BAD_ARGS && afx_tagset_spend_dev(s, c.T, nullptr, count, c.seen.get()) == AFX_E_BAD_ARGS);
    CHECK(afx_tagset_contains(s, c.T, count, c.seen.get()) == AFX_E_BAD_ARGS && afx_tagset_contains_dev(s, c.T, count, c.seen.get()) == AFX_E_BAD_ARGS);
  }
  // 2^32 - 3 items is a count the call accepts: what refuses it is the bound
  CHECK(afx_tagset_spend(s, c.T, nullptr, (size_t)0xfffffffdull, c.seen.get()) == AFX_E_FULL && afx_tagset_spend_dev(s, c.T, nullptr, (size_t)0xfffffffdull, c.seen.get()) == AFX_E_FULL);
  // count 0 is no call, whatever the pointers
  CHECK(afx_tagset_spend(s, nullptr, nullptr, 0, nullptr) == AFX_OK && afx_tagset_spend_dev(s, nullptr, nullptr, 0, nullptr) == AFX_OK);
  CHECK(afx_tagset_contains(s, nullptr, 0, nullptr) == AFX_OK && afx_tagset_contains_dev(s, nullptr, 0, nullptr) == AFX_OK);
  CHECK(c.untouched() && fake_tagset_launches(0) == l0 && fake_tagset_launches(1) == l1);
  size_is(s, 0, 64);
  spend(s, HOST, m, tags(6, 0, 4));                                         // the refusals left a set that works
  uint64_t n = 0;
  CHECK(afx_tagset_size(s, &n, nullptr) == AFX_OK && n == 4 && afx_tagset_size(s, nullptr, &n) == AFX_OK && n == 64 && afx_tagset_size(s, nullptr, nullptr) == AFX_OK);
  afx_tagset_destroy(s);
}

// every call of both forms on a set that has failed: the first error's code, a text, nothing launched, nothing written
static void every_call_returns(afx_tagset* s, int rc) {
  const uint64_t l0 = fake_tagset_launches(0), l1 = fake_tagset_launches(1);
  for (int round = 0; round < 3; round++) {
    Call c(tags(7, 100, 3), nullptr);
    uint64_t n = 123, cap = 456;
    CHECK(afx_tagset_size(s, &n, &cap) == rc && afx_last_error()[0] && n == 123 && cap == 456);
    CHECK(spend_rc(s, HOST, c) == rc && afx_last_error()[0]);
    CHECK(spend_rc(s, DEV, c) == rc && afx_last_error()[0]);
    CHECK(contains_rc(s, HOST, c) == rc && afx_last_error()[0]);
    CHECK(contains_rc(s, DEV, c) == rc && afx_last_error()[0]);
    CHECK(afx_tagset_spend(s, nullptr, nullptr, 0, nullptr) == rc);         // (an empty call on a broken set says so too)
    CHECK(c.untouched());
  }
  CHECK(fake_tagset_launches(0) == l0 && fake_tagset_launches(1) == l1);
}

static void a_launcher_error() {
  for (int which = 0; which < 4; which++) {                                // the failing call: spend, contains, spend_dev, contains_dev
    afx_tagset *a = make(64), *b = make(64);
    Model ma, mb;
    spend(a, HOST, ma, tags(7, 0, 10));
    Call c(tags(7, 5, 10), nullptr);
    fake_tagset_set("fail_next", 1);
    const Form f = which < 2 ? HOST : DEV;
    const int rc = (which & 1) ? contains_rc(a, f, c) : spend_rc(a, f, c);
    CHECK(rc != AFX_OK && rc != AFX_E_BAD_ARGS && rc != AFX_E_FULL && afx_last_error()[0]);
    CHECK(c.untouched());
    every_call_returns(a, rc);
    spend(b, HOST, mb, tags(7, 0, 10));                                     // another set on the same context still works
    spend(b, DEV, mb, tags(7, 5, 10));
    size_is(b, 15, 64);
    afx_tagset_destroy(a);                                                  // destroy after a failure
    afx_tagset_destroy(b);
  }
}

static void the_error_word() {
  // the host forms read the two words back before they hand out an answer
  for (int lookup = 0; lookup < 2; lookup++) {
    afx_tagset* s = make(64);
    Model m;
    spend(s, HOST, m, tags(8, 0, 10));
    Call c(tags(8, 5, 10), nullptr);
    fake_tagset_set("error_next", 1);
    CHECK((lookup ? contains_rc(s, HOST, c) : spend_rc(s, HOST, c)) == AFX_E_HIP && afx_last_error()[0]);
    CHECK(c.untouched());
    every_call_returns(s, AFX_E_HIP);
    afx_tagset_destroy(s);
  }
  // a _dev call cannot know: the next afx_tagset_size reports it
  for (int lookup = 0; lookup < 2; lookup++) {
    afx_tagset* s = make(64);
    Model m;
    spend(s, DEV, m, tags(8, 0, 10));
    Call c(tags(8, 5, 10), nullptr);
    fake_tagset_set("error_next", 1);
    CHECK((lookup ? contains_rc(s, DEV, c) : spend_rc(s, DEV, c)) == AFX_OK);
    CHECK(afx_ctx_synchronize(ctx) == AFX_OK);
    CHECK(c.untouched());                                                   // (the kernels' guard: no item runs once the word is set)
    uint64_t n = 123;
    CHECK(afx_tagset_size(s, &n, nullptr) == AFX_E_HIP && afx_last_error()[0] && n == 123);
    every_call_returns(s, AFX_E_HIP);
    afx_tagset_destroy(s);
  }
}

// Calls of every size over the lanes' scratch buffers.  A host-pointer call of 30 000 items needs T | slot_of | status_in | seen_out =
// 1 140 000 bytes, more than the megabyte a lane's buffer starts with: the buffer is replaced under the call.  With pipelining on,
// calls alternate between the two lanes, each with a buffer of its own, and must still run behind each other.
static void both_pipelining_settings() {
  for (int pipelining : { 0, 1, 0 }) {
    CHECK(afx_ctx_set_pipelining(ctx, pipelining) == AFX_OK);
    afx_tagset* s = make((size_t)1 << 16);
    Model m;
    const uint32_t BIG = 30000;
    Tags big = tags(9, 0, BIG);
    Bytes st(BIG, 0);
    for (uint32_t i = 0; i < BIG; i++) {
      if (i % 7 == 3) big[i] = big[i / 2];                                  // repeats, far apart
      if (i % 11 == 5) st[i] = (uint8_t)(1 + i % 3);
    }
    st[BIG - 1] = 1;                                                        // the last bytes of the status and answer regions
    const Bytes st5 = { 0, 1, 0, 2, 0 };
    spend(s, HOST, m, tags(9, 0, 5), &st5);
    contains(s, HOST, m, tags(9, 0, 6));
    spend(s, DEV, m, tags(9, 3, 4));
    spend(s, HOST, m, big, &st);                                            // outgrows the lane's buffer
    contains(s, HOST, m, big);                                              // ... and the other lane's, with pipelining
    contains(s, DEV, m, tags(9, BIG - 3, 6));
    spend(s, HOST, m, tags(9, BIG - 2, 4));
    spend(s, HOST, m, big);                                                 // without status: that region is not staged
    spend(s, DEV, m, tags(10, 0, 70), nullptr);
    spend(s, HOST, m, tags(10, 60, 20), nullptr);
    size_is(s, m.in.size(), (size_t)1 << 16);
    afx_tagset_destroy(s);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: tagset_doors <dir> SCENARIO...\n"); return 2; }
  const std::string dir = argv[1];
  const Bytes params = rd(dir + "/params.bin"), ip = rd(dir + "/ip.bin");
  CHECK(ip.size() == 64);
  CHECK(afx_ctx_create(&ctx, 0, params.data(), params.size(), nullptr, 0, ip.data()) == AFX_OK);   // the set needs no key
  for (int i = 0; i < 32; i++) SALT[i] = (uint8_t)(3 * i + 1);

  afx_tagset_destroy(nullptr);
  for (int pipelining : { 0, 1 }) {
    CHECK(afx_ctx_set_pipelining(ctx, pipelining) == AFX_OK);
    for (int a = 2; a < argc; a++) {
      if (pipelining == 0) printf("scenario %d\n", a - 2);
      scenario(argv[a], pipelining == 0);
    }
  }
  CHECK(afx_ctx_set_pipelining(ctx, 0) == AFX_OK);
  the_bound();
  arguments();
  a_launcher_error();
  the_error_word();
  both_pipelining_settings();
  CHECK(afx_ctx_set_pipelining(ctx, 1) == AFX_OK);                          // the refusals and the broken state on alternating lanes
  the_bound();
  a_launcher_error();
  the_error_word();
  CHECK(afx_ctx_set_pipelining(ctx, 0) == AFX_OK);
  afx_tagset_destroy(nullptr);
  afx_ctx_destroy(ctx);
  printf("tagset doors ok\n");
  return 0;
}
