// The lane bodies of the spent-tag set (aeonflux_amd/csrc/tagset.cuh: tagset_slot, tagset_claim_item, tagset_resolve_item,
// tagset_contains_item - what k_tagset_claim, k_tagset_resolve and k_tagset_contains run per lane) compiled for the host and run lane by
// lane, so that the CPU test-suite checks them without a GPU (tests/test_tagset_on_host.py).  A stand-alone program, built with
// -fsanitize=address,undefined: every array is a heap block of exactly its size.  Test infrastructure only.
//
//   tagset_host SCENARIO        SCENARIO: text, one word list per line
//       set <capacity> <salt: 64 hex digits>
//       call <count>            followed by <count> lines "<T: 64 hex digits> <status_in>"
//       contains <count>        followed by <count> lines "<T>"
//
// Every `call` runs in ORDERS universes, each with a table of its own: the claim lanes run in one seeded shuffled order, then the resolve
// lanes in another (universe 0: ascending, universe 1: descending) - each one legal interleaving at lane granularity.  The answers must
// be identical across universes, and so must the sets' contents AS SETS (which key took which slot of a chain may differ); a
// difference, an error word, or a size word that is not the number of kept slots ends the program with status 1.  Printed, for the test
// to compare with its own model and with hashlib:  "slot <T> <slot>" per item of a call, "seen <digits>" per call, "has <digits>" per
// lookup, and at the end "size <n>" and the sorted "key <T>" lines.
//
// Built with -DAFX_TAGSET_TEST_THREADS -fsanitize=thread (tagset.cuh then takes its atomics as relaxed __atomic builtins) the universes
// are ROUNDS of real concurrency: the claim lanes of a call run on 16 threads that start together, the threads are joined - the edge
// between the two launches on a stream - and the resolve lanes run on 16 threads.  Thread k takes every 16th lane of the round's
// shuffled order, so neighbours of the order run at the same time and a lane that joins a slot may arrive between the claimer's
// compare-and-swap and its minimum.  The same checks; a data race in the lane bodies is ThreadSanitizer's to report.
//
//   tagset_host error-paths     (the single-threaded build) the lane bodies where a table is not what a finished call leaves: a slot
//                               owned by an item number the call does not have, and a table with no empty slot.  Prints "error paths ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <fstream>
#include <memory>
#include <random>
#include <set>
#include <sstream>
#include <string>
#include <vector>
#include "../../aeonflux_amd/csrc/tagset.cuh"

#if defined(AFX_TAGSET_TEST_THREADS)
#include <atomic>
#include <thread>
#endif

namespace {
#if defined(AFX_TAGSET_TEST_THREADS)
constexpr int ORDERS = 20, THREADS = 16;   // 16 whatever the machine has: the interleavings come from preemption as much as from cores
// body(lane, thread) for every lane of the order, thread k on lanes k, k + 16, ...; returns when all threads are joined
template <class F>
void run_lanes(const std::vector<uint32_t>& order, F body) {
  std::atomic<int> ready{ 0 };
  std::vector<std::thread> threads;
  for (int k = 0; k < THREADS; k++)
    threads.emplace_back([&order, &ready, &body, k] {
      ready.fetch_add(1);
      while (ready.load() < THREADS) std::this_thread::yield();   // (start together: a thread is slower to make than its lanes are to run)
      for (size_t j = (size_t)k; j < order.size(); j += THREADS) body(order[j], k);
    });
  for (std::thread& t : threads) t.join();
}
#else
constexpr int ORDERS = 10, THREADS = 1;
template <class F>
void run_lanes(const std::vector<uint32_t>& order, F body) {
  for (uint32_t i : order) body(i, 0);
}
#endif
using Row = std::vector<uint8_t>;

struct Table {
  uint32_t n_slots = 0;
  // heap blocks of exactly their size (16-byte alignment is what the device rows have; the host loads are memcpy)
  std::unique_ptr<uint8_t[]> keys;
  std::unique_ptr<uint32_t[]> owner, lowest;
  std::unique_ptr<unsigned long long[]> words;
  afx_tagset_table t;
  void init(uint64_t capacity, const uint8_t salt[32]) {
    n_slots = 2;
    while (n_slots < 2 * capacity) n_slots <<= 1;
    keys.reset(new uint8_t[32 * (size_t)n_slots]());
    owner.reset(new uint32_t[n_slots]);
    lowest.reset(new uint32_t[n_slots]);
    words.reset(new unsigned long long[2]());
    std::fill(owner.get(), owner.get() + n_slots, AFX_TAGSET_EMPTY);
    std::fill(lowest.get(), lowest.get() + n_slots, 0xffffffffu);
    t.keys = keys.get(); t.owner = owner.get(); t.lowest = lowest.get(); t.words = words.get();
    t.mask = n_slots - 1; t.pad = 0;
    for (int k = 0; k < 4; k++) {
      t.salt[k] = 0;
      for (int b = 0; b < 8; b++) t.salt[k] |= (uint64_t)salt[8 * k + b] << (8 * b);
    }
  }
  std::set<Row> contents(uint64_t* kept) const {
    std::set<Row> s;
    *kept = 0;
    for (uint32_t i = 0; i < n_slots; i++) {
      if (owner[i] == AFX_TAGSET_EMPTY) continue;
      if (owner[i] != AFX_TAGSET_KEPT) { fprintf(stderr, "slot %u is left claimed by item %u\n", i, owner[i]); exit(1); }
      ++*kept;
      s.insert(Row(keys.get() + 32 * (size_t)i, keys.get() + 32 * (size_t)i + 32));
    }
    return s;
  }
};

bool unhex(const std::string& h, uint8_t* out, size_t n) {
  if (h.size() != 2 * n) return false;
  for (size_t i = 0; i < n; i++) {
    unsigned v = 0;
    if (sscanf(h.c_str() + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}
std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
  return s;
}
std::vector<uint32_t> lane_order(int universe, int phase, uint32_t call, uint32_t count) {
  std::vector<uint32_t> o(count);
  for (uint32_t i = 0; i < count; i++) o[i] = i;
  if (universe == 1) std::reverse(o.begin(), o.end());
  if (universe >= 2) {
    std::mt19937_64 g(1000003ull * universe + 7919ull * call + phase);
    std::shuffle(o.begin(), o.end(), g);
  }
  return o;
}
[[noreturn]] void bad(const char* what, uint32_t call, int universe) {
  fprintf(stderr, "%s (call %u, universe %d)\n", what, call, universe);
  exit(1);
}

// ---- error-paths -------------------------------------------------------------------------------------------------------------------
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "error-paths, line %d: %s\n", __LINE__, #cond); return 1; } } while (0)
// tag number k of a family: any 32 bytes do
Row numbered(uint32_t family, uint32_t k) {
  Row r(32, (uint8_t)family);
  memcpy(r.data(), &k, 4);
  return r;
}
uint32_t start_of(const Table& tb, const Row& r) { return tagset_slot(tb.t.salt, ts_load(r.data()), tb.t.mask); }
// the first tags of a family whose probe sequences start at `slot`
std::vector<Row> aimed(const Table& tb, uint32_t family, uint32_t slot, size_t how_many) {
  std::vector<Row> out;
  for (uint32_t k = 0; out.size() < how_many; k++)
    if (start_of(tb, numbered(family, k)) == slot) out.push_back(numbered(family, k));
  return out;
}
void keep(Table& tb, uint32_t slot, const Row& key) {
  memcpy(tb.keys.get() + 32 * (size_t)slot, key.data(), 32);
  tb.owner[slot] = AFX_TAGSET_KEPT;
}

int error_paths() {
  uint8_t salt[32];
  for (int i = 0; i < 32; i++) salt[i] = (uint8_t)(7 * i + 1);
  {
    // A slot on an item's probe path whose owner is an item number the call does not have (an earlier call died between its launches).
    // X starts at slot 40, which keeps another key, and meets the stale owner at slot 41; A and B go elsewhere.
    Table tb;
    tb.init(64, salt);
    const std::vector<Row> at40 = aimed(tb, 1, 40, 2);
    const Row A = aimed(tb, 2, 90, 1)[0], B = aimed(tb, 2, 10, 1)[0], &X = at40[1];
    keep(tb, 40, at40[0]);
    const uint32_t count = 3, stale = 1000;
    tb.owner[41] = stale;
    std::unique_ptr<uint8_t[]> T(new uint8_t[32 * count]), seen(new uint8_t[count]);
    std::unique_ptr<uint32_t[]> slot_of(new uint32_t[count]);
    memcpy(T.get(), A.data(), 32); memcpy(T.get() + 32, X.data(), 32); memcpy(T.get() + 64, B.data(), 32);
    memset(seen.get(), 0xee, count);
    for (uint32_t i = 0; i < count; i++) slot_of[i] = 0x12345678u;
    for (uint32_t i : { 2u, 1u, 0u }) tagset_claim_item(tb.t, T.get(), nullptr, count, i, slot_of.get());
    EXPECT(tb.words[1] != 0);                                            // the claim sets the error word ...
    EXPECT(slot_of[1] == AFX_TAGSET_NO_SLOT);                            // ... and records no slot
    EXPECT(slot_of[0] == 90 && slot_of[2] == 10);
    EXPECT(tb.owner[41] == stale && tb.owner[40] == AFX_TAGSET_KEPT && tb.owner[42] == AFX_TAGSET_EMPTY);
    unsigned inserted = 0;
    for (uint32_t i = 0; i < count; i++) inserted += tagset_resolve_item(tb.t, T.get(), i, slot_of.get(), seen.get()) ? 1 : 0;
    EXPECT(seen[1] == 0xee);                                             // no answer for it
    EXPECT(seen[0] == AFX_TAG_FRESH && seen[2] == AFX_TAG_FRESH && inserted == 2);
    // a lookup through that slot
    tb.words[1] = 0;
    uint8_t has[2] = { 0xee, 0xee };
    tagset_contains_item(tb.t, T.get(), 1, has);
    EXPECT(tb.words[1] != 0 && has[0] == 0xee && has[1] == 0);
    tb.words[1] = 0;
    tagset_contains_item(tb.t, at40[0].data(), 0, has);                  // the key in front of the stale slot is found as ever
    EXPECT(tb.words[1] == 0 && has[0] == 1);
  }
  {
    // A table in which every slot is kept by other keys; P sits in the slot BEFORE its start slot: the last step of its probe.
    Table tb;
    tb.init(64, salt);
    const uint32_t n = tb.n_slots;
    EXPECT(n == 128);
    const Row P = aimed(tb, 3, 0, 1)[0], absent = aimed(tb, 4, 64, 1)[0];
    for (uint32_t s = 0; s < n; s++) keep(tb, s, numbered(5, s));
    keep(tb, n - 1, P);
    std::vector<uint32_t> owner_before(tb.owner.get(), tb.owner.get() + n);
    std::vector<uint8_t> keys_before(tb.keys.get(), tb.keys.get() + 32 * (size_t)n);
    uint8_t has[1] = { 0xee };
    tagset_contains_item(tb.t, absent.data(), 0, has);
    EXPECT(tb.words[1] != 0 && has[0] == 0);                             // n_slots steps, then the error word
    tb.words[1] = 0;
    has[0] = 0xee;
    tagset_contains_item(tb.t, P.data(), 0, has);
    EXPECT(tb.words[1] == 0 && has[0] == 1);                             // found on the last step
    uint32_t slot_of[1] = { 0x12345678u };
    tagset_claim_item(tb.t, P.data(), nullptr, 1, 0, slot_of);
    EXPECT(tb.words[1] == 0 && slot_of[0] == AFX_TAGSET_OLD);
    slot_of[0] = 0x12345678u;
    tagset_claim_item(tb.t, absent.data(), nullptr, 1, 0, slot_of);
    EXPECT(tb.words[1] != 0 && slot_of[0] == AFX_TAGSET_NO_SLOT);
    EXPECT(std::equal(owner_before.begin(), owner_before.end(), tb.owner.get()));   // never written
    EXPECT(std::equal(keys_before.begin(), keys_before.end(), tb.keys.get()));
    for (uint32_t s = 0; s < n; s++) EXPECT(tb.lowest[s] == 0xffffffffu);
    uint8_t seen[1] = { 0xee };
    EXPECT(!tagset_resolve_item(tb.t, absent.data(), 0, slot_of, seen) && seen[0] == 0xee);
  }
  printf("error paths ok\n");
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: tagset_host SCENARIO | error-paths\n"); return 2; }
  if (!strcmp(argv[1], "error-paths")) return error_paths();
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::vector<Table> tables(ORDERS);
  bool have_set = false;
  uint32_t call = 0;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string word;
    if (!(ls >> word)) continue;
    if (word == "set") {
      uint64_t capacity = 0;
      std::string salt_hex;
      uint8_t salt[32];
      if (!(ls >> capacity >> salt_hex) || !unhex(salt_hex, salt, 32) || capacity == 0 || capacity > (1u << 20)) { fprintf(stderr, "bad set line\n"); return 2; }
      for (Table& tb : tables) tb.init(capacity, salt);
      have_set = true;
      continue;
    }
    if ((word != "call" && word != "contains") || !have_set) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
    const bool spend = word == "call";
    uint32_t count = 0;
    if (!(ls >> count)) { fprintf(stderr, "bad count\n"); return 2; }
    // the call's rows: blocks of exactly count rows
    std::unique_ptr<uint8_t[]> T(new uint8_t[32 * (size_t)count]), status(new uint8_t[count]);
    for (uint32_t i = 0; i < count; i++) {
      std::string th;
      unsigned st = 0;
      if (!std::getline(in, line)) { fprintf(stderr, "scenario ends inside a call\n"); return 2; }
      std::istringstream is(line);
      if (!(is >> th) || !unhex(th, T.get() + 32 * (size_t)i, 32) || (spend && !(is >> st))) { fprintf(stderr, "bad item line: %s\n", line.c_str()); return 2; }
      status[i] = (uint8_t)st;
    }
    std::string first;
    for (int u = 0; u < ORDERS; u++) {
      Table& tb = tables[u];
      std::unique_ptr<uint8_t[]> seen(new uint8_t[count]);
      memset(seen.get(), 0xee, count);
      if (spend) {
        std::unique_ptr<uint32_t[]> slot_of(new uint32_t[count]);
        run_lanes(lane_order(u, 0, call, count), [&](uint32_t i, int) { tagset_claim_item(tb.t, T.get(), status.get(), count, i, slot_of.get()); });
        if (tb.words[1]) bad("the claim launch set the error word", call, u);
        unsigned long long inserted[THREADS] = {};
        run_lanes(lane_order(u, 1, call, count), [&](uint32_t i, int k) { inserted[k] += tagset_resolve_item(tb.t, T.get(), i, slot_of.get(), seen.get()) ? 1 : 0; });
        for (unsigned long long n : inserted) TS_ADD(&tb.words[0], n);
      } else {
        run_lanes(lane_order(u, 0, call, count), [&](uint32_t i, int) { tagset_contains_item(tb.t, T.get(), i, seen.get()); });
        if (tb.words[1]) bad("the lookup set the error word", call, u);
      }
      std::string digits;
      for (uint32_t i = 0; i < count; i++) {
        if (seen[i] > 2) bad("an item got no answer", call, u);
        digits += (char)('0' + seen[i]);
      }
      if (u == 0) first = digits;
      else if (digits != first) bad("the answers depend on the lane order", call, u);
    }
    if (spend)
      for (uint32_t i = 0; i < count; i++) {
        const ts_row r = ts_load(T.get() + 32 * (size_t)i);
        printf("slot %s %u\n", hex(T.get() + 32 * (size_t)i, 32).c_str(), tagset_slot(tables[0].t.salt, r, tables[0].t.mask));
      }
    printf("%s %s\n", spend ? "seen" : "has", first.c_str());
    call++;
  }
  if (!have_set) { fprintf(stderr, "no set line\n"); return 2; }
  uint64_t kept0 = 0;
  const std::set<Row> want = tables[0].contents(&kept0);
  for (int u = 0; u < ORDERS; u++) {
    uint64_t kept = 0;
    const std::set<Row> got = tables[u].contents(&kept);
    if (got != want) bad("the sets' contents depend on the lane order", call, u);
    if (kept != got.size()) bad("a key sits in two slots", call, u);
    if (tables[u].words[0] != kept) bad("the size word is not the number of kept slots", call, u);
  }
  printf("size %llu\n", (unsigned long long)kept0);
  for (const Row& k : want) printf("key %s\n", hex(k.data(), 32).c_str());
  return 0;
}
