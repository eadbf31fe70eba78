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

namespace {
constexpr int ORDERS = 10;
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
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: tagset_host SCENARIO\n"); return 2; }
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
        for (uint32_t i : lane_order(u, 0, call, count)) tagset_claim_item(tb.t, T.get(), status.get(), count, i, slot_of.get());
        if (tb.words[1]) bad("the claim launch set the error word", call, u);
        unsigned long long inserted = 0;
        for (uint32_t i : lane_order(u, 1, call, count)) inserted += tagset_resolve_item(tb.t, T.get(), i, slot_of.get(), seen.get()) ? 1 : 0;
        TS_ADD(&tb.words[0], inserted);
      } else {
        for (uint32_t i : lane_order(u, 0, call, count)) tagset_contains_item(tb.t, T.get(), i, seen.get());
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
