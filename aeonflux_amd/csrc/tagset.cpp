// The spent-tag set (include/aeonflux_gpu.h "The spent-tag set"): the host side.  The table lives in HBM (plan.h afx_tagset_table) and
// is only ever touched by the three kernels of tagset.cuh, direct launches on a lane's stream like k_sc_invert - no launch kind of a plan.
// What the host keeps: an upper bound of the size (exact after every host-pointer call and after afx_tagset_size), which decides
// AFX_E_FULL before anything runs; the lane and an event of the set's latest call, so that calls on one set run behind each other on the
// device whichever lane they take (two claim launches on one table at once would read each other's item numbers); and the first error.
// Per-item scratch (slot_of, and a host-pointer call's staged rows) lies in a buffer per lane, owned by the set.
#include "statements.hpp"

struct afx_tagset {
  afx_ctx* ctx = nullptr;
  uint64_t capacity = 0, n_slots = 0;
  uint64_t size_bound = 0;           // the set holds at most this many tags
  afx::DevBuf table;                 // keys | owner | lowest | the two words
  afx_tagset_table t = {};
  afx::DevBuf scratch[afx_ctx::AFX_LANES];
  hipEvent_t done = nullptr;         // end of the latest call's launches
  int last_lane = -1;
  int broken = 0;                    // the first error of a call that may have left the table half way, returned by every later call
  std::string broken_text;
};

namespace {
constexpr uint64_t MAX_CAPACITY = 1ull << 30;   // n_slots <= 2^31: slots are 32-bit words below the AFX_TAGSET_* marks
constexpr size_t MAX_COUNT = 0xfffffffdull;    // 2^32 - 3: item numbers stay below AFX_TAGSET_KEPT

int fail(afx_tagset* s, int rc) {
  if (!s->broken) { s->broken = rc; s->broken_text = std::string("the spent-tag set is unusable after: ") + afx::last_error(); }
  return rc;
}
int usable(afx_tagset* s) {
  if (!s->broken) return AFX_OK;
  set_error(s->broken_text);
  return s->broken;
}
// the lane a direct call takes (run_chunked's choice; a direct call is a call of its own: with pipelining it takes the next lane in turn)
int pick_lane(afx_ctx* c) { return c->force_lane >= 0 ? c->force_lane : (c->pipelining ? (int)(c->lane_next++ & 1u) : 0); }
int room(afx_tagset* s, size_t count) {
  if (count > MAX_COUNT) { set_error("too many items in one call"); return AFX_E_BAD_ARGS; }
  if (s->size_bound + count > s->capacity) {
    set_error("the spent-tag set may hold " + std::to_string(s->size_bound) + " of its " + std::to_string(s->capacity) + " tags: no room for " + std::to_string(count) + " more");
    return AFX_E_FULL;
  }
  return AFX_OK;
}
// the launches of one call behind the set's previous call
template <class F>
int ordered(afx_tagset* s, int lane, F launch) {
  hipStream_t stream = s->ctx->lane[lane].stream;
  if (s->last_lane >= 0 && s->last_lane != lane) AFX_HIP(hipStreamWaitEvent(stream, s->done, 0));
  AFX_HIP(launch(stream));
  AFX_HIP(hipEventRecord(s->done, stream));
  s->last_lane = lane;
  return AFX_OK;
}
// the two words back: the exact size, the error word
int read_words(afx_tagset* s, hipStream_t stream) {
  unsigned long long w[2] = { 0, 0 };
  AFX_HIP(hipMemcpyAsync(w, s->t.words, sizeof w, hipMemcpyDeviceToHost, stream));
  AFX_HIP(hipStreamSynchronize(stream));
  if (w[1] != 0 || w[0] > s->capacity) { set_error("the spent-tag set's kernels found its table inconsistent"); return AFX_E_HIP; }
  s->size_bound = w[0];
  return AFX_OK;
}
constexpr size_t up16(size_t n) { return (n + 15) & ~size_t(15); }
}  // namespace

extern "C" int afx_tagset_create(afx_ctx* ctx, size_t capacity, const uint8_t* salt, afx_tagset** out) try {
  if (!ctx || !out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  *out = nullptr;
  if (capacity == 0 || capacity > MAX_CAPACITY) { set_error("a spent-tag set holds 1 .. 2^30 tags"); return AFX_E_BAD_ARGS; }
  if (!afxk_tagset_spend || !afxk_tagset_contains) { set_error("the spent-tag set: no k_tagset_claim launcher in this build"); return AFX_E_NO_DEVICE; }
  CtxLock lock__(ctx);
  AFX_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<afx_tagset, void (*)(afx_tagset*)> s(new afx_tagset(), afx_tagset_destroy);
  s->ctx = ctx;
  s->capacity = capacity;
  s->n_slots = 2;
  while (s->n_slots < 2 * capacity) s->n_slots <<= 1;
  uint8_t salt_bytes[32];
  if (salt) memcpy(salt_bytes, salt, 32);
  else
    for (size_t got = 0; got < 32;) {
      const ssize_t r = getrandom(salt_bytes + got, 32 - got, 0);
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) { set_error("getrandom failed"); return AFX_E_BAD_ARGS; }
      got += (size_t)r;
    }
  for (int k = 0; k < 4; k++) {
    s->t.salt[k] = 0;
    for (int b = 0; b < 8; b++) s->t.salt[k] |= (uint64_t)salt_bytes[8 * k + b] << (8 * b);
  }
  s->table.sensitive = false;
  for (auto& b : s->scratch) b.sensitive = false;
  const size_t n = (size_t)s->n_slots;
  int rc = s->table.ensure(32 * n + 4 * n + 4 * n + 16);
  if (rc) return rc;
  uint8_t* base = (uint8_t*)s->table.p;
  s->t.keys = base;
  s->t.owner = (uint32_t*)(base + 32 * n);
  s->t.lowest = (uint32_t*)(base + 36 * n);
  s->t.words = (unsigned long long*)(base + 40 * n);
  s->t.mask = (uint32_t)(n - 1);
  // keys 0, owner AFX_TAGSET_EMPTY, lowest all ones, both words 0; the lanes' streams do not wait for the null stream: the device does
  AFX_HIP(hipMemset(base, 0, 32 * n));
  AFX_HIP(hipMemset(base + 32 * n, 0xff, 8 * n));
  AFX_HIP(hipMemset(base + 40 * n, 0, 16));
  AFX_HIP(hipDeviceSynchronize());
  AFX_HIP(hipEventCreateWithFlags(&s->done, hipEventDisableTiming));
  *out = s.release();
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }

extern "C" void afx_tagset_destroy(afx_tagset* s) {
  if (!s) return;
  if (s->ctx) {
    CtxLock lock__(s->ctx);
    (void)hipSetDevice(s->ctx->device);
    for (auto& L : s->ctx->lane)
      if (L.stream) (void)hipStreamSynchronize(L.stream);
    s->table.release(false);
    for (auto& b : s->scratch) b.release(false);
    if (s->done) (void)hipEventDestroy(s->done);
  }
  delete s;
}

extern "C" int afx_tagset_size(afx_tagset* s, uint64_t* size_out, uint64_t* capacity_out) try {
  if (!s) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  CtxLock lock__(s->ctx);
  int rc = usable(s);
  if (rc) return rc;
  AFX_HIP(hipSetDevice(s->ctx->device));
  const int lane = s->last_lane >= 0 ? s->last_lane : 0;
  if ((rc = read_words(s, s->ctx->lane[lane].stream))) return fail(s, rc);
  if (size_out) *size_out = s->size_bound;
  if (capacity_out) *capacity_out = s->capacity;
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_tagset_spend_dev(afx_tagset* s, const uint8_t* T, const uint8_t* status_in, size_t count, uint8_t* seen_out) try {
  if (!s) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  CtxLock lock__(s->ctx);
  int rc = usable(s);
  if (rc) return rc;
  if (count == 0) return AFX_OK;
  if (!T || !seen_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if ((uintptr_t)T & 15u) { set_error("tag rows are not 16-byte aligned"); return AFX_E_BAD_ARGS; }
  if ((rc = room(s, count))) return rc;
  AFX_HIP(hipSetDevice(s->ctx->device));
  const int lane = pick_lane(s->ctx);
  if ((rc = s->scratch[lane].ensure(4 * count))) return rc;
  uint32_t* slot_of = (uint32_t*)s->scratch[lane].p;
  rc = ordered(s, lane, [&](hipStream_t st) { return afxk_tagset_spend(st, &s->t, T, status_in, (uint32_t)count, slot_of, seen_out); });
  if (rc) return fail(s, rc);
  s->size_bound += count;
  return AFX_OK;
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_tagset_contains_dev(afx_tagset* s, const uint8_t* T, size_t count, uint8_t* seen_out) try {
  if (!s) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  CtxLock lock__(s->ctx);
  int rc = usable(s);
  if (rc) return rc;
  if (count == 0) return AFX_OK;
  if (!T || !seen_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if ((uintptr_t)T & 15u) { set_error("tag rows are not 16-byte aligned"); return AFX_E_BAD_ARGS; }
  if (count > MAX_COUNT) { set_error("too many items in one call"); return AFX_E_BAD_ARGS; }
  AFX_HIP(hipSetDevice(s->ctx->device));
  const int lane = pick_lane(s->ctx);
  rc = ordered(s, lane, [&](hipStream_t st) { return afxk_tagset_contains(st, &s->t, T, (uint32_t)count, seen_out); });
  return rc ? fail(s, rc) : AFX_OK;
} catch (...) { return afx::exception_rc(); }

// The host-pointer forms: the rows go to the lane's scratch in one piece (T | slot_of | status_in | seen_out), the answers come back into
// an image of the host's own, so that a call that fails has written nothing to seen_out.
static int host_call(afx_tagset* s, const uint8_t* T, const uint8_t* status_in, size_t count, uint8_t* seen_out, bool spend) {
  if (!s) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  CtxLock lock__(s->ctx);
  int rc = usable(s);
  if (rc) return rc;
  if (count == 0) return AFX_OK;
  if (!T || !seen_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (spend) {
    if ((rc = room(s, count))) return rc;
  } else if (count > MAX_COUNT) { set_error("too many items in one call"); return AFX_E_BAD_ARGS; }
  AFX_HIP(hipSetDevice(s->ctx->device));
  const int lane = pick_lane(s->ctx);
  const size_t o_slot = 32 * count, o_st = o_slot + up16(4 * count), o_seen = o_st + up16(count);
  if ((rc = s->scratch[lane].ensure(o_seen + up16(count)))) return rc;
  uint8_t* d = (uint8_t*)s->scratch[lane].p;
  hipStream_t stream = s->ctx->lane[lane].stream;
  std::vector<uint8_t> seen(count);
  AFX_HIP(hipMemcpyAsync(d, T, 32 * count, hipMemcpyHostToDevice, stream));
  if (spend && status_in) AFX_HIP(hipMemcpyAsync(d + o_st, status_in, count, hipMemcpyHostToDevice, stream));
  rc = ordered(s, lane, [&](hipStream_t st) {
    return spend ? afxk_tagset_spend(st, &s->t, d, status_in ? d + o_st : nullptr, (uint32_t)count, (uint32_t*)(d + o_slot), d + o_seen)
                 : afxk_tagset_contains(st, &s->t, d, (uint32_t)count, d + o_seen);
  });
  if (rc) return fail(s, rc);
  hipError_t e = hipMemcpyAsync(seen.data(), d + o_seen, count, hipMemcpyDeviceToHost, stream);
  if (e != hipSuccess) { set_error(std::string("hipMemcpyAsync: ") + hipGetErrorString(e)); return fail(s, AFX_E_HIP); }
  if ((rc = read_words(s, stream))) return fail(s, rc);
  memcpy(seen_out, seen.data(), count);
  return AFX_OK;
}
extern "C" int afx_tagset_spend(afx_tagset* s, const uint8_t* T, const uint8_t* status_in, size_t count, uint8_t* seen_out) try {
  return host_call(s, T, status_in, count, seen_out, true);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_tagset_contains(afx_tagset* s, const uint8_t* T, size_t count, uint8_t* seen_out) try {
  return host_call(s, T, nullptr, count, seen_out, false);
} catch (...) { return afx::exception_rc(); }
