// What the entry points that take bytes in and give bytes out (the "doors": wire.cpp, wire_issue.cpp, wire_user.cpp, wire_batchable.cpp,
// wire_blind.cpp, wire_blind_user.cpp) and the calls over several groups or devices (mixed.cpp, group.cpp) share on the host:
// little-endian words, the scheduling of a request's batches on one context, and one host thread per member of a group.  What a
// format's header looks like is wire_formats.hpp's (which includes this), the transposition of records on the GPU is records.hpp's,
// the splitting of a request stream request_stream.hpp's.  A header, not a source file: the host simulations under tests/ keep their
// own source lists.
#pragma once
#include <memory>
#include <string>
#include <system_error>
#include <thread>
#include <vector>
#include "statements.hpp"

namespace {   // (every source file its own copy, as before: nothing here is exported from the library)

inline uint32_t rd32(const uint8_t* b) { return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24); }
inline void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// does a request of several batches on this context leave its small batches with the collector's sessions (plans.cpp)?
inline bool joins_the_collector(afx_ctx* ctx) {
  CtxLock probe(ctx, true);
  return ctx->lock_depth == 1 && ctx->co.enabled && ctx->co.max_items && ctx->small_batch_items && !ctx->trace && !ctx->pipelining && !ctx->session;
}

// Every batch of a request on one context, as afx_issue_mixed runs its groups (mixed.cpp run_groups): `run(b)` does batch b whole;
// counts[b] == 0: nothing to launch.  With the collector on, the small batches join the collecting session; otherwise they are
// assembled into ONE set of launches of the request's own; a large batch runs by itself, in between.  `what` names a batch in the
// error of a request of several ("batch 1: ...").
template <class Run>
int run_batches(afx_ctx* ctx, const std::vector<size_t>& counts, Run&& run, const char* what = "batch") {
  size_t live = 0, only = 0;
  for (size_t b = 0; b < counts.size(); b++)
    if (counts[b]) { live++; only = b; }
  if (live == 0) return AFX_OK;
  if (live == 1) return run(only);
  int rc = AFX_OK;
  afx::Deferred deferred;
  std::unique_ptr<afx::DeferScope> defer;
  std::unique_ptr<CtxLock> lock;
  std::unique_ptr<afx::Session> ses;
  const bool join = joins_the_collector(ctx);
  if (join) defer.reset(new afx::DeferScope(&deferred));
  else lock.reset(new CtxLock(ctx));   // the session owns the context until its last flush
  if (lock && ctx->small_batch_items && !ctx->trace && !ctx->session) {
    ses.reset(new afx::Session(ctx));
    if ((rc = ses->ensure_images(0, 0))) return rc;
    uint64_t width = 0;   // as in mixed.cpp run_groups
    for (size_t cnt : counts)
      if (cnt && cnt <= ctx->small_batch_items) width += (cnt + 63) / 64;
    ctx->merge_class = afx_ctx::merge_class_of(width);
  }
  struct WidthReset { afx_ctx* c; ~WidthReset() { if (c) c->merge_class = 0; } } width_reset = { ses ? ctx : nullptr };
  try {   // (an exception must not pass the drain below: other threads' calls may sit in a session only this thread launches)
    for (size_t b = 0; b < counts.size() && !rc; b++) {
      if (!counts[b]) continue;
      const bool collect = ses && counts[b] <= ctx->small_batch_items;
      if (ses && !collect) {
        if ((rc = ses->flush())) break;
        ses->paused = true;
      }
      rc = run(b);
      if (ses) ses->paused = false;
      if (rc) set_error(std::string(what) + " " + std::to_string(b) + ": " + afx_last_error());
    }
  } catch (...) {
    if (!join) throw;
    rc = afx::exception_rc();
  }
  if (ses) {
    if (rc) ses->drop();
    else rc = ses->flush();
    ses.reset();
  }
  if (join) {
    CtxLock lk(ctx, true);
    const int rc2 = afx::drain_deferred(ctx, deferred);   // (also after a failure: the staged rows point into this request's buffers)
    if (!rc) rc = rc2;
    defer.reset();
  }
  return rc;
}

// Runs body(member k, k) for every member k of `group` on a thread of its own (member 0: the caller's thread; a member whose thread
// cannot be started runs on the caller's too); the first failure (lowest member index) is returned, with its message.  A body that
// throws - the bodies allocate - fails its member: no exception leaves a member's thread.
template <class Body>
int on_members(afx_group* group, uint32_t m, Body&& body) {
  std::vector<int> rcs(m, AFX_OK);
  std::vector<std::string> errs(m);
  auto one = [&](uint32_t k) {
    GroupPin pin(group, k, k == 0);   // the member's thread on its device's NUMA node (member 0: the caller's thread, restored)
    try {
      rcs[k] = body(afx_group_member(group, k), k);
    } catch (...) { rcs[k] = afx::exception_rc(); }
    if (rcs[k]) errs[k] = afx_last_error();   // (the error string is per thread)
  };
  std::vector<std::thread> threads;
  threads.reserve(m);
  for (uint32_t k = 1; k < m; k++) {
    try { threads.emplace_back(one, k); } catch (const std::system_error&) { one(k); }
  }
  one(0);
  for (std::thread& t : threads) t.join();
  for (uint32_t k = 0; k < m; k++)
    if (rcs[k]) { set_error("member " + std::to_string(k) + ": " + errs[k]); return rcs[k]; }
  return AFX_OK;
}

// The two ways a door's batches go over a group's members, shared by every group door (request_stream.hpp group_door, wire_blind_user.cpp).
// A small stream whole on ONE member, the next in turn (afx_group_pick_small), the calling thread on that member's NUMA node; the
// error of a group of several names the member.
template <class Body>
int on_one_member(afx_group* group, uint32_t m, Body&& body) {
  const uint32_t k = afx_group_pick_small(group);
  GroupPin pin(group, k, true);
  const int rc = body(afx_group_member(group, k));
  if (rc && m > 1) { const std::string why = afx_last_error(); set_error("member " + std::to_string(k) + ": " + why); }
  return rc;
}
// Every batch b of counts[b] items split over the members (afx_shard_bounds), one host thread per member: run(member, b, first, n)
template <class Run>
int shard_over_members(afx_group* group, uint32_t m, const std::vector<size_t>& counts, Run&& run) {
  return on_members(group, m, [&](afx_ctx* c, uint32_t k) -> int {
    for (size_t b = 0; b < counts.size(); b++) {
      size_t first = 0, n = 0;
      afx_shard_bounds(counts[b], m, k, &first, &n);
      if (n) { const int r = run(c, b, first, n); if (r) return r; }
    }
    return AFX_OK;
  });
}

}  // namespace
