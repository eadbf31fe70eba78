// Kernels of the spent-tag set (include/aeonflux_gpu.h "The spent-tag set"): a hash set of 32-byte tags in HBM with a check-and-insert
// call whose answers equal a sequential loop over the call's items - among equal tags of one call the LOWEST index is the fresh one,
// whatever order the hardware runs the lanes in.
//
// No lane ever waits for another lane: no spin loop, no retry-until-visible.  Every probe loop is bounded by n_slots steps and an
// overrun sets the error word, which fails the call and the set.  Inside one launch lanes talk only through device-scope atomics on
// `owner` and `lowest`; a key written to the table is read only by LATER launches; within a launch a lane compares against the
// claimer's tag in the INPUT array, which no lane writes.
//
//   k_tagset_claim    a lane per item walks its probe sequence with old = atomicCAS(&owner[s], EMPTY, i):
//                       won the slot          atomicMin(&lowest[s], i), remember s
//                       old == KEPT           keys[s] == T[i]: spent before this call; otherwise move on
//                       old == j              T[j] == T[i]: join (atomicMin(&lowest[s], i), remember s); otherwise move on
//                     A claimed slot never changes inside the launch and a lane passes a slot only after seeing it claimed by another
//                     key, so all items of one key end at one slot - and at the slot an earlier call left the key in, if one did:
//                     nothing is ever removed, so every slot in front of it on the key's probe sequence holds another key for good.
//   k_tagset_resolve  a lane per item: seen = lowest[s] == i ? FRESH : SPENT; the fresh lane writes keys[s] = T[i] and owner[s] = KEPT
//                     and is counted (one atomic per wave).  lowest of a KEPT slot is never consulted again: it needs no reset.
//   k_tagset_contains the probe alone, nothing written but the answers.
//
// The per-lane bodies (tagset_slot, tagset_claim_item, tagset_resolve_item, tagset_contains_item) are plain C++ over four atomics
// (TS_CAS, TS_MIN, TS_OR, TS_ADD): tests/hostsim/tagset_host.cpp compiles these very statements for the host and runs them lane by
// lane in shuffled orders, and on threads under ThreadSanitizer; tests/hostsim/fake_tagset.cpp runs them behind tagset.cpp.  The
// kernels and their launchers need the HIP compiler.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/aeonflux_gpu.h"
#include "keccak.cuh"
#include "plan.h"

#if defined(__HIPCC__)
#define TS_CAS(p, expected, desired) atomicCAS((p), (expected), (desired))
#define TS_MIN(p, v) atomicMin((p), (v))
#define TS_OR(p, v) atomicOr((p), (v))
#define TS_ADD(p, v) atomicAdd((p), (v))
#elif defined(AFX_TAGSET_TEST_THREADS)
// a host build whose lanes run on threads (only tests/hostsim/tagset_host.cpp defines the macro): the four as relaxed atomics, which is
// all the device's are - ordering between the launches comes from the stream there and from joining the threads here
static inline uint32_t ts_host_cas(uint32_t* p, uint32_t expected, uint32_t desired) {
  __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
  return expected;   // (the builtin leaves the word's value here when it differs)
}
static inline uint32_t ts_host_min(uint32_t* p, uint32_t v) {
  uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v < old && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old;
}
#define TS_CAS(p, expected, desired) ts_host_cas((p), (uint32_t)(expected), (uint32_t)(desired))
#define TS_MIN(p, v) ts_host_min((p), (uint32_t)(v))
#define TS_OR(p, v) __atomic_fetch_or((p), (v), __ATOMIC_RELAXED)
#define TS_ADD(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)
#else
// the host build runs one lane at a time (each order of whole lanes is one legal interleaving)
template <class T> static inline T ts_host_cas(T* p, T expected, T desired) { const T old = *p; if (old == expected) *p = desired; return old; }
template <class T> static inline T ts_host_min(T* p, T v) { const T old = *p; if (v < old) *p = v; return old; }
#define TS_CAS(p, expected, desired) ts_host_cas((p), (uint32_t)(expected), (uint32_t)(desired))
#define TS_MIN(p, v) ts_host_min((p), (uint32_t)(v))
#define TS_OR(p, v) (*(p) |= (v))
#define TS_ADD(p, v) (*(p) += (v))
#endif

struct ts_row { uint32_t w[8]; };
// 32 bytes, 16-byte aligned
__device__ __forceinline__ ts_row ts_load(const uint8_t* p) {
  ts_row r;
#if defined(__HIPCC__)
  const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
  r.w[0] = a.x; r.w[1] = a.y; r.w[2] = a.z; r.w[3] = a.w; r.w[4] = b.x; r.w[5] = b.y; r.w[6] = b.z; r.w[7] = b.w;
#else
  memcpy(r.w, p, 32);
#endif
  return r;
}
__device__ __forceinline__ void ts_store(uint8_t* p, const ts_row& r) {
#if defined(__HIPCC__)
  uint4 a, b;
  a.x = r.w[0]; a.y = r.w[1]; a.z = r.w[2]; a.w = r.w[3]; b.x = r.w[4]; b.y = r.w[5]; b.z = r.w[6]; b.w = r.w[7];
  reinterpret_cast<uint4*>(p)[0] = a;
  reinterpret_cast<uint4*>(p)[1] = b;
#else
  memcpy(p, r.w, 32);
#endif
}
__device__ __forceinline__ bool ts_equal(const ts_row& a, const ts_row& b) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) d |= a.w[i] ^ b.w[i];
  return d == 0;
}

// slot(T) = u64le(SHAKE256("aeonflux-amd/tagset/v1" || salt || T)[0..8)) mod n_slots.  The message is 86 bytes, one block at SHAKE256's
// rate of 136: the padding goes in at byte 86 (0x1F) and byte 135 (0x80), one permutation, the answer is the first lane.  The 22-byte
// prefix leaves salt || T 6 bytes off the lane grid: lane 3 + k holds words k and k + 1 of salt || T shifted by 16 bits.
__device__ __forceinline__ uint32_t tagset_slot(const uint64_t salt[4], const ts_row& t, uint32_t mask) {
  uint64_t w[8];
#pragma unroll
  for (int k = 0; k < 4; k++) { w[k] = salt[k]; w[4 + k] = (uint64_t)t.w[2 * k] | ((uint64_t)t.w[2 * k + 1] << 32); }
  uint64_t st[25];
  st[0] = 0x78756c666e6f6561ULL;   // "aeonflux"
  st[1] = 0x6761742f646d612dULL;   // "-amd/tag"
  st[2] = 0x31762f746573ULL | (w[0] << 48);   // "set/v1" || salt[0..2)
#pragma unroll
  for (int k = 0; k < 7; k++) st[3 + k] = (w[k] >> 16) | (w[k + 1] << 48);
  st[10] = (w[7] >> 16) | (0x1FULL << 48);   // byte 86: SHAKE's domain bits and the first padding bit
#pragma unroll
  for (int l = 11; l < 25; l++) st[l] = 0;
  st[16] = 0x80ULL << 56;          // byte 135: the last padding bit of the block
  keccak_f1600(st);
  return (uint32_t)st[0] & mask;   // (n_slots <= 2^31)
}

// One item of a claim launch.  T: [count][32], the call's input; slot_of[i] receives the slot the item ended at or an AFX_TAGSET_* word.
__device__ __forceinline__ void tagset_claim_item(const afx_tagset_table& t, const uint8_t* T, const uint8_t* status_in, uint32_t count, uint32_t i, uint32_t* slot_of) {
  if (status_in && status_in[i] != 0) { slot_of[i] = AFX_TAGSET_SKIP; return; }
  const ts_row me = ts_load(T + (uint64_t)i * 32);
  uint32_t s = tagset_slot(t.salt, me, t.mask);
  uint32_t found = AFX_TAGSET_NO_SLOT;
  for (uint32_t step = 0; step <= t.mask; step++, s = (s + 1) & t.mask) {
    const uint32_t old = TS_CAS(&t.owner[s], AFX_TAGSET_EMPTY, i);
    if (old == AFX_TAGSET_EMPTY) { TS_MIN(&t.lowest[s], i); found = s; break; }
    if (old != AFX_TAGSET_KEPT && old >= count) break;   // no item of this call: an earlier call died half way (the error word is set below)
    const ts_row other = old == AFX_TAGSET_KEPT ? ts_load(t.keys + (uint64_t)s * 32) : ts_load(T + (uint64_t)old * 32);
    if (!ts_equal(other, me)) continue;
    if (old == AFX_TAGSET_KEPT) found = AFX_TAGSET_OLD;
    else { TS_MIN(&t.lowest[s], i); found = s; }
    break;
  }
  if (found == AFX_TAGSET_NO_SLOT) TS_OR(&t.words[1], 1ull);
  slot_of[i] = found;
}

// One item of the resolve launch (behind the claim launch on the stream): its answer; true when the item was inserted.
__device__ __forceinline__ bool tagset_resolve_item(const afx_tagset_table& t, const uint8_t* T, uint32_t i, const uint32_t* slot_of, uint8_t* seen_out) {
  const uint32_t s = slot_of[i];
  if (s == AFX_TAGSET_SKIP) { seen_out[i] = AFX_TAG_SKIPPED; return false; }
  if (s == AFX_TAGSET_OLD) { seen_out[i] = AFX_TAG_SPENT; return false; }
  if (s > t.mask) return false;   // AFX_TAGSET_NO_SLOT: the call fails (the error word), no answer
  const bool fresh = t.lowest[s] == i;
  if (fresh) {
    ts_store(t.keys + (uint64_t)s * 32, ts_load(T + (uint64_t)i * 32));
    t.owner[s] = AFX_TAGSET_KEPT;
  }
  seen_out[i] = fresh ? AFX_TAG_FRESH : AFX_TAG_SPENT;
  return fresh;
}

// One item of a lookup: nothing in the table is written
__device__ __forceinline__ void tagset_contains_item(const afx_tagset_table& t, const uint8_t* T, uint32_t i, uint8_t* seen_out) {
  const ts_row me = ts_load(T + (uint64_t)i * 32);
  uint32_t s = tagset_slot(t.salt, me, t.mask);
  uint8_t seen = 0;
  bool ended = false;
  for (uint32_t step = 0; step <= t.mask; step++, s = (s + 1) & t.mask) {
    const uint32_t o = t.owner[s];
    if (o == AFX_TAGSET_EMPTY) { ended = true; break; }
    if (o != AFX_TAGSET_KEPT) break;   // an earlier call died half way
    if (ts_equal(ts_load(t.keys + (uint64_t)s * 32), me)) { seen = 1; ended = true; break; }
  }
  if (!ended) TS_OR(&t.words[1], 1ull);
  seen_out[i] = seen;
}

#if defined(__HIPCC__)
#include "kernels.h"

// (a set whose error word is set answers nothing and changes nothing: the host reports it at its next look)
__global__ void __launch_bounds__(AFX_BLOCK) k_tagset_claim(const afx_tagset_table t, const uint8_t* __restrict__ T, const uint8_t* __restrict__ status_in, uint32_t count,
                                                            uint32_t* __restrict__ slot_of) {
  const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= count || t.words[1] != 0) return;
  tagset_claim_item(t, T, status_in, count, item, slot_of);
}
__global__ void __launch_bounds__(AFX_BLOCK) k_tagset_resolve(const afx_tagset_table t, const uint8_t* __restrict__ T, uint32_t count, const uint32_t* __restrict__ slot_of,
                                                              uint8_t* __restrict__ seen_out) {
  const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
  bool fresh = false;
  if (item < count && t.words[1] == 0) fresh = tagset_resolve_item(t, T, item, slot_of, seen_out);
  const unsigned long long inserted = __ballot(fresh);   // every lane of the wave is here
  if ((threadIdx.x & 63u) == 0 && inserted) TS_ADD(&t.words[0], (unsigned long long)__popcll(inserted));
}
__global__ void __launch_bounds__(AFX_BLOCK) k_tagset_contains(const afx_tagset_table t, const uint8_t* __restrict__ T, uint32_t count, uint8_t* __restrict__ seen_out) {
  const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= count || t.words[1] != 0) return;
  tagset_contains_item(t, T, item, seen_out);
}

hipError_t afxk_tagset_spend(hipStream_t s, const afx_tagset_table* t, const uint8_t* T, const uint8_t* status_in, uint32_t count, uint32_t* slot_of, uint8_t* seen_out) {
  if (count == 0) return hipSuccess;
  const dim3 grid((count + AFX_BLOCK - 1) / AFX_BLOCK);
  hipLaunchKernelGGL(k_tagset_claim, grid, dim3(AFX_BLOCK), 0, s, *t, T, status_in, count, slot_of);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_tagset_resolve, grid, dim3(AFX_BLOCK), 0, s, *t, T, count, (const uint32_t*)slot_of, seen_out);
  return hipGetLastError();
}
hipError_t afxk_tagset_contains(hipStream_t s, const afx_tagset_table* t, const uint8_t* T, uint32_t count, uint8_t* seen_out) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_tagset_contains, dim3((count + AFX_BLOCK - 1) / AFX_BLOCK), dim3(AFX_BLOCK), 0, s, *t, T, count, seen_out);
  return hipGetLastError();
}
#endif   // __HIPCC__
