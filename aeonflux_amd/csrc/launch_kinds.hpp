// The launch kinds of a plan, each described ONCE (KINDS below): its name in afx_ctx_get_timing, its job struct (size, and the
// relocation of its device pointers, generated from pointers-to-members), whether its grid rows walk, what Launch::odd means when
// launches merge, and - where the launcher has the common signature - the launcher.  Host sources only (engine.hpp includes it).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include "../../include/aeonflux_gpu.h"
#include "kernels.h"
#include "plan.h"

// The optional launchers, weak: a host simulation build of the engine links the launchers it needs from tests/hostsim, and a call
// that reaches one it did not bring answers AFX_E_NO_DEVICE ("no <name> launcher in this build").  Who brings what:
//   afxk_coef, afxk_batch_weights                          fake_batchable.cpp (the batchable simulation)
//   afxk_mask_rows                                         fake_blind.cpp (blind issuance)
//   afxk_sha512_jobs, afxk_encode_to_group, afxk_sha512    fake_plaintext.cpp (without them tests/test_hostsim.py's calls of
//                                                          afx_keypairs_derive, afx_encrypt and afx_decrypt hash on the host)
//   afxk_draw                                              fake_draw.cpp (device draws)
//   afxk_encode_at, afxk_msg_gather / _expand / _status    fake_messages.cpp (whole messages)
//   afxk_sc_invert, afxk_tag_broadcast, _tag_scope_check   fake_tags.cpp (presentation tags)
//   afxk_tagset_spend, afxk_tagset_contains                fake_tagset.cpp (the spent-tag set: it runs tagset.cuh's lane bodies, as tests/hostsim/tagset_host.cpp does)
hipError_t afxk_coef(hipStream_t s, const afx_coef_job* jobs, uint32_t njobs, const afx_row* rows, const afx_pass* passes, uint32_t max_count) __attribute__((weak));
hipError_t afxk_mask_rows(hipStream_t s, const afx_mask_job* jobs, uint32_t njobs, const afx_row* rows, const afx_pass* passes, uint32_t max_count) __attribute__((weak));
hipError_t afxk_sha512_jobs(hipStream_t s, const afx_sha512_job* jobs, uint32_t njobs, const afx_row* rows, const afx_pass* passes, uint32_t max_count) __attribute__((weak));
hipError_t afxk_encode_to_group(hipStream_t s, const afx_encode_job* jobs, uint32_t njobs, const afx_row* rows, const afx_pass* passes, uint32_t max_count) __attribute__((weak));
hipError_t afxk_encode_at(hipStream_t s, const afx_encode_at_job* jobs, uint32_t njobs, const afx_row* rows, const afx_pass* passes, uint32_t max_count) __attribute__((weak));
hipError_t afxk_sha512(hipStream_t s, const uint8_t* src, uint32_t stride, uint32_t offset, uint32_t len, uint8_t* out, uint32_t count) __attribute__((weak));
hipError_t afxk_draw(hipStream_t s, const afx_draw_job* jobs, uint32_t njobs, uint32_t max_count) __attribute__((weak));
hipError_t afxk_batch_weights(hipStream_t s, const uint8_t* seed, uint64_t index0, uint32_t label, uint32_t n_weights, uint32_t count, uint8_t* weights) __attribute__((weak));
hipError_t afxk_msg_gather(hipStream_t s, const afx_gather_job* job) __attribute__((weak));
hipError_t afxk_msg_expand(hipStream_t s, const afx_expand_job* job) __attribute__((weak));
hipError_t afxk_msg_status(hipStream_t s, const afx_msgstat_job* job) __attribute__((weak));
hipError_t afxk_sc_invert(hipStream_t s, const uint8_t* a, const uint8_t* b, uint8_t* out, uint32_t count) __attribute__((weak));
hipError_t afxk_tag_broadcast(hipStream_t s, const uint8_t* enc, uint8_t* rows, uint32_t count) __attribute__((weak));
hipError_t afxk_tag_scope_check(hipStream_t s, const uint8_t* enc, uint8_t* ok) __attribute__((weak));
hipError_t afxk_tagset_spend(hipStream_t s, const afx_tagset_table* t, const uint8_t* T, const uint8_t* status_in, uint32_t count, uint32_t* slot_of, uint8_t* seen_out)
    __attribute__((weak));
hipError_t afxk_tagset_contains(hipStream_t s, const afx_tagset_table* t, const uint8_t* T, uint32_t count, uint8_t* seen_out) __attribute__((weak));

namespace afx {

void set_error(const std::string& s);

// The order and the values stay: timing slots are indexed by them (L_MSM_WINDOW keeps the slot the single k_msm kernel had).
enum LaunchKind { L_FILL_BAD, L_DECODE, L_SCCHECK, L_POINTOP, L_SCALAROP, L_MSM_WINDOW, L_HASH, L_FROM_UNIFORM, L_REDUCE_WIDE, L_COPY, L_FINISH,
                  L_MSM_FIXED, L_MSM_NAF, L_MSM_TABLES, L_COMPRESS, L_POINTSUM, L_NEGENC, L_TABLE_AFFINE, L_POWERS, L_COEF, L_SHA512, L_ENCODE, L_MASK, L_ENCODE_AT, L_KINDS };
// Timing slots past the launch kinds: the two cooperative kernels an L_HASH launch may take instead of k_hash (kernels.hip
// afxk_hash_coop), counted apart so that a test can say which kernel it ran.  "k_hash" (afx_ctx_get_timing) stays the three together.
// T_SC_INVERT: the direct launch in front of a tagged show's passes (statements_tags.cpp), no launch kind of a plan.
enum TimingSlot { T_HASH_COOP = L_KINDS, T_HASH_COOP64, T_SC_INVERT, T_SLOTS };

// Relocation: a pointer moves with the range it points into (end inclusive: one-past-the-end pointers of empty rows move along)
struct Mover {
  struct R { uintptr_t lo, hi; intptr_t delta; } r[4];
  template <class T>
  void fix(T*& p) const {
    const uintptr_t v = (uintptr_t)p;
    if (!v) return;
    for (const R& x : r)
      if (x.hi > x.lo && v >= x.lo && v <= x.hi) { p = (T*)(v + x.delta); return; }
  }
  template <class T>
  void fix(const T*& p) const { T* q = const_cast<T*>(p); fix(q); p = q; }
  template <class T, size_t N>
  void fix(T (&a)[N]) const { for (T& p : a) fix(p); }   // (an array of pointers: afx_powers_job::out)
};
// the relocation of a job array from the struct's pointer members: a member that holds no pointer, or of another struct, does not compile
template <class J, auto... M>
void fix_jobs(const Mover& m, uint8_t* j0, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) {
    J& j = ((J*)j0)[i];
    (m.fix(j.*M), ...);
  }
}
// Launch::odd when the same kernel stands at the head of several plans (run_plans): it says nothing, only launches of equal `odd`
// merge (k_msm_tables: the kind of table), or the merged launch has it when one of its parts has (k_decode: Elligator jobs;
// k_pointsum: a sum of sixteen parts or more)
enum OddRule { ODD_IGNORED, ODD_EQUAL, ODD_OR };

struct KindInfo {
  LaunchKind kind;
  const char* name;        // afx_ctx_get_timing
  size_t job_size;         // bytes of one job; 0: the launch has no jobs (L_COPY: its two pointers are in the Launch)
  const char* job_type;    // job_tag<J>()
  void (*fix)(const Mover& m, uint8_t* jobs, uint32_t njobs);
  bool walks;              // grid rows WALK a range of the launch's jobs (afx_walk_row) instead of taking one job each (afx_row)
  OddRule odd;
  // the launcher, where it has the common signature (null: run_plans has a case of its own): AFX_OK, AFX_E_NO_DEVICE when this
  // build lacks it, or AFX_E_HIP with `call` in the error text
  int (*run)(const KindInfo& k, hipStream_t s, const uint8_t* jobs, uint32_t njobs, const afx_row* rows, const afx_pass* passes, uint32_t max_count);
  const char* call;
};

// names the job's type in constant expressions (a text that holds "J = <type>"; compared with same_text below)
template <class J> constexpr const char* job_tag() { return __PRETTY_FUNCTION__; }
constexpr bool same_text(const char* a, const char* b) { while (*a && *a == *b) a++, b++; return *a == *b; }
template <class J>
using Launcher = hipError_t(hipStream_t, const J*, uint32_t, const afx_row*, const afx_pass*, uint32_t);
// OPTIONAL: a build may lack the launcher (a weak reference, above)
template <class J, Launcher<J>* F, bool OPTIONAL>
int run_common(const KindInfo& k, hipStream_t s, const uint8_t* jobs, uint32_t njobs, const afx_row* rows, const afx_pass* passes, uint32_t max_count) {
  if constexpr (OPTIONAL)
    if (!F) { set_error(std::string("no ") + k.name + " launcher in this build"); return AFX_E_NO_DEVICE; }
  const hipError_t e = F(s, (const J*)jobs, njobs, rows, passes, max_count);
  if (e != hipSuccess) { set_error(std::string(k.call) + ": " + hipGetErrorString(e)); return AFX_E_HIP; }
  return AFX_OK;
}
#define AFX_COMMON(J, F) &run_common<J, F, false>, #F "(s, (const " #J "*)jobs, nrows, rw, passes, max_count)"
#define AFX_OPTIONAL(J, F) &run_common<J, F, true>, #F "(s, (const " #J "*)jobs, nrows, rw, passes, max_count)"

template <class J, auto... M>
constexpr KindInfo kind_of(LaunchKind k, const char* name, bool walks = false, OddRule odd = ODD_IGNORED, decltype(KindInfo::run) run = nullptr, const char* call = nullptr) {
  return { k, name, sizeof(J), job_tag<J>(), &fix_jobs<J, M...>, walks, odd, run, call };
}
template <class J, auto... M>
constexpr KindInfo kind_of(LaunchKind k, const char* name, decltype(KindInfo::run) run, const char* call) { return kind_of<J, M...>(k, name, false, ODD_IGNORED, run, call); }

// the three chain kernels share a job struct (its terms lie in a side table: term_tables_)
constexpr KindInfo msm_kind(LaunchKind k, const char* name) {
  return kind_of<afx_msm_djob, &afx_msm_djob::naf_sched, &afx_msm_djob::addend, &afx_msm_djob::out_enc, &afx_msm_djob::out_var, &afx_msm_djob::half_var>(k, name);
}

// In the enum's order (checked below).  Side tables that hold pointers themselves (a job's terms, a sum's parts, a transcript's field
// and output tables) are not here: the Assembler lists them as it writes them (put_ptrs, term_tables_).
inline constexpr KindInfo KINDS[] = {
  kind_of<afx_fill_job, &afx_fill_job::p>(L_FILL_BAD, "k_fill_u32"),
  kind_of<afx_decode_job, &afx_decode_job::enc, &afx_decode_job::out>(L_DECODE, "k_decode", false, ODD_OR),
  kind_of<afx_sccheck_job, &afx_sccheck_job::sc>(L_SCCHECK, "k_sccheck", AFX_COMMON(afx_sccheck_job, afxk_sccheck)),
  kind_of<afx_pointop_job, &afx_pointop_job::a, &afx_pointop_job::b, &afx_pointop_job::b_const, &afx_pointop_job::out, &afx_pointop_job::out_enc>(
      L_POINTOP, "k_pointop", AFX_COMMON(afx_pointop_job, afxk_pointop)),
  kind_of<afx_scalarop_job, &afx_scalarop_job::a, &afx_scalarop_job::b, &afx_scalarop_job::c, &afx_scalarop_job::out>(
      L_SCALAROP, "k_scalarop", AFX_COMMON(afx_scalarop_job, afxk_scalarop)),
  msm_kind(L_MSM_WINDOW, "k_msm_window"),
  kind_of<afx_hash_program, &afx_hash_program::init_state, &afx_hash_program::load_state, &afx_hash_program::save_state, &afx_hash_program::records,
          &afx_hash_program::fields, &afx_hash_program::outs, &afx_hash_program::challenge, &afx_hash_program::trace>(L_HASH, "k_hash"),
  kind_of<afx_uniform_job, &afx_uniform_job::wide, &afx_uniform_job::out_enc, &afx_uniform_job::out_var>(
      L_FROM_UNIFORM, "k_from_uniform", AFX_COMMON(afx_uniform_job, afxk_from_uniform_jobs)),
  kind_of<afx_reduce_job, &afx_reduce_job::wide, &afx_reduce_job::out>(L_REDUCE_WIDE, "k_reduce_wide", AFX_COMMON(afx_reduce_job, afxk_reduce_wide_jobs)),
  { L_COPY, "copy", 0, nullptr, nullptr, false, ODD_IGNORED, nullptr, nullptr },
  kind_of<afx_finish_job, &afx_finish_job::bad, &afx_finish_job::status>(L_FINISH, "k_finish"),
  msm_kind(L_MSM_FIXED, "k_msm_fixed"),
  msm_kind(L_MSM_NAF, "k_msm_naf"),
  kind_of<afx_table_job, &afx_table_job::var>(L_MSM_TABLES, "k_msm_tables", false, ODD_EQUAL),
  kind_of<afx_compress_job, &afx_compress_job::var, &afx_compress_job::out_enc>(L_COMPRESS, "k_compress2x", true),
  kind_of<afx_pointsum_job, &afx_pointsum_job::parts, &afx_pointsum_job::addend, &afx_pointsum_job::out_var, &afx_pointsum_job::half_var, &afx_pointsum_job::out_enc>(
      L_POINTSUM, "k_pointsum", false, ODD_OR),
  kind_of<afx_negenc_job, &afx_negenc_job::enc, &afx_negenc_job::var, &afx_negenc_job::out_enc>(L_NEGENC, "k_negenc", true),
  kind_of<afx_table_job, &afx_table_job::var>(L_TABLE_AFFINE, "k_table_affine", true),
  kind_of<afx_powers_job, &afx_powers_job::src, &afx_powers_job::out>(L_POWERS, "k_powers", AFX_COMMON(afx_powers_job, afxk_powers)),
  kind_of<afx_coef_job, &afx_coef_job::weights, &afx_coef_job::triples, &afx_coef_job::operands, &afx_coef_job::out>(L_COEF, "k_coef", AFX_OPTIONAL(afx_coef_job, afxk_coef)),
  kind_of<afx_sha512_job, &afx_sha512_job::src, &afx_sha512_job::out, &afx_sha512_job::copy>(L_SHA512, "k_sha512", AFX_OPTIONAL(afx_sha512_job, afxk_sha512_jobs)),
  kind_of<afx_encode_job, &afx_encode_job::msgs, &afx_encode_job::M1, &afx_encode_job::counters, &afx_encode_job::zero_a, &afx_encode_job::zero_b>(
      L_ENCODE, "k_encode_to_group", AFX_OPTIONAL(afx_encode_job, afxk_encode_to_group)),
  kind_of<afx_mask_job, &afx_mask_job::p>(L_MASK, "k_mask_rows", AFX_OPTIONAL(afx_mask_job, afxk_mask_rows)),
  kind_of<afx_encode_at_job, &afx_encode_at_job::msgs, &afx_encode_at_job::counters_in, &afx_encode_at_job::M1, &afx_encode_at_job::zero_a, &afx_encode_at_job::zero_b>(
      L_ENCODE_AT, "k_encode_at", AFX_OPTIONAL(afx_encode_at_job, afxk_encode_at)),
};
#undef AFX_COMMON
#undef AFX_OPTIONAL
inline constexpr const char* TIMING_SLOT_NAMES[] = { "k_hash_coop", "k_hash_coop64", "k_sc_invert" };   // T_HASH_COOP, T_HASH_COOP64, T_SC_INVERT

constexpr bool kinds_in_enum_order() {
  for (int k = 0; k < (int)L_KINDS; k++) if (KINDS[k].kind != k) return false;
  return true;
}
static_assert(sizeof KINDS / sizeof KINDS[0] == L_KINDS && kinds_in_enum_order(), "one KINDS entry per launch kind, in the enum's order");
static_assert(sizeof TIMING_SLOT_NAMES / sizeof TIMING_SLOT_NAMES[0] == T_SLOTS - L_KINDS, "one name per timing slot past the launch kinds");
inline const KindInfo& kind_info(LaunchKind k) { return KINDS[k]; }
inline const char* timing_name(int slot) { return slot < (int)L_KINDS ? KINDS[slot].name : TIMING_SLOT_NAMES[slot - L_KINDS]; }

// the kind a job struct belongs to; a struct that serves several kinds (afx_table_job, afx_msm_djob) has none: its caller names the kind
template <class J>
constexpr bool job_of_kind(LaunchKind k) { return KINDS[k].job_type && same_text(KINDS[k].job_type, job_tag<J>()); }
template <class J>
constexpr LaunchKind kind_of_job() {
  int found = L_KINDS, n = 0;
  for (int k = 0; k < (int)L_KINDS; k++) if (job_of_kind<J>((LaunchKind)k)) { found = k; n++; }
  return n == 1 ? (LaunchKind)found : L_KINDS;
}

}  // namespace afx
