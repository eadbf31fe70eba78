// The column structs of the C ABI (include/aeonflux_gpu.h), described once: which arrays each has, in struct order, how many rows each
// holds for a shape and when a call reads it - and, from that description, what every door does with them: refuse a null array the
// shape reads, stage the arrays through the door's own `in` / `res`, view consecutive rows of a transposed record as the struct, and
// list a record's cells.  Host only.  Like records.hpp, nothing here decides a staging layout: the order in which a door stages the
// main arrays, the proofs and its own arrays between them stays with the door.
#pragma once
#include <stddef.h>
#include "statements.hpp"

namespace {   // (every source file its own copy: nothing here is exported from the library)

// what a shape gives the row rules: counts, and which attribute positions are revealed (bit i)
struct Dims { uint32_t attributes, responses, proofs, revealed; };
inline Dims dims_of(const afx_shape& sh) {
  Dims d = { sh.n_attributes, sh.n_responses, sh.n_enc_proofs, 0 };
  for (uint32_t i = 0; i < sh.n_attributes && i < AFX_MAX_ATTRIBUTES; i++)
    if (sh.kinds[i] == AFX_ENC_PUBLIC_SCALAR || sh.kinds[i] == AFX_ENC_PUBLIC_POINT) d.revealed |= 1u << i;
  return d;
}
// ... of the presentation a show of these credentials makes (AFX_ATTR_* kinds; statements_prove.cpp show_dev_impl)
inline Dims dims_of(const afx_credentials_soa& cr) {
  Dims d = { cr.n_attributes, 3, 0, 0 };
  for (uint32_t i = 0; i < cr.n_attributes && i < AFX_MAX_ATTRIBUTES; i++) {
    d.responses += cr.kinds[i] == AFX_ATTR_SECRET_SCALAR;
    d.proofs += cr.kinds[i] == AFX_ATTR_SECRET_POINT;
    if (cr.kinds[i] != AFX_ATTR_SECRET_SCALAR && cr.kinds[i] != AFX_ATTR_SECRET_POINT) d.revealed |= 1u << i;
  }
  return d;
}
// an output struct's attr_values is the caller's choice whatever is revealed
inline Dims outputs(Dims d) { d.revealed = 0; return d; }

enum Per : uint8_t { FIXED, PER_ATTRIBUTE, PER_RESPONSE, PER_PROOF };
// ALWAYS; IF_ROWS: when it has rows; IF_PROOFS: with hidden group elements; IF_REVEALED: an input is read when some kind is revealed -
// and staged whenever the caller gives it, read or not, as the doors always have
enum When : uint8_t { ALWAYS, IF_ROWS, IF_PROOFS, IF_REVEALED };
struct Col {
  uint16_t at;     // offsetof the member: a pointer to bytes
  Per per;
  uint8_t fixed;   // the rows of a FIXED array
  When when;
  uint8_t elem;    // bytes per item and row
  uint32_t rows(const Dims& d) const { return per == FIXED ? fixed : per == PER_ATTRIBUTE ? d.attributes : per == PER_RESPONSE ? d.responses : d.proofs; }
  bool read(const Dims& d) const { return when == ALWAYS || (when == IF_ROWS && rows(d)) || (when == IF_PROOFS && d.proofs) || (when == IF_REVEALED && d.revealed); }
  bool staged(const Dims& d) const { return when == IF_REVEALED || read(d); }
};
#define AFX_COL(S, m, ...) { (uint16_t)offsetof(S, m), __VA_ARGS__ }
#define AFX_TWIN(A, B, m) static_assert(offsetof(A, m) == offsetof(B, m) && sizeof(A::m) == sizeof(B::m), "twin structs disagree")

// ProofOfEncryption: afx_encproof_soa and its output twin
constexpr uint32_t ENC_ROWS = 14;      // the rows of one proof: a proof's share of an AFXP record
constexpr uint32_t CM_ENC_ROWS = 5;    // afx_commitments_soa.enc[e]: the commitments of one proof, in the challenge's place in the batchable form
constexpr Col ENCPROOF_COLS[] = {
  AFX_COL(afx_encproof_soa, challenge, FIXED, 1, ALWAYS, 32), AFX_COL(afx_encproof_soa, responses, FIXED, 6, ALWAYS, 32),
  AFX_COL(afx_encproof_soa, pk, FIXED, 1, ALWAYS, 32),        AFX_COL(afx_encproof_soa, E1, FIXED, 1, ALWAYS, 32),
  AFX_COL(afx_encproof_soa, E2, FIXED, 1, ALWAYS, 32),        AFX_COL(afx_encproof_soa, C_y_1, FIXED, 1, ALWAYS, 32),
  AFX_COL(afx_encproof_soa, C_y_2, FIXED, 1, ALWAYS, 32),     AFX_COL(afx_encproof_soa, C_y_3, FIXED, 1, ALWAYS, 32),
  AFX_COL(afx_encproof_soa, C_y_2p, FIXED, 1, ALWAYS, 32),
};
static_assert(sizeof(afx_encproof_soa) == sizeof(afx_encproof_out) && sizeof(afx_encproof_soa) == 9 * sizeof(void*), "a proof of encryption has nine arrays");
AFX_TWIN(afx_encproof_soa, afx_encproof_out, challenge); AFX_TWIN(afx_encproof_soa, afx_encproof_out, responses); AFX_TWIN(afx_encproof_soa, afx_encproof_out, pk);
AFX_TWIN(afx_encproof_soa, afx_encproof_out, E1); AFX_TWIN(afx_encproof_soa, afx_encproof_out, E2); AFX_TWIN(afx_encproof_soa, afx_encproof_out, C_y_1);
AFX_TWIN(afx_encproof_soa, afx_encproof_out, C_y_2); AFX_TWIN(afx_encproof_soa, afx_encproof_out, C_y_3); AFX_TWIN(afx_encproof_soa, afx_encproof_out, C_y_2p);

// ProofOfValidCredential: afx_presentation_soa and its output twin.  `enc`, the host array of proofs, is no column: it is read when
// the shape has proofs (and no more than AFX_MAX_ATTRIBUTES), one ENCPROOF_COLS struct per proof.
constexpr Col PRESENTATION_COLS[] = {
  AFX_COL(afx_presentation_soa, challenge, FIXED, 1, ALWAYS, 32),      AFX_COL(afx_presentation_soa, responses, PER_RESPONSE, 0, IF_ROWS, 32),
  AFX_COL(afx_presentation_soa, C_x_0, FIXED, 1, ALWAYS, 32),          AFX_COL(afx_presentation_soa, C_x_1, FIXED, 1, ALWAYS, 32),
  AFX_COL(afx_presentation_soa, C_V, FIXED, 1, ALWAYS, 32),            AFX_COL(afx_presentation_soa, C_y, PER_ATTRIBUTE, 0, IF_ROWS, 32),
  AFX_COL(afx_presentation_soa, attr_values, PER_ATTRIBUTE, 0, IF_REVEALED, 32),
};
constexpr size_t NO_CHALLENGE = 1, NO_VALUES = 6;   // column ranges: [NO_CHALLENGE, ..) the batchable form's; [.., NO_VALUES) without attr_values
static_assert(sizeof(afx_presentation_soa) == sizeof(afx_presentation_out) && sizeof(afx_presentation_soa) == 8 * sizeof(void*), "a presentation has seven arrays and enc");
AFX_TWIN(afx_presentation_soa, afx_presentation_out, challenge); AFX_TWIN(afx_presentation_soa, afx_presentation_out, responses);
AFX_TWIN(afx_presentation_soa, afx_presentation_out, C_x_0); AFX_TWIN(afx_presentation_soa, afx_presentation_out, C_x_1); AFX_TWIN(afx_presentation_soa, afx_presentation_out, C_V);
AFX_TWIN(afx_presentation_soa, afx_presentation_out, C_y); AFX_TWIN(afx_presentation_soa, afx_presentation_out, attr_values); AFX_TWIN(afx_presentation_soa, afx_presentation_out, enc);

// what a show reads (Dims: dims_of(credentials))
constexpr Col CREDENTIALS_COLS[] = {
  AFX_COL(afx_credentials_soa, values, PER_ATTRIBUTE, 0, ALWAYS, 32), AFX_COL(afx_credentials_soa, M2, PER_ATTRIBUTE, 0, IF_PROOFS, 32),
  AFX_COL(afx_credentials_soa, m3, PER_ATTRIBUTE, 0, IF_PROOFS, 32),  AFX_COL(afx_credentials_soa, t, FIXED, 1, ALWAYS, 32),
  AFX_COL(afx_credentials_soa, U, FIXED, 1, ALWAYS, 32),              AFX_COL(afx_credentials_soa, V, FIXED, 1, ALWAYS, 32),
};
constexpr Col KEYPAIRS_COLS[] = {   // (read with hidden group elements; the doors ask only then)
  AFX_COL(afx_keypairs_soa, a, FIXED, 1, ALWAYS, 32), AFX_COL(afx_keypairs_soa, a0, FIXED, 1, ALWAYS, 32), AFX_COL(afx_keypairs_soa, a1, FIXED, 1, ALWAYS, 32),
  AFX_COL(afx_keypairs_soa, pk, FIXED, 1, ALWAYS, 32),
};
constexpr Col RANDOMNESS_COLS[] = {
  AFX_COL(afx_show_randomness, z_wide, FIXED, 1, ALWAYS, 64), AFX_COL(afx_show_randomness, rng_seed, FIXED, 1, ALWAYS, 32),
  AFX_COL(afx_show_randomness, enc_seeds, PER_PROOF, 0, IF_PROOFS, 32),
};
constexpr Col TAGS_COLS[] = {
  AFX_COL(afx_tags_soa, nonce, FIXED, 1, ALWAYS, 32), AFX_COL(afx_tags_soa, T, FIXED, 1, ALWAYS, 32), AFX_COL(afx_tags_soa, challenge, FIXED, 1, ALWAYS, 32),
  AFX_COL(afx_tags_soa, responses, FIXED, 2, ALWAYS, 32),
};
constexpr Col TAGS_OUT_COLS[] = {
  AFX_COL(afx_tags_out, T, FIXED, 1, ALWAYS, 32), AFX_COL(afx_tags_out, challenge, FIXED, 1, ALWAYS, 32), AFX_COL(afx_tags_out, responses, FIXED, 2, ALWAYS, 32),
};
#undef AFX_TWIN
#undef AFX_COL

// which table describes a struct, and what its members point at
template <class S> struct Described;
template <class P_, size_t N> struct DescribedBy { using P = P_; static constexpr size_t n = N; };
template <> struct Described<afx_encproof_soa> : DescribedBy<const uint8_t*, 9> { static constexpr const Col* cols = ENCPROOF_COLS; };
template <> struct Described<afx_encproof_out> : DescribedBy<uint8_t*, 9> { static constexpr const Col* cols = ENCPROOF_COLS; };
template <> struct Described<afx_presentation_soa> : DescribedBy<const uint8_t*, 7> { static constexpr const Col* cols = PRESENTATION_COLS; };
template <> struct Described<afx_presentation_out> : DescribedBy<uint8_t*, 7> { static constexpr const Col* cols = PRESENTATION_COLS; };
template <> struct Described<afx_credentials_soa> : DescribedBy<const uint8_t*, 6> { static constexpr const Col* cols = CREDENTIALS_COLS; };
template <> struct Described<afx_keypairs_soa> : DescribedBy<const uint8_t*, 4> { static constexpr const Col* cols = KEYPAIRS_COLS; };
template <> struct Described<afx_show_randomness> : DescribedBy<const uint8_t*, 3> { static constexpr const Col* cols = RANDOMNESS_COLS; };
template <> struct Described<afx_tags_soa> : DescribedBy<const uint8_t*, 4> { static constexpr const Col* cols = TAGS_COLS; };
template <> struct Described<afx_tags_out> : DescribedBy<uint8_t*, 3> { static constexpr const Col* cols = TAGS_OUT_COLS; };
static_assert(sizeof ENCPROOF_COLS / sizeof(Col) == 9 && sizeof PRESENTATION_COLS / sizeof(Col) == 7 && sizeof CREDENTIALS_COLS / sizeof(Col) == 6 &&
              sizeof KEYPAIRS_COLS / sizeof(Col) == 4 && sizeof RANDOMNESS_COLS / sizeof(Col) == 3 && sizeof TAGS_COLS / sizeof(Col) == 4 &&
              sizeof TAGS_OUT_COLS / sizeof(Col) == 3, "column counts");
template <class S> using ptr_of = typename Described<S>::P;
template <class S> inline ptr_of<S>& array_at(S& s, const Col& c) { return *(ptr_of<S>*)((char*)&s + c.at); }
template <class S> inline ptr_of<S> array_at(const S& s, const Col& c) { return *(const ptr_of<S>*)((const char*)&s + c.at); }
constexpr size_t ALL = ~size_t(0);

// ---- is an array the shape reads null: columns [from, ..) of one struct, and a presentation's with its proofs' ----
template <class S> inline bool any_null(const S& s, const Dims& d, size_t from = 0) {
  for (size_t k = from; k < Described<S>::n; k++)
    if (Described<S>::cols[k].read(d) && !array_at(s, Described<S>::cols[k])) return true;
  return false;
}
// (from = NO_CHALLENGE: the batchable form, whose callers look at the commitment arrays themselves; an output struct: outputs(d))
template <class S> inline bool any_null_with_proofs(const S& b, const Dims& d, size_t from = 0) {
  if (any_null(b, d, from) || (d.proofs && !b.enc)) return true;
  for (uint32_t e = 0; e < d.proofs; e++)
    if (any_null(b.enc[e], d, from)) return true;
  return false;
}

// the batchable form: no challenges, the commitment rows in their place
inline bool batchable_any_null(const afx_presentation_soa& b, const afx_commitments_soa& cm, const Dims& d) {
  if (!cm.main || (d.proofs && !cm.enc) || any_null_with_proofs(b, d, NO_CHALLENGE)) return true;
  for (uint32_t e = 0; e < d.proofs; e++)
    if (!cm.enc[e]) return true;
  return false;
}

// ---- staging: columns [from, to) in struct order through the door's own callable ----
// f(pointer, rows, elem) stages one array and returns where (a Stager offset), or NO_ARRAY: the device struct gets a null pointer
// there.  It is given a null pointer for an array the shape does not read.  Where the offsets point is known only after the upload:
// on_device() then makes the struct.
constexpr size_t NO_ARRAY = ~size_t(0);
template <class S> struct Offsets { size_t at[Described<S>::n]; Offsets() { for (size_t& o : at) o = NO_ARRAY; } };
template <class S, class F> inline void stage(Offsets<S>& o, const S& s, const Dims& d, F&& f, size_t from = 0, size_t to = ALL) {
  for (size_t k = from; k < Described<S>::n && k < to; k++) {
    const Col& c = Described<S>::cols[k];
    o.at[k] = f(c.staged(d) ? array_at(s, c) : ptr_of<S>(nullptr), (size_t)c.rows(d), (size_t)c.elem);
  }
}
template <class S, class F> inline Offsets<S> stage(const S& s, const Dims& d, F&& f, size_t from = 0, size_t to = ALL) {
  Offsets<S> o;
  stage(o, s, d, f, from, to);
  return o;
}
// the struct over the staged arrays; `base` gives the members that are no arrays (a credential's kinds)
template <class S> inline S on_device(const Stager& st, const Offsets<S>& o, S base = S()) {
  for (size_t k = 0; k < Described<S>::n; k++) array_at(base, Described<S>::cols[k]) = o.at[k] == NO_ARRAY ? nullptr : st.dev(o.at[k]);
  return base;
}
template <class S> inline std::vector<S> on_device(const Stager& st, const std::vector<Offsets<S>>& o) {
  std::vector<S> v(o.size());
  for (size_t e = 0; e < o.size(); e++) v[e] = on_device(st, o[e]);
  return v;
}

// ---- a run of consecutive rows of a transposed record as the struct: columns [from, to) from row `first` on ----
template <class S, class RowP> inline void view_rows(S& s, const Dims& d, RowP&& rowp, uint32_t first, size_t from = 0, size_t to = ALL) {
  for (size_t k = from; k < Described<S>::n && k < to; k++) {
    array_at(s, Described<S>::cols[k]) = rowp(first);
    first += Described<S>::cols[k].rows(d);
  }
}

// ---- the cells of a record in order: fn(array, row) for every row of columns [from, ..) that is sent - of attr_values the rows of
// revealed kinds; an absent array has none ----
template <class S, class Fn> inline void each_cell(const S& s, const Dims& d, Fn&& fn, size_t from = 0) {
  for (size_t k = from; k < Described<S>::n; k++) {
    const Col& c = Described<S>::cols[k];
    const ptr_of<S> p = array_at(s, c);
    for (uint32_t r = 0; p && r < c.rows(d); r++)
      if (c.when != IF_REVEALED || (d.revealed >> r & 1)) fn(p, r);
  }
}

}  // namespace
