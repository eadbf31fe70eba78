// Records to struct-of-arrays rows and back on the GPU (kernels.hip k_aos_to_soa, k_soa_to_aos), in one place for every door that
// reads or writes serialized records: the cell -> row maps, and the two launches with what a collected call asks of them.  Nothing
// here stages anything: the Stager calls - and their order, which is the staging layout - stay with each door (batch_arrays.hpp walks
// a column struct's arrays for them, through the door's own callable).
#pragma once
#include "kernels.h"
#include "statements.hpp"

namespace {   // (every source file its own copy: nothing here is exported from the library)

// cell c of a record is row first_row + c
inline std::vector<uint32_t> identity_map(uint32_t cells, uint32_t first_row = 0) {
  std::vector<uint32_t> row_of_cell(cells);
  for (uint32_t c = 0; c < cells; c++) row_of_cell[c] = first_row + c;
  return row_of_cell;
}
// A presentation record (AFXP: lead = 1, the challenge, and 14 rows per proof of encryption; AFXB: lead = the main proof's commitments,
// 18 per proof): the rows lead | responses | C_x_0 C_x_1 C_V | C_y[n] in order, a revealed value's cell at values_row + its
// attribute position, then the proofs' rows in order from enc_row on
inline std::vector<uint32_t> presentation_map(const afx_shape& sh, uint32_t lead, uint32_t per_proof, uint32_t values_row, uint32_t enc_row) {
  std::vector<uint32_t> row_of_cell = identity_map(lead + sh.n_responses + 3 + sh.n_attributes);
  for (uint32_t i = 0; i < sh.n_attributes; i++)
    if (sh.kinds[i] == AFX_ENC_PUBLIC_SCALAR || sh.kinds[i] == AFX_ENC_PUBLIC_POINT) row_of_cell.push_back(values_row + i);
  for (uint32_t r = enc_row; r < enc_row + per_proof * sh.n_enc_proofs; r++) row_of_cell.push_back(r);
  return row_of_cell;
}
// A blind request record: its first rq cells (D, A, B, challenge, responses) are the rows from first_row on, a revealed value's cell is
// at values_row + its attribute position (the value rows of hidden positions are in no record)
inline std::vector<uint32_t> blind_request_map(const uint8_t* kinds, uint32_t n, uint32_t rq, uint32_t first_row, uint32_t values_row) {
  std::vector<uint32_t> row_of_cell = identity_map(rq, first_row);
  for (uint32_t i = 0; i < n; i++)
    if (kinds[i] != AFX_ATTR_SECRET_SCALAR && kinds[i] != AFX_ATTR_SECRET_POINT) row_of_cell.push_back(values_row + i);
  return row_of_cell;
}

// A launch beside the call's plans: nothing for a call that took item slots of an earlier call's pass (that call's transposition covers
// them), queued with the session that collects the call (`pre`: after the session's one upload; `post`: after its plans), else now.
inline int beside_the_plans(Stager& st, bool before, std::function<int()> launch) {
  if (st.app) return AFX_OK;
  if (!st.ses) return launch();
  if (before) st.ses->pre.push_back(std::move(launch));
  else st.ses->post.push_back(std::move(launch));
  return AFX_OK;
}
// (The two below are kept out of line - one copy per source file, not one per door: inlined, the std::function each builds pushes the
// doors past the compiler's growth limits and the library starts to export template instances it did not export before.)
// after the upload: the staged records at `rec` ([dn][cells][32]) into the rows of `soa` that `map` names
[[gnu::noinline]] inline int transpose_in(Stager& st, size_t rec, size_t soa, size_t map, uint32_t cells, size_t dn) {
  hipStream_t strm = st.stream();
  const uint8_t* rec_d = st.dev(rec);
  uint8_t* soa_d = st.dev(soa);
  const uint32_t* map_d = (const uint32_t*)st.dev(map);
  const uint32_t dn_ = (uint32_t)dn;
  return beside_the_plans(st, true, [=]() -> int { AFX_HIP(afxk_aos_to_soa(strm, rec_d, soa_d, map_d, cells, dn_)); return AFX_OK; });
}
// after the plan: the rows of `soa` that `map` names into the records at `out` - zeros for an item whose status (at `status`) is a failure
[[gnu::noinline]] inline int transpose_out(Stager& st, size_t soa, size_t out, size_t map, size_t status, uint32_t cells, size_t dn) {
  hipStream_t strm = st.stream();
  const uint8_t* soa_d = st.dev(soa);
  uint8_t* out_d = st.dev(out);
  const uint32_t* map_d = (const uint32_t*)st.dev(map);
  const uint8_t* st_d = st.dev(status);
  const uint32_t dn_ = (uint32_t)dn;
  return beside_the_plans(st, false, [=]() -> int { AFX_HIP(afxk_soa_to_aos(strm, soa_d, out_d, map_d, st_d, cells, dn_)); return AFX_OK; });
}

}  // namespace
