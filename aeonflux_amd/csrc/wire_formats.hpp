// The six serialized formats (include/aeonflux_gpu.h: AFXP, AFXB, AFXR, AFXI, AFXQ, AFXJ), each described ONCE: FORMATS has one entry
// per format and everything that reads or writes a header - the *_wire_header_bytes, *_wire_parse, *_wire_section_bytes and *_wire_pack
// functions, the doors' answers and the stream splitters - goes through the four functions below it.  Every format is
//   magic | u32 version (1) | u32 count | u32 cells_per_record | layout words | kinds | u16 index lists (AFXP, AFXB) | zeros to 32 | records
// with count * cells_per_record * 32 bytes of records.  A seventh format is one more entry.  Where two formats differ in what they
// refuse or in the words of an error, the difference is a field of the entry: the texts are API (afx_last_error) and stay as they are.
// A header, not a source file, like doors.hpp: the host simulations under tests/ keep their own source lists.
#pragma once
#include "doors.hpp"

namespace {   // (every source file its own copy: nothing here is exported from the library)

inline bool is_hidden_kind(uint8_t k) { return k == AFX_ATTR_SECRET_SCALAR || k == AFX_ATTR_SECRET_POINT; }
// h and hs of a layout (kinds already checked to be in range)
struct Hidden { uint32_t h = 0, hs = 0; };
inline Hidden hidden_of(const uint8_t* kinds, uint32_t n) {
  Hidden r;
  for (uint32_t i = 0; i < n; i++) {
    r.h += is_hidden_kind(kinds[i]);
    r.hs += kinds[i] == AFX_ATTR_SECRET_SCALAR;
  }
  return r;
}
inline bool revealed(uint8_t kind) { return kind == AFX_ENC_PUBLIC_SCALAR || kind == AFX_ENC_PUBLIC_POINT; }
inline bool shape_ok(const afx_shape& sh) {
  if (sh.n_attributes > AFX_MAX_ATTRIBUTES || sh.n_responses > 3 + AFX_MAX_ATTRIBUTES || sh.n_hidden_scalars > AFX_MAX_ATTRIBUTES ||
      sh.n_enc_proofs > AFX_MAX_ATTRIBUTES)
    return false;
  for (uint32_t i = 0; i < sh.n_attributes; i++)
    if (sh.kinds[i] > AFX_ENC_SECRET_POINT) return false;
  return true;
}
// cells of a presentation record: `lead` rows (AFXP: the challenge; AFXB: the main proof's commitments), the responses, C_x_0 C_x_1 C_V,
// C_y, the revealed values, `per_proof` cells per proof of encryption (AFXP 14, AFXB 18)
inline uint32_t presentation_cells(const afx_shape& sh, uint32_t lead, uint32_t per_proof) {
  uint32_t pub = 0;
  for (uint32_t i = 0; i < sh.n_attributes; i++) pub += revealed(sh.kinds[i]);
  return lead + sh.n_responses + 3 + sh.n_attributes + pub + per_proof * sh.n_enc_proofs;
}
// a main proof has the commitments of the reference's statement or of the strict one: nothing else is a well-formed AFXB header
inline bool n_main_ok(const afx_shape& sh, uint32_t n_main) { return n_main == afx_batchable_n_main_of(sh, false) || n_main == afx_batchable_n_main_of(sh, true); }

// A header as read, or to be written.  The layout words a format does not carry are 0.
struct Header {
  uint32_t count = 0, cells = 0;
  uint32_t n = 0, nr = 0, hs = 0, ne = 0, n_main = 0;   // the layout words, in the order they follow cells_per_record
  size_t hdr = 0, section = 0;       // header bytes; header and records (read_section)
  const uint8_t* kinds = nullptr;    // [n]
  const uint8_t* lists = nullptr;    // u16le hidden_scalar_indices[hs], enc_indices[ne] (where the format has them)
};
constexpr uint32_t Header::* WORDS[5] = { &Header::n, &Header::nr, &Header::hs, &Header::ne, &Header::n_main };
inline afx_shape shape_of(const Header& H) {
  afx_shape sh;
  memset(&sh, 0, sizeof sh);
  sh.n_attributes = H.n; sh.n_responses = H.nr; sh.n_hidden_scalars = H.hs; sh.n_enc_proofs = H.ne;
  memcpy(sh.kinds, H.kinds, H.n);
  const uint8_t* p = H.lists;
  for (uint32_t i = 0; i < H.hs; i++, p += 2) sh.hidden_scalar_indices[i] = (uint16_t)(p[0] | (p[1] << 8));
  for (uint32_t i = 0; i < H.ne; i++, p += 2) sh.enc_indices[i] = (uint16_t)(p[0] | (p[1] << 8));
  return sh;
}

struct Format {
  const char* magic;
  uint32_t fixed;           // bytes in front of the kinds: 16 + 4 per layout word
  uint32_t n_words;         // how many of WORDS follow cells_per_record
  uint32_t max[5];          // the words' upper bounds as parse checks them at once (ANY: left to `check`)
  const char* range_text;   // ... and what it says of a word beyond
  uint8_t max_kind;
  const char* kind_text;
  bool lists;               // u16 index lists follow the kinds
  bool zero_padding;        // parse refuses padding that is not zero
  const char* noun;         // "not an AFXP v1 <noun>" from parse
  // "cells and responses match the layout": the format's own check of a header whose words, kinds and padding passed; the error, or null
  const char* (*check)(const Header&);
  // section_bytes.  section_check: what it asks of the words before it believes count and cells (null: all that parse asks - the whole
  // header is read); past_text: its error for a section longer than the blob
  const char* section_noun;
  const char* (*section_check)(const Header&);
  const char* past_text;
};
constexpr uint32_t ANY = 0xffffffffu, NA = AFX_MAX_ATTRIBUTES;
enum { AFXP, AFXB, AFXR, AFXI, AFXQ, AFXJ };
const char* const CELLS_SHAPE = "cells_per_record does not match the shape";
const char* const CELLS_LAYOUT = "cells_per_record does not match the layout";
const char* const KIND_RANGE = "attribute kind out of range";
const char* const PAST_END = "section runs past the end of the blob";
const Format FORMATS[6] = {
  { "AFXP", 32, 4, { NA, 3 + NA, NA, NA, ANY }, "shape field out of range", AFX_ENC_SECRET_POINT, CELLS_SHAPE /* (AFXP has no text of its own for a kind) */,
    true, false, "batch",
    [](const Header& H) -> const char* { return H.cells != presentation_cells(shape_of(H), 1, 14) ? CELLS_SHAPE : nullptr; },
    "section",
    [](const Header& H) -> const char* {   // bounds cells by what the largest shape has, with an error of its own
      if (H.n > NA || H.nr > 3 + NA || H.hs > NA || H.ne > NA) return "shape field out of range";
      return H.cells > 4 + 3 * NA + 14 * NA + 3 ? "cells_per_record out of range" : nullptr;
    },
    PAST_END },
  { "AFXB", 36, 5, { NA, 3 + NA, NA, NA, ANY }, "shape field out of range", AFX_ENC_SECRET_POINT, KIND_RANGE, true, false, "batch",
    [](const Header& H) -> const char* {
      const afx_shape sh = shape_of(H);
      if (!n_main_ok(sh, H.n_main)) return "n_main_commitments does not match the shape";
      return H.cells != presentation_cells(sh, H.n_main, 18) ? CELLS_SHAPE : nullptr;
    },
    "batch",   // (AFXB's section_bytes says "batch" too)
    [](const Header& H) -> const char* {   // does not bound n_responses; bounds cells by 1 .. 4096
      return H.n > NA || H.hs > NA || H.ne > NA || H.cells == 0 || H.cells > 4096 ? "shape field out of range" : nullptr;
    },
    "truncated section" },
  { "AFXR", 20, 1, { NA, ANY, ANY, ANY, ANY }, "n_attributes out of range", AFX_ATTR_SECRET_POINT, KIND_RANGE, false, false, "batch",
    [](const Header& H) -> const char* { return H.cells != H.n ? CELLS_LAYOUT : nullptr; },
    "section",
    [](const Header& H) -> const char* { return H.n > NA || H.cells != H.n ? "layout field out of range" : nullptr; },
    PAST_END },
  { "AFXI", 24, 2, { NA, NA + 5, ANY, ANY, ANY }, "layout field out of range", AFX_ATTR_SECRET_POINT, KIND_RANGE, false, false, "batch",
    [](const Header& H) -> const char* { return H.cells != 4 + H.nr + H.n ? CELLS_LAYOUT : nullptr; },
    "section",
    [](const Header& H) -> const char* { return H.n > NA || H.nr > NA + 5 || H.cells != 4 + H.nr + H.n ? "layout field out of range" : nullptr; },
    PAST_END },
  { "AFXQ", 24, 2, { NA, ANY, ANY, ANY, ANY }, "n_attributes out of range", AFX_ATTR_SECRET_POINT, KIND_RANGE, false, true, "section",
    [](const Header& H) -> const char* {
      const Hidden hd = hidden_of(H.kinds, H.n);
      if (H.nr != 1 + hd.h + hd.hs) return "n_responses does not match the kinds";
      return H.cells != 3 + 2 * hd.h + hd.hs + H.n ? CELLS_LAYOUT : nullptr;
    },
    "section", nullptr, PAST_END },
  { "AFXJ", 24, 2, { NA, ANY, ANY, ANY, ANY }, "n_attributes out of range", AFX_ATTR_SECRET_POINT, KIND_RANGE, false, true, "section",
    [](const Header& H) -> const char* {   // (n_responses is bounded behind the kinds and the padding, in words of its own)
      if (H.nr > NA + 6) return "n_responses out of range";
      return H.cells != 5 + H.nr ? CELLS_LAYOUT : nullptr;
    },
    "section", nullptr, PAST_END },
};

inline int bad_wire(const std::string& why) { set_error(why); return AFX_E_BAD_ARGS; }

// bytes of a header; 0 for counts no header carries
inline size_t header_bytes(const Format& f, uint32_t n, uint32_t hs = 0, uint32_t ne = 0) {
  if (n > NA || hs > NA || ne > NA) return 0;
  return (f.fixed + (size_t)n + (f.lists ? 2 * (size_t)hs + 2 * (size_t)ne : 0) + 31) & ~size_t(31);
}
// magic, version, count, cells and the layout words (what both readers start with)
inline int read_words(const Format& f, const uint8_t* blob, size_t len, const char* noun, Header& H) {
  if (len < f.fixed || memcmp(blob, f.magic, 4) != 0 || rd32(blob + 4) != 1) return bad_wire(std::string("not an ") + f.magic + " v1 " + noun);
  H = Header();
  H.count = rd32(blob + 8); H.cells = rd32(blob + 12);
  for (uint32_t k = 0; k < f.n_words; k++) H.*WORDS[k] = rd32(blob + 16 + 4 * k);
  return AFX_OK;
}
// The header reader: a blob of `len` bytes as one batch of the format.  whole: the records must fill the blob to its last byte
// (section_bytes reads the header alone).
inline int read_header(const Format& f, const uint8_t* blob, size_t len, Header& H, bool whole = true) {
  int rc = read_words(f, blob, len, f.noun, H);
  if (rc) return rc;
  for (uint32_t k = 0; k < f.n_words; k++)
    if (f.max[k] != ANY && H.*WORDS[k] > f.max[k]) return bad_wire(f.range_text);
  H.hdr = header_bytes(f, H.n, H.hs, H.ne);
  if (len < H.hdr) return bad_wire("truncated header");
  H.kinds = blob + f.fixed;
  H.lists = H.kinds + H.n;
  for (uint32_t i = 0; i < H.n; i++)
    if (H.kinds[i] > f.max_kind) return bad_wire(f.kind_text);
  if (f.zero_padding)   // (the padding is part of the format: a section that parses packs to the same bytes)
    for (size_t k = f.fixed + (size_t)H.n; k < H.hdr; k++)
      if (blob[k]) return bad_wire("header padding is not zero");
  if (const char* why = f.check(H)) return bad_wire(why);
  if (whole && len - H.hdr != (uint64_t)H.count * H.cells * 32) return bad_wire("record area length");   // (count * cells * 32 < 2^48)
  return AFX_OK;
}
// the length of the section that starts at blob (its header names it); the section itself is checked by read_header
inline int section_bytes(const Format& f, const uint8_t* blob, size_t len, size_t* section_len_out) {
  if (!blob || !section_len_out) return bad_wire("null argument");
  Header H;
  int rc = f.section_check ? read_words(f, blob, len, f.section_noun, H) : read_header(f, blob, len, H, false);
  if (rc) return rc;
  if (f.section_check) {
    if (const char* why = f.section_check(H)) return bad_wire(why);
    H.hdr = header_bytes(f, H.n, H.hs, H.ne);
  }
  const uint64_t total = (uint64_t)H.hdr + (uint64_t)H.count * H.cells * 32;   // (< 2^32 * 2^12 * 2^5)
  if (total > len) return bad_wire(f.past_text);
  *section_len_out = (size_t)total;
  return AFX_OK;
}
// *_wire_parse of the formats whose layout is n_attributes, n_responses and the kinds (AFXR: no n_responses, 0 comes out)
inline int parse_layout(const Format& f, const uint8_t* blob, size_t len, uint32_t* n_out, uint8_t* kinds_out, uint32_t* nr_out, size_t* count_out,
                        size_t* records_offset_out) {
  if (!blob || !n_out || !kinds_out || !nr_out || !count_out || !records_offset_out) return bad_wire("null argument");
  Header H;
  const int rc = read_header(f, blob, len, H);
  if (rc) return rc;
  memset(kinds_out, 0, AFX_MAX_ATTRIBUTES);
  memcpy(kinds_out, H.kinds, H.n);
  *n_out = H.n; *nr_out = H.nr; *count_out = H.count; *records_offset_out = H.hdr;
  return AFX_OK;
}
// what the stream splitters do at every section: its length, then the section in full
inline int read_section(const Format& f, const uint8_t* blob, size_t len, Header& H) {
  size_t sl = 0;
  int rc = section_bytes(f, blob, len, &sl);
  if (!rc) rc = read_header(f, blob, sl, H);
  H.section = sl;
  return rc;
}
// The header writer: H's count, cells, layout words and kinds; the index lists from `sh` where the format has them.
inline void write_header(const Format& f, uint8_t* h, const Header& H, const afx_shape* sh = nullptr) {
  memset(h, 0, header_bytes(f, H.n, H.hs, H.ne));
  memcpy(h, f.magic, 4);
  wr32(h + 4, 1); wr32(h + 8, H.count); wr32(h + 12, H.cells);
  for (uint32_t k = 0; k < f.n_words; k++) wr32(h + 16 + 4 * k, H.*WORDS[k]);
  memcpy(h + f.fixed, H.kinds, H.n);
  if (!f.lists) return;
  uint8_t* p = h + f.fixed + H.n;
  for (uint32_t i = 0; i < H.hs; i++) { *p++ = (uint8_t)sh->hidden_scalar_indices[i]; *p++ = (uint8_t)(sh->hidden_scalar_indices[i] >> 8); }
  for (uint32_t i = 0; i < H.ne; i++) { *p++ = (uint8_t)sh->enc_indices[i]; *p++ = (uint8_t)(sh->enc_indices[i] >> 8); }
}
// ... of a presentation format, from the shape
inline void write_header(const Format& f, uint8_t* h, const afx_shape& sh, size_t count, uint32_t cells, uint32_t n_main = 0) {
  Header H;
  H.count = (uint32_t)count; H.cells = cells;
  H.n = sh.n_attributes; H.nr = sh.n_responses; H.hs = sh.n_hidden_scalars; H.ne = sh.n_enc_proofs; H.n_main = n_main;
  H.kinds = sh.kinds;
  write_header(f, h, H, &sh);
}
// ... of a format whose layout is n_attributes, n_responses (AFXR: none) and the kinds
inline void write_header(const Format& f, uint8_t* h, size_t count, uint32_t cells, uint32_t n, uint32_t nr, const uint8_t* kinds) {
  Header H;
  H.count = (uint32_t)count; H.cells = cells; H.n = n; H.nr = nr; H.kinds = kinds;
  write_header(f, h, H);
}

}  // namespace
