// TEST INFRASTRUCTURE (CPU only): what the engine's statements feed their transcripts - labels, allocations, constraints - as text.
// tests/test_framing.py links this file with the engine's host sources (engine.cpp built with -DAFX_FRAMING_LOG, which makes
// SchnorrBuilder log) and the fake HIP runtime, no sanitizer, and compares the log with the reference's source text
// (tests/golden/framing.json).
//   framing_log <params file> <key file> <issuer-parameters file> <issue kinds> <show kinds> [the same five again ...]
// kinds: one digit per attribute (AFX_ATTR_*: 0 public scalar, 1 secret scalar, 2 public point, 3 either point, 4 secret point);
// "-" for <show kinds> = no presentation for this shape; a leading "!" = the user has no symmetric keypair (then only show runs).  For every shape the program makes a context and runs one item of zeros
// through afx_issue, afx_verify_issuances, afx_show and afx_verify_presentations: the kernels are no-ops, the plans are assembled as
// for any batch.  Prints one JSON line per statement built,
//   {"shape": k, "call": "issue" | "issuance_verify" | "show" | "verify", "transcript": ..., "proof": ...,
//    "allocs": [[kind, label], ...], "constraints": [[lhs point, [[scalar, point], ...]], ...]}
// variables as allocation indices (scalars and points count apart), and exits 0; a failing call is reported on stderr, exit 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/aeonflux_gpu.h"

extern "C" const char* afx_framing_log_text(void);
extern "C" void afx_framing_log_clear(void);

typedef std::vector<uint8_t> Bytes;

static Bytes rd(const char* p) {
  FILE* f = fopen(p, "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", p); exit(2); }
  Bytes v;
  uint8_t buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

static std::string quoted(const std::string& s) {
  std::string o = "\"";
  for (char c : s) {
    if (c == '"' || c == '\\') o += '\\';
    o += c;
  }
  return o + "\"";
}

static std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out(1);
  for (char c : s) {
    if (c == sep) out.emplace_back();
    else out.back() += c;
  }
  return out;
}

// the log lines since the last call, one JSON line per builder
static void flush(size_t shape, const char* call) {
  std::string open;
  std::vector<std::string> allocs, cons;
  auto emit = [&] {
    if (open.empty()) return;
    std::string line = "{\"shape\": " + std::to_string(shape) + ", \"call\": \"" + call + "\", " + open + ", \"allocs\": [";
    for (size_t i = 0; i < allocs.size(); i++) line += (i ? ", " : "") + allocs[i];
    line += "], \"constraints\": [";
    for (size_t i = 0; i < cons.size(); i++) line += (i ? ", " : "") + cons[i];
    puts((line + "]}").c_str());
    open.clear(); allocs.clear(); cons.clear();
  };
  for (const std::string& l : split(afx_framing_log_text(), '\n')) {
    if (l.empty()) continue;
    const std::vector<std::string> f = split(l, '\t');
    if (f[0] == "new" && f.size() == 3) {
      emit();
      open = "\"transcript\": " + quoted(f[1]) + ", \"proof\": " + quoted(f[2]);
    } else if ((f[0] == "scalar" || f[0] == "point") && f.size() == 2) {
      allocs.push_back("[\"" + f[0] + "\", " + quoted(f[1]) + "]");
    } else if (f[0] == "constrain" && f.size() == 3) {
      std::string c = "[" + f[1] + ", [";
      bool first = true;
      for (const std::string& t : split(f[2], ',')) {
        if (t.empty()) continue;
        const std::vector<std::string> sp = split(t, ':');
        c += std::string(first ? "" : ", ") + "[" + sp.at(0) + ", " + sp.at(1) + "]";
        first = false;
      }
      cons.push_back(c + "]]");
    } else {
      fprintf(stderr, "framing log line not understood: %s\n", l.c_str());
      exit(1);
    }
  }
  emit();
  afx_framing_log_clear();
}

#define CHECK(cond)                                                                                                 \
  do {                                                                                                              \
    if (!(cond)) {                                                                                                  \
      fprintf(stderr, "%s:%d: check failed: %s (last error: %s)\n", __FILE__, __LINE__, #cond, afx_last_error()); \
      exit(1);                                                                                                      \
    }                                                                                                               \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 6 || (argc - 1) % 5) { fprintf(stderr, "usage: framing_log <params> <key> <issuer params> <issue kinds> <show kinds> ...\n"); return 2; }
  for (int a = 1, shape = 0; a + 4 < argc; a += 5, shape++) {
    const Bytes params = rd(argv[a]), key = rd(argv[a + 1]), ip = rd(argv[a + 2]);
    const std::string ik = argv[a + 3];
    std::string sk = argv[a + 4];
    const bool no_keypair = !sk.empty() && sk[0] == '!';
    if (no_keypair) sk.erase(0, 1);
    CHECK(ip.size() == 64 && ik.size() <= AFX_MAX_ATTRIBUTES && sk.size() <= AFX_MAX_ATTRIBUTES);
    afx_ctx* ctx = nullptr;
    CHECK(afx_ctx_create(&ctx, 0, params.data(), params.size(), key.data(), key.size(), ip.data()) == AFX_OK);
    const uint32_t n = afx_ctx_n_attributes(ctx);
    afx_framing_log_clear();
    // one item; every array is zeros (and large enough for any row count the calls index: n + 5 response rows, n attribute rows)
    Bytes zeros(64 * (AFX_MAX_ATTRIBUTES + 8), 0), out(64 * (AFX_MAX_ATTRIBUTES + 8) * 16, 0);
    uint8_t status = 0;
    afx_attributes_soa attrs;
    memset(&attrs, 0, sizeof attrs);
    attrs.n_attributes = (uint32_t)ik.size();
    for (size_t i = 0; i < ik.size(); i++) attrs.kinds[i] = (uint8_t)(ik[i] - '0');
    attrs.values = zeros.data();
    const afx_issue_randomness irnd = { zeros.data(), zeros.data(), zeros.data() };
    uint8_t* o = out.data();
    const size_t row = 64 * (AFX_MAX_ATTRIBUTES + 8);
    const afx_issuance_soa iss = { o, o + row, o + 2 * row, o + 3 * row, o + 4 * row };
    CHECK(afx_issue(ctx, &attrs, &irnd, 1, &iss, &status) == AFX_OK);
    flush((size_t)shape, "issue");
    CHECK(afx_verify_issuances(ctx, &attrs, &iss, n + 5, 1, &status) == AFX_OK);
    flush((size_t)shape, "issuance_verify");
    if (sk != "-") {
      afx_credentials_soa creds;
      memset(&creds, 0, sizeof creds);
      creds.n_attributes = (uint32_t)sk.size();
      for (size_t i = 0; i < sk.size(); i++) creds.kinds[i] = (uint8_t)(sk[i] - '0');
      creds.values = creds.M2 = creds.m3 = creds.t = creds.U = creds.V = zeros.data();
      const afx_keypairs_soa kp = { zeros.data(), zeros.data(), zeros.data(), zeros.data() };
      const afx_show_randomness srnd = { zeros.data(), zeros.data(), zeros.data() };
      std::vector<afx_encproof_out> eo(AFX_MAX_ATTRIBUTES);
      for (auto& e : eo) e = afx_encproof_out{ o + 5 * row, o + 6 * row, o + 7 * row, o + 7 * row, o + 7 * row, o + 7 * row, o + 7 * row, o + 7 * row, o + 7 * row };
      const afx_presentation_out po = { o + 8 * row, o + 9 * row, o + 10 * row, o + 10 * row, o + 10 * row, o + 11 * row, o + 12 * row, eo.data() };
      afx_shape sh;
      memset(&sh, 0, sizeof sh);
      CHECK(afx_show(ctx, &creds, no_keypair ? nullptr : &kp, &srnd, 1, &po, &sh, &status) == AFX_OK);
      flush((size_t)shape, "show");
      if (no_keypair) { afx_ctx_destroy(ctx); continue; }
      std::vector<afx_encproof_soa> es(AFX_MAX_ATTRIBUTES);
      for (auto& e : es) e = afx_encproof_soa{ zeros.data(), zeros.data(), zeros.data(), zeros.data(), zeros.data(), zeros.data(), zeros.data(), zeros.data(), zeros.data() };
      const afx_presentation_soa ps = { zeros.data(), zeros.data(), zeros.data(), zeros.data(), zeros.data(), zeros.data(), zeros.data(), es.data() };
      CHECK(afx_verify_presentations(ctx, &sh, &ps, 1, &status) == AFX_OK);
      flush((size_t)shape, "verify");
    }
    afx_ctx_destroy(ctx);
  }
  return 0;
}
