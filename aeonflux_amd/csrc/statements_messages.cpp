// Whole messages (include/aeonflux_gpu.h "whole messages"): application data of any length, one key per message.
//   Plaintext::from_slice                          src/symmetric.rs:118-133 (chunks(30), the last one zero-padded)
//   CredentialRequestConstructor::append_plaintext src/user.rs:69-77
//   impl From<&RistrettoPoint> for Plaintext       src/symmetric.rs:152-161
//   "XXX shortcut if counter is known"             src/encoding.rs:54
// A batch is a byte blob and offsets[count + 1]; message i's chunks are rows chunk_first[i] .. chunk_first[i + 1] - 1 of every
// per-chunk array.  The per-chunk work is the three plans of statements_setup.cpp (plaintexts_on_device, encrypt_on_device,
// decrypt_on_device) over rows that k_msg_gather / k_msg_expand lay out in front of the first pass; what a MESSAGE's result is - its
// status, and zeros in everything of a failed one - is decided by k_msg_status behind the LAST pass, because run_chunked cuts the chunk
// rows wherever afx_ctx_set_chunk_items falls and a message's chunks straddle passes.  Everything runs in order on lane 0's stream.
#include "statements.hpp"

// (weak references, launch_kinds.hpp: a build without kernels.hip's launchers answers AFX_E_NO_DEVICE)
static int need_message_kernels() {
  if (afxk_sha512_jobs && afxk_encode_to_group && afxk_encode_at && afxk_mask_rows && afxk_msg_gather && afxk_msg_expand && afxk_msg_status) return AFX_OK;
  set_error("no whole-message kernels (k_msg_gather, k_msg_expand, k_msg_status, k_encode_at) in this build");
  return AFX_E_NO_DEVICE;
}

// ------------------------------------------------------------------------------------------------
// host only: the chunk table
// ------------------------------------------------------------------------------------------------
extern "C" uint64_t afx_message_chunks(uint64_t len) { return len / 30 + (len % 30 != 0); }   // (len + 29) / 30 without the overflow

// chunk_first[0 .. count] from offsets[0 .. count]; nothing is written unless the table is well-formed
static int chunk_table(const uint64_t* offsets, size_t count, uint32_t* chunk_first) {
  if (count > 0xfffffffeull) { set_error("too many messages in one call"); return AFX_E_BAD_ARGS; }
  uint64_t total = 0;
  for (size_t i = 0; i < count; i++) {
    if (offsets[i + 1] < offsets[i]) { set_error("message offsets decrease"); return AFX_E_BAD_ARGS; }
    total += afx_message_chunks(offsets[i + 1] - offsets[i]);
    if (total > 0xffffffffull) { set_error("more than 2^32 - 1 chunks in one call"); return AFX_E_BAD_ARGS; }
  }
  uint32_t at = 0;
  for (size_t i = 0; i < count; i++) { chunk_first[i] = at; at += (uint32_t)afx_message_chunks(offsets[i + 1] - offsets[i]); }
  chunk_first[count] = at;
  return AFX_OK;
}
extern "C" int afx_messages_chunk_table(const uint64_t* offsets, size_t count, uint32_t* chunk_first_out) try {
  if (!offsets || !chunk_first_out) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  return chunk_table(offsets, count, chunk_first_out);
} catch (...) { return afx::exception_rc(); }
// a caller's chunk_first (afx_decrypt_messages): starts at 0 and does not decrease
static int check_chunk_first(const uint32_t* chunk_first, size_t count) {
  if (count > 0xfffffffeull) { set_error("too many messages in one call"); return AFX_E_BAD_ARGS; }
  if (chunk_first[0] != 0) { set_error("chunk_first[0] is not 0"); return AFX_E_BAD_ARGS; }
  for (size_t i = 0; i < count; i++)
    if (chunk_first[i + 1] < chunk_first[i]) { set_error("chunk_first decreases"); return AFX_E_BAD_ARGS; }
  return AFX_OK;
}

// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------
namespace {
constexpr size_t align256(size_t n) { return (n + 255) & ~size_t(255); }
// the *_dev calls made while this lives run on lane 0, whose stream (afx_ctx_stream) the direct launches here use
struct OnLane0 {
  afx_ctx* c;
  int prev;
  explicit OnLane0(afx_ctx* ctx) : c(ctx), prev(ctx->force_lane) { c->force_lane = 0; }
  ~OnLane0() { c->force_lane = prev; }
};
// a batch as the kernels see it: the two tables on the device
struct Batch {
  const uint64_t* offsets = nullptr;      // device, or null where only the chunk map is needed
  const uint32_t* chunk_first = nullptr;  // device
  uint64_t bias = 0;                      // `blob` points at this byte of the caller's blob
  uint32_t count = 0, n_chunks = 0;
};
// carves device scratch out of one range
struct Carve {
  uint8_t* base;
  size_t used = 0;
  explicit Carve(uint8_t* b) : base(b) {}
  uint8_t* take(size_t n) { uint8_t* p = base ? base + used : nullptr; used += align256(n); return p; }
};

// scratch bytes of the three calls (the layout their *_core functions carve)
size_t scratch_from_messages(size_t n) { return align256(30 * n); }
size_t scratch_encrypt(size_t n) { return align256(30 * n) + 6 * align256(32 * n) + 2 * align256(n); }
size_t scratch_decrypt(size_t n) { return 6 * align256(32 * n) + align256(n); }

int gather(hipStream_t s, const uint8_t* blob, const Batch& b, uint8_t* rows30) {
  afx_gather_job g;
  memset(&g, 0, sizeof g);
  g.blob = blob; g.offsets = b.offsets; g.chunk_first = b.chunk_first; g.rows = rows30; g.bias = b.bias; g.count = b.count; g.n_chunks = b.n_chunks;
  AFX_HIP(afxk_msg_gather(s, &g));
  return AFX_OK;
}
int expand_keys(hipStream_t s, const uint8_t* a, const uint8_t* a0, const uint8_t* a1, const Batch& b, uint8_t* ka, uint8_t* ka0, uint8_t* ka1) {
  afx_expand_job e;
  memset(&e, 0, sizeof e);
  e.src[0] = a; e.src[1] = a0; e.src[2] = a1; e.dst[0] = ka; e.dst[1] = ka0; e.dst[2] = ka1;
  e.chunk_first = b.chunk_first; e.count = b.count; e.n_chunks = b.n_chunks; e.n_rows = 3;
  AFX_HIP(afxk_msg_expand(s, &e));
  return AFX_OK;
}

// afx_plaintexts_from_messages: rows of afx_plaintexts_from_bytes on the gathered chunks; per-chunk status
int from_messages_core(afx_ctx* ctx, const uint8_t* blob, const Batch& b, uint8_t* M1, uint8_t* M2, uint8_t* m3, uint32_t* counters, uint8_t* chunk_status,
                       uint8_t* scratch) {
  hipStream_t s = ctx->lane[0].stream;
  Carve cv(scratch);
  uint8_t* rows30 = cv.take(30 * (size_t)b.n_chunks);
  int rc = gather(s, blob, b, rows30);
  if (rc) return rc;
  return plaintexts_on_device(ctx, rows30, b.n_chunks, M1, M2, m3, counters, chunk_status);
}

// afx_encrypt_messages: a, a0, a1 [count] per MESSAGE; E1, E2, counters per chunk; status per message
int encrypt_messages_core(afx_ctx* ctx, const uint8_t* a, const uint8_t* a0, const uint8_t* a1, const uint8_t* blob, const Batch& b, uint8_t* E1, uint8_t* E2,
                          uint32_t* counters, uint8_t* status, uint8_t* scratch) {
  hipStream_t s = ctx->lane[0].stream;
  const size_t n = b.n_chunks;
  Carve cv(scratch);
  uint8_t* rows30 = cv.take(30 * n);
  uint8_t *ka = cv.take(32 * n), *ka0 = cv.take(32 * n), *ka1 = cv.take(32 * n);
  uint8_t *M1 = cv.take(32 * n), *M2 = cv.take(32 * n), *m3 = cv.take(32 * n);
  uint8_t *st_plain = cv.take(n), *st_enc = cv.take(n);
  int rc = AFX_OK;
  hipError_t e = hipSuccess;
  if (!(rc = gather(s, blob, b, rows30)) && !(rc = expand_keys(s, a, a0, a1, b, ka, ka0, ka1)) &&
      !(rc = plaintexts_on_device(ctx, rows30, n, M1, M2, m3, counters, st_plain)) && !(rc = encrypt_on_device(ctx, ka, ka0, ka1, M1, M2, m3, n, E1, E2, st_enc))) {
    // behind the last pass: a message fails as a whole
    afx_msgstat_job j;
    memset(&j, 0, sizeof j);
    j.chunk_status[0] = st_plain; j.chunk_status[1] = st_enc; j.status = status; j.chunk_first = b.chunk_first;
    j.keys[0] = a; j.keys[1] = a0; j.keys[2] = a1; j.n_keys = 3;
    j.rows32[0] = E1; j.rows32[1] = E2; j.words = counters;
    j.count = b.count; j.n_chunks = b.n_chunks; j.fail_code = AFX_ST_VERIFICATION_FAILURE;
    e = hipMemsetAsync(status, 0, b.count, s);
    if (e == hipSuccess) e = afxk_msg_status(s, &j);
  }
  // the per-chunk copies of the key (and the plaintext rows beside them) do not outlive the call - also when it could not be completed
  const hipError_t e2 = cv.used ? hipMemsetAsync(scratch, 0, cv.used, s) : hipSuccess;
  if (rc) return rc;
  AFX_HIP(e);
  AFX_HIP(e2);
  return AFX_OK;
}

// afx_decrypt_messages: messages [n_chunks][30], message i's bytes at 30 * chunk_first[i]
int decrypt_messages_core(afx_ctx* ctx, const uint8_t* a, const uint8_t* a0, const uint8_t* a1, const uint8_t* E1, const uint8_t* E2, const Batch& b,
                          uint8_t* messages, uint8_t* status, uint8_t* scratch) {
  hipStream_t s = ctx->lane[0].stream;
  const size_t n = b.n_chunks;
  Carve cv(scratch);
  uint8_t *ka = cv.take(32 * n), *ka0 = cv.take(32 * n), *ka1 = cv.take(32 * n);
  uint8_t *M1 = cv.take(32 * n), *M2 = cv.take(32 * n), *m3 = cv.take(32 * n);
  uint8_t* st_dec = cv.take(n);
  int rc = AFX_OK;
  hipError_t e = hipSuccess;
  if (!(rc = expand_keys(s, a, a0, a1, b, ka, ka0, ka1)) && !(rc = decrypt_on_device(ctx, ka, ka0, ka1, E1, E2, n, M1, M2, m3, messages, st_dec))) {
    // behind the last pass: nothing is released of a message one of whose chunks did not decrypt
    afx_msgstat_job j;
    memset(&j, 0, sizeof j);
    j.chunk_status[0] = st_dec; j.status = status; j.chunk_first = b.chunk_first;
    j.rows30 = messages;
    j.count = b.count; j.n_chunks = b.n_chunks; j.fail_code = AFX_ST_UNDECRYPTABLE;
    e = hipMemsetAsync(status, 0, b.count, s);
    if (e == hipSuccess) e = afxk_msg_status(s, &j);
  }
  // the per-chunk copies of the key and M1', M2', m3' of every chunk (those of failed messages included)
  const hipError_t e2 = cv.used ? hipMemsetAsync(scratch, 0, cv.used, s) : hipSuccess;
  if (rc) return rc;
  AFX_HIP(e);
  AFX_HIP(e2);
  return AFX_OK;
}

afx_sha512_job sha_job(const uint8_t* src, uint32_t stride, uint32_t len, uint8_t* out) {
  afx_sha512_job j;
  memset(&j, 0, sizeof j);
  j.src = src; j.out = out; j.stride = stride; j.len = len;
  return j;
}
// impl From<&RistrettoPoint> for Plaintext (symmetric.rs:152-161): wide = SHA-512(the point's 32 bytes); M2 = from_uniform_bytes(wide),
// m3 = wide mod l.  The decoding only decides the status (a ristretto encoding that decodes is canonical: the bytes hashed are the
// bytes given); a point that does not decode leaves zero rows.
int from_points_core(afx_ctx* ctx, const uint8_t* points, size_t count, uint8_t* M2, uint8_t* m3, uint8_t* status) {
  return run_chunked(ctx, count, [&](Assembler& as, size_t off, uint32_t) {
    uint8_t* wide = as.new_wide();
    as.decode({ { points + 32 * off, nullptr, 0, 0 } });
    as.sha512(sha_job(points + 32 * off, 32, 32, wide));
    as.reduce_wide(wide, m3 + 32 * off);
    as.from_uniform(wide, M2 + 32 * off, nullptr);
    as.wipe(wide, 64);   // the hash of what may be a hidden attribute
    as.mask({ M2 + 32 * off, m3 + 32 * off });
    as.finish(status + off, AFX_ST_VERIFICATION_FAILURE);
  });
}
// afx_plaintexts_from_bytes_at: plaintexts_on_device with the candidate at the caller's counter instead of the search
int from_bytes_at_core(afx_ctx* ctx, const uint8_t* msgs, const uint32_t* counters_in, size_t count, uint8_t* M1, uint8_t* M2, uint8_t* m3, uint8_t* status) {
  return run_chunked(ctx, count, [&](Assembler& as, size_t off, uint32_t) {
    uint8_t* wide = as.new_wide();
    as.sha512(sha_job(msgs + 30 * off, 30, 30, wide));
    as.reduce_wide(wide, m3 + 32 * off);
    as.from_uniform(wide, M2 + 32 * off, nullptr);
    const afx_encode_at_job e = { msgs + 30 * off, counters_in + off, M1 + 32 * off, M2 + 32 * off, m3 + 32 * off };
    as.encode_at(e);
    as.finish(status + off, AFX_ST_VERIFICATION_FAILURE);
  });
}

// A *_dev call's tables and scratch in the lane's own buffer (afx_ctx::Lane::msg_ws): the host tables go through a pinned image and
// have been read when this returns; the buffer is reused by the next call, which is ordered behind this one on the lane's stream.
struct DevWork {
  Batch b;
  uint8_t* scratch = nullptr;
};
int dev_work(afx_ctx* ctx, const uint64_t* offsets, const uint32_t* chunk_first, size_t count, uint64_t n_chunks, size_t scratch_bytes, DevWork& w) {
  afx_ctx::Lane& L = ctx->lane[0];
  const size_t off_bytes = offsets ? align256(8 * (count + 1)) : 0, cf_bytes = align256(4 * (count + 1));
  int rc = L.msg_ws.ensure(off_bytes + cf_bytes + scratch_bytes);
  if (rc) return rc;
  if (!L.msg_copied) AFX_HIP(hipEventCreateWithFlags(&L.msg_copied, hipEventDisableTiming));
  if (off_bytes + cf_bytes > L.msg_pin_cap) {   // (no copy is reading it: every call waits for its own below)
    if (L.msg_pin) { (void)hipHostFree(L.msg_pin); L.msg_pin = nullptr; L.msg_pin_cap = 0; }
    const size_t want = (off_bytes + cf_bytes + (size_t(1) << 16) - 1) & ~((size_t(1) << 16) - 1);
    AFX_HIP(hipHostMalloc(&L.msg_pin, want, hipHostMallocDefault));
    L.msg_pin_cap = want;
  }
  uint8_t* pin = (uint8_t*)L.msg_pin;
  if (offsets) memcpy(pin, offsets, 8 * (count + 1));
  memcpy(pin + off_bytes, chunk_first, 4 * (count + 1));
  uint8_t* dev = (uint8_t*)L.msg_ws.p;
  AFX_HIP(hipMemcpyAsync(dev, pin, off_bytes + cf_bytes, hipMemcpyHostToDevice, L.stream));
  AFX_HIP(hipEventRecord(L.msg_copied, L.stream));
  AFX_HIP(hipEventSynchronize(L.msg_copied));
  w.b.offsets = offsets ? (const uint64_t*)dev : nullptr;
  w.b.chunk_first = (const uint32_t*)(dev + off_bytes);
  w.b.bias = 0;
  w.b.count = (uint32_t)count;
  w.b.n_chunks = (uint32_t)n_chunks;
  w.scratch = dev + off_bytes + cf_bytes;
  return AFX_OK;
}
// a host-pointer call's scratch: the same buffer, never part of the staged image (nothing of it is sent)
int host_scratch(afx_ctx* ctx, size_t bytes, uint8_t** out) {
  int rc = ctx->lane[0].msg_ws.ensure(bytes + 256);
  if (rc) return rc;
  *out = (uint8_t*)ctx->lane[0].msg_ws.p;
  return AFX_OK;
}
int fetch_sync(afx_ctx* c, hipStream_t s) {
  (void)c;
  AFX_HIP(hipStreamSynchronize(s));
  return AFX_OK;
}
const uint8_t NO_BYTES[4] = { 0 };
}  // namespace

// ------------------------------------------------------------------------------------------------
// plaintexts
// ------------------------------------------------------------------------------------------------
extern "C" int afx_plaintexts_from_messages_dev(afx_ctx* ctx, const uint8_t* blob, const uint64_t* offsets, size_t count, uint8_t* M1, uint8_t* M2, uint8_t* m3,
                                                uint32_t* counters, uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !blob || !offsets || !M1 || !M2 || !m3 || !status) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  std::vector<uint32_t> cf(count + 1);
  int rc = chunk_table(offsets, count, cf.data());
  if (rc) return rc;
  const size_t n = cf[count];
  if (n == 0) return AFX_OK;
  if ((rc = need_message_kernels())) return rc;
  AFX_HIP(hipSetDevice(ctx->device));
  OnLane0 lane(ctx);
  DevWork w;
  if ((rc = dev_work(ctx, offsets, cf.data(), count, n, scratch_from_messages(n), w))) return rc;
  return from_messages_core(ctx, blob, w.b, M1, M2, m3, counters, status, w.scratch);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_plaintexts_from_messages(afx_ctx* ctx, const uint8_t* blob, const uint64_t* offsets, size_t count, uint8_t* M1, uint8_t* M2, uint8_t* m3,
                                            uint32_t* counters) try {
  CtxLock lock__(ctx);
  if (!ctx || !blob || !offsets || !M1 || !M2 || !m3) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  std::vector<uint32_t> cf(count + 1);
  int rc = chunk_table(offsets, count, cf.data());
  if (rc) return rc;
  const size_t n = cf[count], row = 32 * n;
  if (n == 0) return AFX_OK;
  if ((rc = need_message_kernels())) return rc;
  AFX_HIP(hipSetDevice(ctx->device));
  // the blob, the two tables: staged once
  Stager st(ctx);
  const size_t blob_len = (size_t)(offsets[count] - offsets[0]);
  const size_t o_blob = st.add(blob + offsets[0], blob_len), o_off = st.add((const uint8_t*)offsets, 8 * (count + 1)), o_cf = st.add((const uint8_t*)cf.data(), 4 * (count + 1)),
               o_M1 = st.add(nullptr, row), o_M2 = st.add(nullptr, row), o_m3 = st.add(nullptr, row),
               o_ctr = st.add(nullptr, 4 * n), o_st = st.add(nullptr, n);
  if ((rc = st.upload())) return rc;
  uint8_t* scratch = nullptr;
  if ((rc = host_scratch(ctx, scratch_from_messages(n), &scratch))) return rc;
  Batch b;
  b.offsets = (const uint64_t*)st.dev(o_off); b.chunk_first = (const uint32_t*)st.dev(o_cf); b.bias = offsets[0]; b.count = (uint32_t)count; b.n_chunks = (uint32_t)n;
  if ((rc = from_messages_core(ctx, st.dev(o_blob), b, st.dev(o_M1), st.dev(o_M2), st.dev(o_m3), (uint32_t*)st.dev(o_ctr), st.dev(o_st), scratch))) return rc;
  std::vector<uint8_t> status(n);
  hipStream_t s = ctx->lane[0].stream;
  AFX_HIP(hipMemcpyAsync(status.data(), st.dev(o_st), n, hipMemcpyDeviceToHost, s));
  if ((rc = fetch_sync(ctx, s))) return rc;
  for (size_t i = 0; i < n; i++)
    if (status[i]) { set_error("encode_to_group found no representative (the reference panics)"); return AFX_E_BAD_ARGS; }
  AFX_HIP(hipMemcpyAsync(M1, st.dev(o_M1), row, hipMemcpyDeviceToHost, s));
  AFX_HIP(hipMemcpyAsync(M2, st.dev(o_M2), row, hipMemcpyDeviceToHost, s));
  AFX_HIP(hipMemcpyAsync(m3, st.dev(o_m3), row, hipMemcpyDeviceToHost, s));
  if (counters) AFX_HIP(hipMemcpyAsync(counters, st.dev(o_ctr), 4 * n, hipMemcpyDeviceToHost, s));
  return fetch_sync(ctx, s);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_plaintexts_from_points_dev(afx_ctx* ctx, const uint8_t* points, size_t count, uint8_t* M2, uint8_t* m3, uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !points || !M2 || !m3 || !status) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  int rc = need_message_kernels();
  if (rc) return rc;
  return from_points_core(ctx, points, count, M2, m3, status);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_plaintexts_from_points(afx_ctx* ctx, const uint8_t* points, size_t count, uint8_t* M2, uint8_t* m3, uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !points || !M2 || !m3 || !status) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  int rc = need_message_kernels();
  if (rc) return rc;
  AFX_HIP(hipSetDevice(ctx->device));
  Stager st(ctx);
  const size_t row = 32 * count;
  const size_t o_pt = st.add(points, row), o_M2 = st.add(nullptr, row), o_m3 = st.add(nullptr, row), o_st = st.add(nullptr, count);
  if ((rc = st.upload())) return rc;
  if ((rc = from_points_core(ctx, st.dev(o_pt), count, st.dev(o_M2), st.dev(o_m3), st.dev(o_st)))) return rc;
  hipStream_t s = st.stream();
  AFX_HIP(hipMemcpyAsync(M2, st.dev(o_M2), row, hipMemcpyDeviceToHost, s));
  AFX_HIP(hipMemcpyAsync(m3, st.dev(o_m3), row, hipMemcpyDeviceToHost, s));
  AFX_HIP(hipMemcpyAsync(status, st.dev(o_st), count, hipMemcpyDeviceToHost, s));
  return fetch_sync(ctx, s);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_plaintexts_from_bytes_at_dev(afx_ctx* ctx, const uint8_t* msgs, const uint32_t* counters_in, size_t count, uint8_t* M1, uint8_t* M2, uint8_t* m3,
                                                uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !msgs || !counters_in || !M1 || !M2 || !m3 || !status) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  int rc = need_message_kernels();
  if (rc) return rc;
  return from_bytes_at_core(ctx, msgs, counters_in, count, M1, M2, m3, status);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_plaintexts_from_bytes_at(afx_ctx* ctx, const uint8_t* msgs, const uint32_t* counters_in, size_t count, uint8_t* M1, uint8_t* M2, uint8_t* m3,
                                            uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !msgs || !counters_in || !M1 || !M2 || !m3 || !status) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  int rc = need_message_kernels();
  if (rc) return rc;
  AFX_HIP(hipSetDevice(ctx->device));
  Stager st(ctx);
  const size_t row = 32 * count;
  const size_t o_msg = st.add(msgs, 30 * count), o_ctr = st.add((const uint8_t*)counters_in, 4 * count), o_M1 = st.add(nullptr, row), o_M2 = st.add(nullptr, row),
               o_m3 = st.add(nullptr, row), o_st = st.add(nullptr, count);
  if ((rc = st.upload())) return rc;
  if ((rc = from_bytes_at_core(ctx, st.dev(o_msg), (const uint32_t*)st.dev(o_ctr), count, st.dev(o_M1), st.dev(o_M2), st.dev(o_m3), st.dev(o_st)))) return rc;
  hipStream_t s = st.stream();
  AFX_HIP(hipMemcpyAsync(M1, st.dev(o_M1), row, hipMemcpyDeviceToHost, s));
  AFX_HIP(hipMemcpyAsync(M2, st.dev(o_M2), row, hipMemcpyDeviceToHost, s));
  AFX_HIP(hipMemcpyAsync(m3, st.dev(o_m3), row, hipMemcpyDeviceToHost, s));
  AFX_HIP(hipMemcpyAsync(status, st.dev(o_st), count, hipMemcpyDeviceToHost, s));
  return fetch_sync(ctx, s);
} catch (...) { return afx::exception_rc(); }

// ------------------------------------------------------------------------------------------------
// encryption and decryption of whole messages
// ------------------------------------------------------------------------------------------------
extern "C" int afx_encrypt_messages_dev(afx_ctx* ctx, const afx_keypairs_soa* kp, const uint8_t* blob, const uint64_t* offsets, size_t count, uint8_t* E1, uint8_t* E2,
                                        uint32_t* counters, uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !kp || !kp->a || !kp->a0 || !kp->a1 || !blob || !offsets || !E1 || !E2 || !status) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  std::vector<uint32_t> cf(count + 1);
  int rc = chunk_table(offsets, count, cf.data());
  if (rc) return rc;
  const size_t n = cf[count];
  if ((rc = need_message_kernels())) return rc;
  AFX_HIP(hipSetDevice(ctx->device));
  OnLane0 lane(ctx);
  DevWork w;
  if ((rc = dev_work(ctx, offsets, cf.data(), count, n, scratch_encrypt(n), w))) return rc;
  return encrypt_messages_core(ctx, kp->a, kp->a0, kp->a1, blob, w.b, E1, E2, counters, status, w.scratch);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_encrypt_messages(afx_ctx* ctx, const afx_keypairs_soa* kp, const uint8_t* blob, const uint64_t* offsets, size_t count, uint8_t* E1, uint8_t* E2,
                                    uint32_t* counters, uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !kp || !kp->a || !kp->a0 || !kp->a1 || !blob || !offsets || !E1 || !E2 || !status) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  std::vector<uint32_t> cf(count + 1);
  int rc = chunk_table(offsets, count, cf.data());
  if (rc) return rc;
  const size_t n = cf[count], row = 32 * n, krow = 32 * count;
  if ((rc = need_message_kernels())) return rc;
  AFX_HIP(hipSetDevice(ctx->device));
  // the blob, the two tables and the keys: staged once; one key row per MESSAGE goes to the device
  Stager st(ctx);
  const size_t blob_len = (size_t)(offsets[count] - offsets[0]);
  const size_t o_blob = st.add(blob_len ? blob + offsets[0] : NO_BYTES, blob_len ? blob_len : sizeof NO_BYTES), o_off = st.add((const uint8_t*)offsets, 8 * (count + 1)),
               o_cf = st.add((const uint8_t*)cf.data(), 4 * (count + 1)), o_a = st.add(kp->a, krow), o_a0 = st.add(kp->a0, krow), o_a1 = st.add(kp->a1, krow),
               o_E1 = st.add(nullptr, row + 32), o_E2 = st.add(nullptr, row + 32), o_ctr = st.add(nullptr, 4 * n + 4),
               o_st = st.add(nullptr, count);
  if ((rc = st.upload())) return rc;
  uint8_t* scratch = nullptr;
  if ((rc = host_scratch(ctx, scratch_encrypt(n), &scratch))) return rc;
  Batch b;
  b.offsets = (const uint64_t*)st.dev(o_off); b.chunk_first = (const uint32_t*)st.dev(o_cf); b.bias = offsets[0]; b.count = (uint32_t)count; b.n_chunks = (uint32_t)n;
  if ((rc = encrypt_messages_core(ctx, st.dev(o_a), st.dev(o_a0), st.dev(o_a1), st.dev(o_blob), b, st.dev(o_E1), st.dev(o_E2), (uint32_t*)st.dev(o_ctr), st.dev(o_st),
                                  scratch))) return rc;
  hipStream_t s = ctx->lane[0].stream;
  if (n) {
    AFX_HIP(hipMemcpyAsync(E1, st.dev(o_E1), row, hipMemcpyDeviceToHost, s));
    AFX_HIP(hipMemcpyAsync(E2, st.dev(o_E2), row, hipMemcpyDeviceToHost, s));
    if (counters) AFX_HIP(hipMemcpyAsync(counters, st.dev(o_ctr), 4 * n, hipMemcpyDeviceToHost, s));
  }
  AFX_HIP(hipMemcpyAsync(status, st.dev(o_st), count, hipMemcpyDeviceToHost, s));
  return fetch_sync(ctx, s);
} catch (...) { return afx::exception_rc(); }

extern "C" int afx_decrypt_messages_dev(afx_ctx* ctx, const afx_keypairs_soa* kp, const uint8_t* E1, const uint8_t* E2, const uint32_t* chunk_first, size_t count,
                                        uint8_t* messages, uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !kp || !kp->a || !kp->a0 || !kp->a1 || !E1 || !E2 || !chunk_first || !messages || !status) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  int rc = check_chunk_first(chunk_first, count);
  if (rc) return rc;
  const size_t n = chunk_first[count];
  if ((rc = need_message_kernels())) return rc;
  AFX_HIP(hipSetDevice(ctx->device));
  OnLane0 lane(ctx);
  DevWork w;
  if ((rc = dev_work(ctx, nullptr, chunk_first, count, n, scratch_decrypt(n), w))) return rc;
  return decrypt_messages_core(ctx, kp->a, kp->a0, kp->a1, E1, E2, w.b, messages, status, w.scratch);
} catch (...) { return afx::exception_rc(); }
extern "C" int afx_decrypt_messages(afx_ctx* ctx, const afx_keypairs_soa* kp, const uint8_t* E1, const uint8_t* E2, const uint32_t* chunk_first, size_t count,
                                    uint8_t* messages, uint8_t* status) try {
  CtxLock lock__(ctx);
  if (!ctx || !kp || !kp->a || !kp->a0 || !kp->a1 || !E1 || !E2 || !chunk_first || !messages || !status) { set_error("null argument"); return AFX_E_BAD_ARGS; }
  if (count == 0) return AFX_OK;
  int rc = check_chunk_first(chunk_first, count);
  if (rc) return rc;
  const size_t n = chunk_first[count], row = 32 * n, krow = 32 * count;
  if ((rc = need_message_kernels())) return rc;
  AFX_HIP(hipSetDevice(ctx->device));
  Stager st(ctx);
  const size_t o_cf = st.add((const uint8_t*)chunk_first, 4 * (count + 1)), o_a = st.add(kp->a, krow), o_a0 = st.add(kp->a0, krow), o_a1 = st.add(kp->a1, krow),
               o_E1 = st.add(n ? E1 : NO_BYTES, n ? row : sizeof NO_BYTES), o_E2 = st.add(n ? E2 : NO_BYTES, n ? row : sizeof NO_BYTES),
               o_msg = st.add(nullptr, 30 * n + 32), o_st = st.add(nullptr, count);
  if ((rc = st.upload())) return rc;
  uint8_t* scratch = nullptr;
  if ((rc = host_scratch(ctx, scratch_decrypt(n), &scratch))) return rc;
  Batch b;
  b.chunk_first = (const uint32_t*)st.dev(o_cf); b.count = (uint32_t)count; b.n_chunks = (uint32_t)n;
  if ((rc = decrypt_messages_core(ctx, st.dev(o_a), st.dev(o_a0), st.dev(o_a1), st.dev(o_E1), st.dev(o_E2), b, st.dev(o_msg), st.dev(o_st), scratch))) return rc;
  hipStream_t s = ctx->lane[0].stream;
  if (n) AFX_HIP(hipMemcpyAsync(messages, st.dev(o_msg), 30 * n, hipMemcpyDeviceToHost, s));
  AFX_HIP(hipMemcpyAsync(status, st.dev(o_st), count, hipMemcpyDeviceToHost, s));
  return fetch_sync(ctx, s);
} catch (...) { return afx::exception_rc(); }
