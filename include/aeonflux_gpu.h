/*
 * aeonflux_gpu.h — C ABI of the MI355X batch engine for aeonflux's credential NIZKs.
 *
 * This is the drop-in boundary: the entry points a Rust `extern "C"` shim
 *  would bind behind `Issuer::issue` (/root/reference/src/issuer.rs:111-124),
 * `Issuer::verify` (src/issuer.rs:141-147), `CredentialIssuance::verify` (src/issuer.rs:48-57)
 * and `AnonymousCredential::show` (src/credential.rs:37-46).  The reference has no FFI/plugin
 * layer of its own (Cargo.toml:22 is commented out), so the batch forms below are new; each
 * item of a batch has exactly the semantics of one call of the cited reference method.
 *
 * Conventions
 *  - Sc = 32-byte little-endian canonical scalar mod l; Pt = 32-byte compressed ristretto255.
 *  - All per-item data is struct-of-arrays: a field `f` of a batch of `count` items is one
 *    contiguous array `[count][32]`; repeated fields are `[k][count][32]` (k-major).
 *  - Pointers in the *_soa structs are HOST pointers for afx_*() calls and DEVICE pointers for
 *    the afx_*_dev() calls (inputs already resident in HBM; no PCIe in the call).
 *  - Return value: AFX_OK or a negative AFX_E_* batch-level error.  Per-item results go to
 *    status[i] (AFX_ST_*).  Inputs that would make the reference panic (out-of-range indices,
 *    length mismatches: src/nizk/presentation.rs:81,100,346,351,407) and encodings the reference
 *    cannot hold in memory (non-canonical scalars, undecodable points) give
 *    AFX_ST_VERIFICATION_FAILURE, never a fault.
 *  - The engine has NO CPU fallback: every arithmetic step runs in HIP kernels on gfx950; calls
 *    fail with AFX_E_NO_DEVICE when no GPU is usable.
 *  - Every random draw the reference makes (caller csprng and zkp's hidden thread_rng()) is an
 *    explicit input, so runs are reproducible (SURVEY.md §8b "Randomness").
 */
#ifndef AEONFLUX_GPU_H
#define AEONFLUX_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFX_MAX_ATTRIBUTES 32

/* batch-level return codes */
#define AFX_OK 0
#define AFX_E_BAD_ARGS (-1)    /* null pointer, bad length, n mismatch, unsupported shape        */
#define AFX_E_BAD_PARAMS (-2)  /* SystemParameters / key bytes do not parse (parameters.rs:92-153) */
#define AFX_E_NO_DEVICE (-3)   /* no usable HIP device / kernel image (there is no CPU fallback)  */
#define AFX_E_HIP (-4)         /* a HIP runtime call failed; see afx_last_error()                 */
#define AFX_E_NO_KEY (-5)      /* operation needs the issuer secret key but ctx has none          */
#define AFX_E_NO_MEMORY (-6)   /* host allocation (or thread creation) failed inside the library    */
#define AFX_E_FULL (-7)        /* a spent-tag set cannot be sure to hold this call's tags (afx_tagset_*) */

/* per-item status == the reference's CredentialError outcome (src/errors.rs:73-89) */
#define AFX_ST_OK 0
#define AFX_ST_VERIFICATION_FAILURE 1  /* CredentialError::VerificationFailure (errors.rs:152-156) */
#define AFX_ST_MAC_CREATION 2          /* CredentialError::MacCreation (amacs.rs:285-287)          */
#define AFX_ST_NO_SYMMETRIC_KEY 3      /* CredentialError::NoSymmetricKey (presentation.rs:150-157) */
#define AFX_ST_UNDECRYPTABLE 4         /* CredentialError::UndecryptableAttribute (symmetric.rs:285-288) */

/* amacs::Attribute (src/amacs.rs:168-179): kinds of a credential's attributes */
#define AFX_ATTR_PUBLIC_SCALAR 0
#define AFX_ATTR_SECRET_SCALAR 1
#define AFX_ATTR_PUBLIC_POINT 2
#define AFX_ATTR_EITHER_POINT 3
#define AFX_ATTR_SECRET_POINT 4

/* amacs::EncryptedAttribute (src/amacs.rs:207-217): kinds as sent in a presentation */
#define AFX_ENC_PUBLIC_SCALAR 0
#define AFX_ENC_SECRET_SCALAR 1
#define AFX_ENC_PUBLIC_POINT 2
#define AFX_ENC_SECRET_POINT 3

typedef struct afx_ctx afx_ctx;

/* The batch-uniform part of a ProofOfValidCredential (src/nizk/presentation.rs:118-127): everything
 * that is not a Sc or Pt.  Heterogeneous traffic is grouped by shape on the host. */
typedef struct {
  uint32_t n_attributes;                                /* encrypted_attributes.len()                  */
  uint8_t kinds[AFX_MAX_ATTRIBUTES];                    /* AFX_ENC_* per position                      */
  uint32_t n_responses;                                 /* proof.responses.len()                       */
  uint32_t n_hidden_scalars;                            /* hidden_scalar_indices.len()                 */
  uint16_t hidden_scalar_indices[AFX_MAX_ATTRIBUTES];
  uint32_t n_enc_proofs;                                /* proofs_of_encryption.len()                  */
  uint16_t enc_indices[AFX_MAX_ATTRIBUTES];             /* ProofOfEncryption.index (encryption.rs:36)  */
} afx_shape;

/* ProofOfEncryption (src/nizk/encryption.rs:32-41), SoA over the batch */
typedef struct {
  const uint8_t* challenge;  /* [count] Sc                      proof.challenge        */
  const uint8_t* responses;  /* [6][count] Sc                   proof.responses a,a0,a1,m3,z,z1 */
  const uint8_t* pk;         /* [count] Pt                      public_key.pk          */
  const uint8_t* E1;         /* [count] Pt                      ciphertext.E1          */
  const uint8_t* E2;         /* [count] Pt                      ciphertext.E2          */
  const uint8_t* C_y_1;      /* [count] Pt */
  const uint8_t* C_y_2;      /* [count] Pt */
  const uint8_t* C_y_3;      /* [count] Pt */
  const uint8_t* C_y_2p;     /* [count] Pt                      C_y_2_prime            */
} afx_encproof_soa;

/* ProofOfValidCredential (src/nizk/presentation.rs:118-127), SoA over the batch */
typedef struct {
  const uint8_t* challenge;    /* [count] Sc                            proof.challenge               */
  const uint8_t* responses;    /* [n_responses][count] Sc               proof.responses               */
  const uint8_t* C_x_0;        /* [count] Pt */
  const uint8_t* C_x_1;        /* [count] Pt */
  const uint8_t* C_V;          /* [count] Pt */
  const uint8_t* C_y;          /* [n_attributes][count] Pt */
  const uint8_t* attr_values;  /* [n_attributes][count] 32 B: Sc for PUBLIC_SCALAR rows, Pt for
                                  PUBLIC_POINT rows; rows of secret kinds are never read            */
  const afx_encproof_soa* enc; /* [n_enc_proofs] (host array of structs, also for *_dev calls)     */
} afx_presentation_soa;

/* ---- context ------------------------------------------------------------------------------- */

/* Build an engine context on HIP device `device`.
 *   sysparams      : SystemParameters::to_bytes layout (src/parameters.rs:155-184)
 *   amacs_key      : amacs::SecretKey::to_bytes layout (src/amacs.rs:110-125), or NULL/0 for a
 *                    user-side context (show / issuance-verify only).  Every y_i is read (the
 *                    reference's from_bytes re-reads one chunk, src/amacs.rs:148-150 — a bug).
 *   issuer_params  : C_W || I (64 B; intended IssuerParameters layout, src/issuer.rs:155,163)
 * Decompresses the generators, builds the fixed-base window tables in HBM.  A ctx may be called from any number of threads
 * at once, like the `&self` methods it stands behind: small host-pointer calls that arrive while the device is busy share
 * ONE set of kernel launches (afx_ctx_set_coalescing below); everything else takes the context in turn. */
int afx_ctx_create(afx_ctx** out, int device, const uint8_t* sysparams, size_t sysparams_len,
                   const uint8_t* amacs_key, size_t amacs_key_len, const uint8_t issuer_params[64]);
/* Overwrites device and host copies of the key and tables before freeing (Zeroize+Drop on
 * amacs::SecretKey, src/amacs.rs:64-82). */
void afx_ctx_destroy(afx_ctx* ctx);
const char* afx_last_error(void);
uint32_t afx_ctx_n_attributes(const afx_ctx* ctx);
/* The HIP stream (hipStream_t) every call on this ctx launches on; for event timing in bench.py. */
void* afx_ctx_stream(const afx_ctx* ctx);

/* Cross-call pipelining (off by default).  Off: every *_dev call runs on afx_ctx_stream(ctx), strictly ordered.
 * On: successive *_dev calls alternate between two internal streams (each with its own workspace), so the launch
 * tail and small kernels of one call overlap the next call's work; the caller guarantees the calls are independent
 * (they may share read-only inputs) and waits with afx_ctx_synchronize (or a device-wide synchronise). */
int afx_ctx_set_pipelining(afx_ctx* ctx, int enable);
int afx_ctx_synchronize(afx_ctx* ctx);

/* Strict mode (opt-in, off by default, NOT bit-compatible with the reference):
 *  - constraint #3 of the presentation proof (presentation.rs:267-273 prover, :427-433 verifier) pairs the j-th kept
 *    commitment with the generators and kind of its OWN attribute position instead of position j, in afx_show and in
 *    afx_verify_presentations; with hidden group elements only in trailing positions both modes give the same bytes,
 *    otherwise only strict-mode presentations verify, and only under a strict-mode verifier;
 *  - afx_verify_presentations requires exactly one proof of encryption per SECRET_POINT attribute, with
 *    enc_indices equal to those positions in increasing order (the reference verifies whatever is attached,
 *    presentation.rs:438-440).
 *  - the DLEQ the reference's README.md:121-122 lists as TODO: for every hidden group element i the presentation proof also
 *    shows, with its own nonce z, that C_y[i] - C_y_1 = z*(G_y[i] - G_y[0]), C_y_1 being the commitment inside that
 *    attribute's proof of encryption (C_y[i] = z*G_y[i] + M1, presentation.rs:173; C_y_1 = z*G_y[0] + M1, encryption.rs:70):
 *    the plaintext that is proven encrypted is the one the credential commits to.  Prover (afx_show) and verifier. */
int afx_ctx_set_strict(afx_ctx* ctx, int enable);

/* Schedule of the issuer key's scalars (x0, x1, y_i in Issuer::verify's Z and in Amac::tag).  Default (0): the host recodes
 * them to width-5 NAF and every lane runs that addition schedule - the fastest form, whose running time depends on the
 * key's NAF weight (a per-key constant, the same for every batch under that key; nothing depends on the items).  1: the key
 * scalars take the per-item window path instead (64 additions per term, whatever the key): running time independent of
 * the key, 3-5 % slower.  The reference computes these products with dalek's constant-time `*` / `multiscalar_mul`
 * (src/nizk/presentation.rs:342-351, src/amacs.rs:267-270); DESIGN.md section 1 "Secrets" (the threat model: docs/HISTORY.md section 1).
 * It applies to every call that multiplies by the key: afx_issue* (afx_issue_wire too), afx_verify_presentations*.
 * Results are identical in both modes. */
int afx_ctx_set_fixed_key_schedule(afx_ctx* ctx, int enable);

/* Secret-independent addressing.  The reference multiplies by secrets - the issuer key, the prover's nonces, blindings and
 * witnesses - with dalek's constant-time `*` / `multiscalar_mul` (src/amacs.rs:267-270, src/nizk/presentation.rs:162-184, zkp's
 * Prover), whose table lookups read every entry and select.  This engine's INSTRUCTION stream never depends on a per-item secret
 * in any mode; what the mode decides is whether the window digit of a secret may pick WHICH table entry a lane gathers from HBM:
 *   AFX_SECRETS_PROVER_SIDE (2, the default of a new context): not on the prover-side calls - afx_issue* (afx_issue_wire too), afx_show* and the
 *     symmetric-key helpers (afx_keypairs_derive, afx_encrypt, afx_decrypt): every scalar of every multiscalar job there but the
 *     constant 1 is treated as a secret.  What a user of the crate gets from its constant-time arithmetic.  Issuer::verify runs
 *     the fast tables (its only secret is the issuer key, see afx_ctx_set_fixed_key_schedule).
 *   AFX_SECRETS_EVERYWHERE (1): additionally on afx_verify_presentations*: every scalar of the job that computes Z - the issuer
 *     key's (which then also run the fixed schedule, whatever afx_ctx_set_fixed_key_schedule says) and the per-item products
 *     y_i * m_i of the key with revealed scalar attributes, whose digits would give the key away just the same.
 *   AFX_SECRETS_NOWHERE (0): the fastest tables everywhere (rounds 1-3 of this engine; a device of the engine's own, or inputs
 *     that are no secrets: synthetic benchmark data).  Prover-side calls of up to 2048 items run the secret-independent plan in
 *     this mode too: at those sizes it is the faster one (its chains run in segments over the bases' powers).
 * Where the mode applies no load's address is made from a digit of a secret.  A secret term on a per-item base runs 2-bit signed
 * windows: every addition reads both stored (affine) entries of its lane's table and keeps the digit's with selects - 128 additions
 * per term instead of 64.  A secret term on a generator runs 6-bit signed windows over positional tables (155 KB per generator,
 * part of every context): each lane of the wave loads one of the window's 32 multiples, the one its lane id names, and every lane
 * takes the multiple its digit names from the lane that holds it (ds_bpermute_b32: a register exchange, no memory access, source
 * lanes chosen so that no pattern of digits conflicts in the crossbar) - 43 additions per term instead of 20.  Results are
 * byte-identical in every mode.  Cost against mode 0, measured on one MI355X: issue -35 %, show -24 %;
 * verification unchanged in mode 2, -8 % in mode 1. */
#define AFX_SECRETS_NOWHERE 0
#define AFX_SECRETS_EVERYWHERE 1
#define AFX_SECRETS_PROVER_SIDE 2
int afx_ctx_set_secret_independent_addressing(afx_ctx* ctx, int mode);

/* Items per internal pass (tuning; 0 restores the default of 2^19).  A batch larger than this is processed in passes
 * of this many items, which bounds the device workspace (about 25-70 KB per item and pass, depending on the
 * statement); smaller values trade throughput for memory.  Accepted range 256 .. 2^22. */
int afx_ctx_set_chunk_items(afx_ctx* ctx, uint32_t items);

/* Small passes (default 4096 items; 0 switches the latency plans off, at most 2^16).  A call of few items leaves most of the
 * device idle, and its duration is that of its LONGEST chain of field operations - one Issuer::verify of the reference is one
 * presentation (src/issuer.rs:141-147).  Passes of at most this many items therefore give every variable-base term of every
 * multiscalar multiplication a chain of its own (a 3-term commitment becomes 3 lanes with 64 additions each instead of one
 * with 192), add the partial sums up afterwards, and encode an item's commitments in several rows.  More work in all, less
 * time per call (measured, C3 shape: 3.2 ms against 4.3 ms at 2^12 items, level at 2^13).  Passes of up to FOUR times this many items split
 * only the job that multiplies by the issuer key (Z: one grid row that cannot fill the device at such sizes) into one NAF
 * chain per term (5.0 ms against 5.8 ms at 2^13 items, 8.7 against 9.0 at 2^14).  Results are identical under every plan. */
int afx_ctx_set_small_batch_items(afx_ctx* ctx, uint32_t items);

/* Concurrent small calls (on by default).  Issuer::verify takes `&self`, keeps no state and is called one presentation at a time
 * from as many threads as a server has (src/issuer.rs:141-147); Issuer::issue (:111-124), CredentialIssuance::verify (:48-57) and
 * AnonymousCredential::show (src/credential.rs:37-46) likewise.  One such call costs one chain of field operations on a device
 * that is otherwise idle (0.8 ms), so calls that queue behind each other would cap a server at ~1.2 k calls/s whatever its thread
 * count.  Instead, host-pointer calls (afx_verify_presentations[_range,_wire,_wire_range], afx_issue[_range,_wire],
 * afx_verify_issuances[_range,_wire,_mixed_wire], afx_show[_range,_wire]) of at most 512 items that arrive while another call's kernels run are
 * COLLECTED: each stages its rows - calls of one statement, shape and mode into the free item slots of ONE pass, so 64 callers of
 * one shape are one pass of 64 items - and sleeps until the flush that carries its rows completes.  The caller that opened a
 * collection launches it as soon as the device is free, at the latest `max_wait_us` after it opened it (default 2000) or when it
 * holds `max_items` items (default 4096; at most 2^16).  A call that finds the device idle is launched at once: a single thread
 * sees the latency it saw before.  Results are byte-identical to separate calls; a flush that fails (AFX_E_HIP ...) fails every call
 * it carried with the same code and message, and the context stays usable.  max_items == 0 switches collection off (every call
 * then takes the context in turn).  Large calls, device-pointer calls and the afx_ctx_set_* functions wait for the collections
 * in flight and then have the context to themselves. */
int afx_ctx_set_coalescing(afx_ctx* ctx, uint32_t max_wait_us, uint32_t max_items);
typedef struct afx_coalescing_stats {
  uint64_t sessions;        /* sets of launches that carried collected calls                                    */
  uint64_t calls;           /* calls that went through them                                                     */
  uint64_t items;           /* ... and their items                                                              */
  uint64_t appended_calls;  /* calls that took free item slots of another call's pass (no plan of their own)    */
  uint64_t max_calls;       /* most calls one set of launches carried                                           */
  uint64_t leader_waits;    /* times a collection's opener slept because an earlier one was still computing     */
  uint64_t staging_ns;      /* time the context's lock was held while calls staged their rows (sum)             */
  uint64_t launch_ns;       /* ... and while collections were launched (sum): what serialises the callers       */
} afx_coalescing_stats;
int afx_ctx_get_coalescing_stats(afx_ctx* ctx, afx_coalescing_stats* out);

/* Plan variants (test aid; 0 = every choice automatic, the default).  Which of several equivalent layouts a SMALL pass takes is
 * decided by its size and by the width of the launch set it shares with other calls: secret scalars of a prover pass in 8, 4 or 1
 * segment(s); chains on four waves per item or one; a transcript on a wave or on 32 lanes; sums of many parts with a lane per part
 * or per item.  Every combination returns the same bytes.  The flags force the alternatives at any size, so that tests can compare
 * each of them with the CPU oracle (tests/test_gpu_plan_variants.py) instead of reaching them only through particular sizes and
 * concurrency.  AFX_VARIANT_SELFCHECK: every plan is assembled twice against different provisional addresses and the two copies,
 * relocated to the same place, must be equal byte for byte (also: AFX_PLAN_SELFCHECK=1 in the environment at context creation).
 * The flags are part of every plan's cache key.  Not a tuning interface: the automatic choice is the measured best. */
#define AFX_VARIANT_SEGMENTS_1 0x01u        /* small prover passes: whole chains                                       */
#define AFX_VARIANT_SEGMENTS_2 0x02u        /* ... two segments per secret scalar                                      */
#define AFX_VARIANT_SEGMENTS_4 0x04u        /* ... four (what passes of 257 .. 2048 items take by themselves)          */
#define AFX_VARIANT_ONE_WAVE_CHAINS 0x08u   /* no four-wave chains (what launch sets wider than 512 blocks take)       */
#define AFX_VARIANT_HASH_HALF_WAVE 0x10u    /* cooperative transcripts on 32 lanes per item (more than 2048 of them)   */
#define AFX_VARIANT_NO_POINTSUM_TREE 0x20u  /* sums of many parts on one lane per item                                 */
#define AFX_VARIANT_SELFCHECK 0x40u
#define AFX_VARIANT_ALL 0x7fu
int afx_ctx_set_plan_variants(afx_ctx* ctx, uint32_t flags);

/* Host copies of LARGE host-pointer calls (default 0: off).  Issuer::verify on a batch in host memory (src/issuer.rs:141-147
 * called over a vector of presentations) hands the engine ~2.4 KB per presentation in pageable memory.  A call of more than 16 MB
 * of rows is cut into slices of 2^17 items on two streams; each slice's rows are gathered into a pinned image by `threads` host
 * threads (the caller's own among them) that run on the CPUs of the NUMA node the device hangs off, and go to HBM in one
 * transfer per contiguous run while the previous slice computes; large results come back the same way.  0 (the default): the
 * runtime's own copies out of pageable memory, one per row, on the calling thread wherever it runs.  Measured on a two-socket
 * EPYC 9575F host (profiles/r06_host_pointer_numa.txt): with 0 the call keeps 95.6-96.6 % of the device-resident rate whether the
 * caller's thread and arrays sit on the device's node or the other one; the pool keeps 93-95.4 % (its gather is a second pass over
 * the rows that the runtime's pin-in-place transfer does not make).  It is for hosts whose runtime stages pageable copies through a
 * single thread far from the device; this pool's boxes do not.  At most 64; no more threads are started than the node has CPUs the
 * process may use.  Small calls are not affected (their rows already travel as one pinned image). */
int afx_ctx_set_host_copy_threads(afx_ctx* ctx, uint32_t threads);

/* Challenge trace (parity aid; off by default).  set(rows, count) allocates a device array [rows][count][32]; while it
 * exists, every verification call (presentations, proofs of encryption, issuances) of at most `count` items also
 * stores the challenge it RECOMPUTES for item i of proof r in cell (r, i): r = 0 for the main proof (or the only
 * one), r = 1 + e for the e-th attached proof of encryption; a call that needs more rows or items fails with
 * AFX_E_BAD_ARGS.  get() waits for the context's work and copies the array to host_out (rows * count * 32 bytes).
 * The value is what zkp's verify_compact compares with the proof's challenge (presentation.rs:435,
 * encryption.rs:209, issuance.rs:217), so equal traces mean every recomputed commitment of the item was equal too.
 * Items rejected before the transcript stage (non-canonical scalar, undecodable point) still get a value; it is
 * computed with the identity in place of the undecodable point and means nothing.  set(0, 0) frees the array. */
int afx_ctx_set_challenge_trace(afx_ctx* ctx, size_t rows, size_t count);
int afx_ctx_get_challenge_trace(afx_ctx* ctx, uint8_t* host_out);

/* Per-item operation counts of the context's most recent call (measurement aid: the compute-side figure beside the
 * HBM roofline is derived from these).  Counts are what ONE item executes, summed over all
 * the jobs of its statement; every lane executes the same schedule, so they do not depend on the data. */
typedef struct afx_plan_stats {
  uint64_t msm_jobs;           /* multiscalar multiplications (grid rows of k_msm plus chained jobs)            */
  uint64_t doublings;          /* point doublings in their shared doubling chains (4S + 3M, every fourth 4S + 4M) */
  uint64_t var_additions;      /* additions of a per-item window-table entry (8M, last of a window 7M)          */
  uint64_t fixed_additions;    /* additions of a generator-table entry (7M, last of a window 6M)                */
  uint64_t table_additions;    /* additions spent building the per-item window tables (8M)                      */
  uint64_t encodings;          /* ristretto255 encodings (1 inverse square root = 254S + 11M, plus ~14M)        */
  uint64_t decodings;          /* ristretto255 decodings (same size)                                            */
  uint64_t keccak_permutations;
  uint64_t field_mul, field_sq; /* GF(2^255-19) multiplications / squarings of all of the above, from the kernels' own
                                  schedule (tests/test_device_arith_on_host.py pins the per-block counts)        */
  uint64_t secret_terms;       /* terms of the multiscalar jobs that run with secret-independent addressing (0 unless
                                  afx_ctx_set_secret_independent_addressing is on)                               */
  uint64_t chain_mul, chain_sq; /* the share of field_mul / field_sq inside the inversion and square-root chains, which run in the
                                  10 x 25.5-bit form of the field (100 / 55 multiply-adds each instead of 98 / 62)              */
} afx_plan_stats;
int afx_ctx_get_plan_stats(afx_ctx* ctx, afx_plan_stats* out);

/* The cache of assembled plans (small host-pointer calls reuse the plan of their statement, shape, mode and padded size: about 0.3 ms
 * of host work per call).  At most 512 entries / 64 MB; the least recently used entry makes room for a new one, so a stream of
 * unusual shapes - a serialized batch names its own shape - cannot pin the cache against the shapes a server really sees. */
typedef struct afx_plan_cache_stats {
  uint64_t hits, misses;   /* small host-pointer calls that reused a plan / assembled (and cached) one                     */
  uint64_t evictions;      /* entries dropped to make room                                                                 */
  uint64_t entries, bytes; /* what the cache holds now                                                                     */
} afx_plan_cache_stats;
int afx_ctx_get_plan_cache_stats(afx_ctx* ctx, afx_plan_cache_stats* out);

/* Per-kernel device timing with HIP events on afx_ctx_stream(ctx) (measurement aid; off by default).
 * set_timing(ctx, 1) resets the counters and starts recording every launch; get_timing synchronises the
 * stream and returns the summed duration and launch count of one kernel: "k_msm_window", "k_msm_naf", "k_msm_fixed"
 * (the three multiscalar kernels: per-item windows, uniform width-5 NAF terms, fixed bases only), "k_msm_tables", or
 * "k_msm" for those four together; "k_hash" (every transcript launch, whichever kernel it took), of which "k_hash_coop" and
 * "k_hash_coop64" are the launches of the two cooperative kernels (32 lanes / a wave per item; the rest took one lane per item);
 * "k_decode", "k_pointop", "k_scalarop", "k_sccheck", "k_finish", "k_from_uniform", "k_reduce_wide", "k_fill_u32". */
int afx_ctx_set_timing(afx_ctx* ctx, int enable);
int afx_ctx_get_timing(afx_ctx* ctx, const char* kernel, double* total_ms, uint64_t* launches);
/* The core clock the k_msm_window launches recorded since set_timing(ctx, 1) actually ran at, in MHz (0 if none ran): one lane of
 * each of 64 blocks per launch - spread evenly over the launch's block order, that is over its duration and over the eight XCDs -
 * reads the shader-clock counter and the constant 100 MHz counter around its chain; get_core_clock_mhz is the MEDIAN of the 64
 * ratios, get_core_clock_samples all of them in increasing order (at most `cap` written, *n_out = how many there are).  The path
 * runs at the socket power cap, so this is below the nominal clock the multiply-add peak is usually quoted at, and a launch's
 * first blocks run faster than its last. */
int afx_ctx_get_core_clock_mhz(afx_ctx* ctx, double* mhz);
int afx_ctx_get_core_clock_samples(afx_ctx* ctx, double* mhz_out, uint32_t cap, uint32_t* n_out);

/* ---- Issuer::verify (src/issuer.rs:141-147 -> src/nizk/presentation.rs:324-443) ------------- */

/* status[i] = AFX_ST_OK iff Issuer::verify(presentation_i).is_ok().  Host pointers. */
int afx_verify_presentations(afx_ctx* ctx, const afx_shape* shape, const afx_presentation_soa* batch,
                             size_t count, uint8_t* status);
/* Same, all SoA arrays and `status` in device memory; asynchronous on afx_ctx_stream(ctx). */
int afx_verify_presentations_dev(afx_ctx* ctx, const afx_shape* shape, const afx_presentation_soa* batch,
                                 size_t count, uint8_t* status_dev);

/* Items [first, first + n) of a batch of `total` presentations.  Every array of `batch` and `status` is the whole batch's
 * ([k][total][32], status[total]); the call reads and writes only the elements of its range, so several contexts (one per
 * GPU) can work on one batch from several host threads.  The range is staged to HBM in slices that alternate between
 * two streams: the copy of one slice overlaps the kernels of the previous one. */
int afx_verify_presentations_range(afx_ctx* ctx, const afx_shape* shape, const afx_presentation_soa* batch, size_t total,
                                   size_t first, size_t n, uint8_t* status);

/* ---- several GPUs behind one call -------------------------------------------------------------------
 * Issuer::verify and Issuer::issue are single `&self` methods in one process (src/issuer.rs:141-147, :111-124).  A group is
 * that issuer on a node of GPUs: one context per listed device (the same device may be listed twice), each with its own
 * copy of parameters, key and tables.  A group call splits [0, count) into contiguous ranges (afx_shard_bounds), one host
 * thread per member runs afx_*_range on its range, and every member writes its part of the caller's arrays.  No data moves
 * between devices; there is no collective.  Host pointers only.  Settings (strict mode, pass size ...) are per member:
 * afx_group_member().  A call of at most afx_ctx_set_small_batch_items items (member 0's setting) is not cut up - its duration
 * is one chain's either way - but handed whole to ONE member, the next in turn: small calls from several host threads then
 * spread over the devices. */
typedef struct afx_group afx_group;
int afx_group_create(afx_group** out, const int* devices, uint32_t n_devices, const uint8_t* sysparams, size_t sysparams_len,
                     const uint8_t* amacs_key, size_t amacs_key_len, const uint8_t issuer_params[64]);
void afx_group_destroy(afx_group* group);
uint32_t afx_group_size(const afx_group* group);
afx_ctx* afx_group_member(afx_group* group, uint32_t index);
/* member `index` of `members` takes items [*first, *first + *n): contiguous, the first count % members ranges one item longer */
void afx_shard_bounds(size_t count, uint32_t members, uint32_t index, size_t* first, size_t* n);
int afx_group_verify_presentations(afx_group* group, const afx_shape* shape, const afx_presentation_soa* batch, size_t count,
                                   uint8_t* status);

/* ---- wire format (the reference defines none: presentation.rs:117-127 holds decoded
 *      points and has no to_bytes) ------------------------------------------------------------------
 * A batch of same-shape presentations, in the crate's "u32le n || 32-byte items" style (parameters.rs:155-184):
 *   header : "AFXP" | u32le version (1) | u32le count | u32le cells_per_record
 *            | u32le n_attributes | u32le n_responses | u32le n_hidden_scalars | u32le n_enc_proofs
 *            | kinds[n_attributes] (u8) | hidden_scalar_indices[..] (u16le) | enc_indices[..] (u16le) | zero pad to 32 B
 *   records: count x cells_per_record x 32 bytes, array of structs, each record =
 *            challenge | responses[n_responses] | C_x_0 | C_x_1 | C_V | C_y[n_attributes]
 *            | value of every PUBLIC_SCALAR / PUBLIC_POINT attribute, in position order
 *            | per proof of encryption: challenge | responses[6] | pk | E1 | E2 | C_y_1 | C_y_2 | C_y_3 | C_y_2'
 * A single ProofOfValidCredential::to_bytes is the same with count = 1. */
size_t afx_wire_header_bytes(const afx_shape* shape);
uint32_t afx_wire_cells_per_record(const afx_shape* shape);
/* Parse the header (host).  Returns AFX_OK and fills shape/count/records offset, or AFX_E_BAD_ARGS. */
int afx_wire_parse(const uint8_t* blob, size_t len, afx_shape* shape_out, size_t* count_out, size_t* records_offset_out);
/* Write such a batch from the struct-of-arrays (HOST pointers) that afx_show returned: what a user sends to the issuer.  blob == NULL
 * only reports the length needed in *len_out.  Bytes only. */
int afx_wire_pack_presentations(const afx_shape* shape, const afx_presentation_soa* batch, size_t count, uint8_t* blob, size_t blob_cap,
                                size_t* len_out);
/* Issuer::verify over a serialized batch: the records are copied to HBM, transposed to struct-of-arrays by a
 * kernel, and verified.  status must hold `count` bytes (status_cap >= count). */
int afx_verify_presentations_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, uint8_t* status, size_t status_cap, size_t* count_out);
/* Records [first, first + n) of the blob's batch (status is the whole batch's array: element first + i answers record first + i), and the
 * whole blob over a group's devices: the records are contiguous, so every member takes a byte range of the caller's blob. */
int afx_verify_presentations_wire_range(afx_ctx* ctx, const uint8_t* blob, size_t len, size_t first, size_t n, uint8_t* status, size_t status_cap,
                                        size_t* count_out);
int afx_group_verify_presentations_wire(afx_group* group, const uint8_t* blob, size_t len, uint8_t* status, size_t status_cap, size_t* count_out);

/* ---- presentations of DIFFERENT shapes in one call ------------------------------------------------------------------
 * Issuer::verify takes any presentation (src/issuer.rs:141-147): the shape - which attributes are hidden, how many proofs of
 * encryption ride along - is per presentation (src/nizk/presentation.rs:118-127, :293-309), and a server's request stream
 * mixes them.  The two entry points below group such a stream by shape inside the library, run one GPU batch per distinct
 * shape and put every status byte where its presentation stood in the caller's order.  Two shapes are the same group when
 * their used fields are equal (counts, kinds[0..n), hidden_scalar_indices[0..hs), enc_indices[0..ne)); array tails are ignored. */

/* Length in bytes (header + records) of the AFXP v1 section that starts at `blob`, from its header alone; AFX_E_BAD_ARGS if the
 * header is malformed or the section would run past `len`. */
int afx_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out);
/* `blob` = AFXP v1 sections back to back, in arrival order; each section is a complete same-shape batch (count >= 1; one
 * serialized presentation is a section with count = 1).  Sections of equal shape are merged into one batch whatever their
 * position in the stream.  status[i] answers the i-th presentation of the stream; *count_out = their number.
 * A section whose shape the reference would panic on fails its own items only.  Records are copied once on the host when
 * a group spans several sections (bytes only; no arithmetic leaves the GPU). */
int afx_verify_presentations_mixed_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, uint8_t* status, size_t status_cap, size_t* count_out);
/* ... every shape group split over a group's devices */
int afx_group_verify_presentations_mixed_wire(afx_group* group, const uint8_t* blob, size_t len, uint8_t* status, size_t status_cap, size_t* count_out);

/* The same over struct-of-arrays groups (host pointers).  `positions`, when not NULL, holds for each of the group's items its
 * index in the caller's order: status[positions[i]] answers item i of the group (every index < status_len, each used once
 * over all groups - checked before anything runs).  With positions == NULL the group's statuses are written contiguously,
 * after those of the groups before it.  Groups may repeat a shape. */
typedef struct {
  afx_shape shape;
  afx_presentation_soa batch;  /* the group's own arrays: [k][count][32]                        */
  size_t count;
  const uint64_t* positions;   /* [count] or NULL                                               */
} afx_presentation_group;
int afx_verify_presentations_mixed(afx_ctx* ctx, const afx_presentation_group* groups, size_t n_groups, uint8_t* status, size_t status_len);
/* ... and over a group of GPUs: every shape group is split over the members like afx_group_verify_presentations. */
int afx_group_verify_presentations_mixed(afx_group* group, const afx_presentation_group* groups, size_t n_groups, uint8_t* status,
                                         size_t status_len);

/* A batch of CredentialIssuance messages of one attribute layout (issuer.rs:42-45: proof + credential{amac, attributes};
 * the reference has no to_bytes for it either), same style:
 *   header : "AFXI" | u32le version (1) | u32le count | u32le cells_per_record | u32le n_attributes | u32le n_responses
 *            | kinds[n_attributes] (u8, AFX_ATTR_*) | zero pad to 32 B
 *   records: count x cells_per_record x 32 bytes, each record =
 *            t | U | V | challenge | responses[n_responses] | value of every attribute (Sc, or Pt = M1), position order
 * cells_per_record = 4 + n_responses + n_attributes. */
size_t afx_issuance_wire_header_bytes(uint32_t n_attributes);
int afx_issuance_wire_parse(const uint8_t* blob, size_t len, uint32_t* n_attributes_out, uint8_t kinds_out[AFX_MAX_ATTRIBUTES],
                            uint32_t* n_responses_out, size_t* count_out, size_t* records_offset_out);
/* CredentialIssuance::verify (issuer.rs:48-57) over a serialized batch; the context needs no issuer key. */
int afx_verify_issuances_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, uint8_t* status, size_t status_cap, size_t* count_out);
/* Length (header + records) of the AFXI v1 section that starts at `blob`; AFX_E_BAD_ARGS if its header is malformed or it runs past `len`. */
int afx_issuance_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out);
/* CredentialIssuance::verify over a stream of AFXI v1 sections back to back, exactly as afx_issue_wire writes them (a user context: no
 * issuer key).  status[i] answers the i-th issuance of the stream; *count_out = their number.
 *  - The status bytes are what afx_verify_issuances_wire gives when it is called on each section in turn, concatenated: sections whose
 *    n_attributes is not the context's and the all-zero records afx_issue_wire writes for failed items included.
 *  - AFX_E_BAD_ARGS, with nothing written to status, for a malformed section anywhere in the stream or status_cap below the item count.
 *    An empty stream is AFX_OK with a count of 0.
 *  - Sections of one (n_attributes, n_responses, kinds) are merged into one batch wherever they stand; its records go to the GPU from
 *    where they lie in `blob`, section by section (no host copy), and are transposed there (k_aos_to_soa).  Small batches
 *    of several layouts run as one set of launches (as afx_verify_issuances_mixed), calls of at most 512 items are collected with other
 *    threads' calls (afx_ctx_set_coalescing), large batches go through the two lanes in slices. */
int afx_verify_issuances_mixed_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, uint8_t* status, size_t status_cap, size_t* count_out);
/* ... over a group's devices: every merged batch is split over the members (afx_shard_bounds); a stream of at most
 * afx_ctx_set_small_batch_items issuances goes whole to one member, in turn.  Statuses equal afx_verify_issuances_mixed_wire's. */
int afx_group_verify_issuances_mixed_wire(afx_group* group, const uint8_t* blob, size_t len, uint8_t* status, size_t status_cap,
                                          size_t* count_out);

/* IssuerParameters in the byte form the crate intends (C_W || I, 64 bytes; issuer.rs:155,163 - its own
 * to_bytes/from_bytes are unimplemented!(), parameters.rs:365-372): what afx_ctx_create was given, or what an
 * issuer context derived from its key. */
int afx_ctx_issuer_parameters(afx_ctx* ctx, uint8_t out[64]);

/* ProofOfEncryption::verify alone (src/nizk/encryption.rs:154-210); `index` = ProofOfEncryption.index */
int afx_verify_encryption_proofs(afx_ctx* ctx, uint16_t index, const afx_encproof_soa* batch, size_t count,
                                 uint8_t* status);
int afx_verify_encryption_proofs_dev(afx_ctx* ctx, uint16_t index, const afx_encproof_soa* batch, size_t count,
                                     uint8_t* status_dev);

/* ---- Issuer::issue (src/issuer.rs:111-124 = Amac::tag src/amacs.rs:276-294 +
 *      ProofOfIssuance::prove src/nizk/issuance.rs:40-129) ----------------------------------- */

/* Attributes of a batch of credential requests of one layout (user.rs:137-139). */
typedef struct {
  uint32_t n_attributes;              /* request.attributes.len(); != ctx n => every status MAC_CREATION */
  uint8_t kinds[AFX_MAX_ATTRIBUTES];  /* AFX_ATTR_* per position                                         */
  const uint8_t* values;              /* [n_attributes][count] 32 B: Sc for scalar kinds; Pt (M1) for point kinds */
} afx_attributes_soa;

typedef struct {
  const uint8_t* t_wide;    /* [count][64]  the 64 bytes Scalar::random draws        (amacs.rs:289)  */
  const uint8_t* U_wide;    /* [count][64]  the 64 bytes RistrettoPoint::random draws (amacs.rs:290) */
  const uint8_t* rng_seed;  /* [count][32]  the 32 bytes zkp's prove_compact draws from thread_rng() */
} afx_issue_randomness;

typedef struct {
  uint8_t* t;          /* [count] Sc    amac.t */
  uint8_t* U;          /* [count] Pt    amac.U */
  uint8_t* V;          /* [count] Pt    amac.V */
  uint8_t* challenge;  /* [count] Sc    ProofOfIssuance.0.challenge */
  uint8_t* responses;  /* [n+5][count] Sc  ProofOfIssuance.0.responses (w,w',x_0,x_1,y_0..y_{n-1},1) */
} afx_issuance_soa;

int afx_issue(afx_ctx* ctx, const afx_attributes_soa* requests, const afx_issue_randomness* rnd, size_t count,
              const afx_issuance_soa* out, uint8_t* status);
int afx_issue_dev(afx_ctx* ctx, const afx_attributes_soa* requests, const afx_issue_randomness* rnd, size_t count,
                  const afx_issuance_soa* out, uint8_t* status_dev);

/* Requests [first, first + n) of a batch of `total`; arrays are the whole batch's, as for afx_verify_presentations_range. */
int afx_issue_range(afx_ctx* ctx, const afx_attributes_soa* requests, const afx_issue_randomness* rnd, size_t total, size_t first,
                    size_t n, const afx_issuance_soa* out, uint8_t* status);
int afx_group_issue(afx_group* group, const afx_attributes_soa* requests, const afx_issue_randomness* rnd, size_t count,
                    const afx_issuance_soa* out, uint8_t* status);

/* CredentialIssuance::verify (src/issuer.rs:48-57 -> src/nizk/issuance.rs:132-218), user side. */
int afx_verify_issuances(afx_ctx* ctx, const afx_attributes_soa* attrs, const afx_issuance_soa* issuances,
                         uint32_t n_responses, size_t count, uint8_t* status);
int afx_verify_issuances_dev(afx_ctx* ctx, const afx_attributes_soa* attrs, const afx_issuance_soa* issuances,
                             uint32_t n_responses, size_t count, uint8_t* status_dev);
/* Issuances [first, first + n) of a batch of `total`, and the whole batch over a group's devices. */
int afx_verify_issuances_range(afx_ctx* ctx, const afx_attributes_soa* attrs, const afx_issuance_soa* issuances,
                               uint32_t n_responses, size_t total, size_t first, size_t n, uint8_t* status);
int afx_group_verify_issuances(afx_group* group, const afx_attributes_soa* attrs, const afx_issuance_soa* issuances,
                               uint32_t n_responses, size_t count, uint8_t* status);
/* Write an AFXI batch (the wire format above) from what afx_issue returned (HOST pointers): what the issuer sends back to its users.  blob == NULL only
 * reports the length needed. */
int afx_issuance_wire_pack(const afx_attributes_soa* attrs, const afx_issuance_soa* issuances, uint32_t n_responses, size_t count, uint8_t* blob,
                           size_t blob_cap, size_t* len_out);

/* A batch of CredentialRequests of one attribute layout (user.rs:137-139: the attributes; the crate serialises none), same style:
 *   header : "AFXR" | u32le version (1) | u32le count | u32le cells_per_record | u32le n_attributes
 *            | kinds[n_attributes] (u8, AFX_ATTR_*) | zero pad to 32 B
 *   records: count x n_attributes x 32 bytes, each record = the value of every attribute in position order (Sc for scalar kinds,
 *            Pt = M1 for point kinds: what afx_attributes_soa.values holds)
 * cells_per_record = n_attributes.  One CredentialRequest is a section with count = 1; a request stream is sections back to back.
 * n_attributes = 0 is well formed (every item of such a section is MAC_CREATION against any context).  A kind above
 * AFX_ATTR_SECRET_POINT, n_attributes > AFX_MAX_ATTRIBUTES, a wrong cells_per_record or a wrong length: AFX_E_BAD_ARGS. */
size_t afx_request_wire_header_bytes(uint32_t n_attributes);   /* 0 if n_attributes > AFX_MAX_ATTRIBUTES */
int afx_request_wire_parse(const uint8_t* blob, size_t len, uint32_t* n_attributes_out, uint8_t kinds_out[AFX_MAX_ATTRIBUTES],
                           size_t* count_out, size_t* records_offset_out);
/* Length (header + records) of the AFXR v1 section that starts at `blob`; AFX_E_BAD_ARGS if its header is malformed or it runs past `len`. */
int afx_request_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out);
/* Write such a batch from column arrays (HOST pointers; values [n][count][32]): what a user sends.  blob == NULL only reports the
 * length needed.  Bytes only. */
int afx_request_wire_pack(const afx_attributes_soa* requests, size_t count, uint8_t* blob, size_t blob_cap, size_t* len_out);
/* Issuer::issue over a stream of AFXR sections: request bytes in, AFXI bytes out, both transpositions on the GPU.
 *  - rnd: host arrays in stream order (item i of the stream uses t_wide[i], U_wide[i], rng_seed[i]), as for afx_issue.
 *  - out: one AFXI v1 section per request section, in the same order, with the same count and kinds and n_responses = ctx n + 5:
 *    response section k answers request section k.  status[i] answers the i-th request of the stream; *count_out = their number.
 *  - An item whose status is not AFX_ST_OK has a record of zeros (attribute values included).  A section whose n_attributes is not
 *    the context's is all MAC_CREATION (amacs.rs:285-287); undecodable points and non-canonical scalars give what afx_issue gives.
 *    Every other record is byte for byte what afx_issue + afx_issuance_wire_pack make of the same inputs.
 *  - out == NULL: only *out_len (and *count_out) from the headers and the context's n; no device work, rnd may be NULL.
 *  - AFX_E_BAD_ARGS, with nothing written to out or status, for out_cap < *out_len, status_cap < the item count or a malformed
 *    section anywhere in the stream; AFX_E_NO_KEY for a context without the issuer key.
 *  - Sections of one layout are merged into one batch wherever they stand.  Small batches of several layouts run as one set of
 *    launches (as afx_issue_mixed), calls of at most 512 items are collected with other threads' calls (afx_ctx_set_coalescing), large
 *    batches go through the two lanes in slices (as afx_issue). */
int afx_issue_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_issue_randomness* rnd, uint8_t* out, size_t out_cap,
                   size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out);
/* ... over a group's devices: every merged batch is split over the members (afx_shard_bounds), each writing its own record range of
 * `out`; a stream of at most afx_ctx_set_small_batch_items requests goes whole to one member, in turn.  Bytes equal afx_issue_wire's. */
int afx_group_issue_wire(afx_group* group, const uint8_t* blob, size_t len, const afx_issue_randomness* rnd, uint8_t* out,
                         size_t out_cap, size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out);

/* ---- AnonymousCredential::show (src/credential.rs:37-46 -> src/nizk/presentation.rs:139-321) - */

/* A batch of credentials of one layout, as the user holds them. */
typedef struct {
  uint32_t n_attributes;
  uint8_t kinds[AFX_MAX_ATTRIBUTES];  /* AFX_ATTR_* per position (after hide_attribute/reveal_attribute) */
  const uint8_t* values;              /* [n][count] 32 B: Sc (scalar kinds) or Pt M1 (point kinds)        */
  const uint8_t* M2;                  /* [n][count] Pt: Plaintext.M2 rows for SECRET_POINT positions     */
  const uint8_t* m3;                  /* [n][count] Sc: Plaintext.m3 rows for SECRET_POINT positions     */
  const uint8_t* t;                   /* [count] Sc */
  const uint8_t* U;                   /* [count] Pt */
  const uint8_t* V;                   /* [count] Pt */
} afx_credentials_soa;

/* symmetric::Keypair (src/symmetric.rs:52-56,68-81); one keypair per item */
typedef struct {
  const uint8_t* a;   /* [count] Sc */
  const uint8_t* a0;  /* [count] Sc */
  const uint8_t* a1;  /* [count] Sc */
  const uint8_t* pk;  /* [count] Pt */
} afx_keypairs_soa;

typedef struct {
  const uint8_t* z_wide;     /* [count][64]   Scalar::random for the nonce z (presentation.rs:162)       */
  const uint8_t* rng_seed;   /* [count][32]   thread_rng() draw of the presentation's prove_compact      */
  const uint8_t* enc_seeds;  /* [n_secret_points][count][32]  same for each ProofOfEncryption, in order   */
} afx_show_randomness;

/* Output arrays mirror afx_presentation_soa / afx_encproof_soa but writable. */
typedef struct {
  uint8_t* challenge; uint8_t* responses;
  uint8_t* pk; uint8_t* E1; uint8_t* E2; uint8_t* C_y_1; uint8_t* C_y_2; uint8_t* C_y_3; uint8_t* C_y_2p;
} afx_encproof_out;
typedef struct {
  uint8_t* challenge; uint8_t* responses;      /* [3+hs][count] */
  uint8_t* C_x_0; uint8_t* C_x_1; uint8_t* C_V;
  uint8_t* C_y;                                /* [n][count] */
  uint8_t* attr_values;                        /* [n][count]: revealed values copied through */
  const afx_encproof_out* enc;                 /* [n_secret_points] */
} afx_presentation_out;

/* keypairs == NULL with a SECRET_POINT attribute => every status AFX_ST_NO_SYMMETRIC_KEY.
 * `shape_out` receives the presentation shape (kinds, hidden indices, enc indices). */
int afx_show(afx_ctx* ctx, const afx_credentials_soa* creds, const afx_keypairs_soa* keypairs,
             const afx_show_randomness* rnd, size_t count, const afx_presentation_out* out, afx_shape* shape_out,
             uint8_t* status);
int afx_show_dev(afx_ctx* ctx, const afx_credentials_soa* creds, const afx_keypairs_soa* keypairs,
                 const afx_show_randomness* rnd, size_t count, const afx_presentation_out* out, afx_shape* shape_out,
                 uint8_t* status_dev);
/* Credentials [first, first + n) of a batch of `total` (every output array indexed like the inputs; shape_out is the same
 * for every range of one batch), and the whole batch over a group's devices (a user-side group is created with
 * amacs_key == NULL). */
int afx_show_range(afx_ctx* ctx, const afx_credentials_soa* creds, const afx_keypairs_soa* keypairs,
                   const afx_show_randomness* rnd, size_t total, size_t first, size_t n, const afx_presentation_out* out,
                   afx_shape* shape_out, uint8_t* status);
int afx_group_show(afx_group* group, const afx_credentials_soa* creds, const afx_keypairs_soa* keypairs,
                   const afx_show_randomness* rnd, size_t count, const afx_presentation_out* out, afx_shape* shape_out,
                   uint8_t* status);

/* ---- requests, credentials and issuances of DIFFERENT layouts in one call -------------------------------------------
 * Issuer::issue takes any request (src/issuer.rs:111-124: the attribute kinds are per attribute, src/amacs.rs:168-179),
 * AnonymousCredential::show any credential in whatever state its hide_attribute / reveal_attribute calls left it
 * (src/credential.rs:37-46, :53-97) and CredentialIssuance::verify any issuance (src/issuer.rs:48-57).  As for
 * afx_verify_presentations_mixed above, the caller hands over one struct-of-arrays group per distinct layout; each group has its
 * own input AND output arrays ([k][count][32], item i of the group in element i), and only the status bytes go back to the
 * caller's order: status[positions[i]] answers item i of the group (positions == NULL: contiguous, after the groups before it;
 * every index < status_len and used once over all groups - checked before anything runs).  Groups may repeat a layout.  Small
 * groups are assembled into ONE set of kernel launches (mixed.cpp), so a stream of many layouts costs about one small call. */
typedef struct {
  afx_attributes_soa requests;   /* n_attributes != ctx n => the group's statuses are all MAC_CREATION (amacs.rs:285-287)      */
  afx_issue_randomness rnd;
  afx_issuance_soa out;          /* the group's own output arrays; responses [ctx n + 5][count][32]                           */
  size_t count;
  const uint64_t* positions;     /* [count] or NULL                                                                           */
} afx_issue_group;
int afx_issue_mixed(afx_ctx* ctx, const afx_issue_group* groups, size_t n_groups, uint8_t* status, size_t status_len);
int afx_group_issue_mixed(afx_group* group, const afx_issue_group* groups, size_t n_groups, uint8_t* status, size_t status_len);

typedef struct {
  afx_attributes_soa attrs;
  afx_issuance_soa issuances;    /* read only here                                                                            */
  uint32_t n_responses;          /* proof.responses.len() of the group's issuances                                            */
  size_t count;
  const uint64_t* positions;
} afx_issuance_group;
int afx_verify_issuances_mixed(afx_ctx* ctx, const afx_issuance_group* groups, size_t n_groups, uint8_t* status, size_t status_len);
int afx_group_verify_issuances_mixed(afx_group* group, const afx_issuance_group* groups, size_t n_groups, uint8_t* status, size_t status_len);

typedef struct {
  afx_credentials_soa creds;
  const afx_keypairs_soa* keypairs;  /* or NULL (see afx_show)                                                                */
  afx_show_randomness rnd;
  afx_presentation_out out;          /* the group's own output arrays                                                         */
  afx_shape shape_out;               /* written: the presentation shape of this group                                         */
  size_t count;
  const uint64_t* positions;
} afx_show_group;
int afx_show_mixed(afx_ctx* ctx, afx_show_group* groups, size_t n_groups, uint8_t* status, size_t status_len);
int afx_group_show_mixed(afx_group* group, afx_show_group* groups, size_t n_groups, uint8_t* status, size_t status_len);
/* AnonymousCredential::show straight into AFXP bytes: what a user sends, ready for afx_verify_presentations_mixed_wire.
 *  - groups: as for afx_show_mixed (creds, keypairs, rnd, count and positions mean what they mean there; shape_out is written), except
 *    that each group's `out` member is NOT read: a caller may leave it zeroed.
 *  - out: one AFXP v1 section per group, in group order, with the group's count and the shape afx_show gives its kinds; records in
 *    the group's item order.  Statuses go through positions exactly as in afx_show_mixed.
 *  - An item whose status is not AFX_ST_OK has a record of zeros; every other record is byte for byte what afx_show_mixed +
 *    afx_wire_pack_presentations make of the same inputs.  A group with a SECRET_POINT attribute and keypairs == NULL gives a section of
 *    zero records, every status AFX_ST_NO_SYMMETRIC_KEY.
 *  - out == NULL: only *out_len and every shape_out, from the kinds on the host; no device work, rnd may be NULL.
 *  - AFX_E_BAD_ARGS, with nothing written to out or status, for out_cap < *out_len, a bad status_len or positions (as afx_show_mixed
 *    checks them) or any group afx_show would refuse (n_attributes 0 or above the context's n, a kind out of range, missing arrays).
 *    The layout is checked for groups of count 0 too: their section still has a shape.
 *  - afx_show_dev writes into the rows of one scratch region per pass, the revealed attribute values are read from the credential's
 *    value rows, and k_soa_to_aos turns the region into AFXP records on the GPU (failed items zeroed), fetched in one piece.  Small
 *    groups share one set of launches, calls of at most 512 items are collected with other threads' calls, large groups go through
 *    the two lanes in slices. */
int afx_show_wire(afx_ctx* ctx, afx_show_group* groups, size_t n_groups, uint8_t* out, size_t out_cap, size_t* out_len,
                  uint8_t* status, size_t status_len);
/* ... over a group's devices: every group is split over the members (afx_shard_bounds), each writing its own record range of `out`;
 * a request of at most afx_ctx_set_small_batch_items credentials goes whole to one member, in turn.  Bytes equal afx_show_wire's. */
int afx_group_show_wire(afx_group* group, afx_show_group* groups, size_t n_groups, uint8_t* out, size_t out_cap, size_t* out_len,
                        uint8_t* status, size_t status_len);

/* ---- Randomness drawn on the device ----------------------------------------------------------
 * The wire doors above take the random draws of every item from the host (afx_issue_randomness: 160 B per request,
 * afx_show_randomness: 96 B + 32 B per hidden point per credential).  The *_rng forms draw them on the GPU instead, as a documented
 * deterministic function of a 32-byte seed and a 64-bit stream number (normative):
 *
 *   draw(seed, stream, index, label) = SHAKE256("aeonflux-amd/device-rng/v1"     26 ASCII bytes, no terminator
 *                                               || seed                          32 bytes
 *                                               || u64le(stream) || u64le(index) 8 + 8 bytes
 *                                               || u8(label))                    75 bytes: one block at SHAKE256's rate of 136
 *                                      truncated to the label's length (AFX_DRAW_BYTES).
 *
 *  - An issuance draws labels AFX_DRAW_T_WIDE, AFX_DRAW_U_WIDE and AFX_DRAW_ISSUE_SEED: its t_wide, U_wide and rng_seed.  Its index
 *    is the item's ordinal in the request stream (= its status index).
 *  - A show draws AFX_DRAW_Z_WIDE (z_wide), AFX_DRAW_SHOW_SEED (rng_seed) and AFX_DRAW_ENC_SEED(j) (enc_seeds[j], the j-th SECRET_POINT
 *    in position order).  Its index is the item's ordinal over the groups in group order: the counts of the earlier groups plus i,
 *    whatever `positions` says.
 * The calls are specified as equivalences, which is also how they are tested: afx_issue_wire_rng(ctx, blob, {S, k}, ...) returns the
 * bytes, statuses, lengths and error codes afx_issue_wire(ctx, blob, rnd, ...) returns when rnd holds draw(S, k, i, .) for item i;
 * afx_show_wire_rng likewise against afx_show_wire with every group's rnd filled at its ordinal indices.  The group forms give the
 * one-context bytes however the items are split: a draw depends on the global index only.
 *  - rng == NULL: AFX_E_BAD_ARGS.  out == NULL: the size query, nothing drawn.
 *  - The seed is a secret: whoever holds it can recompute every nonce.  The library zeroes its copies (the pinned staging image and
 *    the device staging area) when the call completes, failures included.  Never reuse a (seed, stream) pair: a caller that keeps one
 *    seed gives every call its own stream.
 * The Rust crate's own calls keep passing the crate's csprng draws (integration/: crate semantics); these forms are for C and Python
 * servers on the wire doors. */
#define AFX_DRAW_T_WIDE 0u
#define AFX_DRAW_U_WIDE 1u
#define AFX_DRAW_ISSUE_SEED 2u
#define AFX_DRAW_Z_WIDE 3u
#define AFX_DRAW_SHOW_SEED 4u
#define AFX_DRAW_ENC_SEED(j) (5u + (uint32_t)(j))   /* j < AFX_MAX_ATTRIBUTES */
/* the blind issuer's draws (afx_issue_blind_wire_rng, "Blind issuance on bytes" below): above AFX_DRAW_BATCH_WEIGHTS (64), because
 * afx_rng_expand keeps serving the labels up to AFX_DRAW_ENC_SEED(31) only */
#define AFX_DRAW_BLIND_T_WIDE 65u        /* 64 bytes */
#define AFX_DRAW_BLIND_U_WIDE 66u        /* 64 bytes */
#define AFX_DRAW_BLIND_RPRIME_WIDE 67u   /* 64 bytes */
#define AFX_DRAW_BLIND_ISSUE_SEED 68u    /* 32 bytes */
/* the blind user's draws (afx_blind_request_wire_rng, afx_unblind_issuances_wire_rng: "Blind issuance on bytes: the user's doors" below) */
#define AFX_DRAW_BLINDREQ_D_WIDE 69u     /* 64 bytes: d = from_bytes_mod_order_wide of them */
#define AFX_DRAW_BLINDREQ_SEED 70u       /* 32 bytes */
#define AFX_DRAW_BLINDREQ_R_WIDE(j) (71u + (uint32_t)(j))   /* 64 bytes; j < AFX_MAX_ATTRIBUTES: the j-th hidden position */
#define AFX_DRAW_BYTES(label) (((label) == AFX_DRAW_T_WIDE || (label) == AFX_DRAW_U_WIDE || (label) == AFX_DRAW_Z_WIDE || \
                                ((label) >= AFX_DRAW_BLIND_T_WIDE && (label) <= AFX_DRAW_BLIND_RPRIME_WIDE) || (label) == AFX_DRAW_BLINDREQ_D_WIDE || \
                                ((label) >= AFX_DRAW_BLINDREQ_R_WIDE(0) && (label) <= AFX_DRAW_BLINDREQ_R_WIDE(31))) ? 64u : 32u)
/* (declared apart from its typedef: unlike the batch structs above, the Rust shim does not bind it - it keeps the crate's explicit draws,
 * INTEGRATION.md - and tests/test_integration_layouts.py checks the typedef'd structs against the shim's) */
struct afx_device_rng {
  const uint8_t* seed;  /* 32 bytes, or NULL: the library reads 32 bytes from getrandom(2) for this call (one seed per group call) */
  uint64_t stream;      /* a caller that keeps one seed gives every call its own stream; never reuse (seed, stream) */
};
typedef struct afx_device_rng afx_device_rng;
/* out[i] = draw(seed, stream, first + i, label) for i < count: [count][AFX_DRAW_BYTES(label)] bytes (label <= AFX_DRAW_ENC_SEED(31)).
 * `first` is the 64-bit index of the first draw (size_t: 64 bits on the LP64 hosts the library builds for). */
int afx_rng_expand(afx_ctx* ctx, const afx_device_rng* rng, uint32_t label, size_t first, size_t count, uint8_t* out);
int afx_issue_wire_rng(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_device_rng* rng, uint8_t* out, size_t out_cap,
                       size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out);
int afx_group_issue_wire_rng(afx_group* group, const uint8_t* blob, size_t len, const afx_device_rng* rng, uint8_t* out,
                             size_t out_cap, size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out);
/* groups[g].rnd is not read */
int afx_show_wire_rng(afx_ctx* ctx, afx_show_group* groups, size_t n_groups, const afx_device_rng* rng, uint8_t* out, size_t out_cap,
                      size_t* out_len, uint8_t* status, size_t status_len);
int afx_group_show_wire_rng(afx_group* group, afx_show_group* groups, size_t n_groups, const afx_device_rng* rng, uint8_t* out,
                            size_t out_cap, size_t* out_len, uint8_t* status, size_t status_len);

/* ---- Batchable presentation proofs -------------------------------------------------------------
 * zkp's toolbox has two encodings of one proof: CompactProof { challenge, responses } (Prover::prove_compact, what the crate sends
 * today) and BatchableProof { commitments, responses } (Prover::prove_batchable / Verifier::verify_batchable): the prover sends the
 * commitments it hashed instead of the challenge it got.  Transcript, statement, labels and responses are the same.  Off unless
 * called: nothing above changes.
 *
 * Semantics (normative).  A batchable presentation is a compact one with every `challenge` - of the main proof and of each proof of
 * encryption - replaced by that proof's commitments R_0 .. R_(m-1), 32-byte ristretto255 encodings in constraint order.  m is the
 * number of constraints the verifier builds for the shape: afx_batchable_main_commitments() for the main proof (2 + one per kept
 * commitment whose constraint-#3 position is not a hidden group element, + in strict mode one per hidden group element at a position
 * other than 0), 5 for a proof of encryption.  An item's status is AFX_ST_OK iff
 *  1. everything afx_verify_presentations checks before a transcript holds unchanged (canonical scalars, decodable points, the shapes
 *     the reference would panic on, an identity generator, strict-mode pairing);
 *  2. every commitment decodes and none is the identity encoding (32 zero bytes): zkp's validate_and_append_blinding_commitment;
 *  3. with c = the transcript's challenge after the received commitments were appended as its "blindcom" values, every constraint
 *     holds as an equation of group elements:  R_j = sum_s resp_s * P_(j,s) - c * LHS_j.
 * Hence (R, resp) is accepted iff the compact proof (c(R), resp) is accepted by afx_verify_presentations AND its recomputed
 * commitments encode to exactly R.
 *
 * The engine checks 3 with ONE sum per item, over the main proof and all the proofs of encryption together:
 *     sum_j rho_j * ( sum_s resp_s * P_(j,s) - c * LHS_j - R_j ) == identity.
 *  - The weights rho_j are 128 bits each, one per (item, proof, constraint), unpredictable to whoever made the proofs.  A false accept
 *    has probability at most 2^-128 per item.
 *  - "identity" is the ristretto255 identity - any of the four Edwards points of its coset (X == 0 or Y == 0), not only (0, 1) - with
 *    no cofactor multiplication: the sum is encoded and the encoding compared with 32 zero bytes.
 *  - Weights (normative bytes): item `index` = its ordinal in the call draws
 *        draw(seed, stream, index, AFX_DRAW_BATCH_WEIGHTS)   squeezed to 16 * M bytes (SHAKE256 over as many blocks as that takes),
 *    M = n_main + 5 * n_enc_proofs; weight w (main proof's constraints first, then proof of encryption 0's five, ...) is bytes
 *    [16 w, 16 w + 16) as a little-endian integer.  The label is not reachable through afx_rng_expand.
 *  - `weights` NULL, or a NULL seed: the library reads a seed from getrandom(2) per call (what a server uses); a given seed makes a run
 *    reproducible (tests).  A verifier whose seed the prover can predict has no soundness beyond the prover's honesty.  The library
 *    zeroes its copies of the seed (a pinned image and the device's) as soon as the weights are drawn; for that the *_dev form waits
 *    for the seed's copy, which is queued behind the lane's earlier work.
 *  - Z = C_V - W - x0*C_x0 - ... stays its own multiscalar job on the issuer key exactly as in afx_verify_presentations and enters the
 *    sum as a per-item base; every scalar of the sum itself is public, so the sum runs the fast tables in every secret mode:
 *    afx_ctx_set_fixed_key_schedule and afx_ctx_set_secret_independent_addressing(1) govern the Z job only.
 *  - A batchable call takes the context in turn (it is not collected with other threads' calls); the host-pointer forms stage a
 *    call (the wire doors: a group) in one piece.  Statuses are per item: a failed item fails alone.
 * afx_show_batchable writes everything afx_show writes (challenges included, byte for byte) plus the commitments: one call yields both
 * encodings. */
#define AFX_DRAW_BATCH_WEIGHTS 64u
/* (declared apart from their typedefs, like afx_device_rng: the Rust shim does not bind them) */
struct afx_commitments_soa {            /* the R_j of a batch; read by verify, written by show */
  uint8_t* main;                        /* [n_main][count] Pt                                   */
  uint8_t* const* enc;                  /* [n_enc_proofs] pointers, each [5][count] Pt           */
};
typedef struct afx_commitments_soa afx_commitments_soa;
/* n_main under the context's strict setting; 0: every item of the shape fails (no commitment array is read) */
uint32_t afx_batchable_main_commitments(const afx_ctx* ctx, const afx_shape* shape);
/* batch->challenge and batch->enc[e].challenge are not read and may be NULL */
int afx_verify_presentations_batchable(afx_ctx* ctx, const afx_shape* shape, const afx_presentation_soa* batch,
                                       const afx_commitments_soa* commitments, const afx_device_rng* weights, size_t count, uint8_t* status);
int afx_verify_presentations_batchable_dev(afx_ctx* ctx, const afx_shape* shape, const afx_presentation_soa* batch,
                                           const afx_commitments_soa* commitments, const afx_device_rng* weights, size_t count,
                                           uint8_t* status_dev);
/* commitments_out->main must hold afx_batchable_main_commitments(ctx, shape_out) rows: size it from the credential kinds (2 + the
 * attributes that are not hidden group elements in the reference's shapes; ask afx_batchable_main_commitments with the shape of an
 * empty afx_show call when in doubt) */
int afx_show_batchable(afx_ctx* ctx, const afx_credentials_soa* creds, const afx_keypairs_soa* keypairs, const afx_show_randomness* rnd,
                       size_t count, const afx_presentation_out* out, const afx_commitments_soa* commitments_out, afx_shape* shape_out,
                       uint8_t* status);
int afx_show_batchable_dev(afx_ctx* ctx, const afx_credentials_soa* creds, const afx_keypairs_soa* keypairs, const afx_show_randomness* rnd,
                           size_t count, const afx_presentation_out* out, const afx_commitments_soa* commitments_out, afx_shape* shape_out,
                           uint8_t* status_dev);

/* Batchable presentations on bytes: "AFXB" version 1 (a format of its own, not a version of AFXP, whose parsers stay as they are).
 *   header  = "AFXB" | u32le 1 | u32le count | u32le cells_per_record | u32le n_attributes | u32le n_responses | u32le n_hidden_scalars
 *             | u32le n_enc_proofs | u32le n_main_commitments | kinds[n_attributes] | u16le hidden_scalar_indices[] | u16le enc_indices[]
 *             | zero padding to a multiple of 32 bytes  (the AFXP header's fields plus n_main_commitments)
 *   record  = the AFXP record with `challenge` replaced by R[n_main_commitments] and each proof of encryption's `challenge` by R[5]:
 *             R[n_main] | responses | C_x_0 C_x_1 C_V | C_y[n] | the revealed attribute values | per proof: R[5] responses[6] pk E1 E2
 *             C_y_1 C_y_2 C_y_3 C_y_2p,  32-byte cells.
 * The host-only functions accept as n_main_commitments what the shape's main proof has under the reference's statement or under the
 * strict one and refuse anything else (AFX_E_BAD_ARGS, like a wrong magic, version, count, cell count, a truncated header or trailing
 * bytes); the verifier's door also refuses a section whose n_main_commitments is not afx_batchable_main_commitments(ctx, shape). */
size_t afx_batchable_wire_header_bytes(const afx_shape* shape);                                   /* 0: shape out of range */
uint32_t afx_batchable_wire_cells_per_record(const afx_shape* shape, uint32_t n_main_commitments); /* 0: shape or n_main out of range */
int afx_batchable_wire_parse(const uint8_t* blob, size_t len, afx_shape* shape_out, uint32_t* n_main_commitments_out, size_t* count_out,
                             size_t* records_offset_out);
int afx_batchable_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out);
/* host, bytes only; blob == NULL: the size query */
int afx_batchable_wire_pack(const afx_shape* shape, const afx_presentation_soa* batch, const afx_commitments_soa* commitments,
                            uint32_t n_main_commitments, size_t count, uint8_t* blob, size_t blob_cap, size_t* len_out);
/* AFXB sections back to back, merged by shape; status[i] answers the i-th presentation of the stream.  The error contract of
 * afx_verify_presentations_mixed_wire: a malformed section anywhere is AFX_E_BAD_ARGS and nothing is written; *count_out is set once
 * the stream has parsed.  Weights: each merged group is one column call - its items draw at their ordinals within the group, the
 * g-th group (in order of first appearance) under stream number weights->stream + g. */
int afx_verify_presentations_batchable_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_device_rng* weights, uint8_t* status,
                                            size_t status_cap, size_t* count_out);
/* one AFXB section per group, the error contract of afx_show_wire: out == NULL is the size query (shapes and *out_len only), failed
 * items are records of zeros, groups without the symmetric key they need get AFX_ST_NO_SYMMETRIC_KEY and zero records; a group whose
 * shape has no batchable form fails the call. */
int afx_show_batchable_wire(afx_ctx* ctx, afx_show_group* groups, size_t n_groups, uint8_t* out, size_t out_cap, size_t* out_len,
                            uint8_t* status, size_t status_len);

/* ---- Blind issuance: hidden attributes stay encrypted at the issuer ----------------------------
 * Issuer::issue reads every attribute in the clear (src/issuer.rs:96-98, "unblinded"); the crate's
 * CredentialRequestConstructor::append_hidden_scalar / append_hidden_point / append_ciphertext are stubs (src/user.rs:86-128).  These
 * four calls are the standard blind issuance of MAC_GGM (CMZ'14 section 4; the 2019/1416 paper the crate's labels cite): the user
 * ElGamal-encrypts the hidden attributes under a one-time key and proves the request well formed, the issuer evaluates the MAC on the
 * ciphertexts and proves it did so under its published parameters, the user verifies and decrypts V.  The credential (t, U, V) is byte
 * for byte the one afx_issue makes from the same t_wide, U_wide and attribute values, so afx_show and the verifiers need no change.
 * Off unless called: nothing above changes.
 *
 * Protocol (normative).  G = SystemParameters.G.  H = the positions whose kind is AFX_ATTR_SECRET_SCALAR or AFX_ATTR_SECRET_POINT, in
 * increasing order, h = |H|, hs = how many of them are scalars.  M_i as in Messages::from_attributes (m_i*G_m[i], or the point M1).
 * Every proof uses Transcript::new(b"2019/1416 anonymous credential") and zkp's compact proofs, exactly as the statements above.
 *
 * 1. Request (user; needs no issuer key).  Per item: the attribute values of all n positions, a one-time scalar d, r_j =
 *    from_bytes_mod_order_wide(r_wide[j]) per hidden position, rng_seed.  D = d*G, A_j = r_j*G, B_j = r_j*D + M_i for the j-th hidden
 *    position i, and a proof under the label "2019/1416 blind request proof":
 *      scalars  "d", then per hidden position "r" and, for a scalar kind, "m" directly after it
 *      points   "G", "D", then per hidden position "A", "B" and, for a scalar kind, "G_m" (= G_m[i])
 *      constraints  D = d*G;  per hidden position A = r*G and, for a scalar kind, B = r*D + m*G_m[i]
 *    A hidden point's B is allocated but not constrained (any pair encrypts some point; A = r*G makes it extractable, allocating B
 *    binds it into the challenge).  1 + h + hs responses.
 * 2. Blind issue (issuer).  The request is verified as a zkp Verifier verifies it: canonical scalars, points that decode, no allocated
 *    point whose encoding is 32 zero bytes, the recomputed challenge equal to the received one.  For an item that passes: t and U from
 *    t_wide / U_wide exactly as afx_issue draws them, r' = from_bytes_mod_order_wide(rprime_wide),
 *      V'  = W + x0*U + (x1*t)*U + sum_{i not in H} y_i*M_i
 *      S1  = r'*G + sum_{i in H} y_i*A_i
 *      S2  = r'*D + V' + sum_{i in H} y_i*B_i
 *    and a proof under the label "2019/1416 blind issuance proof":
 *      scalars  w, w', x_0, x_1, y (n times), "1", "r'"                                   (n + 6 responses)
 *      points   the issuance proof's own allocations in its order and with its labels, without its V: G_V, G_w, G_w_prime, -G_x_0,
 *               -G_x_1, every -G_y (all max(3, n)), C_W, I, U, tU; then "G", "D", "S1", "S2"; then per position 0 .. n-1 "A", "B"
 *               for a hidden position, "M" for a revealed one
 *      constraints  C_W = w*G_w + w'*G_w';  I = 1*G_V + x_0*(-G_x_0) + x_1*(-G_x_1) + sum_{i<n} y_i*(-G_y_i);
 *                   S1 = r'*G + sum_H y_i*A_i;  S2 = w*G_w + x_0*U + x_1*tU + r'*D + sum_i y_i*(B_i or M_i)
 * 3. Unblind (user).  The issuance proof is verified, tU recomputed from t and U; then V = S2 - d*S1.  The credential is (t, U, V) with
 *    the attributes the user already holds.
 *
 * Statuses.  One failure code per call: afx_blind_request AFX_ST_MAC_CREATION (a non-canonical d or scalar value, a point value that
 * does not decode - all n positions are checked - or a D, A or B that would be the identity encoding); afx_verify_blind_requests,
 * afx_issue_blind (anything wrong with the item's request or its revealed values) and afx_unblind_issuances (anything wrong with the
 * issuance, the proof, d or the user's own D, A, B) AFX_ST_VERIFICATION_FAILURE.  Whole shapes: n_attributes != the context's n or a
 * kind above AFX_ATTR_SECRET_POINT fails every item - AFX_ST_MAC_CREATION from afx_blind_request and afx_issue_blind (amacs.rs:285-287,
 * as afx_issue), AFX_ST_VERIFICATION_FAILURE from the other two; a wrong response count (n_responses != 1 + h + hs of a request,
 * != n + 6 of an issuance) fails every item with AFX_ST_VERIFICATION_FAILURE.
 * AN ITEM THAT FAILS GETS ZEROS IN EVERY OUTPUT ROW OF THE CALL, written on the device (k_mask_rows, in front of k_finish) before
 * the call completes: the issuer releases no S1, S2 or response for a request whose proof it did not accept.  (A whole-shape failure
 * of a host-pointer form is answered on the host: the statuses, and zeros in the outputs.)
 *
 * Secrets.  d, r_j, m_i and the request proof's blindings; the key, t, r' and the issuance proof's blindings; d again in d*S1: the
 * plans of afx_blind_request, afx_issue_blind and afx_unblind_issuances are prover-side plans and run under the context's
 * secret-independent addressing (afx_ctx_set_secret_independent_addressing, mode 2 by default) like afx_issue and afx_show.  The
 * PUBLIC verification inside afx_issue_blind (the request) and inside afx_unblind_issuances (the issuance proof) SHARES its plan's
 * secret setting - the flag is not toggled within a plan - so it runs the secret-independent tables too; afx_verify_blind_requests,
 * which holds no secret, runs the fast ones.  Rows that hold r', x0 + x1*t, y_i*m_i or d*S1 are zeroed on the device, in stream
 * order, before the call completes.
 *
 * Out of scope: mixed small layouts in one set of launches, coalescing, the batchable encoding of the two proofs, the Rust shim,
 * bench.py.  The issuer's side on bytes, over one context or a group and with its randomness drawn on the device, is "Blind issuance
 * on bytes" below, the user's side "Blind issuance on bytes: the user's doors" behind it.  The host-pointer forms
 * take the context in turn and stage a call in one piece; counts beyond afx_ctx_set_chunk_items run as several passes.  `_dev`:
 * every pointer a device pointer, rows 16-byte aligned, the call asynchronous on afx_ctx_stream. */
/* (declared apart from their typedefs, like afx_device_rng: the Rust shim does not bind them) */
struct afx_blind_request_randomness {
  const uint8_t* r_wide;      /* [h][count][64]  one-time encryption randomness per hidden position */
  const uint8_t* rng_seed;    /* [count][32]     the 32 bytes zkp's prove_compact draws              */
};
typedef struct afx_blind_request_randomness afx_blind_request_randomness;
struct afx_blind_request_soa {  /* written by afx_blind_request, read by the other three */
  uint8_t* D;                 /* [count] Pt                 */
  uint8_t* A;                 /* [h][count] Pt              */
  uint8_t* B;                 /* [h][count] Pt              */
  uint8_t* challenge;         /* [count] Sc                 */
  uint8_t* responses;         /* [1 + h + hs][count] Sc     */
};
typedef struct afx_blind_request_soa afx_blind_request_soa;
struct afx_blind_issue_randomness {
  const uint8_t* t_wide;      /* [count][64]  as afx_issue_randomness */
  const uint8_t* U_wide;      /* [count][64]                           */
  const uint8_t* rprime_wide; /* [count][64]  r'                       */
  const uint8_t* rng_seed;    /* [count][32]                           */
};
typedef struct afx_blind_issue_randomness afx_blind_issue_randomness;
struct afx_blind_issuance_soa { /* written by afx_issue_blind, read by afx_unblind_issuances */
  uint8_t* t;                 /* [count] Sc            */
  uint8_t* U;                 /* [count] Pt            */
  uint8_t* S1;                /* [count] Pt            */
  uint8_t* S2;                /* [count] Pt            */
  uint8_t* challenge;         /* [count] Sc            */
  uint8_t* responses;         /* [n + 6][count] Sc     */
};
typedef struct afx_blind_issuance_soa afx_blind_issuance_soa;
/* attrs->values: [n][count], all positions.  d: [count] Sc.  Any context. */
int afx_blind_request(afx_ctx* ctx, const afx_attributes_soa* attrs, const uint8_t* d, const afx_blind_request_randomness* rnd, size_t count,
                      const afx_blind_request_soa* out, uint8_t* status);
int afx_blind_request_dev(afx_ctx* ctx, const afx_attributes_soa* attrs, const uint8_t* d, const afx_blind_request_randomness* rnd, size_t count,
                          const afx_blind_request_soa* out, uint8_t* status_dev);
/* statuses only; attrs->values is not read (may be NULL).  Any context. */
int afx_verify_blind_requests(afx_ctx* ctx, const afx_attributes_soa* attrs, const afx_blind_request_soa* requests, uint32_t n_responses, size_t count,
                              uint8_t* status);
int afx_verify_blind_requests_dev(afx_ctx* ctx, const afx_attributes_soa* attrs, const afx_blind_request_soa* requests, uint32_t n_responses,
                                  size_t count, uint8_t* status_dev);
/* needs the issuer key (AFX_E_NO_KEY).  attrs->values: [n][count]; the rows of hidden positions are never read. */
int afx_issue_blind(afx_ctx* ctx, const afx_attributes_soa* attrs, const afx_blind_request_soa* requests, uint32_t request_n_responses,
                    const afx_blind_issue_randomness* rnd, size_t count, const afx_blind_issuance_soa* out, uint8_t* status);
int afx_issue_blind_dev(afx_ctx* ctx, const afx_attributes_soa* attrs, const afx_blind_request_soa* requests, uint32_t request_n_responses,
                        const afx_blind_issue_randomness* rnd, size_t count, const afx_blind_issuance_soa* out, uint8_t* status_dev);
/* requests: the user's own (D, A, B are read); attrs->values: the revealed positions' rows are read.  V: [count] Pt.  Any context. */
int afx_unblind_issuances(afx_ctx* ctx, const afx_attributes_soa* attrs, const uint8_t* d, const afx_blind_request_soa* requests,
                          const afx_blind_issuance_soa* issuances, uint32_t n_responses, size_t count, uint8_t* V, uint8_t* status);
int afx_unblind_issuances_dev(afx_ctx* ctx, const afx_attributes_soa* attrs, const uint8_t* d, const afx_blind_request_soa* requests,
                              const afx_blind_issuance_soa* issuances, uint32_t n_responses, size_t count, uint8_t* V, uint8_t* status_dev);

/* ---- Presentation tags: rate-limited shows with a per-scope pseudonym -------------------------
 * A presentation is unlinkable and afx_show takes no nonce or counter: nothing stops one credential from being shown a million times.
 * A TAGGED presentation also carries T = (m + n)^-1 * H, where m is a hidden scalar attribute of the credential, n a public per-item
 * counter and H a public generator that names the scope, with a proof that T was made from the attribute the MAC covers.  T is a
 * function of (attribute, n, scope) alone: a second show under the same counter and scope gives the same 32 bytes, shows under another
 * scope cannot be linked to it.  "At most N shows per credential and scope" is then the verifier's rule n < N on its own public rows plus
 * a set lookup on T.  (CMZ'14 MAC_GGM with a Dodis-Yampolskiy style tag, as the IETF ARC draft does.)  The crate has no counterpart.
 * Off unless called: nothing above changes.
 *
 * Protocol (normative).  p = the tag's position, whose credential kind is AFX_ATTR_SECRET_SCALAR; H = the scope generator, 32 bytes, one
 * per call; n = the item's counter, a canonical scalar (the library requires nothing else of it: enforcing n < limit is the caller's
 * policy); m = values[p].
 *
 * Scope generator.  afx_tag_scope_generator computes H = RistrettoPoint::from_uniform_bytes(SHA-512(scope)), dalek's
 * hash_from_bytes::<Sha512>, for a scope of 0 .. 1024 bytes.  A caller may pass any H; the soundness of the link between T and the
 * attribute, and unlinkability across scopes, need an H whose discrete logarithms to the system generators and to other scopes' H are
 * unknown.  Every call refuses an H that does not decode, or whose encoding is 32 zero bytes, with AFX_E_BAD_ARGS.
 *
 * 1. Show (user).  Everything afx_show does, byte for byte, from the same z_wide, rng_seed and enc_seeds.  In addition, per item,
 *      s = m + n mod l,   T = s^-1 * H,   C' = C_y[p] + n*G_m[p]  ( = z*G_y[p] + s*G_m[p] )
 *    and a compact proof under Transcript::new(b"2019/1416 anonymous credential") and the label "2019/1416 presentation tag proof":
 *      scalars      "z" (the presentation's z), "s"
 *      points       "G_y" = G_y[p], "G_m" = G_m[p], "H", "T", "C_y+nG_m" = C'
 *      constraints  C' = z*G_y + s*G_m;   H = s*T
 *    whose prove_compact draws from tag_seed[item].  Outputs: T, the challenge, two responses in the order (z, s).  An item whose n is
 *    not canonical, whose s is 0, or which fails afx_show itself fails with AFX_ST_VERIFICATION_FAILURE, and
 *    AN ITEM THAT FAILS GETS ZEROS IN EVERY OUTPUT ROW OF THE CALL - the presentation's rows included - written on the device
 *    (k_mask_rows, in front of k_finish) before the call completes.
 * 2. Verify (issuer).  status = AFX_ST_OK iff afx_verify_presentations accepts the presentation unchanged AND the tag proof verifies as a
 *    zkp Verifier verifies it: n, the challenge and both responses canonical, T decodes, neither T nor C' (computed from the received
 *    C_y[p]) encodes to 32 zero bytes, the recomputed challenge equals the received one.  A shape whose kinds[p] is not
 *    AFX_ENC_SECRET_SCALAR, or with p >= n_attributes, fails every item and no tag array is read.  The tag proof does not depend on
 *    strict mode; where the crate's constraint-#3 behaviour rejects honest presentations of a shape, the combined status rejects them too.
 *    afx_verify_tag_proofs is the analogue of afx_verify_encryption_proofs: the tag proof alone, on a row of received C_y[p]; any context.
 *
 * Why T is bound to the credential.  Constraint 1 extracts (z', s) with C_y[p] = z'*G_y[p] + (s - n)*G_m[p]; the presentation proof
 * extracts (z, m) for the same C_y[p]; binding under the discrete logarithm between G_y[p] and G_m[p] gives s = m + n; constraint 2
 * then fixes T = (m + n)^-1 * H.  Detecting equal T is a set lookup: afx_tagset (below) keeps such a set on the device.
 *
 * Secrets.  m, s and s^-1: the show is a prover-side plan under the context's secret-independent addressing like afx_show; s^-1 is made
 * by a kernel whose instruction stream and addresses do not depend on s (Fermat's inverse over the bits of the public l - 2), and the
 * rows that hold s and s^-1 are zeroed on the device, in stream order, before the call completes.  Verification is a public plan, as
 * afx_verify_presentations in each mode.
 *
 * Conventions.  `scope_generator` is a HOST pointer in every form, `_dev` included, read before the call returns.  The host-pointer
 * forms take the context in turn (they join no collecting session) and stage a call in one piece; counts beyond
 * afx_ctx_set_chunk_items run as several passes; small ones keep their plans like the other host-pointer calls (a plan-cache key of their
 * own, which holds the position).  `_dev`: every other pointer a device pointer, rows 16-byte aligned, the call asynchronous on
 * afx_ctx_stream with one exception: a call whose H is not the one its lane's buffer already holds waits for the work queued on that
 * stream (the copy of H leaves a pinned image; a new H also has its decoding read back).  Calls that repeat a scope - the usual case -
 * copy nothing and wait for nothing from the second call on each lane on (with afx_ctx_set_pipelining calls alternate between two lanes,
 * each of which copies H once), until a call needs a larger buffer: the buffer that replaces it receives H again.
 * Out of scope: a wire format for tagged presentations, afx_group_* forms, _rng draws of tag_seed, the batchable encoding of the tag
 * proof, mixed layouts and coalescing, the Rust shim, bench.py. */
/* (declared apart from their typedefs, like afx_device_rng: the Rust shim does not bind them) */
struct afx_tag_statement {
  uint32_t position;               /* p                                            */
  const uint8_t* scope_generator;  /* H, 32 bytes, HOST memory in every form       */
};
typedef struct afx_tag_statement afx_tag_statement;
struct afx_tags_soa {              /* a batch of received tags                     */
  const uint8_t* nonce;            /* [count] Sc     n                             */
  const uint8_t* T;                /* [count] Pt                                   */
  const uint8_t* challenge;        /* [count] Sc                                   */
  const uint8_t* responses;        /* [2][count] Sc  (z, s)                        */
};
typedef struct afx_tags_soa afx_tags_soa;
struct afx_tags_out {              /* written by afx_show_tagged                   */
  uint8_t* T;                      /* [count] Pt                                   */
  uint8_t* challenge;              /* [count] Sc                                   */
  uint8_t* responses;              /* [2][count] Sc                                */
};
typedef struct afx_tags_out afx_tags_out;
/* scope: scope_len bytes (0 .. 1024; may be NULL when 0).  Any context.  A cold-path helper: two calls of count 1. */
int afx_tag_scope_generator(afx_ctx* ctx, const uint8_t* scope, size_t scope_len, uint8_t out[32]);
/* as afx_show; nonce: [count] Sc; tag_seed: [count][32].  A position that is no hidden scalar of the credentials: AFX_E_BAD_ARGS. */
int afx_show_tagged(afx_ctx* ctx, const afx_credentials_soa* creds, const afx_keypairs_soa* keypairs, const afx_show_randomness* rnd,
                    const afx_tag_statement* tag, const uint8_t* nonce, const uint8_t* tag_seed, size_t count, const afx_presentation_out* out,
                    const afx_tags_out* tags_out, afx_shape* shape_out, uint8_t* status);
int afx_show_tagged_dev(afx_ctx* ctx, const afx_credentials_soa* creds, const afx_keypairs_soa* keypairs, const afx_show_randomness* rnd,
                        const afx_tag_statement* tag, const uint8_t* nonce, const uint8_t* tag_seed, size_t count, const afx_presentation_out* out,
                        const afx_tags_out* tags_out, afx_shape* shape_out, uint8_t* status_dev);
/* as afx_verify_presentations (needs the issuer key) */
int afx_verify_presentations_tagged(afx_ctx* ctx, const afx_shape* shape, const afx_presentation_soa* batch, const afx_tag_statement* tag,
                                    const afx_tags_soa* tags, size_t count, uint8_t* status);
int afx_verify_presentations_tagged_dev(afx_ctx* ctx, const afx_shape* shape, const afx_presentation_soa* batch, const afx_tag_statement* tag,
                                        const afx_tags_soa* tags, size_t count, uint8_t* status_dev);
/* C_y_p: [count] Pt, the presentations' C_y[p].  A position >= the context's n fails every item. */
int afx_verify_tag_proofs(afx_ctx* ctx, const afx_tag_statement* tag, const uint8_t* C_y_p, const afx_tags_soa* tags, size_t count, uint8_t* status);
int afx_verify_tag_proofs_dev(afx_ctx* ctx, const afx_tag_statement* tag, const uint8_t* C_y_p, const afx_tags_soa* tags, size_t count,
                              uint8_t* status_dev);

/* ---- The spent-tag set: check-and-insert of tags on the device ----------------------------------
 * "At most N shows per credential and scope" is n < N plus a set lookup on T.  An afx_tagset is that set, kept in HBM beside the rows a
 * tagged verification has just written: one call marks a batch of tags spent and says which of them were spent already.  Off unless
 * called: nothing above changes.
 *
 * Semantics of afx_tagset_spend (normative): the call answers as this loop would, for i = 0 .. count - 1 IN ORDER:
 *   - status_in given and status_in[i] != 0:   seen_out[i] = AFX_TAG_SKIPPED, nothing inserted (an item that failed verification);
 *   - else the 32 bytes T[i] are in the set:   seen_out[i] = AFX_TAG_SPENT;
 *   - else                                     seen_out[i] = AFX_TAG_FRESH and T[i] is inserted.
 * So among equal tags of one call the lowest index is the fresh one, whatever order the hardware takes them in.  Tags are compared as
 * the 32 bytes given, with no decoding (a tag that passed verification is canonical already).  afx_tagset_contains looks up and inserts
 * nothing: seen_out[i] = 1 iff T[i] is in the set.
 *
 * Capacity.  The set holds at most `capacity` tags (1 .. 2^30).  A call is refused with AFX_E_FULL, before anything is read or written,
 * unless (the known upper bound of the size) + count <= capacity, skipped items included: the host cannot know how many of a call's
 * tags are new before it runs.  The host forms refresh the exact size after every call; after _dev calls the bound is the last exact
 * size plus the counts since, until afx_tagset_size (which waits for the queued calls) refreshes it.  count > 2^32 - 3: AFX_E_BAD_ARGS.
 *
 * Layout and slot function (normative, so that tests can aim at slots).  n_slots = the smallest power of two >= 2 * capacity; open
 * addressing, linear probing with wrap-around;
 *   slot(T) = u64le( SHAKE256("aeonflux-amd/tagset/v1" (22 ASCII bytes) || salt (32) || T (32)) [0..8) ) mod n_slots
 * The salt (the caller's 32 bytes, or getrandom(2) for NULL) keeps a user who picks their own hidden scalar from aiming tags at one probe
 * chain; the answers do not depend on it.  Memory: 40 bytes per slot.
 *
 * Conventions.  A set belongs to the context it was created on (and to its device) and is destroyed BEFORE that context.  The host
 * forms take the context in turn and stage a call in one piece.  `_dev`: device pointers, rows 16-byte aligned, the call asynchronous on
 * afx_ctx_stream (with afx_ctx_set_pipelining calls alternate between two lanes; calls on one set are ordered behind each other on the
 * device whichever lane they take).  A HIP failure inside a call, or a table the kernels find inconsistent, leaves the set unusable:
 * every later call returns the first error.  No lane of the kernels ever waits for another lane (tagset.cuh).
 * Out of scope: removal, export and import of a set (a server that must survive a restart logs the tags it accepted). */
typedef struct afx_tagset afx_tagset;
#define AFX_TAG_FRESH 0
#define AFX_TAG_SPENT 1
#define AFX_TAG_SKIPPED 2
/* salt: 32 bytes or NULL (getrandom); capacity is a size_t like every count of this header */
int afx_tagset_create(afx_ctx* ctx, size_t capacity, const uint8_t* salt, afx_tagset** out);
void afx_tagset_destroy(afx_tagset* set);
/* waits for the queued calls; either output may be NULL */
int afx_tagset_size(afx_tagset* set, uint64_t* size_out, uint64_t* capacity_out);
/* T: [count][32]; status_in: [count] or NULL; seen_out: [count] */
int afx_tagset_spend(afx_tagset* set, const uint8_t* T, const uint8_t* status_in, size_t count, uint8_t* seen_out);
int afx_tagset_spend_dev(afx_tagset* set, const uint8_t* T, const uint8_t* status_in, size_t count, uint8_t* seen_out);
int afx_tagset_contains(afx_tagset* set, const uint8_t* T, size_t count, uint8_t* seen_out);
int afx_tagset_contains_dev(afx_tagset* set, const uint8_t* T, size_t count, uint8_t* seen_out);

/* ---- Blind issuance on bytes: AFXQ requests in, AFXJ issuances out ----------------------------
 * The issuer's side of the section above with the two doors the plain issuer has (afx_issue_wire, afx_issue_wire_rng): serialized
 * records, and randomness drawn on the device, over one context or a group.  Off unless called: nothing above changes.  H, h, hs as
 * above.  Both formats are the engine's own, in the style of AFXR / AFXI (32-byte cells, little-endian header words).
 *
 * "AFXQ" version 1: a batch of blind credential requests of one layout.
 *   header  = "AFXQ" | u32le 1 | u32le count | u32le cells_per_record | u32le n_attributes | u32le n_responses
 *             | kinds[n_attributes] (u8) | zero padding to a multiple of 32 bytes                -> (24 + n + 31) & ~31 bytes
 *   record  = D | A[h] | B[h] | challenge | responses[1 + h + hs] | the value of every REVEALED position, in position order
 *             (Sc for scalar kinds, Pt = M1 for point kinds); hidden positions have no value cell
 *   cells_per_record = 3 + 2h + hs + n_attributes.
 * Malformed (AFX_E_BAD_ARGS): a wrong magic or version, n_attributes > AFX_MAX_ATTRIBUTES, a kind above AFX_ATTR_SECRET_POINT,
 * n_responses != 1 + h + hs of the section's own kinds, a cells_per_record that does not match, a truncated header, header padding
 * that is not zero, a record area of the wrong length: a section that parses packs to the same bytes.  n_attributes = 0 is well
 * formed (cells_per_record 3, n_responses 1).
 *
 * "AFXJ" version 1: a batch of blind issuances.
 *   header  = "AFXJ" | u32le 1 | u32le count | u32le cells_per_record | u32le n_attributes | u32le n_responses | kinds[n_attributes]
 *             | zero padding to a multiple of 32 bytes
 *   record  = t | U | S1 | S2 | challenge | responses[n_responses]
 *   cells_per_record = 5 + n_responses.
 * n_attributes and the kinds echo the request section the AFXJ section answers; n_responses is the issuer context's n + 6, so a
 * section that answers a request of another n still parses (as in AFXI).  Malformed: as above, with n_responses >
 * AFX_MAX_ATTRIBUTES + 6 in the place of the response-count rule.  AFXJ carries no attribute values: the user holds them.
 *
 * Host only, bytes only, no context; each mirrors the AFXR function of the same role. */
size_t afx_blind_request_wire_header_bytes(uint32_t n_attributes);    /* 0 if n_attributes > AFX_MAX_ATTRIBUTES */
int afx_blind_request_wire_parse(const uint8_t* blob, size_t len, uint32_t* n_attributes_out, uint8_t kinds_out[AFX_MAX_ATTRIBUTES],
                                 uint32_t* n_responses_out, size_t* count_out, size_t* records_offset_out);
int afx_blind_request_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out);
/* attrs: n_attributes, kinds and values [n][count][32] (the value rows of hidden positions are not read); requests: host columns as
 * afx_blind_request wrote them.  blob == NULL only reports the length needed. */
int afx_blind_request_wire_pack(const afx_attributes_soa* attrs, const afx_blind_request_soa* requests, size_t count, uint8_t* blob,
                                size_t blob_cap, size_t* len_out);
size_t afx_blind_issuance_wire_header_bytes(uint32_t n_attributes);
int afx_blind_issuance_wire_parse(const uint8_t* blob, size_t len, uint32_t* n_attributes_out, uint8_t kinds_out[AFX_MAX_ATTRIBUTES],
                                  uint32_t* n_responses_out, size_t* count_out, size_t* records_offset_out);
int afx_blind_issuance_wire_section_bytes(const uint8_t* blob, size_t len, size_t* section_len_out);
/* attrs: n_attributes and kinds only (values is not read); issuances: host columns as afx_issue_blind wrote them */
int afx_blind_issuance_wire_pack(const afx_attributes_soa* attrs, const afx_blind_issuance_soa* issuances, uint32_t n_responses, size_t count,
                                 uint8_t* blob, size_t blob_cap, size_t* len_out);
/* afx_issue_blind over a stream of AFXQ sections: request bytes in, AFXJ bytes out, both transpositions on the GPU.
 *  - blob: AFXQ sections back to back.  Every section is parsed in full before anything runs or is written: a malformed section
 *    anywhere is AFX_E_BAD_ARGS with out and status untouched.
 *  - rnd: host arrays in stream order (item i of the stream uses t_wide[i], U_wide[i], rprime_wide[i], rng_seed[i]).
 *  - out: one AFXJ section per request section, in the same order, with the same count, n_attributes and kinds and n_responses =
 *    ctx n + 6.  status[i] answers the i-th request of the stream; *count_out = their number.
 *  - A section whose n_attributes is not the context's, or is 0, is all AFX_ST_MAC_CREATION with zero records (what afx_issue_blind
 *    answers a layout that does not fit).  An item whose status is not AFX_ST_OK has a record of zeros.  Every other record is byte for
 *    byte what afx_issue_blind + afx_blind_issuance_wire_pack make of the same inputs, and every status is that column path's.
 *  - out == NULL: only *out_len and *count_out, from the headers and the context's n; no device work, rnd may be NULL.
 *  - AFX_E_BAD_ARGS, with nothing written to out or status, for out_cap < *out_len, status_cap < the item count or a NULL randomness
 *    array; AFX_E_NO_KEY for a context without the issuer key.
 *  - Sections of one layout (n, kinds) are merged into one batch wherever they stand in the stream; a batch larger than
 *    afx_ctx_set_chunk_items runs as several slices, so staged memory stays bounded.
 *  - Like the column forms the call takes the context in turn and is NOT collected with other threads' calls: it stages slice after
 *    slice on the context's two lanes (host_pipe's lanes, asked never to hand the call, however small, to the collector).  Per
 *    slice the request records are transposed to struct-of-arrays rows (k_aos_to_soa: D, A, B, challenge and responses in front,
 *    each revealed value on the row of its attribute position; the rows of hidden positions exist and are never read),
 *    afx_issue_blind_dev runs on those rows, and k_soa_to_aos writes the AFXJ records: two launches beyond the plan.
 * The group form splits every merged batch over the members (afx_shard_bounds); a stream of at most afx_ctx_set_small_batch_items
 * requests goes whole to one member, in turn.  Bytes equal the one-context call's. */
int afx_issue_blind_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_blind_issue_randomness* rnd, uint8_t* out, size_t out_cap,
                         size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out);
int afx_group_issue_blind_wire(afx_group* group, const uint8_t* blob, size_t len, const afx_blind_issue_randomness* rnd, uint8_t* out,
                               size_t out_cap, size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out);
/* afx_verify_blind_requests on each section of the stream, the statuses concatenated; needs no key.  A section of another n is all
 * AFX_ST_VERIFICATION_FAILURE, as the column call answers it.  The same parsing and error contract; nothing but statuses is written. */
int afx_verify_blind_requests_wire(afx_ctx* ctx, const uint8_t* blob, size_t len, uint8_t* status, size_t status_cap, size_t* count_out);
/* The four draws of every request made on the device ("Randomness drawn on the device" above): t_wide, U_wide, rprime_wide and
 * rng_seed of the request with ordinal i in the stream are draw(seed, stream, i, AFX_DRAW_BLIND_T_WIDE / _U_WIDE / _RPRIME_WIDE /
 * _ISSUE_SEED).  Specified as an equivalence: the call returns what afx_issue_blind_wire returns when rnd holds those draws, error
 * codes included.  rng == NULL: AFX_E_BAD_ARGS.  A NULL seed is read from getrandom(2) once per call (a group call: one seed for the
 * whole group); the library zeroes its copies of the seed as the other *_rng forms do. */
int afx_issue_blind_wire_rng(afx_ctx* ctx, const uint8_t* blob, size_t len, const afx_device_rng* rng, uint8_t* out, size_t out_cap,
                             size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out);
int afx_group_issue_blind_wire_rng(afx_group* group, const uint8_t* blob, size_t len, const afx_device_rng* rng, uint8_t* out,
                                   size_t out_cap, size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out);

/* ---- Blind issuance on bytes: the user's doors -------------------------------------------------
 * The user's side of the two sections above on bytes (normative): attribute columns in, AFXQ request sections out, and AFXJ issuance
 * sections in, the credential's t, U, V out - with d, r_wide and rng_seed drawn on the device in the _rng forms, and over a group's
 * devices.  With them the blind protocol runs on bytes end to end: attributes -> AFXQ -> afx_issue_blind_wire -> AFXJ -> t, U, V ->
 * afx_show_wire -> AFXP -> verification.  Off unless called: nothing above changes.  Like the issuer's doors these calls take the
 * context in turn, stage slice after slice on the context's two lanes and are never collected with other threads' calls.  The Rust
 * shim and bench.py stay out of scope.
 *
 * afx_blind_request_wire: afx_blind_request over several groups of columns, one AFXQ v1 section per group out, in group order.
 *  - status[i] answers item i of the stream, counting the earlier groups' items (there is no positions array); *count_out = their
 *    number.  An item with status AFX_ST_OK gets a record that equals, byte for byte, what afx_blind_request followed by
 *    afx_blind_request_wire_pack makes of the same inputs.  Every other item gets a record of zeros, written on the device, and the
 *    column call's status (AFX_ST_MAC_CREATION).
 *  - A group whose n_attributes is not the context's, or is 0, gets a section of zero records, all AFX_ST_MAC_CREATION (as the issuer's
 *    door answers such a section).  Where n_attributes is 0 or above AFX_MAX_ATTRIBUTES the section has zero kinds: a header of
 *    afx_blind_request_wire_header_bytes(0) bytes with n_attributes 0, cells_per_record 3 and n_responses 1 - no array has a length
 *    beyond AFX_MAX_ATTRIBUTES.
 *  - AFX_E_BAD_ARGS, with out and status untouched: a kind above AFX_ATTR_SECRET_POINT among the first min(n_attributes,
 *    AFX_MAX_ATTRIBUTES) kinds of a group (no AFXQ header can carry it); a missing array (attrs.values, d, rnd.rng_seed, rnd.r_wide
 *    where a position is hidden) in a group with count > 0; out_cap or status_cap too small.  The layout is checked for groups of count
 *    0 too: their section still has a header.
 *  - out == NULL: only *out_len and *count_out, from the kinds and the counts; no device work, the arrays may be NULL.
 *  - Per slice afx_blind_request_dev writes D, A, B, the challenge and the responses into rows that lie behind the staged value rows,
 *    k_soa_to_aos makes the records of those rows and the value rows of the revealed positions (failed items zeroed), and the records
 *    come back in one fetch.  Groups run one after another; groups of one layout are not merged.
 *
 * afx_unblind_issuances_wire: afx_unblind_issuances over a stream of AFXJ sections and the AFXQ stream they answer.
 *  - requests: the AFXQ stream the user sent (the user's own D, A, B and the revealed values are read; hidden values are not needed).
 *    d: [total] Sc in stream order.  out: t, U, V, [total] each in stream order, ready to be afx_credentials_soa's t, U, V.
 *  - Both streams are parsed in full before anything runs.  The k-th AFXJ section pairs with the k-th AFXQ section: the section counts
 *    must match and each pair must agree on count, n_attributes and kinds.  Anything else, or a malformed section anywhere, is
 *    AFX_E_BAD_ARGS with nothing written; so are status_cap below the item count and a missing array.
 *  - A pair whose n_attributes is not the context's (or is 0), or whose AFXJ n_responses is not the context's n + 6, fails every item
 *    with AFX_ST_VERIFICATION_FAILURE, answered on the host as the column call answers it.
 *  - t and U are the record's, V = S2 - d*S1; the statuses and V equal afx_unblind_issuances' on the unpacked columns.  A failed item
 *    gets zeros in all three, written on the device before the call completes.  The zero records the issuer's door writes for the
 *    requests it refused fail here like any other issuance that does not verify.
 *  - Pairs of one layout are merged into one batch wherever they stand; a batch larger than afx_ctx_set_chunk_items runs as slices.  Per
 *    slice two k_aos_to_soa launches (the AFXJ cells, then the AFXQ cells) fill one row region, afx_unblind_issuances_dev runs on
 *    it, and k_soa_to_aos copies t, U and V out, a row each.
 *
 * The _rng forms ("Randomness drawn on the device" above), specified as equivalences:
 *  - afx_blind_request_wire_rng does not read the groups' d and rnd.  Item i of the stream uses d = from_bytes_mod_order_wide(draw(seed,
 *    stream, i, AFX_DRAW_BLINDREQ_D_WIDE)), reduced on the device (k_reduce_wide), r_wide[j] = draw(seed, stream, i,
 *    AFX_DRAW_BLINDREQ_R_WIDE(j)) for the j-th hidden position and rng_seed = draw(seed, stream, i, AFX_DRAW_BLINDREQ_SEED); it returns
 *    the bytes, statuses, lengths and error codes afx_blind_request_wire returns on those draws.  d_out, [total] Sc, receives d, zeros
 *    for a failed item; it may be NULL only when rng->seed is given - with a seed from getrandom(2) and no d_out the user could
 *    never unblind: AFX_E_BAD_ARGS.  The staged seed, the d_wide rows and the d rows are zeroed on the device before the call completes,
 *    failures included.  d is copied out of its scratch row - into a staged output row, itself zeroed on the device behind the copy
 *    that fetches it - only when d_out is given: with d_out == NULL no d leaves the device or outlives the call there.  What a caller
 *    asked for in d_out is an output like any other on the host (it passes the library's pinned result buffer on its way).
 *  - afx_unblind_issuances_wire_rng needs rng->seed (NULL: AFX_E_BAD_ARGS) and derives d again on the device from the same (seed,
 *    stream, index): a user who keeps the 32-byte seed and the AFXQ bytes holds no per-item secret, and d never crosses the bus.  It
 *    returns what afx_unblind_issuances_wire returns on the re-derived d.
 * The group forms split every group (the request door) or merged batch (the unblinding door) over the members (afx_shard_bounds), one
 * host thread per member; a stream of at most afx_ctx_set_small_batch_items items (member 0's) goes whole to one member, in turn.
 * The bytes equal the one-context call's: a draw depends on the item's index in the stream only. */
/* (declared apart from their typedefs, like the other blind structs: the Rust shim does not bind them) */
struct afx_blind_request_group {
  afx_attributes_soa attrs;            /* values [n][count], all positions            */
  const uint8_t* d;                    /* [count] Sc                                  */
  afx_blind_request_randomness rnd;    /* r_wide [h][count][64], rng_seed [count][32] */
  size_t count;
};
typedef struct afx_blind_request_group afx_blind_request_group;
struct afx_credential_out {
  uint8_t* t;                          /* [total] Sc, stream order */
  uint8_t* U;                          /* [total] Pt               */
  uint8_t* V;                          /* [total] Pt               */
};
typedef struct afx_credential_out afx_credential_out;
int afx_blind_request_wire(afx_ctx* ctx, const afx_blind_request_group* groups, size_t n_groups, uint8_t* out, size_t out_cap, size_t* out_len,
                           uint8_t* status, size_t status_cap, size_t* count_out);
int afx_group_blind_request_wire(afx_group* group, const afx_blind_request_group* groups, size_t n_groups, uint8_t* out, size_t out_cap,
                                 size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out);
int afx_blind_request_wire_rng(afx_ctx* ctx, const afx_blind_request_group* groups, size_t n_groups, const afx_device_rng* rng, uint8_t* d_out,
                               uint8_t* out, size_t out_cap, size_t* out_len, uint8_t* status, size_t status_cap, size_t* count_out);
int afx_group_blind_request_wire_rng(afx_group* group, const afx_blind_request_group* groups, size_t n_groups, const afx_device_rng* rng,
                                     uint8_t* d_out, uint8_t* out, size_t out_cap, size_t* out_len, uint8_t* status, size_t status_cap,
                                     size_t* count_out);
int afx_unblind_issuances_wire(afx_ctx* ctx, const uint8_t* issuances, size_t issuances_len, const uint8_t* requests, size_t requests_len,
                               const uint8_t* d, const afx_credential_out* out, uint8_t* status, size_t status_cap, size_t* count_out);
int afx_group_unblind_issuances_wire(afx_group* group, const uint8_t* issuances, size_t issuances_len, const uint8_t* requests,
                                     size_t requests_len, const uint8_t* d, const afx_credential_out* out, uint8_t* status, size_t status_cap,
                                     size_t* count_out);
int afx_unblind_issuances_wire_rng(afx_ctx* ctx, const uint8_t* issuances, size_t issuances_len, const uint8_t* requests, size_t requests_len,
                                   const afx_device_rng* rng, const afx_credential_out* out, uint8_t* status, size_t status_cap,
                                   size_t* count_out);
int afx_group_unblind_issuances_wire_rng(afx_group* group, const uint8_t* issuances, size_t issuances_len, const uint8_t* requests,
                                         size_t requests_len, const afx_device_rng* rng, const afx_credential_out* out, uint8_t* status,
                                         size_t status_cap, size_t* count_out);

/* ---- setup helpers (cold path; still GPU arithmetic) ---------------------------------------- */

/* IssuerParameters::generate (src/parameters.rs:349-362) and W = w*G_w (src/amacs.rs:104): given
 * sysparams and the key scalars laid out as amacs::SecretKey::to_bytes minus the trailing W
 * (u32 n || w || w' || x0 || x1 || y[n]), writes W (32 B) and C_W || I (64 B). */
int afx_issuer_keygen(int device, const uint8_t* sysparams, size_t sysparams_len, const uint8_t* key_scalars,
                      size_t key_scalars_len, uint8_t W_out[32], uint8_t issuer_params_out[64]);

/* SystemParameters::hash_and_pray (src/parameters.rs:196-326).  `rng_stream` stands in for csprng.fill_bytes: it is
 * consumed 32 bytes per attempt, in the reference's order (G_w, G_w', G_x0, G_x1, G_y.., G_m.., G_V, G_a, G_a0, G_a1);
 * the decompression tests run on the GPU.  Writes SystemParameters::to_bytes; *consumed_out = bytes of the stream used.
 * AFX_E_BAD_ARGS if the stream runs out, AFX_E_BAD_PARAMS for CredentialError::NoSystemParameters (duplicates). */
int afx_system_parameters_generate(int device, uint32_t n_attributes, const uint8_t* rng_stream, size_t stream_len,
                                   uint8_t* params_out, size_t params_cap, size_t* consumed_out);
/* ---- application data <-> attributes: plaintexts, keypairs, encryption, decryption ------------
 * Each of the four is ONE plan on the device - SHA-512 (k_sha512), encode_to_group's counter search (k_encode_to_group), Elligator,
 * the reductions and the multiscalar chains - in a host-pointer form, which stages its rows once and fetches once, and a *_dev
 * form: every pointer a device pointer (rows 16-byte aligned, counters 4-byte), the call asynchronous on afx_ctx_stream.  Counts
 * beyond afx_ctx_set_chunk_items run as several passes.  Rows that hold key material or a recovered plaintext on the way (the
 * wide hashes of the derive chain; decrypt's hash of the recovered message and a0 + a1*m3') are zeroed on the device, in stream
 * order, before the call completes. */

/* impl From<&[u8; 30]> for Plaintext (src/symmetric.rs:135-143): M1 = encode_to_group (src/encoding.rs:56-70; counter out),
 * M2 = hash-to-group, m3 = hash-to-scalar of SHA-512(msg).  msgs [count][30]: the only bytes that go to the device.
 * encode_to_group tries the counters 0 .. 8191 in the reference's order until a candidate decodes: ITS TRIP COUNT DEPENDS ON THE
 * MESSAGE, exactly as the reference's loop does (four tries on average; a lane per message).  counters may be NULL.
 * A message none of whose candidates decodes (the reference panics; probability (3/4)^8192): the host form returns AFX_E_BAD_ARGS,
 * the _dev form gives the item AFX_ST_VERIFICATION_FAILURE and zeroed outputs. */
int afx_plaintexts_from_bytes(afx_ctx* ctx, const uint8_t* msgs, size_t count, uint8_t* M1, uint8_t* M2, uint8_t* m3, uint32_t* counters);
int afx_plaintexts_from_bytes_dev(afx_ctx* ctx, const uint8_t* msgs, size_t count, uint8_t* M1, uint8_t* M2, uint8_t* m3, uint32_t* counters /* or NULL */,
                                  uint8_t* status);
/* Keypair::derive (src/symmetric.rs:197-215): master_secrets [count][64] -> a, a0, a1, pk ([count][32] each).  The three hashes
 * and reductions run as one chain on the device; pk under the context's secret-independent addressing. */
int afx_keypairs_derive(afx_ctx* ctx, const uint8_t* master_secrets, size_t count, uint8_t* a, uint8_t* a0, uint8_t* a1, uint8_t* pk);
int afx_keypairs_derive_dev(afx_ctx* ctx, const uint8_t* master_secrets, size_t count, uint8_t* a, uint8_t* a0, uint8_t* a1, uint8_t* pk);
/* Keypair::encrypt (src/symmetric.rs:252-261): status AFX_ST_VERIFICATION_FAILURE for a non-canonical scalar or an M1 / M2 that does
 * not decode.  keypairs->pk is not read. */
int afx_encrypt(afx_ctx* ctx, const afx_keypairs_soa* keypairs, const uint8_t* M1, const uint8_t* M2, const uint8_t* m3, size_t count,
                uint8_t* E1, uint8_t* E2, uint8_t* status);
int afx_encrypt_dev(afx_ctx* ctx, const afx_keypairs_soa* keypairs, const uint8_t* M1, const uint8_t* M2, const uint8_t* m3, size_t count,
                    uint8_t* E1, uint8_t* E2, uint8_t* status);
/* Keypair::decrypt (src/symmetric.rs:273-289): M1' = E2 - a*E1, m' = bytes 1..30 of its encoding (decode_from_group), m3' and M2'
 * from SHA-512(m'), E1' = (a0 + a1*m3')*M2'; status AFX_ST_UNDECRYPTABLE unless E1 - E1' is the identity (and for inputs that do not
 * decode or are not canonical).  M1, M2, m3 receive M1', M2', m3' for every item; `messages` [count][30] = m', may be NULL.
 * keypairs->pk is not read. */
int afx_decrypt(afx_ctx* ctx, const afx_keypairs_soa* keypairs, const uint8_t* E1, const uint8_t* E2, size_t count, uint8_t* M1,
                uint8_t* M2, uint8_t* m3, uint8_t* messages, uint8_t* status);
int afx_decrypt_dev(afx_ctx* ctx, const afx_keypairs_soa* keypairs, const uint8_t* E1, const uint8_t* E2, size_t count, uint8_t* M1,
                    uint8_t* M2, uint8_t* m3, uint8_t* messages /* or NULL */, uint8_t* status);

/* SHA-512 (FIPS 180-4) of `count` messages of msg_len bytes each (0 .. 1024; longer: AFX_E_BAD_ARGS), out [count][64]: the kernel the
 * four calls above hash with, as a batch primitive - published vectors run on the device.  Host pointers. */
int afx_sha512(afx_ctx* ctx, const uint8_t* msgs /*[count][msg_len]*/, size_t msg_len, size_t count, uint8_t* out /*[count][64]*/);

/* ---- whole messages: any length, one key per message -----------------------------------------
 * The request constructor of the crate takes application data of any length: CredentialRequestConstructor::append_plaintext
 * (src/user.rs:69-77) calls Plaintext::from_slice (src/symmetric.rs:118-133), which cuts the message into 30-byte chunks
 * (`chunks(30)`: the doc comment's "31-byte segments" is not what the code does), zero-pads the last one and makes one Plaintext per
 * chunk.  These calls do the same for a batch, and encrypt and decrypt whole messages under one key each.  Off unless called: no
 * existing call, plan or kernel changes.
 *
 * A batch of `count` messages is a byte `blob` and offsets[count + 1] (non-decreasing); message i is blob[offsets[i] .. offsets[i+1]).
 *  - Message i has chunks(i) = (len_i + 29) / 30 chunks.  An empty message has none, as slice.chunks(30) yields none.
 *  - chunk_first[i] is the sum of the earlier messages' chunk counts; n_chunks = chunk_first[count].
 *  - Chunk k of message i is row chunk_first[i] + k of every per-chunk array.  Its 30 bytes are the message's bytes 30k .. 30k + 29,
 *    zero-padded.
 *  - The length is not carried: b"abc" and b"abc\0" give the same rows, as in the crate.  A recovered message has 30 * chunks(i) bytes.
 * offsets and chunk_first are HOST arrays in every form, the *_dev forms included: they size the plan and are read before the call
 * returns.  Malformed input - decreasing offsets, a chunk_first that does not start at 0 or decreases, more than 2^32 - 1 chunks - is
 * AFX_E_BAD_ARGS and nothing is written.
 * In the *_dev forms the data pointers are device pointers, rows are 16-byte aligned (counters 4-byte), the blob has any alignment, and
 * the call is asynchronous on afx_ctx_stream.  The host-pointer forms stage the blob, the two tables and the keys (one row per
 * MESSAGE) once and fetch once.  Chunk rows beyond afx_ctx_set_chunk_items run as several passes, cut wherever that falls: a message's
 * chunks may lie in several passes, and what is decided per message is decided behind the last one.
 *
 * Secrets: the per-chunk copies of a, a0, a1, the hashes of recovered chunks, a0 + a1*m3' and the per-chunk M1', M2', m3' are zeroed on
 * the device, in stream order, before the call completes.  The encrypting and decrypting plans are afx_encrypt's and afx_decrypt's and
 * run under the context's secret-independent addressing.  The chunk -> message map depends on the public lengths only. */

/* (len + 29) / 30, for any len (no overflow).  Host only, no context. */
uint64_t afx_message_chunks(uint64_t len);
/* chunk_first_out[0 .. count] from offsets[0 .. count].  Host only, no context.  AFX_E_BAD_ARGS, nothing written: a NULL argument,
 * decreasing offsets, more than 2^32 - 1 chunks. */
int afx_messages_chunk_table(const uint64_t* offsets, size_t count, uint32_t* chunk_first_out /* [count + 1] */);

/* Plaintext::from_slice over a batch: M1, M2, m3 [n_chunks][32], counters [n_chunks] or NULL.  Row for row what
 * afx_plaintexts_from_bytes gives on the padded chunks, with its failure contract: the host form returns AFX_E_BAD_ARGS, the _dev form
 * gives a status per CHUNK (status [n_chunks]) and zeroed rows. */
int afx_plaintexts_from_messages(afx_ctx* ctx, const uint8_t* blob, const uint64_t* offsets, size_t count, uint8_t* M1, uint8_t* M2, uint8_t* m3,
                                 uint32_t* counters /* or NULL */);
int afx_plaintexts_from_messages_dev(afx_ctx* ctx, const uint8_t* blob, const uint64_t* offsets /* host */, size_t count, uint8_t* M1, uint8_t* M2,
                                     uint8_t* m3, uint32_t* counters /* or NULL */, uint8_t* status /* [n_chunks] */);
/* impl From<&RistrettoPoint> for Plaintext (src/symmetric.rs:152-161) - how a user rebuilds M2 and m3 of a point attribute held only as
 * a point: wide = SHA-512(the 32 bytes), M2 = from_uniform_bytes(wide), m3 = wide mod l.  points [count][32]; M2, m3 [count][32].  An
 * encoding that does not decode gets AFX_ST_VERIFICATION_FAILURE and zero rows; the identity is a valid input.  A ristretto encoding
 * that decodes is canonical, so the bytes hashed are the bytes given.  (This is NOT the triple afx_plaintexts_from_bytes gives for the
 * message a point encodes: the crate hashes different bytes.) */
int afx_plaintexts_from_points(afx_ctx* ctx, const uint8_t* points, size_t count, uint8_t* M2, uint8_t* m3, uint8_t* status);
int afx_plaintexts_from_points_dev(afx_ctx* ctx, const uint8_t* points, size_t count, uint8_t* M2, uint8_t* m3, uint8_t* status);
/* afx_plaintexts_from_bytes for a caller that kept the counters it returned ("XXX shortcut if counter is known", src/encoding.rs:54):
 * msgs [count][30], counters_in [count].  M1 is the candidate at counters_in[i] (bytes[0] = 2 * (c mod 128), bytes[31] = c / 128): ONE
 * decoding, no search.  c >= 8192, or a candidate that does not decode, gets AFX_ST_VERIFICATION_FAILURE and zero rows (M1, M2, m3).
 * The result equals afx_plaintexts_from_bytes' result if and only if c is the counter that call returns.  Any other accepted c gives
 * ANOTHER M1, which decode_from_group maps to the same 30 bytes (M2 and m3 do not depend on c). */
int afx_plaintexts_from_bytes_at(afx_ctx* ctx, const uint8_t* msgs, const uint32_t* counters_in, size_t count, uint8_t* M1, uint8_t* M2, uint8_t* m3,
                                 uint8_t* status);
int afx_plaintexts_from_bytes_at_dev(afx_ctx* ctx, const uint8_t* msgs, const uint32_t* counters_in, size_t count, uint8_t* M1, uint8_t* M2, uint8_t* m3,
                                     uint8_t* status);
/* Keypair::encrypt of every chunk of every message under the MESSAGE's key: keypairs->a, a0, a1 [count][32] (pk is not read);
 * E1, E2 [n_chunks][32], counters [n_chunks] or NULL, status [count] per MESSAGE.  Per chunk it is afx_encrypt of
 * afx_plaintexts_from_bytes.  A message fails as a whole - AFX_ST_VERIFICATION_FAILURE, zeros in all its E1 / E2 rows (and counters) -
 * if its key has a non-canonical scalar or any of its chunks fails.  A message of zero chunks writes no row. */
int afx_encrypt_messages(afx_ctx* ctx, const afx_keypairs_soa* keypairs, const uint8_t* blob, const uint64_t* offsets, size_t count, uint8_t* E1,
                         uint8_t* E2, uint32_t* counters /* or NULL */, uint8_t* status);
int afx_encrypt_messages_dev(afx_ctx* ctx, const afx_keypairs_soa* keypairs, const uint8_t* blob, const uint64_t* offsets /* host */, size_t count,
                             uint8_t* E1, uint8_t* E2, uint32_t* counters /* or NULL */, uint8_t* status);
/* Keypair::decrypt of every chunk (afx_decrypt) under the message's key: E1, E2 [n_chunks][32], chunk_first [count + 1] (host;
 * afx_messages_chunk_table), messages [n_chunks][30] - message i's 30 * chunks(i) bytes at 30 * chunk_first[i] - status [count].
 * A message is AFX_ST_UNDECRYPTABLE iff any of its chunks is, and ALL its 30 * chunks(i) bytes are then zeros, written on the device
 * before the call completes: nothing is released of a message that was not accepted (the rule of the blind calls' outputs), the chunks
 * that by themselves decrypted included.  A neighbour's bytes are untouched.  A message of zero chunks is AFX_ST_OK. */
int afx_decrypt_messages(afx_ctx* ctx, const afx_keypairs_soa* keypairs, const uint8_t* E1, const uint8_t* E2, const uint32_t* chunk_first, size_t count,
                         uint8_t* messages, uint8_t* status);
int afx_decrypt_messages_dev(afx_ctx* ctx, const afx_keypairs_soa* keypairs, const uint8_t* E1, const uint8_t* E2, const uint32_t* chunk_first /* host */,
                             size_t count, uint8_t* messages, uint8_t* status);

/* Batch ristretto255 primitives (dalek CompressedRistretto::decompress -> compress round trip,
 * RistrettoPoint::from_uniform_bytes, Scalar::from_bytes_mod_order_wide); used to build synthetic
 * attribute values and by the parity tests of the K* rows. */
int afx_points_from_uniform_bytes(afx_ctx* ctx, const uint8_t* wide /*[count][64]*/, size_t count, uint8_t* out /*[count] Pt*/);
int afx_scalars_from_wide_bytes(afx_ctx* ctx, const uint8_t* wide /*[count][64]*/, size_t count, uint8_t* out /*[count] Sc*/);
int afx_points_validate(afx_ctx* ctx, const uint8_t* pts /*[count] Pt*/, size_t count, uint8_t* ok /*[count]*/,
                        uint8_t* reencoded /*[count] Pt or NULL*/);
/* out[i] = sum_k scalars[k][i] * points[k][i]  (RistrettoPoint::multiscalar_mul, amacs.rs:270) */
int afx_multiscalar_mul(afx_ctx* ctx, uint32_t n_terms, const uint8_t* scalars /*[n_terms][count] Sc*/,
                        const uint8_t* points /*[n_terms][count] Pt*/, size_t count, uint8_t* out /*[count] Pt*/,
                        uint8_t* ok /*[count]*/);

/* A merlin transcript over a batch (the K* row's STROBE-128 / Keccak-f[1600] layer by itself: every proof of the crate is bound to a
 * merlin transcript through zkp's TranscriptProtocol [3P], e.g. src/nizk/presentation.rs:355-356 and :435).  The
 * transcript is given as a script - the operations of merlin::Transcript, byte strings length-prefixed with u32 LE:
 *     AFX_MERLIN_NEW          label                      Transcript::new(label); first, once
 *     AFX_MERLIN_APPEND       label, message             append_message(label, message): the same bytes for every item
 *     AFX_MERLIN_APPEND_FIELD label, u32 field index     append_message(label, fields[index][item]): a 32-byte per-item message
 *     AFX_MERLIN_CHALLENGE    label, u32 n (1 .. 64)     challenge_bytes(label, n bytes); the script ends with one
 * and out64[item] receives 64 bytes of which the first n are the LAST challenge (the rest is what the sponge's state held behind
 * them).  A challenge earlier in the script acts on the transcript as it must - label and length absorbed, the sponge permuted, its
 * bytes zeroed - but is not returned: a caller that chains challenges (each absorbed again) runs one call per challenge and feeds
 * the earlier ones back as fields.
 * Compiled and run exactly like the statements' own transcripts (strobe_sim.hpp, k_hash): all-constant leading blocks are absorbed
 * once on the host, everything from the first per-item field on by the kernel.  tests/test_gpu_primitives.py runs merlin's published
 * conformance vectors through it. */
#define AFX_MERLIN_NEW 1
#define AFX_MERLIN_APPEND 2
#define AFX_MERLIN_APPEND_FIELD 3
#define AFX_MERLIN_CHALLENGE 4
int afx_merlin_challenges(afx_ctx* ctx, const uint8_t* script, size_t script_len, const uint8_t* const* fields /* n_fields x [count][32] */,
                          uint32_t n_fields, size_t count, uint8_t* out64 /* [count][64] */);

#ifdef __cplusplus
}
#endif
#endif /* AEONFLUX_GPU_H */
