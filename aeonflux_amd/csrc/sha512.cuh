// SHA-512 (FIPS 180-4) for gfx950 and for the host: one hash per GPU lane, the eight state words and the sixteen words of the
// message schedule in registers.  Underlies what the reference hashes application data with: Plaintext::from (HashToG / HashToZZq of
// the 30 message bytes), Keypair::derive (three chained hashes of key material) and Keypair::decrypt (the recovered message).
//
// The 80 rounds are spelled out, so that every index into the schedule and the round constants is a compile-time value: a run-time
// index would send the schedule to scratch.  Nothing here looks a table up by, or branches on, a message byte - the reference calls
// these hashes on key material.  What the code does branch on is the message LENGTH and the position inside the message, which are
// the same for every item of a launch.
//
// Written on 64-bit words whose rotations are spelled on 32-bit halves (two v_alignbit_b32, or a swap of the halves for 32), as
// keccak.cuh does for the same reason.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define AFX_DEV __device__ __forceinline__

__device__ __constant__ const uint64_t SHA512_K[80] = {
  0x428a2f98d728ae22ULL, 0x7137449123ef65cdULL, 0xb5c0fbcfec4d3b2fULL, 0xe9b5dba58189dbbcULL, 0x3956c25bf348b538ULL, 0x59f111f1b605d019ULL,
  0x923f82a4af194f9bULL, 0xab1c5ed5da6d8118ULL, 0xd807aa98a3030242ULL, 0x12835b0145706fbeULL, 0x243185be4ee4b28cULL, 0x550c7dc3d5ffb4e2ULL,
  0x72be5d74f27b896fULL, 0x80deb1fe3b1696b1ULL, 0x9bdc06a725c71235ULL, 0xc19bf174cf692694ULL, 0xe49b69c19ef14ad2ULL, 0xefbe4786384f25e3ULL,
  0x0fc19dc68b8cd5b5ULL, 0x240ca1cc77ac9c65ULL, 0x2de92c6f592b0275ULL, 0x4a7484aa6ea6e483ULL, 0x5cb0a9dcbd41fbd4ULL, 0x76f988da831153b5ULL,
  0x983e5152ee66dfabULL, 0xa831c66d2db43210ULL, 0xb00327c898fb213fULL, 0xbf597fc7beef0ee4ULL, 0xc6e00bf33da88fc2ULL, 0xd5a79147930aa725ULL,
  0x06ca6351e003826fULL, 0x142929670a0e6e70ULL, 0x27b70a8546d22ffcULL, 0x2e1b21385c26c926ULL, 0x4d2c6dfc5ac42aedULL, 0x53380d139d95b3dfULL,
  0x650a73548baf63deULL, 0x766a0abb3c77b2a8ULL, 0x81c2c92e47edaee6ULL, 0x92722c851482353bULL, 0xa2bfe8a14cf10364ULL, 0xa81a664bbc423001ULL,
  0xc24b8b70d0f89791ULL, 0xc76c51a30654be30ULL, 0xd192e819d6ef5218ULL, 0xd69906245565a910ULL, 0xf40e35855771202aULL, 0x106aa07032bbd1b8ULL,
  0x19a4c116b8d2d0c8ULL, 0x1e376c085141ab53ULL, 0x2748774cdf8eeb99ULL, 0x34b0bcb5e19b48a8ULL, 0x391c0cb3c5c95a63ULL, 0x4ed8aa4ae3418acbULL,
  0x5b9cca4f7763e373ULL, 0x682e6ff3d6b2b8a3ULL, 0x748f82ee5defb2fcULL, 0x78a5636f43172f60ULL, 0x84c87814a1f0ab72ULL, 0x8cc702081a6439ecULL,
  0x90befffa23631e28ULL, 0xa4506cebde82bde9ULL, 0xbef9a3f7b2c67915ULL, 0xc67178f2e372532bULL, 0xca273eceea26619cULL, 0xd186b8c721c0c207ULL,
  0xeada7dd6cde0eb1eULL, 0xf57d4f7fee6ed178ULL, 0x06f067aa72176fbaULL, 0x0a637dc5a2c898a6ULL, 0x113f9804bef90daeULL, 0x1b710b35131c471bULL,
  0x28db77f523047d84ULL, 0x32caab7b40c72493ULL, 0x3c9ebe0a15c9bebcULL, 0x431d67c49c100d4cULL, 0x4cc5d4becb3e42b6ULL, 0x597f299cfc657e2aULL,
  0x5fcb6fab3ad6faecULL, 0x6c44198c4a475817ULL };

// low 32 bits of ((hi:lo) >> s), 0 < s < 32
AFX_DEV uint32_t sh_align(uint32_t hi, uint32_t lo, int s) {
#if defined(__HIPCC__)
  return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)s);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> s);
#endif
}
template <int N>
AFX_DEV uint64_t sh_rotr(uint64_t x) {
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  uint32_t rl, rh;
  if constexpr (N == 32) { rl = hi; rh = lo; }
  else if constexpr (N < 32) { rl = sh_align(hi, lo, N); rh = sh_align(lo, hi, N); }
  else { rl = sh_align(lo, hi, N - 32); rh = sh_align(hi, lo, N - 32); }
  return (uint64_t)rl | ((uint64_t)rh << 32);
}
AFX_DEV uint64_t sh_bsig0(uint64_t x) { return sh_rotr<28>(x) ^ sh_rotr<34>(x) ^ sh_rotr<39>(x); }
AFX_DEV uint64_t sh_bsig1(uint64_t x) { return sh_rotr<14>(x) ^ sh_rotr<18>(x) ^ sh_rotr<41>(x); }
AFX_DEV uint64_t sh_ssig0(uint64_t x) { return sh_rotr<1>(x) ^ sh_rotr<8>(x) ^ (x >> 7); }
AFX_DEV uint64_t sh_ssig1(uint64_t x) { return sh_rotr<19>(x) ^ sh_rotr<61>(x) ^ (x >> 6); }

AFX_DEV void sha512_init(uint64_t h[8]) {
  h[0] = 0x6a09e667f3bcc908ULL; h[1] = 0xbb67ae8584caa73bULL; h[2] = 0x3c6ef372fe94f82bULL; h[3] = 0xa54ff53a5f1d36f1ULL;
  h[4] = 0x510e527fade682d1ULL; h[5] = 0x9b05688c2b3e6c1fULL; h[6] = 0x1f83d9abfb41bd6bULL; h[7] = 0x5be0cd19137e2179ULL;
}
// Round I of a block.  The working variables a..h are s[(k - I) & 7], k = 0..7: a round renames them instead of moving them.  I is a
// template argument and the 80 rounds are spelled out below (SHA512_ROUNDS16): a loop of 80 such bodies is past what `#pragma
// unroll` unrolls, and left as a loop it indexes the schedule at run time.
template <int I>
AFX_DEV void sha512_round(uint64_t s[8], uint64_t w[16]) {
  if constexpr (I >= 16) w[I & 15] += sh_ssig1(w[(I - 2) & 15]) + w[(I - 7) & 15] + sh_ssig0(w[(I - 15) & 15]);
  const uint64_t a = s[(0 - I) & 7], b = s[(1 - I) & 7], c = s[(2 - I) & 7], e = s[(4 - I) & 7], f = s[(5 - I) & 7], g = s[(6 - I) & 7];
  const uint64_t t1 = s[(7 - I) & 7] + sh_bsig1(e) + ((e & f) ^ (~e & g)) + SHA512_K[I] + w[I & 15];
  const uint64_t t2 = sh_bsig0(a) + ((a & b) ^ (a & c) ^ (b & c));
  s[(3 - I) & 7] += t1;
  s[(7 - I) & 7] = t1 + t2;
}
#define SHA512_ROUNDS4(B) sha512_round<(B)>(s, w); sha512_round<(B) + 1>(s, w); sha512_round<(B) + 2>(s, w); sha512_round<(B) + 3>(s, w);
#define SHA512_ROUNDS16(B) SHA512_ROUNDS4(B) SHA512_ROUNDS4((B) + 4) SHA512_ROUNDS4((B) + 8) SHA512_ROUNDS4((B) + 12)
// one 1024-bit block, given as its sixteen big-endian words; w is used up
AFX_DEV void sha512_block(uint64_t h[8], uint64_t w[16]) {
  uint64_t s[8];
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = h[i];
  SHA512_ROUNDS16(0) SHA512_ROUNDS16(16) SHA512_ROUNDS16(32) SHA512_ROUNDS16(48) SHA512_ROUNDS16(64)
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] += s[i];
}

// The big-endian dword at bytes [4k, 4k + 4) of one block of the padded message  m || 0x80 || 0 ...  (the length field is the
// caller's): `mb` points at the block's first byte, `rem` = how many message bytes lie at and after it (negative once the 0x80 byte
// is behind).  k is a constant at every call, so that each load is the block's one address plus an immediate offset.
// ALIGNED: mb is 4-byte aligned, whole dwords inside the message are read as such.  Never reads at or past the message's end.
template <bool ALIGNED>
AFX_DEV uint32_t sha512_msg_dword(const uint8_t* mb, int32_t rem, int32_t k) {
  const int32_t p = 4 * k;
  if (ALIGNED && p + 4 <= rem) {
    const uint32_t v = reinterpret_cast<const uint32_t*>(mb)[k];
    return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
  }
  uint32_t v = 0;
#pragma unroll
  for (int32_t b = 0; b < 4; b++) {
    const int32_t q = p + b;
    const uint32_t byte = q < rem ? (uint32_t)mb[q] : (q == rem ? 0x80u : 0u);
    v = (v << 8) | byte;
  }
  return v;
}
// h = SHA-512(m[0 .. len)) as eight big-endian words: one block while len <= 111, a loop over blocks beyond
template <bool ALIGNED>
AFX_DEV void sha512_words(uint64_t h[8], const uint8_t* m, uint32_t len) {
  sha512_init(h);
  const uint32_t nblocks = (len + 17 + 127) / 128;   // the 0x80 byte and the 16-byte length field
#pragma unroll 1
  for (uint32_t blk = 0; blk < nblocks; blk++) {
    const uint8_t* mb = m + 128 * blk;
    const int32_t rem = (int32_t)len - (int32_t)(128 * blk);
    uint64_t w[16];
#pragma unroll
    for (int32_t j = 0; j < 16; j++)
      w[j] = ((uint64_t)sha512_msg_dword<ALIGNED>(mb, rem, 2 * j) << 32) | sha512_msg_dword<ALIGNED>(mb, rem, 2 * j + 1);
    if (blk + 1 == nblocks) w[15] |= (uint64_t)len * 8;   // (the padding left the field's words zero)
    sha512_block(h, w);
  }
}
// the digest's 64 bytes as sixteen little-endian dwords, the form the rows of the engine are stored in
AFX_DEV void sha512_digest_dwords(uint32_t out[16], const uint64_t h[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t hi = (uint32_t)(h[i] >> 32), lo = (uint32_t)h[i];
    out[2 * i] = (hi >> 24) | ((hi >> 8) & 0xff00u) | ((hi << 8) & 0xff0000u) | (hi << 24);
    out[2 * i + 1] = (lo >> 24) | ((lo >> 8) & 0xff00u) | ((lo << 8) & 0xff0000u) | (lo << 24);
  }
}

// encode_to_group's candidate `ctr` of a 30-byte message (the reference's src/encoding.rs:56-68, counter order `i` fastest):
// b[0] = 2 * (ctr % 128), b[1..31] = msg, b[31] = ctr / 128, as the eight little-endian dwords a decoding takes.  `mw`: the message
// as dwords - byte k of the message is byte k of mw, bytes 30 and 31 are ignored.
AFX_DEV void encode_candidate(uint32_t w[8], const uint32_t mw[8], uint32_t ctr) {
  w[0] = (2u * (ctr & 127u)) | (mw[0] << 8);
#pragma unroll
  for (int i = 1; i < 8; i++) w[i] = (mw[i - 1] >> 24) | (mw[i] << 8);
  w[7] = (w[7] & 0x00ffffffu) | ((ctr >> 7) << 24);
}
