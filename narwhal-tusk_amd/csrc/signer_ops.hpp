// signer_ops.hpp -- per-lane operations of a signer bound to ONE key, shared by the gfx950
// kernels (k_signer.hip) and the host (cpu_lane.cpp, tests/cpp/signer/): the outbound half of a
// primary -- Vote::new + bincode of PrimaryMessage::Vote (primary/src/messages.rs:114-129,
// crypto/src/lib.rs:185-191) and SignatureService::request_signature (crypto/src/lib.rs:229-250).
//
//   signer_key_setup   the key record of a seed: the first half of sign_one, done once per signer
//   sign_fixed_one     RFC 8032 signature of a 32-byte message held in registers with that record:
//                      no key expansion and no [a]B; the bytes sign_one gives for the seed
//   vote_digest_words  Vote::digest = SHA-512(id || round LE || origin)[..32], one block from registers
//   b64_encode32       a 32-byte key's canonical base64 text (44 characters, as ingest_gpu.cpp b64_32)
//   vote_wire_words    the 212 bytes of PrimaryMessage::Vote (msg_plan.hpp) as 53 little-endian dwords
//
// NOT CONSTANT TIME: the comb lookups are indexed by digits of the secret nonce and the
// conversion of R to bytes inverts Z with the variable-time binary GCD; like
// nt_ed25519_sign_batch this is for a node that trusts the machine it runs on.
#pragma once
#include "ed25519_ops.hpp"

namespace nt {

// 192 bytes, three 64-byte lines.
struct SignerKey {
  uint32_t a[8];       // the clamped scalar (SHA-512(seed)[..32], clamped)
  uint32_t ared[8];    // a mod L
  uint32_t prefix[8];  // SHA-512(seed)[32..]
  uint32_t A[8];       // the public key bytes [a]B
  uint32_t text[11];   // A's base64 text, 44 characters
  uint32_t pad[5];
};
static_assert(sizeof(SignerKey) == 192, "SignerKey is three 64-byte lines");

constexpr int kVoteWireBytes = 212;
constexpr int kVoteWireWords = kVoteWireBytes / 4;
static_assert(kVoteWireWords * 4 == kVoteWireBytes, "a vote is whole dwords");

// byte i of little-endian words (i a compile-time constant after unrolling)
NT_HD NT_INLINE uint32_t word_byte(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// one base64 character (standard alphabet) of a 6-bit value, without a table
NT_HD NT_INLINE uint32_t b64_char(uint32_t c) {
  uint32_t r = c + 65u;                 // 'A' + c
  r = c >= 26u ? c + 71u : r;           // 'a' + c - 26
  r = c >= 52u ? c - 4u : r;            // '0' + c - 52
  r = c == 62u ? 43u : r;               // '+'
  r = c == 63u ? 47u : r;               // '/'
  return r;
}

// text[0..11) = the 44 characters of base64(k[0..32)), '=' padded
NT_HD NT_INLINE void b64_encode32(uint32_t text[11], const uint32_t k[8]) {
#pragma unroll
  for (int g = 0; g < 11; ++g) {
    const uint32_t b0 = word_byte(k, 3 * g);
    const uint32_t b1 = 3 * g + 1 < 32 ? word_byte(k, 3 * g + 1 < 32 ? 3 * g + 1 : 0) : 0u;
    const uint32_t b2 = 3 * g + 2 < 32 ? word_byte(k, 3 * g + 2 < 32 ? 3 * g + 2 : 0) : 0u;
    const uint32_t v = (b0 << 16) | (b1 << 8) | b2;
    const uint32_t c0 = b64_char((v >> 18) & 63u), c1 = b64_char((v >> 12) & 63u);
    const uint32_t c2 = 3 * g + 1 < 32 ? b64_char((v >> 6) & 63u) : 61u;  // '='
    const uint32_t c3 = 3 * g + 2 < 32 ? b64_char(v & 63u) : 61u;
    text[g] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
  }
}

// Conversion of R (and of A at setup) to bytes: ge_tobytes_w with the variable-time binary GCD
// of fe_inv_vt.hpp in place of the Fermat chain -- measured 21 % off the kernel's time (DESIGN.md
// section 12).  -DNT_SIGNER_INV_VT=0 (A/B builds) restores what sign_one does.  Neither is
// constant time.
#ifndef NT_SIGNER_INV_VT
#define NT_SIGNER_INV_VT 1
#endif
NT_HD NT_INLINE void signer_tobytes_w(uint32_t w[8], const ge_p2& p) {
#if NT_SIGNER_INV_VT
  fe zi, x, y;
  fe_invert_vt(zi, p.Z);
  fe_mul(x, p.X, zi);
  fe_mul(y, p.Y, zi);
  fe_tobytes_w(w, y);
  w[7] ^= fe_isneg(x) << 31;
#else
  ge_tobytes_w(w, p);
#endif
}

// The key record of a 32-byte seed (sw = its words); wb = a wide comb of B.
template <class WComb>
NT_HD NT_INLINE void signer_key_setup(SignerKey& key, const uint32_t sw[8], const WComb& wb) {
  uint64_t st[8];
  sha512_prefixed<8>(st, sw, nullptr, 0);
  uint32_t h[16];
  sha512_out_words(h, st, 16);
#pragma unroll
  for (int q = 0; q < 8; ++q) { key.a[q] = h[q]; key.prefix[q] = h[8 + q]; }
  key.a[0] &= 0xfffffff8u;
  key.a[7] &= 0x3fffffffu;
  key.a[7] |= 0x40000000u;
  sc_reduce256(key.ared, key.a);
  ge_p3 P;
  ge_p2 P2;
  wcomb_acc<WComb, true>(P, key.ared, wb);
  ge_p3_to_p2(P2, P);
  signer_tobytes_w(key.A, P2);
  b64_encode32(key.text, key.A);
#pragma unroll
  for (int q = 0; q < 5; ++q) key.pad[q] = 0u;
}

// SHA-512 of NW message words (4 NW <= 111 bytes: one block) built from registers
template <int NW>
NT_HD NT_INLINE void sha512_words_1block(uint64_t st[8], const uint32_t* m) {
  static_assert(NW <= 27, "one block");
  sha512_init(st);
  uint32_t blk[32];
#pragma unroll
  for (int i = 0; i < NW; ++i) blk[i] = m[i];
  blk[NW] = 0x80u;
#pragma unroll
  for (int i = NW + 1; i < 31; ++i) blk[i] = 0u;
  blk[31] = bswap32((uint32_t)NW * 32u);  // big-endian bit length
  sha512_compress_words(st, blk);
}

// (R, s) = the RFC 8032 signature of the 32-byte message m under `key`.
template <class WComb>
NT_HD NT_INLINE void sign_fixed_one(uint32_t Rw[8], uint32_t s[8], const SignerKey& key, const uint32_t m[8],
                                    const WComb& wb) {
  uint32_t in[16];
#pragma unroll
  for (int q = 0; q < 8; ++q) { in[q] = key.prefix[q]; in[8 + q] = m[q]; }
  uint64_t st[8];
  sha512_words_1block<16>(st, in);
  uint32_t hr[16], r[8];
  sha512_out_words(hr, st, 16);
  sc_reduce512(r, hr);
  ge_p3 P;
  ge_p2 P2;
  wcomb_acc<WComb, true>(P, r, wb);
  ge_p3_to_p2(P2, P);
  signer_tobytes_w(Rw, P2);
  // k = SHA-512(R || A || M) mod L: the one-block path hram_scalar<true> takes for a 32-byte M,
  // fed from registers
  uint32_t ra[16];
#pragma unroll
  for (int q = 0; q < 8; ++q) { ra[q] = Rw[q]; ra[8 + q] = key.A[q]; }
  sha512_96(st, ra, m);
  uint32_t hk[16], k[8];
  sha512_out_words(hk, st, 16);
  sc_reduce512(k, hk);
  sc_muladd(s, k, key.a, r);
}

// out8 = SHA-512(id || round LE || origin)[..32]
NT_HD NT_INLINE void vote_digest_words(uint32_t out8[8], const uint32_t id[8], uint64_t round, const uint32_t origin[8]) {
  uint32_t in[18];
#pragma unroll
  for (int q = 0; q < 8; ++q) { in[q] = id[q]; in[10 + q] = origin[q]; }
  in[8] = (uint32_t)round;
  in[9] = (uint32_t)(round >> 32);
  uint64_t st[8];
  sha512_words_1block<18>(st, in);
  sha512_out_words(out8, st, 8);
}

// u32 1 | id 32 | u64 round | u64 44 | origin text 44 | u64 44 | author text 44 | R 32 | s 32
NT_HD NT_INLINE void vote_wire_words(uint32_t out[kVoteWireWords], const uint32_t id[8], uint64_t round,
                                     const uint32_t origin[8], const uint32_t author_text[11], const uint32_t R[8],
                                     const uint32_t s[8]) {
  uint32_t otext[11];
  b64_encode32(otext, origin);
  out[0] = 1u;
#pragma unroll
  for (int q = 0; q < 8; ++q) out[1 + q] = id[q];
  out[9] = (uint32_t)round;
  out[10] = (uint32_t)(round >> 32);
  out[11] = 44u;
  out[12] = 0u;
#pragma unroll
  for (int q = 0; q < 11; ++q) out[13 + q] = otext[q];
  out[24] = 44u;
  out[25] = 0u;
#pragma unroll
  for (int q = 0; q < 11; ++q) out[26 + q] = author_text[q];
#pragma unroll
  for (int q = 0; q < 8; ++q) { out[37 + q] = R[q]; out[45 + q] = s[q]; }
}

// One vote: the wire dwords and the digest that was signed.
template <class WComb>
NT_HD NT_INLINE void vote_one(uint32_t out[kVoteWireWords], uint32_t dg[8], const SignerKey& key, const uint32_t id[8],
                              uint64_t round, const uint32_t origin[8], const WComb& wb) {
  vote_digest_words(dg, id, round, origin);
  uint32_t Rw[8], s[8];
  sign_fixed_one(Rw, s, key, dg, wb);
  vote_wire_words(out, id, round, origin, key.text, Rw, s);
}

}  // namespace nt
