/* ntsigner.h -- the signer bound to a node's own key (libntcrypto.so, beside ntcrypto.h).
 *
 * The outbound half of a primary: what Core does with every header it accepts
 * (primary/src/core.rs:184-211 -> Vote::new, primary/src/messages.rs:114-129) and what
 * SignatureService::request_signature does for the node's own headers
 * (crypto/src/lib.rs:185-191, 229-250), for n items in one launch:
 *
 *   nts_votes_sign     (id, round, origin) -> Vote::digest, its signature and the 212 bytes
 *                      of bincode(PrimaryMessage::Vote), ready to send
 *   nts_sign_digests   32-byte digests -> 64-byte signatures
 *
 * A signer holds the expanded key (SHA-512(seed), the public key and its base64 text),
 * computed once at nts_signer_create: a call performs no key expansion and no [a]B.
 * The signatures are the RFC 8032 ones nt_ed25519_sign_batch gives for the seed.
 *
 * NOT constant time (as nt_ed25519_sign_batch): table lookups are indexed by digits of the
 * secret nonce.  The secret lives in the caller's memory, in the signer's host copy and in
 * one 192-byte record per device entry; nts_signer_free zeroes the latter two.  Nothing is
 * persisted.
 *
 * The calls need no key set and no committee; like signing they build nothing but the comb
 * of B.  They follow the small-call path of the context (nt_set_small_call_path): a call
 * that a key-cache verification of the same size would keep on the host stays on the host.
 * Thread safety and error codes are those of ntcrypto.h.
 */
#ifndef NTSIGNER_H
#define NTSIGNER_H

#include "ntcrypto.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NTS_VOTE_BYTES 212 /* u32 1 | id 32 | u64 round | u64 44 | origin b64 44 | u64 44 | author b64 44 | sig 64 */

typedef struct nts_signer nts_signer;

/* The signer of seed32 on ctx: a key record on every device entry and a host copy.  The
 * signer must be freed before its context. */
int nts_signer_create(nt_ctx *ctx, const uint8_t seed32[32], nts_signer **out);
/* Zeroes the host copy and the device records, then frees them.  NULL is ignored. */
void nts_signer_free(nts_signer *s);
int nts_signer_public(const nts_signer *s, uint8_t pk32[32]);

/* sig64[i] = the signature of digest32[i] (n x 32 bytes in, n x 64 out). */
int nts_sign_digests(nt_ctx *ctx, const nts_signer *s, const uint8_t *digest32, uint64_t n, uint8_t *sig64);

/* Vote i for header (id32[i], round[i]) of author origin32[i] (the raw 32-byte key; it need
 * not be a curve point): out_vote212[i] = the wire bytes of PrimaryMessage::Vote,
 * out_digest32[i] (nullable array) = Vote::digest.  n == 0 returns NT_OK; a NULL array with
 * n > 0 returns NT_EINVAL.  out_vote212 may be pageable or nt_host_alloc memory. */
int nts_votes_sign(nt_ctx *ctx, const nts_signer *s, const uint8_t *id32, const uint64_t *round,
                   const uint8_t *origin32, uint64_t n, uint8_t *out_vote212, uint8_t *out_digest32);

/* The same over device buffers of device entry `dev`, enqueued on the caller's stream
 * (stream-ordered, nothing is waited for).  d_id32, d_origin32, d_vote212 and d_digest32
 * (nullable) are 16-byte aligned and d_round 8-byte aligned, else NT_EINVAL. */
int nts_dev_votes_sign(nt_ctx *ctx, const nts_signer *s, int dev, void *stream, const uint8_t *d_id32,
                       const uint64_t *d_round, const uint8_t *d_origin32, uint64_t n, uint8_t *d_vote212,
                       uint8_t *d_digest32);

#ifdef __cplusplus
}
#endif
#endif /* NTSIGNER_H */
