"""ntcrypto -- MI355X (gfx950) backend for Narwhal/Tusk's crypto hot path.

Bulk API: `Backend` (numpy in/out over the C ABI, include/ntcrypto.h).
Crate mirror: `Digest, PublicKey, SecretKey, Signature, SignatureService,
CryptoError, generate_keypair` (crypto/src/lib.rs) and the primary/worker
callers in `ntcrypto.narwhal` (primary/src/messages.rs, worker/src/processor.rs).
"""
from ._lib import (EXPORTED, LIB_PATH, NT_KEY_STRICT_BIT, NT_MODE_COFACTORLESS, NT_MODE_MIXED, NT_MODE_STRICT,
                   NT_SMALL_ALWAYS, NT_SMALL_AUTO, NT_SMALL_OFF, RECEIPT_DTYPE, RECEIPT_GENESIS, RECEIPT_KIND_HOST,
                   SIGNER_EXPORTED, VOTE_BYTES, Signer,
                   WMSG_HOST, WMSG_OK, WMSG_SERIALIZATION, WORKER_KIND_BATCH, WORKER_KIND_NONE, WORKER_KIND_REQUEST,
                   WORKER_RECEIPT_DTYPE, WORKER_RECEIPT_UNIFORM, Backend, Committee, Keyset, NtError, default_backend,
                   load_library, nbytes)
from .crypto import (CryptoError, Digest, PublicKey, SecretKey, Signature, SignatureService,
                     generate_keypair, generate_production_keypair, sha512_digest, sha512_digest_batch)

__all__ = [
    "Backend", "Committee", "Keyset", "NtError", "default_backend", "load_library", "EXPORTED", "LIB_PATH",
    "NT_MODE_STRICT", "NT_MODE_COFACTORLESS", "NT_MODE_MIXED", "NT_KEY_STRICT_BIT", "NT_SMALL_OFF", "NT_SMALL_AUTO",
    "NT_SMALL_ALWAYS", "RECEIPT_DTYPE", "RECEIPT_GENESIS", "RECEIPT_KIND_HOST", "CryptoError", "Digest", "nbytes",
    "PublicKey", "SecretKey", "WORKER_RECEIPT_DTYPE", "WORKER_RECEIPT_UNIFORM", "WMSG_OK", "WMSG_SERIALIZATION",
    "WMSG_HOST", "WORKER_KIND_BATCH", "WORKER_KIND_REQUEST", "WORKER_KIND_NONE",
    "Signature", "SignatureService", "generate_keypair", "generate_production_keypair",
    "sha512_digest", "sha512_digest_batch", "Signer", "SIGNER_EXPORTED", "VOTE_BYTES",
]
