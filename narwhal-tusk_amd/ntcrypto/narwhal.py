"""ctypes binding of libntnarwhal.so (narwhal-tusk_amd/host/capi.cpp): the C++
mirror of the primary's callers of the crypto hot path.

  Core            primary::Core batched sanitize over bincode wire messages
                  (core.rs:306-411, SURVEY §8(f).1 + (f).2); verdicts are
                  primary::DagError codes (DAG_ERRORS)
  wire_reencode   decode + re-encode one bincode PrimaryMessage (codec check)

Signature work runs on the GPU through libntcrypto.so; the wire decode runs on
host threads.  A backend failure raises, it is never turned into a verdict.
"""
import ctypes
import os

import numpy as np

from ._lib import PKG_ROOT, RECEIPT_DTYPE, WORKER_RECEIPT_DTYPE, NtError

LIB_PATH = os.path.join(PKG_ROOT, "lib", "libntnarwhal.so")
DAG_ERRORS = ["Ok", "InvalidSignature", "InvalidHeaderId", "MalformedHeader", "UnknownAuthority",
              "AuthorityReuse", "CertificateRequiresQuorum", "TooOld", "UnexpectedVote", "SerializationError",
              "UnexpectedMessage"]
_u8p = ctypes.POINTER(ctypes.c_uint8)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NtError("libntnarwhal.so not built (%s); run `make -C narwhal-tusk_amd`" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        lib.ntn_wire_reencode.argtypes = [_u8p, ctypes.c_uint64, _u8p, ctypes.c_uint64, _u64p]
        lib.ntn_wire_reencode.restype = ctypes.c_int64
        lib.ntn_wire_header_preimage.argtypes = [_u8p, ctypes.c_uint64, _u8p, ctypes.c_uint64]
        lib.ntn_wire_header_preimage.restype = ctypes.c_int64
        lib.ntn_core_new.argtypes = [_u8p, _u32p, _u32p, ctypes.c_uint32, ctypes.c_uint64, _u8p, ctypes.c_uint64,
                                     ctypes.c_int]
        lib.ntn_core_new.restype = ctypes.c_void_p
        lib.ntn_core_free.argtypes = [ctypes.c_void_p]
        lib.ntn_core_free.restype = None
        lib.ntn_core_ingest.argtypes = [ctypes.c_void_p, _u8p, _u64p, _u64p, ctypes.c_uint64, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), ctypes.c_int]
        lib.ntn_core_ingest.restype = ctypes.c_int
        lib.ntn_core_ingest_receipts.argtypes = [ctypes.c_void_p, _u8p, _u64p, _u64p, ctypes.c_uint64, ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, _u64p]
        lib.ntn_core_ingest_receipts.restype = ctypes.c_int
        lib.ntn_core_ingest_pipelined.argtypes = [ctypes.c_void_p, _u8p, _u64p, _u64p, ctypes.c_uint64, ctypes.c_int,
                                                  ctypes.c_uint64, ctypes.POINTER(ctypes.c_int32)]
        lib.ntn_core_ingest_pipelined.restype = ctypes.c_int
        lib.ntn_core_set_signer.argtypes = [ctypes.c_void_p, _u8p, _u8p]
        lib.ntn_core_set_signer.restype = ctypes.c_int
        lib.ntn_core_votes_for.argtypes = [ctypes.c_void_p, ctypes.c_void_p, _u32p, ctypes.c_uint64, _u8p]
        lib.ntn_core_votes_for.restype = ctypes.c_int
        lib.ntn_last_ingest_stats.argtypes = [ctypes.POINTER(ctypes.c_double)]
        lib.ntn_last_ingest_stats.restype = None
        lib.ntn_batcher_new.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
        lib.ntn_batcher_new.restype = ctypes.c_void_p
        lib.ntn_batcher_free.argtypes = [ctypes.c_void_p]
        lib.ntn_batcher_free.restype = None
        lib.ntn_batcher_submit.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, _u8p, ctypes.c_uint64]
        lib.ntn_batcher_submit.restype = ctypes.c_void_p
        lib.ntn_batcher_wait.argtypes = [ctypes.c_void_p, _u8p, _u8p]
        lib.ntn_batcher_wait.restype = ctypes.c_int
        lib.ntn_batcher_flush.argtypes = [ctypes.c_void_p]
        lib.ntn_batcher_flush.restype = None
        lib.ntn_batcher_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
        lib.ntn_batcher_stats.restype = None
        lib.ntn_set_small_call_path.argtypes = [ctypes.c_int, ctypes.c_int]
        lib.ntn_set_small_call_path.restype = ctypes.c_int
        lib.ntn_worker_decode.argtypes = [_u8p, ctypes.c_uint64, _u64p, _u8p]
        lib.ntn_worker_decode.restype = ctypes.c_int
        lib.ntn_worker_ingest.argtypes = [ctypes.c_uint32, _u8p, _u64p, _u64p, ctypes.c_uint64, _u8p, _u8p, _u8p, _u8p,
                                          _u32p, ctypes.c_void_p, _u64p]
        lib.ntn_worker_ingest.restype = ctypes.c_int
        _lib = lib
    return _lib


def _buf(b):
    a = np.frombuffer(b, np.uint8) if len(b) else np.zeros(1, np.uint8)
    return a, a.ctypes.data_as(_u8p)


def wire_reencode(msg: bytes):
    """(re-encoded bytes, bytes consumed) or None on a bincode decode error"""
    a, p = _buf(msg)
    out = np.zeros(2 * len(msg) + 64, np.uint8)
    used = ctypes.c_uint64(0)
    r = load().ntn_wire_reencode(p, len(msg), out.ctypes.data_as(_u8p), len(out), ctypes.byref(used))
    return None if r < 0 else (out[:r].tobytes(), used.value)


def wire_header_preimage(msg: bytes):
    a, p = _buf(msg)
    out = np.zeros(len(msg) + 64, np.uint8)
    r = load().ntn_wire_header_preimage(p, len(msg), out.ctypes.data_as(_u8p), len(out))
    return None if r < 0 else out[:r].tobytes()


def pack(messages):
    """packed buffer + offsets + lengths of a list of byte strings"""
    ln = np.array([len(m) for m in messages], np.uint64)
    off = np.zeros(len(messages), np.uint64)
    if len(messages) > 1:
        off[1:] = np.cumsum(ln)[:-1]
    data = np.frombuffer(b"".join(messages), np.uint8) if messages else np.zeros(1, np.uint8)
    return data, off, ln


class Core:
    """primary::Core for one committee: keys (n x 32 B), stakes, workers per
    authority, GC round and the header currently being voted on (bincode of a
    PrimaryMessage::Header, or None); use_keyset builds the committee key cache."""

    def __init__(self, keys, stakes, nworkers, gc_round=0, current_header=None, use_keyset=True):
        lib = load()
        keys = np.ascontiguousarray(np.asarray(keys, np.uint8).reshape(-1, 32))
        stakes = np.ascontiguousarray(stakes, np.uint32)
        nworkers = np.ascontiguousarray(nworkers, np.uint32)
        ch, chp = _buf(current_header or b"")
        self._h = lib.ntn_core_new(keys.ctypes.data_as(_u8p), stakes.ctypes.data_as(_u32p),
                                   nworkers.ctypes.data_as(_u32p), len(keys), gc_round,
                                   chp if current_header else None, len(current_header or b""), int(use_keyset))
        if not self._h:
            raise NtError("ntn_core_new failed (no gfx950 device, or a bad current header)")

    def ingest(self, data, off, ln, threads=8, general=False, device=False, receipts=False):
        """DagError codes for n packed wire messages; also returns the host decode
        seconds.  general=True: the object-model decoder (cross-check path).
        device=True: Core::ingest_device -- certificates parsed and checked on the
        GPU from the wire bytes (nt_certificates_ingest), the rest on the host;
        the second value is then the count of messages the host decided.
        device="all": Core::ingest_device_all -- headers, votes and requests are
        decided on the GPU too (nt_primary_messages_ingest); only irregular bytes
        are left to the host, counted in the second value.
        receipts=True (with device="all"): Core::ingest_device_receipts -- a third
        value, the RECEIPT_DTYPE record of every message (ntcrypto.h
        nt_msg_receipt); a message the host decided keeps kind 0xff and a zeroed
        record."""
        n = len(off)
        codes = np.zeros(max(n, 1), np.int32)
        dec = ctypes.c_double(0)
        data = np.ascontiguousarray(data, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        ln = np.ascontiguousarray(ln, np.uint64)
        if receipts:
            if device != "all":
                raise ValueError('receipts=True needs device="all"')
            rec = np.zeros(max(n, 1), RECEIPT_DTYPE)
            host = ctypes.c_uint64(0)
            rc = load().ntn_core_ingest_receipts(self._h, data.ctypes.data_as(_u8p), off.ctypes.data_as(_u64p),
                                                 ln.ctypes.data_as(_u64p), n, threads,
                                                 codes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                 rec.ctypes.data_as(ctypes.c_void_p), ctypes.byref(host))
            if rc != 0:
                raise NtError("ntn_core_ingest_receipts: backend failure")
            return codes[:n], int(host.value), rec[:n]
        rc = load().ntn_core_ingest(self._h, data.ctypes.data_as(_u8p), off.ctypes.data_as(_u64p),
                                    ln.ctypes.data_as(_u64p), n, threads,
                                    codes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(dec),
                                    (3 if device == "all" else 2) if device else int(general))
        if rc != 0:
            raise NtError("ntn_core_ingest: backend failure")
        return codes[:n], (int(dec.value) if device else dec.value)

    def set_signer(self, seed):
        """The node's own key (32-byte seed; None removes it): returns the public key."""
        name = np.zeros(32, np.uint8)
        sp = np.frombuffer(bytes(seed), np.uint8) if seed is not None else None
        if sp is not None and len(sp) != 32:
            raise ValueError("seed: 32 bytes")
        rc = load().ntn_core_set_signer(self._h, sp.ctypes.data_as(_u8p) if sp is not None else None,
                                        name.ctypes.data_as(_u8p))
        if rc != 0:
            raise NtError("ntn_core_set_signer: backend failure")
        return name.tobytes() if seed is not None else None

    def votes_for(self, receipts, selected):
        """Core::votes_for: the node's votes for the headers receipts[selected] (records
        of ingest(..., device="all", receipts=True)), signed in one call: an
        (m, 212) uint8 array of PrimaryMessage::Vote wire bytes ready to send."""
        if receipts.dtype != RECEIPT_DTYPE or receipts.ndim != 1 or not receipts.flags.c_contiguous:
            raise ValueError("receipts: a C-contiguous RECEIPT_DTYPE array")
        sel = np.ascontiguousarray(selected, np.uint32).reshape(-1)
        if len(sel) and int(sel.max()) >= len(receipts):
            raise ValueError("selected: indices into receipts")
        out = np.zeros((max(len(sel), 1), 212), np.uint8)
        rc = load().ntn_core_votes_for(self._h, receipts.ctypes.data_as(ctypes.c_void_p), sel.ctypes.data_as(_u32p),
                                       len(sel), out.ctypes.data_as(_u8p))
        if rc == -1:
            raise ValueError("votes_for: a selected receipt is not a header's")
        if rc != 0:
            raise NtError("ntn_core_votes_for: backend failure (no signer set?)")
        return out[:len(sel)]

    def ingest_pipelined(self, data, off, ln, threads=8, chunk=25000):
        """Core::ingest_pipelined: chunks of `chunk` messages, two in flight"""
        n = len(off)
        codes = np.zeros(max(n, 1), np.int32)
        data = np.ascontiguousarray(data, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        ln = np.ascontiguousarray(ln, np.uint64)
        rc = load().ntn_core_ingest_pipelined(self._h, data.ctypes.data_as(_u8p), off.ctypes.data_as(_u64p),
                                              ln.ctypes.data_as(_u64p), n, threads, chunk,
                                              codes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        if rc != 0:
            raise NtError("ntn_core_ingest_pipelined: backend failure")
        return codes[:n]

    @staticmethod
    def last_stats():
        """phase seconds of the last SoA ingest on this thread"""
        a = (ctypes.c_double * 6)()
        load().ntn_last_ingest_stats(a)
        return dict(zip(("decode", "prep", "digest", "verify_strict", "verify_batch", "total"), list(a)))

    def close(self):
        if self._h:
            load().ntn_core_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def set_small_call_path(mode, threads=0):
    """The small-call path of the mirror's shared context (nt_set_small_call_path)."""
    rc = load().ntn_set_small_call_path(int(mode), int(threads))
    if rc != 0:
        raise NtError("ntn_set_small_call_path failed (%d)" % rc)


def worker_decode(msg: bytes):
    """worker::decode_message, the plain host decoder of a bincode WorkerMessage (CPU only):
    None on a bincode error, else a dict -- kind (0 batch, 1 request), n (transactions /
    digests), used (bytes consumed), tx_bytes, requestor (a request's raw key, else None)."""
    a, p = _buf(msg)
    out = (ctypes.c_uint64 * 3)()
    key = np.zeros(32, np.uint8)
    kind = load().ntn_worker_decode(p, len(msg), out, key.ctypes.data_as(_u8p))
    if kind < 0:
        return None
    return {"kind": kind, "n": int(out[0]), "used": int(out[1]), "tx_bytes": int(out[2]),
            "requestor": key.tobytes() if kind == 1 else None}


def worker_ingest(worker_id, messages):
    """worker::ingest_device: the drain of a worker through nt_worker_messages_ingest, the
    messages it leaves to the host through worker::decode_message.  Returns a dict of
    arrays with one row per message -- code (0 / 9), kind (0 batch, 1 request, 0xff),
    message (a batch: the Processor's 40-byte OthersBatch(digest, worker_id)), requestor,
    nd -- plus receipts (WORKER_RECEIPT_DTYPE, as the device wrote them) and host_decided."""
    data, off, ln = pack(messages)
    n = len(messages)
    m = max(n, 1)
    codes, kinds = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    msg40, key32 = np.zeros((m, 40), np.uint8), np.zeros((m, 32), np.uint8)
    nd = np.zeros(m, np.uint32)
    rec = np.zeros(m, WORKER_RECEIPT_DTYPE)
    host = ctypes.c_uint64(0)
    data = data if len(data) else np.zeros(1, np.uint8)
    rc = load().ntn_worker_ingest(int(worker_id), data.ctypes.data_as(_u8p), off.ctypes.data_as(_u64p),
                                  ln.ctypes.data_as(_u64p), n, codes.ctypes.data_as(_u8p), kinds.ctypes.data_as(_u8p),
                                  msg40.ctypes.data_as(_u8p), key32.ctypes.data_as(_u8p), nd.ctypes.data_as(_u32p),
                                  rec.ctypes.data_as(ctypes.c_void_p), ctypes.byref(host))
    if rc != 0:
        raise NtError("ntn_worker_ingest: backend failure")
    return {"code": codes[:n], "kind": kinds[:n], "message": msg40[:n], "requestor": key32[:n], "nd": nd[:n],
            "receipts": rec[:n], "host_decided": int(host.value)}


class DigestBatcher:
    """worker::DigestBatcher (host/narwhal.hpp): both Processor
    tasks of a worker submit serialized batches from their own threads; a
    flusher hashes everything queued in one nt_sha512_trunc32 call when
    max_bytes / max_batches is reached or the oldest batch is max_delay_us old.

    submit() returns a ticket; wait(ticket) -> (digest32 bytes, 40-byte
    WorkerPrimaryMessage).  ctypes releases the GIL in both, so Python threads
    submit and wait concurrently."""

    def __init__(self, max_bytes=256 << 20, max_batches=4096, max_delay_us=1000):
        self._lib = load()
        self._h = self._lib.ntn_batcher_new(max_bytes, max_batches, max_delay_us)
        if not self._h:
            raise NtError("ntn_batcher_new failed")

    def submit(self, worker_id, own, batch):
        a, p = _buf(batch)
        t = self._lib.ntn_batcher_submit(self._h, worker_id, 1 if own else 0, p, len(batch))
        if not t:
            raise NtError("ntn_batcher_submit failed")
        return t

    def wait(self, ticket):
        d = np.zeros(32, np.uint8)
        m = np.zeros(40, np.uint8)
        rc = self._lib.ntn_batcher_wait(ticket, d.ctypes.data_as(_u8p), m.ctypes.data_as(_u8p))
        if rc != 0:
            raise NtError("digest batcher: backend failure")
        return d.tobytes(), m.tobytes()

    def process(self, worker_id, own, batch):
        return self.wait(self.submit(worker_id, own, batch))

    def flush(self):
        self._lib.ntn_batcher_flush(self._h)

    def stats(self):
        out = (ctypes.c_double * 4)()
        self._lib.ntn_batcher_stats(self._h, out)
        return {"flushes": int(out[0]), "batches": int(out[1]), "bytes": int(out[2]), "hash_seconds": out[3]}

    def close(self):
        if self._h:
            self._lib.ntn_batcher_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
