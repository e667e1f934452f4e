"""ctypes binding of libntcrypto.so (include/ntcrypto.h).

The product path: every call goes to the gfx950 HIP kernels through the C ABI.
There is no CPU fallback -- if the library or a gfx950 device is missing the
calls raise NtError.
"""
import ctypes
import os

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("NTCRYPTO_LIB", os.path.join(PKG_ROOT, "lib", "libntcrypto.so"))

NT_MODE_STRICT = 0
NT_MODE_COFACTORLESS = 1
NT_MODE_MIXED = 2             # key-cache only: key_idx bit 31 = strict
NT_KEY_STRICT_BIT = 0x80000000
NT_SMALL_OFF = 0              # small-call path (include/ntcrypto.h): everything on the GPU
NT_SMALL_AUTO = 1             # calls below the host/GPU crossover on host threads
NT_SMALL_ALWAYS = 2           # every host entry point on host threads (tests)

_u8p = ctypes.POINTER(ctypes.c_uint8)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p
_u64 = ctypes.c_uint64

NT_INFO_KTAB = 0x10000

EXPORTED = [
    "nt_init", "nt_init_device", "nt_init_devices", "nt_free", "nt_num_devices", "nt_strerror", "nt_version",
    "nt_sha512_trunc32", "nt_ed25519_verify_strict", "nt_ed25519_verify_batch_groups",
    "nt_ed25519_sign_batch", "nt_ed25519_keypair_batch", "nt_dev_sha512_trunc32",
    "nt_dev_sha512_trunc32_bounded",
    "nt_dev_ed25519_verify", "nt_dev_group_and", "nt_dev_ed25519_sign", "nt_keyset_create",
    "nt_keyset_free", "nt_keyset_flags", "nt_keyset_info", "nt_ed25519_verify_keyset", "nt_ed25519_verify_batch_groups_keyset",
    "nt_dev_ed25519_verify_keyset", "nt_host_alloc", "nt_host_free", "nt_set_small_call_path", "nt_call_counts",
    "nt_committee_create", "nt_committee_free", "nt_certificates_ingest", "nt_small_call_model",
    "nt_set_hbm_budget", "nt_memory_info", "nt_dev_stream", "nt_set_key_cache", "nt_key_cache_add",
    "nt_key_cache_sync", "nt_key_cache_info", "nt_dev_clock_probe", "nt_dev_ed25519_verify_keyset_groups",
    "nt_primary_messages_ingest", "nt_primary_messages_ingest_receipts", "nt_worker_messages_ingest",
]
# the signer bound to one key (include/ntsigner.h): a prefix of its own, same library
SIGNER_EXPORTED = [
    "nts_signer_create", "nts_signer_free", "nts_signer_public", "nts_sign_digests", "nts_votes_sign",
    "nts_dev_votes_sign",
]
VOTE_BYTES = 212              # NTS_VOTE_BYTES: bincode of PrimaryMessage::Vote
# nt_msg_receipt (include/ntcrypto.h): one 128-byte record per ingested message
RECEIPT_DTYPE = np.dtype({
    "names": ["code", "kind", "flags", "author", "origin", "np", "nq", "nv", "round", "off_payload", "off_parents",
              "off_id", "off_sig", "off_votes", "id", "digest", "reserved"],
    "formats": ["u1", "u1", "<u2", "<u4", "<u4", "<u4", "<u4", "<u4", "<u8", "<u4", "<u4", "<u4", "<u4", "<u4",
                ("u1", 32), ("u1", 32), ("u1", 12)],
    "offsets": [0, 1, 2, 4, 8, 12, 16, 20, 24, 32, 36, 40, 44, 48, 52, 84, 116],
    "itemsize": 128,
})
RECEIPT_KIND_HOST = 0xFF
# nt_worker_receipt (include/ntcrypto.h): one 64-byte record per ingested worker message
WORKER_RECEIPT_DTYPE = np.dtype({
    "names": ["code", "kind", "flags", "n", "used", "tx_bytes", "tx_len", "off_key", "digest"],
    "formats": ["u1", "u1", "<u2", "<u4", "<u8", "<u8", "<u4", "<u4", ("u1", 32)],
    "offsets": [0, 1, 2, 4, 8, 16, 24, 28, 32],
    "itemsize": 64,
})
WMSG_OK, WMSG_SERIALIZATION, WMSG_HOST = 0, 9, 0xFF
WORKER_KIND_BATCH, WORKER_KIND_REQUEST, WORKER_KIND_NONE = 0, 1, 0xFF
WORKER_RECEIPT_UNIFORM = 1    # flags bit 0
RECEIPT_GENESIS = 1           # flags bit 0
KEY_CACHE_INFO_KEYS = ("keys", "max_keys", "comb_bits", "bytes_per_device", "hits", "misses", "admitted", "refused",
                       "pending", "error", "alloc_us", "build_us")
MEMORY_INFO_KEYS = ("comb_b_bits", "comb_b_bytes", "key_comb_bytes", "workspace_bytes", "stash_bytes",
                    "staging_bytes", "budget", "held")


class NtError(RuntimeError):
    pass


_lib = None


def load_library(path=None):
    """Load libntcrypto.so and declare prototypes (no GPU needed)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise NtError("libntcrypto.so not built (%s); run `make -C narwhal-tusk_amd`" % p)
    lib = ctypes.CDLL(p)
    lib.nt_init.argtypes = [ctypes.POINTER(_vp), ctypes.c_int]
    lib.nt_init_device.argtypes = [ctypes.POINTER(_vp), ctypes.c_int]
    lib.nt_init_devices.argtypes = [ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.nt_free.argtypes = [_vp]
    lib.nt_free.restype = None
    lib.nt_host_alloc.argtypes = [ctypes.c_uint64]
    lib.nt_host_alloc.restype = _vp
    lib.nt_host_free.argtypes = [_vp]
    lib.nt_host_free.restype = None
    lib.nt_num_devices.argtypes = [_vp]
    lib.nt_strerror.restype = ctypes.c_char_p
    lib.nt_version.restype = ctypes.c_char_p
    lib.nt_sha512_trunc32.argtypes = [_vp, _u8p, _u64p, _u64p, _u64, _u8p]
    lib.nt_ed25519_verify_strict.argtypes = [_vp, _u8p, _u8p, _u8p, _u64p, _u64p, _u64, _u8p]
    lib.nt_ed25519_verify_batch_groups.argtypes = [_vp, _u8p, _u8p, _u64p, _u32p, _u8p, _u64, _u8p, _u8p]
    lib.nt_ed25519_sign_batch.argtypes = [_vp, _u8p, _u8p, _u64p, _u64p, _u64, _u8p, _u8p]
    lib.nt_ed25519_keypair_batch.argtypes = [_vp, _u8p, _u64, _u8p]
    lib.nt_dev_sha512_trunc32.argtypes = [_vp, ctypes.c_int, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]
    lib.nt_dev_sha512_trunc32_bounded.argtypes = [_vp, ctypes.c_int, _vp, _vp, _u64, _vp, _vp, _u64, _u64, _vp, _vp]
    lib.nt_dev_ed25519_verify.argtypes = [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, _vp, _u64, _vp, _vp,
                                          _u64, _vp]
    lib.nt_dev_group_and.argtypes = [_vp, ctypes.c_int, _vp, _vp, _vp, _u64, _vp, _vp]
    lib.nt_dev_ed25519_sign.argtypes = [_vp, ctypes.c_int, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]
    lib.nt_keyset_create.argtypes = [_vp, _u8p, ctypes.c_uint32, ctypes.POINTER(_vp)]
    lib.nt_keyset_free.argtypes = [_vp]
    lib.nt_keyset_free.restype = None
    lib.nt_keyset_flags.argtypes = [_vp, ctypes.c_uint32, _u32p]
    lib.nt_keyset_info.argtypes = [_vp, _u32p, _u64p]
    lib.nt_ed25519_verify_keyset.argtypes = [_vp, _vp, ctypes.c_int, _u32p, _u8p, _u8p, _u64p, _u64p, _u64, _u8p]
    lib.nt_ed25519_verify_batch_groups_keyset.argtypes = [_vp, _vp, _u32p, _u8p, _u64p, _u32p, _u8p, _u64, _u8p,
                                                          _u8p]
    lib.nt_dev_ed25519_verify_keyset.argtypes = [_vp, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, _vp, _u64,
                                                 _vp, _vp, _u64, _vp]
    lib.nt_set_small_call_path.argtypes = [_vp, ctypes.c_int, ctypes.c_int]
    lib.nt_call_counts.argtypes = [_vp, _u64p, _u64p]
    if hasattr(lib, "nt_small_call_model"):  # absent from older A/B builds (NTCRYPTO_LIB)
        lib.nt_small_call_model.argtypes = [_vp, ctypes.POINTER(ctypes.c_double)]
    lib.nt_committee_create.argtypes = [_vp, _vp, _u32p, _u64p, _u32p, ctypes.c_uint32, ctypes.POINTER(_vp)]
    lib.nt_committee_free.argtypes = [_vp]
    lib.nt_committee_free.restype = None
    lib.nt_certificates_ingest.argtypes = [_vp, _vp, _u8p, _u64p, _u64p, _u64, _u64, _u8p]
    if hasattr(lib, "nt_primary_messages_ingest"):  # absent from older A/B builds (NTCRYPTO_LIB)
        lib.nt_primary_messages_ingest.argtypes = [_vp, _vp, _u8p, _u64p, _u64p, _u64, _u64, _u8p, _u64, _u8p, _u8p]
    if hasattr(lib, "nt_primary_messages_ingest_receipts"):  # absent from older A/B builds (NTCRYPTO_LIB)
        lib.nt_primary_messages_ingest_receipts.argtypes = [_vp, _vp, _u8p, _u64p, _u64p, _u64, _u64, _u8p, _u64, _u8p,
                                                            _u8p, _vp]
    if hasattr(lib, "nt_worker_messages_ingest"):  # absent from older A/B builds (NTCRYPTO_LIB)
        lib.nt_worker_messages_ingest.argtypes = [_vp, _u8p, _u64p, _u64p, _u64, _u8p, _vp]
    if hasattr(lib, "nt_memory_info"):  # absent from round-3 A/B builds (NTCRYPTO_LIB)
        lib.nt_set_hbm_budget.argtypes = [_vp, ctypes.c_uint64]
        lib.nt_memory_info.argtypes = [_vp, ctypes.c_int, _u64p]
        lib.nt_dev_stream.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]
    if hasattr(lib, "nt_set_key_cache"):  # absent from round-5 A/B builds (NTCRYPTO_LIB)
        lib.nt_set_key_cache.argtypes = [_vp, ctypes.c_uint32, ctypes.c_uint32]
        lib.nt_key_cache_add.argtypes = [_vp, _u8p, ctypes.c_uint32]
        lib.nt_key_cache_sync.argtypes = [_vp]
        lib.nt_key_cache_info.argtypes = [_vp, _u64p]
        lib.nt_dev_clock_probe.argtypes = [_vp, ctypes.c_int, _vp, ctypes.c_uint32, _vp, _u64p]
        lib.nt_dev_ed25519_verify_keyset_groups.argtypes = [_vp, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, _vp,
                                                            _u64, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]
    if hasattr(lib, "nts_signer_create"):  # absent from older A/B builds (NTCRYPTO_LIB)
        lib.nts_signer_create.argtypes = [_vp, _u8p, ctypes.POINTER(_vp)]
        lib.nts_signer_free.argtypes = [_vp]
        lib.nts_signer_free.restype = None
        lib.nts_signer_public.argtypes = [_vp, _u8p]
        lib.nts_sign_digests.argtypes = [_vp, _vp, _u8p, _u64, _u8p]
        lib.nts_votes_sign.argtypes = [_vp, _vp, _u8p, _u64p, _u8p, _u64, _u8p, _u8p]
        lib.nts_dev_votes_sign.argtypes = [_vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, _u64, _vp, _vp]
    _lib = lib
    return lib


def _p(a, t=_u8p):
    return a.ctypes.data_as(t)


def _u8(a, shape_tail=None):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a


def _check(rc, what):
    if rc != 0:
        raise NtError("%s failed: %s (%d)" % (what, load_library().nt_strerror(rc).decode(), rc))


def _unpack(bm, n):
    return np.unpackbits(bm, bitorder="little")[:n].astype(bool)


def _torch_first():
    """PyTorch-ROCm wheels bundle their own HIP runtime.  Two runtimes in one
    process work when torch's starts first; torch's first HIP init AFTER
    libntcrypto has mapped its tables fails ("PyTorch in the
    same process").  If this process has imported torch, start its runtime now."""
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available() and not torch.cuda.is_initialized():
        torch.cuda.init()


def nbytes(t):
    """Byte size of a device buffer given as a torch tensor (the msg_bytes /
    data_bytes argument of the device-resident entry points)."""
    return int(t.numel()) * int(t.element_size())


class Backend:
    """A context over one or more gfx950 devices (nt_init / nt_init_device)."""

    def __init__(self, num_gpus=0, device=None, devices=None):
        self.lib = load_library()
        _torch_first()
        ctx = _vp()
        if devices is not None:
            arr = (ctypes.c_int * len(devices))(*devices)
            rc = self.lib.nt_init_devices(ctypes.byref(ctx), arr, len(devices))
        elif device is not None:
            rc = self.lib.nt_init_device(ctypes.byref(ctx), int(device))
        else:
            rc = self.lib.nt_init(ctypes.byref(ctx), int(num_gpus))
        _check(rc, "nt_init")
        self.ctx = ctx

    def close(self):
        if self.ctx:
            self.lib.nt_free(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_devices(self):
        return self.lib.nt_num_devices(self.ctx)

    def set_small_call_path(self, mode=NT_SMALL_AUTO, threads=0):
        """Small calls on host threads (include/ntcrypto.h)."""
        _check(self.lib.nt_set_small_call_path(self.ctx, int(mode), int(threads)), "nt_set_small_call_path")

    def pinned(self, shape, dtype=np.uint8):
        """A numpy array in nt_host_alloc memory (pinned, registered with every
        device of the process): inputs placed there are DMA'd by the host entry
        points without the staging copy.  Freed when the array is collected."""
        dt = np.dtype(dtype)
        count = int(np.prod(shape)) if np.ndim(shape) else int(shape)
        nbytes = max(1, count * dt.itemsize)
        p = self.lib.nt_host_alloc(nbytes)
        if not p:
            raise MemoryError("nt_host_alloc(%d)" % nbytes)
        buf = (ctypes.c_uint8 * nbytes).from_address(p)
        arr = np.frombuffer(buf, dtype=np.uint8, count=count * dt.itemsize).view(dt).reshape(shape)
        import weakref
        weakref.finalize(buf, self.lib.nt_host_free, ctypes.c_void_p(p))
        return arr

    def small_call_model(self):
        """The small-call cost model AUTO routes by (nt_small_call_model): the
        host-lane rates and one GPU floor per verify kernel (uncached, key cache)."""
        out = (ctypes.c_double * 10)()
        _check(self.lib.nt_small_call_model(self.ctx, out), "nt_small_call_model")
        keys = ("cpu_verify_us", "gpu_verify_us", "cpu_sha_mbs", "gpu_lane_mbs", "gpu_call_us", "pcie_gbs",
                "spawn_us", "threads", "calibrated", "gpu_keyset_us")
        d = dict(zip(keys, list(out)))
        d["threads"] = int(d["threads"])
        d["calibrated"] = bool(d["calibrated"])
        return d

    def set_hbm_budget(self, nbytes):
        """Cap the tables (comb of B + key combs) this context holds per device
        entry; 0 = no cap (nt_set_hbm_budget)."""
        _check(self.lib.nt_set_hbm_budget(self.ctx, int(nbytes)), "nt_set_hbm_budget")

    def memory_info(self, dev=0):
        """What device entry `dev` of this context holds (nt_memory_info)."""
        out = np.zeros(8, np.uint64)
        _check(self.lib.nt_memory_info(self.ctx, int(dev), _p(out, _u64p)), "nt_memory_info")
        return dict(zip(MEMORY_INFO_KEYS, (int(x) for x in out)))

    def ktab_info(self, dev=0):
        """The verify kernel's key-table cache on device entry `dev` (nt_memory_info with NT_INFO_KTAB; a
        library older than the cache refuses it), once the launches
        of interest have completed: entries used, capacity, bytes, and the wave rows that took the
        short ladder / built entries / ran the balanced path."""
        out = np.zeros(8, np.uint64)
        _check(self.lib.nt_memory_info(self.ctx, int(dev) | NT_INFO_KTAB, _p(out, _u64p)), "nt_memory_info")
        keys = ("used", "capacity", "bytes", "fast_rows", "builds", "old_rows", "index_slots")
        return dict(zip(keys, (int(x) for x in out)))

    def dev_stream(self, dev=0, which=0):
        """Raw hipStream_t of device entry `dev`'s compute stream `which` (0 / 1):
        the streams the host entry points pipeline on (nt_dev_stream)."""
        p = _vp()
        _check(self.lib.nt_dev_stream(self.ctx, int(dev), int(which), ctypes.byref(p)), "nt_dev_stream")
        return int(p.value)

    # ---- the key registry (nt_set_key_cache): the key cache behind the plain entry points ----
    def set_key_cache(self, max_keys, admit_after=1):
        """Enable (max_keys > 0) or disable (0) the context's key registry."""
        _check(self.lib.nt_set_key_cache(self.ctx, int(max_keys), int(admit_after)), "nt_set_key_cache")

    def key_cache_add(self, pks):
        """Admit these 32-byte keys now (waits for their tables)."""
        pks = np.ascontiguousarray(pks, np.uint8).reshape(-1, 32)
        buf = pks if len(pks) else np.zeros((1, 32), np.uint8)
        _check(self.lib.nt_key_cache_add(self.ctx, _p(buf), len(pks)), "nt_key_cache_add")

    def key_cache_sync(self):
        """Wait until queued admissions are published (nt_key_cache_sync)."""
        _check(self.lib.nt_key_cache_sync(self.ctx), "nt_key_cache_sync")

    def key_cache_info(self):
        out = np.zeros(12, np.uint64)
        _check(self.lib.nt_key_cache_info(self.ctx, _p(out, _u64p)), "nt_key_cache_info")
        d = dict(zip(KEY_CACHE_INFO_KEYS, (int(x) for x in out)))
        d["error"] = -d["error"]
        return d

    def dev_clock_probe(self, dev, stream, iters, d_out2):
        """Enqueue the clock probe (nt_dev_clock_probe) on `stream`; returns the
        wall clock's rate in kHz.  d_out2: device uint64[2] (cycles, wall ticks)."""
        khz = np.zeros(1, np.uint64)
        _check(self.lib.nt_dev_clock_probe(self.ctx, int(dev), stream, int(iters), d_out2, _p(khz, _u64p)),
               "nt_dev_clock_probe")
        return int(khz[0])

    def call_counts(self):
        """(host-lane calls, GPU calls) of the host entry points so far."""
        h = np.zeros(1, np.uint64)
        g = np.zeros(1, np.uint64)
        _check(self.lib.nt_call_counts(self.ctx, _p(h, _u64p), _p(g, _u64p)), "nt_call_counts")
        return int(h[0]), int(g[0])

    # ---- SHA-512 ----
    def sha512_trunc32(self, data, off, ln):
        data = _u8(data) if len(data) else np.zeros(1, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        ln = np.ascontiguousarray(ln, np.uint64)
        n = len(off)
        out = np.zeros((max(n, 1), 32), np.uint8)
        _check(self.lib.nt_sha512_trunc32(self.ctx, _p(data), _p(off, _u64p), _p(ln, _u64p), n, _p(out)),
               "nt_sha512_trunc32")
        return out[:n]

    def digest_many(self, messages):
        ln = np.array([len(m) for m in messages], np.uint64)
        off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64) if len(messages) else np.zeros(0, np.uint64)
        data = np.frombuffer(b"".join(messages), np.uint8) if messages else np.zeros(0, np.uint8)
        return self.sha512_trunc32(data, off, ln)

    # ---- the worker's drain ----
    def ingest_worker_messages(self, messages, receipts=True, data=None, off=None, ln=None):
        """The worker's drain on the device (nt_worker_messages_ingest): bincode
        WorkerMessage bytes, batches and requests alike.  Returns the codes
        (WMSG_OK, WMSG_SERIALIZATION, WMSG_HOST = left to the host decoder) and,
        with receipts=True, a WORKER_RECEIPT_DTYPE array: a batch's record carries
        the Processor's digest.  An array passed as `receipts` (n records,
        C-contiguous) is filled in place and returned; receipts=False returns the
        codes alone (nothing is hashed).  messages: a list of byte strings, or
        None with data / off / ln already packed (data may be a Backend.pinned
        array: it is then DMA'd in place)."""
        if messages is not None:
            n = len(messages)
            ln = np.array([len(m) for m in messages], np.uint64)
            off = np.zeros(n, np.uint64)
            if n > 1:
                off[1:] = np.cumsum(ln)[:-1]
            data = np.frombuffer(b"".join(messages), np.uint8) if n else np.zeros(1, np.uint8)
        else:
            off = np.ascontiguousarray(off, np.uint64)
            ln = np.ascontiguousarray(ln, np.uint64)
            n = len(off)
            if len(ln) != n or data.dtype != np.uint8 or not data.flags.c_contiguous:
                raise ValueError("data: C-contiguous uint8; off and ln: one entry per message")
            size = np.uint64(len(data))          # compared before anything is added: uint64 sums wrap
            if n and (bool((off > size).any()) or bool((ln > size - np.minimum(off, size)).any())):
                raise ValueError("a message reaches past the end of data")
        data = data if len(data) else np.zeros(1, np.uint8)
        out = np.zeros(max(n, 1), np.uint8)
        if receipts is False or receipts is None:
            rec = None
        elif receipts is True:
            rec = np.zeros(max(n, 1), WORKER_RECEIPT_DTYPE)
        else:
            rec = receipts
            if rec.dtype != WORKER_RECEIPT_DTYPE or rec.ndim != 1 or len(rec) != n or not rec.flags.c_contiguous:
                raise ValueError("receipts: a C-contiguous WORKER_RECEIPT_DTYPE array of one record per message")
        _check(self.lib.nt_worker_messages_ingest(self.ctx, _p(data), _p(off, _u64p), _p(ln, _u64p), n, _p(out),
                                                  rec.ctypes.data_as(_vp) if rec is not None and n else None),
               "nt_worker_messages_ingest")
        return out[:n] if rec is None else (out[:n], rec[:n])

    # ---- Ed25519 ----
    def verify_strict(self, pk, sig, msg, off, ln):
        pk = _u8(pk).reshape(-1, 32)
        sig = _u8(sig).reshape(-1, 64)
        n = len(pk)
        msg = _u8(msg) if len(msg) else np.zeros(1, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        ln = np.ascontiguousarray(ln, np.uint64)
        bm = np.zeros((n + 7) // 8 + 1, np.uint8)
        _check(self.lib.nt_ed25519_verify_strict(self.ctx, _p(pk), _p(sig), _p(msg), _p(off, _u64p),
                                                  _p(ln, _u64p), n, _p(bm)), "nt_ed25519_verify_strict")
        return _unpack(bm, n)

    def verify_batch_groups(self, pk, sig, first, cnt, msg32, with_sig_bits=False):
        pk = _u8(pk).reshape(-1, 32)
        sig = _u8(sig).reshape(-1, 64)
        if len(pk) == 0:
            pk = np.zeros((1, 32), np.uint8)
            sig = np.zeros((1, 64), np.uint8)
        first = np.ascontiguousarray(first, np.uint64)
        cnt = np.ascontiguousarray(cnt, np.uint32)
        msg32 = _u8(msg32).reshape(-1, 32)
        G = len(cnt)
        nsig = int((first + cnt).max()) if G else 0
        gb = np.zeros((G + 7) // 8 + 1, np.uint8)
        sb = np.zeros((nsig + 7) // 8 + 1, np.uint8)
        _check(self.lib.nt_ed25519_verify_batch_groups(
            self.ctx, _p(pk), _p(sig), _p(first, _u64p), _p(cnt, _u32p), _p(msg32), G, _p(gb),
            _p(sb) if with_sig_bits else None), "nt_ed25519_verify_batch_groups")
        if with_sig_bits:
            return _unpack(gb, G), _unpack(sb, nsig)
        return _unpack(gb, G)

    def sign_batch(self, seeds, msg=None, off=None, ln=None):
        seeds = _u8(seeds).reshape(-1, 32)
        n = len(seeds)
        pk = np.zeros((max(n, 1), 32), np.uint8)
        if msg is None:
            _check(self.lib.nt_ed25519_keypair_batch(self.ctx, _p(seeds), n, _p(pk)), "nt_ed25519_keypair_batch")
            return pk[:n]
        msg = _u8(msg) if len(msg) else np.zeros(1, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        ln = np.ascontiguousarray(ln, np.uint64)
        sig = np.zeros((max(n, 1), 64), np.uint8)
        _check(self.lib.nt_ed25519_sign_batch(self.ctx, _p(seeds), _p(msg), _p(off, _u64p), _p(ln, _u64p), n,
                                              _p(pk), _p(sig)), "nt_ed25519_sign_batch")
        return pk[:n], sig[:n]

    # ---- committee key cache ----
    def keyset(self, pks):
        return Keyset(self, pks)

    # ---- the node's own key ----
    def signer(self, seed):
        return Signer(self, seed)

    # ---- device-resident (raw device pointers; stream 0 = HIP's NULL stream) ----
    # Message buffers come with their byte size, as in the C ABI: an item whose
    # slice d_msg[off, off + len) lies outside [0, msg_bytes) is never read.
    def dev_verify(self, dev, stream, mode, d_pk, d_sig, d_msg, msg_bytes, d_off, d_len, n, d_out):
        _check(self.lib.nt_dev_ed25519_verify(self.ctx, dev, stream, mode, d_pk, d_sig, d_msg, int(msg_bytes), d_off,
                                              d_len, n, d_out), "nt_dev_ed25519_verify")

    def dev_sha512(self, dev, stream, d_data, data_bytes, d_off, d_len, n, d_out, max_len=None, d_bad=None):
        """max_len: an upper bound of the message lengths, if known (selects the
        kernel: nt_dev_sha512_trunc32_bounded); d_bad: device uint32 counter of
        out-of-bounds items (zero digests), or None"""
        if max_len is None:
            _check(self.lib.nt_dev_sha512_trunc32(self.ctx, dev, stream, d_data, int(data_bytes), d_off, d_len, n,
                                                  d_bad, d_out), "nt_dev_sha512_trunc32")
        else:
            _check(self.lib.nt_dev_sha512_trunc32_bounded(self.ctx, dev, stream, d_data, int(data_bytes), d_off, d_len,
                                                          n, int(max_len), d_bad, d_out),
                   "nt_dev_sha512_trunc32_bounded")

    def dev_sign(self, dev, stream, d_seed, d_msg, msg_bytes, d_off, d_len, n, d_pk, d_sig):
        _check(self.lib.nt_dev_ed25519_sign(self.ctx, dev, stream, d_seed, d_msg, int(msg_bytes), d_off, d_len, n,
                                            d_pk, d_sig), "nt_dev_ed25519_sign")

    def dev_group_and(self, dev, stream, d_first, d_cnt, G, d_sig_words, d_group_words):
        _check(self.lib.nt_dev_group_and(self.ctx, dev, stream, d_first, d_cnt, G, d_sig_words, d_group_words),
               "nt_dev_group_and")


class Keyset:
    """Per-key comb tables of a static committee on every device (nt_keyset_*)."""

    def __init__(self, backend, pks):
        self.be = backend
        pks = np.ascontiguousarray(pks, np.uint8).reshape(-1, 32)
        self.nkeys = len(pks)
        h = _vp()
        buf = pks if len(pks) else np.zeros((1, 32), np.uint8)
        _check(backend.lib.nt_keyset_create(backend.ctx, _p(buf), self.nkeys, ctypes.byref(h)), "nt_keyset_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.be.lib.nt_keyset_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def flags(self, i):
        f = ctypes.c_uint32()
        _check(self.be.lib.nt_keyset_flags(self.h, i, ctypes.byref(f)), "nt_keyset_flags")
        return int(f.value)

    def info(self):
        """(comb digit width, device bytes per device) -- nt_keyset_info"""
        b, nb = ctypes.c_uint32(), ctypes.c_uint64()
        _check(self.be.lib.nt_keyset_info(self.h, ctypes.byref(b), ctypes.byref(nb)), "nt_keyset_info")
        return int(b.value), int(nb.value)

    def verify(self, mode, key_idx, sig, msg, off, ln):
        key_idx = np.ascontiguousarray(key_idx, np.uint32)
        sig = _u8(sig).reshape(-1, 64)
        n = len(key_idx)
        msg = _u8(msg) if len(msg) else np.zeros(1, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        ln = np.ascontiguousarray(ln, np.uint64)
        bm = np.zeros((n + 7) // 8 + 1, np.uint8)
        _check(self.be.lib.nt_ed25519_verify_keyset(self.be.ctx, self.h, mode, _p(key_idx, _u32p), _p(sig), _p(msg),
                                                    _p(off, _u64p), _p(ln, _u64p), n, _p(bm)),
               "nt_ed25519_verify_keyset")
        return _unpack(bm, n)

    def verify_batch_groups(self, key_idx, sig, first, cnt, msg32, with_sig_bits=False):
        key_idx = np.ascontiguousarray(key_idx, np.uint32)
        sig = _u8(sig).reshape(-1, 64)
        if len(key_idx) == 0:
            key_idx = np.zeros(1, np.uint32)
            sig = np.zeros((1, 64), np.uint8)
        first = np.ascontiguousarray(first, np.uint64)
        cnt = np.ascontiguousarray(cnt, np.uint32)
        msg32 = _u8(msg32).reshape(-1, 32)
        G = len(cnt)
        nsig = int((first + cnt).max()) if G else 0
        gb = np.zeros((G + 7) // 8 + 1, np.uint8)
        sb = np.zeros((nsig + 7) // 8 + 1, np.uint8)
        _check(self.be.lib.nt_ed25519_verify_batch_groups_keyset(
            self.be.ctx, self.h, _p(key_idx, _u32p), _p(sig), _p(first, _u64p), _p(cnt, _u32p), _p(msg32), G,
            _p(gb), _p(sb) if with_sig_bits else None), "nt_ed25519_verify_batch_groups_keyset")
        if with_sig_bits:
            return _unpack(gb, G), _unpack(sb, nsig)
        return _unpack(gb, G)

    def dev_verify_groups(self, dev, stream, mode, d_key_idx, d_sig, d_msg, msg_bytes, d_off, d_len, n, d_first,
                          d_cnt, G, d_out, d_group_out):
        """Key-cache verification + the AND per certificate group in one launch chain
        (nt_dev_ed25519_verify_keyset_groups): no verdict-pack / group-AND launch after it."""
        _check(self.be.lib.nt_dev_ed25519_verify_keyset_groups(self.be.ctx, self.h, dev, stream, mode, d_key_idx, d_sig,
                                                               d_msg, int(msg_bytes), d_off, d_len, n, d_first, d_cnt,
                                                               int(G), d_out, d_group_out),
               "nt_dev_ed25519_verify_keyset_groups")

    def dev_verify(self, dev, stream, mode, d_key_idx, d_sig, d_msg, msg_bytes, d_off, d_len, n, d_out):
        _check(self.be.lib.nt_dev_ed25519_verify_keyset(self.be.ctx, self.h, dev, stream, mode, d_key_idx, d_sig,
                                                        d_msg, int(msg_bytes), d_off, d_len, n, d_out),
               "nt_dev_ed25519_verify_keyset")


class Signer:
    """A signer bound to one key (nts_signer_*, include/ntsigner.h): the node's own
    votes and header signatures without a key expansion or [a]B per call.  Not
    constant time.  Close it before its Backend."""

    def __init__(self, backend, seed):
        self.be = backend
        seed = np.frombuffer(bytes(seed), np.uint8)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        h = _vp()
        _check(backend.lib.nts_signer_create(backend.ctx, _p(seed), ctypes.byref(h)), "nts_signer_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.be.lib.nts_signer_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def public(self):
        pk = np.zeros(32, np.uint8)
        _check(self.be.lib.nts_signer_public(self.h, _p(pk)), "nts_signer_public")
        return pk.tobytes()

    def sign_digests(self, digests):
        """64-byte signatures of n 32-byte digests (SignatureService::request_signature)."""
        digests = _u8(digests).reshape(-1, 32)
        n = len(digests)
        sig = np.zeros((max(n, 1), 64), np.uint8)
        _check(self.be.lib.nts_sign_digests(self.be.ctx, self.h, _p(digests) if n else None, n, _p(sig)),
               "nts_sign_digests")
        return sig[:n]

    def votes(self, ids, rounds, origins, with_digests=False, out=None):
        """The wire bytes of PrimaryMessage::Vote for headers (ids[i], rounds[i]) of
        authors origins[i] (raw 32-byte keys): an (n, 212) uint8 array, and with
        with_digests the (n, 32) Vote digests that were signed.  out: an (n, 212)
        C-contiguous uint8 array (pageable or Backend.pinned) to fill instead."""
        ids = _u8(ids).reshape(-1, 32)
        origins = _u8(origins).reshape(-1, 32)
        rounds = np.ascontiguousarray(rounds, np.uint64).reshape(-1)
        n = len(ids)
        if len(origins) != n or len(rounds) != n:
            raise ValueError("ids, rounds and origins: one entry per vote")
        if out is None:
            out = np.zeros((max(n, 1), VOTE_BYTES), np.uint8)[:n]
        elif out.dtype != np.uint8 or out.shape != (n, VOTE_BYTES) or not out.flags.c_contiguous:
            raise ValueError("out: a C-contiguous (n, 212) uint8 array")
        dg = np.zeros((max(n, 1), 32), np.uint8) if with_digests else None
        _check(self.be.lib.nts_votes_sign(self.be.ctx, self.h, _p(ids) if n else None, _p(rounds, _u64p) if n else None,
                                          _p(origins) if n else None, n, _p(out) if n else None,
                                          _p(dg) if dg is not None else None), "nts_votes_sign")
        return (out, dg[:n]) if with_digests else out

    def dev_votes(self, dev, stream, d_ids, d_rounds, d_origins, n, d_votes, d_digests=None):
        """Enqueue the same over device buffers (raw pointers) on `stream` (nts_dev_votes_sign)."""
        _check(self.be.lib.nts_dev_votes_sign(self.be.ctx, self.h, int(dev), stream, d_ids, d_rounds, d_origins, int(n),
                                              d_votes, d_digests), "nts_dev_votes_sign")


_default = None


def default_backend():
    """Process-wide backend over all visible devices (created on first use)."""
    global _default
    if _default is None:
        _default = Backend(0)
    return _default


class Committee:
    """A committee over a keyset (nt_committee_*): stake and worker ids per key,
    the quorum threshold; ingest() runs Certificate::verify on wire bytes on the
    device (nt_certificates_ingest), ingest_messages() Core's checks of every kind
    of PrimaryMessage (nt_primary_messages_ingest).  It keeps the keyset's device tables alive:
    the Keyset may be closed first."""

    def __init__(self, keyset, stakes, workers, quorum):
        self.be = keyset.be
        stakes = np.ascontiguousarray(stakes, np.uint32)
        wfirst = np.zeros(len(workers) + 1, np.uint64)
        wfirst[1:] = np.cumsum([len(w) for w in workers])
        wids = np.ascontiguousarray(np.concatenate([np.asarray(w, np.uint32) for w in workers] + [np.zeros(1, np.uint32)]),
                                    np.uint32)
        h = _vp()
        _check(self.be.lib.nt_committee_create(self.be.ctx, keyset.h, _p(stakes, _u32p), _p(wfirst, _u64p),
                                               _p(wids, _u32p), int(quorum), ctypes.byref(h)), "nt_committee_create")
        self.h = h

    @staticmethod
    def _packed(messages):
        n = len(messages)
        ln = np.array([len(m) for m in messages], np.uint64)
        off = np.zeros(n, np.uint64)
        if n > 1:
            off[1:] = np.cumsum(ln)[:-1]
        data = np.frombuffer(b"".join(messages), np.uint8) if n else np.zeros(1, np.uint8)
        data = data if len(data) else np.zeros(1, np.uint8)
        return data, off, ln, np.zeros(max(n, 1), np.uint8)

    def ingest(self, messages, gc_round=0):
        """primary::DagError code per wire message (NT_DAG_HOST = 0xff: left to the host decoder)."""
        n = len(messages)
        data, off, ln, out = self._packed(messages)
        _check(self.be.lib.nt_certificates_ingest(self.be.ctx, self.h, _p(data), _p(off, _u64p), _p(ln, _u64p), n,
                                                  int(gc_round), _p(out)), "nt_certificates_ingest")
        return out[:n]

    def ingest_messages(self, messages, gc_round=0, cur_id=None, cur_round=0, cur_author=None, receipts=False):
        """The whole drain on the device (nt_primary_messages_ingest): headers, votes,
        certificates and requests.  cur_id / cur_round / cur_author: the header being
        voted on (32-byte id, round, the author's raw 32-byte key; None = zero bytes).
        Returns the raw codes, NT_DAG_HOST (0xff) included.  receipts=True
        (nt_primary_messages_ingest_receipts): (codes, receipts), the second a
        RECEIPT_DTYPE array with one record per message; an array passed as
        `receipts` (n records, C-contiguous) is filled in place and returned."""
        n = len(messages)
        data, off, ln, out = self._packed(messages)
        cid = np.frombuffer(bytes(cur_id), np.uint8) if cur_id is not None else None
        cau = np.frombuffer(bytes(cur_author), np.uint8) if cur_author is not None else None
        if (cid is not None and len(cid) != 32) or (cau is not None and len(cau) != 32):
            raise ValueError("cur_id and cur_author are 32 bytes each")
        args = (self.be.ctx, self.h, _p(data), _p(off, _u64p), _p(ln, _u64p), n, int(gc_round),
                _p(cid) if cid is not None else None, int(cur_round), _p(cau) if cau is not None else None, _p(out))
        if receipts is False or receipts is None:
            _check(self.be.lib.nt_primary_messages_ingest(*args), "nt_primary_messages_ingest")
            return out[:n]
        if receipts is True:
            rec = np.zeros(max(n, 1), RECEIPT_DTYPE)
        else:
            rec = receipts
            if rec.dtype != RECEIPT_DTYPE or rec.ndim != 1 or len(rec) != n or not rec.flags.c_contiguous:
                raise ValueError("receipts: a C-contiguous RECEIPT_DTYPE array of one record per message")
        _check(self.be.lib.nt_primary_messages_ingest_receipts(*args, rec.ctypes.data_as(_vp) if n else None),
               "nt_primary_messages_ingest_receipts")
        return out[:n], rec[:n]

    def close(self):
        if getattr(self, "h", None):
            self.be.lib.nt_committee_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
