#!/usr/bin/env python3
"""Wire-to-receipt rate of a worker's drain: nt_worker_messages_ingest (every
message validated, measured and, if a batch, digested on the GPU) against what
a caller needs today for the same bytes -- nt_sha512_trunc32, which validates
nothing, plus worker::decode_message over every message on host threads.

Workload: --batches copies of one sealed batch (--tx-bytes per transaction,
as many transactions as fit in 508,052 wire bytes: 977 of 512, 20,321 of 17),
each with its index in its first transaction so no two digests are equal, back
to back in one pinned buffer.  The calls alternate inside one process; one JSON
line comes out.  With NTCRYPTO_LIB naming another build of libntcrypto.so that
lacks the call, only the digest call is timed: run the two builds in processes
of their own, alternating, for an A/B of the digest-only baseline.

    python tools/ingest_worker_rate.py [--batches 4096] [--tx-bytes 512] [--reps 7] [--threads 16]
"""
import argparse
import ctypes
import hashlib
import json
import os
import struct
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "narwhal-tusk_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)
import ntcrypto  # noqa: E402
from ntcrypto import narwhal as N  # noqa: E402

SEALED = 508052      # the wire bytes of a batch sealed at 500,000 bytes of 512-byte transactions


def one_batch(tx_bytes):
    ntx = (SEALED - 12) // (8 + tx_bytes)
    rng = np.random.default_rng(tx_bytes)
    body = np.zeros((ntx, 8 + tx_bytes), np.uint8)
    body[:, :8] = np.frombuffer(struct.pack("<Q", tx_bytes), np.uint8)
    body[:, 8:] = rng.integers(0, 256, (ntx, tx_bytes), dtype=np.uint8)
    return ntx, struct.pack("<IQ", 0, ntx) + body.tobytes()


def stats(ts, nbytes):
    ts = sorted(ts)
    med = float(np.median(ts))
    return {"ms_per_call": [round(t * 1e3, 3) for t in ts], "median_ms": round(med * 1e3, 3),
            "best_ms": round(ts[0] * 1e3, 3), "spread_ms": round((ts[-1] - ts[0]) * 1e3, 3),
            "gb_per_s": round(nbytes / med / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4096)
    ap.add_argument("--tx-bytes", type=int, default=512, help="bytes per transaction (at least 8)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16, help="host decoder threads")
    ap.add_argument("--no-decode", action="store_true", help="skip the host decoder's timing")
    args = ap.parse_args()
    assert args.tx_bytes >= 8
    be = ntcrypto.Backend(device=0)
    try:
        has_call = hasattr(be.lib, "nt_worker_messages_ingest")
        t0 = time.perf_counter()
        ntx, one = one_batch(args.tx_bytes)
        n, L = args.batches, len(one)
        data = be.pinned((n * L,))
        rows = data.reshape(n, L)
        rows[...] = np.frombuffer(one, np.uint8)
        rows[:, 20:28] = np.arange(n, dtype="<u8").view(np.uint8).reshape(n, 8)      # the nonce
        off = np.arange(n, dtype=np.uint64) * np.uint64(L)
        ln = np.full(n, L, np.uint64)
        gen_s = time.perf_counter() - t0
        u8, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
        dig = np.zeros((n, 32), np.uint8)
        codes = np.full(n, 0xEE, np.uint8)
        rec = np.zeros(n, ntcrypto.WORKER_RECEIPT_DTYPE) if has_call else None
        common = (be.ctx, data.ctypes.data_as(u8), off.ctypes.data_as(u64), ln.ctypes.data_as(u64), n)
        calls = {"digest_only": lambda: be.lib.nt_sha512_trunc32(*common, dig.ctypes.data_as(u8))}
        if has_call:
            calls["ingest"] = lambda: be.lib.nt_worker_messages_ingest(*common, codes.ctypes.data_as(u8),
                                                                       rec.ctypes.data_as(ctypes.c_void_p))
        res = {k: [] for k in calls}
        for k, f in calls.items():                    # warm-up: buffers, staging
            assert f() == 0, k
        for _ in range(args.reps):
            for k, f in calls.items():                # alternating
                t0 = time.perf_counter()
                rc = f()
                res[k].append(time.perf_counter() - t0)
                assert rc == 0, (k, rc)
        picks = sorted({0, 1, n // 2, n - 1})
        for i in picks:
            want = hashlib.sha512(rows[i].tobytes()).digest()[:32]
            assert dig[i].tobytes() == want, i
            if has_call:
                r = rec[i]
                assert (codes[i], r["kind"], r["n"], r["flags"], r["tx_len"], r["used"]) == (0, 0, ntx, 1, args.tx_bytes,
                                                                                             L), (i, r)
                assert bytes(r["digest"]) == want, i
        if has_call:
            assert not codes.any() and (rec["digest"] == dig).all() and len({bytes(d) for d in dig}) == n
        decode = None
        if has_call and not args.no_decode:           # the plain host decoder over every message, on host threads
            def work(t):
                ok = 0
                for i in range(t, n, args.threads):
                    ok += N.worker_decode(rows[i]) is not None
                return ok
            ts = []
            with ThreadPoolExecutor(args.threads) as pool:
                for _ in range(3):
                    t0 = time.perf_counter()
                    assert sum(pool.map(work, range(args.threads))) == n
                    ts.append(time.perf_counter() - t0)
            decode = stats(ts, n * L)
    finally:
        be.close()
    out = {"batches": n, "transactions": ntx, "tx_bytes": args.tx_bytes, "wire_bytes": n * L, "reps": args.reps,
           "library": "NTCRYPTO_LIB" if "NTCRYPTO_LIB" in os.environ else "this tree", "generate_s": round(gen_s, 1)}
    for k, v in res.items():
        out[k] = stats(v, n * L)
    if "ingest" in res:
        out["ingest_vs_digest_only"] = round(out["ingest"]["median_ms"] / out["digest_only"]["median_ms"], 4)
    if decode:
        out["host_decode"] = dict(decode, threads=args.threads)
        both = out["digest_only"]["median_ms"] + decode["median_ms"]
        out["digest_plus_decode_ms"] = round(both, 3)
        out["ingest_speedup_over_digest_plus_decode"] = round(both / out["ingest"]["median_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
