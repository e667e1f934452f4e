#!/usr/bin/env python3
"""Wire-to-verdict rate of a primary's whole drain: Core.ingest(device="all")
(nt_primary_messages_ingest: headers, votes and certificates decided on the
GPU) against Core.ingest(device=True) (nt_certificates_ingest: certificates on
the GPU, headers and votes bounced to the host decoder and three more calls)
on the same bytes.

Workload: an n = 100 committee; one steady-state round is 99 headers and 99
certificates of config 3's shape (32 payload digests, 67 parents, 67 votes)
and 67 votes on the header currently being voted on; --rounds distinct rounds
are built and repeated to about --messages messages, in a pinned input
buffer.  Every message is valid, so every code must be Ok.  The two paths
alternate inside one process; one JSON line comes out.

--receipts adds a third path to the alternation: Core.ingest(device="all",
receipts=True) (nt_primary_messages_ingest_receipts: the same codes plus a
128-byte receipt per message), checks every receipt's id and digest against
the message it names, and reports its ratio to "all" and what it replaces --
"all" plus the host decoder's time over the same bytes (Core.last_stats()
["decode"] of Core.ingest, the host SoA path, once).

--abi times the C entry points themselves instead, with no Core around them:
nt_primary_messages_ingest and (where the library has it)
nt_primary_messages_ingest_receipts alternating on the same pinned bytes, into
output buffers allocated and touched once.  With NTCRYPTO_LIB naming another
build of libntcrypto.so this is the A/B of the plain call between two builds.

    python tools/ingest_mixed_rate.py [--messages 100000] [--reps 3] [--receipts | --abi]
"""
import argparse
import base64
import ctypes
import hashlib
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "narwhal-tusk_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _wire as W  # noqa: E402
import ntcrypto  # noqa: E402
from ntcrypto import narwhal as N  # noqa: E402


def build_rounds(be, nk, rounds, rng):
    """wire messages of `rounds` rounds, the current header, the committee keys"""
    quorum = 2 * nk // 3 + 1
    seeds = np.stack([np.frombuffer(hashlib.sha512(b"nt-mixed-key" + struct.pack("<Q", i)).digest()[:32], np.uint8)
                      for i in range(nk)])
    pks = be.sign_batch(seeds)
    keys = [p.tobytes() for p in pks]

    def rb(n):
        return rng.bytes(n)

    def header(a, rnd):
        return W.Header(keys[a], rnd, {rb(32): 0 for _ in range(32)}, {rb(32) for _ in range(quorum)})

    cur = header(0, 1000)
    objs, tasks = [], [(0, cur.id)]          # tasks: (key index, 32-byte message) in signing order
    for r in range(rounds):
        for a in range(1, nk):
            h = header(a, 1000 + r)
            tasks.append((a, h.id))
            objs.append(h)
            c = W.Certificate(header(a, 999 + r), [])
            tasks.append((a, c.header.id))
            voters = rng.permutation(nk)[:quorum]
            d = c.digest()
            c.votes = [(int(v), None) for v in voters]
            tasks += [(int(v), d) for v in voters]
            objs.append(c)
        for v in rng.permutation(nk)[:quorum]:
            vote = W.Vote(cur.id, cur.round, cur.author, keys[int(v)])
            tasks.append((int(v), vote.digest()))
            objs.append(vote)
    msg = np.frombuffer(b"".join(m for _, m in tasks), np.uint8)
    _, sig = be.sign_batch(seeds[[k for k, _ in tasks]], msg, np.arange(len(tasks), dtype=np.uint64) * 32,
                           np.full(len(tasks), 32, np.uint64))
    cur.sig = sig[0].tobytes()
    t = 1
    for o in objs:
        if isinstance(o, W.Certificate):
            o.header.sig = sig[t].tobytes()
            o.votes = [(keys[v], sig[t + 1 + j].tobytes()) for j, (v, _) in enumerate(o.votes)]
            t += 1 + len(o.votes)
        else:
            o.sig = sig[t].tobytes()
            t += 1
    assert t == len(tasks)
    order = rng.permutation(len(objs))        # a drained channel interleaves the kinds
    return [W.message(objs[i]) for i in order], cur, pks


def check_receipts(rec, wires, times, off):
    """every receipt against the message it names: kind, the id at off_id, the digest hashlib gives"""
    per = len(wires)
    assert len(rec) == per * times and rec.dtype.itemsize == 128
    for i, w in enumerate(wires):
        r = rec[i]
        assert r["code"] == 0 and r["kind"] == w[0] and r["flags"] == 0, (i, r)
        o = int(r["off_id"])
        assert bytes(r["id"]) == w[o:o + 32], i
        if r["kind"] == 0:
            want = bytes(r["id"])                          # a valid header's id is its digest
        else:
            origin = w[52:96] if r["kind"] == 1 else w[12:56]
            want = hashlib.sha512(bytes(r["id"]) + struct.pack("<Q", int(r["round"])) +
                                  base64.b64decode(origin)).digest()[:32]
        assert bytes(r["digest"]) == want, i
    for t in range(1, times):                              # the repeats of the drain: the same records
        assert rec[t * per:(t + 1) * per].tobytes() == rec[:per].tobytes(), t


def abi_times(be, pks, cur, data, off, ln, reps, wires, times):
    """ms per call of the C entry points, alternating, after one warm-up call each"""
    u8, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    nk, n = len(pks), len(off)
    ks = be.keyset(np.ascontiguousarray(pks).reshape(-1))
    cm = ntcrypto.Committee(ks, np.ones(nk, np.uint32), [[0]] * nk, 2 * nk // 3 + 1)
    try:
        codes = np.full(n, 0xEE, np.uint8)
        cid, cau = np.frombuffer(cur.id, np.uint8), np.frombuffer(cur.author, np.uint8)
        common = (be.ctx, cm.h, data.ctypes.data_as(u8), off.ctypes.data_as(u64), ln.ctypes.data_as(u64), n, 0,
                  cid.ctypes.data_as(u8), int(cur.round), cau.ctypes.data_as(u8), codes.ctypes.data_as(u8))
        calls = {"all": lambda: be.lib.nt_primary_messages_ingest(*common)}
        rec = None
        if hasattr(be.lib, "nt_primary_messages_ingest_receipts"):
            rec = np.zeros(n, ntcrypto.RECEIPT_DTYPE)
            rec.view(np.uint8)[...] = 0xEE                 # touched once: no page faults inside the timed calls
            recp = rec.ctypes.data_as(ctypes.c_void_p)
            calls["receipts"] = lambda: be.lib.nt_primary_messages_ingest_receipts(*common, recp)
        res = {k: [] for k in calls}
        for k, f in calls.items():
            assert f() == 0, k
        for _ in range(reps):
            for k, f in calls.items():
                codes[...] = 0xEE
                t0 = time.perf_counter()
                rc = f()
                res[k].append(time.perf_counter() - t0)
                assert rc == 0 and not codes.any(), (k, rc)
        if rec is not None:
            check_receipts(rec, wires, times, off)
    finally:
        cm.close()
        ks.close()
    out = {k: {"ms_per_call": [round(t * 1e3, 3) for t in v], "best_ms": round(min(v) * 1e3, 3),
               "median_ms": round(float(np.median(v)) * 1e3, 3), "messages_per_s": round(n / min(v), 1)}
           for k, v in res.items()}
    if "receipts" in res:
        out["receipts_vs_all"] = {"best": round(min(res["all"]) / min(res["receipts"]), 4),
                                  "median": round(float(np.median(res["all"]) / np.median(res["receipts"])), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=4, help="distinct rounds built before repeating")
    ap.add_argument("--committee", type=int, default=100)
    ap.add_argument("--threads", type=int, default=16, help="host decoder threads")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--receipts", action="store_true", help="also time the receipts call (see above)")
    ap.add_argument("--abi", action="store_true", help="time the C entry points alone (see above)")
    args = ap.parse_args()
    rng = np.random.default_rng(20240611)
    be = ntcrypto.Backend(device=0)
    try:
        t0 = time.perf_counter()
        wires, cur, pks = build_rounds(be, args.committee, args.rounds, rng)
        per = len(wires)
        times = max(1, round(args.messages / per))
        n = per * times
        blob = b"".join(wires)
        ln = np.tile(np.array([len(w) for w in wires], np.uint64), times)
        off = np.zeros(n, np.uint64)
        off[1:] = np.cumsum(ln)[:-1]
        data = be.pinned((len(blob) * times,))
        data.reshape(times, len(blob))[...] = np.frombuffer(blob, np.uint8)
        gen_s = time.perf_counter() - t0
        if args.abi:
            out = {"messages": n, "wire_bytes": int(len(blob) * times),
                   "library": "NTCRYPTO_LIB" if "NTCRYPTO_LIB" in os.environ else "this tree",
                   "ingest_chunk": os.environ.get("NT_INGEST_CHUNK", "6250"), "generate_s": round(gen_s, 1)}
            out.update(abi_times(be, pks, cur, data, off, ln, args.reps, wires, times))
            print(json.dumps(out))
            return
        core = N.Core(pks, np.ones(args.committee, np.uint32), np.ones(args.committee, np.uint32), 0,
                      W.message(cur), True)
        try:
            res = {"all": [], "certificates_only": []}
            host = {}
            bad = {}
            modes = (("all", "all"), ("certificates_only", True))
            if args.receipts:
                res["receipts"] = []
                modes = (("all", "all"), ("receipts", "all"), ("certificates_only", True))
            rec = None
            for name, dev in modes:                       # warm-up: committee tables, buffers, staging
                core.ingest(data, off, ln, args.threads, device=dev, receipts=name == "receipts")
            for _ in range(args.reps):
                for name, dev in modes:                   # alternating
                    t0 = time.perf_counter()
                    if name == "receipts":
                        got, h, rec = core.ingest(data, off, ln, args.threads, device=dev, receipts=True)
                    else:
                        got, h = core.ingest(data, off, ln, args.threads, device=dev)
                    res[name].append(time.perf_counter() - t0)
                    host[name] = int(h)
                    bad[name] = int((got != 0).sum())
            decode_s = None
            if args.receipts:
                check_receipts(rec, wires, times, off)
                got, _ = core.ingest(data, off, ln, args.threads)          # the host SoA path: its decoder's time
                decode_s = N.Core.last_stats()["decode"]
                bad["host_soa"] = int((got != 0).sum())
        finally:
            core.close()
    finally:
        be.close()
    kinds = {"headers": sum(w[0] == 0 for w in wires) * times, "votes": sum(w[0] == 1 for w in wires) * times,
             "certificates": sum(w[0] == 2 for w in wires) * times}
    out = {"messages": n, "kinds": kinds, "wire_bytes": int(len(blob) * times), "committee": args.committee,
           "host_threads": args.threads, "ingest_chunk": os.environ.get("NT_INGEST_CHUNK", "6250"),
           "generate_s": round(gen_s, 1)}
    for name in res:
        best = min(res[name])
        out[name] = {"messages_per_s": round(n / best, 1), "ms_per_call": [round(t * 1e3, 2) for t in res[name]],
                     "host_decided": host[name], "not_ok": bad[name]}
    out["speedup"] = round(min(res["certificates_only"]) / min(res["all"]), 3)
    if args.receipts:
        a, c = min(res["all"]), min(res["receipts"])
        out["receipts_vs_all"] = {"rate_ratio": round(a / c, 4), "extra_ms": round((c - a) * 1e3, 3),
                                  "receipt_bytes": 128 * n,
                                  "median_ms": {"all": round(float(np.median(res["all"])) * 1e3, 3),
                                                "receipts": round(float(np.median(res["receipts"])) * 1e3, 3)}}
        out["host_decode"] = {"decode_ms": round(decode_s * 1e3, 2), "not_ok": bad["host_soa"],
                              "all_plus_decode_ms": round((a + decode_s) * 1e3, 2),
                              "receipts_speedup_over_all_plus_decode": round((a + decode_s) / c, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
