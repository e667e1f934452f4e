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

    python tools/ingest_mixed_rate.py [--messages 100000] [--reps 3]
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=4, help="distinct rounds built before repeating")
    ap.add_argument("--committee", type=int, default=100)
    ap.add_argument("--threads", type=int, default=16, help="host decoder threads")
    ap.add_argument("--reps", type=int, default=3)
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
        core = N.Core(pks, np.ones(args.committee, np.uint32), np.ones(args.committee, np.uint32), 0,
                      W.message(cur), True)
        try:
            res = {"all": [], "certificates_only": []}
            host = {}
            bad = {}
            modes = (("all", "all"), ("certificates_only", True))
            for name, dev in modes:                       # warm-up: committee tables, buffers, staging
                core.ingest(data, off, ln, args.threads, device=dev)
            for _ in range(args.reps):
                for name, dev in modes:                   # alternating
                    t0 = time.perf_counter()
                    got, h = core.ingest(data, off, ln, args.threads, device=dev)
                    res[name].append(time.perf_counter() - t0)
                    host[name] = int(h)
                    bad[name] = int((got != 0).sum())
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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
