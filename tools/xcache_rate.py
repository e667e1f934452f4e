"""What the x cache (decompressed public keys kept across calls) buys
nt_dev_ed25519_verify, against the share of keys the context has never seen.

One process, one GPU.  A batch of N strict verifications over N distinct keys
(config 2's shape without its edge cases) is made known to the context; every
timed step then replaces a fraction f of its entries, at random positions, by
signatures of keys that have never been verified before (a fresh pool per step).
A wave skips the square root only when all 64 of its lanes find their key, so the
rate falls with 0.99^64 ... rather than with f.  Also timed: the same seen batch
with the cache off (NT_XCACHE_SLOTS=0 is read at every launch).
Prints one JSON line.
Usage: python tools/xcache_rate.py [--sigs N] [--steps K] [--fractions 0,0.01,0.1,1]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "narwhal-tusk_amd"))


def nbytes(t):
    return int(t.numel()) * int(t.element_size())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sigs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--msg-len", type=int, default=64)
    ap.add_argument("--fractions", default="0,0.01,0.1,1")
    args = ap.parse_args()
    fracs = [float(x) for x in args.fractions.split(",")]
    n, L, K = args.sigs, args.msg_len, args.steps
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    import ntcrypto
    os.environ.pop("NT_XCACHE_SLOTS", None)
    be = ntcrypto.Backend(device=0)
    cur = torch.cuda.Stream(dev)
    torch.cuda.set_stream(cur)
    g = torch.Generator(device=dev)
    g.manual_seed(77)
    off = torch.arange(n, dtype=torch.int64, device=dev) * L
    ln = torch.full((n,), L, dtype=torch.int64, device=dev)

    def signed():
        """n signatures of n fresh keys: (pk, sig, msgs)"""
        seeds = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=g)
        msgs = torch.randint(0, 256, (n * L + 64,), dtype=torch.uint8, device=dev, generator=g)
        pk = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        sig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        be.dev_sign(0, cur.cuda_stream, seeds.data_ptr(), msgs.data_ptr(), nbytes(msgs), off.data_ptr(), ln.data_ptr(), n,
                    pk.data_ptr(), sig.data_ptr())
        torch.cuda.synchronize(dev)
        return pk, sig, msgs

    seen = signed()
    out = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    st = torch.cuda.ExternalStream(be.dev_stream(0, 0), device=dev)
    torch.cuda.synchronize(dev)

    def verify(b):
        be.dev_verify(0, st.cuda_stream, ntcrypto.NT_MODE_STRICT, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(),
                      nbytes(b[2]), off.data_ptr(), ln.data_ptr(), n, out.data_ptr())

    def all_accepted():
        torch.cuda.synchronize(dev)
        bits = np.unpackbits(out.cpu().numpy().view(np.uint8), bitorder="little")[:n]
        return bool(bits.all())

    def timed(batches):
        """M verifies/s over the batches, one launch each, back to back on one stream"""
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        for x in batches:
            verify(x)
        b.record(st)
        torch.cuda.synchronize(dev)
        assert all_accepted()
        return round(n * len(batches) / a.elapsed_time(b) / 1e3, 2)

    res = {"sigs": n, "steps": K, "msg_len": L}
    os.environ["NT_XCACHE_SLOTS"] = "0"
    for _ in range(2):
        verify(seen)
    res["cache_off"] = timed([seen] * K)
    os.environ.pop("NT_XCACHE_SLOTS")
    for _ in range(4):  # the seen keys settle in the table
        verify(seen)
    res["rate_by_unseen_fraction"] = {}
    for f in fracs:
        batches = []
        for _ in range(K):
            if f <= 0:
                batches.append(seen)
                continue
            fresh = signed()
            if f >= 1:
                batches.append(fresh)
                continue
            take = torch.rand(n, device=dev, generator=g) < f
            pk = torch.where(take[:, None], fresh[0], seen[0])
            sig = torch.where(take[:, None], fresh[1], seen[1])
            m = torch.where(take.repeat_interleave(L), fresh[2][:n * L], seen[2][:n * L])
            batches.append((pk, sig, torch.cat([m, seen[2][n * L:]])))
        torch.cuda.synchronize(dev)
        res["rate_by_unseen_fraction"][str(f)] = timed(batches)
        for _ in range(2):  # the seen keys settle again before the next row
            verify(seen)
    res["unit"] = "M verifies/s"
    be.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
