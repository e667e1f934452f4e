"""What the key-table cache (window tables of A, [2^64]A, [2^128]A kept for keys
seen before) costs and buys nt_dev_ed25519_verify, by how well the context knows the keys.

One process, one GPU.  Batches of N strict verifications over N distinct keys (config 2's shape
without its edge cases); every figure is taken `--repeats` times, the kinds interleaved, one launch
each (the never-seen and seen-once batches are fresh ones every time), and reported with its median:
  seen        a batch verified often before (every row on the short ladder)
  unseen      keys never seen (the probe; the x cache misses and stores)
  seen_once   keys seen exactly once (the launch that claims and builds every entry)
  mixed_0.01 / mixed_0.1   the seen batch with that share of never-seen keys at random places
  cache_off   the seen batch with NT_KTAB_KEYS=0 (read at every launch)
Run it in turn with NTCRYPTO_LIB=<a parent build's library> for the rates to compare with
(tools/ab_ktab_rate.sh alternates the two and prints the medians side by side).  Default 200 k
signatures per launch: the distinct keys of one run stay well inside the index and the pool.
Prints one JSON line.
Usage: python tools/ktab_rate.py [--sigs N] [--repeats R]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "narwhal-tusk_amd"))


KINDS = ("seen", "cache_off", "unseen", "seen_once", "mixed_0.01", "mixed_0.1")


def nbytes(t):
    return int(t.numel()) * int(t.element_size())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sigs", type=int, default=200_000)
    ap.add_argument("--msg-len", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    n, L = args.sigs, args.msg_len
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    import ntcrypto
    os.environ.pop("NT_KTAB_KEYS", None)
    be = ntcrypto.Backend(device=0)
    cur = torch.cuda.Stream(dev)
    torch.cuda.set_stream(cur)
    g = torch.Generator(device=dev)
    g.manual_seed(78)
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

    out = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    st = torch.cuda.ExternalStream(be.dev_stream(0, 0), device=dev)
    torch.cuda.synchronize(dev)

    def verify(b):
        be.dev_verify(0, st.cuda_stream, ntcrypto.NT_MODE_STRICT, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(),
                      nbytes(b[2]), off.data_ptr(), ln.data_ptr(), n, out.data_ptr())

    def timed(b):
        """M verifies/s of one launch"""
        torch.cuda.synchronize(dev)
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        verify(b)
        z.record(st)
        torch.cuda.synchronize(dev)
        assert bool(np.unpackbits(out.cpu().numpy().view(np.uint8), bitorder="little")[:n].all())
        return round(n / a.elapsed_time(z) / 1e3, 2)

    def mixed(seen, f):
        fresh = signed()
        take = torch.rand(n, device=dev, generator=g) < f
        pk = torch.where(take[:, None], fresh[0], seen[0])
        sig = torch.where(take[:, None], fresh[1], seen[1])
        m = torch.where(take.repeat_interleave(L), fresh[2][:n * L], seen[2][:n * L])
        return pk, sig, torch.cat([m, seen[2][n * L:]])

    def median(v):
        return sorted(v)[len(v) // 2]

    R = args.repeats
    res = {"sigs": n, "msg_len": L, "repeats": R, "library": "NTCRYPTO_LIB" if os.environ.get("NTCRYPTO_LIB") else "this tree"}
    seen = signed()
    for _ in range(4):  # met, built, and the x cache settled
        verify(seen)
    fresh = [signed() for _ in range(R)]      # never seen: each launched exactly once
    once = [signed() for _ in range(R)]       # seen once before their timed launch
    for b in once:
        verify(b)
    m1 = [mixed(seen, 0.01) for _ in range(R)]
    m10 = [mixed(seen, 0.1) for _ in range(R)]
    rows = {k: [] for k in KINDS}
    for r in range(R):  # the kinds interleaved
        rows["seen"].append(timed(seen))
        os.environ["NT_KTAB_KEYS"] = "0"
        rows["cache_off"].append(timed(seen))
        os.environ.pop("NT_KTAB_KEYS")
        rows["unseen"].append(timed(fresh[r]))
        rows["seen_once"].append(timed(once[r]))
        rows["mixed_0.01"].append(timed(m1[r]))
        rows["mixed_0.1"].append(timed(m10[r]))
    res["runs"] = rows
    res["median"] = {k: median(v) for k, v in rows.items()}
    try:
        res["ktab"] = be.ktab_info(0)
    except ntcrypto.NtError:  # a library from before the cache
        pass
    res["unit"] = "M verifies/s"
    be.close()
    print(json.dumps(res), flush=True)


def summarize(out, rounds):
    """medians over all launches of <out>/{new,parent}_r<k>.json (tools/ab_ktab_rate.sh), side by side"""
    med = lambda v: sorted(v)[len(v) // 2]
    runs = {k: [json.load(open("%s/%s_r%d.json" % (out, k, r)))["runs"] for r in range(1, rounds + 1)]
            for k in ("new", "parent")}
    print("%-12s %10s %10s %8s   (M verifies/s, median over every launch of %d runs each)"
          % ("kind", "this tree", "parent", "ratio", rounds))
    for kind in KINDS:
        a = med([x for r in runs["new"] for x in r[kind]])
        b = med([x for r in runs["parent"] for x in r[kind]])
        print("%-12s %10.2f %10.2f %8.4f" % (kind, a, b, a / b))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], int(sys.argv[3]))
    else:
        main()
