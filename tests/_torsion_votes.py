"""Helpers over tests/golden/torsion_votes.npz (not a test module): 12 keys
(seven mixed-order, two of order 8, three prime-order controls) x 40
certificate digests, entry (key, g) at row 40 * key + g, labelled by the
generator's Python-integer model (`strict`, `batch_rule`) with
k = H(R || A || M) mod L beside each entry.

The reduced-scalar key combs (21 bits) take k as k or k - L; only a key with a
torsion component owes its [L](-A) entry, and only on the second branch
(k > (L - 1) / 2: `high`).  Everything here is arranged around that branch."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
L = 2 ** 252 + 27742317777372353535851937790883648493
HALF_L = (L - 1) // 2
SORT_MIN = 65536          # key-cache launches of at least this many signatures run in key-grouped order
MIN_PER_BRANCH = 8        # the generator's bound: accepted entries per torsion key and branch


def load():
    d = np.load(os.path.join(GOLD, "torsion_votes.npz"))
    tv = {k: d[k] for k in d.files}
    k = np.array([int.from_bytes(x.tobytes(), "little") for x in tv["k"]], dtype=object)
    tv["high"] = np.array([x > HALF_L for x in k], bool)
    tv["torsion_key"] = tv["kind"][tv["key"]] != 0          # per entry: its key has a torsion component
    n = len(tv["key"])
    tv["off"] = tv["group"].astype(np.uint64) * 32          # entry i signs digest group[i] of msg32
    tv["len"] = np.full(n, 32, np.uint64)
    return tv


def branch_counts(tv):
    """per key: (batch-rule-accepted entries on the low branch, on the high branch)"""
    acc = tv["batch_rule"].astype(bool)
    return [(int((acc & ~tv["high"] & (tv["key"] == ki)).sum()), int((acc & tv["high"] & (tv["key"] == ki)).sum()))
            for ki in range(len(tv["keys"]))]


def tiled_order(tv, seed=21):
    """Row numbers of the entries tiled to the smallest multiple of their
    number that reaches SORT_MIN, every entry the same number of times, in an
    order made for the counting sort (k_key_scatter: blocks of 4,096
    consecutive signatures, each block's share of a key in one contiguous run
    of slots): about two thirds of each entry's copies lie in a stretch of
    high-branch entries only or in a stretch of low-branch entries only, the
    last third is shuffled among all.  So whatever order the blocks reserve
    their runs in, every key has waves of 64 slots that are all on the high
    branch, waves with no lane on it and waves that mix both."""
    n0 = len(tv["key"])
    reps = -(-SORT_MIN // n0)
    rng = np.random.default_rng(seed)
    pure = 2 * reps // 3
    hi = np.repeat(np.flatnonzero(tv["high"]), pure)
    lo = np.repeat(np.flatnonzero(~tv["high"]), pure)
    mix = np.repeat(np.arange(n0), reps - pure)
    order = np.concatenate([rng.permutation(hi), rng.permutation(lo), rng.permutation(mix)])
    assert len(order) == n0 * reps >= SORT_MIN and np.array_equal(np.bincount(order), np.full(n0, reps))
    return order


def wave_branches(tv, order, bucket):
    """The waves of a key-grouped launch as slots follow the key-grouped order
    (a stable sort by bucket; the device's order differs inside a bucket by
    which block reserved first, see tiled_order).  Per key with a torsion
    component: [waves all on the high branch, waves with no lane on it, mixed
    waves], counting waves whose 64 slots hold that key only."""
    slots = np.argsort(bucket, kind="stable")
    nw = len(slots) // 64
    key = bucket[slots][:nw * 64].reshape(nw, 64)
    high = tv["high"][order][slots][:nw * 64].reshape(nw, 64)
    one_key = (key == key[:, :1]).all(axis=1)
    out = {}
    for ki in np.flatnonzero(tv["kind"] != 0):
        h = high[one_key & (key[:, 0] == ki)].sum(axis=1)
        out[int(ki)] = [int((h == 64).sum()), int((h == 0).sum()), int(((h > 0) & (h < 64)).sum())]
    return out, int(one_key.sum()), nw


def certificates(tv, seed=22, min_sigs=SORT_MIN):
    """Certificates over the fixture: group g's votes are entries of digest
    g % 40 under a seeded choice of 1-12 distinct keys; two groups have no
    votes; the last group is accepted and ends at the last signature.  Returns
    (rows, first, cnt, msg32, want_group, want_sig): rows = the entry of each
    vote, want_group = the AND of batch_rule over each group's votes (an empty
    group accepts), want_sig = batch_rule per vote."""
    rng = np.random.default_rng(seed)
    nk, nd = len(tv["keys"]), len(tv["msg32"])
    G = min_sigs // 4 + 256                                     # 6.5 votes a group on average: enough
    cnt = rng.integers(1, nk + 1, G).astype(np.uint32)
    cnt[[7, 200]] = 0
    # cut at the first group that reaches min_sigs; the closing group follows it
    G = int(np.searchsorted(np.cumsum(cnt), min_sigs)) + 1
    cnt = cnt[:G]
    acc = tv["batch_rule"].astype(bool).reshape(nk, nd)
    d_last = G % nd
    good = np.flatnonzero(acc[:, d_last])[:3]
    assert len(good) == 3
    keys = rng.permuted(np.tile(np.arange(nk), (G + 1, 1)), axis=1)
    keys[G, :3] = good
    cnt = np.append(cnt, np.uint32(3))
    G += 1
    take = np.arange(nk)[None, :] < cnt[:, None]
    digest = (np.arange(G) % nd)
    rows = (keys * nd + digest[:, None])[take]                 # row-major: group after group
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint64)
    want_sig = tv["batch_rule"][rows].astype(bool)
    want_group = np.array([want_sig[int(f):int(f) + int(c)].all() for f, c in zip(first, cnt)])
    n = len(rows)
    assert n >= min_sigs and int(first[-1]) + 3 == n and want_group[-1]
    f, c = first.astype(np.int64), cnt.astype(np.int64)
    assert ((f % 64 == 0) & (c > 0) & (f > 0)).any()           # a boundary on a multiple of 64
    assert ((c > 0) & (f // 64 != (f + c - 1) // 64)).any()    # a group across one
    assert (cnt == 0).sum() == 2 and 0 < want_group.sum() < G
    return rows, first, cnt, tv["msg32"][digest], want_group, want_sig
