"""Subprocess helper of test_gpu_parity.test_keyset_per_lane_counts (not a test
module): the corpus through the key cache in mixed mode with the per-lane
row cap and waves per SIMD the parent chose (NT_KEYSET_PER_LANE,
NT_KEYSET_WAVES, read once per process by libntcrypto), as the plain corpus
(input order), tiled to 72k signatures (key-grouped order, one row per
chunk) and to ~1M signatures (multi-row chunks, several rounds at small
caps).  Prints one JSON line: mismatches per launch.

With the argument `torsion` (test_gpu_keycache_width.test_width_plans_and_caps):
the key set of tests/golden/torsion_votes.npz at the width in
NT_KEYSET_COMB_BITS instead, its 480 entries and their tiling to 65,760
signatures (_torsion_votes.tiled_order), and the width the device gave."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "narwhal-tusk_amd"))
import ntcrypto  # noqa: E402


def corpus_mode(be, out):
    d = np.load(os.path.join(ROOT, "tests", "golden", "ed25519_corpus.npz"))
    uniq, inv = np.unique(d["pk"], axis=0, return_inverse=True)
    inv = inv.ravel().astype(np.uint32)
    ks = be.keyset(uniq)
    for reps in (1, 200, 2800):
        n0 = len(inv)
        idx = np.tile(inv, reps)
        unknown = (np.arange(n0 * reps) % 97) == 5
        idx[unknown] = len(uniq) + 3
        strict = (np.arange(n0 * reps) % 3) == 1
        midx = (idx | np.where(strict, np.uint32(ntcrypto.NT_KEY_STRICT_BIT), np.uint32(0))).astype(np.uint32)
        got = ks.verify(ntcrypto.NT_MODE_MIXED, midx, np.tile(d["sig"], (reps, 1)), d["msg"], np.tile(d["off"], reps),
                        np.tile(d["len"], reps))
        want = np.where(strict, np.tile(d["strict"], reps), np.tile(d["batch_rule"], reps)).astype(bool) & ~unknown
        out["mismatches_%d" % (n0 * reps)] = int((got != want).sum())
    ks.close()


def torsion_mode(be, out):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _torsion_votes as T
    tv = T.load()
    ks = be.keyset(tv["keys"])
    out["comb_bits"] = ks.info()[0]
    nk = len(tv["keys"])
    for rows in (np.arange(len(tv["key"])), T.tiled_order(tv)):
        n = len(rows)
        unknown = (np.arange(n) % 97) == 5
        strict = (np.arange(n) % 3) == 1
        idx = np.where(unknown, nk + 3, tv["key"][rows]).astype(np.uint32)
        midx = (idx | np.where(strict, np.uint32(ntcrypto.NT_KEY_STRICT_BIT), np.uint32(0))).astype(np.uint32)
        got = ks.verify(ntcrypto.NT_MODE_MIXED, midx, tv["sig"][rows], tv["msg32"].reshape(-1), tv["off"][rows],
                        tv["len"][rows])
        want = np.where(strict, tv["strict"][rows], tv["batch_rule"][rows]).astype(bool) & ~unknown
        out["mismatches_%d" % n] = int((got != want).sum())
    ks.close()


be = ntcrypto.Backend(0)
out = {"per_lane": os.environ.get("NT_KEYSET_PER_LANE"), "waves": os.environ.get("NT_KEYSET_WAVES")}
if sys.argv[1:] == ["torsion"]:
    torsion_mode(be, out)
else:
    corpus_mode(be, out)
be.close()
print(json.dumps(out))
