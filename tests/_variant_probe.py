"""Subprocess helper of tests/test_gpu_variants.py (not a test module): kernel variants that libntcrypto
selects by variables it reads once per process, so each runs in a process of its own.  Prints one JSON line.

  verify <data.npz>   (parent: NT_BCOMB_BITS=20, NT_WS_SLOTS=1, NT_VERIFY_OCC unset / 1 / 3)
      batch X of tests/test_gpu_passes.py in both modes through nt_dev_ed25519_verify, then verify_strict on X
      and Y and verify_batch_groups on batch_groups.npz tiled 3 times; Y and the oracle's per-signature bits
      come from the parent's file.  Reports mismatches per call and the key-table cache's counters.
  unfused             (parent: NT_KEYSET_FUSE=0, NT_KEYSET_COMB_BITS=16, NT_KEYSET_STREAM unset / 0)
      the corpus once and tiled 183 times through a key set in mixed mode, batch_groups.npz once and tiled 105
      times (66,150 signatures, n mod 64 = 38) through Keyset.verify_batch_groups with per-signature bits."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "narwhal-tusk_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402,F401  (its HIP runtime starts before libntcrypto's: ntcrypto._lib._torch_first)
import ntcrypto  # noqa: E402
import _passes as P  # noqa: E402


def verify_mode(be, out, path):
    d = np.load(path)
    c = P.corpus()
    out["workspace_bytes"] = P.workspace_after_four(be, c)
    out["comb_b_bits"] = be.memory_info()["comb_b_bits"]
    X = P.batch_x(c)
    Y = P.Batch(d["pk"], d["sig"], d["msg"], d["off"], d["len"], d["strict"], d["strict"])
    s = be.dev_stream(0, 0)
    bx = P.DevBatch(be, X)
    for rnd in range(2):  # the second round finds the keys of the first
        out["dev_strict_%d" % rnd] = int((bx.bits(ntcrypto.NT_MODE_STRICT, s) != X.strict).sum())
        out["dev_cofactorless_%d" % rnd] = int((bx.bits(ntcrypto.NT_MODE_COFACTORLESS, s) != X.cofactorless).sum())
    out["strict_x"] = int((be.verify_strict(*X.args()) != X.strict).sum())
    out["strict_y"] = int((be.verify_strict(*Y.args()) != Y.strict).sum())
    g = P.Groups(sig_bits=d["group_sig_bits"]).tiled(3)
    gb, sb = be.verify_batch_groups(g.pk, g.sig, g.first, g.cnt, g.msg32, with_sig_bits=True)
    out["groups"] = int((gb != g.expect).sum())
    out["group_sig_bits"] = int((sb != g.sig_bits).sum())
    out["ktab"] = {k: v for k, v in be.ktab_info(0).items() if k in P.Counters.KEYS}


def unfused_mode(be, out, path):
    d = np.load(path)
    c = P.corpus()
    uniq = np.unique(c["pk"], axis=0)
    ks = be.keyset(uniq)
    out["comb_bits"] = ks.info()[0]
    for reps in (1, 183):
        midx, want = P.mixed_keyset_case(c, reps, len(uniq))
        got = ks.verify(ntcrypto.NT_MODE_MIXED, midx, np.tile(c["sig"], (reps, 1)), c["msg"], np.tile(c["off"], reps),
                        np.tile(c["len"], reps))
        out["mixed_%d" % len(midx)] = int((got != want).sum())
    ks.close()
    groups = P.Groups(sig_bits=d["group_sig_bits"])
    ks = be.keyset(groups.uniq)
    for reps in (1, 105):
        g = groups.tiled(reps)
        gb, sb = ks.verify_batch_groups(g.key_idx, g.sig, g.first, g.cnt, g.msg32, with_sig_bits=True)
        out["groups_%d" % g.n] = int((gb != g.expect).sum())
        out["group_sig_bits_%d" % g.n] = int((sb != g.sig_bits).sum())
    ks.close()


mode, path = sys.argv[1], sys.argv[2]
out = {"mode": mode, "occ": os.environ.get("NT_VERIFY_OCC"), "fuse": os.environ.get("NT_KEYSET_FUSE"),
       "stream": os.environ.get("NT_KEYSET_STREAM")}
be = ntcrypto.Backend(device=0)
try:
    (verify_mode if mode == "verify" else unfused_mode)(be, out, path)
finally:
    be.close()
print(json.dumps(out))
