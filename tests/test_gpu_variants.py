"""GPU: kernel variants that are compiled and documented and that nothing else launches,
each in a child process (tests/_variant_probe.py: libntcrypto reads these variables once per process), one
child at a time.

  NT_VERIFY_OCC=1 / 3   k_ed25519_verify<mode, 1|3, 24|20, 2, false>: other register budgets, no key-table
                        cache -- so the cache's counters staying at zero is the proof that they ran, and the
                        same child without the variable must move them
  NT_KEYSET_FUSE=0      the key-cache kernels' verdict-bytes epilogue, k_pack_bytes (no other caller) and a
                        k_group_and launch after a key-cache launch, for the streamed and the chunked kernel.
                        Nothing observable shows that this switch took effect: the child only reports that it
                        ran under the variable, and its verdicts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _passes as P

pytestmark = pytest.mark.gpu
PROBE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_variant_probe.py")
SWITCHES = ("NT_VERIFY_OCC", "NT_KEYSET_FUSE", "NT_KEYSET_STREAM", "NT_KEYSET_SORT", "NT_KEYSET_PER_LANE",
            "NT_KEYSET_WAVES", "NT_VERIFY_NPER")


@pytest.fixture(scope="module")
def data(oracle, tmp_path_factory):
    """batch Y of tests/test_gpu_passes.py and the oracle's per-signature bits of batch_groups.npz, made once
    for every child"""
    y = P.batch_y(oracle)
    path = str(tmp_path_factory.mktemp("variants") / "data.npz")
    np.savez(path, pk=y.pk, sig=y.sig, msg=y.msg, off=y.off, len=y.ln, strict=y.strict,
             group_sig_bits=P.Groups(oracle).sig_bits)
    return path


def child(mode, data, **env):
    e = {k: v for k, v in os.environ.items() if k not in P.KNOBS + SWITCHES}
    e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, PROBE, mode, data], env=e, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


CALLS = ("dev_strict_0", "dev_cofactorless_0", "dev_strict_1", "dev_cofactorless_1", "strict_x", "strict_y", "groups",
         "group_sig_bits")


def test_verify_occupancy_variants(data):
    """Batch X in both modes through the device API, verify_strict on X and Y and verify_batch_groups, at one
    workspace slot (every launch runs later passes) and the 20-bit comb of B, at 2 (default), 1 and 3 waves
    per SIMD: no mismatch anywhere."""
    ws = set()
    for occ in (None, 1, 3):
        env = {"NT_BCOMB_BITS": 20, "NT_WS_SLOTS": 1}
        if occ:
            env["NT_VERIFY_OCC"] = occ
        res = child("verify", data, **env)
        assert res["occ"] == (str(occ) if occ else None) and res["comb_b_bits"] == 20, res
        assert [res[k] for k in CALLS] == [0] * len(CALLS), (occ, res)
        moved = {k: v for k, v in res["ktab"].items() if v}
        if occ:
            assert not moved, (occ, res["ktab"])
        else:
            assert set(moved) == set(P.Counters.KEYS), res["ktab"]
        ws.add(res["workspace_bytes"])
    assert len(ws) == 1 and min(ws) > 0, ws   # one slot of the same size in every child


@pytest.mark.parametrize("stream", [None, 0])
def test_keyset_unfused_epilogue(data, stream):
    """NT_KEYSET_FUSE=0 at 16-bit key combs: the corpus (input order) and its tiling to 65,880 signatures
    (key-grouped order: verdict bytes and k_pack_bytes) in mixed mode against the labels; batch_groups.npz once
    and tiled to 66,150 signatures (n mod 64 = 38) through Keyset.verify_batch_groups against `expect` and the
    oracle's per-signature bits (k_group_and after the key-cache launch).  The switch leaves no trace to
    assert: the outputs are the same words either way."""
    env = {"NT_KEYSET_FUSE": 0, "NT_KEYSET_COMB_BITS": 16}
    if stream is not None:
        env["NT_KEYSET_STREAM"] = stream
    res = child("unfused", data, **env)
    assert res["fuse"] == "0" and res["stream"] == (None if stream is None else str(stream)), res
    assert res["comb_bits"] == 16
    want = {"mixed_360": 0, "mixed_65880": 0, "groups_630": 0, "group_sig_bits_630": 0, "groups_66150": 0,
            "group_sig_bits_66150": 0}
    assert {k: res.get(k) for k in want} == want, res
