"""The signer's per-lane operations (narwhal-tusk_amd/csrc/signer_ops.hpp) on the
host.  CPU only: tests/cpp/signer/ builds signer_check, a stand-alone program under
the address and undefined-behaviour sanitizers that runs signer_key_setup,
vote_digest_words, sign_fixed_one, vote_wire_words, sign_one and b64_encode32 over a
host comb of B and writes the vote records into a buffer of exactly n x 212 bytes.
Everything is compared byte for byte with the model: tests/_wire.py's Vote, the
oracle's pubkey / sign, Python's base64."""
import base64
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import _wire as W
from _signer_model import edge_triples, model_vote

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SDIR = os.path.join(ROOT, "tests", "cpp", "signer")
CHECK = os.path.join(ROOT, "tests", "cpp", "build", "signer_check")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def checker():
    subprocess.run(["make", "-s", "-C", SDIR], check=True)
    return CHECK


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(GOLD, "fixtures_reference.json")) as f:
        return json.load(f)


def run(checker, tmp_path, name, seeds=(), votes=(), digests=(), pairs=(), keys=()):
    blob = [struct.pack("<5I", len(seeds), len(votes), len(digests), len(pairs), len(keys))] + list(seeds)
    blob += [struct.pack("<I", k) + id_ + struct.pack("<Q", r) + o for k, id_, r, o in votes]
    blob += [struct.pack("<I", k) + d for k, d in digests]
    blob += [s + m for s, m in pairs] + list(keys)
    src, dst = tmp_path / (name + ".in"), tmp_path / (name + ".out")
    src.write_bytes(b"".join(blob))
    r = subprocess.run([checker, str(src), str(dst)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "%d votes" % len(votes) in r.stdout and "(0 differ)" in r.stdout
    out = dst.read_bytes()
    at = 0

    def take(n, size):
        nonlocal at
        got = [out[at + size * i:at + size * (i + 1)] for i in range(n)]
        at += size * n
        return got

    res = {"keys": take(len(seeds), 76), "votes": take(len(votes), 212), "vote_digests": take(len(votes), 32),
           "sigs": take(len(digests), 64), "pairs": take(len(pairs), 160), "texts": take(len(keys), 44)}
    assert at == len(out)
    return res


def test_key_records_and_hello_signatures(checker, tmp_path, oracle, ref):
    seeds = [bytes.fromhex(k["seed"]) for k in ref["keys"]]
    hello = bytes.fromhex(ref["hello_digest"])
    got = run(checker, tmp_path, "keys", seeds=seeds, digests=[(i, hello) for i in range(len(seeds))])
    assert len(seeds) == 4
    for i, k in enumerate(ref["keys"]):
        pk = bytes.fromhex(k["pk"])
        assert oracle.pubkey(seeds[i]) == pk
        assert got["keys"][i] == pk + base64.b64encode(pk)
        assert got["sigs"][i] == bytes.fromhex(ref["hello_signatures"][i]) == oracle.sign(seeds[i], pk, hello)


def test_votes_match_the_model(checker, tmp_path, oracle, ref):
    rng = np.random.default_rng(20)
    seeds = [bytes.fromhex(k["seed"]) for k in ref["keys"]] + [rng.integers(0, 256, 32, dtype=np.uint8).tobytes()]
    votes = []
    for i in range(2000):
        votes.append((i % len(seeds), rng.integers(0, 256, 32, dtype=np.uint8).tobytes(),
                      int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)),
                      rng.integers(0, 256, 32, dtype=np.uint8).tobytes()))
    for k in (0, 4):
        votes += [(k,) + t for t in edge_triples(rng, oracle.pubkey(seeds[k]))]
    got = run(checker, tmp_path, "votes", seeds=seeds, votes=votes)
    for i, (k, id_, round_, origin) in enumerate(votes):
        wire, digest = model_vote(oracle, seeds[k], id_, round_, origin)
        assert len(wire) == 212
        assert got["votes"][i] == wire, i
        assert got["vote_digests"][i] == digest, i
    # the fixture's votes: the reference's own signatures over its header's vote digest
    by_pk = {bytes.fromhex(k["pk"]): i for i, k in enumerate(ref["keys"])}
    fx = [(by_pk[bytes.fromhex(v["author"])], bytes.fromhex(v["digest"])) for v in ref["votes"]]
    sigs = run(checker, tmp_path, "fixture_votes", seeds=seeds[:4], digests=fx)["sigs"]
    assert sigs == [bytes.fromhex(v["signature"]) for v in ref["votes"]] and len(sigs) > 0


def test_sign_fixed_one_equals_sign_one(checker, tmp_path, oracle):
    rng = np.random.default_rng(21)
    pairs = [(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
             for _ in range(500)]
    got = run(checker, tmp_path, "pairs", pairs=pairs)["pairs"]
    for (seed, msg), g in zip(pairs, got):
        fixed, one, pk = g[:64], g[64:128], g[128:]
        assert fixed == one
        assert pk == oracle.pubkey(seed) and one == oracle.sign(seed, pk, msg)


def test_b64_encode32(checker, tmp_path):
    rng = np.random.default_rng(22)
    keys = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(1000)] + [bytes(32), b"\xff" * 32]
    got = run(checker, tmp_path, "b64", keys=keys)["texts"]
    assert got == [base64.b64encode(k) for k in keys]
    assert all(len(t) == 44 and t.endswith(b"=") for t in got)
