"""GPU: the key-table cache's comb path: for a key whose comb is cached the verify
kernel computes [k](-A) from 64 signed lookups of 33 affine lines with 15 doublings (ladder_kc),
k recoded as K = k | 1 with one correcting addition for even k.  Verdicts are the oracle's (or the
corpus labels) in both modes, for both parities of k, for keys with a torsion component and for
keys that do not decode; every test asserts the kernel's own row counters, so none passes with
the comb path idle."""
import hashlib
import os

import numpy as np
import pytest

import _arith_checks as C
from test_gpu_ktab import Batch, Counters
from test_gpu_ktab4 import expected, modes, sign

pytestmark = pytest.mark.gpu
ENTRY, COMB = 3968, 4224
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL_FAST = lambda b: {"used": 0, "fast_rows": b.rows(), "builds": 0, "old_rows": 0}


@pytest.fixture(scope="module")
def be():
    import ntcrypto
    os.environ.pop("NT_KTAB_KEYS", None)
    b = ntcrypto.Backend(0)
    yield b
    b.close()


def hram(pk, sig, data, off, ln):
    """k = SHA-512(R || A || M) mod L of every signature, as Python integers"""
    return [int.from_bytes(hashlib.sha512(bytes(sig[i, :32]) + bytes(pk[i]) +
                                          data[int(off[i]):int(off[i] + ln[i])].tobytes()).digest(), "little") % C.L
            for i in range(len(pk))]


@pytest.mark.parametrize("mode", (0, 1), ids=("strict", "cofactorless"))
@pytest.mark.parametrize("parity", (0, 1), ids=("even", "odd"))
def test_both_parities_alone(be, oracle, monkeypatch, parity, mode):
    """One signature whose k is even (the correction adds +A) or odd (it adds the identity), alone
    in its launch, three launches: met, built, hit -- the third is all fast rows.  Then the same
    signature with s corrupted (k unchanged) through the cached comb: the oracle's verdicts."""
    monkeypatch.delenv("NT_KTAB_KEYS", raising=False)
    # 16 signatures of one new key over different messages: the first with the wanted parity of k
    rng = np.random.default_rng(500 + 2 * parity + mode)
    seed = np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), 16, axis=0)
    ln = np.full(16, 40, np.uint64)
    off = (np.arange(16) * 40).astype(np.uint64)
    data = rng.integers(0, 256, 16 * 40 + 1, dtype=np.uint8)
    pk, sig = be.sign_batch(seed, data, off, ln)
    ks = hram(pk, sig, data, off, ln)
    i = next(j for j, k in enumerate(ks) if k & 1 == parity)
    pk, sig, off, ln = pk[i:i + 1], sig[i:i + 1].copy(), off[i:i + 1], ln[i:i + 1]
    assert expected(oracle, pk, sig, data, off, ln)[mode].all()
    b = Batch(be, pk, sig, data, off, ln)
    c = Counters(be)
    for launch in range(3):
        assert b.bits(b.launch(modes()[mode][0], be.dev_stream(0, 0))).all(), launch
        dl = c.delta()
    assert dl == ALL_FAST(b), dl
    sig[0, 40] ^= 0x04
    assert hram(pk, sig, data, off, ln)[0] == ks[i] and not expected(oracle, pk, sig, data, off, ln)[mode].any()
    b = Batch(be, pk, sig, data, off, ln)
    assert not b.bits(b.launch(modes()[mode][0], be.dev_stream(0, 0))).any()
    assert c.delta() == ALL_FAST(b)


@pytest.mark.parametrize("mode", (0, 1), ids=("strict", "cofactorless"))
@pytest.mark.parametrize("n", (65, 513))
def test_distinct_keys_three_launches(be, oracle, monkeypatch, n, mode):
    """n = 65 and 513 new keys (more than one row, more than one block), a tenth of the signatures
    corrupted, both parities of k in the batch, three launches: the oracle's verdicts each time; on
    the third every row is a fast row and nothing is built.  The cache reports 8,192 bytes a key."""
    monkeypatch.delenv("NT_KTAB_KEYS", raising=False)
    pk, sig, data, off, ln = sign(be, n, n, 7000 + 10 * n + mode)
    flip = np.random.default_rng(n + 1).random(n) < 0.1
    sig[flip, 7] ^= 0x10
    parities = {k & 1 for k in hram(pk, sig, data, off, ln)}
    assert parities == {0, 1}
    want = expected(oracle, pk, sig, data, off, ln)[mode]
    assert np.array_equal(want, ~flip) and flip.any()
    b = Batch(be, pk, sig, data, off, ln)
    c = Counters(be)
    for launch in range(3):
        assert np.array_equal(b.bits(b.launch(modes()[mode][0], be.dev_stream(0, 0))), want), launch
        dl = c.delta()
    assert dl == ALL_FAST(b), dl
    info = be.ktab_info(0)
    assert ENTRY + COMB == 8192 and info["capacity"] >= n and info["bytes"] >= info["capacity"] * 8192, info


def test_torsion_and_undecodable_keys(be, monkeypatch):
    """The corpus entries whose keys are of mixed or small order or do not decode, padded to whole
    rows with honest signatures of new keys, three launches in each mode: the labels each time, and
    the third launch is all fast rows -- the comb's sum is an integer identity, so a torsion
    component changes nothing, and a key without a comb is a flagged hit."""
    monkeypatch.delenv("NT_KTAB_KEYS", raising=False)
    M = C.model()
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    kinds = {}
    for e in dict.fromkeys(bytes(k) for k in d["pk"]):
        A = M.decode(e)
        kinds[e] = "undecodable" if A is None else ("small" if M.is_small(A) else ("mixed" if M.has_torsion(A) else "honest"))
    pick = np.array([kinds[bytes(k)] != "honest" for k in d["pk"]])
    assert {kinds[bytes(k)] for k in d["pk"][pick]} == {"undecodable", "small", "mixed"}
    m = int(pick.sum())
    pad = -m % 64 or 64
    hpk, hsig, hdata, hoff, hln = sign(be, pad, pad, 8080)
    pk, sig = np.concatenate([d["pk"][pick], hpk]), np.concatenate([d["sig"][pick], hsig])
    data = np.concatenate([d["msg"], hdata])
    off = np.concatenate([d["off"][pick].astype(np.uint64), hoff + np.uint64(len(d["msg"]))])
    ln = np.concatenate([d["len"][pick].astype(np.uint64), hln])
    assert len(pk) % 64 == 0
    b = Batch(be, pk, sig, data, off, ln)
    c = Counters(be)
    for (nt_mode, _), label in zip(modes(), ("strict", "batch_rule")):
        want = np.concatenate([d[label][pick].astype(bool), np.ones(pad, bool)])
        for launch in range(3):
            got = b.bits(b.launch(nt_mode, be.dev_stream(0, 0)))
            assert np.array_equal(got, want), (label, launch, np.nonzero(got != want)[0])
            dl = c.delta()
        assert dl == ALL_FAST(b), (label, dl)
