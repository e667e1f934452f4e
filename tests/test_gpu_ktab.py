"""GPU: the verify kernel's key-table cache (window tables of A, [2^64]A, [2^128]A kept for
keys seen before) never changes a verdict -- first sighting, build, hit,
mixed rows, concurrent builders and readers on the library's two streams, a pool that
runs out, and switched off -- and really takes the short ladder: every test asserts the
kernel's own row counters (nt_memory_info with NT_INFO_KTAB), so none passes with the cache idle."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu


def nbytes(t):
    return int(t.numel()) * int(t.element_size())


@pytest.fixture(scope="module")
def be():
    import ntcrypto
    os.environ.pop("NT_KTAB_KEYS", None)
    b = ntcrypto.Backend(0)
    yield b
    b.close()


class Batch:
    """device copies of one batch, verified through nt_dev_ed25519_verify"""

    def __init__(self, be, pk, sig, msg, off, ln):
        import torch
        self.be, self.torch, self.n = be, torch, len(pk)
        self.dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.host = (pk, sig, msg, off, ln)
        self.pk, self.sig, self.msg = up(pk), up(sig), up(msg)
        self.off, self.ln = up(np.asarray(off, np.uint64).view(np.int64)), up(np.asarray(ln, np.uint64).view(np.int64))
        torch.cuda.synchronize(self.dev)

    def on(self, be):
        return Batch(be, *self.host)

    def outs(self, k):
        o = [self.torch.zeros((self.n + 63) // 64, dtype=self.torch.int64, device=self.dev) for _ in range(k)]
        self.torch.cuda.synchronize(self.dev)  # zeroed on torch's stream, written on the library's
        return o

    def launch(self, mode, stream, out=None):
        out = self.outs(1)[0] if out is None else out
        self.be.dev_verify(0, stream, mode, self.pk.data_ptr(), self.sig.data_ptr(), self.msg.data_ptr(), nbytes(self.msg),
                           self.off.data_ptr(), self.ln.data_ptr(), self.n, out.data_ptr())
        return out

    def words(self, out):
        self.torch.cuda.synchronize(self.dev)
        return out.cpu().numpy().copy()

    def bits(self, out):
        return np.unpackbits(self.words(out).view(np.uint8), bitorder="little")[:self.n].astype(bool)

    def rows(self):
        """wave rows a launch runs: whole blocks of 4 waves x 2 rows (lanes past n repeat entry n - 1)"""
        return 8 * ((self.n + 511) // 512)


class Counters:
    """nt_memory_info | NT_INFO_KTAB deltas of one context (the launches synchronised first)"""

    def __init__(self, be):
        import torch
        self.be, self.torch = be, torch
        self.last = self.read()

    def read(self):
        self.torch.cuda.synchronize()
        return self.be.ktab_info(0)

    def delta(self):
        now = self.read()
        d = {k: now[k] - self.last[k] for k in ("used", "fast_rows", "builds", "old_rows")}
        self.last = now
        return d


def test_corpus_four_rounds(be, monkeypatch):
    """The 360-entry corpus (small-order, mixed-order, non-canonical-y, y = +-1 and off-curve keys)
    four times in one context, strict and cofactorless: the labels each time.  A key is left to the
    x cache when first met (only marked if the x cache can never hold it: it does not decode, or
    x = 0) and built when met again: after the first round every key has its entry, and from the
    second round on every row takes the short ladder and none builds -- undecodable and
    small-order keys included (flagged entries are hits)."""
    import ntcrypto
    monkeypatch.delenv("NT_KTAB_KEYS", raising=False)
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    b = Batch(be, d["pk"], d["sig"], d["msg"], d["off"], d["len"])
    s = be.dev_stream(0, 0)
    c = Counters(be)
    nkeys = len(np.unique(d["pk"], axis=0))
    used = 0
    for rnd in range(4):
        for mode, label in ((ntcrypto.NT_MODE_STRICT, "strict"), (ntcrypto.NT_MODE_COFACTORLESS, "batch_rule")):
            got = b.bits(b.launch(mode, s))
            assert np.array_equal(got, d[label].astype(bool)), (rnd, label, np.nonzero(got != d[label].astype(bool))[0])
        dl = c.delta()
        used += dl["used"]
        if rnd == 0:
            assert used == nkeys and dl["builds"] > 0, (used, dl)
        else:
            assert dl == {"used": 0, "fast_rows": 2 * b.rows(), "builds": 0, "old_rows": 0}, (rnd, dl)
    info = be.ktab_info(0)
    assert info["capacity"] >= nkeys and info["bytes"] >= info["capacity"] * 3968 and info["index_slots"] == 1 << 21  # 16 MB of 8-byte slots


@pytest.fixture(scope="module")
def signer(be):
    def make(n, nkeys, seed, corrupt=0.05):
        """n signatures of nkeys seeded keys, a fraction corrupted: (pk, sig, data, off, ln, ok)"""
        rng = np.random.default_rng(seed)
        # every key at least once, the rest at random
        which = rng.permutation(np.concatenate([np.arange(nkeys), rng.integers(0, nkeys, n - nkeys)])) if nkeys < n else np.arange(n)
        seeds = rng.integers(0, 256, (nkeys, 32), dtype=np.uint8)[which]
        ln = rng.integers(0, 200, n).astype(np.uint64)
        off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
        data = rng.integers(0, 256, int(ln.sum()) + 1, dtype=np.uint8)
        pk, sig = be.sign_batch(seeds, data, off, ln)
        assert len(np.unique(pk, axis=0)) == min(n, nkeys)
        sig = sig.copy()
        flip = rng.random(n) < corrupt
        sig[flip, 7] ^= 0x10
        return pk, sig, data, off, ln, ~flip
    return make


def test_small_shapes(be, signer, oracle, monkeypatch):
    """n = 1 (one live lane, the other 511 repeat it without sightings: one entry), n = 65 (a full row
    and a row of one), and a row of 63 cached keys + 1 never seen (the balanced path, right
    verdicts)."""
    import ntcrypto
    monkeypatch.delenv("NT_KTAB_KEYS", raising=False)
    s = be.dev_stream(0, 0)
    c = Counters(be)
    pk, sig, data, off, ln, ok = signer(65, 65, 31, corrupt=0.1)
    want = oracle.verify_strict_many(pk, sig, data, off, ln).astype(bool)
    assert np.array_equal(want, ok) and not ok.all()
    one = Batch(be, pk[64:], sig[64:], data, off[64:], ln[64:])
    # A launch runs whole blocks of 8 rows; lanes past n repeat entry n - 1 (their verdicts dropped)
    # and neither mark nor claim, so the one live lane does it all: met, built, hit.
    steps = []
    for _ in range(3):
        assert np.array_equal(one.bits(one.launch(ntcrypto.NT_MODE_STRICT, s)), want[64:])
        steps.append(c.delta())
    assert steps[0] == {"used": 0, "fast_rows": 0, "builds": 0, "old_rows": 8}, steps
    # (the building wave's second row comes after its build and may already hit)
    assert (steps[1]["used"], steps[1]["builds"], steps[1]["fast_rows"] + steps[1]["old_rows"]) == (1, 1, 8), steps
    assert steps[1]["old_rows"] >= 4 and steps[2] == {"used": 0, "fast_rows": 8, "builds": 0, "old_rows": 0}, steps
    b = Batch(be, pk, sig, data, off, ln)
    steps = []
    for _ in range(3):
        assert np.array_equal(b.bits(b.launch(ntcrypto.NT_MODE_STRICT, s)), want)
        steps.append(c.delta())
    # row 0: 64 new keys; the other 7 rows: the key cached above
    assert steps == [{"used": 0, "fast_rows": 7, "builds": 0, "old_rows": 1},
                     {"used": 64, "fast_rows": 7, "builds": 1, "old_rows": 1},
                     {"used": 0, "fast_rows": 8, "builds": 0, "old_rows": 0}], steps
    pk2, sig2, data2, off2, ln2, ok2 = signer(1, 1, 32, corrupt=0.0)
    mix = Batch(be, np.concatenate([pk[:63], pk2]), np.concatenate([sig[:63], sig2]), np.concatenate([data, data2]),
                np.concatenate([off[:63], off2 + len(data)]), np.concatenate([ln[:63], ln2]))
    assert np.array_equal(mix.bits(mix.launch(ntcrypto.NT_MODE_STRICT, s)), np.concatenate([want[:63], ok2]))
    assert c.delta() == {"used": 0, "fast_rows": 0, "builds": 0, "old_rows": 8}


@pytest.fixture(scope="module")
def repeated(be, signer, oracle):
    """4,096 signatures of 512 distinct keys (every wave mixes repeated keys), 5 % corrupted"""
    pk, sig, data, off, ln, ok = signer(4096, 512, 4242)
    want = oracle.verify_strict_many(pk, sig, data, off, ln, nthreads=8).astype(bool)
    assert np.array_equal(want, ok)
    return Batch(be, pk, sig, data, off, ln), want


def test_repeated_keys_two_streams_unsynchronised(be, repeated, monkeypatch):
    """The batch twice per stream on the library's two streams with nothing between the four
    calls: launches mark, claim, build and read the one cache at once (a reader's second pass
    has the index lines of its first in reach).  Then the same twice more; then one launch alone,
    all of whose rows must take the short ladder."""
    import ntcrypto
    monkeypatch.delenv("NT_KTAB_KEYS", raising=False)
    b, want = repeated
    c = Counters(be)
    total = {"used": 0, "builds": 0}
    for run in ("cold", "again", "warm"):
        outs = b.outs(4)
        for k in range(4):  # back to back: no synchronisation between the calls
            b.launch(ntcrypto.NT_MODE_STRICT, be.dev_stream(0, k & 1), outs[k])
        for o in outs:
            assert np.array_equal(b.bits(o), want), run
        dl = c.delta()
        assert dl["fast_rows"] + dl["old_rows"] == 4 * b.rows(), (run, dl)
        total = {k: total[k] + dl[k] for k in total}
        if run == "warm":  # 8 launches earlier: met, marked and built, whatever overlapped
            assert total["used"] >= 512 and total["builds"] > 0 and dl["fast_rows"] > 0, (total, dl)
    assert np.array_equal(b.bits(b.launch(ntcrypto.NT_MODE_STRICT, be.dev_stream(0, 1))), want)
    assert c.delta() == {"used": 0, "fast_rows": b.rows(), "builds": 0, "old_rows": 0}


def test_tiny_pool_and_switch_off(be, repeated, monkeypatch):
    """NT_KTAB_KEYS=64 in a fresh context: the pool runs out after 64 of the 512 keys, the rest
    stay on the balanced path for good.  NT_KTAB_KEYS=0, per launch and for a whole fresh
    context, gives byte-equal verdict words."""
    import ntcrypto
    b, want = repeated
    monkeypatch.delenv("NT_KTAB_KEYS", raising=False)
    on = b.words(b.launch(ntcrypto.NT_MODE_STRICT, be.dev_stream(0, 0)))
    c = Counters(be)
    monkeypatch.setenv("NT_KTAB_KEYS", "0")
    off = b.words(b.launch(ntcrypto.NT_MODE_STRICT, be.dev_stream(0, 0)))
    assert np.array_equal(on, off)
    assert c.delta() == {"used": 0, "fast_rows": 0, "builds": 0, "old_rows": 0}
    fresh = ntcrypto.Backend(0)  # a context that never has a cache
    try:
        b2 = b.on(fresh)
        assert np.array_equal(b2.words(b2.launch(ntcrypto.NT_MODE_STRICT, fresh.dev_stream(0, 0))), on)
        assert fresh.ktab_info(0)["capacity"] == 0
    finally:
        fresh.close()
    monkeypatch.setenv("NT_KTAB_KEYS", "64")
    tiny = ntcrypto.Backend(0)
    try:
        b3 = b.on(tiny)
        c3 = Counters(tiny)
        for _ in range(4):  # met, built (64 of them), and twice more
            assert np.array_equal(b3.words(b3.launch(ntcrypto.NT_MODE_STRICT, tiny.dev_stream(0, 0))), on)
        info = tiny.ktab_info(0)
        assert info["capacity"] == 64 and info["used"] == 64, info
        dl = c3.delta()
        assert dl["builds"] > 0 and dl["old_rows"] >= 2 * b3.rows(), dl
    finally:
        tiny.close()
