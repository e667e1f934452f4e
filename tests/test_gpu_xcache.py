"""GPU: the verify kernel's x cache (decompressed public keys kept across calls,
DESIGN.md §5.1) never changes a verdict -- cold, warm, with a table so small that
nearly every store replaces another key, with concurrent writers on the
library's two streams, and switched off."""
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
        self.pk, self.sig, self.msg = up(pk), up(sig), up(msg)
        self.off, self.ln = up(np.asarray(off, np.uint64).view(np.int64)), up(np.asarray(ln, np.uint64).view(np.int64))
        torch.cuda.synchronize(self.dev)

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


def test_corpus_cold_warm_and_tiny_table(be, monkeypatch):
    """The 360-entry corpus (small-order, mixed-order, non-canonical-y, y = +-1 and off-curve keys)
    in one context: cold, warm, and warm through the first 64 slots only -- 324 distinct keys,
    so stores keep replacing other keys' entries, and every index is masked to that size."""
    import ntcrypto
    monkeypatch.delenv("NT_XCACHE_SLOTS", raising=False)
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    b = Batch(be, d["pk"], d["sig"], d["msg"], d["off"], d["len"])
    s = be.dev_stream(0, 0)
    for run in ("cold", "warm", "tiny", "tiny again"):
        if run == "tiny":
            monkeypatch.setenv("NT_XCACHE_SLOTS", "64")
        for mode, label in ((ntcrypto.NT_MODE_STRICT, "strict"), (ntcrypto.NT_MODE_COFACTORLESS, "batch_rule")):
            got = b.bits(b.launch(mode, s))
            assert np.array_equal(got, d[label].astype(bool)), (run, label, np.nonzero(got != d[label].astype(bool))[0])


@pytest.fixture(scope="module")
def repeated(be, oracle):
    """4,096 signatures of 512 distinct keys (every wave mixes repeated keys), 5 % corrupted"""
    rng = np.random.default_rng(4242)
    n, nk = 4096, 512
    seeds = rng.integers(0, 256, (nk, 32), dtype=np.uint8)[rng.integers(0, nk, n)]
    ln = rng.integers(0, 200, n).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    data = rng.integers(0, 256, int(ln.sum()) + 1, dtype=np.uint8)
    pk, sig = be.sign_batch(seeds, data, off, ln)
    assert len(np.unique(pk, axis=0)) == nk
    sig = sig.copy()
    flip = rng.random(n) < 0.05
    sig[flip, 7] ^= 0x10
    want = oracle.verify_strict_many(pk, sig, data, off, ln, nthreads=8).astype(bool)
    assert np.array_equal(want, ~flip)
    return Batch(be, pk, sig, data, off, ln), want


def test_repeated_keys_two_streams_unsynchronised(be, repeated, monkeypatch):
    """Two calls on the library's two streams with nothing between them: both launches probe and
    fill the one table at once.  Then once more, warm."""
    import ntcrypto
    monkeypatch.delenv("NT_XCACHE_SLOTS", raising=False)
    b, want = repeated
    for run in ("cold", "warm"):
        outs = b.outs(2)
        for k in range(2):  # back to back: no synchronisation between the two calls
            b.launch(ntcrypto.NT_MODE_STRICT, be.dev_stream(0, k), outs[k])
        for o in outs:
            assert np.array_equal(b.bits(o), want), run


def test_cache_off_gives_the_same_words(be, repeated, monkeypatch):
    import ntcrypto
    b, want = repeated
    monkeypatch.delenv("NT_XCACHE_SLOTS", raising=False)
    on = b.words(b.launch(ntcrypto.NT_MODE_STRICT, be.dev_stream(0, 0)))
    monkeypatch.setenv("NT_XCACHE_SLOTS", "0")
    off = b.words(b.launch(ntcrypto.NT_MODE_STRICT, be.dev_stream(0, 0)))
    assert np.array_equal(on, off)
    # a context that never had a table
    fresh = ntcrypto.Backend(0)
    try:
        b2 = Batch(fresh, b.pk.cpu().numpy(), b.sig.cpu().numpy(), b.msg.cpu().numpy(),
                   b.off.cpu().numpy().view(np.uint64), b.ln.cpu().numpy().view(np.uint64))
        assert np.array_equal(b2.words(b2.launch(ntcrypto.NT_MODE_STRICT, fresh.dev_stream(0, 0))), on)
        assert np.array_equal(b2.bits(b2.launch(ntcrypto.NT_MODE_STRICT, fresh.dev_stream(0, 1))), want)
    finally:
        fresh.close()
