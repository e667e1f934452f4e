"""GPU: the key-table cache's four-table path: for a key whose tables are cached
the verify kernel computes R' = [s]B - [k]A from four cached tables and compares it with R's
bytes after one inversion -- R is never decompressed.  Verdicts are the oracle's in both modes,
for good and corrupted R, in mixed lane pairs, on later grid-stride passes and with builders
and readers on two streams; every test asserts the kernel's own row counters, so none passes
with the new path idle."""
import os

import numpy as np
import pytest

import _passes as P
from test_gpu_ktab import Batch, Counters

pytestmark = pytest.mark.gpu
ENTRY, EXT = 3968, 1280


@pytest.fixture(scope="module")
def be():
    import ntcrypto
    os.environ.pop("NT_KTAB_KEYS", None)
    b = ntcrypto.Backend(0)
    yield b
    b.close()


def xcache_buckets(pk):
    """the two x-cache buckets of each key in the default table of 2^21 slots (ed25519_ops.hpp
    xcache_hash / xcache_bucket), as (n, 2) bucket numbers"""
    w = np.ascontiguousarray(pk).view(np.uint32).reshape(len(pk), 8).astype(np.uint64)
    out = []
    for seed in (0x9e3779b9, 0x7f4a7c15):
        h = np.full(len(pk), seed, np.uint64)
        for i in range(8):
            h = ((h ^ w[:, i]) * np.uint64(0x85ebca6b)) & np.uint64(0xffffffff)
            h ^= h >> np.uint64(15)
        h = (h * np.uint64(0xc2b2ae35)) & np.uint64(0xffffffff)
        out.append((h ^ (h >> np.uint64(16))) & np.uint64((1 << 19) - 1))
    return np.stack(out, axis=1)


def key_seeds(be, nkeys, rng):
    """nkeys key seeds no two of whose keys share an x-cache bucket.  Two new keys of one wave that
    share a bucket see it empty together and store their x in the same slot; the one overwritten is
    met anew at the next launch and gets its entry one launch later.  That is the x cache's rate on
    such pairs (the parent commit's too) and not what these tests are about: they count launches."""
    cand = rng.integers(0, 256, (nkeys + nkeys // 4 + 8, 32), dtype=np.uint8)
    z = np.zeros(len(cand), np.uint64)
    pk, _ = be.sign_batch(cand, np.zeros(1, np.uint8), z, z)
    taken, keep = set(), []
    for i, (b0, b1) in enumerate(xcache_buckets(pk).tolist()):
        if b0 != b1 and b0 not in taken and b1 not in taken:
            taken |= {b0, b1}
            keep.append(i)
    assert len(keep) >= nkeys
    return cand[keep[:nkeys]]


def sign(be, n, nkeys, seed, msglen=200):
    """n signatures of nkeys seeded keys (every key at least once), none corrupted"""
    rng = np.random.default_rng(seed)
    which = rng.permutation(np.concatenate([np.arange(nkeys), rng.integers(0, nkeys, n - nkeys)])) if nkeys < n else np.arange(n)
    seeds = key_seeds(be, nkeys, rng)[which]
    ln = rng.integers(0, msglen, n).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    data = rng.integers(0, 256, int(ln.sum()) + 1, dtype=np.uint8)
    pk, sig = be.sign_batch(seeds, data, off, ln)
    assert len(np.unique(pk, axis=0)) == min(n, nkeys)
    return pk, sig.copy(), data, off, ln


def expected(oracle, pk, sig, data, off, ln):
    """the oracle's verdicts: (strict, cofactorless)"""
    strict = oracle.verify_strict_many(pk, sig, data, off, ln, nthreads=8).astype(bool)
    cof = np.array([oracle.verify_cofactorless(bytes(pk[i]), bytes(sig[i]), data[int(off[i]):int(off[i] + ln[i])].tobytes())
                    for i in range(len(pk))], bool)
    return strict, cof


def modes():
    import ntcrypto
    return (ntcrypto.NT_MODE_STRICT, 0), (ntcrypto.NT_MODE_COFACTORLESS, 1)


def warm(be, b, launches=3):
    """met, built, hit: after three launches every key of the batch has its entry"""
    import ntcrypto
    for _ in range(launches):
        b.words(b.launch(ntcrypto.NT_MODE_STRICT, be.dev_stream(0, 0)))


@pytest.mark.parametrize("mode", (0, 1), ids=("strict", "cofactorless"))
@pytest.mark.parametrize("n", (1, 65, 513))
def test_small_shapes_three_launches(be, oracle, monkeypatch, n, mode):
    """n = 1, 65 and 513 new keys, a tenth of the signatures corrupted, three launches: the oracle's
    verdicts each time, and on the third every row is a fast row.  The cache holds its extension."""
    monkeypatch.delenv("NT_KTAB_KEYS", raising=False)
    pk, sig, data, off, ln = sign(be, n, n, 1000 + 10 * n + mode)
    flip = np.random.default_rng(n).random(n) < 0.1
    sig[flip, 7] ^= 0x10
    want = expected(oracle, pk, sig, data, off, ln)[mode]
    assert np.array_equal(want, ~flip)
    b = Batch(be, pk, sig, data, off, ln)
    c = Counters(be)
    for launch in range(3):
        assert np.array_equal(b.bits(b.launch(modes()[mode][0], be.dev_stream(0, 0))), want), launch
        dl = c.delta()
    assert dl == {"used": 0, "fast_rows": b.rows(), "builds": 0, "old_rows": 0}, dl
    info = be.ktab_info(0)
    assert info["capacity"] >= n and info["bytes"] >= info["capacity"] * (ENTRY + EXT), info


@pytest.fixture(scope="module")
def cached64(be):
    """64 keys with their entries built, and 1,024 good signatures of them"""
    pk, sig, data, off, ln = sign(be, 1024, 64, 77)
    warm(be, Batch(be, pk, sig, data, off, ln))
    return pk, sig, data, off, ln


def test_lane_pairs_that_mix_paths(be, oracle, cached64, monkeypatch):
    """1,024 signatures: rows 0, 2, 4, ... hold 64 cached keys, rows 1, 3, ... 63 cached keys and one
    never seen -- each lane runs a fast row, then a balanced one.  The oracle's verdicts, half the
    rows on each path."""
    monkeypatch.delenv("NT_KTAB_KEYS", raising=False)
    pk, sig, data, off, ln = (a.copy() for a in cached64)
    fpk, fsig, fdata, foff, fln = sign(be, 8, 8, 78)
    data = np.concatenate([data, fdata])
    for r in range(8):
        i = 64 * (2 * r + 1) + (7 * r + 3) % 64  # one lane of every odd row
        pk[i], sig[i], off[i], ln[i] = fpk[r], fsig[r], foff[r] + len(cached64[2]), fln[r]
    flip = np.random.default_rng(5).random(1024) < 0.1
    sig[flip, 40] ^= 0x04
    b = Batch(be, pk, sig, data, off, ln)
    want = expected(oracle, pk, sig, data, off, ln)
    assert np.array_equal(want[0], ~flip)
    c = Counters(be)
    import ntcrypto
    assert np.array_equal(b.bits(b.launch(ntcrypto.NT_MODE_STRICT, be.dev_stream(0, 0))), want[0])
    assert c.delta() == {"used": 0, "fast_rows": 8, "builds": 0, "old_rows": 8}


def test_corrupted_r_under_cached_keys(be, oracle, cached64, monkeypatch):
    """A tenth of the lanes with R corrupted four ways -- a flipped bit of y, a flipped sign bit, R
    replaced by an off-curve y, R replaced by an encoding of small order -- under cached keys: the
    oracle's verdicts in both modes with no row on the old path, so the byte compare decided them."""
    monkeypatch.delenv("NT_KTAB_KEYS", raising=False)
    pk, sig, data, off, ln = (a.copy() for a in cached64)
    rng = np.random.default_rng(9)
    offcurve = next(e for e in ((y | s << 255).to_bytes(32, "little") for y in range(2, 64) for s in (0, 1))
                    if not oracle.point_decodes(e))
    small = [bytes(oracle.torsion_point(i)) for i in range(8)]
    kinds = np.zeros(1024, int)
    for i in np.nonzero(rng.random(1024) < 0.1)[0]:
        kinds[i] = kind = 1 + int(rng.integers(0, 4))
        if kind == 1:
            sig[i, int(rng.integers(0, 31))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 2:
            sig[i, 31] ^= 0x80
        elif kind == 3:
            sig[i, :32] = np.frombuffer(offcurve, np.uint8)
        else:
            sig[i, :32] = np.frombuffer(small[int(rng.integers(0, 8))], np.uint8)
    assert all((kinds == k).sum() >= 8 for k in range(1, 5))
    want = expected(oracle, pk, sig, data, off, ln)
    assert np.array_equal(want[0], kinds == 0) and np.array_equal(want[1], kinds == 0)
    b = Batch(be, pk, sig, data, off, ln)
    c = Counters(be)
    for m, which in modes():
        assert np.array_equal(b.bits(b.launch(m, be.dev_stream(0, 0))), want[which]), which
        assert c.delta() == {"used": 0, "fast_rows": b.rows(), "builds": 0, "old_rows": 0}


def test_later_grid_stride_passes(oracle):
    """NT_GRID_CUS=2 in a fresh context: 16 blocks, 24,576 signatures of 64 keys, so every block runs
    three passes of its grid-stride loop; warm cache: the oracle's verdicts, all rows fast."""
    import ntcrypto
    c = P.corpus()
    per_slot = P.slot_bytes(c)
    blocks = 2 * P.VERIFY_OCC * 4
    n = 3 * blocks * P.DEV_PER_BLOCK
    with P.context(c, per_slot, blocks, NT_GRID_CUS=2) as be:
        pk, sig, data, off, ln = sign(be, n, 64, 303, msglen=40)
        flip = np.random.default_rng(11).random(n) < 0.05
        sig[flip, 3] ^= 0x20
        want = oracle.verify_strict_many(pk, sig, data, off, ln, nthreads=8).astype(bool)
        assert np.array_equal(want, ~flip) and P.passes(n, P.DEV_PER_BLOCK, blocks) == 3
        b = Batch(be, pk, sig, data, off, ln)
        warm(be, b)
        cnt = Counters(be)
        assert np.array_equal(b.bits(b.launch(ntcrypto.NT_MODE_STRICT, be.dev_stream(0, 0))), want)
        assert cnt.delta() == {"used": 0, "fast_rows": b.rows(), "builds": 0, "old_rows": 0}


def test_two_streams_unsynchronised(be, oracle, monkeypatch):
    """4,096 signatures of 512 new keys, twice per stream on the library's two streams with nothing
    between the four calls, three times over: builders store extension lines while readers probe.
    Then one launch alone, all of whose rows are fast: the extension's lines were covered by the
    same publication as the entry's."""
    import ntcrypto
    monkeypatch.delenv("NT_KTAB_KEYS", raising=False)
    pk, sig, data, off, ln = sign(be, 4096, 512, 909)
    flip = np.random.default_rng(13).random(4096) < 0.05
    sig[flip, 7] ^= 0x10
    want = oracle.verify_strict_many(pk, sig, data, off, ln, nthreads=8).astype(bool)
    assert np.array_equal(want, ~flip)
    b = Batch(be, pk, sig, data, off, ln)
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
    assert total["used"] == 512 and total["builds"] > 0, total
    assert np.array_equal(b.bits(b.launch(ntcrypto.NT_MODE_STRICT, be.dev_stream(0, 1))), want)
    assert c.delta() == {"used": 0, "fast_rows": b.rows(), "builds": 0, "old_rows": 0}
