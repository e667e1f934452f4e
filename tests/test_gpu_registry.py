"""GPU parity of the key registry (include/ntcrypto.h nt_set_key_cache): the
committee key cache behind the PLAIN entry points the crate binds
(nt_ed25519_verify_strict / nt_ed25519_verify_batch_groups <-
Signature::verify / verify_batch, crypto/src/lib.rs:200-219), keys passed as
raw 32-byte encodings.  Registered keys verify through the key-cache kernel,
the others through the uncached kernel in the same call; the verdicts must be
the corpus labels and the oracle's whichever way each key goes.

Key combs at 16 bits (67 MB per key) where a test registers a few hundred
corpus keys, so that they fit beside everything else.  The kernel's arithmetic
is NOT the same at every width: only the 21-bit reduced-scalar combs -- what a
registry gets by default -- take k as k or k - L and owe a torsion key's
[L](-A) entry.  The test_registry_default_width_* tests below run the registry
with no width override over tests/golden/torsion_votes.npz (votes under
mixed-order and order-8 keys), admissions at growing offsets included."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def corpus():
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture()
def reg(monkeypatch):
    """A fresh context with a registry (16-bit key combs); closed after the test."""
    import ntcrypto
    monkeypatch.setenv("NT_KEYSET_COMB_BITS", "16")
    b = ntcrypto.Backend(device=0)
    b.set_key_cache(1024)
    yield b
    b.close()


def _pack(msgs):
    ln = np.array([len(m) for m in msgs], np.uint64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    return np.frombuffer(b"".join(msgs), np.uint8), off, ln


def _corpus_msg32(c):
    sel = np.nonzero(c["len"] == 32)[0]
    return sel, np.stack([c["msg"][int(c["off"][i]):int(c["off"][i]) + 32] for i in sel])


def test_registry_corpus_all_registered(reg, corpus):
    """Every corpus key offered to the registry: keys that decode are admitted
    (off-curve / non-canonical-garbage keys are refused and stay on the
    uncached path); strict verdicts and the batch rule equal the corpus labels."""
    c = corpus
    uniq = np.unique(c["pk"], axis=0)
    reg.key_cache_add(uniq)
    info = reg.key_cache_info()
    assert info["error"] == 0 and info["pending"] == 0
    assert info["keys"] + info["refused"] == len(uniq) and info["keys"] > 0 and info["comb_bits"] == 16
    got = reg.verify_strict(c["pk"], c["sig"], c["msg"], c["off"], c["len"])
    assert np.array_equal(got, c["strict"].astype(bool))
    i1 = reg.key_cache_info()
    assert i1["hits"] > 0
    sel, msg32 = _corpus_msg32(c)
    gb = reg.verify_batch_groups(c["pk"][sel], c["sig"][sel], np.arange(len(sel), dtype=np.uint64),
                                 np.ones(len(sel), np.uint32), msg32)
    assert np.array_equal(gb, c["batch_rule"][sel].astype(bool))


def test_registry_corpus_half_registered(reg, corpus):
    """Half of the corpus keys registered, the other half not: one call mixes
    both kernels; verdicts equal the labels (strict and batch rule), and the
    per-signature bits of the groups call equal the uncached path's."""
    c = corpus
    uniq = np.unique(c["pk"], axis=0)
    reg.key_cache_add(uniq[::2])
    got = reg.verify_strict(c["pk"], c["sig"], c["msg"], c["off"], c["len"])
    assert np.array_equal(got, c["strict"].astype(bool))
    info = reg.key_cache_info()
    assert info["hits"] > 0 and info["misses"] > 0
    sel, msg32 = _corpus_msg32(c)
    # certificates of 1..7 votes over the corpus' 32-byte entries
    rng = np.random.default_rng(5)
    cnt = []
    left = len(sel)
    while left:
        k = int(min(left, rng.integers(1, 8)))
        cnt.append(k)
        left -= k
    cnt = np.array(cnt, np.uint32)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint64)
    # each group signs one message: use entry i's own message as group g's only where the
    # group holds one vote; otherwise compare with the uncached path on the same inputs
    pk, sig = c["pk"][sel], c["sig"][sel]
    gmsg = msg32[first.astype(np.int64)]
    gb, sb = reg.verify_batch_groups(pk, sig, first, cnt, gmsg, with_sig_bits=True)
    import ntcrypto
    plain = ntcrypto.Backend(device=0)
    try:
        gb2, sb2 = plain.verify_batch_groups(pk, sig, first, cnt, gmsg, with_sig_bits=True)
    finally:
        plain.close()
    assert np.array_equal(gb, gb2) and np.array_equal(sb, sb2)
    one = cnt == 1
    assert np.array_equal(gb[one], c["batch_rule"][sel][first[one].astype(np.int64)].astype(bool))


def test_registry_mixed_certificates_vs_oracle(reg, oracle):
    """A committee of 100, 60 keys registered: 400 certificates of 5-67 votes
    from all 100 (so most certificates mix registered and unregistered keys),
    some votes corrupted, plus strict header signatures; against the oracle."""
    rng = np.random.default_rng(11)
    nk, G = 100, 400
    seeds = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    pks = reg.sign_batch(seeds)
    reg.key_cache_add(pks[:60])
    assert reg.key_cache_info()["keys"] == 60
    digests = rng.integers(0, 256, (G, 32), dtype=np.uint8)
    cnt = rng.integers(5, 68, G).astype(np.uint32)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint64)
    voters = np.concatenate([rng.permutation(nk)[:k] for k in cnt])
    V = len(voters)
    gidx = np.repeat(np.arange(G), cnt)
    msg = digests[gidx].reshape(-1)
    _, vsig = reg.sign_batch(seeds[voters], msg, np.arange(V, dtype=np.uint64) * 32, np.full(V, 32, np.uint64))
    vsig = vsig.copy()
    bad = rng.random(V) < 0.01
    vsig[bad, 50] ^= 4
    vpk = pks[voters]
    gb, sb = reg.verify_batch_groups(vpk, vsig, first, cnt, digests, with_sig_bits=True)
    og, osb = oracle.verify_batch_groups(vpk, vsig, first, cnt, digests, nthreads=8)
    assert np.array_equal(gb, og.astype(bool)) and np.array_equal(sb, osb.astype(bool))
    assert np.array_equal(sb, ~bad)
    want_g = np.array([not bad[int(f):int(f) + int(k)].any() for f, k in zip(first, cnt)])
    assert np.array_equal(gb, want_g)
    # strict: one signature per certificate (the header), registered and unregistered authors
    author = rng.integers(0, nk, G)
    _, hsig = reg.sign_batch(seeds[author], digests.reshape(-1), np.arange(G, dtype=np.uint64) * 32,
                             np.full(G, 32, np.uint64))
    hsig = hsig.copy()
    hsig[::9, 3] ^= 1
    got = reg.verify_strict(pks[author], hsig, digests.reshape(-1), np.arange(G, dtype=np.uint64) * 32,
                            np.full(G, 32, np.uint64))
    want = oracle.verify_strict_many(pks[author], hsig, digests.reshape(-1), np.arange(G, dtype=np.uint64) * 32,
                                     np.full(G, 32, np.uint64), nthreads=8).astype(bool)
    assert np.array_equal(got, want) and got.sum() == G - len(range(0, G, 9))


def test_registry_admits_on_sight(reg):
    """An empty registry: the first call's keys go through the uncached kernel
    and are queued; after nt_key_cache_sync the next call finds all of them.
    Keys that do not decode are refused; the capacity bounds admissions."""
    rng = np.random.default_rng(12)
    nk = 20
    seeds = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    pks, sig = reg.sign_batch(seeds, np.tile(d, nk), np.arange(nk, dtype=np.uint64) * 32, np.full(nk, 32, np.uint64))
    first, cnt = np.zeros(1, np.uint64), np.full(1, nk, np.uint32)
    assert reg.verify_batch_groups(pks, sig, first, cnt, d)[0]
    reg.key_cache_sync()
    info = reg.key_cache_info()
    assert info["keys"] == nk and info["admitted"] == nk
    h0 = info["hits"]
    assert reg.verify_batch_groups(pks, sig, first, cnt, d)[0]
    assert reg.key_cache_info()["hits"] - h0 == nk
    # a key that does not decode (y = 2: not on the curve) is refused, and the call rejects it
    junk = np.zeros((1, 32), np.uint8)
    junk[0, 0] = 2
    assert not reg.verify_batch_groups(junk, sig[:1], first, np.ones(1, np.uint32), d)[0]
    reg.key_cache_sync()
    info = reg.key_cache_info()
    assert info["keys"] == nk and info["refused"] == 1
    # capacity: a registry of 4 keys admits 4
    reg.set_key_cache(4)
    assert reg.verify_batch_groups(pks, sig, first, cnt, d)[0]
    reg.key_cache_sync()
    assert reg.key_cache_info()["keys"] == 4


def test_registry_multi_device_entries(monkeypatch, oracle):
    """Two device entries (the same GPU twice): certificate groups shard over
    both, each entry with its own registry tables; partial registration."""
    import ntcrypto
    monkeypatch.setenv("NT_KEYSET_COMB_BITS", "16")
    b = ntcrypto.Backend(devices=[0, 0])
    try:
        b.set_key_cache(64)
        rng = np.random.default_rng(13)
        nk, G = 40, 300
        seeds = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
        pks = b.sign_batch(seeds)
        b.key_cache_add(pks[:25])
        digests = rng.integers(0, 256, (G, 32), dtype=np.uint8)
        cnt = np.full(G, 27, np.uint32)
        first = (np.arange(G, dtype=np.uint64) * 27)
        voters = np.concatenate([rng.permutation(nk)[:27] for _ in range(G)])
        V = len(voters)
        msg = digests[np.repeat(np.arange(G), 27)].reshape(-1)
        _, vsig = b.sign_batch(seeds[voters], msg, np.arange(V, dtype=np.uint64) * 32, np.full(V, 32, np.uint64))
        vsig = vsig.copy()
        vsig[::101, 10] ^= 8
        gb = b.verify_batch_groups(pks[voters], vsig, first, cnt, digests)
        bad = np.zeros(V, bool)
        bad[::101] = True
        assert np.array_equal(gb, ~bad.reshape(G, 27).any(axis=1))
    finally:
        b.close()


def test_registry_small_call_routing(reg):
    """The calibrated model carries both GPU floors: the
    key-cache floor is below the uncached one, and AUTO routes a lone
    certificate by the floor of the kernel it would run."""
    import math

    import ntcrypto
    T = 16
    reg.set_small_call_path(ntcrypto.NT_SMALL_AUTO, T)
    try:
        m = reg.small_call_model()
        assert m["calibrated"] and 0 < m["gpu_keyset_us"] < m["gpu_verify_us"], m
        rng = np.random.default_rng(14)
        n = 67
        seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        pks, sig = reg.sign_batch(seeds, np.tile(d, n), np.arange(n, dtype=np.uint64) * 32, np.full(n, 32, np.uint64))
        reg.key_cache_add(pks)
        t = min(m["threads"], n)
        cpu = math.ceil(n / t) * m["cpu_verify_us"] + (m["spawn_us"] if t > 1 else 0)
        h0, g0 = reg.call_counts()
        assert reg.verify_batch_groups(pks, sig, np.zeros(1, np.uint64), np.full(1, n, np.uint32), d)[0]
        h1, g1 = reg.call_counts()
        want_host = cpu < m["gpu_keyset_us"]
        assert (h1 - h0, g1 - g0) == ((1, 0) if want_host else (0, 1)), (cpu, m)
    finally:
        reg.set_small_call_path(ntcrypto.NT_SMALL_OFF)


def test_registry_concurrent_calls_during_admission(reg):
    """Four threads call the plain entry points at once while the registry
    admits the committee's keys on sight (the primary's tasks share one context):
    every verdict is the expected one whichever snapshot a call ran with, and
    by the end every decodable key is registered."""
    import threading
    rng = np.random.default_rng(15)
    nk, G, q = 40, 64, 13
    seeds = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    pks = reg.sign_batch(seeds)
    batches = []
    for t in range(4):
        digests = rng.integers(0, 256, (G, 32), dtype=np.uint8)
        voters = np.concatenate([rng.permutation(nk)[:q] for _ in range(G)])
        msg = digests[np.repeat(np.arange(G), q)].reshape(-1)
        _, vsig = reg.sign_batch(seeds[voters], msg, np.arange(G * q, dtype=np.uint64) * 32,
                                 np.full(G * q, 32, np.uint64))
        vsig = vsig.copy()
        bad = rng.random(G * q) < 0.05
        vsig[bad, 5] ^= 1
        want = ~bad.reshape(G, q).any(axis=1)
        batches.append((pks[voters], vsig, digests, want))
    first = np.arange(G, dtype=np.uint64) * q
    cnt = np.full(G, q, np.uint32)
    errors = []

    def work(t):
        try:
            pk, sig, dg, want = batches[t]
            for _ in range(12):
                got = reg.verify_batch_groups(pk, sig, first, cnt, dg)
                if not np.array_equal(got, want):
                    errors.append((t, int((got != want).sum())))
                reg.key_cache_info()
        except Exception as e:  # surfaced below
            errors.append((t, repr(e)))

    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    reg.key_cache_sync()
    info = reg.key_cache_info()
    assert info["keys"] == nk and info["error"] == 0 and info["hits"] > 0, info


# ------------------------------------------------------------------ the registry at its default width
@pytest.fixture(scope="module")
def tv():
    import _torsion_votes as T
    return T.load()


@pytest.fixture(scope="module")
def certs(tv):
    import _torsion_votes as T
    return T.certificates(tv)


@pytest.fixture()
def reg21(monkeypatch):
    """A fresh context with a registry of capacity 16 and no width override:
    21-bit reduced-scalar combs, 1.61 GB per admitted key."""
    import ntcrypto
    monkeypatch.delenv("NT_KEYSET_COMB_BITS", raising=False)
    b = ntcrypto.Backend(device=0)
    b.set_key_cache(16)
    yield b
    b.close()


def _strict_of_keys(b, tv, keys):
    """verify_strict over the entries of these keys: (verdicts, labels, hits and misses the call added)"""
    sel = np.flatnonzero(np.isin(tv["key"], keys))
    i0 = b.key_cache_info()
    got = b.verify_strict(tv["pk"][sel], tv["sig"][sel], tv["msg32"].reshape(-1), tv["off"][sel], tv["len"][sel])
    i1 = b.key_cache_info()
    return got, tv["strict"][sel].astype(bool), i1["hits"] - i0["hits"], i1["misses"] - i0["misses"]


def _plain_calls(b, tv, certs):
    """verify_strict over all entries and verify_batch_groups over the certificates: the three
    result arrays and each call's (hits, misses, signatures)"""
    rows, first, cnt, msg32, _, _ = certs
    i0 = b.key_cache_info()
    st = b.verify_strict(tv["pk"], tv["sig"], tv["msg32"].reshape(-1), tv["off"], tv["len"])
    i1 = b.key_cache_info()
    gb, sb = b.verify_batch_groups(tv["pk"][rows], tv["sig"][rows], first, cnt, msg32, with_sig_bits=True)
    i2 = b.key_cache_info()
    counts = [(i1["hits"] - i0["hits"], i1["misses"] - i0["misses"], len(tv["pk"])),
              (i2["hits"] - i1["hits"], i2["misses"] - i1["misses"], len(rows))]
    return st, gb, sb, counts


def test_registry_default_width_admissions(reg21, tv):
    """Admissions one after another at 1.61 GB per key (registry.cpp build():
    an admission's combs start at words * nk): 5 keys, then 4, then a call
    that also offers a key that does not decode, then the last 3 on sight (a
    groups call that holds them, nt_key_cache_sync).  After every step the
    counters are what the step admitted, the width is 21 bits, and the strict
    verdicts of the entries of EVERY key admitted so far -- through the key
    cache: all hits -- equal the labels: a later admission must not disturb an
    earlier key's comb."""
    keys = tv["keys"]

    def check(step, nkeys, refused):
        info = reg21.key_cache_info()
        print(step, info)
        assert (info["keys"], info["refused"], info["pending"], info["error"], info["comb_bits"]) == \
            (nkeys, refused, 0, 0, 21), (step, info)
        got, want, hits, misses = _strict_of_keys(reg21, tv, np.arange(nkeys))
        assert (hits, misses) == (len(want), 0), (step, hits, misses)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (step, bad[:16].tolist())

    reg21.key_cache_add(keys[:5])
    check("5 keys", 5, 0)
    reg21.key_cache_add(keys[5:9])
    check("then 4", 9, 0)
    junk = np.zeros((1, 32), np.uint8)
    junk[0, 0] = 2                                  # y = 2: not on the curve
    reg21.key_cache_add(np.concatenate([keys[:1], junk, keys[8:9]]))
    check("a key that does not decode", 9, 1)
    sel = np.flatnonzero(tv["key"] >= 9)
    gb = reg21.verify_batch_groups(tv["pk"][sel], tv["sig"][sel], np.arange(len(sel), dtype=np.uint64),
                                   np.ones(len(sel), np.uint32), tv["msg32"][tv["group"][sel]])
    assert np.array_equal(gb, tv["batch_rule"][sel].astype(bool))
    reg21.key_cache_sync()
    check("3 on sight", 12, 1)
    assert reg21.key_cache_info()["admitted"] == 12


def test_registry_default_width_plain_entry_points(reg21, tv, certs):
    """All 12 keys registered, raw keys through the crate's two calls:
    verify_strict over the 480 entries equals `strict`; verify_batch_groups
    over the certificates (65,5xx signatures: the registry path reaches the
    key-grouped, fused launch at 21 bits) equals the AND of `batch_rule` per
    group with signature bits equal to `batch_rule`.  A context with no
    registry gives the same arrays.  Each call's hits and misses add up to its
    signatures (here: all hits)."""
    import ntcrypto
    rows, first, cnt, msg32, want_group, want_sig = certs
    assert len(rows) >= 65536
    reg21.key_cache_add(tv["keys"])
    info = reg21.key_cache_info()
    assert (info["keys"], info["refused"], info["pending"], info["error"], info["comb_bits"]) == (12, 0, 0, 0, 21), info
    st, gb, sb, counts = _plain_calls(reg21, tv, certs)
    print(counts)
    assert np.array_equal(st, tv["strict"].astype(bool)), np.flatnonzero(st != tv["strict"].astype(bool))[:16].tolist()
    assert np.array_equal(sb, want_sig), np.flatnonzero(sb != want_sig)[:16].tolist()
    assert np.array_equal(gb, want_group), np.flatnonzero(gb != want_group)[:16].tolist()
    assert [(h, m) for h, m, _ in counts] == [(n, 0) for _, _, n in counts], counts
    plain = ntcrypto.Backend(device=0)
    try:
        st2, gb2, sb2, counts2 = _plain_calls(plain, tv, certs)
    finally:
        plain.close()
    assert np.array_equal(st, st2) and np.array_equal(gb, gb2) and np.array_equal(sb, sb2)
    assert all(h == 0 and m == 0 for h, m, _ in counts2)


def test_registry_default_width_half_registered(monkeypatch, tv, certs):
    """Only the even-numbered keys registered (four mixed-order keys, one of
    order 8, one control) in a registry whose capacity is their number, so the
    others can never be admitted: every call mixes the key-cache kernel at 21
    bits with the uncached one.  Same expected arrays; hits and misses both
    positive and adding up to the call's signatures."""
    import ntcrypto
    monkeypatch.delenv("NT_KEYSET_COMB_BITS", raising=False)
    rows, first, cnt, msg32, want_group, want_sig = certs
    even = np.arange(0, len(tv["keys"]), 2)
    b = ntcrypto.Backend(device=0)
    try:
        b.set_key_cache(len(even))
        b.key_cache_add(tv["keys"][even])
        st, gb, sb, counts = _plain_calls(b, tv, certs)
        b.key_cache_sync()
        info = b.key_cache_info()
    finally:
        b.close()
    print(counts, info)
    assert (info["keys"], info["pending"], info["error"], info["comb_bits"]) == (len(even), 0, 0, 21), info
    assert np.array_equal(st, tv["strict"].astype(bool)), np.flatnonzero(st != tv["strict"].astype(bool))[:16].tolist()
    assert np.array_equal(sb, want_sig), np.flatnonzero(sb != want_sig)[:16].tolist()
    assert np.array_equal(gb, want_group), np.flatnonzero(gb != want_group)[:16].tolist()
    for h, m, n in counts:
        assert h > 0 and m > 0 and h + m == n, counts
    assert counts[0][0] == int(np.isin(tv["key"], even).sum())
    assert counts[1][0] == int(np.isin(tv["key"][rows], even).sum())
