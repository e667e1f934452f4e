"""The key-table cache's comb path on the host (tests/cpp/kcomb/): the recoding of the full hash
scalar into 64 signed lookups (ktab_comb.hpp kc_recode / kc_pick), the 33 affine lines that
ktab_build stores for a key, the 15-doubling ladder over them (ladder_kc), the verdicts of
verify_kc and of the whole path (verify_n) with a cold cache, and the stand-alone programs under
the sanitizers."""
import ctypes
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import _arith_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KCDIR = os.path.join(ROOT, "tests", "cpp", "kcomb")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
GOLD = os.path.join(ROOT, "tests", "golden")
P, L = C.P, C.L
ENTRY, HEADER, COMB, LINE = 3968, 128, 4224, 128
UNDECODABLE, SMALL_ORDER = 1, 2
EDGES = [0, 1, 2, 3, L - 1, L - 2, 1 << 252, (1 << 253) - 1, (1 << 253) - 2]


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", KCDIR], check=True)
    h = ctypes.CDLL(os.path.join(BUILD, "libnthost_kcomb.so"))
    for f in ("ntkc_verify", "ntkc_ladder", "ntkc_recode", "ntkc_build", "ntkc_comb_bytes"):
        getattr(h, f).restype = ctypes.c_int
    assert h.ntkc_comb_bytes() == COMB
    return h


@pytest.fixture(scope="module")
def corpus():
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    return {k: d[k] for k in d.files}


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _msg(corpus, j):
    o, n = int(corpus["off"][j]), int(corpus["len"][j])
    return bytes(corpus["msg"][o:o + n])


def corpus_keys(corpus):
    """an honest key, a mixed-order key and a small-order key of the corpus: (kind, encoding, point)"""
    M = C.model()
    out = {}
    for e in dict.fromkeys(bytes(k) for k in corpus["pk"]):
        A = M.decode(e)
        if A is None:
            continue
        kind = "small" if M.is_small(A) else ("mixed" if M.has_torsion(A) else "honest")
        out.setdefault(kind, (e, A))
    assert set(out) == {"honest", "mixed", "small"}, set(out)
    return out


def affine(M, p):
    zi = M.inv(p[2])
    return p[0] * zi % P, p[1] * zi % P


def test_recoding_rebuilds_k_exactly(lib):
    """The 64 (block, index, negate) lookups and c, summed the way the ladder sums them (one
    doubling before every column but the first; a negated entry counts positive, because the
    ladder sums -[K]A over tables of +A): exactly k + c = k | 1 as an integer, c = 1 - (k & 1),
    for the edge scalars and 2,000 seeded random ones."""
    rng = random.Random(20261021)
    out = (ctypes.c_int32 * 192)()
    for k in EDGES + [rng.randrange(L) for _ in range(2000)]:
        c = lib.ntkc_recode(k.to_bytes(32, "little"), out)
        t = list(out)
        acc = 0
        for i in range(64):
            block, index, neg = t[3 * i:3 * i + 3]
            assert 0 <= block < 4 and 0 <= index < 8 and neg in (0, 1), (hex(k), i)
            assert block == i % 4, (hex(k), i)
            if i % 4 == 0 and i:
                acc *= 2
            acc += (1 if neg else -1) * C.entry_scalar(block, index)
        assert c == 1 - (k & 1) and acc == k + c, hex(k)


def _niels(M, pt):
    x, y = affine(M, pt)
    return ((y + x) % P, (y - x) % P, 2 * M.D * x * y % P)


@pytest.mark.parametrize("kind", ("honest", "mixed", "small"))
def test_table_bytes(lib, corpus, kind):
    """Each of the 33 lines, read back from the pool bytes and reduced mod p, is the affine niels
    entry of its point; bytes 120..127 of every line and everything outside the key's 4,224 bytes
    keep the prefill; of the entry pool only the key's 128-byte header is written."""
    M = C.model()
    e, A = corpus_keys(corpus)[kind]
    cap, idx = 3, 1
    pool, comb = np.full(cap * ENTRY, 0xA5, np.uint8), np.full(cap * COMB, 0xA5, np.uint8)
    assert lib.ntkc_build(e, 2, _vp(pool), _vp(comb), ctypes.c_uint32(cap), ctypes.c_uint32(idx)) == 0
    hdr = pool[idx * ENTRY:idx * ENTRY + HEADER]
    assert bytes(hdr[:32]) == e and int(hdr.view(np.uint32)[8]) == (SMALL_ORDER if kind == "small" else 0)
    rest = pool.copy()
    rest[idx * ENTRY:idx * ENTRY + HEADER] = 0xA5
    assert (rest == 0xA5).all()
    assert (comb[:idx * COMB] == 0xA5).all() and (comb[(idx + 1) * COMB:] == 0xA5).all()
    lines = comb[idx * COMB:(idx + 1) * COMB].reshape(33, LINE)
    assert (lines[:, 120:] == 0xA5).all()
    mul = C.Mul(A)
    for n in range(33):
        pt = A if n == 32 else mul(C.entry_scalar(n // 8, n % 8))
        w = lines[n, :120].view(np.uint32).reshape(3, 10)
        got = tuple(C.value([int(v) for v in w[c]]) % P for c in range(3))
        assert got == _niels(M, pt), (kind, n)


def test_null_comb_pool_builds_the_window_tables(lib, corpus):
    """A comb policy with a null comb pool writes what the three-table policy writes, byte for
    byte, and nothing else; an undecodable key gets its header alone under every policy."""
    M = C.model()
    undec = next(bytes(k) for k in corpus["pk"] if M.decode(bytes(k)) is None)
    for e in [v[0] for v in corpus_keys(corpus).values()] + [undec]:
        pools, combs = [], []
        for kind in (0, 1, 2):
            pool, comb = np.full(ENTRY, 0xA5, np.uint8), np.full(COMB, 0xA5, np.uint8)
            assert lib.ntkc_build(e, kind, _vp(pool), _vp(comb), ctypes.c_uint32(1), ctypes.c_uint32(0)) == 0
            pools.append(pool)
            combs.append(comb)
        assert np.array_equal(pools[0], pools[1]) and (combs[0] == 0xA5).all() and (combs[1] == 0xA5).all()
        assert np.array_equal(pools[2][:HEADER], pools[0][:HEADER]) and (pools[2][HEADER:] == 0xA5).all()
        if e == undec:
            assert (combs[2] == 0xA5).all() and int(pools[2].view(np.uint32)[8]) == UNDECODABLE


def ladder_scalars():
    rng = random.Random(20261021)
    ks = EDGES + [x % L for j in range(1, 4) for x in ((1 << (64 * j)) - 1, (1 << (64 * j)) + 1, 1 << (64 * j))]
    return ks + [rng.randrange(L) for _ in range(300)]


@pytest.mark.parametrize("kind", ("honest", "mixed", "small"))
def test_ladder_kc_against_the_point_model(lib, corpus, kind):
    """ladder_kc = [k](-A) for the edge scalars (both parities), the tooth boundaries and seeded
    random k -- as an integer multiple, so also for keys with a torsion component; a lane told
    that its key is dead gets the identity."""
    M = C.model()
    e, A = corpus_keys(corpus)[kind]
    mul = C.Mul(M.pneg(A))
    ks = ladder_scalars()
    assert {k & 1 for k in ks[:9]} == {0, 1}
    out = ctypes.create_string_buffer(32)
    for k in ks:
        flags = lib.ntkc_ladder(e, k.to_bytes(32, "little"), 0, out)
        assert flags == (SMALL_ORDER if kind == "small" else 0), flags
        assert out.raw == M.encode(mul(k)), (kind, hex(k))
    for k in (L - 1, L - 2):
        assert lib.ntkc_ladder(e, k.to_bytes(32, "little"), 1, out) >= 0 and out.raw == M.encode(M.IDENT)


def test_corpus_through_the_comb(lib, corpus):
    """All 360 corpus entries, strict and batch rule, through ktab_build (comb) + verify_kc: the
    labels (which the oracle tests pin to the oracle)."""
    bad = []
    for j in range(len(corpus["pk"])):
        pk, sig, msg = bytes(corpus["pk"][j]), bytes(corpus["sig"][j]), _msg(corpus, j)
        for mode, label in ((0, "strict"), (1, "batch_rule")):
            got = lib.ntkc_verify(mode, pk, sig, msg, ctypes.c_uint64(len(msg)))
            assert got in (0, 1), (j, got)
            if bool(got) != bool(corpus[label][j]):
                bad.append((j, label))
    assert not bad, bad


def test_corpus_through_verify_n_with_a_cold_cache(lib, corpus):
    """The whole corpus through verify_n<MODE, 1> over one cache that starts empty, three passes:
    the labels each time.  The first pass marks, the second builds one comb per distinct key and
    the third runs every row through verify_kc."""
    pk, sig, msg, off, ln = (np.ascontiguousarray(corpus[k]) for k in ("pk", "sig", "msg", "off", "len"))
    off, ln = off.astype(np.uint64), ln.astype(np.uint64)
    n, distinct = len(pk), len(np.unique(pk, axis=0))
    for mode, label in ((0, "strict"), (1, "batch_rule")):
        want = corpus[label].astype(bool)
        slots, ctl = np.zeros(1 << 11, np.uint64), np.zeros(4, np.uint32)
        pool, comb = np.zeros(distinct * ENTRY, np.uint8), np.zeros(distinct * COMB, np.uint8)
        for p in range(3):
            out = np.zeros(n, np.uint8)
            lib.ntkc_verify_many(ctypes.c_int(mode), ctypes.c_uint64(n), _vp(pk), _vp(sig), _vp(msg), _vp(off), _vp(ln),
                                 _vp(slots), ctypes.c_uint32(len(slots) - 1), _vp(pool), ctypes.c_uint32(distinct),
                                 _vp(comb), _vp(ctl), _vp(out))
            assert np.array_equal(out.astype(bool), want), (label, p, np.nonzero(out.astype(bool) != want)[0][:8])
        taken, fast, builds, _old = (int(x) for x in ctl)
        assert taken == distinct and builds == distinct and fast >= n, (taken, fast, builds)
        # the window-table area of every entry is never written
        assert not pool.reshape(distinct, ENTRY)[:, HEADER:].any()


def _corpus_file(corpus, path):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(corpus["pk"])))
        for j in range(len(corpus["pk"])):
            m = _msg(corpus, j)
            f.write(bytes(corpus["pk"][j]) + bytes(corpus["sig"][j]))
            f.write(struct.pack("<BBI", int(bool(corpus["strict"][j])), int(bool(corpus["batch_rule"][j])), len(m)) + m)


def test_corpus_under_the_sanitizers(corpus, tmp_path):
    """The stand-alone program (its own main, -fsanitize=address,undefined, run directly): build
    with a comb pool + verify_kc over the corpus on the host policy."""
    subprocess.run(["make", "-s", "-C", KCDIR], check=True)
    path = tmp_path / "corpus.bin"
    _corpus_file(corpus, path)
    r = subprocess.run([os.path.join(BUILD, "kcomb_asan"), str(path)], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_threads_under_the_thread_sanitizer():
    """The stand-alone program (its own main, -fsanitize=thread, run directly): claim, build,
    publish, probe and verify_kc by 8 threads over one index, one pool and one comb pool."""
    subprocess.run(["make", "-s", "-C", KCDIR], check=True)
    r = subprocess.run([os.path.join(BUILD, "kcomb_threads_tsan")], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, r.stdout + r.stderr
