"""The key-table cache's four-table path on the host (tests/cpp/ktab4/): ktab_build with an
extension pool, the 16-window ladder over the full hash scalar (ktab_tables.hpp ladder_k4), the
check that compares R' = [s]B - [k]A with R's bytes after one inversion (verify_k4,
compare_one), and a policy without an extension, whose bytes and paths stay what they were."""
import ctypes
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import _arith_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4DIR = os.path.join(ROOT, "tests", "cpp", "ktab4")
KDIR = os.path.join(ROOT, "tests", "cpp", "ktab")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
GOLD = os.path.join(ROOT, "tests", "golden")
P, L = C.P, C.L
ENTRY, EXT = 3968, 1280
UNDECODABLE, SMALL_ORDER = 1, 2


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", K4DIR], check=True)
    h = ctypes.CDLL(os.path.join(BUILD, "libnthost_ktab4.so"))
    for f in ("ntk4_verify", "ntk4_ladder", "ntk4_compare", "ntk4_build", "ntk4_ext_bytes"):
        getattr(h, f).restype = ctypes.c_int
    assert h.ntk4_ext_bytes() == EXT
    return h


@pytest.fixture(scope="module")
def lib3():
    """the three-table harness as it is (tests/cpp/ktab/), HostKTab untouched"""
    subprocess.run(["make", "-s", "-C", KDIR], check=True)
    return ctypes.CDLL(os.path.join(BUILD, "libnthost_ktab.so"))


@pytest.fixture(scope="module")
def corpus():
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    return {k: d[k] for k in d.files}


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _msg(corpus, j):
    o, n = int(corpus["off"][j]), int(corpus["len"][j])
    return bytes(corpus["msg"][o:o + n])


def test_corpus_through_four_tables(lib, corpus):
    """All 360 corpus entries, strict and batch rule, through ktab_build (four tables) + verify_k4:
    the labels (which the oracle tests pin to the oracle)."""
    bad = []
    for j in range(len(corpus["pk"])):
        pk, sig, msg = bytes(corpus["pk"][j]), bytes(corpus["sig"][j]), _msg(corpus, j)
        for mode, label in ((0, "strict"), (1, "batch_rule")):
            got = lib.ntk4_verify(mode, pk, sig, msg, ctypes.c_uint64(len(msg)))
            assert got in (0, 1), (j, got)
            if bool(got) != bool(corpus[label][j]):
                bad.append((j, label))
    assert not bad, bad


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


def ladder_scalars():
    nib = lambda d: sum(d << (4 * i) for i in range(64)) % L
    ks = [0, 1, 8, L - 1, 1 << 252, (1 << 252) + (1 << 64) - 1]
    ks += [nib(8), nib(0xf), nib(7)]  # the longest carry chains of the signed recoding
    ks += [x % L for j in range(1, 4) for x in ((1 << (64 * j)) - 1, (1 << (64 * j)) + 1)]  # the string boundaries
    rng = random.Random(20261021)
    return ks + [rng.randrange(L) for _ in range(2000)]


def test_recoding_top_digit_absorbs_the_carry(lib):
    """k < L < 2^253: 64 signed nibbles in [-8, 7] that sum to k, the top one never negative and at
    most 2 -- no carry leaves the 64th digit."""
    out = (ctypes.c_int8 * 64)()
    for k in ladder_scalars() + [L - 1 - i for i in range(64)]:
        lib.ntk4_digits(k.to_bytes(32, "little"), out)
        d = list(out)
        assert all(-8 <= x <= 7 for x in d) and 0 <= d[63] <= 2, (hex(k), d)
        assert sum(x << (4 * i) for i, x in enumerate(d)) == k, hex(k)


@pytest.mark.parametrize("kind", ("honest", "mixed", "small"))
def test_ladder_k4_against_the_point_model(lib, corpus, kind):
    """ladder_k4 = [k](-A) for the edge scalars, the string boundaries and 2,000 seeded random k;
    a lane told that its key is dead gets the identity."""
    M = C.model()
    e, A = corpus_keys(corpus)[kind]
    mul = C.Mul(M.pneg(A))
    assert M.peq(mul(L - 1), M.pmul(L - 1, M.pneg(A)))  # the helper against the model's own multiply
    out = ctypes.create_string_buffer(32)
    for k in ladder_scalars():
        flags = lib.ntk4_ladder(e, k.to_bytes(32, "little"), 0, out)
        assert flags == (SMALL_ORDER if kind == "small" else 0), flags
        assert out.raw == M.encode(mul(k)), (kind, hex(k))
    assert lib.ntk4_ladder(e, (L - 1).to_bytes(32, "little"), 1, out) >= 0 and out.raw == M.encode(M.IDENT)


def compare(lib, mode, pt, R, z=0x1234567 << 200 | 99):
    x, y = pt
    return lib.ntk4_compare(mode, (x % P).to_bytes(32, "little"), (y % P).to_bytes(32, "little"),
                            (z % P).to_bytes(32, "little"), R)


def affine(M, p):
    zi = M.inv(p[2])
    return p[0] * zi % P, p[1] * zi % P


def test_compare_at_function_level(lib):
    """compare_one with a chosen R': its own encoding, the other sign, x = 0 under a set sign bit,
    y + p where that fits in 255 bits, and an R' of small order."""
    M = C.model()
    rng = random.Random(7)
    for _ in range(20):
        Rp = M.pmul(rng.randrange(1, L), M.BASE)
        x, y = affine(M, Rp)
        enc = M.encode(Rp)
        other = bytes(enc[:31]) + bytes([enc[31] ^ 0x80])
        z = rng.randrange(1, P)
        for mode in (0, 1):
            assert compare(lib, mode, (x, y), enc, z) == 1
            assert compare(lib, mode, (x, y), other, z) == 0  # enc(-R'): same y, other sign
            wrong = (int.from_bytes(enc, "little") ^ 2).to_bytes(32, "little")
            assert compare(lib, mode, (x, y), wrong, z) == 0
    # x' = 0: the points (0, 1) and (0, -1); R's sign bit set ("negative zero") is accepted by the
    # cofactorless rule, and both are of small order: strict rejects
    for y in (1, P - 1):
        for sign in (0, 1):
            R = (y | sign << 255).to_bytes(32, "little")
            assert compare(lib, 1, (0, y), R) == 1, (y, sign)
            assert compare(lib, 0, (0, y), R) == 0, (y, sign)
    # y_R = y' + p fits in 255 bits only for y' < 19: the curve points with such y
    seen = 0
    for y in range(19):
        pt = M.decode(y.to_bytes(32, "little"))
        if pt is None:
            continue
        x, _ = affine(M, pt)
        R = ((y + P) | (x & 1) << 255).to_bytes(32, "little")
        assert compare(lib, 1, (x, y), R) == 1, y
        assert compare(lib, 0, (x, y), R) == (0 if M.is_small(pt) else 1), y
        assert compare(lib, 1, (x, y), ((y + P) | ((x & 1) ^ 1) << 255).to_bytes(32, "little")) == (1 if x == 0 else 0), y
        seen += 1
    assert seen >= 2
    # every point of small order: rejected in strict, accepted in cofactorless
    for t in M.TORSION:
        x, y = affine(M, t)
        assert compare(lib, 0, (x, y), M.encode(t)) == 0
        assert compare(lib, 1, (x, y), M.encode(t)) == 1


def test_policy_without_extension_writes_the_same_bytes(lib, lib3, corpus):
    """ktab_build under the three-table policy (HostKTab as it is), under a policy with a null
    extension and under one with an extension: the 3,968-byte entry is byte-equal in all three
    -- and equal to the entry the three-table harness builds on its own second sighting -- a null
    extension stores nothing else, and the fourth table holds j [2^192]A, j = 1..8."""
    M = C.model()
    keys = corpus_keys(corpus)
    undec = next(bytes(k) for k in corpus["pk"] if M.decode(bytes(k)) is None)
    for kind, e in [(k, v[0]) for k, v in keys.items()] + [("undecodable", undec)]:
        pools, exts = [], []
        for build in (0, 1, 2):
            pool, ext = np.full(ENTRY, 0xA5, np.uint8), np.full(EXT, 0xA5, np.uint8)
            assert lib.ntk4_build(e, build, _vp(pool), _vp(ext)) == 0
            pools.append(pool)
            exts.append(ext)
        assert np.array_equal(pools[0], pools[1]) and np.array_equal(pools[0], pools[2]), kind
        assert (exts[0] == 0xA5).all() and (exts[1] == 0xA5).all(), kind
        # the existing harness: one key met twice builds entry 0 of a pool it owns
        slots, pool3, ctl = np.zeros(64, np.uint64), np.full(ENTRY, 0xA5, np.uint8), np.zeros(4, np.uint32)
        idx = next(j for j in range(len(corpus["pk"])) if bytes(corpus["pk"][j]) == e)
        pk, sig = np.ascontiguousarray(corpus["pk"][idx:idx + 1]), np.ascontiguousarray(corpus["sig"][idx:idx + 1])
        off, ln = corpus["off"][idx:idx + 1].astype(np.uint64), corpus["len"][idx:idx + 1].astype(np.uint64)
        out = np.zeros(1, np.uint8)
        for _ in range(2):
            lib3.ntk_verify_many(ctypes.c_int(0), ctypes.c_uint64(1), _vp(pk), _vp(sig), _vp(corpus["msg"]), _vp(off), _vp(ln),
                                 _vp(slots), ctypes.c_uint32(63), _vp(pool3), ctypes.c_uint32(1), _vp(ctl), _vp(out))
        assert ctl[0] == 1 and ctl[2] == 1 and np.array_equal(pool3, pools[0]), kind
        if kind == "undecodable":
            assert (exts[2] == 0xA5).all() and int(pools[0].view(np.uint32)[8]) == UNDECODABLE
            continue
        # the fourth table: cached (Y+X, Y-X, 2Z, 2dT) of j [2^192]A
        base = M.pmul(1 << 192, keys[kind][1])
        acc = M.IDENT
        w = exts[2].view(np.uint32).reshape(8, 4, 10)
        for j in range(8):
            acc = M.padd(acc, base)
            ypx, ymx, z2 = (C.value([int(v) for v in w[j, c]]) % P for c in range(3))
            zi = M.inv(z2)
            x, y = (ypx - ymx) * zi % P, (ypx + ymx) * zi % P
            assert (x, y) == affine(M, acc), (kind, j)


class Cache4:
    """an index, a pool and an extension the test owns (ext=False: a cache without a fourth table)"""

    def __init__(self, lib, slots, cap, ext=True):
        self.lib, self.smask, self.cap = lib, slots - 1, cap
        self.slots = np.zeros(slots, np.uint64)
        self.pool = np.zeros(cap * ENTRY, np.uint8)
        self.ext = np.zeros(cap * EXT, np.uint8) if ext else None
        self.ctl = np.zeros(4, np.uint32)

    def verify(self, mode, pk, sig, msg, off, ln):
        n = len(pk)
        out = np.zeros(n, np.uint8)
        pk, sig, msg = np.ascontiguousarray(pk), np.ascontiguousarray(sig), np.ascontiguousarray(msg)
        off, ln = np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(ln, np.uint64)
        self.lib.ntk4_verify_many(ctypes.c_int(mode), ctypes.c_uint64(n), _vp(pk), _vp(sig), _vp(msg), _vp(off), _vp(ln),
                                  _vp(self.slots), ctypes.c_uint32(self.smask), _vp(self.pool), ctypes.c_uint32(self.cap),
                                  _vp(self.ext) if self.ext is not None else None, _vp(self.ctl), _vp(out))
        return out.astype(bool)

    def counts(self):
        c = tuple(int(x) for x in self.ctl)
        self.ctl[1:] = 0
        return c


def test_states_mark_build_hit_with_and_without_extension(lib, corpus):
    """verify_n over every distinct corpus key: first sighting marks, second builds, third hits
    through verify_k4 -- the labels each time.  A cache with a null extension builds its entries
    too but no row ever takes the fast path (and nothing dereferences the null)."""
    pk, sig, msg, off, ln = (corpus[k] for k in ("pk", "sig", "msg", "off", "len"))
    first = np.unique(pk, axis=0, return_index=True)[1]
    first.sort()
    pk, sig, off, ln = pk[first], sig[first], off[first], ln[first]
    n = len(first)
    for mode, label in ((0, "strict"), (1, "batch_rule")):
        want = corpus[label][first].astype(bool)
        c = Cache4(lib, 1 << 11, n)
        assert np.array_equal(c.verify(mode, pk, sig, msg, off, ln), want) and c.counts() == (0, 0, 0, n)
        assert np.array_equal(c.verify(mode, pk, sig, msg, off, ln), want) and c.counts() == (n, 0, n, n)
        assert np.array_equal(c.verify(mode, pk, sig, msg, off, ln), want) and c.counts() == (n, n, 0, 0)
        c = Cache4(lib, 1 << 11, n, ext=False)
        for want_counts in ((0, 0, 0, n), (n, 0, n, n), (n, 0, 0, n)):
            assert np.array_equal(c.verify(mode, pk, sig, msg, off, ln), want) and c.counts() == want_counts


def test_corpus_under_the_sanitizers(corpus, tmp_path):
    """The stand-alone program (its own main, -fsanitize=address,undefined, run directly): build
    with an extension + verify_k4 over the corpus on the host policy."""
    subprocess.run(["make", "-s", "-C", K4DIR], check=True)
    path = tmp_path / "corpus.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(corpus["pk"])))
        for j in range(len(corpus["pk"])):
            m = _msg(corpus, j)
            f.write(bytes(corpus["pk"][j]) + bytes(corpus["sig"][j]))
            f.write(struct.pack("<BBI", int(bool(corpus["strict"][j])), int(bool(corpus["batch_rule"][j])), len(m)) + m)
    r = subprocess.run([os.path.join(BUILD, "k4_corpus_asan"), str(path)], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
