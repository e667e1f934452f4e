"""The verify kernel's key-table cache on the host (tests/cpp/ktab/): the unbalanced
lattice vector (sc25519.hpp sc_unbalanced), the three-table ladder (ktab_tables.hpp
verify_uv3) for every kind of valid vector, and the cache's states -- first sighting
marks, second builds, third hits -- over an index and a pool the test owns and may
corrupt.  A verdict never depends on the cache; only the path does."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import _arith_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "tests", "cpp", "ktab")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
GOLD = os.path.join(ROOT, "tests", "golden")
L = C.L
SEEN, CLAIMED, READY0 = 1, 2, 16
UNDECODABLE, SMALL_ORDER = 1, 2


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", KDIR], check=True)
    h = ctypes.CDLL(os.path.join(BUILD, "libnthost_ktab.so"))
    h.ntk_verify_uv3.restype = ctypes.c_int
    h.ntk_slots.restype = ctypes.c_uint32
    h.ntk_entry_bytes.restype = ctypes.c_int
    h.ntk_candidates.restype = ctypes.c_int
    h.nth_sign.restype = None
    return h


@pytest.fixture(scope="module")
def corpus():
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    return {k: d[k] for k in d.files}


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def words(ks):
    return np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ks), np.uint32).copy()


def unbalanced(lib, ks, lehmer):
    """(u signed, v, ubits, vbits) per scalar from sc_unbalanced_t<lehmer>"""
    n = len(ks)
    k8 = words(ks)
    u8, v8 = np.zeros(8 * n, np.uint32), np.zeros(8 * n, np.uint32)
    neg, ub, vb = np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.ntk_unbalanced(ctypes.c_uint64(n), _vp(k8), _vp(u8), _vp(neg), _vp(v8), _vp(ub), _vp(vb), ctypes.c_int(lehmer))
    ub8, vb8 = u8.tobytes(), v8.tobytes()
    out = []
    for i in range(n):
        u = int.from_bytes(ub8[32 * i:32 * i + 32], "little")
        out.append((-u if neg[i] else u, int.from_bytes(vb8[32 * i:32 * i + 32], "little"), int(ub[i]), int(vb[i])))
    return out


def test_unbalanced_lattice_vector(lib):
    """200 k seeded random scalars and the ~700 edge scalars of the half-size test through the
    2^191.5 stop: u == +-v k (mod 8L) in the sign the function reports (u == v k with u signed),
    v odd, 0 < v < L, the bit lengths never underestimate, and the Lehmer-batched reduction
    equals the one-step loop.  Size: never more than the trivial vector's 32 windows, and 17
    for all but a few per cent."""
    edge = [k for k in C.halfsize_scalars(0)]
    rng = random.Random(20261020)
    ks = edge + [rng.randrange(L) for _ in range(200_000)]
    leh = unbalanced(lib, ks, 1)
    one = unbalanced(lib, ks, 0)
    L8 = 8 * L
    wide = 0
    for k, a, b in zip(ks, leh, one):
        assert a == b, ("lehmer != one-step", hex(k), a, b)
        u, v, ub, vb = a
        assert (u - v * k) % L8 == 0, hex(k)
        assert v % 2 == 1 and 0 < v < L, hex(k)
        assert abs(u).bit_length() <= ub <= 253 and v.bit_length() <= vb <= 253, (hex(k), ub, vb)
        win = max(16, (vb + 5) >> 2, ((ub + 5) >> 2) - 32)  # verify_uv3's window count
        assert win <= 32, (hex(k), ub, vb)
        wide += win > 17
    # 17 windows hold |u| < 2^194 and v < 2^66 while |u| v ~ 8L = 2^255: 5 bits of slack, which the
    # odd-v fix-up's neighbour exceeds after a quotient above ~2^5, i.e. for < 2^-5 of the scalars
    assert wide * 32 <= len(ks), wide


@pytest.mark.parametrize("which", (0, 1, 2), ids=("unbalanced", "balanced", "trivial"))
def test_corpus_through_the_three_table_ladder(lib, corpus, which):
    """All 360 corpus entries, strict and batch rule, through verify_uv3 with the key's tables
    built by ktab_build: the labels (which the oracle tests pin to the oracle) for every kind of
    valid lattice vector."""
    bad = []
    for j in range(len(corpus["pk"])):
        pk, sig = bytes(corpus["pk"][j]), bytes(corpus["sig"][j])
        o, n = int(corpus["off"][j]), int(corpus["len"][j])
        msg = bytes(corpus["msg"][o:o + n])
        for mode, label in ((0, "strict"), (1, "batch_rule")):
            got = lib.ntk_verify_uv3(mode, pk, sig, msg, ctypes.c_uint64(n), which)
            assert got in (0, 1), got
            if bool(got) != bool(corpus[label][j]):
                bad.append((j, label))
    assert not bad, bad


def test_corpus_labels_are_the_oracles(corpus, oracle):
    got = oracle.verify_strict_many(corpus["pk"], corpus["sig"], corpus["msg"], corpus["off"].astype(np.uint64),
                                    corpus["len"].astype(np.uint64)).astype(bool)
    assert np.array_equal(got, corpus["strict"].astype(bool))


class Cache:
    """an index of `slots` words and a pool of `cap` entries, zeroed"""

    def __init__(self, lib, slots, cap):
        self.lib, self.smask, self.cap = lib, slots - 1, cap
        self.eb = lib.ntk_entry_bytes()
        self.slots = np.zeros(slots, np.uint64)
        self.pool = np.zeros(max(cap, 1) * self.eb, np.uint8)
        self.ctl = np.zeros(4, np.uint32)

    def verify(self, mode, pk, sig, msg, off, ln, on=True):
        n = len(pk)
        out = np.zeros(n, np.uint8)
        pk, sig, msg = np.ascontiguousarray(pk), np.ascontiguousarray(sig), np.ascontiguousarray(msg)
        off, ln = np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(ln, np.uint64)
        self.lib.ntk_verify_many(ctypes.c_int(mode), ctypes.c_uint64(n), _vp(pk), _vp(sig), _vp(msg), _vp(off), _vp(ln),
                                 _vp(self.slots) if on else None, ctypes.c_uint32(self.smask), _vp(self.pool),
                                 ctypes.c_uint32(self.cap), _vp(self.ctl), _vp(out))
        return out.astype(bool)

    def counts(self):
        """(entries handed out, fast rows, builds, old-path rows) since the last call"""
        c = tuple(int(x) for x in self.ctl)
        self.ctl[1:] = 0
        return c

    def candidates(self, pk):
        s = (ctypes.c_uint32 * 64)()
        fp = self.lib.ntk_slots(bytes(pk), ctypes.c_uint32(self.smask), s)
        return list(s)[:self.lib.ntk_candidates()], int(fp)

    def state(self, pk):
        """furthest state of the key's slots: 0 none, SEEN, CLAIMED, or READY0 + index"""
        cand, fp = self.candidates(pk)
        st = [int(self.slots[i]) >> 32 for i in cand if int(self.slots[i]) & 0xffffffff == fp and int(self.slots[i]) >> 32]
        return max(st, default=0)


def signed(lib, n, nkeys, seed, corrupt=0.05):
    """n signatures of nkeys seeded keys over short messages, a fraction corrupted"""
    rng = np.random.default_rng(seed)
    seeds = [rng.bytes(32) for _ in range(nkeys)]
    which = rng.integers(0, nkeys, n) if nkeys < n else np.arange(n)
    ln = rng.integers(0, 100, n).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    data = rng.integers(0, 256, int(ln.sum()) + 1, dtype=np.uint8)
    pk, sig = np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8)
    for i in range(n):
        p, s = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
        m = data[int(off[i]):int(off[i] + ln[i])].tobytes()
        lib.nth_sign(seeds[int(which[i])], m, ctypes.c_uint64(len(m)), p, s)
        pk[i], sig[i] = np.frombuffer(p.raw, np.uint8), np.frombuffer(s.raw, np.uint8)
    flip = rng.random(n) < corrupt
    sig[flip, 7] ^= 0x10
    return pk, sig, data, off, ln, flip


def test_random_signatures_against_the_oracle(lib, oracle):
    """4,096 random signatures of 256 keys, 5 % corrupted, three passes through one cache: the
    oracle's verdicts each time, and by the third pass every row is a fast-path row."""
    pk, sig, data, off, ln, flip = signed(lib, 4096, 256, 99)
    want = oracle.verify_strict_many(pk, sig, data, off, ln, nthreads=8).astype(bool)
    assert np.array_equal(want, ~flip)
    c = Cache(lib, 1 << 12, 512)
    for run in range(3):
        assert np.array_equal(c.verify(0, pk, sig, data, off, ln), want), run
    used, fast, builds, old = c.counts()
    assert used == 256 and builds == 256 and fast + old == 3 * 4096 and fast >= 4096
    assert np.array_equal(c.verify(0, pk, sig, data, off, ln), want)
    assert c.counts() == (256, 4096, 0, 0)


def test_states_mark_build_hit(lib, corpus):
    """First sighting marks, second builds, third hits -- for every corpus key, undecodable and
    small-order ones included (header-only / flagged entries are hits too), with the labels as
    verdicts each time; then with the cache off, the same."""
    pk, sig, msg, off, ln = (corpus[k] for k in ("pk", "sig", "msg", "off", "len"))
    first = np.unique(pk, axis=0, return_index=True)[1]  # one signature per distinct key: a sighting each
    first.sort()
    pk, sig, off, ln = pk[first], sig[first], off[first], ln[first]
    n = len(first)
    for mode, label in ((0, "strict"), (1, "batch_rule")):
        want = corpus[label][first].astype(bool)
        c = Cache(lib, 1 << 11, n)
        assert np.array_equal(c.verify(mode, pk, sig, msg, off, ln), want)
        assert c.counts() == (0, 0, 0, n) and all(c.state(k) == SEEN for k in pk)
        assert np.array_equal(c.verify(mode, pk, sig, msg, off, ln), want)
        assert c.counts() == (n, 0, n, n) and all(c.state(k) >= READY0 for k in pk)
        assert np.array_equal(c.verify(mode, pk, sig, msg, off, ln), want)
        assert c.counts() == (n, n, 0, 0)
        assert np.array_equal(c.verify(mode, pk, sig, msg, off, ln, on=False), want)
        assert c.counts() == (n, 0, 0, 0)
        flags = {int(c.pool.view(np.uint32)[(c.state(k) - READY0) * c.eb // 4 + 8]) for k in pk}
        assert {0, UNDECODABLE, SMALL_ORDER} <= flags


def test_wrong_tag_exhausted_pool_crowded_buckets_and_wild_index(lib, oracle):
    pk, sig, data, off, ln, flip = signed(lib, 40, 40, 5, corrupt=0.2)
    want = ~flip
    one = lambda c, i: bool(c.verify(0, pk[i:i + 1], sig[i:i + 1], data, off[i:i + 1], ln[i:i + 1])[0])
    # a ready slot whose entry carries another key's tag: a miss, the old path, the same verdict
    c = Cache(lib, 64, 4)
    for _ in range(3):
        assert one(c, 0) == want[0]
    assert c.counts() == (1, 1, 1, 2)
    c.pool[:32] = pk[1]
    assert one(c, 0) == want[0] and c.counts() == (1, 0, 0, 1)
    cand, fp1 = c.candidates(pk[1])
    c.slots[cand[0]] = fp1 | (READY0 << 32)  # ... and key 1 led to key 0's tables by a forged slot
    c.pool[:32] = pk[0]
    assert one(c, 1) == want[1] and c.counts() == (1, 0, 0, 1)
    # a pool of 2 entries: the third key is never cached, its slot stays SEEN
    c = Cache(lib, 64, 2)
    for _ in range(4):
        for i in range(3):
            assert one(c, i) == want[i]
    assert c.state(pk[2]) == SEEN and c.state(pk[0]) >= READY0 and c.state(pk[1]) >= READY0
    assert c.counts()[0] == 2
    # 40 keys over ONE bucket pair (16 slots): at most 16 find a home, everyone verifies right
    c = Cache(lib, 16, 64)
    for _ in range(3):
        assert np.array_equal(c.verify(0, pk, sig, data, off, ln), want)
    used, fast, builds, old = c.counts()
    homed = sum(c.state(k) != 0 for k in pk)
    assert 8 <= homed <= 16 and all(c.state(k) in (0,) or c.state(k) >= READY0 for k in pk)
    assert used == builds == fast == homed and old == 3 * 40 - homed
    # an index out of range in a slot: bounds-checked, a miss
    c = Cache(lib, 64, 4)
    cand, fp0 = c.candidates(pk[0])
    for wild in (READY0 + 4, READY0 + 5, 0xffffffff):
        c.slots[cand[3]] = fp0 | (wild << 32)
        assert one(c, 0) == want[0] and c.counts() == (0, 0, 0, 1)


def test_protocol_under_threads():
    """Claim / build / publish / probe by 8 threads over one index and a pool smaller than the key
    set (ktab_threads.cpp): plain, and under the thread sanitizer where the host compiler links
    it (a sanitizer that cannot map its shadow memory on this host proves nothing either way:
    only that outcome is passed over; the captured output says which variant ran).  The host
    policy carries the hand-off on acquire loads and release stores of the slot words -- the
    sanitizer does not model fences -- so this checks the ORDER of stores, publication, slot
    loads and pool loads in ktab_build and the probe, not the device's fence instructions."""
    subprocess.run(["make", "-s", "-C", KDIR], check=True)
    r = subprocess.run([os.path.join(BUILD, "ktab_threads")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print("plain:", r.stdout.strip())
    tsan = os.path.join(BUILD, "ktab_threads_tsan")
    if not os.path.exists(tsan):
        print("thread sanitizer: NOT RUN, the host compiler did not link ktab_threads_tsan")
        return
    r = subprocess.run([tsan], capture_output=True, text=True)
    if "unexpected memory mapping" in r.stderr:
        print("thread sanitizer: NOT RUN, its runtime could not map its shadow memory on this host")
        return
    print("thread sanitizer:", r.stdout.strip())
    assert r.returncode == 0 and "WARNING: ThreadSanitizer" not in r.stderr, r.stdout + r.stderr
