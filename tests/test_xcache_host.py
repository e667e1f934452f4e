"""The x cache of the verify kernel (ed25519_ops.hpp XCache, ge_frombytes_cached)
on the host: the decompression of a public key with its table slots holding
whatever a stale, colliding or torn entry can be.  A slot is only ever a
candidate: the right x must be taken (the square root skipped), anything else
must be recomputed, and the point handed on -- hence every verdict -- is the same
in all cases (tests/cpp/xcache/nt_xcache_harness.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XDIR = os.path.join(ROOT, "tests", "cpp", "xcache")
GOLD = os.path.join(ROOT, "tests", "golden")
P = 2 ** 255 - 19
KINDS = ("right", "wrong_parity", "other_key", "torn", "zero", "plus_p", "random")


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", XDIR], check=True)
    h = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "build", "libnthost_xcache.so"))
    h.nthx_frombytes.restype = ctypes.c_int
    h.nthx_verify.restype = ctypes.c_int
    return h


def frombytes(lib, pk, tab=None, mask=0):
    """(flags, x, t) of the decompression of pk through table `tab` (uint32 array of 8 (mask + 1)
    words, updated in place; None = no table); flags: 1 decodes, 2 square root skipped, 4 stored"""
    x = ctypes.create_string_buffer(32)
    t = ctypes.create_string_buffer(32)
    p = tab.ctypes.data_as(ctypes.c_void_p) if tab is not None else None
    fl = lib.nthx_frombytes(pk, p, ctypes.c_uint32(mask), x, t)
    return fl, x.raw, t.raw


def table(content32, slots=1):
    return np.tile(np.frombuffer(content32, np.uint32), slots).copy()


@pytest.fixture(scope="module")
def corpus():
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def keys(lib, corpus):
    """(pk, decodes, x) of every distinct corpus key and of 256 seeded random keys, the slow path's"""
    rng = np.random.default_rng(2024)
    pks = [bytes(k) for k in np.unique(corpus["pk"], axis=0)]
    lib.nth_sign.restype = None
    for _ in range(256):
        pk = ctypes.create_string_buffer(32)
        sig = ctypes.create_string_buffer(64)
        lib.nth_sign(rng.bytes(32), b"", ctypes.c_uint64(0), pk, sig)
        pks.append(pk.raw)
    out = []
    for pk in pks:
        fl, x, t = frombytes(lib, pk)
        assert not fl & 6
        out.append((pk, bool(fl & 1), x, t))
    assert sum(1 for k in out if not k[1]) > 0 and sum(1 for k in out if k[1] and k[2] == bytes(32)) > 0
    return out


def slot_content(kind, i, keys, rng):
    """what the table holds when key i is probed; None: the case does not exist for this key"""
    pk, ok, x, _ = keys[i]
    xi = int.from_bytes(x, "little")
    others = [k for k in keys if k[1] and k[2] != bytes(32) and k[0][:31] != pk[:31]]
    other = others[i % len(others)][2]
    if kind == "right":
        return x if ok else None
    if kind == "wrong_parity":
        return ((P - xi) % P).to_bytes(32, "little") if ok and xi else None
    if kind == "other_key":
        return other
    if kind == "torn":
        return (x[:16] if ok else bytes(16)) + other[16:]
    if kind == "zero":
        return bytes(32)
    if kind == "plus_p":
        return (xi + P).to_bytes(32, "little") if ok else None
    return rng.bytes(32)


@pytest.mark.parametrize("kind", KINDS)
def test_slot_contents_hit_only_on_the_right_x(lib, keys, kind):
    """Every decodable key with the right x in its slots skips the square root (x = 0, the keys
    y = +-1, never does); every other content misses; the point handed on is the slow path's in
    every case, and a miss of a decodable key with x != 0 leaves the right x behind."""
    rng = np.random.default_rng(7)
    for slots in (1, 64):
        for i, (pk, ok, x, t) in enumerate(keys):
            c = slot_content(kind, i, keys, rng)
            if c is None:
                continue
            tab = table(c, slots)
            fl, gx, gt = frombytes(lib, pk, tab, slots - 1)
            assert bool(fl & 1) == ok
            if ok:
                assert (gx, gt) == (x, t)
            hit = kind == "right" and x != bytes(32)
            assert bool(fl & 2) == hit, (kind, i, slots)
            assert bool(fl & 4) == (not hit and ok and x != bytes(32)), (kind, i, slots)
            if fl & 4:  # stored: now it hits, from the slot the store chose
                fl2, gx2, gt2 = frombytes(lib, pk, tab, slots - 1)
                assert fl2 == 3 and (gx2, gt2) == (x, t)


def test_stores_fill_both_buckets_before_replacing(lib, keys):
    """A table of 8 slots = 2 buckets and keys whose two buckets differ (they probe all of it): the
    first 8 all find an empty slot -- the emptier bucket's, then the other's -- so all 8 hit
    afterwards; the 9th replaces one."""
    def both(pk):
        s = (ctypes.c_uint32 * 8)()
        lib.nthx_slots(pk, ctypes.c_uint32(7), s)
        assert all(v < 8 for v in s)
        return len(set(s)) == 8
    good = [k for k in keys if k[1] and k[2] != bytes(32) and both(k[0])][:9]
    assert len(good) == 9
    tab = np.zeros(8 * 8, np.uint32)
    for pk, _, x, t in good[:8]:
        assert frombytes(lib, pk, tab, 7)[0] == 5
    for pk, _, x, t in good[:8]:
        assert frombytes(lib, pk, tab, 7) == (3, x, t)
    assert frombytes(lib, good[8][0], tab, 7)[0] == 5
    # (each probe on a copy: a miss would store and replace another key)
    assert sum(frombytes(lib, pk, tab.copy(), 7)[0] == 3 for pk, _, _, _ in good) == 8


@pytest.mark.parametrize("kind", KINDS)
def test_corpus_verdicts_do_not_depend_on_the_table(lib, corpus, keys, kind):
    """All 360 corpus entries (small-order, mixed-order, non-canonical-y, y = +-1, off-curve keys
    among them), strict and cofactorless, with the key's slots holding each kind of content."""
    rng = np.random.default_rng(11)
    index = {k[0]: i for i, k in enumerate(keys)}
    bad = []
    for j in range(len(corpus["pk"])):
        pk, sig = bytes(corpus["pk"][j]), bytes(corpus["sig"][j])
        o, n = int(corpus["off"][j]), int(corpus["len"][j])
        msg = bytes(corpus["msg"][o:o + n])
        c = slot_content(kind, index[pk], keys, rng)
        if c is None:
            c = slot_content("other_key", index[pk], keys, rng)
        for mode, label in ((0, "strict"), (1, "batch_rule")):
            tab = table(c, 4)
            got = lib.nthx_verify(mode, pk, sig, msg, ctypes.c_uint64(n), tab.ctypes.data_as(ctypes.c_void_p),
                                  ctypes.c_uint32(3))
            if bool(got) != bool(corpus[label][j]):
                bad.append((j, label))
    assert not bad, bad
