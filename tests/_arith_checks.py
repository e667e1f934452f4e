"""Edge-case checks of the Ed25519 arithmetic in narwhal-tusk_amd/csrc/*.hpp, each
written once as a function of a *runner* and run twice: on the host build of the
headers (tests/test_host_arith.py, every CPU run) and on the gfx950 build behind
the device probe (tests/test_gpu_device_arith.py).  A runner is a `Runner` over a
library whose bulk entry points share one argument list: `nthb_*` of
tests/cpp/nt_host_harness.cpp or `ntp_*` of tests/cpp/nt_device_probe.hip.

Every comparison is exact: Python integers, hashlib, or the textbook curve model
in tests/golden/make_golden.py.  Item i of a device call runs in wave i // 64,
lane i % 64, which is how the checks below choose what shares a wave.
"""
import ctypes
import functools
import hashlib
import importlib.util
import os
import random

import numpy as np

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
SH = [26, 25] * 5
WEIGHT = [sum(SH[:i]) for i in range(10)]
M26, M25 = (1 << 26) - 1, (1 << 25) - 1
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# largest limbs the formulas in ge25519.hpp can feed into mul/sq (see fe25519.hpp header)
F_MAX = [0xFFFFFB4 + 0x8000000 if i == 0 else (0xFFFFFFC + 0x8000000 if i % 2 == 0 else 0x7FFFFFC + 0x4000000)
         for i in range(10)]                                   # fe_sub4 of (2x reduced) -> f side only
G_MAX = [0x7FFFFDA + 0x4000000 if i == 0 else (0x7FFFFFE + 0x4000000 if i % 2 == 0 else 0x3FFFFFE + 0x2000000 + (1 << 18))
         for i in range(10)]                                   # fe_sub of reduced -> either side
S_MAX = [2 * M26 if i % 2 == 0 else 2 * M25 + (1 << 18) for i in range(10)]  # sum of two reduced -> sq_wide input
# fe_sq contract: even limbs < 2^26.1, odd < 2^25.1 (reduced outputs, d y^2 + 1)
R_MAX = [int(2 ** 26.1) - 1 if i % 2 == 0 else int(2 ** 25.1) - 1 for i in range(10)]


def is_reduced(limbs):
    return all(int(l) <= (M26 if i % 2 == 0 else M25 + (1 << 19)) for i, l in enumerate(limbs))


def rand_limbs(rng, mx):
    return [rng.randint(0, m) for m in mx]


def value(limbs):
    return sum(int(l) << w for l, w in zip(limbs, WEIGHT))


def to_limbs(x):
    out = []
    for s in SH:
        out.append(x & ((1 << s) - 1))
        x >>= s
    return out


@functools.lru_cache(maxsize=None)
def model():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# --------------------------------------------------------------------------
# the runner
# --------------------------------------------------------------------------
def _words(ints, nbytes=32):
    """ints -> (n, nbytes / 4) little-endian uint32"""
    buf = b"".join(int(x).to_bytes(nbytes, "little") for x in ints)
    return np.frombuffer(buf, np.uint32).reshape(len(ints), nbytes // 4).copy()


def _ints(arr):
    """(n, w) uint32 -> ints"""
    raw = np.ascontiguousarray(arr, np.uint32).tobytes()
    w = 4 * arr.shape[1]
    return [int.from_bytes(raw[i:i + w], "little") for i in range(0, len(raw), w)]


def _limbs(rows):
    return np.ascontiguousarray(np.array(rows, dtype=np.uint64).astype(np.uint32).reshape(len(rows), 10))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


ENTRIES = ["fe_mul", "fe_sq", "fe_sq_wide", "fe_carry", "fe_tobytes", "fe_frombytes", "fe_invert", "sc_reduce512",
           "sc_muladd", "sc_mul", "sc_reduce_half", "sc_recode_w4", "sc_is_canonical", "sc_halfsize", "hram",
           "point_checks", "ladder_uv", "sc_unbalanced", "ktab_fill", "ktab_point", "ladder_uv3", "wcomb_build",
           "wcomb_free", "wcomb_entries", "wcomb_guard", "wcomb_digits", "wcomb_acc", "key_comb_sum",
           "kcomb_fill", "kcomb_line", "kc_picks", "ladder_kc", "compare_one", "verify_kc"]

# the probe's key table (tests/cpp/nt_probe_items.hpp, laid out as kernels_common.hpp DevKTab reads it):
# a 128-byte control block (word 0: entries handed out), KT_SLOTS index slots of 8 bytes
# {fingerprint, state}, then `capacity` pool entries of KT_ENTRY_BYTES (a 128-byte header: 8 tag
# words, the flags; 3 tables of 8 cached points of 40 words)
KT_SLOTS, KT_CTL_BYTES, KT_ENTRY_BYTES, KT_HEADER_BYTES, KT_POINT_BYTES = 4096, 128, 3968, 128, 160
KT_POOL_OFF = KT_CTL_BYTES + 8 * KT_SLOTS
KT_SEEN, KT_CLAIMED, KT_READY0, KT_NO_SLOT = 1, 2, 16, 0xffffffff
KT_UNDECODABLE, KT_SMALL_ORDER = 1, 2


def ktab_blob(capacity):
    """an empty key table of `capacity` entries"""
    return np.zeros(KT_POOL_OFF + capacity * KT_ENTRY_BYTES, np.uint8)


# the comb items' table (nt_probe_items.hpp kcomb_probe_bytes): the layout above, then `capacity` combs of
# KC_COMB_BYTES (33 lines of KC_LINE_BYTES: 30 limbs, 8 bytes never written) and KC_GUARD_BYTES that
# nothing may write.  Pool, combs and guard start as KC_FILL, so that every byte a build stores shows.
KC_COMB_BYTES, KC_LINE_BYTES, KC_LINES, KC_SIGNED, KC_GUARD_BYTES, KC_FILL = 4224, 128, 33, 32, 8192, 0xA5


def kcomb_comb_off(capacity):
    return KT_POOL_OFF + capacity * KT_ENTRY_BYTES


def kcomb_blob(capacity):
    """an empty key table of `capacity` entries with a comb pool and the guard behind it"""
    blob = np.full(kcomb_comb_off(capacity) + capacity * KC_COMB_BYTES + KC_GUARD_BYTES, KC_FILL, np.uint8)
    blob[:KT_POOL_OFF] = 0
    return blob


class Runner:
    """Bulk calls into a library of `<prefix><entry>(n, ...)` functions; a nonzero
    return (a hipError_t on the device) raises."""

    def __init__(self, lib, prefix, name):
        self.lib, self.prefix, self.name = lib, prefix, name
        self.waves = prefix == "ntp_"  # 64 consecutive items run in lockstep (the host: one after the other)

    def _call(self, entry, n, *args):
        fn = getattr(self.lib, self.prefix + entry)
        fn.restype = ctypes.c_int
        rc = fn(ctypes.c_uint64(n), *args)
        if rc != 0:
            raise RuntimeError("%s%s returned %d on %s" % (self.prefix, entry, rc, self.name))

    def _fe_op(self, entry, *ins):
        arrs = [_limbs(x) for x in ins]
        n = len(arrs[0])
        out = np.zeros((n, 10), np.uint32)
        self._call(entry, n, *[_p(a) for a in arrs], _p(out))
        return out

    def fe_mul(self, fs, gs):
        return self._fe_op("fe_mul", fs, gs)

    def fe_sq(self, fs):
        return self._fe_op("fe_sq", fs)

    def fe_sq_wide(self, fs):
        return self._fe_op("fe_sq_wide", fs)

    def fe_carry(self, fs):
        return self._fe_op("fe_carry", fs)

    def fe_tobytes(self, fs):
        a = _limbs(fs)
        out = np.zeros((len(a), 8), np.uint32)
        self._call("fe_tobytes", len(a), _p(a), _p(out))
        return _ints(out)

    def fe_frombytes(self, ints):
        a = _words(ints)
        out = np.zeros((len(a), 10), np.uint32)
        self._call("fe_frombytes", len(a), _p(a), _p(out))
        return out

    def fe_invert(self, fs, vt):
        a = _limbs(fs)
        out = np.zeros((len(a), 8), np.uint32)
        self._call("fe_invert", len(a), _p(a), _p(out), ctypes.c_int(int(vt)))
        return _ints(out)

    def _sc_op(self, entry, *ins, nbytes=32):
        arrs = [_words(x, nbytes) for x in ins]
        n = len(arrs[0])
        out = np.zeros((n, 8), np.uint32)
        self._call(entry, n, *[_p(a) for a in arrs], _p(out))
        return out

    def sc_reduce512(self, xs):
        return _ints(self._sc_op("sc_reduce512", xs, nbytes=64))

    def sc_muladd(self, a, b, c):
        return _ints(self._sc_op("sc_muladd", a, b, c))

    def sc_mul(self, a, b):
        return _ints(self._sc_op("sc_mul", a, b))

    def sc_recode_w4(self, xs):
        """64 signed digits per scalar"""
        out = self._sc_op("sc_recode_w4", xs)
        nib = (out[:, :, None] >> (4 * np.arange(8, dtype=np.uint32))[None, None, :]) & 15
        return ((nib.reshape(len(out), 64).astype(np.int64) ^ 8) - 8).tolist()

    def sc_reduce_half(self, ks):
        """(magnitude, negative) per scalar"""
        a = _words(ks)
        out = np.zeros((len(a), 8), np.uint32)
        neg = np.zeros(len(a), np.uint32)
        self._call("sc_reduce_half", len(a), _p(a), _p(out), _p(neg))
        return list(zip(_ints(out), [int(x) for x in neg]))

    def sc_is_canonical(self, xs):
        a = _words(xs)
        out = np.zeros(len(a), np.uint32)
        self._call("sc_is_canonical", len(a), _p(a), _p(out))
        return [int(x) for x in out]

    def sc_halfsize(self, ks, lehmer):
        """(u signed, v, bits, sign word of u) per scalar from sc_halfsize_t<lehmer>"""
        a = _words(ks)
        n = len(a)
        u, v = np.zeros((n, 8), np.uint32), np.zeros((n, 8), np.uint32)
        neg, bits = np.zeros(n, np.uint32), np.zeros(n, np.int32)
        self._call("sc_halfsize", n, _p(a), _p(u), _p(neg), _p(v), _p(bits), ctypes.c_int(int(lehmer)))
        return [(-uu if ng else uu, vv, int(b), int(ng)) for uu, ng, vv, b in zip(_ints(u), neg, _ints(v), bits)]

    def hram(self, Rs, As, buf, offs, lens, fast):
        """k = H(R || A || buf[off : off + len]) mod L per item"""
        r = np.frombuffer(b"".join(Rs), np.uint32).copy()
        a = np.frombuffer(b"".join(As), np.uint32).copy()
        m = np.frombuffer(bytes(buf) + b"\0", np.uint8).copy()
        off, ln = np.array(offs, np.uint64), np.array(lens, np.uint64)
        out = np.zeros((len(offs), 8), np.uint32)
        self._call("hram", len(offs), _p(r), _p(a), _p(m), ctypes.c_uint64(len(buf)), _p(off), _p(ln), _p(out),
                   ctypes.c_int(int(fast)))
        return _ints(out)

    def point_checks(self, encs):
        """(decodes, [8]P == 0 by doublings, torsion-y of the decoded point, torsion_y_words) per encoding"""
        e = np.frombuffer(b"".join(encs), np.uint32).copy()
        out = np.zeros((len(encs), 4), np.uint32)
        self._call("point_checks", len(encs), _p(e), _p(out))
        return [tuple(bool(x) for x in row) for row in out]

    def ladder_uv(self, As, Rs, uvb):
        """encoding of -[u]A - [v]R per item; uvb = (u signed, v, bits) per item"""
        a = np.frombuffer(b"".join(As), np.uint32).copy()
        r = np.frombuffer(b"".join(Rs), np.uint32).copy()
        u = _words([abs(x[0]) for x in uvb])
        neg = np.array([1 if x[0] < 0 else 0 for x in uvb], np.uint32)
        v = _words([x[1] for x in uvb])
        bits = np.array([x[2] for x in uvb], np.int32)
        out = np.zeros((len(uvb), 8), np.uint32)
        self._call("ladder_uv", len(uvb), _p(a), _p(r), _p(u), _p(neg), _p(v), _p(bits), _p(out))
        raw = out.tobytes()
        return [raw[i:i + 32] for i in range(0, len(raw), 32)]

    def sc_unbalanced(self, ks, lehmer):
        """(u signed, v, ubits, vbits) per scalar from sc_unbalanced_t<lehmer>"""
        a = _words(ks)
        n = len(a)
        u, v = np.zeros((n, 8), np.uint32), np.zeros((n, 8), np.uint32)
        neg, ub, vb = np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._call("sc_unbalanced", n, _p(a), _p(u), _p(neg), _p(v), _p(ub), _p(vb), ctypes.c_int(int(lehmer)))
        return [(-uu if ng else uu, vv, int(x), int(y)) for uu, ng, vv, x, y in zip(_ints(u), neg, _ints(v), ub, vb)]

    def ktab_fill(self, keys, blob, capacity):
        """builds the table of each key (probe, take, build) in `blob`; the index slot each item won, or KT_NO_SLOT"""
        a = np.frombuffer(b"".join(keys), np.uint32).copy()
        slot = np.zeros(len(keys), np.uint32)
        self._call("ktab_fill", len(keys), _p(a), _p(blob), ctypes.c_uint32(capacity), _p(slot))
        return [int(x) for x in slot]

    def ktab_point(self, keys, tds, blob, capacity):
        """(entry index or KT_NO_SLOT, tag match, header flags, encoding of the cached point
        tab_load_signed(index, t, d)) per (key, (t, d))"""
        a = np.frombuffer(b"".join(keys), np.uint32).copy()
        td = np.array(tds, np.int32).reshape(len(keys), 2)
        out3, enc = np.zeros((len(keys), 3), np.uint32), np.zeros((len(keys), 8), np.uint32)
        self._call("ktab_point", len(keys), _p(a), _p(td), _p(blob), ctypes.c_uint32(capacity), _p(out3), _p(enc))
        raw = enc.tobytes()
        return [(int(o[0]), int(o[1]), int(o[2]), raw[32 * i:32 * i + 32]) for i, o in enumerate(out3)]

    def ladder_uv3(self, kidx, Rs, vecs, blob, capacity):
        """encoding of -[u]A - [v]R per item through the cached tables of pool entry kidx;
        vecs = (u signed, v, ubits, vbits, dead) per item"""
        ki = np.array(kidx, np.uint32)
        r = np.frombuffer(b"".join(Rs), np.uint32).copy()
        u = _words([abs(x[0]) for x in vecs])
        v = _words([x[1] for x in vecs])
        sc = np.array([[1 if x[0] < 0 else 0, x[2], x[3], x[4]] for x in vecs], np.uint32)
        out = np.zeros((len(vecs), 8), np.uint32)
        self._call("ladder_uv3", len(vecs), _p(ki), _p(r), _p(u), _p(v), _p(sc), _p(blob), ctypes.c_uint32(capacity),
                   _p(out))
        raw = out.tobytes()
        return [raw[i:i + 32] for i in range(0, len(raw), 32)]

    # the key-table cache's comb path, over a kcomb_blob(capacity)
    def kcomb_fill(self, keys, blob, capacity):
        """builds the comb of each key (probe, take, the four-argument ktab_build) in `blob`; the index slot
        each item won, or KT_NO_SLOT"""
        a = np.frombuffer(b"".join(keys), np.uint32).copy()
        slot = np.zeros(len(keys), np.uint32)
        self._call("kcomb_fill", len(keys), _p(a), _p(blob), ctypes.c_uint32(capacity), _p(slot))
        return [int(x) for x in slot]

    def kcomb_line(self, keys, lines, blob, capacity):
        """(entry index or KT_NO_SLOT, tag match, header flags, the 30 limbs comb_load hands out for line
        `line` of the key's comb) per (key, line)"""
        a = np.frombuffer(b"".join(keys), np.uint32).copy()
        ln = np.array(lines, np.uint32)
        out3, limbs = np.zeros((len(keys), 3), np.uint32), np.zeros((len(keys), 30), np.uint32)
        self._call("kcomb_line", len(keys), _p(a), _p(ln), _p(blob), ctypes.c_uint32(capacity), _p(out3), _p(limbs))
        return [(int(o[0]), int(o[1]), int(o[2]), q) for o, q in zip(out3, limbs)]

    def kc_picks(self, ks):
        """per scalar: (the 64 lookups (block, index within the block, negate) in ladder_kc's order, c)"""
        a = _words(ks)
        out = np.zeros((len(a), 65), np.uint32)
        self._call("kc_picks", len(a), _p(a), _p(out))
        return [([((int(w) & 0xff) // 8, (int(w) & 0xff) % 8, int(w) >> 8) for w in row[:64]], int(row[64])) for row in out]

    def ladder_kc(self, kidx, ks, dead, blob, capacity):
        """encoding of ladder_kc's [k](-A) over the comb of pool entry kidx per item (dead: the identity)"""
        ki, dd = np.array(kidx, np.uint32), np.array(dead, np.uint32)
        k = _words(ks)
        out = np.zeros((len(k), 8), np.uint32)
        self._call("ladder_kc", len(k), _p(ki), _p(k), _p(dd), _p(blob), ctypes.c_uint32(capacity), _p(out))
        raw = out.tobytes()
        return [raw[i:i + 32] for i in range(0, len(raw), 32)]

    def compare_one(self, items):
        """compare_one's bit per item (x, y, z, R encoding, mode): R' = (x z : y z : z) against R's bytes;
        mode 0 strict, 1 cofactorless"""
        x, y, z = (_words([it[j] % P for it in items]) for j in range(3))
        r = np.frombuffer(b"".join(it[3] for it in items), np.uint32).copy()
        mode = np.array([it[4] for it in items], np.uint32)
        out = np.zeros(len(items), np.uint32)
        self._call("compare_one", len(items), _p(x), _p(y), _p(z), _p(r), _p(mode), _p(out))
        return [int(b) for b in out]

    def verify_kc(self, items, blob, capacity):
        """verify_kc's bit per item (entry index, header flags, R encoding, s, k, mode) over the combs in
        `blob` and the live comb set's comb of B (16 bits)"""
        ki, kf = (np.array([it[j] for it in items], np.uint32) for j in (0, 1))
        r = np.frombuffer(b"".join(it[2] for it in items), np.uint32).copy()
        s, k = _words([it[3] for it in items]), _words([it[4] for it in items])
        mode = np.array([it[5] for it in items], np.uint32)
        out = np.zeros(len(items), np.uint32)
        self._call("verify_kc", len(items), _p(ki), _p(kf), _p(r), _p(s), _p(k), _p(mode), _p(blob),
                   ctypes.c_uint32(capacity), _p(out))
        return [int(b) for b in out]

    # the wide combs: one comb set is live per library, between wcomb_build and wcomb_free
    def _raw(self, entry, *args):
        fn = getattr(self.lib, self.prefix + entry)
        fn.restype = ctypes.c_int
        rc = fn(*args)
        if rc != 0:
            raise RuntimeError("%s%s returned %d on %s" % (self.prefix, entry, rc, self.name))

    def wcomb_build(self, bits, encs, negate, batch):
        """builds the `bits`-bit combs of the encodings (negate: of the negated points), `batch` keys per
        fill launch; the kKey* word per key"""
        e = np.frombuffer(b"".join(encs), np.uint32).copy()
        meta = np.zeros(len(encs), np.uint32)
        self._raw("wcomb_build", ctypes.c_int(bits), ctypes.c_uint32(len(encs)), _p(e), ctypes.c_int(int(negate)),
                  ctypes.c_uint32(batch), _p(meta))
        return [int(m) for m in meta]

    def wcomb_free(self):
        self._raw("wcomb_free")

    def wcomb_guard(self):
        out = np.zeros(1, np.uint32)
        self._raw("wcomb_guard", _p(out))
        return bool(out[0])

    def wcomb_digits(self, bits, xs):
        """per scalar: (the kPos + 1 signed digits of wcomb_acc's schedule, the number of loads
        wcomb_acc itself issued for it, their (position, index) in order)"""
        a = _words(xs)
        out = np.zeros((len(a), 64), np.uint32)
        self._raw("wcomb_digits", ctypes.c_int(bits), ctypes.c_uint64(len(a)), _p(a), _p(out))
        npos = comb_geom(bits)[0]
        dig = out[:, :npos + 1].astype(np.int32).tolist()
        loads = out[:, 18:18 + 2 * (npos + 1)].reshape(len(a), npos + 1, 2).tolist()
        return [(d, int(r[17]), [tuple(x) for x in ld]) for d, r, ld in zip(dig, out, loads)]

    def wcomb_entries(self, items):
        """(n, 32) words: the 30 limbs WideComb::load hands out for (key, pos, idx) -- idx =
        COMB_CORR: load_corr -- then words 30 and 31 of the entry as they lie in memory"""
        k, p, i = (np.array([it[j] for it in items], np.uint32) for j in range(3))
        out = np.zeros((len(items), 32), np.uint32)
        self._raw("wcomb_entries", ctypes.c_uint64(len(items)), _p(k), _p(p), _p(i), _p(out))
        return out

    def wcomb_acc(self, items):
        """encoding of start + [+-x]P(key) per item (key, x, flags, start encoding); flags bit 0: from the
        identity (start unused), bit 1: neg_all"""
        k = np.array([it[0] for it in items], np.uint32)
        x = _words([it[1] for it in items])
        f = np.array([it[2] for it in items], np.uint32)
        st = np.frombuffer(b"".join(it[3] for it in items), np.uint32).copy()
        out = np.zeros((len(items), 8), np.uint32)
        self._raw("wcomb_acc", ctypes.c_uint64(len(items)), _p(k), _p(x), _p(f), _p(st), _p(out))
        raw = out.tobytes()
        return [raw[i:i + 32] for i in range(0, len(raw), 32)]

    def key_comb_sum(self, items):
        """encoding of [k](-A) as cached_point forms it from the key's comb, per item (key, meta, k)"""
        k = np.array([it[0] for it in items], np.uint32)
        m = np.array([it[1] for it in items], np.uint32)
        x = _words([it[2] for it in items])
        out = np.zeros((len(items), 8), np.uint32)
        self._raw("key_comb_sum", ctypes.c_uint64(len(items)), _p(k), _p(m), _p(x), _p(out))
        raw = out.tobytes()
        return [raw[i:i + 32] for i in range(0, len(raw), 32)]


# --------------------------------------------------------------------------
# field multiply / square at the limb bounds, canonical bytes
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fe_mul_cases():
    rng = random.Random(1)
    cases = [(F_MAX, G_MAX), (F_MAX, F_MAX[:0] + [min(a, b) for a, b in zip(G_MAX, G_MAX)])]
    for _ in range(3000):
        cases.append((rand_limbs(rng, F_MAX), rand_limbs(rng, G_MAX)))
    for k in range(10):  # single-limb maxima
        f = [0] * 10
        f[k] = F_MAX[k]
        cases.append((f, G_MAX))
    for k in range(10):
        g = [0] * 10
        g[k] = G_MAX[k]
        cases.append((F_MAX, g))
    want = [value(f) * value(g) % P for f, g in cases]
    return cases, want


def check_fe_mul_bounds(run):
    """fe_mul at F_MAX x G_MAX, the single-limb maxima of either side and 3,000
    random limb vectors under the bounds: value mod p and a reduced output"""
    cases, want = _fe_mul_cases()
    out = run.fe_mul([c[0] for c in cases], [c[1] for c in cases])
    for (f, g), o, w in zip(cases, out, want):
        assert value(o) % P == w, (run.name, f, g)
        assert is_reduced(o), (run.name, f, g, list(o))


@functools.lru_cache(maxsize=None)
def _fe_sq_cases():
    rng = random.Random(2)
    res = {}
    for name, mx in (("fe_sq", R_MAX), ("fe_sq_wide", S_MAX)):
        cases = [mx] + [rand_limbs(rng, mx) for _ in range(3000)]
        for k in range(10):  # single-limb maxima
            f = [0] * 10
            f[k] = mx[k]
            cases.append(f)
        res[name] = (cases, [value(f) ** 2 % P for f in cases])
    return res


def check_fe_sq_bounds(run):
    """fe_sq at R_MAX and fe_sq_wide at S_MAX, single-limb maxima, 3,000 random each"""
    for name, (cases, want) in _fe_sq_cases().items():
        out = getattr(run, name)(cases)
        for f, o, w in zip(cases, out, want):
            assert value(o) % P == w, (run.name, name, f)
            assert is_reduced(o), (run.name, name, f, list(o))


def check_fe_bytes(run):
    """fe_tobytes is canonical on p, p + 18, 2^255 - 1, ... and on unreduced
    limbs; fe_carry keeps the value and reduces the limbs; fe_frombytes drops bit
    255 and keeps the rest"""
    vals = [0, 1, P - 1, P, P + 1, P + 18, 2 ** 255 - 1, 2 ** 255 - 20, 19, 2 ** 254]
    rng = random.Random(3)
    vals += [rng.randrange(0, 2 ** 255) for _ in range(500)]
    limbs = [to_limbs(v) for v in vals]
    # unreduced limb patterns (carry input) also canonicalize
    limbs += [G_MAX] + [rand_limbs(rng, G_MAX) for _ in range(500)]
    got = run.fe_tobytes(limbs)
    for f, g in zip(limbs, got):
        assert g == value(f) % P, (run.name, f)
    carried = run.fe_carry(limbs)
    for f, c in zip(limbs, carried):
        assert value(c) % P == value(f) % P and is_reduced(c), (run.name, f, list(c))
    enc = vals + [v | (1 << 255) for v in vals[:64]] + [2 ** 256 - 1]
    for e, f in zip(enc, run.fe_frombytes(enc)):
        assert value(f) == e & (2 ** 255 - 1) and is_reduced(f), (run.name, hex(e))


# --------------------------------------------------------------------------
# inversion: chosen wave compositions
# --------------------------------------------------------------------------
N_INV_RANDOM = 32768


@functools.lru_cache(maxsize=None)
def inversion_inputs():
    """(values, z^(p-2) mod p).  Waves of 64 (the list is cut at multiples of 64):
    on the GPU a wave leaves fe_invert_vt's loop only when a = 0 in all of its
    lanes, so a lane that finished early runs further full iterations with a = 0
    -- the zeros and ones beside random values below."""
    rng = random.Random(11)
    rnd = lambda: rng.randrange(P)
    waves = [[0] * 64, [1] * 64,
             [rnd()] + [0] * 63, [0] * 63 + [rnd()],
             [1 if i % 2 == 0 else rnd() for i in range(64)]]
    vals = [v for w in waves for v in w]
    pw = [1 << k for k in range(255)]                      # 2^k in order: 4 waves
    vals += pw + [0] * (-len(pw) % 64)
    pm = [P - (1 << k) for k in range(255)]
    vals += pm + [1] * (-len(pm) % 64)
    nc = [P + s for s in range(19)]                        # non-canonical p + s (reduced-size limbs)
    vals += (nc + [2 ** 255 - 1 - s for s in range(19)] + nc + [rnd() for _ in range(7)])[:64]
    edge = [0, 1, 2, P - 1, (P - 1) // 2, (P + 1) // 2]
    vals += [edge[i // 2 % 6] if i % 2 == 0 else rnd() for i in range(64)]
    # the edge list of the host test
    more = [0, 1, 2, 3, 19, P - 1, P - 2, P + 1, P + 18, 2 ** 254, 2 ** 255 - 20, 2 ** 128, 2 ** 128 - 1,
            (P - 1) // 2, (P + 1) // 2, 2 ** 62, 2 ** 62 - 1, 2 ** 30, 2 ** 31 + 1]
    more += [rng.randrange(1 << rng.randrange(1, 255)) for _ in range(1000)]
    vals += more + [rnd() for _ in range(-len(more) % 64)]
    assert len(vals) % 64 == 0
    vals += [rnd() for _ in range(N_INV_RANDOM)]
    return vals, [pow(v % P, P - 2, P) for v in vals]


def check_inversion(run):
    """fe_invert_vt == z^(p-2) == fe_invert on every input of inversion_inputs()"""
    vals, want = inversion_inputs()
    limbs = [to_limbs(v) for v in vals]
    vt = run.fe_invert(limbs, 1)
    for i, (g, w) in enumerate(zip(vt, want)):
        assert g == w, (run.name, "fe_invert_vt", i // 64, i % 64, hex(vals[i]))
    fermat = run.fe_invert(limbs, 0)
    for i, (g, w) in enumerate(zip(fermat, want)):
        assert g == w, (run.name, "fe_invert", i // 64, i % 64, hex(vals[i]))


# --------------------------------------------------------------------------
# scalars
# --------------------------------------------------------------------------
def check_sc_reduce512(run):
    rng = random.Random(4)
    xs = [rng.randrange(0, 2 ** 512) for _ in range(2000)]
    xs += [x % 2 ** 512 for x in (0, L - 1, L, L + 1, 2 ** 512 - 1, L * (2 ** 259))]
    xs += [2 ** 512 - L, L << 250, (L << 259) - 1, 2 ** 256, 2 ** 256 - 1, 2 ** 252]
    for x, g in zip(xs, run.sc_reduce512(xs)):
        assert g == x % L, (run.name, hex(x))


def check_sc_mul(run):
    """sc_muladd and sc_mul on every combination of the edge operands and 2,000
    random triples, and sc_is_canonical around L"""
    edges = [0, 1, L - 1, L, 2 ** 252, 2 ** 256 - 1]
    rng = random.Random(41)
    tri = [(a, b, c) for a in edges for b in edges for c in edges]
    tri += [tuple(rng.randrange(2 ** 256) for _ in range(3)) for _ in range(1000)]
    tri += [tuple(rng.randrange(L) for _ in range(3)) for _ in range(1000)]
    a, b, c = zip(*tri)
    for (x, y, z), g in zip(tri, run.sc_muladd(a, b, c)):
        assert g == (x * y + z) % L, (run.name, "sc_muladd", hex(x), hex(y), hex(z))
    for (x, y, _), g in zip(tri, run.sc_mul(a, b)):
        assert g == x * y % L, (run.name, "sc_mul", hex(x), hex(y))
    ss = [0, 1, L - 2, L - 1, L, L + 1, 2 ** 252, 2 ** 252 - 1, 2 ** 255, 2 ** 255 - 1, 2 ** 256 - 1, L + 2 ** 255,
          L - 2 ** 32, L + 2 ** 32, L - 2 ** 128, L + 2 ** 128] + [rng.randrange(2 ** 253) for _ in range(200)]
    for s, g in zip(ss, run.sc_is_canonical(ss)):
        assert g == int(s < L), (run.name, "sc_is_canonical", hex(s))


def check_sc_reduce_half(run):
    """k < L -> (|k'|, sign) with k' = k or k - L, |k'| <= (L - 1) / 2, and the
    sign and magnitude reconstruct k mod L"""
    edges = [0, 1, 2, (L - 1) // 2, (L + 1) // 2, (L + 3) // 2, L - 1, L - 2, (1 << 251) - 1, 1 << 251,
             (1 << 251) + 1, (1 << 252) - 1, (L - 3) // 2, 1 << 252, L - (1 << 32), (L - 1) // 2 - (1 << 32),
             (L + 1) // 2 + (1 << 32), (L + 1) // 2 + (1 << 224)]
    rng = random.Random(42)
    ks = edges + [rng.randrange(L) for _ in range(2000)]
    for k, (m, neg) in zip(ks, run.sc_reduce_half(ks)):
        assert neg == int(k > (L - 1) // 2), (run.name, hex(k))
        assert m <= (L - 1) // 2, (run.name, hex(k))
        assert (-m if neg else m) % L == k, (run.name, hex(k))


def check_sc_recode_w4(run):
    """signed radix-16 digits of values of 1 .. 253 bits: every digit but the top
    one in [-8, 8), and the digits sum back to the input"""
    rng = random.Random(43)
    xs = [0]
    for b in range(1, 254):
        xs += [1 << (b - 1), (1 << b) - 1, rng.randrange(1 << (b - 1), 1 << b)]
    xs += [int("8" * n, 16) for n in range(1, 64)] + [int("7" * n, 16) for n in range(1, 64)]
    xs += [L - 1, (L - 1) // 2, 2 ** 253 - 1]
    for x, d in zip(xs, run.sc_recode_w4(xs)):
        assert all(-8 <= t < 8 for t in d), (run.name, hex(x))
        assert sum(t << (4 * i) for i, t in enumerate(d)) == x, (run.name, hex(x), d)
        top = (x.bit_length() + 5) >> 2  # the ladder's window count for bits = bitlen
        assert all(t == 0 for t in d[max(top, 1):]), (run.name, hex(x), d)


# --------------------------------------------------------------------------
# half-size scalars
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def halfsize_scalars(n_random=20000):
    """every structured scalar of the two host half-size tests plus random ones"""
    ks = [L - 1 - i for i in range(64)] + [(1 << 252) + i for i in range(64)] + [(1 << 252) - 1 - i for i in range(64)]
    ks += [0, 1, 2, 3] + [1 << b for b in range(0, 253)] + [(1 << b) - 1 for b in range(1, 253)]
    # k / 8L close to a ratio of consecutive Fibonacci numbers -> long runs of quotient 1
    fa, fb = 1, 1
    while fb < 1 << 126:
        fa, fb = fb, fa + fb
    ks += [(8 * L * fa // fb + d) % L for d in range(-32, 33)]
    # huge first quotients: k tiny relative to 8L, and 8L / k just above an integer
    ks += [(8 * L) // q + d for q in (3, 1 << 20, 1 << 31, (1 << 32) + 1, 1 << 40, 1 << 60) for d in range(-3, 4)]
    L8 = 8 * L
    ks += [0, 1, 2, 7, 8, 9, L - 1, L - 2, L // 2, (L - 1) // 8, 1 << 127, (1 << 127) + 1, 1 << 128,
           (1 << 200) + 12345, (1 << 252) - 1, L - (1 << 126), L8 // 3, L8 // 5]
    ks += [(L8 * j) // (1 << 40) for j in range(1, 6)]
    ks += [(L8 // q) + d for q in (3, 1 << 33, 1 << 70) for d in (-1, 0, 1)]
    ks = [k % L for k in ks]
    rng = random.Random(1234)
    return tuple(ks + [rng.randrange(L) for _ in range(n_random)])


def check_halfsize_properties(ks, res, who):
    """u == v k (mod 8L), v odd, 0 < v < L, bitlen <= bits <= 253"""
    L8 = 8 * L
    for k, (u, v, bits, _) in zip(ks, res):
        assert (u - v * k) % L8 == 0, (who, hex(k))
        assert v % 2 == 1 and 0 < v < L, (who, hex(k))
        assert max(abs(u).bit_length(), v.bit_length()) <= bits <= 253, (who, hex(k), bits)


def check_halfsize(run, euclid):
    """The runner's Lehmer-batched reduction (sc_halfsize_t<true>: on the GPU the
    quotients come from v_rcp_f64 and one correction step) has the lattice
    properties, equals the runner's own one-step loop, and equals `euclid` -- the
    HOST one-step loop on the same scalars -- as sc25519.hpp promises ("lands on
    the same remainder pairs")."""
    ks = halfsize_scalars()
    leh = run.sc_halfsize(ks, 1)
    check_halfsize_properties(ks, leh, run.name + " lehmer")
    one = run.sc_halfsize(ks, 0)
    check_halfsize_properties(ks, one, run.name + " one-step")
    for k, a, b, c in zip(ks, leh, one, euclid):
        assert a == b, (run.name, "lehmer != one-step", hex(k), a, b)
        assert a == c, (run.name, "lehmer != host euclid", hex(k), a, c)


# --------------------------------------------------------------------------
# k = H(R || A || M) mod L at every message alignment
# --------------------------------------------------------------------------
HRAM_LENS = (0, 1, 31, 32, 33, 47, 48, 63, 64, 111, 112, 127, 128, 175, 176, 239, 240, 1000)


def check_hram(run):
    """each length at each of the byte offsets 0 .. 7 of an aligned buffer, through
    the one-block fast path (32-byte messages; other lengths fall through) and the
    general path, against hashlib"""
    rng = random.Random(96)
    buf = bytearray()
    Rs, As, offs, lens, want = [], [], [], [], []
    for n in HRAM_LENS:
        for sh in range(8):
            while len(buf) % 16:
                buf.append(rng.getrandbits(8))
            off = len(buf) + sh
            buf += bytes(rng.getrandbits(8) for _ in range(sh + n))
            R = bytes(rng.getrandbits(8) for _ in range(32))
            A = bytes(rng.getrandbits(8) for _ in range(32))
            Rs.append(R)
            As.append(A)
            offs.append(off)
            lens.append(n)
            want.append(int.from_bytes(hashlib.sha512(R + A + bytes(buf[off:off + n])).digest(), "little") % L)
    for fast in (1, 0):
        got = run.hram(Rs, As, buf, offs, lens, fast)
        for g, w, off, n in zip(got, want, offs, lens):
            assert g == w, (run.name, "fast" if fast else "general", "len", n, "offset", off % 16)


# --------------------------------------------------------------------------
# point decoding and the small-order predicates
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _point_cases():
    M = model()
    encs = list(M.small_order_encodings()) + [M.encode(t) for t in M.TORSION]
    rng = random.Random(5)
    for t in M.TORSION:
        for _ in range(3):
            encs.append(M.encode(M.padd(t, M.pmul(rng.randrange(1, M.L), M.BASE))))
    encs += [M.encode(M.pmul(rng.randrange(1, M.L), M.BASE)) for _ in range(20)]
    encs += list(M.noncanonical_encodings())
    # y values off the curve (decode fails) and their sign-bit twins
    y, bad = 2, []
    while len(bad) < 8:
        e = y.to_bytes(32, "little")
        if M.decode(e) is None:
            bad += [e, (y | 1 << 255).to_bytes(32, "little")]
        y += 1
    encs += bad
    want = []
    for e in encs:
        pt = M.decode(e)
        want.append((pt is not None, None if pt is None else M.is_small(pt)))
    return encs, want


def check_point_checks(run):
    """ge_frombytes_w's verdict and the three small-order predicates against the
    model, on canonical, y + p and negative-zero encodings of the torsion points,
    on mixed-order points T + aB, random points and undecodable encodings"""
    encs, want = _point_cases()
    n_small = 0
    for e, (ok, by_dbl, by_y, by_words), (wok, wsmall) in zip(encs, run.point_checks(encs), want):
        assert ok == wok, (run.name, e.hex())
        if ok:
            assert by_dbl == by_y == by_words == wsmall, (run.name, e.hex(), by_dbl, by_y, by_words)
            n_small += by_y
    assert n_small >= 8


# --------------------------------------------------------------------------
# the joint ladder with lane-mixed window counts
# --------------------------------------------------------------------------
def _bits(u, v):
    return max(abs(u).bit_length(), v.bit_length())


@functools.lru_cache(maxsize=None)
def ladder_cases(halfsize):
    """(A encodings, R encodings, (u, v, bits) per lane, expected encodings) of four
    waves; halfsize(ks) -> (u, v, bits, ...) per scalar (the host reduction)."""
    M = model()
    rng = random.Random(77)
    pt = lambda: M.encode(M.pmul(rng.randrange(1, M.L), M.BASE))
    ks = [rng.randrange(L) for _ in range(256)]
    hs = halfsize(tuple(ks))
    As, Rs, uvb = [], [], []
    tors = [M.encode(t) for t in M.TORSION]
    mixed = [M.encode(M.padd(t, M.pmul(rng.randrange(1, M.L), M.BASE))) for t in M.TORSION[1:]]
    for i in range(256):
        wave, lane = divmod(i, 64)
        k = ks[i]
        A, R, x = pt(), pt(), hs[i][:3]
        if wave in (1, 3) and lane in (0, 17, 63):
            x = (k, 1, 253)  # the trivial vector beside half-size ones: the wave runs 64 windows
        if wave == 2:
            u, v = [(0, 1), (1, 1), (-1, 1), (2 ** 128 - 1, 2 ** 128 - 1), (-(2 ** 127), 1), (k, 1)][lane % 6]
            x = (u, v, _bits(u, v))
        if wave == 3:
            A = (tors + mixed)[lane % 15]
            R = (tors + [M.encode(M.IDENT)])[(lane // 3) % 9]
        As.append(A)
        Rs.append(R)
        uvb.append(x)
    want = []
    for A, R, (u, v, _) in zip(As, Rs, uvb):
        a, r = M.decode(A), M.decode(R)
        ua = M.pmul(abs(u), a if u < 0 else M.pneg(a))
        want.append(M.encode(M.padd(ua, M.pmul(v, M.pneg(r)))))
    return tuple(As), tuple(Rs), tuple(uvb), tuple(want)


def check_ladder(run, halfsize):
    """-[u]A - [v]R per lane equals the model's, in waves whose lanes need
    different window counts (on the GPU every lane runs its wave's maximum: a
    short (u, v) beside a 253-bit one takes leading zero windows)"""
    As, Rs, uvb, want = ladder_cases(halfsize)
    got = run.ladder_uv(As, Rs, uvb)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (run.name, "wave", i // 64, "lane", i % 64, uvb[i])


# --------------------------------------------------------------------------
# the unbalanced lattice vector (sc_unbalanced: the remainder sequence stopped at 2^191.5)
# --------------------------------------------------------------------------
L8 = 8 * L
ISQRT = __import__("math").isqrt
STOP_U = ISQRT(1 << 383)  # floor(2^191.5): sc25519.hpp lat_stop(kLatUnbalanced)


def _euclid(k):
    """(dividend, divisor, quotient) of every step of Euclid on (8L, k)"""
    r0, r1 = L8, k
    while r1:
        q = r0 // r1
        yield r0, r1, q
        r0, r1 = r1, r0 - q * r1


@functools.lru_cache(maxsize=None)
def unbalanced_quotient_scalars():
    """k = floor(8L p / q) +- (2^e + j): the continued fraction of k / 8L follows p / q down to a
    remainder of about 8L / q = 2^(255 - qb), where the perturbation leaves a partial quotient of
    about 2^(255 - 2 qb - e): 2^40, 2^30, 2^20 and (e = 0) 2^125 .. 2^155 with dividends across the
    final stop (2^191.5), the batch threshold (2^196) and the Lehmer stop (2^200)"""
    rng = random.Random(191)
    gcd = __import__("math").gcd
    ks = []
    for qb in range(50, 66):
        for _ in range(2):
            while True:
                q = rng.randrange(1 << qb, 3 << (qb - 1)) | 1
                p = rng.randrange(1, q // 8 - 1) | 1
                if gcd(p, q) == 1:
                    break
            for e in (0, 215 - 2 * qb, 225 - 2 * qb, 235 - 2 * qb):
                if e < 0:
                    continue
                for sign in (1, -1):
                    for j in (0, 1):
                        ks.append(L8 * p // q + sign * ((1 << e) + j))
    assert len(ks) == 512 and all(0 < k < L for k in ks)
    return tuple(ks)


@functools.lru_cache(maxsize=None)
def unbalanced_scalars(n_random=20000):
    """(a) the structured scalars of the half-size check, (b) scalars at the stop and the Lehmer
    stop, (c) huge quotients placed there, (d) Fibonacci ratios (runs of quotient 1 ending
    there), (e) random ones"""
    ks = list(halfsize_scalars(0))
    for b in range(186, 207):
        ks += [(1 << b) - 1, 1 << b, (1 << b) + 1]
    ks += [STOP_U + d for d in range(-2, 3)] + [ISQRT(1 << 399) + d for d in range(-2, 3)]
    ks += [(1 << 200) - 1, (1 << 200) + 1]
    ks += unbalanced_quotient_scalars()
    for top in (62, 66):
        fa, fb = 1, 1
        while fb < 1 << top:
            fa, fb = fb, fa + fb
        ks += [(L8 * fa // fb + d) % L for d in range(-32, 33)]
    rng = random.Random(4321)
    return tuple(ks + [rng.randrange(L) for _ in range(n_random)])


def _bitlens(x):
    """the bit length of |x|; of a value whose leading 48 bits are all ones also the next one
    (the header takes bit lengths from fp64 images, which may round up to the power of two:
    "never underestimates")"""
    x = abs(x)
    n = x.bit_length()
    return {n, n + 1} if (x + (x >> 48)).bit_length() > n else {n}


def _cost3(r, t):
    """what a vector may cost the three-table ladder (sc25519.hpp: bitlen |u| - 128 against bitlen v)"""
    return {max(a - 128, b) for a in _bitlens(r) for b in _bitlens(t)}


@functools.lru_cache(maxsize=None)
def unbalanced_model(k):
    """The vectors (u signed, v) sc_unbalanced may return for k, from Python integers: Euclid on
    (8L, k) with signed cofactors (r_i == t_i k mod 8L) up to the first remainder below 2^191.5;
    (r1, t1) if t1 is odd, else whichever of b0 = (r0, t0) and b2 = b0 - q b1, q = min(floor(r0 /
    r1), 2^32 - 1), costs the three-table ladder fewer windows (b0 on a tie).  More than one
    vector only where the header's fp64 images cannot tell: a remainder within 2^-45 of the
    stop (either side is taken as it falls), a ratio r0 / r1 within 2^-38 of an integer (lat_quot
    rounds down by a 2^-40 margin: q or q - 1).  A vector over 250 bits falls back to (k, 1), and so
    does a sequence of 600 steps (quotients of 2^41 and more before the stop)."""
    out = set()
    r0, r1, t0, t1 = L8, k, 0, 1
    steps = 0  # of the one-step loop: a quotient above 2^32 - 1 is taken in clamped parts
    while True:
        # kLatMaxSteps = 600 gives up on the sequence: (k, 1).  The header's count is this one plus one per
        # quotient that lat_quot's margin splits (ordinary scalars: ~110 steps, none split)
        if steps >= 584:
            out.add((k, 1))
            if steps >= 600:
                return out
        near = abs(r1 - STOP_U) <= (STOP_U >> 45)
        if r1 < STOP_U or near:
            if t1 & 1:
                cand = [(r1 if t1 > 0 else -r1, abs(t1))]
            else:
                cand = []
                qs = [0]
                if r1:
                    q = r0 // r1
                    qs = [min(q, 2 ** 32 - 1)]
                    if q < 2 ** 32 and q > 1 and ((r0 - q * r1) << 38) <= r0:
                        qs.append(q - 1)
                for q in qs:
                    b0, b2 = (r0, t0), (r0 - q * r1, t0 - q * t1)
                    c0, c2 = _cost3(*b0), _cost3(*b2)
                    pick = ([b2] if r1 and min(c2) < max(c0) else []) + ([b0] if not r1 or max(c2) >= min(c0) else [])
                    cand += [(r if t > 0 else -r, abs(t)) for r, t in pick]
            for u, v in cand:
                out.add((k, 1) if max(abs(u).bit_length(), v.bit_length()) > 250 else (u, v))
            if not near:
                return out
        q = r0 // r1
        steps += max(1, -(-q // (2 ** 32 - 1)))
        r0, r1, t0, t1 = r1, r0 - q * r1, t1, t0 - q * t1


def windows3(ubits, vbits):
    """the window count of a lane of the three-table ladder (ktab_tables.hpp ladder_uv3)"""
    return min(64, max(16, (vbits + 5) >> 2, ((ubits + 5) >> 2) - 32))


UNBALANCED_WINDOWS_MAX = 32  # what the default host build keeps on every scalar of unbalanced_scalars()


def check_unbalanced_properties(ks, res, who):
    """u == v k (mod 8L) with u signed as reported, v odd, 0 < v < L, bitlen <= bits <= 253 for
    each of |u| and v, and never more windows than the trivial vector's"""
    for k, (u, v, ub, vb) in zip(ks, res):
        assert (u - v * k) % L8 == 0, (who, hex(k))
        assert v % 2 == 1 and 0 < v < L, (who, hex(k))
        assert abs(u).bit_length() <= ub <= 253 and v.bit_length() <= vb <= 253, (who, hex(k), ub, vb)
        w = max(16, (vb + 5) >> 2, ((ub + 5) >> 2) - 32)
        assert w <= UNBALANCED_WINDOWS_MAX, (who, hex(k), ub, vb, w)


def check_unbalanced(run, euclid):
    """sc_unbalanced_t<true> of the runner (on the GPU: quotients from v_rcp_f64) has the lattice
    properties, equals the runner's own one-step loop and `euclid` -- the default HOST build's
    one-step loop on the same scalars -- and is the vector the integer model allows: the
    remainder pair at 2^191.5 and, for an even cofactor, the cheaper neighbour."""
    # the construction has not decayed: a quotient >= 2^12 whose dividend (about 8L / q) lies in
    # 2^190 .. 2^208 -- for qb = 65 (32 of the 512) in 2^189.4 .. 2^190, below the stop already:
    # there it is the fix-up's quotient
    in_range = 0
    for k in unbalanced_quotient_scalars():
        big = [r0 for r0, _, q in _euclid(k) if q >= 1 << 12 and 1 << 189 <= r0 < 1 << 208]
        assert big, hex(k)
        in_range += any(r0 >= 1 << 190 for r0 in big)
    assert in_range >= 480, in_range
    ks = unbalanced_scalars()
    leh = run.sc_unbalanced(ks, 1)
    check_unbalanced_properties(ks, leh, run.name + " lehmer")
    one = run.sc_unbalanced(ks, 0)
    check_unbalanced_properties(ks, one, run.name + " one-step")
    for k, a, b, c in zip(ks, leh, one, euclid):
        assert a == b, (run.name, "lehmer != one-step", hex(k), a, b)
        assert a == c, (run.name, "lehmer != host euclid", hex(k), a, c)
        assert a[:2] in unbalanced_model(k), (run.name, "not the model's vector", hex(k), a)


# --------------------------------------------------------------------------
# the key-table cache: index, pool and the cached window tables
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ktab_keys():
    """(encodings in lane order, kind per encoding).  One random key on lanes 0 .. 4 of wave 0 (one
    CAS winner, one entry), 23 more random points, the 8 torsion points (y = 1 and y = -1, x = 0,
    among them), 7 mixed-order points T + aB, the non-canonical encodings of the model (y + p,
    negative zero) and 8 undecodable encodings: two waves."""
    M = model()
    rng = random.Random(55)
    rnd = [M.encode(M.pmul(rng.randrange(1, M.L), M.BASE)) for _ in range(24)]
    keys = [(rnd[0], "random")] * 5 + [(e, "random") for e in rnd[1:]]
    keys += [(M.encode(t), "torsion") for t in M.TORSION]
    keys += [(M.encode(M.padd(t, M.pmul(rng.randrange(1, M.L), M.BASE))), "mixed") for t in M.TORSION[1:]]
    keys += [(e, "noncanonical") for e in M.noncanonical_encodings()]
    y = 2
    while sum(kind == "undecodable" for _, kind in keys) < 8:
        e = (y | (y & 1) << 255).to_bytes(32, "little")
        if M.decode(e) is None:
            keys.append((e, "undecodable"))
        y += 1
    assert 64 < len(keys) <= 128 and len(set(e for e, _ in keys)) == len(keys) - 4
    assert M.encode(M.IDENT) in [e for e, _ in keys] and (P - 1).to_bytes(32, "little") in [e for e, _ in keys]
    return tuple(e for e, _ in keys), tuple(kind for _, kind in keys)


@functools.lru_cache(maxsize=None)
def ktab_expected():
    """per distinct key: None (undecodable) or (is_small, {(t, d): encode(d [2^(64 t)]A)}), d = -8 .. 8"""
    M = model()
    want = {}
    for e in dict.fromkeys(ktab_keys()[0]):
        A = M.decode(e)
        if A is None:
            want[e] = None
            continue
        tab = {}
        for t in range(3):
            base = M.pmul(1 << (64 * t), A)
            acc = M.IDENT
            tab[(t, 0)] = M.encode(M.IDENT)
            for d in range(1, 9):
                acc = M.padd(acc, base)
                tab[(t, d)], tab[(t, -d)] = M.encode(acc), M.encode(M.pneg(acc))
        want[e] = (M.is_small(A), tab)
    return want


KT_CAPACITY = 128


def _slot_state(blob, slot):
    return int(blob[KT_CTL_BYTES:KT_POOL_OFF].view(np.uint64)[slot]) >> 32


def ktab_filled(run):
    """the runner's table of ktab_keys(), filled once by one ktab_fill call: (blob, slots won,
    entry index per key).  Kept on the runner: check_ktab_tables and check_ladder3 read the same table."""
    if not hasattr(run, "_ktab"):
        keys, _ = ktab_keys()
        blob = ktab_blob(KT_CAPACITY)
        slots = run.ktab_fill(keys, blob, KT_CAPACITY)
        seen = run.ktab_point(keys, [(0, 1)] * len(keys), blob, KT_CAPACITY)  # a second call: a second launch
        run._ktab = (blob, slots, {k: s[0] for k, s in zip(keys, seen)})
    return run._ktab


def check_ktab_tables(run):
    """ktab_probe / ktab_take / ktab_build over the runner's key table, then what a reader finds:
    one entry per distinct key, every key ready with its tag and the model's flags, and every
    cached point -- through tab_load_signed and straight from the pool's bytes -- the model's
    d [2^(64 t)]A.  Then a pool of 4 entries: 4 entries, nothing past them, losers left as seen."""
    keys, kinds = ktab_keys()
    want = ktab_expected()
    distinct = list(want)
    blob, slots, idx_of = ktab_filled(run)
    assert int(blob[:4].view(np.uint32)[0]) == len(distinct), (run.name, "pool used")
    for k in distinct:  # one CAS winner per key, and its slot names the entry
        won = [s for kk, s in zip(keys, slots) if kk == k and s != KT_NO_SLOT]
        assert len(won) == 1 and won[0] < KT_SLOTS, (run.name, k.hex(), won)
        assert _slot_state(blob, won[0]) == KT_READY0 + idx_of[k], (run.name, k.hex())
    assert sorted(idx_of[k] for k in distinct) == list(range(len(distinct))), (run.name, "entry indices")
    items = [(k, (t, d)) for k in distinct for t in range(3) for d in range(-8, 9)]
    got = run.ktab_point([k for k, _ in items], [td for _, td in items], blob, KT_CAPACITY)
    n_small = n_dead = 0
    for (k, td), (idx, same, flags, enc) in zip(items, got):
        assert idx == idx_of[k] and same == 1, (run.name, k.hex(), td, idx, same)
        if want[k] is None:
            assert flags == KT_UNDECODABLE, (run.name, k.hex(), flags)
            n_dead += 1
            continue
        small, tab = want[k]
        assert flags == (KT_SMALL_ORDER if small else 0), (run.name, k.hex(), flags)
        n_small += small
        assert enc == tab[td], (run.name, k.hex(), "table", td[0], "digit", td[1])
    assert n_small >= 8 * 51 and n_dead == 8 * 51
    # the pool's bytes: point j of table t sits at entry + 128 + (8 t + j - 1) 160 as (Y+X, Y-X, 2Z, 2dT)
    pool = blob[KT_POOL_OFF:].view(np.uint32)
    for k in distinct:
        e0 = idx_of[k] * KT_ENTRY_BYTES // 4
        assert pool[e0:e0 + 8].tobytes() == k, (run.name, k.hex(), "tag")
        if want[k] is None:
            continue
        for t in range(3):
            for j in range(1, 9):
                w = pool[e0 + KT_HEADER_BYTES // 4 + (8 * t + j - 1) * 40:][:40]
                ypx, ymx, z2 = value(w[:10]), value(w[10:20]), value(w[20:30])
                zi = pow(z2, P - 2, P)
                x, y = (ypx - ymx) * zi % P, (ypx + ymx) * zi % P
                assert (y | (x & 1) << 255).to_bytes(32, "little") == want[k][1][(t, j)], (run.name, k.hex(), t, j)
                assert (value(w[30:]) * z2 - model().D * (ypx * ypx - ymx * ymx)) % P == 0, (run.name, k.hex(), t, j)
    # a pool of 4 entries, the keys again in a fresh table
    cap = 4
    blob4 = ktab_blob(cap)
    slots4 = run.ktab_fill(keys, blob4, cap)
    seen = run.ktab_point(keys, [(0, 1)] * len(keys), blob4, cap)
    ready = {k: s[0] for k, s in zip(keys, seen) if s[0] != KT_NO_SLOT}
    assert sorted(ready.values()) == list(range(cap)), (run.name, sorted(ready.values()))
    for k, s, (idx, same, _, enc) in zip(keys, slots4, seen):
        if idx != KT_NO_SLOT:
            assert idx < cap and same == 1, (run.name, k.hex(), idx)
            assert want[k] is None or enc == want[k][1][(0, 1)], (run.name, k.hex())
        elif s != KT_NO_SLOT:  # a loser that had won a slot: seen for good
            assert _slot_state(blob4, s) == KT_SEEN, (run.name, k.hex(), _slot_state(blob4, s))
    states = blob4[KT_CTL_BYTES:KT_POOL_OFF].view(np.uint64) >> np.uint64(32)
    assert sorted(int(s) for s in states[states >= KT_READY0]) == [KT_READY0 + i for i in range(cap)], run.name
    assert not np.any(states == KT_CLAIMED), (run.name, "a slot left claimed")


# --------------------------------------------------------------------------
# the three-table ladder with lane-mixed window counts
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ladder3_cases(unbalanced, halfsize):
    """(A encodings, R encodings, (u, v, ubits, vbits, dead) per lane, expected encodings) of
    five waves; unbalanced(ks) -> (u, v, ubits, vbits), halfsize(ks) -> (u, v, bits, ...) per
    scalar: the HOST reductions."""
    M = model()
    keys, kinds = ktab_keys()
    of = lambda kind: [k for k, x in dict(zip(keys, kinds)).items() if x == kind]
    # the seed: wave 0 gets three lanes of 18 windows (1.2 % of random scalars) beside 17s, and the
    # balanced vectors of wave 1 are 127 or 128 bits long (33 windows)
    rng = random.Random(76)
    pt = lambda: M.encode(M.pmul(rng.randrange(1, M.L), M.BASE))
    ks = [rng.randrange(L) for _ in range(320)]
    ub = unbalanced(tuple(ks))
    hs = halfsize(tuple(ks))
    win = [windows3(x[2], x[3]) for x in ub]
    # wave 0 mixes 17-window lanes with longer ones
    assert sum(w >= 18 for w in win[:64]) >= 3 and sum(w == 17 for w in win[:64]) >= 32, win[:64]
    hand_u = [0] + [s * m for m in ((1 << 64) - 1, 1 << 64, (1 << 128) - 1, 1 << 128, (1 << 192) - 1, (1 << 194) - 1, 1)
                    for s in (1, -1)]
    hand_u += [int(c * n, 16) for c in "87f" for n in (16, 17, 32, 33, 48)]
    hand_v = [1, (1 << 64) - 1, (1 << 66) - 1, (1 << 128) - 1]
    tors = [M.encode(t) for t in M.TORSION]
    As, Rs, vecs = [], [], []
    for i in range(320):
        wave, lane = divmod(i, 64)
        A, R, x = of("random")[i % 24], pt(), ub[i] + (0,)
        if wave == 1 and lane in (0, 17, 63):
            x = (ks[i], 1, 253, 1, 0)                    # the trivial vector: 32 windows
        if wave == 1 and lane in (5, 40):
            x = (hs[i][0], hs[i][1], hs[i][2], hs[i][2], 0)  # the balanced vector: 33 windows
            assert windows3(x[2], x[3]) == 33, x
        if wave == 2:
            u, v = hand_u[lane % len(hand_u)], hand_v[(lane // len(hand_u) + lane) % 4]
            if lane == 63:
                u, v = L - 1, L - 2                      # the upper clamp: 64 windows
            x = (u, v, abs(u).bit_length(), v.bit_length(), 0)
        if wave == 3:
            A = (tors + of("mixed"))[lane % 15]
            R = (tors + [M.encode(M.IDENT)])[(lane // 3) % 9]
        if wave == 4:
            A, x = of("undecodable")[lane % 8], x[:4] + (1,)
        As.append(A)
        Rs.append(R)
        vecs.append(x)
    assert windows3(*vecs[64][2:4]) == 32 and windows3(*vecs[191][2:4]) == 64
    assert {u < 0 for u, *_ in vecs[192:256]} == {True, False}
    want = []
    for A, R, (u, v, _, _, dead) in zip(As, Rs, vecs):
        r = M.pmul(v, M.pneg(M.decode(R)))
        if not dead:
            a = M.decode(A)
            r = M.padd(M.pmul(abs(u), a if u < 0 else M.pneg(a)), r)
        want.append(M.encode(r))
    return tuple(As), tuple(Rs), tuple(vecs), tuple(want)


def check_ladder3(run, unbalanced, halfsize):
    """-[u]A - [v]R per lane through the key's three cached tables (ladder_uv3: recoding, window
    rule, wave_max, ladder_a3r) equals the model's: unbalanced vectors of mixed window counts,
    the trivial and the balanced vector beside them, hand vectors at the 16- and 32-digit string
    boundaries and both clamps, torsion and mixed-order keys, and dead keys (-[v]R alone)"""
    As, Rs, vecs, want = ladder3_cases(unbalanced, halfsize)
    blob, _, idx_of = ktab_filled(run)
    got = run.ladder_uv3([idx_of[A] for A in As], Rs, vecs, blob, KT_CAPACITY)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (run.name, "wave", i // 64, "lane", i % 64, vecs[i])


# --------------------------------------------------------------------------
# the wide combs: construction, digit schedule, sums (ed25519_ops.hpp wcomb_*, wcomb_build.hpp,
# kernels_common.hpp WideComb)
# --------------------------------------------------------------------------
COMB_WIDTHS = (16, 18, 20, 21, 24)   # kKeyCombNarrow / Mid / Wide / Reduced, kBCombBits
COMB_REDUCED, COMB_B = 21, 24
COMB_CORR = 0xffffffff               # "the [L]P entry" where an entry index is expected
KEY_DECODES, KEY_SMALL_ORDER, KEY_TORSION = 1, 2, 4
HALF_L = (L - 1) // 2


def comb_geom(bits):
    """(positions, chunks per position, entries per position) of CombGeom<bits>"""
    red = bits == COMB_REDUCED
    npos = (252 + bits - 1) // bits if red else (254 + bits - 1) // bits
    chunks = (1 << (bits - 1)) // 64 + (1 if red else 0)
    return npos, chunks, 64 * chunks + 1


def comb_digits(x, bits):
    """the integer model of wcomb_acc's digit schedule on a 256-bit x: kPos signed radix-2^bits
    digits (the reduced comb's top one unsigned, no carry out) and the digit behind the last
    round's reload"""
    npos = comb_geom(bits)[0]
    half, carry, out = 1 << (bits - 1), 0, []
    for j in range(npos + 1):
        raw = (x & ((1 << bits) - 1)) + carry
        carry = 1 if raw > half and not (bits == COMB_REDUCED and j == npos - 1) else 0
        x >>= bits
        out.append(raw - (carry << bits))
    return out


def comb_in_table(x, bits):
    return all(abs(d) < comb_geom(bits)[2] for d in comb_digits(x, bits))


@functools.lru_cache(maxsize=None)
def comb_committee():
    """(encodings, points -- None: undecodable) of the 5-key committee: an honest key of the corpus,
    a point of order 8, a mixed-order point T + aB, an undecodable encoding, the identity"""
    M = model()
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    import json
    cats = json.load(open(os.path.join(GOLD, "ed25519_corpus.json")))["categories"]
    honest = next(d["pk"][i].tobytes() for i in range(len(d["cat"])) if cats[int(d["cat"][i])] == "honest")
    t8 = M.TORSION[1]
    assert M.is_ident(M.pmul(8, t8)) and not M.is_ident(M.pmul(4, t8))
    y = 2
    while M.decode(y.to_bytes(32, "little")) is not None:
        y += 1
    encs = (honest, M.encode(t8), M.encode(M.padd(M.TORSION[3], M.pmul(0x1234567, M.BASE))), y.to_bytes(32, "little"),
            M.encode(M.IDENT))
    pts = tuple(M.decode(e) for e in encs)
    assert [p is None for p in pts] == [False, False, False, True, False]
    assert [M.has_torsion(p) for p in pts if p is not None] == [False, True, True, False]
    return encs, pts


def _comb_sets(bits):
    """the comb sets a width is checked on: (encodings, negate, batch, comb point per key)"""
    M = model()
    sets = [((M.encode(M.BASE),), 0, 1, (M.BASE,))]
    if bits != COMB_B:
        encs, pts = comb_committee()
        sets.append((encs, 1, 2, tuple(M.IDENT if p is None else M.pneg(p) for p in pts)))
    return sets


def _niels(pt):
    M = model()
    X, Y, Z, _ = pt
    zi = M.inv(Z)
    x, y = X * zi % P, Y * zi % P
    return ((y + x) % P, (y - x) % P, 2 * M.D * x * y % P)


@functools.lru_cache(maxsize=None)
def comb_table_cases(bits):
    """per comb set of the width: (encodings, negate, batch, expected meta -- None: only "does not
    decode" is pinned --, items (key, pos, idx), expected (y + x, y - x, 2dxy) per item)"""
    M = model()
    npos, chunks, entries = comb_geom(bits)
    regular = (1 << (bits - 1)) // 64
    chunk_list = [0, 1, regular // 2, regular - 1] + ([chunks - 1] if bits == COMB_REDUCED else [])
    out = []
    for encs, negate, batch, pts in _comb_sets(bits):
        meta = []
        for e in encs:
            a = M.decode(e)
            meta.append(None if a is None else KEY_DECODES | (KEY_SMALL_ORDER if M.is_small(a) else 0) |
                        (KEY_TORSION if bits == COMB_REDUCED and M.has_torsion(a) else 0))
        items, want = [], []
        for key in (0, 2, 4) if len(encs) > 1 else (0,):
            for pos in (0, 1, npos - 1):
                base = M.pmul(1 << (bits * pos), pts[key])
                for c in chunk_list:
                    q = M.pmul(64 * c, base)
                    for idx in range(64 * c, 64 * c + 65):
                        if idx > 64 * c or c == 0:
                            items.append((key, pos, idx))
                            want.append(_niels(q))
                        q = M.padd(q, base)
        if len(encs) > 1:  # the undecodable key: the identity everywhere
            for pos in (0, npos - 1):
                for idx in (0, 1, 64, 65, entries - 1):
                    items.append((3, pos, idx))
                    want.append((1, 1, 0))
        if bits == COMB_REDUCED:  # [L](-A) behind the positions
            for key in range(len(encs)):
                items.append((key, 0, COMB_CORR))
                want.append(_niels(M.pmul(L, pts[key])))
        out.append((encs, negate, batch, tuple(meta), tuple(items), tuple(want)))
    return out


def check_wcomb_tables(run, bits):
    """The product's wcomb_build<bits> -- B alone, and (every width but 24) the 5-key committee
    negated, two keys per fill launch: three launches, the last with one key -- read back
    through WideComb::load / load_corr: entry (pos, j) is j 2^(bits pos) P for the first, second
    and last position, the first, second, a middle and the last chunk (21: and the extra one) of
    keys 0, 2 and 4, words 30 and 31 zero; the identity everywhere for the undecodable key; the
    kKey* bits; the [L](-A) entry (21); nothing unwritten (the allocation starts as 0xA5) and the
    guard behind the combs intact.  Returns the number of entries compared."""
    n = 0
    for encs, negate, batch, meta, items, want in comb_table_cases(bits):
        try:
            got_meta = run.wcomb_build(bits, encs, negate, batch)
            for k, (g, w) in enumerate(zip(got_meta, meta)):
                if w is None:
                    assert not g & KEY_DECODES, (run.name, bits, "key", k, g)
                else:
                    assert g == w, (run.name, bits, "meta of key", k, g, w)
            got = run.wcomb_entries(items)
            for (key, pos, idx), e, w in zip(items, got, want):
                g = tuple(value(e[10 * k:10 * k + 10]) % P for k in range(3))
                assert g == w, (run.name, bits, "key", key, "pos", pos, "entry", idx if idx != COMB_CORR else "corr")
                assert e[30] == 0 and e[31] == 0, (run.name, bits, key, pos, idx, int(e[30]), int(e[31]))
            if bits == COMB_REDUCED and len(encs) > 1:
                assert want[-5] == (1, 1, 0) and want[-4] != (1, 1, 0)  # honest: the identity; order 8: not
            assert run.wcomb_guard(), (run.name, bits, "guard")
            n += len(items)
        finally:
            run.wcomb_free()
    return n


@functools.lru_cache(maxsize=None)
def comb_digit_inputs(bits):
    """(scalars, their model digits)"""
    npos = comb_geom(bits)[0]
    half = 1 << (bits - 1)
    xs = [0, 1, 2 ** 253 - 1, 2 ** 255 - 1, 2 ** 256 - 1, L, L - 1, HALF_L, (L + 1) // 2, 2 ** 251, 2 ** 251 - 1,
          2 ** 251 + 1]
    xs.append(sum(half << (bits * i) for i in range(npos - 1)))        # no carry, the maximal index everywhere
    xs.append(sum((half + 1) << (bits * i) for i in range(npos - 1)))  # a carry through every position
    if bits == COMB_REDUCED:
        xs += [t << (bits * (npos - 1)) for t in (2 ** 20, 2 ** 20 + 1, 2 ** 20 + 64)]
    rng = random.Random(1000 + bits)
    for i in range(4096):
        xs.append(rng.randrange(HALF_L + 1) if bits == COMB_REDUCED and i % 2 else rng.getrandbits(256 if i % 4 == 0 else 253))
    return tuple(xs), tuple(tuple(comb_digits(x, bits)) for x in xs)


def check_wcomb_digits(run, bits):
    """wcomb_digit under wcomb_acc's schedule against the integer model, and the loads wcomb_acc
    itself issues (a recording comb): position j gets |digit j|, the reload past the last
    position an in-range index.  The two range facts the headers state: a non-reduced comb never
    leaves its table for ANY 256-bit input, and sums exactly below 2^253; the reduced comb keeps
    its top digit <= 2^20 for every magnitude <= (L - 1) / 2 and sums exactly below 2^252.
    Returns the number of digit vectors compared."""
    xs, want = comb_digit_inputs(bits)
    npos, _, entries = comb_geom(bits)
    half, red = 1 << (bits - 1), bits == COMB_REDUCED
    # the integer model itself has the properties (so the device is held to them through it)
    for x, d in zip(xs, want):
        if not red:
            assert all(abs(t) <= half for t in d), (bits, hex(x))
        if x < (1 << 252 if red else 1 << 253):
            assert sum(t << (bits * i) for i, t in enumerate(d[:npos])) == x and d[npos] == 0, (bits, hex(x))
        if red and x <= HALF_L:
            assert all(abs(t) <= half for t in d) and 0 <= d[npos - 1] <= half, hex(x)
    assert set(want[12][:npos - 1]) == {half} and want[12][npos - 1] == 0                 # the maximal index, no carry
    assert all(t < 0 for t in want[13][:npos - 1]) and want[13][npos - 1] == 1           # a carry out of every position
    if red:
        assert [w[npos - 1] for w in want[14:17]] == [2 ** 20, 2 ** 20 + 1, 2 ** 20 + 64] and max(w[npos - 1] for w in want[14:17]) < entries
    got = run.wcomb_digits(bits, xs)
    for x, w, (d, count, loads) in zip(xs, want, got):
        assert tuple(d) == w, (run.name, bits, hex(x), d, w)
        assert count == npos + 1, (run.name, bits, hex(x), count)
        assert loads == [(min(j, npos - 1), abs(t)) for j, t in enumerate(w)], (run.name, bits, hex(x), loads)
    return len(xs)


@functools.lru_cache(maxsize=None)
def comb_acc_cases(bits):
    """(encodings, negate, batch, items (key, x, flags, start encoding), expected encodings) on the
    width's last comb set (the committee; 24: B)"""
    M = model()
    encs, negate, batch, pts = _comb_sets(bits)[-1]
    nk = len(encs)
    npos, _, entries = comb_geom(bits)
    red = bits == COMB_REDUCED
    rng = random.Random(2000 + bits)
    top = HALF_L + 1 if red else 1 << 253
    ident = M.encode(M.IDENT)
    rpt = lambda: M.pmul(rng.randrange(1, L), M.BASE)
    items, starts = [], []   # starts: the start point (None: from the identity)

    def add(key, x, neg, start):
        assert comb_in_table(x, bits), (bits, hex(x))
        items.append((key, x, (1 if start is None else 0) | (2 if neg else 0), ident if start is None else M.encode(start)))
        starts.append(start)

    def target(key, x, neg):
        t = M.pmul(x, pts[key])
        return M.pneg(t) if neg else t

    edges = [x for x in comb_digit_inputs(bits)[0][:14] if x < top] + [0]
    for x in edges:                                      # edge scalars, both signs, from the identity and added
        for neg in (0, 1):
            add(0, x, neg, None)
            add(2 % nk, x, neg, M.IDENT)
    for _ in range(3):                                   # first digit zero
        x = rng.randrange(top) >> bits << bits
        for neg in (0, 1):
            add(0, x, neg, None)
    if red:                                              # the extra chunk: top digit 2^20, +1, +64
        for t in (2 ** 20, 2 ** 20 + 1, 2 ** 20 + 64):
            x = (t << (bits * (npos - 1))) + rng.randrange(1 << (bits * (npos - 1) - 1))
            for neg in (0, 1):
                add(1, x, neg, None)
                add(2, x, neg, rpt())
    for i in range(8):                                   # the four starts
        x, key = rng.randrange(top), i % nk
        for neg in (0, 1):
            add(key, x, neg, M.IDENT)
            add(key, x, neg, rpt())
            add(key, x, neg, M.pneg(target(key, x, neg)))    # the sum is the identity
            add(key, x, neg, target(key, x, neg))            # start = the term itself
    for pos in (0, 1, npos - 1):                         # one digit: the addition of entry j to j 2^(W pos) P doubles
        x = rng.randrange(1, max(2, 1 << (min(bits, (252 if red else 253) - bits * pos) - 1))) << (bits * pos)
        for neg in (0, 1):
            add(0, x, neg, target(0, x, neg))
    for i in range(256):                                 # random scalars
        add(i % nk, rng.randrange(top), rng.getrandbits(1), None if rng.getrandbits(1) else rpt())
    while len(items) % 64:                               # the wave below starts on a wave boundary
        add(len(items) % nk, rng.randrange(top), 0, None)
    for lane in range(64):                               # one wave: its lanes differ in key, sign and start
        add(lane % nk, rng.randrange(top), (lane // nk) & 1, None if lane % 3 else rpt())
    want = []
    for (key, x, flags, _), st in zip(items, starts):
        t = target(key, x, flags & 2)
        want.append(M.encode(t if st is None else M.padd(st, t)))
    return encs, negate, batch, tuple(items), tuple(want)


def check_wcomb_acc(run, bits):
    """out = start + [+-x]P through wcomb_acc over the product's tables (see comb_acc_cases): edge
    scalars, a zero first digit from the identity, x = 0, the reduced comb's extra chunk, both
    neg_all values, the four starts, one-digit scalars whose addition is a doubling, random
    scalars, and a wave whose lanes differ in key and sign.  Returns the number of sums."""
    encs, negate, batch, items, want = comb_acc_cases(bits)
    try:
        run.wcomb_build(bits, encs, negate, batch)
        got = run.wcomb_acc(items)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (run.name, bits, "wave", i // 64, "lane", i % 64, "key", items[i][0], hex(items[i][1]),
                            "flags", items[i][2])
        assert run.wcomb_guard(), (run.name, bits, "guard")
    finally:
        run.wcomb_free()
    return len(items)


KEY_SUM_EDGES = (0, 1, 2, HALF_L, (L + 1) // 2, (L + 3) // 2, L - 1, L - 2, (1 << 251) - 1, 1 << 251, (1 << 251) + 1,
                 (1 << 252) - 1)  # test_reduced_comb_sum_equals_full_comb's


@functools.lru_cache(maxsize=None)
def key_sum_cases():
    """(items (key, k), expected encodings of [k](-A)) on the committee: whole waves first, chosen by
    which lanes owe the reduced comb's correction (a key with torsion and k > (L - 1) / 2)"""
    M = model()
    encs, pts = comb_committee()
    rng = random.Random(2121)
    lo = lambda: rng.randrange(HALF_L + 1)         # k' = k
    hi = lambda: rng.randrange(HALF_L + 1, L)      # k' = k - L
    tors, free = (1, 2), (0, 4, 3)                 # keys with / without a torsion component (3: undecodable)
    items = []
    for lane in range(64):                         # no lane owes the correction: the branch is skipped
        items.append((tors[lane % 2], lo()) if lane % 2 else (free[lane % 3], hi()))
    for owing in (0, 31, 63):                      # exactly one lane owes it
        for lane in range(64):
            items.append((tors[lane % 2], hi()) if lane == owing else ((tors[lane % 2], lo()) if lane % 3 else (free[lane % 3], hi())))
    for lane in range(64):                         # all do
        items.append((tors[lane % 2], hi()))
    for lane in range(64):                         # torsion and torsion-free keys alternate, both signs of k - L
        items.append(((tors + free)[lane % 5] if lane % 2 else free[(lane // 2) % 3], hi() if (lane // 2) % 2 else lo()))
        if lane % 2 == 0:
            items[-1] = (tors[(lane // 2) % 2], items[-1][1])
    for key in range(5):
        items += [(key, k) for k in KEY_SUM_EDGES]
    items += [(i % 5, rng.randrange(L)) for i in range(64)]
    owes = [key in tors and k > HALF_L for key, k in items]
    assert not any(owes[:64]) and [sum(owes[64 * w:64 * w + 64]) for w in (1, 2, 3)] == [1, 1, 1] and all(owes[256:320])
    assert owes[64] and owes[128 + 31] and owes[192 + 63] and 8 < sum(owes[320:384]) < 56
    want = [M.encode(M.IDENT if pts[key] is None else M.pmul(k, M.pneg(pts[key]))) for key, k in items]
    return tuple(items), tuple(want)


def check_key_comb_sum(run):
    """[k](-A) as cached_point forms it (key_comb_sum: sc_reduce_half, wcomb_acc with neg_all, the
    wave_any(corr) branch with load_corr) from the 21-bit committee combs and from the 20-bit ones:
    both equal the model's.  Returns the number of sums per width."""
    items, want = key_sum_cases()
    encs, _ = comb_committee()
    got = {}
    for bits in (COMB_REDUCED, 20):
        try:
            meta = run.wcomb_build(bits, encs, 1, 2)
            got[bits] = run.key_comb_sum([(key, meta[key], k) for key, k in items])
        finally:
            run.wcomb_free()
        for i, (g, w) in enumerate(zip(got[bits], want)):
            assert g == w, (run.name, bits, "wave", i // 64, "lane", i % 64, "key", items[i][0], hex(items[i][1]))
    assert got[COMB_REDUCED] == got[20], run.name
    return len(items)


def check_wcomb_refusals(run):
    """The comb entry points check their arguments before anything runs: a key past the set, a
    position or entry past the geometry, the [L]P marker at a width without that entry, an
    unknown flag, and -- at 21 bits -- a scalar whose digits the integer schedule puts outside
    the table are refused (an error return, nothing launched); so is any call without a live
    comb set, and a 24-bit set of more than one point.  Returns the number of refused calls."""
    M = model()
    B, ident = M.encode(M.BASE), M.encode(M.IDENT)
    refused = 0

    def refuses(call, *args):
        nonlocal refused
        try:
            call(*args)
        except RuntimeError:
            refused += 1
            return
        raise AssertionError((run.name, "not refused", call.__name__, args))

    refuses(run.wcomb_entries, [(0, 0, 0)])                       # no live set
    refuses(run.wcomb_acc, [(0, 1, 1, ident)])
    refuses(run.key_comb_sum, [(0, 1, 1)])
    refuses(run.wcomb_build, COMB_B, (B, B), 0, 1)
    refuses(run.wcomb_build, COMB_B, (B,), 1, 1)
    refuses(run.wcomb_build, 17, (B,), 0, 1)
    refuses(run.wcomb_build, 16, (B,), 0, 0)
    for bits in (16, COMB_REDUCED):
        npos, _, entries = comb_geom(bits)
        try:
            run.wcomb_build(bits, (B,), 0, 1)
            good = [(0, npos - 1, entries - 1)]
            assert len(run.wcomb_entries(good)) == 1
            for bad in ((1, 0, 0), (0, npos, 0), (0, 0, entries), (0, 0, 2 ** 31)) + (((0, 0, COMB_CORR),) if bits == 16 else ()):
                refuses(run.wcomb_entries, good + [bad])
            refuses(run.wcomb_acc, [(0, 1, 1, ident), (1, 1, 1, ident)])
            refuses(run.wcomb_acc, [(0, 1, 4, ident)])
            refuses(run.key_comb_sum, [(0, 1, 1), (1, 1, 1)])
            if bits == COMB_REDUCED:
                for x in (2 ** 256 - 1, 2 ** 252 - 1, (2 ** 20 + 65) << 231, (2 ** 21 - 1) << 231):
                    assert not comb_in_table(x, bits), hex(x)
                    refuses(run.wcomb_acc, [(0, 1, 1, ident), (0, x, 1, ident)])
                k = 2 ** 253 + 3 * 2 ** 250                     # >= L: sc_reduce_half leaves it as it is
                assert (L - k) % 2 ** 256 > k and not comb_in_table(k, bits)
                refuses(run.key_comb_sum, [(0, 1, 1), (0, 1, k)])
            else:
                assert comb_in_table(2 ** 256 - 1, bits)
                assert len(run.wcomb_acc([(0, 2 ** 256 - 1, 1, ident)])) == 1   # any 256-bit input stays inside
            assert run.wcomb_guard()
        finally:
            run.wcomb_free()
    refuses(run.wcomb_guard)                                       # freed: no live set
    return refused


# --------------------------------------------------------------------------
# the key-table cache's comb path: ktab_build_comb, kc_recode / kc_pick, ladder_kc, compare_one,
# verify_kc (ktab_comb.hpp; compare_one: ed25519_ops.hpp), over the runner's comb table
# --------------------------------------------------------------------------
KC_CAPACITY = 80
KC_EDGES = (0, 1, 2, 3, L - 1, L - 2, 1 << 252, (1 << 253) - 1, (1 << 253) - 2)
# the block boundaries 2^(16 j) -1, +0, +1; j = 4, 8, 12 are the tooth boundaries
KC_BOUNDS = tuple((1 << (16 * j)) + d for j in range(1, 16) for d in (-1, 0, 1))


class Mul:
    """[k]Q for many k and one Q of the point model: the powers [2^i]Q once, then additions"""

    def __init__(self, Q):
        self.M, self.pw = model(), [Q]
        for _ in range(255):
            self.pw.append(self.M.padd(self.pw[-1], self.pw[-1]))

    def __call__(self, k):
        acc, i = self.M.IDENT, 0
        while k:
            if k & 1:
                acc = self.M.padd(acc, self.pw[i])
            k >>= 1
            i += 1
        return acc


def entry_scalar(block, index):
    """the integer multiple of A that comb line 8 block + index holds (ktab_comb.hpp, "The comb")"""
    r = [1 if index >> t & 1 else -1 for t in range(3)]
    return (1 << 16 * block) * ((1 << 192) + r[2] * (1 << 128) + r[1] * (1 << 64) + r[0])


@functools.lru_cache(maxsize=None)
def kcomb_fill_order():
    """ktab_keys() in the order one fill call takes them, three waves:
    wave 0 -- the duplicated random key on all 64 lanes (64 racing for one slot: exactly one claimer);
    wave 1 -- 64 distinct keys met nowhere else (every lane a claimer), the 8 undecodable ones among them;
    wave 2 -- the 8 keys left and 5 duplicates of two of them: a ragged wave of 13 lanes."""
    keys, kinds = ktab_keys()
    kind_of = dict(zip(keys, kinds))
    k0 = keys[0]
    assert keys[:5] == (k0,) * 5
    others = [k for k in dict.fromkeys(keys) if k != k0]
    undec = [k for k in others if kind_of[k] == "undecodable"]
    rest = [k for k in others if kind_of[k] != "undecodable"]
    assert len(undec) == 8 and len(rest) == 64
    wave1 = rest[4:60] + undec
    left = rest[:4] + rest[60:]
    wave2 = left + [left[0]] * 3 + [left[5]] * 2
    order = [k0] * 64 + wave1 + wave2
    assert len(wave1) == 64 and len(set(wave1)) == 64 and set(order) == set(keys) and len(order) % 64 == 13
    return tuple(order)


@functools.lru_cache(maxsize=None)
def kcomb_expected():
    """per distinct key: None (undecodable) or (is_small, the 33 affine niels triples of its comb lines)"""
    M = model()
    want = {}
    for e in dict.fromkeys(ktab_keys()[0]):
        A = M.decode(e)
        if A is None:
            want[e] = None
            continue
        mul = Mul(A)
        pts = [mul(entry_scalar(n // 8, n % 8)) for n in range(KC_SIGNED)] + [A]
        want[e] = (M.is_small(A), tuple(_niels(p) for p in pts))
    return want


def _comb_lines(blob, capacity):
    """the comb pool of a blob as (capacity, 33, 128) bytes"""
    off = kcomb_comb_off(capacity)
    return blob[off:off + capacity * KC_COMB_BYTES].reshape(capacity, KC_LINES, KC_LINE_BYTES)


def _pool_entries(blob, capacity):
    return blob[KT_POOL_OFF:KT_POOL_OFF + capacity * KT_ENTRY_BYTES].reshape(capacity, KT_ENTRY_BYTES)


def kcomb_filled(run):
    """the runner's comb table of ktab_keys(), filled once by one kcomb_fill call in kcomb_fill_order():
    (blob, slots won, entry index per key).  Kept on the runner: the ladder and the verdicts read it."""
    if not hasattr(run, "_kcomb"):
        order = kcomb_fill_order()
        blob = kcomb_blob(KC_CAPACITY)
        slots = run.kcomb_fill(order, blob, KC_CAPACITY)
        distinct = list(dict.fromkeys(order))
        seen = run.kcomb_line(distinct, [KC_SIGNED] * len(distinct), blob, KC_CAPACITY)  # a second launch
        run._kcomb = (blob, slots, {k: s[0] for k, s in zip(distinct, seen)})
    return run._kcomb


def check_kcomb_tables(run):
    """ktab_probe / ktab_take / ktab_build with a comb pool (ktab_build_comb: the 16 bases parked in the
    lane's table workspace, 12 additions per block, one inversion for 32 lines read back from the
    pool) over the runner's table, in the waves of kcomb_fill_order().  One entry per distinct key
    with the model's tag and flags; lines 0..31 through comb_load, reduced mod p, are the affine
    niels form of entry_scalar(block, index) A and line 32 is A, a line number past 32 is line 32;
    the pool's own bytes say the same, bytes 120..127 of every line keep the prefill, of the entry
    pool only headers are written, an undecodable key gets a header alone, nothing past the last
    entry or in the guard is touched.  Then a pool of 4 filled by one wave of 64 claimers (4 win,
    60 find the pool exhausted, undecodable keys among them) and a second call that finds it full.
    Returns the number of lines compared."""
    order, want = kcomb_fill_order(), kcomb_expected()
    distinct = list(want)
    blob, slots, idx_of = kcomb_filled(run)
    cap = KC_CAPACITY
    assert int(blob[:4].view(np.uint32)[0]) == len(distinct), (run.name, "pool used")
    assert not blob[16:28].any() and not blob[32:40].any(), (run.name, "addresses handed back")
    won = [s != KT_NO_SLOT for s in slots]
    assert sum(won[:64]) == 1, (run.name, "wave 0: one claimer", sum(won[:64]))
    assert all(won[64:128]), (run.name, "wave 1: 64 claimers")
    for k in distinct:  # one CAS winner per key, and its slot names the entry
        mine = [s for kk, s in zip(order, slots) if kk == k and s != KT_NO_SLOT]
        assert len(mine) == 1 and mine[0] < KT_SLOTS, (run.name, k.hex(), mine)
        assert _slot_state(blob, mine[0]) == KT_READY0 + idx_of[k], (run.name, k.hex())
    assert sorted(idx_of[k] for k in distinct) == list(range(len(distinct))), (run.name, "entry indices")
    lines, entries = _comb_lines(blob, cap), _pool_entries(blob, cap)
    numbers = list(range(KC_LINES)) + [KC_LINES, 40, 0xffffffff]   # the last three: comb_line's clamp
    items = [(k, n) for k in distinct for n in numbers]
    got = run.kcomb_line([k for k, _ in items], [n for _, n in items], blob, cap)
    n_small = n_dead = n_lines = 0
    for (k, n), (idx, same, flags, limbs) in zip(items, got):
        assert idx == idx_of[k] and same == 1, (run.name, k.hex(), n, idx, same)
        line = min(n, KC_SIGNED)
        raw = lines[idx, line]
        assert limbs.tobytes() == raw[:120].tobytes(), (run.name, k.hex(), "line", n, "comb_load != the pool's bytes")
        assert (raw[120:] == KC_FILL).all(), (run.name, k.hex(), "line", n, "bytes 120..127")
        if want[k] is None:
            assert flags == KT_UNDECODABLE, (run.name, k.hex(), flags)
            assert (raw == KC_FILL).all(), (run.name, k.hex(), "line", n, "an undecodable key has no lines")
            n_dead += 1
            continue
        small, niels = want[k]
        assert flags == (KT_SMALL_ORDER if small else 0), (run.name, k.hex(), flags)
        n_small += small
        g = tuple(value(limbs[10 * c:10 * c + 10]) % P for c in range(3))
        assert g == niels[line], (run.name, k.hex(), "line", n)
        assert is_reduced(limbs[:10]) and is_reduced(limbs[10:20]) and is_reduced(limbs[20:]), (run.name, k.hex(), n)
        n_lines += 1
    assert n_small >= 8 * len(numbers) and n_dead == 8 * len(numbers)
    for k in distinct:  # the entry pool: the tag and the flags, and nothing behind the header
        e = entries[idx_of[k]]
        assert e[:32].tobytes() == k, (run.name, k.hex(), "tag")
        assert (e[KT_HEADER_BYTES:] == KC_FILL).all(), (run.name, k.hex(), "bytes behind the header")
    used = len(distinct)
    assert (entries[used:] == KC_FILL).all() and (lines[used:] == KC_FILL).all(), (run.name, "past the last entry")
    assert (blob[-KC_GUARD_BYTES:] == KC_FILL).all(), (run.name, "guard")
    # a pool of 4 entries in a fresh table: one wave of 64 distinct claimers, then everything else
    cap = 4
    blob4 = kcomb_blob(cap)
    wave = list(order[64:128])
    slots4 = run.kcomb_fill(wave, blob4, cap)
    # in lockstep all 64 lanes find the pool empty, claim a slot and ask the pool: 4 win, 60 find it
    # exhausted; one after the other, the fifth key on finds the pool full and claims nothing
    claimers = sum(s != KT_NO_SLOT for s in slots4)
    assert claimers == (64 if run.waves else cap), (run.name, "claimers", claimers)
    assert int(blob4[:4].view(np.uint32)[0]) == claimers, (run.name, "every claimer asked the pool")
    later = run.kcomb_fill([k for k in order if k not in wave], blob4, cap)
    assert all(s == KT_NO_SLOT for s in later), (run.name, "a full pool is left alone")
    assert int(blob4[:4].view(np.uint32)[0]) == claimers
    seen = run.kcomb_line(distinct, [KC_SIGNED] * len(distinct), blob4, cap)
    ready = {k: s for k, s in zip(distinct, seen) if s[0] != KT_NO_SLOT}
    assert sorted(s[0] for s in ready.values()) == list(range(cap)) and set(ready) <= set(wave), (run.name, sorted(ready))
    lines4, entries4 = _comb_lines(blob4, cap), _pool_entries(blob4, cap)
    for k, (idx, same, flags, limbs) in ready.items():
        assert same == 1 and entries4[idx, :32].tobytes() == k, (run.name, k.hex())
        assert (entries4[idx, KT_HEADER_BYTES:] == KC_FILL).all(), (run.name, k.hex())
        if want[k] is None:
            assert flags == KT_UNDECODABLE and (lines4[idx] == KC_FILL).all(), (run.name, k.hex())
            continue
        for n in range(KC_LINES):
            w = lines4[idx, n, :120].view(np.uint32)
            assert tuple(value(w[10 * c:10 * c + 10]) % P for c in range(3)) == want[k][1][n], (run.name, k.hex(), n)
            assert (lines4[idx, n, 120:] == KC_FILL).all(), (run.name, k.hex(), n)
        n_lines += KC_LINES
    for k, s in zip(wave, slots4):  # the claimers that found the pool exhausted: seen for good
        if k not in ready and s != KT_NO_SLOT:
            assert _slot_state(blob4, s) == KT_SEEN, (run.name, k.hex(), _slot_state(blob4, s))
    states = blob4[KT_CTL_BYTES:KT_POOL_OFF].view(np.uint64) >> np.uint64(32)
    assert sorted(int(s) for s in states[states >= KT_READY0]) == [KT_READY0 + i for i in range(cap)], run.name
    assert not np.any(states == KT_CLAIMED), (run.name, "a slot left claimed")
    # every byte behind the four combs -- here: the guard -- and behind the four entries is untouched
    assert blob4[kcomb_comb_off(cap) + cap * KC_COMB_BYTES:].size == KC_GUARD_BYTES
    assert (blob4[kcomb_comb_off(cap) + cap * KC_COMB_BYTES:] == KC_FILL).all(), (run.name, "guard of the pool of 4")
    return n_lines


@functools.lru_cache(maxsize=None)
def kc_pick_scalars():
    rng = random.Random(20261021)
    return KC_EDGES + KC_BOUNDS + tuple(rng.randrange(L) for _ in range(330))


def check_kc_picks(run):
    """kc_recode + the 64 kc_pick lookups in ladder_kc's order (on the device through the LDS digit
    cells): block i mod 4, index below 8, and summed the way the ladder sums them -- one doubling
    before every column but the first; a negated entry counts positive, because the ladder sums
    -[K]A over tables of +A -- exactly k + c = k | 1 with c = 1 - (k & 1), for the edge scalars,
    the tooth and block boundaries and seeded random k.  Returns the number of pick vectors."""
    ks = kc_pick_scalars()
    assert {k & 1 for k in ks[:9]} == {0, 1} and all(k < 1 << 253 for k in ks)
    for k, (picks, c) in zip(ks, run.kc_picks(ks)):
        acc = 0
        for i, (block, index, neg) in enumerate(picks):
            assert block == i % 4 and 0 <= index < 8 and neg in (0, 1), (run.name, hex(k), i, block, index, neg)
            if i % 4 == 0 and i:
                acc *= 2
            acc += (1 if neg else -1) * entry_scalar(block, index)
        assert c == 1 - (k & 1) and acc == k + c == k | 1, (run.name, hex(k), c)
    return len(ks)


def _keys_of_kind(kind, n):
    keys, kinds = ktab_keys()
    return [k for k, x in dict(zip(keys, kinds)).items() if x == kind][:n]


@functools.lru_cache(maxsize=None)
def ladder_kc_cases():
    """(key encodings, scalars, dead flags, expected encodings) of five waves and a tail of 21 lanes.
    Waves 0..2 carry the 9 edge and 45 boundary scalars and 10 random ones, lane l of wave r on key
    (l + r) mod 8 of {3 honest, 2 mixed-order, 2 small-order, 1 undecodable}: both parities, eight
    entries and -- the undecodable key's lanes, as verify_kc runs them -- dead lanes beside live
    ones in every wave, and every scalar live on at least two keys.  Wave 3: one k on every lane;
    wave 4: 64 distinct random k; the tail: random."""
    M = model()
    keyset = _keys_of_kind("random", 3) + _keys_of_kind("mixed", 2) + _keys_of_kind("torsion", 8)[3:5] + \
        _keys_of_kind("undecodable", 1)
    assert len(keyset) == 8 and M.is_small(M.decode(keyset[5])) and not M.is_ident(M.decode(keyset[5]))
    rng = random.Random(4242)
    base = list(KC_EDGES + KC_BOUNDS) + [rng.randrange(L) for _ in range(10)]
    assert len(base) == 64
    same = rng.randrange(L)
    As, ks = [], []
    for r in range(3):
        for lane in range(64):
            As.append(keyset[(lane + r) % 8])
            ks.append(base[lane])
    for lane in range(64):
        As.append(keyset[lane % 8])
        ks.append(same)
    for lane in range(64 + 21):
        As.append(keyset[(3 * lane + 1) % 8])
        ks.append(rng.randrange(L))
    assert len(set(ks[256:320])) == 64
    dead = [1 if M.decode(A) is None else 0 for A in As]
    for w in range(5):
        sl = slice(64 * w, 64 * w + 64)
        assert 0 < sum(dead[sl]) < 64 and len(set(As[sl])) == 8, w
        assert w == 3 or {k & 1 for k, d in zip(ks[sl], dead[sl]) if not d} == {0, 1}, w
    for lane in range(64):  # every edge and boundary scalar: live on two keys at least
        assert sum(1 - dead[64 * r + lane] for r in range(3)) >= 2
    mul = {A: Mul(M.pneg(M.decode(A))) for A in keyset if M.decode(A) is not None}
    want = [M.encode(M.IDENT if d else mul[A](k)) for A, k, d in zip(As, ks, dead)]
    return tuple(As), tuple(ks), tuple(dead), tuple(want)


def check_ladder_kc(run):
    """ladder_kc's result is [k](-A) by the model, as an integer multiple, for honest, mixed-order
    and small-order keys over the combs the runner built (see ladder_kc_cases): lanes of one wave
    differ in parity -- kc_load's `off` of the correction --, in entry, and in dead or live.
    Returns the number of results compared."""
    As, ks, dead, want = ladder_kc_cases()
    blob, _, idx_of = kcomb_filled(run)
    got = run.ladder_kc([idx_of[A] for A in As], ks, dead, blob, KC_CAPACITY)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (run.name, "wave", i // 64, "lane", i % 64, "k", hex(ks[i]), "key", As[i].hex(), "dead", dead[i])
    return len(ks)


def _affine(p):
    zi = model().inv(p[2])
    return p[0] * zi % P, p[1] * zi % P


@functools.lru_cache(maxsize=None)
def compare_one_cases():
    """(x, y, z, R encoding, mode, expected bit): the cases of tests/test_ktab4_host.py's
    test_compare_at_function_level, z random (never 1) unless said"""
    M = model()
    rng = random.Random(7)
    z = lambda: rng.randrange(2, P)
    cases = []
    for i in range(20):
        Rp = M.pmul(rng.randrange(1, L), M.BASE)
        x, y = _affine(Rp)
        enc = M.encode(Rp)
        other = bytes(enc[:31]) + bytes([enc[31] ^ 0x80])
        wrong = (int.from_bytes(enc, "little") ^ 2).to_bytes(32, "little")
        for mode in (0, 1):
            zz = 1 if i == 0 else z()
            cases += [(x, y, zz, enc, mode, 1),       # R's own encoding
                      (x, y, zz, other, mode, 0),     # enc(-R'): same y, the other sign
                      (x, y, zz, wrong, mode, 0)]
    # x' = 0: (0, 1) and (0, -1); a set sign bit ("negative zero") passes the cofactorless rule; both
    # points are of small order: strict rejects
    for y in (1, P - 1):
        for sign in (0, 1):
            R = (y | sign << 255).to_bytes(32, "little")
            cases += [(0, y, z(), R, 1, 1), (0, y, z(), R, 0, 0)]
    # y_R = y' + p fits in 255 bits only for y' < 19: the curve points with such y
    seen = 0
    for y in range(19):
        pt = M.decode(y.to_bytes(32, "little"))
        if pt is None:
            continue
        x, _ = _affine(pt)
        R = ((y + P) | (x & 1) << 255).to_bytes(32, "little")
        flip = ((y + P) | ((x & 1) ^ 1) << 255).to_bytes(32, "little")
        cases += [(x, y, z(), R, 1, 1), (x, y, z(), R, 0, 0 if M.is_small(pt) else 1),
                  (x, y, z(), flip, 1, 1 if x == 0 else 0)]
        seen += 1
    assert seen >= 2
    for t in M.TORSION:  # every point of small order: rejected in strict, accepted in cofactorless
        x, y = _affine(t)
        cases += [(x, y, z(), M.encode(t), 0, 0), (x, y, z(), M.encode(t), 1, 1)]
    return tuple(cases)


def check_compare_one(run):
    """compare_one with a chosen R' = (x z : y z : z), z inverted by fe_invert_batch, in both modes:
    R's own encoding, the other sign, one bit of y off, x = 0 under a set sign bit, y >= p
    encodings, R' of small order under strict, z = 1 and z != 1.  Returns the number of bits."""
    cases = compare_one_cases()
    got = run.compare_one([c[:5] for c in cases])
    for i, (c, g) in enumerate(zip(cases, got)):
        assert g == c[5], (run.name, "item", i, "mode", c[4], "x", hex(c[0]), "y", hex(c[1]), "R", c[3].hex(), g)
    return len(cases)


def model_verify_kc(A_enc, kflags, R, s, k, mode):
    """verify_kc's verdict from the point model: s < L, the key decodes (its header says so),
    (strict) the key is not of small order, R' = [s]B - [k]A equals the point R's bytes decode to
    -- y taken mod p, the sign bit ignored where x = 0, as dalek compares --, (strict) R' is not
    of small order"""
    M = model()
    if s >= L or kflags & KT_UNDECODABLE or (mode == 0 and kflags & KT_SMALL_ORDER):
        return 0
    Rp = M.padd(M.pmul(s, M.BASE), M.pmul(k, M.pneg(M.decode(A_enc))))
    Rd = M.decode(R)
    ok = Rd is not None and M.peq(Rd, Rp)
    if mode == 0:
        ok = ok and not M.is_small(Rp)
    return int(ok)


@functools.lru_cache(maxsize=None)
def verify_kc_cases():
    """(key encoding, header flags -- None: the entry's own --, R, s, k, what) per case; each runs in
    both modes, and all of them share one wave"""
    M = model()
    keys, kinds = ktab_keys()
    rng = random.Random(55)  # ktab_keys' own generator: the seeds a of its random keys A = [a]B
    seeds = [rng.randrange(1, M.L) for _ in range(24)]
    a, A = seeds[1], keys[5]
    assert M.encode(M.pmul(a, M.BASE)) == A and kinds[5] == "random"
    rng = random.Random(56)
    ident = M.encode(M.IDENT)
    flip = lambda e, bit: (int.from_bytes(e, "little") ^ (1 << bit)).to_bytes(32, "little")
    cases = [(A, None, ident, 0, 0, "s = 0, k = 0: R' is the identity")]
    for k in (1, 2, L - 1, rng.randrange(L)):
        cases.append((A, None, ident, k * a % L, k, "s = k a: R' is the identity, k != 0"))
    for k in (rng.randrange(L), rng.randrange(L) | 1, rng.randrange(L) & ~1, 0, L - 1):
        r = rng.randrange(1, L)
        R, s = M.encode(M.pmul(r, M.BASE)), (r + k * a) % L
        cases.append((A, None, R, s, k, "honest"))
        if len(cases) < 12:
            cases.append((A, None, R, s + L, k, "s + L"))
            cases.append((A, None, flip(R, 3), s, k, "a bit of R's y flipped"))
            cases.append((A, None, flip(R, 255), s, k, "R's sign bit flipped"))
            cases.append((A, KT_UNDECODABLE, R, s, k, "honest, header says undecodable"))
            cases.append((A, KT_SMALL_ORDER, R, s, k, "honest, header says small order"))
    undec = _keys_of_kind("undecodable", 1)[0]
    cases.append((undec, None, ident, 0, 0, "an undecodable key's own entry"))
    T = _keys_of_kind("torsion", 8)[3]
    for k in (rng.randrange(L), 5):
        r = rng.randrange(1, L)
        R = M.encode(M.padd(M.pmul(r, M.BASE), M.pmul(k, M.pneg(M.decode(T)))))
        cases.append((T, None, R, r, k, "a small-order key, R exact"))
    cases.append((T, 0, R, r, k, "a small-order key whose header does not say so"))
    mixed = _keys_of_kind("mixed", 1)[0]
    k, r = rng.randrange(L), rng.randrange(1, L)
    R = M.encode(M.padd(M.pmul(r, M.BASE), M.pmul(k, M.pneg(M.decode(mixed)))))
    cases.append((mixed, None, R, r, k, "a mixed-order key, R exact"))
    cases.append((mixed, None, R, (r + 1) % L, k, "a mixed-order key, s off by one"))
    assert 2 * len(cases) <= 64, len(cases)
    return tuple(cases)


def check_verify_kc(run):
    """verify_kc's bit for chosen (R, s, k) that no hash reaches, over the runner's combs and the
    16-bit comb of B the probe builds, both modes of every case in ONE wave.  Expected bits:
    model_verify_kc.  The corpus rule each case restates (tests/golden):
      s = 0, k = 0 and s = k a, R = the identity's encoding -- small_order_R / all_zero_sig: the
        cofactorless rule accepts the exact equation, strict rejects a small-order R;
      honest -- honest; s + L -- s_plus_L (s >= L: rejected in both modes);
      a bit of R flipped -- wrong_msg_bitflip / R_not_on_curve (the equation fails, or R decodes to nothing);
      header undecodable -- A_not_on_curve (rejected in both modes);
      header small order, and a small-order key with R exact -- small_order_A / small_A_R_exact
        (strict rejects, the cofactorless rule accepts);
      a mixed-order key with R exact -- mixed_A_valid (accepted in both modes: the check is the
        cofactorless single-signature equation, nothing is multiplied by 8).
    Returns the number of verdicts compared."""
    M = model()
    cases = verify_kc_cases()
    blob, _, idx_of = kcomb_filled(run)
    items, want = [], []
    for A, kflags, R, s, k, _ in cases:
        own = (KT_UNDECODABLE if M.decode(A) is None else (KT_SMALL_ORDER if M.is_small(M.decode(A)) else 0))
        f = own if kflags is None else kflags
        for mode in (0, 1):
            items.append((idx_of[A], f, R, s, k, mode))
            want.append(0 if M.decode(A) is None else model_verify_kc(A, f, R, s, k, mode))
    assert len(items) <= 64 and 8 <= sum(want) <= len(want) - 8
    try:
        run.wcomb_build(16, (M.encode(M.BASE),), 0, 1)
        got = run.verify_kc(items, blob, KC_CAPACITY)
    finally:
        run.wcomb_free()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (run.name, "lane", i, cases[i // 2][5], "mode", items[i][5], "got", g, "want", w)
    return len(items)


def check_kcomb_refusals(run):
    """The comb entry points refuse, before anything runs: a capacity of 0, an entry index at the
    capacity, a scalar k >= 2^253, a mode other than 0 or 1, a dead flag or header flags out of
    range, and verify_kc without a 16-bit comb of B.  Returns the number of refused calls."""
    M = model()
    blob, _, idx_of = kcomb_filled(run)
    cap = KC_CAPACITY
    ident, key = M.encode(M.IDENT), ktab_keys()[0][0]
    refused = 0

    def refuses(call, *args):
        nonlocal refused
        try:
            call(*args)
        except RuntimeError:
            refused += 1
            return
        raise AssertionError((run.name, "not refused", call.__name__))

    refuses(run.kcomb_fill, [key], blob, 0)
    refuses(run.kcomb_line, [key], [0], blob, 0)
    refuses(run.kc_picks, [1, 1 << 253])
    refuses(run.ladder_kc, [0, cap], [1, 1], [0, 0], blob, cap)
    refuses(run.ladder_kc, [0, 0], [1, 1 << 253], [0, 0], blob, cap)
    refuses(run.ladder_kc, [0, 0], [1, 1], [0, 2], blob, cap)
    refuses(run.compare_one, [(0, 1, 1, ident, 0), (0, 1, 1, ident, 2)])
    good = (0, 0, ident, 0, 0, 1)
    refuses(run.verify_kc, [good], blob, cap)                      # no live comb of B
    try:
        run.wcomb_build(16, (M.encode(M.BASE),), 0, 1)
        assert run.verify_kc([good], blob, cap) == [1]
        for bad in ((cap, 0, ident, 0, 0, 1), (0, 4, ident, 0, 0, 1), (0, 0, ident, 0, 1 << 253, 1), (0, 0, ident, 0, 0, 2)):
            refuses(run.verify_kc, [good, bad], blob, cap)
    finally:
        run.wcomb_free()
    try:
        run.wcomb_build(18, (M.encode(M.BASE),), 0, 1)
        refuses(run.verify_kc, [good], blob, cap)                  # not the narrowest width
    finally:
        run.wcomb_free()
    return refused
