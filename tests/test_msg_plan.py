"""The layout walk of the device message parser (narwhal-tusk_amd/csrc/
msg_plan.hpp) on the host: untrusted bytes must never make it read outside the
message, and whatever it calls decidable on the device the host decoder
(wire.cpp, through N.wire_reencode) decodes to the same kind, round, counts
and length.  CPU only: tests/cpp/msgplan/ builds the walk for the host, once as
a stand-alone program under the address and undefined-behaviour sanitizers and
once as a plain library for ctypes."""
import base64
import ctypes
import os
import random
import struct
import subprocess
import sys

import pytest

import _wire as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "narwhal-tusk_amd"))
from ntcrypto import narwhal as N  # noqa: E402

MDIR = os.path.join(ROOT, "tests", "cpp", "msgplan")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
HOST = 0xFF
ALL, CERT_ONLY = 0xF, 1 << 2
FIELDS = ("kind", "round", "np", "nq", "nv", "nd", "off_par", "off_id", "off_sig", "off_votes", "key0", "key1",
          "decidable", "oob", "extent")


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", MDIR], check=True)
    return BUILD


@pytest.fixture(scope="module")
def walk(built):
    lib = ctypes.CDLL(os.path.join(built, "libnthost_msgplan.so"))
    lib.ntmp_walk.restype = None

    def run(msg, keys44, kinds=ALL):
        # an exact-size copy, so the offsets the walk reports are offsets into `msg`
        buf = (ctypes.c_uint8 * max(len(msg), 1)).from_buffer_copy(bytes(msg) or b"\0")
        out = (ctypes.c_uint64 * 15)()
        lib.ntmp_walk(buf, ctypes.c_uint64(len(msg)), ctypes.c_uint32(kinds), keys44, ctypes.c_uint32(len(keys44) // 44),
                      out)
        return dict(zip(FIELDS, list(out)))

    return run


def test_sanitized_driver_is_clean(built):
    """200,000 mutated messages through the walk under ASan + UBSan, behind a loader
    that aborts on a read outside [0, len): exit status 0, every kind decided."""
    r = subprocess.run([os.path.join(built, "msg_plan_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "decidable headers" in r.stdout


def _rb(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def _objects(rng, keys, count):
    out = []
    for i in range(count):
        kind = i % 4
        if kind == 0:
            out.append(W.Header(rng.choice(keys), rng.getrandbits(64),
                                {_rb(rng, 32): rng.getrandbits(32) for _ in range(rng.randrange(0, 5))},
                                {_rb(rng, 32) for _ in range(rng.choice([0, 1, 4, 70]))}, sig=_rb(rng, 64)))
        elif kind == 1:
            out.append(W.Vote(_rb(rng, 32), rng.getrandbits(64), rng.choice(keys), rng.choice(keys), _rb(rng, 64)))
        elif kind == 2:
            h = W.Header(rng.choice(keys), rng.getrandbits(20), {_rb(rng, 32): 0}, {_rb(rng, 32)}, sig=_rb(rng, 64))
            out.append(W.Certificate(h, [(rng.choice(keys), _rb(rng, 64)) for _ in range(rng.randrange(0, 8))]))
        else:
            out.append(([_rb(rng, 32) for _ in range(rng.randrange(0, 4))], rng.choice(keys)))
    return out


def _canon_counts(canon):
    """(kind, round, np, nq, nv, nd) of a canonical encoding, read at its fixed offsets"""
    tag = struct.unpack_from("<I", canon, 0)[0]
    if tag == 1:
        return tag, struct.unpack_from("<Q", canon, 36)[0], 0, 0, 0, 0
    if tag == 3:
        return tag, 0, 0, 0, 0, struct.unpack_from("<Q", canon, 4)[0]
    # the author's key decodes from any valid base64 text of >= 32 bytes; the walk only
    # passes 44-character ones, which the encoder writes back at the same length
    klen = struct.unpack_from("<Q", canon, 4)[0]
    assert klen == 44
    rnd, np_ = struct.unpack_from("<QQ", canon, 56)
    nq = struct.unpack_from("<Q", canon, 72 + 36 * np_)[0]
    end = 72 + 36 * np_ + 8 + 32 * nq + 96
    nv = struct.unpack_from("<Q", canon, end)[0] if tag == 2 else 0
    return tag, rnd, np_, nq, nv, 0


def test_walk_agrees_with_host_decoder(walk):
    rng = random.Random(20240607)
    keys = [_rb(rng, 32) for _ in range(6)]
    keys44 = b"".join(base64.b64encode(k) for k in keys)
    seeds = [W.message(o) for o in _objects(rng, keys, 48)]
    # every seed as built: decidable, with the layout the encoder wrote
    for m in seeds:
        p = walk(m, keys44)
        assert p["decidable"] == 1 and p["oob"] == 0 and p["extent"] == len(m), p
        assert walk(m + b"tail!", keys44)["extent"] == len(m)              # trailing bytes are allowed
        assert walk(m[:-1], keys44)["kind"] == HOST                         # one byte short is not
        only = walk(m, keys44, CERT_ONLY)                                   # the certificate-only mask
        assert only["kind"] == (2 if m[0] == 2 else HOST)
    decided = {0: 0, 1: 0, 2: 0, 3: 0}
    host = 0
    for it in range(6000):
        m = bytearray(rng.choice(seeds))
        op = it % 5
        if op == 0:                       # flip random bits
            for _ in range(rng.randrange(1, 6)):
                m[rng.randrange(len(m))] ^= 1 << rng.randrange(8)
        elif op == 1:                     # overwrite a length / count field region
            p = rng.randrange(max(1, len(m) - 8))
            m[p:p + 8] = struct.pack("<Q", rng.choice([0, 1, 44, 45, 1 << 20, 1 << 32, (1 << 64) - 1,
                                                       rng.getrandbits(64)]))
        elif op == 2:                     # truncate
            m = m[:rng.randrange(len(m))]
        elif op == 3:                     # splice two messages
            o = rng.choice(seeds)
            m = m[:rng.randrange(len(m))] + o[rng.randrange(len(o)):]
        else:                             # garbage with tags 0..4
            m = bytearray(struct.pack("<I", rng.randrange(5)) + _rb(rng, rng.randrange(200)))
        m = bytes(m)
        p = walk(m, keys44)
        assert p["oob"] == 0, (it, p)
        if p["kind"] == HOST:
            assert p["decidable"] == 0
            host += 1
            continue
        assert p["extent"] <= len(m), (it, p)
        assert p["kind"] == struct.unpack_from("<I", m, 0)[0]
        if not p["decidable"]:
            continue
        decided[p["kind"]] += 1
        r = N.wire_reencode(m)
        assert r is not None, (it, p)
        canon, used = r
        assert used == p["extent"], (it, used, p)
        kind, rnd, np_, nq, nv, nd = _canon_counts(canon)
        assert kind == p["kind"]
        if kind != 3:
            assert rnd == p["round"]
        # the decoder's map / set drop repeated digests; the walk counts wire entries
        pay = {m[72 + 36 * k:72 + 36 * k + 32] for k in range(p["np"])}
        par = {m[p["off_par"] + 32 * k:p["off_par"] + 32 * k + 32] for k in range(p["nq"])}
        assert (np_, nq, nv, nd) == (len(pay), len(par), p["nv"], p["nd"]), (it, p)
    assert min(decided.values()) > 100 and host > 1000, (decided, host)


def test_walk_caps_and_prefixes(walk):
    """Counts over the caps, key length prefixes other than 44 and a tag above 3 go to the host."""
    rng = random.Random(9)
    key = _rb(rng, 32)
    keys44 = base64.b64encode(key)
    vote = W.message(W.Vote(_rb(rng, 32), 3, key, key, _rb(rng, 64)))
    assert len(vote) == 212 and walk(vote, keys44)["decidable"] == 1
    for pos in (44, 96):
        bad = vote[:pos] + struct.pack("<Q", 43) + vote[pos + 8:]
        assert walk(bad, keys44)["kind"] == HOST
    assert walk(struct.pack("<I", 4) + vote[4:], keys44)["kind"] == HOST
    other = base64.b64encode(_rb(rng, 32))
    assert walk(vote, other)["decidable"] == 0                              # not a committee key
    cert = W.message(W.Certificate(W.Header(key, 1, {}, set()), [(key, _rb(rng, 64))] * 3))
    p = walk(cert, keys44)
    assert (p["decidable"], p["nv"]) == (1, 3)
    q = p["off_votes"] + 116
    assert walk(cert[:q] + struct.pack("<Q", 45) + cert[q + 8:], keys44)["decidable"] == 0
    big = cert[:p["off_votes"] - 8] + struct.pack("<Q", 1025) + cert[p["off_votes"]:] + bytes(116 * 1025)
    assert walk(big, keys44)["kind"] == HOST                               # more votes than the cap
    req = W.message(([_rb(rng, 32)] * 2, key))
    p = walk(req, keys44)
    assert (p["decidable"], p["nd"], p["extent"]) == (1, 2, len(req))
    assert walk(req[:4] + struct.pack("<Q", 1 << 60) + req[12:], keys44)["kind"] == HOST
    assert walk(b"", keys44)["kind"] == HOST and walk(b"\x01\x00\x00", keys44)["kind"] == HOST
