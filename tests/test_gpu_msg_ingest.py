"""nt_primary_messages_ingest: the whole PrimaryMessage drain -- headers, votes,
certificates, requests -- parsed and decided on the device from wire bytes
(k_ingest.hip, csrc/msg_plan.hpp), through Core.ingest(device="all") and
Committee.ingest_messages.

Expected codes come from tests/_wire.py's model_sanitize driven by the CPU
oracle's signature verdicts, never from the code under test; the host SoA path
(Core.ingest) is cross-checked against the same codes.  Which messages the
device leaves to the host (0xff) is computed from how each message was built.
"""
import os
import random
import struct
import sys

import numpy as np
import pytest

import _wire as W

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "narwhal-tusk_amd"))
import ntcrypto  # noqa: E402
from ntcrypto import narwhal as N  # noqa: E402

HOST = 0xFF
pytestmark = pytest.mark.gpu


def _rb(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


class _Signer:
    """keys of a small committee + a stranger; signatures and verdicts from the CPU oracle"""

    def __init__(self, orc, nkeys, tag):
        self.orc = orc
        seeds = [bytes([i + 1, tag]) * 16 for i in range(nkeys)]
        self.keys = [orc.pubkey(s) for s in seeds]
        self.sk = dict(zip(self.keys, seeds))
        self.stranger = orc.pubkey(b"\x55" * 32)
        self.sk[self.stranger] = b"\x55" * 32

    def sign(self, pk, d):
        return self.orc.sign(self.sk[pk], pk, d)

    def strict(self, d, pk, s):
        return self.orc.verify_strict(pk, s, d)

    def batch(self, d, votes):
        return self.orc.verify_batch([v[0] for v in votes], [v[1] for v in votes], d)

    def header(self, rng, author, rnd, nworker=0, bad_sig=False, bad_id=False, np_=2, nq=3):
        h = W.Header(author, rnd, {_rb(rng, 32): (nworker if k == 0 else 0) for k in range(np_)},
                     {_rb(rng, 32) for _ in range(nq)})
        if bad_id:
            h.id = _rb(rng, 32)
        h.sig = self.sign(author, h.id)
        if bad_sig:
            h.sig = h.sig[:40] + bytes([h.sig[40] ^ 1]) + h.sig[41:]
        return h

    def vote(self, author, target, rnd=None, bad_sig=False, origin=None, id_=None):
        v = W.Vote(target.id if id_ is None else id_, target.round if rnd is None else rnd,
                   target.author if origin is None else origin, author)
        v.sig = self.sign(author, v.digest())
        if bad_sig:
            v.sig = v.sig[:33] + bytes([v.sig[33] ^ 4]) + v.sig[34:]
        return v

    def cert(self, h, voters, bad_vote=None):
        c = W.Certificate(h, [])
        d = c.digest()
        for pk in voters:
            s = self.sign(pk, d)
            if bad_vote is not None and pk == bad_vote:
                s = bytes(32) + s[32:]
            c.votes.append((pk, s))
        return c


class _Batch:
    """wire messages, the model's code per message, and the indices built irregular"""

    def __init__(self, signer, stakes, nworkers, gc_round, cur):
        self.s, self.stakes, self.nworkers, self.gc_round, self.cur = signer, stakes, nworkers, gc_round, cur
        self.com = W.Committee(signer.keys, stakes, nworkers)
        self.wires, self.expect, self.irregular, self.objs = [], [], set(), []

    def add(self, obj, irregular=False, wire=None):
        """obj None: bytes no decoder accepts (SerializationError on the host)"""
        if irregular:
            self.irregular.add(len(self.wires))
        self.objs.append(obj)
        self.wires.append(W.message(obj) if wire is None else wire)
        self.expect.append(W.SERIALIZATION_ERROR if obj is None else
                           W.model_sanitize(self.com, self.gc_round, self.cur, obj, self.s.strict, self.s.batch))

    def raw_expect(self):
        """what the device call returns: the model's code, 0xff where the host must decide"""
        return [HOST if i in self.irregular else e for i, e in enumerate(self.expect)]

    def core(self, current=True):
        return N.Core(np.frombuffer(b"".join(self.s.keys), np.uint8), self.stakes, self.nworkers, self.gc_round,
                      W.message(self.cur) if current else None, True)

    def committee(self, be):
        """nt_committee over the same authorities (workers 0 .. nworkers[i] - 1)"""
        ks = be.keyset(np.frombuffer(b"".join(self.s.keys), np.uint8))
        return ks, ntcrypto.Committee(ks, self.stakes, [list(range(w)) for w in self.nworkers], self.com.quorum())

    def cur_args(self):
        return dict(gc_round=self.gc_round, cur_id=self.cur.id, cur_round=self.cur.round, cur_author=self.cur.author)


def _names(codes):
    return ["host" if c == HOST else N.DAG_ERRORS[c] for c in codes]


@pytest.fixture(scope="module")
def scenario(oracle):
    """test_wire.py::_scenario's messages, plus a vote whose origin and a request
    whose requestor is the stranger; every message that names the stranger, the
    two undecodable ones and the non-canonical header are marked irregular."""
    rng = random.Random(2024)
    s = _Signer(oracle, 7, 1)
    keys, stranger = s.keys, s.stranger
    gc_round, cur_round = 5, 8
    cur = s.header(rng, keys[0], cur_round)
    b = _Batch(s, [1, 1, 1, 1, 2, 1, 0], [2] * 7, gc_round, cur)  # the last authority has no voting rights
    h = lambda *a, **k: s.header(rng, *a, **k)
    b.add(h(keys[1], 9))
    b.add(h(keys[2], 4))
    b.add(h(keys[1], 9, bad_sig=True))
    b.add(h(keys[1], 9, bad_id=True))
    b.add(h(stranger, 9), irregular=True)
    b.add(h(keys[6], 9))
    b.add(h(keys[3], 9, nworker=5))
    b.add(s.vote(keys[2], cur))
    b.add(s.vote(keys[3], cur, rnd=7))
    b.add(s.vote(keys[4], h(keys[1], cur_round)))
    b.add(s.vote(stranger, cur), irregular=True)
    b.add(s.vote(keys[6], cur))
    b.add(s.vote(keys[5], cur, bad_sig=True))
    b.add(s.vote(keys[1], cur, rnd=9))
    b.add(s.vote(keys[1], h(stranger, cur_round)), irregular=True)           # the stranger as origin
    b.add(s.cert(h(keys[2], 9), keys[:5]))
    b.add(s.cert(h(keys[2], 3), keys[:5]))
    b.add(s.cert(W.Header(keys[3], 0, {}, set(), id_=bytes(32)), []))        # genesis (TooOld at GC round 5)
    b.add(s.cert(h(keys[2], 9, bad_sig=True), keys[:5]))
    b.add(s.cert(h(keys[2], 9), keys[:3]))
    b.add(s.cert(h(keys[2], 9), keys[:4] + [keys[1]]))
    b.add(s.cert(h(keys[2], 9), keys[:4] + [stranger]), irregular=True)
    b.add(s.cert(h(keys[2], 9), keys[:5], bad_vote=keys[3]))
    b.add(s.cert(h(keys[5], 10), keys[1:6]))
    b.add(([_rb(rng, 32)], keys[1]))
    b.add(([_rb(rng, 32), _rb(rng, 32)], stranger), irregular=True)          # the stranger as requestor
    b.add(s.cert(h(keys[2], 9, bad_sig=True), keys[:3]))
    b.add(s.cert(h(keys[2], 9, bad_sig=True), keys[:4] + [keys[1]]))
    b.add(s.cert(h(keys[2], 9, bad_sig=True), keys[:4] + [stranger]), irregular=True)
    b.add(None, irregular=True, wire=b"\x02\x00\x00\x00garbage")
    b.add(None, irregular=True, wire=b"")
    # a valid header whose payload entries arrive in descending order: the decoder's
    # BTreeMap sorts them, so the id still matches -- but not canonical bytes
    hd = h(keys[3], 9)
    body = hd.encode()
    a = 8 + 44 + 8 + 8
    ents = [body[a + 36 * k:a + 36 * (k + 1)] for k in range(len(hd.payload))]
    b.add(hd, irregular=True, wire=W.message(hd)[:4] + body[:a] + b"".join(ents[::-1]) + body[a + 36 * len(ents):])
    return b


def test_every_outcome_every_kind(scenario, monkeypatch):
    monkeypatch.setenv("NT_KEYSET_COMB_BITS", "16")
    b = scenario
    assert set(b.expect) == set(range(11))  # all 11 DagError values occur
    core = b.core()
    try:
        soa, _ = core.ingest(*N.pack(b.wires), threads=3)
        assert _names(soa) == _names(b.expect)
        got, host = core.ingest(*N.pack(b.wires), threads=3, device="all")
        assert _names(got) == _names(b.expect)
        assert host == len(b.irregular)
    finally:
        core.close()
    be = ntcrypto.Backend(device=0)
    try:
        ks, cm = b.committee(be)
        raw = cm.ingest_messages(b.wires, **b.cur_args())
        print("device codes:", _names(raw))
        assert _names(raw) == _names(b.raw_expect())
        # exactly the messages built irregular are left to the host, nothing else
        assert {i for i, c in enumerate(raw) if c == HOST} == b.irregular
        cm.close()
        ks.close()
    finally:
        be.close()


def test_unchanged_certificate_path(scenario, monkeypatch):
    """nt_certificates_ingest on the mixed batch: 0xff for every non-certificate,
    and for certificates the code the new call gives."""
    monkeypatch.setenv("NT_KEYSET_COMB_BITS", "16")
    b = scenario
    be = ntcrypto.Backend(device=0)
    try:
        ks, cm = b.committee(be)
        old = cm.ingest(b.wires, b.gc_round)
        new = cm.ingest_messages(b.wires, **b.cur_args())
        ncert = 0
        for i, o in enumerate(b.objs):
            if isinstance(o, W.Certificate):
                ncert += 1
                assert old[i] == new[i] == b.raw_expect()[i], (i, old[i], new[i])
            else:
                assert old[i] == HOST, (i, old[i])
        assert ncert == 12
        cm.close()
        ks.close()
    finally:
        be.close()


def test_rules_easy_to_get_wrong(oracle, monkeypatch):
    monkeypatch.setenv("NT_KEYSET_COMB_BITS", "16")
    rng = random.Random(31337)
    s = _Signer(oracle, 7, 2)
    keys = s.keys
    cur = s.header(rng, keys[0], 8)
    b = _Batch(s, [1, 1, 1, 1, 2, 1, 0], [2] * 7, 0, cur)
    zero = W.Header(keys[2], 0, {}, set(), id_=bytes(32))
    zero.sig = s.sign(keys[2], zero.id)
    cases = [
        (zero, W.INVALID_HEADER_ID),                                         # genesis is a certificate rule
        (s.vote(keys[1], cur, rnd=7, id_=_rb(rng, 32)), W.TOO_OLD),           # the round filter comes first
        (s.vote(keys[1], cur, rnd=9), W.UNEXPECTED_VOTE),
        (s.vote(keys[6], cur), W.UNKNOWN_AUTHORITY),                         # a zero-stake voter, the right header
        (s.vote(keys[1], cur, origin=keys[3]), W.UNEXPECTED_VOTE),           # another member as origin
        (s.vote(keys[1], cur), W.OK),
        (s.header(rng, keys[1], 3), W.OK),
    ]
    for obj, want in cases:
        b.add(obj)
        assert b.expect[-1] == want, (len(b.expect), b.expect[-1], want)    # the model agrees with the issue's table
    n0 = len(b.wires)
    for i in (5, 6, 0, 3):                                                   # a vote and headers + 5 trailing bytes
        b.add(b.objs[i], wire=b.wires[i] + b"\x01\x02\x03\x04\x05")
    b.add(None, irregular=True, wire=b.wires[6][:-1])                        # a header truncated by one byte
    b.add(None, irregular=True, wire=b.wires[5][:211])                       # a 211-byte vote
    assert len(b.wires[5]) == 212
    assert b.expect[n0:n0 + 4] == [b.expect[i] for i in (5, 6, 0, 3)]
    # with no current header (Header::default()): every vote UnexpectedVote or TooOld
    nul = _Batch(s, b.stakes, b.nworkers, 0, W.Header(bytes(32), 0, {}, set(), id_=bytes(32)))
    for o in b.objs:
        if isinstance(o, W.Vote):
            nul.add(o)
    nul.add(W.Vote(bytes(32), 0, bytes(32), keys[1], s.sign(keys[1], W.Vote(bytes(32), 0, bytes(32), keys[1]).digest())),
            irregular=True)                                                  # the zero key is no committee key
    assert set(nul.expect[:-1]) <= {W.UNEXPECTED_VOTE, W.TOO_OLD}
    for batch, current in ((b, True), (nul, False)):
        core = batch.core(current)
        try:
            got, host = core.ingest(*N.pack(batch.wires), threads=2, device="all")
            soa, _ = core.ingest(*N.pack(batch.wires), threads=2)
        finally:
            core.close()
        assert _names(got) == _names(batch.expect) == _names(soa)
        assert host == len(batch.irregular)
    be = ntcrypto.Backend(device=0)
    try:
        ks, cm = b.committee(be)
        raw = cm.ingest_messages(b.wires, **b.cur_args())
        assert _names(raw) == _names(b.raw_expect())
        raw = cm.ingest_messages(nul.wires, gc_round=0)                      # NULL id and author
        assert _names(raw) == _names(nul.raw_expect())
        cm.close()
        ks.close()
    finally:
        be.close()


def test_device_all_vs_host_on_mutations(scenario, monkeypatch):
    """Mutated messages of every kind (a flipped bit in a key, count, digest, round or
    signature; truncations; trailing bytes): the device pass plus the host decoder for
    what it leaves give the DagError the host SoA path gives alone."""
    monkeypatch.setenv("NT_KEYSET_COMB_BITS", "16")
    monkeypatch.setenv("NT_INGEST_CHUNK", "512")
    rng = random.Random(99)
    seeds = [w for i, w in enumerate(scenario.wires) if i not in scenario.irregular]
    batch = []
    for it in range(3000):
        m = bytearray(rng.choice(seeds))
        if it % 4 == 0:
            m[rng.randrange(len(m))] ^= 1 << rng.randrange(8)
        elif it % 4 == 1:
            m = m[:rng.randrange(1, len(m) + 1)]
        elif it % 4 == 2:
            m += _rb(rng, rng.randrange(1, 9))
        batch.append(bytes(m))
    core = scenario.core()
    try:
        a, _ = core.ingest(*N.pack(batch), threads=4)
        c, host = core.ingest(*N.pack(batch), threads=4, device="all")
    finally:
        core.close()
    diff = [(i, N.DAG_ERRORS[x], N.DAG_ERRORS[y]) for i, (x, y) in enumerate(zip(a, c)) if x != y]
    assert not diff, diff[:10]
    assert host < len(batch) // 2 and len(set(a.tolist())) >= 10, (host, set(a.tolist()))


@pytest.fixture(scope="module")
def shapes(oracle):
    """About 400 messages of a 10-key committee for chunks of 64: a seeded shuffle
    of kinds, then 64 votes only (a chunk whose vote total V is 0), then 64 headers
    only, then a shuffle again.  Odd-length fillers and trailing bytes shift the
    alignment; headers with np = nq = 0 and with 70 parents; the last message ends
    at the buffer's last byte."""
    rng = random.Random(777)
    s = _Signer(oracle, 10, 3)
    keys = s.keys
    cur = s.header(rng, keys[0], 20)
    b = _Batch(s, [1] * 9 + [0], [2] * 10, 12, cur)
    count = [0]

    def one(kind):
        k = count[0]
        count[0] += 1
        author = keys[1 + rng.randrange(9)]                                  # keys[9] has no stake
        if kind == "header":
            shape = k % 4
            obj = s.header(rng, author, 12 + rng.randrange(4) - (k % 11 == 0), nworker=3 if k % 13 == 0 else 0,
                           bad_sig=k % 5 == 0, bad_id=k % 7 == 0, np_=0 if shape == 0 else 1 + rng.randrange(4),
                           nq=(0, 70, 3, 7)[shape])
        elif kind == "vote":
            obj = s.vote(author, cur, rnd=19 if k % 9 == 0 else 21 if k % 6 == 0 else None, bad_sig=k % 4 == 0,
                         origin=keys[2] if k % 10 == 0 else None)
        elif kind == "cert":
            voters = rng.sample(keys[:9], 7)
            if k % 5 == 0:
                voters = voters[:6]
            obj = s.cert(s.header(rng, author, 13, np_=rng.randrange(3), nq=rng.choice([0, 7, 70])), voters,
                         bad_vote=voters[2] if k % 4 == 0 else None)
        elif kind == "request":
            obj = ([_rb(rng, 32) for _ in range(rng.randrange(3))], author)
        else:                                                                # a filler no decoder accepts, odd length
            return b.add(None, irregular=True, wire=struct.pack("<I", 7) + _rb(rng, 2 * rng.randrange(20) + 1))
        # bytes after a complete message are allowed: 0-3 of them on every other message
        b.add(obj, wire=W.message(obj) + _rb(rng, (k // 2) % 4 if k % 2 else 0))

    mix = ["header"] * 3 + ["vote"] * 3 + ["cert"] * 2 + ["request", "filler"]
    for _ in range(64):
        one(rng.choice(mix))
    for _ in range(64):
        one("vote")
    for _ in range(64):
        one("header")
    for _ in range(207):
        one(rng.choice(mix))
    v = s.vote(keys[3], cur)
    b.add(v)                                                                 # ends at the buffer's last byte
    return b


def test_shapes_chunks_alignment_sharding(shapes, monkeypatch):
    monkeypatch.setenv("NT_KEYSET_COMB_BITS", "16")
    monkeypatch.setenv("NT_INGEST_CHUNK", "64")
    b = shapes
    n = len(b.wires)
    assert n == 400
    off = np.concatenate([[0], np.cumsum([len(w) for w in b.wires])[:-1]])
    assert {int(o) % 4 for o in off} == {0, 1, 2, 3}
    assert all(isinstance(o, W.Vote) for o in b.objs[64:128]) and all(isinstance(o, W.Header) for o in b.objs[128:192])
    hdrs = [o for o in b.objs if isinstance(o, W.Header)]
    assert any(not o.payload and not o.parents for o in hdrs) and any(len(o.parents) == 70 for o in hdrs)
    assert b.irregular and len(set(b.expect)) >= 8, set(b.expect)
    want = _names(b.raw_expect())
    first_of = {}
    for i, o in enumerate(b.objs):
        first_of.setdefault(type(o).__name__, i)
    assert len(first_of) == 5                                                # Header, Vote, Certificate, tuple, NoneType
    for devices in ([0], [0, 0]):                                            # [0, 0]: a shard boundary at message 200
        be = ntcrypto.Backend(devices=devices)
        try:
            ks, cm = b.committee(be)
            raw = cm.ingest_messages(b.wires, **b.cur_args())
            diff = [(i, want[i], g) for i, g in enumerate(_names(raw)) if g != want[i]]
            assert not diff, (devices, diff[:10])
            for i in first_of.values():                                      # one call of n = 1 per kind
                one = cm.ingest_messages([b.wires[i]], **b.cur_args())
                assert _names(one) == [want[i]], (devices, i)
            old = cm.ingest(b.wires, b.gc_round)                             # the certificate-only call, same chunks
            for i, o in enumerate(b.objs):
                assert old[i] == (raw[i] if isinstance(o, W.Certificate) else HOST), i
            cm.close()
            ks.close()
        finally:
            be.close()
    core = b.core()
    try:
        got, host = core.ingest(*N.pack(b.wires), threads=4, device="all")
        soa, _ = core.ingest(*N.pack(b.wires), threads=4)
    finally:
        core.close()
    assert _names(got) == _names(b.expect) == _names(soa)
    assert host == len(b.irregular)
