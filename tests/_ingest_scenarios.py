"""TEST INFRASTRUCTURE: the message batches of tests/test_gpu_msg_ingest.py
(copies of its _Signer, _Batch, the 32-message scenario and the 400-message
shapes, as plain functions) and the Python model of a message's receipt
(include/ntcrypto.h nt_msg_receipt), for the receipt tests.

The model comes from how each message was built -- tests/_wire.py objects,
hashlib, the oracle-driven model_sanitize -- never from the code under test.
A receipt is modelled as its 128 bytes (RECEIPT_STRUCT, spelled here on its
own; tests/test_msg_receipt_abi.py pins the package's dtype and the C header
against each other).
"""
import base64
import random
import struct

import numpy as np

import _wire as W

HOST = 0xFF
KIND_HEADER, KIND_VOTE, KIND_CERT, KIND_REQUEST = 0, 1, 2, 3
GENESIS = 1
# code kind flags | author origin np nq nv | round | off_payload off_parents off_id off_sig off_votes | id digest reserved
RECEIPT_STRUCT = struct.Struct("<BBH5IQ5I32s32s12s")
RECEIPT_FIELDS = ("code", "kind", "flags", "author", "origin", "np", "nq", "nv", "round", "off_payload",
                  "off_parents", "off_id", "off_sig", "off_votes", "id", "digest", "reserved")
assert RECEIPT_STRUCT.size == 128
HOST_RECEIPT = bytes([HOST, HOST]) + bytes(126)


def _rb(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


class Signer:
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


class Batch:
    """wire messages, the model's code per message, and the indices built irregular"""

    def __init__(self, signer, stakes, nworkers, gc_round, cur):
        self.s, self.stakes, self.nworkers, self.gc_round, self.cur = signer, stakes, nworkers, gc_round, cur
        self.com = W.Committee(signer.keys, stakes, nworkers)
        self.wires, self.expect, self.irregular, self.objs = [], [], set(), []
        self.named = {}

    def add(self, obj, irregular=False, wire=None, name=None):
        """obj None: bytes no decoder accepts (SerializationError on the host)"""
        if irregular:
            self.irregular.add(len(self.wires))
        if name:
            self.named[name] = len(self.wires)
        self.objs.append(obj)
        self.wires.append(W.message(obj) if wire is None else wire)
        self.expect.append(W.SERIALIZATION_ERROR if obj is None else
                           W.model_sanitize(self.com, self.gc_round, self.cur, obj, self.s.strict, self.s.batch))

    def regauged(self, gc_round):
        """the same messages under another GC round (the model's codes recomputed)"""
        b = Batch(self.s, self.stakes, self.nworkers, gc_round, self.cur)
        for i, (o, w) in enumerate(zip(self.objs, self.wires)):
            b.add(o, irregular=i in self.irregular, wire=w)
        b.named = dict(self.named)
        return b

    def raw_expect(self):
        """what the device call returns: the model's code, 0xff where the host must decide"""
        return [HOST if i in self.irregular else e for i, e in enumerate(self.expect)]

    def core(self, current=True):
        from ntcrypto import narwhal as N
        return N.Core(np.frombuffer(b"".join(self.s.keys), np.uint8), self.stakes, self.nworkers, self.gc_round,
                      W.message(self.cur) if current else None, True)

    def committee(self, be):
        """nt_committee over the same authorities (workers 0 .. nworkers[i] - 1)"""
        import ntcrypto
        ks = be.keyset(np.frombuffer(b"".join(self.s.keys), np.uint8))
        return ks, ntcrypto.Committee(ks, self.stakes, [list(range(w)) for w in self.nworkers], self.com.quorum())

    def cur_args(self):
        return dict(gc_round=self.gc_round, cur_id=self.cur.id, cur_round=self.cur.round, cur_author=self.cur.author)

    # ---- the receipt model --------------------------------------------------
    def index(self, pk):
        return self.s.keys.index(pk)

    def digest_slots(self, i):
        """the SHA-512 outputs the device holds for message i: slot i (a header's or
        certificate's header digest, a vote's digest) and slot n + i (a certificate's
        digest); a slot the receipt must not use is filled with 0xEE"""
        o, junk = self.objs[i], b"\xee" * 32
        if i in self.irregular or o is None:
            return junk, junk
        if isinstance(o, W.Header):
            return o.digest(), junk
        if isinstance(o, W.Vote):
            return o.digest(), junk
        if isinstance(o, W.Certificate):
            return o.header.digest(), o.digest()
        return junk, junk

    def indices(self, i):
        """(author, origin) committee indices of a message the device decides"""
        o = self.objs[i]
        if i in self.irregular or o is None:
            return 0, 0
        if isinstance(o, W.Vote):
            return self.index(o.author), self.index(o.origin)
        a = self.index(o.header.author if isinstance(o, W.Certificate) else o.author if isinstance(o, W.Header) else o[1])
        return a, a

    def receipt(self, i):
        """the 128 bytes of message i's receipt"""
        o = self.objs[i]
        if i in self.irregular or o is None:
            return HOST_RECEIPT
        code = self.expect[i]
        author, origin = self.indices(i)
        z = bytes(32)
        if isinstance(o, W.Vote):
            return RECEIPT_STRUCT.pack(code, KIND_VOTE, 0, author, origin, 0, 0, 0, o.round, 0, 0, 4, 148, 0, o.id,
                                       o.digest(), bytes(12))
        if isinstance(o, tuple):
            return RECEIPT_STRUCT.pack(code, KIND_REQUEST, 0, author, origin, 0, len(o[0]), 0, 0, 0, 12, 0, 0, 0, z, z,
                                       bytes(12))
        cert = isinstance(o, W.Certificate)
        h = o.header if cert else o
        np_, nq = len(h.payload), len(h.parents)
        off_par = 4 + 8 + 44 + 8 + 8 + 36 * np_ + 8
        off_id = off_par + 32 * nq
        genesis = cert and h.round == 0 and h.id == z and not h.round < self.gc_round
        assert not genesis or code == W.OK
        return RECEIPT_STRUCT.pack(code, KIND_CERT if cert else KIND_HEADER, GENESIS if genesis else 0, author, origin,
                                   np_, nq, len(o.votes) if cert else 0, h.round, 72 if np_ else 0, off_par, off_id,
                                   off_id + 32, off_id + 32 + 64 + 8 if cert else 0, h.id,
                                   o.digest() if cert else h.digest(), bytes(12))

    def receipts(self):
        return [self.receipt(i) for i in range(len(self.wires))]


def fields(rec):
    """a 128-byte record as a dict (bytes fields in hex), for assertion messages"""
    d = dict(zip(RECEIPT_FIELDS, RECEIPT_STRUCT.unpack(bytes(rec))))
    return {k: (v.hex() if isinstance(v, bytes) else v) for k, v in d.items()}


def receipt_diffs(got, want):
    """[(index, field, got, want)] over two lists of 128-byte records"""
    out = []
    for i, (g, w) in enumerate(zip(got, want)):
        if bytes(g) != bytes(w):
            fg, fw = fields(g), fields(w)
            out += [(i, k, fg[k], fw[k]) for k in RECEIPT_FIELDS if fg[k] != fw[k]]
    return out


def check_in_place(batch, i, rec):
    """what a caller reads through record `rec` of message i in its own wire bytes"""
    o, w = batch.objs[i], batch.wires[i]
    r = dict(zip(RECEIPT_FIELDS, RECEIPT_STRUCT.unpack(bytes(rec))))
    if r["kind"] == HOST:
        return
    if isinstance(o, tuple):
        assert [w[r["off_parents"] + 32 * k:r["off_parents"] + 32 * k + 32] for k in range(r["nq"])] == list(o[0]), i
        return
    assert w[r["off_id"]:r["off_id"] + 32] == r["id"], i
    assert w[r["off_sig"]:r["off_sig"] + 64] == (o.header.sig if isinstance(o, W.Certificate) else o.sig), i
    if isinstance(o, W.Vote):
        return
    h = o.header if isinstance(o, W.Certificate) else o
    par = [w[r["off_parents"] + 32 * k:r["off_parents"] + 32 * k + 32] for k in range(r["nq"])]
    assert par == sorted(h.parents), i
    pay = [w[r["off_payload"] + 36 * k:r["off_payload"] + 36 * k + 36] for k in range(r["np"])]
    assert pay == [d + struct.pack("<I", h.payload[d]) for d in sorted(h.payload)], i
    if isinstance(o, W.Certificate):
        for k, (pk, sig) in enumerate(o.votes):
            q = r["off_votes"] + 116 * k
            assert w[q + 8:q + 52] == base64.b64encode(pk) and w[q + 52:q + 116] == sig, (i, k)


def build_scenario(oracle):
    """test_gpu_msg_ingest.py's scenario: 7 keys, 32 messages, all 11 DagError values,
    9 irregular messages.  named: "bad_id" (the header whose id is not its digest) and
    "genesis" (a committee member's genesis certificate)."""
    rng = random.Random(2024)
    s = Signer(oracle, 7, 1)
    keys, stranger = s.keys, s.stranger
    gc_round, cur_round = 5, 8
    cur = s.header(rng, keys[0], cur_round)
    b = Batch(s, [1, 1, 1, 1, 2, 1, 0], [2] * 7, gc_round, cur)  # the last authority has no voting rights
    h = lambda *a, **k: s.header(rng, *a, **k)
    b.add(h(keys[1], 9))
    b.add(h(keys[2], 4))
    b.add(h(keys[1], 9, bad_sig=True))
    b.add(h(keys[1], 9, bad_id=True), name="bad_id")
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
    b.add(s.cert(W.Header(keys[3], 0, {}, set(), id_=bytes(32)), []), name="genesis")  # TooOld at GC round 5
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
    assert len(b.wires) == 32 and len(b.irregular) == 9 and set(b.expect) == set(range(11))
    return b


def build_shapes(oracle):
    """test_gpu_msg_ingest.py's shapes: 400 messages of a 10-key committee for chunks
    of 64: a seeded shuffle of kinds, then 64 votes only (a chunk whose vote total V is
    0), then 64 headers only, then a shuffle again.  Odd-length fillers and trailing
    bytes shift the alignment; headers with np = nq = 0 and with 70 parents; the last
    message ends at the buffer's last byte."""
    rng = random.Random(777)
    s = Signer(oracle, 10, 3)
    keys = s.keys
    cur = s.header(rng, keys[0], 20)
    b = Batch(s, [1] * 9 + [0], [2] * 10, 12, cur)
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
    assert len(b.wires) == 400
    return b
