"""An independent model of the worker's message ingestion (include/ntcrypto.h
nt_worker_messages_ingest): the two bincode layouts of WorkerMessage, the code
and the 64-byte receipt of every message, written from the format --

    Batch         u32 0 | u64 ntx | ntx x (u64 len_k | len_k bytes)
    BatchRequest  u32 1 | u64 nd  | nd x digest 32 | u64 44 | requestor b64 (44)

-- one field at a time, the way bincode reads them, with hashlib for the
digests; never from csrc/wmsg_plan.hpp.  Also the message builders and the
scenario lists the CPU and GPU tests share.
"""
import base64
import hashlib
import random
import struct

OK, SERIALIZATION, HOST = 0, 9, 0xFF
BATCH, REQUEST, NONE = 0, 1, 0xFF
MAX_DIGESTS, MAX_TX = 1 << 20, 1 << 24
U64 = (1 << 64) - 1
RECEIPT = struct.Struct("<BBHIQQII32s")       # code kind flags n used tx_bytes tx_len off_key digest
FIELDS = ("code", "kind", "flags", "n", "used", "tx_bytes", "tx_len", "off_key", "digest")
ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
assert RECEIPT.size == 64
# where lane 63 reads its prefix in the second round of a batch of >= 65 transactions that starts
# with 16-byte ones (speculation_shapes), and the message ends placed around and inside it
LANE63_PREFIX = (1548, 1556)
LANE63_ENDS = tuple(range(1546, 1559))


def _undecided(code):
    return RECEIPT.pack(code, NONE, 0, 0, 0, 0, 0, 0, bytes(32))


def receipt(msg, digest=True):
    """the 64 bytes nt_worker_messages_ingest writes for `msg` (digest=False: an accepted
    batch's digest left zero, what the walk alone knows)"""
    msg = bytes(msg)
    L = len(msg)
    if L < 4:
        return _undecided(SERIALIZATION)
    tag = struct.unpack_from("<I", msg, 0)[0]
    if tag > 1 or L < 12:
        return _undecided(SERIALIZATION)
    count = struct.unpack_from("<Q", msg, 4)[0]
    if tag == 0:
        if 12 + 8 * count > L:                    # Python integers: nothing wraps
            return _undecided(SERIALIZATION)
        if count > MAX_TX:
            return _undecided(HOST)
        pos, lens = 12, []
        for _ in range(count):
            if pos + 8 > L:
                return _undecided(SERIALIZATION)
            n = struct.unpack_from("<Q", msg, pos)[0]
            if pos + 8 + n > L:
                return _undecided(SERIALIZATION)
            lens.append(n)
            pos += 8 + n
        uniform = count >= 1 and len(set(lens)) == 1
        dig = hashlib.sha512(msg).digest()[:32] if digest else bytes(32)
        return RECEIPT.pack(OK, BATCH, 1 if uniform else 0, count, pos, sum(lens), lens[0] if uniform else 0, 0, dig)
    if 12 + 32 * count > L:
        return _undecided(SERIALIZATION)
    if count > MAX_DIGESTS:
        return _undecided(HOST)
    pos = 12 + 32 * count
    if pos + 8 > L:
        return _undecided(SERIALIZATION)
    klen = struct.unpack_from("<Q", msg, pos)[0]
    if pos + 8 + klen > L:
        return _undecided(SERIALIZATION)
    if klen != 44:
        return _undecided(HOST)
    text = msg[pos + 8:pos + 52]
    if any(c not in ALPHABET for c in text[:43]) or text[43:] != b"=":
        return _undecided(HOST)
    key = base64.b64decode(text)
    if base64.b64encode(key) != text:             # trailing bits set: not the canonical text
        return _undecided(HOST)
    assert len(key) == 32
    return RECEIPT.pack(OK, REQUEST, 0, count, pos + 52, 0, 0, pos + 8, key)


def code(msg):
    return receipt(msg, digest=False)[0]


def fields(rec):
    return dict(zip(FIELDS, RECEIPT.unpack(bytes(rec))))


# ---- builders ----
def batch(txs):
    return struct.pack("<IQ", 0, len(txs)) + b"".join(struct.pack("<Q", len(t)) + bytes(t) for t in txs)


def request(digests, key=None, text=None):
    """text: the requestor string as written (default: the canonical base64 of `key`)"""
    text = base64.b64encode(key) if text is None else text
    return struct.pack("<IQ", 1, len(digests)) + b"".join(digests) + struct.pack("<Q", len(text)) + text


def _rb(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def speculation_shapes(rng):
    """[(name, message)]: the smallest batches at which a 64-lane speculative walk can go wrong"""
    out = []
    for ntx in (0, 1, 63, 64, 65, 128, 129):
        for ln in (0, 1, 512):
            out.append(("uniform_%d_x_%d" % (ntx, ln), batch([_rb(rng, ln) for _ in range(ntx)])))
    for at in (0, 1, 62, 63, 64, 129):               # 130 transactions of 16 bytes, one of 17
        out.append(("odd_at_%d" % at, batch([_rb(rng, 17 if k == at else 16) for k in range(130)])))
    out.append(("all_different", batch([_rb(rng, k) for k in range(131)])))
    out.append(("all_different_down", batch([_rb(rng, 140 - k) for k in range(131)])))
    out.append(("runs", batch([_rb(rng, 8 * (k // 70)) for k in range(200)])))
    # after one round the hypothesis is 16 (stride 24) at p = 36 with 63 transactions left: lane 62
    # reads at 1524.  50 transactions of 16 bytes and 14 empty ones end at 1324; trailing bytes put
    # the end of the message inside, just before and just after that prefix
    short = batch([_rb(rng, 16)] * 50 + [b""] * 14)
    assert len(short) == 1324
    for end in range(1523, 1534):
        out.append(("straddle_end_%d" % end, short + _rb(rng, end - 1324)))
    # the same with the message cut there: the 64 transactions are claimed, the bytes are not
    full = batch([_rb(rng, 16) for _ in range(64)])
    for end in (1524, 1527, 1531, 1532, 1547, 1548):
        out.append(("straddle_cut_%d" % end, full[:end]))
    # Lane 63, the ballot's top bit.  With 65 transactions or more, 64 are left after the first round
    # (hypothesis 0, the first prefix 16: one proven, p = 36, hypothesis 16, stride 24), so all 64 lanes
    # vote and lane 63 reads at 36 + 63 * 24 = 1548.  One message per byte of that prefix [1548, 1556),
    # one ending just before it and just after, and the same one byte further out on each side:
    # a valid batch (50 transactions of 16 bytes and 15 empty ones end at 1332) with trailing bytes ...
    short65 = batch([_rb(rng, 16)] * 50 + [b""] * 15)
    assert len(short65) == 1332 and LANE63_PREFIX == (36 + 63 * 24, 36 + 63 * 24 + 8) == (1548, 1556)
    for end in LANE63_ENDS:
        out.append(("lane63_end_%d" % end, short65 + _rb(rng, end - 1332)))
    # ... and 65 (and 130) transactions of 16 bytes cut there: lanes 0 .. 62 agree, lane 63 reads
    # nothing or a whole prefix whose transaction does not fit
    full65, full130 = batch([_rb(rng, 16) for _ in range(65)]), batch([_rb(rng, 16) for _ in range(130)])
    assert len(full65) == 12 + 65 * 24
    for end in LANE63_ENDS:
        out.append(("lane63_cut_%d" % end, full65[:end]))
        out.append(("lane63_cut130_%d" % end, full130[:end]))
    # the value 16 inside transaction data where the speculated positions land: five transactions
    # of 16, then one of 40 / 41 / 64 whose data holds u64 16 at every 8 bytes, then 16s again
    for mid in (40, 41, 64, 16):
        txs = [_rb(rng, 16) for _ in range(5)] + [(struct.pack("<Q", 16) * 9)[:mid]] + [_rb(rng, 16) for _ in range(70)]
        out.append(("coincidence_%d" % mid, batch(txs)))
    # ... and where the data spells a prefix that would run to exactly the end of the message
    txs = [_rb(rng, 16) for _ in range(3)] + [bytes(16) + struct.pack("<Q", 16) + bytes(24)] + [_rb(rng, 16)] * 3
    out.append(("coincidence_in_data", batch(txs)))
    return out


def key_cases(rng):
    """[(name, message)]: requests"""
    key = _rb(rng, 32)
    text = base64.b64encode(key)
    d = [_rb(rng, 32) for _ in range(3)]
    out = [("request_%d" % nd, request(d[:nd], key)) for nd in (0, 1, 3)]
    out.append(("request_trailing", request(d, key) + b"tail"))
    out.append(("request_key_43", request(d[:1], text=text[:43])))
    out.append(("request_key_45", request(d[:1], text=text + b"=")))
    out.append(("request_key_0", request(d[:1], text=b"")))
    for bad in (b"-", b"_", b" ", b"\x00", b"\xc3", b"="):
        out.append(("request_alphabet_%02x" % bad[0], request(d[:1], text=text[:7] + bad + text[8:])))
    out.append(("request_no_pad", request(d[:1], text=text[:43] + b"A")))
    out.append(("request_early_pad", request(d[:1], text=text[:42] + b"==")))
    v = ALPHABET.index(text[42:43])
    for bits in (1, 2, 3):                           # the 43rd character carries two unused bits
        out.append(("request_trailing_bits_%d" % bits, request(d[:1], text=text[:42] + ALPHABET[v | bits:(v | bits) + 1] + b"=")))
    out.append(("request_cap_plus_1_claimed", request(d[:1], key)[:4] + struct.pack("<Q", MAX_DIGESTS + 1) + request(d[:1], key)[12:]))
    whole = request(d, key)
    for cut in (11, 12, 13, 12 + 95, 12 + 96, 12 + 96 + 7, 12 + 96 + 8, 12 + 96 + 8 + 43):
        out.append(("request_cut_%d" % cut, whole[:cut]))
    for x in (U64, U64 - 7, U64 - 51, 1 << 63, 45 + (1 << 32)):
        out.append(("request_key_len_%x" % x, whole[:12 + 96] + struct.pack("<Q", x) + whole[12 + 96 + 8:]))
        out.append(("request_nd_%x" % x, whole[:4] + struct.pack("<Q", x) + whole[12:]))
    return out


def edge_cases(rng):
    """[(name, message)]: tags, tiny lengths, truncations, trailing bytes, prefixes near 2^64"""
    small = batch([_rb(rng, n) for n in (5, 0, 9, 9, 1)])
    out = [("len_%d" % n, small[:n]) for n in range(4)]
    out += [("tag_2", struct.pack("<I", 2) + small[4:]), ("tag_ffffffff", struct.pack("<I", 0xFFFFFFFF) + small[4:]),
            ("tag_256", struct.pack("<I", 256) + small[4:])]
    out += [("batch_cut_%d" % cut, small[:cut]) for cut in range(4, len(small))]
    out += [("batch_trailing_%d" % n, small + _rb(rng, n)) for n in (1, 7, 8, 64)]
    first = 12
    for x in (U64, U64 - 7, U64 - 8, U64 - 19, U64 - 20, U64 - 11, 1 << 63, 1 << 56, (1 << 56) - 1, 1 << 32,
              len(small) - 20, len(small) - 19):
        out.append(("batch_prefix_%x" % x, small[:first] + struct.pack("<Q", x) + small[first + 8:]))
        out.append(("batch_ntx_%x" % x, small[:4] + struct.pack("<Q", x) + small[12:]))
    # a later prefix, after a round that proved some: 70 transactions of 4 bytes, number 66 overwritten
    many = batch([_rb(rng, 4) for _ in range(70)])
    at = 12 + 66 * 12
    for x in (U64, U64 - at, U64 - at - 7, U64 - at - 8, len(many) - at - 8, len(many) - at - 7):
        out.append(("batch_late_prefix_%x" % x, many[:at] + struct.pack("<Q", x) + many[at + 8:]))
    return out


def scenario(seed=20260701):
    """about 200 named messages: every shape above"""
    rng = random.Random(seed)
    items = speculation_shapes(rng) + key_cases(rng) + edge_cases(rng)
    names = [n for n, _ in items]
    assert len(set(names)) == len(names)
    return items
