"""nt_primary_messages_ingest_receipts: the receipt of every message of the
drain -- ids, digests and layout -- written on the device (k_ingest.hip
k_msg_receipt, csrc/msg_receipt.hpp), through Committee.ingest_messages(...,
receipts=True) and Core.ingest(..., device="all", receipts=True).

Every expectation comes from tests/_ingest_scenarios.py: tests/_wire.py objects,
hashlib and the oracle-driven model_sanitize, never from the code under test.
"""
import numpy as np
import pytest

import _ingest_scenarios as S
import ntcrypto
from ntcrypto import narwhal as N

HOST = S.HOST
W = S.W
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenario(oracle):
    return S.build_scenario(oracle)


@pytest.fixture(scope="module")
def shapes(oracle):
    return S.build_shapes(oracle)


def _rows(rec):
    """a RECEIPT_DTYPE array as a list of 128-byte strings"""
    assert rec.dtype == ntcrypto.RECEIPT_DTYPE and rec.dtype.itemsize == 128
    raw = rec.tobytes()
    return [raw[128 * i:128 * (i + 1)] for i in range(len(rec))]


def _check(batch, codes, rec):
    """codes and receipts of one device call against the model, with no exclusions"""
    assert list(codes) == batch.raw_expect()
    got = _rows(rec)
    diffs = S.receipt_diffs(got, batch.receipts())
    assert not diffs, diffs[:10]
    for i, r in enumerate(got):
        S.check_in_place(batch, i, r)
    return got


def test_scenario_receipts(scenario, monkeypatch):
    monkeypatch.setenv("NT_KEYSET_COMB_BITS", "16")
    b = scenario
    n = len(b.wires)
    be = ntcrypto.Backend(device=0)
    try:
        ks, cm = b.committee(be)
        plain = cm.ingest_messages(b.wires, **b.cur_args()).copy()
        rec = np.frombuffer(bytearray(b"\xab" * (128 * n)), ntcrypto.RECEIPT_DTYPE)
        codes, out = cm.ingest_messages(b.wires, receipts=rec, **b.cur_args())
        assert out.ctypes.data == rec.ctypes.data
        assert list(codes) == list(plain)                                    # the codes of the call without receipts
        got = _check(b, codes, rec)
        for i in range(n):
            if i in b.irregular:                                             # 0xff, 0xff and 126 zero bytes
                assert (rec["code"][i], rec["kind"][i]) == (HOST, HOST) and got[i] == S.HOST_RECEIPT, i
            else:
                assert rec["code"][i] == codes[i] != HOST and rec["kind"][i] != HOST, i
        # every row was written: no byte of the fill is left -- the only 0xab bytes are the ones the
        # model's random ids and digests hold themselves, and never two running
        assert rec.tobytes().count(b"\xab") == sum(r.count(b"\xab") for r in b.receipts())
        assert b"\xab\xab" not in rec.tobytes()
        assert not any(set(r[116:]) - {0} for r in got)                      # reserved
        bad = b.named["bad_id"]
        assert codes[bad] == W.INVALID_HEADER_ID and bytes(rec["digest"][bad]) != bytes(rec["id"][bad])
        assert bytes(rec["digest"][bad]) == b.objs[bad].digest()
        g = b.named["genesis"]
        assert (codes[g], rec["flags"][g]) == (W.TOO_OLD, 0)                 # GC round 5 filters it first
        # the genesis certificate under its own GC round 0, where it is accepted
        b0 = b.regauged(0)
        assert b0.expect[g] == W.OK
        codes0, rec0 = cm.ingest_messages(b0.wires, receipts=True, **b0.cur_args())
        _check(b0, codes0, rec0)
        assert (codes0[g], rec0["flags"][g], rec0["kind"][g]) == (W.OK, ntcrypto.RECEIPT_GENESIS, 2)
        assert int(rec0["flags"].sum()) == 1
        with pytest.raises(ValueError):
            cm.ingest_messages(b.wires, receipts=np.zeros(n + 1, ntcrypto.RECEIPT_DTYPE), **b.cur_args())
        cm.close()
        ks.close()
    finally:
        be.close()


def test_null_receipts_is_refused(scenario, monkeypatch):
    monkeypatch.setenv("NT_KEYSET_COMB_BITS", "16")
    import ctypes
    b = scenario
    be = ntcrypto.Backend(device=0)
    try:
        ks, cm = b.committee(be)
        data, off, ln, out = cm._packed(b.wires[:3])
        u8, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
        rc = be.lib.nt_primary_messages_ingest_receipts(be.ctx, cm.h, data.ctypes.data_as(u8), off.ctypes.data_as(u64),
                                                        ln.ctypes.data_as(u64), 3, 0, None, 0, None,
                                                        out.ctypes.data_as(u8), None)
        assert rc == -1                                                      # NT_EINVAL
        codes, rec = cm.ingest_messages([], receipts=True)                   # n = 0: nothing to write
        assert len(codes) == 0 and len(rec) == 0
        cm.close()
        ks.close()
    finally:
        be.close()


def test_shapes_chunks_alignment_sharding(shapes, monkeypatch):
    """400 messages in chunks of 64: seven chunks, so both lanes' side buffers are
    reused three times; a chunk of votes only (V = 0), one of headers only; every
    start alignment; a shard boundary at message 200 with devices=[0, 0]."""
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
    assert any(len(w) > len(W.message(o)) for w, o in zip(b.wires, b.objs) if o is not None)   # trailing bytes
    assert b.irregular and len(set(b.expect)) >= 8, set(b.expect)
    want = b.receipts()
    first_of = {}
    for i, o in enumerate(b.objs):
        first_of.setdefault(type(o).__name__, i)
    assert len(first_of) == 5                                                # Header, Vote, Certificate, tuple, NoneType
    runs = []
    for devices in ([0], [0, 0]):
        be = ntcrypto.Backend(devices=devices)
        try:
            ks, cm = b.committee(be)
            codes, rec = cm.ingest_messages(b.wires, receipts=True, **b.cur_args())
            runs.append((codes.tobytes(), rec.tobytes()))
            _check(b, codes, rec)
            for i in first_of.values():                                      # one call of n = 1 per kind
                c1, r1 = cm.ingest_messages([b.wires[i]], receipts=True, **b.cur_args())
                assert list(c1) == [b.raw_expect()[i]] and _rows(r1) == [want[i]], (devices, i)
            cm.close()
            ks.close()
        finally:
            be.close()
    assert runs[0] == runs[1]


def test_core_mirror(scenario, monkeypatch):
    monkeypatch.setenv("NT_KEYSET_COMB_BITS", "16")
    b = scenario
    core = b.core()
    try:
        plain, host = core.ingest(*N.pack(b.wires), threads=3, device="all")
        got, host_r, rec = core.ingest(*N.pack(b.wires), threads=3, device="all", receipts=True)
        with pytest.raises(ValueError):
            core.ingest(*N.pack(b.wires), threads=3, receipts=True)
    finally:
        core.close()
    assert list(got) == list(plain) == b.expect                              # the host decoder's code where it decided
    assert host_r == host == len(b.irregular)
    rows = _rows(rec)
    # a Core numbers its authorities in its committee map's order (ascending key bytes): the same
    # committee handed to nt_committee in that order gives the same rows, and the model's rows with
    # its indices renumbered
    keys = b.s.keys
    order = sorted(range(len(keys)), key=lambda k: keys[k])
    assert order != list(range(len(keys)))                                   # the renumbering is not the identity
    be = ntcrypto.Backend(device=0)
    try:
        ks = be.keyset(np.frombuffer(b"".join(keys[k] for k in order), np.uint8))
        cm = ntcrypto.Committee(ks, [b.stakes[k] for k in order], [list(range(b.nworkers[k])) for k in order],
                                b.com.quorum())
        ccodes, crec = cm.ingest_messages(b.wires, receipts=True, **b.cur_args())
        crow = _rows(crec)
        cm.close()
        ks.close()
    finally:
        be.close()
    assert list(ccodes) == b.raw_expect()

    def renumbered(r):
        f = list(S.RECEIPT_STRUCT.unpack(r))
        f[3], f[4] = order.index(f[3]), order.index(f[4])
        return S.RECEIPT_STRUCT.pack(*f)

    for i in range(len(b.wires)):
        if i in b.irregular:
            assert rows[i] == crow[i] == S.HOST_RECEIPT and got[i] == b.expect[i] != HOST, i
        else:
            assert rows[i] == crow[i] == renumbered(b.receipt(i)), (i, S.fields(rows[i]), S.fields(crow[i]))


def test_other_calls_unchanged_after_receipts(scenario, monkeypatch):
    """cm.ingest and cm.ingest_messages return after a receipts call what they returned before it"""
    monkeypatch.setenv("NT_KEYSET_COMB_BITS", "16")
    b = scenario
    be = ntcrypto.Backend(device=0)
    try:
        ks, cm = b.committee(be)
        old0 = cm.ingest(b.wires, b.gc_round).copy()
        new0 = cm.ingest_messages(b.wires, **b.cur_args()).copy()
        assert list(new0) == b.raw_expect()
        codes, _ = cm.ingest_messages(b.wires, receipts=True, **b.cur_args())
        old1 = cm.ingest(b.wires, b.gc_round)
        new1 = cm.ingest_messages(b.wires, **b.cur_args())
        assert isinstance(new1, np.ndarray)                                  # not a tuple: the default is unchanged
        assert list(old1) == list(old0) and list(new1) == list(new0) == list(codes)
        cm.close()
        ks.close()
    finally:
        be.close()
