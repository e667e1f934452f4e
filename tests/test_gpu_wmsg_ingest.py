"""nt_worker_messages_ingest: the worker's drain decided on the device from wire
bytes (k_wingest.hip, csrc/wmsg_plan.hpp, wingest_gpu.cpp) -- a code and a
64-byte receipt per message, an accepted batch's with the Processor's digest --
through Backend.ingest_worker_messages and the C++ mirror's
worker::ingest_device.

Every expectation comes from tests/_wmsg.py (an independent serial reading of
the format, hashlib for the digests) or from the reference's own fixtures in
tests/golden/, never from the code under test.
"""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

import _wmsg as M
import ntcrypto
from _oracle import expand
from ntcrypto import narwhal as N

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def items():
    """the scenario list plus a request at the digest cap and one above it (33.5 MB each)"""
    key = bytes(range(7, 39))
    extra = [("request_at_cap", M.request([bytes(32)] * M.MAX_DIGESTS, key)),
             ("request_over_cap", M.request([bytes(32)] * (M.MAX_DIGESTS + 1), key))]
    return M.scenario() + extra


@pytest.fixture(scope="module")
def wires(items):
    return [m for _, m in items]


@pytest.fixture(scope="module")
def want(wires):
    """the model's receipts, computed once"""
    return [M.receipt(m) for m in wires]


@pytest.fixture(scope="module")
def backend():
    be = ntcrypto.Backend(device=0)
    yield be
    be.close()


def _rows(rec):
    assert rec.dtype == ntcrypto.WORKER_RECEIPT_DTYPE and rec.dtype.itemsize == 64
    raw = rec.tobytes()
    return [raw[64 * i:64 * (i + 1)] for i in range(len(rec))]


def _check(items, want, codes, rec):
    got = _rows(rec)
    assert len(got) == len(want) == len(codes)
    bad = [(items[i][0], M.fields(got[i]), M.fields(want[i])) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, bad[:5]
    assert bytes(codes) == bytes(w[0] for w in want)
    for r in got:                                    # kind != 0xff exactly when the code is OK; else zero after it
        assert (r[1] != 0xFF) == (r[0] == M.OK) and (r[0] == M.OK or r[2:] == bytes(62))


def test_reference_fixtures(backend):
    """processor_tests.rs' 228-byte batch and the golden 508,052-byte batch at three byte phases"""
    with open(os.path.join(GOLD, "sha512_vectors.json")) as f:
        ref = json.load(f)["reference_fixtures"]
    small = bytes.fromhex(ref["processor_batch_228B"]["hex"])
    assert len(small) == 228 and ref["processor_batch_228B"]["digest32"].startswith("24d00f74")
    codes, rec = backend.ingest_worker_messages([small])
    # the fixture is vec![transaction(), transaction()] with transaction() = vec![0; 100]
    # (worker/src/tests/common.rs:86-95): two transactions, and its bytes say so (u64 2 at offset 4)
    assert struct.unpack_from("<IQQ", small, 0) == (0, 2, 100)
    assert (codes[0], rec["kind"][0], rec["n"][0], rec["used"][0]) == (0, 0, 2, 228)
    assert bytes(rec["digest"][0]).hex() == ref["processor_batch_228B"]["digest32"]
    assert (rec["flags"][0], rec["tx_len"][0], rec["tx_bytes"][0]) == (1, 100, 200)
    rb = ref["real_batch_977x512"]
    txs = [expand((rb["tx_label"] % i).encode(), rb["tx_len"]) for i in range(rb["ntx"])]
    real = M.batch(txs)
    assert len(real) == rb["len"] == 508052
    off = np.array([0, 508052 + 1, 2 * 508052 + 3], np.uint64)               # phases 0, 1 and 3 mod 4
    assert [int(o) % 4 for o in off] == [0, 1, 3]
    data = np.full(3 * 508052 + 16, 0xEE, np.uint8)
    for o in off:
        data[int(o):int(o) + 508052] = np.frombuffer(real, np.uint8)
    codes, rec = backend.ingest_worker_messages(None, data=data, off=off, ln=np.full(3, 508052, np.uint64))
    for i in range(3):
        assert (codes[i], rec["kind"][i], rec["n"][i], rec["flags"][i], rec["tx_len"][i]) == (0, 0, 977, 1, 512), i
        assert (rec["used"][i], rec["tx_bytes"][i], rec["off_key"][i]) == (508052, 977 * 512, 0), i
        assert bytes(rec["digest"][i]).hex() == rb["digest32"], i


def test_scenario_against_the_model(backend, items, wires, want):
    n = len(wires)
    rec = np.frombuffer(bytearray(b"\xab" * (64 * n)), ntcrypto.WORKER_RECEIPT_DTYPE)
    codes, out = backend.ingest_worker_messages(wires, receipts=rec)
    assert out.ctypes.data == rec.ctypes.data
    _check(items, want, codes, rec)
    assert {w[0] for w in want} == {M.OK, M.SERIALIZATION, M.HOST}
    names = [nm for nm, _ in items]
    # the two rules: the digest covers the trailing bytes; an empty batch and an empty transaction are valid
    t = names.index("batch_trailing_7")
    f = M.fields(_rows(rec)[t])
    assert f["code"] == 0 and f["used"] == len(wires[t]) - 7
    import hashlib
    assert f["digest"] == hashlib.sha512(wires[t]).digest()[:32] != hashlib.sha512(wires[t][:-7]).digest()[:32]
    e = M.fields(_rows(rec)[names.index("uniform_0_x_0")])
    assert (e["code"], e["kind"], e["n"], e["used"]) == (0, 0, 0, 12)
    assert e["digest"] == hashlib.sha512(struct.pack("<IQ", 0, 0)).digest()[:32]
    z = M.fields(_rows(rec)[names.index("uniform_65_x_0")])
    assert (z["code"], z["n"], z["flags"], z["tx_len"], z["tx_bytes"]) == (0, 65, 1, 0, 0)
    assert M.fields(_rows(rec)[names.index("request_over_cap")])["code"] == M.HOST
    assert M.fields(_rows(rec)[names.index("request_at_cap")])["digest"] == bytes(range(7, 39))
    with pytest.raises(ValueError):
        backend.ingest_worker_messages(wires, receipts=np.zeros(n + 1, ntcrypto.WORKER_RECEIPT_DTYPE))


def test_chunk_and_shard_seams(backend, items, wires, want, monkeypatch):
    """chunks of three messages (both parities' buffers reused dozens of times), two device entries on
    one ordinal (a shard seam in the middle), pinned and pageable input: the same bytes every time"""
    ref_codes, ref_rec = backend.ingest_worker_messages(wires)
    _check(items, want, ref_codes, ref_rec)
    ref = (ref_codes.tobytes(), ref_rec.tobytes())
    data, off, ln = N.pack(wires)
    pinned = backend.pinned(len(data) + 3)
    pinned[3:] = data                                # every message moves three bytes
    monkeypatch.setenv("NT_WINGEST_CHUNK", "3")
    c, r = backend.ingest_worker_messages(wires)
    assert (c.tobytes(), r.tobytes()) == ref
    c, r = backend.ingest_worker_messages(None, data=pinned, off=off + np.uint64(3), ln=ln)
    assert (c.tobytes(), r.tobytes()) == ref
    monkeypatch.setenv("NT_WINGEST_CHUNK_BYTES", "4096")     # ... and cut by bytes
    monkeypatch.setenv("NT_WINGEST_CHUNK", "50")
    c, r = backend.ingest_worker_messages(wires)
    assert (c.tobytes(), r.tobytes()) == ref
    monkeypatch.delenv("NT_WINGEST_CHUNK_BYTES")
    monkeypatch.delenv("NT_WINGEST_CHUNK")
    c, r = backend.ingest_worker_messages(None, data=pinned, off=off + np.uint64(3), ln=ln)
    assert (c.tobytes(), r.tobytes()) == ref
    two = ntcrypto.Backend(devices=[0, 0])
    try:
        for chunk in (None, "3"):
            if chunk:
                monkeypatch.setenv("NT_WINGEST_CHUNK", chunk)
            c, r = two.ingest_worker_messages(wires)
            assert (c.tobytes(), r.tobytes()) == ref, chunk
        for i in (0, len(wires) // 2, len(wires) - 3):                       # calls of one message
            c1, r1 = two.ingest_worker_messages([wires[i]])
            assert _rows(r1) == [want[i]] and c1[0] == want[i][0], i
    finally:
        two.close()


def test_call_variants(backend, wires, want):
    codes = backend.ingest_worker_messages(wires, receipts=False)             # out_receipt = NULL
    assert isinstance(codes, np.ndarray) and bytes(codes) == bytes(w[0] for w in want)
    u8, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    data, off, ln = N.pack(wires[:4])
    out = np.full(4, 0xAB, np.uint8)
    rec = np.frombuffer(bytearray(b"\xab" * 256), ntcrypto.WORKER_RECEIPT_DTYPE)
    args = (data.ctypes.data_as(u8), off.ctypes.data_as(u64), ln.ctypes.data_as(u64))
    assert backend.lib.nt_worker_messages_ingest(backend.ctx, *args, 0, out.ctypes.data_as(u8),
                                                 rec.ctypes.data_as(ctypes.c_void_p)) == 0
    assert out.tobytes() == b"\xab" * 4 and rec.tobytes() == b"\xab" * 256    # n = 0 writes nothing
    assert backend.lib.nt_worker_messages_ingest(backend.ctx, None, None, None, 0, None, None) == 0
    assert backend.lib.nt_worker_messages_ingest(backend.ctx, *args, 4, None, None) == -1      # NT_EINVAL
    c, r = backend.ingest_worker_messages([])
    assert len(c) == 0 and len(r) == 0
    # packed input is bounded before the call, without a sum that wraps
    for bad_off, bad_ln in ((len(data) - 3, 4), (2 ** 64 - 2, 4), (1, 2 ** 64 - 1), (len(data) + 1, 0)):
        with pytest.raises(ValueError):
            backend.ingest_worker_messages(None, data=data, off=np.array([0, bad_off], np.uint64),
                                           ln=np.array([4, bad_ln], np.uint64))
    c, r = backend.ingest_worker_messages(None, data=data, off=np.array([len(data) - 4], np.uint64),
                                          ln=np.array([4], np.uint64))
    assert len(c) == 1


def test_small_call_path(items, wires, want):
    be = ntcrypto.Backend(device=0)
    try:
        gpu = be.ingest_worker_messages(wires)
        h0, g0 = be.call_counts()
        assert g0 >= 1 and h0 == 0
        be.set_small_call_path(ntcrypto.NT_SMALL_ALWAYS, 4)
        h1, g1 = be.call_counts()
        codes, rec = be.ingest_worker_messages(wires)
        assert be.call_counts() == (h1 + 1, g1)                              # the call went to the host lane
        _check(items, want, codes, rec)
        assert (codes.tobytes(), rec.tobytes()) == (gpu[0].tobytes(), gpu[1].tobytes())
        only = be.ingest_worker_messages(wires, receipts=False)
        assert only.tobytes() == codes.tobytes() and be.call_counts() == (h1 + 2, g1)
    finally:
        be.close()


def test_no_tables(wires):
    """a context that has only made this call holds no comb of B, no key combs, no verify workspace"""
    be = ntcrypto.Backend(device=0)
    try:
        be.ingest_worker_messages(wires)
        be.ingest_worker_messages(wires[:5], receipts=False)
        info = be.memory_info(0)
        assert (info["comb_b_bits"], info["comb_b_bytes"], info["key_comb_bytes"]) == (0, 0, 0), info
        assert (info["workspace_bytes"], info["stash_bytes"], info["held"]) == (0, 0, 0), info
    finally:
        be.close()


def test_mirrors(backend, items, wires, want):
    """worker::ingest_device and Backend.ingest_worker_messages give the same rows; an accepted
    batch's output is Processor::process's; what the device leaves, the host decoder decides"""
    codes, rec = backend.ingest_worker_messages(wires)
    got = N.worker_ingest(11, wires)
    assert got["receipts"].tobytes() == rec.tobytes()
    assert got["host_decided"] == sum(1 for w in want if w[0] == M.HOST) > 0
    names = [nm for nm, _ in items]
    batcher = N.DigestBatcher()
    try:
        checked = 0
        for i, w in enumerate(want):
            f = M.fields(w)
            if f["code"] == M.HOST:
                assert got["code"][i] in (M.OK, M.SERIALIZATION), names[i]
                continue
            assert (got["code"][i], got["kind"][i]) == (f["code"], f["kind"]), names[i]
            if f["code"] == M.OK and f["kind"] == M.BATCH:
                assert got["message"][i].tobytes() == struct.pack("<I", 1) + f["digest"] + struct.pack("<I", 11)
                if len(wires[i]) < 2000 and checked < 12:
                    assert batcher.process(11, False, wires[i]) == (f["digest"], got["message"][i].tobytes()), names[i]
                    checked += 1
            elif f["code"] == M.OK:
                assert got["requestor"][i].tobytes() == f["digest"] and got["nd"][i] == f["n"], names[i]
        assert checked == 12
    finally:
        batcher.close()
    # the host decoder's verdicts on what the device left: 44 unpadded characters are a 33-byte key
    # (accepted, first 32 bytes); a count over the cap that the bytes hold is accepted; the rest are
    # bincode errors
    i = names.index("request_no_pad")
    assert (got["code"][i], got["kind"][i]) == (M.OK, M.REQUEST)
    i = names.index("request_over_cap")
    assert (got["code"][i], got["kind"][i], got["nd"][i]) == (M.OK, M.REQUEST, M.MAX_DIGESTS + 1)
    assert got["requestor"][i].tobytes() == bytes(range(7, 39))
    for nm in ("request_key_43", "request_key_45", "request_key_0", "request_trailing_bits_1", "request_alphabet_2d"):
        assert got["code"][names.index(nm)] == M.SERIALIZATION, nm
