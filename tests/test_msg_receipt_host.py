"""The receipt assembly of the device ingestion (narwhal-tusk_amd/csrc/
msg_receipt.hpp over msg_plan.hpp's walk) on the host.  CPU only:
tests/cpp/msgreceipt/ builds msg_receipt_check, a stand-alone program under the
address and undefined-behaviour sanitizers that assembles the records the way
k_msg_receipt does; this test feeds it the scenario's and the shapes' messages
with the code, the committee indices and the two SHA-512 outputs the device
would hold (all from the Python model: tests/_wire.py objects, hashlib, the
oracle-driven model_sanitize) and compares every record with the model's."""
import os
import struct
import subprocess

import pytest

import _ingest_scenarios as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MDIR = os.path.join(ROOT, "tests", "cpp", "msgreceipt")
CHECK = os.path.join(ROOT, "tests", "cpp", "build", "msg_receipt_check")
ALL = 0xF


@pytest.fixture(scope="module")
def checker():
    subprocess.run(["make", "-s", "-C", MDIR], check=True)
    return CHECK


def _run(checker, tmp_path, batch, name):
    """the checker's records for the batch, one 128-byte string per message"""
    n = len(batch.wires)
    blob = [struct.pack("<IIQ", n, ALL, batch.gc_round)]
    for i, w in enumerate(batch.wires):
        author, origin = batch.indices(i)
        blob.append(struct.pack("<IIII", len(w), batch.raw_expect()[i], author, origin) + b"".join(batch.digest_slots(i))
                    + w)
    src, dst = tmp_path / (name + ".in"), tmp_path / (name + ".out")
    src.write_bytes(b"".join(blob))
    r = subprocess.run([checker, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "%d records" % n in r.stdout
    out = dst.read_bytes()
    assert len(out) == 128 * n
    return [out[128 * i:128 * (i + 1)] for i in range(n)]


def _compare(batch, got):
    want = batch.receipts()
    diffs = S.receipt_diffs(got, want)
    assert not diffs, diffs[:10]
    for i, r in enumerate(got):
        if i in batch.irregular:
            assert r == S.HOST_RECEIPT, i
        S.check_in_place(batch, i, r)


def test_scenario_records(checker, tmp_path, oracle):
    b = S.build_scenario(oracle)
    got = _run(checker, tmp_path, b, "scenario")
    _compare(b, got)
    f = S.fields(got[b.named["bad_id"]])
    assert f["digest"] != f["id"] and b.expect[b.named["bad_id"]] == S.W.INVALID_HEADER_ID
    g = S.fields(got[b.named["genesis"]])
    assert g["flags"] == 0 and g["code"] == S.W.TOO_OLD                      # GC round 5 filters it first
    kinds = {S.fields(r)["kind"] for r in got}
    assert kinds == {0, 1, 2, 3, S.HOST}
    # every field of a decided message is defined whatever its code
    codes = {S.fields(r)["code"] for i, r in enumerate(got) if i not in b.irregular}
    assert codes == set(range(11)) - {S.W.SERIALIZATION_ERROR}
    # under GC round 0 the genesis certificate is accepted, and flagged
    b0 = b.regauged(0)
    got0 = _run(checker, tmp_path, b0, "scenario_gc0")
    _compare(b0, got0)
    g0 = S.fields(got0[b0.named["genesis"]])
    assert (g0["flags"], g0["code"], g0["round"], g0["id"]) == (S.GENESIS, S.W.OK, 0, bytes(32).hex())
    assert sum(S.fields(r)["flags"] for r in got0) == 1                      # nothing else is flagged


def test_shapes_records(checker, tmp_path, oracle):
    b = S.build_shapes(oracle)
    got = _run(checker, tmp_path, b, "shapes")
    _compare(b, got)
    f = [S.fields(r) for r in got]
    hdr = [x for x in f if x["kind"] == 0]
    assert any(x["np"] == 0 and x["nq"] == 0 and x["off_payload"] == 0 for x in hdr)
    assert any(x["nq"] == 70 for x in hdr) and any(x["nq"] == 70 for x in f if x["kind"] == 2)
    assert any(x["kind"] == 3 and x["nq"] == 0 for x in f) and any(x["kind"] == 3 and x["nq"] == 2 for x in f)


def test_checker_refuses_a_wrong_digest_slot(checker, tmp_path, oracle):
    """the comparison is not vacuous: with a certificate's two digest slots swapped
    the checker's record differs from the model's in `digest` alone"""
    b = S.build_scenario(oracle)
    real = b.digest_slots
    b.digest_slots = lambda i: real(i)[::-1]
    got = _run(checker, tmp_path, b, "swapped")
    diffs = S.receipt_diffs(got, b.receipts())
    assert diffs and {d[1] for d in diffs} == {"digest"}
