"""The signer bound to a node's own key on the device (include/ntsigner.h,
csrc/k_signer.hip): votes from (id, round, origin) to the wire bytes of
PrimaryMessage::Vote, and signatures of digests, through ntcrypto.Signer.

Every expectation comes from the model -- tests/_wire.py's Vote signed by the CPU
oracle -- and Ed25519 is deterministic, so every comparison is byte for byte."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import _ingest_scenarios as S
import _passes as P
import _wire as W
import ntcrypto
from _signer_model import edge_triples, model_vote

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = bytes(range(7, 39))
NMAX = 4097
SHAPES = [1, 63, 64, 65, 129, 193, NMAX]       # row seams, partial last rows, the dword tail, several workgroups
GUARD = 64


@pytest.fixture(scope="module")
def pair():
    one = ntcrypto.Backend(devices=[0])
    three = ntcrypto.Backend(devices=[0, 0, 0])
    yield one, three
    one.close()
    three.close()


@pytest.fixture(scope="module")
def signer(pair):
    s = pair[0].signer(SEED)
    yield s
    s.close()


@pytest.fixture(scope="module")
def corpus(oracle):
    """NMAX random triples and the model's votes and digests for SEED, computed once"""
    rng = np.random.default_rng(77)
    ids = rng.integers(0, 256, (NMAX, 32), dtype=np.uint8)
    origins = rng.integers(0, 256, (NMAX, 32), dtype=np.uint8)
    rounds = rng.integers(0, 1 << 63, NMAX, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, NMAX, dtype=np.uint64)
    want = [model_vote(oracle, SEED, ids[i].tobytes(), int(rounds[i]), origins[i].tobytes()) for i in range(NMAX)]
    wires = np.frombuffer(b"".join(w for w, _ in want), np.uint8).reshape(NMAX, 212)
    digests = np.frombuffer(b"".join(d for _, d in want), np.uint8).reshape(NMAX, 32)
    return ids, rounds, origins, wires, digests


def guarded(n):
    """an (n, 212) output inside a buffer with GUARD pattern bytes on each side"""
    buf = np.full(2 * GUARD + 212 * n, 0xA5, np.uint8)
    return buf, buf[GUARD:GUARD + 212 * n].reshape(n, 212)


def guards_intact(buf):
    return bool((buf[:GUARD] == 0xA5).all() and (buf[-GUARD:] == 0xA5).all())


def check_votes(signer, corpus, n):
    """the first n votes of the corpus into a guarded buffer, without and with digests, against the model"""
    ids, rounds, origins, wires, digests = corpus
    for with_digests in (False, True):
        buf, out = guarded(n)
        got = signer.votes(ids[:n], rounds[:n], origins[:n], with_digests=with_digests, out=out)
        if with_digests:
            got, dg = got
            assert dg.shape == (n, 32) and np.array_equal(dg, digests[:n])
        assert got.ctypes.data == out.ctypes.data and guards_intact(buf)
        bad = np.flatnonzero((out != wires[:n]).any(axis=1))
        assert len(bad) == 0, bad[:10]


@pytest.mark.parametrize("n", SHAPES)
def test_votes_shapes(signer, corpus, oracle, n):
    assert signer.public == oracle.pubkey(SEED)
    check_votes(signer, corpus, n)


def test_votes_none_and_argument_rules(pair, signer, corpus):
    ids, rounds, origins, _, _ = corpus
    out, dg = signer.votes(ids[:0], rounds[:0], origins[:0], with_digests=True)
    assert out.shape == (0, 212) and dg.shape == (0, 32)
    assert signer.sign_digests(np.zeros((0, 32), np.uint8)).shape == (0, 64)
    be = pair[0]
    u8, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    a = [ids[:2].ctypes.data_as(u8), rounds[:2].ctypes.data_as(u64), origins[:2].ctypes.data_as(u8)]
    o = np.zeros((2, 212), np.uint8)
    for hole in range(4):                                                    # a NULL array with n > 0
        args = a + [o.ctypes.data_as(u8)]
        args[hole] = None
        assert be.lib.nts_votes_sign(be.ctx, signer.h, args[0], args[1], args[2], 2, args[3], None) == -1
        assert be.lib.nts_votes_sign(be.ctx, signer.h, args[0], args[1], args[2], 0, args[3], None) == 0
    assert be.lib.nts_sign_digests(be.ctx, signer.h, None, 2, o.ctypes.data_as(u8)) == -1
    assert be.lib.nts_votes_sign(be.ctx, None, a[0], a[1], a[2], 2, o.ctypes.data_as(u8), None) == -1
    assert not o.any()
    with pytest.raises(ValueError):
        signer.votes(ids[:2], rounds[:3], origins[:2])


def test_votes_pinned_output(pair, signer, corpus):
    ids, rounds, origins, wires, _ = corpus
    out = pair[0].pinned((193, 212))
    signer.votes(ids[:193], rounds[:193], origins[:193], out=out)
    assert np.array_equal(out, wires[:193])


def test_edge_values_in_lanes_0_31_63_64(signer, oracle):
    rng = np.random.default_rng(78)
    edges = edge_triples(rng, oracle.pubkey(SEED))
    lanes = (0, 31, 63, 64)
    while len(edges) % len(lanes):
        edges.append(edges[0])
    for g in range(0, len(edges), len(lanes)):
        n = 65
        ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        origins = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        rounds = rng.integers(0, 1 << 40, n, dtype=np.uint64)
        for lane, (id_, round_, origin) in zip(lanes, edges[g:g + len(lanes)]):
            ids[lane] = np.frombuffer(id_, np.uint8)
            rounds[lane] = round_
            origins[lane] = np.frombuffer(origin, np.uint8)
        out, dg = signer.votes(ids, rounds, origins, with_digests=True)
        for i in list(lanes) + [1, 30, 32, 62]:
            wire, digest = model_vote(oracle, SEED, ids[i].tobytes(), int(rounds[i]), origins[i].tobytes())
            assert out[i].tobytes() == wire and dg[i].tobytes() == digest, (g, i)


@pytest.mark.parametrize("n", SHAPES)
def test_sign_digests_shapes(signer, corpus, oracle, n):
    digests = corpus[4]
    pk = oracle.pubkey(SEED)
    sig = signer.sign_digests(digests[:n])
    assert sig.shape == (n, 64)
    # a vote's signature is the signature of its digest: the model's wires carry it
    assert np.array_equal(sig, corpus[3][:n, 148:])
    for i in {0, n // 2, n - 1}:
        assert sig[i].tobytes() == oracle.sign(SEED, pk, digests[i].tobytes())


def test_hello_signatures(pair):
    with open(os.path.join(GOLD, "fixtures_reference.json")) as f:
        ref = json.load(f)
    hello = np.frombuffer(bytes.fromhex(ref["hello_digest"]), np.uint8)
    for k, want in zip(ref["keys"], ref["hello_signatures"]):
        s = pair[0].signer(bytes.fromhex(k["seed"]))
        try:
            assert s.public == bytes.fromhex(k["pk"])
            assert s.sign_digests(hello)[0].tobytes() == bytes.fromhex(want)
        finally:
            s.close()


@pytest.mark.parametrize("n", [193, NMAX])
def test_sharding_three_entries(pair, corpus, n):
    ids, rounds, origins, wires, digests = corpus
    s3 = pair[1].signer(SEED)
    try:
        out, dg = s3.votes(ids[:n], rounds[:n], origins[:n], with_digests=True)
        assert np.array_equal(out, wires[:n]) and np.array_equal(dg, digests[:n])
        assert np.array_equal(s3.sign_digests(digests[:n]), wires[:n, 148:])
    finally:
        s3.close()


def test_dev_votes_on_a_library_stream(pair, signer, corpus):
    import torch
    ids, rounds, origins, wires, digests = corpus
    be = pair[0]
    dev = torch.device("cuda", 0)
    n = 193
    d_id = torch.from_numpy(ids[:n].copy()).to(dev)
    d_round = torch.from_numpy(rounds[:n].view(np.int64).copy()).to(dev)
    d_origin = torch.from_numpy(origins[:n].copy()).to(dev)
    d_vote = torch.full((n * 212 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_dg = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    stream = be.dev_stream(0, 0)
    signer.dev_votes(0, stream, d_id.data_ptr(), d_round.data_ptr(), d_origin.data_ptr(), n, d_vote.data_ptr(),
                     d_dg.data_ptr())
    signer.dev_votes(0, stream, d_id.data_ptr(), d_round.data_ptr(), d_origin.data_ptr(), 0, None, None)
    host = signer.votes(ids[:n], rounds[:n], origins[:n])      # the host call drains the same stream
    torch.cuda.synchronize(dev)
    got = d_vote.cpu().numpy()
    assert np.array_equal(got[:n * 212].reshape(n, 212), host) and np.array_equal(host, wires[:n])
    assert (got[n * 212:] == 0xA5).all()
    assert np.array_equal(d_dg.cpu().numpy(), digests[:n])
    with pytest.raises(ntcrypto.NtError):                                    # a misaligned output array
        signer.dev_votes(0, stream, d_id.data_ptr(), d_round.data_ptr(), d_origin.data_ptr(), n, d_vote.data_ptr() + 4,
                         None)


def test_round_trip_through_ingestion(oracle, monkeypatch):
    """130 votes of committee member 2 for the current header go back through the device
    ingestion: every code Ok, every receipt's digest the signer's, author 2; a stranger's
    votes are left to the host decoder, which answers UnknownAuthority."""
    monkeypatch.setenv("NT_KEYSET_COMB_BITS", "16")
    from ntcrypto import narwhal as N
    rng = random.Random(5)
    s = S.Signer(oracle, 5, 3)
    cur = s.header(rng, s.keys[0], 8)
    n = 130
    ids = np.tile(np.frombuffer(cur.id, np.uint8), (n, 1))
    rounds = np.full(n, cur.round, np.uint64)
    origins = np.tile(np.frombuffer(cur.author, np.uint8), (n, 1))
    stakes, nworkers = [1] * 5, [2] * 5
    com = W.Committee(s.keys, stakes, nworkers)
    be = ntcrypto.Backend(device=0)
    try:
        ks = be.keyset(np.frombuffer(b"".join(s.keys), np.uint8))
        cm = ntcrypto.Committee(ks, stakes, [[0, 1]] * 5, com.quorum())
        cur_args = dict(gc_round=0, cur_id=cur.id, cur_round=cur.round, cur_author=cur.author)
        member = be.signer(s.sk[s.keys[2]])
        assert member.public == s.keys[2]
        votes, dg = member.votes(ids, rounds, origins, with_digests=True)
        assert votes[0].tobytes() == W.message(s.vote(s.keys[2], cur))
        codes, rec = cm.ingest_messages([v.tobytes() for v in votes], receipts=True, **cur_args)
        assert list(codes) == [W.OK] * n
        assert np.array_equal(rec["digest"], dg) and (rec["author"] == 2).all() and (rec["origin"] == 0).all()
        assert (rec["kind"] == 1).all() and all(bytes(r) == cur.id for r in rec["id"])
        member.close()
        stranger = be.signer(s.sk[s.stranger])
        strange = [v.tobytes() for v in stranger.votes(ids, rounds, origins)]
        stranger.close()
        assert strange[0] == W.message(s.vote(s.stranger, cur))
        raw = cm.ingest_messages(strange, **cur_args)
        assert list(raw) == [S.HOST] * n                                     # the device leaves an unknown key to the host
        cm.close()
        ks.close()
    finally:
        be.close()
    core = N.Core(np.frombuffer(b"".join(s.keys), np.uint8), stakes, nworkers, 0, W.message(cur), True)
    try:
        final, host = core.ingest(*N.pack(strange), threads=2, device="all")
    finally:
        core.close()
    assert list(final) == [W.UNKNOWN_AUTHORITY] * n and host == n


def test_small_call_path(corpus):
    ids, rounds, origins, wires, digests = corpus
    be = ntcrypto.Backend(device=0)
    try:
        s = be.signer(SEED)
        be.set_small_call_path(ntcrypto.NT_SMALL_ALWAYS, 4)
        for n in (1, 67):
            h0, g0 = be.call_counts()
            out, dg = s.votes(ids[:n], rounds[:n], origins[:n], with_digests=True)
            sig = s.sign_digests(digests[:n])
            assert be.call_counts() == (h0 + 2, g0)
            assert np.array_equal(out, wires[:n]) and np.array_equal(dg, digests[:n])
            assert np.array_equal(sig, wires[:n, 148:])
        be.set_small_call_path(ntcrypto.NT_SMALL_OFF, 4)
        h0, g0 = be.call_counts()
        assert np.array_equal(s.votes(ids[:67], rounds[:67], origins[:67]), wires[:67])
        assert np.array_equal(s.sign_digests(digests[:1]), wires[:1, 148:])
        assert be.call_counts() == (h0, g0 + 2)
        s.close()
    finally:
        be.close()


def test_signer_lifetime(pair, corpus, oracle):
    ids, rounds, origins, wires, _ = corpus
    be = pair[0]
    other = bytes(range(100, 132))
    a = be.signer(SEED)
    assert np.array_equal(a.votes(ids[:5], rounds[:5], origins[:5]), wires[:5])
    a.close()
    a.close()                                                                # closing twice is harmless
    b = be.signer(other)
    try:
        assert b.public == oracle.pubkey(other) != oracle.pubkey(SEED)
        out = b.votes(ids[:5], rounds[:5], origins[:5])
        for i in range(5):
            wire, _ = model_vote(oracle, other, ids[i].tobytes(), int(rounds[i]), origins[i].tobytes())
            assert out[i].tobytes() == wire
            assert out[i, 104:148].tobytes() == W.b64(b.public)              # the author text is the second key's
    finally:
        b.close()


def test_narrow_comb_of_b(corpus, monkeypatch):
    """the kernels' other instantiation: the 20-bit comb of B"""
    monkeypatch.setenv("NT_BCOMB_BITS", "20")
    ids, rounds, origins, wires, digests = corpus
    be = ntcrypto.Backend(device=0)
    try:
        assert be.memory_info()["comb_b_bits"] == 0
        s = be.signer(SEED)
        out, dg = s.votes(ids[:129], rounds[:129], origins[:129], with_digests=True)
        assert be.memory_info()["comb_b_bits"] == 20
        assert np.array_equal(out, wires[:129]) and np.array_equal(dg, digests[:129])
        assert np.array_equal(s.sign_digests(digests[:129]), wires[:129, 148:])
        s.close()
    finally:
        be.close()


def test_core_votes_for(oracle, monkeypatch):
    """a 400-message drain ingested with receipts; the node votes for every accepted header"""
    monkeypatch.setenv("NT_KEYSET_COMB_BITS", "16")
    monkeypatch.setenv("NT_INGEST_CHUNK", "64")
    from ntcrypto import narwhal as N
    b = S.build_shapes(oracle)
    assert len(b.wires) == 400
    seed = b.s.sk[b.s.keys[1]]
    core = b.core()
    try:
        with pytest.raises(ntcrypto.NtError):                                # no signer yet
            core.votes_for(np.zeros(1, ntcrypto.RECEIPT_DTYPE), [0])
        assert core.set_signer(seed) == b.s.keys[1]
        codes, _, rec = core.ingest(*N.pack(b.wires), threads=3, device="all", receipts=True)
        assert list(codes) == b.expect
        sel = [i for i in range(400) if codes[i] == W.OK and rec["kind"][i] == 0]
        assert sel == [i for i, o in enumerate(b.objs)
                       if isinstance(o, W.Header) and b.expect[i] == W.OK and i not in b.irregular]
        assert len(sel) > 64 and len({b.objs[i].author for i in sel}) > 1
        votes = core.votes_for(rec, sel)
        assert votes.shape == (len(sel), 212)
        for k, i in enumerate(sel):
            h = b.objs[i]
            wire, _ = model_vote(oracle, seed, h.id, h.round, h.author)
            assert votes[k].tobytes() == wire, (k, i)
        assert core.votes_for(rec, []).shape == (0, 212)
        other = next(i for i in range(400) if rec["kind"][i] == 1)
        with pytest.raises(ValueError):                                      # a vote's receipt
            core.votes_for(rec, [sel[0], other])
    finally:
        core.close()


# ---- later passes of the grid-stride loops: a context sized for one CU (NT_GRID_CUS=1) ----
@pytest.fixture(scope="module")
def one_cu():
    """A signer in a context made under NT_GRID_CUS=1: k_signer_votes runs at most 32 rows of 64 votes and
    k_signer_digests 8 blocks of 256 digests -- 2,048 items -- per pass.  The context's workspace proves that
    the variable was read (tests/_passes.py)."""
    c = P.corpus()
    per_slot = P.slot_bytes(c)
    with P.environment(NT_GRID_CUS=1):
        be = ntcrypto.Backend(device=0)
    try:
        assert P.workspace_after_four(be, c) == P.VERIFY_OCC * 4 * per_slot
        s = be.signer(SEED)
        try:
            yield s
        finally:
            s.close()
    finally:
        be.close()


@pytest.mark.parametrize("n", [2049, 2175, NMAX])
def test_votes_later_passes(one_cu, corpus, n):
    """2,049: pass 2 is a row of one vote (13 16-byte stores and 1 dword); 2,175: a full row and a row of 63;
    4,097: three passes.  Every later pass reuses the wave's LDS row."""
    assert P.passes(n, 64, 32) == {2049: 2, 2175: 2, NMAX: 3}[n]
    assert (n - P.SIGN_PER_CU) % 64 == {2049: 1, 2175: 63, NMAX: 1}[n] and (212 // 16, 212 % 16 // 4) == (13, 1)
    check_votes(one_cu, corpus, n)


@pytest.mark.parametrize("n", [2049, NMAX])
def test_sign_digests_later_passes(one_cu, corpus, n):
    assert P.passes(n, 256, 8) == {2049: 2, NMAX: 3}[n]
    sig = one_cu.sign_digests(corpus[4][:n])
    bad = np.flatnonzero((sig != corpus[3][:n, 148:]).any(axis=1))  # the model's wires carry the digests' signatures
    assert sig.shape == (n, 64) and len(bad) == 0, bad[:10]
