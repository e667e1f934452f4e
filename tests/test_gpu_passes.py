"""GPU: the passes after the first of the grid-stride kernels -- k_ed25519_verify over its workspace slots,
k_ed25519_sign over its blocks, the key-cache kernels' persistent grid -- at launch geometries smaller than one
256-CU device's, where a few thousand items take them (a CU partition's normal path, and any launch beyond a
full grid).  NT_WS_SLOTS caps the verify grid; NT_GRID_CUS=<n> sizes every launch as for a device of n CUs.

Every test makes its own context under the variable, proves from the workspace the context then allocates
that the variable was read (tests/_passes.py: context), and asserts the passes its shape makes.  Expected
outputs are the fixtures' labels or the CPU oracle's; every comparison is exact."""
import os

import numpy as np
import pytest

import _passes as P
import ntcrypto

pytestmark = pytest.mark.gpu
STRICT, COFACTORLESS = ntcrypto.NT_MODE_STRICT, ntcrypto.NT_MODE_COFACTORLESS


@pytest.fixture(scope="module")
def corpus():
    return P.corpus()


@pytest.fixture(scope="module", autouse=True)
def combs():
    """Two contexts that hold the comb of B at both widths while the module runs: the comb is shared per device
    and width and freed with its last user, so the tests' short-lived contexts do not each build their own."""
    held = []
    try:
        for bits in (24, 20):
            with P.environment(NT_BCOMB_BITS=bits):
                be = ntcrypto.Backend(device=0)
                held.append(be)
                be.sign_batch(np.zeros((1, 32), np.uint8))
        assert [b.memory_info()["comb_b_bits"] for b in held] == [24, 20]
        yield
    finally:
        for b in held:
            b.close()


@pytest.fixture(scope="module")
def per_slot(corpus, combs):
    return P.slot_bytes(corpus)


@pytest.fixture(scope="module")
def X(corpus):
    x = P.batch_x(corpus)
    assert x.n == 2880 and len(np.unique(corpus["pk"], axis=0)) == 324
    return x


@pytest.fixture(scope="module")
def Y(oracle):
    return P.batch_y(oracle)


@pytest.fixture(scope="module")
def groups(oracle):
    return P.Groups(oracle)


def test_grid_cus_is_clamped(corpus, per_slot):
    """NT_GRID_CUS below 1 is one CU, above the device's count the device's: the workspace of the default context"""
    with P.environment():
        be = ntcrypto.Backend(device=0)
        try:
            full = P.workspace_after_four(be, corpus)
        finally:
            be.close()
    assert full % (per_slot * P.VERIFY_OCC * 4) == 0 and full > per_slot * P.VERIFY_OCC * 4
    with P.context(corpus, per_slot, P.VERIFY_OCC * 4, NT_GRID_CUS=0):
        pass
    with P.context(corpus, per_slot, full // per_slot, NT_GRID_CUS=1 << 20):
        pass
    with P.context(corpus, per_slot, 3, NT_GRID_CUS=2, NT_WS_SLOTS=3):  # NT_WS_SLOTS still overrides the slots
        pass


def dev_verify_passes(corpus, per_slot, X, Y, oracle, slots, **env):
    """Test 1's body: nt_dev_ed25519_verify (two signatures per lane, 512 per block iteration) in a cold context
    of `slots` workspace slots."""
    rows = 8 * -(-X.n // 512)   # wave rows of a launch: whole blocks of 4 waves x 2 rows
    assert (P.passes(X.n, P.DEV_PER_BLOCK, slots), P.passes(Y.n, P.DEV_PER_BLOCK, slots)) == \
        {1: (6, 6), 4: (2, 2), 5: (2, 2)}[slots]
    with P.context(corpus, per_slot, slots, NT_WS_SLOTS=slots, **env) as be:
        if "NT_BCOMB_BITS" in env:
            assert be.memory_info()["comb_b_bits"] == int(env["NT_BCOMB_BITS"])
        s = be.dev_stream(0, 0)
        bx, by = P.DevBatch(be, X), P.DevBatch(be, Y)
        c = P.Counters(be)
        # three identical launches: keys met and, on later passes of the same launch, built and hit; the rest
        # built; all hit.  (The context has met the corpus's first four keys once: the proof's call.)
        steps = []
        for _ in range(3):
            got = bx.bits(STRICT, s)
            assert np.array_equal(got, X.strict), np.flatnonzero(got != X.strict)[:10]
            steps.append(c.delta())
        assert all(d["fast_rows"] + d["old_rows"] == rows for d in steps), steps
        if slots == 1:
            # one block runs the six passes in turn: a key met in one pass is claimed in a later one and its
            # entry, published by this launch, read by a still later one -- no kernel boundary in between
            assert steps[0]["builds"] > 0 and steps[0]["fast_rows"] > 0, steps
        assert steps[0]["used"] + steps[1]["used"] == 324, steps
        assert steps[2] == {"used": 0, "fast_rows": rows, "builds": 0, "old_rows": 0}, steps
        got = bx.bits(COFACTORLESS, s)
        assert np.array_equal(got, X.cofactorless), np.flatnonzero(got != X.cofactorless)[:10]
        # Y's 200 keys are new to the context: cofactorless first (cold), then strict
        cof = by.bits(COFACTORLESS, s)
        assert np.array_equal(cof, Y.cofactorless), np.flatnonzero(cof != Y.cofactorless)[:10]
        for i in np.random.default_rng(5).choice(Y.n, 64, replace=False):
            m = Y.msg[int(Y.off[i]):int(Y.off[i] + Y.ln[i])].tobytes()
            assert cof[i] == oracle.verify_cofactorless(Y.pk[i].tobytes(), Y.sig[i].tobytes(), m), int(i)
        got = by.bits(STRICT, s)
        assert np.array_equal(got, Y.strict), np.flatnonzero(got != Y.strict)[:10]
        # the caches switched off per launch: byte-equal verdict words
        c.delta()
        for mode in (STRICT, COFACTORLESS):
            on = bx.words(mode, s)
            for off in ({"NT_KTAB_KEYS": "0"}, {"NT_XCACHE_SLOTS": "0"}, {"NT_KTAB_KEYS": "0", "NT_XCACHE_SLOTS": "0"}):
                os.environ.update(off)
                try:
                    c.delta()
                    assert np.array_equal(bx.words(mode, s), on), (mode, off)
                    d = c.delta()
                    assert (d["fast_rows"] + d["old_rows"] == 0) == ("NT_KTAB_KEYS" in off), (off, d)
                finally:
                    for k in off:
                        del os.environ[k]
        # three out-of-bounds slices in the last block iteration -- a later pass at every slot count: rejected,
        # their neighbours unchanged
        ok = np.flatnonzero(X.strict & X.cofactorless & (np.arange(X.n) >= 5 * 512))
        at = (int(ok[0]), int(ok[len(ok) // 2]), int(ok[-1]))
        assert len(set(at)) == 3 and P.passes(at[0] + 1, P.DEV_PER_BLOCK, slots) >= 2
        bad = P.with_bad_slices(X, at)
        bb = P.DevBatch(be, bad)
        for mode, want in ((STRICT, bad.strict), (COFACTORLESS, bad.cofactorless)):
            got = bb.bits(mode, s)
            assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]


@pytest.mark.parametrize("slots", [1, 4, 5])
def test_dev_verify_later_passes(corpus, per_slot, X, Y, oracle, slots):
    """1 slot: six passes of one block; 4 slots: two passes, blocks 2 and 3 idle in the second; 5 slots: only
    block 0 returns.  Every pass after the first reuses the block's [k]A workspace slot and meets the x cache
    and the key-table cache as its own launch left them."""
    dev_verify_passes(corpus, per_slot, X, Y, oracle, slots)


def host_verify_passes(corpus, per_slot, X, Y, groups, slots, **env):
    """Test 2's body: the host entry points.  A verify_strict call of at most one round is one chunk at one
    signature per lane, 256 per block iteration; verify_batch_groups launches two per lane, 512."""
    g = groups.tiled(3)
    assert g.n == 1890
    with P.context(corpus, per_slot, slots, NT_WS_SLOTS=slots, **env) as be:
        if "NT_BCOMB_BITS" in env:
            assert be.memory_info()["comb_b_bits"] == int(env["NT_BCOMB_BITS"])
        want_passes = {1: (12, 12, 4), 5: (3, 3, 1)}[slots]
        assert (P.passes(X.n, P.HOST_PER_BLOCK, slots), P.passes(Y.n, P.HOST_PER_BLOCK, slots),
                P.passes(g.n, P.DEV_PER_BLOCK, slots)) == want_passes
        for b in (X, Y):
            got = be.verify_strict(*b.args())
            assert np.array_equal(got, b.strict), np.flatnonzero(got != b.strict)[:10]
        # certificates of 0 .. 67 votes; with one slot groups straddle the seams between passes
        first, cnt = g.first.astype(np.int64), g.cnt.astype(np.int64)
        assert slots != 1 or ((cnt > 0) & (first // 512 != (first + cnt - 1) // 512)).any()
        gb, sb = be.verify_batch_groups(g.pk, g.sig, g.first, g.cnt, g.msg32, with_sig_bits=True)
        assert np.array_equal(gb, g.expect), np.flatnonzero(gb != g.expect)[:10]
        assert np.array_equal(sb, g.sig_bits), np.flatnonzero(sb != g.sig_bits)[:10]


@pytest.mark.parametrize("slots", [1, 5])
def test_host_verify_later_passes(corpus, per_slot, X, Y, groups, slots):
    host_verify_passes(corpus, per_slot, X, Y, groups, slots)


def test_later_passes_narrow_comb_of_b(corpus, per_slot, X, Y, groups, oracle):
    """both bodies at one slot with the 20-bit comb of B: the kernels' b20 instantiations"""
    dev_verify_passes(corpus, per_slot, X, Y, oracle, 1, NT_BCOMB_BITS=20)
    host_verify_passes(corpus, per_slot, X, Y, groups, 1, NT_BCOMB_BITS=20)


@pytest.fixture(scope="module")
def signed(oracle):
    """4,500 seeded seeds and messages of 0 .. 700 bytes with the oracle's keys and signatures, computed once"""
    rng = np.random.default_rng(99)
    n = 4500
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ln = rng.integers(0, 701, n).astype(np.uint64)
    ln[[0, 2048, n - 1]] = (0, 700, 0)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    data = rng.integers(0, 256, int(ln.sum()) + 1, dtype=np.uint8)
    pk = [oracle.pubkey(s.tobytes()) for s in seeds]
    sig = [oracle.sign(seeds[i].tobytes(), pk[i], data[int(off[i]):int(off[i] + ln[i])].tobytes()) for i in range(n)]
    return (seeds, data, off, ln, np.frombuffer(b"".join(pk), np.uint8).reshape(n, 32),
            np.frombuffer(b"".join(sig), np.uint8).reshape(n, 64))


@pytest.mark.parametrize("bits", [24, 20])
def test_sign_later_passes(corpus, per_slot, signed, bits):
    """k_ed25519_sign for one CU: 8 blocks, 2,048 signatures a pass.  4,500 take three passes, the third with
    blocks 0 and 1 only, block 1 with 148 live lanes; the keygen-only form at 2,049 leaves one key to pass 2."""
    seeds, data, off, ln, pk, sig = signed
    n = len(seeds)
    assert P.passes(n, 256, 8) == 3 and n - 2 * P.SIGN_PER_CU - 256 == 148 and P.passes(2049, 256, 8) == 2
    with P.context(corpus, per_slot, P.VERIFY_OCC * 4, NT_GRID_CUS=1, NT_BCOMB_BITS=bits) as be:
        assert be.memory_info()["comb_b_bits"] == bits
        gpk, gsig = be.sign_batch(seeds, data, off, ln)
        assert np.array_equal(gpk, pk), np.flatnonzero((gpk != pk).any(axis=1))[:10]
        assert np.array_equal(gsig, sig), np.flatnonzero((gsig != sig).any(axis=1))[:10]
        gpk = be.sign_batch(seeds[:2049])
        assert np.array_equal(gpk, pk[:2049]), np.flatnonzero((gpk != pk[:2049]).any(axis=1))[:10]


@pytest.mark.parametrize("cus", [1, 3])
def test_key_cache_small_grid(corpus, per_slot, cus):
    """The key-cache kernel for 1 and 3 CUs at 16-bit key combs, mixed mode, unknown key indices and strict bits
    as tests/_keyset_per_lane_probe.py sets them: its persistent grid is 12 waves per CU at most, so the corpus
    tiled 183 times (65,880 signatures, n mod 64 = 24) is 86 rows a wave on one CU -- more than the 64 one
    inversion batch holds -- and 29 on three.  Run as the host call cuts it (chunks of rounds for that many
    CUs, each in input order) and as one launch (NT_PIPE_CHUNKS=1: key-grouped order); torsion_votes.npz (keys
    with a torsion component) in input order.  Expected: the labels."""
    import _torsion_votes as T
    n0, reps = len(corpus["pk"]), 183
    rows = -(-n0 * reps // 64)
    assert (n0 * reps, n0 * reps % 64) == (65880, 24) and n0 * reps >= T.SORT_MIN
    assert rows >= 16 * 3 * 4 * cus and (-(-rows // (12 * cus)) > 64) == (cus == 1)   # ks_stream_plan: 3 waves per SIMD
    uniq = np.unique(corpus["pk"], axis=0)
    with P.context(corpus, per_slot, cus * P.VERIFY_OCC * 4, NT_GRID_CUS=cus, NT_KEYSET_COMB_BITS=16) as be:
        ks = be.keyset(uniq)
        try:
            assert ks.info()[0] == 16
            for r, chunks in ((1, None), (reps, None), (reps, "1")):
                midx, want = P.mixed_keyset_case(corpus, r, len(uniq))
                if chunks:
                    os.environ["NT_PIPE_CHUNKS"] = chunks
                got = ks.verify(ntcrypto.NT_MODE_MIXED, midx, np.tile(corpus["sig"], (r, 1)), corpus["msg"],
                                np.tile(corpus["off"], r), np.tile(corpus["len"], r))
                assert np.array_equal(got, want), (r, chunks, np.flatnonzero(got != want)[:10])
        finally:
            ks.close()
        tv = T.load()
        ks = be.keyset(tv["keys"])
        try:
            n, nk = len(tv["key"]), len(tv["keys"])
            unknown, strict = (np.arange(n) % 97) == 5, (np.arange(n) % 3) == 1
            idx = np.where(unknown, nk + 3, tv["key"]).astype(np.uint32)
            midx = (idx | np.where(strict, np.uint32(ntcrypto.NT_KEY_STRICT_BIT), np.uint32(0))).astype(np.uint32)
            got = ks.verify(ntcrypto.NT_MODE_MIXED, midx, tv["sig"], tv["msg32"].reshape(-1), tv["off"], tv["len"])
            want = np.where(strict, tv["strict"], tv["batch_rule"]).astype(bool) & ~unknown
            assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        finally:
            ks.close()
