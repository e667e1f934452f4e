"""Every path of the certificate-group host entry points
(nt_ed25519_verify_batch_groups / ..._keyset): three input layouts x four key
forms x three chunkings, all on the same few thousand signatures, against the
oracle's verdicts computed once on the dense layout.

Layouts: dense in pageable memory (HIP stages each copy), dense in
nt_host_alloc memory (every copy a DMA, chunk c + 1 queued ahead), and
scattered (groups stored in reverse order with three unused all-zero slots
between neighbours, so the runtime gathers them on a helper thread).
Key forms: raw keys without a registry (uncached kernel), key-set indices,
raw keys with a registry that holds all 50 keys (lookups on the look-ahead
thread), and raw keys with a registry that holds 30 of the 50 (the misses
verify afterwards through the uncached kernel and their groups' verdicts are
recomputed).  Chunkings: one chunk, and up to 16 chunks of rounds 64 and 640.
The registry forms also count: hits + misses of a call are its signatures."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G, NKEYS, NREG, GAP = 203, 50, 30, 3
LAYOUTS = ("pageable", "pinned", "scattered")
FORMS = ("raw", "keyset", "reg_all", "reg_part")
CHUNKINGS = {"one": ("1", None), "r64": ("16", "64"), "r640": ("16", "640")}


def _registry(devices, pks, cap):
    import ntcrypto
    b = ntcrypto.Backend(devices=devices)
    b.set_key_cache(cap)
    b.key_cache_add(pks)
    info = b.key_cache_info()
    assert info["keys"] == len(pks) and info["error"] == 0 and info["pending"] == 0, info
    return b


@pytest.fixture(scope="module")
def world(oracle):
    """Inputs in the three layouts, the oracle's verdicts mapped to each, and one context per key form."""
    import ntcrypto
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("NT_KEYSET_COMB_BITS", "16")
        plain = ntcrypto.Backend(device=0)
        rng = np.random.default_rng(99)
        kseeds = rng.integers(0, 256, (NKEYS, 32), dtype=np.uint8)
        cnt = rng.integers(0, 30, G).astype(np.uint32)
        cnt[[3, 77]] = 0
        first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint64)
        m = int(cnt.sum())
        kidx = rng.integers(0, NKEYS, m).astype(np.uint32)
        msg32 = rng.integers(0, 256, (G, 32), dtype=np.uint8)
        gmsg = np.repeat(msg32, cnt.astype(np.int64), axis=0).ravel()
        pk, sig = plain.sign_batch(kseeds[kidx], gmsg, np.arange(m, dtype=np.uint64) * 32, np.full(m, 32, np.uint64))
        sig = sig.copy()
        sig[rng.choice(m, 25, replace=False), 50] ^= 1
        kpk = plain.sign_batch(kseeds)
        want_g, want_s = (x.astype(bool) for x in oracle.verify_batch_groups(pk, sig, first, cnt, msg32, nthreads=8))
        assert want_s.sum() == m - 25 and want_g[[3, 77]].all() and 0 < want_g.sum() < G

        # scattered: group G-1 first, GAP zero slots between neighbours; dense slot e -> scattered slot perm[e]
        first_s = np.zeros(G, np.uint64)
        pos = 0
        for g in range(G - 1, -1, -1):
            first_s[g] = pos
            pos += int(cnt[g]) + GAP
        n_s = int((first_s + cnt).max())
        perm = (np.repeat(first_s, cnt.astype(np.int64)) + np.arange(m, dtype=np.uint64)
                - np.repeat(first, cnt.astype(np.int64))).astype(np.int64)
        assert len(np.unique(perm)) == m and not np.all(np.diff(first_s.astype(np.int64)) > 0)

        def scatter(a):
            out = np.zeros((n_s,) + a.shape[1:], a.dtype)
            out[perm] = a
            return out

        def pin(a):
            p = plain.pinned(a.shape, a.dtype)
            p[...] = a
            return p

        want_s_scat = scatter(want_s)
        assert want_s_scat.sum() == want_s.sum()
        lay = {
            "pageable": dict(pk=pk, kidx=kidx, sig=sig, msg32=msg32, first=first, want_s=want_s),
            "pinned": dict(pk=pin(pk), kidx=pin(kidx), sig=pin(sig), msg32=pin(msg32), first=first, want_s=want_s),
            "scattered": dict(pk=scatter(pk), kidx=scatter(kidx), sig=scatter(sig), msg32=msg32, first=first_s,
                              want_s=want_s_scat),
        }
        w = dict(lay=lay, cnt=cnt, want_g=want_g, m=m, registered=int((kidx < NREG).sum()),
                 plain=plain, ks=plain.keyset(kpk),
                 reg_all=_registry([0], kpk, NKEYS), reg_part=_registry([0], kpk[:NREG], NREG),
                 reg_part2=_registry([0, 0], kpk[:NREG], NREG))
        yield w
        w["ks"].close()
        for k in ("plain", "reg_all", "reg_part", "reg_part2"):
            w[k].close()


def _call(w, form, layout):
    """One groups call; returns (group bits, signature bits, registry hits, registry misses)."""
    d = w["lay"][layout]
    if form == "keyset":
        gb, sb = w["ks"].verify_batch_groups(d["kidx"], d["sig"], d["first"], w["cnt"], d["msg32"], with_sig_bits=True)
        return gb, sb, None, None
    be = w["plain" if form == "raw" else form]
    i0 = be.key_cache_info()
    gb, sb = be.verify_batch_groups(d["pk"], d["sig"], d["first"], w["cnt"], d["msg32"], with_sig_bits=True)
    i1 = be.key_cache_info()
    return gb, sb, i1["hits"] - i0["hits"], i1["misses"] - i0["misses"]


def _check(w, form, layout, got):
    gb, sb, hits, misses = got
    assert np.array_equal(gb, w["want_g"]), (form, layout, "group bits")
    assert np.array_equal(sb, w["lay"][layout]["want_s"]), (form, layout, "signature bits")
    if form.startswith("reg"):
        reg = w["m"] if form == "reg_all" else w["registered"]
        assert (hits, misses) == (reg, w["m"] - reg), (form, layout, hits, misses)


@pytest.mark.parametrize("chunking", list(CHUNKINGS))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_group_paths_match_oracle(world, monkeypatch, layout, form, chunking):
    chunks, rnd = CHUNKINGS[chunking]
    monkeypatch.setenv("NT_PIPE_CHUNKS", chunks)
    if rnd:
        monkeypatch.setenv("NT_PIPE_ROUND", rnd)
    else:
        monkeypatch.delenv("NT_PIPE_ROUND", raising=False)
    _check(world, form, layout, _call(world, form, layout))


def test_miss_fallback_on_second_shard(world, monkeypatch):
    """Two device entries: the second shard starts at group 128, so its misses'
    verdict bits and group words are relative to a shard start that is not 0."""
    monkeypatch.setenv("NT_PIPE_CHUNKS", "16")
    monkeypatch.setenv("NT_PIPE_ROUND", "64")
    assert world["reg_part2"].num_devices == 2
    _check(world, "reg_part", "scattered", _call(world, "reg_part2", "scattered"))
