"""The committee key cache at the widths production runs: 21-bit reduced-scalar
combs (the default whenever they fit) and 20-bit combs (the first fallback of
the HBM budget), over tests/golden/torsion_votes.npz -- votes under
mixed-order and order-8 keys beside prime-order controls, every label from the
generator's Python-integer model.

Only the 21-bit width takes k = H(R || A || M) mod L as k or k - L, and for a
key with a torsion component it then owes the key's [L](-A) comb entry
(ed25519_ops.hpp key_comb_sum).  Everything around that kernel that decides a
verdict -- the counting sort and the scattered verdicts of launches of at
least 65,536 signatures, the fused group epilogue, the per-lane caps and the
chunked plan -- runs here at that width, with whole waves on one such key.

One key set of the 12 keys per width (19 GB at 21 bits), closed before the
next width's is built.  Every test asserts the width the device gave: a test
fails, it does not skip, when that is another one.

The key-cache kernel loads each signature's key by the signature's own index
and writes the verdict there, so no verdict can tell whether the counting sort
grouped anything: test_key_sort_groups_by_key reads the permutation itself
through the device probe (tests/cpp/nt_device_probe.hip ntp_key_sort, which
calls the product's launch_key_sort of csrc/key_sort.hpp)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _torsion_votes as T

pytestmark = pytest.mark.gpu


def nbytes(t):
    return int(t.numel()) * int(t.element_size())


@pytest.fixture(scope="module")
def tv():
    return T.load()


@pytest.fixture(scope="module")
def be():
    import ntcrypto
    b = ntcrypto.Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module", params=[21, 20])
def wks(request, be, tv):
    """(bits, key set of the fixture's 12 keys).  21 is what the library picks
    with no override; 20 is forced, as the budget would when 21 does not fit."""
    bits = request.param
    old = os.environ.pop("NT_KEYSET_COMB_BITS", None)
    if bits != 21:
        os.environ["NT_KEYSET_COMB_BITS"] = str(bits)
    try:
        ks = be.keyset(tv["keys"])
    finally:
        os.environ.pop("NT_KEYSET_COMB_BITS", None)
        if old is not None:
            os.environ["NT_KEYSET_COMB_BITS"] = old
    yield bits, ks
    ks.close()


def _want_mixed(tv, rows, strict):
    return np.where(strict, tv["strict"][rows], tv["batch_rule"][rows]).astype(bool)


def test_width_input_order(be, tv, wks):
    """The 480 entries in input order (below 65,536 signatures a launch keeps
    it): strict, cofactorless and mixed mode (strict bit on i % 3 == 1), as the
    fixture has them -- 40 neighbouring lanes on one key -- and with the rows
    interleaved so that neighbouring lanes hold different keys (the wave_any
    branch of the [L](-A) entry taken by some lanes of a wave only)."""
    import ntcrypto
    bits, ks = wks
    assert ks.info()[0] == bits
    msg = tv["msg32"].reshape(-1)
    n = len(tv["key"])
    nk, nd = len(tv["keys"]), len(tv["msg32"])
    for name, rows in (("fixture order", np.arange(n)), ("interleaved", np.arange(n).reshape(nk, nd).T.ravel())):
        key = tv["key"][rows].astype(np.uint32)
        if name == "interleaved":
            assert (key[1:] != key[:-1]).all()
        args = (tv["sig"][rows], msg, tv["off"][rows], tv["len"][rows])
        got_s = ks.verify(ntcrypto.NT_MODE_STRICT, key, *args)
        got_c = ks.verify(ntcrypto.NT_MODE_COFACTORLESS, key, *args)
        strict = (np.arange(n) % 3) == 1
        midx = (key | np.where(strict, np.uint32(ntcrypto.NT_KEY_STRICT_BIT), np.uint32(0))).astype(np.uint32)
        got_m = ks.verify(ntcrypto.NT_MODE_MIXED, midx, *args)
        for mode, got, want in (("strict", got_s, tv["strict"][rows].astype(bool)),
                                ("cofactorless", got_c, tv["batch_rule"][rows].astype(bool)),
                                ("mixed", got_m, _want_mixed(tv, rows, strict))):
            bad = np.flatnonzero(got != want)
            print("%d bits, %s, %s: %d of %d differ from the labels" % (bits, name, mode, len(bad), n))
            assert len(bad) == 0, (bits, name, mode, rows[bad][:16].tolist())


def _tiled_call(tv):
    """The entries tiled past 65,535 signatures (T.tiled_order), mixed mode with
    an unknown key index on i % 97 == 5: (rows, key indices with the strict
    bit, sort buckets, expected verdicts)."""
    import ntcrypto
    rows = T.tiled_order(tv)
    n = len(rows)
    i = np.arange(n)
    unknown = (i % 97) == 5
    strict = (i % 3) == 1
    nk = len(tv["keys"])
    bucket = np.where(unknown, nk, tv["key"][rows]).astype(np.uint32)
    idx = np.where(unknown, nk + 3, tv["key"][rows]).astype(np.uint32)
    midx = (idx | np.where(strict, np.uint32(ntcrypto.NT_KEY_STRICT_BIT), np.uint32(0))).astype(np.uint32)
    return rows, midx, bucket, _want_mixed(tv, rows, strict) & ~unknown


def test_width_key_grouped_order(be, tv, wks):
    """A launch of 65,760 signatures: the counting sort by key runs, each wave
    walks one key's comb, the verdicts are scattered back to the signatures'
    own indices.  Mixed mode, unknown key indices; the verdict per signature is
    the label.  As slots follow the key-grouped order every key with a torsion
    component has waves of 64 with every lane on the high branch (all owe the
    [L](-A) entry), waves with none on it and waves with both (checked on the
    stable sort; T.tiled_order says why the device's order has them too)."""
    import ntcrypto
    bits, ks = wks
    assert ks.info()[0] == bits
    rows, midx, bucket, want = _tiled_call(tv)
    n = len(rows)
    assert n >= T.SORT_MIN and n % len(tv["key"]) == 0 and n - len(tv["key"]) < T.SORT_MIN
    waves, one_key, nw = T.wave_branches(tv, rows, bucket)
    print("%d signatures, %d waves of 64 slots, %d on one key" % (n, nw, one_key))
    for ki, (allhi, none, mixed) in sorted(waves.items()):
        print("  key %2d: %3d waves all on the high branch, %3d with none, %3d mixed" % (ki, allhi, none, mixed))
        assert allhi >= 1 and none >= 1 and mixed >= 1, (ki, waves)
    assert one_key >= nw - 13
    got = ks.verify(ntcrypto.NT_MODE_MIXED, midx, tv["sig"][rows], tv["msg32"].reshape(-1), tv["off"][rows],
                    tv["len"][rows])
    bad = np.flatnonzero(got != want)
    print("%d bits, key-grouped order: %d of %d differ from the labels" % (bits, len(bad), n))
    assert len(bad) == 0, (bits, bad[:16].tolist(), rows[bad][:16].tolist())
    assert 0.5 * n < want.sum() < n


@pytest.fixture(scope="module")
def certs(tv):
    return T.certificates(tv)


def test_width_groups_fused(be, tv, wks, certs):
    """Certificates of 0-12 votes from the fixture, 65,5xx signatures in one
    key-grouped launch whose epilogue ANDs each group's verdicts: through
    ks.verify_batch_groups (host entry point: the call's n is the end of its
    last group, an accepted one) and through
    nt_dev_ed25519_verify_keyset_groups, where one more group starts two
    signatures before n and reaches three past it (the host entry point cannot
    express that: it takes no n), so it must reject although the signatures it
    does have are valid.  Group verdict = AND of batch_rule over the group's
    votes, signature bits = batch_rule."""
    import ntcrypto
    import torch
    bits, ks = wks
    assert ks.info()[0] == bits
    rows, first, cnt, msg32, want_group, want_sig = certs
    n, G = len(rows), len(cnt)
    kidx = tv["key"][rows].astype(np.uint32)
    sig = np.ascontiguousarray(tv["sig"][rows])
    gb, sb = ks.verify_batch_groups(kidx, sig, first, cnt, msg32, with_sig_bits=True)
    print("%d bits, host entry: %d of %d groups, %d of %d signature bits differ" % (
        bits, int((gb != want_group).sum()), G, int((sb != want_sig).sum()), n))
    assert np.array_equal(sb, want_sig), np.flatnonzero(sb != want_sig)[:16].tolist()
    assert np.array_equal(gb, want_group), np.flatnonzero(gb != want_group)[:16].tolist()
    # the device entry point, one more group reaching past n
    first2 = np.concatenate([first, [n - 2]]).astype(np.uint64)
    cnt2 = np.concatenate([cnt, [5]]).astype(np.uint32)
    assert want_sig[n - 2:].all() and (np.diff(first2.astype(np.int64)) >= 0).all()
    G2 = G + 1
    goff = np.repeat(np.arange(G, dtype=np.uint64) * 32, cnt)
    dev = torch.device("cuda", 0)
    t = {"k": torch.from_numpy(kidx.view(np.int32)).to(dev), "sig": torch.from_numpy(sig).to(dev),
         "msg": torch.from_numpy(np.ascontiguousarray(msg32).reshape(-1)).to(dev),
         "off": torch.from_numpy(goff.view(np.int64)).to(dev),
         "len": torch.full((n,), 32, dtype=torch.int64, device=dev),
         "first": torch.from_numpy(first2.view(np.int64)).to(dev), "cnt": torch.from_numpy(cnt2.view(np.int32)).to(dev)}
    w = torch.full(((n + 63) // 64 + 1,), -1, dtype=torch.int64, device=dev)      # garbage: the call owns the words
    gw = torch.full(((G2 + 63) // 64 + 1,), 0x5A5A, dtype=torch.int64, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    ks.dev_verify_groups(0, st.cuda_stream, ntcrypto.NT_MODE_COFACTORLESS, t["k"].data_ptr(), t["sig"].data_ptr(),
                         t["msg"].data_ptr(), nbytes(t["msg"]), t["off"].data_ptr(), t["len"].data_ptr(), n,
                         t["first"].data_ptr(), t["cnt"].data_ptr(), G2, w.data_ptr(), gw.data_ptr())
    st.synchronize()
    s1 = np.unpackbits(w.cpu().numpy()[:(n + 63) // 64].view(np.uint8), bitorder="little")[:n].astype(bool)
    gws = (G2 + 63) // 64
    b1 = np.unpackbits(gw.cpu().numpy()[:gws].view(np.uint8), bitorder="little").astype(bool)
    print("%d bits, device entry: %d of %d groups, %d of %d signature bits differ; group past n: %d" % (
        bits, int((b1[:G] != want_group).sum()), G, int((s1 != want_sig).sum()), n, int(b1[G])))
    assert np.array_equal(s1, want_sig), np.flatnonzero(s1 != want_sig)[:16].tolist()
    assert np.array_equal(b1[:G], want_group), np.flatnonzero(b1[:G] != want_group)[:16].tolist()
    assert b1[G - 1] and not b1[G]      # the group ending at n accepts, the one reaching past it rejects
    assert not b1[G2:].any()            # bits past the last group stay clear


@pytest.mark.parametrize("stream,cap,waves,srt", [("1", 3, "3", "1"), ("1", 64, "", "0"), ("0", 5, "2", "1")],
                         ids=["streamed-cap3-3waves", "streamed-cap64-input-order", "chunked-cap5"])
def test_width_plans_and_caps(stream, cap, waves, srt):
    """The per-lane caps and the two plans at 21 bits (read once per process,
    so in a subprocess each): streamed rows with an inversion every 3 rows at
    three waves per SIMD, streamed rows at the full cap in input order at both
    sizes, the chunked plan with cap 5 -- over the fixture's key set, 480 and
    65,760 signatures, mixed mode with unknown key indices."""
    probe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_keyset_per_lane_probe.py")
    env = dict(os.environ, NT_KEYSET_PER_LANE=str(cap), NT_KEYSET_COMB_BITS="21", NT_KEYSET_STREAM=stream,
               NT_KEYSET_SORT=srt)
    env.pop("NT_KEYSET_WAVES", None)
    if waves:
        env["NT_KEYSET_WAVES"] = waves
    r = subprocess.run([sys.executable, probe, "torsion"], env=env, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["per_lane"] == str(cap) and res["comb_bits"] == 21
    sizes = sorted(int(k.split("_")[1]) for k in res if k.startswith("mismatches"))
    assert len(sizes) == 2 and sizes[0] == 480 and T.SORT_MIN <= sizes[1] < T.SORT_MIN + 480
    assert not {k: v for k, v in res.items() if k.startswith("mismatches") and v}, res


def _bucket(idx, mixed, nkeys):
    k = idx & np.uint32(0x7FFFFFFF) if mixed else idx
    return np.where(k < nkeys, k, nkeys).astype(np.int64)


def _sort_cases(tv):
    """(name, key indices as a launch gets them, mixed, nkeys): the tiled fixture call (12 keys,
    strict bits, unknown indices, a partial last block of the scatter), single blocks and one
    signature more, and 300 keys (more buckets than threads of a block, an odd size), where
    bit 31 outside mixed mode is just an unknown key"""
    _, midx, _, _ = _tiled_call(tv)
    rng = np.random.default_rng(23)
    yield "tiled fixture", midx, 1, len(tv["keys"])
    for n in (1, 63, 4096, 4097):
        yield "n=%d" % n, rng.integers(0, 14, n).astype(np.uint32), 0, 12
    wide = rng.integers(0, 310, 70001).astype(np.uint32)
    wide[::11] |= np.uint32(1 << 31)
    yield "300 keys", wide, 0, 300
    yield "300 keys, mixed", wide, 1, 300


def test_key_sort_groups_by_key(tv):
    """The permutation a key-cache launch of >= 65,536 signatures walks (k_key_hist,
    k_key_scatter through launch_key_sort, with the launcher's own grid and LDS sizes): every
    signature exactly once, and slot after slot the bucket never decreases -- the committee
    keys in index order, every unknown index last -- so a wave of 64 slots holds one key
    except where two buckets meet."""
    import _devprobe
    lib = _devprobe.load()
    for name, idx, mixed, nkeys in _sort_cases(tv):
        idx = np.ascontiguousarray(idx, np.uint32)
        n = len(idx)
        perm = np.zeros(n, np.uint32)
        rc = lib.ntp_key_sort(ctypes.c_uint64(n), idx.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(mixed),
                              ctypes.c_uint32(nkeys), perm.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0, (name, rc)
        assert np.array_equal(np.sort(perm), np.arange(n, dtype=np.uint32)), name
        b = _bucket(idx, mixed, nkeys)[perm]
        breaks = int((np.diff(b) < 0).sum())
        waves = b[:n // 64 * 64].reshape(-1, 64)
        one_key = int((waves == waves[:, :1]).all(axis=1).sum())
        print("%s: %d signatures, %d buckets in use, %d places where the bucket decreases, %d of %d waves on one key"
              % (name, n, len(np.unique(b)), breaks, one_key, len(waves)))
        assert breaks == 0, name
        assert one_key >= len(waves) - len(np.unique(b)), name
