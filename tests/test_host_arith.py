"""CPU tests of the exact device arithmetic (narwhal-tusk_amd/csrc/*.hpp compiled
for the host by tests/cpp/).  These stress the radix-2^25.5 bound discipline at
the extreme limb values the point formulas can produce (a silent u64 overflow
would only show on adversarial limbs, never on random signatures), and replay
the golden corpus through the same verify_n<> / verify_cached_n<> / sign_one the
kernels run, and check the wide-comb construction against a textbook curve model.
"""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import _arith_checks as C
import _hostarith as H

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def host():
    return H.runner("")


# The checks of tests/_arith_checks.py take a runner: here the host build of the
# headers, in tests/test_gpu_device_arith.py the gfx950 build behind the device probe.
def test_fe_mul_extreme_bounds(host):
    C.check_fe_mul_bounds(host)


def test_fe_sq_extreme_bounds(host):
    C.check_fe_sq_bounds(host)


def test_fe_tobytes_canonical(host):
    C.check_fe_bytes(host)


def test_sc_reduce512(host):
    C.check_sc_reduce512(host)


def test_sc_muladd_mul_canonical(host):
    C.check_sc_mul(host)


def test_sc_reduce_half(host):
    C.check_sc_reduce_half(host)


def test_sc_recode_w4(host):
    C.check_sc_recode_w4(host)


def test_hram_every_alignment(host):
    C.check_hram(host)


def test_point_decoding_and_small_order(host):
    C.check_point_checks(host)


@pytest.mark.parametrize("variant", ["", "_fullgcd"])
def test_inversion_wave_compositions(variant):
    """default build: the loop is left per value once a = 0; _fullgcd
    (-DNT_GCD_EARLY_EXIT=0): all 17 outer iterations for every value, which is what
    a GPU lane runs whose wave still has work (iterations with a = 0)"""
    C.check_inversion(H.runner(variant))


def test_inversion_inputs_take_the_negation_branch():
    """gcd_lincomb_shift negates a negative matrix row about once in 3,000
    inversions; the inputs of the inversion check must reach that branch"""
    vals, _ = C.inversion_inputs()
    counts = [H.gcd_neg_count(C.to_limbs(v)) for v in vals]
    assert min(counts) >= 0  # -1: the harness's restated loop no longer ends in a = 0, b = 1
    took = sum(c > 0 for c in counts)
    print("inversion inputs that negate a row: %d of %d" % (took, len(vals)))
    assert took >= 3


@pytest.mark.parametrize("variant", ["", "_rcp"])
def test_halfsize_twin(variant):
    """default build: exact quotients floor(a / b); _rcp: floor(a * r) with r = 1 / b
    off by up to 2 ulp (NT_LAT_RCP_MODEL, a model of the device's v_rcp_f64), so the
    quotient corrections of lat_lehmer_batch run; both must equal the default
    build's one-step loop"""
    C.check_halfsize(H.runner(variant), H.runner("").sc_halfsize(C.halfsize_scalars(), 0))


def test_ladder_lane_mixed_window_counts(host):
    C.check_ladder(host, H.host_halfsize)


@pytest.mark.parametrize("variant", ["", "_rcp"])
def test_unbalanced_twin(variant):
    """the unbalanced lattice vector (the 2^191.5 stop) on the scalars of
    C.unbalanced_scalars(): both builds, as in test_halfsize_twin, must equal the default
    build's one-step loop and the integer model"""
    C.check_unbalanced(H.runner(variant), H.runner("").sc_unbalanced(C.unbalanced_scalars(), 0))


def test_key_table_entries_and_cached_points(host):
    C.check_ktab_tables(host)


def test_three_table_ladder_lane_mixed_window_counts(host):
    C.check_ladder3(host, H.host_unbalanced, H.host_halfsize)


@pytest.mark.parametrize("bits", C.COMB_WIDTHS)
def test_wide_comb_tables(host, bits):
    """wcomb_key_bases + wcomb_fill through wcomb_fill_target at all five widths (16 bits: whole
    combs, built batch by batch as wcomb_build launches them)"""
    print("comb entries compared at %d bits: %d" % (bits, C.check_wcomb_tables(host, bits)))


@pytest.mark.parametrize("bits", C.COMB_WIDTHS)
def test_wide_comb_digits(host, bits):
    print("digit vectors compared at %d bits: %d" % (bits, C.check_wcomb_digits(host, bits)))


@pytest.mark.parametrize("bits", C.COMB_WIDTHS)
def test_wide_comb_sums(host, bits):
    print("comb sums compared at %d bits: %d" % (bits, C.check_wcomb_acc(host, bits)))


def test_key_comb_sum_lane_mixed_corrections(host):
    print("key comb sums compared per width: %d" % C.check_key_comb_sum(host))


def test_wide_comb_entry_points_refuse_bad_arguments(host):
    print("comb calls refused: %d" % C.check_wcomb_refusals(host))


def test_key_comb_lines_and_claim_compositions(host):
    """ktab_build with a comb pool over HostKComb, every line against the point model"""
    print("comb lines compared: %d" % C.check_kcomb_tables(host))


def test_comb_recoding_picks(host):
    print("pick vectors compared: %d" % C.check_kc_picks(host))


def test_comb_ladder_lane_mixed_parity_entry_and_dead(host):
    print("comb ladder results compared: %d" % C.check_ladder_kc(host))


def test_compare_one_chosen_points(host):
    print("compare_one bits compared: %d" % C.check_compare_one(host))


def test_verify_kc_chosen_scalars(host):
    print("verify_kc verdicts compared: %d" % C.check_verify_kc(host))


def test_comb_entry_points_refuse_bad_arguments(host):
    print("comb-path calls refused: %d" % C.check_kcomb_refusals(host))


def test_comb_items_under_the_sanitizers():
    """The stand-alone program (its own main, -fsanitize=address,undefined, run directly): the
    probe's comb items over HostKComb on exact-size heap allocations, the key set of
    ktab_items_check with room for every key and with a pool of 4."""
    import subprocess
    subprocess.run(["make", "-s", "-C", H.CPP, "build/kcomb_items_check"], check=True)
    r = subprocess.run([os.path.join(H.CPP, "build", "kcomb_items_check")], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_shared_entry_points_under_the_sanitizers():
    """The stand-alone program (its own main, -fsanitize=address,undefined, run directly): every
    entry of nt_probe_entries.inc on the host runner at n = 0, 1 and 65, on heap buffers of exactly
    the described sizes, byte for byte against a direct loop over the same items; every refusal of
    the argument checks returns non-zero and leaves outputs and blob untouched."""
    import subprocess
    subprocess.run(["make", "-s", "-C", H.CPP, "build/probe_entries_check"], check=True)
    r = subprocess.run([os.path.join(H.CPP, "build", "probe_entries_check")], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr


def _fill_targets(bits, nkeys, t):
    """wcomb_fill_target of the threads t: (live, key, pos, chunk, dst, tmp) columns and the width's
    geometry (kPos, kChunks, kEntries, kWordsPerPoint, kCorrWord, comb / bases / tmp bytes per key, batch)"""
    import ctypes
    t = np.ascontiguousarray(t, np.uint64)
    out, geom = np.zeros((len(t), 6), np.uint64), np.zeros(9, np.uint64)
    rc = H.load().nth_wcomb_fill_targets(bits, ctypes.c_uint32(nkeys), ctypes.c_uint64(len(t)), C._p(t), C._p(out), C._p(geom))
    assert rc == 0
    return out.astype(np.int64), [int(g) for g in geom]


@pytest.mark.parametrize("bits", C.COMB_WIDTHS)
def test_wcomb_fill_target_map(bits):
    """The thread -> (key, position, chunk) map of k_wcomb_fill for 1, 2 and 5 keys, every thread of
    the grid (24 bits: every 61st, and the first and last thread of every key and position): key,
    position and chunk invert to t; the chunks' 64-entry destinations are disjoint, cover each
    position of each key exactly from entry 1 on (entry 0 is chunk 0's extra write) and stay inside
    the keys' combs; the tmp slices are disjoint and inside the product's tmp size for the batch;
    threads past the work are dead.  Then the per-batch offsets of wcomb_build's launches."""
    import ctypes
    npos, chunks, entries = C.comb_geom(bits)
    per_key = npos * chunks
    for nkeys in (1, 2, 5):
        threads = per_key * nkeys
        if bits == C.COMB_B:
            firsts = np.arange(0, threads, chunks)
            t = np.unique(np.concatenate([np.arange(0, threads, 61), firsts, firsts + chunks - 1]))
        else:
            t = np.arange(threads)
        t = np.concatenate([t, threads + np.array([0, 1, 63, per_key, 1 << 33])]).astype(np.uint64)
        got, geom = _fill_targets(bits, nkeys, t)
        assert geom[:3] == [npos, chunks, entries]
        wpp, corr_word, comb_bytes, bases_bytes, tmp_bytes, batch = geom[3:]
        assert corr_word == npos * entries * 32 and wpp == corr_word + (32 if bits == C.COMB_REDUCED else 0)
        assert comb_bytes == 4 * wpp and bases_bytes == 160 * npos and tmp_bytes == per_key * 2560
        assert batch == max(1, (128 << 10) // per_key)
        live, key, pos, chunk, dst, tmp = got.T
        ti = t.astype(np.int64)
        assert np.array_equal(live != 0, ti < threads)
        m = live != 0
        ti, key, pos, chunk, dst, tmp = ti[m], key[m], pos[m], chunk[m], dst[m], tmp[m]
        assert np.all((key < nkeys) & (pos < npos) & (chunk < chunks))
        assert np.array_equal((key * npos + pos) * chunks + chunk, ti)
        # a chunk writes entries [first, first + 64) of its position; chunk 0 also the entry before
        assert np.all(dst % 32 == 0)
        first = dst // 32 - key * (wpp // 32) - pos * entries       # entry index inside the position
        assert np.array_equal(first, 1 + 64 * chunk)
        assert np.all(first + 64 <= entries) and first.min() == 1 and (first + 64).max() == entries
        if bits != C.COMB_B:                                        # every thread: disjoint, exact cover
            order = np.argsort(dst)
            assert np.all(np.diff(dst[order]) >= 64 * 32)
            assert len(np.unique(key * npos + pos)) == nkeys * npos and len(dst) == nkeys * npos * chunks
        assert dst.max() + 64 * 32 <= wpp * nkeys - (32 if bits == C.COMB_REDUCED else 0)
        assert np.all(tmp % 640 == 0) and len(np.unique(tmp)) == len(tmp)
        assert tmp.max() + 640 <= tmp_bytes // 4 * nkeys
    out = np.zeros(4, np.uint64)
    for total, batch in ((5, 2), (1, 1), (5, 16), (2, 2), (5, 1)):
        k0, seen = 0, []
        while k0 < total:
            assert H.load().nth_wcomb_fill_launch(bits, ctypes.c_uint32(k0), ctypes.c_uint32(total), ctypes.c_uint32(batch), C._p(out)) == 0
            nk, threads, bases_off, comb_off = (int(x) for x in out)
            assert 1 <= nk <= batch and nk == min(batch, total - k0) and threads == nk * per_key
            assert bases_off == k0 * npos * 40 and comb_off == k0 * wpp
            seen.append(nk)
            k0 += batch
        assert sum(seen) == total and len(seen) == -(-total // batch)


def test_device_probe_exports_every_entry():
    """tests/cpp/build/libntprobe.so (the gfx950 build of the same item functions)
    exports one ntp_* entry point per check; loading it needs no GPU"""
    import subprocess
    import _devprobe
    subprocess.run(["make", "-s", "-C", H.CPP, "build/libntprobe.so"], check=True)
    lib = _devprobe.load()
    for sym in _devprobe.EXPORTS:
        getattr(lib, sym)
    assert len(_devprobe.EXPORTS) == 34
    lib.ntp_key_sort  # device-only: the product's counting sort (csrc/key_sort.hpp), no host twin


def test_sha512_host_build():
    """both block loops: sha512_prefixed and the one-compression-site form the
    digest kernel uses (sha512_prefixed_1site), at every padding boundary"""
    for n in (0, 1, 111, 112, 113, 127, 128, 129, 239, 240, 255, 256, 1000, 3336, 5000):
        m = bytes(range(256)) * (n // 256 + 1)
        m = m[:n]
        assert H.sha512(m) == hashlib.sha512(m).digest()
        assert H.sha512(m, one_site=True) == hashlib.sha512(m).digest()


def test_hram_one_block_path_matches_hashlib():
    """hram_scalar<true> (the key-cache kernels: a 32-byte message hashed as one
    block built from registers) and the general path both equal
    SHA-512(R || A || M) mod L; other lengths fall through to the general path."""
    rng = random.Random(96)
    for n in (32, 32, 32, 0, 31, 33, 64):
        sig = bytes(rng.getrandbits(8) for _ in range(64))
        pk = bytes(rng.getrandbits(8) for _ in range(32))
        m = bytes(rng.getrandbits(8) for _ in range(n))
        want = (int.from_bytes(hashlib.sha512(sig[:32] + pk + m).digest(), "little") % H.L).to_bytes(32, "little")
        assert H.hram(sig, pk, m, True) == want, n
        assert H.hram(sig, pk, m, False) == want, n


def test_corpus_through_device_code():
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    for i in range(len(d["cat"])):
        o, n = int(d["off"][i]), int(d["len"][i])
        pk, sig, m = d["pk"][i].tobytes(), d["sig"][i].tobytes(), d["msg"][o:o + n].tobytes()
        assert H.verify(0, pk, sig, m) == bool(d["strict"][i]), i
        assert H.verify(1, pk, sig, m) == bool(d["batch_rule"][i]), i


def test_corpus_pairs_through_device_code():
    """The two-per-lane path (one shared inversion) the verify kernels run, and the
    key-cache path; each corpus entry is paired with its neighbour."""
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    n = len(d["cat"])

    def entry(i):
        o, ln = int(d["off"][i]), int(d["len"][i])
        return d["pk"][i].tobytes(), d["sig"][i].tobytes(), d["msg"][o:o + ln].tobytes()

    for i in range(n):
        j = (i + 1) % n
        a, b = entry(i), entry(j)
        for mode, key in ((0, "strict"), (1, "batch_rule")):
            want = (bool(d[key][i]), bool(d[key][j]))
            assert H.verify_pair(mode, *a, *b) == want, (i, mode)
            if i % 3 == 0:
                assert H.verify_pair(mode, *a, *b, cached=True) == want, (i, mode, "cached")


def test_corpus_through_fallback_ladder():
    """The same verdicts through the trivial lattice vector (k, 1) -- the full
    253-bit ladder sc_halfsize falls back to (step cap / oversized vectors)."""
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    for i in range(0, len(d["cat"]), 2):
        o, n = int(d["off"][i]), int(d["len"][i])
        pk, sig, m = d["pk"][i].tobytes(), d["sig"][i].tobytes(), d["msg"][o:o + n].tobytes()
        assert H.verify_trivial(0, pk, sig, m) == bool(d["strict"][i]), i
        assert H.verify_trivial(1, pk, sig, m) == bool(d["batch_rule"][i]), i


def test_corpus_through_keyset_path():
    """The key-cache kernel's batch of 8 signatures per lane (one inversion for
    all eight, R'_j staged): every corpus entry in a group of 8 with seven
    neighbours, plus groups of 3 (the count is a kernel argument)."""
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    n = len(d["cat"])

    def entry(i):
        o, ln = int(d["off"][i]), int(d["len"][i])
        return d["pk"][i].tobytes(), d["sig"][i].tobytes(), d["msg"][o:o + ln].tobytes()

    for g, step in ((8, 8), (3, 37)):
        for i in range(0, n, step):
            idx = [(i + k) % n for k in range(g)]
            for mode, key in ((0, "strict"), (1, "batch_rule")):
                want = tuple(bool(d[key][j]) for j in idx)
                assert H.verify_cached_n(mode, [entry(j) for j in idx]) == want, (i, mode)
            # mixed mode (one launch for header + vote signatures): per-entry strictness
            mask = (i * 37 // step) % (1 << g)
            want = tuple(bool(d["strict" if (mask >> k) & 1 else "batch_rule"][j]) for k, j in enumerate(idx))
            assert H.verify_cached_n(2, [entry(j) for j in idx], strict_mask=mask) == want, (i, "mixed", mask)


@pytest.mark.parametrize("bits", [21])
def test_corpus_through_reduced_key_combs(bits):
    """The same corpus through 21-bit key combs (the device's first choice): k
    taken as k or k - L, 12 positions, and the key's [L](-A) entry added when
    k - L was used -- small-order and mixed-order keys included, every mode."""
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    n = len(d["cat"])

    def entry(i):
        o, ln = int(d["off"][i]), int(d["len"][i])
        return d["pk"][i].tobytes(), d["sig"][i].tobytes(), d["msg"][o:o + ln].tobytes()

    for i in range(0, n, 8):
        idx = [(i + k) % n for k in range(8)]
        for mode, key in ((0, "strict"), (1, "batch_rule")):
            want = tuple(bool(d[key][j]) for j in idx)
            assert H.verify_cached_n(mode, [entry(j) for j in idx], bits=bits) == want, (i, mode)
        mask = (i * 37 // 8) % 256
        want = tuple(bool(d["strict" if (mask >> k) & 1 else "batch_rule"][j]) for k, j in enumerate(idx))
        assert H.verify_cached_n(2, [entry(j) for j in idx], strict_mask=mask, bits=bits) == want, (i, "mixed")


def test_reduced_comb_sum_equals_full_comb():
    """[k](-A) from the 21-bit reduced-scalar comb equals the 20-bit comb's for
    honest, small-order and mixed-order keys of the corpus and for scalars at
    the reduction's edges ((L - 1) / 2, (L + 1) / 2, L - 1, 0, 1, 2^251 +- 1) and
    random ones; the key's torsion flag is set exactly for keys with a torsion
    component (the corpus's small- and mixed-order categories but the identity)."""
    d = np.load(os.path.join(GOLD, "ed25519_corpus.npz"))
    meta = json.load(open(os.path.join(GOLD, "ed25519_corpus.json")))
    cats = meta["categories"]
    rng = np.random.default_rng(21)
    L = H.L
    edges = [0, 1, 2, (L - 1) // 2, (L + 1) // 2, (L + 3) // 2, L - 1, L - 2, (1 << 251) - 1, 1 << 251,
             (1 << 251) + 1, (1 << 252) - 1]
    seen = {}
    for i in range(len(d["cat"])):
        cat = cats[int(d["cat"][i])]
        if cat not in ("honest", "small_order_A", "mixed_A_valid") or seen.get(cat, 0) >= 6:
            continue
        seen[cat] = seen.get(cat, 0) + 1
        A = d["pk"][i].tobytes()
        ks = edges + [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % L
                      for _ in range(24)]
        for k in ks:
            e21, m21 = H.key_comb_sum(21, A, k)
            e20, m20 = H.key_comb_sum(20, A, k)
            assert e21 == e20, (cat, i, k)
            # the identity (y = 1, either sign bit) is small order without a torsion component
            ident = A[0] == 1 and not any(A[1:31]) and A[31] in (0, 0x80)
            assert bool(m21 & H.KEY_TORSION) == (cat != "honest" and not ident), (cat, i)
            assert (m21 & ~H.KEY_TORSION) == m20
    assert set(seen) == {"honest", "small_order_A", "mixed_A_valid"}


def test_sc_halfsize_lehmer_equals_one_step():
    """The Lehmer-batched reduction the kernels run lands on exactly the
    (u, v, sign, bits) of the one-step Euclid loop: random k < L, k near L,
    near 2^252, small / power-of-two / Fibonacci-ratio scalars (all-ones
    quotient runs) and huge partial quotients."""
    rng = random.Random(1234)
    ks = [rng.randrange(H.L) for _ in range(200_000)]
    ks += [H.L - 1 - i for i in range(64)] + [(1 << 252) + i for i in range(64)] + [(1 << 252) - 1 - i for i in range(64)]
    ks += [0, 1, 2, 3] + [1 << b for b in range(0, 253)] + [(1 << b) - 1 for b in range(1, 253)]
    # k / 8L close to a ratio of consecutive Fibonacci numbers -> long runs of quotient 1
    fa, fb = 1, 1
    while fb < 1 << 126:
        fa, fb = fb, fa + fb
    ks += [(8 * H.L * fa // fb + d) % H.L for d in range(-32, 33)]
    # huge first quotients: k tiny relative to 8L, and 8L / k just above an integer
    ks += [(8 * H.L) // q + d for q in (3, 1 << 20, 1 << 31, (1 << 32) + 1, 1 << 40, 1 << 60) for d in range(-3, 4)]
    ks = [k % H.L for k in ks]
    assert H.halfsize_disagree(ks) == 0


def test_sc_halfsize_properties():
    """Half-size scalars (sc25519.hpp): for every k < L the result satisfies
    u == v k (mod 8L), v odd, 0 < v < L, and bits >= bitlen(|u|), bitlen(v)
    (the window count is never too small); typical sizes ~2^128.  Edge inputs
    include k = 0, tiny k (loop not entered), k near L, powers of two and
    values with huge partial quotients."""
    L8 = 8 * H.L
    rng = random.Random(9)
    ks = [0, 1, 2, 7, 8, 9, H.L - 1, H.L - 2, H.L // 2, (H.L - 1) // 8, 1 << 127, (1 << 127) + 1, 1 << 128,
          (1 << 200) + 12345, (1 << 252) - 1, H.L - (1 << 126), L8 // 3, L8 // 5]
    ks += [(L8 * j) // (1 << 40) for j in range(1, 6)]          # huge first quotients
    ks += [(L8 // q) + d for q in (3, 1 << 33, 1 << 70) for d in (-1, 0, 1)]
    ks = [k % H.L for k in ks] + [rng.randrange(H.L) for _ in range(3000)]
    big = 0
    for k in ks:
        u, v, bits = H.sc_halfsize(k)
        assert (u - v * k) % L8 == 0, k
        assert v % 2 == 1 and 0 < v < H.L, k
        assert bits >= max(abs(u).bit_length(), v.bit_length()) and bits <= 253, k
        big += bits > 136
    assert big < 30  # random k: almost always ~128 bits


def _model():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_small_order_by_torsion_y():
    """The kernels' small-order test (y in {1, -1, 0, +-y8}) equals [8]P == 0 by
    doublings (and the textbook model) on every small-order encoding the corpus
    uses -- canonical, non-canonical (y + p) and negative-zero forms -- on
    mixed-order points T + aB and on random points."""
    M = _model()
    encs = list(M.small_order_encodings()) + [M.encode(t) for t in M.TORSION]
    rng = random.Random(5)
    for t in M.TORSION:
        for _ in range(3):
            encs.append(M.encode(M.padd(t, M.pmul(rng.randrange(1, M.L), M.BASE))))
    encs += [M.encode(M.pmul(rng.randrange(1, M.L), M.BASE)) for _ in range(20)]
    n_small = 0
    for e in encs:
        ok, by_dbl, by_y = H.small_order(e)
        assert ok == (M.decode(e) is not None)
        if ok:
            assert by_dbl == by_y == M.is_small(M.decode(e)), e.hex()
            n_small += by_y
    assert n_small >= 8


@pytest.mark.parametrize("bits", [20, 16])
def test_wide_comb_construction_vs_model(bits):
    """wcomb_bases + wcomb_fill (the device build of j * 2^(W i) * P, affine niels
    with one batched inversion per chunk) against the textbook model, for both
    comb widths the device builds (20-bit: B and committee keys that fit in HBM;
    16-bit: committee keys otherwise): first, second and last position, first,
    second and last chunk."""
    M = _model()
    with open(os.path.join(GOLD, "fixtures_reference.json")) as f:
        pk = bytes.fromhex(json.load(f)["keys"][1]["pk"])
    npos = (254 + bits - 1) // bits
    last_chunk = (1 << (bits - 1)) // 64 - 1
    cases = [(M.encode(M.BASE), 0, M.BASE), (pk, 1, M.pneg(M.decode(pk)))]
    for enc, neg, pt in cases:
        for pos in (0, 1, npos - 1):
            base = M.pmul(2 ** (bits * pos), pt)
            for c in (0, 1, last_chunk):
                meta, e = H.wcomb_chunk(bits, enc, neg, pos, c)
                assert meta == 1
                q = M.pmul(64 * c, base)
                for idx in range(65):
                    if idx or c == 0:
                        X, Y, Z, _ = q
                        zi = M.inv(Z)
                        x, y = X * zi % M.P, Y * zi % M.P
                        want = ((y + x) % M.P, (y - x) % M.P, 2 * M.D * x * y % M.P)
                        got = tuple(H.value(e[idx][10 * k:10 * k + 10]) % M.P for k in range(3))
                        assert got == want, (pos, c, idx)
                    q = M.padd(q, base)


def test_sign_fixture_through_device_code():
    with open(os.path.join(GOLD, "fixtures_reference.json")) as f:
        ref = json.load(f)
    d = bytes.fromhex(ref["hello_digest"])
    for k, s in zip(ref["keys"], ref["hello_signatures"]):
        pk, sig = H.sign(bytes.fromhex(k["seed"]), d)
        assert pk.hex() == k["pk"]
        assert sig.hex() == s


def _invert(limbs, vt):
    import ctypes
    lib = H.load()
    out = (ctypes.c_uint8 * 32)()
    lib.nth_fe_invert((ctypes.c_uint32 * 10)(*limbs), out, vt)
    return int.from_bytes(bytes(out), "little")


def test_fe_invert_vt_vs_fermat_and_bigint():
    """The key-cache kernel's variable-time inversion (fe_inv_vt.hpp: Pornin's
    optimized binary GCD, up to 17 x 30 steps on 62-bit approximations, leaving
    the loop once a = 0 -- on the host per value, so small inputs exercise the
    skipped iterations' direct factor 2^30) equals
    z^(p-2) mod p (Python big integers) on edge values and random inputs, and
    equals the Fermat chain (fe_invert) on 200k more inputs drawn in the C
    harness (half of them structured: small, p - small, powers of two, p + s
    as a non-canonical encoding)."""
    import ctypes
    P = H.P
    rng = random.Random(11)
    vals = [0, 1, 2, 3, 19, P - 1, P - 2, P + 1, P + 18, 2 ** 254, 2 ** 255 - 20, 2 ** 128, 2 ** 128 - 1,
            (P - 1) // 2, (P + 1) // 2, 2 ** 62, 2 ** 62 - 1, 2 ** 30, 2 ** 31 + 1]
    vals += [1 << k for k in range(255)]
    vals += [P - (1 << k) for k in range(1, 254)]
    vals += [rng.randrange(P) for _ in range(3000)]
    vals += [rng.randrange(1 << rng.randrange(1, 255)) for _ in range(1000)]
    for v in vals:
        limbs = H.to_limbs(v)
        want = pow(v % P, P - 2, P)
        assert _invert(limbs, 1) == want, hex(v)
    lib = H.load()
    lib.nth_fe_invert_cmp.restype = ctypes.c_ulonglong
    assert lib.nth_fe_invert_cmp(ctypes.c_ulonglong(200_000), ctypes.c_ulonglong(0x9E3779B97F4A7C15)) == 0


def test_opcount_matches_committed_profile():
    """profiles/opcount.json (roofline numerator) must match the current code."""
    path = os.path.join(os.path.dirname(GOLD), "..", "profiles", "opcount.json")
    if not os.path.exists(path):
        pytest.skip("profiles/opcount.json not generated yet (tools/opcount.py)")
    with open(path) as f:
        committed = json.load(f)
    import importlib.util
    spec = importlib.util.spec_from_file_location("opcount", os.path.join(os.path.dirname(GOLD), "..",
                                                                          "tools", "opcount.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cur = mod.measure()
    for key in ("verify_strict_fe_mul", "verify_strict_fe_sq", "verify_strict_mads"):
        assert cur[key] == committed[key], key


def test_device_probe_refuses_a_missing_or_stale_library(tmp_path):
    """the GPU tests never compile: a probe library that is missing or older than
    one of its sources raises (a failure, not a skip) and names the file"""
    import _devprobe
    lib, src = tmp_path / "libx.so", tmp_path / "x.hpp"
    src.write_text("")
    with pytest.raises(RuntimeError, match="missing"):
        _devprobe.check_fresh(str(lib), [str(src)])
    lib.write_text("")
    os.utime(src, (1000, 1000))
    os.utime(lib, (2000, 2000))
    _devprobe.check_fresh(str(lib), [str(src)])
    os.utime(src, (3000, 3000))
    with pytest.raises(RuntimeError, match="older than"):
        _devprobe.check_fresh(str(lib), [str(src)])
