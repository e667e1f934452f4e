"""The edge-case checks of the Ed25519 arithmetic (tests/_arith_checks.py) on the
code the GPU executes: the gfx950 build of narwhal-tusk_amd/csrc/*.hpp behind the
device probe (tests/cpp/nt_device_probe.hip).  The other GPU tests only see a
signature's accept/reject bit, and every scalar they reach is a SHA-512 output;
here the device functions get the inputs that stress them directly -- limbs at
their bounds, chosen wave compositions for the wave-level exits (fe_invert_vt,
wave_max), scalars with huge partial quotients through the v_rcp_f64 Lehmer
quotient, messages at every byte alignment -- and, behind the key-table cache, the
unbalanced lattice vector with huge quotients at its own stop (2^191.5), the
product's DevKTab filled and read back point by point, and the three-table ladder
with chosen digits and window counts.  The wide combs behind every fixed-point
multiplication ([s]B, [k](-A)) are built here by the product's own wcomb_build at
all five digit widths and read back through WideComb::load entry by entry -- entry
2^(W-1), entry 0, the reduced comb's extra chunk and its [L](-A) entry, a short last
fill batch -- with the digit schedule and the sums at chosen scalars: a carry
through every position, a zero first digit from the identity, waves in which only
some lanes owe the reduced comb's correction.  The comb path of cached rows runs over
DevKTab with a comb pool: ktab_build_comb in chosen claim compositions, every comb
line, kc_recode / kc_pick, ladder_kc with lanes of mixed parity, entry and liveness,
compare_one and verify_kc at chosen (R, s, k).  tests/test_host_arith.py runs the
same checks on the host build.  The per-item entry points are one text for both
builds (tests/cpp/nt_probe_entries.inc); the last test here holds the device
runner's outputs to the host runner's, byte for byte, at one lane, a second wave
and a second block.  Nothing is compiled here: a missing or stale probe library
fails at once.
"""
import ctypes
import glob
import os
import random

import numpy as np
import pytest

import _arith_checks as C
import _devprobe
import _hostarith as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return _devprobe.runner()


@pytest.fixture(scope="module")
def host():
    """the host build as build() left it (the half-size reference and the ladder's vectors)"""
    lib = os.path.join(H.CPP, "build", "libnthost.so")
    srcs = [os.path.join(H.CPP, "nt_host_harness.cpp"), os.path.join(H.CPP, "nt_probe_items.hpp"),
            os.path.join(H.CPP, "nt_probe_entries.inc"),
            os.path.join(H.CPP, "ktab", "host_ktab.hpp"), os.path.join(H.CPP, "kcomb", "host_kcomb.hpp")] + \
        glob.glob(os.path.join(_devprobe.CSRC, "*.hpp"))
    _devprobe.check_fresh(lib, srcs)
    return H.runner("", build=False)


def test_fe_mul_at_bounds(dev):
    C.check_fe_mul_bounds(dev)


def test_fe_sq_at_bounds(dev):
    C.check_fe_sq_bounds(dev)


def test_fe_bytes(dev):
    C.check_fe_bytes(dev)


def test_inversion_wave_compositions(dev):
    C.check_inversion(dev)


def test_sc_reduce512(dev):
    C.check_sc_reduce512(dev)


def test_sc_muladd_mul_canonical(dev):
    C.check_sc_mul(dev)


def test_sc_reduce_half(dev):
    C.check_sc_reduce_half(dev)


def test_sc_recode_w4(dev):
    C.check_sc_recode_w4(dev)


def test_halfsize_on_device_reciprocal(dev, host):
    C.check_halfsize(dev, host.sc_halfsize(C.halfsize_scalars(), 0))


def test_hram_every_alignment(dev):
    C.check_hram(dev)


def test_point_decoding_and_small_order(dev):
    C.check_point_checks(dev)


def test_ladder_lane_mixed_window_counts(dev, host):
    C.check_ladder(dev, H.host_halfsize)


def test_unbalanced_on_device_reciprocal(dev, host):
    C.check_unbalanced(dev, host.sc_unbalanced(C.unbalanced_scalars(), 0))


def test_key_table_entries_and_cached_points(dev):
    C.check_ktab_tables(dev)


def test_three_table_ladder_lane_mixed_window_counts(dev, host):
    C.check_ladder3(dev, H.host_unbalanced, H.host_halfsize)


@pytest.mark.parametrize("bits", C.COMB_WIDTHS)
def test_wide_comb_tables(dev, bits):
    print("comb entries compared at %d bits: %d" % (bits, C.check_wcomb_tables(dev, bits)))


@pytest.mark.parametrize("bits", C.COMB_WIDTHS)
def test_wide_comb_digits(dev, bits):
    print("digit vectors compared at %d bits: %d" % (bits, C.check_wcomb_digits(dev, bits)))


@pytest.mark.parametrize("bits", C.COMB_WIDTHS)
def test_wide_comb_sums(dev, bits):
    print("comb sums compared at %d bits: %d" % (bits, C.check_wcomb_acc(dev, bits)))


def test_key_comb_sum_lane_mixed_corrections(dev):
    print("key comb sums compared per width: %d" % C.check_key_comb_sum(dev))


def test_wide_comb_entry_points_refuse_bad_arguments(dev):
    print("comb calls refused: %d" % C.check_wcomb_refusals(dev))


def test_key_comb_lines_and_claim_compositions(dev):
    print("comb lines compared: %d" % C.check_kcomb_tables(dev))


def test_comb_recoding_picks(dev):
    print("pick vectors compared: %d" % C.check_kc_picks(dev))


def test_comb_ladder_lane_mixed_parity_entry_and_dead(dev):
    print("comb ladder results compared: %d" % C.check_ladder_kc(dev))


def test_compare_one_chosen_points(dev):
    print("compare_one bits compared: %d" % C.check_compare_one(dev))


def test_verify_kc_chosen_scalars(dev):
    print("verify_kc verdicts compared: %d" % C.check_verify_kc(dev))


def test_comb_entry_points_refuse_bad_arguments(dev):
    print("comb-path calls refused: %d" % C.check_kcomb_refusals(dev))


# --------------------------------------------------------------------------
# The entry points both runners compile from tests/cpp/nt_probe_entries.inc: the device runner's
# outputs, byte for byte, against the host runner's for the same call.  (The host runner of each
# entry is pinned to the Python model by tests/test_host_arith.py.)
# --------------------------------------------------------------------------
PARITY_CAP = 4  # key-table capacity of the blob entries: the comb blob stays under 40 KB


def _cyc(xs, n, start=0):
    return [xs[(start + i) % len(xs)] for i in range(n)]


def _enc(es):
    return np.frombuffer(b"".join(es), np.uint32).copy()


def _out(dtype, words):
    return ("out", dtype, words)


def _parity_keys():
    """three keys that get an entry and one that never does"""
    return C._keys_of_kind("random", 4)


def _fill_keys(n):
    """Key lists of the fill calls, which run one after the other on one blob.  Which lane wins a
    key that several live lanes bring, and the order in which winners take pool entries, is the
    GPU's to choose; so each call brings exactly one new key, on its last item -- n = 1: the only
    lane; n = 65: the one live lane of the second wave, beside 63 tail lanes; n = 257: the one
    lane of the second block -- and every other item a key that is ready already."""
    k = _parity_keys()
    return {1: [k[0]], 65: [k[0]] * 64 + [k[1]], 257: _cyc(k[:2], 256) + [k[2]]}[n]


def _parity_calls(n, ktab, kcomb):
    """(entry, arguments after n, arguments before n) of every shared entry at n items: an argument
    is an input array, ("out", dtype, words per item), ("blob", table per runner) or a ctypes scalar.
    ktab, kcomb: per runner, the table its fill calls build and its readers and ladders run over."""
    rng = random.Random(9000 + n)
    W, u32, cap = C._words, (lambda xs: np.array(xs, np.uint32)), ctypes.c_uint32(PARITY_CAP)
    o8, o10, o1 = _out(np.uint32, 8), _out(np.uint32, 10), _out(np.uint32, 1)
    mul, sq = C._fe_mul_cases()[0], C._fe_sq_cases()
    f, g = C._limbs(_cyc([c[0] for c in mul], n)), C._limbs(_cyc([c[1] for c in mul], n))
    r256 = lambda: W([rng.getrandbits(256) for _ in range(n)])
    calls = [("fe_mul", [f, g, o10]),
             ("fe_sq", [C._limbs(_cyc(sq["fe_sq"][0], n)), o10]),
             ("fe_sq_wide", [C._limbs(_cyc(sq["fe_sq_wide"][0], n)), o10]),
             ("fe_carry", [g, o10]), ("fe_tobytes", [g, o8]), ("fe_frombytes", [r256(), o10]),
             ("sc_reduce512", [W([rng.getrandbits(512) for _ in range(n)], 64), o8]),
             ("sc_muladd", [r256(), r256(), r256(), o8]), ("sc_mul", [r256(), r256(), o8]),
             ("sc_reduce_half", [W([rng.randrange(C.L) for _ in range(n)]), o8, o1]),
             ("sc_recode_w4", [W([rng.getrandbits(253) for _ in range(n)]), o8]),
             ("sc_is_canonical", [W([C.L + rng.randrange(-2, 3) for _ in range(n)]), o1]),
             ("point_checks", [_enc(_cyc(C._point_cases()[0], n)), _out(np.uint32, 4)])]
    inv = C._limbs([C.to_limbs(v) for v in _cyc(C.inversion_inputs()[0], n, 128)])  # a value beside zeros, then ones
    ks = W(_cyc(C.halfsize_scalars(), n, 190))
    lens = [C.HRAM_LENS[i % 17] for i in range(n)]
    offs = [sum(lens[:i]) + 8 * i + i % 8 for i in range(n)]
    buf = bytes(rng.getrandbits(8) for _ in range(offs[-1] + lens[-1]))
    msg = np.frombuffer(buf + b"\0", np.uint8).copy()
    R, A = r256(), r256()
    for sw in (ctypes.c_int(1), ctypes.c_int(0)):
        i1 = _out(np.int32, 1)
        calls += [("fe_invert", [inv, o8, sw]), ("sc_halfsize", [ks, o8, o1, o8, i1, sw]),
                  ("sc_unbalanced", [ks, o8, o1, o8, i1, i1, sw]),
                  ("hram", [R, A, msg, ctypes.c_uint64(len(buf)), np.array(offs, np.uint64), np.array(lens, np.uint64), o8, sw])]
    for bits in C.COMB_WIDTHS:
        calls.append(("wcomb_digits", [W(_cyc(C.comb_digit_inputs(bits)[0], n)), _out(np.uint32, 64)], [ctypes.c_int(bits)]))
    As, Rs, uvb, _ = C.ladder_cases(H.host_halfsize)
    uvb = _cyc(uvb, n)
    calls.append(("ladder_uv", [_enc(_cyc(As, n)), _enc(_cyc(Rs, n)), W([abs(x[0]) for x in uvb]), u32([x[0] < 0 for x in uvb]),
                                W([x[1] for x in uvb]), np.array([x[2] for x in uvb], np.int32), o8]))
    # the tables: the fills (ktab, kcomb: what the earlier fills of this runner left), then the readers
    keys = _enc(_cyc(_parity_keys(), n))
    kidx = u32([i % 3 for i in range(n)])
    calls += [("ktab_fill", [_enc(_fill_keys(n)), ("blob", ktab), cap, o1]),
              ("kcomb_fill", [_enc(_fill_keys(n)), ("blob", kcomb), cap, o1])]
    td = np.array([(i % 3, i % 17 - 8) for i in range(n)], np.int32)
    _, Rs3, vecs, _ = C.ladder3_cases(H.host_unbalanced, H.host_halfsize)
    vecs = _cyc(vecs, n)
    sc4 = u32([[x[0] < 0, x[2], x[3], x[4]] for x in vecs])
    calls += [("ktab_point", [keys, td, ("blob", ktab), cap, _out(np.uint32, 3), o8]),
              ("ladder_uv3", [kidx, _enc(_cyc(Rs3, n)), W([abs(x[0]) for x in vecs]), W([x[1] for x in vecs]), sc4,
                              ("blob", ktab), cap, o8]),
              ("kcomb_line", [keys, u32([i % 36 for i in range(n)]), ("blob", kcomb), cap, _out(np.uint32, 3), _out(np.uint32, 30)]),
              ("kc_picks", [W(_cyc(C.kc_pick_scalars(), n)), _out(np.uint32, 65)])]
    _, kk, dead, _ = C.ladder_kc_cases()
    calls.append(("ladder_kc", [kidx, W(_cyc(kk, n)), u32(_cyc(dead, n)), ("blob", kcomb), cap, o8]))
    cmp1 = _cyc(C.compare_one_cases(), n)
    calls.append(("compare_one", [W([c[0] % C.P for c in cmp1]), W([c[1] % C.P for c in cmp1]), W([c[2] % C.P for c in cmp1]),
                                  _enc([c[3] for c in cmp1]), u32([c[4] for c in cmp1]), o1]))
    vk = _cyc(C.verify_kc_cases(), n)
    calls.append(("verify_kc", [kidx, u32([c[1] or 0 for c in vk]), _enc([c[2] for c in vk]), W([c[3] for c in vk]),
                                W([c[4] for c in vk]), u32([i // len(C.verify_kc_cases()) % 2 for i in range(n)]),
                                ("blob", kcomb), cap, o1]))
    return calls


def _parity_run(run, n, entry, args, head=()):
    """one call on `run`: its output arrays, and each blob as the call left it (kept for the next call)"""
    outs, ptrs = [], []
    for a in args:
        if isinstance(a, tuple) and a[0] == "out":
            a = np.full((n, a[2]), 0xC3C3C3C3, np.uint32).view(a[1])
            outs.append(a)
        elif isinstance(a, tuple):
            a = a[1][run.name]
            outs.append(a)
        ptrs.append(C._p(a) if isinstance(a, np.ndarray) else a)
    run._raw(entry, *head, ctypes.c_uint64(n), *ptrs)
    return outs


PARITY_NS = (1, 65, 257)


def _parity_kcomb_blob():
    """an empty comb table whose entry headers start as zeros: DevKTab's hdr_store writes the whole
    128-byte header line (zeros behind tag and flags), the host policy tag and flags alone, and
    from zeros the two leave the same bytes"""
    blob = C.kcomb_blob(PARITY_CAP)
    pool = blob[C.KT_POOL_OFF:C.kcomb_comb_off(PARITY_CAP)].reshape(PARITY_CAP, C.KT_ENTRY_BYTES)
    pool[:, :C.KT_HEADER_BYTES] = 0
    return blob


def _parity_fill(dev, host):
    tabs = {"ktab": {r.name: C.ktab_blob(PARITY_CAP) for r in (dev, host)},
            "kcomb": {r.name: _parity_kcomb_blob() for r in (dev, host)}, "fills": {}}
    for n in PARITY_NS:
        for entry, args, *_ in _parity_calls(n, tabs["ktab"], tabs["kcomb"]):
            if entry.endswith("_fill"):
                tabs["fills"][entry, n] = [[a.copy() for a in _parity_run(r, n, entry, args)] for r in (dev, host)]
    return tabs


@pytest.fixture(scope="module")
def parity_tables(dev, host):
    """per runner: an empty table of each kind, filled by the fill calls of n = 1, 65 and 257 in
    this order; what each fill returned is kept for the test of its n"""
    return _parity_fill(dev, host)


@pytest.mark.parametrize("n", PARITY_NS)
def test_shared_entries_device_equals_host(dev, host, parity_tables, n):
    """Every entry of nt_probe_entries.inc at n = 1 (one live lane), n = 65 (a second wave of one
    live lane and 63 tail lanes) and n = 257 (a second block: blockIdx.x picks a second WsATab
    slice): the device runner's outputs and blobs equal the host runner's byte for byte.  Blob
    entries run at capacity 4 over three keys; verify_kc over the 16-bit comb of B alone."""
    M = C.model()
    seen = set()

    def same(entry, d, h):
        for j, (x, y) in enumerate(zip(d, h)):
            diff = np.flatnonzero(x.view(np.uint8).ravel() != y.view(np.uint8).ravel())
            assert diff.size == 0, (entry, n, "output", j, "bytes that differ", diff.size, diff[:8], diff[-8:])
        seen.add(entry)

    try:
        for r in (dev, host):
            r.wcomb_build(16, (M.encode(M.BASE),), 0, 1)
        for entry, args, *head in _parity_calls(n, parity_tables["ktab"], parity_tables["kcomb"]):
            if entry.endswith("_fill"):
                same(entry, *parity_tables["fills"][entry, n])
            else:
                same(entry, *(_parity_run(r, n, entry, args, *head) for r in (dev, host)))
    finally:
        for r in (dev, host):
            r.wcomb_free()
    assert seen == set(C.ENTRIES) - {"wcomb_build", "wcomb_free", "wcomb_guard", "wcomb_entries", "wcomb_acc", "key_comb_sum"}
    used = int(parity_tables["ktab"][dev.name][:4].view(np.uint32)[0])
    assert used == int(parity_tables["kcomb"][dev.name][:4].view(np.uint32)[0]) == 3, "one entry per fill call"
