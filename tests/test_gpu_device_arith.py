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
same checks on the host build.  Nothing is compiled here: a missing or stale
probe library fails at once.
"""
import glob
import os

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
