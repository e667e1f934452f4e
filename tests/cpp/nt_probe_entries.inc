// nt_probe_entries.inc -- TEST INFRASTRUCTURE: the per-item entry points of the arithmetic
// probe, written once and compiled twice: nt_device_probe.hip includes this file with
// NTP_NAME(x) = ntp_x and runs item i on GPU thread i, nt_host_harness.cpp with NTP_NAME(x) =
// nthb_x and runs the items in a loop.  An entry is the argument check, on the host before
// anything is allocated or run (a refused call returns 1 = hipErrorInvalidValue), then one
// run<Tail>(n, item, arguments in the item's order); the vocabulary of the arguments is at the
// end of nt_probe_items.hpp.  Besides NTP_NAME and run, the includer provides live_bcomb_ok() /
// live_bcomb(): key 0 of its live comb set as verify_kc's comb of B.
// A new item: its function in nt_probe_items.hpp, its entry here, its name in
// tests/_arith_checks.py ENTRIES.
// The one forwarding wrapper around the overloaded or templated ntp::item_<name>.  Forced inline
// as the items are: left to the inliner's choice, the gfx950 kernels of ladder_uv and kcomb_fill
// spill to scratch, which no kernel of the product's functions does.
#define NTP_ITEM(name) [] NT_HD(auto&&... a) __attribute__((always_inline)) { ntp::item_##name(a...); }

extern "C" {

int NTP_NAME(fe_mul)(uint64_t n, const uint32_t* f, const uint32_t* g, uint32_t* out) {
  return run<Leave>(n, NTP_ITEM(fe_mul), in(f, 40), in(g, 40), out_(out, 40));
}
int NTP_NAME(fe_sq)(uint64_t n, const uint32_t* f, uint32_t* out) {
  return run<Leave>(n, NTP_ITEM(fe_sq), in(f, 40), out_(out, 40));
}
int NTP_NAME(fe_sq_wide)(uint64_t n, const uint32_t* f, uint32_t* out) {
  return run<Leave>(n, NTP_ITEM(fe_sq_wide), in(f, 40), out_(out, 40));
}
int NTP_NAME(fe_carry)(uint64_t n, const uint32_t* f, uint32_t* out) {
  return run<Leave>(n, NTP_ITEM(fe_carry), in(f, 40), out_(out, 40));
}
int NTP_NAME(fe_tobytes)(uint64_t n, const uint32_t* f, uint32_t* out8) {
  return run<Leave>(n, NTP_ITEM(fe_tobytes), in(f, 40), out_(out8, 32));
}
int NTP_NAME(fe_frombytes)(uint64_t n, const uint32_t* in8, uint32_t* out) {
  return run<Leave>(n, NTP_ITEM(fe_frombytes), in(in8, 32), out_(out, 40));
}
// vt: fe_invert_vt, whose wave-level exit sees exactly the lanes the caller filled
int NTP_NAME(fe_invert)(uint64_t n, const uint32_t* f, uint32_t* out8, int vt) {
  return flag(vt, [&](auto c) { return run<Leave>(n, NTP_ITEM(fe_invert), in(f, 40), out_(out8, 32), c); });
}
int NTP_NAME(sc_reduce512)(uint64_t n, const uint32_t* in16, uint32_t* out8) {
  return run<Leave>(n, NTP_ITEM(sc_reduce512), in(in16, 64), out_(out8, 32));
}
int NTP_NAME(sc_muladd)(uint64_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out8) {
  return run<Leave>(n, NTP_ITEM(sc_muladd), in(a, 32), in(b, 32), in(c, 32), out_(out8, 32));
}
int NTP_NAME(sc_mul)(uint64_t n, const uint32_t* a, const uint32_t* b, uint32_t* out8) {
  return run<Leave>(n, NTP_ITEM(sc_mul), in(a, 32), in(b, 32), out_(out8, 32));
}
int NTP_NAME(sc_reduce_half)(uint64_t n, const uint32_t* k8, uint32_t* out8, uint32_t* neg) {
  return run<Leave>(n, NTP_ITEM(sc_reduce_half), in(k8, 32), out_(out8, 32), out_(neg, 4));
}
int NTP_NAME(sc_recode_w4)(uint64_t n, const uint32_t* s8, uint32_t* out8) {
  return run<Leave>(n, NTP_ITEM(sc_recode_w4), in(s8, 32), out_(out8, 32));
}
int NTP_NAME(sc_is_canonical)(uint64_t n, const uint32_t* s8, uint32_t* out1) {
  return run<Leave>(n, NTP_ITEM(sc_is_canonical), in(s8, 32), out_(out1, 4));
}
// lehmer 1: sc_halfsize_t<true> (the kernels'), 0: sc_halfsize_t<false> = sc_halfsize_euclid
int NTP_NAME(sc_halfsize)(uint64_t n, const uint32_t* k8, uint32_t* u8, uint32_t* uneg, uint32_t* v8, int32_t* bits,
                          int lehmer) {
  return flag(lehmer, [&](auto c) {
    return run<Leave>(n, NTP_ITEM(sc_halfsize), in(k8, 32), out_(u8, 32), out_(uneg, 4), out_(v8, 32), out_(bits, 4), c);
  });
}
// msg: one buffer of msg_bytes bytes; byte offset off[i] into the runner's aligned copy fixes
// message i's alignment, and every off[i] + len[i] <= msg_bytes is checked here
int NTP_NAME(hram)(uint64_t n, const uint32_t* R8, const uint32_t* A8, const uint8_t* msg, uint64_t msg_bytes,
                   const uint64_t* off, const uint64_t* len, uint32_t* out8, int fast) {
  for (uint64_t i = 0; i < n; ++i)
    if (!msg_slice(off[i], len[i], msg_bytes).ok) return 1;
  return flag(fast, [&](auto c) {
    return run<Leave>(n, NTP_ITEM(hram), in(R8, 32), in(A8, 32), Msg{msg, msg_bytes}, in(off, 8), in(len, 8), out_(out8, 32), c);
  });
}
int NTP_NAME(point_checks)(uint64_t n, const uint32_t* enc8, uint32_t* out4) {
  return run<Leave>(n, NTP_ITEM(point_checks), in(enc8, 32), out_(out4, 16));
}
// Repeat: wave_max shuffles across all 64 lanes of a wave, so every lane of a launched wave
// stays active (on the host wave_max is the identity: each item runs its own window count)
int NTP_NAME(ladder_uv)(uint64_t n, const uint32_t* A8, const uint32_t* R8, const uint32_t* u8, const uint32_t* uneg,
                        const uint32_t* v8, const int32_t* bits, uint32_t* out8) {
  for (uint64_t i = 0; i < n; ++i)  // 4 W <= 256 digits of the recoded strings
    if (bits[i] < 0 || bits[i] > 253) return 1;
  return run<Repeat>(n, NTP_ITEM(ladder_uv), in(A8, 32), in(R8, 32), in(u8, 32), in(uneg, 4), in(v8, 32), in(bits, 4), Ws{},
                     out_(out8, 32));
}
// lehmer 1: sc_unbalanced_t<true> (verify_one_kt's), 0: the one-step loop
int NTP_NAME(sc_unbalanced)(uint64_t n, const uint32_t* k8, uint32_t* u8, uint32_t* uneg, uint32_t* v8, int32_t* ubits,
                            int32_t* vbits, int lehmer) {
  return flag(lehmer, [&](auto c) {
    return run<Leave>(n, NTP_ITEM(sc_unbalanced), in(k8, 32), out_(u8, 32), out_(uneg, 4), out_(v8, 32), out_(ubits, 4),
                      out_(vbits, 4), c);
  });
}

// ---- the key-table cache's three-table items.  blob: ktab_probe_bytes(capacity) bytes laid
// out as DevKTab reads them (control block, kKtProbeSlots index slots, `capacity` pool
// entries), words 8..9 of the control block zero.  ktab_build is wave-uniform, as in verify_n:
// lanes past n run it on the last key with no claim (they neither probe nor store).
int NTP_NAME(ktab_fill)(uint64_t n, const uint32_t* A8, uint8_t* blob, uint32_t capacity, uint32_t* slot) {
  if (!kcomb_cap_ok(capacity)) return 1;
  return run<Repeat>(n, NTP_ITEM(ktab_fill), in(A8, 32), Blob<false>{blob, capacity}, out_(slot, 4));
}
int NTP_NAME(ktab_point)(uint64_t n, const uint32_t* A8, const int32_t* td2, uint8_t* blob, uint32_t capacity,
                         uint32_t* out3, uint32_t* enc8) {
  if (!kcomb_cap_ok(capacity) || !ktab_point_args_ok(n, td2)) return 1;
  return run<Leave>(n, NTP_ITEM(ktab_point), in(A8, 32), in(td2, 8), Blob<false>{blob, capacity}, out_(out3, 12),
                    out_(enc8, 32));
}
int NTP_NAME(ladder_uv3)(uint64_t n, const uint32_t* kidx, const uint32_t* R8, const uint32_t* u8, const uint32_t* v8,
                         const uint32_t* sc4, uint8_t* blob, uint32_t capacity, uint32_t* out8) {
  if (!kcomb_cap_ok(capacity) || !ladder_uv3_args_ok(n, kidx, sc4, capacity)) return 1;
  return run<Repeat>(n, NTP_ITEM(ladder_uv3), in(kidx, 4), in(R8, 32), in(u8, 32), in(v8, 32), in(sc4, 16), Ws{},
                     Blob<false>{blob, capacity}, out_(out8, 32));
}

// needs no table (the loads go to a recording comb): any 256-bit x, at any of the five widths
int NTP_NAME(wcomb_digits)(int bits, uint64_t n, const uint32_t* x8, uint32_t* out) {
  int rc = 1;
  wcomb_width(bits, [&](auto w) {
    rc = run<Leave>(n, NTP_ITEM(wcomb_digits), in(x8, 32), out_(out, 4 * kWcDigitWords), w);
  });
  return rc;
}

// ---- the key-table cache's comb path.  blob: kcomb_probe_bytes(capacity) bytes -- control
// block, index, pool entries, comb pool (its address in words 8..9 of the control block while the
// items run, so has_comb() holds as in the product), guard -- prefilled by the caller; entry
// indices, scalars (k < 2^253) and modes are checked here.  The build is wave-uniform: lanes
// past n run it on the last key with no claim.
int NTP_NAME(kcomb_fill)(uint64_t n, const uint32_t* A8, uint8_t* blob, uint32_t capacity, uint32_t* slot) {
  if (!kcomb_cap_ok(capacity)) return 1;
  return run<Repeat>(n, NTP_ITEM(kcomb_fill), in(A8, 32), Blob<true>{blob, capacity}, Ws{}, out_(slot, 4));
}
// line[i]: any number (comb_line clamps it to the last line)
int NTP_NAME(kcomb_line)(uint64_t n, const uint32_t* A8, const uint32_t* line, uint8_t* blob, uint32_t capacity,
                         uint32_t* out3, uint32_t* limbs30) {
  if (!kcomb_cap_ok(capacity)) return 1;
  return run<Leave>(n, NTP_ITEM(kcomb_line), in(A8, 32), in(line, 4), Blob<true>{blob, capacity}, out_(out3, 12),
                    out_(limbs30, 120));
}
int NTP_NAME(kc_picks)(uint64_t n, const uint32_t* k8, uint32_t* out65) {
  if (!kc_scalars_ok(n, k8)) return 1;
  return run<Leave>(n, NTP_ITEM(kc_picks), in(k8, 32), NoTable{}, out_(out65, 4 * kKcPickWords));
}
int NTP_NAME(ladder_kc)(uint64_t n, const uint32_t* kidx, const uint32_t* k8, const uint32_t* dead, uint8_t* blob,
                        uint32_t capacity, uint32_t* out8) {
  if (!kcomb_cap_ok(capacity) || !ladder_kc_args_ok(n, kidx, k8, dead, capacity)) return 1;
  return run<Repeat>(n, NTP_ITEM(ladder_kc), in(kidx, 4), in(k8, 32), in(dead, 4), Blob<true>{blob, capacity},
                     out_(out8, 32));
}
// Leave: fe_invert_vt's wave-level exit sees the lanes the caller filled
int NTP_NAME(compare_one)(uint64_t n, const uint32_t* x8, const uint32_t* y8, const uint32_t* z8, const uint32_t* R8,
                          const uint32_t* mode, uint32_t* out1) {
  if (!modes_ok(n, mode)) return 1;
  return run<Leave>(n, NTP_ITEM(compare_one), in(x8, 32), in(y8, 32), in(z8, 32), in(R8, 32), in(mode, 4), out_(out1, 4));
}
// the comb of B: key 0 of the live comb set, which must be the narrowest width (wcomb_build of
// B alone, not negated); any 256-bit s stays inside that table
int NTP_NAME(verify_kc)(uint64_t n, const uint32_t* kidx, const uint32_t* kflags, const uint32_t* R8, const uint32_t* S8,
                        const uint32_t* k8, const uint32_t* mode, uint8_t* blob, uint32_t capacity, uint32_t* out1) {
  if (!live_bcomb_ok() || !kcomb_cap_ok(capacity) || !verify_kc_args_ok(n, kidx, kflags, k8, mode, capacity))
    return 1;
  for (uint64_t i = 0; i < n; ++i)
    if (!wcomb_scalar_ok<kKeyCombNarrow>(S8 + 8 * i)) return 1;
  return run<Repeat>(n, NTP_ITEM(verify_kc), in(kidx, 4), in(kflags, 4), in(R8, 32), in(S8, 32), in(k8, 32), in(mode, 4),
                     live_bcomb(), Blob<true>{blob, capacity}, out_(out1, 4));
}

}  // extern "C"
#undef NTP_ITEM
