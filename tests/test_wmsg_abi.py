"""nt_worker_receipt and nt_worker_messages_ingest at the C boundary (CPU only):
the layout a C99 and a C++17 compiler give the struct in include/ntcrypto.h is
64 bytes and is, field by field, the numpy dtype the Python binding reads it
with and the struct the model packs; libntcrypto.so exports the call, and every
export it had before is still there."""
import os
import re
import subprocess

import _wmsg as M
import ntcrypto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "narwhal-tusk_amd", "lib", "libntcrypto.so")
FIELDS = ("code", "kind", "flags", "n", "used", "tx_bytes", "tx_len", "off_key", "digest")
OFFSETS = {"code": (0, 1), "kind": (1, 1), "flags": (2, 2), "n": (4, 4), "used": (8, 8), "tx_bytes": (16, 8),
           "tx_len": (24, 4), "off_key": (28, 4), "digest": (32, 32)}
# the exports of the library before this call was added (include/ntcrypto.h)
BEFORE = """nt_init nt_init_device nt_init_devices nt_free nt_num_devices nt_strerror nt_version nt_sha512_trunc32
nt_ed25519_verify_strict nt_ed25519_verify_batch_groups nt_ed25519_sign_batch nt_ed25519_keypair_batch
nt_dev_sha512_trunc32 nt_dev_sha512_trunc32_bounded nt_dev_ed25519_verify nt_dev_group_and nt_dev_ed25519_sign
nt_keyset_create nt_keyset_free nt_keyset_flags nt_keyset_info nt_ed25519_verify_keyset
nt_ed25519_verify_batch_groups_keyset nt_dev_ed25519_verify_keyset nt_host_alloc nt_host_free nt_set_small_call_path
nt_call_counts nt_committee_create nt_committee_free nt_certificates_ingest nt_small_call_model nt_set_hbm_budget
nt_memory_info nt_dev_stream nt_set_key_cache nt_key_cache_add nt_key_cache_sync nt_key_cache_info nt_dev_clock_probe
nt_dev_ed25519_verify_keyset_groups nt_primary_messages_ingest nt_primary_messages_ingest_receipts""".split()

PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "ntcrypto.h"
#define F(f) printf(#f " %lu %lu\n", (unsigned long)offsetof(nt_worker_receipt, f), \
                    (unsigned long)sizeof(((nt_worker_receipt *)0)->f))
int main(void) {
  printf("sizeof %lu %lu\n", (unsigned long)sizeof(nt_worker_receipt), (unsigned long)sizeof(nt_worker_receipt[3]));
  printf("codes %d %d\n", NT_WMSG_SERIALIZATION, NT_WMSG_HOST);
  FIELDS
  return 0;
}
"""


def _layout(tmp_path, compiler, std, suffix):
    src = tmp_path / ("wlayout_%s.%s" % (std.replace("+", "x"), suffix))
    src.write_text(PROGRAM.replace("FIELDS", " ".join("F(%s);" % f for f in FIELDS)))
    exe = tmp_path / ("wlayout_" + std.replace("+", "x"))
    subprocess.run([compiler, "-std=" + std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, str(src), "-o",
                    str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in out.splitlines()}


def test_c_layout_is_the_dtype(tmp_path):
    dt = ntcrypto.WORKER_RECEIPT_DTYPE
    assert dt.itemsize == 64 and dt.names == FIELDS == M.FIELDS and M.RECEIPT.size == 64
    for compiler, std, suffix in (("gcc", "c99", "c"), ("g++", "c++17", "cpp")):
        lay = _layout(tmp_path, compiler, std, suffix)
        assert lay.pop("sizeof") == (64, 3 * 64), std                        # no tail padding in an array either
        assert lay.pop("codes") == (9, 255)
        assert lay == OFFSETS, (std, lay)
        for f in FIELDS:
            assert lay[f] == (dt.fields[f][1], dt.fields[f][0].itemsize), (std, f, lay[f])
        spans = sorted(lay.values())                                         # the fields tile the 64 bytes
        assert spans[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(spans, spans[1:]))
        assert sum(n for _, n in spans) == 64
    # the model's struct reads the same bytes
    rec = M.RECEIPT.pack(9, 255, 0x0102, 0x03040506, 7 << 40, 8 << 41, 9, 10, bytes(range(32)))
    import numpy as np
    a = np.frombuffer(rec, dt)[0]
    assert [int(a[f]) for f in FIELDS[:8]] == [9, 255, 0x0102, 0x03040506, 7 << 40, 8 << 41, 9, 10]
    assert bytes(a["digest"]) == bytes(range(32))
    assert (ntcrypto.WMSG_OK, ntcrypto.WMSG_SERIALIZATION, ntcrypto.WMSG_HOST) == (M.OK, M.SERIALIZATION, M.HOST)


def test_header_pins_the_size_for_every_dialect():
    src = open(os.path.join(INC, "ntcrypto.h")).read()
    assert re.search(r"static_assert\(sizeof\(nt_worker_receipt\) == 64", src)
    assert re.search(r"_Static_assert\(sizeof\(nt_worker_receipt\) == 64", src)
    assert re.search(r"\[sizeof\(nt_worker_receipt\) == 64 \? 1 : -1\]", src)
    assert re.search(r"#define NT_WMSG_SERIALIZATION 9\b", src)               # SerializationError among NT_DAG_*


def test_library_exports_the_call_and_every_earlier_one():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (nt_[a-z0-9_]+)", out))
    assert "nt_worker_messages_ingest" in exported
    assert not [s for s in BEFORE if s not in exported]
    assert exported - set(BEFORE) == {"nt_worker_messages_ingest"}
    assert "nt_worker_messages_ingest" in ntcrypto.EXPORTED and set(BEFORE) <= set(ntcrypto.EXPORTED)
    lib = ntcrypto.load_library()
    assert lib.nt_worker_messages_ingest.argtypes is not None and len(lib.nt_worker_messages_ingest.argtypes) == 7
