"""nt_msg_receipt at the C boundary (CPU only): the layout a C99 compiler gives
the struct in include/ntcrypto.h is 128 bytes and is, field by field, the
numpy dtype the Python binding reads it with; libntcrypto.so exports the call
that fills it."""
import os
import re
import subprocess

import ntcrypto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "narwhal-tusk_amd", "lib", "libntcrypto.so")
FIELDS = ("code", "kind", "flags", "author", "origin", "np", "nq", "nv", "round", "off_payload", "off_parents",
          "off_id", "off_sig", "off_votes", "id", "digest", "reserved")

PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "ntcrypto.h"
#define F(f) printf(#f " %lu %lu\n", (unsigned long)offsetof(nt_msg_receipt, f), \
                    (unsigned long)sizeof(((nt_msg_receipt *)0)->f))
int main(void) {
  printf("sizeof %lu %lu\n", (unsigned long)sizeof(nt_msg_receipt), (unsigned long)sizeof(nt_msg_receipt[3]));
  FIELDS
  return 0;
}
"""


def _layout(tmp_path, std):
    src = tmp_path / ("layout_%s.c" % std)
    src.write_text(PROGRAM.replace("FIELDS", " ".join("F(%s);" % f for f in FIELDS)))
    exe = tmp_path / ("layout_" + std)
    subprocess.run(["gcc", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, str(src), "-o",
                    str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in out.splitlines()}


def test_c_layout_is_the_dtype(tmp_path):
    dt = ntcrypto.RECEIPT_DTYPE
    assert dt.itemsize == 128 and dt.names == FIELDS
    for std in ("c99", "c11"):
        lay = _layout(tmp_path, std)
        assert lay.pop("sizeof") == (128, 3 * 128), std                      # no tail padding in an array either
        assert set(lay) == set(FIELDS)
        for f in FIELDS:
            assert lay[f] == (dt.fields[f][1], dt.fields[f][0].itemsize), (std, f, lay[f])
        # no implicit padding: the fields tile the 128 bytes
        spans = sorted(lay.values())
        assert spans[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(spans, spans[1:]))
        assert sum(n for _, n in spans) == 128
    assert all(dt.fields[f][0].byteorder in ("<", "=", "|") for f in FIELDS)


def test_header_pins_the_size_for_every_dialect():
    """a static assertion for C++, C11 and (as an array-size trick) C99"""
    src = open(os.path.join(INC, "ntcrypto.h")).read()
    assert re.search(r"static_assert\(sizeof\(nt_msg_receipt\) == 128", src)
    assert re.search(r"_Static_assert\(sizeof\(nt_msg_receipt\) == 128", src)
    assert re.search(r"\[sizeof\(nt_msg_receipt\) == 128 \? 1 : -1\]", src)


def test_library_exports_the_call():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT nt_primary_messages_ingest_receipts\b", out)
    assert "nt_primary_messages_ingest_receipts" in ntcrypto.EXPORTED
    lib = ntcrypto.load_library()
    assert lib.nt_primary_messages_ingest_receipts.argtypes is not None
