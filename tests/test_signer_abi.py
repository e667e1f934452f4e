"""include/ntsigner.h at the C boundary (CPU only): the header compiles as C99, C11
and C++17 under -Wall -Wextra -Werror -pedantic; every nts_* call it declares is
exported by libntcrypto.so and bound by the Python package; the nt_* export set is
what it was before the signer."""
import os
import re
import subprocess

import pytest

import ntcrypto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "narwhal-tusk_amd", "lib", "libntcrypto.so")
ARGS = {"nts_signer_create": 3, "nts_signer_free": 1, "nts_signer_public": 2, "nts_sign_digests": 5,
        "nts_votes_sign": 8, "nts_dev_votes_sign": 10}

PROGRAM = r"""
#include <stdio.h>
#include "ntsigner.h"
int main(void) {
  /* every declaration is usable: take each call's address through its own type */
  int (*create)(nt_ctx *, const uint8_t *, nts_signer **) = nts_signer_create;
  void (*destroy)(nts_signer *) = nts_signer_free;
  int (*pub)(const nts_signer *, uint8_t *) = nts_signer_public;
  int (*digests)(nt_ctx *, const nts_signer *, const uint8_t *, uint64_t, uint8_t *) = nts_sign_digests;
  int (*votes)(nt_ctx *, const nts_signer *, const uint8_t *, const uint64_t *, const uint8_t *, uint64_t, uint8_t *,
               uint8_t *) = nts_votes_sign;
  int (*dev)(nt_ctx *, const nts_signer *, int, void *, const uint8_t *, const uint64_t *, const uint8_t *, uint64_t,
             uint8_t *, uint8_t *) = nts_dev_votes_sign;
  nts_signer *s = 0;
  uint8_t pk[32];
  /* no context: the calls refuse without touching a device */
  printf("%d %d %d %d %d\n", NTS_VOTE_BYTES, create(0, pk, &s), pub(0, pk), digests(0, 0, 0, 0, 0),
         votes(0, 0, 0, 0, 0, 0, 0, 0) + dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0));
  destroy(0);
  return s != 0;
}
"""


@pytest.mark.parametrize("compiler,std,suffix", [("gcc", "c99", "c"), ("gcc", "c11", "c"), ("g++", "c++17", "cpp")])
def test_header_compiles_and_links(tmp_path, compiler, std, suffix):
    src = tmp_path / ("signer_abi." + suffix)
    src.write_text(PROGRAM)
    exe = tmp_path / "signer_abi"
    r = subprocess.run([compiler, "-std=" + std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, str(src), "-o",
                        str(exe), "-L", os.path.dirname(LIB), "-lntcrypto", "-Wl,-rpath," + os.path.dirname(LIB)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["212", "-1", "-1", "-1", "-2"], (out.stdout, out.stderr)


def test_declared_calls_are_exported_and_bound():
    src = open(os.path.join(INC, "ntsigner.h")).read()
    assert '#include "ntcrypto.h"' in src and re.search(r"not constant time", src, re.I)
    declared = set(re.findall(r"\b(nts_[a-z0-9_]+)\s*\(", src))
    assert declared == set(ARGS)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (nts_[a-z0-9_]+)", out)) == declared
    assert set(ntcrypto.SIGNER_EXPORTED) == declared
    lib = ntcrypto.load_library()
    for name, nargs in ARGS.items():
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert ntcrypto.VOTE_BYTES == 212 and re.search(r"#define NTS_VOTE_BYTES 212\b", src)


def test_nt_export_set_is_unchanged():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (nt_[a-z0-9_]+)", out)) == set(ntcrypto.EXPORTED)
    assert not [s for s in ntcrypto.EXPORTED if s.startswith("nts_")]
    assert "nts_" not in open(os.path.join(INC, "ntcrypto.h")).read()        # the signer lives in its own header
