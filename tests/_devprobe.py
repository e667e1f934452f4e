"""ctypes binding of tests/cpp/build/libntprobe.so -- the device functions of
narwhal-tusk_amd/csrc/*.hpp behind gfx950 kernels (TEST INFRASTRUCTURE; see
tests/cpp/nt_device_probe.hip and the entry points of tests/cpp/nt_probe_entries.inc).  build() compiles the library; a GPU test run
never does: a missing or stale library fails the test at once."""
import ctypes
import glob
import os

import _arith_checks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "narwhal-tusk_amd", "csrc")
LIB = os.path.join(CPP, "build", "libntprobe.so")
EXPORTS = ["ntp_" + e for e in _arith_checks.ENTRIES]

_lib = None


def sources():
    return [os.path.join(CPP, f) for f in ("nt_device_probe.hip", "nt_probe_items.hpp", "nt_probe_entries.inc")] + \
        sorted(glob.glob(os.path.join(CSRC, "*.hpp")))


def check_fresh(lib=LIB, srcs=None):
    """raise unless `lib` exists and is no older than each of its sources"""
    if not os.path.exists(lib):
        raise RuntimeError("%s is missing: run build() (make -C tests/cpp) before the GPU tests; "
                           "they never compile" % os.path.relpath(lib, ROOT))
    t = os.path.getmtime(lib)
    stale = [os.path.relpath(s, ROOT) for s in (srcs or sources()) if os.path.getmtime(s) > t]
    if stale:
        raise RuntimeError("%s is older than %s: run build() (make -C tests/cpp) before the GPU tests; "
                           "they never compile" % (os.path.relpath(lib, ROOT), ", ".join(stale)))


def load():
    global _lib
    if _lib is None:
        check_fresh()
        _lib = ctypes.CDLL(LIB)
    return _lib


def runner():
    """the probe's entry points (ntp_*) as an _arith_checks.Runner"""
    return _arith_checks.Runner(load(), "ntp_", "gfx950")
