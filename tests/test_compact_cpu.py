"""CPU-side checks of the compaction surface: the library exports the
auxiliary entry points and the kernel hook, and they refuse a NULL
engine without touching a device."""
import ctypes
import subprocess

import pytest

import __graft_entry__ as entry


@pytest.fixture(scope="module")
def libpath():
    entry.build()
    return entry.SO


def test_compact_exports(libpath):
    out = subprocess.check_output(["nm", "-D", libpath]).decode()
    syms = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in ("GammaCompact", "GammaCompactStats",
                 "GammaKTestBucketCompact"):
        assert name in syms, name


def test_compact_null_engine(libpath):
    L = ctypes.CDLL(libpath)
    i64p = ctypes.POINTER(ctypes.c_int64)
    L.GammaCompact.argtypes = [ctypes.c_void_p, ctypes.c_float, i64p]
    L.GammaCompactStats.argtypes = [ctypes.c_void_p, i64p]
    st = (ctypes.c_int64 * 3)(7, 7, 7)
    assert L.GammaCompact(None, 0.3, st) == -1
    assert L.GammaCompactStats(None, st) == -1
    assert list(st) == [7, 7, 7]
