"""Builds and loads tests/ratecoeff_cpu_ref.cpp -- TEST INFRASTRUCTURE of test_ratecoeff.py and test_gpu_ratecoeff.py.

The CPU yardsticks of the rate-coefficient lookup tables: the oracle's qag restatement on the four integrands, and a
dense Gauss-Legendre quadrature that knows the integrands' kinks.  Results are computed once per (atom, epsrel) and
shared; callers must not write to them.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from artis_amd import ffi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spontrecombcoeff", "corrphotoioncoeff", "bfheating_coeff", "bfcooling_coeff")
THREADS = 16
_lib = None
_cache = {}


def load(builddir):
    """g++-build the helper into builddir (once per session) and return the ctypes library."""
    global _lib
    if _lib is None:
        so = os.path.join(str(builddir), "libratecoeff_cpu_ref.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-fPIC", "-shared",
                        "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tests", "ratecoeff_cpu_ref.cpp"),
                        "-o", so], check=True, timeout=600)
        L = C.CDLL(so)
        L.ratecoeff_cpu_qag.argtypes = [C.c_void_p, C.c_double] + [C.c_void_p] * 6 + [C.c_int]
        L.ratecoeff_cpu_dense.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int]
        _lib = L
    return _lib


class Ref:
    def __init__(self, ts, nbf, diagnostics):
        for n in NAMES:
            setattr(self, n, np.zeros((ts, nbf)))
        self.status = np.zeros((4, ts, nbf), np.uint8) if diagnostics else None
        self.intervals = np.zeros((4, ts, nbf), np.int32) if diagnostics else None

    def tables(self):
        return [getattr(self, n) for n in NAMES]

    def freeze(self):
        for a in self.tables() + [x for x in (self.status, self.intervals) if x is not None]:
            a.setflags(write=False)
        return self


def _shape(model):
    h = ffi.AtomicTables.from_address(model.atomic)
    return int(h.tablesize), int(h.nbfcontinua)


def qag(lib, model, epsrel):
    """The four tables through the oracle's gsl_qag61 at epsrel, with status and interval count per integral."""
    key = (model.atomic, "qag", float(epsrel))
    if key not in _cache:
        r = Ref(*_shape(model), True)
        rc = lib.ratecoeff_cpu_qag(model.atomic, float(epsrel), *[a.ctypes.data for a in r.tables()],
                                   r.status.ctypes.data, r.intervals.ctypes.data, THREADS)
        assert rc == 0, rc
        _cache[key] = r.freeze()
    return _cache[key]


def dense(lib, model):
    """The four tables from the 8-point Gauss-Legendre rule on each quarter of every cross-section table interval."""
    key = (model.atomic, "dense")
    if key not in _cache:
        r = Ref(*_shape(model), False)
        rc = lib.ratecoeff_cpu_dense(model.atomic, *[a.ctypes.data for a in r.tables()], THREADS)
        assert rc == 0, rc
        _cache[key] = r.freeze()
    return _cache[key]


def max_rel(a, b):
    """Largest |a - b| / |b| over every entry (b == 0 entries must match exactly)."""
    a, b = np.asarray(a), np.asarray(b)
    zero = b == 0
    assert np.array_equal(a[zero], b[zero])
    return float(np.max(np.abs(a[~zero] - b[~zero]) / np.abs(b[~zero]))) if (~zero).any() else 0.
