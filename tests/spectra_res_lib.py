"""Shared by tests/test_spectra_res.py and tests/test_gpu_spectra_res.py: the inputs the two files agree on, the
oracle's direction-resolved set built from oracle_lib.spectra one bin at a time, comparisons and file parsers."""
import numpy as np

import oracle_lib
from artis_amd import ffi

NTS = 9
NNUBINS = 60
SYN_DIR = (0.3, 0.4, float(np.sqrt(0.75)))
RTOL_SUMS = 1e-9   # device float64 atomics against serial sums, per array and slot (tests/test_spectrum.py:166)
RTOL_FILES = 1e-5  # the writers print "%g": 6 significant digits (tests/test_spectrum.py:59)
LSUN = 3.826e33


def oracle_res(model, packets, nprocs=1, abin_first=0, abin_count=ffi.MABINS, with_average=True, emission_res=True,
               stokes=False, out=None):
    """The oracle's arrays for the slots of one spectra_res request, ADDED into out (made when None): one
    oracle_lib.spectra call per slot."""
    if out is None:
        out = ffi.SpectraResArrays(model.cfg.ntstep, NNUBINS, model.nelements, model.maxnions, abin_first, abin_count,
                                   with_average, emission_res, stokes)
    for abin in out.abins():
        o = oracle_lib.spectra(model, packets, nnubins=NNUBINS, nprocs=nprocs, abin=abin, syn_dir=SYN_DIR,
                               emission_res=emission_res, stokes=stokes)
        for name, view in out.slot(abin).arrays().items():
            view += getattr(o, name)
    return out


def assert_sums_close(expect, got, what):
    """max|a - b| <= 1e-9 max|a| for every array `expect` holds (a dict of arrays or an object with .arrays())."""
    ea = expect if isinstance(expect, dict) else expect.arrays()
    for name, a in ea.items():
        b = got[name] if isinstance(got, dict) else getattr(got, name)
        assert b is not None and b.shape == a.shape, (what, name)
        scale = max(np.abs(a).max(), 1e-300)
        err = np.abs(a - b).max()
        assert err <= RTOL_SUMS * scale, (what, name, err, scale)


def rows(path):
    return [[float(v) for v in ln.split()] for ln in open(path).read().splitlines()]


def read_spec(path):
    """spec.out -> flux [numtimesteps, nnubins] (the header row and the nu column dropped)."""
    r = rows(path)
    return np.array(r[1:])[:, 1:].T


def read_columns(path, nnubins, nt):
    """emission.out / absorption.out -> [nt, nnubins, columns] (rows run over (frequency bin, timestep))."""
    a = np.array(rows(path))
    return a.reshape(nnubins, nt, a.shape[1]).transpose(1, 0, 2)


def read_specpol(path, nt):
    """specpol.out -> [3, nt, nnubins]."""
    a = np.array(rows(path)[1:])[:, 1:]
    return a.reshape(a.shape[0], 3, nt).transpose(1, 2, 0)


def assert_file_close(back, expect, what):
    assert back.shape == expect.shape, (what, back.shape, expect.shape)
    assert np.allclose(back, expect, rtol=RTOL_FILES, atol=0), what
