"""The rate-coefficient lookup tables of ratecoefficients_init built on the device (artis_gpu_ratecoeff_tables).

build() runs the integrals for a model's atomic tables and returns the arrays; with_tables() hands them to the
engine and the oracle in place of the tables the model came with.
"""
import ctypes as C

import numpy as np

from . import ffi, gpu_lib

# integral order of the status / intervals arrays
INTEGRALS = ("spontrecombcoeff", "corrphotoioncoeff", "bfheating_coeff", "bfcooling_coeff")


class RatecoeffError(RuntimeError):
    pass


class Tables:
    """The arrays of one artis_gpu_ratecoeff_tables call: the four [tablesize, nbfcontinua] float64 tables in
    get_bflutindex order (None for one not built), ion_alpha_sp [nions_total, tablesize] float32, the GSL status
    and final interval count of every integral [4, tablesize, nbfcontinua], and the kernel's milliseconds."""

    def __init__(self, tablesize, nbfcontinua, nions_total, photoion=True, bfheating=True, diagnostics=True):
        shape = (tablesize, nbfcontinua)
        self.spontrecombcoeff = np.zeros(shape)
        self.corrphotoioncoeff = np.zeros(shape) if photoion else None
        self.bfheating_coeff = np.zeros(shape) if bfheating else None
        self.bfcooling_coeff = np.zeros(shape)
        self.ion_alpha_sp = np.zeros((nions_total, tablesize), dtype=np.float32)
        self.status = np.zeros((4,) + shape, dtype=np.uint8) if diagnostics else None
        self.intervals = np.zeros((4,) + shape, dtype=np.int32) if diagnostics else None
        self.kernel_ms = 0.0

    def struct(self):
        s = ffi.RatecoeffOut()
        for name in ffi.RatecoeffOut._fields_:
            a = getattr(self, name[0])
            setattr(s, name[0], a.ctypes.data if a is not None else None)
        return s


def build(model, epsrel, device=0, photoion=True, bfheating=True, list_lds_capacity=0, out=None):
    """Build the tables of `model` (anything with an .atomic address of an artis_atomic_tables) at the relative
    accuracy epsrel (RATECOEFF_INTEGRAL_ACCURACY).  Needs no Engine and leaves a live one untouched."""
    hdr = ffi.AtomicTables.from_address(model.atomic)
    t = out if out is not None else Tables(hdr.tablesize, hdr.nbfcontinua, hdr.nions_total, photoion, bfheating)
    req = ffi.RatecoeffRequest(epsrel=float(epsrel), list_lds_capacity=int(list_lds_capacity))
    s = t.struct()
    lib = gpu_lib()
    rc = lib.artis_gpu_ratecoeff_tables(int(device), model.atomic, C.byref(req), C.byref(s))
    if rc != 0:
        msg = lib.artis_gpu_last_error()
        raise RatecoeffError(f"artis_gpu_ratecoeff_tables -> {rc}: {msg.decode() if msg else ''}")
    t.kernel_ms = float(lib.artis_gpu_last_ratecoeff_ms())
    return t


def _md5_array(md5):
    if len(md5) != 3:
        raise ValueError("md5: the hashes of adata.txt, compositiondata.txt and the phixs file")
    return (C.c_char_p * 3)(*[h.encode() if isinstance(h, str) else h for h in md5])


def write_dat(path, model, tables, md5):
    """ratecoeff.dat as the reference writes it (artis_write_ratecoeff_dat); a table that is None goes out as -1."""
    from . import io as aio

    s = tables.struct()
    rc = aio.lib().artis_write_ratecoeff_dat(str(path).encode(), model.atomic, C.byref(s), _md5_array(md5))
    if rc != 0:
        raise RatecoeffError(f"artis_write_ratecoeff_dat({path}) -> {rc}")


def read_dat(path, model, md5):
    """Read a ratecoeff.dat that matches `model` and the hashes: a Tables (corrphotoioncoeff / bfheating_coeff None
    where the file holds -1, ion_alpha_sp left zero), or None for "no match" (where the reference recalculates)."""
    from . import io as aio

    hdr = ffi.AtomicTables.from_address(model.atomic)
    t = Tables(hdr.tablesize, hdr.nbfcontinua, hdr.nions_total, diagnostics=False)
    s = t.struct()
    hg, hh = C.c_int32(1), C.c_int32(1)
    rc = aio.lib().artis_read_ratecoeff_dat(str(path).encode(), model.atomic, _md5_array(md5), C.byref(s),
                                            C.byref(hg), C.byref(hh))
    if rc < 0:
        raise RatecoeffError(f"artis_read_ratecoeff_dat({path}) -> {rc}")
    if rc == 0:
        return None
    if not hg.value:
        t.corrphotoioncoeff = None
    if not hh.value:
        t.bfheating_coeff = None
    return t


class ModelWithTables:
    """A model whose .atomic is a patched copy of the struct pointing at `tables`, and whose artis_te_tables are
    built from them; everything else is the wrapped model's.  Keeps the arrays alive."""

    def __init__(self, model, tables):
        if tables.corrphotoioncoeff is None or tables.bfheating_coeff is None:
            raise ValueError("with_tables needs all four tables")
        self._base = model
        self.ratecoeff_tables = tables
        self._atomic = ffi.AtomicTables.from_buffer_copy(ffi.AtomicTables.from_address(model.atomic))
        self._atomic.spontrecombcoeff = tables.spontrecombcoeff.ctypes.data
        self._atomic.corrphotoioncoeff = tables.corrphotoioncoeff.ctypes.data
        self._atomic.bfcooling_coeff = tables.bfcooling_coeff.ctypes.data
        self.atomic = C.addressof(self._atomic)
        self._te = ffi.TeTables(bfheating_coeff=tables.bfheating_coeff.ctypes.data,
                                ion_alpha_sp=tables.ion_alpha_sp.ctypes.data)
        self.te_tables = C.c_void_p(C.addressof(self._te))

    def __getattr__(self, name):
        return getattr(self._base, name)


def with_tables(model, tables):
    return ModelWithTables(model, tables)
