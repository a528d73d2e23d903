"""The rate-coefficient lookup tables (artis_gpu_ratecoeff_tables) as far as they can be checked without a GPU: the
entry point and what it refuses, the ctypes mirror of artis_atomic_tables, the host header ratecoeff_tables.h
(ion_alpha_sp, the clamp), the ratecoeff.dat file, and the CPU yardsticks of the GPU tests against each other."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ratecoeff_ref
from artis_amd import GPU_SO, ffi, gpu_lib, ratecoeff

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = -3  # ARTIS_ERR_BAD_ARGUMENT (include/artis_gpu.h)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
MD5 = ("0123456789abcdef0123456789abcdef", "fedcba9876543210fedcba9876543210", "00112233445566778899aabbccddeeff")


@pytest.fixture(scope="module")
def cpu_ref(tmp_path_factory):
    return ratecoeff_ref.load(tmp_path_factory.mktemp("ratecoeff_cpu_ref"))


def test_entry_point_is_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", GPU_SO], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"artis_gpu_ratecoeff_tables", "artis_gpu_last_ratecoeff_ms"} <= exported


def test_bad_arguments_are_refused_before_any_hip_call(small_model):
    """Every bad argument returns ARTIS_ERR_BAD_ARGUMENT with a message and leaves the arrays alone.  A HIP call made
    first would show as ARTIS_ERR_HIP on a machine without a GPU."""
    L = gpu_lib()
    good = ffi.AtomicTables.from_address(small_model.atomic)
    t = ratecoeff.Tables(good.tablesize, good.nbfcontinua, good.nions_total)
    for a in (t.spontrecombcoeff, t.corrphotoioncoeff, t.bfheating_coeff, t.bfcooling_coeff):
        a[:] = -7.

    def call(atomic=None, req=None, out=None, null=None):
        a = ffi.AtomicTables.from_buffer_copy(good)
        for k, v in (atomic or {}).items():
            setattr(a, k, v)
        r = ffi.RatecoeffRequest(epsrel=1e-3, list_lds_capacity=0)
        for k, v in (req or {}).items():
            setattr(r, k, v)
        o = t.struct()
        for k, v in (out or {}).items():
            setattr(o, k, v)
        args = [C.addressof(a), C.byref(r), C.byref(o)]
        if null is not None:
            args[null] = None
        rc = L.artis_gpu_ratecoeff_tables(0, *args)
        return rc, L.artis_gpu_last_error().decode()

    cases = {
        "epsrel 0": dict(req={"epsrel": 0.}),
        "epsrel negative": dict(req={"epsrel": -1e-3}),
        "epsrel nan": dict(req={"epsrel": float("nan")}),
        "unknown list capacity": dict(req={"list_lds_capacity": 7}),
        "negative list capacity": dict(req={"list_lds_capacity": -16}),
        "tablesize 1": dict(atomic={"tablesize": 1}),
        "mintemp 0": dict(atomic={"mintemp": 0.}),
        "mintemp negative": dict(atomic={"mintemp": -1.}),
        "mintemp == maxtemp": dict(atomic={"mintemp": good.maxtemp}),
        "mintemp > maxtemp": dict(atomic={"mintemp": 2 * good.maxtemp}),
        "NULL phixs_xs": dict(atomic={"phixs_xs": None}),
        "NULL level_cont_index": dict(atomic={"level_cont_index": None}),
        "NULL level_epsilon": dict(atomic={"level_epsilon": None}),
        "NULL spontrecombcoeff": dict(out={"spontrecombcoeff": None}),
        "NULL bfcooling_coeff": dict(out={"bfcooling_coeff": None}),
        "NULL ion_alpha_sp": dict(out={"ion_alpha_sp": None}),
        "a continuum count that does not match cont_index": dict(atomic={"nbfcontinua": good.nbfcontinua - 1}),
        "NULL atomic": dict(null=0),
        "NULL request": dict(null=1),
        "NULL output": dict(null=2),
    }
    for name, kw in cases.items():
        rc, msg = call(**kw)
        assert rc == BAD_ARGUMENT, (name, rc, msg)
        assert msg.startswith("ratecoeff_tables:"), (name, msg)
    rc, msg = C.CDLL(GPU_SO).artis_gpu_ratecoeff_tables(-1, None, None, None), ""
    assert rc == BAD_ARGUMENT
    for a in (t.spontrecombcoeff, t.corrphotoioncoeff, t.bfheating_coeff, t.bfcooling_coeff):
        assert (a == -7.).all()
    # the LUT pointers of the atomic tables are not among the needed arrays: the call comes before artis_gpu_init
    a = ffi.AtomicTables.from_buffer_copy(good)
    a.spontrecombcoeff = a.corrphotoioncoeff = a.bfcooling_coeff = None
    r = ffi.RatecoeffRequest(epsrel=0., list_lds_capacity=0)  # refused for epsrel, not for the NULL tables
    o = t.struct()
    assert L.artis_gpu_ratecoeff_tables(0, C.addressof(a), C.byref(r), C.byref(o)) == BAD_ARGUMENT
    assert "epsrel" in L.artis_gpu_last_error().decode()


def test_ctypes_mirror_of_atomic_tables_matches_the_compiler(tmp_path):
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "artis_gpu.h"
#define O(f) printf(#f " %zu\n", offsetof(artis_atomic_tables, f));
int main(void) {
  printf("sizeof %zu\n", sizeof(artis_atomic_tables));
  O(nelements) O(nphixsnuincrement) O(phixs_file_version) O(mintemp) O(elem_anumber) O(ion_ionstage) O(level_epsilon)
  O(phixs_xs) O(line_nu) O(allcont_nu_edge) O(groundcont_nu_edge) O(spontrecombcoeff) O(corrphotoioncoeff)
  O(bfcooling_coeff) O(coolinglist_type) O(ion_nlevels_nlte) O(total_nlte_levels) O(radfield_nbins)
  O(radfield_nu_upper) O(radfield_nu_lower_first)
  printf("request %zu\n", sizeof(artis_ratecoeff_request));
  printf("out %zu\n", sizeof(artis_ratecoeff_out));
  printf("out_intervals %zu\n", offsetof(artis_ratecoeff_out, intervals));
  return 0;
}
"""
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lay = {ln.split()[0]: int(ln.split()[1]) for ln in out.strip().splitlines()}
    assert lay.pop("sizeof") == C.sizeof(ffi.AtomicTables)
    assert lay.pop("request") == C.sizeof(ffi.RatecoeffRequest)
    assert lay.pop("out") == C.sizeof(ffi.RatecoeffOut)
    assert lay.pop("out_intervals") == ffi.RatecoeffOut.intervals.offset
    for name, off in lay.items():
        assert getattr(ffi.AtomicTables, name).offset == off, name
    # the header every other mirror reads is its leading part
    for name, _ in ffi.AtomicHeader._fields_:
        assert getattr(ffi.AtomicHeader, name).offset == getattr(ffi.AtomicTables, name).offset, name


@pytest.mark.parametrize("sanitized", [False, True])
def test_host_tables_header(tmp_path, sanitized):
    """tests/ratecoeff_tables_check.cpp compiles ratecoeff_tables.h alone: ion_alpha_sp and the clamp on hand-made
    tables, plain and as a stand-alone executable under the host address / undefined sanitizers."""
    exe = tmp_path / "ratecoeff_tables_check"
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", *(SANITIZE if sanitized else []),
                        "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "artis_amd", "csrc", "engine"),
                        os.path.join(REPO, "tests", "ratecoeff_tables_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    if sanitized and b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitizer" in b.stderr):
        pytest.skip("the host sanitizer runtime is not installed")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bad 0" in r.stdout


def _through_g(a):
    """what printf("%g") followed by scanf("%lg") makes of every value"""
    return np.array([float("%g" % v) for v in a.ravel()]).reshape(a.shape)


def _model_tables(model):
    """the model generator's own tables as a Tables (values to carry through the file; not a yardstick)"""
    h = ffi.AtomicTables.from_address(model.atomic)
    t = ratecoeff.Tables(h.tablesize, h.nbfcontinua, h.nions_total, diagnostics=False)
    te = ffi.TeTables.from_address(model._lib.artis_model_te_tables(model._h))
    n = h.tablesize * h.nbfcontinua
    for name, p in (("spontrecombcoeff", h.spontrecombcoeff), ("corrphotoioncoeff", h.corrphotoioncoeff),
                    ("bfcooling_coeff", h.bfcooling_coeff), ("bfheating_coeff", te.bfheating_coeff)):
        getattr(t, name)[:] = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), (n,)).reshape(h.tablesize, -1)
    return t


def test_ratecoeff_dat_round_trip(tmp_path, small_model):
    t = _model_tables(small_model)
    # distinct per-column values, so that a row read into the wrong column shows
    assert len(np.unique(t.spontrecombcoeff[50])) > 100
    path = tmp_path / "ratecoeff.dat"
    ratecoeff.write_dat(path, small_model, t, MD5)
    lines = path.read_text().splitlines()
    h = ffi.AtomicTables.from_address(small_model.atomic)
    assert lines[:3] == list(MD5)
    assert lines[3] == "%g %g %d %d" % (h.mintemp, h.maxtemp, h.tablesize, h.nlines)
    assert len(lines) == 4 + h.nions_total + h.tablesize * h.nbfcontinua
    assert all(len(ln.split()) == 4 for ln in lines[4:])
    back = ratecoeff.read_dat(path, small_model, MD5)
    assert back is not None
    for name in ratecoeff.INTEGRALS:
        assert np.array_equal(getattr(back, name), _through_g(getattr(t, name))), name
    # the file's rows run over (element, ion, level, target, temperature): the first rows are column 0 at every T
    first = np.array([[float(x) for x in ln.split()] for ln in lines[4 + h.nions_total:4 + h.nions_total + h.tablesize]])
    assert np.array_equal(first[:, 0], _through_g(t.spontrecombcoeff[:, 0]))
    assert np.array_equal(first[:, 1], _through_g(t.bfcooling_coeff[:, 0]))
    assert np.array_equal(first[:, 2], _through_g(t.corrphotoioncoeff[:, 0]))
    assert np.array_equal(first[:, 3], _through_g(t.bfheating_coeff[:, 0]))


def test_ratecoeff_dat_absent_tables_and_mismatches(tmp_path, small_model):
    t = _model_tables(small_model)
    h = ffi.AtomicTables.from_address(small_model.atomic)
    path = tmp_path / "ratecoeff.dat"
    # NO_LUT_PHOTOION / NO_LUT_BFHEATING files hold -1 in those columns
    t.corrphotoioncoeff = None
    ratecoeff.write_dat(path, small_model, t, MD5)
    assert all(ln.split()[2] == "-1" for ln in path.read_text().splitlines()[4 + h.nions_total:])
    back = ratecoeff.read_dat(path, small_model, MD5)
    assert back.corrphotoioncoeff is None and back.bfheating_coeff is not None
    assert np.array_equal(back.bfheating_coeff, _through_g(t.bfheating_coeff))
    t.bfheating_coeff = None
    ratecoeff.write_dat(path, small_model, t, MD5)
    back = ratecoeff.read_dat(path, small_model, MD5)
    assert back.corrphotoioncoeff is None and back.bfheating_coeff is None
    assert np.array_equal(back.spontrecombcoeff, _through_g(t.spontrecombcoeff))
    # "no match": a missing file, another hash, a changed nlines, a changed ion line
    good = path.read_text().splitlines()
    assert ratecoeff.read_dat(tmp_path / "none.dat", small_model, MD5) is None
    assert ratecoeff.read_dat(path, small_model, (MD5[0], MD5[1], MD5[0])) is None

    def rewritten(lineno, text):
        p = tmp_path / "changed.dat"
        p.write_text("\n".join(good[:lineno] + [text] + good[lineno + 1:]) + "\n")
        return p

    assert ratecoeff.read_dat(rewritten(3, "%g %g %d %d" % (h.mintemp, h.maxtemp, h.tablesize, h.nlines + 1)),
                              small_model, MD5) is None
    assert ratecoeff.read_dat(rewritten(3, "%g %g %d %d" % (h.mintemp, h.maxtemp, h.tablesize + 1, h.nlines)),
                              small_model, MD5) is None
    z, stage, nlev, nion = (int(x) for x in good[5].split())
    assert ratecoeff.read_dat(rewritten(5, f"{z} {stage} {nlev} {nion + 1}"), small_model, MD5) is None
    assert ratecoeff.read_dat(rewritten(5, f"{z} {stage + 1} {nlev} {nion}"), small_model, MD5) is None
    assert ratecoeff.read_dat(rewritten(5, good[5]), small_model, MD5) is not None
    # a truncated file is an error, not a match
    p = tmp_path / "short.dat"
    p.write_text("\n".join(good[:-3]) + "\n")
    with pytest.raises(ratecoeff.RatecoeffError):
        ratecoeff.read_dat(p, small_model, MD5)
    with pytest.raises(ratecoeff.RatecoeffError):
        ratecoeff.write_dat(path, small_model, _model_tables(small_model), ("short", MD5[1], MD5[2]))


@pytest.mark.parametrize("epsrel", [1e-3, 1e-2])
def test_cpu_qag_agrees_with_the_dense_quadrature(cpu_ref, small_model, epsrel):
    """Guards the yardsticks of the GPU tests: the oracle's qag on the four integrands ends with status 0 everywhere
    and within epsrel of the quadrature that knows where the cross-section table's kinks are."""
    q = ratecoeff_ref.qag(cpu_ref, small_model, epsrel)
    d = ratecoeff_ref.dense(cpu_ref, small_model)
    assert (q.status == 0).all()
    assert q.intervals.min() >= 1
    for name in ratecoeff_ref.NAMES:
        assert (getattr(d, name) > 0).all(), name
        rel = ratecoeff_ref.max_rel(getattr(q, name), getattr(d, name))
        print(f"epsrel {epsrel:g} {name}: max rel deviation from the dense quadrature {rel:.3e}, "
              f"most intervals {int(q.intervals.max())}")
        assert rel <= epsrel, (name, rel)
