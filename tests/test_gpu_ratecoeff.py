"""The rate-coefficient lookup tables built on the GPU (artis_gpu_ratecoeff_tables, k_ratecoeff_lut) on the
small_model atom (186 continua x 100 temperatures x 4 integrals).  Needs an MI355X.

Yardsticks (tests/ratecoeff_cpu_ref.cpp): a dense Gauss-Legendre quadrature that knows the integrands' kinks, which is
independent of qag, and the oracle's CPU restatement of the same qag.  Against the first the bar is the requested
epsrel; against the second the project's GPU-to-oracle floating-point bar of 1e-9 wherever both took the same
bisections.  Where an ocml / glibc last-ulp difference flips a bisection decision the interval counts differ: such
entries must still meet the quadrature bound and may be at most 0.1 % of all entries.
"""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
import parity
import ratecoeff_ref
from artis_amd import Engine, ffi, ratecoeff

pytestmark = pytest.mark.gpu

NAMES = ratecoeff.INTEGRALS
FP_RTOL = 1e-9        # tests/parity.py FP_RTOL
MAX_FLIPPED = 1e-3    # fraction of entries whose interval count may differ from the CPU restatement's
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, "artis_amd", "lib", "artis_gpu_driver")
_gpu = {}


@pytest.fixture(scope="module")
def cpu_ref(tmp_path_factory):
    return ratecoeff_ref.load(tmp_path_factory.mktemp("ratecoeff_cpu_ref"))


def gpu_tables(model, epsrel):
    """the device tables at epsrel, built once and shared; callers do not write to them"""
    if epsrel not in _gpu:
        _gpu[epsrel] = ratecoeff.build(model, epsrel)
    return _gpu[epsrel]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_tables(a, b, names=NAMES + ("ion_alpha_sp", "status", "intervals")):
    for n in names:
        assert same_bits(getattr(a, n), getattr(b, n)), n


@pytest.mark.parametrize("epsrel", [1e-3, 1e-2])
def test_against_the_independent_quadrature(cpu_ref, small_model, epsrel):
    t = gpu_tables(small_model, epsrel)
    d = ratecoeff_ref.dense(cpu_ref, small_model)
    assert (t.status == 0).all(), np.unique(t.status, return_counts=True)
    assert t.intervals.min() >= 1
    for n in NAMES:
        # every entry, none excluded: max_rel divides by the yardstick, which is positive everywhere
        assert (getattr(d, n) > 0).all()
        rel = ratecoeff_ref.max_rel(getattr(t, n), getattr(d, n))
        print(f"epsrel {epsrel:g} {n}: max rel deviation from the dense quadrature {rel:.3e}")
        assert rel <= epsrel, (n, rel)


def test_tables_are_in_bflutindex_order(cpu_ref, small_model):
    """The yardstick's columns come from the helper's own get_bflutindex (-1 - cont_index + target).  Both targets of
    every two-target ground level are looked at by name: they sit in adjacent columns, differ from each other by far
    more than the bound, and each matches the yardstick's column."""
    t = gpu_tables(small_model, 1e-3)
    d = ratecoeff_ref.dense(cpu_ref, small_model)
    h = ffi.AtomicTables.from_address(small_model.atomic)
    i32 = lambda p, n: np.ctypeslib.as_array(ffi.C.cast(p, ffi.C.POINTER(ffi.C.c_int32)), (n,))  # noqa: E731
    ntg = i32(h.level_nphixstargets, h.nlevels_total)
    cont = i32(h.level_cont_index, h.nlevels_total)
    two = [ul for ul in oracle_lib.ionising_levels(small_model) if ntg[ul] == 2]
    assert two, "the small model has two-target ground levels"
    for ul in two:
        c0 = -1 - cont[ul]
        for n in NAMES:
            for c in (c0, c0 + 1):
                col, ref = getattr(t, n)[:, c], getattr(d, n)[:, c]
                assert np.max(np.abs(col - ref) / ref) <= 1e-3, (n, ul, c)
        # the two targets differ (other threshold and probability), so a swap would show above
        assert np.max(np.abs(d.spontrecombcoeff[:, c0] - d.spontrecombcoeff[:, c0 + 1]) /
                      d.spontrecombcoeff[:, c0]) > 1e-2


@pytest.mark.parametrize("epsrel,bound", [(1e-3, 1e-3), (1e-6, 1e-3)])
def test_against_the_cpu_restatement(cpu_ref, small_model, epsrel, bound):
    """1e-6 drives qpsrt through long error lists and ends 1,452 integrals with GSL_EROUND (18)."""
    t = gpu_tables(small_model, epsrel)
    q = ratecoeff_ref.qag(cpu_ref, small_model, epsrel)
    d = ratecoeff_ref.dense(cpu_ref, small_model)
    assert set(np.unique(q.status)) <= {0, 18}
    if epsrel == 1e-6:
        assert (q.status == 18).sum() > 1000 and q.intervals.max() > 16
    assert np.array_equal(t.status, q.status), (np.unique(t.status, return_counts=True))
    flipped_total = 0
    for k, n in enumerate(NAMES):
        g, c, y = getattr(t, n), getattr(q, n), getattr(d, n)
        same = t.intervals[k] == q.intervals[k]
        rel = np.abs(g - c) / np.abs(c)
        worst = float(rel[same].max())
        nflip = int((~same).sum())
        flipped_total += nflip
        print(f"epsrel {epsrel:g} {n}: {nflip} entries with another interval count; max rel vs the CPU restatement "
              f"{worst:.3e} where the counts agree")
        assert worst <= FP_RTOL, (n, worst)
        if nflip:
            assert float((np.abs(g - y) / y)[~same].max()) <= bound, n
    print(f"epsrel {epsrel:g}: {flipped_total} of {t.status.size} entries with another interval count")
    assert flipped_total <= MAX_FLIPPED * t.status.size, flipped_total


def test_error_list_spill_changes_nothing(small_model):
    """list_lds_capacity 16: from the 17th interval on the error list and its order live in the global workspace
    (the 1e-6 run reaches 64 intervals); the bits are those of the default run."""
    t = gpu_tables(small_model, 1e-6)
    assert t.intervals.max() > 16
    s = ratecoeff.build(small_model, 1e-6, list_lds_capacity=16)
    assert_same_tables(s, t)
    e = ratecoeff.build(small_model, 1e-6, list_lds_capacity=64)
    assert_same_tables(e, t)


def test_determinism_and_skipped_integrals(small_model):
    t = gpu_tables(small_model, 1e-3)
    again = ratecoeff.build(small_model, 1e-3)
    assert_same_tables(again, t)
    # NO_LUT_PHOTOION: corrphotoioncoeff NULL.  The other tables keep their bits and the skipped integral's
    # diagnostics are zero
    h = ffi.AtomicTables.from_address(small_model.atomic)
    out = ratecoeff.Tables(h.tablesize, h.nbfcontinua, h.nions_total, photoion=False)
    # the one corrphotoioncoeff buffer the call can see is the atomic tables' own: it stays as it is
    own = np.ctypeslib.as_array(ffi.C.cast(h.corrphotoioncoeff, ffi.C.POINTER(ffi.C.c_double)),
                                (h.tablesize * h.nbfcontinua,))
    before = own.copy()
    s = ratecoeff.build(small_model, 1e-3, out=out)
    assert s.corrphotoioncoeff is None and same_bits(own, before)
    assert_same_tables(s, t, names=("spontrecombcoeff", "bfheating_coeff", "bfcooling_coeff", "ion_alpha_sp"))
    assert not s.status[1].any() and not s.intervals[1].any()
    for k in (0, 2, 3):
        assert same_bits(s.status[k], t.status[k]) and same_bits(s.intervals[k], t.intervals[k])
    # NO_LUT_BFHEATING likewise, and without the optional diagnostics
    out = ratecoeff.Tables(h.tablesize, h.nbfcontinua, h.nions_total, bfheating=False, diagnostics=False)
    s = ratecoeff.build(small_model, 1e-3, out=out)
    assert s.bfheating_coeff is None and s.status is None
    assert_same_tables(s, t, names=("spontrecombcoeff", "corrphotoioncoeff", "bfcooling_coeff", "ion_alpha_sp"))


def test_ion_alpha_sp_is_the_host_function_of_spontrecombcoeff(small_model):
    """precalculate_ion_alpha_sp / get_spontrecombcoeff (ratecoeff.cc:686-710, 970-992) restated here in numpy on the
    returned spontrecombcoeff: the lookup at the float T_e, the sum over an ion's columns in double, stored as float."""
    t = gpu_tables(small_model, 1e-3)
    h = ffi.AtomicTables.from_address(small_model.atomic)
    C = ffi.C
    i32 = lambda p, n: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), (n,))  # noqa: E731
    ts, ni = h.tablesize, h.nions_total
    nions, ionoff = i32(h.elem_nions, h.nelements), i32(h.elem_uniqueionoffset, h.nelements)
    lvoff, nionis = i32(h.ion_uniqueleveloffset, ni), i32(h.ion_ionisinglevels, ni)
    ntg, cont = i32(h.level_nphixstargets, h.nlevels_total), i32(h.level_cont_index, h.nlevels_total)
    T_step_log = (np.log(h.maxtemp) - np.log(h.mintemp)) / (ts - 1.)
    want = np.zeros((ni, ts), np.float32)
    for it in range(ts):
        T_e = np.float32(h.mintemp * np.exp(it * T_step_log))
        lower = int(np.floor(np.log(float(T_e) / h.mintemp) / T_step_log))
        for e in range(h.nelements):
            for i in range(nions[e] - 1):
                ui = ionoff[e] + i
                zeta = 0.
                for lv in range(nionis[ui]):
                    ul = lvoff[ui] + lv
                    for tg in range(ntg[ul]):
                        col = -1 - cont[ul] + tg
                        if lower < ts - 1:
                            T_lower = h.mintemp * np.exp(lower * T_step_log)
                            T_upper = h.mintemp * np.exp((lower + 1) * T_step_log)
                            f_upper, f_lower = t.spontrecombcoeff[lower + 1, col], t.spontrecombcoeff[lower, col]
                            zeta += (f_lower + (f_upper - f_lower) / (T_upper - T_lower) * (float(T_e) - T_lower))
                        else:
                            zeta += t.spontrecombcoeff[ts - 1, col]
                want[ui, it] = np.float32(zeta)
    assert (want[[ionoff[e] + nions[e] - 1 for e in range(h.nelements)]] == 0).all()
    assert (want > 0).sum() == (ni - h.nelements) * ts
    assert same_bits(t.ion_alpha_sp, want)


def test_live_engine_is_left_untouched(small_model):
    """With an Engine alive: a step from restored state before the call and one after it give the same bytes."""
    m = small_model
    nts = 5
    m.set_timestep(nts)
    pk0 = m.init_rpackets(nts, 512, seed=21)
    eng = Engine(m)
    try:
        eng.upload_cellstate(nts)
        eng.upload(pk0)
        eng.snapshot()

        def step():
            eng.restore()
            eng.zero_estimators()
            eng.step_resident(nts)
            out = pk0.copy()
            eng.download(out)
            return out, eng.download_estimators()

        before, est_before = step()
        t = ratecoeff.build(m, 1e-3)
        after, est_after = step()
    finally:
        eng.close()
    assert before.tobytes() == after.tobytes()
    assert before.tobytes() != pk0.tobytes()
    assert np.array_equal(est_before.counters, est_after.counters)
    assert_same_tables(t, gpu_tables(m, 1e-3))


def test_transport_with_the_device_built_tables(small_model):
    """Engine(with_tables(model, tables)) against the oracle on the same patched tables: one step of 512 packets."""
    wm = ratecoeff.with_tables(small_model, gpu_tables(small_model, 1e-3))
    nts = 6
    small_model.set_timestep(nts)
    pk0 = small_model.init_rpackets(nts, 512, seed=9)
    eng = Engine(wm)
    try:
        eng.upload_cellstate(nts)
        pg = pk0.copy()
        eg = eng.update_packets(nts, pg)
    finally:
        eng.close()
    po = pk0.copy()
    eo, _ = oracle_lib.update_packets(wm, nts, po)
    parity.assert_packets_match(pg, po)
    parity.assert_estimators_match(eg, eo)


def test_solve_temperatures_with_the_device_built_tables(small_model):
    from test_gpu_te_solver import compare

    wm = ratecoeff.with_tables(small_model, gpu_tables(small_model, 1e-3))
    small_model.set_timestep(6)
    te = ffi.TeArrays(wm, t_current=12 * 86400.0, thick_frac=0.3, seed=5)
    te.tables = wm.te_tables
    cpu = te.copy()
    assert oracle_lib.solve_temperatures(wm, cpu) == 0
    eng = Engine(wm)
    try:
        eng.solve_temperatures(te)
    finally:
        eng.close()
    frac, rooted = compare(wm, te, cpu)
    assert rooted > 10
    print(f"cells {len(te.mgi_list)}, agreeing {frac:.3f}, rooted {rooted}")


def test_driver_builds_its_tables_on_the_device(tmp_path):
    env = dict(os.environ, ARTIS_DRIVER_RATECOEFF="1")
    r = subprocess.run([DRIVER, str(tmp_path), "10", "60", "20", "8000", "30", "8", "1", "512", "5"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ratecoeff_tables ms ")]
    assert len(line) == 1, r.stdout
    f = line[0].split()
    vals = dict(zip(f[1::2], f[2::2]))
    assert float(vals["ms"]) > 0 and float(vals["kernel_ms"]) > 0
    assert int(vals["integrals"]) == 4 * 186 * 100
    assert int(vals["status0"]) == int(vals["integrals"])
    assert any(ln.startswith("nts 8 ") for ln in r.stdout.splitlines())
