"""Pins of the oracle's nebular update_grid (oracle/nebular_update_grid.cc, the checker of artis_gpu_update_grid_nlte)
against independent computations: the restated GSL LU with refinement against LAPACK (numpy), the Spencer-Fano
triangular solve against scipy, the qag Planck integrals against their closed forms, the Spencer-Fano source / loss
terms against energy conservation, the NLTE rate matrices against particle conservation (every column sums to zero
before the normalisation row), and the converged one-zone solution against its own consistency relations.  CPU only.
"""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.linalg

import nebular_ref as nr
import oracle_lib
from artis_amd import ffi
from artis_amd.model import Model

TWOHOVERCLIGHTSQUARED, HOVERKB = 1.4745007e-47, 4.799243681748932e-11  # the reference's constants (constants.h)


def _lib():
    L = oracle_lib.lib()
    d, i, vp = C.c_double, C.c_int, C.c_void_p
    L.oracle_nl_matrix_solve.argtypes = [vp, vp, i, vp]
    L.oracle_sf_solve.argtypes = [vp, vp, i, vp]
    L.oracle_sf_solve.restype = None
    L.oracle_planck_integral.argtypes = [d, d, d, i]
    L.oracle_planck_integral.restype = d
    L.oracle_sf_grid.argtypes = [i, d, d, d, vp, vp, vp, vp]
    L.oracle_sf_grid.restype = d
    return L


def _lu_solve(A, b):
    n = len(b)
    Acol = np.ascontiguousarray(A.T)  # column-major
    x = np.zeros(n)
    rc = _lib().oracle_nl_matrix_solve(Acol.ctypes.data, np.ascontiguousarray(b).ctypes.data, n, x.ctypes.data)
    return rc, x


@pytest.mark.parametrize("n,seed", [(5, 1), (43, 2), (120, 3)])
def test_lu_solve_matches_lapack(n, seed):
    """nltepop_matrix_solve's LU (partial pivoting, GSL <= 2.6 order) + refinement against LAPACK's dgesv, on rate-matrix
    shaped systems (negative diagonals, non-negative off-diagonals, a normalisation row) whose rows are permuted so
    that pivoting is needed."""
    rng = np.random.default_rng(seed)
    A = rng.random((n, n)) * (rng.random((n, n)) < 0.3)
    np.fill_diagonal(A, 0.)
    A -= np.diag(A.sum(axis=0) + rng.random(n))
    A[0, :] = 1.
    A = A[rng.permutation(n)]
    b = np.zeros(n)
    b[np.argmax(A[:, 0] == 1.)] = 3.7
    rc, x = _lu_solve(A, b)
    assert rc == 0
    ref = np.linalg.solve(A, b)
    np.testing.assert_allclose(x, ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max())


def test_lu_solve_reports_singular():
    A = np.array([[1., 2., 3.], [2., 4., 6.], [0., 1., 1.]])
    rc, _ = _lu_solve(A, np.array([1., 2., 3.]))
    assert rc == 1


def test_sf_solve_matches_triangular():
    """sfmatrix_solve: column-oriented back substitution with 9 refinement passes against scipy's triangular solve."""
    rng = np.random.default_rng(5)
    n = 300
    U = np.triu(rng.random((n, n)) * 1e-3) + np.diag(1. + rng.random(n))
    b = rng.random(n)
    y = np.zeros(n)
    _lib().oracle_sf_solve(np.ascontiguousarray(U).ctypes.data, b.ctypes.data, n, y.ctypes.data)
    np.testing.assert_allclose(y, scipy.linalg.solve_triangular(U, b), rtol=1e-13)


def _planck_closed(T, nu1, nu2, times_nu):
    """2h/c^2 (kT/h)^(4|5) [G(x2) - G(x1)] with G(x) = int_0^x t^p / (e^t - 1) dt from its exponential series
    (x > 0), difference taken tail-minus-tail; the reference's TWOHOVERCLIGHTSQUARED and HOVERKB."""
    x1, x2 = HOVERKB * nu1 / T, HOVERKB * nu2 / T
    k = np.arange(1, 200001, dtype=np.float64)

    def tail(x):  # int_x^inf
        e = np.exp(-k * x)
        if times_nu:
            return np.sum(e * (x ** 4 / k + 4 * x ** 3 / k ** 2 + 12 * x ** 2 / k ** 3 + 24 * x / k ** 4 + 24 / k ** 5))
        return np.sum(e * (x ** 3 / k + 3 * x ** 2 / k ** 2 + 6 * x / k ** 3 + 6 / k ** 4))

    scale = TWOHOVERCLIGHTSQUARED * (T / HOVERKB) ** (5 if times_nu else 4)
    if x2 < 1.:
        # Rayleigh-Jeans side: t^p / (e^t - 1) = sum_n B_n t^(n+p-1) / n!, integrated term by term (the tails would
        # cancel catastrophically)
        from fractions import Fraction as F
        bern = {0: F(1), 1: F(-1, 2), 2: F(1, 6), 4: F(-1, 30), 6: F(1, 42), 8: F(-1, 30), 10: F(5, 66),
                12: F(-691, 2730), 14: F(7, 6), 16: F(-3617, 510)}
        p = 4 if times_nu else 3
        fact = 1
        tot = 0.
        for nn in range(17):
            fact = fact * max(nn, 1)
            if nn in bern:
                q = nn + p
                tot += float(bern[nn]) / fact / q * (x2 ** q - x1 ** q)
        return scale * tot
    return scale * (tail(x1) - tail(x2))


@pytest.mark.parametrize("T,nu1,nu2", [(5000., 1e14, 1.2e14), (20000., 3e14, 6e14), (250000., 7.5e13, 1e14),
                                       (3000., 2e15, 2.5e15), (10000., 1e15, 1e17)])
@pytest.mark.parametrize("times_nu", [0, 1])
def test_planck_integral_closed_form(T, nu1, nu2, times_nu):
    """radfield.cc planck_integral (the oracle's GSL qag, epsrel 1e-10) against the closed form."""
    got = _lib().oracle_planck_integral(T, nu1, nu2, times_nu)
    np.testing.assert_allclose(got, _planck_closed(T, nu1, nu2, times_nu), rtol=1e-9)


@pytest.mark.parametrize("nne", [1e4, 1e7])
def test_sf_loss_only_solution_conserves_energy(nne):
    """With only the Coulomb loss term the Spencer-Fano matrix is diagonal and y(E) = (source integral above E) / L(E);
    the energy it degrades, sum_i y_i L_i dE, is the injected energy E_init to the grid's resolution."""
    n, emin, emax = 4096, 0.1, 16000.
    env, src, rhs, loss = (np.zeros(n) for _ in range(4))
    e_init = _lib().oracle_sf_grid(n, emin, emax, nne, env.ctypes.data, src.ctypes.data, rhs.ctypes.data,
                                   loss.ctypes.data)
    de = (emax - emin) / (n - 1)
    np.testing.assert_allclose(env, emin + np.arange(n) * de, rtol=1e-15)
    assert src[:-137].max() == 0. and np.all(src[-137:] > 0)  # SF source: the top 3.333 % of the grid
    assert e_init == pytest.approx(np.sum(np.abs(src * de * env)), rel=1e-14)
    U = np.diag(loss)
    y = np.zeros(n)
    _lib().oracle_sf_solve(np.ascontiguousarray(U).ctypes.data, rhs.ctypes.data, n, y.ctypes.data)
    degraded = np.sum(y * loss) * de
    assert degraded == pytest.approx(e_init, rel=2e-3)
    # the Coulomb loss rate falls with energy above the plasma regime (nonthermal.cc:820-840)
    assert np.all(np.diff(loss[np.searchsorted(env, 20.):]) < 0)


@pytest.fixture(scope="module")
def onezone_solved(tmp_path_factory):
    """The nebularonezone reference inputs at timestep 6 solved by the oracle from its own transport step, with the
    first pass's rate matrices dumped."""
    ref = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_inputs", "nebularonezone")
    m = Model(files=(os.path.join(ref, "input-newrun.txt"), os.path.join(ref, "model.txt"),
                     os.path.join(ref, "abundances.txt")), ngrid_1d=10, nlevels_per_ion=30, n_ionising=10,
              max_lines=2000, nebular=1, nlte_level_max=12, ionpot_scale=0.5)
    nts = 6
    m.set_timestep(nts - 1)
    est, _ = oracle_lib.update_packets(m, nts - 1, m.init_rpackets(nts - 1, 6000, seed=5), nthreads=8)
    m.set_timestep(nts)
    nt = ffi.NtDataHandle(m)
    arr = ffi.NlteArrays(m, nts, est=est, dep_scale=3e-4)
    arr.params.num_lte_timesteps = 4
    prefix = str(tmp_path_factory.mktemp("nl") / "d")
    os.environ["ORACLE_NL_DUMP"] = prefix
    try:
        assert oracle_lib.update_grid_nlte(m, nt, arr, nthreads=8) == 0
    finally:
        del os.environ["ORACLE_NL_DUMP"]
    return m, arr, prefix


def test_rate_matrices_conserve_particles(onezone_solved):
    """Every process the NLTE rate matrix holds moves population from one level to another (nltepop.cc:421-591):
    each column of the summed matrix, before the normalisation row replaces row 0, sums to zero."""
    m, arr, prefix = onezone_solved
    checked = 0
    for e in range(m.nelements):
        fn = f"{prefix}_p0_ora_e{e}.bin"
        if not os.path.exists(fn):
            continue
        with open(fn, "rb") as f:
            D, _ = np.frombuffer(f.read(8), np.int32)
            f.read(8 * (D * D + 3 * D))  # normalised matrix, b, norm, populations
            raw = np.frombuffer(f.read(8 * D * D), np.float64).reshape(D, D).T  # [row, col]
        colsum = raw.sum(axis=0)
        scale = np.abs(raw).max(axis=0)
        assert np.all(np.abs(colsum) <= 1e-12 * scale), (e, np.max(np.abs(colsum) / scale))
        assert np.all(np.diag(raw) <= 0.)
        checked += 1
    assert checked >= 2


def test_onezone_solution_is_consistent(onezone_solved):
    """The converged state obeys the relations update_grid relies on: each element's level populations add up to its
    number density (within the 1 % the reference tolerates before resetting), n_e = sum_ions (stage - 1) n_ion,
    the Spencer-Fano fractions add up to one, T_e inside [MINTEMP, MAXTEMP], positive non-thermal rates."""
    m, arr, _ = onezone_solved
    c = int(arr.mgi_list[0])
    ni = m.nions_total
    g0 = m.ion_ground_statweight().astype(np.float64)
    nion = arr.groundlevelpop.reshape(-1, ni)[c] * arr.partfunct.reshape(-1, ni)[c].astype(np.float64) / g0
    stage = m.ion_ionstage()
    el = m.ion_element()
    nne = float(np.sum((stage - 1) * nion))
    assert arr.nne[c] == pytest.approx(nne, rel=1e-6)
    rho = float(arr.rho[c])
    ab = arr.elem_abundance.reshape(-1, m.nelements)[c]
    mw = arr.elem_meanweight.reshape(-1, m.nelements)[c]
    for e in range(m.nelements):
        if ab[e] <= 0:
            continue
        assert nion[el == e].sum() == pytest.approx(ab[e] / mw[e] * rho, rel=1e-2)
    assert arr.nt_frac_heating[c] + arr.nt_frac_ionization[c] + arr.nt_frac_excitation[c] == pytest.approx(1., abs=1e-6)
    assert arr.params.T_min <= arr.Te[c] <= arr.params.T_max and arr.iters[c] >= 2
    Y = arr.nt_ionization_ratecoeff.reshape(-1, ni)[c]
    assert np.all(Y[stage < np.array([stage[el == e].max() for e in el])] > 0)


# ------------------------------------------------------------------------------------------------------------
# The reference's own margins on the cases of tests/test_gpu_nebular_update_grid.py, pinned without a GPU.  Measured
# by tools/nebular_ref_floors.py; the GPU tests derive the engine's bounds from the same figures (nebular_ref.bound).
SF_SOLVE_ERROR = 1.4e-15  # tools/nebular_ref_floors.py: Spencer-Fano solution against longdouble, max-norm
LU_SOLVE_ERROR = 1.9e-06  # tools/nebular_ref_floors.py: rate-matrix solutions against a 40-digit solve, L1
BIN_W_SPREAD = 2.2e-08    # tools/nebular_ref_floors.py: spread of W P(T_R) / J_bin over the fitted synthetic bins


@pytest.mark.parametrize("nbins,T_R_min", nr.SYNTH_BIN_CASES)
def test_bin_fits_synthetic_oracle(nbins, T_R_min):
    """fit_parameters on bins with known answers (nebular_ref.SyntheticBins: Planck spectra from 30-digit integrals
    below, inside and above [T_R_min, T_R_max], an empty bin, the W > 1e4 fallback to T_R_max, the -99 outcome, T_e in
    the last bin): every kind ends in its class; around every Brent root the 30-digit mean-frequency residual changes
    sign within 1.5e-4 (the 1e-4 bracket of find_T_R); W P(T_R) / J_bin is the same for every bin to a float32 ulp."""
    sb = nr.SyntheticBins(nr.oracle_estimators, nbins, T_R_min)
    a = sb.arr.copy()
    assert oracle_lib.update_grid_nlte(sb.model, sb.nt, a, params=sb.params, nthreads=8) == 0
    want = {"planck": None, **sb.expected()}
    classes = {}
    for (c, b), (kind, T, J) in sb.bins.items():
        cls = sb.outcome(a, c, b)
        if kind == "planck":
            want_cls = "min" if T < T_R_min else "max" if T > nr.T_R_MAX else "root"
            assert cls == want_cls, (c, b, T, cls)
            if cls == "root":  # the spectrum's own temperature, to the bracket
                assert a.bin_TR[c * nbins + b] == pytest.approx(T, rel=nr.ROOT_RTOL)
        else:
            assert cls == want[kind], (c, b, kind, cls)
        classes[cls] = classes.get(cls, 0) + 1
    assert set(classes) == {"empty", "minus99", "min", "max", "Te", "root"} and classes["root"] == 4, classes
    nroot, spread = sb.check(a, "oracle")
    assert nroot == 4
    assert spread <= 10 * BIN_W_SPREAD and spread <= 2 * nr.F32_ULP, spread


@pytest.mark.parametrize("sfpts,sf_emax", nr.SF_SHAPES)
def test_sf_solution_against_longdouble(sfpts, sf_emax, tmp_path, monkeypatch):
    """sfmatrix_solve on the one-zone model's own matrix at the grid sizes of the GPU tests: the kept solution against
    a plain longdouble back substitution, a finite solution with heating fractions just below one and Auger
    probabilities that add up to one."""
    prefix = str(tmp_path / "sf")
    monkeypatch.setenv("ORACLE_NL_DUMP", prefix)
    m, p, nt, arr, nts = nr.onezone_case(nr.oracle_estimators, 12, True, sfpts=sfpts, sf_emax=sf_emax, one_pass=True,
                                         npkts=6000)
    assert oracle_lib.update_grid_nlte(m, nt, arr, params=p, nthreads=8) == 0
    c = int(arr.mgi_list[0])
    mgi, M, rhs, y = nr.read_dump_sf(prefix + "_sf_ora.bin", column_major=False)
    assert mgi == c and M.shape == (sfpts, sfpts) and np.all(np.isfinite(y)) and np.all(np.diag(M) > 0)
    assert nr.sf_solution_error(M, rhs, y) <= 10 * SF_SOLVE_ERROR
    assert 0.9999 < arr.nt_frac_heating[c] < 1.
    psum = arr.nt_prob_num_auger.reshape(m.npts_model, m.nions_total, -1)[c].sum(axis=1)
    assert np.all((np.abs(psum - 1.) < 1e-6) | (psum == 0.)), psum


def test_lu_solution_against_high_precision(tmp_path, monkeypatch):
    """nltepop_matrix_solve on the one-zone model's first-pass rate matrices against a 40-digit solve of the same
    systems: the L1 error stays within 10 x the committed floor (populations spanning 40 decades; LAPACK on random
    well-conditioned systems, above, reaches 1e-10)."""
    prefix = str(tmp_path / "nl")
    monkeypatch.setenv("ORACLE_NL_DUMP", prefix)
    m, p, nt, arr, nts = nr.onezone_case(nr.oracle_estimators, 12, True, sfpts=48, sf_emax=500., one_pass=True,
                                         npkts=6000)
    assert oracle_lib.update_grid_nlte(m, nt, arr, params=p, nthreads=8) == 0
    checked = 0
    for e in range(m.nelements):
        fn = f"{prefix}_p0_ora_e{e}.bin"
        if not os.path.exists(fn):
            continue
        d = nr.read_dump_oracle(fn)
        D = d["D"]
        err, ref = nr.lu_solution_error(d["A"].reshape(D, D).T, d["b"], d["norm"], d["pv"])
        assert d["status"] == 0 and err <= 10 * LU_SOLVE_ERROR, (e, err)
        assert ref.sum() == pytest.approx(d["b"][0], rel=1e-12)  # row 0: the populations add up to the element's
        assert len(d["pops"]) == m.nlevels_total and np.all(d["pops"] >= 0.)
        checked += 1
    assert checked >= 2


def test_element_number_density_quotient_in_double():
    """get_elem_numberdens (grid.cc:231-236) promotes the element's mean weight to double before dividing the float
    abundance by it.  The adiabatic cooling rate p dV / V with p = n_tot k T_e, n_tot = sum_Z Z n_element
    (thermalbalance.cc:380-388) shows it: a float quotient moves it by up to 6e-8, the double one reproduces it to
    rounding."""
    m, p, nt, arr, nts = nr.onezone_case(nr.oracle_estimators, 12, True, sfpts=48, sf_emax=500., one_pass=True,
                                         npkts=6000)
    a = arr.copy()
    assert oracle_lib.update_grid_nlte(m, nt, a, params=p, nthreads=8) == 0
    c = int(arr.mgi_list[0])
    ne = m.nelements
    hdr = ffi.AtomicHeader.from_address(m.atomic)
    Z = np.ctypeslib.as_array(C.cast(hdr.elem_anumber, C.POINTER(C.c_int32)), (ne,)).astype(np.float64)
    ab, mw = arr.elem_abundance.reshape(-1, ne)[c], arr.elem_meanweight.reshape(-1, ne)[c]
    assert ab.dtype == mw.dtype == np.float32
    KB = 1.38064852e-16
    par = arr.params
    vol = arr.vol_init[c]
    dV_over_V = (3 * vol / par.tmin ** 3 * par.t_current_te ** 2) / (vol * (par.t_current_te / par.tmin) ** 3)

    def adiabatic(quotient, T_e):
        return float(np.sum(quotient * np.float64(arr.rho[c]) * Z)) * KB * T_e * dV_over_V

    got = a.rates.reshape(-1, 8)[c, 3]
    in_double = [adiabatic(ab / mw.astype(np.float64), T) for T in (par.T_min, par.T_max)]
    in_float = [adiabatic((ab / mw).astype(np.float64), T) for T in (par.T_min, par.T_max)]
    assert min(abs(got / v - 1.) for v in in_double) < 1e-14
    assert min(abs(got / v - 1.) for v in in_float) > 1e-10  # the case can tell the two apart
