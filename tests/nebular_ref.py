"""References, metrics and dump readers shared by the nebular update_grid tests (tests/test_nebular_update_grid.py,
tests/test_gpu_nebular_update_grid.py) and the script that measures the reference's own noise floors
(tools/nebular_ref_floors.py).  No GPU here: numpy longdouble and mpmath only.

Tolerance rule of these tests: a compared quantity's bound is the larger of 10 x the oracle's own response (to a
one-ulp change of every float64 estimator input, or, for a solve, its error against a high-precision solution of its
own system) and a floor set by the number format -- one float32 ulp for float32 outputs, 1e-10 for doubles, 1e-12 of
the largest entry for matrix elements.  Nothing is taken from an engine-oracle difference.
"""
import functools
import os

import numpy as np

FIELDS = ("Te", "TR", "TJ", "W", "nne", "nnetot", "nt_frac_heating", "nt_frac_ionization", "nt_frac_excitation",
          "nt_nneperion_when_solved", "totalcooling", "bin_TR", "bin_W", "bfrate_estimator", "groundlevelpop",
          "partfunct", "nlte_pops", "cooling_contrib_ion", "rates", "nt_eff_ionpot", "nt_fracdep_ionization_ion",
          "nt_prob_num_auger", "nt_ionenfrac_num_auger", "nt_ionization_ratecoeff")
# One pass (nlteiter = 0) with a T_e interval that holds no root, by NlCall::pass (update_grid_host.h): what is
# written before the first k_nl_lu is a function of the caller's arrays alone -- k_nl_prepare (TR, TJ, W),
# k_nl_bfnorm (bfrate_estimator), k_nl_binfit (bin_TR, bin_W), the Spencer-Fano solve and analysis from the initial
# populations (nt_frac_*, nt_nneperion_when_solved, nt_eff_ionpot, nt_fracdep_ionization_ion, nt_prob_num_auger,
# nt_ionenfrac_num_auger), k_nl_ntrates (nt_ionization_ratecoeff = deposition / n_tot / eff_ionpot, n_tot from rho
# and the abundances), call_T_e_finder (Te: the interval's end point; rates: heating and cooling there).
BEFORE_LU = ("Te", "TR", "TJ", "W", "bin_TR", "bin_W", "bfrate_estimator", "nt_frac_heating", "nt_frac_ionization",
             "nt_frac_excitation", "nt_nneperion_when_solved", "nt_eff_ionpot", "nt_fracdep_ionization_ion",
             "nt_prob_num_auger", "nt_ionenfrac_num_auger", "nt_ionization_ratecoeff", "rates")
# ... and what k_nl_store and the final k_te_solve (cooling) write from the LU solution
AFTER_LU = ("nne", "nnetot", "groundlevelpop", "partfunct", "nlte_pops", "totalcooling", "cooling_contrib_ion")
assert sorted(BEFORE_LU + AFTER_LU) == sorted(FIELDS)

POP_ATOL = 1e-20  # cm^-3: populations (of 1e-3..1e6 totals) below this compare absolutely
F32_ULP = 1.2e-7  # type floors of the tolerance rule
F64_FLOOR = 1e-10
MATRIX_FLOOR = 1e-12
# the float64 estimator inputs of an NlteArrays block (the transport step's raw sums)
ESTIMATOR_INPUTS = ("J", "nuJ", "ffheating", "colheating", "bfrate_raw", "bin_J_raw", "bin_nuJ_raw")


def bound(response, dtype=np.float64):
    """The tolerance rule: max(10 x the reference's own response, the type floor)."""
    floor = F32_ULP if np.dtype(dtype) == np.float32 else F64_FLOOR
    return max(10. * response, floor)


def perturbed(arr, up):
    """A copy of an NlteArrays block with every float64 estimator input moved one ulp up (towards +inf) or down."""
    out = arr.copy()
    for name in ESTIMATOR_INPUTS:
        v = getattr(out, name)
        assert v.dtype == np.float64, name
        setattr(out, name, np.nextafter(v, np.inf if up else -np.inf))
    return out


def rel_diff(g, o, floor):
    g = np.asarray(g, dtype=np.float64)
    o = np.asarray(o, dtype=np.float64)
    both_nan = np.isnan(g) & np.isnan(o)
    d = np.abs(g - o) / np.maximum(np.maximum(np.abs(o), np.abs(g)), floor)
    d[both_nan] = 0.
    return float(np.nanmax(d, initial=0.)) if d.size else 0.


def report(ao, ag):
    """max relative difference per output (relative to max(|x|, floor): tiny populations compare absolutely); the -1
    "no NLTE solution" markers of nlte_pops must coincide"""
    out = {}
    for f in FIELDS:
        g, o = getattr(ag, f), getattr(ao, f)
        if f == "nlte_pops":
            mo = o < -0.9
            assert np.array_equal(mo, g < -0.9), "NLTE solution markers differ"
            g, o = g[~mo], o[~mo]
        floor = POP_ATOL if f in ("groundlevelpop", "nlte_pops") else 1e-300
        out[f] = rel_diff(g, o, floor)
    return out


def field_dtype(arr, f):
    return getattr(arr, f).dtype


def solve_report(model, ao, ag, cells, per_cell=False):
    """The AFTER_LU outputs on the scale the solve's error is measured on.  nltepop_matrix_solve's error is an L1
    error relative to the L1 norm of one element's solution, so a population far below its element's largest carries
    no relative accuracy: populations and per-ion cooling compare relative to the largest entry of the same element
    in the same cell and array, the partition function through the ion population it scales (groundlevelpop *
    partfunct / g_0); n_e, n_e,tot and the total cooling relative to themselves.  Every element of every cell is
    held to this by itself: a trace element is not measured against the dominant one.  An element absent from a
    cell (all zero in the oracle) must be absent in the other run.  The -1 markers of nlte_pops must coincide."""
    ni = model.nions_total
    cells = np.asarray(cells)
    f64 = lambda a, f, w: getattr(a, f).reshape(len(ao.Te), w)[cells].astype(np.float64)  # noqa: E731
    out = {}
    for f in ("nne", "nnetot", "totalcooling"):
        o, g = f64(ao, f, 1), f64(ag, f, 1)
        out[f] = np.abs(g - o)[:, 0] / np.maximum(np.abs(o)[:, 0], 1e-300)
    g0 = model.ion_ground_statweight().astype(np.float64)
    ion_el, slot_el = model.ion_element(), model.nlte_slot_element()
    rows = {"groundlevelpop": (f64(ao, "groundlevelpop", ni), f64(ag, "groundlevelpop", ni), ion_el),
            "partfunct": (f64(ao, "groundlevelpop", ni) * f64(ao, "partfunct", ni) / g0,
                          f64(ag, "groundlevelpop", ni) * f64(ag, "partfunct", ni) / g0, ion_el),
            "cooling_contrib_ion": (f64(ao, "cooling_contrib_ion", ni), f64(ag, "cooling_contrib_ion", ni), ion_el)}
    ntl = ao.nlte_pops.size // len(ao.Te)
    po, pg = f64(ao, "nlte_pops", ntl).copy(), f64(ag, "nlte_pops", ntl).copy()
    mo = po < -0.9
    assert np.array_equal(mo, pg < -0.9), "NLTE solution markers differ"
    po[mo] = pg[mo] = 0.
    rows["nlte_pops"] = (po, pg, slot_el)
    for f, (o, g, el) in rows.items():
        worst = np.zeros(len(cells))
        for e in range(model.nelements):
            sel = el == e
            if not sel.any():
                continue
            scale = np.abs(o[:, sel]).max(axis=1)
            diff = np.abs(g[:, sel] - o[:, sel]).max(axis=1)
            assert np.all(diff[scale == 0.] == 0.), (f, e, "present in one run only")
            worst = np.maximum(worst, diff / np.where(scale > 0., scale, 1.))
        out[f] = worst
    assert sorted(out) == sorted(AFTER_LU)
    return out if per_cell else {f: float(v.max(initial=0.)) for f, v in out.items()}


def ion_fractions(model, arr):
    """[npts_model, nions_total] each ion's share of its element's number density (ionstagepop, ltepop.cc:558-564)"""
    ni = model.nions_total
    g0 = model.ion_ground_statweight().astype(np.float64)
    pop = arr.groundlevelpop.reshape(-1, ni).astype(np.float64) * arr.partfunct.reshape(-1, ni) / g0
    el = model.ion_element()
    tot = np.zeros((pop.shape[0], model.nelements))
    for u in range(ni):
        tot[:, el[u]] += pop[:, u]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.nan_to_num(pop / tot[:, el])


PHYSICAL = ("Te", "TR", "TJ", "W", "nne", "nnetot", "totalcooling", "ion_fractions", "nt_frac_heating",
            "nt_frac_ionization", "nt_frac_excitation", "bin_TR", "rates")


def physical_report(model, ao, ag, cells):
    """The converged solution's aggregate differences over the listed cells: relative for the scalars, absolute for
    fractions, bin T_R relative over the fitted bins, rates relative to each cell's largest."""
    rel = lambda f: float(np.max(np.abs(getattr(ag, f)[cells].astype(np.float64) - getattr(ao, f)[cells]) /  # noqa: E731
                                np.maximum(np.abs(getattr(ao, f)[cells]), 1e-300)))
    rep = {f: rel(f) for f in ("Te", "TR", "TJ", "W", "nne", "nnetot", "totalcooling")}
    fo, fg = ion_fractions(model, ao)[cells], ion_fractions(model, ag)[cells]
    rep["ion_fractions"] = float(np.max(np.abs(fg - fo)))
    for f in ("nt_frac_heating", "nt_frac_ionization", "nt_frac_excitation"):
        rep[f] = float(np.max(np.abs(getattr(ag, f)[cells] - getattr(ao, f)[cells])))
    nb = model.radfield_nbins
    bo, bg = ao.bin_TR.reshape(-1, nb)[cells], ag.bin_TR.reshape(-1, nb)[cells]
    fit = bo > 0
    rep["bin_TR"] = float(np.max(np.abs(bg[fit] - bo[fit]) / bo[fit], initial=0.))
    rates_o, rates_g = ao.rates.reshape(-1, 8)[cells], ag.rates.reshape(-1, 8)[cells]
    scale = np.maximum(np.abs(rates_o).max(axis=1, keepdims=True), 1e-300)
    rep["rates"] = float(np.max(np.abs(rates_g - rates_o) / scale))
    return rep


# every PHYSICAL quantity is a float32 output or derived from float32 outputs, but totalcooling and rates (doubles)
PHYSICAL_DTYPE = {k: (np.float64 if k in ("totalcooling", "rates") else np.float32) for k in PHYSICAL}


# ------------------------------------------------------------------------------------------------ dump readers
def read_dump_gpu(path):
    """ARTIS_GPU_NL_DUMP <prefix>_p<pass>_gpu.bin: the first active cell's rate matrices of every element
    (column-major, concatenated), balance vectors, LTE normalisations, LU solutions; its level populations [nl],
    corrected photoionisation coefficients [ntargets]; the bf-heating levels (unique level index) with their
    coefficients."""
    with open(path, "rb") as f:
        ne, cell1, cell2, nl, ntg = (int(v) for v in np.frombuffer(f.read(20), np.int32))
        d = {"el_D": np.frombuffer(f.read(4 * ne), np.int32), "status": np.frombuffer(f.read(4 * ne), np.int32)}
        for k, n in (("A", cell2), ("b", cell1), ("norm", cell1), ("pv", cell1), ("pops", nl), ("corr", ntg)):
            d[k] = np.frombuffer(f.read(8 * n), np.float64)
        nhb = int(np.frombuffer(f.read(4), np.int32)[0])
        d["hb_ul"] = np.frombuffer(f.read(4 * nhb), np.int32)
        d["hbc"] = np.frombuffer(f.read(8 * nhb), np.float64)
        assert len(d["hbc"]) == nhb and f.read() == b""
    return d


def read_dump_oracle(path):
    """ORACLE_NL_DUMP <prefix>_p<pass>_ora_e<element>.bin: one element's normalised rate matrix (column-major), balance
    vector, LTE normalisation, solution, the matrix before normalisation, the cell's level populations and the
    corrected photoionisation coefficients this element read (-99: not read)."""
    with open(path, "rb") as f:
        D, status = (int(v) for v in np.frombuffer(f.read(8), np.int32))
        d = {"D": D, "status": status}
        for k, n in (("A", D * D), ("b", D), ("norm", D), ("pv", D), ("raw", D * D)):
            d[k] = np.frombuffer(f.read(8 * n), np.float64)
        nl, ntg = (int(v) for v in np.frombuffer(f.read(8), np.int32))
        d["pops"] = np.frombuffer(f.read(8 * nl), np.float64)
        d["corr"] = np.frombuffer(f.read(8 * ntg), np.float64)
        assert len(d["corr"]) == ntg and f.read() == b""
    return d


def read_dump_bfheat_oracle(path):
    """ORACLE_NL_DUMP <prefix>_bfheat_ora.bin: the first iterated cell's bf-heating coefficient of every level, and
    the lowest photoionisation edge frequency of the atomic data"""
    with open(path, "rb") as f:
        n = int(np.frombuffer(f.read(4), np.int32)[0])
        c = np.frombuffer(f.read(8 * n), np.float64)
        nu_edge_min = float(np.frombuffer(f.read(8), np.float64)[0])
        assert len(c) == n and f.read() == b""
    return c, nu_edge_min


def bins_read_difference(model, ao, ag, cell, nu_edge_min):
    """How far the fitted radiation field J_nu = W_b B_nu(T_b) of two runs can differ, relatively, at any frequency
    an integral from a photoionisation edge upwards reads: over the bins reaching above the lowest edge,
    |dW / W| + (x + 1) |dT / T| with x = h nu_upper / k T (d ln B_nu / d ln T = x e^x / (e^x - 1) <= x + 1).
    0 where the two runs fitted identical bins."""
    nb = model.radfield_nbins
    worst = 0.
    for b, (lo, hi) in enumerate(bin_edges(model)):
        if hi <= nu_edge_min:
            continue
        To, Tg = float(ao.bin_TR[cell * nb + b]), float(ag.bin_TR[cell * nb + b])
        Wo, Wg = float(ao.bin_W[cell * nb + b]), float(ag.bin_W[cell * nb + b])
        if (To, Wo) == (Tg, Wg):
            continue
        assert To > 0. and Tg > 0. and Wo > 0. and Wg > 0., (b, To, Tg, Wo, Wg)  # the same outcome class
        x = HOVERKB * hi / min(To, Tg)
        worst = max(worst, abs(Wg - Wo) / Wo + (x + 1.) * abs(Tg - To) / To)
    return worst


def read_dump_sf(path, column_major):
    """<prefix>_sf_gpu.bin (column-major) / <prefix>_sf_ora.bin (row-major): the first Spencer-Fano solve's matrix
    as M[row, column], its right-hand side and the kept solution.  The engine neither writes nor reads the strictly
    lower part of its matrix (k_sf_matrix returns for i > j; the solves and residuals run over j >= i): what the
    dump holds there is whatever the buffer held before, and is dropped here."""
    with open(path, "rb") as f:
        n, mgi = (int(v) for v in np.frombuffer(f.read(8), np.int32))
        M = np.frombuffer(f.read(8 * n * n), np.float64).reshape(n, n)
        rhs = np.frombuffer(f.read(8 * n), np.float64)
        y = np.frombuffer(f.read(8 * n), np.float64)
        assert len(y) == n and f.read() == b""
    return mgi, (np.triu(M.T) if column_major else M), rhs, y


# ------------------------------------------------------------------------------------- high-precision references
def backsub_longdouble(U, b):
    """U x = b for an upper-triangular U[row, column], plain row-oriented back substitution in np.longdouble"""
    U = np.asarray(U, dtype=np.longdouble)
    n = len(b)
    x = np.zeros(n, dtype=np.longdouble)
    bl = np.asarray(b, dtype=np.longdouble)
    for i in range(n - 1, -1, -1):
        x[i] = (bl[i] - U[i, i + 1:] @ x[i + 1:]) / U[i, i]
    return x


def sf_solution_error(U, b, y):
    """max |y - x| / max |x| against the longdouble back substitution x of the same system"""
    assert np.all(np.tril(U, -1) == 0.), "the Spencer-Fano matrix is upper triangular"
    x = backsub_longdouble(U, b)
    return float(np.max(np.abs(np.asarray(y, dtype=np.longdouble) - x)) / np.max(np.abs(x)))


def sf_matrix_error(Mg, Mo):
    """max over elements of |Mg - Mo| relative to the largest entry of the element's row in Mo"""
    scale = np.maximum(np.abs(Mo).max(axis=1, keepdims=True), 1e-300)
    return float((np.abs(Mg - Mo) / scale).max())


def lu_solution_error(A, b, norm, pv, dps=40):
    """L1 error of a rate-matrix solution pv (populations: x * norm, nltepop.cc:770-790) against the mpmath solve of
    the same normalised system A x = b (A[row, column]), relative to the L1 norm of that solution"""
    import mpmath

    with mpmath.workdps(dps):
        x = mpmath.lu_solve(mpmath.matrix(A.tolist()), mpmath.matrix(b.tolist()))
        ref = [x[k] * mpmath.mpf(float(norm[k])) for k in range(len(b))]
        err = sum(abs(mpmath.mpf(float(pv[k])) - ref[k]) for k in range(len(b)))
        return float(err / sum(abs(r) for r in ref)), np.array([float(r) for r in ref])


# -------------------------------------------------------------------------- Planck integrals over a frequency bin
TWOHOVERCLIGHTSQUARED, HOVERKB = 1.4745007e-47, 4.799243681748932e-11  # the reference's constants (constants.h)


def planck_mp(T, nu1, nu2, times_nu=False, dps=30):
    return _planck_mp(float(T), float(nu1), float(nu2), bool(times_nu), dps)


def _bose_tail(x, p, mp):
    """int_x^inf t^p / (e^t - 1) dt = sum_k e^(-k x) sum_j p! / (p - j)! x^(p - j) / k^(j + 1), to the working
    precision"""
    coef, c = [], mp.mpf(1)
    for j in range(p + 1):  # p! / (p - j)! x^(p - j)
        coef.append(c * x ** (p - j))
        c *= p - j
    ex = mp.exp(-x)
    ek, total, k = mp.mpf(1), mp.mpf(0), 0
    eps = mp.mpf(10) ** (-mp.mp.dps - 2)
    while True:
        k += 1
        ek *= ex
        kk, inner = mp.mpf(k), mp.mpf(0)
        for j in range(p + 1):
            inner += coef[j] / kk ** (j + 1)
        term = ek * inner
        total += term
        if term <= eps * total:
            return total


@functools.lru_cache(maxsize=None)
def _planck_mp(T, nu1, nu2, times_nu, dps):
    """int_nu1^nu2 2h/c^2 nu^3 (nu) / (exp(h nu / kT) - 1) dnu from the exponential series of the Bose integral, the
    difference tail(x1) - tail(x2) taken with 15 guard digits (it cancels on the Rayleigh-Jeans side); with the
    reference's constants.  No quadrature: mpmath's tanh-sinh rule under-resolves a panel across which the Wien tail
    falls by e^-30 (1e-5 off at h nu / kT > 200)."""
    import mpmath

    with mpmath.workdps(dps + 15):
        T, nu1, nu2 = mpmath.mpf(T), mpmath.mpf(nu1), mpmath.mpf(nu2)
        hk, pre = mpmath.mpf(HOVERKB), mpmath.mpf(TWOHOVERCLIGHTSQUARED)
        p = 4 if times_nu else 3
        val = pre * (T / hk) ** (p + 1) * (_bose_tail(hk * nu1 / T, p, mpmath) - _bose_tail(hk * nu2 / T, p, mpmath))
    with mpmath.workdps(dps):
        return +val


def planck_mean_nu_residual(T, nu1, nu2, nu_bar, dps=30):
    """delta_nu_bar (radfield.cc:1020-1066) in mpmath, as a float"""
    import mpmath

    with mpmath.workdps(dps):
        return float(planck_mp(T, nu1, nu2, True, dps) / planck_mp(T, nu1, nu2, False, dps) - mpmath.mpf(float(nu_bar)))


def golden(*parts):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", *parts)


# ------------------------------------------------------------------------------------ synthetic radiation-field bins
T_R_MAX = 250000.
SYNTH_BIN_CASES = ((12, 500.), (12, 50.), (4, 500.), (4, 50.))  # (radfield_nbins, T_R_min)
ROOT_RTOL = 1.5e-4  # find_T_R's Brent loop stops at a bracket of relative width 1e-4 that holds the true root and the
#                     returned one; the float32 store adds 6e-8


def bin_edges(model):
    """[(nu_lower, nu_upper)] of the model's radiation-field bins (radfield.cc:292-330; model_synth.cc)"""
    nb = model.radfield_nbins
    lo, hi = 2.99792458e+10 / 40000e-8, 2.99792458e+10 / 1085e-8
    dnu = (hi - lo) / (nb - 1)
    up = [lo + (b + 1) * dnu for b in range(nb - 1)] + [2.99792458e+10 / 10e-8]
    return [(lo if b == 0 else up[b - 1], up[b]) for b in range(nb)]


class SyntheticBins:
    """Bin estimators with known answers for one (radfield_nbins, T_R_min): Planck spectra (mpmath, 30 digits) below
    T_R_min, at 1.7 T_R_min, 5000, 40000, 240000 K and above T_R_max, an empty bin, a bin whose fitted W exceeds 1e4
    but not at T_R_max, and one that ends as -99 / 0 -- one kind per (cell, bin) over the bins whose integrals do not
    underflow at T_R_min, plus cell 0's last bin (T_R = T_e).  J is scaled so that the stored float32 W is 1e-2
    (1 for the T_R_max fallback)."""

    def __init__(self, est_fn, nbins, T_R_min):
        from artis_amd import ffi
        from artis_amd.model import Model

        self.model = m = Model(**{**NEB, "radfield_nbins": nbins})
        assert m.radfield_nbins == nbins
        nts = 5
        self.params = p = ffi.RunParams.from_buffer_copy(m.params)
        p.first_nlte_radfield_timestep = 12  # the rate matrices and heating integrals do not read the bins
        p.detailed_bf_usefromtimestep = 13
        est = est_fn(m, p, nts - 1, 2000, 7)
        m.set_timestep(nts)
        self.nt = ffi.NtDataHandle(m, sfpts=48, sf_emax=500.)
        self.arr = arr = ffi.NlteArrays(m, nts, est=est, seed=11)
        arr.params.num_lte_timesteps = 8  # the non-thermal skip path
        arr.params.T_R_min = T_R_min
        pin_one_pass(arr)
        self.T_R_min = T_R_min
        self.edges = edges = bin_edges(m)
        valid = [b for b in range(nbins - 1) if float(planck_mp(T_R_min, *edges[b])) > 1e-290]
        kinds = [("planck", 0.6 * T_R_min), ("planck", 1.7 * T_R_min), ("planck", 5000.), ("planck", 40000.),
                 ("planck", 240000.), ("planck", 1.6 * T_R_MAX), ("empty", 0.), ("fallback", 1.7 * T_R_min),
                 ("minus99", 5000.)]
        ncell = -(-len(kinds) // len(valid))
        arr.mgi_list = arr.mgi_list[:ncell].copy()
        self.cells = cells = [int(c) for c in arr.mgi_list]
        arr.bin_J_raw[:] = 0.
        arr.bin_nuJ_raw[:] = 0.
        arr.bin_contribcount[:] = 0
        slots = [(c, b) for c in cells for b in valid][:len(kinds)]
        self.bins = {}  # (cell, bin) -> (kind, shape temperature, J_bin)
        for (c, b), (kind, T) in zip(slots, kinds):
            if kind == "empty":
                self.bins[(c, b)] = (kind, T, 0.)
                continue
            lo, hi = edges[b]
            p_shape = planck_mp(T, lo, hi)
            if float(p_shape) < 1e-290:  # the double-precision integral underflows: not a case
                continue
            nu_bar = planck_mp(T, lo, hi, True) / p_shape
            if kind == "planck":
                J = 1e-2 * planck_mp(min(max(T, T_R_min), T_R_MAX), lo, hi)
            else:
                p_max = planck_mp(T_R_MAX, lo, hi)
                # W at the fitted T_R is far above 1e4: J / P(T_R) = p_max / p_shape, or 1e6 times that
                assert p_max / p_shape > (1e6 if kind == "fallback" else 1.), (b, T)
                J = (1. if kind == "fallback" else 1e6) * p_max
            self._set(c, b, float(J), float(J * nu_bar))
            self.bins[(c, b)] = (kind, T, float(J))
        c, b = cells[0], nbins - 1  # the last bin takes T_e whatever its fit gives
        J = 1e-2 * planck_mp(float(arr.Te[c]), *edges[b])
        self._set(c, b, float(J), float(J * planck_mp(20000., *edges[b], True) / planck_mp(20000., *edges[b])))
        self.bins[(c, b)] = ("last", 20000., float(J))

    def _set(self, c, b, J_bin, nuJ_bin):
        a, nb = self.arr, self.model.radfield_nbins
        # radfield.cc:1177-1190: J_bin = raw / (4 pi dV dt nprocs)
        normfactor = 1. / (4. * np.pi) / (a.vol_init[c] * a.params.tratmid ** 3) / a.params.deltat / a.params.nprocs
        a.bin_J_raw[c * nb + b] = J_bin / normfactor
        a.bin_nuJ_raw[c * nb + b] = nuJ_bin / normfactor
        a.bin_contribcount[c * nb + b] = 7

    def outcome(self, sol, c, b):
        """the outcome class of a fitted bin: 'empty', 'minus99', 'min', 'max', 'Te' or 'root'"""
        nb = self.model.radfield_nbins
        T, W = float(sol.bin_TR[c * nb + b]), float(sol.bin_W[c * nb + b])
        if T == 0.:
            assert W == 0.
            return "empty"
        if T == -99.:
            assert W == 0.
            return "minus99"
        assert W > 0. and np.isfinite(W), (c, b, T, W)
        if b == nb - 1:
            assert T == self.arr.Te[c]  # the T_e the call started from (fit_parameters runs before the T_e finder)
            return "Te"
        if T == np.float32(self.T_R_min):
            return "min"
        if T == np.float32(T_R_MAX):
            return "max"
        assert self.T_R_min < T < T_R_MAX
        return "root"

    def check(self, sol, who):
        """The mpmath checks of one side's fit; returns (number of root bins, spread of W P(T_R) / J_bin)."""
        nb = self.model.radfield_nbins
        nroot, ratio = 0, []
        for (c, b), (kind, T, J) in self.bins.items():
            cls = self.outcome(sol, c, b)
            lo, hi = self.edges[b]
            Ts, Ws = float(sol.bin_TR[c * nb + b]), float(sol.bin_W[c * nb + b])
            if cls == "root":
                nu_bar = self.arr.bin_nuJ_raw[c * nb + b] / self.arr.bin_J_raw[c * nb + b]
                r_lo = planck_mean_nu_residual(Ts * (1. - ROOT_RTOL), lo, hi, nu_bar)
                r_hi = planck_mean_nu_residual(Ts * (1. + ROOT_RTOL), lo, hi, nu_bar)
                assert r_lo < 0. < r_hi, (who, c, b, kind, T, Ts, r_lo, r_hi)
                nroot += 1
            if Ws > 0.:
                ratio.append(Ws * float(planck_mp(Ts, lo, hi)) / J)
        ratio = np.array(ratio)
        return nroot, float(np.max(np.abs(ratio / np.median(ratio) - 1.)))

    def expected(self):
        """What the construction implies for the kinds whose class does not depend on the solver's accuracy."""
        return {"empty": "empty", "fallback": "max", "minus99": "minus99", "last": "Te"}


# ------------------------------------------------------------------------------------------------------- cases
# est_fn(model, params, nts_prev, npkts, seed) -> the raw estimators of one transport step: the engine's in the GPU
# tests, the oracle's (oracle_estimators) where the reference's floors are measured without a GPU
ONEZONE = dict(ngrid_1d=10, nlevels_per_ion=30, n_ionising=10, max_lines=2000, nebular=1, nlte_level_max=12,
               ionpot_scale=0.5)
NEB = dict(ngrid_1d=6, nlevels_per_ion=30, n_ionising=10, max_lines=2000, ntstep=20, nebular=1, nlte_level_max=12,
           tmin_days=100., tmax_days=300., T0=6000., ionpot_scale=0.5)
SF_SHAPES = ((48, 500.), (200, 2000.), (1100, 16000.))  # (sfpts, sf_emax): n < 64; n < 256, partial 64-block;
#                                            n > 1024, partial 64-block, five residual chunks, the strided loops


def oracle_estimators(model, params, nts_prev, npkts, seed):
    import oracle_lib

    model.set_timestep(nts_prev)
    est, _ = oracle_lib.update_packets(model, nts_prev, model.init_rpackets(nts_prev, npkts, seed=seed), nthreads=16,
                                       params=params)
    return est


def onezone_model(**overrides):
    from artis_amd.model import Model

    ref = golden("ref_inputs", "nebularonezone")
    return Model(files=(os.path.join(ref, "input-newrun.txt"), os.path.join(ref, "model.txt"),
                        os.path.join(ref, "abundances.txt")), **{**ONEZONE, **overrides})


def pin_one_pass(arr):
    """One pass, no T_e root: every output is a fixed function of the inputs."""
    arr.params.nlteiter = 0
    arr.params.T_min, arr.params.T_max = 15000., 15001.


def onezone_case(est_fn, first_rf, pinned, sfpts=4096, sf_emax=16000., one_pass=False, npkts=20000):
    """The nebularonezone reference model at timestep 6 (NUM_LTE_TIMESTEPS 4) from a transport step's estimators."""
    from artis_amd import ffi

    m = onezone_model()
    nts = 6
    p = ffi.RunParams.from_buffer_copy(m.params)
    p.first_nlte_radfield_timestep = first_rf
    p.detailed_bf_usefromtimestep = first_rf + 1
    est = est_fn(m, p, nts - 1, npkts, 5)
    m.set_timestep(nts)
    nt = ffi.NtDataHandle(m, sfpts=sfpts, sf_emax=sf_emax)
    arr = ffi.NlteArrays(m, nts, est=est, dep_scale=3e-4)
    arr.params.num_lte_timesteps = 4
    if pinned:
        arr.params.T_min, arr.params.T_max = 15000., 15001.
    if one_pass:
        pin_one_pass(arr)
    return m, p, nt, arr, nts


def multicell_sf_case(est_fn, sfpts):
    """The 6-shell synthetic nebular model at timestep 12 (NUM_LTE_TIMESTEPS 2: every iterated cell solves the
    Spencer-Fano equation), a third of the cells thick (the LTE branch), one pass at a pinned T_e."""
    from artis_amd import ffi
    from artis_amd.model import Model

    m = Model(**NEB)
    nts = 12
    p = ffi.RunParams.from_buffer_copy(m.params)
    est = est_fn(m, p, nts - 1, 8000, 8)
    m.set_timestep(nts)
    nt = ffi.NtDataHandle(m, sfpts=sfpts)
    arr = ffi.NlteArrays(m, nts, est=est, seed=12, thick_frac=0.35)
    arr.params.num_lte_timesteps = 2
    pin_one_pass(arr)
    return m, p, nt, arr, nts
