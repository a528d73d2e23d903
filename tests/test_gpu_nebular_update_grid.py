"""update_grid for the nebular options on the GPU (artis_gpu_update_grid_nlte, nlte_solver.h) against the oracle's
restatement (oracle/nebular_update_grid.cc).  Needs an MI355X.

Per listed cell: the radiation-field fits (radfield.cc:1136-1291), the NO_LUT bf-heating coefficients, the
Spencer-Fano solution and its analysis (nonthermal.cc:1996-2713), call_T_e_finder, the NLTE rate matrices with
their LU solve and refinement (nltepop.cc:421-1113), the convergence loop of solve_Te_nltepops
(update_grid.cc:763-886) and the cooling rates.  Both sides read the same raw estimators (a GPU transport step of
the same model).  Integer outputs (pass counts, solved-timestep marks, the -1 "no NLTE solution" markers) must be
identical; the two sides differ only by last-bit differences of the device libm, amplified by the iterative solves
(Brent, LU refinement), so every floating-point bound is derived from the oracle's own noise floor (the constants
below; tests/nebular_ref.py states the rule).  The one-pass tests assert every output, the Spencer-Fano kernels at
grid sizes that are no multiple of their tiles, the bin fits on synthetic bins against 30-digit integrals and the LU
solve against a 40-digit one; the converged tests compare the physics of the whole loop.
"""
import functools
import os

import numpy as np
import pytest

import nebular_ref as nr
import oracle_lib
import parity
from artis_amd import Engine, EngineError, ffi
from artis_amd.model import Model
from nebular_ref import FIELDS, NEB

pytestmark = pytest.mark.gpu

# The reference's own noise floors, measured on the CPU by tools/nebular_ref_floors.py (the largest of four runs): the
# oracle's response to a one-ulp change, up or down, of every float64 estimator input, per compared quantity, and the
# error of its solves against high-precision solutions of its own systems.  Every bound below is nebular_ref.bound of
# one of these -- 10 x the figure, or the type floor (1.2e-7 float32, 1e-10 double) -- never an engine-oracle
# difference.
# tools/nebular_ref_floors.py: one pass at a pinned T_e (one zone first_rf 12 / 4, sfpts 48 / 200 / 1100; multicell
# sfpts 200 / 1100), element by element (nebular_ref.report); every other BEFORE_LU output is bit-identical
ONEPASS_RESPONSE = {"bin_TR": 9.7e-05, "bin_W": 1.6e-03, "rates": 3.9e-16}
# tools/nebular_ref_floors.py: the same runs, AFTER_LU outputs on the solve's scale (nebular_ref.solve_report)
ONEPASS_SOLVE_RESPONSE = {"nne": 0., "nnetot": 0., "totalcooling": 4.1e-10, "groundlevelpop": 1.7e-22,
                          "partfunct": 4.7e-21, "cooling_contrib_ion": 7.2e-10, "nlte_pops": 2.4e-09}
# tools/nebular_ref_floors.py: the oracle's Spencer-Fano solution against a longdouble back substitution of its own
# matrix (max-norm, sfpts 48 / 200 / 1100), its rate-matrix LU solutions against a 40-digit solve of its own systems
# (L1, the worst of the one-zone elements: populations spanning 40 decades)
SF_SOLVE_ERROR = 1.4e-15
LU_SOLVE_ERROR = 1.9e-06
# tools/nebular_ref_floors.py: the dumped level populations the first rate matrix is built from (the state before any
# solve), the corrected photoionisation coefficients and the bf-heating coefficients: all bit-identical
DUMP_RESPONSE = {"pops": 0., "corr": 0., "hbc": 0.}
# tools/nebular_ref_floors.py: the converged one-zone cases (nebular_ref.physical_report) with a pinned T_e interval
# (2 passes) and with the full one (4 passes).  Only what no LU solve precedes is listed: the response of everything
# computed from the populations (at most 2.2e-10) is below those cases' solve errors further down.
PINNED_RESPONSE = {"bin_TR": 8.2e-05}
FREE_RESPONSE = {"bin_TR": 9.3e-05}
# tools/nebular_ref_floors.py (nebular_ref.SyntheticBins.check): the spread of W P(T_R) / J_bin over the oracle's
# fitted synthetic bins, the same 2.2e-8 in all four cases (the float32 rounding of W)
BIN_W_SPREAD = 2.2e-08
# tools/nebular_ref_floors.py: the same error over every pass of the converged one-zone cases (first_rf 12 / 4, the
# estimator inputs as given and one ulp up and down).  Later passes meet far worse systems than the first: the
# heaviest element's second-pass matrix has a condition number of 1.7e17.
PINNED_LU_SOLVE_ERROR = 6.1e-03
FREE_LU_SOLVE_ERROR = 7.9e-04
# tools/nebular_ref_floors.py: the converged cases of the 6-shell model (136 cells with an LTE branch; the 17-cell
# subset with Spencer-Fano solutions; up to 6 passes) measured by themselves -- the response as above (everything
# but bin T_R at most 1e-26) and the solve error over the passes of the first two iterated cells of each case, solved
# one at a time.  This model's matrices are well conditioned: its bounds are the type floors.
MULTICELL_RESPONSE = {"bin_TR": 9.3e-05}
MULTICELL_LU_SOLVE_ERROR = 1.6e-16
# what follows an LU solve inherits that solve's error: no output computed from the populations can be asked to agree
# better than the reference's own solution agrees with the exact one
SOLVE_BOUND = nr.bound(LU_SOLVE_ERROR)
# the single tolerance the converged tests had before their per-quantity bounds: no bound may exceed it
FORMER_AGG_TOL = 2e-2
# not downstream of any LU solve, whatever the number of passes
NOT_SOLVED = ("TR", "TJ", "W", "bin_TR", "nnetot")


def _estimators(model, params, nts_prev, npkts, seed):
    """The raw estimators of one GPU transport step at nts_prev."""
    eng = Engine(model, params=params)
    try:
        model.set_timestep(nts_prev)
        eng.upload_cellstate(nts_prev)
        pk = model.init_rpackets(nts_prev, npkts, seed=seed)
        return eng.update_packets(nts_prev, pk)
    finally:
        eng.close()


def _solve_both(model, params, arr, nt):
    """The same NlteArrays block through the oracle and the engine; returns (oracle, gpu, ms)."""
    ao, ag = arr.copy(), arr.copy()
    rc = oracle_lib.update_grid_nlte(model, nt, ao, params=params, nthreads=16)
    assert rc == 0, f"oracle update_grid_nlte -> {rc}"
    eng = Engine(model, params=params)
    try:
        ms = eng.update_grid_nlte(nt, ag)
    finally:
        eng.close()
    return ao, ag, ms


def _compare(model, ao, ag, cells):
    """Every output of a one-pass, T_e-pinned call -- a fixed function of the inputs.  Pass counts and solved-timestep
    marks exactly; the BEFORE_LU outputs element by element, the AFTER_LU outputs on the solve's scale -- every
    chemical element of every cell relative to its own largest entry (nebular_ref.solve_report) -- each against the
    bound its measured floor gives.  Figures are printed first."""
    rep = nr.report(ao, ag)
    print("  element by element, for the record: " + ", ".join(f"{k} {rep[k]:.1e}" for k in nr.AFTER_LU))
    rep.update(nr.solve_report(model, ao, ag, cells))
    tol = {}
    for f in FIELDS:
        dt = nr.field_dtype(ag, f)
        if f in nr.BEFORE_LU:
            tol[f] = nr.bound(ONEPASS_RESPONSE.get(f, 0.), dt)
        else:
            tol[f] = max(nr.bound(ONEPASS_SOLVE_RESPONSE[f], dt), SOLVE_BOUND)
    print("  max diff (bound): " + ", ".join(f"{k} {rep[k]:.1e} ({tol[k]:.1e})" for k in FIELDS))
    assert np.array_equal(ag.iters, ao.iters), (ag.iters[cells], ao.iters[cells])
    assert np.array_equal(ag.nt_timestep_last_solved, ao.nt_timestep_last_solved)
    bad = {k: (rep[k], tol[k]) for k in FIELDS if not rep[k] <= tol[k]}
    for k in bad:  # the worst element of each, with both values
        g, o = getattr(ag, k).astype(np.float64), getattr(ao, k).astype(np.float64)
        q = int(np.nanargmax(np.abs(g - o) / np.maximum(np.maximum(np.abs(g), np.abs(o)), 1e-300)))
        print(f"  {k}[{q}] (row length {g.size // len(ag.Te)}): gpu {g[q]!r}, oracle {o[q]!r}")
    assert not bad, f"outside tolerance (difference, bound): {bad}"


def _compare_physical(model, ao, ag, cells, te_rtol, response, solve_error, equal_passes):
    """The converged solution: T_e to the solver accuracy; per quantity the bound its measured floor gives
    (response: PINNED_, FREE_ or MULTICELL_RESPONSE), and for everything computed from LU-solved populations the bound
    the oracle's worst solve error over the passes gives (solve_error: the case's *_LU_SOLVE_ERROR); never more
    than the former 2e-2.  Pass counts equal where T_e is pinned, within one otherwise."""
    rep = nr.physical_report(model, ao, ag, cells)
    tol = {}
    for k in nr.PHYSICAL:
        tol[k] = nr.bound(response.get(k, 0.), nr.PHYSICAL_DTYPE[k])
        if k not in NOT_SOLVED:
            tol[k] = max(tol[k], nr.bound(solve_error))
        tol[k] = min(tol[k], FORMER_AGG_TOL)
    tol["Te"] = te_rtol
    print("  physical max diff (bound): " + ", ".join(f"{k} {v:.1e} ({tol[k]:.1e})" for k, v in rep.items()))
    if equal_passes:
        assert np.array_equal(ag.iters[cells], ao.iters[cells]), (ag.iters[cells], ao.iters[cells])
    else:
        assert np.all(np.abs(ag.iters[cells] - ao.iters[cells]) <= 1), (ag.iters[cells], ao.iters[cells])
    bad = {k: (v, tol[k]) for k, v in rep.items() if not v <= tol[k]}
    assert not bad, f"outside tolerance (difference, bound): {bad}"


def _onezone_case(first_rf, pinned, **kw):
    return nr.onezone_case(_estimators, first_rf, pinned, **kw)


def _dumped(monkeypatch, tmp_path):
    prefix = str(tmp_path / "nl")
    monkeypatch.setenv("ARTIS_GPU_NL_DUMP", prefix)
    monkeypatch.setenv("ORACLE_NL_DUMP", prefix)
    return prefix


# ------------------------------------------------------------------------------- one pass: every output
@pytest.mark.parametrize("first_rf", [12, 4])
def test_one_pass_every_output_onezone(first_rf):
    """One pass (nlteiter 0) of the one-zone model with a T_e interval that holds no root, sfpts 1100: every name in
    FIELDS against the oracle (_compare).  first_rf = 4: the bf-heating integrals, the corrected photoionisation
    coefficients and the rate matrices read the fitted bins."""
    m, p, nt, arr, nts = _onezone_case(first_rf, True, sfpts=1100, one_pass=True)
    ao, ag, ms = _solve_both(m, p, arr, nt)
    cells = arr.mgi_list
    print(f"one pass, one zone, first_rf={first_rf}: gpu {ms:.1f} ms")
    assert (ao.iters[cells] == 1).all() and (ao.nt_timestep_last_solved[cells] == nts).all()
    assert (ao.nlte_pops > -0.9).any() and (ao.bin_W > 0).any() and (ao.nt_eff_ionpot > 0).any()
    _compare(m, ao, ag, cells)


@functools.lru_cache(maxsize=None)
def _multicell_sf_case(sfpts):
    return nr.multicell_sf_case(_estimators, sfpts)


def test_one_pass_every_output_multicell():
    """One pass of the 6-shell model at a pinned T_e, sfpts 1100: every non-empty cell, a third of them in the LTE
    branch, the others each with a Spencer-Fano solution; every name in FIELDS (_compare)."""
    m, p, nt, arr, nts = _multicell_sf_case(1100)
    ao, ag, ms = _solve_both(m, p, arr, nt)
    cells = arr.mgi_list
    thick = arr.thick[cells] == 1
    print(f"one pass, multicell: gpu {ms:.1f} ms for {len(cells)} cells")
    assert (ao.iters[cells][thick] == 0).all() and (ao.iters[cells][~thick] == 1).all()
    assert (ao.nt_timestep_last_solved[cells][~thick] == nts).all()
    _compare(m, ao, ag, cells)


# ------------------------------------------------------------------------------- Spencer-Fano at small shapes
@pytest.mark.parametrize("sfpts,sf_emax", nr.SF_SHAPES)
def test_spencer_fano_small_grids(sfpts, sf_emax, tmp_path, monkeypatch):
    """The Spencer-Fano kernels away from SFPTS = 4096: n < 64 (one partial tile in k_sf_backsub); n < 256 with a
    partial 64-block (one residual chunk, k_sf_best below its stride); n > 1024 with a partial 64-block, five residual
    chunks and the strided loops of k_sf_backsub and k_sf_best.  The matrix of the dumped solve: every element within
    1e-12 of the largest entry of its row of the oracle's.  The kept solution: against a longdouble back substitution
    of the engine's own matrix, to the bound the oracle's own error gives.  Every output as in _compare."""
    prefix = _dumped(monkeypatch, tmp_path)
    m, p, nt, arr, nts = _onezone_case(12, True, sfpts=sfpts, sf_emax=sf_emax, one_pass=True)
    ao, ag, ms = _solve_both(m, p, arr, nt)
    cells = arr.mgi_list
    cg, Mg, rg, yg = nr.read_dump_sf(prefix + "_sf_gpu.bin", column_major=True)
    co, Mo, ro, yo = nr.read_dump_sf(prefix + "_sf_ora.bin", column_major=False)
    assert cg == co == cells[0] and Mg.shape == Mo.shape == (sfpts, sfpts)
    merr = nr.sf_matrix_error(Mg, Mo)
    serr = nr.sf_solution_error(Mg, rg, yg)
    print(f"sfpts {sfpts}: gpu {ms:.1f} ms, matrix {merr:.1e}, solution vs longdouble {serr:.1e}, "
          f"vs oracle {np.max(np.abs(yg - yo)) / np.max(np.abs(yo)):.1e}, f_heat {ag.nt_frac_heating[cells]}")
    assert np.array_equal(rg, ro)
    assert merr <= nr.MATRIX_FLOOR, merr
    assert serr <= nr.bound(SF_SOLVE_ERROR), serr
    c = int(cells[0])
    prob = ag.nt_prob_num_auger.reshape(m.npts_model, m.nions_total, ffi.NT_MAX_AUGER + 1)[c]
    psum = prob.sum(axis=1)
    assert np.all((np.abs(psum - 1.) < 1e-6) | (psum == 0.)), psum
    assert 0.9999 < ag.nt_frac_heating[c] < 1.
    _compare(m, ao, ag, cells)


def test_spencer_fano_batch_tail(monkeypatch):
    """The multicell model at sfpts 200 with a Spencer-Fano batch of one cell (ARTIS_GPU_SF_BATCH_GB below two
    matrices): the batch loop's tail runs for every cell.  Byte-identical to the default batch (all cells at once) of
    the same engine, and against the oracle as in _compare."""
    m, p, nt, arr, nts = _multicell_sf_case(200)
    ao, ag, ms = _solve_both(m, p, arr, nt)
    nsolved = int((ao.nt_timestep_last_solved[arr.mgi_list] == nts).sum())
    # the default batch (8 GiB of 8 * sfpts^2-byte matrices) held every solved cell at once, the small one holds one
    assert 1 < nsolved <= 8 * 2 ** 30 // (8 * 200 * 200) and "ARTIS_GPU_SF_BATCH_GB" not in os.environ
    monkeypatch.setenv("ARTIS_GPU_SF_BATCH_GB", repr(1.5 * 8 * 200 * 200 / 2 ** 30))
    eng = Engine(m, params=p)
    try:
        a1 = arr.copy()
        ms1 = eng.update_grid_nlte(nt, a1)
    finally:
        eng.close()
    print(f"batch of one: gpu {ms1:.1f} ms (all at once {ms:.1f} ms) for {len(arr.mgi_list)} cells")
    for f in FIELDS + ("iters", "nt_timestep_last_solved"):
        assert getattr(a1, f).tobytes() == getattr(ag, f).tobytes(), f
    _compare(m, ao, a1, arr.mgi_list)


# ------------------------------------------------------------------------------- bin fits on synthetic bins
@pytest.mark.parametrize("nbins,T_R_min", nr.SYNTH_BIN_CASES)
def test_bin_fits_synthetic(nbins, T_R_min):
    """k_nl_binfit on bins with known answers (nebular_ref.SyntheticBins): every outcome class -- 0, -99, T_R_min,
    T_R_max (clamped, and the W > 1e4 fallback), T_e in the last bin, a Brent root -- equals the oracle's; around
    every root the 30-digit mean-frequency residual changes sign within 1.5e-4; W P(T_R) / J_bin is the same for
    every bin to the bound the oracle's own spread gives.  At 4 bins and T_R_min 50 K a bin is wider than 800 kT/h:
    nl_planck_integral's panel loop with its 40-panel cap, the cut-off and the early break (deviation D14; the oracle
    integrates with qag)."""
    sb = nr.SyntheticBins(_estimators, nbins, T_R_min)
    ao, ag, ms = _solve_both(sb.model, sb.params, sb.arr, sb.nt)
    classes = {}
    for (c, b), (kind, T, J) in sb.bins.items():
        co, cg = sb.outcome(ao, c, b), sb.outcome(ag, c, b)
        print(f"  cell {c} bin {b} {kind} {T:g} K: oracle {ao.bin_TR[c * nbins + b]!r} {ao.bin_W[c * nbins + b]!r}, "
              f"gpu {ag.bin_TR[c * nbins + b]!r} {ag.bin_W[c * nbins + b]!r}")
        assert cg == co, (c, b, kind, cg, co)
        assert co == sb.expected().get(kind, co), (c, b, kind, co)
        classes[co] = classes.get(co, 0) + 1
    assert set(classes) == {"empty", "minus99", "min", "max", "Te", "root"} and classes["root"] >= 4, classes
    nroot, spread = sb.check(ag, "gpu")
    print(f"bins {nbins}, T_R_min {T_R_min}: {classes}, spread of W P / J {spread:.1e}")
    assert nroot == classes["root"]
    assert spread <= nr.bound(BIN_W_SPREAD, np.float32), spread


# ------------------------------------------------------------------------------- the first pass's dumps
@pytest.mark.parametrize("first_rf", [12, 4])
def test_nlte_lu_against_high_precision(first_rf, tmp_path, monkeypatch):
    """k_nl_lu alone: each element's dumped solution against the 40-digit solve of the engine's own A x = b (L1), to
    the bound the oracle's error against the exact solution of its own systems gives -- apart from the sensitivity
    of the system to last-bit differences in A.  The dumped inputs of the rate matrices -- level populations,
    corrected photoionisation coefficients -- and the bf-heating coefficients of k_nl_bfheat against the oracle's:
    to the double floor.  At first_rf 4 the two integrals read each side's own fitted bins, which may differ inside
    find_T_R's bracket: they are then allowed what the bins they can read -- those reaching above the lowest
    photoionisation edge -- differ by on the two sides (nebular_ref.bins_read_difference), nothing where those bins
    are identical."""
    prefix = _dumped(monkeypatch, tmp_path)
    m, p, nt, arr, nts = _onezone_case(first_rf, True, sfpts=1100, one_pass=True)
    ao, ag, ms = _solve_both(m, p, arr, nt)
    g = nr.read_dump_gpu(prefix + "_p0_gpu.bin")
    o1 = o2 = 0
    checked = 0
    corr_o = np.full(len(g["corr"]), -99.)
    for e, D in enumerate(int(d) for d in g["el_D"]):
        Ag, bg, ng, pg = (g["A"][o2:o2 + D * D].reshape(D, D).T, g["b"][o1:o1 + D], g["norm"][o1:o1 + D],
                          g["pv"][o1:o1 + D])
        o1, o2 = o1 + D, o2 + D * D
        fn = f"{prefix}_p0_ora_e{e}.bin"
        if D == 0 or not os.path.exists(fn):
            continue
        o = nr.read_dump_oracle(fn)
        assert o["D"] == D and o["status"] == g["status"][e] == 0
        err_g, _ = nr.lu_solution_error(Ag, bg, ng, pg)
        err_o, _ = nr.lu_solution_error(o["A"].reshape(D, D).T, o["b"], o["norm"], o["pv"])
        print(f"  element {e}: D {D}, solution L1 error against the 40-digit solve: gpu {err_g:.1e}, "
              f"oracle {err_o:.1e}")
        assert err_g <= SOLVE_BOUND, (e, err_g)
        assert err_o <= SOLVE_BOUND, (e, err_o)  # the oracle meets the bound its own floor sets
        if checked == 0:  # the oracle solves element after element: only its first dump holds the state before any
            dp = nr.rel_diff(g["pops"], o["pops"], nr.POP_ATOL)
        read = o["corr"] != -99.
        assert np.all((corr_o[read] == -99.) | (corr_o[read] == o["corr"][read]))
        corr_o[read] = o["corr"][read]
        checked += 1
    assert checked >= 2
    read = corr_o != -99.
    dc = nr.rel_diff(g["corr"][read], corr_o[read], 1e-300)
    hbo, nu_edge_min = nr.read_dump_bfheat_oracle(prefix + "_bfheat_ora.bin")
    from_bins = nr.bins_read_difference(m, ao, ag, int(arr.mgi_list[0]), nu_edge_min) if first_rf == 4 else 0.
    dh = nr.rel_diff(g["hbc"], hbo[g["hb_ul"]], 1e-300)
    print(f"first_rf {first_rf}: level populations {dp:.1e}, corrected photoionisation coefficients {dc:.1e} "
          f"({read.sum()} read), bf-heating coefficients {dh:.1e} ({len(g['hbc'])} levels, {(g['hbc'] > 0).sum()} > 0); "
          f"the bins they read differ by {from_bins:.1e}")
    assert read.sum() > 0 and (g["hbc"] > 0).any()
    assert dp <= nr.bound(DUMP_RESPONSE["pops"]), dp
    assert dc <= max(nr.bound(DUMP_RESPONSE["corr"]), from_bins), dc
    assert dh <= max(nr.bound(DUMP_RESPONSE["hbc"]), from_bins), dh


def test_nlte_rate_matrices_first_pass(tmp_path, monkeypatch):
    """The first pass's NLTE rate matrices (nltepop.cc:421-628, 832-920) of every element, their LTE normalisation
    and LU solutions, dumped by both sides (ARTIS_GPU_NL_DUMP / ORACLE_NL_DUMP) from the same state: matrix
    columns to 1e-12 of their largest entry, the solution to 1e-5 in the L1 norm (the solve's backward error on
    matrices whose populations span 40 decades).  The balance vector, to 1e-15, is the element's number density
    with the quotient abundance / mean weight taken in double on both sides, as get_elem_numberdens
    (grid.cc:231-236) takes it: a float quotient on either side shows here as 7e-9 to 1.6e-8."""
    prefix = str(tmp_path / "nl")
    monkeypatch.setenv("ARTIS_GPU_NL_DUMP", prefix)
    monkeypatch.setenv("ORACLE_NL_DUMP", prefix)
    m, p, nt, arr, nts = _onezone_case(12, pinned=True)
    arr.params.nlteiter = 0
    ao, ag, ms = _solve_both(m, p, arr, nt)
    el_D, status, A, b, nrm, pv = (nr.read_dump_gpu(prefix + "_p0_gpu.bin")[k]
                                   for k in ("el_D", "status", "A", "b", "norm", "pv"))
    o1 = o2 = 0
    checked = 0
    for e, D in enumerate(el_D):
        D = int(D)
        Ag, bg, ng, pg = A[o2:o2 + D * D].reshape(D, D).T, b[o1:o1 + D], nrm[o1:o1 + D], pv[o1:o1 + D]
        o1, o2 = o1 + D, o2 + D * D
        fn = f"{prefix}_p0_ora_e{e}.bin"
        if D == 0 or not os.path.exists(fn):
            continue
        so, Ao, bo, no, po = (nr.read_dump_oracle(fn)[k] for k in ("status", "A", "b", "norm", "pv"))
        assert len(bo) == D
        Ao = Ao.reshape(D, D).T
        assert so == status[e]
        colerr = (np.abs(Ag - Ao) / np.maximum(np.abs(Ao).max(axis=0), 1e-300)).max()
        assert colerr < 1e-12, (e, colerr)
        np.testing.assert_allclose(bg, bo, rtol=1e-15)
        np.testing.assert_allclose(ng, no, rtol=1e-12)
        l1 = np.abs(pg - po).sum() / np.abs(po).sum()
        print(f"  element {e}: D {D}, matrix {colerr:.1e}, solution L1 {l1:.1e}")
        assert l1 < 1e-5, (e, l1)
        checked += 1
    assert checked >= 2


@pytest.mark.parametrize("first_rf", [12, 4])
def test_update_grid_nlte_onezone_pinned(first_rf):
    """The nebularonezone reference model at timestep 6 (NUM_LTE_TIMESTEPS 4) with a T_e interval holding no root
    (T_e is the same end point on both sides): the Spencer-Fano solution, NLTE passes, partition functions,
    electron densities, cooling.  first_rf = 4: the rate matrices and bf-heating integrals use the fitted bins
    (FIRST_NLTE_RADFIELD_TIMESTEP, DETAILED_BF_ESTIMATORS_USEFROMTIMESTEP).

    The second pass's system of the heaviest element is ill-conditioned (condition number 1.7e17): the oracle's own
    solution of it is 6e-3 off the exact one (PINNED_LU_SOLVE_ERROR), and the oracle alone answers a one-ulp change of
    its float32 state inputs (n_e, T_e, ground-level populations) with n_e 1.8e-3, cooling 2.5e-3, ion fractions
    3.1e-3 (STATE_RESPONSE_PINNED of tools/nebular_ref_floors.py).  So what is computed from the populations keeps
    the former 2e-2 here; the one-pass tests hold the same case to 1.9e-5."""
    m, p, nt, arr, nts = _onezone_case(first_rf, pinned=True)
    ao, ag, ms = _solve_both(m, p, arr, nt)
    cells = arr.mgi_list
    print(f"onezone pinned first_rf={first_rf}: gpu {ms:.1f} ms, passes {ag.iters[cells]}, T_e {ag.Te[cells]}")
    assert (ao.nt_timestep_last_solved[cells] == nts).all()
    _compare_physical(m, ao, ag, cells, te_rtol=1e-6, response=PINNED_RESPONSE,
                      solve_error=PINNED_LU_SOLVE_ERROR, equal_passes=True)


@pytest.mark.parametrize("first_rf", [12, 4])
def test_update_grid_nlte_onezone(first_rf):
    """The same model with the full T_e interval: the NLTE loop converges in a few passes.

    What is computed from the populations: to 10 x the oracle's worst solve error over the passes
    (FREE_LU_SOLVE_ERROR)."""
    m, p, nt, arr, nts = _onezone_case(first_rf, pinned=False)
    ao, ag, ms = _solve_both(m, p, arr, nt)
    cells = arr.mgi_list
    print(f"onezone first_rf={first_rf}: gpu {ms:.1f} ms, passes {ag.iters[cells]}, T_e {ag.Te[cells]} "
          f"(oracle {ao.Te[cells]}), f_heat {ag.nt_frac_heating[cells]}")
    assert (ao.iters[cells] > 1).all() and (ao.nt_timestep_last_solved[cells] == nts).all()
    _compare_physical(m, ao, ag, cells, te_rtol=1e-3, response=FREE_RESPONSE,
                      solve_error=FREE_LU_SOLVE_ERROR, equal_passes=False)


@functools.lru_cache(maxsize=None)
def _multicell_case():
    """The 6-shell synthetic nebular model with a GPU transport step's estimators, a third of the cells thick, at a
    non-thermal skip timestep; shared by the tests below (each solves a copy of arr)."""
    m = Model(**NEB)
    nts = 5
    p = ffi.RunParams.from_buffer_copy(m.params)
    est = _estimators(m, p, nts - 1, 8000, seed=7)
    m.set_timestep(nts)
    nt = ffi.NtDataHandle(m)
    arr = ffi.NlteArrays(m, nts, est=est, seed=11, thick_frac=0.35)
    arr.params.num_lte_timesteps = 8
    return m, p, nt, arr


def test_update_grid_nlte_multicell_lte_branch():
    """A 6-shell synthetic nebular model: every non-empty cell at once, a third of them thick (the LTE branch of
    update_grid_cell, T_e = T_J and LTE ionisation) and a non-thermal skip timestep (nts < NUM_LTE_TIMESTEPS + 1:
    the Spencer-Fano defaults)."""
    m, p, nt, arr = _multicell_case()
    ao, ag, ms = _solve_both(m, p, arr, nt)
    cells = arr.mgi_list
    print(f"multicell: gpu {ms:.1f} ms for {len(cells)} cells, passes {ag.iters[cells]}")
    assert (ao.iters[cells][arr.thick[cells] == 1] == 0).all()
    _compare_physical(m, ao, ag, cells, te_rtol=1e-3, response=MULTICELL_RESPONSE,
                      solve_error=MULTICELL_LU_SOLVE_ERROR, equal_passes=False)


def _ndarrays(arr):
    return {k: v for k, v in arr.__dict__.items() if isinstance(v, np.ndarray)}


def test_update_grid_nlte_refused_allocation_writes_nothing(monkeypatch):
    """A call-scoped device allocation refused in mid-call (ARTIS_GPU_FAIL_ALLOC_ABOVE, read at every allocation,
    set below the Spencer-Fano matrix block of 8 sfpts^2 bytes per batched cell and above the call's other buffers):
    ARTIS_ERR_HIP, and no caller array is written.  Without the limit the same engine solves the same block."""
    ERR_HIP = -2  # include/artis_gpu.h
    m, p, nt, arr = _multicell_case()
    cells = arr.mgi_list
    ao = arr.copy()
    assert oracle_lib.update_grid_nlte(m, nt, ao, params=p, nthreads=16) == 0
    eng = Engine(m, params=p)
    try:
        ag = arr.copy()
        monkeypatch.setenv("ARTIS_GPU_FAIL_ALLOC_ABOVE", str(8 * int(nt.shells.sfpts) ** 2 // 2))
        with pytest.raises(EngineError, match=f"update_grid_nlte -> {ERR_HIP}:"):
            eng.update_grid_nlte(nt, ag)
        monkeypatch.delenv("ARTIS_GPU_FAIL_ALLOC_ABOVE")
        for k, v in _ndarrays(arr).items():
            assert getattr(ag, k).tobytes() == v.tobytes(), k
        ms = eng.update_grid_nlte(nt, ag)
    finally:
        eng.close()
    print(f"after the refused allocation: gpu {ms:.1f} ms for {len(cells)} cells, passes {ag.iters[cells]}")
    assert (ag.iters[cells][arr.thick[cells] == 1] == 0).all() and (ag.iters[cells][arr.thick[cells] != 1] > 0).all()
    _compare_physical(m, ao, ag, cells, te_rtol=1e-3, response=MULTICELL_RESPONSE,
                      solve_error=MULTICELL_LU_SOLVE_ERROR, equal_passes=False)


def test_update_grid_nlte_subset_roundtrip():
    """Cells not listed come back unchanged; the listed ones match the oracle."""
    m = Model(**NEB)
    nts = 12
    p = ffi.RunParams.from_buffer_copy(m.params)
    est = _estimators(m, p, nts - 1, 8000, seed=8)
    m.set_timestep(nts)
    nt = ffi.NtDataHandle(m)
    arr = ffi.NlteArrays(m, nts, est=est, seed=12)
    arr.params.num_lte_timesteps = 2
    full = arr.mgi_list.copy()
    arr.mgi_list = full[::8].copy()
    before = arr.copy()
    ao, ag, ms = _solve_both(m, p, arr, nt)
    print(f"subset: gpu {ms:.1f} ms for {len(arr.mgi_list)} cells")
    _compare_physical(m, ao, ag, arr.mgi_list, te_rtol=1e-3, response=MULTICELL_RESPONSE,
                      solve_error=MULTICELL_LU_SOLVE_ERROR, equal_passes=False)
    untouched = np.setdiff1d(np.arange(m.npts_model), arr.mgi_list)
    for f in FIELDS + ("iters", "nt_timestep_last_solved"):
        g, b0 = getattr(ag, f).reshape(m.npts_model, -1), getattr(before, f).reshape(m.npts_model, -1)
        assert g[untouched].tobytes() == b0[untouched].tobytes(), f


def test_transport_reads_the_gpu_solution():
    """The next update_packets from the GPU's nebular update_grid output (NLTE / superlevel populations, the fitted
    bins, the bf-rate estimators, the Spencer-Fano rates and Auger fractions, cooling): the engine's transport and
    the oracle's, both reading that state, agree packet by packet (tests/parity.py)."""
    m, p, nt, arr, nts = _onezone_case(4, pinned=False)
    eng = Engine(m, params=p)
    try:
        ag = arr.copy()
        eng.update_grid_nlte(nt, ag)
        assert (ag.nlte_pops > -0.9).any() and (ag.bin_W > 0).any()
        ag.apply_to_cellstate(m)
        eng.upload_cellstate(nts)
        pk = m.init_rpackets(nts, 4000, seed=91)
        pg, po = pk.copy(), pk.copy()
        eg = eng.update_packets(nts, pg)
    finally:
        eng.close()
    eo, wo = oracle_lib.update_packets(m, nts, po, params=p, nthreads=16)
    parity.assert_packets_match(pg, po)
    parity.assert_estimators_match(eg, eo)
    assert eo.radfield_count.sum() > 0
