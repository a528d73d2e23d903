#!/usr/bin/env python3
"""The oracle's own noise floors for the nebular update_grid tests (CPU only, a few minutes).

For every case of tests/test_gpu_nebular_update_grid.py, with the oracle's transport step in place of the engine's:
the oracle's response to a one-ulp change (up, down; the larger) of every float64 estimator input, per compared
quantity; the error of its Spencer-Fano solution against a longdouble back substitution of its own matrix; the error
of its rate-matrix LU solutions against a 40-digit solve of its own systems.  Prints the constants the tests commit
(ONEPASS_RESPONSE, ONEPASS_SOLVE_RESPONSE, PINNED_RESPONSE, FREE_RESPONSE, SF_SOLVE_ERROR, LU_SOLVE_ERROR,
PINNED_LU_SOLVE_ERROR, FREE_LU_SOLVE_ERROR, MULTICELL_RESPONSE, MULTICELL_LU_SOLVE_ERROR, DUMP_RESPONSE,
BIN_W_SPREAD); the tests derive their bounds from them with nebular_ref.bound (10 x, or the type floor).  Also
prints, for the record only, the converged cases' response to one ulp of the call's state inputs
(STATE_RESPONSE_*).

    python tools/nebular_ref_floors.py [--skip-converged]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import nebular_ref as nr  # noqa: E402
import oracle_lib  # noqa: E402
from artis_amd import ffi  # noqa: E402
from artis_amd.model import Model  # noqa: E402


def solve(m, p, nt, arr):
    a = arr.copy()
    rc = oracle_lib.update_grid_nlte(m, nt, a, params=p, nthreads=16)
    assert rc == 0, rc
    return a


def merge(into, rep):
    for k, v in rep.items():
        into[k] = max(into.get(k, 0.), v)


def response(name, m, p, nt, arr, into, physical=None, solved=None):
    """the base run against the two perturbed ones, merged into the dicts; pass counts must not move"""
    t0 = time.time()
    base = solve(m, p, nt, arr)
    cells = arr.mgi_list
    for up in (True, False):
        pert = solve(m, p, nt, nr.perturbed(arr, up))
        assert np.array_equal(pert.iters, base.iters), (name, "pass counts moved")
        assert np.array_equal(pert.nt_timestep_last_solved, base.nt_timestep_last_solved)
        rep = nr.report(base, pert)
        merge(into, rep)
        if physical is not None:
            merge(physical, nr.physical_report(m, base, pert, cells))
        if solved is not None:
            merge(solved, nr.solve_report(m, base, pert, cells))
    print(f"# {name}: passes {sorted(set(base.iters[cells].tolist()))}, {time.time() - t0:.1f} s, "
          + ", ".join(f"{k} {v:.1e}" for k, v in rep.items() if v > 0), flush=True)
    return base


def dump_run(m, p, nt, arr, prefix):
    os.environ["ORACLE_NL_DUMP"] = prefix
    try:
        return solve(m, p, nt, arr)
    finally:
        del os.environ["ORACLE_NL_DUMP"]


def element_dumps(prefix, m, ps=0):
    out = {}
    for e in range(m.nelements):
        fn = f"{prefix}_p{ps}_ora_e{e}.bin"
        if os.path.exists(fn):
            out[e] = nr.read_dump_oracle(fn)
    return out


def worst_lu_error(name, m, p, nt, arr, prefix):
    """the largest L1 error, over the dumped passes (the first four) and elements, of the oracle's rate-matrix
    solutions against the 40-digit solve of its own systems"""
    worst = 0.
    for tag, a in (("b", arr), ("u", nr.perturbed(arr, True)), ("d", nr.perturbed(arr, False))):
        dump_run(m, p, nt, a, prefix + tag)
        for ps in range(4):
            for e, d in element_dumps(prefix + tag, m, ps).items():
                D = d["D"]
                err, _ = nr.lu_solution_error(d["A"].reshape(D, D).T, d["b"], d["norm"], d["pv"])
                if err > worst:
                    worst = err
                    print(f"# {name}: pass {ps} element {e}: oracle LU solution L1 error vs mpmath {err:.2e}",
                          flush=True)
    return worst


def single_cell_lu_error(name, m, p, nt, arr, tmp, ncells=2):
    """worst_lu_error of a multicell case: the dumps hold one cell's solves, so the first iterated cells of the
    case are solved one at a time"""
    worst = 0.
    iterated = [int(c) for c in arr.mgi_list if arr.thick[c] != 1][:ncells]
    for c in iterated:
        one = arr.copy()
        one.mgi_list = np.array([c], dtype=np.int32)
        worst = max(worst, worst_lu_error(f"{name}, cell {c}", m, p, nt, one, os.path.join(tmp, f"mc{len(name)}_{c}")))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-converged", action="store_true", help="only the one-pass cases and the solves")
    args = ap.parse_args()
    est = nr.oracle_estimators
    tmp = tempfile.mkdtemp(prefix="nlfloors")
    onepass, onepass_solved, sf_err, lu_err, dump_resp = {}, {}, {}, 0., {}

    for first_rf in (12, 4):
        m, p, nt, arr, nts = nr.onezone_case(est, first_rf, True, sfpts=1100, one_pass=True)
        response(f"one pass, one zone, first_rf {first_rf}", m, p, nt, arr, onepass, solved=onepass_solved)
        # the first pass's dumps: the LU solve against mpmath, the dumped inputs' response
        runs = {}
        for tag, a in (("base", arr), ("up", nr.perturbed(arr, True)), ("down", nr.perturbed(arr, False))):
            prefix = os.path.join(tmp, f"rf{first_rf}{tag}")
            dump_run(m, p, nt, a, prefix)
            runs[tag] = (element_dumps(prefix, m), nr.read_dump_bfheat_oracle(prefix + "_bfheat_ora.bin"))
        for e, d in runs["base"][0].items():
            D = d["D"]
            err, _ = nr.lu_solution_error(d["A"].reshape(D, D).T, d["b"], d["norm"], d["pv"])
            print(f"# first_rf {first_rf} element {e}: D {D}, oracle LU solution L1 error vs mpmath {err:.2e}",
                  flush=True)
            lu_err = max(lu_err, err)
            for tag in ("up", "down"):
                q = runs[tag][0][e]
                merge(dump_resp, {"corr": nr.rel_diff(q["corr"], d["corr"], 1e-300)})
                # the oracle solves element after element: only its first dump holds the populations before any
                # solve, which is what the tests compare
                if e == min(runs["base"][0]):
                    merge(dump_resp, {"pops": nr.rel_diff(q["pops"], d["pops"], nr.POP_ATOL)})
        for tag in ("up", "down"):
            merge(dump_resp, {"hbc": nr.rel_diff(runs[tag][1][0], runs["base"][1][0], 1e-300)})

    for sfpts, emax in nr.SF_SHAPES:
        m, p, nt, arr, nts = nr.onezone_case(est, 12, True, sfpts=sfpts, sf_emax=emax, one_pass=True)
        response(f"one pass, one zone, sfpts {sfpts}", m, p, nt, arr, onepass, solved=onepass_solved)
        prefix = os.path.join(tmp, f"sf{sfpts}")
        a = dump_run(m, p, nt, arr, prefix)
        c = int(arr.mgi_list[0])
        A1 = ffi.NT_MAX_AUGER + 1
        prob = a.nt_prob_num_auger.reshape(-1, m.nions_total, A1)[c]
        assert np.all(np.isfinite(prob)), prob
        psum = prob.sum(axis=1)  # 1 for every ion with a solution (0: none stored)
        assert np.all((np.abs(psum - 1.) < 1e-6) | (psum == 0.)), psum
        _, M, rhs, y = nr.read_dump_sf(prefix + "_sf_ora.bin", column_major=False)
        sf_err[sfpts] = nr.sf_solution_error(M, rhs, y)
        print(f"# sfpts {sfpts}: f_heat {a.nt_frac_heating[c]:.6f}, oracle SF solution error vs longdouble "
              f"{sf_err[sfpts]:.2e}", flush=True)

    for sfpts in (1100, 200):
        m, p, nt, arr, nts = nr.multicell_sf_case(est, sfpts)
        response(f"one pass, multicell, sfpts {sfpts}", m, p, nt, arr, onepass, solved=onepass_solved)

    # the synthetic bins: the spread of W P(T_R) / J_bin over the oracle's fitted bins against 30-digit integrals
    spread = 0.
    for nbins, T_R_min in nr.SYNTH_BIN_CASES:
        sb = nr.SyntheticBins(est, nbins, T_R_min)
        nroot, sp = sb.check(solve(sb.model, sb.params, sb.nt, sb.arr), "oracle")
        print(f"# synthetic bins {nbins}, T_R_min {T_R_min}: {nroot} roots inside 1.5e-4, spread {sp:.2e}", flush=True)
        spread = max(spread, sp)

    # the AFTER_LU outputs are judged on the solve's scale (nebular_ref.solve_report), the others element by element
    onepass = {k: v for k, v in onepass.items() if k in nr.BEFORE_LU}
    out = {"ONEPASS_RESPONSE": onepass, "ONEPASS_SOLVE_RESPONSE": onepass_solved,
           "SF_SOLVE_ERROR": max(sf_err.values()), "LU_SOLVE_ERROR": lu_err, "DUMP_RESPONSE": dump_resp,
           "BIN_W_SPREAD": spread}

    if not args.skip_converged:
        pinned, free, multicell, scratch = {}, {}, {}, {}
        lu_multicell = 0.
        lu_pinned = lu_free = 0.
        for first_rf in (12, 4):
            m, p, nt, arr, nts = nr.onezone_case(est, first_rf, True)
            response(f"pinned, first_rf {first_rf}", m, p, nt, arr, scratch, pinned)
            lu_pinned = max(lu_pinned, worst_lu_error(f"pinned, first_rf {first_rf}", m, p, nt, arr,
                                                      os.path.join(tmp, f"cp{first_rf}")))
            m, p, nt, arr, nts = nr.onezone_case(est, first_rf, False)
            response(f"free, first_rf {first_rf}", m, p, nt, arr, scratch, free)
            lu_free = max(lu_free, worst_lu_error(f"free, first_rf {first_rf}", m, p, nt, arr,
                                                  os.path.join(tmp, f"cf{first_rf}")))
        out["PINNED_LU_SOLVE_ERROR"], out["FREE_LU_SOLVE_ERROR"] = lu_pinned, lu_free
        # the multicell LTE-branch case and the subset case of the GPU tests
        m = Model(**nr.NEB)
        p = ffi.RunParams.from_buffer_copy(m.params)
        e5 = est(m, p, 4, 8000, 7)
        m.set_timestep(5)
        nt = ffi.NtDataHandle(m)
        arr = ffi.NlteArrays(m, 5, est=e5, seed=11, thick_frac=0.35)
        arr.params.num_lte_timesteps = 8
        response("multicell with LTE branch", m, p, nt, arr, scratch, multicell)
        lu_multicell = max(lu_multicell, single_cell_lu_error("multicell with LTE branch", m, p, nt, arr, tmp))
        m = Model(**nr.NEB)
        p = ffi.RunParams.from_buffer_copy(m.params)
        e12 = est(m, p, 11, 8000, 8)
        m.set_timestep(12)
        nt = ffi.NtDataHandle(m)
        arr = ffi.NlteArrays(m, 12, est=e12, seed=12)
        arr.params.num_lte_timesteps = 2
        arr.mgi_list = arr.mgi_list[::8].copy()
        response("multicell subset", m, p, nt, arr, scratch, multicell)
        lu_multicell = max(lu_multicell, single_cell_lu_error("multicell subset", m, p, nt, arr, tmp))
        out["PINNED_RESPONSE"], out["FREE_RESPONSE"], out["MULTICELL_RESPONSE"] = pinned, free, multicell
        out["MULTICELL_LU_SOLVE_ERROR"] = lu_multicell
        # For the record, not used by any bound: the converged one-zone cases' response to a one-ulp change of the
        # call's state inputs (float32 n_e, T_e, ground-level populations; the NLTE populations), one array at a
        # time, at sfpts 1100.  At first_rf 12 the estimator inputs above do not reach the rate matrices; these do.
        for pin, key in ((True, "STATE_RESPONSE_PINNED"), (False, "STATE_RESPONSE_FREE")):
            state = {}
            for first_rf in (12, 4):
                m, p, nt, arr, nts = nr.onezone_case(est, first_rf, pin, sfpts=1100)
                base = solve(m, p, nt, arr)
                for name in ("nne", "Te", "groundlevelpop", "nlte_pops"):
                    for up in (True, False):
                        a = arr.copy()
                        v = getattr(a, name)
                        setattr(a, name, np.nextafter(v, np.inf if up else -np.inf, dtype=v.dtype))
                        merge(state, nr.physical_report(m, base, solve(m, p, nt, a), arr.mgi_list))
            out[key] = state

    shutil.rmtree(tmp, ignore_errors=True)  # the dumps
    for k, v in out.items():
        if isinstance(v, dict):
            print(f"{k} = {{" + ", ".join(f'"{f}": {x:.1e}' for f, x in v.items()) + "}")
        else:
            print(f"{k} = {v:.1e}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
