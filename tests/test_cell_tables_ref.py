"""Qualifies tests/cell_tables_ref.py, the numpy restatement the GPU table tests compare the device with, on the CPU.

(a) numpy float64 against the oracle's own calculate_levelpop, cumulative cooling list and
    calculate_macroatom_transitionrates (oracle_cell_tables): two restatements of the reference by different routes
    -- per transition in C++, per level over (transition x cell) in numpy.  They agree to the rounding of the
    library functions (glibc's exp / expm1 / log / pow against numpy's); a misreading of the reference by either
    shows as a gap many orders larger.
(b) numpy float64 against numpy longdouble: the rounding error of a float64 evaluation in the reference's order,
    which the GPU tests' bars are 8 x of (tests/test_gpu_cell_tables.py GAP_B).

Both on the models and the reference cells of the GPU tests (cells by position among the non-empty model cells here,
by the engine's centre-outwards numbering there; the recorded gaps are over every non-empty cell)."""
import numpy as np
import pytest

import cell_tables_ref as R
import oracle_lib
from test_gpu_cell_tables import GAP_B, NTS_NEB, NTS_WIDE, _prepare, assert_wide_preconditions, reference_cells

# gap (a), numpy float64 against the oracle, over every non-empty cell (relative to the row's largest entry; the
# running sums normalised by their totals).  Measured: wide 6.0e-17 / 8.8e-17 / 4.3e-16 / 4.4e-16, NEB nts 5
# 5.9e-18 / 0 / 3.8e-16 / 2.2e-16, NEB nts 14 3.9e-18 / 0 / 4.3e-16 / 2.2e-16.  Recorded: twice the largest.
GAP_A = {"pops": 1.2e-16, "cooling": 1.8e-16, "marates": 8.8e-16, "sums": 8.8e-16}

CONFIGS = [("wide", NTS_WIDE)] + [("neb", nts) for nts in NTS_NEB]


def _nonempty(ref):
    return np.nonzero(ref.S["rho"] > 0)[0]


def _oracle_corrphot(m, ref, nts, mgi):
    """the NO_LUT photoionisation integrals the reference is fed (the device's own on the GPU)"""
    if not m.params.no_lut_photoion:
        return None
    ref._setup(np.float64, mgi)
    ul, t = ref._targets()
    f = oracle_lib.lib().oracle_corrphotoioncoeff
    return np.array([[f(m.atomic, m.geometry, m.cellstate, m.params, nts, int(g), int(u), int(tt), 0)
                      for u, tt in zip(ul, t)] for g in mgi])


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: f"{c[0]}-nts{c[1]}")
def state(request):
    name, nts = request.param
    m, special = _prepare(name, nts)
    ref = R.CellTablesRef(m, nts)
    ne = _nonempty(ref)
    if name == "wide":
        assert_wide_preconditions(m, len(ne))
    mgi = ne[reference_cells(len(ne), also=np.searchsorted(ne, special))]
    feed = _oracle_corrphot(m, ref, nts, mgi)
    t64 = ref.tables(mgi, np.float64, device_corrphot=feed)
    tld = ref.tables(mgi, np.longdouble, device_corrphot=feed)
    orc = [oracle_lib.cell_tables(m, nts, int(g)) for g in mgi]
    return (name, nts), ref, mgi, t64, tld, orc


def test_float64_matches_the_oracle(state):
    cfg, ref, mgi, t64, _, orc = state
    A = ref.A
    worst = {"pops": 0., "cooling": 0., "marates": 0., "sums": 0.}
    for j, o in enumerate(orc):
        worst["pops"] = max(worst["pops"], R.rel_to_rowmax(t64["pops"][j], o["pops"]))
        worst["cooling"] = max(worst["cooling"], R.rel_to_rowmax(t64["cooling"][j], o["cooling"]))
        worst["marates"] = max(worst["marates"], R.rel_to_rowmax(t64["marates"][j], o["processrates"]))
        s = t64["ma_sums"][j]
        for ul in range(A["nlevels_total"]):
            nd, nu, p0 = int(ref.nd[ul]), int(ref.nu[ul]), int(ref.key_off[ul]) + R.N_ACTIONS
            d0, u0 = int(A["level_downtrans_offset"][ul]), int(A["level_uptrans_offset"][ul])
            for pos, n_, arr, a0 in ((p0, nd, "cum_down_same", d0), (p0 + nd, nu, "cum_up_same", u0),
                                     (p0 + nd + nu, nd, "cum_rad_deexc", d0)):
                mine, theirs = s[pos:pos + n_], o[arr][a0:a0 + n_]
                if n_ and theirs[-1] > 0:
                    worst["sums"] = max(worst["sums"], float(np.max(np.abs(mine / mine[-1] - theirs / theirs[-1]))))
    print(cfg, "gap (a)", {k: f"{v:.3g}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= GAP_A[k], (k, v)


def test_float64_rounding_error_is_what_the_gpu_bars_assume(state):
    cfg, ref, mgi, t64, tld, _ = state
    # (a departure ratio that is 0 / 0, or 0 * an overflowed Saha factor, in float64 -- the absent element's -- has
    # no rounding error to measure)
    d64 = t64["bfcell"][..., 1]
    dld = np.where(np.isfinite(d64), tld["bfcell"][..., 1], d64)
    gap = {
        "pops": R.rel_to_rowmax(t64["pops"], tld["pops"]),
        "bfcell_dep": R.rel_to_rowmax(d64, dld),
        "corrphot": R.rel_to_rowmax(t64["corrphot"], tld["corrphot"]),
        "cooling": R.rel_to_rowmax(t64["cooling"], tld["cooling"]),
        "marates": R.rel_to_rowmax(t64["marates"], tld["marates"]),
        "keys": float(np.max(np.abs(R.expected_keys(t64["ma_sums"], t64["ma_norm"]) -
                                    R.expected_keys(tld["ma_sums"], tld["ma_norm"])))),
    }
    print(cfg, "gap (b)", {k: f"{v:.3g}" for k, v in gap.items()})
    for k, v in gap.items():
        assert v <= GAP_B[cfg][k], (k, v)
    # the tables without a transcendental function in them round the same way in both
    for k in ("ionpop", "ffsum", "linecoef"):
        assert R.rel_to_rowmax(t64[k], tld[k]) < 4e-15, k
    assert not any(np.isnan(np.asarray(v, dtype=np.float64)).any() for k, v in t64.items() if k != "bfcell")


def test_reference_covers_every_branch(state):
    """The branches the issue lists, on the inputs the tests use."""
    cfg, ref, mgi, t64, _, _ = state
    A, S, p = ref.A, ref.S, ref.P
    coll, forb = A["line_coll_str"], A["line_forbidden"] != 0
    assert (coll >= 0).any() and ((coll < 0) & forb).any() and ((coll < 0) & ~forb).any()  # macroatom.h:52-150
    incl = t64["bfcell"][..., 0]
    assert (incl > 0).any() and (incl == 0).any()                                           # rpkt.cc:1116-1118
    assert (t64["marates"][..., :R.INTERNALUPHIGHERNT] > 0).any(axis=(0, 1)).all(), "every action total occurs"
    if cfg[0] == "neb":
        nl = S["nlte_pops"][mgi]
        assert (nl < -0.9).any() and (nl >= 0).any()                                        # ltepop.cc:367-370
        ui = A["level_ui"]
        lloc = np.arange(A["nlevels_total"]) - A["ion_uniqueleveloffset"][ui]
        assert (lloc > A["ion_nlevels_nlte"][ui]).any() and ((lloc >= 1) & (lloc <= A["ion_nlevels_nlte"][ui])).any()
        assert (t64["marates"][..., R.INTERNALUPHIGHERNT] > 0).any() and (t64["nt_total"] > 0).any()
        assert p.detailed_bf_estimators and p.multibin_radfield
    # the MINPOP clamps, with and without abundance (ltepop.cc:307-327, 417-430)
    glp, has = S["groundlevelpop"][mgi], S["elem_abundance"][mgi][:, A["ion_element"]] > 0
    assert ((glp < ref.minpop) & has).any() and ((glp < ref.minpop) & ~has).any()
    assert (t64["pops"] == ref.minpop).any() and (t64["pops"] == 0).any()
