"""Every per-cell table artis_gpu_upload_cellstate builds, read back (Engine.cell_table / cell_ma_keys) and compared
with the numpy restatement tests/cell_tables_ref.py, which tests/test_cell_tables_ref.py qualifies against the oracle
on the CPU.  Needs an MI355X.

Two models.  The wide atom reaches what no other checked model does: all four branches of the key-record layout
(engine_dev.h ma_layout), blocked down- and up-arrays of more than one 64-key block, a partial 64-row group of
cells, level and line counts that are no multiples of the tiles.  The nebular model (tests/test_nebular.py NEB), at a
timestep before and one after FIRST_NLTE_RADFIELD_TIMESTEP / DETAILED_BF_ESTIMATORS_USEFROMTIMESTEP, supplies the
NLTE / superlevel populations, the binned radiation field, the bf-rate estimator override and the non-thermal tables.

Exact where the arithmetic allows it: the transposes, and the tables made of + - * / on inputs both sides share
(ionpop, ffsum, nt_cum / nt_total; linecoef and the inclusion half of bfcell from the device's own populations).
The tables with exp / log / pow / expm1 in them are compared relative to the largest entry of their row, within
MARGIN x the rounding error of the float64 reference itself (float64 against longdouble, gap (b)), never looser
than parity.FP_RTOL.  Measured on the CPU over every non-empty cell of each configuration (gap (a) is numpy float64
against the oracle, test_cell_tables_ref.py):

  configuration   table        gap (a)    gap (b)    bar = 8 x (b)
  wide, nts 10    pops         6.0e-17    1.4e-16    1.1e-15
                  bfcell dep   -          1.3e-14    1.0e-13
                  corrphot     -          4.5e-15    3.6e-14
                  cooling      8.8e-17    4.4e-14    3.5e-13
                  marates      4.3e-16    1.3e-15    1.0e-14
                  keys (2^32)  1.9e-6     1.5e-5     1.2e-4   (running sums / total: 4.4e-16, 3.5e-15)
  NEB, nts 5      pops         5.9e-18    5.2e-17    4.2e-16
                  bfcell dep   -          1.0e-14    8.0e-14
                  cooling      0          2.9e-15    2.3e-14
                  marates      3.8e-16    9.6e-15    7.7e-14
                  keys (2^32)  9.5e-7     7.1e-6     5.7e-5
  NEB, nts 14     pops         3.9e-18    6.3e-17    5.0e-16
                  bfcell dep   -          1.1e-14    8.8e-14
                  cooling      0          2.3e-15    1.8e-14
                  marates      4.3e-16    4.8e-15    3.8e-14
                  keys (2^32)  9.5e-7     3.3e-6     2.6e-5
(NEB's corrphot is the NO_LUT integral, which tests/test_nebular.py checks by quadrature, or the estimator, which is
copied: the reference is fed the device's values for the integral slots and the override slots are compared exactly.)

The key records' bound.  ma_key_cmp (physics.h) takes a key to lie within MA_KEY_BAND = 0.5 + 1e-4 of the exact value
on the 2^32 scale.  8 x gap (b) of the wide atom's normalised running sums is 1.2e-4 -- a float64 running sum of
several hundred terms is itself 1.5e-5 from the longdouble one -- so the margin the tables above get does NOT fit
under 1e-4 for this atom.  Nothing is widened for it: the keys are asserted within 0.5 + min(8 x gap (b), 1e-4) of
the longdouble value, i.e. within MA_KEY_BAND itself for the wide atom.

On an MI355X the device measured, against the float64 reference: pops 1.2e-16 (wide) / 5.9e-18 / 3.9e-18 (NEB),
bfcell departure ratios 5.6e-16 / 4.5e-16 / 3.6e-16, corrphot 1.5e-15 (wide), cooling 8.8e-17 / 0 / 1.9e-16,
marates 5.2e-16 / 3.9e-16 / 4.3e-16; max |key - x| 0.5000001 (wide), 0.4999951, 0.4999848 (NEB).  Row mode with one
level per batch gave byte-identical keys, and every level-mode record's high halves equalled the row-mode keys'.

Two cells of each cell state are edited before the upload (cell_tables_ref.perturb_cellstate): the synthetic states
have every element everywhere and no population near MINPOP, so the clamps, a population of 0 and the other outcome
of the inclusion rule would otherwise never run."""
import functools

import numpy as np
import pytest

import cell_tables_ref as R
import oracle_lib
import parity
from artis_amd import Engine
from artis_amd.model import Model

pytestmark = pytest.mark.gpu

WIDE = dict(ngrid_1d=6, nlevels_per_ion=160, n_ionising=20, max_lines=200003, line_window=100, n_resonance=4,
            ntstep=30)
NEB = dict(ngrid_1d=4, nlevels_per_ion=30, n_ionising=10, max_lines=2000, ntstep=20, nebular=1, nlte_level_max=12,
           tmin_days=100., tmax_days=300., T0=6000., ionpot_scale=0.5)
NTS_WIDE = 10
NTS_NEB = (5, 14)  # before / after FIRST_NLTE_RADFIELD_TIMESTEP (12) and DETAILED_BF_ESTIMATORS_USEFROMTIMESTEP (13)

MARGIN = 8.
# gap (b), float64 against longdouble of the reference alone, over every non-empty cell (module docstring)
GAP_B = {
    ("wide", 10): {"pops": 1.4e-16, "bfcell_dep": 1.3e-14, "corrphot": 4.5e-15, "cooling": 4.4e-14,
                   "marates": 1.3e-15, "keys": 1.5e-5},
    ("neb", 5): {"pops": 5.2e-17, "bfcell_dep": 1.0e-14, "corrphot": 0., "cooling": 2.9e-15, "marates": 9.6e-15,
                 "keys": 7.1e-6},
    ("neb", 14): {"pops": 6.3e-17, "bfcell_dep": 1.1e-14, "corrphot": 0., "cooling": 2.3e-15, "marates": 4.8e-15,
                  "keys": 3.3e-6},
}
KEY_BAND_MARGIN = 1e-4  # MA_KEY_BAND - 0.5 (physics.h)


def bar(cfg, table):
    return min(MARGIN * GAP_B[cfg][table], parity.FP_RTOL)


def key_margin(cfg):
    return min(MARGIN * GAP_B[cfg]["keys"], KEY_BAND_MARGIN)


# ---------------------------------------------------------------------------------------------------- models
@functools.lru_cache(maxsize=None)
def _model(name):
    return Model(**(WIDE if name == "wide" else NEB))


def _prepare(name, nts):
    """the model at timestep nts with the two perturbed cells (cell_tables_ref.perturb_cellstate): (model, their
    model-grid indices)"""
    m = _model(name)
    m.set_timestep(nts)
    return m, R.perturb_cellstate(m)


MA_AREA = 55


def _layout(nd, nu):
    """(branch, nbd, nbu) of engine_dev.h ma_layout / ma_blocks, restated for the preconditions only"""
    if nd + nu <= MA_AREA:
        br, sd, su = 0, nd, nu
    elif nd <= MA_AREA // 2:
        br, sd, su = 1, nd, MA_AREA - nd
    elif nu <= MA_AREA // 2:
        br, sd, su = 2, MA_AREA - nu, nu
    else:
        br, sd, su = 3, MA_AREA // 2, MA_AREA - MA_AREA // 2
    blocks = lambda c, s: 0 if c <= s else (c - s + 62) // 63  # noqa: E731
    return br, blocks(nd, sd), blocks(nu, su)


def assert_wide_preconditions(model, n_nonempty):
    """What makes the wide atom worth its name, from the atomic tables: a change of the generator cannot hollow the
    tests out unnoticed."""
    A = R.atomic_arrays(model)
    lay = np.array([_layout(int(d), int(u)) for d, u in zip(A["level_ndowntrans"], A["level_nuptrans"])])
    assert set(lay[:, 0]) == {0, 1, 2, 3}, "every ma_layout branch"
    assert lay[:, 1].max() >= 2 and lay[:, 2].max() >= 2, "down and up arrays of more than one block"
    assert ((lay[:, 1] > 0) & (lay[:, 2] > 0)).any(), "levels with both arrays blocked"
    assert n_nonempty > 128 and n_nonempty % 64 != 0
    assert A["nlevels_total"] % 64 != 0
    assert A["nlines"] % 8 != 0


def reference_cells(n, also=()):
    """Non-empty cell indices the reference is evaluated at: the edges of the 64-row groups, the last cell (every
    cell has a linecoef row in the default engine), the cells in `also`, and 16 more drawn with a fixed seed."""
    must = [k for k in (0, 1, 62, 63, 64, 65, 127, 128, n - 1) if 0 <= k < n] + [int(k) for k in also]
    rest = np.setdiff1d(np.arange(n), must)
    extra = np.random.default_rng(20240611).choice(rest, size=min(16, len(rest)), replace=False)
    return np.array(sorted(set(must) | set(int(x) for x in extra)), dtype=np.int64)


# ------------------------------------------------------------------------------------- device state, read once
def _all_keys(eng, ncells):
    keys, has, hi_only, sep_bad = [], [], None, 0
    for k in range(ncells):
        kk, hh, hi_only, sb = eng.cell_ma_keys(k)
        keys.append(kk)
        has.append(hh)
        sep_bad += sb
    return np.array(keys), np.array(has), hi_only, sep_bad


TABLES = ("ionpop", "ffsum", "pops", "popsT", "bfcell", "corrphot", "corrphotT", "cooling", "nt_cum", "nt_total",
          "linecoef", "linecoef_neg", "cell_mgi")


@functools.lru_cache(maxsize=None)
def _default_state(name, nts):
    """One default engine (row mode, every linecoef row) on the model at nts: every table and every cell's keys, and
    the reference (float64; longdouble running sums for the keys) at the reference cells."""
    m, special = _prepare(name, nts)
    eng = Engine(m)
    try:
        info = eng.table_info()
        n = info["cells"]
        if name == "wide":
            assert_wide_preconditions(m, n)
        assert info["macache_rows"] == n and info["linecoef_rows"] == n, info
        eng.upload_cellstate(nts)
        dev = {t: eng.cell_table(t) for t in TABLES}
        dev["keys"], dev["has"], dev["hi_only"], dev["sep_bad"] = _all_keys(eng, n)
    finally:
        eng.close()
    ref = R.CellTablesRef(m, nts)
    cells = reference_cells(n, also=[int(np.nonzero(dev["cell_mgi"] == g)[0][0]) for g in special])
    mgi = dev["cell_mgi"][cells]
    feed = dev["corrphot"][cells] if m.params.no_lut_photoion else None
    t64 = ref.tables(mgi, np.float64, device_corrphot=feed, linecoef=False)
    tld = ref.tables(mgi, np.longdouble, device_corrphot=feed, linecoef=False)
    x = R.expected_keys(tld["ma_sums"], tld["ma_norm"])
    return {"model": m, "n": n, "dev": dev, "ref": ref, "cells": cells, "mgi": mgi, "t64": t64, "x": x,
            "norm_pos": tld["ma_norm"] > 0}


def _segments(ref):
    """(start, length) of every key array of a cell's key list: per level the 9 action keys and the six arrays"""
    nd, nu, nr, nt, off = ref.nd, ref.nu, ref.nr, ref.nt, ref.key_off
    lens = np.stack([np.full_like(nd, R.N_ACTIONS), nd, nu, nd, nr, nr, nt], axis=1)
    starts = off[:-1, None] + np.concatenate([np.zeros((len(nd), 1), dtype=np.int64), np.cumsum(lens, axis=1)[:, :-1]],
                                             axis=1)
    return starts.ravel(), lens.ravel()


def assert_key_structure(keys, ref, has=None):
    """Needs no reference: within each array the keys do not decrease, and the array ends at 2^32 - 1 or is all 0.
    keys [cells, nkeys] (has [cells, levels]: only the levels with a record)."""
    starts, lens = _segments(ref)
    ne = lens > 0
    starts, lens = starts[ne], lens[ne]
    seg_of = np.repeat(np.arange(len(starts)), lens)
    assert len(seg_of) == keys.shape[1]
    first = np.zeros(keys.shape[1], dtype=bool)
    first[starts] = True
    k64 = keys.astype(np.int64)
    step_ok = (k64[:, 1:] >= k64[:, :-1]) | first[None, 1:]
    last = k64[:, starts + lens - 1]
    segmax = np.maximum.reduceat(k64, starts, axis=1)
    end_ok = (last == R.KEY_SCALE) | (segmax == 0)
    if has is not None:
        lvl_of_seg = np.repeat(np.arange(len(ref.nd)), 7)[ne]
        end_ok |= ~has[:, lvl_of_seg]
    assert step_ok.all(), f"{(~step_ok).sum()} keys below their predecessor"
    assert end_ok.all(), f"{(~end_ok).sum()} arrays neither end at 2^32 - 1 nor are all 0"


# ------------------------------------------------------------------------------------------------ the tables
def _check_tables(cfg):
    name, nts = cfg
    st = _default_state(name, nts)
    m, dev, ref, cells, mgi, t64 = st["model"], st["dev"], st["ref"], st["cells"], st["mgi"], st["t64"]
    p = m.params
    n = st["n"]
    assert sorted(dev["cell_mgi"]) == sorted(np.nonzero(ref.S["rho"] > 0)[0]), "the non-empty cells"
    # transposes, bit for bit
    assert np.array_equal(dev["popsT"], dev["pops"].T)
    assert np.array_equal(dev["corrphotT"], dev["corrphot"].T)
    # + - * / on shared inputs: bit-identical to numpy float64
    assert np.array_equal(dev["ionpop"][cells], t64["ionpop"])
    assert np.array_equal(dev["ffsum"][cells, 0], t64["ffsum"])
    if p.nt_on:
        assert np.array_equal(dev["nt_cum"][cells], t64["nt_cum"])
        assert np.array_equal(dev["nt_total"][cells, 0], t64["nt_total"])
        assert (dev["nt_total"] > 0).any()
    else:
        assert dev["nt_cum"] is None and dev["nt_total"] is None
    # the inclusion half of bfcell and linecoef from the device's own populations -- every cell
    allmgi = dev["cell_mgi"]
    incl = ref.bfcell_from(allmgi, dev["pops"], dev["ionpop"])[..., 0]
    assert np.array_equal(dev["bfcell"][..., 0], incl)
    assert (incl > 0).any() and (incl == 0).any(), "both outcomes of the inclusion rule"
    lc = dev["linecoef"]
    nlines = m.nlines
    assert lc.shape == (n, (nlines + 15) // 16 * 16) and (lc.shape[1] > nlines or name != "wide")
    assert not lc[:, nlines:].any(), "the padding columns are exactly 0"
    want = ref.linecoef_from(allmgi, dev["pops"])
    assert np.array_equal(lc[:, :nlines], want)
    assert dev["linecoef_neg"] == int((want < 0).any())
    # the tables with transcendental functions in them, relative to the row's largest entry
    worst = {
        "pops": R.rel_to_rowmax(dev["pops"][cells], t64["pops"]),
        "bfcell_dep": R.rel_to_rowmax(dev["bfcell"][cells][..., 1], t64["bfcell"][..., 1]),
        "corrphot": R.rel_to_rowmax(dev["corrphot"][cells], t64["corrphot"]),
        "cooling": R.rel_to_rowmax(dev["cooling"][cells], t64["cooling"]),
    }
    print(cfg, {k: f"{v:.3g} (bar {bar(cfg, k):.3g})" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= bar(cfg, k), (k, v, bar(cfg, k))
    return st


def test_wide_tables():
    _check_tables(("wide", NTS_WIDE))


@pytest.mark.parametrize("nts", NTS_NEB)
def test_nebular_tables(nts):
    st = _check_tables(("neb", nts))
    m, dev, ref, cells, mgi = st["model"], st["dev"], st["ref"], st["cells"], st["mgi"]
    p = m.params
    assert p.nlte_pops_on and p.multibin_radfield and p.detailed_bf_estimators and p.no_lut_photoion and p.nt_on
    # the branches the populations take (ltepop.cc:349-415): NLTE, superlevel and "no solution yet"
    nl = ref.S["nlte_pops"][mgi]
    assert (nl < -0.9).any() and (nl >= 0).any()
    # the estimator override (ratecoeff.cc:1255-1261) from DETAILED_BF_ESTIMATORS_USEFROMTIMESTEP on, exactly
    ref._setup(np.float64, mgi)
    none = ref._corrphot(np.full_like(dev["corrphot"][cells], -1.))
    over = none != -1.
    assert over.any() == (nts >= p.detailed_bf_usefromtimestep)
    assert np.array_equal(dev["corrphot"][cells][over], none[over])
    # the binned field of rad_exc: a fitted bin, no bin, a bin without a fit (from FIRST_NLTE_RADFIELD_TIMESTEP on)
    if nts >= p.first_nlte_radfield_timestep:
        A = ref.A
        nu = (A["level_epsilon"][ref.line_up] - A["level_epsilon"][ref.line_lo]) / R.K["H"]
        _, W, ok = ref._radfield_TW(nu)
        b = np.searchsorted(A["radfield_nu_upper"], nu, side="right")
        inbin = (nu >= A["radfield_nu_lower_first"]) & (b < A["radfield_nbins"])
        assert ok.any() and (~inbin).any() and (inbin[:, None] & ~ok).any()


# ---------------------------------------------------------------------------------------------- key records
def _check_row_keys(cfg):
    st = _default_state(*cfg)
    dev, ref, cells = st["dev"], st["ref"], st["cells"]
    keys = dev["keys"]
    assert dev["has"].all() and not dev["hi_only"] and dev["sep_bad"] == 0
    assert keys.shape == (st["n"], ref.key_off[-1])
    assert_key_structure(keys, ref)
    # against the longdouble running sums, every level of every reference cell
    k = keys[cells].astype(np.longdouble)
    err = np.abs(k - st["x"])
    m = key_margin(cfg)
    print(cfg, f"max |key - x| = {float(err.max()):.7f} (bound 0.5 + {m:.3g})")
    assert err.max() <= 0.5 + m
    # a positive total ends its array at 2^32 - 1, a zero total gives an array of zeros
    starts, lens = _segments(ref)
    ne = lens > 0
    last = (starts + lens - 1)[ne]
    pos = st["norm_pos"][:, last]
    assert np.array_equal(keys[cells][:, last] == R.KEY_SCALE, pos)
    assert not keys[cells][~st["norm_pos"]].any()
    return st


def test_wide_key_records_row_mode():
    _check_row_keys(("wide", NTS_WIDE))


@pytest.mark.parametrize("nts", NTS_NEB)
def test_nebular_key_records_row_mode(nts):
    _check_row_keys(("neb", nts))


def _level_engine_keys(m, nts, n, monkeypatch, env):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    eng = Engine(m)
    try:
        assert eng.table_info()["macache_rows"] == 0
        eng.upload_cellstate(nts)
        info = eng.table_info()
        keys, has, hi_only, sep_bad = _all_keys(eng, n)
        marates = eng.cell_table("marates")
    finally:
        eng.close()
    return info, keys, has, hi_only, sep_bad, marates


def _check_level_keys(st, info, keys, has, hi_only, sep_bad):
    ref = st["ref"]
    row = st["dev"]["keys"]
    assert info["ma_level_records"] == has.sum() > 0 and sep_bad == 0
    lvl = np.repeat(np.arange(len(ref.nd)), np.diff(ref.key_off))
    present = has[:, lvl]
    shift = 16 if hi_only else 0
    assert np.array_equal((keys >> shift)[present], (row >> shift)[present]), \
        "k_ma_build's keys differ from k_marates + k_mapack's"
    assert not keys[~present].any()
    if hi_only:  # (the row-mode keys these high halves equal passed assert_key_structure)
        assert not (keys & 0xffff).any()
    else:
        assert_key_structure(keys, ref, has)


def test_wide_key_records_one_level_per_batch(monkeypatch):
    """k_marates + k_mapack with a scratch of one level (ARTIS_GPU_MAREC_SCRATCH_MB=0): byte-identical records."""
    st = _default_state("wide", NTS_WIDE)
    m, _ = _prepare("wide", NTS_WIDE)
    monkeypatch.setenv("ARTIS_GPU_MAREC_SCRATCH_MB", "0")
    eng = Engine(m)
    try:
        assert eng.table_info()["macache_rows"] == st["n"]
        eng.upload_cellstate(NTS_WIDE)
        keys, has, hi_only, sep_bad = _all_keys(eng, st["n"])
    finally:
        eng.close()
    assert has.all() and not hi_only and sep_bad == 0
    assert np.array_equal(keys, st["dev"]["keys"])


@pytest.mark.parametrize("small", [None, "0", "64"], ids=["default_split", "large_builds", "mixed_builds"])
def test_wide_key_records_level_mode(monkeypatch, small):
    """Level mode at half the rows (k_ma_build, through its small-level and its large-level launch): every record's
    high halves equal the row-mode keys' exactly -- the code's claim that ma_rate_at's terms summed per action are
    ma_accumulate's sequence bit for bit.  The per-pair action totals (k_marates<false>) within their bar."""
    cfg = ("wide", NTS_WIDE)
    st = _default_state(*cfg)
    m, _ = _prepare(*cfg)
    env = {"ARTIS_GPU_MACACHE_ROWS": str(st["n"] // 2)}
    if small is not None:
        env["ARTIS_GPU_MA_BUILD_SMALL"] = small
    info, keys, has, hi_only, sep_bad, marates = _level_engine_keys(m, NTS_WIDE, st["n"], monkeypatch, env)
    _check_level_keys(st, info, keys, has, hi_only, sep_bad)
    if small is None:
        _check_marates(cfg, st, marates)


def _check_marates(cfg, st, marates):
    nl = len(st["ref"].nd)
    got = marates.reshape(st["n"], nl, R.N_ACTIONS)[st["cells"]]
    worst = R.rel_to_rowmax(got, st["t64"]["marates"])
    print(cfg, f"marates {worst:.3g} (bar {bar(cfg, 'marates'):.3g})")
    assert worst <= bar(cfg, "marates")
    if st["model"].params.nt_on:
        assert (got[..., R.INTERNALUPHIGHERNT] > 0).any()


@pytest.mark.parametrize("nts", NTS_NEB)
def test_nebular_level_mode(monkeypatch, nts):
    cfg = ("neb", nts)
    st = _default_state(*cfg)
    m, _ = _prepare(*cfg)
    info, keys, has, hi_only, sep_bad, marates = _level_engine_keys(
        m, nts, st["n"], monkeypatch, {"ARTIS_GPU_MACACHE_ROWS": str(st["n"] // 2)})
    _check_level_keys(st, info, keys, has, hi_only, sep_bad)
    _check_marates(cfg, st, marates)


# ------------------------------------------------------------------------------------------------- linecoef
@pytest.mark.parametrize("env", [{"ARTIS_GPU_LINECOEF_GATHER": "1"}, {"ARTIS_GPU_LINECOEF_ROWS": "half"},
                                 {"ARTIS_GPU_LINECOEF_GATHER": "1", "ARTIS_GPU_LINECOEF_ROWS": "half"}],
                         ids=["gather_kernel", "half_rows", "half_rows_gather_kernel"])
def test_wide_linecoef_kernels_and_budgets(monkeypatch, env):
    """k_linecoef_lds (default) and k_linecoef (ARTIS_GPU_LINECOEF_GATHER) write the same table byte for byte; with
    rows for half the cells, the rows present are the same rows of the full table."""
    st = _default_state("wide", NTS_WIDE)
    m, _ = _prepare("wide", NTS_WIDE)
    full = st["dev"]["linecoef"]
    for k_, v in env.items():
        monkeypatch.setenv(k_, str(st["n"] // 2) if v == "half" else v)
    eng = Engine(m)
    try:
        eng.upload_cellstate(NTS_WIDE)
        lc = eng.cell_table("linecoef")
        neg = eng.cell_table("linecoef_neg")
    finally:
        eng.close()
    rows = st["n"] // 2 if "ARTIS_GPU_LINECOEF_ROWS" in env else st["n"]
    assert lc.shape == (rows, full.shape[1])
    assert lc.tobytes() == full[:rows].tobytes()
    assert neg == int((full[:rows] < 0).any())


# ------------------------------------------------------------- the device search over the new record shapes
@pytest.mark.parametrize("level_mode", [False, True], ids=["row_mode", "level_mode_half_rows"])
def test_wide_transport_matches_oracle(monkeypatch, level_mode):
    """One transport step of the wide atom against the oracle: k_ma's two-pass search over blocked down arrays and
    arrays of more than one block, from whole rows and from level-mode records."""
    m = _model("wide")
    m.set_timestep(NTS_WIDE)
    pk = m.init_rpackets(NTS_WIDE, 2000, seed=17)
    if level_mode:
        probe = Engine(m)
        n = probe.table_info()["cells"]
        probe.close()
        monkeypatch.setenv("ARTIS_GPU_MACACHE_ROWS", str(n // 2))
    eng = Engine(m)
    try:
        eng.upload_cellstate(NTS_WIDE)
        pg, po = pk.copy(), pk.copy()
        eg = eng.update_packets(NTS_WIDE, pg)
        work = eng.last_work()
        info = eng.table_info()
    finally:
        eng.close()
    eo, wo = oracle_lib.update_packets(m, NTS_WIDE, po, nthreads=16)
    parity.assert_packets_match(pg, po)
    parity.assert_estimators_match(eg, eo)
    assert work[8] > 0 and work[8] == wo[8]  # WK_MA_JUMPS
    if level_mode:
        assert info["macache_rows"] == 0 and info["ma_jumps"] > 0 and info["ma_jumps_recorded"] > 0, info
    else:
        assert info["macache_rows"] == info["cells"]
