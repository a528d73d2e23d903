"""The host side of the per-line emission / absorption trace (artis_gpu_line_trace): the ABI, the unit conversion of
the regions, the ranking and the table writer (printout_tracemission_stats, spectrum.cc:58-136) on hand-made
arrays.  No GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import line_trace_lib as T
from artis_amd import GPU_SO, exspec, ffi


def test_library_exports_the_entry_point_and_keeps_the_abi():
    out = subprocess.run(["nm", "-D", "--defined-only", GPU_SO], check=True, capture_output=True, text=True).stdout
    assert "artis_gpu_line_trace" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    lib = C.CDLL(GPU_SO)
    assert lib.artis_gpu_abi_version() == 12
    lib.artis_gpu_line_trace.argtypes = [C.POINTER(ffi.LineTraceRequest), C.POINTER(ffi.LineTraceOut)]
    arr = ffi.LineTraceArrays(10, 1)
    req = ffi.line_trace_request([T.REGIONS[0]], T.NNUBINS)
    assert lib.artis_gpu_line_trace(C.byref(req), C.byref(arr.struct)) == -1  # ARTIS_ERR_NOT_INITIALISED
    assert not arr.lines.any() and not arr.totals.any()


def test_struct_layout_matches_the_header():
    assert C.sizeof(ffi.LineTraceRegion) == 32
    assert ffi.LineTraceRequest.syn_dir.offset == 16 and ffi.LineTraceRequest.regions.offset == 40
    assert C.sizeof(ffi.LineTraceRequest) == 48 and C.sizeof(ffi.LineTraceOut) == 16
    assert ffi.LINE_TRACE_MAX_REGIONS == 16


def test_region_units():
    """Days and Angstroms to s and Hz with the reference's expressions (spectrum.cc:13-18)."""
    nu_lower, nu_upper, time_min, time_max = ffi.line_trace_region(320., 340., 1000., 25000.)
    assert nu_lower == 1.e8 * T.CLIGHT / 25000. and nu_upper == 1.e8 * T.CLIGHT / 1000.
    assert time_min == 320. * T.DAY and time_max == 340. * T.DAY
    assert T.CLIGHT == 2.99792458e10 and T.DAY == 86400. and T.PI == 3.1415926535987
    for reg in T.REGIONS:
        assert ffi.line_trace_region(*reg) == T.region_bounds(reg)
    req = ffi.line_trace_request(T.REGIONS, nnubins=60, nprocs=2, abin=37, syn_dir=(0.3, 0.4, 0.5))
    assert (req.nnubins, req.nprocs, req.abin, req.nregions) == (60, 2, 37, 4)
    assert list(req.syn_dir) == [0.3, 0.4, 0.5]
    for k, reg in enumerate(T.REGIONS):
        r = req.regions[k]
        assert (r.nu_lower, r.nu_upper, r.time_min, r.time_max) == T.region_bounds(reg)
    arr = ffi.LineTraceArrays(8000, 4)
    assert arr.lines.shape == (4, 8000, 4) and arr.totals.shape == (4, 2)
    assert C.addressof(arr.struct.lines.contents) == arr.lines.ctypes.data


def _numpy_rank(lines, column, maxlines=500):
    e = lines[:, column]
    order = np.lexsort((np.arange(len(e)), -e))
    order = order[e[order] > 0]
    return order[:maxlines]


def test_ranking():
    lines = np.zeros((40, 4))
    lines[[3, 17, 5, 30, 9], 0] = [2., 5., 2., 2., 7.]   # ties at 2.: ascending line index
    lines[[8, 2], 2] = [1., 1.]
    lines[11, 0] = -4.                                   # never listed
    assert list(exspec.rank_line_trace(lines, 0)) == [9, 17, 3, 5, 30]
    assert list(exspec.rank_line_trace(lines, 2)) == [2, 8]
    assert list(exspec.rank_line_trace(lines, 0, maxlines=2)) == [9, 17]
    assert len(exspec.rank_line_trace(np.zeros((40, 4)), 0)) == 0
    rng = np.random.default_rng(3)
    big = np.zeros((3000, 4))
    big[:, 0] = rng.integers(0, 50, 3000)                # many ties, many zeros, more than 500 positive
    big[:, 2] = rng.random(3000) * (rng.random(3000) < 0.4)
    assert (big[:, 0] > 0).sum() > 500 and (big[:, 2] > 0).sum() > 500
    for col in (0, 2):
        got = exspec.rank_line_trace(big, col)
        assert len(got) == 500 and np.array_equal(got, _numpy_rank(big, col))
        assert np.array_equal(exspec.rank_line_trace(big, col, maxlines=3000), _numpy_rank(big, col, 3000))
    with pytest.raises(ValueError):
        exspec.rank_line_trace(big, 1)


def test_writer(tmp_path, small_model):
    a = T.atomic(small_model)
    nlines = small_model.nlines
    assert nlines == a["nlines"] >= 2000
    regions = [T.REGIONS[1], T.REGIONS[3], T.REGIONS[0]]
    arr = ffi.LineTraceArrays(nlines, 3)
    rng = np.random.default_rng(5)
    # region 0: 700 emitting lines (cut at 500) with ties, 30 absorbing lines
    em = rng.choice(nlines, 700, replace=False)
    arr.lines[0, em, 0] = rng.integers(1, 200, 700) * 1e-13
    arr.lines[0, em, 1] = arr.lines[0, em, 0] * rng.uniform(2e8, 9e8, 700)
    ab = rng.choice(nlines, 30, replace=False)
    arr.lines[0, ab, 2] = rng.uniform(1e-14, 1e-12, 30)
    arr.lines[0, ab, 3] = arr.lines[0, ab, 2] * rng.uniform(2e8, 9e8, 30)
    arr.totals[0] = arr.lines[0, :, 0].sum() * 1.25, arr.lines[0, :, 2].sum()
    # region 1: nothing at all (totals zero: no row, so no division by them); region 2: one absorbing line only
    arr.lines[2, 123, 2:] = 3e-12, 3e-12 * 4.5e8
    arr.totals[2] = 0., 3e-12
    path = tmp_path / exspec.LINE_TRACE_FILE
    exspec.write_line_trace(path, small_model, arr, regions)
    text = path.read_text()
    assert "nan" not in text.lower() and "inf" not in text.lower()
    blocks = T.parse_trace(path)
    assert len(blocks) == 3
    for b, reg in zip(blocks, regions):
        assert b["time"] == (reg[0], reg[1]) and np.allclose(b["lambda"], reg[2:], rtol=0, atol=0.051)
    b0 = blocks[0]
    for name, col in (("emission", 0), ("absorption", 2)):
        rows = b0[name]["rows"]
        ranked = exspec.rank_line_trace(arr.lines[0], col)
        assert np.array_equal(ranked, _numpy_rank(arr.lines[0], col))
        assert len(rows) == len(ranked) == (500 if col == 0 else 30)
        assert [T.row_identity(r) for r in rows] == [T.line_identity(a, li) for li in ranked]
        total = arr.totals[0, col // 2]
        assert np.isclose(b0[name]["total"], total, rtol=1e-5)
        for k in (0, 1, 7, len(rows) - 1):
            li, row = ranked[k], rows[k]
            lam, B_lu, B_ul = T.line_columns(a, li)
            e = arr.lines[0, li, col]
            assert np.isclose(row["energy"], e, rtol=6e-3)                      # %7.2e
            assert abs(row["percent"] - 100 * e / total) <= 0.051               # %5.1f
            assert abs(row["lambda"] - lam) <= 0.051                            # %7.1f
            assert abs(row["v_rad"] - arr.lines[0, li, col + 1] / e / 1e5) <= 0.051
            assert np.isclose(row["B_lu"], B_lu, rtol=6e-2) and np.isclose(row["B_ul"], B_ul, rtol=6e-2)  # %7.1e
            assert np.isclose(row["A"], a["line_einstein_A"][li], rtol=6e-3)
            assert abs(row["coll_str"] - a["line_coll_str"][li]) <= 0.051
            assert row["forb"] == a["line_forbidden"][li]
    assert blocks[1]["emission"] == {"total": 0., "rows": []} and blocks[1]["absorption"] == {"total": 0., "rows": []}
    assert blocks[2]["emission"]["rows"] == [] and len(blocks[2]["absorption"]["rows"]) == 1
    assert T.row_identity(blocks[2]["absorption"]["rows"][0]) == T.line_identity(a, 123)
    assert blocks[2]["absorption"]["rows"][0]["percent"] == 100.
    # the arrays must belong to the regions and the model
    with pytest.raises(ValueError):
        exspec.write_line_trace(path, small_model, arr, regions[:2])
