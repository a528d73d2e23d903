"""artis_gpu_line_trace (k_line_trace): the per-line emission / absorption trace of add_to_spec
(TRACE_EMISSION_ABSORPTION_REGION_ON, spectrum.cc:395-447) for several regions in one pass over the resident packets,
against the numpy restatement of tests/line_trace_lib.py and against artis_gpu_spectra; regions, ranks, ADD,
hand-made boundary packets, refusals, and the two drivers (artis_amd.exspec.run with trace_regions, artis_gpu_driver
with ARTIS_DRIVER_EXSPEC_TRACE)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import line_trace_lib as T
from artis_amd import exspec, ffi

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, "artis_amd", "lib", "artis_gpu_driver")
BAD_ARGUMENT = -3  # ARTIS_ERR_BAD_ARGUMENT
ERR_HIP = -2       # ARTIS_ERR_HIP: what a failed device allocation returns
SYN_DIR = (0.3, 0.4, float(np.sqrt(0.75)))


@pytest.fixture(scope="module")
def eng(small_model):
    from artis_amd import Engine

    e = Engine(small_model)
    yield e
    e.close()


def _propagate(eng, model, nts, pk):
    """Engine-propagated packets (as tests/test_gpu_spectra_res.py): pk is updated in place."""
    model.set_timestep(nts)
    eng.upload_cellstate(nts)
    eng.update_packets(nts, pk)
    return pk


@pytest.fixture(scope="module")
def pk20k(eng, small_model):
    return _propagate(eng, small_model, T.NTS, small_model.init_rpackets(T.NTS, 20000, seed=26))


@pytest.fixture(scope="module")
def ref20k(small_model, pk20k):
    """The numpy reference of the four regions for pk20k; computed once and left unchanged."""
    return T.reference(small_model, pk20k, T.REGIONS)


@pytest.fixture(scope="module")
def sets4k(eng, small_model):
    return [_propagate(eng, small_model, T.NTS, small_model.init_rpackets(T.NTS, 4000, seed=s)) for s in (26, 27)]


def _trace(eng, regions, **kw):
    kw.setdefault("nnubins", T.NNUBINS)
    return eng.line_trace(regions, **kw)


def _pair(arr):
    return arr.lines, arr.totals


def test_propagated_packets_against_the_numpy_reference(eng, pk20k, ref20k):
    lines, totals = ref20k
    # an empty comparison cannot pass
    for r in range(3):
        assert (lines[r, :, 0] > 0).sum() >= 500 and (lines[r, :, 2] > 0).sum() >= 500, r
        assert (lines[r, :, 1] > 0).sum() >= 500 and (lines[r, :, 3] > 0).sum() >= 500, r
        assert totals[r, 0] > 0 and totals[r, 1] > 0
    assert not lines[3].any() and not totals[3].any()
    # the branch that drops an absorption outside the binned band is taken
    g = T.geometry(eng.model)
    esc = pk20k[(pk20k["type"] == ffi.TYPE_ESCAPE) & (pk20k["escape_type"] == ffi.TYPE_RPKT)]
    af = esc["absorptionfreq"][esc["absorptiontype"] >= 0]
    assert ((af <= g["nu_min"]) | (af >= g["nu_max"])).any()
    eng.upload(pk20k)
    got = _trace(eng, T.REGIONS)
    T.assert_close(ref20k, _pair(got), "20000 propagated packets")
    assert not got.lines[3].any() and not got.totals[3].any()


def test_identity_with_the_spectra(eng, small_model, pk20k):
    """Summed over an ion's lines, the trace of a region that holds every admitted packet is that ion's bound-bound
    trueemission / absorption column of artis_gpu_spectra, for the angle average and for a direction bin."""
    a = T.atomic(small_model)
    ioncount = small_model.nelements * small_model.maxnions
    ionof = a["line_elementindex"] * a["maxnions"] + a["line_ionindex"]
    eng.upload(pk20k)
    for abin in (-1, 0, 37, 99):
        tr = _trace(eng, T.REGIONS[:1], abin=abin, syn_dir=SYN_DIR)
        s = eng.spectra(nnubins=T.NNUBINS, abin=abin, syn_dir=SYN_DIR, emission_res=True)
        assert s.flux.any(), abin
        for col, spec in ((0, s.trueemission.sum((0, 1))[:ioncount]), (2, s.absorption.sum((0, 1)))):
            per_ion = np.bincount(ionof, tr.lines[0, :, col], ioncount)
            err, scale = np.abs(per_ion - spec).max(), np.abs(spec).max()
            print(f"abin {abin} column {col}: max|a-b| {err:.3e} max|a| {scale:.3e}")
            assert scale > 0 and err <= T.RTOL_SUMS * scale, (abin, col, err, scale)
            total = tr.totals[0, col // 2]
            assert abs(total - spec.sum()) <= T.RTOL_SUMS * spec.sum(), (abin, col, total, spec.sum())
        ref = T.reference(small_model, pk20k, T.REGIONS[:1], abin=abin, syn_dir=SYN_DIR)
        T.assert_close(ref, _pair(tr), f"abin {abin}")


def test_regions_ranks_and_add(eng, small_model, pk20k, ref20k, sets4k):
    eng.upload(pk20k)
    four = _trace(eng, T.REGIONS)
    for r, reg in enumerate(T.REGIONS):
        one = _trace(eng, [reg])
        T.assert_close((four.lines[r:r + 1], four.totals[r:r + 1]), _pair(one), f"region {r} alone")
    # ADD: a pre-filled out keeps what it held
    pre = ffi.LineTraceArrays(small_model.nlines, len(T.REGIONS))
    pre.lines[...] = four.lines
    pre.totals[...] = four.totals
    assert _trace(eng, T.REGIONS, out=pre) is pre
    T.assert_close((2 * ref20k[0], 2 * ref20k[1]), _pair(pre), "added to a pre-filled out")
    # the rank loop: two packet sets into one out with nprocs 2
    out, expect = None, None
    for pk in sets4k:
        eng.upload(pk)
        out = _trace(eng, T.REGIONS, nprocs=2, out=out)
        expect = T.reference(small_model, pk, T.REGIONS, nprocs=2, out=expect)
    assert expect[1][:3].all() and not expect[0][3].any()
    T.assert_close(expect, _pair(out), "two ranks")


def _handmade(model, n=4099):
    """Escaped r-packets at pos 0 (t_arrive == escape_time exactly) on three lines, with the rows that must add
    nothing and the rows on the region bounds mixed in.  Returns (packets, regions)."""
    g = T.geometry(model)
    t0, t1 = 6.0, 6.25                              # days; whole seconds
    T0, T1 = int(t0 * T.DAY), int(t1 * T.DAY)
    assert t0 * T.DAY == T0 and t1 * T.DAY == T1 and g["tmin"] < T0 - 30000 and T1 + 30000 < g["tmax"]
    lmin, lmax = 2000., 5000.
    NL, NU = 1.e8 * T.CLIGHT / lmax, 1.e8 * T.CLIGHT / lmin
    assert g["nu_min"] < 0.8 * NL and 1.2 * NU < g["nu_max"]

    def days_above(sec):  # the smallest day count whose product with DAY lies above sec
        d = sec / T.DAY
        while d * T.DAY <= sec:
            d = np.nextafter(d, np.inf)
        return float(d)

    def days_below(sec):
        d = sec / T.DAY
        while d * T.DAY >= sec:
            d = np.nextafter(d, -np.inf)
        return float(d)

    regions = [(t0, t1, lmin, lmax),                            # bounds on the boundary packets: counted
               (days_above(T0), days_below(T1), lmin, lmax),    # time bounds just inside them: not counted
               (3., 30., 599., 29980.)]                         # wider than the binned band
    rng = np.random.default_rng(41)
    lines3 = np.array([5, model.nlines // 2, model.nlines - 1], dtype=np.int32)
    i = np.arange(n)
    pk = np.zeros(n, dtype=ffi.PACKET_DTYPE)
    pk["type"] = ffi.TYPE_ESCAPE
    pk["escape_type"] = ffi.TYPE_RPKT
    pk["dir"][:, 2] = 1.
    pk["e_rf"] = rng.uniform(1e38, 2e38, n)
    pk["e_cmf"] = pk["e_rf"]
    pk["nu_rf"] = rng.uniform(0.8 * NL, 1.2 * NU, n)
    pk["escape_time"] = rng.integers(T0 - 20000, T1 + 20000, n)
    pk["trueemissiontype"] = lines3[(i // 64) % 3]   # whole waves on one record
    pk["trueemissionvelocity"] = rng.uniform(2e8, 9e8, n).astype(np.float32)
    pk["absorptiontype"] = np.where(i % 5 == 0, -1, lines3[(i // 7) % 3])
    pk["absorptionfreq"] = rng.uniform(1.2 * g["nu_min"], 0.8 * g["nu_max"], n)
    pk["absorptionfreq"][i % 11 == 3] = 0.5 * g["nu_min"]       # an absorbing line outside the binned band
    pk["absorptionfreq"][i % 11 == 7] = 2. * g["nu_max"]
    pk["em_pos"] = rng.uniform(-1e14, 1e14, (n, 3))
    pk["em_time"] = rng.integers(300000, 500000, n)
    k = i % 32
    inside = rng.integers(T0 + 1, T1, n)
    pk["escape_time"][k == 6] = T0
    pk["escape_time"][k == 7] = T1
    pk["escape_time"][k == 22] = T0 - 1
    pk["escape_time"][k == 23] = T1 + 1
    for kk, nu in ((8, NL), (9, NU), (10, np.nextafter(NL, 0.)), (11, np.nextafter(NU, np.inf))):
        pk["nu_rf"][k == kk] = nu
        pk["escape_time"][k == kk] = inside[k == kk]
    pk["type"][k == 12] = ffi.TYPE_RPKT                         # not escaped
    pk["escape_type"][k == 13] = ffi.TYPE_GAMMA                 # an escaped gamma packet
    nothing = k == 14                                           # admitted, but no line emitted or absorbed it
    pk["trueemissiontype"][nothing] = np.array([-1, -9999999, -3], dtype=np.int32)[(i[nothing] // 32) % 3]
    pk["absorptiontype"][nothing] = -1
    pk["absorptionfreq"][nothing] = 0.
    pk["nu_rf"][k == 15] = np.where(i[k == 15] % 64 < 32, 0.5 * g["nu_min"], 2. * g["nu_max"])
    pk["escape_time"][k == 31] = np.where(i[k == 31] % 64 < 32, int(g["tmin"]) - 5, int(g["tmax"]) + 5)
    for kk in (6, 7, 22, 23):                                   # the time rows lie inside the frequency window
        pk["nu_rf"][k == kk] = rng.uniform(NL, NU, (k == kk).sum())
    return pk, regions


def test_handmade_packets_on_the_bounds(eng, small_model):
    pk, regions = _handmade(small_model)
    assert len(pk) % 256 != 0 and len(pk) % 64 != 0
    ref = T.reference(small_model, pk, regions)
    lines, totals = ref
    # only the three lines; the boundary packets separate region 0 from region 1; region 2 holds more than both
    assert (lines[:, :, 0] > 0).sum(1).tolist() == [3, 3, 3] and (lines[:, :, 2] > 0).sum(1).tolist() == [3, 3, 3]
    assert (totals[2] > totals[0]).all() and (totals[0] > totals[1]).all() and (totals[1] > 0).all()
    # each kind of row on a bound changes the reference when it is dropped: the bounds are exercised
    k = np.arange(len(pk)) % 32
    for kk in (6, 7, 8, 9):
        less = T.reference(small_model, pk[k != kk], regions[:1])
        assert less[1][0, 0] < totals[0, 0], kk
    for kk in (10, 11, 12, 13, 14, 15, 22, 23, 31):
        same = T.reference(small_model, pk[k != kk], regions[:1])
        assert np.array_equal(same[0][0], lines[0]), kk
    eng.upload(pk)
    got = _trace(eng, regions)
    T.assert_close(ref, _pair(got), "hand-made packets")
    # the same through the direction bin that holds them all (every dir is z), and through another bin
    b = int(T.escapedirectionbin(pk["dir"][:1], SYN_DIR)[0])
    assert 0 <= b < T.MABINS
    gotb = _trace(eng, regions, abin=b, syn_dir=SYN_DIR)
    T.assert_close((T.MABINS * lines, T.MABINS * totals), _pair(gotb), "hand-made packets, their direction bin")
    other = _trace(eng, regions, abin=(b + 50) % 100, syn_dir=SYN_DIR)
    assert not other.lines.any() and not other.totals.any()
    # one packet; no escaped packet
    traced = np.flatnonzero((k == 6) & (pk["absorptiontype"] >= 0))[:1]
    eng.upload(pk[traced])
    one = _trace(eng, regions)
    T.assert_close(T.reference(small_model, pk[traced], regions), _pair(one), "one packet")
    assert one.totals[0, 0] > 0 and one.totals[1, 0] == 0
    eng.upload(pk[k == 12])
    none = _trace(eng, regions)
    assert not none.lines.any() and not none.totals.any()


def _refusal_cases(model):
    """(label, request or None, arrays or None) for every refusal of include/artis_gpu.h; the arrays pre-filled."""
    def arrays(nregions=2):
        a = ffi.LineTraceArrays(model.nlines, nregions)
        a.lines[...] = 7.
        a.totals[...] = 7.
        return a

    def req(regions=T.REGIONS[:2], **kw):
        base = dict(nnubins=T.NNUBINS, nprocs=1, abin=-1, syn_dir=SYN_DIR)
        base.update(kw)
        return ffi.line_trace_request(list(regions), **base)

    def nulled(field):
        a = arrays()
        setattr(a.struct, field, None)
        return a

    def bent(field, value, other=None):
        r = req()
        setattr(r.regions[1], field, value)
        if other:
            setattr(r.regions[1], *other)
        return r

    no_regions = req()
    no_regions.regions = None
    cases = [
        ("NULL request", None, arrays()),
        ("NULL output", req(), None),
        ("NULL lines", req(), nulled("lines")),
        ("NULL totals", req(), nulled("totals")),
        ("NULL regions", no_regions, arrays()),
        ("nnubins 0", req(nnubins=0), arrays()),
        ("nnubins < 0", req(nnubins=-5), arrays()),
        ("nprocs 0", req(nprocs=0), arrays()),
        ("abin -2", req(abin=-2), arrays()),
        ("abin MABINS", req(abin=ffi.MABINS), arrays()),
        ("no regions", req(regions=[]), arrays()),
        ("17 regions", req(regions=[T.REGIONS[0]] * 17), arrays(17)),
        ("nu_lower > nu_upper", bent("nu_lower", 2e15, ("nu_upper", 1e15)), arrays()),
        ("time_min > time_max", bent("time_min", 6e5, ("time_max", 5e5)), arrays()),
    ]
    for field in ("nu_lower", "nu_upper", "time_min", "time_max"):
        cases.append((f"{field} NaN", bent(field, float("nan")), arrays()))
        # the infinity that keeps lower <= upper, so that only the finiteness test can refuse it
        inf = float("inf") if field in ("nu_upper", "time_max") else float("-inf")
        cases.append((f"{field} infinite", bent(field, inf), arrays()))
    return cases


def test_refusals_leave_the_arrays_and_the_engine_alone(eng, small_model, pk20k, ref20k):
    eng.upload(pk20k)
    lib = eng.lib
    for label, req, out in _refusal_cases(small_model):
        rc = lib.artis_gpu_line_trace(C.byref(req) if req is not None else None,
                                      C.byref(out.struct) if out is not None else None)
        assert rc == BAD_ARGUMENT, (label, rc)
        msg = lib.artis_gpu_last_error().decode()
        assert msg.startswith("line_trace:"), (label, msg)
        if out is not None:
            assert np.all(out.lines == 7.) and np.all(out.totals == 7.), label
    # device memory: an allocation that fails is the HIP status, says the bytes, adds nothing
    out = ffi.LineTraceArrays(small_model.nlines, len(T.REGIONS))
    req = ffi.line_trace_request(T.REGIONS, T.NNUBINS)
    os.environ["ARTIS_GPU_FAIL_ALLOC_ABOVE"] = str(1 << 19)
    try:
        rc = lib.artis_gpu_line_trace(C.byref(req), C.byref(out.struct))
    finally:
        del os.environ["ARTIS_GPU_FAIL_ALLOC_ABOVE"]
    msg = lib.artis_gpu_last_error().decode()
    nbytes = 8 * T.NNUBINS + out.lines.nbytes + out.totals.nbytes
    assert nbytes > 1 << 19
    assert rc == ERR_HIP and msg.startswith("line_trace:") and str(nbytes) in msg, (rc, msg)
    assert not out.lines.any() and not out.totals.any()
    # the engine still answers: the same request now succeeds and gives the reference result
    assert lib.artis_gpu_line_trace(C.byref(req), C.byref(out.struct)) == 0
    T.assert_close(ref20k, _pair(out), "after the refusals")


def _check_trace_file(path, model, regions, ref, nrows=20):
    """The file's blocks against the reference arrays: totals to the writer's digits and, for the second region, the
    first rows of both tables naming the lines rank_line_trace gives for the reference."""
    a = T.atomic(model)
    blocks = T.parse_trace(path)
    assert len(blocks) == len(regions)
    lines, totals = ref
    for r, b in enumerate(blocks):
        for name, col in (("emission", 0), ("absorption", 2)):
            assert np.isclose(b[name]["total"], totals[r, col // 2], rtol=1e-5, atol=0), (r, name)  # %g
            assert len(b[name]["rows"]) == min(500, (lines[r, :, col] > 0).sum()), (r, name)
    for name, col in (("emission", 0), ("absorption", 2)):
        ranked = exspec.rank_line_trace(lines[1], col)
        e = lines[1, ranked[:nrows + 1], col]
        assert len(e) == nrows + 1 and (e[:-1] - e[1:] > 1e-6 * e[:-1]).all(), "the reference's order is not well defined"
        rows = blocks[1][name]["rows"][:nrows]
        assert [T.row_identity(x) for x in rows] == [T.line_identity(a, li) for li in ranked[:nrows]], name


def test_exspec_run_with_trace_regions(eng, small_model, pk20k, ref20k, sets4k, tmp_path):
    usual = exspec.file_set(range(-1, 100), True, False)
    # the resident packets
    eng.upload(pk20k)
    res = exspec.run(eng, tmp_path / "resident", nnubins=T.NNUBINS, syn_dir=SYN_DIR, trace_regions=T.REGIONS)
    assert len(res) == 3
    written, arrays, trace = res
    assert written == sorted(usual + [exspec.LINE_TRACE_FILE]) == sorted(os.listdir(tmp_path / "resident"))
    assert arrays.nslots == 101 and isinstance(trace, ffi.LineTraceArrays)
    T.assert_close(ref20k, _pair(trace), "exspec.run, resident packets")
    _check_trace_file(tmp_path / "resident" / exspec.LINE_TRACE_FILE, small_model, T.REGIONS, ref20k)
    # two rank files, in chunks of 37 slots: every file is traced once
    files, expect = [], None
    for rank, pk in enumerate(sets4k):
        files.append(tmp_path / f"packets_{rank:04d}_ts{T.NTS}.tmp")
        pk.tofile(files[-1])
        expect = T.reference(small_model, pk, T.REGIONS, nprocs=2, out=expect)
    per_slot = exspec.slot_bytes(small_model.cfg.ntstep, T.NNUBINS, small_model.nelements, small_model.maxnions, True,
                                 False)
    written, first, trace = exspec.run(eng, tmp_path / "ranks", files, nnubins=T.NNUBINS, syn_dir=SYN_DIR,
                                       max_bytes=37 * per_slot, trace_regions=T.REGIONS)
    assert written == sorted(usual + [exspec.LINE_TRACE_FILE]) == sorted(os.listdir(tmp_path / "ranks"))
    assert first.nslots == 37
    T.assert_close(expect, _pair(trace), "exspec.run, two rank files")
    _check_trace_file(tmp_path / "ranks" / exspec.LINE_TRACE_FILE, small_model, T.REGIONS, expect)
    # without the argument: two values and exactly the usual files
    eng.upload(pk20k)
    res = exspec.run(eng, tmp_path / "plain", nnubins=T.NNUBINS, syn_dir=SYN_DIR, emission_res=False)
    assert len(res) == 2
    assert res[0] == exspec.file_set(range(-1, 100), False, False) == sorted(os.listdir(tmp_path / "plain"))


def test_cpp_driver_writes_the_trace(tmp_path):
    """ARTIS_DRIVER_EXSPEC_TRACE: the C++ mirror's PacketEngine::line_trace and the C++ writer.  The driver's packets
    are its own, so names and shapes are compared, not values."""
    out = tmp_path / "exspec"
    args = [DRIVER, str(tmp_path), "10", "60", "20", "8000", "30", "8", "2", "20000", "5"]
    env = {**os.environ, "ARTIS_DRIVER_EXSPEC": str(out), "ARTIS_DRIVER_EXSPEC_NNUBINS": "40",
           "ARTIS_DRIVER_EXSPEC_TRACE": "1,100,599,29980;320,340,1000,25000"}
    r = subprocess.run(args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(out)) == sorted(exspec.file_set(range(-1, 100), True, True) + [exspec.LINE_TRACE_FILE])
    blocks = T.parse_trace(out / exspec.LINE_TRACE_FILE)
    assert len(blocks) == 2
    assert blocks[0]["time"] == (1., 100.) and blocks[1]["lambda"] == (1000., 25000.)
    rows = blocks[0]["emission"]["rows"]
    assert 0 < len(rows) <= 500 and blocks[0]["emission"]["total"] > 0
    e = [x["energy"] for x in rows]
    assert e == sorted(e, reverse=True) and all(x["Z"] > 0 and x["upper"] != x["lower"] for x in rows)
    assert all(np.isfinite(list(x.values())).all() for x in rows)
    assert blocks[1]["emission"]["rows"] == [] and blocks[1]["absorption"]["rows"] == []
