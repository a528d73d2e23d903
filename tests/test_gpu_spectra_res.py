"""artis_gpu_spectra_res (k_spectra_res): the angle average and the direction bins in one pass over the resident
packets, against the 101 artis_gpu_spectra passes it replaces and against the oracle; ranges, rank accumulation,
gamma packets, refusals, and the two drivers (artis_amd.exspec.run, artis_gpu_driver with ARTIS_DRIVER_EXSPEC)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
import spectra_res_lib as S
from artis_amd import EngineError, exspec, ffi

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, "artis_amd", "lib", "artis_gpu_driver")
BAD_ARGUMENT = -3  # ARTIS_ERR_BAD_ARGUMENT
ERR_HIP = -2       # ARTIS_ERR_HIP: what a failed device allocation returns


@pytest.fixture(scope="module")
def eng(small_model):
    from artis_amd import Engine

    e = Engine(small_model)
    yield e
    e.close()


def _propagate(eng, model, nts, pk):
    """Engine-propagated packets (as tests/test_spectrum.py:144): pk is updated in place."""
    model.set_timestep(nts)
    eng.upload_cellstate(nts)
    eng.update_packets(nts, pk)
    return pk


@pytest.fixture(scope="module")
def pk20k(eng, small_model):
    return _propagate(eng, small_model, S.NTS, small_model.init_rpackets(S.NTS, 20000, seed=26))


@pytest.fixture(scope="module")
def full(eng, pk20k):
    """One spectra_res call, average + 100 bins, emission and Stokes on; computed once and left unchanged."""
    eng.upload(pk20k)
    return eng.spectra_res(nnubins=S.NNUBINS, syn_dir=S.SYN_DIR, emission_res=True, stokes=True)


def _res(eng, **kw):
    return eng.spectra_res(nnubins=S.NNUBINS, syn_dir=S.SYN_DIR, emission_res=True, stokes=True, **kw)


def _one(eng, abin, **kw):
    return eng.spectra(nnubins=S.NNUBINS, abin=abin, syn_dir=S.SYN_DIR, emission_res=True, stokes=True, **kw)


def _oracle(model, pk, abin, nprocs=1):
    return oracle_lib.spectra(model, pk, nnubins=S.NNUBINS, nprocs=nprocs, abin=abin, syn_dir=S.SYN_DIR,
                              emission_res=True, stokes=True)


def test_one_pass_equals_101_passes_and_the_oracle(eng, small_model, pk20k, full):
    esc = (pk20k["type"] == ffi.TYPE_ESCAPE) & (pk20k["escape_type"] == ffi.TYPE_RPKT)
    assert esc.sum() > 6000
    eng.upload(pk20k)
    for abin in range(-1, ffi.MABINS):
        got = full.slot(abin).arrays()
        o = _oracle(small_model, pk20k, abin).arrays()
        g = _one(eng, abin).arrays()
        if abin >= 0:  # a direction bin has no cmf and no gamma-ray light curve: the single-bin arrays stay zero
            for name in ("lc_lumcmf", "gamma_lc_lum", "gamma_lc_lumcmf"):
                assert not o.pop(name).any() and not g.pop(name).any()
        assert set(got) == set(o) == set(g)
        S.assert_sums_close(o, got, f"oracle, abin {abin}")
        S.assert_sums_close(g, got, f"artis_gpu_spectra, abin {abin}")
        # an empty comparison cannot pass: every bin has flux and absorption in a fair number of cells
        assert np.count_nonzero(got["flux"]) >= 31 and got["absorption"].any() and got["emission"].any(), abin
        assert got["lc_lum"].any() and got["stokes_flux"][0].any(), abin
    assert full.slot(-1).stokes_flux[1].any(), "Stokes Q is zero: the polarised blocks are not exercised"
    assert full.lc_lumcmf.any()
    # the bins sum to MABINS times the average
    assert np.allclose(full.flux[1:].sum(0), ffi.MABINS * full.flux[0], rtol=1e-9, atol=0)


def test_ranges(eng, pk20k, full):
    eng.upload(pk20k)
    a = _res(eng, abin_first=0, abin_count=37, with_average=False)
    assert a.nslots == 37 and a.lc_lumcmf is None
    for abin in range(37):
        S.assert_sums_close(full.slot(abin), a.slot(abin), f"[0, 37) bin {abin}")
    b = _res(eng, abin_first=37, abin_count=63, with_average=True)
    assert b.nslots == 64
    for abin in [-1] + list(range(37, 100)):
        S.assert_sums_close(full.slot(abin), b.slot(abin), f"[37, 100) bin {abin}")
    c = _res(eng, abin_first=99, abin_count=1, with_average=False)
    S.assert_sums_close(full.slot(99), c.slot(99), "[99, 100)")
    g99 = _one(eng, 99).arrays()
    for name in ("lc_lumcmf", "gamma_lc_lum", "gamma_lc_lumcmf"):
        g99.pop(name)
    S.assert_sums_close(g99, c.slot(99), "[99, 100) against artis_gpu_spectra")
    d = _res(eng, abin_first=0, abin_count=0, with_average=True)
    assert d.nslots == 1
    S.assert_sums_close(full.slot(-1), d.slot(-1), "average only")
    S.assert_sums_close(_one(eng, -1), d.slot(-1), "average only against artis_gpu_spectra")
    assert c.slot(99).flux.any() and d.flux.any()


def test_rank_accumulation_and_exspec_run_on_files(eng, small_model, tmp_path):
    sets = [_propagate(eng, small_model, S.NTS, small_model.init_rpackets(S.NTS, 4000, seed=s)) for s in (26, 27)]
    out = None
    for pk in sets:
        eng.upload(pk)
        out = _res(eng, nprocs=2, out=out)
    expect = None
    for pk in sets:
        expect = S.oracle_res(small_model, pk, nprocs=2, emission_res=True, stokes=True, out=expect)
    assert all(expect.flux[k].any() and expect.absorption[k].any() for k in range(101))
    for abin in range(-1, ffi.MABINS):
        S.assert_sums_close(expect.slot(abin), out.slot(abin), f"two ranks, abin {abin}")
    # the same through the driver, from the two sets as raw rank packet files, in chunks of 37 slots
    files = []
    for rank, pk in enumerate(sets):
        files.append(tmp_path / f"packets_{rank:04d}_ts{S.NTS}.tmp")
        pk.tofile(files[-1])
    per_slot = exspec.slot_bytes(small_model.cfg.ntstep, S.NNUBINS, small_model.nelements, small_model.maxnions, True,
                                 True)
    written, first = exspec.run(eng, tmp_path / "chunked", files, nnubins=S.NNUBINS, syn_dir=S.SYN_DIR,
                                emission_res=True, stokes=True, max_bytes=37 * per_slot)
    assert written == exspec.file_set(range(-1, 100), True, True) and first.nslots == 37
    for abin in first.abins():
        S.assert_sums_close(out.slot(abin), first.slot(abin), f"exspec.run chunk 0, abin {abin}")
    S.assert_file_close(S.read_spec(tmp_path / "chunked" / "spec_res_99.out"), expect.slot(99).flux,
                        "spec_res_99.out of the last chunk")
    written, whole = exspec.run(eng, tmp_path / "whole", files, nnubins=S.NNUBINS, syn_dir=S.SYN_DIR,
                                emission_res=False, stokes=False, max_bytes=None)
    assert written == exspec.file_set(range(-1, 100), False, False) and whole.nslots == 101
    for abin in range(-1, ffi.MABINS):
        v = out.slot(abin)
        S.assert_sums_close({"flux": v.flux, "lc_lum": v.lc_lum}, whole.slot(abin), f"exspec.run, abin {abin}")


def test_gamma_packets(eng, small_model):
    pk = _propagate(eng, small_model, 0, small_model.init_pellets(4000, seed=5))
    escg = (pk["type"] == ffi.TYPE_ESCAPE) & (pk["escape_type"] == ffi.TYPE_GAMMA)
    assert escg.sum() >= 10
    r = _res(eng)
    g = _one(eng, -1)
    o = _oracle(small_model, pk, -1)
    assert o.gamma_lc_lum.any() and o.gamma_lc_lumcmf.any()
    for name in ("gamma_lc_lum", "gamma_lc_lumcmf", "lc_lumcmf"):
        S.assert_sums_close({name: getattr(o, name)}, r, f"oracle {name}")
        S.assert_sums_close({name: getattr(g, name)}, r, f"artis_gpu_spectra {name}")
    S.assert_sums_close(g, r.slot(-1), "average")
    for abin in range(ffi.MABINS):
        ga = _one(eng, abin).arrays()
        for name in ("lc_lumcmf", "gamma_lc_lum", "gamma_lc_lumcmf"):
            assert not ga.pop(name).any()
        S.assert_sums_close(ga, r.slot(abin), f"bin {abin}")
    # the gamma-ray curves belong to the average; a range beyond the last bin does not exist
    bins_only = ffi.SpectraResArrays(small_model.cfg.ntstep, S.NNUBINS, small_model.nelements, small_model.maxnions,
                                     0, 100, True, True, True)
    for kw in (dict(abin_first=0, abin_count=100, with_average=False), dict(abin_first=50, abin_count=51)):
        with pytest.raises(EngineError) as ei:
            _res(eng, out=bins_only, **kw)
        assert f"-> {BAD_ARGUMENT}:" in str(ei.value)
        assert not any(a.any() for a in bins_only.arrays().values())


def _refusal_cases(model):
    """(label, request, out-struct or None) for every refusal of include/artis_gpu.h; `out` arrays pre-filled."""
    def arrays(with_average=True, first=0, count=2):
        a = ffi.SpectraResArrays(model.cfg.ntstep, S.NNUBINS, model.nelements, model.maxnions, first, count,
                                 with_average, True, True)
        for v in a.arrays().values():
            v[...] = 7.
        return a

    def req(**kw):
        base = dict(nnubins=S.NNUBINS, nprocs=1, abin_first=0, abin_count=2, with_average=True, syn_dir=S.SYN_DIR)
        base.update(kw)
        return ffi.spectra_res_request(**base)

    def nulled(*fields, **kw):
        a = arrays(**kw)
        for f in fields:
            setattr(a.struct, f, None)
        return a

    no_avg = req(with_average=False)
    return [
        ("NULL request", None, arrays()),
        ("NULL output", req(), None),
        ("abin_first < 0", req(abin_first=-1), arrays()),
        ("abin_first > MABINS", req(abin_first=101, abin_count=0), arrays()),
        ("range past MABINS", req(abin_first=99, abin_count=2), arrays()),
        ("abin_count < 0", req(abin_count=-1), arrays()),
        ("abin_count > MABINS", req(abin_count=101), arrays()),
        ("no slots", req(abin_count=0, with_average=False), arrays()),
        ("nnubins 0", req(nnubins=0), arrays()),
        ("nprocs 0", req(nprocs=0), arrays()),
        ("emission without absorption", req(), nulled("absorption")),
        ("absorption without emission", req(), nulled("emission", "trueemission", "stokes_emission",
                                                      "stokes_absorption")),
        ("trueemission without emission", req(), nulled("emission", "absorption", "stokes_emission",
                                                        "stokes_absorption")),
        ("Stokes emission without emission", req(), nulled("emission", "trueemission", "absorption")),
        ("lc_lumcmf without the average", no_avg, nulled("gamma_lc_lum", "gamma_lc_lumcmf")),
        ("gamma_lc_lum without the average", no_avg, nulled("lc_lumcmf", "gamma_lc_lumcmf")),
        ("gamma_lc_lumcmf without the average", no_avg, nulled("lc_lumcmf", "gamma_lc_lum")),
    ]


def test_refusals_leave_the_arrays_and_the_engine_alone(eng, small_model, pk20k, full):
    eng.upload(pk20k)
    lib = eng.lib
    for label, req, out in _refusal_cases(small_model):
        rc = lib.artis_gpu_spectra_res(C.byref(req) if req is not None else None,
                                       C.byref(out.struct) if out is not None else None)
        assert rc == BAD_ARGUMENT, (label, rc)
        msg = lib.artis_gpu_last_error().decode()
        assert msg.startswith("spectra_res:"), (label, msg)
        if out is not None:
            assert all(np.all(v == 7.) for v in out.arrays().values()), label
    # device memory: an allocation that fails is the out-of-memory status, says the bytes, adds nothing
    out = ffi.SpectraResArrays(small_model.cfg.ntstep, S.NNUBINS, small_model.nelements, small_model.maxnions, 0, 100,
                               True, True, True)
    req = ffi.spectra_res_request(S.NNUBINS, 1, 0, 100, True, S.SYN_DIR)
    os.environ["ARTIS_GPU_FAIL_ALLOC_ABOVE"] = str(1 << 20)
    try:
        rc = lib.artis_gpu_spectra_res(C.byref(req), C.byref(out.struct))
    finally:
        del os.environ["ARTIS_GPU_FAIL_ALLOC_ABOVE"]
    msg = lib.artis_gpu_last_error().decode()
    nbytes = 8 * S.NNUBINS + sum(a.nbytes for a in out.arrays().values())
    assert rc == ERR_HIP and str(nbytes) in msg and "abin_count" in msg, (rc, msg)
    assert not any(a.any() for a in out.arrays().values())
    # the engine still answers: the same request now succeeds and gives the reference result
    assert lib.artis_gpu_spectra_res(C.byref(req), C.byref(out.struct)) == 0
    for abin in (-1, 0, 37, 99):
        S.assert_sums_close(full.slot(abin), out.slot(abin), f"after the refusals, abin {abin}")
    # k_spectra, which now shares the per-packet function with k_spectra_res, against the oracle
    g = _one(eng, 37)
    o = _oracle(small_model, pk20k, 37)
    S.assert_sums_close(o, g, "artis_gpu_spectra abin 37")
    assert o.flux.any() and o.emission.any() and o.absorption.any()


def test_exspec_run_on_resident_packets(eng, small_model, pk20k, tmp_path):
    eng.upload(pk20k)
    written, arr = exspec.run(eng, tmp_path, nnubins=S.NNUBINS, syn_dir=S.SYN_DIR, emission_res=True, stokes=True)
    assert sorted(os.listdir(tmp_path)) == written == exspec.file_set(range(-1, 100), True, True)
    assert len(written) == 10 + 100 * 8
    nt = small_model.cfg.ntstep
    o = _oracle(small_model, pk20k, 37)
    assert o.flux.any() and o.emission.any() and o.stokes_flux[0].any()
    S.assert_file_close(S.read_spec(tmp_path / "spec_res_37.out"), o.flux, "spec_res_37.out")
    S.assert_file_close(S.read_columns(tmp_path / "emission_res_37.out", S.NNUBINS, nt), o.emission,
                        "emission_res_37.out")
    S.assert_file_close(S.read_specpol(tmp_path / "specpol_res_37.out", nt), o.stokes_flux, "specpol_res_37.out")


def test_cpp_driver_writes_the_exspec_directory(tmp_path):
    """ARTIS_DRIVER_EXSPEC: the C++ mirror's PacketEngine::spectra_res and the same file set.  The driver's packets
    are its own, so names and shapes are compared, not values."""
    out = tmp_path / "exspec"
    nt = 30
    args = [DRIVER, str(tmp_path), "10", "60", "20", "8000", str(nt), "8", "2", "20000", "5"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "ARTIS_DRIVER_EXSPEC": str(out), "ARTIS_DRIVER_EXSPEC_NNUBINS": "40"})
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(out)) == exspec.file_set(range(-1, 100), True, True)
    for name in ("spec.out", "spec_res_00.out"):
        flux = S.read_spec(out / name)
        assert flux.shape == (nt, 40) and np.isfinite(flux).all() and flux.any(), name
    assert len(S.rows(out / "emission_res_99.out")) == 40 * nt
