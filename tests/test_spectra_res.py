"""The exspec output set on the host (artis_amd/exspec.py, ffi.SpectraResArrays): file names and contents of
write_outputs against the oracle's per-bin arrays, the slot views, the chunk planner.  CPU only."""
import os

import numpy as np
import pytest

import oracle_lib
import spectra_res_lib as S
from artis_amd import exspec, ffi

_cache = {}


def _oracle_set(model):
    """The oracle's average + 100 direction bins (emission and Stokes on) for 4000 packets, seed 26; made once and
    left unchanged."""
    if "set" not in _cache:
        model.set_timestep(S.NTS)
        pk = model.init_rpackets(S.NTS, 4000, seed=26)
        oracle_lib.update_packets(model, S.NTS, pk)
        _cache["set"] = (pk, S.oracle_res(model, pk, emission_res=True, stokes=True))
    return _cache["set"]


def test_write_outputs_file_set_and_contents(tmp_path, small_model):
    pk, arr = _oracle_set(small_model)
    esc = (pk["type"] == ffi.TYPE_ESCAPE) & (pk["escape_type"] == ffi.TYPE_RPKT)
    assert esc.sum() == 1292
    assert all(arr.slot(a).flux.any() and arr.slot(a).absorption.any() for a in range(ffi.MABINS))
    written = exspec.write_outputs(tmp_path, small_model, arr)
    # exactly the file set of exspec.cc:205-250 with do_emission_res and POL_ON
    expect = ["light_curve.out", "gamma_light_curve.out", "spec.out", "emission.out", "emissiontrue.out",
              "absorption.out", "specpol.out", "emissionpol.out", "absorptionpol.out", "gamma_spec.out"]
    for a in range(100):
        expect += [f"{stem}_res_{a:02d}.out" for stem in (
            "light_curve", "spec", "emission", "emissiontrue", "absorption", "specpol", "emissionpol",
            "absorptionpol")]
    assert sorted(os.listdir(tmp_path)) == sorted(expect) == written
    assert written == exspec.file_set(range(-1, 100), emission_res=True, stokes=True)
    nt, nnb = small_model.cfg.ntstep, S.NNUBINS
    o5 = oracle_lib.spectra(small_model, pk, nnubins=nnb, abin=5, syn_dir=S.SYN_DIR, emission_res=True, stokes=True)
    assert o5.flux.any() and o5.lc_lum.any()
    S.assert_file_close(S.read_spec(tmp_path / "spec_res_05.out"), o5.flux, "spec_res_05.out")
    lc = np.array(S.rows(tmp_path / "light_curve_res_05.out"))
    assert lc.shape == (nt, 3)  # a direction bin has no deposition rows (light_curve.cc:21)
    S.assert_file_close(lc[:, 1] * S.LSUN, o5.lc_lum, "light_curve_res_05.out")
    assert not lc[:, 2].any()
    em = S.rows(tmp_path / "emission_res_37.out")
    assert len(em) == nnb * nt and all(len(r) == arr.proccount for r in em)
    o37 = oracle_lib.spectra(small_model, pk, nnubins=nnb, abin=37, syn_dir=S.SYN_DIR, emission_res=True, stokes=True)
    S.assert_file_close(S.read_columns(tmp_path / "emission_res_37.out", nnb, nt), o37.emission, "emission_res_37.out")
    # the angle-averaged files hold slot -1
    om = oracle_lib.spectra(small_model, pk, nnubins=nnb, abin=-1, syn_dir=S.SYN_DIR, emission_res=True, stokes=True)
    S.assert_file_close(S.read_spec(tmp_path / "spec.out"), om.flux, "spec.out")
    S.assert_file_close(S.read_specpol(tmp_path / "specpol.out", nt), om.stokes_flux, "specpol.out")
    assert len(S.rows(tmp_path / "light_curve.out")) == 2 * nt
    # gamma_spec.out: the shape of spec.out, zero flux (spectrum.cc:349-350)
    spec_rows, gam_rows = S.rows(tmp_path / "spec.out"), S.rows(tmp_path / "gamma_spec.out")
    assert [len(r) for r in gam_rows] == [len(r) for r in spec_rows] and len(gam_rows) == nnb + 1
    assert gam_rows[0] == spec_rows[0]
    g = np.array(gam_rows[1:])
    assert not g[:, 1:].any() and np.all(g[:, 0] > 1e18)  # bin centres of [0.05, 4] MeV


def test_write_outputs_without_emission_res(tmp_path, small_model):
    _, arr = _oracle_set(small_model)
    written = exspec.write_outputs(tmp_path, small_model, arr, emission_res=False, stokes=False)
    expect = ["light_curve.out", "gamma_light_curve.out", "spec.out", "gamma_spec.out"]
    for a in range(100):
        expect += [f"light_curve_res_{a:02d}.out", f"spec_res_{a:02d}.out"]
    assert sorted(os.listdir(tmp_path)) == sorted(expect) == written
    assert not any("emission" in n or "absorption" in n for n in os.listdir(tmp_path))


def test_write_outputs_1d_model_gets_the_average_only(tmp_path, shell_model):
    """exspec.cc:140: amax = 0 for RHO_1D_READ."""
    assert exspec.is_1d_read(shell_model)
    arr = ffi.SpectraResArrays(shell_model.cfg.ntstep, S.NNUBINS, shell_model.nelements, shell_model.maxnions, 0, 3,
                               True, True, True)
    arr.flux[:] = 1.
    written = exspec.write_outputs(tmp_path, shell_model, arr)
    assert sorted(os.listdir(tmp_path)) == written == exspec.file_set([-1], emission_res=True, stokes=True)
    assert len(written) == 10 and not any("_res_" in n for n in written)
    assert exspec.plan_chunks(None, 1, nbins=0) == [(0, 0, True)]


@pytest.mark.parametrize("with_average", [True, False])
def test_slot_views_alias_the_block(with_average):
    arr = ffi.SpectraResArrays(4, 5, 2, 3, abin_first=37, abin_count=6, with_average=with_average, emission_res=True,
                               stokes=True)
    off = 1 if with_average else 0
    assert arr.nslots == 6 + off and arr.flux.shape == (6 + off, 4, 5)
    assert arr.stokes_emission.shape == (6 + off, 3, 4, 5, arr.proccount) and arr.lc_lum.shape == (6 + off, 4)
    assert arr.abins() == ([-1] if with_average else []) + list(range(37, 43))
    for k, abin in enumerate(arr.abins()):
        v = arr.slot(abin)
        assert arr.slot_index(abin) == k
        for name in arr.SLOTTED:
            view, parent = getattr(v, name), getattr(arr, name)
            assert np.shares_memory(view, parent) and view.shape == parent.shape[1:], name
            view[...] = 100 * k + 1  # through the view ...
            assert np.all(parent[k] == 100 * k + 1), name  # ... into the parent
        assert (v.lc_lumcmf is arr.lc_lumcmf and v.gamma_lc_lum is arr.gamma_lc_lum) if abin == -1 else \
            (v.lc_lumcmf is None and v.gamma_lc_lum is None)
    # slot k of every block holds k's value and nothing else: the order is average first, then the bins
    assert [int(arr.flux[k, 0, 0]) for k in range(arr.nslots)] == [100 * k + 1 for k in range(arr.nslots)]
    if not with_average:
        assert arr.lc_lumcmf is None and arr.gamma_lc_lum is None and not arr.struct.lc_lumcmf
        with pytest.raises(KeyError):
            arr.slot(-1)
    for bad in (36, 43, 100):
        with pytest.raises(KeyError):
            arr.slot(bad)
    with pytest.raises(ValueError):
        ffi.SpectraResArrays(4, 5, 2, 3, abin_first=99, abin_count=2)
    with pytest.raises(ValueError):
        ffi.SpectraResArrays(4, 5, 2, 3, abin_first=0, abin_count=0, with_average=False)


@pytest.mark.parametrize("slots", [1, 37, 101, None])
def test_chunk_planner_covers_every_bin_once(slots):
    per_slot = exspec.slot_bytes(30, S.NNUBINS, 3, 4, True, True)
    assert per_slot == ffi.SpectraResArrays(30, S.NNUBINS, 3, 4, 5, 1, False, True, True).flux.nbytes * (
        1 + 2 * 25 + 12 + 3 * (1 + 25 + 12)) + 8 * 30
    budget = None if slots is None else slots * per_slot + per_slot // 2
    chunks = exspec.plan_chunks(budget, per_slot)
    bins = [a for first, count, _ in chunks for a in range(first, first + count)]
    assert bins == list(range(100))
    assert [avg for _, _, avg in chunks] == [True] + [False] * (len(chunks) - 1)
    cap = 101 if slots is None else slots
    assert all(count + int(avg) <= cap for _, count, avg in chunks)
    assert len(chunks) == -(-101 // cap)  # no chunk smaller than the budget allows
    for first, count, avg in chunks:  # every chunk is a request SpectraResArrays accepts
        assert count > 0 or avg
    with pytest.raises(ValueError):
        exspec.plan_chunks(per_slot - 1, per_slot)
