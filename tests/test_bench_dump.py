"""bench.py --dump-outputs: the writer on a stand-in engine (no GPU): float arrays only, the same files from the same
inputs, the packet sample drawn from the ensemble by packet_index, and the byte budget kept."""
import os

import numpy as np

import bench


class _Engine:
    """What dump_outputs asks of an Engine: the estimators and the resident packets."""

    def __init__(self, model, packets):
        self.model, self.packets = model, packets

    def download_estimators(self):
        est = self.model.new_estimators()
        est.J[:] = np.arange(len(est.J))
        est.ecounter[:] = 3
        return est

    def download(self, out):
        out[:] = self.packets


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_is_reproducible_and_samples_packets(small_model, tmp_path):
    small_model.set_timestep(4)
    pk = small_model.init_rpackets(4, 3001, seed=7)
    eng = _Engine(small_model, pk)
    shapes = bench.dump_outputs(str(tmp_path / "a"), eng, pk)
    bench.dump_outputs(str(tmp_path / "b"), eng, pk)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(b) == sorted(shapes)
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert list(a[name].shape) == shapes[name]
        assert np.array_equal(a[name], b[name]), name
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_BUDGET_BYTES
    assert np.array_equal(a["est_J"], np.arange(small_model.npts_model))
    assert np.all(a["est_ecounter"] == 3)
    idx = a["packet_index"].astype(np.int64)
    assert len(idx) == len(pk) and np.array_equal(idx, np.arange(len(pk)))  # fewer packets than the sample: all
    col = 0
    for f in bench.DUMP_PACKET_FIELDS:
        v = np.asarray(pk[f], dtype=np.float64).reshape(len(pk), -1)
        assert np.array_equal(a["packets"][:, col:col + v.shape[1]], v), f
        col += v.shape[1]
    assert col == a["packets"].shape[1]


def test_dump_outputs_shrinks_the_sample_to_the_budget(small_model, tmp_path, monkeypatch):
    small_model.set_timestep(4)
    pk = small_model.init_rpackets(4, 3001, seed=7)
    eng = _Engine(small_model, pk)
    est_bytes = sum(x.nbytes for n, x in _dump(eng, pk, tmp_path / "full").items() if n.startswith("est_"))
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", est_bytes + 100 * 8 * 50)
    out = _dump(eng, pk, tmp_path / "small")
    assert sum(x.nbytes for x in out.values()) <= bench.DUMP_BUDGET_BYTES
    idx = out["packet_index"].astype(np.int64)
    assert 0 < len(idx) <= 100 and np.all(np.diff(idx) > 0) and idx[-1] < len(pk)
    assert np.array_equal(out["packets"][:, 6:9], pk["pos"][idx])


def _dump(eng, pk, d):
    bench.dump_outputs(str(d), eng, pk)
    return _load(d)
