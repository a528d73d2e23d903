"""k_ma_finish's queue appends gathered in LDS (ARTIS_GPU_FIN_GATHER; wavefront.h WaveOut).  Needs an MI355X.

A wave keeps the R- and K-queue entries of its loop passes in LDS and appends them WAVE_OUT_CAP - 63 or more at a time,
and what is left when its loop ends.  Only the queues' order changes, and a packet's history depends on its own RNG
stream alone, so the step's packets are the same bytes with the switch on and off: each case below is compared byte
for byte (packets, integer counters) with this build's default run, and the default run with the CPU oracle (no
discrete mismatch, counters equal).  Estimators are sums of unordered float atomics and are compared within
parity.ESTIMATOR_RTOL of their largest entry.

Every engine step runs in a child process under `timeout -k 10` (this file run as a script, see _child): the failure
to guard against is an entry that is never appended, which ends a round loop early or not at all.  One child makes
the steps of every ensemble size for one environment.  ARTIS_GPU_WAVE_GRID=8 makes k_ma_finish's grid 2 blocks (512
lanes).  The sizes: an F queue shorter than a wave (1, 63 packets), at most one wave (64), one lane into a second
wave (65), short of a block (100), many grid strides with every wave's buffer flushed only at its loop's end (4000),
and 30000 packets, whose first F queue gives each of the 8 waves about three times WAVE_OUT_CAP entries, so that
buffers are flushed inside the loop.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTS = 10
SEED = 23
SIZES = [1, 63, 64, 65, 100, 4000, 30000]  # prefixes of one ensemble (packets are independent: a prefix is an ensemble)
MODEL = dict(ngrid_1d=7, nlevels_per_ion=30, n_ionising=12, max_lines=3000, ntstep=20)
EST_NAMES = ("J", "nuJ", "ffheating", "colheating", "gamma", "bfheating", "rpkt_emiss")
CHILD_TIMEOUT_S = 180  # a child takes a few seconds; a round loop that does not end takes this long to fail
# the virtual-packet case: a spawn buffer of the minimum size, drained several times by 20000 packets
VMODEL = dict(ngrid_1d=8, nlevels_per_ion=30, n_ionising=12, max_lines=3000, ntstep=20)
VNTS = 14
VNPKTS = 20000

pytestmark = pytest.mark.gpu


def _model_and_packets():
    from artis_amd.model import Model

    m = Model(**MODEL)
    m.set_timestep(NTS)
    return m, m.init_rpackets(NTS, max(SIZES), seed=SEED)


def _child(out, mode):
    sys.path.insert(0, REPO)
    from artis_amd import Engine, ffi
    from artis_amd.model import Model

    res = {}
    if mode == "vpkt":
        m = Model(**VMODEL)
        m.set_timestep(VNTS)
        pg = m.init_rpackets(VNTS, VNPKTS, seed=44)
        vc = ffi.VpktConfig(nz_obs=(0.3, -0.5), phi_obs_deg=(0.0, 120.0), exclude=(0.0, -1.0), spawn_capacity=16)
        eng = Engine(m)
        eng.vpkt_init(vc)
        eng.upload_cellstate(VNTS)
        eg = eng.update_packets(VNTS, pg)
        vg = eng.vpkt_download()
        _, spawns, traces = eng.vpkt_last_stats()
        res.update(packets=pg.view(np.uint8), counters=np.asarray(eg.counters), drains=eng.vpkt_last_drains(),
                   spawns=spawns, traces=traces, vcounters=np.array([v for _, v in sorted(vg.counters().items())]),
                   vstokes=vg.vstokes)
        eng.close()
    else:
        m, pk = _model_and_packets()
        eng = Engine(m)
        eng.upload_cellstate(NTS)
        for n in SIZES:
            pg = pk[:n].copy()
            eg = eng.update_packets(NTS, pg)
            res.update({f"packets{n}": pg.view(np.uint8), f"counters{n}": np.asarray(eg.counters),
                        f"work{n}": eng.last_work(), f"nesc{n}": int(eg.struct.nesc)})
            res.update({f"{name}{n}": np.asarray(getattr(eg, name)).copy() for name in EST_NAMES})
        eng.close()
    np.savez(out, **res)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """run(env, mode="steps") -> the child's arrays, one child process per distinct case (results are shared)."""
    d = tmp_path_factory.mktemp("finish_gather")
    done = {}

    def go(env=None, mode="steps"):
        env = dict(env or {})
        key = (mode, tuple(sorted(env.items())))
        if key not in done:
            out = str(d / f"run{len(done)}.npz")
            cenv = dict(os.environ, ARTIS_GPU_WAVE_GRID="8", **env)
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__),
                                out, mode], env=cenv, capture_output=True, text=True)
            assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
            done[key] = dict(np.load(out))
        return done[key]

    return go


@pytest.fixture(scope="module")
def oracle():
    """oracle(npkts) -> (packets, estimators, work) of the CPU oracle on the same prefix, computed once per size."""
    import oracle_lib

    m, pk = _model_and_packets()
    done = {}

    def go(npkts):
        if npkts not in done:
            po = pk[:npkts].copy()
            eo, wo = oracle_lib.update_packets(m, NTS, po, nthreads=16)
            done[npkts] = (po, eo, wo)
        return done[npkts]

    return go


def _assert_estimators_close(get_a, get_b):
    import parity

    for name in EST_NAMES:
        x, y = get_a(name), get_b(name)
        scale = max(np.abs(y).max(), 1e-300) if y.size else 1e-300
        assert np.abs(x - y).max(initial=0.0) <= parity.ESTIMATOR_RTOL * scale, (name, np.abs(x - y).max() / scale)


@pytest.mark.parametrize("npkts", SIZES)
def test_default_matches_oracle(run, oracle, npkts):
    import parity

    r = run()
    po, eo, wo = oracle(npkts)
    pg = r[f"packets{npkts}"].view(po.dtype)
    parity.assert_packets_match(pg, po)  # no discrete mismatch, FP fields within parity.FP_RTOL
    assert parity.counters_equal(r[f"counters{npkts}"], eo.counters), (r[f"counters{npkts}"], eo.counters)
    assert int(r[f"nesc{npkts}"]) == eo.struct.nesc
    keep = np.arange(len(wo)) != 9  # WK_MA_TRANS counts the cached walk's probes, the oracle's its linear scans
    assert (r[f"work{npkts}"][keep] == wo[keep]).all(), (r[f"work{npkts}"], wo)
    _assert_estimators_close(lambda name: r[f"{name}{npkts}"], lambda name: np.asarray(getattr(eo, name)))


VARIANTS = {"gather_off": {"ARTIS_GPU_FIN_GATHER": "0"}, "mega": {"ARTIS_GPU_ENGINE": "mega"},
            # the fallback side state: the F queue's entries read from the per-packet pend arrays, the M queue's
            # tickets gathered by the scatter
            "mf_rec_off": {"ARTIS_GPU_MF_REC": "0"}, "ma_pre_off": {"ARTIS_GPU_MA_PRE": "0"}}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_variants_are_byte_identical(run, variant):
    a, b = run(), run(VARIANTS[variant])
    for n in SIZES:
        assert np.array_equal(a[f"packets{n}"], b[f"packets{n}"]), n
        assert np.array_equal(a[f"counters{n}"], b[f"counters{n}"]), n
        assert int(a[f"nesc{n}"]) == int(b[f"nesc{n}"]), n
        _assert_estimators_close(lambda name: b[f"{name}{n}"], lambda name: a[f"{name}{n}"])


def test_virtual_packets_with_a_draining_spawn_buffer(run):
    """k_ma_finish takes its slots through wave_reserve and stops on a full spawn buffer, appending what its waves
    have gathered; the resumed launches finish the queue.  The switch on and off: the same packets, counters and
    trace counts."""
    import parity

    a, b = run(mode="vpkt"), run({"ARTIS_GPU_FIN_GATHER": "0"}, mode="vpkt")
    assert int(a["drains"]) > 0 and int(b["drains"]) > 0
    assert np.array_equal(a["packets"], b["packets"])
    assert np.array_equal(a["counters"], b["counters"])
    assert int(a["traces"]) == int(b["traces"]) > 0 and int(a["spawns"]) == int(b["spawns"])
    assert np.array_equal(a["vcounters"], b["vcounters"])
    fa, fb = np.isfinite(a["vstokes"]), np.isfinite(b["vstokes"])
    assert np.array_equal(fa, fb)
    scale = max(np.abs(b["vstokes"][fb]).max(initial=0.0), 1e-300)
    assert np.abs(a["vstokes"][fa] - b["vstokes"][fb]).max(initial=0.0) <= parity.ESTIMATOR_RTOL * scale


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
