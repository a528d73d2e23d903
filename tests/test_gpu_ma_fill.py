"""k_ma's lane filling: the refill threshold (ARTIS_GPU_REFILL_MA) and the parking of a long launch's tail walks
(ARTIS_GPU_MA_PARK).  Needs an MI355X.

A packet's history depends only on its own RNG stream, so whichever lane, pass or round makes a jump, the step's
packets are the same bytes: every case below is compared byte for byte with this build's default run, and the
default run with the CPU oracle (no discrete mismatch, integer event counters equal).

Every engine step runs in a child process of its own under `timeout -k 10`: the failure to guard against is a
round loop that does not end.  The child is this file run as a script (see _child).  ARTIS_GPU_WAVE_GRID=8 makes
k_ma's persistent grid 4 blocks (1024 lanes), so a few thousand packets refill every lane several times, use the
queue up, and -- from MA_PARK_FILL = 4 walks per lane of the grid, 4096 queue entries -- park the tail's walks.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTS = 10
SEED = 23
NMAX = 12000   # the ensemble every case takes a prefix of (packets are independent: a prefix is an ensemble)
MODEL = dict(ngrid_1d=7, nlevels_per_ion=30, n_ionising=12, max_lines=3000, ntstep=20)
STEP_TIMEOUT_S = 180  # a step takes a second or two; a round loop that does not end takes this long to fail
MA_LANES = 4 * 256    # k_ma's grid with ARTIS_GPU_WAVE_GRID=8
PARK_MIN_QUEUE = 4 * MA_LANES

pytestmark = pytest.mark.gpu


def _model_and_packets():
    from artis_amd.model import Model

    m = Model(**MODEL)
    m.set_timestep(NTS)
    return m, m.init_rpackets(NTS, NMAX, seed=SEED)


def _child(out, npkts, level):
    """One update_packets of the first npkts packets; the packets, counters and work counts go to `out`."""
    sys.path.insert(0, REPO)
    from artis_amd import Engine

    m, pk = _model_and_packets()
    if level:  # level mode: a record pool of half the rows, as the suite's table-budget tests make it
        probe = Engine(m)
        cells = probe.table_info()["cells"]
        probe.close()
        os.environ["ARTIS_GPU_MACACHE_ROWS"] = str(cells // 2)
    eng = Engine(m)
    eng.upload_cellstate(NTS)
    if level:
        assert eng.table_info()["macache_rows"] == 0 and eng.table_info()["ma_level_records"] > 0
    pg = pk[:npkts].copy()
    eg = eng.update_packets(NTS, pg)
    np.savez(out, packets=pg.view(np.uint8), counters=np.asarray(eg.counters), work=eng.last_work(),
             rounds=eng.last_rounds(), nesc=int(eg.struct.nesc))
    eng.close()


class Run:
    def __init__(self, path, stderr):
        z = np.load(path)
        self.packets = z["packets"]
        self.counters = z["counters"]
        self.work = z["work"]
        self.rounds = int(z["rounds"])
        self.nesc = int(z["nesc"])
        # (the split-kernel engine's ARTIS_GPU_STATS line; the megakernel has no queues and prints none)
        m = re.search(r"walks parked (\d+) .*first M queue (\d+)", stderr)
        self.parked, self.first_mq = (int(m.group(1)), int(m.group(2))) if m else (None, None)


@pytest.fixture(scope="module")
def step(tmp_path_factory):
    """step(npkts, env, level=False) -> Run, one child process per distinct case (results are shared)."""
    d = tmp_path_factory.mktemp("ma_fill")
    done = {}

    def run(npkts, env=None, level=False):
        env = dict(env or {})
        key = (npkts, tuple(sorted(env.items())), level)
        if key not in done:
            out = str(d / f"run{len(done)}.npz")
            cenv = dict(os.environ, ARTIS_GPU_WAVE_GRID="8", ARTIS_GPU_STATS="1", **env)
            p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__),
                                out, str(npkts), "1" if level else "0"], env=cenv, capture_output=True, text=True)
            assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
            done[key] = Run(out, p.stderr)
        return done[key]

    return run


@pytest.fixture(scope="module")
def oracle():
    """oracle(npkts) -> (packets, estimators, work) of the CPU oracle on the same prefix, computed once per size."""
    import oracle_lib

    m, pk = _model_and_packets()
    done = {}

    def run(npkts):
        if npkts not in done:
            po = pk[:npkts].copy()
            eo, wo = oracle_lib.update_packets(m, NTS, po, nthreads=16)
            done[npkts] = (po, eo, wo)
        return done[npkts]

    return run


def _assert_matches_oracle(r, o):
    import parity

    po, eo, wo = o
    pg = r.packets.view(po.dtype)
    parity.assert_packets_match(pg, po)  # no discrete mismatch, FP fields within parity.FP_RTOL
    assert parity.counters_equal(r.counters, eo.counters), (r.counters, eo.counters)
    assert r.nesc == eo.struct.nesc
    keep = np.arange(len(wo)) != 9  # WK_MA_TRANS counts the cached walk's probes, the oracle's its linear scans
    assert (r.work[keep] == wo[keep]).all(), (r.work, wo)


VARIANTS = {"park_off": {"ARTIS_GPU_MA_PARK": "0"}, "park_any_idle_lane": {"ARTIS_GPU_MA_PARK": "64"},
            "refill_1": {"ARTIS_GPU_REFILL_MA": "1"}, "refill_64": {"ARTIS_GPU_REFILL_MA": "64"},
            "mega": {"ARTIS_GPU_ENGINE": "mega"}}
# on the ensemble long enough to park, also without the producers' pre-tickets and bins (the parked walk is then
# looked up by the binning kernels from the packet's side state, as a walk parked by k_ma_exact)
VARIANTS_LONG = dict(VARIANTS, park_any_gathered_tickets={"ARTIS_GPU_MA_PARK": "64", "ARTIS_GPU_MA_PRE": "0",
                                                          "ARTIS_GPU_BIN_PUSH": "0"})
CASES = [(4000, v) for v in sorted(VARIANTS)] + [(NMAX, v) for v in sorted(VARIANTS_LONG)]


@pytest.mark.parametrize("npkts", [4000, NMAX])
def test_defaults_match_oracle(step, oracle, npkts):
    r = step(npkts)
    _assert_matches_oracle(r, oracle(npkts))
    assert r.first_mq > MA_LANES  # every lane is refilled; the queue is used up while walks are under way


@pytest.mark.parametrize("npkts,variant", CASES, ids=[f"{n}-{v}" for n, v in CASES])
def test_variants_are_byte_identical(step, npkts, variant):
    env = VARIANTS_LONG[variant]
    a, b = step(npkts), step(npkts, env)
    assert np.array_equal(a.packets, b.packets)
    assert np.array_equal(a.counters, b.counters)
    if variant != "mega":
        assert b.first_mq == a.first_mq
        if env.get("ARTIS_GPU_MA_PARK") == "0":
            assert b.parked == 0
    if npkts == NMAX and env.get("ARTIS_GPU_MA_PARK") == "64":
        # the large ensemble's first queue fills the grid MA_PARK_FILL times: its tail walks are parked
        assert a.first_mq >= PARK_MIN_QUEUE and b.parked > 0


def test_short_queue_ends_without_parking(step, oracle):
    """100 packets: the queue is shorter than one block's lanes; the rounds end and nothing is parked, whatever
    the threshold."""
    for env in ({}, {"ARTIS_GPU_MA_PARK": "64"}):
        r = step(100, env)
        assert r.first_mq < 256 and r.parked == 0
        _assert_matches_oracle(r, oracle(100))


# the smallest prefix above 4000 packets whose first M queue is a multiple of 64 (the queue grows by at most one
# per packet of the prefix, so every length is reached); the test checks the length it finds
NPKTS_MQ_MULTIPLE_OF_64 = 4010  # (first M queue 3392 = 53 * 64)


def test_first_queue_a_multiple_of_64(step, oracle):
    """The last full wave of tickets ends exactly at the queue's end: the next reservation is abandoned."""
    r = step(NPKTS_MQ_MULTIPLE_OF_64)
    assert r.first_mq > 0 and r.first_mq % 64 == 0, r.first_mq
    _assert_matches_oracle(r, oracle(NPKTS_MQ_MULTIPLE_OF_64))
    b = step(NPKTS_MQ_MULTIPLE_OF_64, {"ARTIS_GPU_REFILL_MA": "1"})
    assert np.array_equal(r.packets, b.packets)


def test_level_mode_matches_oracle(step, oracle):
    """Level mode (half the rows' records) parks nothing."""
    r = step(4000, level=True)
    _assert_matches_oracle(r, oracle(4000))
    assert r.parked == 0


if __name__ == "__main__":
    _child(sys.argv[1], int(sys.argv[2]), sys.argv[3] == "1")
