"""Times the per-line emission / absorption trace (Engine.line_trace, k_line_trace) of the bench model's packets
against the existing angle-averaged pass over the same packets.  1e6 packets made resident by one step_resident,
nnubins 1000.  Legs, each the wall time of the Python call (the minimum of --repeats runs after one warm-up, all runs
listed):
  spectra        Engine.spectra(abin=-1, emission_res=False): the yardstick, existing code
  trace_1        one line_trace with 1 region that holds every admitted packet
  trace_16       one line_trace with 16 such regions (every traced packet adds to all 16)
  trace_16x1     16 line_trace calls with 1 region each
  trace_16_tiled / trace_16x1_tiled   the same pair with 16 wavelength windows that tile the binned band, so that a
                 packet adds to one region, not to sixteen
All legs run in one child process under `timeout` (the setup is shared); a failure ends the run.  Prints one JSON
line; "one_call_faster" / "one_call_faster_tiled" say whether trace_16 < trace_16x1 held for each pair.
  python tools/line_trace_time.py [--packets 1000000] [--repeats 3] [--timeout 480]"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)

EVERYTHING = (0.01, 10000., 100., 1e6)  # days, days, Angstrom, Angstrom: wider than the run and the binned band


def child(args):
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    from artis_amd import Engine, ffi
    from artis_amd.model import Model

    m = Model(ngrid_1d=args.ngrid)
    m.set_timestep(args.nts)
    pk = m.init_rpackets(args.nts, args.packets, seed=1000)
    eng = Engine(m, params=m.params)
    out = {"nlines": int(m.nlines)}
    try:
        eng.upload_cellstate(args.nts)
        eng.upload(pk)
        eng.zero_estimators()
        eng.step_resident(args.nts)
        nreg = ffi.LINE_TRACE_MAX_REGIONS
        one, sixteen = [EVERYTHING], [EVERYTHING] * nreg
        # 16 wavelength windows that tile the binned band: a packet lies in one of them
        edges = np.geomspace(599., 29980., nreg + 1)
        tiled = [(EVERYTHING[0], EVERYTHING[1], float(edges[k]), float(edges[k + 1])) for k in range(nreg)]

        # every trace leg ADDS into arrays made before the clock starts, so that the time is the call's own: device
        # allocation and memset, the kernel, the copy back and the host add
        def arrays(nregions):
            return ffi.LineTraceArrays(m.nlines, nregions)

        def in_one_call(regions):
            acc = arrays(len(regions))
            return lambda: eng.line_trace(regions, nnubins=args.nnubins, out=acc)

        def one_by_one(regions):
            outs = [arrays(1) for _ in regions]
            return lambda: [eng.line_trace([reg], nnubins=args.nnubins, out=o) for reg, o in zip(regions, outs)]

        legs = (("spectra", lambda: eng.spectra(nnubins=args.nnubins, abin=-1, emission_res=False)),
                ("trace_1", in_one_call(one)),
                ("trace_16", in_one_call(sixteen)),
                ("trace_16x1", one_by_one(sixteen)),
                ("trace_16_tiled", in_one_call(tiled)),
                ("trace_16x1_tiled", one_by_one(tiled)))
        for name, fn in legs:
            fn()  # warm-up: code objects loaded, host pages touched
            ts = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            out[name] = {"seconds": min(ts), "seconds_all": ts}
        # untimed: what was traced, and that the forms agree with each other and with the yardstick's flux
        results = {"spectra": eng.spectra(nnubins=args.nnubins, abin=-1, emission_res=False),
                   "trace_1": eng.line_trace(one, nnubins=args.nnubins),
                   "trace_16": eng.line_trace(sixteen, nnubins=args.nnubins),
                   "trace_16_tiled": eng.line_trace(tiled, nnubins=args.nnubins),
                   "trace_16x1_tiled": [eng.line_trace([reg], nnubins=args.nnubins) for reg in tiled]}
        flux = results["spectra"].flux
        t1, t16 = results["trace_1"], results["trace_16"]
        out["traced_lines_emission"] = int(np.count_nonzero(t1.lines[0, :, 0]))
        out["traced_lines_absorption"] = int(np.count_nonzero(t1.lines[0, :, 2]))
        out["emission_total_over_flux"] = float(t1.totals[0, 0] / flux.sum())
        out["max_rel_diff_16_vs_1"] = float(max(
            np.abs(t16.lines[r] - t1.lines[0]).max() / max(np.abs(t1.lines[0]).max(), 1e-300) for r in range(nreg)))
        tt, tx = results["trace_16_tiled"], results["trace_16x1_tiled"]
        out["tiled_total_over_everything"] = float(tt.totals[:, 0].sum() / t1.totals[0, 0])
        out["max_rel_diff_tiled_vs_16x1"] = float(max(
            np.abs(tt.lines[r] - tx[r].lines[0]).max() / max(np.abs(tt.lines[r]).max(), 1e-300) for r in range(nreg)))
    finally:
        eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1_000_000)
    ap.add_argument("--ngrid", type=int, default=50)
    ap.add_argument("--nts", type=int, default=10)
    ap.add_argument("--nnubins", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=480)
    ap.add_argument("--child", action="store_true", help="internal: run the legs in this process")
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    result = {"packets": args.packets, "nnubins": args.nnubins, "ngrid": args.ngrid, "nts": args.nts}
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child",
           "--packets", str(args.packets), "--ngrid", str(args.ngrid), "--nts", str(args.nts), "--nnubins",
           str(args.nnubins), "--repeats", str(args.repeats)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:  # a fault, an abort or the time limit: nothing more is started on the GPU
        sys.stderr.write(r.stderr[-4000:])
        result["failed"] = {"status": r.returncode}
        print(json.dumps(result), flush=True)
        raise SystemExit(1)
    result.update(json.loads(r.stdout.strip().splitlines()[-1]))
    result["one_call_faster"] = result["trace_16"]["seconds"] < result["trace_16x1"]["seconds"]
    result["one_call_faster_tiled"] = result["trace_16_tiled"]["seconds"] < result["trace_16x1_tiled"]["seconds"]
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
