"""Times the direction-resolved spectra of the bench model's packets: the 101 Engine.spectra calls (abin -1 .. 99)
against the one Engine.spectra_res call that replaces them.  1e6 packets made resident by one step_resident,
nnubins 1000, emission_res on.  Every leg is a child process under its own `timeout`; a leg that fails ends the run.
Prints one JSON line: wall seconds per leg (the minimum of --repeats runs after one warm-up), the same with
emission_res off (small arrays: the binning kernel weighs more), and the largest relative difference between the
one-call and the 101-call results.
  python tools/spectra_res_time.py [--packets 1000000] [--repeats 3] [--leg-timeout 240]"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)

LEGS = ("loop101", "one_call")


def leg(args):
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
    out = {}
    try:
        eng.upload_cellstate(args.nts)
        eng.upload(pk)
        eng.zero_estimators()
        eng.step_resident(args.nts)
        nt = m.cfg.ntstep

        def loop101(emission_res, keep=False):
            """The 101 calls; keep: gather their arrays into one block (not part of the timed work)."""
            res = ffi.SpectraResArrays(nt, args.nnubins, m.nelements, m.maxnions, emission_res=emission_res) \
                if keep else None
            for abin in range(-1, ffi.MABINS):
                g = eng.spectra(nnubins=args.nnubins, abin=abin, emission_res=emission_res)
                if keep:
                    for name, view in res.slot(abin).arrays().items():
                        view += getattr(g, name)
            return res

        def one_call(emission_res):
            return eng.spectra_res(nnubins=args.nnubins, emission_res=emission_res)

        fn = loop101 if args.leg == "loop101" else one_call
        for emission_res, key in ((True, "seconds"), (False, "seconds_flux_only")):
            fn(emission_res)  # warm-up: code objects loaded, host pages touched
            ts = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                res = fn(emission_res)
                ts.append(time.perf_counter() - t0)
            out[key] = min(ts)
            out[key + "_all"] = ts
            if emission_res and args.check:
                out["flux_cells"] = int(np.count_nonzero(res.flux[0]))
                out["bytes"] = int(sum(a.nbytes for a in res.arrays().values()))
                ref = loop101(True, keep=True)
                out["max_rel_diff_vs_101"] = max(
                    float(np.abs(a - getattr(ref, n)).max() / max(np.abs(a).max(), 1e-300))
                    for n, a in res.arrays().items())
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
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--leg", choices=LEGS, default=None, help="internal: run one leg in this process")
    ap.add_argument("--check", action="store_true", help="internal: compare the leg's result with the 101 calls")
    args = ap.parse_args()
    if args.leg:
        leg(args)
        return
    result = {"packets": args.packets, "nnubins": args.nnubins, "ngrid": args.ngrid, "nts": args.nts}
    for name in LEGS:
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
               "--packets", str(args.packets), "--ngrid", str(args.ngrid), "--nts", str(args.nts), "--nnubins",
               str(args.nnubins), "--repeats", str(args.repeats)] + ([] if name == "loop101" else ["--check"])
        print(f"[spectra_res_time] {name} ...", file=sys.stderr, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:  # a fault, an abort or the time limit: nothing more is started on the GPU
            sys.stderr.write(r.stderr[-4000:])
            result["failed"] = {"leg": name, "status": r.returncode}
            print(json.dumps(result), flush=True)
            raise SystemExit(1)
        result[name] = json.loads(r.stdout.strip().splitlines()[-1])
    result["speedup"] = result["loop101"]["seconds"] / result["one_call"]["seconds"]
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
