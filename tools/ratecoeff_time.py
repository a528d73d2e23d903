"""Times the rate-coefficient lookup tables built on the device (artis_amd.ratecoeff.build, k_ratecoeff_lut) against
the same tables from the CPU restatement of the same qag (tests/ratecoeff_cpu_ref.cpp, built here with g++) on
--threads OpenMP threads of the same machine.  Atoms: the bench atom and the 5x-lines atom (bench.py
level_mode_workload's: line window 160); the tables depend on the continua, not on the lines, and the grid plays no
part, so the models are made on a 4^3 grid.  Per atom: the wall time of the call (the minimum of --repeats runs after
one warm-up, all runs listed), the kernel's own milliseconds, the mean intervals per integral, the statuses, the CPU
helper's wall time (minimum of --repeats) and the largest relative difference between the two sets of tables.
All legs run in one child process under `timeout`; a failure ends the run.  Prints one JSON line.
  python tools/ratecoeff_time.py [--epsrel 1e-3] [--repeats 3] [--threads 16] [--timeout 480]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, REPO)

ATOMS = {"bench": dict(ngrid_1d=4), "lines_5x": dict(ngrid_1d=4, line_window=160, max_lines=1_000_000)}


def build_cpu_helper(d):
    so = os.path.join(d, "libratecoeff_cpu_ref.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-fPIC", "-shared",
                    "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tests", "ratecoeff_cpu_ref.cpp"),
                    "-o", so], check=True)
    L = C.CDLL(so)
    L.ratecoeff_cpu_qag.argtypes = [C.c_void_p, C.c_double] + [C.c_void_p] * 6 + [C.c_int]
    return L


def child(args):
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    from artis_amd import ffi, ratecoeff
    from artis_amd.model import Model

    out = {}
    with tempfile.TemporaryDirectory() as d:
        cpu = build_cpu_helper(d)
        for name, cfg in ATOMS.items():
            m = Model(**cfg)
            hdr = ffi.AtomicTables.from_address(m.atomic)
            r = {"nbfcontinua": int(hdr.nbfcontinua), "tablesize": int(hdr.tablesize), "nlines": int(hdr.nlines)}
            t = ratecoeff.build(m, args.epsrel)  # warm-up: code object loaded, host pages touched
            wall, kern = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                ratecoeff.build(m, args.epsrel, out=t)
                wall.append(time.perf_counter() - t0)
                kern.append(t.kernel_ms)
            r["gpu_wall_ms"] = 1e3 * min(wall)
            r["gpu_wall_ms_all"] = [1e3 * w for w in wall]
            r["gpu_kernel_ms"] = min(kern)
            r["integrals"] = int(t.status.size)
            r["status0"] = int((t.status == 0).sum())
            r["mean_intervals"] = float(t.intervals.mean())
            r["max_intervals"] = int(t.intervals.max())
            ref = ratecoeff.Tables(hdr.tablesize, hdr.nbfcontinua, hdr.nions_total)
            cw = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                rc = cpu.ratecoeff_cpu_qag(m.atomic, args.epsrel, ref.spontrecombcoeff.ctypes.data,
                                           ref.corrphotoioncoeff.ctypes.data, ref.bfheating_coeff.ctypes.data,
                                           ref.bfcooling_coeff.ctypes.data, ref.status.ctypes.data,
                                           ref.intervals.ctypes.data, args.threads)
                cw.append(time.perf_counter() - t0)
                assert rc == 0, rc
            r["cpu_threads"] = args.threads
            r["cpu_wall_ms"] = 1e3 * min(cw)
            r["cpu_mean_intervals"] = float(ref.intervals.mean())
            rel = 0.
            for k in ratecoeff.INTEGRALS:
                a, b = getattr(t, k), getattr(ref, k)
                nz = b != 0
                rel = max(rel, float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))))
            r["max_rel_diff_gpu_vs_cpu"] = rel
            r["intervals_differ"] = int((t.intervals != ref.intervals).sum())
            out[name] = r
            m.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epsrel", type=float, default=1e-3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--timeout", type=int, default=480)
    ap.add_argument("--child", action="store_true", help="internal: run the legs in this process")
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    result = {"epsrel": args.epsrel, "repeats": args.repeats}
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--epsrel",
           str(args.epsrel), "--repeats", str(args.repeats), "--threads", str(args.threads)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:  # a fault, an abort or the time limit: nothing more is started on the GPU
        sys.stderr.write(r.stderr[-4000:])
        result["failed"] = {"status": r.returncode}
        print(json.dumps(result), flush=True)
        raise SystemExit(1)
    result.update(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
