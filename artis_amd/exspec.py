"""The reference's exspec program (exspec.cc:140-263) on the device-binned spectra: the angle-averaged outputs and
the 100 line-of-sight sets (spec_res_XX.out, light_curve_res_XX.out, emission_res_XX.out, ...).

run() bins the engine's resident packets, or a list of rank packet files / arrays, with Engine.spectra_res -- one
pass per packet set and chunk of direction bins -- and write_outputs() writes a block of slots with the C++ writers
of libartis_io under the reference's file names.  With trace_regions, run() also takes the per-line emission /
absorption trace of TRACE_EMISSION_ABSORPTION_REGION_ON (spectrum.cc:11-142, 395-447) for those regions in every
packet set's pass (Engine.line_trace) and writes its tables to emission_absorption_trace.out (write_line_trace); the
reference prints them into its log, so that file name is this project's.
"""
import ctypes as C
import os

import numpy as np

from . import ffi
from . import io as aio
from .spectrum import write_light_curve, write_spec_out, write_specpol

MEV = 1.6021772e-6
H = 6.6260755e-27
# the gamma-ray spectrum's band (exspec.cc:158-159)
NU_MIN_GAMMA = 0.05 * MEV / H
NU_MAX_GAMMA = 4. * MEV / H

AVERAGE_FILES = ("light_curve.out", "gamma_light_curve.out", "spec.out", "gamma_spec.out")
AVERAGE_EMISSION_FILES = ("emission.out", "emissiontrue.out", "absorption.out")
AVERAGE_POL_FILES = ("specpol.out",)
AVERAGE_POL_EMISSION_FILES = ("emissionpol.out", "absorptionpol.out")
RES_FILES = ("light_curve_res_%.2d.out", "spec_res_%.2d.out")
RES_EMISSION_FILES = ("emission_res_%.2d.out", "emissiontrue_res_%.2d.out", "absorption_res_%.2d.out")
RES_POL_FILES = ("specpol_res_%.2d.out",)
RES_POL_EMISSION_FILES = ("emissionpol_res_%.2d.out", "absorptionpol_res_%.2d.out")
LINE_TRACE_FILE = "emission_absorption_trace.out"


def is_1d_read(model):
    """grid::get_model_type() == RHO_1D_READ: exspec writes the angle-averaged files only (exspec.cc:140)."""
    return getattr(model, "model_type", 3) == 1


def file_set(abins, emission_res=True, stokes=False):
    """The names exspec.cc:205-250 writes for the given abins (-1: the angle-averaged files), sorted."""
    names = []
    for a in abins:
        if a == -1:
            names += AVERAGE_FILES
            names += AVERAGE_EMISSION_FILES if emission_res else ()
            names += AVERAGE_POL_FILES if stokes else ()
            names += AVERAGE_POL_EMISSION_FILES if stokes and emission_res else ()
        else:
            pats = RES_FILES + (RES_EMISSION_FILES if emission_res else ()) + (RES_POL_FILES if stokes else ())
            pats += RES_POL_EMISSION_FILES if stokes and emission_res else ()
            names += [p % a for p in pats]
    return sorted(names)


def slot_bytes(ntstep, nnubins, nelements, maxnions, emission_res=True, stokes=False):
    """Bytes one slot (the average or one direction bin) takes in a ffi.SpectraResArrays -- and, the same number, in
    the device accumulators of one artis_gpu_spectra_res call."""
    ioncount = nelements * maxnions
    proccount = 2 * ioncount + 1
    nb = ntstep * nnubins
    n = nb + ntstep
    if emission_res:
        n += nb * (2 * proccount + ioncount)
    if stokes:
        n += 3 * nb
        if emission_res:
            n += 3 * nb * (proccount + ioncount)
    return 8 * n


def plan_chunks(max_bytes, bytes_per_slot, nbins=ffi.MABINS):
    """Split the average and the direction bins 0 .. nbins-1 into spectra_res requests of at most max_bytes each:
    [(abin_first, abin_count, with_average), ...].  The average is slot 0 of the first request; every bin appears in
    exactly one request.  max_bytes None: everything in one request."""
    if nbins < 0 or bytes_per_slot <= 0:
        raise ValueError("plan_chunks: nbins >= 0 and bytes_per_slot > 0")
    cap = 1 + nbins if max_bytes is None else min(int(max_bytes) // int(bytes_per_slot), 1 + nbins)
    if cap < 1:
        raise ValueError(f"plan_chunks: max_bytes {max_bytes} is below one slot ({bytes_per_slot} bytes)")
    chunks = [(0, min(cap - 1, nbins), True)]
    first = chunks[0][1]
    while first < nbins:
        count = min(cap, nbins - first)
        chunks.append((first, count, False))
        first += count
    return chunks


def default_max_bytes():
    """Half of the host memory available now (the arrays are held once on the host; the engine's copy-back staging
    is bounded), or None (no limit) where the system does not say."""
    try:
        return os.sysconf("SC_AVPHYS_PAGES") * os.sysconf("SC_PAGE_SIZE") // 2
    except (ValueError, OSError, AttributeError):
        return None


def _geometry(model):
    g = ffi.Geometry.from_address(model.geometry)
    nt = g.ntstep
    ts_mid = np.ctypeslib.as_array(g.ts_mid, shape=(nt,)).copy()
    ts_width = np.ctypeslib.as_array(g.ts_width, shape=(nt,)).copy()
    return nt, ts_mid, ts_width, g.nu_min_r, g.nu_max_r


def write_outputs(outdir, model, arrays, emission_res=None, stokes=None, gamma_dep=None, cmf_lum=None):
    """Write the slots of `arrays` (ffi.SpectraResArrays) into outdir under the reference's names
    (exspec.cc:205-250); returns the sorted list of the names written.

    The average (when arrays has it): light_curve.out, gamma_light_curve.out, spec.out, gamma_spec.out, with
    emission_res emission.out / emissiontrue.out / absorption.out, with stokes specpol.out (and emissionpol.out /
    absorptionpol.out).  Every direction bin a: light_curve_res_%.2d.out, spec_res_%.2d.out and the _res forms of
    the emission and polarisation files.  emission_res / stokes default to what arrays holds; a 1D-read model gets
    the angle-averaged files only (exspec.cc:140).  gamma_dep / cmf_lum [ntstep]: the deposition and cmf-luminosity
    rows of light_curve.out (time_step[].gamma_dep / cmf_lum, light_curve.cc:21-28), zeros when not given.

    gamma_spec.out has zero flux: add_to_spec admits a packet only inside the r-packet band [nu_min_r, nu_max_r]
    (spectrum.cc:349-350), which no gamma packet's nu_rf lies in, so the reference's file is all zeros over the
    gamma band's bins (exspec.cc:158-160, 214)."""
    outdir = os.fspath(outdir)
    os.makedirs(outdir, exist_ok=True)
    emission_res = arrays.emission_res if emission_res is None else bool(emission_res)
    stokes = arrays.stokes if stokes is None else bool(stokes)
    if emission_res and arrays.emission is None:
        raise ValueError("write_outputs: emission_res asked for, but arrays holds no emission / absorption spectra")
    if stokes and arrays.stokes_flux is None:
        raise ValueError("write_outputs: stokes asked for, but arrays holds no Stokes spectra")
    nt, ts_mid, ts_width, nu_min, nu_max = _geometry(model)
    if nt != arrays.ntstep:
        raise ValueError(f"write_outputs: arrays has {arrays.ntstep} timesteps, the model {nt}")
    nnb = arrays.nnubins
    zeros = np.zeros(nt)
    written = []

    def path(name):
        written.append(name)
        return os.path.join(outdir, name)

    def opt(name, on):
        return path(name) if on else None

    for abin in arrays.abins():
        if abin >= 0 and is_1d_read(model):
            break
        s = arrays.slot(abin)
        res = "" if abin == -1 else "_res_%.2d" % abin
        if abin == -1:
            write_light_curve(path("light_curve.out"), ts_mid, ts_width, s.lc_lum, s.lc_lumcmf, gamma_dep, cmf_lum,
                              numtimesteps=nt, abin=-1)
            write_light_curve(path("gamma_light_curve.out"), ts_mid, ts_width, s.gamma_lc_lum, s.gamma_lc_lumcmf,
                              gamma_dep, cmf_lum, numtimesteps=nt, abin=-1)
        else:
            write_light_curve(path(f"light_curve{res}.out"), ts_mid, ts_width, s.lc_lum, zeros, numtimesteps=nt,
                              abin=abin)
        write_spec_out(path(f"spec{res}.out"), ts_mid, s.flux, nu_min, nu_max, numtimesteps=nt,
                       emission=s.emission if emission_res else None,
                       trueemission=s.trueemission if emission_res else None,
                       absorption=s.absorption if emission_res else None,
                       emission_path=opt(f"emission{res}.out", emission_res),
                       trueemission_path=opt(f"emissiontrue{res}.out", emission_res),
                       absorption_path=opt(f"absorption{res}.out", emission_res))
        if stokes:
            pol_em = emission_res and s.stokes_emission is not None
            write_specpol(path(f"specpol{res}.out"), ts_mid, s.stokes_flux, nu_min, nu_max,
                          s.stokes_emission if pol_em else None, s.stokes_absorption if pol_em else None,
                          opt(f"emissionpol{res}.out", pol_em), opt(f"absorptionpol{res}.out", pol_em))
        if abin == -1:
            write_spec_out(path("gamma_spec.out"), ts_mid, np.zeros((nt, nnb)), NU_MIN_GAMMA, NU_MAX_GAMMA,
                           numtimesteps=nt)
    return sorted(written)


def rank_line_trace(lines_region, column, maxlines=500):
    """The line indices of one region's lines [nlines, 4] in the order printout_tracemission_stats lists them
    (spectrum.cc:58-136): descending energy of `column` (0 emission, 2 absorption), equal energies by ascending line
    index, at most maxlines, only lines with energy > 0."""
    a = np.ascontiguousarray(lines_region, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("rank_line_trace: lines_region must be [nlines, 4]")
    L = aio.lib()
    L.artis_rank_line_trace.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
    ranked = np.zeros(max(int(maxlines), 1), dtype=np.int32)
    n = L.artis_rank_line_trace(a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0], int(column), int(maxlines),
                                ranked.ctypes.data_as(C.POINTER(C.c_int32)))
    if n < 0:
        raise ValueError(f"rank_line_trace: column {column} (0 or 2), maxlines {maxlines} (>= 0)")
    return ranked[:n].copy()


def write_line_trace(path, model, arrays, regions):
    """The tables of printout_tracemission_stats (spectrum.cc:58-136) for every region of `arrays`
    (ffi.LineTraceArrays), one block per region, with the C++ writer artis_write_line_trace.  regions: the
    (time_min_days, time_max_days, lambda_min_A, lambda_max_A) tuples the arrays were taken for."""
    regions = list(regions)
    if len(regions) != arrays.nregions or arrays.nlines != model.nlines:
        raise ValueError("write_line_trace: arrays do not belong to these regions / this model")
    regs = (ffi.LineTraceRegion * max(len(regions), 1))()
    for k, reg in enumerate(regions):
        regs[k].nu_lower, regs[k].nu_upper, regs[k].time_min, regs[k].time_max = ffi.line_trace_region(*reg)
    L = aio.lib()
    dp = C.POINTER(C.c_double)
    L.artis_write_line_trace.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.POINTER(ffi.LineTraceRegion), dp, dp]
    lines = np.ascontiguousarray(arrays.lines, dtype=np.float64)
    totals = np.ascontiguousarray(arrays.totals, dtype=np.float64)
    rc = L.artis_write_line_trace(os.fspath(path).encode(), model.atomic, len(regions), regs,
                                  lines.ctypes.data_as(dp), totals.ctypes.data_as(dp))
    if rc != 0:
        raise OSError(f"artis_write_line_trace({path}) -> {rc}")


def load_packets(source):
    """One packet set: a PACKET_DTYPE array as it is, a raw packets_RRRR_tsN.tmp file (sn3d.cc:387-398), or a text
    packetsXX_RRRR.out file (packet.cc:152-196; %g precision)."""
    if isinstance(source, np.ndarray):
        if source.dtype != ffi.PACKET_DTYPE:
            raise TypeError("a packet array must have ffi.PACKET_DTYPE")
        return np.ascontiguousarray(source)
    p = os.fspath(source)
    if p.endswith(".tmp"):
        return np.fromfile(p, dtype=ffi.PACKET_DTYPE)
    with open(p) as f:
        n = sum(1 for ln in f if ln.strip() and not ln.lstrip().startswith("#"))
    pk = np.zeros(n, dtype=ffi.PACKET_DTYPE)
    aio.read_packets(p, pk)
    return pk


def run(engine, outdir, packet_sources=None, nnubins=1000, syn_dir=(0., 0., 1.), emission_res=True, stokes=False,
        max_bytes=None, gamma_dep=None, cmf_lum=None, trace_regions=None):
    """The body of exspec.cc:140-263: bin and write the angle-averaged files and, for a 3D model, the 100
    direction-bin sets into outdir.

    packet_sources None: the engine's resident packets (nprocs 1).  Otherwise a list of packet files / arrays (see
    load_packets), one per rank: each is uploaded and binned into the same arrays with nprocs = len(packet_sources)
    (the rank loop of exspec.cc:162; the engine's resident packets are then the last source).  The direction bins are
    taken in chunks whose host arrays stay within max_bytes (default: default_max_bytes()); with more than one chunk
    every source is uploaded once per chunk.  Returns (sorted names written, the arrays of the first chunk -- the
    whole result when one chunk was enough).

    trace_regions: (time_min_days, time_max_days, lambda_min_A, lambda_max_A) tuples.  When given, every source's
    pass of the first chunk also takes the per-line emission / absorption trace of those regions (Engine.line_trace,
    angle-averaged, the same nnubins and nprocs), emission_absorption_trace.out is written into outdir and named in
    the list, and the ffi.LineTraceArrays are returned as a third value."""
    model = engine.model
    nt = model.cfg.ntstep
    nbins = 0 if is_1d_read(model) else ffi.MABINS
    per_slot = slot_bytes(nt, nnubins, model.nelements, model.maxnions, emission_res, stokes)
    budget = default_max_bytes() if max_bytes is None else max_bytes
    chunks = plan_chunks(budget, per_slot, nbins)
    sources = [None] if packet_sources is None else list(packet_sources)
    if not sources:
        raise ValueError("exspec.run: an empty list of packet sources")
    nprocs = len(sources)
    reload = len(chunks) > 1 or len(sources) > 1
    if packet_sources is not None and not reload:
        engine.upload(load_packets(sources[0]))
    written, first = [], None
    trace = None
    if trace_regions is not None:
        trace_regions = list(trace_regions)
        trace = ffi.LineTraceArrays(model.nlines, len(trace_regions))
    for abin_first, abin_count, with_average in chunks:
        arrays = ffi.SpectraResArrays(nt, nnubins, model.nelements, model.maxnions, abin_first, abin_count,
                                      with_average, emission_res, stokes)
        for src in sources:
            if src is not None and reload:
                engine.upload(load_packets(src))
            engine.spectra_res(nnubins=nnubins, nprocs=nprocs, abin_first=abin_first, abin_count=abin_count,
                               with_average=with_average, syn_dir=syn_dir, out=arrays)
            if trace is not None and first is None:
                engine.line_trace(trace_regions, nnubins=nnubins, nprocs=nprocs, abin=-1, syn_dir=syn_dir, out=trace)
        written += write_outputs(outdir, model, arrays, gamma_dep=gamma_dep, cmf_lum=cmf_lum)
        if first is None:
            first = arrays
    if trace is None:
        return sorted(written), first
    write_line_trace(os.path.join(os.fspath(outdir), LINE_TRACE_FILE), model, trace, trace_regions)
    written.append(LINE_TRACE_FILE)
    return sorted(written), first, trace
