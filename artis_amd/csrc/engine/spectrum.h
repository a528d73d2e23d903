// spectrum.h -- emergent spectrum and light curve of the escaped r-packets, binned on the device.
//
// The binning of write_partial_lightcurve_spectra (spectrum.cc:641-721): every packet with type TYPE_ESCAPE and
// escape_type TYPE_RPKT goes through add_to_lc_res (light_curve.cc:34-54) and add_to_spec (spectrum.cc:339-362),
// angle-averaged (abin -1), without the emission-resolved columns.  Sums are float64 atomics; the reference's
// serial loop adds in packet order, so sums agree to rounding (tests/test_spectrum.py).
#ifndef ARTIS_SPECTRUM_H
#define ARTIS_SPECTRUM_H

#include "physics.h"

// sn3d.h:168-180 get_timestep (linear search, as the reference)
DEVFN int spec_timestep(const Ctx &K, int ntstep, double t) {
  for (int nts = 0; nts < ntstep; nts++) {
    const double tsend = (nts < ntstep - 1) ? K.G.ts_start[nts + 1] : K.G.tmax;
    if (t >= K.G.ts_start[nts] && t < tsend) return nts;
  }
  return -1;
}

__global__ void k_spectrum(const Ctx *__restrict__ ctxp, const uint64_t *__restrict__ soa, int64_t n, int ntstep,
                           int nnubins, double dlognu, const double *__restrict__ delta_freq, double nprocs,
                           double *spec, double *lc_lum, double *lc_lumcmf) {
  const Ctx &K = *ctxp;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (hi32(soa[PW(n, i, 0)]) != ARTIS_TYPE_ESCAPE) return;
  const uint64_t w32 = soa[PW(n, i, 32)];
  if (lo32(w32) != ARTIS_TYPE_RPKT) return;
  const int escape_time = hi32(w32);
  const double pos[3] = {asd(soa[PW(n, i, 3)]), asd(soa[PW(n, i, 4)]), asd(soa[PW(n, i, 5)])};
  const double dir[3] = {asd(soa[PW(n, i, 6)]), asd(soa[PW(n, i, 7)]), asd(soa[PW(n, i, 8)])};
  const double e_cmf = asd(soa[PW(n, i, 9)]);
  const double e_rf = asd(soa[PW(n, i, 10)]);
  const double nu_rf = asd(soa[PW(n, i, 12)]);
  const double tmin = K.G.tmin, tmax = K.G.tmax;
  // light_curve.cc:39-52 (vectors.h:146-156 get_arrive_time / get_arrive_time_cmf)
  const double t_arrive = escape_time - (dot(pos, dir) / ARTIS_CLIGHT_PROP);
  if (t_arrive > tmin && t_arrive < tmax) {
    const int nt = spec_timestep(K, ntstep, t_arrive);
    if (nt >= 0) unsafeAtomicAdd(&lc_lum[nt], e_rf / K.G.ts_width[nt] / nprocs);
  }
  const double cmfcorr = sqrt(1. - (K.G.vmax * K.G.vmax / ARTIS_CLIGHTSQUARED));
  const double t_arrive_cmf = escape_time * cmfcorr;
  if (t_arrive_cmf > tmin && t_arrive_cmf < tmax) {
    const int nt = spec_timestep(K, ntstep, t_arrive_cmf);
    if (nt >= 0) unsafeAtomicAdd(&lc_lumcmf[nt], e_cmf / K.G.ts_width[nt] / nprocs / cmfcorr);
  }
  // spectrum.cc:348-362
  const double nu_min = K.G.nu_min_r, nu_max = K.G.nu_max_r;
  if (t_arrive > tmin && t_arrive < tmax && nu_rf > nu_min && nu_rf < nu_max) {
    const int nt = spec_timestep(K, ntstep, t_arrive);
    const int nnu = (int)((log(nu_rf) - log(nu_min)) / dlognu);
    if (nt >= 0 && nnu >= 0 && nnu < nnubins) {
      const double deltaE =
          e_rf / K.G.ts_width[nt] / delta_freq[nnu] / 4.e12 / ARTIS_PI / ARTIS_PARSEC / ARTIS_PARSEC / nprocs;
      unsafeAtomicAdd(&spec[(int64_t)nt * nnubins + nnu], deltaE);
    }
  }
}

// ---- exspec spectra (spectrum.cc:306-452, light_curve.cc:34-62) -------------------------------------------------
struct SpecArgs {
  int nnubins, nprocs, abin, ntstep, proccount, ioncount, maxnions, nbf;
  double syn_dir[3];
  double dlognu;
  const double *delta_freq;  // [nnubins] (init_spectra, host libm)
  const int32_t *bf_col;     // [nbf] bflist index -> element * maxnions + ion (columnindex_from_emissiontype)
  const int32_t *line_elem, *line_ion;
  double *flux, *emission, *trueemission, *absorption;
  double *sflux, *semission, *sabsorption;  // Stokes I, Q, U blocks one after the other
  double *lc, *lccmf, *glc, *glccmf;
};

// spectrum.cc:306-337 columnindex_from_emissiontype
DEVFN int spec_column(const SpecArgs &A, int et) {
  if (et >= 0) return A.line_elem[et] * A.maxnions + A.line_ion[et];
  if (et == -9999999 || A.nbf == 0) return 2 * A.ioncount;
  return A.ioncount + A.bf_col[-1 - et];
}

// vectors.h:158-193 get_escapedirectionbin (NPHIBINS = NCOSTHETABINS = 10, exspec.h:7-9)
DEVFN int escapedirectionbin(const double dir_in[3], const double syn_dir[3]) {
  const double xhat[3] = {1.0, 0.0, 0.0};
  const double dirmag = sqrt((dir_in[0] * dir_in[0]) + (dir_in[1] * dir_in[1]) + (dir_in[2] * dir_in[2]));
  const double dir[3] = {dir_in[0] / dirmag, dir_in[1] / dirmag, dir_in[2] / dirmag};
  const double costheta = dot(dir, syn_dir);
  const int costhetabin = (int)((costheta + 1.0) * 10 / 2.0);
  double vec1[3], vec2[3], vec3[3];
  cross_prod(dir, syn_dir, vec1);
  cross_prod(xhat, syn_dir, vec2);
  const double cosphi = dot(vec1, vec2) / vec_len(vec1) / vec_len(vec2);
  cross_prod(vec2, syn_dir, vec3);
  const double testphi = dot(vec1, vec3);
  int phibin;
  if (testphi > 0)
    phibin = (int)(acos(cosphi) / 2. / ARTIS_PI * 10);
  else
    phibin = (int)((acos(cosphi) + ARTIS_PI) / 2. / ARTIS_PI * 10);
  return (costhetabin * 10) + phibin;
}

// One escaped packet as both exspec kernels see it: the words every contribution needs, read once.
struct SpecPkt {
  int escape_type, escape_time;
  double dir[3];
  double e_cmf, e_rf;
  double t_arrive, cmfcorr, t_arrive_cmf;
};

// false: packet i has not escaped
DEVFN bool spec_load(const Ctx &K, const uint64_t *__restrict__ soa, int64_t n, int64_t i, SpecPkt &P) {
  if (hi32(soa[PW(n, i, 0)]) != ARTIS_TYPE_ESCAPE) return false;
  const uint64_t w32 = soa[PW(n, i, 32)];
  P.escape_type = lo32(w32);
  P.escape_time = hi32(w32);
  const double pos[3] = {asd(soa[PW(n, i, 3)]), asd(soa[PW(n, i, 4)]), asd(soa[PW(n, i, 5)])};
  P.dir[0] = asd(soa[PW(n, i, 6)]);
  P.dir[1] = asd(soa[PW(n, i, 7)]);
  P.dir[2] = asd(soa[PW(n, i, 8)]);
  P.e_cmf = asd(soa[PW(n, i, 9)]);
  P.e_rf = asd(soa[PW(n, i, 10)]);
  P.t_arrive = P.escape_time - (dot(pos, P.dir) / ARTIS_CLIGHT_PROP);
  P.cmfcorr = sqrt(1. - (K.G.vmax * K.G.vmax / ARTIS_CLIGHTSQUARED));
  P.t_arrive_cmf = P.escape_time * P.cmfcorr;
  return true;
}

// add_to_lc_res for the gamma-ray light curve (spectrum.cc:678-680): angle-averaged only
DEVFN void spec_add_gamma(const Ctx &K, const SpecArgs &A, const SpecPkt &P) {
  const double tmin = K.G.tmin, tmax = K.G.tmax;
  if (P.t_arrive > tmin && P.t_arrive < tmax && A.glc) {
    const int nt = spec_timestep(K, A.ntstep, P.t_arrive);
    if (nt >= 0) unsafeAtomicAdd(&A.glc[nt], P.e_rf / K.G.ts_width[nt] / A.nprocs);
  }
  if (P.t_arrive_cmf > tmin && P.t_arrive_cmf < tmax && A.glccmf) {
    const int nt = spec_timestep(K, A.ntstep, P.t_arrive_cmf);
    if (nt >= 0) unsafeAtomicAdd(&A.glccmf[nt], P.e_cmf / K.G.ts_width[nt] / A.nprocs / P.cmfcorr);
  }
}

// Everything one escaped r-packet adds to one output set: add_to_lc_res (light_curve.cc:34-62) and add_to_spec_res
// (spectrum.cc:339-452) with weight anglefactor, into slot `slot` of the spectrum arrays ([slot][ntstep][nnubins]
// [columns]; the Stokes blocks [slot][3]...) and into the light curves lc / lccmf ([ntstep], NULL: not produced --
// a direction bin has no cmf light curve).  Shared by k_spectra (slot 0) and k_spectra_res, so the two add the same
// numbers.  Every index is int64_t from its first product: slots * ntstep * nnubins * proccount * 3 passes 2^31.
DEVFN void spec_add_rpkt(const Ctx &K, const uint64_t *__restrict__ soa, int64_t n, int64_t i, const SpecArgs &A,
                         const SpecPkt &P, double anglefactor, int64_t slot, double *lc, double *lccmf) {
  const double tmin = K.G.tmin, tmax = K.G.tmax;
  const double t_arrive = P.t_arrive, t_arrive_cmf = P.t_arrive_cmf, e_rf = P.e_rf;
  if (t_arrive > tmin && t_arrive < tmax && lc) {
    const int nt = spec_timestep(K, A.ntstep, t_arrive);
    if (nt >= 0) unsafeAtomicAdd(&lc[nt], e_rf / K.G.ts_width[nt] * anglefactor / A.nprocs);
  }
  if (t_arrive_cmf > tmin && t_arrive_cmf < tmax && lccmf) {
    const int nt = spec_timestep(K, A.ntstep, t_arrive_cmf);
    if (nt >= 0) unsafeAtomicAdd(&lccmf[nt], P.e_cmf / K.G.ts_width[nt] / A.nprocs / P.cmfcorr);
  }
  // spectrum.cc:339-452 add_to_spec
  const double nu_rf = asd(soa[PW(n, i, 12)]);
  const double nu_min = K.G.nu_min_r, nu_max = K.G.nu_max_r;
  if (!(t_arrive > tmin && t_arrive < tmax && nu_rf > nu_min && nu_rf < nu_max)) return;
  const int nt = spec_timestep(K, A.ntstep, t_arrive);
  const int nnu = (int)((log(nu_rf) - log(nu_min)) / A.dlognu);
  if (nt < 0 || nnu < 0 || nnu >= A.nnubins) return;
  const double deltaE = e_rf / K.G.ts_width[nt] / A.delta_freq[nnu] / 4.e12 / ARTIS_PI / ARTIS_PARSEC / ARTIS_PARSEC /
                        A.nprocs * anglefactor;
  const double stokes[3] = {asd(soa[PW(n, i, 25)]), asd(soa[PW(n, i, 26)]), asd(soa[PW(n, i, 27)])};
  const int64_t nb = (int64_t)A.ntstep * A.nnubins;
  const int64_t fi = (int64_t)nt * A.nnubins + nnu;
  const int64_t pc = A.proccount, ic = A.ioncount;
  if (A.flux) unsafeAtomicAdd(&A.flux[slot * nb + fi], deltaE);
  if (A.sflux)
    for (int s = 0; s < 3; s++) unsafeAtomicAdd(&A.sflux[(slot * 3 + s) * nb + fi], stokes[s] * deltaE);
  if (!A.emission) return;
  const uint64_t w13 = soa[PW(n, i, 13)], w19 = soa[PW(n, i, 19)];
  const int nproc = spec_column(A, hi32(w13));
  const int truenproc = spec_column(A, hi32(w19));
  const int64_t ei = fi * pc;
  unsafeAtomicAdd(&A.emission[slot * nb * pc + ei + nproc], deltaE);
  if (A.trueemission) unsafeAtomicAdd(&A.trueemission[slot * nb * pc + ei + truenproc], deltaE);
  if (A.semission)
    for (int s = 0; s < 3; s++)
      unsafeAtomicAdd(&A.semission[(slot * 3 + s) * nb * pc + ei + nproc], stokes[s] * deltaE);
  const double absorptionfreq = asd(soa[PW(n, i, 21)]);
  const int nnu_abs = (int)((log(absorptionfreq) - log(nu_min)) / A.dlognu);
  const int at = lo32(w19);
  if (nnu_abs >= 0 && nnu_abs < A.nnubins && at >= 0 && A.absorption) {
    const double deltaE_absorption = e_rf / K.G.ts_width[nt] / A.delta_freq[nnu_abs] / 4.e12 / ARTIS_PI /
                                     ARTIS_PARSEC / ARTIS_PARSEC / A.nprocs * anglefactor;
    const int64_t ai = ((int64_t)nt * A.nnubins + nnu_abs) * ic + A.line_elem[at] * A.maxnions + A.line_ion[at];
    unsafeAtomicAdd(&A.absorption[slot * nb * ic + ai], deltaE_absorption);
    if (A.sabsorption)
      for (int s = 0; s < 3; s++)
        unsafeAtomicAdd(&A.sabsorption[(slot * 3 + s) * nb * ic + ai], stokes[s] * deltaE_absorption);
  }
}

__global__ void k_spectra(const Ctx *__restrict__ ctxp, const uint64_t *__restrict__ soa, int64_t n, SpecArgs A) {
  const Ctx &K = *ctxp;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  SpecPkt P;
  if (!spec_load(K, soa, n, i, P)) return;
  if (P.escape_type == ARTIS_TYPE_GAMMA) {
    if (A.abin == -1) spec_add_gamma(K, A, P);
    return;
  }
  if (P.escape_type != ARTIS_TYPE_RPKT) return;
  if (A.abin >= 0 && escapedirectionbin(P.dir, A.syn_dir) != A.abin) return;
  const double anglefactor = (A.abin >= 0) ? ARTIS_MABINS : 1.;
  spec_add_rpkt(K, soa, n, i, A, P, anglefactor, 0, A.lc, (A.abin == -1) ? A.lccmf : nullptr);
}

// ---- one pass for the direction-resolved set (exspec.cc:140-263: a = -1 .. MABINS-1) ---------------------------
// Slot 0 is the angle average when with_average is set; the bins [abin_first, abin_first + abin_count) follow.  An
// escaped r-packet belongs to the average (weight 1) and to the slot of its own direction bin (weight ARTIS_MABINS);
// lc_lumcmf and the gamma-ray light curves exist for the average only.  Everything is a global float64 atomic, the
// light curves included: a per-block LDS copy of them measured no faster.
struct SpecResArgs {
  int abin_first, abin_count, with_average;
};

__global__ void k_spectra_res(const Ctx *__restrict__ ctxp, const uint64_t *__restrict__ soa, int64_t n, SpecArgs A,
                              SpecResArgs R) {
  const Ctx &K = *ctxp;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  SpecPkt P;
  if (!spec_load(K, soa, n, i, P)) return;
  if (P.escape_type == ARTIS_TYPE_GAMMA) {
    if (R.with_average) spec_add_gamma(K, A, P);
    return;
  }
  if (P.escape_type != ARTIS_TYPE_RPKT) return;
  const int b = escapedirectionbin(P.dir, A.syn_dir);
  if (R.with_average) spec_add_rpkt(K, soa, n, i, A, P, 1., 0, A.lc, A.lccmf);
  // a direction outside every bin (b < 0 or b >= ARTIS_MABINS) belongs to no slot, as in k_spectra
  if (b >= R.abin_first && b < R.abin_first + R.abin_count) {
    const int64_t slot = R.with_average + (b - R.abin_first);
    spec_add_rpkt(K, soa, n, i, A, P, ARTIS_MABINS, slot, A.lc ? A.lc + slot * A.ntstep : nullptr, nullptr);
  }
}

// ---- the per-line emission / absorption trace (spectrum.cc:11-30, 395-408, 435-447, 454-468) --------------------
// TRACE_EMISSION_ABSORPTION_REGION_ON of add_to_spec for up to ARTIS_LINE_TRACE_MAX_REGIONS (time, frequency) windows
// in one pass: lines[region][line] is one struct emissionabsorptioncontrib (32 bytes: the two emission sums in one
// 16-byte half, the two absorption sums in the other), totals[region] = traceemission_totalenergy,
// traceabsorption_totalenergy.  The windows travel by value in the kernel arguments.
struct LineTraceArgs {
  int nnubins, nprocs, abin, ntstep, nregions, nlines;
  double syn_dir[3];
  double dlognu;
  const double *delta_freq;  // [nnubins] (init_spectra, host libm)
  double *lines;             // [nregions][nlines][4]
  double *totals;            // [nregions][2]
  artis_line_trace_region regions[ARTIS_LINE_TRACE_MAX_REGIONS];
};

// The sum of v over the wave, in every lane.  All 64 lanes must call it.
DEVFN double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// One thread per packet.  A thread without a contribution (past the end, not an escaped r-packet, outside the
// direction bin, refused by add_to_spec's admission test, in no window) keeps running with an empty window mask:
// the per-window totals are summed across the wave (one atomic per wave, window and total instead of one per
// packet on a single address), and the cross-lane sum needs all 64 lanes.  A window no lane of the wave lies in is
// skipped by a wave-uniform branch.  log(nu_rf), the timestep and deltaE are evaluated once per packet; the trace's
// own words (19, 21, 14-17, 35) are read only by a packet that lies in a window.
__global__ void k_line_trace(const Ctx *__restrict__ ctxp, const uint64_t *__restrict__ soa, int64_t n,
                             LineTraceArgs A) {
  const Ctx &K = *ctxp;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t inwin = 0;  // bit r: the packet lies in window r
  double deltaE = 0., nu_rf = 0., t_arrive = 0., e_rf = 0.;
  int nt = -1;
  SpecPkt P;
  if (i < n && spec_load(K, soa, n, i, P) && P.escape_type == ARTIS_TYPE_RPKT &&
      (A.abin < 0 || escapedirectionbin(P.dir, A.syn_dir) == A.abin)) {
    // spectrum.cc:346-360 add_to_spec, as spec_add_rpkt
    const double anglefactor = (A.abin >= 0) ? ARTIS_MABINS : 1.;
    const double tmin = K.G.tmin, tmax = K.G.tmax;
    const double nu_min = K.G.nu_min_r, nu_max = K.G.nu_max_r;
    t_arrive = P.t_arrive;
    e_rf = P.e_rf;
    nu_rf = asd(soa[PW(n, i, 12)]);
    if (t_arrive > tmin && t_arrive < tmax && nu_rf > nu_min && nu_rf < nu_max) {
      nt = spec_timestep(K, A.ntstep, t_arrive);
      const int nnu = (int)((log(nu_rf) - log(nu_min)) / A.dlognu);
      if (nt >= 0 && nnu >= 0 && nnu < A.nnubins) {
        deltaE = e_rf / K.G.ts_width[nt] / A.delta_freq[nnu] / 4.e12 / ARTIS_PI / ARTIS_PARSEC / ARTIS_PARSEC /
                 A.nprocs * anglefactor;
        // spectrum.cc:398-399, 435-438: both bounds inclusive
        for (int r = 0; r < A.nregions; r++) {
          const artis_line_trace_region &R = A.regions[r];
          if (t_arrive >= R.time_min && t_arrive <= R.time_max && nu_rf >= R.nu_lower && nu_rf <= R.nu_upper)
            inwin |= 1u << r;
        }
      }
    }
  }
  int et = -1, at = -1;
  double vem = 0., deltaE_absorption = 0., vab = 0.;
  if (inwin) {
    const uint64_t w19 = soa[PW(n, i, 19)];
    et = hi32(w19);
    if (et >= A.nlines) et = -1;  // no such line: never written by the transport
    if (et >= 0) vem = (double)__int_as_float(hi32(soa[PW(n, i, 35)])) * deltaE;  // spectrum.cc:402
    // spectrum.cc:410-416
    const double absorptionfreq = asd(soa[PW(n, i, 21)]);
    const int nnu_abs = (int)((log(absorptionfreq) - log(K.G.nu_min_r)) / A.dlognu);
    at = lo32(w19);
    if (!(nnu_abs >= 0 && nnu_abs < A.nnubins) || at >= A.nlines) at = -1;
    if (at >= 0) {
      const double anglefactor = (A.abin >= 0) ? ARTIS_MABINS : 1.;
      deltaE_absorption = e_rf / K.G.ts_width[nt] / A.delta_freq[nnu_abs] / 4.e12 / ARTIS_PI / ARTIS_PARSEC /
                          ARTIS_PARSEC / A.nprocs * anglefactor;
      // spectrum.cc:441-443: get_velocity at em_pos, em_time, then vec_len
      const double em_time = lo32(soa[PW(n, i, 17)]);
      const double vel[3] = {asd(soa[PW(n, i, 14)]) / em_time, asd(soa[PW(n, i, 15)]) / em_time,
                             asd(soa[PW(n, i, 16)]) / em_time};
      vab = vec_len(vel) * deltaE_absorption;
    }
  }
  const double em = (et >= 0) ? deltaE : 0., ab = (at >= 0) ? deltaE_absorption : 0.;
  const int lane = threadIdx.x & 63;
  for (int r = 0; r < A.nregions; r++) {
    const bool in = (inwin >> r) & 1u;
    if (__ballot(in) == 0) continue;  // wave-uniform
    if (in && et >= 0) {
      double *rec = A.lines + ((int64_t)r * A.nlines + et) * 4;
      unsafeAtomicAdd(rec + 0, deltaE);
      unsafeAtomicAdd(rec + 1, vem);
    }
    if (in && at >= 0) {
      double *rec = A.lines + ((int64_t)r * A.nlines + at) * 4;
      unsafeAtomicAdd(rec + 2, deltaE_absorption);
      unsafeAtomicAdd(rec + 3, vab);
    }
    const double sum_em = wave_sum(in ? em : 0.), sum_ab = wave_sum(in ? ab : 0.);
    if (lane == 0) {
      if (sum_em != 0.) unsafeAtomicAdd(&A.totals[2 * r + 0], sum_em);
      if (sum_ab != 0.) unsafeAtomicAdd(&A.totals[2 * r + 1], sum_ab);
    }
  }
}

#endif
