// spectra_host.h -- the host drivers of the spectra kernels (spectrum.h): artis_gpu_spectrum, artis_gpu_spectra,
// artis_gpu_spectra_res and artis_gpu_line_trace.  They share the init_spectra bin widths (spec_bins), the section
// list of artis_spectra_out (SpecSections: one accumulator per array given, with `nslots` leading slots), the
// consistency check of its arrays and the staged copy-back-and-ADD (AddBack); artis_gpu_spectra and
// artis_gpu_spectra_res are their validation and allocation around one body, spectra_run, that differs by the kernel
// launch.  Nothing is added to a caller's array before the stream is synchronised after the kernel: a failed call
// leaves the arrays as they were.  Included once by engine.hip after engine_state.h and its host helpers (G, HIPCHK,
// DevBufs, sync_ctx).
#pragma once

namespace {

// init_spectra (spectrum.cc:495-500): lower_freq and delta_freq are float arrays (spectrum.h:18-19), so the
// bin width every deltaE divides by is the float difference of the float lower edge
inline double spec_delta_freq(double nu_min, double dlognu, int nnu) {
  const float lower_freq = (float)exp(log(nu_min) + (nnu * (dlognu)));
  return (float)(exp(log(nu_min) + ((nnu + 1) * (dlognu))) - lower_freq);
}

// spectrum.cc:352, 491-500: nnubins log bins over [nu_min_r, nu_max_r], the reference's expressions (host libm)
struct SpecBins {
  double dlognu;
  std::vector<double> delta_freq;
};
SpecBins spec_bins(int nnubins) {
  const double nu_min = G.K.G.nu_min_r, nu_max = G.K.G.nu_max_r;
  SpecBins b{(log(nu_max) - log(nu_min)) / nnubins, std::vector<double>(nnubins)};
  for (int nnu = 0; nnu < nnubins; nnu++) b.delta_freq[nnu] = spec_delta_freq(nu_min, b.dlognu, nnu);
  return b;
}

// emission and absorption come together, and everything emission-resolved needs them
bool spec_arrays_consistent(const artis_spectra_out *out) {
  return (!out->emission == !out->absorption) && !(out->trueemission && !out->emission) &&
         !((out->stokes_emission || out->stokes_absorption) && !out->emission);
}

// The arrays of artis_spectra_out with `nslots` leading slots on every spectrum array and on lc_lum (1:
// artis_gpu_spectra): per array its doubles and the member of the kernels' SpecArgs that takes its device accumulator
// (NULL: not asked for)
struct SpecSections {
  struct Sec {
    double *host;
    size_t n;
    double **dev;
  };
  std::vector<Sec> s;
  size_t total = 0;  // doubles of the sections given

  SpecSections(const artis_spectra_out *out, size_t nslots, int nnubins, SpecArgs &A) {
    const size_t nt = G.ntstep, nb = nt * nnubins, ioncount = (size_t)G.nelements * G.maxnions,
                 proccount = 2 * ioncount + 1;
    s = {{out->flux, nslots * nb, &A.flux},
         {out->emission, nslots * nb * proccount, &A.emission},
         {out->trueemission, nslots * nb * proccount, &A.trueemission},
         {out->absorption, nslots * nb * ioncount, &A.absorption},
         {out->stokes_flux, nslots * 3 * nb, &A.sflux},
         {out->stokes_emission, nslots * 3 * nb * proccount, &A.semission},
         {out->stokes_absorption, nslots * 3 * nb * ioncount, &A.sabsorption},
         {out->lc_lum, nslots * nt, &A.lc},
         {out->lc_lumcmf, nt, &A.lccmf},
         {out->gamma_lc_lum, nt, &A.glc},
         {out->gamma_lc_lumcmf, nt, &A.glccmf}};
    for (const Sec &x : s)
      if (x.host) total += x.n;
  }
  void place(double *d) const {  // the accumulators one after the other from d
    for (const Sec &x : s) {
      *x.dev = x.host ? d : nullptr;
      if (x.host) d += x.n;
    }
  }
};

// Copy device sums back through a bounded staging buffer (at most `stage` doubles, allocated once) and ADD them to
// the caller's array.  The caller has synchronised the stream after its kernel.
struct AddBack {
  size_t stage;
  std::vector<double> h;
  int add(double *host, const double *dev, size_t n) {
    for (size_t o = 0; o < n; o += stage) {
      const size_t m = std::min(stage, n - o);
      if (h.size() < m) h.resize(m);
      HIPCHK(hipMemcpyAsync(h.data(), dev + o, m * sizeof(double), hipMemcpyDeviceToHost, G.stream));
      HIPCHK(hipStreamSynchronize(G.stream));
      double *dst = host + o;
      for (size_t j = 0; j < m; j++) dst[j] += h[j];
    }
    return 0;
  }
};
constexpr size_t SPECTRA_STAGE = (size_t)8 << 20;      // doubles (64 MiB)
constexpr size_t LINE_TRACE_STAGE = (size_t)1 << 19;  // doubles (4 MiB): small enough to stay warm

// The body of artis_gpu_spectra and artis_gpu_spectra_res: S lists the caller's arrays and A's members for them, d
// holds nnubins bin widths and then S.total accumulators; launch() starts the binning kernel with A on G.stream.
template <typename Launch>
int spectra_run(const SpecSections &S, SpecArgs &A, double *d, int nnubins, int nprocs, int abin,
                const double syn_dir[3], Launch launch) {
  const SpecBins bins = spec_bins(nnubins);
  if (int rc = sync_ctx()) return rc;
  HIPCHK(hipMemsetAsync(d + nnubins, 0, S.total * sizeof(double), G.stream));
  HIPCHK(hipMemcpyAsync(d, bins.delta_freq.data(), nnubins * sizeof(double), hipMemcpyHostToDevice, G.stream));
  S.place(d + nnubins);
  A.nnubins = nnubins;
  A.nprocs = nprocs;
  A.abin = abin;
  A.ntstep = G.ntstep;
  A.ioncount = G.nelements * G.maxnions;
  A.proccount = 2 * A.ioncount + 1;
  A.maxnions = G.maxnions;
  A.nbf = G.K.T.nbf;
  for (int k = 0; k < 3; k++) A.syn_dir[k] = syn_dir[k];
  A.dlognu = bins.dlognu;
  A.delta_freq = d;
  A.bf_col = G.d_bfcol;
  A.line_elem = G.K.T.line_elem;
  A.line_ion = G.K.T.line_ion;
  if (G.npkts > 0) launch();
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(G.stream));  // a kernel fault is reported before anything is added to the caller's arrays
  AddBack back{SPECTRA_STAGE};
  for (const SpecSections::Sec &x : S.s)
    if (x.host)
      if (int rc = back.add(x.host, *x.dev, x.n)) return rc;
  return 0;
}

}  // namespace

extern "C" {

int artis_gpu_spectrum(int nnubins, int nprocs, double *spec_flux, double *lc_lum, double *lc_lumcmf) {
  if (!G.initialised) return ARTIS_ERR_NOT_INITIALISED;
  if (nnubins <= 0 || nprocs <= 0 || !spec_flux || !lc_lum || !lc_lumcmf) return ARTIS_ERR_BAD_ARGUMENT;
  const int nt = G.ntstep;
  const SpecBins bins = spec_bins(nnubins);
  const size_t nspec = (size_t)nt * nnubins;
  DevBufs B;  // every step below may fail; the scratch is released (hipFree waits for the stream) on all paths
  double *d = nullptr;
  if (int rc = B.get(&d, nspec + 2 * (size_t)nt + nnubins, (const double *)nullptr)) return rc;
  double *d_spec = d, *d_lc = d + nspec, *d_lccmf = d_lc + nt, *d_delta = d_lccmf + nt;
  if (int rc = sync_ctx()) return rc;
  HIPCHK(hipMemsetAsync(d, 0, (nspec + 2 * (size_t)nt) * sizeof(double), G.stream));
  HIPCHK(hipMemcpyAsync(d_delta, bins.delta_freq.data(), nnubins * sizeof(double), hipMemcpyHostToDevice, G.stream));
  if (G.npkts > 0)
    k_spectrum<<<(unsigned)((G.npkts + 255) / 256), 256, 0, G.stream>>>(
        G.d_ctx, G.d_soa, G.npkts, nt, nnubins, bins.dlognu, d_delta, (double)nprocs, d_spec, d_lc, d_lccmf);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(spec_flux, d_spec, nspec * sizeof(double), hipMemcpyDeviceToHost, G.stream));
  HIPCHK(hipMemcpyAsync(lc_lum, d_lc, nt * sizeof(double), hipMemcpyDeviceToHost, G.stream));
  HIPCHK(hipMemcpyAsync(lc_lumcmf, d_lccmf, nt * sizeof(double), hipMemcpyDeviceToHost, G.stream));
  HIPCHK(hipStreamSynchronize(G.stream));
  return 0;
}

int artis_gpu_spectra(const artis_spectra_request *req, artis_spectra_out *out) {
  if (!G.initialised) return ARTIS_ERR_NOT_INITIALISED;
  if (!req || !out || req->nnubins <= 0 || req->nprocs <= 0 || req->abin < -1 || req->abin >= ARTIS_MABINS ||
      !spec_arrays_consistent(out)) {
    G.last_error = "spectra: bad request (nnubins, nprocs, abin) or inconsistent emission/absorption arrays";
    return ARTIS_ERR_BAD_ARGUMENT;
  }
  SpecArgs A{};
  const SpecSections S(out, 1, req->nnubins, A);
  DevBufs B;  // released on every path
  double *d = nullptr;
  if (int rc = B.get(&d, req->nnubins + S.total, (const double *)nullptr)) return rc;
  return spectra_run(S, A, d, req->nnubins, req->nprocs, req->abin, req->syn_dir, [&A] {
    k_spectra<<<(unsigned)((G.npkts + 255) / 256), 256, 0, G.stream>>>(G.d_ctx, G.d_soa, G.npkts, A);
  });
}

// The direction-resolved set in one pass (k_spectra_res): slot 0 the angle average (with_average), then the bins
// [abin_first, abin_first + abin_count); every spectrum array and lc_lum carry the leading slot dimension.
int artis_gpu_spectra_res(const artis_spectra_res_request *req, artis_spectra_out *out) {
  if (!G.initialised) return ARTIS_ERR_NOT_INITIALISED;
  if (!req || !out) {
    G.last_error = "spectra_res: NULL request or output";
    return ARTIS_ERR_BAD_ARGUMENT;
  }
  if (req->nnubins <= 0 || req->nprocs <= 0 || req->abin_first < 0 || req->abin_count < 0 ||
      req->abin_first > ARTIS_MABINS || req->abin_count > ARTIS_MABINS - req->abin_first ||
      (req->with_average != 0 && req->with_average != 1) || (req->abin_count == 0 && !req->with_average)) {
    G.last_error = "spectra_res: bad request (nnubins, nprocs > 0; bins [abin_first, abin_first + abin_count) within "
                   "[0, ARTIS_MABINS]; with_average 0 or 1; no bins needs with_average)";
    return ARTIS_ERR_BAD_ARGUMENT;
  }
  if (!spec_arrays_consistent(out)) {
    G.last_error = "spectra_res: inconsistent emission / absorption / Stokes arrays";
    return ARTIS_ERR_BAD_ARGUMENT;
  }
  if (!req->with_average && (out->lc_lumcmf || out->gamma_lc_lum || out->gamma_lc_lumcmf)) {
    G.last_error = "spectra_res: lc_lumcmf and the gamma-ray light curves belong to the angle average: NULL without "
                   "with_average";
    return ARTIS_ERR_BAD_ARGUMENT;
  }
  const size_t nslots = (size_t)req->with_average + (size_t)req->abin_count;
  SpecArgs A{};
  const SpecSections S(out, nslots, req->nnubins, A);
  const size_t bytes = (req->nnubins + S.total) * sizeof(double);
  {
    // all slots or none: a request that does not fit is refused before anything is allocated or binned
    size_t freeb = 0, totalb = 0;
    HIPCHK(hipMemGetInfo(&freeb, &totalb));
    if (bytes > freeb) {
      G.last_error = "spectra_res: out of device memory: the accumulators of " + std::to_string(nslots) +
                     " slots need " + std::to_string(bytes) + " bytes, " + std::to_string(freeb) +
                     " are free; ask for fewer direction bins per call (a smaller abin_count)";
      return ARTIS_ERR_HIP;
    }
  }
  DevBufs B;  // released on every path
  double *d = nullptr;
  if (int rc = B.get(&d, req->nnubins + S.total, (const double *)nullptr)) {
    (void)hipGetLastError();  // the failed allocation is reported here, not by the next launch check
    G.last_error = "spectra_res: out of device memory: allocating " + std::to_string(bytes) +
                   " bytes of accumulators failed; ask for fewer direction bins per call (a smaller abin_count)";
    return rc;
  }
  const SpecResArgs R{req->abin_first, req->abin_count, req->with_average};
  return spectra_run(S, A, d, req->nnubins, req->nprocs, -1, req->syn_dir, [&A, R] {
    k_spectra_res<<<(unsigned)((G.npkts + 255) / 256), 256, 0, G.stream>>>(G.d_ctx, G.d_soa, G.npkts, A, R);
  });
}

// The per-line emission / absorption trace (k_line_trace): lines [nregions][nlines][4] and totals [nregions][2],
// accumulated on the device per call and ADDED into the caller's arrays.
int artis_gpu_line_trace(const artis_line_trace_request *req, artis_line_trace_out *out) {
  if (!G.initialised) return ARTIS_ERR_NOT_INITIALISED;
  if (!req || !out) {
    G.last_error = "line_trace: NULL request or output";
    return ARTIS_ERR_BAD_ARGUMENT;
  }
  if (!out->lines || !out->totals || !req->regions) {
    G.last_error = "line_trace: NULL lines, totals or regions";
    return ARTIS_ERR_BAD_ARGUMENT;
  }
  if (req->nnubins <= 0 || req->nprocs <= 0 || req->abin < -1 || req->abin >= ARTIS_MABINS || req->nregions < 1 ||
      req->nregions > ARTIS_LINE_TRACE_MAX_REGIONS) {
    G.last_error = "line_trace: bad request (nnubins, nprocs > 0; abin in [-1, ARTIS_MABINS); nregions in "
                   "[1, ARTIS_LINE_TRACE_MAX_REGIONS])";
    return ARTIS_ERR_BAD_ARGUMENT;
  }
  for (int r = 0; r < req->nregions; r++) {
    const artis_line_trace_region &R = req->regions[r];
    if (!std::isfinite(R.nu_lower) || !std::isfinite(R.nu_upper) || !std::isfinite(R.time_min) ||
        !std::isfinite(R.time_max) || R.nu_lower > R.nu_upper || R.time_min > R.time_max) {
      G.last_error = "line_trace: region " + std::to_string(r) +
                     " has a non-finite bound, nu_lower > nu_upper or time_min > time_max";
      return ARTIS_ERR_BAD_ARGUMENT;
    }
  }
  const int nnb = req->nnubins, nreg = req->nregions;
  const SpecBins bins = spec_bins(nnb);
  const size_t nlin = (size_t)nreg * G.nlines * 4, ntot = (size_t)nreg * 2;
  const size_t total = nnb + nlin + ntot;  // delta_freq first, then lines, then totals
  DevBufs B;  // released on every path
  double *d = nullptr;
  if (int rc = B.get(&d, total, (const double *)nullptr)) {
    (void)hipGetLastError();  // the failed allocation is reported here, not by the next launch check
    G.last_error = "line_trace: out of device memory: allocating " + std::to_string(total * sizeof(double)) +
                   " bytes of accumulators failed; ask for fewer regions per call";
    return rc;
  }
  if (int rc = sync_ctx()) return rc;
  HIPCHK(hipMemsetAsync(d + nnb, 0, (nlin + ntot) * sizeof(double), G.stream));
  HIPCHK(hipMemcpyAsync(d, bins.delta_freq.data(), nnb * sizeof(double), hipMemcpyHostToDevice, G.stream));
  LineTraceArgs A{};
  A.nnubins = nnb;
  A.nprocs = req->nprocs;
  A.abin = req->abin;
  A.ntstep = G.ntstep;
  A.nregions = nreg;
  A.nlines = G.nlines;
  for (int k = 0; k < 3; k++) A.syn_dir[k] = req->syn_dir[k];
  A.dlognu = bins.dlognu;
  A.delta_freq = d;
  A.lines = d + nnb;
  A.totals = d + nnb + nlin;
  for (int r = 0; r < nreg; r++) A.regions[r] = req->regions[r];
  if (G.npkts > 0)
    k_line_trace<<<(unsigned)((G.npkts + 255) / 256), 256, 0, G.stream>>>(G.d_ctx, G.d_soa, G.npkts, A);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(G.stream));  // a kernel fault is reported before anything is added to the caller's arrays
  AddBack back{LINE_TRACE_STAGE};
  if (int rc = back.add(out->lines, A.lines, nlin)) return rc;
  return back.add(out->totals, A.totals, ntot);
}

}  // extern "C"
