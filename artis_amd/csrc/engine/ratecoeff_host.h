// ratecoeff_host.h -- the host driver of the rate-coefficient lookup tables: artis_gpu_ratecoeff_tables
// (ratecoefficients_init's precalculate_rate_coefficient_integrals and precalculate_ion_alpha_sp, ratecoeff.cc:450-625,
// 970-992) and artis_gpu_last_ratecoeff_ms.  The call needs no engine and touches none: it validates its arguments
// before any HIP call, then works on a stream, events and allocations of its own, all released before it returns
// (the device that was current is made current again).  Host code only; included once by engine.hip after
// engine_state.h (HIPCHK, DevBufs) and the other host drivers.
#pragma once

namespace {

double g_last_ratecoeff_ms = 0.;

// the stream, events and current device of one call, put back on every path
struct RcScope {
  int prev_device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ~RcScope() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
    if (prev_device >= 0) (void)hipSetDevice(prev_device);
  }
};

int rc_bad(const std::string &why) {
  G.last_error = "ratecoeff_tables: " + why;
  return ARTIS_ERR_BAD_ARGUMENT;
}

}  // namespace

extern "C" {

double artis_gpu_last_ratecoeff_ms(void) { return g_last_ratecoeff_ms; }

int artis_gpu_ratecoeff_tables(int device, const artis_atomic_tables *a, const artis_ratecoeff_request *req,
                               artis_ratecoeff_out *out) {
  // ---- arguments, before any HIP call
  if (!a || !req || !out) return rc_bad("NULL atomic tables, request or output");
  if (device < 0) return rc_bad("negative device");
  if (!(req->epsrel > 0) || !std::isfinite(req->epsrel)) return rc_bad("epsrel must be positive and finite");
  if (req->list_lds_capacity != 0 && req->list_lds_capacity != RC_LIST_DEFAULT &&
      req->list_lds_capacity != RC_LIST_SMALL)
    return rc_bad("unknown list_lds_capacity " + std::to_string(req->list_lds_capacity) + " (0 = default, " +
                  std::to_string(RC_LIST_DEFAULT) + " or " + std::to_string(RC_LIST_SMALL) + ")");
  if (a->tablesize < 2) return rc_bad("tablesize must be at least 2");
  if (!(a->mintemp > 0) || !(a->mintemp < a->maxtemp) || !std::isfinite(a->maxtemp))
    return rc_bad("needs 0 < mintemp < maxtemp");
  if (a->nelements <= 0 || a->nions_total <= 0 || a->nlevels_total <= 0 || a->nbfcontinua <= 0 ||
      a->nphixspoints <= 0 || !(a->nphixsnuincrement > 0) || !(a->last_phixs_nuovernuedge > 1))
    return rc_bad("empty atomic tables (elements, ions, levels, bf continua, cross-section grid)");
  if (a->phixs_file_version != 1 && a->phixs_file_version != 2) return rc_bad("phixs_file_version must be 1 or 2");
  if (!a->elem_nions || !a->elem_uniqueionoffset || !a->ion_nlevels || !a->ion_uniqueleveloffset ||
      !a->ion_ionisinglevels || !a->level_epsilon || !a->level_stat_weight || !a->level_nphixstargets ||
      !a->level_phixstargets_offset || !a->level_cont_index || !a->level_phixstable || !a->phixstarget_levelindex ||
      !a->phixstarget_probability || !a->phixs_xs)
    return rc_bad("a NULL array among the element / ion / level / photoionisation tables");
  if (!out->spontrecombcoeff || !out->bfcooling_coeff) return rc_bad("NULL spontrecombcoeff or bfcooling_coeff");
  if (out->ion_alpha_sp == nullptr) return rc_bad("NULL ion_alpha_sp");
  const int ne = a->nelements, ni = a->nions_total, nl = a->nlevels_total, nbf = a->nbfcontinua, ts = a->tablesize;
  for (int e = 0; e < ne; e++) {
    const int off = a->elem_uniqueionoffset[e], n = a->elem_nions[e];
    if (n <= 0 || off < 0 || (int64_t)off + n > ni) return rc_bad("element " + std::to_string(e) + ": ions out of range");
  }
  for (int ui = 0; ui < ni; ui++) {
    const int off = a->ion_uniqueleveloffset[ui], n = a->ion_nlevels[ui];
    if (n <= 0 || off < 0 || (int64_t)off + n > nl || a->ion_ionisinglevels[ui] < 0 || a->ion_ionisinglevels[ui] > n)
      return rc_bad("ion " + std::to_string(ui) + ": levels out of range");
  }
  std::vector<RcCont> cont;
  if (!ratecoeff_continua(a, &cont))
    return rc_bad("level_cont_index does not number the photoionisation targets 0 .. nbfcontinua-1");
  // what the kernel reads: the target slots and the cross-section rows of the listed continua
  int64_t ntargets = 0, ntables = 0;
  for (int col = 0; col < nbf; col++) {
    const RcCont &c = cont[col];
    const int ui = a->elem_uniqueionoffset[c.e] + c.i;
    const int ul = a->ion_uniqueleveloffset[ui] + c.l;
    const int64_t slot = (int64_t)a->level_phixstargets_offset[ul] + c.t;
    if (a->level_phixstargets_offset[ul] < 0 || a->level_phixstable[ul] < 0)
      return rc_bad("level " + std::to_string(ul) + ": no photoionisation targets or cross-section table");
    const int upper = a->phixstarget_levelindex[slot];
    if (upper < 0 || upper >= a->ion_nlevels[ui + 1])
      return rc_bad("level " + std::to_string(ul) + ": photoionisation target outside the upper ion");
    ntargets = std::max(ntargets, slot + 1);
    ntables = std::max<int64_t>(ntables, (int64_t)a->level_phixstable[ul] + 1);
  }
  const size_t lutsize = (size_t)ts * nbf;
  const double T_step_log = ratecoeff_T_step_log(a->mintemp, a->maxtemp, ts);
  std::vector<float> T_e(ts);
  for (int iter = 0; iter < ts; iter++) {
    T_e[iter] = ratecoeff_table_temperature(a->mintemp, T_step_log, iter);
    if (std::floor(std::log(T_e[iter] / a->mintemp) / T_step_log) < 0)  // get_spontrecombcoeff's assert_always
      return rc_bad("table temperature " + std::to_string(iter) + " rounds below mintemp as a float");
  }

  // ---- device work on a stream of its own
  RcScope S;
  HIPCHK(hipGetDevice(&S.prev_device));
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreate(&S.ev0));
  HIPCHK(hipEventCreate(&S.ev1));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  DevBufs B;  // released on every path
  Ctx K{};
  DevTab &T = K.T;
  T.nelements = ne;
  T.maxnions = a->maxnions;
  T.nions_total = ni;
  T.nlevels_total = nl;
  T.nbf = nbf;
  T.nphixspoints = a->nphixspoints;
  T.phixs_file_version = a->phixs_file_version;
  T.tablesize = ts;
  T.nphixsnuincrement = a->nphixsnuincrement;
  T.last_phixs_nuovernuedge = a->last_phixs_nuovernuedge;
  T.mintemp = a->mintemp;
  T.T_step_log = T_step_log;
  CallerArrays in(B);
  in.in(&T.elem_nions, ne, a->elem_nions);
  in.in(&T.elem_uniqueionoffset, ne, a->elem_uniqueionoffset);
  in.in(&T.ion_uniqueleveloffset, ni, a->ion_uniqueleveloffset);
  in.in(&T.ion_ionisinglevels, ni, a->ion_ionisinglevels);
  in.in(&T.level_epsilon, nl, a->level_epsilon);
  in.in(&T.level_stat_weight, nl, a->level_stat_weight);
  in.in(&T.level_nphixstargets, nl, a->level_nphixstargets);
  in.in(&T.level_phixstargets_offset, nl, a->level_phixstargets_offset);
  in.in(&T.level_cont_index, nl, a->level_cont_index);
  in.in(&T.level_phixstable, nl, a->level_phixstable);
  in.in(&T.phixstarget_levelindex, (size_t)ntargets, a->phixstarget_levelindex);
  in.in(&T.phixstarget_probability, (size_t)ntargets, a->phixstarget_probability);
  in.in(&T.phixs_xs, (size_t)ntables * a->nphixspoints, a->phixs_xs);
  RcArgs A{};
  A.ncont = nbf;
  A.tablesize = ts;
  A.epsrel = req->epsrel;
  in.in(&A.cont, cont.size(), cont.data());
  in.in(&A.T_e, T_e.size(), T_e.data());
  if (in.rc) return in.rc;
  const bool want_gamma = out->corrphotoioncoeff != nullptr, want_heat = out->bfheating_coeff != nullptr;
  if (B.get(&A.spontrecombcoeff, lutsize, (const double *)nullptr) ||
      B.get(&A.bfcooling_coeff, lutsize, (const double *)nullptr) ||
      (want_gamma && B.get(&A.corrphotoioncoeff, lutsize, (const double *)nullptr)) ||
      (want_heat && B.get(&A.bfheating_coeff, lutsize, (const double *)nullptr)) ||
      (out->status && B.get(&A.status, 4 * lutsize, (const uint8_t *)nullptr)) ||
      (out->intervals && B.get(&A.intervals, 4 * lutsize, (const int32_t *)nullptr)))
    return ARTIS_ERR_HIP;
  // one wave per block and a contiguous share of the items per block.  The kernel's registers admit one wave per SIMD
  // (four blocks per CU); eight blocks per CU are launched so that a CU that ends early takes another share.
  const int64_t total = (int64_t)lutsize;
  const int nblocks = (int)std::min<int64_t>(total, (int64_t)std::max(1, prop.multiProcessorCount) * 8);
  QagWs ws{};
  const size_t wsn = (size_t)nblocks * QAG_LIMIT;
  if (B.get(&ws.alist, wsn, (const double *)nullptr) || B.get(&ws.blist, wsn, (const double *)nullptr) ||
      B.get(&ws.rlist, wsn, (const double *)nullptr) || B.get(&ws.elist, wsn, (const double *)nullptr) ||
      B.get(&ws.order, wsn, (const int32_t *)nullptr) || B.get(&ws.level, wsn, (const int32_t *)nullptr))
    return ARTIS_ERR_HIP;
  HIPCHK(hipEventRecord(S.ev0, S.stream));
  if (req->list_lds_capacity == RC_LIST_SMALL)
    k_ratecoeff_lut<RC_LIST_SMALL><<<nblocks, 64, 0, S.stream>>>(K, A, ws);
  else
    k_ratecoeff_lut<RC_LIST_DEFAULT><<<nblocks, 64, 0, S.stream>>>(K, A, ws);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(S.ev1, S.stream));
  HIPCHK(hipStreamSynchronize(S.stream));  // a kernel fault is reported before the caller's arrays are written
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, S.ev0, S.ev1));
  g_last_ratecoeff_ms = ms;
  auto back = [&](void *host, const void *dev, size_t bytes) -> int {
    if (host) HIPCHK(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return 0;
  };
  if (back(out->spontrecombcoeff, A.spontrecombcoeff, lutsize * sizeof(double)) ||
      back(out->bfcooling_coeff, A.bfcooling_coeff, lutsize * sizeof(double)) ||
      back(out->corrphotoioncoeff, A.corrphotoioncoeff, lutsize * sizeof(double)) ||
      back(out->bfheating_coeff, A.bfheating_coeff, lutsize * sizeof(double)) ||
      back(out->status, A.status, 4 * lutsize) || back(out->intervals, A.intervals, 4 * lutsize * sizeof(int32_t)))
    return ARTIS_ERR_HIP;
  // precalculate_ion_alpha_sp: a host function of the table just made (its one refusal was checked above)
  (void)ratecoeff_ion_alpha_sp(a, out->spontrecombcoeff, out->ion_alpha_sp);
  return 0;
}

}  // extern "C"
