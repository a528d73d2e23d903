// update_grid_host.h -- the host drivers of update_grid: artis_gpu_solve_temperatures and
// artis_gpu_prepare_temperatures (LTE-population options, te_solver.h) and artis_gpu_update_grid_nlte (nebular
// options, nlte_solver.h).  Every caller array is copied in, the solution is computed for the listed cells and
// every array is copied back on success, so cells not listed round-trip unchanged; on any failure the caller's
// arrays are not written.  Host code only; included once by engine.hip after engine_state.h, host_tables.h and
// nlte_tables.h (the kernels and their TeDev / UgDev / NlDev / SfDev / NlMat views come from engine.hip's headers)
// and before the readout drivers estimators_host.h and spectra_host.h.
#pragma once

namespace {

template <typename T>
int d2h_vec(std::vector<T> &h, const T *d, size_t n) {
  h.assign(n, T());
  if (n) HIPCHK(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
  return 0;
}

// the entry points of the LTE-population options refuse the nebular ones
int lte_options_only(const char *who) {
  const DevRun &R = G.K.R;
  if (!(R.nlte_on || R.no_lut_photoion || R.no_lut_bfheating || R.nt_on)) return 0;
  G.last_error = std::string(who) + ": only the LTE-population options (NLTE_POPS_ON, NO_LUT_*, NT_ON false)";
  return ARTIS_ERR_UNSUPPORTED;
}

int cells_in_range(const char *who, const int32_t *mgi, int ncells) {
  for (int k = 0; k < ncells; k++)
    if (mgi[k] < 0 || mgi[k] >= G.npts_model) {
      G.last_error = std::string(who) + ": cell index out of range";
      return ARTIS_ERR_BAD_ARGUMENT;
    }
  return 0;
}

// the heating sum's level list (nlte_tables.h bfheat_levels) from the device's ion bookkeeping
int read_bfheat_levels(const char *who, NlAtoms &A, std::vector<int32_t> &hb) {
  const DevTab &T = G.K.T;
  A.ne = G.nelements;
  A.ni = G.nions_total;
  if (d2h_vec(A.nions, T.elem_nions, A.ne) || d2h_vec(A.uoff, T.elem_uniqueionoffset, A.ne) ||
      d2h_vec(A.ionis, T.ion_ionisinglevels, A.ni) || d2h_vec(A.ion_ul0, T.ion_uniqueleveloffset, A.ni))
    return ARTIS_ERR_HIP;
  for (int e = 0; e < A.ne; e++)
    if (A.nions[e] > TE_MAX_IONS_PER_ELEMENT) {
      G.last_error = std::string(who) + ": more ions per element than TE_MAX_IONS_PER_ELEMENT";
      return ARTIS_ERR_UNSUPPORTED;
    }
  hb = bfheat_levels(A);
  return 0;
}

void te_set_params(TeDev &D, double T_min, double T_max, double accuracy, double tmin, double t_current,
                   int initial_iteration) {
  D.T_min = T_min;
  D.T_max = T_max;
  D.accuracy = accuracy;
  D.tmin = tmin;
  D.t_current = t_current;
  D.initial_iteration = initial_iteration;
}

}  // namespace

extern "C" {
// ============================================================================ update_grid temperature solution
int artis_gpu_solve_temperatures(const artis_te_tables *tab, const artis_te_params *par, artis_te_cells *c) {
  if (!G.initialised) return ARTIS_ERR_NOT_INITIALISED;
  if (int rc = lte_options_only("solve_temperatures")) return rc;
  if (!tab || !par || !c || !tab->bfheating_coeff || !tab->ion_alpha_sp || c->ncells < 0 || (c->ncells > 0 && !c->mgi) ||
      !c->TR || !c->W || !c->TJ || !c->rho || !c->thick || !c->elem_abundance || !c->elem_meanweight || !c->vol_init ||
      !c->ffheatingestimator || !c->colheatingestimator || !c->gammaestimator || !c->bfheatingestimator || !c->Te ||
      !c->groundlevelpop || !c->nne || !c->nnetot || !c->partfunct || !c->totalcooling || !c->cooling_contrib_ion ||
      !(par->T_min > 0. && par->T_max > par->T_min && par->accuracy > 0. && par->tmin > 0. && par->t_current > 0.)) {
    G.last_error = "solve_temperatures: NULL table / cell array or bad parameters";
    return ARTIS_ERR_BAD_ARGUMENT;
  }
  if (int rc = cells_in_range("solve_temperatures", c->mgi, c->ncells)) return rc;
  if (c->ncells == 0) return 0;
  const int np = G.npts_model, ne = G.nelements, ni = G.nions_total, nmx = G.maxnions;
  const DevTab &T = G.K.T;
  NlAtoms A;
  std::vector<int32_t> hb;
  if (int rc = read_bfheat_levels("solve_temperatures", A, hb)) return rc;
  DevBufs B;
  CallerArrays io(B);
  TeDev D{};
  const size_t npf = (size_t)np, npi = (size_t)np * ni, npe = (size_t)np * ne, npg = (size_t)np * ne * nmx;
  io.in(&D.bfheat_lut, (size_t)T.tablesize * T.nbf, tab->bfheating_coeff);
  io.in(&D.alpha_sp, (size_t)ni * T.tablesize, tab->ion_alpha_sp);
  io.in(&D.anumber, (size_t)ne, G.h_anumber.data());
  io.in(&D.hb_ul, hb.size(), hb.data());
  io.in(&D.mgi, (size_t)c->ncells, c->mgi);
  io.in(&D.TR, npf, c->TR);
  io.in(&D.W, npf, c->W);
  io.in(&D.TJ, npf, c->TJ);
  io.in(&D.rho, npf, c->rho);
  io.in(&D.thick, npf, c->thick);
  io.in(&D.abund, npe, c->elem_abundance);
  io.in(&D.meanw, npe, c->elem_meanweight);
  io.in(&D.vol, npf, c->vol_init);
  io.in(&D.ffheat, npf, c->ffheatingestimator);
  io.in(&D.colheat, npf, c->colheatingestimator);
  io.in(&D.gamma, npg, c->gammaestimator);
  io.in(&D.bfest, npg, c->bfheatingestimator);
  if (c->heating_dep) io.in(&D.hdep, npf, c->heating_dep);
  io.io(&D.Te, npf, c->Te);
  io.io(&D.gp, npi, c->groundlevelpop);
  io.io(&D.nne, npf, c->nne);
  io.io(&D.nnetot, npf, c->nnetot);
  io.io(&D.pf, npi, c->partfunct);
  io.io(&D.totcool, npf, c->totalcooling);
  io.io(&D.ccion, npi, c->cooling_contrib_ion);
  if (c->heatingcoolingrates) io.io(&D.rates, npf * ARTIS_TE_NRATES, c->heatingcoolingrates);
  if (c->te_iterations) io.io(&D.iters, npf, c->te_iterations);
  // scratch
  io.io(&D.upp, npe, (int32_t *)nullptr);
  io.io(&D.hbc, hb.size() * (size_t)c->ncells, (double *)nullptr);
  io.io(&D.fail, 1, (int32_t *)nullptr);
  if (io.rc) return ARTIS_ERR_HIP;
  HIPCHK(hipMemsetAsync(D.fail, 0, sizeof(int32_t), G.stream));
  D.nhb = (int32_t)hb.size();
  D.ncells = c->ncells;
  te_set_params(D, par->T_min, par->T_max, par->accuracy, par->tmin, par->t_current, par->initial_iteration);
  D.direct_col_heat = par->direct_col_heat;
  HIPCHK(hipEventRecord(G.ev0, G.stream));
  if (D.nhb > 0) {
    const int64_t nw = (int64_t)D.nhb * D.ncells;
    k_te_bfheat<<<(unsigned)((nw + 255) / 256), 256, 0, G.stream>>>(G.K, D);
  }
  // lanes per cell: one per ion for the per-ion collisional-excitation sums of the cooling rate (te_cooling_rates),
  // floor(64 / g) cells per wave (12 ions: 5 cells on 60 lanes); ARTIS_GPU_TE_LANES overrides (1 = one cell per lane)
  const int g = G.knob.te_lanes ? G.knob.te_lanes : te_lanes_per_cell(ni);
  const int cpw = 64 / g;
  Ctx *dK = nullptr;
  TeDev *dD = nullptr;
  if (B.get(&dK, 1, &G.K) || B.get(&dD, 1, &D)) return ARTIS_ERR_HIP;
  k_te_solve<<<(unsigned)((D.ncells + cpw - 1) / cpw), 64, (size_t)cpw * ni * sizeof(double), G.stream>>>(dK, dD, g);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(G.ev1, G.stream));
  HIPCHK(hipEventSynchronize(G.ev1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, G.ev0, G.ev1));
  G.last_te_ms = ms;
  int32_t fail = 0;
  HIPCHK(hipMemcpy(&fail, D.fail, sizeof(int32_t), hipMemcpyDeviceToHost));
  if (fail) {
    // the caller's cell state is left as it was: the reference aborts before writing a partial solution
    char buf[160];
    snprintf(buf, sizeof buf,
             "solve_temperatures: a GSL root-finder error (endpoints do not straddle zero / non-finite value) in "
             "model cell %d -- the reference aborts here",
             fail - 1);
    G.last_error = buf;
    return ARTIS_ERR_PACKET_FAULT;
  }
  return io.download();
}
double artis_gpu_last_te_ms(void) { return G.last_te_ms; }

int artis_gpu_prepare_temperatures(const artis_te_tables *tab, const artis_te_params *par, const artis_ug_prepare *pr,
                                   const artis_te_cells *c) {
  if (!G.initialised) return ARTIS_ERR_NOT_INITIALISED;
  if (int rc = lte_options_only("prepare_temperatures")) return rc;
  if (!tab || !par || !pr || !c || !tab->bfheating_coeff || c->ncells < 0 || (c->ncells > 0 && !c->mgi) || !c->TR ||
      !c->W || !c->TJ || !c->Te || !c->rho || !c->thick || !c->elem_abundance || !c->vol_init || !c->groundlevelpop ||
      !pr->J || !pr->nuJ || !pr->ffheating || !pr->colheating || !pr->gammaestimator || !pr->bfheatingestimator ||
      !pr->nne || !pr->TR_out || !pr->W_out || !pr->TJ_out || !pr->ffheating_out ||
      !pr->colheating_out || !pr->gamma_out || !pr->bfheating_out || !pr->corrphotoionrenorm_out ||
      !(pr->deltat > 0. && pr->tratmid > 0. && pr->nprocs > 0 && par->T_max > par->T_min && par->T_min > 0.)) {
    G.last_error = "prepare_temperatures: NULL array or bad parameters";
    return ARTIS_ERR_BAD_ARGUMENT;
  }
  if (int rc = cells_in_range("prepare_temperatures", c->mgi, c->ncells)) return rc;
  if (c->ncells == 0) return 0;
  const int np = G.npts_model, ne = G.nelements, ni = G.nions_total, nmx = G.maxnions;
  const size_t npf = (size_t)np, npi = (size_t)np * ni, npe = (size_t)np * ne, npg = (size_t)np * ne * nmx;
  DevBufs B;
  CallerArrays io(B);
  UgDev U{};
  io.in(&U.mgi, (size_t)c->ncells, c->mgi);
  io.in(&U.TR, npf, c->TR);
  io.in(&U.W, npf, c->W);
  io.in(&U.TJ, npf, c->TJ);
  io.in(&U.Te, npf, c->Te);
  io.in(&U.nne, npf, pr->nne);
  io.in(&U.gp, npi, c->groundlevelpop);
  io.in(&U.rho, npf, c->rho);
  io.in(&U.abund, npe, c->elem_abundance);
  io.in(&U.thick, npf, c->thick);
  io.in(&U.vol, npf, c->vol_init);
  io.in(&U.J, npf, pr->J);
  io.in(&U.nuJ, npf, pr->nuJ);
  io.in(&U.ff, npf, pr->ffheating);
  io.in(&U.col, npf, pr->colheating);
  io.in(&U.gam, npg, pr->gammaestimator);
  io.in(&U.bfh, npg, pr->bfheatingestimator);
  io.in(&U.bfheat_lut, (size_t)G.K.T.tablesize * G.K.T.nbf, tab->bfheating_coeff);
  io.io(&U.TR_out, npf, pr->TR_out);
  io.io(&U.W_out, npf, pr->W_out);
  io.io(&U.TJ_out, npf, pr->TJ_out);
  io.io(&U.ff_out, npf, pr->ffheating_out);
  io.io(&U.col_out, npf, pr->colheating_out);
  io.io(&U.gam_out, npg, pr->gamma_out);
  io.io(&U.bfh_out, npg, pr->bfheating_out);
  io.io(&U.renorm_out, npg, pr->corrphotoionrenorm_out);
  io.io(&U.fail, 1, (int32_t *)nullptr);
  if (io.rc) return ARTIS_ERR_HIP;
  HIPCHK(hipMemsetAsync(U.fail, 0, sizeof(int32_t), G.stream));
  U.ncells = c->ncells;
  U.nprocs = pr->nprocs;
  U.initial_iteration = par->initial_iteration;
  U.deltat = pr->deltat;
  U.tratmid = pr->tratmid;
  U.T_min = par->T_min;
  U.T_max = par->T_max;
  Ctx *dK = nullptr;
  UgDev *dU = nullptr;
  if (B.get(&dK, 1, &G.K) || B.get(&dU, 1, &U)) return ARTIS_ERR_HIP;
  k_ug_prepare<<<(unsigned)((U.ncells + 255) / 256), 256, 0, G.stream>>>(dK, dU);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(G.stream));
  int32_t fail = 0;
  HIPCHK(hipMemcpy(&fail, U.fail, sizeof(int32_t), hipMemcpyDeviceToHost));
  if (fail) {
    char buf[320];
    snprintf(buf, sizeof buf,
             "prepare_temperatures: non-finite corrphotoionrenorm or bf-heating renormalisation in model cell %d "
             "(e.g. W = 0 or a zero analytic coefficient) -- the reference aborts here (update_grid.cc:911-918, "
             "959-965)",
             fail - 1);
    G.last_error = buf;
    return ARTIS_ERR_PACKET_FAULT;
  }
  return io.download();
}
}  // extern "C"

// ============================================================================== update_grid, nebular options
// artis_gpu_update_grid_nlte: the stages of one call in the order the driver below runs them, sharing this state.
// The kernels of solve_Te_nltepops run per pass for the cells still iterating; the host reads back the convergence
// flags between passes.
namespace {
struct NlCall {
  const artis_nt_shells *nt;
  const artis_nlte_params *p;
  artis_nlte_cells *c;
  const DevRun &R = G.K.R;
  const DevTab &T = G.K.T;
  const int np = G.npts_model, ne = G.nelements, ni = G.nions_total;
  const int nl = T.nlevels_total, nbf = T.nbf, nbins = T.rf_nbins, ntl = T.total_nlte_levels;
  const int64_t ntg = T.ntargets_total;
  const bool sf_on = R.nt_on && R.nt_solve_spencerfano;
  static constexpr int TB = 256;
  // lanes per cell of k_te_solve: always one per ion here (ARTIS_GPU_TE_LANES is the LTE entry point's)
  const int g = te_lanes_per_cell(ni), cpw = 64 / g;
  bool nl_debug = false;  // ARTIS_GPU_NL_DEBUG=1: synchronise after every step and name the first one that fails
  NlAtoms A;
  std::vector<int32_t> hb, lte_list, nl_list;  // bf-heating levels; the LTE-branch and the iterated cells
  int nnl = 0, nact_max = 1;
  DevBufs B;
  CallerArrays io{B};
  // three views of the same device arrays: the solver's, the thermal balance's (te_solver.h) and the engine context
  // with its cell-state pointers at the solver's arrays and the active cells as the "non-empty" list
  NlDev N{};
  TeDev D{};
  Ctx KN = G.K;
  SfDev S{};
  NlMat M{};
  NlLayout L;
  Ctx *dK = nullptr;
  TeDev *dD = nullptr;
  NlDev *dN = nullptr;
  int32_t *d_act = nullptr, *d_actk = nullptr;
  const int32_t *d_lte = nullptr, *d_nl = nullptr;
  double *d_pops = nullptr, *d_corr = nullptr;
  double2 *d_depr = nullptr;
  QagWs ws = G.qag;  // the integration workspace (the engine's, or one of its own)
  int qwaves = G.qag_waves;
  int chunk = 1, sf_batch = 1;  // cells per rate-matrix chunk / Spencer-Fano batch
  std::vector<double> h_none;   // errbest seeds (-1: no solution yet)
  std::vector<int32_t> act, actk, h_iters;  // cells still iterating, their rows in nl_list; passes by model cell

  NlCall(const artis_nt_shells *nt_, const artis_nlte_params *p_, artis_nlte_cells *c_) : nt(nt_), p(p_), c(c_) {}

  int step(const char *what) const {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && nl_debug) e = hipStreamSynchronize(G.stream);
    if (e != hipSuccess) {
      G.last_error = std::string("update_grid_nlte: ") + what + ": " + hipGetErrorString(e);
      return ARTIS_ERR_HIP;
    }
    return 0;
  }

  int read_fail(const char *where) const {
    int32_t f[2] = {0, 0};
    HIPCHK(hipStreamSynchronize(G.stream));
    HIPCHK(hipMemcpy(f, N.fail, sizeof f, hipMemcpyDeviceToHost));
    if (!f[0]) return 0;
    static const char *why[] = {"a GSL root-finder error of call_T_e_finder / calculate_populations",
                                "a GSL root-finder error of the radiation-field bin fit (find_T_R)",
                                "a non-finite bf-heating coefficient",
                                "get_mean_binding_energy has no shell data for the work-function approximation",
                                "non-finite or negative NLTE populations", "the T_e finder"};
    char buf[320];
    snprintf(buf, sizeof buf, "update_grid_nlte (%s): %s in model cell %d -- the reference aborts here", where,
             why[(f[1] >= 0 && f[1] <= 5) ? f[1] : 0], f[0] - 1);
    G.last_error = buf;
    return ARTIS_ERR_PACKET_FAULT;
  }

  int te_launch(const int32_t *list, int n, int mode, const int32_t *hbk) {
    if (n <= 0) return 0;
    D.mgi = list;
    D.ncells = n;
    D.mode = mode;
    D.hbk = hbk;
    HIPCHK(hipStreamSynchronize(G.stream));  // dD is read by the previous launch
    HIPCHK(hipMemcpy(dD, &D, sizeof(TeDev), hipMemcpyHostToDevice));
    k_te_solve<<<(unsigned)((n + cpw - 1) / cpw), 64, (size_t)cpw * ni * sizeof(double), G.stream>>>(dK, dD, g);
    HIPCHK(hipGetLastError());
    return 0;
  }

  template <typename T>
  void up(const T **d, const std::vector<T> &v) {
    io.in(d, v.size(), v.data());
  }

  int validate() const {
    if (!R.nlte_on || !R.no_lut_photoion || !R.no_lut_bfheating || !R.multibin) {
      G.last_error = "update_grid_nlte: needs the nebular options (NLTE_POPS_ON, NO_LUT_PHOTOION / BFHEATING, MULTIBIN)";
      return ARTIS_ERR_UNSUPPORTED;
    }
    if (R.nt_on && R.nt_max_auger != ARTIS_NT_MAX_AUGER) {
      G.last_error = "update_grid_nlte: nt_max_auger_electrons must be ARTIS_NT_MAX_AUGER";
      return ARTIS_ERR_UNSUPPORTED;
    }
    if (!p || !c || c->ncells < 0 || (c->ncells > 0 && !c->mgi) || !c->rho || !c->elem_abundance ||
        !c->elem_meanweight || !c->vol_init || !c->thick || !c->J || !c->nuJ || !c->ffheating || !c->bin_J_raw ||
        !c->bin_nuJ_raw || !c->bin_contribcount || !c->TR || !c->W || !c->TJ || !c->Te || !c->nne || !c->nnetot ||
        !c->groundlevelpop || !c->partfunct || !c->nlte_pops || !c->bin_TR || !c->bin_W || !c->totalcooling ||
        !c->cooling_contrib_ion || (R.detailed_bf && (!c->bfrate_raw || !c->bfrate_estimator)) ||
        (R.nt_on && (!c->deposition_rate_density || !c->nt_ionization_ratecoeff || !c->nt_eff_ionpot ||
                     !c->nt_frac_heating || !c->nt_frac_ionization || !c->nt_frac_excitation ||
                     !c->nt_nneperion_when_solved || !c->nt_timestep_last_solved || !c->nt_fracdep_ionization_ion ||
                     !c->nt_prob_num_auger || !c->nt_ionenfrac_num_auger)) ||
        (sf_on && (!nt || nt->sfpts < 2 || nt->sfpts > SF_NMAX || !(nt->sf_emax > nt->sf_emin) || nt->nshells < 0 ||
                   (nt->nshells > 0 && (!nt->Z || !nt->nelec || !nt->ionpot_ev || !nt->A || !nt->B || !nt->C ||
                                        !nt->D || !nt->prob_num_auger || !nt->en_auger_ev)) ||
                   !nt->electron_binding)) ||
        !(p->T_min > 0. && p->T_max > p->T_min && p->accuracy > 0. && p->tmin > 0. && p->t_current_te > 0. &&
          p->deltat > 0. && p->tratmid > 0. && p->nprocs > 0 && p->T_R_max > p->T_R_min && p->nlteiter >= 0)) {
      G.last_error = "update_grid_nlte: NULL array or bad parameters";
      return ARTIS_ERR_BAD_ARGUMENT;
    }
    return cells_in_range("update_grid_nlte", c->mgi, c->ncells);
  }

  // host copies of the atomic bookkeeping the layouts need
  int read_atoms() {
    if (int rc = read_bfheat_levels("update_grid_nlte", A, hb)) return rc;
    A.nl = nl;
    A.anumber = G.h_anumber.data();
    A.ion_ionpot = G.h_ion_ionpot.data();
    if (d2h_vec(A.ion_nlev, T.ion_nlevels, ni) || d2h_vec(A.nlte_n, T.ion_nlevels_nlte, ni) ||
        d2h_vec(A.ionstage, T.ion_ionstage, ni) || d2h_vec(A.lev_nup, T.level_nuptrans, nl) ||
        d2h_vec(A.lev_upoff, T.level_uptrans_offset, nl) || d2h_vec(A.lev_eps, T.level_epsilon, nl) ||
        d2h_vec(A.lev_g, T.level_stat_weight, nl))
      return ARTIS_ERR_HIP;
    return 0;
  }

  void split_cells() {
    for (int k = 0; k < c->ncells; k++) {
      const int mgi = c->mgi[k];
      (p->initial_iteration || c->thick[mgi] == 1 ? lte_list : nl_list).push_back(mgi);
    }
    nnl = (int)nl_list.size();
    nact_max = std::max(1, nnl);
  }

  // the caller's arrays, each once: io() arrays come back on success (a count of 0 or a NULL pointer: not at all)
  int upload_cells() {
    const size_t npf = np, npi = (size_t)np * ni, npe = (size_t)np * ne, npb = (size_t)np * nbins, A1 = NL_A1;
    N.np = np;
    N.ncells = c->ncells;
    io.in(&N.mgi, (size_t)c->ncells, c->mgi);
    N.nts = p->nts;
    N.num_lte_timesteps = p->num_lte_timesteps;
    N.initial_iteration = p->initial_iteration;
    N.nprocs = p->nprocs;
    N.do_rlc_est = p->do_rlc_est;
    N.nt_on = R.nt_on;
    N.sf_on = sf_on;
    N.deltat = p->deltat;
    N.tratmid = p->tratmid;
    N.T_min = p->T_min;
    N.T_max = p->T_max;
    N.T_R_min = p->T_R_min;
    N.T_R_max = p->T_R_max;
    io.in(&N.rho, npf, c->rho);
    io.in(&N.abund, npe, c->elem_abundance);
    io.in(&N.meanw, npe, c->elem_meanweight);
    io.in(&N.vol, npf, c->vol_init);
    io.in(&N.thick, npf, c->thick);
    io.in(&N.dep, npf, R.nt_on ? c->deposition_rate_density : nullptr);
    io.in(&N.J, npf, c->J);
    io.in(&N.nuJ, npf, c->nuJ);
    io.in(&N.ffraw, npf, c->ffheating);
    io.in(&N.bfraw, (size_t)np * nbf, R.detailed_bf ? c->bfrate_raw : nullptr);
    io.in(&N.binJ, npb, c->bin_J_raw);
    io.in(&N.binnuJ, npb, c->bin_nuJ_raw);
    io.in(&N.bincount, npb, c->bin_contribcount);
    io.io(&N.TR, npf, c->TR);
    io.io(&N.W, npf, c->W);
    io.io(&N.TJ, npf, c->TJ);
    io.io(&N.Te, npf, c->Te);
    io.io(&N.nne, npf, c->nne);
    io.io(&N.nnetot, npf, c->nnetot);
    io.io(&N.gp, npi, c->groundlevelpop);
    io.io(&N.pf, npi, c->partfunct);
    io.io(&N.nlte, (size_t)np * ntl, c->nlte_pops);
    io.io(&N.binTR, npb, c->bin_TR);
    io.io(&N.binW, npb, c->bin_W);
    io.io(&N.bfrate, (size_t)np * nbf, R.detailed_bf ? c->bfrate_estimator : nullptr);
    if (R.nt_on) {
      io.io(&N.nt_fh, npf, c->nt_frac_heating);
      io.io(&N.nt_fi, npf, c->nt_frac_ionization);
      io.io(&N.nt_fe, npf, c->nt_frac_excitation);
      io.io(&N.nt_nneper, npf, c->nt_nneperion_when_solved);
      io.io(&N.nt_tls, npf, c->nt_timestep_last_solved);
      io.io(&N.nt_effion, npi, c->nt_eff_ionpot);
      io.io(&N.nt_fracdep, npi, c->nt_fracdep_ionization_ion);
      io.io(&N.nt_prob, npi * A1, c->nt_prob_num_auger);
      io.io(&N.nt_ionen, npi * A1, c->nt_ionenfrac_num_auger);
      io.io(&N.ntY, npi, c->nt_ionization_ratecoeff);
    }
    io.io(&D.totcool, npf, c->totalcooling);
    io.io(&D.ccion, npi, c->cooling_contrib_ion);
    io.io(&D.rates, npf * ARTIS_TE_NRATES, c->heatingcoolingrates);
    // scratch
    io.io(&N.ffheat, npf, (double *)nullptr);
    io.io(&N.hdep, npf, (double *)nullptr);
    io.io(&N.prevTe, npf, (double *)nullptr);
    io.io(&N.fail, 2, (int32_t *)nullptr);
    io.io(&d_act, (size_t)nact_max, (int32_t *)nullptr);
    io.io(&d_actk, (size_t)nact_max, (int32_t *)nullptr);
    io.in(&d_lte, lte_list.size(), lte_list.data());
    io.in(&d_nl, nl_list.size(), nl_list.data());
    io.io(&d_pops, (size_t)nact_max * nl, (double *)nullptr);
    io.io(&d_corr, (size_t)nact_max * (ntg + 1), (double *)nullptr);
    io.io(&d_depr, (size_t)nact_max * nbf, (double2 *)nullptr);
    io.io(&D.hbc, hb.size() * nact_max, (double *)nullptr);
    io.in(&D.anumber, (size_t)ne, G.h_anumber.data());
    io.in(&D.hb_ul, hb.size(), hb.data());
    io.io(&D.upp, npe, (int32_t *)nullptr);
    if (io.rc) return ARTIS_ERR_HIP;
    if (!c->heatingcoolingrates) HIPCHK(hipMemsetAsync(D.rates, 0, npf * ARTIS_TE_NRATES * sizeof(double), G.stream));
    HIPCHK(hipMemsetAsync(N.fail, 0, 2 * sizeof(int32_t), G.stream));
    HIPCHK(hipMemsetAsync(N.ffheat, 0, npf * sizeof(double), G.stream));
    HIPCHK(hipMemsetAsync(N.hdep, 0, npf * sizeof(double), G.stream));
    return 0;
  }

  int wire_views() {
    KN.R.nts = p->nts;
    KN.C.Te = D.Te = N.Te;
    KN.C.TR = D.TR = N.TR;
    KN.C.TJ = D.TJ = N.TJ;
    KN.C.W = D.W = N.W;
    KN.C.nne = D.nne = N.nne;
    KN.C.nnetot = D.nnetot = N.nnetot;
    KN.C.rho = D.rho = N.rho;
    KN.C.thick = D.thick = N.thick;
    KN.C.elem_abundance = D.abund = N.abund;
    KN.C.groundlevelpop = D.gp = N.gp;
    KN.C.partfunct = D.pf = N.pf;
    KN.C.nlte_pops = D.nlte = N.nlte;
    KN.C.rf_TR = N.binTR;
    KN.C.rf_W = N.binW;
    KN.C.bfrate_est = N.bfrate;
    KN.C.nt_dep = N.dep;
    KN.C.nt_Y = N.ntY;
    KN.C.nt_prob = N.nt_prob;
    KN.C.nt_ionen = N.nt_ionen;
    KN.C.pops = d_pops;
    KN.C.corrphot = d_corr;
    KN.C.bfcell = d_depr;
    KN.C.ionpop = nullptr;  // (k_bfcells writes only the departure ratios here)
    KN.C.ne_mgi = d_act;
    KN.C.n_nonempty = 0;
    KN.C.linecoef = nullptr;
    KN.C.linecoef_rows = 0;
    D.meanw = N.meanw;
    D.vol = N.vol;
    D.ffheat = N.ffheat;
    D.hdep = N.hdep;
    D.fail = N.fail;
    D.nhb = (int32_t)hb.size();
    te_set_params(D, p->T_min, p->T_max, p->accuracy, p->tmin, p->t_current_te, p->initial_iteration);
    D.direct_col_heat = 1;
    D.hbstride = nact_max;
    if (B.get(&dK, 1, &KN) || B.get(&dD, 1, (const TeDev *)nullptr) || B.get(&dN, 1, &N)) return ARTIS_ERR_HIP;
    return 0;
  }

  // update_grid.cc:1104-1150 for every listed cell; the LTE-branch cells: precalculate_partfuncts +
  // calculate_populations (LTE phi) + the cooling rates
  int prepare_and_lte_branch() {
    nl_debug = getenv("ARTIS_GPU_NL_DEBUG") && getenv("ARTIS_GPU_NL_DEBUG")[0] == '1';
    if (int rc = step("uploads")) return rc;
    k_nl_prepare<<<(c->ncells + TB - 1) / TB, TB, 0, G.stream>>>(N);
    if (int rc = step("k_nl_prepare")) return rc;
    if (int rc = te_launch(d_lte, (int)lte_list.size(), 0, nullptr)) return rc;
    return step("k_te_solve (LTE branch)");
  }

  // the Spencer-Fano tables and batch buffers when a cell iterates; with NT_ON at least the binding energies the
  // work-function fallback of nt_ionization_ratecoeff reads
  int upload_sf_tables() {
    if (!R.nt_on) return 0;
    std::vector<double> binding;
    std::vector<int32_t> binding_ok;
    sf_ion_binding(A, nt ? nt->electron_binding : nullptr, binding, binding_ok);
    up(&S.ion_binding, binding);
    up(&S.ion_binding_ok, binding_ok);
    S.anumber = D.anumber;
    if (sf_on && nnl > 0) {
      const int64_t nup = A.lev_upoff.empty() ? 0 : (int64_t)A.lev_upoff[nl - 1] + A.lev_nup[nl - 1];
      if (d2h_vec(A.line_upper, T.line_upper, T.nlines) || d2h_vec(A.line_coll, T.line_coll, T.nlines) ||
          d2h_vec(A.line_f, T.line_f, T.nlines) || d2h_vec(A.line_forb, T.line_forbidden, T.nlines) ||
          d2h_vec(A.upidx, T.uptrans_lineindex, (size_t)std::max<int64_t>(nup, 0)))
        return ARTIS_ERR_HIP;
      const SfTables H = sf_build_tables(nt, A);
      const int n = H.n;
      S.n = n;
      S.emin = H.emin;
      S.emax = H.emax;
      S.DE = H.DE;
      S.E_init_ev = H.E_init_ev;
      S.band = H.band;
      S.nsh = (int32_t)H.sh_k.size();
      S.nitems = S.nsh + (int32_t)H.tr_ul.size();
      up(&S.envec, H.envec);
      up(&S.logenvec, H.logenvec);
      up(&S.pw2, H.pw2);
      up(&S.rhs, H.rhs);
      up(&S.ion_sh_off, H.sh_off);
      up(&S.sh_k, H.sh_k);
      up(&S.sh_xsstart, H.sh_start);
      up(&S.sh_augerstop, H.sh_astop);
      up(&S.sh_ionpot_ev, H.sh_ip);
      up(&S.sh_J, H.sh_J);
      up(&S.sh_xs, H.sh_xs);
      up(&S.sh_ieu, H.sh_ieu);
      up(&S.sh_atn, H.sh_atn);
      up(&S.sh_ie2, H.sh_ie2);
      up(&S.sh_prob, H.sh_prob);
      up(&S.ion_tr_off, H.tr_off);
      up(&S.tr_ul, H.tr_ul);
      up(&S.tr_kind, H.tr_kind);
      up(&S.tr_start, H.tr_start);
      up(&S.tr_build, H.tr_build);
      up(&S.tr_cf, H.tr_cf);
      up(&S.tr_logeps, H.tr_logeps);
      up(&S.tr_eps_ev, H.tr_eps_ev);
      up(&S.tr_eps, H.tr_eps);
      // cells solved together: their matrices (8 n^2 bytes each) within ARTIS_GPU_SF_BATCH_GB (default 8 GiB)
      const double sf_gb = G.knob.sf_batch_gb;
      sf_batch = (int)std::max<double>(1., std::min<double>(nnl, sf_gb * (double)(1ull << 30) / (8.0 * n * n)));
      h_none.assign(sf_batch, -1.);
      const size_t nbq = (size_t)sf_batch;
      io.in(&S.bat_a, nbq, (const int32_t *)nullptr);
      io.in(&S.bat_mgi, nbq, (const int32_t *)nullptr);
      io.io(&S.nnion, nbq * ni, (double *)nullptr);
      io.io(&S.incl, nbq * ni, (int32_t *)nullptr);
      io.io(&S.tot_nion, nbq, (double *)nullptr);
      io.io(&S.MT, nbq * n * n, (double *)nullptr);
      io.io(&S.x, nbq * n, (double *)nullptr);
      io.io(&S.best, nbq * n, (double *)nullptr);
      io.io(&S.work, nbq * n, (double *)nullptr);
      io.io(&S.res, nbq * n, (double *)nullptr);
      io.io(&S.part, nbq * n * ((n + SF_RCHUNK - 1) / SF_RCHUNK), (double *)nullptr);
      io.io(&S.errbest, nbq, (double *)nullptr);
      io.io(&S.dots, nbq * S.nitems, (double *)nullptr);
      io.io(&S.solve, (size_t)nact_max, (int32_t *)nullptr);
    }
    return io.rc ? ARTIS_ERR_HIP : 0;
  }

  int upload_matrix_layout() {
    if (!nl_matrix_layout(A, L)) {
      G.last_error = "update_grid_nlte: an ion with fewer levels than nlevels_nlte + 1";
      return ARTIS_ERR_UNSUPPORTED;
    }
    M.cell1 = L.cell1;
    M.cell2 = L.cell2;
    M.t_mid = p->t_mid;
    const double per_cell = (7.0 * L.cell2 + 8.0 * L.cell1) * 8.0 + 4.0 * (L.cell1 + ne);
    chunk = std::max(1, std::min(nact_max, (int)std::min(1e9, (double)(1ll << 30) / per_cell)));
    up(&M.el_D, L.el_D);
    up(&M.el_off1, L.el_off1);
    up(&M.el_off2, L.el_off2);
    up(&M.col_e, L.col_e);
    up(&M.col_ion, L.col_ion);
    up(&M.col_l0, L.col_l0);
    up(&M.col_l1, L.col_l1);
    io.io(&M.A, (size_t)chunk * L.cell2, (double *)nullptr);
    io.io(&M.LU, (size_t)chunk * L.cell2, (double *)nullptr);
    io.io(&M.P, (size_t)chunk * 5 * L.cell2, (double *)nullptr);
    for (double **v : {&M.b, &M.norm, &M.pv, &M.xv, &M.best, &M.work, &M.res})
      io.io(v, (size_t)chunk * L.cell1, (double *)nullptr);
    io.io(&M.perm, (size_t)chunk * L.cell1, (int32_t *)nullptr);
    io.io(&M.status, (size_t)chunk * ne, (int32_t *)nullptr);
    io.io(&M.slpf, (size_t)nact_max * ni, (double *)nullptr);
    io.io(&M.done, (size_t)nact_max, (int32_t *)nullptr);
    if (qwaves <= 0) {
      qwaves = 64;
      const size_t nw = (size_t)qwaves * QAG_LIMIT;
      io.io(&ws.alist, nw, (double *)nullptr);
      io.io(&ws.blist, nw, (double *)nullptr);
      io.io(&ws.rlist, nw, (double *)nullptr);
      io.io(&ws.elist, nw, (double *)nullptr);
      io.io(&ws.order, nw, (int32_t *)nullptr);
      io.io(&ws.level, nw, (int32_t *)nullptr);
    }
    return io.rc ? ARTIS_ERR_HIP : 0;
  }

  // radiation-field fit and bf-heating coefficients of the iterated cells
  int radfield_and_bfheat() {
    if (nbf > 0 && R.detailed_bf)
      k_nl_bfnorm<<<(unsigned)(((int64_t)nnl * nbf + TB - 1) / TB), TB, 0, G.stream>>>(KN, N, d_nl, nnl);
    if (int rc = step("k_nl_bfnorm")) return rc;
    if (nbins > 0)
      k_nl_binfit<<<(unsigned)(((int64_t)nnl * nbins + 63) / 64), 64, 0, G.stream>>>(dK, dN, d_nl, nnl);
    if (int rc = step("k_nl_binfit")) return rc;
    if (!hb.empty())
      k_nl_bfheat<<<(unsigned)std::min<int64_t>((int64_t)nnl * hb.size(), qwaves), 64, 0, G.stream>>>(
          dK, dN, d_nl, nnl, D.hb_ul, (int)hb.size(), D.hbc, ws);
    if (int rc = step("k_nl_bfheat")) return rc;
    if (int rc = read_fail("radiation field / bf heating")) return rc;
    D.hbstride = nnl;
    return 0;
  }

  // solve_spencerfano for nb cells: active positions sa, model cells sm
  int sf_batch_solve(const int32_t *sa, const int32_t *sm, int nb) {
    const int n = S.n;
    HIPCHK(hipMemcpy((void *)S.bat_a, sa, nb * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy((void *)S.bat_mgi, sm, nb * sizeof(int32_t), hipMemcpyHostToDevice));
    k_sf_ions<<<(nb * ni + 63) / 64, 64, 0, G.stream>>>(KN, N, S, nb);
    if (int rc = step("k_sf_ions")) return rc;
    k_sf_matrix<<<dim3((unsigned)((n + 255) / 256), (unsigned)n, (unsigned)nb), 256, 0, G.stream>>>(KN, N, S, d_pops);
    if (int rc = step("k_sf_matrix")) return rc;
    for (int q = 0; q < nb; q++)
      HIPCHK(hipMemcpyAsync(S.x + (size_t)q * n, S.rhs, n * sizeof(double), hipMemcpyDeviceToDevice, G.stream));
    k_sf_backsub<<<nb, SF_WG, 0, G.stream>>>(S.MT, n, S.x);
    if (int rc = step("k_sf_backsub")) return rc;
    HIPCHK(hipMemcpyAsync(S.errbest, h_none.data(), nb * sizeof(double), hipMemcpyHostToDevice, G.stream));
    const dim3 rgrid((unsigned)((n + 255) / 256), (unsigned)((n + SF_RCHUNK - 1) / SF_RCHUNK), (unsigned)nb);
    const dim3 vgrid((unsigned)((n + 255) / 256), (unsigned)nb);
    for (int it = 0; it < 10; it++) {
      if (it > 0) {
        k_sf_residual_part<<<rgrid, 256, 0, G.stream>>>(S.MT, n, S.x, S.part);
        k_sf_residual_sum<<<vgrid, 256, 0, G.stream>>>(n, S.part, S.rhs, S.work);
        k_sf_backsub<<<nb, SF_WG, 0, G.stream>>>(S.MT, n, S.work);
        k_sf_axpy<<<vgrid, 256, 0, G.stream>>>(n, S.x, S.work);
      }
      k_sf_residual_part<<<rgrid, 256, 0, G.stream>>>(S.MT, n, S.x, S.part);
      k_sf_residual_sum<<<vgrid, 256, 0, G.stream>>>(n, S.part, S.rhs, S.res);
      k_sf_best<<<nb, 1024, 0, G.stream>>>(n, S.res, S.x, S.best, S.errbest);
      if (int rc = step("Spencer-Fano refinement")) return rc;
    }
    k_sf_dots<<<dim3((unsigned)((S.nitems + 63) / 64), (unsigned)nb), 64, 0, G.stream>>>(S, S.best);
    if (int rc = step("k_sf_dots")) return rc;
    k_sf_combine<<<(nb + 63) / 64, 64, 0, G.stream>>>(KN, N, S, d_pops, nb);
    if (int rc = step("k_sf_combine")) return rc;
    HIPCHK(hipStreamSynchronize(G.stream));  // the batch lists and errbest seeds are reused
    if (!sf_dumped && n <= SF_DUMP_NMAX && getenv("ARTIS_GPU_NL_DUMP")) {
      sf_dumped = true;
      if (int rc = dump_sf(getenv("ARTIS_GPU_NL_DUMP"), sm[0])) return rc;
    }
    return 0;
  }

  // diagnostics (ARTIS_GPU_NL_DUMP): the call's first Spencer-Fano solve, batch slot 0 -- the matrix (column-major),
  // the right-hand side and the kept solution; only up to SF_DUMP_NMAX points (32 MB)
  static constexpr int SF_DUMP_NMAX = 2048;
  bool sf_dumped = false;
  int dump_sf(const char *prefix, int mgi) const {
    const size_t n = (size_t)S.n;
    std::vector<double> hM, hrhs, hbest;
    if (d2h_vec(hM, (const double *)S.MT, n * n) || d2h_vec(hrhs, S.rhs, n) || d2h_vec(hbest, (const double *)S.best, n))
      return ARTIS_ERR_HIP;
    const std::string path = std::string(prefix) + "_sf_gpu.bin";
    if (FILE *fp = fopen(path.c_str(), "wb")) {
      const int32_t hdr[2] = {S.n, mgi};
      fwrite(hdr, sizeof hdr, 1, fp);
      fwrite(hM.data(), 8, hM.size(), fp);
      fwrite(hrhs.data(), 8, hrhs.size(), fp);
      fwrite(hbest.data(), 8, hbest.size(), fp);
      fclose(fp);
    }
    return 0;
  }

  // diagnostics (ARTIS_GPU_NL_DUMP): a pass's rate matrices of the first active cell (tools/nl_dump_cmp.py), its level
  // populations, corrected photoionisation coefficients and bf-heating coefficients (by hb_ul)
  int dump_matrices(const char *prefix, int iter) const {
    HIPCHK(hipStreamSynchronize(G.stream));
    std::vector<double> hA, hbv, hn, hp, hpops, hcorr, hhbc;
    std::vector<int32_t> hs;
    if (d2h_vec(hA, M.A, (size_t)L.cell2) || d2h_vec(hbv, M.b, (size_t)L.cell1) ||
        d2h_vec(hn, M.norm, (size_t)L.cell1) || d2h_vec(hp, M.pv, (size_t)L.cell1) ||
        d2h_vec(hs, M.status, (size_t)ne) || d2h_vec(hpops, d_pops, (size_t)nl) ||
        d2h_vec(hcorr, d_corr, (size_t)ntg) || d2h_vec(hhbc, (const double *)D.hbc, hb.size() * (size_t)nnl))
      return ARTIS_ERR_HIP;
    const std::string path = std::string(prefix) + "_p" + std::to_string(iter) + "_gpu.bin";
    if (FILE *fp = fopen(path.c_str(), "wb")) {
      const int32_t hdr[5] = {ne, L.cell1, (int32_t)L.cell2, nl, (int32_t)ntg};
      fwrite(hdr, sizeof hdr, 1, fp);
      fwrite(L.el_D.data(), 4, ne, fp);
      fwrite(hs.data(), 4, ne, fp);
      fwrite(hA.data(), 8, hA.size(), fp);
      fwrite(hbv.data(), 8, hbv.size(), fp);
      fwrite(hn.data(), 8, hn.size(), fp);
      fwrite(hp.data(), 8, hp.size(), fp);
      fwrite(hpops.data(), 8, hpops.size(), fp);
      fwrite(hcorr.data(), 8, hcorr.size(), fp);
      const int32_t nhb = (int32_t)hb.size();
      fwrite(&nhb, 4, 1, fp);
      fwrite(hb.data(), 4, hb.size(), fp);
      for (size_t j = 0; j < hb.size(); j++) fwrite(&hhbc[j * nnl + actk[0]], 8, 1, fp);  // hbc[level][iterated cell]
      fclose(fp);
    }
    return 0;
  }

  // the rate matrices, their LU solutions and the stored populations of active cells a0 .. a0 + nch - 1
  int matrix_chunk(int iter, int a0, int nch) {
    if (L.cell1 > 0) {
      k_nl_matrix<<<(unsigned)(((int64_t)nch * L.cell1 + 63) / 64), 64, 0, G.stream>>>(KN, N, M, d_act, a0, nch);
      if (int rc = step("k_nl_matrix")) return rc;
      k_nl_lu<<<(unsigned)(nch * ne), NL_LU_WG, 0, G.stream>>>(KN, M, nch);
      if (int rc = step("k_nl_lu")) return rc;
      if (a0 == 0 && getenv("ARTIS_GPU_NL_DUMP") && iter < 4)
        if (int rc = dump_matrices(getenv("ARTIS_GPU_NL_DUMP"), iter)) return rc;
    }
    k_nl_store<<<(nch + 63) / 64, 64, 0, G.stream>>>(dK, dD, N, M, d_act, a0, nch);
    return step("k_nl_store");
  }

  // one pass of solve_Te_nltepops for the cells in act; those not converged stay in it
  int pass(int iter) {
    const int nact = (int)act.size();
    HIPCHK(hipMemcpyAsync(d_act, act.data(), nact * sizeof(int32_t), hipMemcpyHostToDevice, G.stream));
    HIPCHK(hipMemcpyAsync(d_actk, actk.data(), nact * sizeof(int32_t), hipMemcpyHostToDevice, G.stream));
    KN.C.n_nonempty = nact;
    const int64_t nlv = (int64_t)nact * nl;
    if (sf_on) {
      k_levelpops<<<(unsigned)((nlv + TB - 1) / TB), TB, 0, G.stream>>>(KN);
      if (int rc = step("k_levelpops (Spencer-Fano)")) return rc;
      k_sf_decide<<<(nact + TB - 1) / TB, TB, 0, G.stream>>>(KN, N, S, d_act, nact);
      if (int rc = step("k_sf_decide")) return rc;
      HIPCHK(hipStreamSynchronize(G.stream));
      std::vector<int32_t> h_solve, sa, sm;  // the cells to solve: active position, model cell
      if (d2h_vec(h_solve, S.solve, nact)) return ARTIS_ERR_HIP;
      for (int a = 0; a < nact; a++)
        if (h_solve[a]) {
          sa.push_back(a);
          sm.push_back(act[a]);
        }
      for (size_t q0 = 0; q0 < sa.size(); q0 += sf_batch)
        if (int rc = sf_batch_solve(sa.data() + q0, sm.data() + q0, (int)std::min<size_t>(sf_batch, sa.size() - q0)))
          return rc;
    }
    k_nl_ntrates<<<(nact + TB - 1) / TB, TB, 0, G.stream>>>(KN, N, S, d_act, nact);
    if (int rc = step("k_nl_ntrates")) return rc;
    if (int rc = te_launch(d_act, nact, 1, d_actk)) return rc;
    if (int rc = step("k_te_solve (call_T_e_finder)")) return rc;
    if (int rc = read_fail("call_T_e_finder")) return rc;
    // populations and corrected photoionisation coefficients at the new T_e; the rate matrices
    k_levelpops<<<(unsigned)((nlv + TB - 1) / TB), TB, 0, G.stream>>>(KN);
    if (int rc = step("k_levelpops")) return rc;
    const int64_t nbt = (int64_t)nact * (nbf + ntg);
    if (nbt > 0) k_bfcells<<<(unsigned)((nbt + TB - 1) / TB), TB, 0, G.stream>>>(KN, G.d_target_ul, G.d_target_t);
    if (int rc = step("k_bfcells")) return rc;
    if (ntg > 0)
      k_corrphot_integral<<<(unsigned)std::min<int64_t>((int64_t)nact * ntg, qwaves), 64, 0, G.stream>>>(
          KN, G.d_target_ul, G.d_target_t, ws);
    if (int rc = step("k_corrphot_integral")) return rc;
    k_nl_slpf<<<(unsigned)(((int64_t)nact * ni + TB - 1) / TB), TB, 0, G.stream>>>(KN, N, M, d_act, nact);
    if (int rc = step("k_nl_slpf")) return rc;
    for (int a0 = 0; a0 < nact; a0 += chunk)
      if (int rc = matrix_chunk(iter, a0, std::min(chunk, nact - a0))) return rc;
    if (int rc = read_fail("solve_nlte_pops_element")) return rc;
    std::vector<int32_t> done, act2, actk2;
    if (d2h_vec(done, M.done, nact)) return ARTIS_ERR_HIP;
    for (int a = 0; a < nact; a++) {
      h_iters[act[a]] = iter + 1;
      if (!done[a]) {
        act2.push_back(act[a]);
        actk2.push_back(actk[a]);
      }
    }
    act.swap(act2);
    actk.swap(actk2);
    return 0;
  }

  int iterate() {
    h_iters.assign(np, 0);
    if (nnl == 0) return 0;
    if (int rc = radfield_and_bfheat()) return rc;
    act = nl_list;
    actk.resize(nnl);
    for (int k = 0; k < nnl; k++) actk[k] = k;
    for (int iter = 0; iter <= p->nlteiter && !act.empty(); iter++)
      if (int rc = pass(iter)) return rc;
    return 0;
  }

  // nt_ionization_ratecoeff of every listed cell, the cooling rates of the iterated ones
  int final_rates_and_cooling() {
    if (R.nt_on) {
      k_nl_ntrates<<<(c->ncells + TB - 1) / TB, TB, 0, G.stream>>>(KN, N, S, N.mgi, c->ncells);
      HIPCHK(hipGetLastError());
    }
    if (int rc = step("k_nl_ntrates (final)")) return rc;
    if (int rc = te_launch(d_nl, nnl, 2, nullptr)) return rc;
    if (int rc = step("k_te_solve (cooling)")) return rc;
    HIPCHK(hipEventRecord(G.ev1, G.stream));
    HIPCHK(hipEventSynchronize(G.ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, G.ev2, G.ev1));
    G.last_nlte_ms = ms;
    return read_fail("update_grid_nlte");
  }

  // success: every array back to the caller
  int download() const {
    if (int rc = io.download()) return rc;
    if (c->nlte_iterations)
      for (int k = 0; k < c->ncells; k++) c->nlte_iterations[c->mgi[k]] = h_iters[c->mgi[k]];
    return 0;
  }
};
}  // namespace

extern "C" {
int artis_gpu_update_grid_nlte(const artis_nt_shells *nt, const artis_nlte_params *p, artis_nlte_cells *c) {
  if (!G.initialised) return ARTIS_ERR_NOT_INITIALISED;
  NlCall U(nt, p, c);
  if (int rc = U.validate()) return rc;
  if (c->ncells == 0) return 0;
  HIPCHK(hipEventRecord(G.ev2, G.stream));
  if (int rc = U.read_atoms()) return rc;
  U.split_cells();
  if (int rc = U.upload_cells()) return rc;
  if (int rc = U.wire_views()) return rc;
  if (int rc = U.prepare_and_lte_branch()) return rc;
  if (int rc = U.upload_sf_tables()) return rc;
  if (int rc = U.upload_matrix_layout()) return rc;
  if (int rc = U.iterate()) return rc;
  if (int rc = U.final_rates_and_cooling()) return rc;
  return U.download();
}
double artis_gpu_last_nlte_ms(void) { return G.last_nlte_ms; }
}  // extern "C"
