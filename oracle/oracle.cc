// oracle.cc -- CPU restatement of the reference ARTIS packet-propagation hot path.
//
// TEST INFRASTRUCTURE ONLY.  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load
// liboracle.so, and only as the checker / the reported CPU baseline.  The product path (libartis_gpu.so) never
// links, loads or calls anything here.
//
// PARITY STATUS: "parity unpinned".  The reference cannot be built in this image (every hot-path TU includes
// GSL via sn3d.h:100 and GSL is absent; stand-in headers are not allowed), and its only golden data are md5
// sums of whole-run outputs that need a network-downloaded atomic dataset (tests/*/results_md5_*.txt,
// tests/setup_*.sh:7).  This file is a line-by-line restatement of the reference algorithm, each function
// citing the file:line it follows; it is checked by physics invariants and by exact-answer unit vectors in
// tests/ (see DESIGN.md "Oracle").
//
// Deliberate, documented deviations from the reference (identical in the HIP engine):
//   D1 RNG: per-packet Philox4x32-10 stream (include/artis_rng.h) instead of per-thread GSL ran3
//       (input.cc:1908-1917).  Same draw sites, same draw order within a packet.
//   D2 No relative-1e-4 kappa cache (rpkt.cc:1216-1221): continuum opacity is recomputed at every get_event;
//       the reference reuses a value computed at a frequency up to 1e-4 away.
//   D3 select_continuum_nu (ratecoeff.cc:628-684): the tail integrals of alpha_sp_E from nu_threshold + i*dnu
//       to nu_max are computed as total - head(i), with total and head(i) sums of per-piece 4-point
//       Gauss-Legendre integrals, instead of repeated GSL qag(GK31, epsrel 1e-2) calls; same piece grid, same
//       inversion formula.
//   D4 acounter is recorded for every packet, not only OpenMP thread 0 (rpkt.cc:481-488).
//   D5 The update_packets pass loop with re-sorting (update_packets.cc:249-330) is flattened: each packet is
//       advanced to the end of the timestep in one go.  With D2 there is no per-thread state that can change a
//       packet's history, so the result per packet is identical.
//   D6 do_kpkt: if the cumulative cooling search lands one past the ion's last term because the update_grid
//       total and the summed terms differ in the last bits, the last term is taken (the reference aborts,
//       kpkt.cc:573).
//   D7 In a grey optically thick cell no continuum opacity is evaluated; the reference's update_estimators then
//       adds ffheating / gamma / bfheating terms with the kappa its OpenMP thread computed last for some other
//       packet (rpkt.cc:583, 1166), a per-thread artefact.  Here those terms are zero.
//   D8 (withdrawn in round 3: the Compton / pair-production emissivity estimators of emissivities.cc:14-136 are
//       restated, artis_run_params.comp_est; gamma packets run with do_r_lc = 0.)
//   D9 Virtual packets (vpkt.cc:76-406): when no redder line is left, rlc_emiss_vpkt's line loop ends and the
//       virtual packet moves on to the cell boundary (the reference keeps ldist = 0 < sdist and spins forever);
//       a spectrum bin index that rounds up to the array end is skipped (the reference writes past the array).
//       The observer directions and bin edges are computed once with the host libm (vpkt.cc:863-865, 425-436).
#include <omp.h>

#include <algorithm>
#include <cfloat>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "artis_constants.h"
#include "artis_gpu.h"
#include "artis_qk61.h"
#include "artis_rng.h"

namespace {

// vpkt.cc globals under VPKT_ON: vpkt.txt parameters, observer directions, bin edges, accumulators
struct VpktCfg {
  artis_vpkt_params p;
  std::vector<double> exclude;                // [nspectra]
  std::vector<double> obs;                    // [nobs * 3] (vpkt.cc:863-865)
  std::vector<float> lower_time, delta_t;     // [vmtbins]  vspecpol.lower_time / delta_t are floats (vpkt.cc:15-19)
  std::vector<float> lower_freq, delta_freq;  // [vmnubins] lower_freq_vspec / delta_freq_vspec (vpkt.cc:25-26)
  double dlogt = 0., dlognu = 0.;
  std::vector<int32_t> anumber;               // [nelements]
  artis_vpkt_result *out = nullptr;
};

struct Ctx {
  const artis_atomic_tables *at;
  const artis_geometry *g;
  const artis_cell_state *cs;
  artis_run_params rp;
  double T_step_log;
  int nts = 0;          // globals::nts_global (sn3d.cc:1038)
  double minpop = 1e-30;  // MINPOP of the options file (artis_run_params.minpop)
  std::vector<int32_t> slot_allcont;  // photoionisation target slot -> allcont index (get_bfcontindex)
  const artis_gamma_spectra *gs;  // may be NULL: no pellets / gamma packets in the ensemble
  const VpktCfg *vp = nullptr;    // NULL: VPKT_ON undefined
  bool do_comp_est = false;       // globals::do_comp_est of this timestep (sn3d.cc:539)
  std::vector<double> gam_freq;   // get_gam_freq over allnuc_gamma_line_list (gammapkt.cc:192-211, 702-718)
};

struct Est {
  artis_estimators *e;
  int nelements, maxnions;
};

// per-thread cellhistory (globals.h:174-208) + rpkt continuum-opacity scratch (globals.h:160-170)
struct ThreadCache {
  int cellnumber = -99;
  std::vector<double> pops;               // [nlevels_total]
  std::vector<double> departureratios;    // [nbfcontinua]
  std::vector<double> processrates;       // [nlevels_total * 9], COLDEEXC < 0 => not computed
  std::vector<double> individ_rad_deexc;  // [sum ndowntrans], same offsets as downtrans
  std::vector<double> individ_internal_down_same;
  std::vector<double> individ_internal_up_same;  // [sum nuptrans]
  std::vector<double> corrphotoioncoeff;          // [nphixstargets total]
  std::vector<double> cooling_contrib;            // [ncoolingterms]
  // kappa_rpkt_cont of the current step
  double kap_total = 0, kap_es = 0, kap_ff = 0, kap_bf = 0, kap_ffheating = 0;
  std::vector<double> kappa_bf_sum;            // [nbfcontinua]
  std::vector<double> groundcont_gamma_contr;  // [nbfcontinua_ground]
  std::vector<double> gamma_contr;             // [nbfcontinua] DETAILED_BF_ESTIMATORS_ON (globals.h:165)
  int64_t work[ARTIS_WORK_COUNT] = {0};
};

// ---------------------------------------------------------------------------------------------- accessors
inline int uion(const Ctx &c, int element, int ion) { return c.at->elem_uniqueionoffset[element] + ion; }
inline int ulev(const Ctx &c, int element, int ion, int level) {
  return c.at->ion_uniqueleveloffset[uion(c, element, ion)] + level;
}
inline double epsilon(const Ctx &c, int e, int i, int l) { return c.at->level_epsilon[ulev(c, e, i, l)]; }
inline double stat_weight(const Ctx &c, int e, int i, int l) { return c.at->level_stat_weight[ulev(c, e, i, l)]; }
inline int get_nions(const Ctx &c, int e) { return c.at->elem_nions[e]; }
inline int get_ionstage(const Ctx &c, int e, int i) { return c.at->ion_ionstage[uion(c, e, i)]; }
inline int get_nlevels(const Ctx &c, int e, int i) { return c.at->ion_nlevels[uion(c, e, i)]; }
inline int get_ionisinglevels(const Ctx &c, int e, int i) { return c.at->ion_ionisinglevels[uion(c, e, i)]; }
inline int get_maxrecombininglevel(const Ctx &c, int e, int i) { return c.at->ion_maxrecombininglevel[uion(c, e, i)]; }
// atomic.cc:408-422
inline int get_nphixstargets(const Ctx &c, int e, int i, int l) {
  if (i < get_nions(c, e) - 1 && l < get_ionisinglevels(c, e, i)) return c.at->level_nphixstargets[ulev(c, e, i, l)];
  return 0;
}
inline int get_phixsupperlevel(const Ctx &c, int e, int i, int l, int t) {
  return c.at->phixstarget_levelindex[c.at->level_phixstargets_offset[ulev(c, e, i, l)] + t];
}
inline double get_phixsprobability(const Ctx &c, int e, int i, int l, int t) {
  return c.at->phixstarget_probability[c.at->level_phixstargets_offset[ulev(c, e, i, l)] + t];
}
// atomic.cc:437-453
inline double get_phixs_threshold(const Ctx &c, int e, int i, int l, int t) {
  return epsilon(c, e, i + 1, get_phixsupperlevel(c, e, i, l, t)) - epsilon(c, e, i, l);
}
inline const float *level_photoion_xs(const Ctx &c, int e, int i, int l) {
  return c.at->phixs_xs + (size_t)c.at->level_phixstable[ulev(c, e, i, l)] * c.at->nphixspoints;
}
// sn3d.h:64-69
inline int get_bflutindex(const Ctx &c, int tempindex, int e, int i, int l, int t) {
  const int contindex = -1 - c.at->level_cont_index[ulev(c, e, i, l)] + t;
  return tempindex * c.at->nbfcontinua + contindex;
}
// atomic.cc:16-30
inline int get_continuumindex(const Ctx &c, int e, int i, int l, int upperionlevel) {
  int target = -1;
  for (int t = 0; t < get_nphixstargets(c, e, i, l); t++)
    if (get_phixsupperlevel(c, e, i, l, t) == upperionlevel) {
      target = t;
      break;
    }
  if (target < 0) {
    fprintf(stderr, "oracle: Could not find phixstargetindex\n");
    abort();
  }
  return c.at->level_cont_index[ulev(c, e, i, l)] - target;
}

inline int cell_mgi(const Ctx &c, int cellindex) { return c.g->cell_mgi[cellindex]; }
inline int npts_model(const Ctx &c) { return c.g->npts_model; }

// ------------------------------------------------------------------------------------------------ vectors
// vectors.h:15-75
inline double vec_len(const double x[3]) { return std::sqrt((x[0] * x[0]) + (x[1] * x[1]) + (x[2] * x[2])); }
inline void vec_norm(const double in[3], double out[3]) {
  const double mag = vec_len(in);
  out[0] = in[0] / mag;
  out[1] = in[1] / mag;
  out[2] = in[2] / mag;
}
inline double dot(const double x[3], const double y[3]) { return (x[0] * y[0]) + (x[1] * y[1]) + (x[2] * y[2]); }
inline void get_velocity(const double x[3], double y[3], double t) {
  y[0] = x[0] / t;
  y[1] = x[1] / t;
  y[2] = x[2] / t;
}
inline void cross_prod(const double v1[3], const double v2[3], double out[3]) {
  out[0] = (v1[1] * v2[2]) - (v2[1] * v1[2]);
  out[1] = (v1[2] * v2[0]) - (v2[2] * v1[0]);
  out[2] = (v1[0] * v2[1]) - (v2[0] * v1[1]);
}
inline void vec_scale(double v[3], double s) {
  v[0] *= s;
  v[1] *= s;
  v[2] *= s;
}
inline void vec_copy(double d[3], const double s[3]) {
  d[0] = s[0];
  d[1] = s[1];
  d[2] = s[2];
}
// vectors.h:63-79
inline void angle_ab(const double dir1[3], const double vel[3], double dir2[3]) {
  const double vsqr = dot(vel, vel) / ARTIS_CLIGHTSQUARED;
  const double gamma_rel = 1. / std::sqrt(1 - vsqr);
  const double ndotv = dot(dir1, vel);
  const double fact1 = gamma_rel * (1 - (ndotv / ARTIS_CLIGHT));
  const double fact2 = (gamma_rel - (gamma_rel * gamma_rel * ndotv / (gamma_rel + 1) / ARTIS_CLIGHT)) / ARTIS_CLIGHT;
  for (int d = 0; d < 3; d++) dir2[d] = (dir1[d] - (vel[d] * fact2)) / fact1;
}
// vectors.h:81-105
inline double doppler_nucmf_on_nurf(const Ctx &c, const double dir_rf[3], const double vel_rf[3]) {
  const double ndotv = dot(dir_rf, vel_rf);
  double dopplerfactor = 1. - (ndotv / ARTIS_CLIGHT);
  if (c.rp.relativistic_doppler) {
    const double betasq = dot(vel_rf, vel_rf) / ARTIS_CLIGHTSQUARED;
    dopplerfactor = dopplerfactor / std::sqrt(1 - betasq);
  }
  return dopplerfactor;
}
inline double doppler_packet_nucmf_on_nurf(const Ctx &c, const artis_packet *p) {
  double v[3] = {0, 0, 0};
  get_velocity(p->pos, v, p->prop_time);
  return doppler_nucmf_on_nurf(c, p->dir, v);
}
// vectors.h:113-144
inline void move_pkt(const Ctx &c, artis_packet *p, double distance) {
  p->pos[0] += (p->dir[0] * distance);
  p->pos[1] += (p->dir[1] * distance);
  p->pos[2] += (p->dir[2] * distance);
  const double dopplerfactor = doppler_packet_nucmf_on_nurf(c, p);
  p->nu_cmf = p->nu_rf * dopplerfactor;
  p->e_cmf = p->e_rf * dopplerfactor;
}
inline void move_pkt_withtime(const Ctx &c, artis_packet *p, double distance) {
  const double nu_cmf_old = p->nu_cmf;
  p->prop_time += distance / ARTIS_CLIGHT_PROP;
  move_pkt(c, p, distance);
  if (p->nu_cmf > nu_cmf_old) p->nu_cmf = nu_cmf_old;
}
// vectors.cc:43-58
inline void get_rand_isotropic_unitvec(artis_rng *rng, double out[3]) {
  const double zrand = artis_rng_uniform(rng);
  const double zrand2 = artis_rng_uniform(rng);
  const double mu = -1 + (2. * zrand);
  const double phi = zrand2 * 2 * ARTIS_PI;
  const double sintheta = std::sqrt(1. - (mu * mu));
  out[0] = sintheta * std::cos(phi);
  out[1] = sintheta * std::sin(phi);
  out[2] = mu;
}

// ------------------------------------------------------------------------------------------ populations
// ltepop.cc:307-327
double get_groundlevelpop(const Ctx &c, int mgi, int e, int i) {
  const double nn = c.cs->groundlevelpop[(size_t)mgi * c.at->nions_total + uion(c, e, i)];
  if (nn < c.minpop) {
    if (c.cs->elem_abundance[(size_t)mgi * c.at->nelements + e] > 0) return c.minpop;
    return 0.;
  }
  return nn;
}
// LTEPOP_EXCITATIONTEMPERATURE (ltepop.cc:338): T_J in artisoptions_classic.h:32, T_e in
// artisoptions_kilonova_lte.h:36 / artisoptions_nltenebular.h:36 (grid::get_Te / get_TJ return float)
inline double excitation_temperature(const Ctx &c, int mgi) {
  return (c.rp.excitation_temperature == ARTIS_TEXC_TE) ? c.cs->Te[mgi] : c.cs->TJ[mgi];
}
// ltepop.cc:329-347
double calculate_levelpop_lte(const Ctx &c, int mgi, int e, int i, int l) {
  if (l == 0) return get_groundlevelpop(c, mgi, e, i);
  const double T_exc = excitation_temperature(c, mgi);
  const double W = 1.;
  const double E_level = epsilon(c, e, i, l);
  const double E_ground = epsilon(c, e, i, 0);
  const double nnground = get_groundlevelpop(c, mgi, e, i);
  return (nnground * W * stat_weight(c, e, i, l) / stat_weight(c, e, i, 0) *
          exp(-(E_level - E_ground) / ARTIS_KB / T_exc));
}
// atomic.cc:235-241, 69-85, 367-371 with LEVEL_IS_NLTE contiguous from the ground state
// (artisoptions_nltenebular.h:26-34): levels 1..nlevels_nlte are NLTE, the rest of the excited levels form the
// superlevel
inline int get_nlevels_nlte(const Ctx &c, int e, int i) { return c.at->ion_nlevels_nlte[uion(c, e, i)]; }
inline bool is_nlte(const Ctx &c, int e, int i, int l) { return c.rp.nlte_pops_on && l <= get_nlevels_nlte(c, e, i); }
// nltepop.cc:1543-1554
double superlevel_boltzmann(const Ctx &c, int mgi, int e, int i, int l) {
  const int superlevel_index = get_nlevels_nlte(c, e, i) + 1;
  const double T_exc = excitation_temperature(c, mgi);
  const double E_level = epsilon(c, e, i, l);
  const double E_superlevel = epsilon(c, e, i, superlevel_index);
  return stat_weight(c, e, i, l) / stat_weight(c, e, i, superlevel_index) * exp(-(E_level - E_superlevel) / ARTIS_KB / T_exc);
}
// ltepop.cc:349-415
double calculate_levelpop_nominpop(const Ctx &c, int mgi, int e, int i, int l, bool *skipminpop) {
  double nn;
  if (l == 0) {
    nn = get_groundlevelpop(c, mgi, e, i);
  } else if (c.rp.nlte_pops_on) {
    const size_t base = (size_t)mgi * c.at->total_nlte_levels + c.at->ion_first_nlte[uion(c, e, i)];
    if (is_nlte(c, e, i, l)) {
      const double nltepop_over_rho = c.cs->nlte_pops[base + l - 1];
      if (nltepop_over_rho < -0.9) {
        nn = calculate_levelpop_lte(c, mgi, e, i, l);
      } else {
        nn = nltepop_over_rho * c.cs->rho[mgi];
        if (!std::isfinite(nn)) {
          fprintf(stderr, "oracle: [fatal] NLTE population failure\n");
          abort();
        }
        *skipminpop = true;
        return nn;
      }
    } else {
      const double superlevelpop_over_rho = c.cs->nlte_pops[base + get_nlevels_nlte(c, e, i)];
      if (superlevelpop_over_rho < -0.9) {
        nn = calculate_levelpop_lte(c, mgi, e, i, l);
      } else {
        nn = superlevelpop_over_rho * c.cs->rho[mgi] * superlevel_boltzmann(c, mgi, e, i, l);
        if (!std::isfinite(nn)) {
          fprintf(stderr, "oracle: [fatal] NLTE population failure\n");
          abort();
        }
        *skipminpop = true;
        return nn;
      }
    }
  } else {
    nn = calculate_levelpop_lte(c, mgi, e, i, l);
  }
  *skipminpop = false;
  return nn;
}
// ltepop.cc:417-430
double calculate_levelpop(const Ctx &c, int mgi, int e, int i, int l) {
  bool skipminpop = false;
  double nn = calculate_levelpop_nominpop(c, mgi, e, i, l, &skipminpop);
  if (!skipminpop && nn < c.minpop) {
    if (c.cs->elem_abundance[(size_t)mgi * c.at->nelements + e] > 0)
      nn = c.minpop;
    else
      nn = 0.;
  }
  return nn;
}
// ltepop.cc:558-564
double ionstagepop(const Ctx &c, int mgi, int e, int i) {
  return get_groundlevelpop(c, mgi, e, i) * c.cs->partfunct[(size_t)mgi * c.at->nions_total + uion(c, e, i)] /
         stat_weight(c, e, i, 0);
}
// ltepop.cc:539-556
double calculate_sahafact(const Ctx &c, int e, int i, int l, int upperionlevel, double T, double E_threshold) {
  const double g_lower = stat_weight(c, e, i, l);
  const double g_upper = stat_weight(c, e, i + 1, upperionlevel);
  return ARTIS_SAHACONST * g_lower / g_upper * pow(T, -1.5) * exp(E_threshold / ARTIS_KB / T);
}

// update_grid.cc:659-761 cellhistory_reset
void cellhistory_reset(const Ctx &c, ThreadCache &tc, int mgi) {
  if (tc.cellnumber == mgi) return;
  tc.cellnumber = mgi;
  const artis_atomic_tables &a = *c.at;
  for (int e = 0; e < a.nelements; e++)
    for (int i = 0; i < get_nions(c, e); i++)
      for (int l = 0; l < get_nlevels(c, e, i); l++) tc.pops[ulev(c, e, i, l)] = calculate_levelpop(c, mgi, e, i, l);
  std::fill(tc.departureratios.begin(), tc.departureratios.end(), -1.);
  for (int lv = 0; lv < a.nlevels_total; lv++) tc.processrates[(size_t)lv * 9 + ARTIS_MA_ACTION_COLDEEXC] = -99.;
  std::fill(tc.corrphotoioncoeff.begin(), tc.corrphotoioncoeff.end(), -99.);
  std::fill(tc.cooling_contrib.begin(), tc.cooling_contrib.end(), -99.);
}
inline double get_levelpop(const ThreadCache &tc, const Ctx &c, int e, int i, int l) { return tc.pops[ulev(c, e, i, l)]; }

// ------------------------------------------------------------------------------------------- radfield
inline double dbb(double nu, double T, double W) {
  return W * ARTIS_TWOHOVERCLIGHTSQUARED * pow(nu, 3) / expm1(ARTIS_HOVERKB * nu / T);  // radfield.h:44-48
}
// radfield.cc:575-600 select_bin: -2 below the first bin, -1 above the last
int select_bin(const Ctx &c, double nu) {
  if (nu < c.at->radfield_nu_lower_first) return -2;
  const double *up = c.at->radfield_nu_upper;
  const int binindex = (int)(std::upper_bound(up, up + c.at->radfield_nbins, nu) - up);
  if (binindex >= c.at->radfield_nbins) return -1;
  return binindex;
}
// radfield.cc:898-943: J_nu of the fitted dilute blackbody of the bin from FIRST_NLTE_RADFIELD_TIMESTEP on
// (MULTIBIN_RADFIELD_MODEL_ON), the full-spectrum dilute blackbody otherwise
inline double radfield(const Ctx &c, double nu, int mgi) {
  if (c.rp.multibin_radfield && c.nts >= c.rp.first_nlte_radfield_timestep) {
    const int binindex = select_bin(c, nu);
    if (binindex >= 0) {
      const size_t mb = (size_t)mgi * c.at->radfield_nbins + binindex;
      const float W = c.cs->radfield_bin_W[mb];
      if (W >= 0.) return dbb(nu, c.cs->radfield_bin_TR[mb], W);
    }
    return 0.;
  }
  const float T_R = c.cs->TR[mgi];
  const float W = c.cs->W[mgi];
  return dbb(nu, T_R, W);
}

// ------------------------------------------------------------------------------------------ photoionisation
// atomic.cc:87-155
double photoionization_crosssection_fromtable(const Ctx &c, const float *xs, double nu_edge, double nu) {
  float sigma_bf;
  const artis_atomic_tables &a = *c.at;
  if (a.phixs_file_version == 1) {
    if (nu == nu_edge) {
      sigma_bf = xs[0];
    } else if (nu <= nu_edge * (1 + a.nphixsnuincrement * a.nphixspoints)) {
      const int i = (int)floor(nu / (a.nphixsnuincrement * nu_edge)) - 10;
      sigma_bf = xs[i];
    } else {
      sigma_bf = xs[a.nphixspoints - 1] * pow(nu_edge * (1 + a.nphixsnuincrement * a.nphixspoints) / nu, 3);
    }
    return sigma_bf;
  }
  const double ireal = (nu / nu_edge - 1.0) / a.nphixsnuincrement;
  const int i = (int)floor(ireal);
  if (i < 0) {
    sigma_bf = 0.0;
  } else if (i < a.nphixspoints - 1) {
    const double sigma_bf_a = xs[i];
    const double sigma_bf_b = xs[i + 1];
    const double factor_b = ireal - i;
    sigma_bf = ((1. - factor_b) * sigma_bf_a) + (factor_b * sigma_bf_b);
  } else {
    const double nu_max_phixs = nu_edge * a.last_phixs_nuovernuedge;
    sigma_bf = xs[a.nphixspoints - 1] * pow(nu_max_phixs / nu, 3);
  }
  return sigma_bf;
}

// ratecoeff.cc:686-710
double get_spontrecombcoeff(const Ctx &c, int e, int i, int l, int t, float T_e) {
  const int tablesize = c.at->tablesize;
  const int lowerindex = (int)floor(log(T_e / c.at->mintemp) / c.T_step_log);
  if (lowerindex < tablesize - 1) {
    const int upperindex = lowerindex + 1;
    const double T_lower = c.at->mintemp * exp(lowerindex * c.T_step_log);
    const double T_upper = c.at->mintemp * exp(upperindex * c.T_step_log);
    const double f_upper = c.at->spontrecombcoeff[get_bflutindex(c, upperindex, e, i, l, t)];
    const double f_lower = c.at->spontrecombcoeff[get_bflutindex(c, lowerindex, e, i, l, t)];
    return (f_lower + (f_upper - f_lower) / (T_upper - T_lower) * (T_e - T_lower));
  }
  return c.at->spontrecombcoeff[get_bflutindex(c, tablesize - 1, e, i, l, t)];
}
// ratecoeff.cc:1026-1041
double interpolate_corrphotoioncoeff(const Ctx &c, int e, int i, int l, int t, double T) {
  const int tablesize = c.at->tablesize;
  const int lowerindex = (int)floor(log(T / c.at->mintemp) / c.T_step_log);
  if (lowerindex < tablesize - 1) {
    const int upperindex = lowerindex + 1;
    const double T_lower = c.at->mintemp * exp(lowerindex * c.T_step_log);
    const double T_upper = c.at->mintemp * exp(upperindex * c.T_step_log);
    const double f_upper = c.at->corrphotoioncoeff[get_bflutindex(c, upperindex, e, i, l, t)];
    const double f_lower = c.at->corrphotoioncoeff[get_bflutindex(c, lowerindex, e, i, l, t)];
    return (f_lower + (f_upper - f_lower) / (T_upper - T_lower) * (T - T_lower));
  }
  return c.at->corrphotoioncoeff[get_bflutindex(c, tablesize - 1, e, i, l, t)];
}
// ---- gsl_integration_qag with GSL_INTEG_GAUSS61 (GSL 2.x integration/qag.c, qk.c, qk61.c, qpsrt.c, util.c,
// err.c), the quadrature calculate_corrphotoioncoeff_integral hands its integrand to (ratecoeff.cc:1225-1226).
// GSL is a dependency the reference links and this image lacks; this is its published algorithm: the 61-point
// Gauss-Kronrod rule (include/artis_qk61.h, generated by tools/gen_qk61.py) and adaptive bisection of the
// interval with the largest error estimate, the error list kept ordered by qpsrt.
constexpr double kGslDblEpsilon = 2.2204460492503131e-16;
constexpr double kGslDblMin = 2.2250738585072014e-308;
const double qk61_xgk[31] = ARTIS_QK61_XGK;
const double qk61_wg[15] = ARTIS_QK61_WG;
const double qk61_wgk[31] = ARTIS_QK61_WGK;

double gsl_rescale_error(double err, const double result_abs, const double result_asc) {
  err = fabs(err);
  if (result_asc != 0 && err != 0) {
    const double scale = pow((200 * err / result_asc), 1.5);
    if (scale < 1)
      err = result_asc * scale;
    else
      err = result_asc;
  }
  if (result_abs > 2 * kGslDblMin / (50 * kGslDblEpsilon)) {
    const double min_err = 50 * kGslDblEpsilon * result_abs;
    if (min_err > err) err = min_err;
  }
  return err;
}

template <typename F>
void gsl_qk61(const F &f, double a, double b, double *result, double *abserr, double *resabs, double *resasc) {
  const int n = 31;
  double fv1[31], fv2[31];
  const double center = 0.5 * (a + b);
  const double half_length = 0.5 * (b - a);
  const double abs_half_length = fabs(half_length);
  const double f_center = f(center);
  double result_gauss = 0;
  double result_kronrod = f_center * qk61_wgk[n - 1];
  double result_abs = fabs(result_kronrod);
  double result_asc = 0;
  for (int j = 0; j < (n - 1) / 2; j++) {
    const int jtw = j * 2 + 1;
    const double abscissa = half_length * qk61_xgk[jtw];
    const double fval1 = f(center - abscissa);
    const double fval2 = f(center + abscissa);
    const double fsum = fval1 + fval2;
    fv1[jtw] = fval1;
    fv2[jtw] = fval2;
    result_gauss += qk61_wg[j] * fsum;
    result_kronrod += qk61_wgk[jtw] * fsum;
    result_abs += qk61_wgk[jtw] * (fabs(fval1) + fabs(fval2));
  }
  for (int j = 0; j < n / 2; j++) {
    const int jtwm1 = j * 2;
    const double abscissa = half_length * qk61_xgk[jtwm1];
    const double fval1 = f(center - abscissa);
    const double fval2 = f(center + abscissa);
    fv1[jtwm1] = fval1;
    fv2[jtwm1] = fval2;
    result_kronrod += qk61_wgk[jtwm1] * (fval1 + fval2);
    result_abs += qk61_wgk[jtwm1] * (fabs(fval1) + fabs(fval2));
  }
  const double mean = result_kronrod * 0.5;
  result_asc = qk61_wgk[n - 1] * fabs(f_center - mean);
  for (int j = 0; j < n - 1; j++) result_asc += qk61_wgk[j] * (fabs(fv1[j] - mean) + fabs(fv2[j] - mean));
  const double err = (result_kronrod - result_gauss) * half_length;
  result_kronrod *= half_length;
  result_abs *= abs_half_length;
  result_asc *= abs_half_length;
  *result = result_kronrod;
  *resabs = result_abs;
  *resasc = result_asc;
  *abserr = gsl_rescale_error(err, result_abs, result_asc);
}

struct GslWorkspace {
  size_t limit = 0, size = 0, nrmax = 0, i = 0, maximum_level = 0;
  std::vector<double> alist, blist, rlist, elist;
  std::vector<size_t> order, level;
  explicit GslWorkspace(size_t n) : limit(n), alist(n), blist(n), rlist(n), elist(n), order(n), level(n) {}
};

void gsl_qpsrt(GslWorkspace &w) {
  const size_t last = w.size - 1;
  const size_t limit = w.limit;
  double *elist = w.elist.data();
  size_t *order = w.order.data();
  size_t i_nrmax = w.nrmax;
  size_t i_maxerr = order[i_nrmax];
  if (last < 2) {
    order[0] = 0;
    order[1] = 1;
    w.i = i_maxerr;
    return;
  }
  const double errmax = elist[i_maxerr];
  while (i_nrmax > 0 && errmax > elist[order[i_nrmax - 1]]) {
    order[i_nrmax] = order[i_nrmax - 1];
    i_nrmax--;
  }
  int top;
  if (last < (limit / 2 + 2))
    top = (int)last;
  else
    top = (int)(limit - last + 1);
  int i = (int)i_nrmax + 1;
  while (i < top && errmax < elist[order[i]]) {
    order[i - 1] = order[i];
    i++;
  }
  order[i - 1] = i_maxerr;
  const double errmin = elist[last];
  int k = top - 1;
  while (k > i - 2 && errmin >= elist[order[k]]) {
    order[k + 1] = order[k];
    k--;
  }
  order[k + 1] = last;
  i_maxerr = order[i_nrmax];
  w.i = i_maxerr;
  w.nrmax = i_nrmax;
}

void gsl_ws_update(GslWorkspace &w, double a1, double b1, double area1, double error1, double a2, double b2,
                   double area2, double error2) {
  const size_t i_max = w.i;
  const size_t i_new = w.size;
  const size_t new_level = w.level[i_max] + 1;
  if (error2 > error1) {
    w.alist[i_max] = a2;
    w.rlist[i_max] = area2;
    w.elist[i_max] = error2;
    w.level[i_max] = new_level;
    w.alist[i_new] = a1;
    w.blist[i_new] = b1;
    w.rlist[i_new] = area1;
    w.elist[i_new] = error1;
    w.level[i_new] = new_level;
  } else {
    w.blist[i_max] = b1;
    w.rlist[i_max] = area1;
    w.elist[i_max] = error1;
    w.level[i_max] = new_level;
    w.alist[i_new] = a2;
    w.blist[i_new] = b2;
    w.rlist[i_new] = area2;
    w.elist[i_new] = error2;
    w.level[i_new] = new_level;
  }
  w.size++;
  if (new_level > w.maximum_level) w.maximum_level = new_level;
  gsl_qpsrt(w);
}

// returns the GSL status (0, GSL_EROUND 18, GSL_ESING 21, GSL_EMAXITER 11, GSL_EFAILED 5)
template <typename F>
int gsl_qag61(const F &f, double a, double b, double epsabs, double epsrel, size_t limit, GslWorkspace &w,
              double *result, double *abserr) {
  w.size = 0;
  w.nrmax = 0;
  w.i = 0;
  w.alist[0] = a;
  w.blist[0] = b;
  w.rlist[0] = 0.0;
  w.elist[0] = 0.0;
  w.order[0] = 0;
  w.level[0] = 0;
  w.maximum_level = 0;
  *result = 0;
  *abserr = 0;
  double result0, abserr0, resabs0, resasc0;
  gsl_qk61(f, a, b, &result0, &abserr0, &resabs0, &resasc0);
  w.size = 1;
  w.rlist[0] = result0;
  w.elist[0] = abserr0;
  double tolerance = std::max(epsabs, epsrel * fabs(result0));
  const double round_off = 50 * kGslDblEpsilon * resabs0;
  if (abserr0 <= round_off && abserr0 > tolerance) {
    *result = result0;
    *abserr = abserr0;
    return 18;
  } else if ((abserr0 <= tolerance && abserr0 != resasc0) || abserr0 == 0.0) {
    *result = result0;
    *abserr = abserr0;
    return 0;
  } else if (limit == 1) {
    *result = result0;
    *abserr = abserr0;
    return 11;
  }
  double area = result0;
  double errsum = abserr0;
  size_t iteration = 1;
  int roundoff_type1 = 0, roundoff_type2 = 0, error_type = 0;
  do {
    const size_t ii = w.i;
    const double a_i = w.alist[ii], b_i = w.blist[ii], r_i = w.rlist[ii], e_i = w.elist[ii];
    const double a1 = a_i;
    const double b1 = 0.5 * (a_i + b_i);
    const double a2 = b1;
    const double b2 = b_i;
    double area1 = 0, area2 = 0, error1 = 0, error2 = 0, resasc1, resasc2, resabs1, resabs2;
    gsl_qk61(f, a1, b1, &area1, &error1, &resabs1, &resasc1);
    gsl_qk61(f, a2, b2, &area2, &error2, &resabs2, &resasc2);
    const double area12 = area1 + area2;
    const double error12 = error1 + error2;
    errsum += (error12 - e_i);
    area += area12 - r_i;
    if (resasc1 != error1 && resasc2 != error2) {
      const double delta = r_i - area12;
      if (fabs(delta) <= 1.0e-5 * fabs(area12) && error12 >= 0.99 * e_i) roundoff_type1++;
      if (iteration >= 10 && error12 > e_i) roundoff_type2++;
    }
    tolerance = std::max(epsabs, epsrel * fabs(area));
    if (errsum > tolerance) {
      if (roundoff_type1 >= 6 || roundoff_type2 >= 20) error_type = 2;
      const double tmp = (1 + 100 * kGslDblEpsilon) * (fabs(a2) + 1000 * kGslDblMin);
      if (fabs(a1) <= tmp && fabs(b2) <= tmp) error_type = 3;
    }
    gsl_ws_update(w, a1, b1, area1, error1, a2, b2, area2, error2);
    iteration++;
  } while (iteration < limit && !error_type && errsum > tolerance);
  double result_sum = 0;
  for (size_t k = 0; k < w.size; k++) result_sum += w.rlist[k];
  *result = result_sum;
  *abserr = errsum;
  if (errsum <= tolerance) return 0;
  if (error_type == 2) return 18;
  if (error_type == 3) return 21;
  if (iteration == limit) return 11;
  return 5;
}

constexpr size_t kGslWsSize = 16384;  // GSLWSIZE (artisoptions_nltenebular.h:75)

// ratecoeff.cc:1159-1245 calculate_corrphotoioncoeff_integral (NO_LUT_PHOTOION)
// epsrel: the reference's 1e-3 (ratecoeff.cc:1199); the tests also call it at a tight tolerance
double calculate_corrphotoioncoeff_integral(const Ctx &c, const ThreadCache &tc, int e, int i, int l, int t, int mgi,
                                            double epsrel = 1e-3) {
  constexpr double epsabs = 0.;
  const double E_threshold = get_phixs_threshold(c, e, i, l, t);
  const double nu_threshold = ARTIS_ONEOVERH * E_threshold;
  const double nu_max_phixs = nu_threshold * c.at->last_phixs_nuovernuedge;
  const float T_e = c.cs->Te[mgi];
  const double nnlevel = get_levelpop(tc, c, e, i, l);
  const double nne = c.cs->nne[mgi];
  const int upperionlevel = get_phixsupperlevel(c, e, i, l, t);
  const double sf = calculate_sahafact(c, e, i, l, upperionlevel, T_e, ARTIS_H * nu_threshold);
  const double nnupperionlevel = get_levelpop(tc, c, e, i + 1, upperionlevel);
  double departure_ratio = nnlevel > 0. ? nnupperionlevel / nnlevel * nne * sf : 1.0;
  if (!std::isfinite(departure_ratio)) departure_ratio = 0.;
  const float *xs = level_photoion_xs(c, e, i, l);
  // integrand_corrphotoioncoeff_custom_radfield (ratecoeff.cc:1159-1181)
  auto integrand = [&](double nu) {
    double corrfactor = 1. - departure_ratio * exp(-ARTIS_HOVERKB * nu / T_e);
    if (corrfactor < 0) corrfactor = 0.;
    const float sigma_bf = (float)photoionization_crosssection_fromtable(c, xs, nu_threshold, nu);
    const double Jnu = radfield(c, nu, mgi);
    return ARTIS_ONEOVERH * sigma_bf / nu * Jnu * corrfactor;
  };
  static thread_local GslWorkspace ws(kGslWsSize);
  double gammacorr = 0.0, error = 0.0;
  const int status = gsl_qag61(integrand, nu_threshold, nu_max_phixs, epsabs, epsrel, kGslWsSize, ws, &gammacorr, &error);
  if (status != 0 && (status != 18 || (error / gammacorr) > 1e-1)) {
    if (!std::isfinite(gammacorr)) gammacorr = 0.;
  }
  gammacorr *= ARTIS_FOURPI * get_phixsprobability(c, e, i, l, t);
  return gammacorr;
}

// ratecoeff.cc:1247-1308 (cached per thread like cellhistory chphixstargets): the previous timestep's bf-rate
// estimator when DETAILED_BF_ESTIMATORS_ON from DETAILED_BF_ESTIMATORS_USEFROMTIMESTEP (radfield.cc:1440-1455,
// get_bfcontindex radfield.cc:1329-1341), else the integral (NO_LUT_PHOTOION) or W * LUT * renormalisation
double get_corrphotoioncoeff(const Ctx &c, ThreadCache &tc, int e, int i, int l, int t, int mgi) {
  const int slot = c.at->level_phixstargets_offset[ulev(c, e, i, l)] + t;
  if (c.rp.detailed_bf_estimators && c.nts >= c.rp.detailed_bf_usefromtimestep) {
    const int allcontindex = c.slot_allcont[slot];
    if (allcontindex >= 0) {
      const double gammacorr = c.cs->bfrate_estimator[(size_t)mgi * c.at->nbfcontinua + allcontindex];
      if (gammacorr > 0) return gammacorr;
    }
  }
  double gammacorr = tc.corrphotoioncoeff[slot];
  if (gammacorr < 0) {
    if (c.rp.no_lut_photoion) {
      gammacorr = calculate_corrphotoioncoeff_integral(c, tc, e, i, l, t, mgi);
    } else {
      const double W = c.cs->W[mgi];
      const double T_R = c.cs->TR[mgi];
      gammacorr = W * interpolate_corrphotoioncoeff(c, e, i, l, t, T_R);
      const int index_in_groundlevelcontestimator = c.at->level_closestgroundlevelcont[ulev(c, e, i, l)];
      if (index_in_groundlevelcontestimator >= 0)
        gammacorr *= c.cs->corrphotoionrenorm[(size_t)mgi * c.at->nelements * c.at->maxnions +
                                              index_in_groundlevelcontestimator];
    }
    tc.corrphotoioncoeff[slot] = gammacorr;
  }
  return gammacorr;
}
// kpkt.cc:69-82
double get_bfcoolingcoeff(const Ctx &c, int e, int i, int l, int t, float T_e) {
  const int tablesize = c.at->tablesize;
  const int lowerindex = (int)floor(log(T_e / c.at->mintemp) / c.T_step_log);
  if (lowerindex < tablesize - 1) {
    const int upperindex = lowerindex + 1;
    const double T_lower = c.at->mintemp * exp(lowerindex * c.T_step_log);
    const double T_upper = c.at->mintemp * exp(upperindex * c.T_step_log);
    const double f_upper = c.at->bfcooling_coeff[get_bflutindex(c, upperindex, e, i, l, t)];
    const double f_lower = c.at->bfcooling_coeff[get_bflutindex(c, lowerindex, e, i, l, t)];
    return (f_lower + (f_upper - f_lower) / (T_upper - T_lower) * (T_e - T_lower));
  }
  return c.at->bfcooling_coeff[get_bflutindex(c, tablesize - 1, e, i, l, t)];
}

// ratecoeff.cc:263-279 alpha_sp_E_integrand_gsl
inline double alpha_sp_E_integrand(const Ctx &c, const float *xs, double nu_edge, float T, double nu) {
  const float sigma_bf = (float)photoionization_crosssection_fromtable(c, xs, nu_edge, nu);
  return ARTIS_TWOOVERCLIGHTSQUARED * sigma_bf * pow(nu, 3) / nu_edge * exp(-ARTIS_HOVERKB * nu / T);
}
// ratecoeff.cc:628-684 select_continuum_nu, with deviation D3 (piecewise Gauss-Legendre tail integrals)
double select_continuum_nu(const Ctx &c, artis_rng *rng, int e, int lowerion, int lower, int upperionlevel,
                           float T_e) {
  int target = -1;
  for (int t = 0; t < get_nphixstargets(c, e, lowerion, lower); t++)
    if (get_phixsupperlevel(c, e, lowerion, lower, t) == upperionlevel) {
      target = t;
      break;
    }
  const double E_threshold = get_phixs_threshold(c, e, lowerion, lower, target);
  const double nu_threshold = ARTIS_ONEOVERH * E_threshold;
  const double nu_max_phixs = nu_threshold * c.at->last_phixs_nuovernuedge;
  const int npieces = c.at->nphixspoints;
  const float *xs = level_photoion_xs(c, e, lowerion, lower);
  const double zrand = 1. - artis_rng_uniform(rng);
  const double deltanu = (nu_max_phixs - nu_threshold) / npieces;
  // piece integrals, 4-point Gauss-Legendre; tail(i) = total - head(i), heads summed bottom-up
  static const double gx[4] = {-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526};
  static const double gw[4] = {0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538};
  const double half = 0.5 * deltanu;
  auto piece = [&](double a) {
    const double mid = a + half;
    double s = 0.;
    for (int q = 0; q < 4; q++) s += gw[q] * alpha_sp_E_integrand(c, xs, nu_threshold, T_e, mid + half * gx[q]);
    return s * half;
  };
  double head = 0.;
  for (int j = 0; j < npieces; j++) head += piece(nu_threshold + j * deltanu);
  const double total_alpha_sp = head;
  double alpha_sp_old = total_alpha_sp;
  double alpha_sp = total_alpha_sp;
  head = 0.;
  int i;
  for (i = 1; i < npieces; i++) {
    alpha_sp_old = alpha_sp;
    head += piece(nu_threshold + (i - 1) * deltanu);
    alpha_sp = total_alpha_sp - head;
    if (zrand >= alpha_sp / total_alpha_sp) break;
  }
  const double nuoffset = (total_alpha_sp * zrand - alpha_sp_old) / (alpha_sp - alpha_sp_old) * deltanu;
  return nu_threshold + (i - 1) * deltanu + nuoffset;
}

// -------------------------------------------------------------------------------------------- rate coeffs
// macroatom.h:52-105
double col_deexcitation_ratecoeff(const Ctx &c, float T_e, float nne, double epsilon_trans, int li, double lowerstatweight,
                                  double upperstatweight) {
  double C = 0.;
  const double coll_str_thisline = c.at->line_coll_str[li];
  if (coll_str_thisline < 0) {
    if (!c.at->line_forbidden[li]) {
      const double eoverkt = epsilon_trans / (ARTIS_KB * T_e);
      const double g_bar = 0.2;
      const double gauntfac =
          (eoverkt > 0.33421) ? g_bar : 0.276 * std::exp(eoverkt) * (-0.5772156649 - std::log(eoverkt));
      const double g_ratio = lowerstatweight / upperstatweight;
      C = ARTIS_C_0 * 14.51039491 * nne * std::sqrt(T_e) * c.at->line_osc_strength[li] *
          std::pow(ARTIS_H_IONPOT / epsilon_trans, 2) * eoverkt * g_ratio * gauntfac;
    } else {
      C = nne * 8.629e-6 * 0.01 * lowerstatweight / std::sqrt(T_e);
    }
  } else {
    C = nne * 8.629e-6 * coll_str_thisline / upperstatweight / std::sqrt(T_e);
  }
  return C;
}
// macroatom.h:107-150
double col_excitation_ratecoeff(const Ctx &c, float T_e, float nne, int li, double epsilon_trans, double lowerstatweight,
                                double upperstatweight) {
  double C = 0.;
  const double coll_strength = c.at->line_coll_str[li];
  const double eoverkt = epsilon_trans / (ARTIS_KB * T_e);
  if (coll_strength < 0) {
    if (!c.at->line_forbidden[li]) {
      const double g_bar = 0.2;
      const double exp_eoverkt = exp(eoverkt);
      const double test = 0.276 * exp_eoverkt * (-0.5772156649 - std::log(eoverkt));
      const double Gamma = g_bar > test ? g_bar : test;
      C = ARTIS_C_0 * nne * std::sqrt(T_e) * 14.51039491 * c.at->line_osc_strength[li] *
          pow(ARTIS_H_IONPOT / epsilon_trans, 2) * eoverkt / exp_eoverkt * Gamma;
    } else {
      C = nne * 8.629e-6 * 0.01 * std::exp(-eoverkt) * upperstatweight / std::sqrt(T_e);
    }
  } else {
    C = nne * 8.629e-6 * coll_strength * std::exp(-eoverkt) / lowerstatweight / std::sqrt(T_e);
  }
  return C;
}
// macroatom.cc:503-548
double rad_deexcitation_ratecoeff(const Ctx &c, const ThreadCache &tc, int e, int i, int upper, int lower,
                                  double epsilon_trans, int li, double t_current) {
  const double n_u = get_levelpop(tc, c, e, i, upper);
  const double n_l = get_levelpop(tc, c, e, i, lower);
  double R = 0.0;
  const double nu_trans = epsilon_trans / ARTIS_H;
  const double A_ul = c.at->line_einstein_A[li];
  const double B_ul = ARTIS_CLIGHTSQUAREDOVERTWOH / std::pow(nu_trans, 3) * A_ul;
  const double B_lu = stat_weight(c, e, i, upper) / stat_weight(c, e, i, lower) * B_ul;
  const double tau_sobolev = (B_lu * n_l - B_ul * n_u) * ARTIS_HCLIGHTOVERFOURPI * t_current;
  if (tau_sobolev > 1e-100) {
    const double beta = 1.0 / tau_sobolev * (-std::expm1(-tau_sobolev));
    R = A_ul * beta;
  } else {
    R = 0.0;
  }
  return R;
}
// macroatom.cc:550-643
double rad_excitation_ratecoeff(const Ctx &c, const ThreadCache &tc, int mgi, int e, int i, int lower, int upper,
                                double epsilon_trans, int li, double t_current) {
  const double n_u = get_levelpop(tc, c, e, i, upper);
  const double n_l = get_levelpop(tc, c, e, i, lower);
  double R = 0.0;
  const double nu_trans = epsilon_trans / ARTIS_H;
  const double A_ul = c.at->line_einstein_A[li];
  const double B_ul = ARTIS_CLIGHTSQUAREDOVERTWOH / pow(nu_trans, 3) * A_ul;
  const double B_lu = stat_weight(c, e, i, upper) / stat_weight(c, e, i, lower) * B_ul;
  const double tau_sobolev = (B_lu * n_l - B_ul * n_u) * ARTIS_HCLIGHTOVERFOURPI * t_current;
  if (tau_sobolev > 1e-100) {
    const double beta = 1.0 / tau_sobolev * (-expm1(-tau_sobolev));
    const double R_over_J_nu = n_l > 0. ? (B_lu - B_ul * n_u / n_l) * beta : B_lu * beta;
    R = R_over_J_nu * radfield(c, nu_trans, mgi);
  } else {
    R = 0.;
  }
  if (R < 0 || !std::isfinite(R)) {
    fprintf(stderr, "oracle: rad_excitation_ratecoeff invalid R %g\n", R);
    abort();
  }
  return R;
}
// macroatom.cc:645-678
double rad_recombination_ratecoeff(const Ctx &c, float T_e, float nne, int e, int upperion, int upper, int lower) {
  double R = 0.0;
  const int nt = get_nphixstargets(c, e, upperion - 1, lower);
  for (int t = 0; t < nt; t++) {
    if (get_phixsupperlevel(c, e, upperion - 1, lower, t) == upper) {
      R = nne * get_spontrecombcoeff(c, e, upperion - 1, lower, t, T_e);
      break;
    }
  }
  return R;
}
// macroatom.cc:704-743
double col_recombination_ratecoeff(const Ctx &c, int mgi, int e, int upperion, int upper, int lower, double epsilon_trans) {
  const int nt = get_nphixstargets(c, e, upperion - 1, lower);
  for (int t = 0; t < nt; t++) {
    if (get_phixsupperlevel(c, e, upperion - 1, lower, t) == upper) {
      const float nne = c.cs->nne[mgi];
      const float T_e = c.cs->Te[mgi];
      const double fac1 = epsilon_trans / ARTIS_KB / T_e;
      const int ionstage = get_ionstage(c, e, upperion);
      double g;
      if (ionstage - 1 == 1)
        g = 0.1;
      else if (ionstage - 1 == 2)
        g = 0.2;
      else
        g = 0.3;
      const double sigma_bf = (level_photoion_xs(c, e, upperion - 1, lower)[0] *
                               get_phixsprobability(c, e, upperion - 1, lower, t));
      const double sf = calculate_sahafact(c, e, upperion - 1, lower, upper, T_e, epsilon_trans);
      return nne * nne * sf * 1.55e13 * pow(T_e, -0.5) * g * sigma_bf * exp(-fac1) / fac1;
    }
  }
  return 0.;
}
// macroatom.cc:745-776
double col_ionization_ratecoeff(const Ctx &c, float T_e, float nne, int e, int i, int lower, int t, double epsilon_trans) {
  double g;
  const int ionstage = get_ionstage(c, e, i);
  if (ionstage == 1)
    g = 0.1;
  else if (ionstage == 2)
    g = 0.2;
  else
    g = 0.3;
  const double fac1 = epsilon_trans / ARTIS_KB / T_e;
  const double sigma_bf = level_photoion_xs(c, e, i, lower)[0] * get_phixsprobability(c, e, i, lower, t);
  return nne * 1.55e13 * pow(T_e, -0.5) * g * sigma_bf * exp(-fac1) / fac1;
}

// --------------------------------------------------------------------------------------------- estimators
inline void safeadd(double *p, double v) {
#pragma omp atomic update
  *p += v;
}
inline void safeadd(float *p, double v) {  // globals::compton_emiss is float (grid.cc:1699)
#pragma omp atomic update
  *p += v;
}
inline void counter_inc(Est &E, int ctr) {
#pragma omp atomic update
  E.e->counters[ctr] += 1;
}

// ---------------------------------------------------------------------------------------------- emission
// rpkt.cc:975-1025
void emitt_rpkt(const Ctx &c, artis_rng *rng, artis_packet *p) {
  p->type = ARTIS_TYPE_RPKT;
  p->last_cross = ARTIS_NONE;
  double dir_cmf[3];
  get_rand_isotropic_unitvec(rng, dir_cmf);
  double vel_vec[3];
  get_velocity(p->pos, vel_vec, -1. * p->prop_time);
  angle_ab(dir_cmf, vel_vec, p->dir);
  const double dopplerfactor = doppler_packet_nucmf_on_nurf(c, p);
  p->nu_rf = p->nu_cmf / dopplerfactor;
  p->e_rf = p->e_cmf / dopplerfactor;
  p->stokes[0] = 1.;
  p->stokes[1] = 0.;
  p->stokes[2] = 0.;
  double dummy_dir[3] = {0., 0., 1.};
  cross_prod(p->dir, dummy_dir, p->pol_dir);
  if ((dot(p->pol_dir, p->pol_dir)) < 1.e-8) {
    dummy_dir[0] = dummy_dir[2] = 0.0;
    dummy_dir[1] = 1.0;
    cross_prod(p->dir, dummy_dir, p->pol_dir);
  }
  vec_norm(p->pol_dir, p->pol_dir);
}

// vpkt.cc:898-929
double rot_angle(const double n1[3], const double n2[3], const double ref1[3], const double ref2[3]) {
  double i = 0;
  double ref1_sc[3];
  ref1_sc[0] = n1[0] * dot(n1, n2) - n2[0];
  ref1_sc[1] = n1[1] * dot(n1, n2) - n2[1];
  ref1_sc[2] = n1[2] * dot(n1, n2) - n2[2];
  vec_norm(ref1_sc, ref1_sc);
  double cos_stokes_rot_1 = dot(ref1_sc, ref1);
  const double cos_stokes_rot_2 = dot(ref1_sc, ref2);
  if (cos_stokes_rot_1 < -1) cos_stokes_rot_1 = -1;
  if (cos_stokes_rot_1 > 1) cos_stokes_rot_1 = 1;
  if ((cos_stokes_rot_1 > 0) && (cos_stokes_rot_2 > 0)) i = acos(cos_stokes_rot_1);
  if ((cos_stokes_rot_1 > 0) && (cos_stokes_rot_2 < 0)) i = 2 * acos(-1.) - acos(cos_stokes_rot_1);
  if ((cos_stokes_rot_1 < 0) && (cos_stokes_rot_2 < 0)) i = acos(-1.) + acos(fabs(cos_stokes_rot_1));
  if ((cos_stokes_rot_1 < 0) && (cos_stokes_rot_2 > 0)) i = acos(-1.) - acos(fabs(cos_stokes_rot_1));
  if (cos_stokes_rot_1 == 0) i = acos(-1.) / 2.;
  if (cos_stokes_rot_2 == 0) i = 0.0;
  return i;
}
// vpkt.cc:932-944
void meridian(const double n[3], double ref1[3], double ref2[3]) {
  ref1[0] = -1. * n[0] * n[2] / sqrt(n[0] * n[0] + n[1] * n[1]);
  ref1[1] = -1. * n[1] * n[2] / sqrt(n[0] * n[0] + n[1] * n[1]);
  ref1[2] = (1 - (n[2] * n[2])) / sqrt(n[0] * n[0] + n[1] * n[1]);
  ref2[0] = n[2] * ref1[1] - n[1] * ref1[2];
  ref2[1] = n[0] * ref1[2] - n[2] * ref1[0];
  ref2[2] = n[1] * ref1[0] - n[0] * ref1[1];
}
// vpkt.cc:1022-1069
void lorentz(const double e_rf[3], const double n_rf[3], const double v[3], double e_cmf[3]) {
  double beta[3], e_par[3], e_perp[3], b_rf[3], b_par[3], b_perp[3], v_cr_b[3], v_cr_e[3], b_cmf[3];
  beta[0] = v[0] / ARTIS_CLIGHT;
  beta[1] = v[1] / ARTIS_CLIGHT;
  beta[2] = v[2] / ARTIS_CLIGHT;
  const double vsqr = dot(beta, beta);
  const double gamma_rel = 1. / (sqrt(1 - vsqr));
  const double edb = (e_rf[0] * beta[0] + e_rf[1] * beta[1] + e_rf[2] * beta[2]);
  e_par[0] = edb * beta[0] / (vsqr);
  e_par[1] = edb * beta[1] / (vsqr);
  e_par[2] = edb * beta[2] / (vsqr);
  e_perp[0] = e_rf[0] - e_par[0];
  e_perp[1] = e_rf[1] - e_par[1];
  e_perp[2] = e_rf[2] - e_par[2];
  b_rf[0] = n_rf[1] * e_rf[2] - n_rf[2] * e_rf[1];
  b_rf[1] = n_rf[2] * e_rf[0] - n_rf[0] * e_rf[2];
  b_rf[2] = n_rf[0] * e_rf[1] - n_rf[1] * e_rf[0];
  const double bdb = (b_rf[0] * beta[0] + b_rf[1] * beta[1] + b_rf[2] * beta[2]);
  b_par[0] = bdb * beta[0] / (vsqr);
  b_par[1] = bdb * beta[1] / (vsqr);
  b_par[2] = bdb * beta[2] / (vsqr);
  b_perp[0] = b_rf[0] - b_par[0];
  b_perp[1] = b_rf[1] - b_par[1];
  b_perp[2] = b_rf[2] - b_par[2];
  v_cr_b[0] = beta[1] * b_rf[2] - beta[2] * b_rf[1];
  v_cr_b[1] = beta[2] * b_rf[0] - beta[0] * b_rf[2];
  v_cr_b[2] = beta[0] * b_rf[1] - beta[1] * b_rf[0];
  v_cr_e[0] = beta[1] * e_rf[2] - beta[2] * e_rf[1];
  v_cr_e[1] = beta[2] * e_rf[0] - beta[0] * e_rf[2];
  v_cr_e[2] = beta[0] * e_rf[1] - beta[1] * e_rf[0];
  e_cmf[0] = e_par[0] + gamma_rel * (e_perp[0] + v_cr_b[0]);
  e_cmf[1] = e_par[1] + gamma_rel * (e_perp[1] + v_cr_b[1]);
  e_cmf[2] = e_par[2] + gamma_rel * (e_perp[2] + v_cr_b[2]);
  b_cmf[0] = b_par[0] + gamma_rel * (b_perp[0] - v_cr_e[0]);
  b_cmf[1] = b_par[1] + gamma_rel * (b_perp[1] - v_cr_e[1]);
  b_cmf[2] = b_par[2] + gamma_rel * (b_perp[2] - v_cr_e[2]);
  vec_norm(e_cmf, e_cmf);
  vec_norm(b_cmf, b_cmf);
}
// vpkt.cc:947-1019
void frame_transform(const double n_rf[3], double *Q, double *U, const double v[3], double n_cmf[3]) {
  double ref1[3], ref2[3], e_rf[3], e_cmf[3];
  double theta_rot = 0.;
  meridian(n_rf, ref1, ref2);
  const double Q0 = *Q;
  const double U0 = *U;
  const double p = sqrt(Q0 * Q0 + U0 * U0);
  double rot_angle_ = 0;
  if (p > 0) {
    const double cos2rot_angle = Q0 / p;
    const double sin2rot_angle = U0 / p;
    if ((cos2rot_angle > 0) && (sin2rot_angle > 0)) rot_angle_ = acos(Q0 / p) / 2.;
    if ((cos2rot_angle < 0) && (sin2rot_angle > 0)) rot_angle_ = (acos(-1.) - acos(fabs(Q0 / p))) / 2.;
    if ((cos2rot_angle < 0) && (sin2rot_angle < 0)) rot_angle_ = (acos(-1.) + acos(fabs(Q0 / p))) / 2.;
    if ((cos2rot_angle > 0) && (sin2rot_angle < 0)) rot_angle_ = (2. * acos(-1.) - acos(fabs(Q0 / p))) / 2.;
    if (cos2rot_angle == 0) {
      rot_angle_ = 0.25 * acos(-1);
      if (U0 < 0) rot_angle_ = 0.75 * acos(-1);
    }
    if (sin2rot_angle == 0) {
      rot_angle_ = 0.0;
      if (Q0 < 0) rot_angle_ = 0.5 * acos(-1);
    }
  }
  e_rf[0] = cos(rot_angle_) * ref1[0] - sin(rot_angle_) * ref2[0];
  e_rf[1] = cos(rot_angle_) * ref1[1] - sin(rot_angle_) * ref2[1];
  e_rf[2] = cos(rot_angle_) * ref1[2] - sin(rot_angle_) * ref2[2];
  angle_ab(n_rf, v, n_cmf);
  lorentz(e_rf, n_rf, v, e_cmf);
  meridian(n_cmf, ref1, ref2);
  const double e_cmf_ref1 = e_cmf[0] * ref1[0] + e_cmf[1] * ref1[1] + e_cmf[2] * ref1[2];
  const double e_cmf_ref2 = e_cmf[0] * ref2[0] + e_cmf[1] * ref2[1] + e_cmf[2] * ref2[2];
  if ((e_cmf_ref1 > 0) && (e_cmf_ref2 < 0)) theta_rot = acos(e_cmf_ref1);
  if ((e_cmf_ref1 < 0) && (e_cmf_ref2 < 0)) theta_rot = acos(-1.) - acos(fabs(e_cmf_ref1));
  if ((e_cmf_ref1 < 0) && (e_cmf_ref2 > 0)) theta_rot = acos(-1.) + acos(fabs(e_cmf_ref1));
  if ((e_cmf_ref1 > 0) && (e_cmf_ref2 > 0)) theta_rot = 2 * acos(-1.) - acos(e_cmf_ref1);
  if (e_cmf_ref1 == 0) theta_rot = acos(-1.) / 2.;
  if (e_cmf_ref2 == 0) theta_rot = 0.0;
  if (e_cmf_ref1 > 1) theta_rot = 0.0;
  if (e_cmf_ref1 < -1) theta_rot = acos(-1.);
  *Q = cos(2 * theta_rot) * p;
  *U = sin(2 * theta_rot) * p;
}

// polarization.cc:6-157
void escat_rpkt(const Ctx &c, artis_rng *rng, artis_packet *p) {
  p->type = ARTIS_TYPE_RPKT;
  p->last_cross = ARTIS_NONE;
  double vel_vec[3];
  get_velocity(p->pos, vel_vec, p->prop_time);
  double Qi = p->stokes[1];
  double Ui = p->stokes[2];
  double old_dir_cmf[3];
  frame_transform(p->dir, &Qi, &Ui, vel_vec, old_dir_cmf);
  double M = 0., mu = 0., phisc = 0.;
  if (c.rp.pol_dipole) {
    double pr = 0., x = 0.;
    do {
      const double zrand = artis_rng_uniform(rng);
      const double zrand2 = artis_rng_uniform(rng);
      const double zrand3 = artis_rng_uniform(rng);
      M = 2 * zrand - 1;
      mu = pow(M, 2.);
      phisc = 2 * ARTIS_PI * zrand2;
      pr = (mu + 1) + (mu - 1) * (cos(2 * phisc) * Qi + sin(2 * phisc) * Ui);
      x = 2 * zrand3;
    } while (x > pr);
  } else {
    const double zrand = artis_rng_uniform(rng);
    const double zrand2 = artis_rng_uniform(rng);
    M = 2. * zrand - 1;
    mu = pow(M, 2.);
    phisc = 2 * ARTIS_PI * zrand2;
  }
  const double tsc = acos(M);
  double new_dir_cmf[3];
  if (fabs(old_dir_cmf[2]) < 0.99999) {
    new_dir_cmf[0] = sin(tsc) / sqrt(1. - pow(old_dir_cmf[2], 2.)) *
                         (old_dir_cmf[1] * sin(phisc) - old_dir_cmf[0] * old_dir_cmf[2] * cos(phisc)) +
                     old_dir_cmf[0] * cos(tsc);
    new_dir_cmf[1] = sin(tsc) / sqrt(1 - pow(old_dir_cmf[2], 2.)) *
                         (-old_dir_cmf[0] * sin(phisc) - old_dir_cmf[1] * old_dir_cmf[2] * cos(phisc)) +
                     old_dir_cmf[1] * cos(tsc);
    new_dir_cmf[2] = sin(tsc) * cos(phisc) * sqrt(1 - pow(old_dir_cmf[2], 2.)) + old_dir_cmf[2] * cos(tsc);
  } else {
    new_dir_cmf[0] = sin(tsc) * cos(phisc);
    new_dir_cmf[1] = sin(tsc) * sin(phisc);
    new_dir_cmf[2] = (old_dir_cmf[2] > 0) ? cos(tsc) : -cos(tsc);
  }
  double ref1[3], ref2[3];
  meridian(old_dir_cmf, ref1, ref2);
  const double i1 = rot_angle(old_dir_cmf, new_dir_cmf, ref1, ref2);
  const double cos2i1 = cos(2 * i1);
  const double sin2i1 = sin(2 * i1);
  const double Qold = Qi * cos2i1 - Ui * sin2i1;
  const double Uold = Qi * sin2i1 + Ui * cos2i1;
  mu = dot(old_dir_cmf, new_dir_cmf);
  const double Inew = 0.75 * ((mu * mu + 1.0) + Qold * (mu * mu - 1.0));
  double Qnew = 0.75 * ((mu * mu - 1.0) + Qold * (mu * mu + 1.0));
  double Unew = 1.5 * mu * Uold;
  Qnew = Qnew / Inew;
  Unew = Unew / Inew;
  const double I = 1.0;
  meridian(new_dir_cmf, ref1, ref2);
  const double i2 = ARTIS_PI + rot_angle(new_dir_cmf, old_dir_cmf, ref1, ref2);
  const double cos2i2 = cos(2 * i2);
  const double sin2i2 = sin(2 * i2);
  double Q = Qnew * cos2i2 + Unew * sin2i2;
  double U = -Qnew * sin2i2 + Unew * cos2i2;
  double vel_rev[3] = {-vel_vec[0], -vel_vec[1], -vel_vec[2]};
  double dummy_dir[3];
  frame_transform(new_dir_cmf, &Q, &U, vel_rev, dummy_dir);
  p->stokes[0] = I;
  p->stokes[1] = Q;
  p->stokes[2] = U;
  p->dir[0] = dummy_dir[0];
  p->dir[1] = dummy_dir[1];
  p->dir[2] = dummy_dir[2];
  const double dopplerfactor = doppler_packet_nucmf_on_nurf(c, p);
  p->nu_rf = p->nu_cmf / dopplerfactor;
  p->e_rf = p->e_cmf / dopplerfactor;
}

// ------------------------------------------------------------------------------------------------ boundary
[[noreturn]] static void shell_fatal(const char *what, double shellradius, const double pos[3]) {
  fprintf(stderr, "oracle: [fatal] get_shellcrossdist: %s (shellradius %g, |pos| %g)\n", what, shellradius,
          sqrt(dot(pos, pos)));
  abort();
}

// boundary.cc:14-99 get_shellcrossdist: the closest forward distance to the intersection of a ray with an expanding
// spherical shell; -1 if there is no forward intersection (or a tangential one)
static double get_shellcrossdist(const double pos[3], const double dir[3], const double shellradius,
                                 const bool isinnerboundary, const double tstart) {
  if (!(shellradius > 0)) shell_fatal("shellradius > 0", shellradius, pos);
  const double speed = vec_len(dir) * ARTIS_CLIGHT_PROP;
  const double a = dot(dir, dir) - pow(shellradius / tstart / speed, 2);
  const double b = 2 * (dot(dir, pos) - pow(shellradius, 2) / tstart / speed);
  const double cc = dot(pos, pos) - pow(shellradius, 2);
  const double discriminant = pow(b, 2) - 4 * a * cc;
  if (discriminant < 0) {
    // no intersection
    if (!(shellradius < vec_len(pos))) shell_fatal("no intersection inside the shell", shellradius, pos);
    return -1;
  } else if (discriminant > 0) {
    // two intersections
    double d1 = (-b + sqrt(discriminant)) / 2 / a;
    double d2 = (-b - sqrt(discriminant)) / 2 / a;
    double posfinal1[3], posfinal2[3];
    for (int d = 0; d < 3; d++) {  // cblas_dcopy, then cblas_daxpy (y += alpha x)
      posfinal1[d] = pos[d];
      posfinal1[d] += d1 * dir[d];
      posfinal2[d] = pos[d];
      posfinal2[d] += d2 * dir[d];
    }
    const double shellradiusfinal1 = shellradius / tstart * (tstart + d1 / speed);
    const double shellradiusfinal2 = shellradius / tstart * (tstart + d2 / speed);
    if (!(fabs(vec_len(posfinal1) / shellradiusfinal1 - 1.) < 1e-3)) shell_fatal("solution 1 off the shell", shellradius, pos);
    if (!(fabs(vec_len(posfinal2) / shellradiusfinal2 - 1.) < 1e-3)) shell_fatal("solution 2 off the shell", shellradius, pos);
    // invalidate any solutions that require entering the boundary from the wrong radial direction
    if (isinnerboundary) {
      if (dot(posfinal1, dir) > 0.) d1 = -1;
      if (dot(posfinal2, dir) > 0.) d2 = -1;
    } else {
      if (dot(posfinal1, dir) < 0.) d1 = -1;
      if (dot(posfinal2, dir) < 0.) d2 = -1;
    }
    // negative d means in the reverse direction along the ray
    if (d1 < 0 && d2 < 0) return -1;
    if (d2 < 0) return d1;
    if (d1 < 0) return d2;
    return fmin(d1, d2);
  }
  // exactly one intersection: ignored (the packet stays in its cell)
  if (!(shellradius <= vec_len(pos))) shell_fatal("single intersection inside the shell", shellradius, pos);
  return -1.;
}

// rpkt.cc:659-661, gammapkt.cc:551-553
static double max_sdist(const Ctx &c, const artis_packet *p, double sdist) {
  return (c.g->grid_type == ARTIS_GRID_SPHERICAL1D) ? 2 * c.g->rmax * (p->prop_time + sdist / ARTIS_CLIGHT_PROP) / c.g->tmin
                                                     : c.g->rmax * p->prop_time / c.g->tmin;
}

// boundary.cc:101-330, GRID_SPHERICAL1D: one radial coordinate (get_ngriddimensions() == 1), cellindex == shell,
// cellcoordmax = pos_min + wid_init(cellindex), get_cellcoordpointnum = cellindex, index increment 1
static double boundary_cross_spherical(const Ctx &c, artis_packet *p, int *snext) {
  const double tstart = p->prop_time;
  const int cellindex = p->where;
  const double tmin = c.g->tmin;
  const int n0 = c.g->ncoordgrid[0];
  const double initpos = vec_len(p->pos);
  const double cellcoordmin = c.g->cell_pos_min[(size_t)cellindex * 3];
  const double cellcoordmax = cellcoordmin + c.g->modelcell_wid_init[cellindex];
  const double vel = dot(p->pos, p->dir) / vec_len(p->pos) * ARTIS_CLIGHT_PROP;  // radial velocity
  int last_cross = p->last_cross;
  for (int flip = 0; flip < 2; flip++) {
    const int direction = flip ? ARTIS_POS_X : ARTIS_NEG_X;
    const int invdirection = !flip ? ARTIS_POS_X : ARTIS_NEG_X;
    const int cellindexstride = flip ? -1 : 1;
    bool isoutside_thisside;
    if (flip)
      isoutside_thisside = initpos < (cellcoordmin / tmin * tstart - 10.);
    else
      isoutside_thisside = initpos > (cellcoordmax / tmin * tstart + 10.);
    if (isoutside_thisside && (last_cross != direction)) {
      if ((vel - (initpos / tstart)) > 0) {
        if ((cellindex == (n0 - 1) && cellindexstride > 0) || (cellindex == 0 && cellindexstride < 0)) {
          *snext = -99;
          return 0;
        }
        *snext = p->where + cellindexstride;
        p->last_cross = invdirection;
        return 0;
      }
      last_cross = direction;
    }
  }
  last_cross = ARTIS_NONE;  // handled by d_inner / d_outer being negative for invalid directions
  const double r_inner = cellcoordmin * tstart / tmin;
  const double d_inner = (r_inner > 0.) ? get_shellcrossdist(p->pos, p->dir, r_inner, true, tstart) : -1.;
  const double t_coordminboundary = d_inner / ARTIS_CLIGHT_PROP;
  const double r_outer = cellcoordmax * tstart / tmin;
  const double d_outer = get_shellcrossdist(p->pos, p->dir, r_outer, false, tstart);
  const double t_coordmaxboundary = d_outer / ARTIS_CLIGHT_PROP;
  double time = 1.e99;
  if ((t_coordmaxboundary > 0) && (t_coordmaxboundary < time) && (last_cross != ARTIS_NEG_X)) {
    time = t_coordmaxboundary;
    if (cellindex == (n0 - 1)) {
      *snext = -99;
    } else {
      *snext = p->where + 1;
      p->last_cross = ARTIS_POS_X;
    }
  }
  if ((t_coordminboundary > 0) && (t_coordminboundary < time) && (last_cross != ARTIS_POS_X)) {
    time = t_coordminboundary;
    if (cellindex == 0) {
      *snext = -99;
    } else {
      *snext = p->where - 1;
      p->last_cross = ARTIS_NEG_X;
    }
  }
  return ARTIS_CLIGHT_PROP * time;
}

// boundary.cc:101-330 (GRID_UNIFORM; GRID_SPHERICAL1D in boundary_cross_spherical)
double boundary_cross(const Ctx &c, Est &E, artis_packet *p, int *snext) {
  if (c.g->grid_type == ARTIS_GRID_SPHERICAL1D) return boundary_cross_spherical(c, p, snext);
  const double tstart = p->prop_time;
  const int cellindex = p->where;
  const double tmin = c.g->tmin;
  const int n[3] = {c.g->ncoordgrid[0], c.g->ncoordgrid[1], c.g->ncoordgrid[2]};
  const int stride[3] = {1, n[0], n[0] * n[1]};
  const double wid = 2 * c.g->coordmax[0] / n[0];  // grid.cc:76-91
  double initpos[3], cellcoordmax[3], cellcoordmin[3], vel[3];
  int pointnum[3];
  for (int d = 0; d < 3; d++) {
    initpos[d] = p->pos[d];
    cellcoordmin[d] = c.g->cell_pos_min[(size_t)cellindex * 3 + d];
    cellcoordmax[d] = cellcoordmin[d] + wid;
    vel[d] = p->dir[d] * ARTIS_CLIGHT_PROP;
  }
  pointnum[0] = cellindex % n[0];
  pointnum[1] = (cellindex / n[0]) % n[1];
  pointnum[2] = (cellindex / (n[0] * n[1])) % n[2];
  int last_cross = p->last_cross;
  const int negdirections[3] = {ARTIS_NEG_X, ARTIS_NEG_Y, ARTIS_NEG_Z};
  const int posdirections[3] = {ARTIS_POS_X, ARTIS_POS_Y, ARTIS_POS_Z};
  for (int d = 0; d < 3; d++) {
    for (int flip = 0; flip < 2; flip++) {
      const int direction = flip ? posdirections[d] : negdirections[d];
      const int invdirection = !flip ? posdirections[d] : negdirections[d];
      const int cellindexstride = flip ? -stride[d] : stride[d];
      bool isoutside_thisside;
      if (flip)
        isoutside_thisside = initpos[d] < (cellcoordmin[d] / tmin * tstart - 10.);
      else
        isoutside_thisside = initpos[d] > (cellcoordmax[d] / tmin * tstart + 10.);
      if (isoutside_thisside && (last_cross != direction)) {
        if ((vel[d] - (initpos[d] / tstart)) > 0) {
          if ((pointnum[d] == (n[d] - 1) && cellindexstride > 0) || (pointnum[d] == 0 && cellindexstride < 0)) {
            *snext = -99;
            return 0;
          } else {
            *snext = p->where + cellindexstride;
            p->last_cross = invdirection;
            return 0;
          }
        } else {
          last_cross = direction;
        }
      }
    }
  }
  double t_coordmaxboundary[3], t_coordminboundary[3];
  for (int d = 0; d < 3; d++) {
    t_coordmaxboundary[d] = ((initpos[d] - (vel[d] * tstart)) / ((cellcoordmax[d]) - (vel[d] * tmin)) * tmin) - tstart;
    t_coordminboundary[d] = ((initpos[d] - (vel[d] * tstart)) / ((cellcoordmin[d]) - (vel[d] * tmin)) * tmin) - tstart;
  }
  int choice = 0;
  double time = 1.e99;
  for (int d = 0; d < 3; d++) {
    if ((t_coordmaxboundary[d] > 0) && (t_coordmaxboundary[d] < time) && (last_cross != negdirections[d])) {
      choice = posdirections[d];
      time = t_coordmaxboundary[d];
      if (pointnum[d] == (n[d] - 1)) {
        *snext = -99;
      } else {
        *snext = p->where + stride[d];
        p->last_cross = posdirections[d];
      }
    }
    if ((t_coordminboundary[d] > 0) && (t_coordminboundary[d] < time) && (last_cross != posdirections[d])) {
      choice = negdirections[d];
      time = t_coordminboundary[d];
      if (pointnum[d] == 0) {
        *snext = -99;
      } else {
        *snext = p->where - stride[d];
        p->last_cross = negdirections[d];
      }
    }
  }
  (void)choice;
  (void)E;
  return ARTIS_CLIGHT_PROP * time;
}
// boundary.cc:332-357
void change_cell(Est &E, artis_packet *p, int snext) {
  if (snext == -99) {
    p->escape_type = p->type;
    p->escape_time = (int)p->prop_time;
    p->type = ARTIS_TYPE_ESCAPE;
#pragma omp atomic update
    E.e->nesc += 1;
  } else {
    p->where = snext;
    counter_inc(E, CTR_CELLCROSSINGS);
  }
}

// --------------------------------------------------------------------------------------- continuum opacity
// rpkt.cc:1027-1073
double calculate_kappa_ff(const Ctx &c, int mgi, double nu) {
  const double g_ff = 1;
  const float nne = c.cs->nne[mgi];
  const float T_e = c.cs->Te[mgi];
  double kappa_ff = 0.;
  for (int e = 0; e < c.at->nelements; e++)
    for (int i = 0; i < get_nions(c, e); i++) {
      const double nnion = ionstagepop(c, mgi, e, i);
      const int Z = get_ionstage(c, e, i) - 1;
      if (Z > 0) kappa_ff += Z * Z * g_ff * nnion;
    }
  kappa_ff *= 3.69255e8 / sqrt((double)T_e) * pow(nu, -3) * nne * (1 - exp(-ARTIS_HOVERKB * nu / T_e));
  return kappa_ff;
}
// rpkt.cc:1075-1207 (SEPARATE_STIMRECOMB false); DETAILED_BF_ESTIMATORS_ON: every continuum of an element
// present in the cell is included (rpkt.cc:1116-1118) and gamma_contr[i] is kept for update_bfestimators
double calculate_kappa_bf_gammacontr(const Ctx &c, ThreadCache &tc, int mgi, double nu) {
  double kappa_bf_sum = 0.;
  const artis_atomic_tables &a = *c.at;
  const bool detailed = c.rp.detailed_bf_estimators;
  for (int g = 0; g < a.nbfcontinua_ground; g++) tc.groundcont_gamma_contr[g] = 0.;
  const double T_e = c.cs->Te[mgi];
  const double nne = c.cs->nne[mgi];
  const double nnetot = c.cs->nnetot[mgi];
  int i = 0;
  const int nbfcontinua = a.nbfcontinua;
  for (i = 0; i < nbfcontinua; i++) {
    if (!(nu < a.allcont_nu_edge[i])) tc.work[WK_BF_ACTIVE]++;
    const int element = a.allcont_element[i];
    const int ion = a.allcont_ion[i];
    const int level = a.allcont_level[i];
    if ((detailed && c.cs->elem_abundance[(size_t)mgi * a.nelements + element] > 0) ||
        (!detailed && ((ionstagepop(c, mgi, element, ion) / nnetot > 1.e-6) || (level == 0)))) {
      const double nu_edge = a.allcont_nu_edge[i];
      const double nnlevel = get_levelpop(tc, c, element, ion, level);
      const double nu_max_phixs = nu_edge * a.last_phixs_nuovernuedge;
      if (nu < nu_edge) break;
      if (nu <= nu_max_phixs && nnlevel > 0) {
        const double sigma_bf = photoionization_crosssection_fromtable(
            c, a.phixs_xs + (size_t)a.allcont_phixstable[i] * a.nphixspoints, nu_edge, nu);
        const double probability = a.allcont_probability[i];
        double departure_ratio = tc.departureratios[i];
        if (departure_ratio < 0) {
          const int upper = a.allcont_upperlevel[i];
          const double nnupperionlevel = get_levelpop(tc, c, element, ion + 1, upper);
          const double sf = calculate_sahafact(c, element, ion, level, upper, T_e, ARTIS_H * nu_edge);
          departure_ratio = nnupperionlevel / nnlevel * nne * sf;
          tc.departureratios[i] = departure_ratio;
        }
        const double stimfactor = departure_ratio * exp(-ARTIS_HOVERKB * nu / T_e);
        double corrfactor = 1 - stimfactor;
        if (corrfactor < 0) corrfactor = 0.;
        const double kappa_bf_contr = nnlevel * sigma_bf * probability * corrfactor;
        if (level == 0) {
          const int gphixsindex = a.allcont_index_in_groundphixslist[i];
          tc.groundcont_gamma_contr[gphixsindex] += sigma_bf * probability * corrfactor;
        }
        if (detailed) tc.gamma_contr[i] = sigma_bf * probability * corrfactor;
        if (!std::isfinite(kappa_bf_contr)) {
          fprintf(stderr, "oracle: non-finite kappa_bf_contr\n");
          abort();
        }
        kappa_bf_sum += kappa_bf_contr;
        tc.kappa_bf_sum[i] = kappa_bf_sum;
      } else {
        tc.kappa_bf_sum[i] = kappa_bf_sum;
        if (detailed) tc.gamma_contr[i] = 0.;
      }
    } else {
      tc.kappa_bf_sum[i] = kappa_bf_sum;
      if (detailed) tc.gamma_contr[i] = 0.;
    }
  }
  for (; i < nbfcontinua; i++) {
    tc.kappa_bf_sum[i] = kappa_bf_sum;
    if (detailed) tc.gamma_contr[i] = 0.;
  }
  return kappa_bf_sum;
}
// rpkt.cc:1209-1295 (deviation D2: always recomputed)
void calculate_kappa_rpkt_cont(const Ctx &c, ThreadCache &tc, const artis_packet *p) {
  const int mgi = cell_mgi(c, p->where);
  const double nu_cmf = p->nu_cmf;
  const float nne = c.cs->nne[mgi];
  double sigma = 0.0, kappa_ff = 0., kappa_bf = 0., kappa_ffheating = 0.;
  tc.work[WK_KAPPA_EVALS]++;
  if (c.rp.do_r_lc) {
    if (c.rp.opacity_case == 4) {
      sigma = ARTIS_SIGMA_T * nne;
      kappa_ff = calculate_kappa_ff(c, mgi, nu_cmf);
      kappa_ffheating = kappa_ff;
      kappa_bf = calculate_kappa_bf_gammacontr(c, tc, mgi, nu_cmf);
    } else {
      sigma = 0.;
      kappa_ff = 1e5 * calculate_kappa_ff(c, mgi, nu_cmf);
      kappa_bf = 0.;
    }
  }
  tc.kap_total = sigma + kappa_bf + kappa_ff;
  tc.kap_es = sigma;
  tc.kap_ff = kappa_ff;
  tc.kap_bf = kappa_bf;
  tc.kap_ffheating = kappa_ffheating;
  if (!std::isfinite(tc.kap_total)) {
    if (std::isfinite(tc.kap_es)) {
      tc.kap_ff = 0.;
      tc.kap_bf = 0.;
      tc.kap_total = tc.kap_es;
    } else {
      fprintf(stderr, "oracle: non-finite kappa_rpkt_cont\n");
      abort();
    }
  }
}

// --------------------------------------------------------------------------------------------- line search
// rpkt.cc:26-65
int closest_transition(const Ctx &c, double nu_cmf, int next_trans) {
  const int nlines = c.at->nlines;
  const double *lnu = c.at->line_nu;
  const int left = next_trans;
  const int right = nlines - 1;
  if (nu_cmf < lnu[right]) return -1;
  if (left > right) return -1;
  if (left > 0) return left;
  if (nu_cmf >= lnu[0]) return 0;
  // lower_bound with comparator line.nu > nu_cmf  (rpkt.cc:24)
  int lo = next_trans, hi = nlines;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (!(lnu[mid] <= nu_cmf))
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}
// rpkt.cc:511-555
void closest_transition_empty(const Ctx &c, artis_packet *p) {
  const int nlines = c.at->nlines;
  const double *lnu = c.at->line_nu;
  const int left = p->next_trans;
  const int right = nlines - 1;
  if (p->nu_cmf < lnu[right]) p->next_trans = nlines + 1;
  if (left > right) p->next_trans = nlines + 1;
  int matchindex;
  if (p->nu_cmf >= lnu[left]) {
    matchindex = left;
  } else {
    int lo = p->next_trans, hi = nlines;
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (!(lnu[mid] <= p->nu_cmf))
        lo = mid + 1;
      else
        hi = mid;
    }
    matchindex = lo;
  }
  p->next_trans = matchindex;
}

// ------------------------------------------------------------------------------------------ virtual packets
// vpkt.cc:374-385: 0 once every spectrum's optical depth exceeds tau_max_vpkt
int check_tau(const VpktCfg &v, const double *tau) {
  int count = 0;
  for (int i = 0; i < v.p.nspectra; i++)
    if (tau[i] > v.p.tau_max_vpkt) count += 1;
  return (count == v.p.nspectra) ? 0 : 1;
}
// vpkt.cc:388-406 (deviation D9: a bin index rounded up to the array end is skipped)
void add_to_vspecpol(const VpktCfg &v, const artis_packet *d, int bin, int ind, double t_arrive) {
  const int ind_comb = v.p.nspectra * bin + ind;
  if (t_arrive > v.p.tmin_vspec && t_arrive < v.p.tmax_vspec) {
    const int nt = (int)((log(t_arrive) - log(v.p.tmin_vspec)) / v.dlogt);
    if (d->nu_rf > v.p.numin_vspec && d->nu_rf < v.p.numax_vspec) {
      const int nnu = (int)((log(d->nu_rf) - log(v.p.numin_vspec)) / v.dlognu);
      if (nt >= v.p.vmtbins || nnu >= v.p.vmnubins) return;
      const double pktcontrib = d->e_rf / v.delta_t[nt] / v.delta_freq[nnu] / 4.e12 / ARTIS_PI / ARTIS_PARSEC /
                                ARTIS_PARSEC / v.p.nprocs * 4 * ARTIS_PI;
      const size_t idx = ((size_t)nt * v.p.nobs * v.p.nspectra + ind_comb) * v.p.vmnubins + nnu;
      safeadd(&v.out->vstokes_i[idx], d->stokes[0] * pktcontrib);
      safeadd(&v.out->vstokes_q[idx], d->stokes[1] * pktcontrib);
      safeadd(&v.out->vstokes_u[idx], d->stokes[2] * pktcontrib);
    }
  }
}
// vpkt.cc:581-627
void add_to_vpkt_grid(const Ctx &c, const VpktCfg &v, const artis_packet *d, const double vel[3], int bin_range,
                      int bin, const double obs[3]) {
  double vref1, vref2;
  const double nx = obs[0], ny = obs[1], nz = obs[2];
  if (nx == 1) {
    vref1 = vel[1];
    vref2 = vel[2];
  } else if (nx == -1) {
    vref1 = -vel[1];
    vref2 = -vel[2];
  } else {
    vref1 = -ny * vel[0] + (nx + nz * nz / (1 + nx)) * vel[1] - ny * nz * (1 - nx) / sqrt(1 - nx * nx) * vel[2];
    vref2 = -nz * vel[0] - ny * nz * (1 - nx) / sqrt(1 - nx * nx) * vel[1] + (nx + ny * ny / (1 + nx)) * vel[2];
  }
  const double vmax = c.g->vmax;
  if (fabs(vref1) >= vmax || fabs(vref2) >= vmax) return;
  const double ybin = 2 * vmax / v.p.ny_vgrid;
  const double zbin = 2 * vmax / v.p.nz_vgrid;
  const int nt = (int)((vmax - vref1) / ybin);
  const int mt = (int)((vmax - vref2) / zbin);
  if (d->nu_rf > v.p.nu_grid_min[bin_range] && d->nu_rf < v.p.nu_grid_max[bin_range]) {
    const size_t idx = (((size_t)nt * v.p.nz_vgrid + mt) * v.p.nrange_grid + bin_range) * v.p.nobs + bin;
    safeadd(&v.out->vgrid_i[idx], d->stokes[0] * d->e_rf);
    safeadd(&v.out->vgrid_q[idx], d->stokes[1] * d->e_rf);
    safeadd(&v.out->vgrid_u[idx], d->stokes[2] * d->e_rf);
  }
}
inline void vcount(int64_t *ctr) {
#pragma omp atomic update
  *ctr += 1;
}
// vpkt.cc:76-368.  The dummy's level populations and continuum opacity come from a cellhistory of its own
// (vtc), as the reference's get_levelpop / calculate_kappa_rpkt_cont compute them for a cell other than the
// thread's cached one.  Deviation D9: when no redder line is left (closest_transition < 0) the line loop ends
// and the dummy moves on to the cell boundary (the reference keeps ldist = 0 < sdist and never leaves the loop).
void rlc_emiss_vpkt(const Ctx &c, ThreadCache &vtc, Est &E, const artis_packet *pkt, double t_current, int bin,
                    double obs[3], int realtype) {
  const VpktCfg &v = *c.vp;
  const artis_atomic_tables &a = *c.at;
  artis_packet dummy = *pkt;
  double tau[ARTIS_VPKT_MAX_SPECTRA];
  for (int ind = 0; ind < v.p.nspectra; ind++) tau[ind] = 0;
  dummy.dir[0] = obs[0];
  dummy.dir[1] = obs[1];
  dummy.dir[2] = obs[2];
  vcount(&v.out->nvpkt);
  double vel_vec[3];
  get_velocity(pkt->pos, vel_vec, t_current);
  dummy.nu_rf = dummy.nu_cmf / doppler_nucmf_on_nurf(c, dummy.dir, vel_vec);
  dummy.e_rf = dummy.e_cmf * dummy.nu_rf / dummy.nu_cmf;
  double Qi = dummy.stokes[1];
  double Ui = dummy.stokes[2];
  double I = 0., Q = 0., U = 0., pn = 0.;
  if (realtype == 1) {
    double old_dir_cmf[3], obs_cmf[3], ref1[3], ref2[3];
    frame_transform(pkt->dir, &Qi, &Ui, vel_vec, old_dir_cmf);
    angle_ab(dummy.dir, vel_vec, obs_cmf);
    meridian(old_dir_cmf, ref1, ref2);
    const double i1 = rot_angle(old_dir_cmf, obs_cmf, ref1, ref2);
    const double cos2i1 = cos(2 * i1);
    const double sin2i1 = sin(2 * i1);
    const double Qold = Qi * cos2i1 - Ui * sin2i1;
    const double Uold = Qi * sin2i1 + Ui * cos2i1;
    const double mu = dot(old_dir_cmf, obs_cmf);
    pn = 3. / (16. * ARTIS_PI) * (1 + pow(mu, 2.) + (pow(mu, 2.) - 1) * Qold);
    const double Inew = 0.75 * ((mu * mu + 1.0) + Qold * (mu * mu - 1.0));
    double Qnew = 0.75 * ((mu * mu - 1.0) + Qold * (mu * mu + 1.0));
    double Unew = 1.5 * mu * Uold;
    Qnew = Qnew / Inew;
    Unew = Unew / Inew;
    I = Inew / Inew;
    meridian(obs_cmf, ref1, ref2);
    const double i2 = ARTIS_PI + rot_angle(obs_cmf, old_dir_cmf, ref1, ref2);
    const double cos2i2 = cos(2 * i2);
    const double sin2i2 = sin(2 * i2);
    Q = Qnew * cos2i2 + Unew * sin2i2;
    U = -Qnew * sin2i2 + Unew * cos2i2;
    const double vel_rev[3] = {-vel_vec[0], -vel_vec[1], -vel_vec[2]};
    frame_transform(obs_cmf, &Q, &U, vel_rev, obs);  // overwrites the caller's obs, as vpkt.cc:179
  }
  if (realtype == 2 || realtype == 3) {
    I = 1;
    Q = 0;
    U = 0;
    pn = 1 / (4 * ARTIS_PI);
  }
  int mgi = cell_mgi(c, dummy.where);
  bool end_packet = false;
  double t_future = t_current;
  while (!end_packet) {
    double ldist = 0;
    int snext;
    const double sdist = boundary_cross(c, E, &dummy, &snext);
    const double s_cont = sdist * t_current * t_current * t_current / (t_future * t_future * t_future);
    cellhistory_reset(c, vtc, mgi);
    calculate_kappa_rpkt_cont(c, vtc, &dummy);
    const double kap_cont = vtc.kap_total;
    const double kap_cont_nobf = kap_cont - vtc.kap_bf;
    const double kap_cont_noff = kap_cont - vtc.kap_ff;
    const double kap_cont_noes = kap_cont - vtc.kap_es;
    for (int ind = 0; ind < v.p.nspectra; ind++) {
      if (v.exclude[ind] == -2)
        tau[ind] += kap_cont_nobf * s_cont;
      else if (v.exclude[ind] == -3)
        tau[ind] += kap_cont_noff * s_cont;
      else if (v.exclude[ind] == -4)
        tau[ind] += kap_cont_noes * s_cont;
      else
        tau[ind] += kap_cont * s_cont;
    }
    if (check_tau(v, tau) == 0) return;
    while (ldist < sdist) {
      const int lineindex = closest_transition(c, dummy.nu_cmf, dummy.next_trans);
      if (lineindex >= 0) {
        const double nutrans = a.line_nu[lineindex];
        const int element = a.line_elementindex[lineindex];
        const int ion = a.line_ionindex[lineindex];
        const int upper = a.line_upperlevelindex[lineindex];
        const int lower = a.line_lowerlevelindex[lineindex];
        const double A_ul = a.line_einstein_A[lineindex];
        const int anumber = v.anumber[element];
        dummy.next_trans = lineindex + 1;
        if (dummy.nu_cmf < nutrans)
          ldist = 0;
        else
          ldist = ARTIS_CLIGHT * t_current * (dummy.nu_cmf / nutrans - 1);
        if (ldist > sdist) {
          dummy.next_trans -= 1;
          break;
        }
        const double t_line = t_current + ldist / ARTIS_CLIGHT;
        const double B_ul = ARTIS_CLIGHTSQUAREDOVERTWOH / pow(nutrans, 3) * A_ul;
        const double B_lu = stat_weight(c, element, ion, upper) / stat_weight(c, element, ion, lower) * B_ul;
        const double n_u = get_levelpop(vtc, c, element, ion, upper);
        const double n_l = get_levelpop(vtc, c, element, ion, lower);
        for (int ind = 0; ind < v.p.nspectra; ind++)
          if (v.exclude[ind] != -1 && (anumber != v.exclude[ind]))
            tau[ind] += (B_lu * n_l - B_ul * n_u) * ARTIS_HCLIGHTOVERFOURPI * t_line;
        if (check_tau(v, tau) == 0) return;
      } else {
        dummy.next_trans = a.nlines + 1;
        break;  // D9
      }
    }
    t_future += (sdist / ARTIS_CLIGHT_PROP);
    dummy.prop_time = t_future;
    move_pkt(c, &dummy, sdist);
    change_cell(E, &dummy, snext);
    end_packet = (dummy.type == ARTIS_TYPE_ESCAPE);
    mgi = cell_mgi(c, dummy.where);
    if (mgi == npts_model(c)) break;
    if (c.cs->thick[mgi] == 1) return;
  }
  if (realtype == 1)
    vcount(&v.out->nvpkt_esc1);
  else if (realtype == 2)
    vcount(&v.out->nvpkt_esc2);
  else if (realtype == 3)
    vcount(&v.out->nvpkt_esc3);
  double t_arrive = 0.;
  for (int ind = 0; ind < v.p.nspectra; ind++) {
    const double prob = pn * exp(-tau[ind]);
    dummy.stokes[0] = I * prob;
    dummy.stokes[1] = Q * prob;
    dummy.stokes[2] = U * prob;
    t_arrive = t_current - (dot(pkt->pos, dummy.dir) / ARTIS_CLIGHT_PROP);
    add_to_vspecpol(v, &dummy, bin, ind, t_arrive);
  }
  if (v.p.vgrid_flag == 1) {
    const double prob = pn * exp(-tau[0]);
    dummy.stokes[0] = I * prob;
    dummy.stokes[1] = Q * prob;
    dummy.stokes[2] = U * prob;
    for (int bin_range = 0; bin_range < v.p.nrange_grid; bin_range++)
      if (dummy.nu_rf > v.p.nu_grid_min[bin_range] && dummy.nu_rf < v.p.nu_grid_max[bin_range])
        if (t_arrive > v.p.tmin_grid && t_arrive < v.p.tmax_grid)
          add_to_vpkt_grid(c, v, &dummy, vel_vec, bin_range, bin, obs);
  }
}
// vpkt.cc:837-896.  The next_trans fix-up of vpkt.cc:853-858 only ever writes 0 over 0 and is omitted; the final
// calculate_kappa_rpkt_cont of the real packet restores per-thread state that deviation D2 does not keep.
void vpkt_call_estimators(const Ctx &c, Est &E, const artis_packet *p, double t_current, int realtype) {
  const VpktCfg &v = *c.vp;
  double vel_vec[3];
  get_velocity(p->pos, vel_vec, t_current);
  const int mgi = cell_mgi(c, p->where);
  if (mgi == npts_model(c) || c.cs->thick[mgi] != 0) return;
  thread_local ThreadCache vtc;
  if (vtc.pops.size() != (size_t)c.at->nlevels_total || vtc.kappa_bf_sum.size() != (size_t)c.at->nbfcontinua) {
    vtc = ThreadCache();
    vtc.pops.assign(c.at->nlevels_total, 0.);
    vtc.departureratios.assign(c.at->nbfcontinua, -1.);
    vtc.processrates.assign((size_t)c.at->nlevels_total * 9, -99.);
    vtc.corrphotoioncoeff.assign(1, -99.);
    vtc.cooling_contrib.assign(c.at->ncoolingterms, -99.);
    vtc.kappa_bf_sum.assign(c.at->nbfcontinua, 0.);
    vtc.groundcont_gamma_contr.assign(c.at->nbfcontinua_ground, 0.);
    vtc.gamma_contr.assign(c.at->nbfcontinua, 0.);
  }
  vtc.cellnumber = -99;  // the cell state may have changed since the last call
  for (int bin = 0; bin < v.p.nobs; bin++) {
    double obs[3] = {v.obs[3 * bin], v.obs[3 * bin + 1], v.obs[3 * bin + 2]};
    const double t_arrive = t_current - (dot(p->pos, obs) / ARTIS_CLIGHT_PROP);
    if (t_arrive >= v.p.tmin_vspec_input && t_arrive <= v.p.tmax_vspec_input) {
      for (int i = 0; i < v.p.nrange; i++) {
        if (p->nu_cmf / doppler_nucmf_on_nurf(c, obs, vel_vec) > v.p.numin_vspec_input[i] &&
            p->nu_cmf / doppler_nucmf_on_nurf(c, obs, vel_vec) < v.p.numax_vspec_input[i]) {
          rlc_emiss_vpkt(c, vtc, E, p, t_current, bin, obs, realtype);
        }
      }
    }
  }
}

// rpkt.cc:67-328
double get_event(const Ctx &c, ThreadCache &tc, int mgi, artis_packet *p, int *rpkt_eventtype, double tau_rnd,
                 double abort_dist) {
  double tau = 0.;
  double dist = 0.;
  double edist = 0.;
  artis_packet dummypkt_abort = *p;
  move_pkt_withtime(c, &dummypkt_abort, abort_dist / 2.);
  move_pkt_withtime(c, &dummypkt_abort, abort_dist / 2.);
  const double nu_cmf_abort = dummypkt_abort.nu_cmf;
  artis_packet dummypkt = *p;
  artis_packet *const dp = &dummypkt;
  calculate_kappa_rpkt_cont(c, tc, p);
  const double kap_cont = tc.kap_total * doppler_packet_nucmf_on_nurf(c, p);
  const artis_atomic_tables &a = *c.at;
  while (true) {
    const int lineindex = closest_transition(c, dp->nu_cmf, dp->next_trans);
    if (lineindex >= 0) {
      tc.work[WK_LINES_SCANNED]++;
      const double nu_trans = a.line_nu[lineindex];
      dp->next_trans = lineindex + 1;
      double ldist;
      if (dp->nu_cmf <= nu_trans) {
        ldist = 0;
      } else if (!c.rp.relativistic_doppler) {
        ldist = ARTIS_CLIGHT * dp->prop_time * (dp->nu_cmf / nu_trans - 1);
      } else {
        const double nu_r = nu_trans / dp->nu_rf;
        const double ct = ARTIS_CLIGHT * dp->prop_time;
        const double r = vec_len(dp->pos);
        const double mu = dot(dp->dir, dp->pos) / r;
        ldist = -mu * r + (ct - nu_r * nu_r * sqrt(ct * ct - (1 + r * r * (1 - mu * mu) * (1 + pow(nu_r, -2))))) /
                              (1 + nu_r * nu_r);
      }
      if (ldist < 0.) {
        if (!(ldist >= -100.)) {
          fprintf(stderr, "oracle: ldist %g < -100\n", ldist);
          abort();
        }
        ldist = 0.;
      }
      const double tau_cont = kap_cont * ldist;
      if (tau_rnd - tau > tau_cont) {
        if (nu_trans < nu_cmf_abort) {
          dp->next_trans -= 1;
          p->next_trans = dp->next_trans;
          return std::numeric_limits<double>::max();
        }
        const int element = a.line_elementindex[lineindex];
        const int ion = a.line_ionindex[lineindex];
        const int upper = a.line_upperlevelindex[lineindex];
        const int lower = a.line_lowerlevelindex[lineindex];
        const double A_ul = a.line_einstein_A[lineindex];
        const double B_ul = ARTIS_CLIGHTSQUAREDOVERTWOH / pow(nu_trans, 3) * A_ul;
        const double B_lu = stat_weight(c, element, ion, upper) / stat_weight(c, element, ion, lower) * B_ul;
        const double n_u = get_levelpop(tc, c, element, ion, upper);
        const double n_l = get_levelpop(tc, c, element, ion, lower);
        double tau_line = (B_lu * n_l - B_ul * n_u) * ARTIS_HCLIGHTOVERFOURPI * dp->prop_time;
        tc.work[WK_LINE_TAUS]++;
        if (tau_line < 0) tau_line = 0.;
        if (tau_rnd - tau > tau_cont + tau_line) {
          dist = dist + ldist;
          tau += tau_cont + tau_line;
          move_pkt_withtime(c, dp, ldist);
        } else {
          p->mastate.element = element;
          p->mastate.ion = ion;
          p->mastate.level = upper;
          p->mastate.activatingline = lineindex;
          edist = dist + ldist;
          if (edist >= abort_dist) edist = abort_dist * (1 - 2e-8);
          *rpkt_eventtype = ARTIS_RPKT_EVENTTYPE_BB;
          p->next_trans = dp->next_trans;
          return edist;
        }
      } else {
        edist = dist + (tau_rnd - tau) / kap_cont;
        dp->next_trans -= 1;
        *rpkt_eventtype = ARTIS_RPKT_EVENTTYPE_CONT;
        p->next_trans = dp->next_trans;
        return edist;
      }
    } else {
      dp->next_trans = a.nlines + 1;
      const double tau_cont = kap_cont * (abort_dist - dist);
      if (tau_rnd - tau > tau_cont) {
        edist = std::numeric_limits<double>::max();
      } else {
        edist = dist + (tau_rnd - tau) / kap_cont;
        *rpkt_eventtype = ARTIS_RPKT_EVENTTYPE_CONT;
      }
      p->next_trans = dp->next_trans;
      return edist;
    }
  }
}

// radfield.cc:764-829 update_bfestimators (DETAILED_BF_ESTIMATORS_ON, DETAILED_BF_ESTIMATORS_BYTYPE false)
void update_bfestimators(const Ctx &c, const ThreadCache &tc, Est &E, int mgi, double distance_e_cmf, double nu_cmf,
                         const artis_packet *p) {
  if (distance_e_cmf == 0) return;
  const int nbfcontinua = c.at->nbfcontinua;
  const double dopplerfactor = doppler_packet_nucmf_on_nurf(c, p);
  const double distance_e_cmf_over_nu = distance_e_cmf / nu_cmf * dopplerfactor;
  for (int allcontindex = 0; allcontindex < nbfcontinua; allcontindex++) {
    const double nu_edge = c.at->allcont_nu_edge[allcontindex];
    const double nu_max_phixs = nu_edge * c.at->last_phixs_nuovernuedge;
    if (nu_cmf >= nu_edge && nu_cmf <= nu_max_phixs) {
      safeadd(&E.e->bfrate_raw[(size_t)mgi * nbfcontinua + allcontindex],
              tc.gamma_contr[allcontindex] * distance_e_cmf_over_nu);
    } else if (nu_cmf < nu_edge) {
      break;
    }
  }
}

// rpkt.cc:557-621 + radfield.cc:831-876
void update_estimators(const Ctx &c, ThreadCache &tc, Est &E, const artis_packet *p, double distance) {
  const int mgi = cell_mgi(c, p->where);
  if (mgi == npts_model(c)) return;
  tc.work[WK_EST_SEGMENTS]++;
  const double distance_e_cmf = distance * p->e_cmf;
  const double nu = p->nu_cmf;
  safeadd(&E.e->J[mgi], distance_e_cmf);
  safeadd(&E.e->nuJ[mgi], distance_e_cmf * nu);
  if (c.rp.detailed_bf_estimators) update_bfestimators(c, tc, E, mgi, distance_e_cmf, nu, p);
  if (c.rp.multibin_radfield) {
    const int binindex = select_bin(c, nu);
    if (binindex >= 0) {
      const size_t mb = (size_t)mgi * c.at->radfield_nbins + binindex;
      safeadd(&E.e->radfield_J_raw[mb], distance_e_cmf);
      safeadd(&E.e->radfield_nuJ_raw[mb], distance_e_cmf * nu);
#pragma omp atomic update
      E.e->radfield_contribcount[mb] += 1;
    }
  }
  safeadd(&E.e->ffheatingestimator[mgi], distance_e_cmf * tc.kap_ffheating);
  // the ground-continuum estimators exist unless both NO_LUT_PHOTOION and NO_LUT_BFHEATING (rpkt.cc:573-614)
  if (c.rp.no_lut_photoion && c.rp.no_lut_bfheating) return;
  const double distance_e_cmf_over_nu = distance_e_cmf / nu;
  const artis_atomic_tables &a = *c.at;
  for (int i = 0; i < a.nbfcontinua_ground; i++) {
    const double nu_edge = a.groundcont_nu_edge[i];
    if (nu > nu_edge) {
      const int element = a.groundcont_element[i];
      if (c.cs->elem_abundance[(size_t)mgi * a.nelements + element] > 0) {
        const int ion = a.groundcont_ion[i];
        const size_t idx = (size_t)mgi * E.nelements * E.maxnions + element * E.maxnions + ion;
        if (!c.rp.no_lut_photoion)
          safeadd(&E.e->gammaestimator[idx], tc.groundcont_gamma_contr[i] * distance_e_cmf_over_nu);
        if (!c.rp.no_lut_bfheating)
          safeadd(&E.e->bfheatingestimator[idx], tc.groundcont_gamma_contr[i] * distance_e_cmf * (1. - nu_edge / nu));
        tc.work[WK_GC_UPDATES]++;
      }
    } else {
      break;
    }
  }
}

// rpkt.cc:330-447
void rpkt_event_continuum(const Ctx &c, ThreadCache &tc, Est &E, artis_rng *rng, artis_packet *p) {
  const double nu = p->nu_cmf;
  const double dopplerfactor = doppler_packet_nucmf_on_nurf(c, p);
  const double kappa_cont = tc.kap_total * dopplerfactor;
  const double sigma = tc.kap_es * dopplerfactor;
  const double kappa_ff = tc.kap_ff * dopplerfactor;
  const double kappa_bf = tc.kap_bf * dopplerfactor;
  const double zrand = artis_rng_uniform(rng);
  tc.work[WK_CONT_EVENTS]++;
  if (zrand * kappa_cont < sigma) {
    p->interactions += 1;
    p->nscatterings += 1;
    p->last_event = 12;
    counter_inc(E, CTR_ESCOUNTER);
    tc.work[WK_ES_SCAT]++;
    if (c.vp) {  // rpkt.cc:358-363
      p->last_cross = ARTIS_NONE;
      vpkt_call_estimators(c, E, p, p->prop_time, 1);
    }
    escat_rpkt(c, rng, p);
    vec_copy(p->em_pos, p->pos);
    p->em_time = (int)p->prop_time;
  } else if (zrand * kappa_cont < sigma + kappa_ff) {
    counter_inc(E, CTR_K_STAT_FROM_FF);
    p->interactions += 1;
    p->last_event = 5;
    p->type = ARTIS_TYPE_KPKT;
    p->absorptiontype = -1;
  } else if (zrand * kappa_cont < sigma + kappa_ff + kappa_bf) {
    p->absorptiontype = -2;
    const double kappa_bf_inrest = tc.kap_bf;
    const int nbf = c.at->nbfcontinua;
    const double zrand2 = artis_rng_uniform(rng);
    const double kappa_bf_rand = zrand2 * kappa_bf_inrest;
    // lower_bound over kappa_bf_sum[0 .. nbf-1)
    int lo = 0, hi = nbf - 1;
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (tc.kappa_bf_sum[mid] < kappa_bf_rand)
        lo = mid + 1;
      else
        hi = mid;
    }
    const int allcontindex = lo;
    const double nu_edge = c.at->allcont_nu_edge[allcontindex];
    const int element = c.at->allcont_element[allcontindex];
    const int ion = c.at->allcont_ion[allcontindex];
    const int level = c.at->allcont_level[allcontindex];
    const int phixstargetindex = c.at->allcont_phixstargetindex[allcontindex];
    const double zrand3 = artis_rng_uniform(rng);
    if (zrand3 < nu_edge / nu) {
      counter_inc(E, CTR_MA_STAT_ACTIVATION_BF);
      p->interactions += 1;
      p->last_event = 3;
      p->type = ARTIS_TYPE_MA;
      p->mastate.element = element;
      p->mastate.ion = ion + 1;
      p->mastate.level = get_phixsupperlevel(c, element, ion, level, phixstargetindex);
      p->mastate.activatingline = -99;
    } else {
      counter_inc(E, CTR_K_STAT_FROM_BF);
      p->interactions += 1;
      p->last_event = 4;
      p->type = ARTIS_TYPE_KPKT;
    }
  } else {
    fprintf(stderr, "oracle: ERROR: could not continuum process\n");
    abort();
  }
}
// rpkt.cc:449-489
void rpkt_event_boundbound(const Ctx &c, ThreadCache &tc, Est &E, artis_packet *p) {
  counter_inc(E, CTR_MA_STAT_ACTIVATION_BB);
  tc.work[WK_BB_EVENTS]++;
  p->interactions += 1;
  p->last_event = 1;
  p->absorptiontype = p->mastate.activatingline;
  p->absorptionfreq = p->nu_rf;
  p->absorptiondir[0] = p->dir[0];
  p->absorptiondir[1] = p->dir[1];
  p->absorptiondir[2] = p->dir[2];
  p->type = ARTIS_TYPE_MA;
  if (c.rp.record_linestat && E.e->acounter) {
#pragma omp atomic update
    E.e->acounter[p->next_trans - 1] += 1;
  }
}
// rpkt.cc:491-509
void rpkt_event_thickcell(const Ctx &c, Est &E, artis_rng *rng, artis_packet *p) {
  p->interactions += 1;
  p->nscatterings += 1;
  p->last_event = 12;
  counter_inc(E, CTR_ESCOUNTER);
  emitt_rpkt(c, rng, p);
  vec_copy(p->em_pos, p->pos);
  p->em_time = (int)p->prop_time;
}

// grey_emissivities.cc:79-122 rlc_emiss_rpkt: the rate at which grey opacity destroys (and re-creates) r-packets,
// called at the midpoint of every r-packet path segment when do_rlc_est is 1 or 2 (rpkt.cc:739-741, 769-771,
// 791-793).  kappagrey * rho is a float product, as grid::get_kappagrey / get_rho return floats.  An empty cell's
// slot (rpkt_emiss[npts_model], grid.cc:1700) only ever receives 0 (rho = 0) and is not part of the ABI array.
void rlc_emiss_rpkt(const Ctx &c, Est &E, const artis_packet *p, double dist) {
  const int mgi = cell_mgi(c, p->where);
  if (mgi == npts_model(c) || !E.e->rpkt_emiss) return;
  if (dist > 0.0) {
    double vel_vec[3];
    get_velocity(p->pos, vel_vec, p->prop_time);
    double cont = (c.cs->kappagrey[mgi] * c.cs->rho[mgi]);
    cont = cont * p->e_rf * dist * (1. - (2. * dot(vel_vec, p->dir) / ARTIS_CLIGHT));
    safeadd(&E.e->rpkt_emiss[mgi], 1.e-20 * cont);
  }
}

// rpkt.cc:623-813
bool do_rpkt_step(const Ctx &c, ThreadCache &tc, Est &E, artis_rng *rng, artis_packet *p, double t2) {
  const bool rlc = c.rp.do_rlc_est != 0 && c.rp.do_rlc_est != 3;
  const int cellindex = p->where;
  int mgi = cell_mgi(c, cellindex);
  const int oldmgi = mgi;
  const int npm = npts_model(c);
  tc.work[WK_RPKT_STEPS]++;
  const double zrand = artis_rng_uniform_pos(rng);
  const double tau_next = -1. * log(zrand);
  int snext;
  double sdist = boundary_cross(c, E, p, &snext);
  if (sdist == 0) {
    change_cell(E, p, snext);
    mgi = cell_mgi(c, p->where);
    return (p->type == ARTIS_TYPE_RPKT && (mgi == npm || mgi == oldmgi));
  }
  const double maxsdist = max_sdist(c, p, sdist);
  if (sdist > maxsdist) {
    fprintf(stderr, "oracle: [fatal] do_rpkt: Unreasonably large sdist for packet %d. %g %g %g\n", p->number,
            c.g->rmax, p->prop_time / c.g->tmin, sdist);
    abort();
  }
  if (((snext != -99) && (snext < 0)) || (snext >= c.g->ngrid)) {
    fprintf(stderr, "oracle: [fatal] r_pkt: Heading for inappropriate grid cell.\n");
    abort();
  }
  if (sdist > c.rp.max_path_step) {
    sdist = c.rp.max_path_step;
    snext = p->where;
  }
  const double tdist = (t2 - p->prop_time) * ARTIS_CLIGHT_PROP;
  if (!(tdist >= 0)) {
    fprintf(stderr, "oracle: tdist < 0\n");
    abort();
  }
  double edist;
  int rpkt_eventtype = -1;
  bool find_nextline = false;
  if (mgi == npm) {
    edist = std::numeric_limits<double>::max();
    find_nextline = true;
  } else if (c.cs->thick[mgi] == 1) {
    // D7: no continuum opacity is evaluated in a grey thick cell, so the estimator terms of this step use zero
    // (the reference uses whatever its thread computed last, rpkt.cc:583, 1166)
    tc.kap_total = tc.kap_es = tc.kap_ff = tc.kap_bf = tc.kap_ffheating = 0.;
    std::fill(tc.groundcont_gamma_contr.begin(), tc.groundcont_gamma_contr.end(), 0.);
    std::fill(tc.gamma_contr.begin(), tc.gamma_contr.end(), 0.);
    const double kappa = c.cs->kappagrey[mgi] * c.cs->rho[mgi] * doppler_packet_nucmf_on_nurf(c, p);
    edist = (tau_next - 0.0) / kappa;
    find_nextline = true;
  } else {
    edist = get_event(c, tc, mgi, p, &rpkt_eventtype, tau_next, fmin(tdist, sdist));
  }
  if (!(edist >= 0)) {
    fprintf(stderr, "oracle: edist < 0\n");
    abort();
  }
  if ((sdist < tdist) && (sdist < edist)) {
    move_pkt_withtime(c, p, sdist / 2.);
    update_estimators(c, tc, E, p, sdist);
    if (rlc) rlc_emiss_rpkt(c, E, p, sdist);
    move_pkt_withtime(c, p, sdist / 2.);
    if (snext != p->where) {
      change_cell(E, p, snext);
      mgi = cell_mgi(c, p->where);
    }
    p->scat_count = 0;
    p->last_event = p->last_event + 100;
    if (find_nextline) {
      if (mgi != npm && c.cs->thick[mgi] != 1) closest_transition_empty(c, p);
    }
    return (p->type == ARTIS_TYPE_RPKT && (mgi == npm || mgi == oldmgi));
  } else if ((edist < sdist) && (edist < tdist)) {
    move_pkt_withtime(c, p, edist / 2.);
    update_estimators(c, tc, E, p, edist);
    if (rlc) rlc_emiss_rpkt(c, E, p, edist);
    move_pkt_withtime(c, p, edist / 2.);
    if (c.cs->thick[mgi] == 1)
      rpkt_event_thickcell(c, E, rng, p);
    else if (rpkt_eventtype == ARTIS_RPKT_EVENTTYPE_BB)
      rpkt_event_boundbound(c, tc, E, p);
    else if (rpkt_eventtype == ARTIS_RPKT_EVENTTYPE_CONT)
      rpkt_event_continuum(c, tc, E, rng, p);
    else {
      fprintf(stderr, "oracle: bad event type\n");
      abort();
    }
    return (p->type == ARTIS_TYPE_RPKT && (mgi == npm || mgi == oldmgi));
  } else if ((tdist < sdist) && (tdist < edist)) {
    move_pkt_withtime(c, p, tdist / 2.);
    update_estimators(c, tc, E, p, tdist);
    if (rlc) rlc_emiss_rpkt(c, E, p, tdist);
    p->prop_time = t2;
    move_pkt(c, p, tdist / 2.);
    p->last_event = p->last_event + 1000;
    if (find_nextline) closest_transition_empty(c, p);
    return false;
  }
  fprintf(stderr, "oracle: [fatal] do_rpkt: Failed to identify event. edist %g, sdist %g, tdist %g pkt %d\n", edist,
          sdist, tdist, p->number);
  abort();
}

// --------------------------------------------------------------------------------------- non-thermal ionisation
// nonthermal.cc:1640-1655
int nt_ionisation_maxupperion(const Ctx &c, int e, int lowerion) {
  const int nions = get_nions(c, e);
  int maxupper = lowerion + 1;
  if (c.rp.nt_solve_spencerfano) maxupper = lowerion + 1 + c.rp.nt_max_auger_electrons;
  if (maxupper > nions - 1) maxupper = nions - 1;
  return maxupper;
}
// nonthermal.cc:1584-1635 (prob_num_auger / ionenfrac_num_auger of the cell's Spencer-Fano solution)
double nt_ionization_upperion_probability(const Ctx &c, int mgi, int e, int lowerion, int upperion, bool energyweighted) {
  const int A = c.rp.nt_max_auger_electrons;
  if (c.rp.nt_solve_spencerfano && A > 0) {
    const int numaugerelec = upperion - lowerion - 1;
    const size_t base = ((size_t)mgi * c.at->nions_total + uion(c, e, lowerion)) * (A + 1);
    const float *tab = energyweighted ? c.cs->nt_ionenfrac_num_auger : c.cs->nt_prob_num_auger;
    if (numaugerelec < A) return tab[base + numaugerelec];
    if (numaugerelec == A) {
      double prob_remaining = 1.;
      for (int k = 0; k < A; k++) prob_remaining -= tab[base + k];
      return prob_remaining;
    }
    return 0.;
  }
  return (upperion == lowerion + 1) ? 1.0 : 0.;
}
// nonthermal.cc:1657-1682
int nt_random_upperion(const Ctx &c, artis_rng *rng, int mgi, int e, int lowerion, bool energyweighted) {
  if (c.rp.nt_solve_spencerfano && c.rp.nt_max_auger_electrons > 0) {
    for (int attempt = 0; attempt < 1000; attempt++) {
      const double zrand = artis_rng_uniform(rng);
      double prob_sum = 0.;
      for (int upperion = lowerion + 1; upperion <= nt_ionisation_maxupperion(c, e, lowerion); upperion++) {
        prob_sum += nt_ionization_upperion_probability(c, mgi, e, lowerion, upperion, energyweighted);
        if (zrand <= prob_sum) return upperion;
      }
    }
    fprintf(stderr, "oracle: nt_random_upperion: probabilities do not sum to one\n");
    abort();
  }
  return lowerion + 1;
}
// nonthermal.cc:1827-1845
double ion_ntion_energyrate(const Ctx &c, int mgi, int e, int lowerion) {
  const double nnlowerion = ionstagepop(c, mgi, e, lowerion);
  double enrate = 0.;
  for (int upperion = lowerion + 1; upperion <= nt_ionisation_maxupperion(c, e, lowerion); upperion++) {
    const double upperionprobfrac = nt_ionization_upperion_probability(c, mgi, e, lowerion, upperion, false);
    const double epsilon_trans = epsilon(c, e, upperion, 0) - epsilon(c, e, lowerion, 0);
    enrate += nnlowerion * upperionprobfrac * epsilon_trans;
  }
  const double gamma_nt = c.cs->nt_ionization_ratecoeff[(size_t)mgi * c.at->nions_total + uion(c, e, lowerion)];
  return gamma_nt * enrate;
}
// nonthermal.cc:1847-1856
double get_ntion_energyrate(const Ctx &c, int mgi) {
  double ratetotal = 0.;
  for (int e = 0; e < c.at->nelements; e++)
    for (int lowerion = 0; lowerion < get_nions(c, e) - 1; lowerion++) ratetotal += ion_ntion_energyrate(c, mgi, e, lowerion);
  return ratetotal;
}
// nonthermal.cc:1858-1875
void select_nt_ionization2(const Ctx &c, artis_rng *rng, int mgi, int *element, int *lowerion) {
  const double ratetotal = get_ntion_energyrate(c, mgi);
  const double zrand = artis_rng_uniform(rng);
  double ratesum = 0.;
  for (int e = 0; e < c.at->nelements; e++)
    for (int li = 0; li < get_nions(c, e) - 1; li++) {
      ratesum += ion_ntion_energyrate(c, mgi, e, li);
      if (ratesum >= zrand * ratetotal) {
        *element = e;
        *lowerion = li;
        return;
      }
    }
  fprintf(stderr, "oracle: select_nt_ionization2 failed\n");
  abort();
}

// ---------------------------------------------------------------------------------------------- macro-atom
// macroatom.cc:57-159
void calculate_macroatom_transitionrates(const Ctx &c, ThreadCache &tc, int mgi, int e, int i, int l, double t_mid) {
  const int ul = ulev(c, e, i, l);
  double *processrates = &tc.processrates[(size_t)ul * 9];
  const float T_e = c.cs->Te[mgi];
  const float nne = c.cs->nne[mgi];
  const double epsilon_current = epsilon(c, e, i, l);
  const double statweight = stat_weight(c, e, i, l);
  const artis_atomic_tables &a = *c.at;
  processrates[ARTIS_MA_ACTION_RADDEEXC] = 0.;
  processrates[ARTIS_MA_ACTION_COLDEEXC] = 0.;
  processrates[ARTIS_MA_ACTION_INTERNALDOWNSAME] = 0.;
  const int ndowntrans = a.level_ndowntrans[ul];
  const int doff = a.level_downtrans_offset[ul];
  for (int k = 0; k < ndowntrans; k++) {
    const int lineindex = a.downtrans_lineindex[doff + k];
    const int lower = a.line_lowerlevelindex[lineindex];
    const double epsilon_target = epsilon(c, e, i, lower);
    const double epsilon_trans = epsilon_current - epsilon_target;
    const double R = rad_deexcitation_ratecoeff(c, tc, e, i, l, lower, epsilon_trans, lineindex, t_mid);
    const double C = col_deexcitation_ratecoeff(c, T_e, nne, epsilon_trans, lineindex, stat_weight(c, e, i, lower),
                                                statweight);
    const double individ_internal_down_same = (R + C) * epsilon_target;
    const double individ_rad_deexc = R * epsilon_trans;
    const double individ_col_deexc = C * epsilon_trans;
    processrates[ARTIS_MA_ACTION_RADDEEXC] += individ_rad_deexc;
    processrates[ARTIS_MA_ACTION_COLDEEXC] += individ_col_deexc;
    processrates[ARTIS_MA_ACTION_INTERNALDOWNSAME] += individ_internal_down_same;
    tc.individ_rad_deexc[doff + k] = individ_rad_deexc;
    tc.individ_internal_down_same[doff + k] = individ_internal_down_same;
  }
  tc.work[WK_MA_TRANS] += ndowntrans;
  processrates[ARTIS_MA_ACTION_RADRECOMB] = 0.;
  processrates[ARTIS_MA_ACTION_COLRECOMB] = 0.;
  processrates[ARTIS_MA_ACTION_INTERNALDOWNLOWER] = 0.;
  if (i > 0 && l <= get_maxrecombininglevel(c, e, i)) {
    const int nlevels = get_ionisinglevels(c, e, i - 1);
    for (int lower = 0; lower < nlevels; lower++) {
      const double epsilon_target = epsilon(c, e, i - 1, lower);
      const double epsilon_trans = epsilon_current - epsilon_target;
      const double R = rad_recombination_ratecoeff(c, T_e, nne, e, i, l, lower);
      const double C = col_recombination_ratecoeff(c, mgi, e, i, l, lower, epsilon_trans);
      processrates[ARTIS_MA_ACTION_INTERNALDOWNLOWER] += (R + C) * epsilon_target;
      processrates[ARTIS_MA_ACTION_RADRECOMB] += R * epsilon_trans;
      processrates[ARTIS_MA_ACTION_COLRECOMB] += C * epsilon_trans;
    }
    tc.work[WK_MA_TRANS] += nlevels;
  }
  processrates[ARTIS_MA_ACTION_INTERNALUPSAME] = 0.;
  const int nuptrans = a.level_nuptrans[ul];
  const int uoff = a.level_uptrans_offset[ul];
  for (int k = 0; k < nuptrans; k++) {
    const int lineindex = a.uptrans_lineindex[uoff + k];
    const int upper = a.line_upperlevelindex[lineindex];
    const double epsilon_trans = epsilon(c, e, i, upper) - epsilon_current;
    const double R = rad_excitation_ratecoeff(c, tc, mgi, e, i, l, upper, epsilon_trans, lineindex, t_mid);
    const double C = col_excitation_ratecoeff(c, T_e, nne, lineindex, epsilon_trans, statweight,
                                              stat_weight(c, e, i, upper));
    const double NT = 0.;  // nonthermal.cc:1746-1750 (NT_EXCITATION_ON false)
    const double individ_internal_up_same = (R + C + NT) * epsilon_current;
    processrates[ARTIS_MA_ACTION_INTERNALUPSAME] += individ_internal_up_same;
    tc.individ_internal_up_same[uoff + k] = individ_internal_up_same;
  }
  tc.work[WK_MA_TRANS] += nuptrans;
  processrates[ARTIS_MA_ACTION_INTERNALUPHIGHERNT] = 0.;
  processrates[ARTIS_MA_ACTION_INTERNALUPHIGHER] = 0.;
  const int ionisinglevels = get_ionisinglevels(c, e, i);
  if (i < get_nions(c, e) - 1 && l < ionisinglevels) {
    if (c.rp.nt_on)  // macroatom.cc:143-146, nonthermal.cc:1684-1712 (the host's nt_ionization_ratecoeff)
      processrates[ARTIS_MA_ACTION_INTERNALUPHIGHERNT] =
          c.cs->nt_ionization_ratecoeff[(size_t)mgi * a.nions_total + uion(c, e, i)] * epsilon_current;
    for (int t = 0; t < get_nphixstargets(c, e, i, l); t++) {
      const double epsilon_trans = get_phixs_threshold(c, e, i, l, t);
      const double R = get_corrphotoioncoeff(c, tc, e, i, l, t, mgi);
      const double C = col_ionization_ratecoeff(c, T_e, nne, e, i, l, t, epsilon_trans);
      processrates[ARTIS_MA_ACTION_INTERNALUPHIGHER] += (R + C) * epsilon_current;
    }
  }
}

// macroatom.cc:416-482
void do_macroatom(const Ctx &c, ThreadCache &tc, Est &E, artis_rng *rng, artis_packet *p, int timestep) {
  const double t_mid = c.g->ts_mid[timestep];
  const int mgi = cell_mgi(c, p->where);
  const float T_e = c.cs->Te[mgi];
  const float nne = c.cs->nne[mgi];
  const artis_atomic_tables &a = *c.at;
  if (c.cs->thick[mgi] == 1) {
    fprintf(stderr, "oracle: macroatom in thick cell\n");
    abort();
  }
  const int element = p->mastate.element;
  int ion = p->mastate.ion;
  int level = p->mastate.level;
  const int activatingline = p->mastate.activatingline;
  bool end_packet = false;
  while (!end_packet) {
    tc.work[WK_MA_JUMPS]++;
    const double epsilon_current = epsilon(c, element, ion, level);
    const int ul = ulev(c, element, ion, level);
    const int nuptrans = a.level_nuptrans[ul];
    double *processrates = &tc.processrates[(size_t)ul * 9];
    if (processrates[ARTIS_MA_ACTION_COLDEEXC] < 0)
      calculate_macroatom_transitionrates(c, tc, mgi, element, ion, level, t_mid);
    double total_transitions = 0.;
    for (int action = 0; action < ARTIS_MA_ACTION_COUNT; action++) total_transitions += processrates[action];
    int selected_action = ARTIS_MA_ACTION_COUNT;
    // the jump's action draw and transition draw come from one Philox block (include/artis_rng.h
    // artis_rng_jump_pair); each advances the counter by one as it is taken
    double zrand, zpair;
    artis_rng_jump_pair(rng, &zrand, &zpair);
    rng->n++;
    auto transition_draw = [&]() {
      rng->n++;
      return zpair;
    };
    const double randomrate = zrand * total_transitions;
    double rate = 0.;
    for (int action = 0; action < ARTIS_MA_ACTION_COUNT; action++) {
      rate += processrates[action];
      if (rate > randomrate) {
        selected_action = action;
        break;
      }
    }
    if (rate <= randomrate) {
      fprintf(stderr, "oracle: [fatal] do_ma: problem with random numbers .. abort (pkt %d Z idx %d ion %d lvl %d)\n",
              p->number, element, ion, level);
      abort();
    }
    switch (selected_action) {
      case ARTIS_MA_ACTION_RADDEEXC: {
        // macroatom.cc:222-296
        const double zr = transition_draw();
        double r = 0.;
        int linelistindex = -99;
        const int ndowntrans = a.level_ndowntrans[ul];
        const int doff = a.level_downtrans_offset[ul];
        for (int k = 0; k < ndowntrans; k++) {
          r += tc.individ_rad_deexc[doff + k];
          if (zr * processrates[ARTIS_MA_ACTION_RADDEEXC] < r) {
            linelistindex = a.downtrans_lineindex[doff + k];
            break;
          }
        }
        if (linelistindex < 0) {
          fprintf(stderr, "oracle: [fatal] problem in selecting radiative downward transition of MA\n");
          abort();
        }
        if (c.rp.record_linestat && E.e->ecounter) {
#pragma omp atomic update
          E.e->ecounter[linelistindex] += 1;
        }
        const int lower = a.line_lowerlevelindex[linelistindex];
        const double epsilon_trans = epsilon(c, element, ion, level) - epsilon(c, element, ion, lower);
        double oldnucmf = 0.;
        if (p->last_event == 1) oldnucmf = p->nu_cmf;
        p->nu_cmf = epsilon_trans / ARTIS_H;
        if (p->last_event == 1) {
          if (oldnucmf < p->nu_cmf)
            counter_inc(E, CTR_UPSCATTER);
          else
            counter_inc(E, CTR_DOWNSCATTER);
        }
        counter_inc(E, CTR_MA_STAT_DEACTIVATION_BB);
        p->interactions += 1;
        p->last_event = 0;
        emitt_rpkt(c, rng, p);
        if (linelistindex == activatingline) counter_inc(E, CTR_RESONANCESCATTERINGS);
        p->next_trans = linelistindex + 1;
        p->emissiontype = linelistindex;
        vec_copy(p->em_pos, p->pos);
        p->em_time = (int)p->prop_time;
        p->nscatterings = 0;
        if (c.vp) vpkt_call_estimators(c, E, p, p->prop_time, 3);  // macroatom.cc:292-295
        end_packet = true;
        break;
      }
      case ARTIS_MA_ACTION_COLDEEXC: {
        counter_inc(E, CTR_MA_STAT_DEACTIVATION_COLLDEEXC);
        p->interactions += 1;
        p->last_event = 10;
        p->type = ARTIS_TYPE_KPKT;
        end_packet = true;
        safeadd(&E.e->colheatingestimator[mgi], p->e_cmf);
        break;
      }
      case ARTIS_MA_ACTION_INTERNALDOWNSAME: {
        // macroatom.cc:174-220
        p->interactions += 1;
        const double zr = transition_draw();
        int lower = -99;
        double r = 0.;
        const int ndowntrans = a.level_ndowntrans[ul];
        const int doff = a.level_downtrans_offset[ul];
        for (int k = 0; k < ndowntrans; k++) {
          r += tc.individ_internal_down_same[doff + k];
          if (zr * processrates[ARTIS_MA_ACTION_INTERNALDOWNSAME] < r) {
            lower = a.line_lowerlevelindex[a.downtrans_lineindex[doff + k]];
            break;
          }
        }
        level = lower;
        break;
      }
      case ARTIS_MA_ACTION_RADRECOMB: {
        // macroatom.cc:298-380
        const int upperion = ion;
        const int upperionlevel = level;
        const double zr = transition_draw();
        double r = 0;
        const int nlevels = get_ionisinglevels(c, element, upperion - 1);
        int lower = 0;
        for (lower = 0; lower < nlevels; lower++) {
          const double epsilon_trans = epsilon_current - epsilon(c, element, upperion - 1, lower);
          const double R = rad_recombination_ratecoeff(c, T_e, nne, element, upperion, upperionlevel, lower);
          r += R * epsilon_trans;
          if (zr * processrates[ARTIS_MA_ACTION_RADRECOMB] < r) break;
        }
        tc.work[WK_MA_TRANS] += lower + 1;
        if (zr * processrates[ARTIS_MA_ACTION_RADRECOMB] >= r) {
          fprintf(stderr, "oracle: could not select lower level to recombine to\n");
          abort();
        }
        ion = upperion - 1;
        level = lower;
        p->nu_cmf = select_continuum_nu(c, rng, element, upperion - 1, lower, upperionlevel, T_e);
        if (!std::isfinite(p->nu_cmf)) {
          fprintf(stderr, "oracle: rad recombination of MA: selected frequency not finite\n");
          abort();
        }
        counter_inc(E, CTR_MA_STAT_DEACTIVATION_FB);
        p->interactions += 1;
        p->last_event = 2;
        emitt_rpkt(c, rng, p);
        p->next_trans = 0;
        p->emissiontype = get_continuumindex(c, element, ion, lower, upperionlevel);
        vec_copy(p->em_pos, p->pos);
        p->em_time = (int)p->prop_time;
        p->nscatterings = 0;
        if (c.vp) vpkt_call_estimators(c, E, p, p->prop_time, 3);  // macroatom.cc:376-379
        end_packet = true;
        break;
      }
      case ARTIS_MA_ACTION_COLRECOMB: {
        counter_inc(E, CTR_MA_STAT_DEACTIVATION_COLLRECOMB);
        p->interactions += 1;
        p->last_event = 11;
        p->type = ARTIS_TYPE_KPKT;
        end_packet = true;
        safeadd(&E.e->colheatingestimator[mgi], p->e_cmf);
        break;
      }
      case ARTIS_MA_ACTION_INTERNALDOWNLOWER: {
        p->interactions += 1;
        counter_inc(E, CTR_MA_STAT_INTERNALDOWNLOWER);
        zrand = transition_draw();
        rate = 0.;
        const int nlevels = get_ionisinglevels(c, element, ion - 1);
        int lower;
        for (lower = 0; lower < nlevels; lower++) {
          const double epsilon_target = epsilon(c, element, ion - 1, lower);
          const double epsilon_trans = epsilon_current - epsilon_target;
          const double R = rad_recombination_ratecoeff(c, T_e, nne, element, ion, level, lower);
          const double C = col_recombination_ratecoeff(c, mgi, element, ion, level, lower, epsilon_trans);
          rate += (R + C) * epsilon_target;
          if (zrand * processrates[ARTIS_MA_ACTION_INTERNALDOWNLOWER] < rate) break;
        }
        tc.work[WK_MA_TRANS] += lower + 1;
        ion -= 1;
        level = lower;
        if (lower >= nlevels) {
          fprintf(stderr, "oracle: internal_down_lower abort\n");
          abort();
        }
        break;
      }
      case ARTIS_MA_ACTION_INTERNALUPSAME: {
        p->interactions += 1;
        zrand = transition_draw();
        int upper = -99;
        rate = 0.;
        const int uoff = a.level_uptrans_offset[ul];
        for (int k = 0; k < nuptrans; k++) {
          rate += tc.individ_internal_up_same[uoff + k];
          if (zrand * processrates[ARTIS_MA_ACTION_INTERNALUPSAME] < rate) {
            upper = a.line_upperlevelindex[a.uptrans_lineindex[uoff + k]];
            break;
          }
        }
        level = upper;
        break;
      }
      case ARTIS_MA_ACTION_INTERNALUPHIGHER: {
        // macroatom.cc:382-414
        p->interactions += 1;
        counter_inc(E, CTR_MA_STAT_INTERNALUPHIGHER);
        int upper = -1;
        const double zr = transition_draw();
        double r = 0.;
        for (int t = 0; t < get_nphixstargets(c, element, ion, level); t++) {
          upper = get_phixsupperlevel(c, element, ion, level, t);
          const double epsilon_trans = get_phixs_threshold(c, element, ion, level, t);
          const double R = get_corrphotoioncoeff(c, tc, element, ion, level, t, mgi);
          const double C = col_ionization_ratecoeff(c, T_e, nne, element, ion, level, t, epsilon_trans);
          r += (R + C) * epsilon_current;
          if (zr * processrates[ARTIS_MA_ACTION_INTERNALUPHIGHER] < r) break;
        }
        if (zr * processrates[ARTIS_MA_ACTION_INTERNALUPHIGHER] >= r) {
          fprintf(stderr, "oracle: could not select upper level to ionise to\n");
          abort();
        }
        ion += 1;
        level = upper;
        break;
      }
      case ARTIS_MA_ACTION_INTERNALUPHIGHERNT: {
        // macroatom.cc:866-884
        p->interactions += 1;
        ion = nt_random_upperion(c, rng, mgi, element, ion, false);
        level = 0;
        counter_inc(E, CTR_MA_STAT_INTERNALUPHIGHERNT);
        break;
      }
      default: {
        fprintf(stderr, "oracle: ERROR: Problem selecting MA_ACTION %d\n", selected_action);
        abort();
      }
    }
  }
  if (p->trueemissiontype < 0) {
    p->trueemissiontype = p->emissiontype;
    p->trueemissionvelocity = (float)(vec_len(p->em_pos) / p->em_time);
    p->trueem_time = p->em_time;
  }
}

// ------------------------------------------------------------------------------------------------- k-packets
// kpkt.cc:167-308
void calculate_kpkt_rates_ion(const Ctx &c, ThreadCache &tc, int mgi, int e, int i, int indexionstart,
                              double oldcoolingsum) {
  const float nne = c.cs->nne[mgi];
  const float T_e = c.cs->Te[mgi];
  double contrib = oldcoolingsum;
  int idx = indexionstart;
  const int nions = get_nions(c, e);
  const int nlevels_currention = get_nlevels(c, e, i);
  const int ionisinglevels = get_ionisinglevels(c, e, i);
  const double nncurrention = ionstagepop(c, mgi, e, i);
  const artis_atomic_tables &a = *c.at;
  const int ioncharge = get_ionstage(c, e, i) - 1;
  if (ioncharge > 0) {
    const double C = 1.426e-27 * sqrt((double)T_e) * pow(ioncharge, 2) * nncurrention * nne;
    contrib += C;
    tc.cooling_contrib[idx] = contrib;
    idx++;
  }
  for (int level = 0; level < nlevels_currention; level++) {
    const double epsilon_current = epsilon(c, e, i, level);
    const double nnlevel = get_levelpop(tc, c, e, i, level);
    const double statweight = stat_weight(c, e, i, level);
    const int ul = ulev(c, e, i, level);
    const int nuptrans = a.level_nuptrans[ul];
    if (nuptrans > 0) {
      for (int ii = 0; ii < nuptrans; ii++) {
        const int li = a.uptrans_lineindex[a.level_uptrans_offset[ul] + ii];
        const int upper = a.line_upperlevelindex[li];
        const double epsilon_trans = epsilon(c, e, i, upper) - epsilon_current;
        const double C = nnlevel *
                         col_excitation_ratecoeff(c, T_e, nne, li, epsilon_trans, statweight,
                                                  stat_weight(c, e, i, upper)) *
                         epsilon_trans;
        contrib += C;
      }
      tc.cooling_contrib[idx] = contrib;
      idx++;
    }
    if (i < (nions - 1) && level < ionisinglevels) {
      const int nt = get_nphixstargets(c, e, i, level);
      for (int t = 0; t < nt; t++) {
        const int upper = get_phixsupperlevel(c, e, i, level, t);
        const double epsilon_upper = epsilon(c, e, i + 1, upper);
        const double epsilon_trans = epsilon_upper - epsilon_current;
        const double C = nnlevel * col_ionization_ratecoeff(c, T_e, nne, e, i, level, t, epsilon_trans) * epsilon_trans;
        contrib += C;
        tc.cooling_contrib[idx] = contrib;
        idx++;
      }
      for (int t = 0; t < nt; t++) {
        const double nnupperion = ionstagepop(c, mgi, e, i + 1);
        const double C = get_bfcoolingcoeff(c, e, i, level, t, T_e) * nnupperion * nne;
        contrib += C;
        tc.cooling_contrib[idx] = contrib;
        idx++;
      }
    }
  }
}

// kpkt.cc:428-446
double sample_planck(const Ctx &c, artis_rng *rng, double T) {
  const double nu_peak = 5.879e10 * T;
  const double B_peak = dbb(nu_peak, T, 1);
  while (true) {
    const double zrand = artis_rng_uniform(rng);
    const double zrand2 = artis_rng_uniform(rng);
    const double nu = c.g->nu_min_r + zrand * (c.g->nu_max_r - c.g->nu_min_r);
    if (zrand2 * B_peak <= dbb(nu, T, 1)) return nu;
  }
}
// kpkt.cc:448-475
void do_kpkt_bb(const Ctx &c, Est &E, artis_rng *rng, artis_packet *p) {
  const int mgi = cell_mgi(c, p->where);
  const float T_e = c.cs->Te[mgi];
  p->nu_cmf = sample_planck(c, rng, T_e);
  emitt_rpkt(c, rng, p);
  p->next_trans = 0;
  counter_inc(E, CTR_K_STAT_TO_R_BB);
  p->interactions++;
  p->last_event = 6;
  p->emissiontype = -9999999;
  vec_copy(p->em_pos, p->pos);
  p->em_time = (int)p->prop_time;
  p->nscatterings = 0;
}
// kpkt.cc:477-797
void do_kpkt(const Ctx &c, ThreadCache &tc, Est &E, artis_rng *rng, artis_packet *p, double t2, int nts) {
  const double t1 = p->prop_time;
  const int mgi = cell_mgi(c, p->where);
  const float T_e = c.cs->Te[mgi];
  const artis_atomic_tables &a = *c.at;
  tc.work[WK_KPKT]++;
  double deltat = 0.;
  if (nts < c.rp.n_kpktdiffusion_timesteps) deltat = c.rp.kpktdiffusion_timescale * c.g->ts_width[nts];
  const double t_current = t1 + deltat;
  if (t_current <= t2) {
    vec_scale(p->pos, t_current / t1);
    p->prop_time = t_current;
    double coolingsum = 0.;
    double zrand = artis_rng_uniform(rng);
    const double rndcool = zrand * c.cs->totalcooling[mgi];
    double oldcoolingsum = 0.;
    int element = -1, ion = -1;
    for (element = 0; element < a.nelements; element++) {
      const int nions = get_nions(c, element);
      for (ion = 0; ion < nions; ion++) {
        oldcoolingsum = coolingsum;
        coolingsum += c.cs->cooling_contrib_ion[(size_t)mgi * a.nions_total + uion(c, element, ion)];
        if (coolingsum > rndcool) break;
      }
      if (coolingsum > rndcool) break;
    }
    if (element >= a.nelements || ion >= get_nions(c, element)) {
      fprintf(stderr, "oracle: do_kpkt: problem selecting a cooling process\n");
      abort();
    }
    const int ui = uion(c, element, ion);
    const int ilow = a.ion_coolingoffset[ui];
    const int ihigh = ilow + a.ion_ncoolingterms[ui] - 1;
    if (tc.cooling_contrib[ilow] < 0.) calculate_kpkt_rates_ion(c, tc, mgi, element, ion, ilow, oldcoolingsum);
    // lower_bound over cooling_contrib[ilow .. ihigh+1)
    int lo = ilow, hi = ihigh + 1;
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (tc.cooling_contrib[mid] < rndcool)
        lo = mid + 1;
      else
        hi = mid;
    }
    int icool = lo;
    if (icool > ihigh) icool = ihigh;  // deviation D6
    tc.work[WK_KPKT_TERMS] += icool - ilow + 1;
    const int ctype = a.coolinglist_type[icool];
    if (ctype == ARTIS_COOLINGTYPE_FF) {
      zrand = artis_rng_uniform_pos(rng);
      p->nu_cmf = -ARTIS_KB * T_e / ARTIS_H * log(zrand);
      emitt_rpkt(c, rng, p);
      p->next_trans = 0;
      counter_inc(E, CTR_K_STAT_TO_R_FF);
      p->interactions += 1;
      p->last_event = 6;
      p->emissiontype = -9999999;
      vec_copy(p->em_pos, p->pos);
      p->em_time = (int)p->prop_time;
      p->nscatterings = 0;
      if (c.vp) vpkt_call_estimators(c, E, p, t_current, 2);  // kpkt.cc:631-634
    } else if (ctype == ARTIS_COOLINGTYPE_FB) {
      const int el = a.coolinglist_element[icool];
      const int lowerion = a.coolinglist_ion[icool];
      const int level = a.coolinglist_level[icool];
      const int upper = a.coolinglist_upperlevel[icool];
      p->nu_cmf = select_continuum_nu(c, rng, el, lowerion, level, upper, T_e);
      emitt_rpkt(c, rng, p);
      p->next_trans = 0;
      counter_inc(E, CTR_K_STAT_TO_R_FB);
      p->interactions += 1;
      p->last_event = 7;
      p->emissiontype = get_continuumindex(c, el, lowerion, level, upper);
      p->trueemissiontype = p->emissiontype;
      vec_copy(p->em_pos, p->pos);
      p->em_time = (int)p->prop_time;
      p->nscatterings = 0;
      if (c.vp) vpkt_call_estimators(c, E, p, t_current, 2);  // kpkt.cc:691-694
    } else if (ctype == ARTIS_COOLINGTYPE_COLLEXC) {
      const float nne = c.cs->nne[mgi];
      const double contrib_low = (icool > ilow) ? tc.cooling_contrib[icool - 1] : oldcoolingsum;
      double contrib = contrib_low;
      const int level = a.coolinglist_level[icool];
      const double epsilon_current = epsilon(c, element, ion, level);
      const double nnlevel = get_levelpop(tc, c, element, ion, level);
      const double statweight = stat_weight(c, element, ion, level);
      int upper = -1;
      const int ul = ulev(c, element, ion, level);
      const int nuptrans = a.level_nuptrans[ul];
      for (int ii = 0; ii < nuptrans; ii++) {
        const int li = a.uptrans_lineindex[a.level_uptrans_offset[ul] + ii];
        const int tmpupper = a.line_upperlevelindex[li];
        const double epsilon_trans = epsilon(c, element, ion, tmpupper) - epsilon_current;
        const double C = nnlevel *
                         col_excitation_ratecoeff(c, T_e, nne, li, epsilon_trans, statweight,
                                                  stat_weight(c, element, ion, tmpupper)) *
                         epsilon_trans;
        contrib += C;
        if (contrib >= rndcool) {
          upper = tmpupper;
          break;
        }
      }
      if (upper < 0 && nuptrans > 0) {
        // deviation D6: the update_grid ion total exceeded the re-summed terms in the last bits
        upper = a.line_upperlevelindex[a.uptrans_lineindex[a.level_uptrans_offset[ul] + nuptrans - 1]];
      }
      if (upper < 0) {
        fprintf(stderr, "oracle: WARNING: Could not select an upper level. pkt %d\n", p->number);
        abort();
      }
      p->mastate.element = element;
      p->mastate.ion = ion;
      p->mastate.level = upper;
      p->mastate.activatingline = -99;
      p->type = ARTIS_TYPE_MA;
      counter_inc(E, CTR_MA_STAT_ACTIVATION_COLLEXC);
      counter_inc(E, CTR_K_STAT_TO_MA_COLLEXC);
      p->interactions += 1;
      p->last_event = 8;
      p->trueemissiontype = -1;
      p->trueemissionvelocity = -1;
    } else if (ctype == ARTIS_COOLINGTYPE_COLLION) {
      p->mastate.element = a.coolinglist_element[icool];
      p->mastate.ion = a.coolinglist_ion[icool] + 1;
      p->mastate.level = a.coolinglist_upperlevel[icool];
      p->mastate.activatingline = -99;
      p->type = ARTIS_TYPE_MA;
      counter_inc(E, CTR_MA_STAT_ACTIVATION_COLLION);
      counter_inc(E, CTR_K_STAT_TO_MA_COLLION);
      p->interactions += 1;
      p->last_event = 9;
      p->trueemissiontype = -1;
      p->trueemissionvelocity = -1;
    } else {
      fprintf(stderr, "oracle: [fatal] do_kpkt: coolinglist.type mismatch\n");
      abort();
    }
  } else {
    vec_scale(p->pos, t2 / t1);
    p->prop_time = t2;
  }
}

// ------------------------------------------------------------------------------------ pellets and gammas
// Cell properties of the model cell mgi; the empty-cell sentinel mgi == npts_model reads as zero, as the
// reference's zero-initialised modelgrid[npts_model] entry does (grid.cc:840).
inline double cell_rho(const Ctx &c, int mgi) { return mgi == npts_model(c) ? 0. : (double)c.cs->rho[mgi]; }
inline double cell_nnetot(const Ctx &c, int mgi) { return mgi == npts_model(c) ? 0. : (double)c.cs->nnetot[mgi]; }
inline double cell_ffegrp(const Ctx &c, int mgi) {
  return (mgi == npts_model(c) || !c.cs->ffegrp) ? 0. : (double)c.cs->ffegrp[mgi];
}

// vectors.cc:10-44
void scatter_dir(artis_rng *rng, const double dir_in[3], double cos_theta, double dir_out[3]) {
  const double zrand = artis_rng_uniform(rng);
  const double phi = zrand * 2 * ARTIS_PI;
  const double sin_theta_sq = 1. - (cos_theta * cos_theta);
  const double sin_theta = std::sqrt(sin_theta_sq);
  const double zprime = cos_theta;
  const double xprime = sin_theta * std::cos(phi);
  const double yprime = sin_theta * std::sin(phi);
  const double norm1 = 1. / std::sqrt((dir_in[0] * dir_in[0]) + (dir_in[1] * dir_in[1]));
  const double norm2 = 1. / std::sqrt((dir_in[0] * dir_in[0]) + (dir_in[1] * dir_in[1]) + (dir_in[2] * dir_in[2]));
  const double r11 = dir_in[1] * norm1;
  const double r12 = -1 * dir_in[0] * norm1;
  const double r13 = 0.0;
  const double r21 = dir_in[0] * dir_in[2] * norm1 * norm2;
  const double r22 = dir_in[1] * dir_in[2] * norm1 * norm2;
  const double r23 = -1 * norm2 / norm1;
  const double r31 = dir_in[0] * norm2;
  const double r32 = dir_in[1] * norm2;
  const double r33 = dir_in[2] * norm2;
  dir_out[0] = (r11 * xprime) + (r21 * yprime) + (r31 * zprime);
  dir_out[1] = (r12 * xprime) + (r22 * yprime) + (r32 * zprime);
  dir_out[2] = (r13 * xprime) + (r23 * yprime) + (r33 * zprime);
}

[[noreturn]] void gamma_fatal(const char *what, const artis_packet *p) {
  fprintf(stderr, "oracle: [fatal] %s (packet %d type %d where %d nu_cmf %g)\n", what, p->number, p->type, p->where,
          p->nu_cmf);
  abort();
}

// gammapkt.cc:227-253
void choose_gamma_ray(const Ctx &c, artis_rng *rng, artis_packet *p) {
  const int nucindex = p->pellet_nucindex;
  const double E_gamma = c.gs->nuc_endecay_gamma[nucindex];
  const double zrand = artis_rng_uniform(rng);
  const int off = c.gs->nuc_line_offset[nucindex];
  int nselected = -1;
  double runtot = 0.;
  for (int n = 0; n < c.gs->nuc_nlines[nucindex]; n++) {
    runtot += c.gs->line_probability[off + n] * c.gs->line_energy[off + n] / E_gamma;
    if (zrand <= runtot) {
      nselected = n;
      break;
    }
  }
  if (nselected < 0) gamma_fatal("Failure to choose line", p);
  p->nu_cmf = c.gs->line_energy[off + nselected] / ARTIS_H;
}

// gammapkt.cc:255-313
void pellet_gamma_decay(const Ctx &c, artis_rng *rng, artis_packet *p) {
  if (c.gs->nuc_nlines[p->pellet_nucindex] == 0) {
    p->type = ARTIS_TYPE_KPKT;
    p->absorptiontype = -6;
    return;
  }
  double dir_cmf[3];
  get_rand_isotropic_unitvec(rng, dir_cmf);
  double vel_vec[3];
  get_velocity(p->pos, vel_vec, -1. * p->tdecay);
  angle_ab(dir_cmf, vel_vec, p->dir);
  choose_gamma_ray(c, rng, p);
  p->prop_time = p->tdecay;
  const double dopplerfactor = doppler_packet_nucmf_on_nurf(c, p);
  p->nu_rf = p->nu_cmf / dopplerfactor;
  p->e_rf = p->e_cmf / dopplerfactor;
  p->type = ARTIS_TYPE_GAMMA;
  p->last_cross = ARTIS_NONE;
  p->stokes[0] = 1.0;
  p->stokes[1] = p->stokes[2] = 0.0;
  double dummy_dir[3] = {0., 0., 1.};
  cross_prod(p->dir, dummy_dir, p->pol_dir);
  if ((dot(p->pol_dir, p->pol_dir)) < 1.e-8) {
    dummy_dir[0] = dummy_dir[2] = 0.0;
    dummy_dir[1] = 1.0;
    cross_prod(p->dir, dummy_dir, p->pol_dir);
  }
  vec_norm(p->pol_dir, p->pol_dir);
}

// gammapkt.cc:315-326
inline double sigma_compton_partial(double x, double f) {
  const double term1 = ((x * x) - (2 * x) - 2) * std::log(f) / x / x;
  const double term2 = (((f * f) - 1) / (f * f)) / 2;
  const double term3 = ((f - 1) / x) * ((1 / x) + (2 / f) + (1 / (x * f)));
  return (3 * ARTIS_SIGMA_T * (term1 + term2 + term3) / (8 * x));
}

// gammapkt.cc:328-354
double sig_comp(const Ctx &c, const artis_packet *p) {
  const double xx = ARTIS_H * p->nu_cmf / ARTIS_ME / ARTIS_CLIGHT / ARTIS_CLIGHT;
  double sigma_cmf;
  if (xx < ARTIS_THOMSON_LIMIT) {
    sigma_cmf = ARTIS_SIGMA_T;
  } else {
    const double fmax = (1 + (2 * xx));
    sigma_cmf = sigma_compton_partial(xx, fmax);
  }
  sigma_cmf *= cell_nnetot(c, cell_mgi(c, p->where));
  return sigma_cmf * doppler_packet_nucmf_on_nurf(c, p);
}

// gammapkt.cc:356-397
double choose_f(double xx, double zrand) {
  double f_max = 1 + (2 * xx);
  double f_min = 1;
  const double norm = zrand * sigma_compton_partial(xx, f_max);
  int count = 0;
  double err = 1e20;
  double ftry = (f_max + f_min) / 2;
  while ((err > 1.e-4) && (count < 1000)) {
    ftry = (f_max + f_min) / 2;
    const double sigma_try = sigma_compton_partial(xx, ftry);
    if (sigma_try > norm) {
      f_max = ftry;
      err = (sigma_try - norm) / norm;
    } else {
      f_min = ftry;
      err = (norm - sigma_try) / norm;
    }
    count++;
  }
  return ftry;
}

// gammapkt.cc:399-420
double thomson_angle(artis_rng *rng, const artis_packet *p) {
  const double zrand = artis_rng_uniform(rng);
  const double B_coeff = (8. * zrand) - 4.;
  double t_coeff = std::sqrt((B_coeff * B_coeff) + 4);
  t_coeff = t_coeff - B_coeff;
  t_coeff = t_coeff / 2;
  t_coeff = std::cbrt(t_coeff);
  const double mu = (1 / t_coeff) - t_coeff;
  if (std::fabs(mu) > 1) gamma_fatal("Error in Thomson", p);
  return mu;
}

// gammapkt.cc:422-531
void compton_scatter(const Ctx &c, Est &E, artis_rng *rng, artis_packet *p) {
  double f;
  const double xx = ARTIS_H * p->nu_cmf / ARTIS_ME / ARTIS_CLIGHT / ARTIS_CLIGHT;
  bool stay_gamma;
  if (xx < ARTIS_THOMSON_LIMIT) {
    f = 1.0;
    stay_gamma = true;
  } else {
    const double zrand = artis_rng_uniform(rng);
    f = choose_f(xx, zrand);
    if ((f < 1) || (f > (2 * xx + 1))) gamma_fatal("Compton f out of bounds", p);
    const double prob_gamma = 1. / f;
    const double zrand2 = artis_rng_uniform(rng);
    stay_gamma = (zrand2 < prob_gamma);
  }
  if (stay_gamma) {
    p->nu_cmf = p->nu_cmf / f;
    double vel_vec[3];
    get_velocity(p->pos, vel_vec, p->prop_time);
    double cmf_dir[3];
    angle_ab(p->dir, vel_vec, cmf_dir);
    double cos_theta;
    if (xx < ARTIS_THOMSON_LIMIT)
      cos_theta = thomson_angle(rng, p);
    else
      cos_theta = 1. - ((f - 1) / xx);
    double new_dir[3];
    scatter_dir(rng, cmf_dir, cos_theta, new_dir);
    const double test = dot(new_dir, new_dir);
    if (std::fabs(1. - test) > 1.e-8) gamma_fatal("Not a unit vector - Compton", p);
    const double test2 = dot(new_dir, cmf_dir);
    if (std::fabs(test2 - cos_theta) > 1.e-8) gamma_fatal("Problem with angle - Compton", p);
    vec_scale(vel_vec, -1.);
    double final_dir[3];
    angle_ab(new_dir, vel_vec, final_dir);
    vec_copy(p->dir, final_dir);
    const double dopplerfactor = doppler_packet_nucmf_on_nurf(c, p);
    p->nu_rf = p->nu_cmf / dopplerfactor;
    p->e_rf = p->e_cmf / dopplerfactor;
    p->last_cross = ARTIS_NONE;
  } else {
    p->type = ARTIS_TYPE_NTLEPTON;
    p->absorptiontype = -3;
    counter_inc(E, CTR_NT_STAT_FROM_GAMMA);
  }
}

// photo_electric.cc:10-48
double sig_photo_electric(const Ctx &c, const artis_packet *p) {
  double sigma_cmf;
  const int mgi = cell_mgi(c, p->where);
  const double rho = cell_rho(c, mgi);
  if (c.rp.gamma_grey < 0) {
    double sigma_cmf_si = 1.16e-24 * std::pow(p->nu_cmf / 2.41326e19, -3.13);
    double sigma_cmf_fe = 25.7e-24 * std::pow(p->nu_cmf / 2.41326e19, -3.0);
    sigma_cmf_si *= rho / ARTIS_MH / 28;
    sigma_cmf_fe *= rho / ARTIS_MH / 56;
    const double f_fe = cell_ffegrp(c, mgi);
    sigma_cmf = (sigma_cmf_fe * f_fe) + (sigma_cmf_si * (1. - f_fe));
  } else {
    sigma_cmf = c.rp.gamma_grey * rho;
  }
  return sigma_cmf * doppler_packet_nucmf_on_nurf(c, p);
}

// photo_electric.cc:50-111
double sig_pair_prod(const Ctx &c, const artis_packet *p) {
  double sigma_cmf;
  const int mgi = cell_mgi(c, p->where);
  const double rho = cell_rho(c, mgi);
  if (c.rp.gamma_grey < 0) {
    if (p->nu_cmf > 2.46636e+20) {
      double sigma_cmf_si;
      double sigma_cmf_fe;
      const double f_fe = cell_ffegrp(c, mgi);
      if (p->nu_cmf > 3.61990e+20) {
        sigma_cmf_si = (0.0481 + (0.301 * ((p->nu_cmf / 2.41326e+20) - 1.5))) * 196.e-27;
        sigma_cmf_fe = (0.0481 + (0.301 * ((p->nu_cmf / 2.41326e+20) - 1.5))) * 784.e-27;
      } else {
        sigma_cmf_si = 1.0063 * ((p->nu_cmf / 2.41326e+20) - 1.022) * 196.e-27;
        sigma_cmf_fe = 1.0063 * ((p->nu_cmf / 2.41326e+20) - 1.022) * 784.e-27;
      }
      sigma_cmf_si *= rho / ARTIS_MH / 28;
      sigma_cmf_fe *= rho / ARTIS_MH / 56;
      sigma_cmf = (sigma_cmf_fe * f_fe) + (sigma_cmf_si * (1. - f_fe));
    } else {
      sigma_cmf = 0.0;
    }
  } else {
    sigma_cmf = 0.0;
  }
  double sigma_rf = sigma_cmf * doppler_packet_nucmf_on_nurf(c, p);
  if (sigma_rf < 0) sigma_rf = 0.0;
  return sigma_rf;
}

// photo_electric.cc:113-166
void pair_prod(const Ctx &c, Est &E, artis_rng *rng, artis_packet *p) {
  const double prob_gamma = 1.022 * ARTIS_MEV / (ARTIS_H * p->nu_cmf);
  if (prob_gamma < 0) gamma_fatal("prob_gamma < 0. pair_prod", p);
  const double zrand = artis_rng_uniform(rng);
  if (zrand > prob_gamma) {
    p->type = ARTIS_TYPE_NTLEPTON;
    p->absorptiontype = -5;
    counter_inc(E, CTR_NT_STAT_FROM_GAMMA);
  } else {
    p->nu_cmf = 0.511 * ARTIS_MEV / ARTIS_H;
    double dir_cmf[3];
    get_rand_isotropic_unitvec(rng, dir_cmf);
    double vel_vec[3];
    get_velocity(p->pos, vel_vec, -1. * p->prop_time);
    angle_ab(dir_cmf, vel_vec, p->dir);
    const double dopplerfactor = doppler_packet_nucmf_on_nurf(c, p);
    p->nu_rf = p->nu_cmf / dopplerfactor;
    p->e_rf = p->e_cmf / dopplerfactor;
    p->type = ARTIS_TYPE_GAMMA;
    p->last_cross = ARTIS_NONE;
  }
}

// grey_emissivities.cc:12-26
inline double meanf_sigma(double x) {
  double f = 1 + (2 * x);
  double term0 = 2 / x;
  double term1 = (1 - (2 / x) - (3 / (x * x))) * std::log(f);
  double term2 = ((4 / x) + (3 / (x * x)) - 1) * 2 * x / f;
  double term3 = (1 - (2 / x) - (1 / (x * x))) * 2 * x * (1 + x) / f / f;
  double term4 = -2. * x * ((4 * x * x) + (6 * x) + 3) / 3 / f / f / f;
  double tot = 3 * ARTIS_SIGMA_T * (term0 + term1 + term2 + term3 + term4) / (8 * x);
  return tot;
}

// grey_emissivities.cc:28-77
void rlc_emiss_gamma(const Ctx &c, Est &E, const artis_packet *p, double dist) {
  const int mgi = cell_mgi(c, p->where);
  if (dist > 0) {
    double vel_vec[3];
    get_velocity(p->pos, vel_vec, p->prop_time);
    const double xx = ARTIS_H * p->nu_cmf / ARTIS_ME / ARTIS_CLIGHT / ARTIS_CLIGHT;
    double heating_cont = ((meanf_sigma(xx) * cell_nnetot(c, mgi)) + sig_photo_electric(c, p) +
                           (sig_pair_prod(c, p) * (1. - (2.46636e+20 / p->nu_cmf))));
    heating_cont = heating_cont * p->e_rf * dist * (1. - (2. * dot(vel_vec, p->dir) / ARTIS_CLIGHT));
    if (E.e->rpkt_emiss) safeadd(&E.e->rpkt_emiss[mgi], 1.e-20 * heating_cont);
  }
}

// gammapkt.cc:720-745
constexpr int RED_OF_LIST = -956;  // gammapkt.cc:33
int get_nul(const Ctx &c, double freq) {
  const std::vector<double> &f = c.gam_freq;
  const double freq_max = f[f.size() - 1];
  const double freq_min = f[0];
  if (freq > freq_max) return (int)f.size() - 1;
  if (freq < freq_min) return RED_OF_LIST;
  if (f.size() == 1) return 0;  // the reference's bisection never ends here (deviation, as gamma.h get_nul)
  int too_high = (int)f.size() - 1;
  int too_low = 0;
  while (too_high != too_low + 1) {
    const int tryindex = (too_high + too_low) / 2;
    const double freq_try = f[tryindex];
    if (freq_try >= freq)
      too_high = tryindex;
    else
      too_low = tryindex;
  }
  return too_low;
}

// emissivities.cc:14-113
void compton_emiss_cont(const Ctx &c, Est &E, const artis_packet *p, double dist) {
  double vel_vec[3];
  double cmf_dir[3];
  double cmf_syn_dir[3];
  get_velocity(p->pos, vel_vec, p->prop_time);
  angle_ab(p->dir, vel_vec, cmf_dir);
  angle_ab(c.rp.syn_dir, vel_vec, cmf_syn_dir);
  const double mu_cmf = dot(cmf_dir, cmf_syn_dir);
  if (mu_cmf > 1 || mu_cmf < -1) gamma_fatal("problem with Compton emissivity", p);
  const double f = 1 + (ARTIS_H * p->nu_cmf / ARTIS_ME / ARTIS_CLIGHT / ARTIS_CLIGHT * (1. - mu_cmf));
  const double freq_out = p->nu_cmf / f;
  const int lindex = get_nul(c, freq_out);
  if ((lindex > c.rp.emiss_offset - 1) && (lindex < c.rp.emiss_offset + c.rp.emiss_max - 1)) {
    const double dsigma_domega_cmf = 0.0596831 * ARTIS_SIGMA_T / f / f * (f + (1. / f) + (mu_cmf * mu_cmf) - 1.);
    const double dop_fac = doppler_nucmf_on_nurf(c, p->dir, vel_vec);
    const double emiss_cont = p->e_rf * dsigma_domega_cmf * dist * dop_fac * dop_fac / f;
    if (lindex >= c.rp.emiss_offset && E.e->compton_emiss)
      safeadd(&E.e->compton_emiss[cell_mgi(c, p->where) * ARTIS_EMISS_MAX + lindex - c.rp.emiss_offset], emiss_cont);
  }
}

// emissivities.cc:115-136
void pp_emiss_cont(const Ctx &c, Est &E, const artis_packet *p, double dist) {
  const double emiss_cont = sig_pair_prod(c, p) * (2.46636e+20 / p->nu_cmf) * p->e_rf * dist;
  if (E.e->compton_emiss)
    safeadd(&E.e->compton_emiss[cell_mgi(c, p->where) * ARTIS_EMISS_MAX + c.rp.emiss_max - 1], 1.e-20 * emiss_cont);
}

// gammapkt.cc:533-700: one step of a gamma packet (cell boundary, end of timestep or interaction)
void do_gamma(const Ctx &c, Est &E, artis_rng *rng, artis_packet *p, double t2) {
  double zrand = artis_rng_uniform_pos(rng);
  const double tau_next = -1. * std::log(zrand);
  const double tau_current = 0.0;
  int snext;
  double sdist = boundary_cross(c, E, p, &snext);
  const double maxsdist = max_sdist(c, p, sdist);
  if (sdist > maxsdist) gamma_fatal("Unreasonably large sdist (gamma)", p);
  if (sdist < 0) sdist = 0;
  if (((snext < 0) && (snext != -99)) || (snext >= c.g->ngrid)) gamma_fatal("Heading for inappropriate grid cell", p);
  if (sdist > c.rp.max_path_step) {
    sdist = c.rp.max_path_step;
    snext = p->where;
  }
  double kap_compton = 0.0;
  if (c.rp.gamma_grey < 0) kap_compton = sig_comp(c, p);
  const double kap_photo_electric = sig_photo_electric(c, p);
  const double kap_pair_prod = sig_pair_prod(c, p);
  const double kap_tot = kap_compton + kap_photo_electric + kap_pair_prod;
  const double edist = (tau_next - tau_current) / kap_tot;
  if (edist < 0) gamma_fatal("Negative distance (edist)", p);
  const double tdist = (t2 - p->prop_time) * ARTIS_CLIGHT_PROP;
  if (tdist < 0) gamma_fatal("Negative distance (tdist)", p);
  const bool rlc = c.rp.do_rlc_est != 0;
  if ((sdist < tdist) && (sdist < edist)) {
    p->prop_time += sdist / 2. / ARTIS_CLIGHT_PROP;
    move_pkt(c, p, sdist / 2.);
    if (kap_tot > 0) {
      if (c.do_comp_est) {
        compton_emiss_cont(c, E, p, sdist);
        pp_emiss_cont(c, E, p, sdist);
      }
      if (rlc) rlc_emiss_gamma(c, E, p, sdist);
    }
    p->prop_time += sdist / 2. / ARTIS_CLIGHT_PROP;
    move_pkt(c, p, sdist / 2.);
    if (snext != p->where) change_cell(E, p, snext);
  } else if ((tdist < sdist) && (tdist < edist)) {
    p->prop_time += tdist / 2. / ARTIS_CLIGHT_PROP;
    move_pkt(c, p, tdist / 2.);
    if (kap_tot > 0) {
      if (c.do_comp_est) {
        compton_emiss_cont(c, E, p, tdist);
        pp_emiss_cont(c, E, p, tdist);
      }
      if (rlc) rlc_emiss_gamma(c, E, p, tdist);
    }
    p->prop_time = t2;
    move_pkt(c, p, tdist / 2.);
  } else if ((edist < sdist) && (edist < tdist)) {
    p->prop_time += edist / 2. / ARTIS_CLIGHT_PROP;
    move_pkt(c, p, edist / 2.);
    if (kap_tot > 0) {
      if (c.do_comp_est) {
        compton_emiss_cont(c, E, p, edist);
        pp_emiss_cont(c, E, p, edist);
      }
      if (rlc) rlc_emiss_gamma(c, E, p, edist);
    }
    p->prop_time += edist / 2. / ARTIS_CLIGHT_PROP;
    move_pkt(c, p, edist / 2.);
    zrand = artis_rng_uniform(rng);
    if (kap_compton > (zrand * kap_tot)) {
      compton_scatter(c, E, rng, p);
    } else if ((kap_compton + kap_photo_electric) > (zrand * kap_tot)) {
      p->type = ARTIS_TYPE_NTLEPTON;
      p->absorptiontype = -4;
      counter_inc(E, CTR_NT_STAT_FROM_GAMMA);
    } else if ((kap_compton + kap_photo_electric + kap_pair_prod) > (zrand * kap_tot)) {
      pair_prod(c, E, rng, p);
    } else {
      gamma_fatal("Failed to identify event. Gamma (1)", p);
    }
  } else {
    gamma_fatal("Failed to identify event. Gamma (2)", p);
  }
}

// update_packets.cc:16-69
void do_nonthermal_predeposit(const Ctx &c, Est &E, artis_rng *rng, artis_packet *p, double t2) {
  const double ts = p->prop_time;
  const double particle_en = ARTIS_H * p->nu_cmf;
  double endot = 0.;
  double t_absorb = ts;
  if (!c.rp.instant_particle_deposition) {
    const double rho = cell_rho(c, cell_mgi(c, p->where));
    endot = (p->pellet_decaytype == ARTIS_DECAYTYPE_ALPHA) ? 5.e11 * ARTIS_MEV * rho : 4.e10 * ARTIS_MEV * rho;
    const double zrand = artis_rng_uniform(rng);
    const double en_absorb = zrand * particle_en;
    t_absorb = ts + en_absorb / endot;
  }
  if (t_absorb <= t2) {
    if (p->pellet_decaytype == ARTIS_DECAYTYPE_ALPHA)
      safeadd(&E.e->alpha_dep, p->e_cmf);
    else if (p->pellet_decaytype == ARTIS_DECAYTYPE_BETAMINUS)
      safeadd(&E.e->electron_dep, p->e_cmf);
    else if (p->pellet_decaytype == ARTIS_DECAYTYPE_BETAPLUS)
      safeadd(&E.e->positron_dep, p->e_cmf);
    vec_scale(p->pos, t_absorb / ts);
    p->prop_time = t_absorb;
    p->type = ARTIS_TYPE_NTLEPTON;
  } else {
    p->nu_cmf = (particle_en - endot * (t2 - ts)) / ARTIS_H;
    vec_scale(p->pos, t2 / ts);
    p->prop_time = t2;
  }
}

// update_packets.cc:71-135
void update_pellet(const Ctx &c, Est &E, artis_rng *rng, artis_packet *p, int nts, double t2) {
  if (!(p->prop_time < t2)) gamma_fatal("update_pellet: prop_time >= t2", p);
  const double ts = p->prop_time;
  const double tdecay = p->tdecay;
  if (tdecay > t2) {
    vec_scale(p->pos, t2 / ts);
    p->prop_time = t2;
  } else if (tdecay > ts) {
#pragma omp atomic update
    E.e->pellet_decays += 1;
    p->prop_time = tdecay;
    vec_scale(p->pos, tdecay / ts);
    if (p->originated_from_particlenotgamma) {
      if (p->pellet_decaytype == ARTIS_DECAYTYPE_BETAPLUS) {
        safeadd(&E.e->positron_dep, p->e_cmf);
        p->type = ARTIS_TYPE_NTLEPTON;
        p->absorptiontype = -10;
      } else if (p->pellet_decaytype == ARTIS_DECAYTYPE_BETAMINUS) {
        safeadd(&E.e->electron_emission, p->e_cmf);
        p->em_time = (int)p->prop_time;
        p->type = ARTIS_TYPE_NONTHERMAL_PREDEPOSIT;
        p->absorptiontype = -10;
      } else if (p->pellet_decaytype == ARTIS_DECAYTYPE_ALPHA) {
        safeadd(&E.e->alpha_emission, p->e_cmf);
        p->em_time = (int)p->prop_time;
        p->type = ARTIS_TYPE_NONTHERMAL_PREDEPOSIT;
        p->absorptiontype = -10;
      }
    } else {
      safeadd(&E.e->gamma_emission, p->e_cmf);
      pellet_gamma_decay(c, rng, p);
    }
  } else if ((tdecay > 0) && (nts == 0)) {
    p->e_cmf *= tdecay / c.g->tmin;
    p->type = ARTIS_TYPE_PRE_KPKT;
    p->absorptiontype = -7;
    counter_inc(E, CTR_K_STAT_FROM_EARLIERDECAY);
    p->prop_time = c.g->tmin;
  } else {
    gamma_fatal("Something gone wrong with decaying pellets", p);
  }
}

// nonthermal.cc:1877-1977 (NT_EXCITATION_ON false): with NT_ON && NT_SOLVE_SPENCERFANO outside thick cells a
// fraction frac_ionization of the deposition activates a macro-atom by non-thermal ionisation; the rest (and
// every deposition under the classic / kilonova-LTE options) becomes a k-packet
void do_ntlepton(const Ctx &c, Est &E, artis_rng *rng, artis_packet *p) {
  safeadd(&E.e->nt_energy_deposited, p->e_cmf);
  const int mgi = cell_mgi(c, p->where);
  if (c.rp.nt_on && c.rp.nt_solve_spencerfano && c.cs->thick[mgi] != 1) {
    const double zrand = artis_rng_uniform(rng);
    const double frac_ionization = get_ntion_energyrate(c, mgi) / c.cs->nt_deposition_rate_density[mgi];
    if (zrand < frac_ionization) {
      int element = -1, lowerion = -1;
      select_nt_ionization2(c, rng, mgi, &element, &lowerion);
      const int upperion = nt_random_upperion(c, rng, mgi, element, lowerion, true);
      p->mastate.element = element;
      p->mastate.ion = upperion;
      p->mastate.level = 0;
      p->mastate.activatingline = -99;
      p->type = ARTIS_TYPE_MA;
      counter_inc(E, CTR_MA_STAT_ACTIVATION_NTCOLLION);
      p->interactions += 1;
      p->last_event = 20;
      p->trueemissiontype = -1;
      p->trueemissionvelocity = -1;
      counter_inc(E, CTR_NT_STAT_TO_IONIZATION);
      return;
    }
  }
  p->last_event = 22;
  p->type = ARTIS_TYPE_KPKT;
  counter_inc(E, CTR_NT_STAT_TO_KPKT);
}

// ------------------------------------------------------------------------------------------- packet driver
// update_packets.cc:137-202 do_packet (r-packet, k-packet and macro-atom paths)
int do_packet(const Ctx &c, ThreadCache &tc, Est &E, artis_rng *rng, artis_packet *p, double t2, int nts) {
  const int pkt_type = p->type;
  switch (pkt_type) {
    case ARTIS_TYPE_RPKT: {
      while (do_rpkt_step(c, tc, E, rng, p, t2)) {
      }
      if (p->type == ARTIS_TYPE_ESCAPE) {
        safeadd(&E.e->cmf_lum, p->e_cmf);
        tc.work[WK_ESCAPED]++;
      }
      return 0;
    }
    case ARTIS_TYPE_KPKT:
    case ARTIS_TYPE_PRE_KPKT:
    case ARTIS_TYPE_GAMMA_KPKT: {
      const int mgi = cell_mgi(c, p->where);
      if (pkt_type == ARTIS_TYPE_PRE_KPKT || c.cs->thick[mgi] == 1)
        do_kpkt_bb(c, E, rng, p);
      else if (pkt_type == ARTIS_TYPE_KPKT)
        do_kpkt(c, tc, E, rng, p, t2, nts);
      else {
        fprintf(stderr, "oracle: kpkt not of type TYPE_KPKT or TYPE_PRE_KPKT\n");
        abort();
      }
      return 0;
    }
    case ARTIS_TYPE_MA:
      do_macroatom(c, tc, E, rng, p, nts);
      return 0;
    case ARTIS_TYPE_RADIOACTIVE_PELLET:
      if (!c.gs) return ARTIS_ERR_UNSUPPORTED;
      update_pellet(c, E, rng, p, nts, t2);
      return 0;
    case ARTIS_TYPE_GAMMA:
      if (!c.gs) return ARTIS_ERR_UNSUPPORTED;
      do_gamma(c, E, rng, p, t2);
      if (p->type != ARTIS_TYPE_GAMMA && p->type != ARTIS_TYPE_ESCAPE) safeadd(&E.e->gamma_dep, p->e_cmf);
      return 0;
    case ARTIS_TYPE_NONTHERMAL_PREDEPOSIT:
      do_nonthermal_predeposit(c, E, rng, p, t2);
      return 0;
    case ARTIS_TYPE_NTLEPTON:
      do_ntlepton(c, E, rng, p);
      return 0;
    default:
      return ARTIS_ERR_UNSUPPORTED;
  }
}

// read_parameterfile_vpkt / init_vspecpol (vpkt.cc:408-443, 667-835): observer unit vectors (vpkt.cc:863-865)
// and the float bin edges, with the host libm, as the engine computes them
int vpkt_config(const artis_vpkt_params *vp, const int32_t *anumber, int nelements, VpktCfg &v) {  // NOLINT
  if (!vp || vp->nobs <= 0 || vp->nspectra <= 0 || vp->nspectra > ARTIS_VPKT_MAX_SPECTRA || vp->nrange < 0 ||
      vp->nrange > ARTIS_VPKT_MRANGE || vp->vmtbins <= 0 || vp->vmnubins <= 0 || !vp->nz_obs || !vp->phi_obs ||
      !vp->exclude || vp->nprocs <= 0)
    return ARTIS_ERR_BAD_ARGUMENT;
  if (vp->vgrid_flag == 1 && (vp->nrange_grid < 0 || vp->nrange_grid > ARTIS_VPKT_MRANGE_GRID || vp->ny_vgrid <= 0 ||
                              vp->nz_vgrid <= 0))
    return ARTIS_ERR_BAD_ARGUMENT;
  v.p = *vp;
  v.exclude.assign(vp->exclude, vp->exclude + vp->nspectra);
  v.obs.resize(3 * vp->nobs);
  for (int b = 0; b < vp->nobs; b++) {
    const double nz = vp->nz_obs[b], phi = vp->phi_obs[b];
    v.obs[3 * b] = sqrt(1 - nz * nz) * cos(phi);
    v.obs[3 * b + 1] = sqrt(1 - nz * nz) * sin(phi);
    v.obs[3 * b + 2] = nz;
  }
  v.dlogt = (log(vp->tmax_vspec) - log(vp->tmin_vspec)) / vp->vmtbins;
  v.dlognu = (log(vp->numax_vspec) - log(vp->numin_vspec)) / vp->vmnubins;
  v.lower_time.resize(vp->vmtbins);
  v.delta_t.resize(vp->vmtbins);
  for (int n = 0; n < vp->vmtbins; n++) {
    v.lower_time[n] = (float)exp(log(vp->tmin_vspec) + (n * (v.dlogt)));
    v.delta_t[n] = (float)(exp(log(vp->tmin_vspec) + ((n + 1) * (v.dlogt))) - v.lower_time[n]);
  }
  v.lower_freq.resize(vp->vmnubins);
  v.delta_freq.resize(vp->vmnubins);
  for (int m = 0; m < vp->vmnubins; m++) {
    v.lower_freq[m] = (float)exp(log(vp->numin_vspec) + (m * (v.dlognu)));
    v.delta_freq[m] = (float)(exp(log(vp->numin_vspec) + ((m + 1) * (v.dlognu))) - v.lower_freq[m]);
  }
  v.anumber.assign(nelements, 0);
  if (anumber)
    for (int e = 0; e < nelements; e++) v.anumber[e] = anumber[e];
  return 0;
}

int update_packets_impl(const artis_atomic_tables *at, const artis_geometry *geom, const artis_cell_state *cs,
                        const artis_run_params *rp, const artis_gamma_spectra *gs, const VpktCfg *vp, int nts,
                        artis_packet *packets, int npkts, artis_estimators *est, int64_t work_out[ARTIS_WORK_COUNT],
                        int nthreads);

// the arrays the nebular options read must be present
int check_nebular_inputs(const artis_atomic_tables *at, const artis_cell_state *cs, const artis_run_params *rp,
                         const artis_estimators *est) {
  if (rp->nlte_pops_on && (!at->ion_nlevels_nlte || !at->ion_first_nlte || !cs->nlte_pops)) return ARTIS_ERR_BAD_ARGUMENT;
  if (rp->multibin_radfield && (at->radfield_nbins <= 0 || !at->radfield_nu_upper || !cs->radfield_bin_TR ||
                                !cs->radfield_bin_W || !est->radfield_J_raw || !est->radfield_nuJ_raw ||
                                !est->radfield_contribcount))
    return ARTIS_ERR_BAD_ARGUMENT;
  if (rp->detailed_bf_estimators && (!cs->bfrate_estimator || !est->bfrate_raw)) return ARTIS_ERR_BAD_ARGUMENT;
  if (rp->nt_on && !cs->nt_ionization_ratecoeff) return ARTIS_ERR_BAD_ARGUMENT;
  if (rp->nt_on && rp->nt_solve_spencerfano &&
      (!cs->nt_deposition_rate_density || (rp->nt_max_auger_electrons > 0 &&
                                           (!cs->nt_prob_num_auger || !cs->nt_ionenfrac_num_auger))))
    return ARTIS_ERR_BAD_ARGUMENT;
  return 0;
}

}  // namespace

// ================================================================================================== C ABI
extern "C" {

// Oracle counterpart of update_packets (update_packets.cc:234-333), deviation D5 (flattened pass loop).
// gs (the gamma-ray line spectra, gammapkt.cc:27-33) may be NULL when no pellets or gamma packets are present.
int oracle_update_packets_g(const artis_atomic_tables *at, const artis_geometry *geom, const artis_cell_state *cs,
                            const artis_run_params *rp, const artis_gamma_spectra *gs, int nts, artis_packet *packets,
                            int npkts, artis_estimators *est, int64_t work_out[ARTIS_WORK_COUNT], int nthreads) {
  return update_packets_impl(at, geom, cs, rp, gs, nullptr, nts, packets, npkts, est, work_out, nthreads);
}

// The same with VPKT_ON: virtual packets of the given vpkt.txt parameters are ADDED into *vout
// (arrays sized as artis_vpkt_result documents).
int oracle_update_packets_v(const artis_atomic_tables *at, const artis_geometry *geom, const artis_cell_state *cs,
                            const artis_run_params *rp, const artis_gamma_spectra *gs, const artis_vpkt_params *vp,
                            artis_vpkt_result *vout, int nts, artis_packet *packets,
                            int npkts, artis_estimators *est, int64_t work_out[ARTIS_WORK_COUNT], int nthreads) {
  VpktCfg v;
  if (int rc = vpkt_config(vp, at->elem_anumber, at->nelements, v)) return rc;
  if (!vout || !vout->vstokes_i || !vout->vstokes_q || !vout->vstokes_u) return ARTIS_ERR_BAD_ARGUMENT;
  if (vp->vgrid_flag == 1 && (!vout->vgrid_i || !vout->vgrid_q || !vout->vgrid_u)) return ARTIS_ERR_BAD_ARGUMENT;
  v.out = vout;
  return update_packets_impl(at, geom, cs, rp, gs, &v, nts, packets, npkts, est, work_out, nthreads);
}

}  // extern "C"

namespace {
int update_packets_impl(const artis_atomic_tables *at, const artis_geometry *geom, const artis_cell_state *cs,
                        const artis_run_params *rp, const artis_gamma_spectra *gs, const VpktCfg *vp, int nts,
                        artis_packet *packets, int npkts, artis_estimators *est, int64_t work_out[ARTIS_WORK_COUNT],
                        int nthreads) {
  Ctx c;
  c.at = at;
  c.g = geom;
  c.cs = cs;
  c.rp = *rp;
  c.gs = gs;
  c.vp = vp;
  c.T_step_log = (log(at->maxtemp) - log(at->mintemp)) / (at->tablesize - 1.);
  c.nts = nts;
  c.minpop = rp->minpop > 0. ? rp->minpop : 1e-30;
  if (int rc = check_nebular_inputs(at, cs, rp, est)) return rc;
  {
    // do_comp_est = do_r_lc ? false : estim_switch(nts) (sn3d.cc:539, emissivities.cc:250-257)
    const double tstart = geom->ts_start[nts];
    const double tend = geom->ts_start[nts] + geom->ts_width[nts];
    const double ts_want = rp->time_syn_first * ((1. - geom->rmax / geom->tmin / ARTIS_CLIGHT_PROP));
    const double te_want = rp->time_syn_last * (1. + geom->rmax / geom->tmin / ARTIS_CLIGHT_PROP);
    c.do_comp_est = rp->comp_est && !rp->do_r_lc && ((tstart > te_want) || (tend < ts_want));
    if (c.do_comp_est && (!gs || rp->emiss_max < 1 || rp->emiss_max > ARTIS_EMISS_MAX)) return ARTIS_ERR_BAD_ARGUMENT;
    if (c.do_comp_est) {  // allnuc_gamma_line_list sorted by energy (init_gamma_linelist, gammapkt.cc:192-211)
      for (int k = 0; k < gs->nnuclides; k++)
        for (int j = 0; j < gs->nuc_nlines[k]; j++) c.gam_freq.push_back(gs->line_energy[gs->nuc_line_offset[k] + j]);
      std::sort(c.gam_freq.begin(), c.gam_freq.end());
      for (double &f : c.gam_freq) f /= ARTIS_H;
      if (c.gam_freq.empty()) return ARTIS_ERR_BAD_ARGUMENT;
    }
  }
  {
    // get_bfcontindex (radfield.cc:1329-1341): the allcont entry of each photoionisation target
    int64_t ntg = 0;
    for (int lv = 0; lv < at->nlevels_total; lv++) ntg += at->level_nphixstargets[lv];
    c.slot_allcont.assign(ntg + 1, -1);
    for (int ib = 0; ib < at->nbfcontinua; ib++) {
      const int ul = at->ion_uniqueleveloffset[at->elem_uniqueionoffset[at->allcont_element[ib]] + at->allcont_ion[ib]] +
                     at->allcont_level[ib];
      c.slot_allcont[at->level_phixstargets_offset[ul] + at->allcont_phixstargetindex[ib]] = ib;
    }
  }
  Est E;
  E.e = est;
  E.nelements = at->nelements;
  E.maxnions = at->maxnions;
  const double ts = geom->ts_start[nts];
  const double tw = geom->ts_width[nts];
  const double t2 = ts + tw;
  std::atomic<int> status{0};
  int64_t work[ARTIS_WORK_COUNT] = {0};
  if (nthreads <= 0) nthreads = omp_get_max_threads();
#pragma omp parallel num_threads(nthreads)
  {
    ThreadCache tc;
    tc.pops.assign(at->nlevels_total, 0.);
    tc.departureratios.assign(at->nbfcontinua, -1.);
    tc.processrates.assign((size_t)at->nlevels_total * 9, -99.);
    size_t ndown = 0, nup = 0, ntg = 0;
    for (int lv = 0; lv < at->nlevels_total; lv++) {
      ndown += at->level_ndowntrans[lv];
      nup += at->level_nuptrans[lv];
      ntg += at->level_nphixstargets[lv];
    }
    tc.individ_rad_deexc.assign(ndown, 0.);
    tc.individ_internal_down_same.assign(ndown, 0.);
    tc.individ_internal_up_same.assign(nup, 0.);
    tc.corrphotoioncoeff.assign(ntg + 1, -99.);
    tc.cooling_contrib.assign(at->ncoolingterms, -99.);
    tc.kappa_bf_sum.assign(at->nbfcontinua, 0.);
    tc.groundcont_gamma_contr.assign(at->nbfcontinua_ground, 0.);
    tc.gamma_contr.assign(at->nbfcontinua, 0.);
#pragma omp for schedule(dynamic, 16)
    for (int n = 0; n < npkts; n++) {
      artis_packet *p = &packets[n];
      p->interactions = 0;  // update_packets.cc:285-288 (pass 0)
      p->scat_count = 0;
      if (p->type == ARTIS_TYPE_ESCAPE || !(p->prop_time < t2)) continue;
      tc.work[WK_PACKETS_ACTIVE]++;
      artis_rng rng = artis_rng_init(rp->seed, p->number, nts, rp->rank);
      long iters = 0;
      while (p->type != ARTIS_TYPE_ESCAPE && p->prop_time < t2) {
        if (++iters > 2000000) {
          fprintf(stderr, "oracle: packet %d stuck: type %d where %d nu_cmf %g prop_time %.17g t2 %.17g ma %d %d %d\n",
                  p->number, p->type, p->where, p->nu_cmf, p->prop_time, t2, p->mastate.element, p->mastate.ion,
                  p->mastate.level);
          if (iters > 2000020) abort();
        }
        const int mgi = cell_mgi(c, p->where);
        if (mgi != npts_model(c) && tc.cellnumber != mgi) {
          counter_inc(E, CTR_UPDATECELL);
          cellhistory_reset(c, tc, mgi);
        }
        const int st = do_packet(c, tc, E, &rng, p, t2, nts);
        if (st != 0) {
          status = st;
          break;
        }
      }
    }
#pragma omp critical
    for (int k = 0; k < ARTIS_WORK_COUNT; k++) work[k] += tc.work[k];
  }
  if (work_out)
    for (int k = 0; k < ARTIS_WORK_COUNT; k++) work_out[k] = work[k];
  return status.load();
}
}  // namespace

extern "C" {

int oracle_update_packets(const artis_atomic_tables *at, const artis_geometry *geom, const artis_cell_state *cs,
                          const artis_run_params *rp, int nts, artis_packet *packets, int npkts,
                          artis_estimators *est, int64_t work_out[ARTIS_WORK_COUNT], int nthreads) {
  return oracle_update_packets_g(at, geom, cs, rp, nullptr, nts, packets, npkts, est, work_out, nthreads);
}

int oracle_abi_version(void) { return 4; }

// Checks of the gsl_integration_qag restatement on integrals with closed forms: fn 0 x^2, 1 exp(x), 2 sqrt(x),
// 3 a step (1 below 0.3, 2 above), 4 1/sqrt(x).  Returns the integral; *status the GSL status.
double oracle_qag61_test(int fn, double a, double b, double epsrel, int *status, double *abserr) {
  auto f = [fn](double x) -> double {
    switch (fn) {
      case 0: return x * x;
      case 1: return exp(x);
      case 2: return sqrt(x);
      case 3: return x < 0.3 ? 1. : 2.;
      default: return 1. / sqrt(x);
    }
  };
  GslWorkspace ws(kGslWsSize);
  double result = 0., err = 0.;
  const int st = gsl_qag61(f, a, b, 0., epsrel, kGslWsSize, ws, &result, &err);
  if (status) *status = st;
  if (abserr) *abserr = err;
  return result;
}

// get_corrphotoioncoeff of model cell mgi, unique level ul, target t at timestep nts (the oracle's
// NO_LUT_PHOTOION integral or estimator, as the macro-atom sees it); brute == 2: the integral by the same qag
// restatement at epsrel 1e-10; brute == 1: the same integrand summed by
// composite 8-point Gauss-Legendre over 4096 pieces per radiation-field bin crossing -- a quadrature check.
// Returns NaN for a (level, target) that has no photoionisation target: get_corrphotoioncoeff is only reached for
// t < get_nphixstargets (macroatom.cc:117-130), and a non-ionising level has no cross-section table
// (level_phixstable = -1).  The caller raises on NaN; a non-finite quadrature result is returned as NaN too.
double oracle_corrphotoioncoeff(const artis_atomic_tables *at, const artis_geometry *geom, const artis_cell_state *cs,
                                const artis_run_params *rp, int nts, int mgi, int ul, int t, int brute) {
  const double bad = std::numeric_limits<double>::quiet_NaN();
  if (ul < 0 || ul >= at->nlevels_total || mgi < 0 || t < 0) return bad;
  Ctx c;
  c.at = at;
  c.g = geom;
  c.cs = cs;
  c.rp = *rp;
  c.gs = nullptr;
  c.T_step_log = (log(at->maxtemp) - log(at->mintemp)) / (at->tablesize - 1.);
  c.nts = nts;
  c.minpop = rp->minpop > 0. ? rp->minpop : 1e-30;
  int64_t ntg = 0;
  for (int lv = 0; lv < at->nlevels_total; lv++) ntg += at->level_nphixstargets[lv];
  c.slot_allcont.assign(ntg + 1, -1);
  for (int ib = 0; ib < at->nbfcontinua; ib++) {
    const int u = at->ion_uniqueleveloffset[at->elem_uniqueionoffset[at->allcont_element[ib]] + at->allcont_ion[ib]] +
                  at->allcont_level[ib];
    c.slot_allcont[at->level_phixstargets_offset[u] + at->allcont_phixstargetindex[ib]] = ib;
  }
  ThreadCache tc;
  tc.pops.assign(at->nlevels_total, 0.);
  tc.departureratios.assign(at->nbfcontinua, -1.);
  tc.processrates.assign((size_t)at->nlevels_total * 9, -99.);
  tc.corrphotoioncoeff.assign(ntg + 1, -99.);
  tc.cooling_contrib.assign(at->ncoolingterms, -99.);
  cellhistory_reset(c, tc, mgi);
  int e = 0;
  while (e + 1 < at->nelements && at->ion_uniqueleveloffset[at->elem_uniqueionoffset[e + 1]] <= ul) e++;
  int i = 0;
  while (i + 1 < at->elem_nions[e] && at->ion_uniqueleveloffset[at->elem_uniqueionoffset[e] + i + 1] <= ul) i++;
  const int l = ul - at->ion_uniqueleveloffset[at->elem_uniqueionoffset[e] + i];
  if (t >= get_nphixstargets(c, e, i, l) || at->level_phixstable[ul] < 0) return bad;
  if (!brute) {
    const double r = get_corrphotoioncoeff(c, tc, e, i, l, t, mgi);
    return std::isfinite(r) ? r : bad;
  }
  if (brute == 2) {  // the same qag restatement at epsrel 1e-10: the integrand + bisection machinery to accuracy
    const double r = calculate_corrphotoioncoeff_integral(c, tc, e, i, l, t, mgi, 1e-10);
    return std::isfinite(r) ? r : bad;
  }
  // brute-force quadrature of the same integrand
  const double nu_threshold = ARTIS_ONEOVERH * get_phixs_threshold(c, e, i, l, t);
  const double nu_max_phixs = nu_threshold * at->last_phixs_nuovernuedge;
  const float T_e = cs->Te[mgi];
  const double nnlevel = get_levelpop(tc, c, e, i, l);
  const int upper = get_phixsupperlevel(c, e, i, l, t);
  const double sf = calculate_sahafact(c, e, i, l, upper, T_e, ARTIS_H * nu_threshold);
  double departure_ratio = nnlevel > 0. ? get_levelpop(tc, c, e, i + 1, upper) / nnlevel * cs->nne[mgi] * sf : 1.0;
  if (!std::isfinite(departure_ratio)) departure_ratio = 0.;
  const float *xs = level_photoion_xs(c, e, i, l);
  auto f = [&](double nu) {
    double corrfactor = 1. - departure_ratio * exp(-ARTIS_HOVERKB * nu / T_e);
    if (corrfactor < 0) corrfactor = 0.;
    const float sigma_bf = (float)photoionization_crosssection_fromtable(c, xs, nu_threshold, nu);
    return ARTIS_ONEOVERH * sigma_bf / nu * radfield(c, nu, mgi) * corrfactor;
  };
  // breakpoints: the phixs table nodes and the radiation-field bin edges inside the range
  std::vector<double> br = {nu_threshold, nu_max_phixs};
  for (int k = 1; k < at->nphixspoints; k++) {
    const double x = nu_threshold * (1. + k * at->nphixsnuincrement);
    if (x < nu_max_phixs) br.push_back(x);
  }
  if (rp->multibin_radfield)
    for (int b = -1; b < at->radfield_nbins; b++) {
      const double x = b < 0 ? at->radfield_nu_lower_first : at->radfield_nu_upper[b];
      if (x > nu_threshold && x < nu_max_phixs) br.push_back(x);
    }
  std::sort(br.begin(), br.end());
  static const double gx[8] = {-0.9602898564975363, -0.7966664774136267, -0.5255324099163290, -0.1834346424956498,
                               0.1834346424956498,  0.5255324099163290,  0.7966664774136267,  0.9602898564975363};
  static const double gw[8] = {0.1012285362903763, 0.2223810344533745, 0.3137066458778873, 0.3626837833783620,
                               0.3626837833783620, 0.3137066458778873, 0.2223810344533745, 0.1012285362903763};
  double sum = 0.;
  for (size_t s0 = 0; s0 + 1 < br.size(); s0++) {
    const int npc = 64;
    const double h = (br[s0 + 1] - br[s0]) / npc;
    for (int p = 0; p < npc; p++) {
      const double mid = br[s0] + (p + 0.5) * h;
      for (int q = 0; q < 8; q++) sum += gw[q] * 0.5 * h * f(mid + 0.5 * h * gx[q]);
    }
  }
  const double r = sum * ARTIS_FOURPI * get_phixsprobability(c, e, i, l, t);
  return std::isfinite(r) ? r : bad;
}

// What the packets of model cell mgi read from the cell history at timestep nts, for tests/cell_tables_ref.py:
// calculate_levelpop of every level (pops [nlevels_total]); the cumulative cooling list as do_kpkt builds it, ion by
// ion from the running sum of cooling_contrib_ion (cooling [ncoolingterms]); calculate_macroatom_transitionrates
// of every level: the nine totals (processrates [nlevels_total * 9]) and the running sums of the three individ_*
// arrays it keeps (down_same, rad_deexc [sum ndowntrans]; up_same [sum nuptrans], at the transitions' offsets).
int oracle_cell_tables(const artis_atomic_tables *at, const artis_geometry *geom, const artis_cell_state *cs,
                       const artis_run_params *rp, int nts, int mgi, double *pops, double *cooling,
                       double *processrates, double *cum_down_same, double *cum_rad_deexc, double *cum_up_same) {
  if (mgi < 0 || mgi >= geom->npts_model || nts < 0 || nts >= geom->ntstep) return ARTIS_ERR_BAD_ARGUMENT;
  if ((rp->nlte_pops_on && (!at->ion_nlevels_nlte || !at->ion_first_nlte || !cs->nlte_pops)) ||
      (rp->multibin_radfield && (at->radfield_nbins <= 0 || !at->radfield_nu_upper || !cs->radfield_bin_TR ||
                                 !cs->radfield_bin_W)) ||
      (rp->detailed_bf_estimators && !cs->bfrate_estimator) || (rp->nt_on && !cs->nt_ionization_ratecoeff))
    return ARTIS_ERR_BAD_ARGUMENT;
  Ctx c;
  c.at = at;
  c.g = geom;
  c.cs = cs;
  c.rp = *rp;
  c.gs = nullptr;
  c.T_step_log = (log(at->maxtemp) - log(at->mintemp)) / (at->tablesize - 1.);
  c.nts = nts;
  c.minpop = rp->minpop > 0. ? rp->minpop : 1e-30;
  size_t ndown = 0, nup = 0, ntg = 0;
  for (int lv = 0; lv < at->nlevels_total; lv++) {
    ndown += at->level_ndowntrans[lv];
    nup += at->level_nuptrans[lv];
    ntg += at->level_nphixstargets[lv];
  }
  c.slot_allcont.assign(ntg + 1, -1);
  for (int ib = 0; ib < at->nbfcontinua; ib++) {
    const int u = at->ion_uniqueleveloffset[at->elem_uniqueionoffset[at->allcont_element[ib]] + at->allcont_ion[ib]] +
                  at->allcont_level[ib];
    c.slot_allcont[at->level_phixstargets_offset[u] + at->allcont_phixstargetindex[ib]] = ib;
  }
  ThreadCache tc;
  tc.pops.assign(at->nlevels_total, 0.);
  tc.departureratios.assign(at->nbfcontinua, -1.);
  tc.processrates.assign((size_t)at->nlevels_total * 9, -99.);
  tc.individ_rad_deexc.assign(ndown, 0.);
  tc.individ_internal_down_same.assign(ndown, 0.);
  tc.individ_internal_up_same.assign(nup, 0.);
  tc.corrphotoioncoeff.assign(ntg + 1, -99.);
  tc.cooling_contrib.assign(at->ncoolingterms, -99.);
  cellhistory_reset(c, tc, mgi);
  for (int lv = 0; lv < at->nlevels_total; lv++) pops[lv] = tc.pops[lv];
  double coolingsum = 0.;
  for (int e = 0; e < at->nelements; e++)
    for (int i = 0; i < get_nions(c, e); i++) {
      const int ui = uion(c, e, i);
      calculate_kpkt_rates_ion(c, tc, mgi, e, i, at->ion_coolingoffset[ui], coolingsum);
      coolingsum += cs->cooling_contrib_ion[(size_t)mgi * at->nions_total + ui];
    }
  for (int k = 0; k < at->ncoolingterms; k++) cooling[k] = tc.cooling_contrib[k];
  const double t_mid = geom->ts_mid[nts];
  for (int e = 0; e < at->nelements; e++)
    for (int i = 0; i < get_nions(c, e); i++)
      for (int l = 0; l < get_nlevels(c, e, i); l++) {
        calculate_macroatom_transitionrates(c, tc, mgi, e, i, l, t_mid);
        const int ul = ulev(c, e, i, l);
        double sd = 0., sr = 0., su = 0.;
        for (int k = 0; k < at->level_ndowntrans[ul]; k++) {
          const size_t j = (size_t)at->level_downtrans_offset[ul] + k;
          cum_down_same[j] = sd += tc.individ_internal_down_same[j];
          cum_rad_deexc[j] = sr += tc.individ_rad_deexc[j];
        }
        for (int k = 0; k < at->level_nuptrans[ul]; k++) {
          const size_t j = (size_t)at->level_uptrans_offset[ul] + k;
          cum_up_same[j] = su += tc.individ_internal_up_same[j];
        }
      }
  for (size_t k = 0; k < (size_t)at->nlevels_total * 9; k++) processrates[k] = tc.processrates[k];
  return 0;
}

// ---- unit hooks for tests/ ---------------------------------------------------------------------------------
// Philox4x32-10 block (known-answer tests against the published Random123 vectors)
void oracle_philox4x32_10(uint32_t ctr[4], uint32_t k0, uint32_t k1) { artis_philox4x32_10(ctr, k0, k1); }

// n draws of select_continuum_nu for (element, lowerion, lower, upperionlevel) at T_e
int oracle_select_continuum_nu_samples(const artis_atomic_tables *at, int element, int lowerion, int lower,
                                       int upperionlevel, float T_e, int n, uint32_t seed, double *out) {
  Ctx c;
  c.at = at;
  c.g = nullptr;
  c.cs = nullptr;
  std::memset(&c.rp, 0, sizeof(c.rp));
  c.T_step_log = (log(at->maxtemp) - log(at->mintemp)) / (at->tablesize - 1.);
  for (int i = 0; i < n; i++) {
    artis_rng rng = artis_rng_init(seed, i, 0, 0);
    out[i] = select_continuum_nu(c, &rng, element, lowerion, lower, upperionlevel, T_e);
  }
  return 0;
}

// Test diagnostic: the (model cell, line) pairs whose Sobolev coefficient (B_lu n_l - B_ul n_u) is negative --
// population inversions, which only the NLTE populations produce (the expression of vpkt.cc:280 / rpkt.cc:168-187
// with calculate_levelpop's populations).  out[0]: inverted pairs, out[1]: pairs counted (cells with rho > 0).
int oracle_inverted_lines(const artis_atomic_tables *at, const artis_geometry *geom, const artis_cell_state *cs,
                          const artis_run_params *rp, int nts, int64_t out[2]) {
  Ctx c;
  c.at = at;
  c.g = geom;
  c.cs = cs;
  c.rp = *rp;
  c.nts = nts;
  c.minpop = rp->minpop > 0. ? rp->minpop : 1e-30;
  out[0] = out[1] = 0;
  for (int mgi = 0; mgi < geom->npts_model; mgi++) {
    if (!(cs->rho[mgi] > 0.f)) continue;
    for (int li = 0; li < at->nlines; li++) {
      const int e = at->line_elementindex[li], i = at->line_ionindex[li];
      const int upper = at->line_upperlevelindex[li], lower = at->line_lowerlevelindex[li];
      const double B_ul = ARTIS_CLIGHTSQUAREDOVERTWOH / pow(at->line_nu[li], 3) * at->line_einstein_A[li];
      const double B_lu = stat_weight(c, e, i, upper) / stat_weight(c, e, i, lower) * B_ul;
      const double n_u = calculate_levelpop(c, mgi, e, i, upper), n_l = calculate_levelpop(c, mgi, e, i, lower);
      if (B_lu * n_l - B_ul * n_u < 0.) out[0]++;
      out[1]++;
    }
  }
  return 0;
}

// photoionisation cross section lookup (atomic.cc:87-155) for table row `table`
double oracle_phixs(const artis_atomic_tables *at, int table, double nu_edge, double nu) {
  Ctx c;
  c.at = at;
  return photoionization_crosssection_fromtable(c, at->phixs_xs + (size_t)table * at->nphixspoints, nu_edge, nu);
}

// write_partial_lightcurve_spectra binning (spectrum.cc:641-721): add_to_lc_res (light_curve.cc:34-54) and
// add_to_spec (spectrum.cc:339-362) for every escaped r-packet, in packet order; timestep lookup sn3d.h:168-180
// init_spectra (spectrum.cc:495-500): lower_freq and delta_freq are float arrays (spectrum.h:18-19), so the
// bin width every deltaE divides by is the float difference of the float lower edge
static inline double spec_delta_freq(double nu_min, double dlognu, int nnu) {
  const float lower_freq = (float)exp(log(nu_min) + (nnu * (dlognu)));
  return (float)(exp(log(nu_min) + ((nnu + 1) * (dlognu))) - lower_freq);
}
static int oracle_get_timestep(const artis_geometry *g, double t) {
  for (int nts = 0; nts < g->ntstep; nts++) {
    const double tsend = (nts < (g->ntstep - 1)) ? g->ts_start[nts + 1] : g->tmax;
    if (t >= g->ts_start[nts] && t < tsend) return nts;
  }
  return -1;
}
int oracle_spectrum(const artis_geometry *g, const artis_packet *pkts, int npkts, int nnubins, int nprocs,
                    double *spec, double *lc_lum, double *lc_lumcmf) {
  const int nt = g->ntstep;
  for (int64_t j = 0; j < (int64_t)nt * nnubins; j++) spec[j] = 0.;
  for (int j = 0; j < nt; j++) lc_lum[j] = lc_lumcmf[j] = 0.;
  const double nu_min = g->nu_min_r, nu_max = g->nu_max_r;
  const double dlognu = (log(nu_max) - log(nu_min)) / nnubins;  // spectrum.cc:352
  std::vector<double> delta_freq(nnubins);
  for (int nnu = 0; nnu < nnubins; nnu++)  // spectrum.cc:497-500
    delta_freq[nnu] = spec_delta_freq(nu_min, dlognu, nnu);
  const double cmfcorr = sqrt(1. - (g->vmax * g->vmax / ARTIS_CLIGHTSQUARED));
  for (int ii = 0; ii < npkts; ii++) {
    const artis_packet *p = &pkts[ii];
    if (p->type != ARTIS_TYPE_ESCAPE || p->escape_type != ARTIS_TYPE_RPKT) continue;
    const double t_arrive = p->escape_time - (dot(p->pos, p->dir) / ARTIS_CLIGHT_PROP);  // vectors.h:146-152
    if (t_arrive > g->tmin && t_arrive < g->tmax) {
      const int nts = oracle_get_timestep(g, t_arrive);
      lc_lum[nts] += p->e_rf / g->ts_width[nts] / nprocs;
    }
    const double t_arrive_cmf = p->escape_time * cmfcorr;  // vectors.h:154-156
    if (t_arrive_cmf > g->tmin && t_arrive_cmf < g->tmax) {
      const int nts = oracle_get_timestep(g, t_arrive_cmf);
      lc_lumcmf[nts] += p->e_cmf / g->ts_width[nts] / nprocs / cmfcorr;
    }
    if (t_arrive > g->tmin && t_arrive < g->tmax && p->nu_rf > nu_min && p->nu_rf < nu_max) {
      const int nts = oracle_get_timestep(g, t_arrive);
      const int nnu = (int)((log(p->nu_rf) - log(nu_min)) / dlognu);
      if (nnu < 0 || nnu >= nnubins) return -1;  // assert_always(nnu < globals::nnubins)
      spec[(int64_t)nts * nnubins + nnu] +=
          p->e_rf / g->ts_width[nts] / delta_freq[nnu] / 4.e12 / ARTIS_PI / ARTIS_PARSEC / ARTIS_PARSEC / nprocs;
    }
  }
  return 0;
}


// exspec spectra (spectrum.cc:306-452 add_to_spec / add_to_spec_res, light_curve.cc:34-62 add_to_lc_res,
// spectrum.cc:671-681 the packet loop) for the escaped packets, in packet order, ADDED into *out
static int oracle_escapedirectionbin(const double dir_in[3], const double syn_dir[3]) {  // vectors.h:158-193
  const double xhat[3] = {1.0, 0.0, 0.0};
  const double dirmag = vec_len(dir_in);
  const double dir[3] = {dir_in[0] / dirmag, dir_in[1] / dirmag, dir_in[2] / dirmag};
  const double costheta = dot(dir, syn_dir);
  const int costhetabin = (int)((costheta + 1.0) * 10 / 2.0);
  double vec1[3] = {0}, vec2[3] = {0}, vec3[3] = {0};
  cross_prod(dir, syn_dir, vec1);
  cross_prod(xhat, syn_dir, vec2);
  const double cosphi = dot(vec1, vec2) / vec_len(vec1) / vec_len(vec2);
  cross_prod(vec2, syn_dir, vec3);
  const double testphi = dot(vec1, vec3);
  int phibin = 0;
  if (testphi > 0)
    phibin = (int)(acos(cosphi) / 2. / ARTIS_PI * 10);
  else
    phibin = (int)((acos(cosphi) + ARTIS_PI) / 2. / ARTIS_PI * 10);
  return (costhetabin * 10) + phibin;
}

int oracle_spectra(const artis_atomic_tables *at, const artis_geometry *g, const artis_packet *pkts, int npkts,
                   const artis_spectra_request *req, artis_spectra_out *out) {
  if (!req || !out || req->nnubins <= 0 || req->nprocs <= 0) return ARTIS_ERR_BAD_ARGUMENT;
  const int nnubins = req->nnubins, nt_all = g->ntstep;
  const int maxnions = at->maxnions, ioncount = at->nelements * maxnions, proccount = 2 * ioncount + 1;
  const double nu_min = g->nu_min_r, nu_max = g->nu_max_r;
  const double dlognu = (log(nu_max) - log(nu_min)) / nnubins;
  std::vector<double> delta_freq(nnubins);
  for (int nnu = 0; nnu < nnubins; nnu++)
    delta_freq[nnu] = spec_delta_freq(nu_min, dlognu, nnu);
  // bflist (input.cc:1153-1160) -> (element, ion)
  std::vector<int> bf_col(std::max(at->nbfcontinua, 1), 0);
  for (int e = 0; e < at->nelements; e++)
    for (int i = 0; i < at->elem_nions[e]; i++) {
      const int ui = at->elem_uniqueionoffset[e] + i;
      for (int l = 0; l < at->ion_nlevels[ui]; l++) {
        const int ul = at->ion_uniqueleveloffset[ui] + l;
        for (int t = 0; t < at->level_nphixstargets[ul]; t++) {
          const int bi = -1 - (at->level_cont_index[ul] - t);
          if (bi >= 0 && bi < at->nbfcontinua) bf_col[bi] = e * maxnions + i;
        }
      }
    }
  auto column = [&](int et) {  // spectrum.cc:306-337
    if (et >= 0) return at->line_elementindex[et] * maxnions + at->line_ionindex[et];
    if (et == -9999999 || at->nbfcontinua == 0) return 2 * ioncount;
    return ioncount + bf_col[-1 - et];
  };
  const size_t nb = (size_t)nt_all * nnubins;
  const double cmfcorr = sqrt(1. - (g->vmax * g->vmax / ARTIS_CLIGHTSQUARED));
  const double anglefactor = (req->abin >= 0) ? ARTIS_MABINS : 1.;
  for (int ii = 0; ii < npkts; ii++) {
    const artis_packet *p = &pkts[ii];
    if (p->type != ARTIS_TYPE_ESCAPE) continue;
    const double t_arrive = p->escape_time - (dot(p->pos, p->dir) / ARTIS_CLIGHT_PROP);
    const double t_arrive_cmf = p->escape_time * cmfcorr;
    if (p->escape_type == ARTIS_TYPE_GAMMA) {
      if (req->abin != -1) continue;
      if (out->gamma_lc_lum && t_arrive > g->tmin && t_arrive < g->tmax) {
        const int nts = oracle_get_timestep(g, t_arrive);
        out->gamma_lc_lum[nts] += p->e_rf / g->ts_width[nts] / req->nprocs;
      }
      if (out->gamma_lc_lumcmf && t_arrive_cmf > g->tmin && t_arrive_cmf < g->tmax) {
        const int nts = oracle_get_timestep(g, t_arrive_cmf);
        out->gamma_lc_lumcmf[nts] += p->e_cmf / g->ts_width[nts] / req->nprocs / cmfcorr;
      }
      continue;
    }
    if (p->escape_type != ARTIS_TYPE_RPKT) continue;
    if (req->abin >= 0 && oracle_escapedirectionbin(p->dir, req->syn_dir) != req->abin) continue;
    // add_to_lc_res
    if (out->lc_lum && t_arrive > g->tmin && t_arrive < g->tmax) {
      const int nts = oracle_get_timestep(g, t_arrive);
      out->lc_lum[nts] += p->e_rf / g->ts_width[nts] * anglefactor / req->nprocs;
    }
    if (req->abin == -1 && out->lc_lumcmf && t_arrive_cmf > g->tmin && t_arrive_cmf < g->tmax) {
      const int nts = oracle_get_timestep(g, t_arrive_cmf);
      out->lc_lumcmf[nts] += p->e_cmf / g->ts_width[nts] / req->nprocs / cmfcorr;
    }
    // add_to_spec
    if (!(t_arrive > g->tmin && t_arrive < g->tmax && p->nu_rf > nu_min && p->nu_rf < nu_max)) continue;
    const int nt = oracle_get_timestep(g, t_arrive);
    const int nnu = (int)((log(p->nu_rf) - log(nu_min)) / dlognu);
    if (nnu < 0 || nnu >= nnubins) return -1;  // assert_always(nnu < globals::nnubins)
    const double deltaE = p->e_rf / g->ts_width[nt] / delta_freq[nnu] / 4.e12 / ARTIS_PI / ARTIS_PARSEC /
                          ARTIS_PARSEC / req->nprocs * anglefactor;
    const size_t fi = (size_t)nt * nnubins + nnu;
    if (out->flux) out->flux[fi] += deltaE;
    if (out->stokes_flux)
      for (int k = 0; k < 3; k++) out->stokes_flux[k * nb + fi] += p->stokes[k] * deltaE;
    if (!out->emission) continue;
    const int nproc = column(p->emissiontype);
    const int truenproc = column(p->trueemissiontype);
    out->emission[fi * proccount + nproc] += deltaE;
    if (out->trueemission) out->trueemission[fi * proccount + truenproc] += deltaE;
    if (out->stokes_emission)
      for (int k = 0; k < 3; k++) out->stokes_emission[k * nb * proccount + fi * proccount + nproc] += p->stokes[k] * deltaE;
    const int nnu_abs = (int)((log(p->absorptionfreq) - log(nu_min)) / dlognu);
    if (nnu_abs >= 0 && nnu_abs < nnubins && out->absorption) {
      const double deltaE_absorption = p->e_rf / g->ts_width[nt] / delta_freq[nnu_abs] / 4.e12 / ARTIS_PI /
                                       ARTIS_PARSEC / ARTIS_PARSEC / req->nprocs * anglefactor;
      const int at_ = p->absorptiontype;
      if (at_ >= 0) {
        const size_t ai = ((size_t)nt * nnubins + nnu_abs) * ioncount + at->line_elementindex[at_] * maxnions +
                          at->line_ionindex[at_];
        out->absorption[ai] += deltaE_absorption;
        if (out->stokes_absorption)
          for (int k = 0; k < 3; k++) out->stokes_absorption[k * nb * ioncount + ai] += p->stokes[k] * deltaE_absorption;
      }
    }
  }
  return 0;
}

}  // extern "C"

// ================================================================================================================
// update_grid's temperature / ionisation solution for the LTE-population options, the
// checker of artis_gpu_solve_temperatures.  Restated in the reference's order throughout (no deviations): GSL's
// Brent root finder, calculate_populations, precalculate_partfuncts, calculate_bfheatingcoeffs (LUT branch),
// calculate_cooling_rates, calculate_heating_rates, T_e_eqn_heating_minus_cooling and call_T_e_finder.
// ================================================================================================================
namespace {

// GSL 2.x roots/brent.c + roots/fsolver.c (gsl_root_fsolver_set / _iterate / _root / _x_lower / _x_upper) and
// roots/convergence.c (gsl_root_test_interval), as update_grid.cc:1583-1599 and thermalbalance.cc:460-477 drive
// them.  A non-finite function value or endpoints that do not straddle zero are GSL_ERROR calls, i.e. an abort()
// under GSL's default error handler (the reference never switches it off): reported here as status -1.
struct GslBrent {
  double a, b, c, d, e, fa, fb, fc;
  double root, x_lower, x_upper;
};
template <class F>
int gsl_brent_set(GslBrent &s, F &f, double x_lower, double x_upper) {
  s.root = 0.5 * (x_lower + x_upper);
  s.x_lower = x_lower;
  s.x_upper = x_upper;
  const double f_lower = f(x_lower);
  if (!std::isfinite(f_lower)) return -1;
  const double f_upper = f(x_upper);
  if (!std::isfinite(f_upper)) return -1;
  s.a = x_lower;
  s.fa = f_lower;
  s.b = x_upper;
  s.fb = f_upper;
  s.c = x_upper;
  s.fc = f_upper;
  s.d = x_upper - x_lower;
  s.e = x_upper - x_lower;
  if ((f_lower < 0.0 && f_upper < 0.0) || (f_lower > 0.0 && f_upper > 0.0)) return -1;
  return 0;
}
template <class F>
int gsl_brent_iterate(GslBrent &s, F &f) {
  double a = s.a, b = s.b, c = s.c, fa = s.fa, fb = s.fb, fc = s.fc, d = s.d, e = s.e;
  int ac_equal = 0;
  if ((fb < 0 && fc < 0) || (fb > 0 && fc > 0)) {
    ac_equal = 1;
    c = a;
    fc = fa;
    d = b - a;
    e = b - a;
  }
  if (fabs(fc) < fabs(fb)) {
    ac_equal = 1;
    a = b;
    b = c;
    c = a;
    fa = fb;
    fb = fc;
    fc = fa;
  }
  const double tol = 0.5 * DBL_EPSILON * fabs(b);
  const double m = 0.5 * (c - b);
  if (fb == 0) {
    s.root = b;
    s.x_lower = b;
    s.x_upper = b;
    return 0;
  }
  if (fabs(m) <= tol) {
    s.root = b;
    if (b < c) {
      s.x_lower = b;
      s.x_upper = c;
    } else {
      s.x_lower = c;
      s.x_upper = b;
    }
    return 0;
  }
  if (fabs(e) < tol || fabs(fa) <= fabs(fb)) {
    d = m;
    e = m;
  } else {
    double p, q, r;
    const double sr = fb / fa;
    if (ac_equal) {
      p = 2 * m * sr;
      q = 1 - sr;
    } else {
      q = fa / fc;
      r = fb / fc;
      p = sr * (2 * m * q * (q - r) - (b - a) * (r - 1));
      q = (q - 1) * (r - 1) * (sr - 1);
    }
    if (p > 0)
      q = -q;
    else
      p = -p;
    if (2 * p < std::min(3 * m * q - fabs(tol * q), fabs(e * q))) {
      e = d;
      d = p / q;
    } else {
      d = m;
      e = m;
    }
  }
  a = b;
  fa = fb;
  if (fabs(d) > tol)
    b += d;
  else
    b += (m > 0 ? +tol : -tol);
  fb = f(b);
  if (!std::isfinite(fb)) return -1;
  s.a = a;
  s.b = b;
  s.c = c;
  s.d = d;
  s.e = e;
  s.fa = fa;
  s.fb = fb;
  s.fc = fc;
  s.root = b;
  if ((fb < 0 && fc < 0) || (fb > 0 && fc > 0)) c = a;
  if (b < c) {
    s.x_lower = b;
    s.x_upper = c;
  } else {
    s.x_lower = c;
    s.x_upper = b;
  }
  return 0;
}
// gsl_root_test_interval: 1 = GSL_CONTINUE
inline int gsl_test_interval(double x_lower, double x_upper, double epsabs, double epsrel) {
  const double abs_lower = fabs(x_lower), abs_upper = fabs(x_upper);
  double min_abs;
  if ((x_lower > 0.0 && x_upper > 0.0) || (x_lower < 0.0 && x_upper < 0.0))
    min_abs = std::min(abs_lower, abs_upper);
  else
    min_abs = 0;
  const double tolerance = epsabs + epsrel * min_abs;
  return fabs(x_upper - x_lower) < tolerance ? 0 : 1;
}

// the mutable grid state one cell's solution writes (grid::modelgrid[mgi]); Ctx::cs points at these arrays
struct TeGrid {
  std::vector<float> Te, TJ, nne, nnetot, gp, pf;
  std::vector<int> uppermost;  // [npts_model * nelements] elements_uppermost_ion
};
struct TeRun {
  const artis_te_tables *tab;
  const artis_te_params *par;
  const artis_te_cells *in;
  TeGrid *g;
};

inline float elem_meanweight(const Ctx &c, const TeRun &r, int mgi, int e) {
  return r.in->elem_meanweight[(size_t)mgi * c.at->nelements + e];
}
inline float elem_abundance(const Ctx &c, int mgi, int e) { return c.cs->elem_abundance[(size_t)mgi * c.at->nelements + e]; }
// grid.cc:231-236
inline double get_elem_numberdens(const Ctx &c, const TeRun &r, int mgi, int e) {
  const double mw = elem_meanweight(c, r, mgi, e);
  return elem_abundance(c, mgi, e) / mw * (double)c.cs->rho[mgi];
}
inline float &gp_ref(const Ctx &c, const TeRun &r, int mgi, int e, int i) {
  return r.g->gp[(size_t)mgi * c.at->nions_total + uion(c, e, i)];
}
inline float &pf_ref(const Ctx &c, const TeRun &r, int mgi, int e, int i) {
  return r.g->pf[(size_t)mgi * c.at->nions_total + uion(c, e, i)];
}

// ltepop.cc:488-537 (LTE populations: calculate_levelpop_nominpop = calculate_levelpop_lte)
double te_calculate_partfunct(const Ctx &c, const TeRun &r, int mgi, int e, int i) {
  int initial = 0;
  double pop_store = 0.;
  if (get_groundlevelpop(c, mgi, e, i) < c.minpop) {
    pop_store = get_groundlevelpop(c, mgi, e, i);
    initial = 1;
    gp_ref(c, r, mgi, e, i) = 1.0;
  }
  double U = 1.;
  const int nlevels = get_nlevels(c, e, i);
  const double groundpop = get_groundlevelpop(c, mgi, e, i);
  for (int level = 1; level < nlevels; level++) {
    bool skipminpop;
    const double nn = calculate_levelpop_nominpop(c, mgi, e, i, level, &skipminpop) / groundpop;
    U += nn;
  }
  U *= stat_weight(c, e, i, 0);
  if (initial == 1) gp_ref(c, r, mgi, e, i) = pop_store;
  return U;
}
// update_grid.cc:23-38
void te_precalculate_partfuncts(const Ctx &c, const TeRun &r, int mgi) {
  for (int e = 0; e < c.at->nelements; e++)
    for (int i = 0; i < get_nions(c, e); i++) pf_ref(c, r, mgi, e, i) = te_calculate_partfunct(c, r, mgi, e, i);
}

// ltepop.cc:97-113
double interpolate_ions_spontrecombcoeff(const Ctx &c, const TeRun &r, int e, int i, double T) {
  const int tablesize = c.at->tablesize;
  const float *alpha = r.tab->ion_alpha_sp + (size_t)uion(c, e, i) * tablesize;
  const int lowerindex = floor(log(T / c.at->mintemp) / c.T_step_log);
  if (lowerindex < tablesize - 1) {
    const int upperindex = lowerindex + 1;
    const double T_lower = c.at->mintemp * exp(lowerindex * c.T_step_log);
    const double T_upper = c.at->mintemp * exp(upperindex * c.T_step_log);
    const double f_upper = alpha[upperindex];
    const double f_lower = alpha[lowerindex];
    return f_lower + (f_upper - f_lower) / (T_upper - T_lower) * (T - T_lower);
  }
  return alpha[tablesize - 1];
}
inline bool te_use_lte_ratio(const TeRun &r, int mgi) { return r.par->initial_iteration || r.in->thick[mgi] == 1; }
inline double gammaestimator(const Ctx &c, const TeRun &r, int mgi, int e, int i) {
  return r.in->gammaestimator[(size_t)mgi * c.at->nelements * c.at->maxnions + e * c.at->maxnions + i];
}
// ltepop.cc:115-239 (NT_ON false: Y_nt = 0; NLTE_POPS_ON false: Alpha_sp from the ion table)
double te_phi(const Ctx &c, const TeRun &r, int mgi, int e, int i) {
  double phi = 0;
  const float T_e = c.cs->Te[mgi];
  if (te_use_lte_ratio(r, mgi)) {
    const double ionpot = epsilon(c, e, i + 1, 0) - epsilon(c, e, i, 0);
    const double partfunct_ratio = pf_ref(c, r, mgi, e, i) / pf_ref(c, r, mgi, e, i + 1);
    phi = partfunct_ratio * ARTIS_SAHACONST * pow(T_e, -1.5) * exp(ionpot / ARTIS_KB / T_e);
  } else {
    const double Gamma = gammaestimator(c, r, mgi, e, i);
    const double Gamma_ion = Gamma * stat_weight(c, e, i, 0) / pf_ref(c, r, mgi, e, i);
    const double Alpha_st = 0.;
    const double Alpha_sp = interpolate_ions_spontrecombcoeff(c, r, e, i, T_e);
    const double Col_rec = 0.;
    const double Y_nt = 0.0;
    phi = (Alpha_sp + Alpha_st + Col_rec) / (Gamma_ion + Y_nt);
  }
  return phi;
}
// ltepop.cc:61-95
void te_get_ionfractions(const Ctx &c, const TeRun &r, int e, int mgi, double nne, double *ionfractions, int uppermost_ion) {
  double nnionfactor[64];
  nnionfactor[uppermost_ion] = 1;
  double denominator = 1.;
  for (int ion = uppermost_ion - 1; ion >= 0; ion--) {
    nnionfactor[ion] = nnionfactor[ion + 1] * nne * te_phi(c, r, mgi, e, ion);
    denominator += nnionfactor[ion];
  }
  for (int ion = 0; ion <= uppermost_ion; ion++) {
    const double numerator = nnionfactor[ion];
    ionfractions[ion] = numerator / denominator;
    if (!std::isfinite(ionfractions[ion])) ionfractions[ion] = 0;
  }
}
// ltepop.cc:20-59
double te_nne_solution_f(const Ctx &c, const TeRun &r, int mgi, double x) {
  const double rho = c.cs->rho[mgi];
  double outersum = 0.;
  for (int e = 0; e < c.at->nelements; e++) {
    const float abundance = elem_abundance(c, mgi, e);
    if (abundance > 0 && get_nions(c, e) > 0) {
      const double elem_mw = elem_meanweight(c, r, mgi, e);
      double innersum = 0.;
      const int uppermost_ion = r.g->uppermost[(size_t)mgi * c.at->nelements + e];
      double ionfractions[64];
      te_get_ionfractions(c, r, e, mgi, x, ionfractions, uppermost_ion);
      for (int ion = 0; ion <= uppermost_ion; ion++) innersum += (get_ionstage(c, e, ion) - 1) * ionfractions[ion];
      outersum += abundance / elem_mw * innersum;
    }
  }
  return rho * outersum - x;
}
// update_grid.cc:1427-1658 (NO_LUT_PHOTOION false, NT_ON false, FORCE_LTE undefined); -1: the GSL abort path
int te_calculate_populations(const Ctx &c, const TeRun &r, int mgi, double *nntot_out) {
  const int nel = c.at->nelements;
  double nne_hi = c.cs->rho[mgi] / ARTIS_MH;
  int only_neutral_ions = 0;
  int nelements_in_cell = 0;
  for (int e = 0; e < nel; e++) {
    const int nions = get_nions(c, e);
    int &upp = r.g->uppermost[(size_t)mgi * nel + e];
    upp = nions - 1;
    const double abundance = elem_abundance(c, mgi, e);
    if (abundance > 0) {
      int uppermost_ion;
      if (te_use_lte_ratio(r, mgi)) {
        uppermost_ion = get_nions(c, e) - 1;
      } else {
        int ion;
        for (ion = 0; ion < nions - 1; ion++) {
          const double Gamma = gammaestimator(c, r, mgi, e, ion);
          if (Gamma == 0) break;
        }
        uppermost_ion = ion;
      }
      double factor = 1.;
      int ion;
      for (ion = 0; ion < uppermost_ion; ion++) {
        factor *= nne_hi * te_phi(c, r, mgi, e, ion);
        if (!std::isfinite(factor)) break;
      }
      uppermost_ion = ion;
      upp = uppermost_ion;
      if (uppermost_ion == 0) only_neutral_ions++;
      nelements_in_cell++;
    }
  }
  float nne = 0.;
  double nne_tot = 0.;
  double nntot = 0.;
  if (only_neutral_ions == nelements_in_cell) {
    for (int e = 0; e < nel; e++) {
      const double nnelement = get_elem_numberdens(c, r, mgi, e);
      nne_tot += nnelement * c.at->elem_anumber[e];
      const int nions = get_nions(c, e);
      for (int ion = 0; ion < nions; ion++) {
        double nnion;
        if (ion == 0)
          nnion = nnelement;
        else if (nnelement > 0.)
          nnion = c.minpop;
        else
          nnion = 0.;
        nntot += nnion;
        nne += nnion * (get_ionstage(c, e, ion) - 1);
        gp_ref(c, r, mgi, e, ion) = (nnion * stat_weight(c, e, ion, 0) / pf_ref(c, r, mgi, e, ion));
      }
    }
    nntot += nne;
    if (nne < c.minpop) nne = c.minpop;
    r.g->nne[mgi] = nne;
  } else {
    double nne_lo = 0.;
    auto f = [&](double x) { return te_nne_solution_f(c, r, mgi, x); };
    GslBrent s;
    if (gsl_brent_set(s, f, nne_lo, nne_hi) != 0) return -1;
    int iter = 0;
    const int maxit = 100;
    const double fractional_accuracy = 1e-3;
    int status;
    do {
      iter++;
      if (gsl_brent_iterate(s, f) != 0) return -1;
      nne = s.root;
      nne_lo = s.x_lower;
      nne_hi = s.x_upper;
      status = gsl_test_interval(nne_lo, nne_hi, 0, fractional_accuracy);
    } while (status == 1 && iter < maxit);
    if (nne < c.minpop) nne = c.minpop;
    r.g->nne[mgi] = nne;
    nne_tot = 0.;
    nntot = nne;
    for (int e = 0; e < nel; e++) {
      const int nions = get_nions(c, e);
      const double nnelement = get_elem_numberdens(c, r, mgi, e);
      nne_tot += nnelement * c.at->elem_anumber[e];
      const int uppermost_ion = r.g->uppermost[(size_t)mgi * nel + e];
      double ionfractions[64];
      if (nnelement > 0) te_get_ionfractions(c, r, e, mgi, nne, ionfractions, uppermost_ion);
      for (int ion = 0; ion < nions; ion++) {
        double nnion;
        if (ion <= uppermost_ion) {
          if (nnelement > 0) {
            nnion = nnelement * ionfractions[ion];
            if (nnion < c.minpop) nnion = c.minpop;
          } else {
            nnion = 0.;
          }
        } else {
          nnion = c.minpop;
        }
        nntot += nnion;
        gp_ref(c, r, mgi, e, ion) = (nnion * stat_weight(c, e, ion, 0) / pf_ref(c, r, mgi, e, ion));
      }
    }
  }
  r.g->nnetot[mgi] = nne_tot;
  *nntot_out = nntot;
  return 0;
}

struct TeRates {
  double cooling_collisional, cooling_fb, cooling_ff, cooling_adiabatic, heating_collisional, heating_bf, heating_ff,
      heating_dep;
};
// kpkt.cc:41-67, 84-165
void te_calculate_cooling_rates(const Ctx &c, int mgi, TeRates *hc, double *totalcooling, double *contrib_ion) {
  const float nne = c.cs->nne[mgi];
  const float T_e = c.cs->Te[mgi];
  const artis_atomic_tables &a = *c.at;
  double C_total = 0., C_ff_all = 0., C_fb_all = 0., C_exc_all = 0., C_ionization_all = 0.;
  for (int e = 0; e < a.nelements; e++) {
    const int nions = get_nions(c, e);
    for (int i = 0; i < nions; i++) {
      double C_ion = 0.;
      const int nionisinglevels = get_ionisinglevels(c, e, i);
      const double nncurrention = ionstagepop(c, mgi, e, i);
      const int ioncharge = get_ionstage(c, e, i) - 1;
      if (ioncharge > 0) {
        const double C_ff_ion = 1.426e-27 * sqrt((double)T_e) * pow(ioncharge, 2) * nncurrention * nne;
        C_ff_all += C_ff_ion;
        C_ion += C_ff_ion;
      }
      double C_exc = 0.;
      const int nlevels = get_nlevels(c, e, i);
      for (int level = 0; level < nlevels; level++) {
        const double nnlevel = calculate_levelpop(c, mgi, e, i, level);
        const double epsilon_current = epsilon(c, e, i, level);
        const double statweight = stat_weight(c, e, i, level);
        const int ul = ulev(c, e, i, level);
        const int nuptrans = a.level_nuptrans[ul];
        for (int ii = 0; ii < nuptrans; ii++) {
          const int li = a.uptrans_lineindex[a.level_uptrans_offset[ul] + ii];
          const int upper = a.line_upperlevelindex[li];
          const double epsilon_trans = epsilon(c, e, i, upper) - epsilon_current;
          const double C = nnlevel *
                           col_excitation_ratecoeff(c, T_e, nne, li, epsilon_trans, statweight, stat_weight(c, e, i, upper)) *
                           epsilon_trans;
          C_exc += C;
        }
      }
      C_exc_all += C_exc;
      C_ion += C_exc;
      if (i < nions - 1) {
        for (int level = 0; level < nionisinglevels; level++) {
          const double epsilon_current = epsilon(c, e, i, level);
          const double nnlevel = calculate_levelpop(c, mgi, e, i, level);
          const int nt = get_nphixstargets(c, e, i, level);
          for (int t = 0; t < nt; t++) {
            const int upper = get_phixsupperlevel(c, e, i, level, t);
            const double epsilon_trans = epsilon(c, e, i + 1, upper) - epsilon_current;
            const double C = nnlevel * col_ionization_ratecoeff(c, T_e, nne, e, i, level, t, epsilon_trans) * epsilon_trans;
            C_ionization_all += C;
            C_ion += C;
          }
          for (int t = 0; t < nt; t++) {
            const double nnupperion = ionstagepop(c, mgi, e, i + 1);
            const double C = get_bfcoolingcoeff(c, e, i, level, t, T_e) * nnupperion * nne;
            C_fb_all += C;
            C_ion += C;
          }
        }
      }
      C_total += C_ion;
      if (contrib_ion) contrib_ion[uion(c, e, i)] = C_ion;
    }
  }
  if (totalcooling) *totalcooling = C_total;
  if (hc) {
    hc->cooling_collisional = C_exc_all + C_ionization_all;
    hc->cooling_fb = C_fb_all;
    hc->cooling_ff = C_ff_all;
  }
}
// thermalbalance.cc:34-57 get_bfheatingcoeff_ana
double te_bfheatingcoeff_ana(const Ctx &c, const TeRun &r, int e, int i, int l, int t, double T, double W) {
  const int tablesize = c.at->tablesize;
  double bfheatingcoeff = 0.;
  const int lowerindex = floor(log(T / c.at->mintemp) / c.T_step_log);
  if (lowerindex < tablesize - 1) {
    const int upperindex = lowerindex + 1;
    const double T_lower = c.at->mintemp * exp(lowerindex * c.T_step_log);
    const double T_upper = c.at->mintemp * exp(upperindex * c.T_step_log);
    const double f_upper = r.tab->bfheating_coeff[get_bflutindex(c, upperindex, e, i, l, t)];
    const double f_lower = r.tab->bfheating_coeff[get_bflutindex(c, lowerindex, e, i, l, t)];
    bfheatingcoeff = (f_lower + (f_upper - f_lower) / (T_upper - T_lower) * (T - T_lower));
  } else {
    bfheatingcoeff = r.tab->bfheating_coeff[get_bflutindex(c, tablesize - 1, e, i, l, t)];
  }
  return W * bfheatingcoeff;
}
// thermalbalance.cc:141-187 (NO_LUT_BFHEATING false): per level of the cell
void te_calculate_bfheatingcoeffs(const Ctx &c, const TeRun &r, int mgi, std::vector<double> &coeff) {
  coeff.assign(c.at->nlevels_total, 0.);
  for (int e = 0; e < c.at->nelements; e++)
    for (int i = 0; i < get_nions(c, e); i++)
      for (int l = 0; l < get_nlevels(c, e, i); l++) {
        double bfheatingcoeff = 0.;
        for (int t = 0; t < get_nphixstargets(c, e, i, l); t++) {
          const double T_R = r.in->TR[mgi];
          const double W = r.in->W[mgi];
          bfheatingcoeff += te_bfheatingcoeff_ana(c, r, e, i, l, t, T_R, W);
        }
        const int g = c.at->level_closestgroundlevelcont[ulev(c, e, i, l)];
        if (g >= 0) bfheatingcoeff *= r.in->bfheatingestimator[(size_t)mgi * c.at->nelements * c.at->maxnions + g];
        coeff[ulev(c, e, i, l)] = bfheatingcoeff;
      }
}
// thermalbalance.cc:189-216 get_heating_ion_coll_deexc
double te_heating_ion_coll_deexc(const Ctx &c, int mgi, int e, int i, float T_e, float nne) {
  double C_deexc = 0.;
  for (int level = 0; level < get_nlevels(c, e, i); level++) {
    const double nnlevel = calculate_levelpop(c, mgi, e, i, level);
    const double epsilon_level = epsilon(c, e, i, level);
    const int ul = ulev(c, e, i, level);
    for (int k = 0; k < c.at->level_ndowntrans[ul]; k++) {
      const int li = c.at->downtrans_lineindex[c.at->level_downtrans_offset[ul] + k];
      const int lower = c.at->line_lowerlevelindex[li];
      const double epsilon_trans = epsilon_level - epsilon(c, e, i, lower);
      const double statweight = stat_weight(c, e, i, level);
      C_deexc += nnlevel * col_deexcitation_ratecoeff(c, T_e, nne, epsilon_trans, li, stat_weight(c, e, i, lower), statweight) *
                 epsilon_trans;
    }
  }
  return C_deexc;
}
// thermalbalance.cc:218-346: the collisional heating is the de-excitation sum with DIRECT_COL_HEAT
// (artis_te_params.direct_col_heat), the normalised estimator otherwise
void te_calculate_heating_rates(const Ctx &c, const TeRun &r, int mgi, const std::vector<double> &coeff, TeRates *hc) {
  double bfheating = 0., C_deexc = 0.;
  for (int e = 0; e < c.at->nelements; e++) {
    const int nions = get_nions(c, e);
    if (r.par->direct_col_heat)
      for (int i = 0; i < nions; i++) C_deexc += te_heating_ion_coll_deexc(c, mgi, e, i, r.g->Te[mgi], r.g->nne[mgi]);
    for (int i = 0; i < nions - 1; i++) {
      const int nbflevels = get_ionisinglevels(c, e, i);
      for (int level = 0; level < nbflevels; level++) {
        const double nnlevel = calculate_levelpop(c, mgi, e, i, level);
        bfheating += nnlevel * coeff[ulev(c, e, i, level)];
      }
    }
  }
  hc->heating_collisional = r.par->direct_col_heat ? C_deexc : r.in->colheatingestimator[mgi];
  hc->heating_bf = bfheating;
  hc->heating_ff = r.in->ffheatingestimator[mgi];
}
// thermalbalance.cc:348-395; -1 in *fail on the GSL abort path
double te_eqn_heating_minus_cooling(const Ctx &c, const TeRun &r, int mgi, double T_e, const std::vector<double> &coeff,
                                    TeRates *hc, int *fail) {
  r.g->Te[mgi] = T_e;
  double nntot = 0.;
  if (te_calculate_populations(c, r, mgi, &nntot) != 0) {
    *fail = 1;
    return NAN;
  }
  te_calculate_cooling_rates(c, mgi, hc, nullptr, nullptr);
  te_calculate_heating_rates(c, r, mgi, coeff, hc);
  hc->heating_dep = r.in->heating_dep ? r.in->heating_dep[mgi] : 0.;
  const double p = nntot * ARTIS_KB * T_e;
  const double volumetmin = r.in->vol_init[mgi];
  const double dV = 3 * volumetmin / pow(r.par->tmin, 3) * pow(r.par->t_current, 2);
  const double V = volumetmin * pow(r.par->t_current / r.par->tmin, 3);
  hc->cooling_adiabatic = p * dV / V;
  const double total_heating_rate = hc->heating_ff + hc->heating_bf + hc->heating_collisional + hc->heating_dep;
  const double total_coolingrate = hc->cooling_ff + hc->cooling_fb + hc->cooling_collisional + hc->cooling_adiabatic;
  return total_heating_rate - total_coolingrate;
}
// thermalbalance.cc:397-597; returns the Brent iteration count (-1: no root in the interval), -2 on the abort path
int te_call_T_e_finder(const Ctx &c, const TeRun &r, int mgi, const std::vector<double> &coeff, TeRates *hc) {
  const double T_min = r.par->T_min, T_max = r.par->T_max;
  const double T_e_old = r.g->Te[mgi];
  int fail = 0;
  auto f = [&](double T) { return te_eqn_heating_minus_cooling(c, r, mgi, T, coeff, hc, &fail); };
  double thermalmin = f(T_min);
  double thermalmax = f(T_max);
  if (fail) return -2;
  if (!std::isfinite(thermalmin) || !std::isfinite(thermalmax)) thermalmax = thermalmin = -1;
  double T_e = 0.;
  int iters = -1;
  if (thermalmin * thermalmax < 0) {
    GslBrent s;
    if (gsl_brent_set(s, f, T_min, T_max) != 0 || fail) return -2;
    const int maxit = 100;
    for (int iternum = 0; iternum < maxit; iternum++) {
      if (gsl_brent_iterate(s, f) != 0 || fail) return -2;
      T_e = s.root;
      iters = iternum + 1;
      if (gsl_test_interval(s.x_lower, s.x_upper, 0, r.par->accuracy) != 1) break;
    }
  } else if (thermalmax < 0) {
    T_e = T_min;
  } else {
    T_e = T_max;
  }
  if (T_e > 2 * T_e_old) {
    T_e = 2 * T_e_old;
    if (T_e > T_max) T_e = T_max;
  } else if (T_e < 0.5 * T_e_old) {
    T_e = 0.5 * T_e_old;
    if (T_e < T_min) T_e = T_min;
  }
  r.g->Te[mgi] = T_e;
  f(T_e);
  if (fail) return -2;
  return iters;
}

}  // namespace

extern "C" {
// artis_gpu_solve_temperatures restated (include/artis_gpu.h): the reference's per-cell update_grid solution for the
// LTE-population options, cells in parallel (OpenMP), each in the reference's serial order.
int oracle_solve_temperatures(const artis_atomic_tables *at, const artis_run_params *rp, const artis_te_tables *tab,
                              const artis_te_params *par, artis_te_cells *in, int npts_model, int nthreads) {
  if (rp->nlte_pops_on || rp->no_lut_photoion || rp->no_lut_bfheating || rp->nt_on) return ARTIS_ERR_UNSUPPORTED;
  const size_t ni = at->nions_total, nel = at->nelements;
  TeGrid g;
  g.Te.assign(in->Te, in->Te + npts_model);
  g.TJ.assign(in->TJ, in->TJ + npts_model);
  g.nne.assign(npts_model, 0.f);
  g.nnetot.assign(npts_model, 0.f);
  g.gp.assign(in->groundlevelpop, in->groundlevelpop + (size_t)npts_model * ni);
  g.pf.assign((size_t)npts_model * ni, 0.f);
  g.uppermost.assign((size_t)npts_model * nel, 0);
  artis_cell_state cs;
  memset(&cs, 0, sizeof(cs));
  cs.Te = g.Te.data();
  cs.TJ = g.TJ.data();
  cs.TR = in->TR;
  cs.W = in->W;
  cs.nne = g.nne.data();
  cs.rho = in->rho;
  cs.elem_abundance = in->elem_abundance;
  cs.groundlevelpop = g.gp.data();
  cs.partfunct = g.pf.data();
  Ctx c;
  c.at = at;
  c.g = nullptr;
  c.cs = &cs;
  c.rp = *rp;
  c.gs = nullptr;
  c.T_step_log = (log(at->maxtemp) - log(at->mintemp)) / (at->tablesize - 1.);
  c.minpop = rp->minpop > 0. ? rp->minpop : 1e-30;
  TeRun r{tab, par, in, &g};
  int rc = 0;
  if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic)
  for (int k = 0; k < in->ncells; k++) {
    const int mgi = in->mgi[k];
    TeRates hc;
    memset(&hc, 0, sizeof(hc));
    int iters = 0;
    if (te_use_lte_ratio(r, mgi)) {
      // update_grid.cc:1111-1124 (T_J from get_T_J_from_J is the caller's TJ)
      g.Te[mgi] = in->TJ[mgi];
      te_precalculate_partfuncts(c, r, mgi);
      double nntot;
      if (te_calculate_populations(c, r, mgi, &nntot) != 0) iters = -2;
    } else {
      // update_grid.cc:763-886 without NLTE_POPS_ON (one pass of the nlte_iter loop)
      std::vector<double> coeff;
      te_calculate_bfheatingcoeffs(c, r, mgi, coeff);
      te_precalculate_partfuncts(c, r, mgi);
      iters = te_call_T_e_finder(c, r, mgi, coeff, &hc);
      double nntot;
      if (iters != -2 && te_calculate_populations(c, r, mgi, &nntot) != 0) iters = -2;
    }
    if (iters == -2) {
#pragma omp critical
      rc = ARTIS_ERR_PACKET_FAULT;
      continue;
    }
    te_calculate_cooling_rates(c, mgi, nullptr, &in->totalcooling[mgi], in->cooling_contrib_ion + (size_t)mgi * ni);
    in->Te[mgi] = g.Te[mgi];
    in->nne[mgi] = g.nne[mgi];
    in->nnetot[mgi] = g.nnetot[mgi];
    for (size_t u = 0; u < ni; u++) {
      in->groundlevelpop[(size_t)mgi * ni + u] = g.gp[(size_t)mgi * ni + u];
      in->partfunct[(size_t)mgi * ni + u] = g.pf[(size_t)mgi * ni + u];
    }
    if (in->heatingcoolingrates) memcpy(in->heatingcoolingrates + (size_t)mgi * ARTIS_TE_NRATES, &hc, sizeof(hc));
    if (in->te_iterations) in->te_iterations[mgi] = iters;
  }
  return rc;
}
}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// update_grid_cell's estimator preparation before the temperature solution (update_grid.cc:1041-1150, LTE options,
// DO_TITER undefined): the checker of artis_gpu_prepare_temperatures.
namespace {
// ratecoeff.cc:686-710-style interpolation of a [tablesize * nbfcontinua] LUT (interpolate_corrphotoioncoeff)
double lut_at(const Ctx &c, const double *lut, int e, int i, int l, int t, double T) {
  const int tablesize = c.at->tablesize;
  const int lowerindex = floor(log(T / c.at->mintemp) / c.T_step_log);
  if (lowerindex < tablesize - 1) {
    const int upperindex = lowerindex + 1;
    const double T_lower = c.at->mintemp * exp(lowerindex * c.T_step_log);
    const double T_upper = c.at->mintemp * exp(upperindex * c.T_step_log);
    const double f_upper = lut[get_bflutindex(c, upperindex, e, i, l, t)];
    const double f_lower = lut[get_bflutindex(c, lowerindex, e, i, l, t)];
    return (f_lower + (f_upper - f_lower) / (T_upper - T_lower) * (T - T_lower));
  }
  return lut[get_bflutindex(c, tablesize - 1, e, i, l, t)];
}
}  // namespace

extern "C" {
int oracle_prepare_temperatures(const artis_atomic_tables *at, const artis_run_params *rp, const artis_te_tables *tab,
                                const artis_te_params *par, const artis_ug_prepare *pr, const artis_te_cells *in,
                                int npts_model, int nthreads) {
  if (rp->nlte_pops_on || rp->no_lut_photoion || rp->no_lut_bfheating || rp->nt_on) return ARTIS_ERR_UNSUPPORTED;
  const int nel = at->nelements, mx = at->maxnions;
  artis_cell_state cs;
  memset(&cs, 0, sizeof(cs));
  cs.Te = in->Te;
  cs.TJ = in->TJ;
  cs.TR = in->TR;
  cs.W = in->W;
  cs.nne = pr->nne;
  cs.rho = in->rho;
  cs.elem_abundance = in->elem_abundance;
  cs.groundlevelpop = in->groundlevelpop;
  cs.partfunct = pr->partfunct;
  Ctx c;
  c.at = at;
  c.g = nullptr;
  c.cs = &cs;
  c.rp = *rp;
  c.gs = nullptr;
  c.T_step_log = (log(at->maxtemp) - log(at->mintemp)) / (at->tablesize - 1.);
  c.minpop = rp->minpop > 0. ? rp->minpop : 1e-30;
  if (nthreads > 0) omp_set_num_threads(nthreads);
  int nfail = 0;  // the reference's [fatal] aborts (update_grid.cc:911-918, 959-965)
#pragma omp parallel for schedule(dynamic) reduction(+ : nfail)
  for (int kk = 0; kk < in->ncells; kk++) {
    const int mgi = in->mgi[kk];
    const size_t row = (size_t)mgi * nel * mx;
    const double deltaV = in->vol_init[mgi] * pow(pr->tratmid, 3);
    const double estimator_normfactor = 1 / deltaV / pr->deltat / pr->nprocs;
    const double estimator_normfactor_over4pi = ARTIS_ONEOVER4PI * estimator_normfactor;
    const double J = pr->J[mgi] * estimator_normfactor_over4pi;  // radfield::normalise_J
    float TR = in->TR[mgi], W = in->W[mgi], TJ = in->TJ[mgi];
    pr->ffheating_out[mgi] = pr->ffheating[mgi];
    pr->colheating_out[mgi] = pr->colheating[mgi];
    for (int q = 0; q < nel * mx; q++) {
      pr->gamma_out[row + q] = pr->gammaestimator[row + q];
      pr->bfheating_out[row + q] = pr->bfheatingestimator[row + q];
    }
    if (par->initial_iteration || in->thick[mgi] == 1) {
      // update_grid.cc:1111-1120, radfield.cc:1464-1481 get_T_J_from_J
      double T_J = pow(J * ARTIS_PI / ARTIS_STEBO, 1. / 4.);
      if (!std::isfinite(T_J))
        T_J = in->TR[mgi];
      else if (T_J > par->T_max)
        T_J = par->T_max;
      else if (T_J < par->T_min)
        T_J = par->T_min;
      TR = T_J;
      TJ = T_J;
      W = 1;
      for (int q = 0; q < nel * mx; q++) pr->corrphotoionrenorm_out[row + q] = 1.;  // set_all_corrphotoionrenorm
    } else {
      const double nuJ = pr->nuJ[mgi] * estimator_normfactor_over4pi;  // radfield::normalise_nuJ
      pr->ffheating_out[mgi] = pr->ffheating[mgi] * estimator_normfactor;
      pr->colheating_out[mgi] = pr->colheating[mgi] * estimator_normfactor;
      // update_grid.cc:888-975 with the previous T_R, W (fit_parameters comes after)
      const double W_old = in->W[mgi], TR_old = in->TR[mgi];
      for (int e = 0; e < nel; e++)
        for (int i = 0; i < get_nions(c, e) - 1; i++) {
          const size_t ix = row + e * mx + i;
          const double g = pr->gammaestimator[ix] * (estimator_normfactor / ARTIS_H);
          pr->corrphotoionrenorm_out[ix] = g / (W_old * lut_at(c, at->corrphotoioncoeff, e, i, 0, 0, TR_old));
          if (!std::isfinite(pr->corrphotoionrenorm_out[ix])) nfail++;  // update_grid.cc:911-918
        }
      for (int e = 0; e < nel; e++)
        for (int i = 0; i < get_nions(c, e) - 1; i++) {
          const size_t ix = row + e * mx + i;
          // ratecoeff.cc:1353-1389 calculate_iongamma_per_gspop
          const float T_e = c.cs->Te[mgi];
          const float nne = c.cs->nne[mgi];
          double Gamma = 0., Col_ion = 0.;
          for (int level = 0; level < get_nlevels(c, e, i); level++) {
            const double nnlevel = calculate_levelpop(c, mgi, e, i, level);
            for (int t = 0; t < get_nphixstargets(c, e, i, level); t++) {
              const int upperlevel = get_phixsupperlevel(c, e, i, level, t);
              // get_corrphotoioncoeff (ratecoeff.cc:1255-1290, LUT branch)
              double gammacorr = W_old * lut_at(c, at->corrphotoioncoeff, e, i, level, t, TR_old);
              const int gi = at->level_closestgroundlevelcont[ulev(c, e, i, level)];
              if (gi >= 0) gammacorr *= pr->corrphotoionrenorm_out[row + gi];
              Gamma += nnlevel * gammacorr;
              const double epsilon_trans = epsilon(c, e, i + 1, upperlevel) - epsilon(c, e, i, level);
              Col_ion += nnlevel * col_ionization_ratecoeff(c, T_e, nne, e, i, level, t, epsilon_trans);
            }
          }
          Gamma += Col_ion;
          Gamma /= get_groundlevelpop(c, mgi, e, i);
          pr->gamma_out[ix] = Gamma;
          const double b = pr->bfheatingestimator[ix] * estimator_normfactor;
          const double ana = W_old * lut_at(c, tab->bfheating_coeff, e, i, 0, 0, TR_old);  // get_bfheatingcoeff_ana
          pr->bfheating_out[ix] = b / ana;
          if (!std::isfinite(pr->bfheating_out[ix])) nfail++;  // update_grid.cc:959-965
        }
      // radfield.cc:1136-1175 set_params_fullspec
      const double nubar = nuJ / J;
      if (std::isfinite(nubar) && nubar != 0.) {
        float T_J = pow(J * ARTIS_PI / ARTIS_STEBO, 1 / 4.);
        if (T_J > par->T_max)
          T_J = par->T_max;
        else if (T_J < par->T_min)
          T_J = par->T_min;
        TJ = T_J;
        float T_R = ARTIS_H * nubar / ARTIS_KB / 3.832229494;
        if (T_R > par->T_max)
          T_R = par->T_max;
        else if (T_R < par->T_min)
          T_R = par->T_min;
        TR = T_R;
        W = J * ARTIS_PI / ARTIS_STEBO / pow(T_R, 4);
      }
    }
    pr->TR_out[mgi] = TR;
    pr->W_out[mgi] = W;
    pr->TJ_out[mgi] = TJ;
  }
  return nfail ? ARTIS_ERR_PACKET_FAULT : 0;
}
}  // extern "C"

// update_grid for the nebular options (the checker of artis_gpu_update_grid_nlte)
#include "nebular_update_grid.cc"
