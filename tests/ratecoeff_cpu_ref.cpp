// CPU yardsticks of the rate-coefficient lookup tables (tests/test_ratecoeff.py, tests/test_gpu_ratecoeff.py build this
// into a shared library).  It includes oracle/oracle.cc unchanged for its restatement of gsl_integration_qag(GAUSS61)
// (gsl_qag61), the cross-section lookup and calculate_sahafact, and exports for an artis_atomic_tables:
//   ratecoeff_cpu_qag:   the four tables of precalculate_rate_coefficient_integrals (ratecoeff.cc:450-625) through that
//                        qag at a given epsrel, with every integral's GSL status and final interval count;
//   ratecoeff_cpu_dense: the same four tables from a quadrature that knows where the integrands' kinks are: an 8-point
//                        Gauss-Legendre rule on each quarter of every interval of the cross-section table.
// Tables are [tablesize * nbfcontinua] in get_bflutindex order, status / intervals [4][tablesize * nbfcontinua] in the
// order alpha_sp, gammacorr, bfheating, bfcooling.
#include "../oracle/oracle.cc"

namespace {

struct RcRefCont {
  int e, i, l, t;
};

std::vector<RcRefCont> rc_ref_continua(const Ctx &c) {
  const artis_atomic_tables *a = c.at;
  std::vector<RcRefCont> out;
  for (int e = 0; e < a->nelements; e++)
    for (int i = 0; i < a->elem_nions[e] - 1; i++)
      for (int l = 0; l < get_ionisinglevels(c, e, i); l++)
        for (int t = 0; t < get_nphixstargets(c, e, i, l); t++) out.push_back({e, i, l, t});
  return out;
}

// the integrands of ratecoeff.cc:249-262, 306-321, 325-352, 379-394 (T and sigma_bf are floats there)
struct RcRefIntegrands {
  const Ctx &c;
  const float *xs;
  double nu_edge;
  float T;
  double alpha_sp(double nu) const {
    const float sigma_bf = photoionization_crosssection_fromtable(c, xs, nu_edge, nu);
    const double x = ARTIS_TWOOVERCLIGHTSQUARED * sigma_bf * pow(nu, 2) * exp(-ARTIS_HOVERKB * nu / T);
    return x;
  }
  double gammacorr(double nu) const {
    const float sigma_bf = photoionization_crosssection_fromtable(c, xs, nu_edge, nu);
    return sigma_bf * ARTIS_ONEOVERH / nu * dbb(nu, T, 1) * (1 - exp(-ARTIS_HOVERKB * nu / T));
  }
  double bfheating(double nu) const {
    const float sigma_bf = photoionization_crosssection_fromtable(c, xs, nu_edge, nu);
    const double x = sigma_bf * (1 - nu_edge / nu) * dbb(nu, T, 1) * (1 - exp(-ARTIS_HOVERKB * nu / T));
    return x;
  }
  double bfcooling(double nu) const {
    const float sigma_bf = photoionization_crosssection_fromtable(c, xs, nu_edge, nu);
    return sigma_bf * (nu - nu_edge) * ARTIS_TWOHOVERCLIGHTSQUARED * nu * nu * exp(-ARTIS_HOVERKB * nu / T);
  }
};

inline double rc_ref_clamp(double v) { return (!std::isfinite(v) || v < 0) ? 0. : v; }

const double kGl8x[4] = {0.1834346424956498, 0.5255324099163290, 0.7966664774136267, 0.9602898564975363};
const double kGl8w[4] = {0.3626837833783620, 0.3137066458778873, 0.2223810344533745, 0.1012285362903763};

template <typename F>
double rc_ref_dense(const F &f, const artis_atomic_tables *a, double nu_edge) {
  double sum = 0.;
  for (int k = 0; k < a->nphixspoints - 1; k++) {
    const double lo = nu_edge * (1. + a->nphixsnuincrement * k), hi = nu_edge * (1. + a->nphixsnuincrement * (k + 1));
    for (int q = 0; q < 4; q++) {
      const double qa = lo + (hi - lo) * 0.25 * q, qb = lo + (hi - lo) * 0.25 * (q + 1);
      const double mid = 0.5 * (qa + qb), half = 0.5 * (qb - qa);
      double s = 0.;
      for (int j = 0; j < 4; j++) s += kGl8w[j] * (f(mid - half * kGl8x[j]) + f(mid + half * kGl8x[j]));
      sum += s * half;
    }
  }
  return sum;
}

// dense = 1: the Gauss-Legendre tables; else qag at epsrel
int rc_ref_tables(const artis_atomic_tables *a, int dense, double epsrel, double *alpha_sp, double *gammacorr,
                  double *bfheating, double *bfcooling, uint8_t *status, int32_t *intervals, int nthreads) {
  Ctx c;
  c.at = a;
  const std::vector<RcRefCont> cont = rc_ref_continua(c);
  const int nbf = a->nbfcontinua, ts = a->tablesize;
  if ((int)cont.size() != nbf) return -1;
  const size_t lutsize = (size_t)ts * nbf;
  const double T_step_log = (log(a->maxtemp) - log(a->mintemp)) / (ts - 1.);
  int bad = 0;
#pragma omp parallel for schedule(dynamic) num_threads(nthreads > 0 ? nthreads : 16) reduction(+ : bad)
  for (int k = 0; k < nbf; k++) {
    const RcRefCont &j = cont[k];
    const int col = -1 - a->level_cont_index[ulev(c, j.e, j.i, j.l)] + j.t;
    if (col < 0 || col >= nbf) {
      bad++;
      continue;
    }
    GslWorkspace ws(kGslWsSize);
    const int upperlevel = get_phixsupperlevel(c, j.e, j.i, j.l, j.t);
    const double prob = get_phixsprobability(c, j.e, j.i, j.l, j.t);
    const double E_threshold = get_phixs_threshold(c, j.e, j.i, j.l, j.t);
    const double nu_threshold = E_threshold / ARTIS_H;
    const double nu_max_phixs = nu_threshold * a->last_phixs_nuovernuedge;
    for (int iter = 0; iter < ts; iter++) {
      const float T_e = a->mintemp * exp(iter * T_step_log);
      const double sfac = calculate_sahafact(c, j.e, j.i, j.l, upperlevel, T_e, E_threshold);
      const RcRefIntegrands I{c, level_photoion_xs(c, j.e, j.i, j.l), nu_threshold, T_e};
      const size_t idx = (size_t)iter * nbf + col;
      auto run = [&](int which, auto f) {
        double value = 0., error = 0.;
        if (dense) return rc_ref_dense(f, a, nu_threshold);
        const int st = gsl_qag61(f, nu_threshold, nu_max_phixs, 0., epsrel, kGslWsSize, ws, &value, &error);
        if (status) status[which * lutsize + idx] = (uint8_t)st;
        if (intervals) intervals[which * lutsize + idx] = (int32_t)ws.size;
        return value;
      };
      alpha_sp[idx] = rc_ref_clamp(run(0, [&](double nu) { return I.alpha_sp(nu); }) * ARTIS_FOURPI * sfac * prob);
      gammacorr[idx] = rc_ref_clamp(run(1, [&](double nu) { return I.gammacorr(nu); }) * ARTIS_FOURPI * prob);
      bfheating[idx] = rc_ref_clamp(run(2, [&](double nu) { return I.bfheating(nu); }) * ARTIS_FOURPI * prob);
      bfcooling[idx] = rc_ref_clamp(run(3, [&](double nu) { return I.bfcooling(nu); }) * ARTIS_FOURPI * sfac * prob);
    }
  }
  return bad ? -1 : 0;
}

}  // namespace

extern "C" {
int ratecoeff_cpu_qag(const artis_atomic_tables *a, double epsrel, double *alpha_sp, double *gammacorr,
                      double *bfheating, double *bfcooling, uint8_t *status, int32_t *intervals, int nthreads) {
  return rc_ref_tables(a, 0, epsrel, alpha_sp, gammacorr, bfheating, bfcooling, status, intervals, nthreads);
}
int ratecoeff_cpu_dense(const artis_atomic_tables *a, double *alpha_sp, double *gammacorr, double *bfheating,
                        double *bfcooling, int nthreads) {
  return rc_ref_tables(a, 1, 0., alpha_sp, gammacorr, bfheating, bfcooling, nullptr, nullptr, nthreads);
}
}
