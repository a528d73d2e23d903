// ratecoeff_lut.h -- the rate-coefficient lookup tables on the GPU: precalculate_rate_coefficient_integrals
// (ratecoeff.cc:450-625), for every (bf continuum, table temperature) up to four gsl_integration_qag(GAUSS61)
// integrals over the level's cross-section table, one wave per (continuum, temperature).
//
// The integrator is qag.h's restatement of GSL's (the 61 integrand evaluations of a rule on the wave's lanes, the
// bookkeeping identical on every lane).  These integrands are smooth between the kinks of the piecewise-linear cross
// section, so an integral ends after a few bisections: the error list keeps RC_LIST_DEFAULT entries in LDS (the rest
// of GSLWSIZE in the wave's global workspace, never reached at the reference's accuracies), which leaves the block at
// about 5 KB of LDS and the occupancy to the registers (one wave per SIMD, see RC_MIN_WAVES).  Items are numbered continuum-major and a block takes a
// contiguous range of them, so a wave meets the temperatures of one level in a row and keeps the level's cross-section
// row in LDS across them.  Lane 0 stores; nothing is accumulated, so two calls give the same bits.
#ifndef ARTIS_RATECOEFF_LUT_H
#define ARTIS_RATECOEFF_LUT_H

#include "qag.h"
#include "ratecoeff_tables.h"

#define RC_LIST_DEFAULT 64  // error-list entries in LDS (the most any integral of the test atom needs at 1e-6)
#define RC_LIST_SMALL 16    // the second instantiation: tests drive the spill into the global workspace with it
#define RC_XS_LDS 1024      // cross-section rows up to this many points are staged in LDS (NPHIXSPOINTS is 100)

struct RcArgs {
  const RcCont *cont;  // [ncont] in get_bflutindex column order
  const float *T_e;    // [tablesize] table temperatures (host-evaluated: ratecoeff.cc:492)
  int32_t ncont, tablesize;
  double epsrel;
  // [tablesize * ncont], get_bflutindex order; corrphotoioncoeff / bfheating_coeff NULL: that integral is skipped
  double *spontrecombcoeff, *corrphotoioncoeff, *bfheating_coeff, *bfcooling_coeff;
  uint8_t *status;     // [4][tablesize * ncont] or NULL
  int32_t *intervals;  // [4][tablesize * ncont] or NULL
};

#ifndef RC_MIN_WAVES
// waves per SIMD the kernel is compiled for.  1: 256 VGPRs + 146 AGPRs, no scratch.  2 halves the registers and spills
// 624 bytes per lane to scratch: 17.0 ms against 8.4 ms on the bench atom, so 1 it is.
#define RC_MIN_WAVES 1
#endif

template <int CAP>
__global__ __launch_bounds__(64, RC_MIN_WAVES) void k_ratecoeff_lut(Ctx K, RcArgs A, QagWs ws) {
  __shared__ double s_f[64];
  __shared__ double s_el[CAP];
  __shared__ int32_t s_ord[CAP];
  __shared__ float s_xs[RC_XS_LDS];
  const int lane = threadIdx.x & 63;
  const int64_t total = (int64_t)A.ncont * A.tablesize;
  const int64_t per = (total + gridDim.x - 1) / gridDim.x;
  const int64_t first = (int64_t)blockIdx.x * per;
  const int64_t last = first + per < total ? first + per : total;
  const int64_t wbase = (int64_t)blockIdx.x * QAG_LIMIT;
  double *al = ws.alist + wbase, *bl = ws.blist + wbase, *rl = ws.rlist + wbase;
  int32_t *lev = ws.level + wbase;
  const QagListsT<CAP> Q{s_el, s_ord, ws.elist + wbase, ws.order + wbase};
  const int npts = K.T.nphixspoints;
  const int64_t lutsize = total;
  int staged_table = -1;
  for (int64_t item = first; item < last; item++) {
    const int col = (int)(item / A.tablesize);
    const int iter = (int)(item % A.tablesize);
    const RcCont c = A.cont[col];
    const int e = c.e, i = c.i, l = c.l, t = c.t;
    const int table = K.T.level_phixstable[ulev(K, e, i, l)];
    const float *xs = K.T.phixs_xs + (int64_t)table * npts;
    if (npts <= RC_XS_LDS) {
      if (table != staged_table) {
        __syncthreads();  // the previous level's integrals have read their row
        for (int k = lane; k < npts; k += 64) s_xs[k] = xs[k];
        __syncthreads();
        staged_table = table;
      }
      xs = s_xs;
    }
    const int upperlevel = get_phixsupperlevel(K, e, i, l, t);
    const double phixstargetprobability = get_phixsprobability(K, e, i, l, t);
    const double E_threshold = get_phixs_threshold(K, e, i, l, t);
    const double nu_threshold = E_threshold / ARTIS_H;
    const double nu_max_phixs = nu_threshold * K.T.last_phixs_nuovernuedge;
    const float T_e = A.T_e[iter];
    const double sfac = calculate_sahafact(K, e, i, l, upperlevel, T_e, E_threshold);
    const double nu_edge = nu_threshold;
    const float T = T_e;
    const int64_t idx = (int64_t)iter * A.ncont + col;
    double value = 0., error = 0.;
    int n = 0;
    auto note = [&](int which, int status) {
      if (lane == 0) {
        if (A.status) A.status[which * lutsize + idx] = (uint8_t)status;
        if (A.intervals) A.intervals[which * lutsize + idx] = n;
      }
    };

    // alpha_sp_integrand_gsl (ratecoeff.cc:249-262), scaled as ratecoeff.cc:524
    {
      auto f = [&](double nu) {
        const float sigma_bf = (float)photoionization_crosssection_fromtable(K, xs, nu_edge, nu);
        const double x = ARTIS_TWOOVERCLIGHTSQUARED * sigma_bf * pow(nu, 2) * exp(-ARTIS_HOVERKB * nu / T);
        return x;
      };
      const int st = qag61(f, nu_threshold, nu_max_phixs, 0., A.epsrel, al, bl, rl, Q, lev, s_f, &value, &error, &n);
      note(0, st);
      double alpha_sp = value;
      alpha_sp *= ARTIS_FOURPI * sfac * phixstargetprobability;
      if (lane == 0) A.spontrecombcoeff[idx] = ratecoeff_clamp(alpha_sp);
    }
    // gammacorr_integrand_gsl (ratecoeff.cc:306-321), scaled as ratecoeff.cc:574
    if (A.corrphotoioncoeff) {
      auto f = [&](double nu) {
        const float sigma_bf = (float)photoionization_crosssection_fromtable(K, xs, nu_edge, nu);
        return sigma_bf * ARTIS_ONEOVERH / nu * dbb(nu, T, 1) * (1 - exp(-ARTIS_HOVERKB * nu / T));
      };
      const int st = qag61(f, nu_threshold, nu_max_phixs, 0., A.epsrel, al, bl, rl, Q, lev, s_f, &value, &error, &n);
      note(1, st);
      double gammacorr = value;
      gammacorr *= ARTIS_FOURPI * phixstargetprobability;
      if (lane == 0) A.corrphotoioncoeff[idx] = ratecoeff_clamp(gammacorr);
    } else {
      n = 0;
      note(1, 0);
    }
    // approx_bfheating_integrand_gsl (ratecoeff.cc:325-352), scaled as ratecoeff.cc:594
    if (A.bfheating_coeff) {
      auto f = [&](double nu) {
        const float sigma_bf = (float)photoionization_crosssection_fromtable(K, xs, nu_edge, nu);
        const double x = sigma_bf * (1 - nu_edge / nu) * dbb(nu, T, 1) * (1 - exp(-ARTIS_HOVERKB * nu / T));
        return x;
      };
      const int st = qag61(f, nu_threshold, nu_max_phixs, 0., A.epsrel, al, bl, rl, Q, lev, s_f, &value, &error, &n);
      note(2, st);
      double bfheating_coeff = value;
      bfheating_coeff *= ARTIS_FOURPI * phixstargetprobability;
      if (lane == 0) A.bfheating_coeff[idx] = ratecoeff_clamp(bfheating_coeff);
    } else {
      n = 0;
      note(2, 0);
    }
    // bfcooling_integrand_gsl (ratecoeff.cc:379-394), scaled as ratecoeff.cc:611
    {
      auto f = [&](double nu) {
        const float sigma_bf = (float)photoionization_crosssection_fromtable(K, xs, nu_edge, nu);
        return sigma_bf * (nu - nu_edge) * ARTIS_TWOHOVERCLIGHTSQUARED * nu * nu * exp(-ARTIS_HOVERKB * nu / T);
      };
      const int st = qag61(f, nu_threshold, nu_max_phixs, 0., A.epsrel, al, bl, rl, Q, lev, s_f, &value, &error, &n);
      note(3, st);
      double bfcooling_coeff = value;
      bfcooling_coeff *= ARTIS_FOURPI * sfac * phixstargetprobability;
      if (lane == 0) A.bfcooling_coeff[idx] = ratecoeff_clamp(bfcooling_coeff);
    }
  }
}

#endif
