// ratecoeff_tables.h -- the host side of the rate-coefficient lookup tables (ratecoeff.cc:450-625, 686-710, 970-992)
// that needs no device: the table temperatures, the list of continua in get_bflutindex order, the clamp every table
// entry passes through, and precalculate_ion_alpha_sp.  Plain C++ on include/artis_gpu.h alone, so it compiles by
// itself (tests/ratecoeff_tables_check.cpp); ratecoeff_lut.h uses the clamp on the device, ratecoeff_host.h the rest.
#ifndef ARTIS_RATECOEFF_TABLES_H
#define ARTIS_RATECOEFF_TABLES_H

#include <cmath>
#include <cstdint>
#include <vector>

#include "artis_gpu.h"

#if defined(__HIPCC__)
#define ARTIS_RC_HD __host__ __device__
#else
#define ARTIS_RC_HD
#endif

// one bf continuum of the tables: (element, ion, level, phixs target); its position in the list is its column
// -1 - cont_index + target of get_bflutindex (sn3d.h:64-69)
struct RcCont {
  int32_t e, i, l, t;
};

// ratecoeff.cc:524-533, 574-579, 594-598, 611-618: a negative or non-finite coefficient is stored as 0
ARTIS_RC_HD inline double ratecoeff_clamp(double v) { return (!std::isfinite(v) || v < 0) ? 0. : v; }

// ratecoeff.cc:1004
inline double ratecoeff_T_step_log(double mintemp, double maxtemp, int tablesize) {
  return (std::log(maxtemp) - std::log(mintemp)) / (tablesize - 1.);
}

// ratecoeff.cc:492, 972: the table temperature is a float
inline float ratecoeff_table_temperature(double mintemp, double T_step_log, int iter) {
  const float T_e = mintemp * std::exp(iter * T_step_log);
  return T_e;
}

// atomic.cc:408-422 get_nphixstargets on the flattened tables
inline int ratecoeff_nphixstargets(const artis_atomic_tables *a, int e, int i, int l) {
  const int ui = a->elem_uniqueionoffset[e] + i;
  if (i < a->elem_nions[e] - 1 && l < a->ion_ionisinglevels[ui])
    return a->level_nphixstargets[a->ion_uniqueleveloffset[ui] + l];
  return 0;
}

// The continua in the loop order of precalculate_rate_coefficient_integrals (ratecoeff.cc:456-476), each placed at
// its get_bflutindex column.  false: a column outside [0, nbfcontinua) or taken twice (inconsistent cont_index).
inline bool ratecoeff_continua(const artis_atomic_tables *a, std::vector<RcCont> *out) {
  const int nbf = a->nbfcontinua;
  out->assign(nbf > 0 ? nbf : 0, RcCont{-1, -1, -1, -1});
  int found = 0;
  for (int e = 0; e < a->nelements; e++)
    for (int i = 0; i < a->elem_nions[e] - 1; i++) {
      const int ui = a->elem_uniqueionoffset[e] + i;
      for (int l = 0; l < a->ion_ionisinglevels[ui]; l++) {
        const int ul = a->ion_uniqueleveloffset[ui] + l;
        for (int t = 0; t < ratecoeff_nphixstargets(a, e, i, l); t++) {
          const int64_t col = -1 - (int64_t)a->level_cont_index[ul] + t;
          if (col < 0 || col >= nbf || (*out)[col].e >= 0) return false;
          (*out)[col] = RcCont{e, i, l, t};
          found++;
        }
      }
    }
  return found == nbf;
}

// ratecoeff.cc:686-710 get_spontrecombcoeff on a [tablesize * nbfcontinua] table, column `col`
inline double ratecoeff_interpolate_spontrecomb(const double *spontrecombcoeff, int nbf, int tablesize, double mintemp,
                                                double T_step_log, int col, float T_e) {
  const int lowerindex = std::floor(std::log(T_e / mintemp) / T_step_log);
  if (lowerindex < tablesize - 1) {
    const int upperindex = lowerindex + 1;
    const double T_lower = mintemp * std::exp(lowerindex * T_step_log);
    const double T_upper = mintemp * std::exp(upperindex * T_step_log);
    const double f_upper = spontrecombcoeff[(size_t)upperindex * nbf + col];
    const double f_lower = spontrecombcoeff[(size_t)lowerindex * nbf + col];
    return (f_lower + (f_upper - f_lower) / (T_upper - T_lower) * (T_e - T_lower));
  }
  return spontrecombcoeff[(size_t)(tablesize - 1) * nbf + col];
}

// ratecoeff.cc:970-992 precalculate_ion_alpha_sp: per ion and table temperature the sum of get_spontrecombcoeff over
// the ion's ionising levels and their targets, looked up at the float T_e (so the floor() of the lookup may land one
// row below iter, as it does in the reference); the top ion of an element keeps 0.  ion_alpha_sp [nions_total *
// tablesize] is OVERWRITTEN.  A lookup below row 0 (the reference's assert_always) returns false.
inline bool ratecoeff_ion_alpha_sp(const artis_atomic_tables *a, const double *spontrecombcoeff, float *ion_alpha_sp) {
  const int nbf = a->nbfcontinua, ts = a->tablesize;
  const double T_step_log = ratecoeff_T_step_log(a->mintemp, a->maxtemp, ts);
  for (size_t k = 0; k < (size_t)a->nions_total * ts; k++) ion_alpha_sp[k] = 0.f;
  for (int iter = 0; iter < ts; iter++) {
    const float T_e = ratecoeff_table_temperature(a->mintemp, T_step_log, iter);
    if (std::floor(std::log(T_e / a->mintemp) / T_step_log) < 0) return false;
    for (int e = 0; e < a->nelements; e++)
      for (int i = 0; i < a->elem_nions[e] - 1; i++) {
        const int ui = a->elem_uniqueionoffset[e] + i;
        double zeta = 0.;
        for (int l = 0; l < a->ion_ionisinglevels[ui]; l++) {
          const int ul = a->ion_uniqueleveloffset[ui] + l;
          for (int t = 0; t < ratecoeff_nphixstargets(a, e, i, l); t++) {
            const int col = -1 - a->level_cont_index[ul] + t;
            zeta += ratecoeff_interpolate_spontrecomb(spontrecombcoeff, nbf, ts, a->mintemp, T_step_log, col, T_e);
          }
        }
        ion_alpha_sp[(size_t)ui * ts + iter] = zeta;
      }
  }
  return true;
}

#endif
