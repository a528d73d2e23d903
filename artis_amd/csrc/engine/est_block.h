// est_block.h -- the estimator block, described once: the ordered sections of the packed double block the device
// accumulates into, the all-reduce sums and artis_estimator_block_pack / _unpack mirror on the host (documented at
// artis_estimator_block_len in artis_gpu.h), each with the member of artis_estimators it carries, and the walks over
// that description.  Pure host code like nlte_tables.h: no HIP call, no engine state (tests/est_block_check.cpp
// includes this file alone).  It defines the host-only entry points artis_estimator_block_*: include it once.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "artis_gpu.h"

namespace {

enum EstKind {  // how a section's member is carried in the block's doubles
  EK_F64,       // double array
  EK_SCALARS,   // the scalar group: EST_SCALAR, then pellet_decays (int64)
  EK_I64,       // int64 array (llrint back)
  EK_F32,       // float array
  EK_I32,       // int32 line counters (llrint back)
  EK_TAIL       // int64 members inside the struct (counters, nesc); on the device DevEst::counters, not the block
};

enum EstSec {  // the sections in block order
  ES_J, ES_NUJ, ES_FFHEAT, ES_COLHEAT, ES_RPKT_EMISS, ES_GAMMA, ES_BFHEAT, ES_SCALARS, ES_BFRATE, ES_RFJ, ES_RFNUJ,
  ES_RFCOUNT, ES_COMPTON, ES_ECOUNTER, ES_ACOUNTER, ES_COUNTERS, ES_NESC, ES_COUNT
};

struct EstSection {
  int64_t off, n;  // doubles
  EstKind kind;
  size_t member;  // offsetof in artis_estimators: a pointer to the array, for EK_TAIL the int64s themselves
};

struct EstBlock {
  EstSection s[ES_COUNT];
  int64_t n_device;  // doubles before ecounter: the device's double block (its counters are integer arrays, DevEst)
  int64_t len;
  int64_t tail() const { return len - n_device; }  // ecounter, acounter, counters, nesc
};

// the scalar group in the order of artis_gpu.h; mpi_reduce_estimators averages the first EST_AVERAGED over the ranks
// after the sum (sn3d.cc:370-377)
typedef artis_estimators AE;
constexpr double AE::*EST_SCALAR[] = {&AE::cmf_lum,           &AE::gamma_dep, &AE::positron_dep,   &AE::electron_dep,
                                      &AE::electron_emission, &AE::alpha_dep, &AE::alpha_emission, &AE::gamma_emission,
                                      &AE::nt_energy_deposited};
constexpr int EST_NSCALAR = sizeof(EST_SCALAR) / sizeof(EST_SCALAR[0]), EST_AVERAGED = 8;

// nbf / nbins: the nebular sections per cell, 0 when their option is off
inline EstBlock est_block(int64_t np, int64_t ne, int64_t mi, int64_t nl, int64_t nbf, int64_t nbins) {
  const int64_t ni = np * ne * mi;
  EstBlock B{{{0, np, EK_F64, offsetof(AE, J)},
              {0, np, EK_F64, offsetof(AE, nuJ)},
              {0, np, EK_F64, offsetof(AE, ffheatingestimator)},
              {0, np, EK_F64, offsetof(AE, colheatingestimator)},
              {0, np, EK_F64, offsetof(AE, rpkt_emiss)},
              {0, ni, EK_F64, offsetof(AE, gammaestimator)},
              {0, ni, EK_F64, offsetof(AE, bfheatingestimator)},
              {0, EST_NSCALAR + 1, EK_SCALARS, 0},
              {0, np * nbf, EK_F64, offsetof(AE, bfrate_raw)},
              {0, np * nbins, EK_F64, offsetof(AE, radfield_J_raw)},
              {0, np * nbins, EK_F64, offsetof(AE, radfield_nuJ_raw)},
              {0, np * nbins, EK_I64, offsetof(AE, radfield_contribcount)},
              {0, (np + 1) * ARTIS_EMISS_MAX, EK_F32, offsetof(AE, compton_emiss)},
              {0, nl, EK_I32, offsetof(AE, ecounter)},
              {0, nl, EK_I32, offsetof(AE, acounter)},
              {0, ARTIS_COUNTER_COUNT, EK_TAIL, offsetof(AE, counters)},
              {0, 1, EK_TAIL, offsetof(AE, nesc)}},
             0, 0};
  for (EstSection &S : B.s) {
    S.off = B.len;
    B.len += S.n;
  }
  B.n_device = B.s[ES_ECOUNTER].off;
  return B;
}

// f(typed pointer to the section's member in *e; NULL: an array not given)
template <typename F>
void est_member(const AE *e, const EstSection &S, F f) {
  char *at = (char *)e + S.member;
  if (S.kind != EK_TAIL) at = *(char **)at;
  switch (S.kind) {
    case EK_F64: return f((double *)at);
    case EK_F32: return f((float *)at);
    case EK_I32: return f((int32_t *)at);
    default: return f((int64_t *)at);
  }
}

// n elements into the block's doubles; an array not given packs as zeros
template <typename T>
void est_get(const T *src, int64_t n, double *b) {
  for (int64_t j = 0; j < n; j++) b[j] = src ? (double)src[j] : 0.;
}

// ... and back: overwritten or, add, added onto what is there (the float array summed in double); counts through
// llrint.  An array not given is skipped.
template <typename T>
void est_put(T *dst, int64_t n, const double *b, bool add) {
  for (int64_t j = 0; dst && j < n; j++)
    if constexpr (std::is_floating_point<T>::value)
      dst[j] = (T)(add ? (double)dst[j] + b[j] : b[j]);
    else
      dst[j] = (T)((add ? (long long)dst[j] : 0) + llrint(b[j]));
}

inline void est_block_pack(const EstBlock &B, const AE *est, double *b) {
  for (const EstSection &S : B.s)
    if (S.kind != EK_SCALARS) est_member(est, S, [&](auto *p) { est_get(p, S.n, b + S.off); });
  double *sc = b + B.s[ES_SCALARS].off;
  for (int j = 0; j < EST_NSCALAR; j++) sc[j] = est->*EST_SCALAR[j];
  sc[EST_NSCALAR] = (double)est->pellet_decays;
}

// unpack (overwrite) or, add, what artis_gpu_estimators_download does with the device's sums
inline void est_block_unpack(const EstBlock &B, const double *b, AE *est, bool add) {
  for (const EstSection &S : B.s)
    if (S.kind != EK_SCALARS) est_member(est, S, [&](auto *p) { est_put(p, S.n, b + S.off, add); });
  const double *sc = b + B.s[ES_SCALARS].off;
  for (int j = 0; j < EST_NSCALAR; j++) est_put(&(est->*EST_SCALAR[j]), 1, sc + j, add);
  est_put(&est->pellet_decays, 1, sc + EST_NSCALAR, add);
}

// The device's double block: the named offsets (doubles) lay_out_estimators_on_device wires DevEst from, and the
// description they are read off, kept for the readout side
struct EstLayout {
  int64_t J, nuJ, ffheat, colheat, rpkt_emiss, gamma, bfheat, scalars, bfrate, rfJ, rfnuJ, rfcount, compton;
  int64_t n_doubles;  // = block.n_device
  EstBlock block;
};

inline EstLayout lay_out_estimators(const artis_atomic_tables *a, const artis_geometry *g, const artis_run_params *rp) {
  const EstBlock B =
      est_block(g->npts_model, a->nelements, a->maxnions, a->nlines, rp->detailed_bf_estimators ? a->nbfcontinua : 0,
                rp->multibin_radfield ? a->radfield_nbins : 0);
  const EstSection *S = B.s;
  return {S[ES_J].off,      S[ES_NUJ].off,     S[ES_FFHEAT].off, S[ES_COLHEAT].off, S[ES_RPKT_EMISS].off,
          S[ES_GAMMA].off,  S[ES_BFHEAT].off,  S[ES_SCALARS].off, S[ES_BFRATE].off, S[ES_RFJ].off,
          S[ES_RFNUJ].off,  S[ES_RFCOUNT].off, S[ES_COMPTON].off, B.n_device,       B};
}

}  // namespace

// ------------------------------------------------------- the host mirror of the device block (artis_gpu.h)
extern "C" {

size_t artis_estimator_block_len(int np, int ne, int mi, int nl, int nbf, int nbins) {
  if (np < 0 || ne < 0 || mi < 0 || nl < 0 || nbf < 0 || nbins < 0) return 0;
  return (size_t)est_block(np, ne, mi, nl, nbf, nbins).len;
}

int artis_estimator_block_pack(const artis_estimators *est, int np, int ne, int mi, int nl, int nbf, int nbins,
                               double *b) {
  if (!est || !b || np < 0 || ne < 0 || mi < 0 || nl < 0 || nbf < 0 || nbins < 0) return ARTIS_ERR_BAD_ARGUMENT;
  est_block_pack(est_block(np, ne, mi, nl, nbf, nbins), est, b);
  return 0;
}

int artis_estimator_block_unpack(const double *b, int np, int ne, int mi, int nl, int nbf, int nbins,
                                 artis_estimators *est) {
  if (!est || !b || np < 0 || ne < 0 || mi < 0 || nl < 0 || nbf < 0 || nbins < 0) return ARTIS_ERR_BAD_ARGUMENT;
  est_block_unpack(est_block(np, ne, mi, nl, nbf, nbins), b, est, false);
  return 0;
}

int artis_estimator_block_average_scalars(double *b, int np, int ne, int mi, int nranks) {
  if (!b || np < 0 || ne < 0 || mi < 0 || nranks <= 0) return ARTIS_ERR_BAD_ARGUMENT;
  double *sc = b + est_block(np, ne, mi, 0, 0, 0).s[ES_SCALARS].off;
  for (int j = 0; j < EST_AVERAGED; j++) sc[j] /= nranks;
  return 0;
}

}  // extern "C"
