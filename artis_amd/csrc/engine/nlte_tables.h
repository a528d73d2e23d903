// nlte_tables.h -- the tables update_grid's host drivers (update_grid_host.h) derive from the atomic bookkeeping
// before they upload them: the bf-heating level list, the mean binding energies, the Spencer-Fano grid with its
// shell and transition tables, the NLTE rate-matrix layout.  Pure host functions like host_tables.h: no HIP call,
// no engine state, nothing of engine.hip's kernels (tests/nlte_tables_check.cpp includes this file alone).  The
// expressions are the reference's, operand for operand (host libm): the GPU parity tests depend on their bits.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "artis_constants.h"
#include "artis_gpu.h"

namespace {

// host copies of the atomic bookkeeping (artis_atomic_tables names in the comments)
struct NlAtoms {
  int ne = 0, ni = 0, nl = 0;
  const int32_t *anumber = nullptr;    // [ne] elem_anumber
  const double *ion_ionpot = nullptr;  // [ni] ion_ionpot
  std::vector<int32_t> nions, uoff;    // [ne] elem_nions, elem_uniqueionoffset
  std::vector<int32_t> ion_nlev, ion_ul0, ionis, nlte_n, ionstage;  // [ni] ion_nlevels, ion_uniqueleveloffset,
                                                                    // ion_ionisinglevels, ion_nlevels_nlte, ion_ionstage
  std::vector<int32_t> lev_nup, lev_upoff;  // [nl] level_nuptrans, level_uptrans_offset
  std::vector<double> lev_eps;              // [nl] level_epsilon
  std::vector<float> lev_g;                 // [nl] level_stat_weight
  // the Spencer-Fano excitation transitions only
  std::vector<int32_t> line_upper, upidx;  // [nlines] line_upper, [uptrans] uptrans_lineindex
  std::vector<float> line_coll, line_f;    // [nlines]
  std::vector<uint8_t> line_forb;          // [nlines]
};

// calculate_heating_rates' bf-heating levels (thermalbalance.cc:304-310): the ionising levels of every ion but the
// top one, in element, ion, level order (needs nions, uoff, ionis, ion_ul0)
inline std::vector<int32_t> bfheat_levels(const NlAtoms &A) {
  std::vector<int32_t> hb;
  for (int e = 0; e < A.ne; e++)
    for (int i = 0; i < A.nions[e] - 1; i++)
      for (int l = 0; l < A.ionis[A.uoff[e] + i]; l++) hb.push_back(A.ion_ul0[A.uoff[e] + i] + l);
  return hb;
}

// nonthermal.cc:994-1007
inline double sf_get_J(int Z, int ionstage, double ionpot_ev) {
  if (ionstage == 1) {
    if (Z == 2) return 15.8;
    if (Z == 10) return 24.2;
    if (Z == 18) return 10.0;
  }
  return 0.6 * ionpot_ev;
}

// nonthermal.cc:1193-1309 get_mean_binding_energy over electron_binding [30 * 10]; false on the reference's abort
// paths
inline bool sf_mean_binding_energy(const double *electron_binding, int Zel, int ioncharge, double ionpot, double *out) {
  const int nbound = Zel - ioncharge;
  double total = 0.0;
  if (nbound > 0) {
    int q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int electron_loop = 0; electron_loop < nbound; electron_loop++) {
      if (q[0] < 2)
        q[0]++;
      else if (q[1] < 2)
        q[1]++;
      else if (q[2] < 2)
        q[2]++;
      else if (q[3] < 4)
        q[3]++;
      else if (q[4] < 2)
        q[4]++;
      else if (q[5] < 2)
        q[5]++;
      else if (q[6] < 4)
        q[6]++;
      else if (ioncharge == 0) {
        if (q[9] < 2)
          q[9]++;
        else if (q[7] < 4)
          q[7]++;
        else if (q[8] < 6)
          q[8]++;
        else
          return false;
      } else if (ioncharge == 1) {
        if (q[9] < 1)
          q[9]++;
        else if (q[7] < 4)
          q[7]++;
        else if (q[8] < 6)
          q[8]++;
        else
          return false;
      } else if (ioncharge > 1) {
        if (q[7] < 4)
          q[7]++;
        else if (q[8] < 6)
          q[8]++;
        else
          return false;
      }
    }
    if (Zel < 1 || Zel > 30) return false;
    for (int electron_loop = 0; electron_loop < 10; electron_loop++) {
      const double electronsinshell = q[electron_loop];
      if (electronsinshell > 0) {
        double use2 = electron_binding[(Zel - 1) * 10 + electron_loop];
        const double use3 = ionpot;
        if (use2 <= 0) {
          if (electron_loop != 8) return false;
          use2 = electron_binding[(Zel - 1) * 10 + electron_loop - 1];
        }
        if (use2 < use3)
          total += electronsinshell / use3;
        else
          total += electronsinshell / use2;
      }
    }
  }
  *out = total;
  return true;
}

// every ion's mean binding energy and whether the reference has one (0: it aborts if the work-function
// approximation is needed); without a table (nullptr) none has
inline void sf_ion_binding(const NlAtoms &A, const double *electron_binding, std::vector<double> &binding,
                           std::vector<int32_t> &binding_ok) {
  binding.assign(A.ni, 0.);
  binding_ok.assign(A.ni, 0);
  if (!electron_binding) return;
  for (int e = 0; e < A.ne; e++)
    for (int i = 0; i < A.nions[e]; i++) {
      const int u = A.uoff[e] + i;
      double bnd = 0.;
      binding_ok[u] = sf_mean_binding_energy(electron_binding, A.anumber[e], A.ionstage[u] - 1, A.ion_ionpot[u], &bnd) ? 1 : 0;
      binding[u] = bnd;
    }
}

// ------------------------------------------------------------------------------------------- Spencer-Fano
// The energy grid with its transcendentals, the shells of every ion (collion.txt entries matching (Z, ionstage))
// with their cross sections and the atan terms of sfmatrix_add_ionization, the excitation transitions (SfDev,
// nlte_solver.h, holds the device copies)
struct SfTables {
  int n = 0, band = 1;
  double emin = 0., emax = 0., DE = 0., E_init_ev = 0.;
  int source_spread_pts = 0;
  std::vector<double> envec, logenvec, sourcevec, pw2, rhs;  // [n]
  std::vector<int32_t> sh_off, sh_k, sh_start, sh_astop;     // sh_off: [ni + 1] CSR of the shell records
  std::vector<double> sh_ip, sh_J, sh_prob;                  // sh_prob: [nsh * (ARTIS_NT_MAX_AUGER + 1)]
  std::vector<double> sh_xs, sh_ieu, sh_atn, sh_ie2;         // [nsh * n]
  std::vector<int32_t> tr_off, tr_ul, tr_kind, tr_start, tr_build;  // tr_off: [ni + 1] CSR of the transitions
  std::vector<double> tr_cf, tr_logeps, tr_eps_ev, tr_eps;
};

inline SfTables sf_build_tables(const artis_nt_shells *nt, const NlAtoms &A) {
  constexpr int A1 = ARTIS_NT_MAX_AUGER + 1;
  SfTables S;
  const int n = nt->sfpts;
  S.n = n;
  S.emin = nt->sf_emin;
  S.emax = nt->sf_emax;
  S.DE = (S.emax - S.emin) / (n - 1);
  S.envec.resize(n);
  S.logenvec.resize(n);
  S.sourcevec.resize(n);
  S.pw2.resize(n);
  S.rhs.assign(n, 0.);
  std::vector<double> &envec = S.envec, &sourcevec = S.sourcevec;
  S.source_spread_pts = (int)ceil(n * 0.03333);
  const double source_spread_en = S.source_spread_pts * S.DE;
  const int sourcelowerindex = n - S.source_spread_pts;
  for (int k = 0; k < n; k++) {
    envec[k] = S.emin + k * S.DE;
    S.logenvec[k] = log(envec[k]);
    sourcevec[k] = (k < sourcelowerindex) ? 0. : 1. / source_spread_en;
    S.pw2[k] = pow(envec[k] * ARTIS_EV, -2);
  }
  double E = 0.;
  for (int k = 0; k < n; k++) E += fabs((sourcevec[k] * S.DE) * envec[k]);
  S.E_init_ev = E;
  for (int i = 0; i < n - 1; i++) {
    double dasum = 0.;
    for (int j = i + 1; j < n; j++) dasum += fabs(sourcevec[j]);
    S.rhs[i] = dasum * S.DE;
  }
  auto gteq = [&S, n](double en) {
    const int index = (int)ceil((en - S.emin) / S.DE);
    return index < 0 ? 0 : (index > n - 1 ? n - 1 : index);
  };
  S.sh_off.assign(A.ni + 1, 0);
  S.tr_off.assign(A.ni + 1, 0);
  for (int e = 0; e < A.ne; e++)
    for (int i = 0; i < A.nions[e]; i++) {
      const int u = A.uoff[e] + i;
      const int Z = A.anumber[e];
      const int ist = A.ionstage[u];
      for (int k = 0; k < nt->nshells; k++) {
        if (!(nt->Z[k] == Z && nt->nelec[k] == Z - ist + 1)) continue;
        const double ionpot_ev = nt->ionpot_ev[k];
        const double J = sf_get_J(Z, ist, ionpot_ev);
        const int xsstart = gteq(ionpot_ev);
        S.sh_k.push_back(k);
        S.sh_ip.push_back(ionpot_ev);
        S.sh_J.push_back(J);
        S.sh_start.push_back(xsstart);
        S.sh_astop.push_back(gteq((double)nt->en_auger_ev[k]));
        for (int q = 0; q < A1; q++) S.sh_prob.push_back(nt->prob_num_auger[k * A1 + q]);
        const double Ac = nt->A[k], Bc = nt->B[k], Cc = nt->C[k], Dc = nt->D[k];
        for (int j = 0; j < n; j++) {  // nonthermal.cc:952-976, 2370-2380
          double xs = 0., ieu = 0., atn = 0.;
          if (j >= xsstart) {
            const double uu = envec[j] / ionpot_ev;
            xs = 1e-14 * (Ac * (1 - 1 / uu) + Bc * pow((1 - 1 / uu), 2) + Cc * log(uu) + Dc * log(uu) / uu) /
                 (uu * pow(ionpot_ev, 2));
            const double endash = envec[j];
            const double epsilon_upper = std::min((endash + ionpot_ev) / 2, endash);
            ieu = atan((epsilon_upper - ionpot_ev) / J);
            atn = atan((endash - ionpot_ev) / 2 / J);
          }
          S.sh_xs.push_back(xs);
          S.sh_ieu.push_back(ieu);
          S.sh_atn.push_back(atn);
          S.sh_ie2.push_back(atan(envec[j] / J));
        }
      }
      S.sh_off[u + 1] = (int32_t)S.sh_k.size();
      // excitation transitions (nonthermal.cc:2282-2341, 872-929)
      const int nlev5 = std::min(A.ion_nlev[u], 5);
      for (int lower = 0; lower < nlev5; lower++) {
        const int ul = A.ion_ul0[u] + lower;
        const double statweight_lower = A.lev_g[ul];
        for (int t = 0; t < A.lev_nup[ul]; t++) {
          const int li = A.upidx[A.lev_upoff[ul] + t];
          const int upper = A.line_upper[li];
          if (upper >= 250) continue;
          const double epsilon_trans = A.lev_eps[A.ion_ul0[u] + upper] - A.lev_eps[ul];
          const double eps_ev = epsilon_trans / ARTIS_EV;
          const double coll_str = A.line_coll[li];
          int kind;
          double cf, logeps = 0.;
          if (coll_str >= 0) {
            kind = 0;
            cf = pow(ARTIS_H_IONPOT, 2) / statweight_lower * coll_str * ARTIS_PI * 2.800285203e-17;
          } else if (!A.line_forb[li]) {
            kind = 1;
            const double fij = A.line_f[li];
            cf = eps_ev * 45.585750051 * 2.800285203e-17 * pow(ARTIS_H_IONPOT / epsilon_trans, 2) * fij;
            logeps = log(eps_ev);
          } else {
            continue;
          }
          S.tr_ul.push_back(ul);
          S.tr_kind.push_back(kind);
          S.tr_start.push_back(gteq(eps_ev));
          S.tr_build.push_back(!(eps_ev < S.emin));
          S.tr_cf.push_back(cf);
          S.tr_logeps.push_back(logeps);
          S.tr_eps_ev.push_back(eps_ev);
          S.tr_eps.push_back(epsilon_trans);
          if (!(eps_ev < S.emin)) S.band = std::max(S.band, (int)ceil(eps_ev / S.DE) + 2);
        }
      }
      S.tr_off[u + 1] = (int32_t)S.tr_ul.size();
    }
  return S;
}

// ------------------------------------------------------------------------------------------ NLTE populations
// the rate-matrix layout (NlMat, nlte_solver.h): per element D = sum over ions of nlevels_nlte + 1 (+ 1 with a
// superlevel), a column per ground / NLTE level and one for the superlevel's level range
struct NlLayout {
  std::vector<int32_t> el_D, el_off1, col_e, col_ion, col_l0, col_l1;
  std::vector<int64_t> el_off2;
  int cell1 = 0;      // sum over elements of D_e
  int64_t cell2 = 0;  // sum of D_e^2
};

// false: an ion with fewer levels than nlevels_nlte + 1
inline bool nl_matrix_layout(const NlAtoms &A, NlLayout &L) {
  L = NlLayout();
  L.el_D.assign(A.ne, 0);
  L.el_off1.assign(A.ne, 0);
  L.el_off2.assign(A.ne, 0);
  for (int e = 0; e < A.ne; e++) {
    L.el_off1[e] = L.cell1;
    L.el_off2[e] = L.cell2;
    int Dm = 0;
    for (int i = 0; i < A.nions[e]; i++) {
      const int u = A.uoff[e] + i;
      const int nn = A.nlte_n[u];
      for (int l = 0; l <= nn && l < A.ion_nlev[u]; l++) {
        L.col_e.push_back(e);
        L.col_ion.push_back(i);
        L.col_l0.push_back(l);
        L.col_l1.push_back(l);
      }
      Dm += nn + 1;
      if (A.ion_nlev[u] > nn + 1) {
        L.col_e.push_back(e);
        L.col_ion.push_back(i);
        L.col_l0.push_back(nn + 1);
        L.col_l1.push_back(A.ion_nlev[u] - 1);
        Dm += 1;
      }
    }
    L.el_D[e] = Dm;
    L.cell1 += Dm;
    L.cell2 += (int64_t)Dm * Dm;
  }
  return (int)L.col_e.size() == L.cell1;
}

}  // namespace
