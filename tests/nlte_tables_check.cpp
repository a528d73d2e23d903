// Host check of artis_amd/csrc/engine/nlte_tables.h, included alone (that it compiles so is the check that the
// header is pure host code): the NLTE rate-matrix layout, the bf-heating level list, get_mean_binding_energy's
// shell occupations and refusals, and the Spencer-Fano grid, shell and transition tables, on hand-sized inputs.
// Built and run by tests/test_nlte_tables.py (a second time under the host address / undefined sanitizers).
#include "nlte_tables.h"

#include <cstdio>
#include <memory>

static long bad = 0, checked = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    checked++;                                                        \
    if (!(cond) && bad++ < 20) printf("line %d: %s\n", __LINE__, #cond); \
  } while (0)

template <typename T>
static bool same(const std::vector<T> &a, std::initializer_list<T> b) {
  return a == std::vector<T>(b);
}

static void check_matrix_layout() {
  // element 0: an ion with nlevels == nlevels_nlte + 1 (no superlevel), one with a superlevel over levels 3..5;
  // element 1: an ion with nlevels_nlte == 0 (ground level + superlevel 1..4), a single-level ion
  NlAtoms A;
  A.ne = 2;
  A.ni = 4;
  A.nions = {2, 2};
  A.uoff = {0, 2};
  A.ion_nlev = {4, 6, 5, 1};
  A.nlte_n = {3, 2, 0, 0};
  NlLayout L;
  CHECK(nl_matrix_layout(A, L));
  CHECK(same(L.el_D, {8, 3}));
  CHECK(same(L.el_off1, {0, 8}));
  CHECK(same<int64_t>(L.el_off2, {0, 64}));
  CHECK(L.cell1 == 11 && L.cell2 == 8 * 8 + 3 * 3);
  CHECK(same(L.col_e, {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1}));
  CHECK(same(L.col_ion, {0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1}));
  CHECK(same(L.col_l0, {0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 0}));
  CHECK(same(L.col_l1, {0, 1, 2, 3, 0, 1, 2, 5, 0, 4, 0}));
  A.ion_nlev[0] = 3;  // fewer levels than nlevels_nlte + 1
  CHECK(!nl_matrix_layout(A, L));
}

static void check_bfheat_levels() {
  // a one-ion element contributes nothing; of the three-ion element the top ion is skipped
  NlAtoms A;
  A.ne = 2;
  A.ni = 4;
  A.nions = {1, 3};
  A.uoff = {0, 1};
  A.ionis = {2, 2, 1, 3};
  A.ion_ul0 = {0, 10, 20, 30};
  CHECK(same(bfheat_levels(A), {10, 11, 20}));
  A.nions = {3, 1};  // element, ion, level order
  A.uoff = {0, 3};
  CHECK(same(bfheat_levels(A), {0, 1, 10, 11}));
}

// shell s of every element bound by 2^(27 - 3 s): with an ionisation potential below all of them the sum of
// q / binding is the occupation vector written in base 8 (q <= 6), exactly
static double occupations(std::initializer_list<int> q) {
  double total = 0.;
  int s = 0;
  for (int qs : q) total += qs / ldexp(1., 27 - 3 * s++);
  return total;
}

static void check_binding_energy() {
  std::unique_ptr<double[]> tab(new double[300]);  // exactly [30 * 10]: the sanitizer run sees any read outside
  for (int Z = 1; Z <= 30; Z++)
    for (int s = 0; s < 10; s++) tab[(Z - 1) * 10 + s] = ldexp(1., 27 - 3 * s);
  const double ionpot = 0.5;
  double b = -1.;
  CHECK(sf_mean_binding_energy(tab.get(), 26, 0, ionpot, &b) && b == occupations({2, 2, 2, 4, 2, 2, 4, 4, 2, 2}));
  CHECK(sf_mean_binding_energy(tab.get(), 26, 1, ionpot, &b) && b == occupations({2, 2, 2, 4, 2, 2, 4, 4, 2, 1}));
  CHECK(sf_mean_binding_energy(tab.get(), 26, 2, ionpot, &b) && b == occupations({2, 2, 2, 4, 2, 2, 4, 4, 2, 0}));
  CHECK(sf_mean_binding_energy(tab.get(), 30, 0, ionpot, &b) && b == occupations({2, 2, 2, 4, 2, 2, 4, 4, 6, 2}));
  CHECK(sf_mean_binding_energy(tab.get(), 1, 1, ionpot, &b) && b == 0.);  // no bound electron
  // a binding energy below the ionisation potential is replaced by it
  CHECK(sf_mean_binding_energy(tab.get(), 2, 0, 1e9, &b) && b == 2 / 1e9);
  CHECK(!sf_mean_binding_energy(tab.get(), 31, 3, ionpot, &b));  // the electrons fit, Z has no table row
  CHECK(!sf_mean_binding_energy(tab.get(), 31, 0, ionpot, &b));  // over-full: 13 electrons beyond the 18 inner ones
  CHECK(sf_mean_binding_energy(tab.get(), 20, 1, ionpot, &b) && b == occupations({2, 2, 2, 4, 2, 2, 4, 0, 0, 1}));
  // shell 8 without an entry takes shell 7's; any other shell without one is refused -- shell 0 of Z = 1 is the
  // table's first entry
  tab[25 * 10 + 8] = -1.;
  CHECK(sf_mean_binding_energy(tab.get(), 26, 0, ionpot, &b) &&
        b == occupations({2, 2, 2, 4, 2, 2, 4, 4, 0, 2}) + 2 / ldexp(1., 27 - 3 * 7));
  tab[0] = 0.;
  CHECK(!sf_mean_binding_energy(tab.get(), 1, 0, ionpot, &b));
  tab[25 * 10 + 3] = 0.;
  CHECK(!sf_mean_binding_energy(tab.get(), 26, 2, ionpot, &b));
  // every ion of a model: Fe I .. Fe III
  for (int s = 0; s < 10; s++) tab[25 * 10 + s] = ldexp(1., 27 - 3 * s);
  const int32_t anumber[1] = {26};
  const double ion_ionpot[3] = {ionpot, ionpot, ionpot};
  NlAtoms A;
  A.ne = 1;
  A.ni = 3;
  A.anumber = anumber;
  A.ion_ionpot = ion_ionpot;
  A.nions = {3};
  A.uoff = {0};
  A.ionstage = {1, 2, 3};
  std::vector<double> binding;
  std::vector<int32_t> ok;
  sf_ion_binding(A, tab.get(), binding, ok);
  CHECK(same(ok, {1, 1, 1}));
  CHECK(same(binding, {occupations({2, 2, 2, 4, 2, 2, 4, 4, 2, 2}), occupations({2, 2, 2, 4, 2, 2, 4, 4, 2, 1}),
                       occupations({2, 2, 2, 4, 2, 2, 4, 4, 2, 0})}));
  sf_ion_binding(A, nullptr, binding, ok);
  CHECK(same(ok, {0, 0, 0}) && same(binding, {0., 0., 0.}));
  CHECK(sf_get_J(2, 1, 50.) == 15.8 && sf_get_J(10, 1, 50.) == 24.2 && sf_get_J(18, 1, 50.) == 10.0);
  CHECK(sf_get_J(2, 2, 50.) == 0.6 * 50. && sf_get_J(26, 1, 50.) == 0.6 * 50.);
}

static void check_spencer_fano(int n) {
  const double emin = 1., emax = 3000.;
  // one Fe I shell (a second entry, of oxygen, matches no ion)
  const int32_t Z[2] = {8, 26}, nelec[2] = {8, 26};
  const double ionpot_ev[2] = {13.6, 500.5}, Ac[2] = {1., 1.}, zero[2] = {0., 0.};
  const double prob[6] = {1., 0., 0., 0.25, 0.5, 0.25};
  const float en_auger[2] = {0.f, 700.f};
  artis_nt_shells nt{};
  nt.nshells = 2;
  nt.sfpts = n;
  nt.sf_emin = emin;
  nt.sf_emax = emax;
  nt.Z = Z;
  nt.nelec = nelec;
  nt.ionpot_ev = ionpot_ev;
  nt.A = Ac;
  nt.B = nt.C = nt.D = zero;
  nt.prob_num_auger = prob;
  nt.en_auger_ev = en_auger;
  // one ion of four levels at 0, 0.5 (below emin), 10 and 20 eV; from the ground level: a collisional line, a
  // permitted one, one below emin, a forbidden one without a collision strength and one to level 250
  const int32_t anumber[1] = {26};
  NlAtoms A;
  A.ne = A.ni = 1;
  A.nl = 4;
  A.anumber = anumber;
  A.nions = {1};
  A.uoff = {0};
  A.ionstage = {1};
  A.ion_nlev = {4};
  A.ion_ul0 = {0};
  A.lev_eps = {0., 0.5 * ARTIS_EV, 10. * ARTIS_EV, 20. * ARTIS_EV};
  A.lev_g = {2.f, 4.f, 6.f, 8.f};
  A.lev_nup = {5, 0, 0, 0};
  A.lev_upoff = {0, 5, 5, 5};
  A.upidx = {0, 1, 2, 3, 4};
  A.line_upper = {2, 3, 1, 2, 250};
  A.line_coll = {1.5f, -1.f, 0.25f, -1.f, 1.f};
  A.line_f = {0.f, 0.5f, 0.f, 0.f, 0.f};
  A.line_forb = {0, 0, 0, 1, 0};
  const SfTables S = sf_build_tables(&nt, A);
  const double DE = (emax - emin) / (n - 1);
  CHECK(S.n == n && S.emin == emin && S.emax == emax && S.DE == DE);
  CHECK(S.source_spread_pts == (int)ceil(0.03333 * n) && S.source_spread_pts == (n == 2 ? 1 : 4));
  CHECK((int)S.envec.size() == n && S.envec[0] == emin && fabs(S.envec[n - 1] - emax) <= 1e-12 * emax);
  double src = 0.;
  int nsrc = 0;
  for (int k = 0; k < n; k++) {
    src += S.sourcevec[k] * DE;
    nsrc += S.sourcevec[k] != 0.;
    CHECK(S.logenvec[k] == log(S.envec[k]) && S.pw2[k] == pow(S.envec[k] * ARTIS_EV, -2));
  }
  CHECK(fabs(src - 1.) <= 1e-14 && nsrc == S.source_spread_pts && S.sourcevec[n - 1] != 0.);
  CHECK(S.E_init_ev <= emax * (1 + 1e-14) && S.E_init_ev >= emax - S.source_spread_pts * DE);
  CHECK(S.rhs[n - 1] == 0. && fabs(S.rhs[0] - 1.) <= 1e-14);
  for (int k = 1; k < n; k++) CHECK(S.rhs[k] <= S.rhs[k - 1]);
  auto gteq = [&](double en) { return std::max(0, std::min(n - 1, (int)ceil((en - emin) / DE))); };
  // the shell
  CHECK(same(S.sh_off, {0, 1}) && same(S.sh_k, {1}) && same(S.sh_ip, {500.5}) && same(S.sh_J, {0.6 * 500.5}));
  const int xsstart = gteq(500.5);
  CHECK(same(S.sh_start, {xsstart}) && xsstart == (n == 2 ? 1 : 17) && same(S.sh_astop, {gteq(700.)}));
  CHECK(same(S.sh_prob, {0.25, 0.5, 0.25}));
  CHECK((int)S.sh_xs.size() == n && (int)S.sh_ieu.size() == n && (int)S.sh_atn.size() == n && (int)S.sh_ie2.size() == n);
  for (int j = 0; j < n; j++) {
    if (j < xsstart)
      CHECK(S.sh_xs[j] == 0. && S.sh_ieu[j] == 0. && S.sh_atn[j] == 0.);
    else
      CHECK(S.sh_xs[j] > 0. && S.sh_atn[j] > 0.);
    CHECK(S.sh_ie2[j] == atan(S.envec[j] / (0.6 * 500.5)));
  }
  // the transitions
  CHECK(same(S.tr_off, {0, 3}) && same(S.tr_ul, {0, 0, 0}));
  CHECK(same(S.tr_kind, {0, 1, 0}) && same(S.tr_build, {1, 1, 0}));
  CHECK((int)S.tr_eps_ev.size() == 3 && fabs(S.tr_eps_ev[0] - 10.) <= 1e-13 && fabs(S.tr_eps_ev[1] - 20.) <= 1e-13 &&
        fabs(S.tr_eps_ev[2] - 0.5) <= 1e-14);
  CHECK(same(S.tr_eps, {10. * ARTIS_EV, 20. * ARTIS_EV, 0.5 * ARTIS_EV}));
  CHECK(same(S.tr_start, {gteq(S.tr_eps_ev[0]), gteq(S.tr_eps_ev[1]), 0}));
  CHECK(S.tr_cf[0] == pow(ARTIS_H_IONPOT, 2) / 2. * 1.5 * ARTIS_PI * 2.800285203e-17);
  CHECK(S.tr_cf[1] ==
        S.tr_eps_ev[1] * 45.585750051 * 2.800285203e-17 * pow(ARTIS_H_IONPOT / (20. * ARTIS_EV), 2) * 0.5);
  CHECK(same(S.tr_logeps, {0., log(S.tr_eps_ev[1]), 0.}));
  CHECK(S.band == (int)ceil(S.tr_eps_ev[1] / DE) + 2 && S.band == 3);
  // alone, the transition below emin is listed, not built, and leaves the band at its floor
  A.lev_nup[0] = 1;
  A.upidx = {2};
  const SfTables S1 = sf_build_tables(&nt, A);
  CHECK(same(S1.tr_build, {0}) && same(S1.tr_kind, {0}) && S1.band == 1);
}

int main() {
  check_matrix_layout();
  check_bfheat_levels();
  check_binding_energy();
  check_spencer_fano(2);
  check_spencer_fano(100);
  printf("checked %ld, bad %ld\n", checked, bad);
  return bad != 0;
}
