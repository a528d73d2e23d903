// Host check of artis_amd/csrc/engine/est_block.h, included alone (that it compiles so is the check that the header
// is pure host code): the section description of the estimator block against the layout artis_gpu.h documents,
// written out here by hand once more, and the walks over it -- pack, unpack, the download's add, the averaged
// scalars -- on small dimension sets.  Every array has exactly its documented length on the heap, so the sanitizer
// run shows a read or write past a section.  Built and run by tests/test_est_block.py (a second time under the host
// address / undefined sanitizers).
#include "est_block.h"

#include <cstdio>
#include <vector>

static long bad = 0, checked = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    checked++;                                                        \
    if (!(cond) && bad++ < 20) printf("line %d: %s\n", __LINE__, #cond); \
  } while (0)

struct Dims {
  int np, ne, mi, nl, nbf, nbins;
};

// an artis_estimators with its storage; field f (in the block's order, 0 .. 16) holds 1000 (f + 1) + j at index j,
// exact in every carrier type
struct Est {
  std::vector<double> J, nuJ, ff, col, rpkt, gamma, bfheat, bfrate, rfJ, rfnuJ;
  std::vector<int64_t> rfcount;
  std::vector<float> compton;
  std::vector<int32_t> ec, ac;
  artis_estimators e{};

  template <typename T>
  static void mark(std::vector<T> &v, size_t n, int f, bool marked) {
    v.resize(n);
    for (size_t j = 0; j < n; j++) v[j] = marked ? (T)(1000 * (f + 1) + (int)j) : (T)-1;
  }
  Est(const Dims &D, bool marked, bool arrays) {
    const size_t np = D.np, ni = np * D.ne * D.mi;
    mark(J, np, 0, marked);
    mark(nuJ, np, 1, marked);
    mark(ff, np, 2, marked);
    mark(col, np, 3, marked);
    mark(rpkt, np, 4, marked);
    mark(gamma, ni, 5, marked);
    mark(bfheat, ni, 6, marked);
    mark(bfrate, np * D.nbf, 8, marked);
    mark(rfJ, np * D.nbins, 9, marked);
    mark(rfnuJ, np * D.nbins, 10, marked);
    mark(rfcount, np * D.nbins, 11, marked);
    mark(compton, (np + 1) * ARTIS_EMISS_MAX, 12, marked);
    mark(ec, D.nl, 13, marked);
    mark(ac, D.nl, 14, marked);
    const double m = marked ? 1. : 0.;
    e.cmf_lum = m * 8000 - (1 - m);
    e.gamma_dep = m * 8001 - (1 - m);
    e.positron_dep = m * 8002 - (1 - m);
    e.electron_dep = m * 8003 - (1 - m);
    e.electron_emission = m * 8004 - (1 - m);
    e.alpha_dep = m * 8005 - (1 - m);
    e.alpha_emission = m * 8006 - (1 - m);
    e.gamma_emission = m * 8007 - (1 - m);
    e.nt_energy_deposited = m * 8008 - (1 - m);
    e.pellet_decays = marked ? 8009 : -1;
    for (int j = 0; j < ARTIS_COUNTER_COUNT; j++) e.counters[j] = marked ? 16000 + j : -1;
    e.nesc = marked ? 17000 : -1;
    if (!arrays) return;
    // vector::data() of an empty vector may be NULL: a zero-length section has nothing to carry either way
    e.J = J.data();
    e.nuJ = nuJ.data();
    e.ffheatingestimator = ff.data();
    e.colheatingestimator = col.data();
    e.rpkt_emiss = rpkt.data();
    e.gammaestimator = gamma.data();
    e.bfheatingestimator = bfheat.data();
    e.bfrate_raw = bfrate.data();
    e.radfield_J_raw = rfJ.data();
    e.radfield_nuJ_raw = rfnuJ.data();
    e.radfield_contribcount = rfcount.data();
    e.compton_emiss = compton.data();
    e.ecounter = ec.data();
    e.acounter = ac.data();
  }

  // the block artis_gpu.h documents, field by field
  std::vector<double> flat() const {
    std::vector<double> b;
    auto put = [&](const auto &v) {
      for (auto x : v) b.push_back((double)x);
    };
    put(J), put(nuJ), put(ff), put(col), put(rpkt), put(gamma), put(bfheat);
    put(std::vector<double>{e.cmf_lum, e.gamma_dep, e.positron_dep, e.electron_dep, e.electron_emission, e.alpha_dep,
                            e.alpha_emission, e.gamma_emission, e.nt_energy_deposited, (double)e.pellet_decays});
    put(bfrate), put(rfJ), put(rfnuJ), put(rfcount), put(compton), put(ec), put(ac);
    put(std::vector<int64_t>(e.counters, e.counters + ARTIS_COUNTER_COUNT));
    b.push_back((double)e.nesc);
    return b;
  }
};

static void check(const Dims &D) {
  const size_t np = D.np, ni = np * D.ne * D.mi, nbn = np * D.nbins;
  // the documented section lengths, in order
  const size_t want[ES_COUNT] = {np, np, np, np, np, ni, ni, 10, np * D.nbf, nbn, nbn, nbn, (np + 1) * ARTIS_EMISS_MAX,
                                 (size_t)D.nl, (size_t)D.nl, ARTIS_COUNTER_COUNT, 1};
  const EstBlock B = est_block(D.np, D.ne, D.mi, D.nl, D.nbf, D.nbins);
  size_t off = 0;
  for (int k = 0; k < ES_COUNT; k++) {
    CHECK(B.s[k].off == (int64_t)off && B.s[k].n == (int64_t)want[k]);
    off += want[k];
  }
  const size_t len = artis_estimator_block_len(D.np, D.ne, D.mi, D.nl, D.nbf, D.nbins);
  CHECK(len == off && (size_t)(B.s[ES_NESC].off + B.s[ES_NESC].n) == len && (size_t)B.len == len);
  CHECK((size_t)B.tail() == 2 * (size_t)D.nl + ARTIS_COUNTER_COUNT + 1 && B.n_device == B.s[ES_ECOUNTER].off);

  // EstLayout's named offsets are the sections', with the nebular sections switched by the run parameters
  artis_atomic_tables a{};
  artis_geometry g{};
  artis_run_params rp{};
  g.npts_model = D.np;
  a.nelements = D.ne;
  a.maxnions = D.mi;
  a.nlines = D.nl;
  a.nbfcontinua = D.nbf ? D.nbf : 7;  // ignored when the option is off
  a.radfield_nbins = D.nbins ? D.nbins : 7;
  rp.detailed_bf_estimators = D.nbf > 0;
  rp.multibin_radfield = D.nbins > 0;
  const EstLayout L = lay_out_estimators(&a, &g, &rp);
  const int64_t named[13] = {L.J,       L.nuJ,    L.ffheat, L.colheat, L.rpkt_emiss, L.gamma,  L.bfheat,
                             L.scalars, L.bfrate, L.rfJ,    L.rfnuJ,   L.rfcount,    L.compton};
  for (int k = 0; k <= ES_COMPTON; k++) CHECK(named[k] == B.s[k].off);
  CHECK(L.n_doubles == B.s[ES_COMPTON].off + B.s[ES_COMPTON].n && L.block.len == B.len);

  // pack: every field's marker in its section and nowhere else
  const Est x(D, true, true);
  const std::vector<double> want_b = x.flat();
  CHECK(want_b.size() == len);
  std::vector<double> b(len, -7.);
  CHECK(artis_estimator_block_pack(&x.e, D.np, D.ne, D.mi, D.nl, D.nbf, D.nbins, b.data()) == 0);
  CHECK(b == want_b);

  // unpack(pack(x)) == x, over whatever was there
  Est y(D, false, true);
  CHECK(artis_estimator_block_unpack(b.data(), D.np, D.ne, D.mi, D.nl, D.nbf, D.nbins, &y.e) == 0);
  CHECK(y.flat() == want_b);

  // the download's walk ADDS: twice x, the float array summed in double
  est_block_unpack(B, b.data(), &y.e, true);
  std::vector<double> twice = want_b;
  for (double &v : twice) v *= 2;
  CHECK(y.flat() == twice);

  // no arrays given: pack writes zeros for them, unpack skips them but still finds the sections behind them
  const Est z(D, true, false);
  std::vector<double> bz(len, -7.), want_z = want_b;
  for (int k = 0; k < ES_COUNT; k++)
    if (k != ES_SCALARS && k != ES_COUNTERS && k != ES_NESC)
      for (int64_t j = 0; j < B.s[k].n; j++) want_z[B.s[k].off + j] = 0.;
  CHECK(artis_estimator_block_pack(&z.e, D.np, D.ne, D.mi, D.nl, D.nbf, D.nbins, bz.data()) == 0);
  CHECK(bz == want_z);
  Est w(D, false, false);
  CHECK(artis_estimator_block_unpack(b.data(), D.np, D.ne, D.mi, D.nl, D.nbf, D.nbins, &w.e) == 0);
  CHECK(!w.e.J && !w.e.nuJ && !w.e.ffheatingestimator && !w.e.colheatingestimator && !w.e.rpkt_emiss &&
        !w.e.gammaestimator && !w.e.bfheatingestimator && !w.e.bfrate_raw && !w.e.radfield_J_raw &&
        !w.e.radfield_nuJ_raw && !w.e.radfield_contribcount && !w.e.compton_emiss && !w.e.ecounter && !w.e.acounter);
  CHECK(w.J == Est(D, false, false).J && w.compton == Est(D, false, false).compton);  // the storage was not reached
  CHECK(w.e.cmf_lum == 8000 && w.e.nt_energy_deposited == 8008 && w.e.pellet_decays == 8009 && w.e.nesc == 17000);
  for (int j = 0; j < ARTIS_COUNTER_COUNT; j++) CHECK(w.e.counters[j] == 16000 + j);

  // average_scalars: exactly the first 8 doubles of the scalar group
  std::vector<double> av = b;
  CHECK(artis_estimator_block_average_scalars(av.data(), D.np, D.ne, D.mi, 4) == 0);
  for (size_t j = 0; j < len; j++) {
    const bool averaged = j >= 5 * np + 2 * ni && j < 5 * np + 2 * ni + 8;
    CHECK(av[j] == (averaged ? b[j] / 4 : b[j]));
  }
}

int main() {
  check({3, 2, 4, 5, 0, 0});
  check({2, 1, 3, 4, 5, 6});
  check({2, 2, 2, 0, 3, 2});  // no lines
  check({2, 1, 2, 3, 4, 0});  // detailed bf estimators only
  check({1, 2, 1, 2, 0, 3});  // radiation field bins only
  // refusals
  double one = 0.;
  artis_estimators e{};
  CHECK(artis_estimator_block_len(-1, 1, 1, 1, 0, 0) == 0);
  CHECK(artis_estimator_block_pack(nullptr, 1, 1, 1, 1, 0, 0, &one) == ARTIS_ERR_BAD_ARGUMENT);
  CHECK(artis_estimator_block_unpack(&one, 1, 1, 1, -1, 0, 0, &e) == ARTIS_ERR_BAD_ARGUMENT);
  CHECK(artis_estimator_block_average_scalars(&one, 1, 1, 1, 0) == ARTIS_ERR_BAD_ARGUMENT);
  printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
