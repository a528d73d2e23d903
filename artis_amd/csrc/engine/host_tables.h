// host_tables.h -- the tables artis_gpu_init derives from the caller's atomic data and geometry before it uploads
// them.  Pure host functions: no HIP call, no engine state.  Their expressions are the reference's, operand for
// operand (host libm): the parity tests compare bit-level results that depend on them.  Included once by
// engine.hip, after its kernels (ma_build_doubles and MA_BUILD_MAX_DOUBLES come from there) and engine_state.h;
// nlte_tables.h holds the tables of update_grid's host drivers (update_grid_host.h), est_block.h the layout of the
// estimator block.
#pragma once

namespace {

inline int64_t sum_i32(const int32_t *a, int n) {
  int64_t s = 0;
  for (int i = 0; i < n; i++) s += a[i];
  return s;
}

// ------------------------------------------------------------------------ per-line and per-transition items
struct LineTables {
  std::vector<LineTau> tau;      // per-line Sobolev coefficients
  std::vector<LineMA> ma;        // macro-atom per-line constants
  std::vector<TeExcItem> exc;    // packed collisional-excitation terms, indexed like uptrans_lineindex
  std::vector<MaDownItem> down;  // k_marates' packed transition items, indexed like downtrans_lineindex
  std::vector<MaUpItem> up;      // ... like uptrans_lineindex
};

inline LineTables derive_line_tables(const artis_atomic_tables *a) {
  const int nl = a->nlevels_total, nli = a->nlines;
  LineTables t;
  // per-line Sobolev coefficients, evaluated on the host with the same expression as rpkt.cc:179-181
  std::vector<LineTau> &lt = t.tau;
  lt.resize(nli);
  for (int li = 0; li < nli; li++) {
    const int e = a->line_elementindex[li], i = a->line_ionindex[li];
    const int off = a->ion_uniqueleveloffset[a->elem_uniqueionoffset[e] + i];
    const int ulo = off + a->line_lowerlevelindex[li], uup = off + a->line_upperlevelindex[li];
    const double nu_trans = a->line_nu[li];
    const double A_ul = a->line_einstein_A[li];
    const double B_ul = ARTIS_CLIGHTSQUAREDOVERTWOH / pow(nu_trans, 3) * A_ul;
    const double B_lu = (double)a->level_stat_weight[uup] / (double)a->level_stat_weight[ulo] * B_ul;
    lt[li] = {nu_trans, B_ul, B_lu, ulo, uup};
  }
  // macro-atom per-line constants (macroatom.cc:518-522, 563-566; radfield.h:47; macroatom.h:93,130)
  std::vector<LineMA> &lm = t.ma;
  lm.resize(nli);
  for (int li = 0; li < nli; li++) {
    const int ulo = lt[li].ul_lower, uup = lt[li].ul_upper;
    const double epsilon_trans = a->level_epsilon[uup] - a->level_epsilon[ulo];
    const double nu_trans = epsilon_trans / ARTIS_H;
    const double A_ul = a->line_einstein_A[li];
    const double B_ul = ARTIS_CLIGHTSQUAREDOVERTWOH / pow(nu_trans, 3) * A_ul;
    const double B_lu = (double)a->level_stat_weight[uup] / (double)a->level_stat_weight[ulo] * B_ul;
    lm[li] = {B_ul, B_lu, pow(nu_trans, 3), pow(ARTIS_H_IONPOT / epsilon_trans, 2)};
  }
  size_t nd_items = 1, nu_items = 1;
  for (int ul = 0; ul < nl; ul++) {
    nd_items = std::max(nd_items, (size_t)a->level_downtrans_offset[ul] + (size_t)a->level_ndowntrans[ul]);
    nu_items = std::max(nu_items, (size_t)a->level_uptrans_offset[ul] + (size_t)a->level_nuptrans[ul]);
  }
  t.exc.resize(nu_items);
  t.down.resize(nd_items);
  t.up.resize(nu_items);
  for (int ui = 0; ui < a->nions_total; ui++) {
    const int ul0 = a->ion_uniqueleveloffset[ui];
    for (int l = 0; l < a->ion_nlevels[ui]; l++) {
      const int ul = ul0 + l;
      for (int j = 0; j < a->level_ndowntrans[ul]; j++) {
        const int li = a->downtrans_lineindex[a->level_downtrans_offset[ul] + j];
        const int lo = a->line_lowerlevelindex[li];
        MaDownItem &x = t.down[a->level_downtrans_offset[ul] + j];
        x = MaDownItem{};
        x.lower = lo;
        x.forbidden = a->line_forbidden[li];
        x.A = a->line_einstein_A[li];
        x.coll = a->line_coll_str[li];
        x.osc_f = a->line_osc_strength[li];
        x.lower_sw = a->level_stat_weight[ul0 + lo];
        x.eps_target = a->level_epsilon[ul0 + lo];
        x.B_ul = lm[li].B_ul;
        x.B_lu = lm[li].B_lu;
        x.P2 = lm[li].P2;
      }
      for (int j = 0; j < a->level_nuptrans[ul]; j++) {
        const int li = a->uptrans_lineindex[a->level_uptrans_offset[ul] + j];
        const int up = a->line_upperlevelindex[li];
        TeExcItem &c = t.exc[a->level_uptrans_offset[ul] + j];
        c.epsilon_trans = a->level_epsilon[ul0 + up] - a->level_epsilon[ul];
        c.P2 = lm[li].P2;
        c.coll_str = a->line_coll_str[li];
        c.osc_f = a->line_osc_strength[li];
        c.upper_sw = a->level_stat_weight[ul0 + up];
        c.forbidden = a->line_forbidden[li];
        MaUpItem &x = t.up[a->level_uptrans_offset[ul] + j];
        x = MaUpItem{};
        x.upper = up;
        x.forbidden = a->line_forbidden[li];
        x.coll = a->line_coll_str[li];
        x.osc_f = a->line_osc_strength[li];
        x.upper_sw = a->level_stat_weight[ul0 + up];
        x.eps_upper = a->level_epsilon[ul0 + up];
        x.B_ul = lm[li].B_ul;
        x.B_lu = lm[li].B_lu;
        x.nu3 = lm[li].nu3;
        x.P2 = lm[li].P2;
      }
    }
  }
  return t;
}

// ----------------------------------------------------------------------------- macro-atom record metadata
struct MaTables {
  std::vector<MaMeta> meta;
  std::vector<MaWalk> walk;
  std::vector<int64_t> dbl_off;  // exact-sum scratch of k_marates (doubles, unpadded), nl + 1 prefix sums
  std::vector<int2> down_target, up_target;
  int64_t key_stride = 0;  // 16-bit keys of one cell's records
  bool cache_ok = true;    // every level's same-ion arrays fit the two-level record layout
};

// macro-atom records per level (engine_dev.h DevCells::ma_rec): recombination targets are the ionising levels
// of the lower ion for levels l <= maxrecombininglevel of ions i > 0 (macroatom.cc:104-124); up-higher targets
// are the phixs targets of ionising levels of non-top ions (get_nphixstargets)
inline MaTables derive_ma_tables(const artis_atomic_tables *a) {
  const int ne = a->nelements, nl = a->nlevels_total;
  const int64_t nup = sum_i32(a->level_nuptrans, nl), ndown = sum_i32(a->level_ndowntrans, nl);
  MaTables t;
  std::vector<MaMeta> &mm = t.meta;
  mm.resize(nl);
  t.dbl_off.assign(nl + 1, 0);
  int64_t marec = 0;
  for (int e = 0; e < ne; e++)
    for (int i = 0; i < a->elem_nions[e]; i++) {
      const int ui = a->elem_uniqueionoffset[e] + i;
      for (int l = 0; l < a->ion_nlevels[ui]; l++) {
        const int ul = a->ion_uniqueleveloffset[ui] + l;
        MaMeta &m = mm[ul];
        m.nr = (i > 0 && l <= a->ion_maxrecombininglevel[ui]) ? a->ion_ionisinglevels[ui - 1] : 0;
        m.nt = (i < a->elem_nions[e] - 1 && l < a->ion_ionisinglevels[ui]) ? a->level_nphixstargets[ul] : 0;
        m.nd = a->level_ndowntrans[ul];
        m.nu = a->level_nuptrans[ul];
        m.doff = a->level_downtrans_offset[ul];
        m.uoff = a->level_uptrans_offset[ul];
        m.base_lower = (i > 0) ? a->ion_uniqueleveloffset[ui - 1] : -1;
        m.rec_off = (int32_t)marec;
        const int64_t len = ARTIS_MA_ACTION_COUNT + 2 * (int64_t)m.nd + m.nu + 2 * (int64_t)m.nr + m.nt;
        // high then low key halves (engine_dev.h ma_layout), records 128-byte aligned
        marec += (2 * (int64_t)ma_layout(m.nd, m.nu, m.nr, m.nt).hot + 63) / 64 * 64;
        t.dbl_off[ul + 1] = len;
        if (!ma_layout_ok(m.nd, m.nu)) t.cache_ok = false;
      }
    }
  t.walk.resize(nl);
  for (int ul = 0; ul < nl; ul++)
    if (!ma_walk_make(mm[ul], &t.walk[ul])) t.cache_ok = false;
  for (int ul = 0; ul < nl; ul++) t.dbl_off[ul + 1] += t.dbl_off[ul];
  // internal same-ion jump targets in the (reference) order of their cumulative arrays
  std::vector<int2> &dt = t.down_target, &ut = t.up_target;
  dt.resize(std::max<int64_t>(ndown, 1));
  ut.resize(std::max<int64_t>(nup, 1));
  for (int e = 0; e < ne; e++)
    for (int i = 0; i < a->elem_nions[e]; i++) {
      const int ui = a->elem_uniqueionoffset[e] + i;
      const int base = a->ion_uniqueleveloffset[ui];
      for (int l = 0; l < a->ion_nlevels[ui]; l++) {
        const int ul = base + l;
        const MaMeta &m = mm[ul];
        for (int j = 0; j < m.nd; j++) {
          const int tl = base + a->line_lowerlevelindex[a->downtrans_lineindex[m.doff + j]];
          dt[m.doff + j] = make_int2(tl, mm[tl].rec_off);
        }
        for (int j = 0; j < m.nu; j++) {
          const int tl = base + a->line_upperlevelindex[a->uptrans_lineindex[m.uoff + j]];
          ut[m.uoff + j] = make_int2(tl, mm[tl].rec_off);
        }
      }
    }
  t.key_stride = marec;
  return t;
}

// level mode: per level, its record size in 128-byte lines (0: never a record -- a layout that does not fit, or
// more rate terms than k_ma_build stages in LDS) and their exclusive prefix sums; the most LDS doubles a record's
// build needs
struct MaLevelTables {
  std::vector<uint32_t> rec_lines, rl_off;
  uint32_t row_lines = 0;  // pool lines of one whole cell's records
  int64_t build_lds_doubles = 0;
};

inline MaLevelTables derive_ma_level_tables(const MaTables &ma, bool hi_only) {
  const std::vector<MaMeta> &mm = ma.meta;
  const int nl = (int)mm.size();
  MaLevelTables t;
  t.rec_lines.assign(nl, 0);
  for (int ul = 0; ul < nl; ul++) {
    const int64_t next = (ul + 1 < nl) ? mm[ul + 1].rec_off : ma.key_stride;
    const int64_t need = ma_build_doubles(mm[ul]);
    if (ma_layout_ok(mm[ul].nd, mm[ul].nu) && need <= MA_BUILD_MAX_DOUBLES) {
      const int64_t hot = ma_layout(mm[ul].nd, mm[ul].nu, mm[ul].nr, mm[ul].nt).hot;
      t.rec_lines[ul] = (uint32_t)(hi_only ? (hot + 63) / 64 : (next - mm[ul].rec_off) / 64);
      t.build_lds_doubles = std::max<int64_t>(t.build_lds_doubles, need);
    }
  }
  t.rl_off.assign(nl, 0);
  uint64_t acc = 0;
  for (int ul = 0; ul < nl; ul++) {
    t.rl_off[ul] = (uint32_t)acc;
    acc += t.rec_lines[ul];
  }
  t.row_lines = (uint32_t)acc;
  return t;
}

// -------------------------------------------------------------------------------------- continuum tables
struct ContTables {
  std::vector<BfCont> bfc;
  std::vector<double2> bf_edge2;              // (nu_edge, nu_max), padded with at least one (inf, inf)
  std::vector<int32_t> gc_cont_off, gc_cont;  // per ground continuum, the ground-level continua that enter it
  std::vector<int32_t> slot_allcont;          // photoionisation target slot -> allcont entry (-1: none)
  std::vector<int32_t> target_ul, target_t;   // photoionisation target slot -> (unique level, target index)
  std::vector<int32_t> bfcol;                 // bflist index -> element * maxnions + ion
};

inline ContTables derive_cont_tables(const artis_atomic_tables *a) {
  const int ne = a->nelements, nl = a->nlevels_total, nb = a->nbfcontinua;
  const int64_t ntg = sum_i32(a->level_nphixstargets, nl);
  ContTables t;
  std::vector<BfCont> &bc = t.bfc;
  bc.resize(std::max(1, nb));
  for (int i = 0; i < nb; i++) {
    bc[i].nu_edge = a->allcont_nu_edge[i];
    bc[i].nu_max = a->allcont_nu_edge[i] * a->last_phixs_nuovernuedge;  // (bf_contribution's expression)
    bc[i].probability = a->allcont_probability[i];
    bc[i].xs_off = a->allcont_phixstable[i] * a->nphixspoints;
    bc[i].pad = 0;
  }
  const int ne2 = (nb / 4 + 1) * 4;  // at least one padding entry
  t.bf_edge2.assign(ne2, make_double2(INFINITY, INFINITY));
  for (int i = 0; i < nb; i++) t.bf_edge2[i] = make_double2(bc[i].nu_edge, bc[i].nu_max);
  {
    // per ground continuum, the allcont indices (ascending) of the ground-level continua that enter its
    // groundcont_gamma_contr (rpkt.cc:1166-1171): update_estimators sums these instead of scanning all continua
    const int nbfg = a->nbfcontinua_ground;
    std::vector<int32_t> &off = t.gc_cont_off, &lst = t.gc_cont;
    off.assign(nbfg + 1, 0);
    for (int g = 0; g < nbfg; g++) {
      off[g] = (int32_t)lst.size();
      for (int i = 0; i < nb; i++)
        if (a->allcont_level[i] == 0 && a->allcont_index_in_groundphixslist[i] == g) lst.push_back(i);
    }
    off[nbfg] = (int32_t)lst.size();
    if (lst.empty()) lst.push_back(0);
  }
  t.target_ul.resize(ntg + 1);
  t.target_t.resize(ntg + 1);
  for (int ul = 0; ul < nl; ul++)
    for (int tg = 0; tg < a->level_nphixstargets[ul]; tg++) {
      t.target_ul[a->level_phixstargets_offset[ul] + tg] = ul;
      t.target_t[a->level_phixstargets_offset[ul] + tg] = tg;
    }
  // get_bfcontindex (radfield.cc:1329-1341): the allcont entry of each photoionisation target slot
  t.slot_allcont.assign(ntg + 1, -1);
  for (int ib = 0; ib < nb; ib++) {
    const int ul = a->ion_uniqueleveloffset[a->elem_uniqueionoffset[a->allcont_element[ib]] + a->allcont_ion[ib]] +
                   a->allcont_level[ib];
    t.slot_allcont[a->level_phixstargets_offset[ul] + a->allcont_phixstargetindex[ib]] = ib;
  }
  // bflist (input.cc:1153-1160: cont_index counts down from -1 over every level's targets) -> ion column
  t.bfcol.assign(std::max(nb, 1), 0);
  for (int e = 0; e < ne; e++)
    for (int i = 0; i < a->elem_nions[e]; i++) {
      const int ui = a->elem_uniqueionoffset[e] + i;
      for (int l = 0; l < a->ion_nlevels[ui]; l++) {
        const int ul = a->ion_uniqueleveloffset[ui] + l;
        for (int tg = 0; tg < a->level_nphixstargets[ul]; tg++) {
          const int bi = -1 - (a->level_cont_index[ul] - tg);
          if (bi >= 0 && bi < nb) t.bfcol[bi] = e * a->maxnions + i;
        }
      }
    }
  return t;
}

// Non-empty model cells: those referenced by a propagation cell, numbered from the centre outwards (the
// distance of the cell's nearest propagation-cell centre at tmin, ties by mgi) -- the per-cell tables that only
// fit the HBM budget for some cells (line coefficients, macro-atom keys) hold the first rows, the cells where
// the packets start and the density peaks; every other cell takes the equivalent table-free path
struct CellNumbering {
  std::vector<int32_t> ne_index;  // model cell -> number (-1: empty)
  std::vector<int32_t> ne_mgi;    // number -> model cell
};

inline CellNumbering number_cells(const artis_geometry *g) {
  const int np = g->npts_model;
  CellNumbering t;
  std::vector<int32_t> &ne_index = t.ne_index, &ne_mgi = t.ne_mgi;
  ne_index.assign(np, -1);
  std::vector<double> rmin(np, DBL_MAX);
  for (int c = 0; c < g->ngrid; c++) {
    const int mgi = g->cell_mgi[c];
    if (mgi >= 0 && mgi < np) {
      double r2 = 0.;
      if (g->grid_type == ARTIS_GRID_SPHERICAL1D) {
        const double r = g->cell_pos_min[3 * (int64_t)c] + 0.5 * g->modelcell_wid_init[c];  // get_cellradialpos
        r2 = r * r;
      } else {
        for (int d = 0; d < 3; d++) {
          const double x = g->cell_pos_min[3 * (int64_t)c + d] + g->coordmax[d] / std::max(1, g->ncoordgrid[d]);
          r2 += x * x;
        }
      }
      rmin[mgi] = std::min(rmin[mgi], r2);
      ne_index[mgi] = 0;
    }
  }
  for (int mgi = 0; mgi < np; mgi++)
    if (ne_index[mgi] == 0) ne_mgi.push_back(mgi);
  std::stable_sort(ne_mgi.begin(), ne_mgi.end(), [&](int a, int b) { return rmin[a] < rmin[b]; });
  for (size_t k = 0; k < ne_mgi.size(); k++) ne_index[ne_mgi[k]] = (int32_t)k;
  return t;
}

// Few-cell models: k_rpkt accumulates the estimators of every non-empty cell per block in LDS, as many of the
// sections as fit EST_LDS_DOUBLES (allow false: none).  Offsets in doubles, -1: the section stays in HBM.
struct EstLdsLayout {
  int32_t J, bf, rf;
};

inline EstLdsLayout lay_out_est_lds(bool allow, int nne_cells, bool detailed_bf, int nbf, bool multibin, int rf_nbins) {
  int64_t off = 0;
  auto take = [&](bool want, int64_t n) -> int32_t {
    if (!allow || !want || n <= 0 || off + n > EST_LDS_DOUBLES) return -1;
    const int32_t o = (int32_t)off;
    off += n;
    return o;
  };
  EstLdsLayout L;
  L.J = take(true, 3 * (int64_t)nne_cells);
  L.bf = take(detailed_bf, (int64_t)nne_cells * nbf);
  L.rf = take(multibin, 3 * (int64_t)nne_cells * rf_nbins);
  return L;
}

}  // namespace
