// engine_state.h -- the host state of the engine: environment knobs, the owners of device memory, the Engine
// singleton, HIPCHK and the call-scoped DevBufs / CallerArrays.  Host code only; included once by engine.hip, after
// its kernels (Ctx, WaveState, QagWs and the MA_BUILD_SMALL / VPKT_OCC_DEFAULT constants come from there) and
// est_block.h (EstLayout), and before host_tables.h, nlte_tables.h and the host drivers update_grid_host.h,
// estimators_host.h and spectra_host.h.
#pragma once

namespace {

// ============================================================================================ environment knobs
// Read once per engine by read_knobs() (artis_gpu_init): a variable set before an engine is created holds for that
// engine's life.  Read elsewhere, at use: ARTIS_GPU_FAIL_ALLOC_ABOVE (every allocation; tests flip it during an
// engine's life), ARTIS_GPU_STATS and the NLTE debug pair ARTIS_GPU_NL_DEBUG / ARTIS_GPU_NL_DUMP.
//
// Names are ARTIS_GPU_<NAME> unless spelled out.  "'c'" tests the value's first character only.
//   name                | default        | parsing, clamp          | the default's measurement / purpose
//   WAVE_GRID=<blocks>  | 8 per CU       | max(8, atoi / 8 * 8)    | 32 waves per CU of 256-thread blocks, late blocks find
//                       |                |                         |   the queue drained; tests shrink the persistent grids
//   ENGINE=mega         | split kernels  | the string "mega"       | DESIGN.md section 5
//   MA_BIN=0            | on             | '0' off                 | M queue binned by cell: 5-15 % faster walks (lanes of a
//                       |                |                         |   wave share a cell's records)
//   MA_XCD=1            | 1 queue range  | '1': 8 ranges           | per-XCD ranges measured neutral-to-negative
//   R_BIN=1             | off            | '1' on                  | no faster k_rpkt (1114 vs 1106 ms per bench step), ~250 ms
//                       |                |                         |   more binning per step (profiles/r03g_ab.txt)
//   RPKT_WALK=1|0       | per transport  | unset -1, '1' 1, else 0 | bounded line walk when the last transport's steps
//                       |                |                         |   scanned > 8 lines each
//   RPKT_COOP=0         | on             | '0' off                 | detailed-bf models: wave-made continuum sums in k_rpkt
//   RPKT_OCC=1|2|3      | 2              | '1' or '3', else 2      | k_rpkt needs ~300 registers; at 1 wave/SIMD nothing hides
//                       |                |                         |   its FP64 latency, forcing 2 (spilling to scratch)
//                       |                |                         |   measured 1.80 s -> 1.53 s per bench step on MI355X
//   MA_PRE=0 MF_REC=0 BIN_PUSH=0 MA_BIN_BLK=0 | on | '0' off       | fallback paths (tests/test_gpu_parity.py FALLBACKS)
//   REFILL=<lanes>      | 32             | atoi clamped to 1..64   | idle lanes at which k_rpkt / k_vpkt refill
//   REFILL_MA=<lanes>   | 12             | atoi clamped to 1..64   | k_ma refills from one coalesced ticket read, so early
//                       |                |                         |   (1e7-packet bench, before tickets: 32 idle lanes 2212 ms,
//                       |                |                         |   16: 2064, 8: 2042; round 5, with the line-0 suffix and the
//                       |                |                         |   F-queue records: 4: 2578 ms, 8: 1694, 12: 1559, 14: 1568,
//                       |                |                         |   16: 1581, 20: 1617, 24: 1659; profiles/r5s_refill_sweep.txt;
//                       |                |                         |   with MA_PARK=32: 8: 1379 ms, 12: 1230, 16: 1249,
//                       |                |                         |   profiles/r7_ma_park_ab.txt)
//   MA_PARK=<lanes>     | 32             | atoi clamped to 0..64   | k_ma parks the walks of a wave whose queue is used up and
//                       |                |                         |   that has fewer busy lanes, for the next round (0: off;
//                       |                |                         |   only in launches of >= 4 walks per lane, row mode with
//                       |                |                         |   tickets).  1e7-packet bench, k_ma per step: parent 1441 ms,
//                       |                |                         |   0: 1500, 8: 1285, 16: 1254, 24: 1237, 32: 1230, 40: 1227,
//                       |                |                         |   48: 1240, 64: 1243; the step 2636 -> 2412 ms at 32
//                       |                |                         |   (profiles/r7_ma_park_ab.txt)
//   FIN_GATHER=0        | on             | '0' off                 | k_ma_finish gathers a wave's R / K appends in LDS and adds
//                       |                |                         |   to the queue counter once per ~960 entries, not once per
//                       |                |                         |   pass: adds to one word take 11.35 ns each device-wide
//                       |                |                         |   (tools/atomrate.hip); k_ma_finish per 1e7 bench step
//                       |                |                         |   199 -> 161 ms, the step 2412 -> 2369 (profiles/r8_pkt_coop_ab.txt)
//   MA_OCC=8            | 1              | '8': 8, else 1          | k_ma minimum waves per SIMD (launch bounds)
//   MA_WAVES=<w>        | 4              | atoi in 1..8, else 4    | k_ma blocks per CU: fewer concurrent walks thrash the
//                       |                |                         |   caches less, the walk is bound by the memory system (1e7
//                       |                |                         |   packets: 2 waves 4694 ms, 3: 3761, 4: 3317, 8: 3725;
//                       |                |                         |   profiles/r02_ab_ma_waves.txt)
//   MA_COOP_MAX=<lanes> | 64             | atoi clamped to 1..64   | WaveState::coop_max
//   MA_LEVEL_COOP=1     | off            | '1' on                  | level mode: k_ma makes the jumps without a record itself;
//                       |                |                         |   off parks them for k_ma_exact and keeps k_ma's registers
//   MA_BUILD_SMALL=<d>  | MA_BUILD_SMALL | max(0, atoll)           | tests run both k_ma_build launches on small atoms
//   NO_EST_LDS=1        | LDS sections   | '1': none               | few-cell models' per-block estimator accumulator
//   MAREC_SCRATCH_MB=<m>| 2 GiB          | atof * 2^20 / 8 doubles | k_marates scratch of row mode
//   MACACHE_MAX_GB=<g>  | half the free HBM | atof * 2^30          | the rest is left for the packet store
//   MACACHE_ROWS=<r>    | unset          | atoll; caps the budget  | tests: level mode with a pool of r rows' records
//   NO_MACACHE=1        | off            | '1' on                  | empty record pool (every jump from the exact sums)
//   LINECOEF_MAX_GB=<g> | 30 % of the free HBM | atof * 2^30       | the packet store comes later
//   LINECOEF_ROWS=<r>   | unset          | min(rows, atoi)         | tests
//   NO_LINECOEF=1       | off            | '1' on                  | every cell gathers its populations per line
//   LINECOEF_GATHER=1   | k_linecoef_lds | atoi != 0               | A/B and test switch: the gather kernel k_linecoef
//   TE_LANES=<g>        | one per ion    | atoi in 1..64, else dflt| k_te_solve lanes per cell
//   SF_BATCH_GB=<g>     | 8              | max(0, atof)            | Spencer-Fano matrices (8 n^2 bytes each) solved together
//   ARTIS_VPKT_OCC=1|2|3| VPKT_OCC_DEFAULT | atoi; 2 or 3, else 1  | more waves hide more of the walk's FP64 and memory
//                       |                |                         |   latency at the price of register spills
//   ARTIS_VPKT_LCONLY=0 | on             | '0' off                 | off forces the general k_vpkt (gather walk) everywhere
//   ARTIS_VPKT_SORT=0   | on             | '0' off                 | off traces in buffer order
// No test sets one of these between creating an engine and the call that uses it.
struct Knobs {
  int wave_grid = 0;  // 0: 8 blocks per CU
  bool use_megakernel = false;
  bool ma_binned = true;
  int ma_ranges = 1;
  bool r_binned = false;    // bin the R queue by cell before k_rpkt
  int rpkt_walk = -1;       // k_rpkt's bounded line walk: -1 by the previous transport's lines per step, 0 off, 1 on
  bool rpkt_coop = true;    // detailed-bf models: wave-made continuum sums in k_rpkt (else per lane)
  int rpkt_occ = 2;         // waves per SIMD k_rpkt is compiled for
  bool ma_pre_on = true;    // M-queue pre-tickets (WaveState::ma_pre; off: gathered by the scatter)
  bool mf_rec_on = true;    // F-queue records (WaveState::mf_rec; off: the per-packet pend arrays)
  bool bin_push_on = true;  // M queue binned by its producers (WaveState::bin_push; off: k_ma_bin)
  bool ma_bin_blk = true;   // few cells: block-local M-queue binning (off: per-entry atomics)
  int refill_min = 32, refill_ma = 12;
  int ma_park = MA_PARK_DEFAULT;  // WaveState::ma_park
  bool fin_gather = true;   // WaveState::fin_gather
  int ma_occ = 1;    // k_ma minimum waves per SIMD (launch bounds): 1 or 8
  int ma_waves = 4;  // k_ma blocks per CU
  int coop_max = 64;
  bool ma_level_coop = false;  // level mode: k_ma makes the jumps without a record itself (else k_ma_exact)
  int64_t ma_build_small = MA_BUILD_SMALL;  // the small-level threshold of the build list (doubles)
  bool no_est_lds = false;
  int64_t marec_scratch_doubles = ((int64_t)2 << 30) / 8;
  bool have_macache_max = false, have_macache_rows = false, no_macache = false;
  double macache_max_bytes = 0.;
  int64_t macache_rows = 0;
  bool have_linecoef_max = false, have_linecoef_rows = false, no_linecoef = false;
  double linecoef_max_bytes = 0.;
  int linecoef_rows = 0;
  bool linecoef_gather = false;
  int te_lanes = 0;  // 0: te_lanes_per_cell
  double sf_batch_gb = 8.;
  int vpkt_occ = 1;
  bool vpkt_lconly = true;
  bool vpkt_sort = true;
};

inline Knobs read_knobs() {
  auto first_is = [](const char *name, char c) {
    const char *e = getenv(name);
    return e && e[0] == c;
  };
  auto lanes = [](const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? std::max(1, std::min(64, atoi(e))) : dflt;
  };
  Knobs k;
  if (const char *wg = getenv("ARTIS_GPU_WAVE_GRID")) k.wave_grid = std::max(8, atoi(wg) / 8 * 8);
  const char *eng = getenv("ARTIS_GPU_ENGINE");
  k.use_megakernel = eng && std::string(eng) == "mega";
  k.ma_binned = !first_is("ARTIS_GPU_MA_BIN", '0');
  k.ma_ranges = first_is("ARTIS_GPU_MA_XCD", '1') ? 8 : 1;
  k.r_binned = first_is("ARTIS_GPU_R_BIN", '1');
  k.rpkt_walk = getenv("ARTIS_GPU_RPKT_WALK") ? (first_is("ARTIS_GPU_RPKT_WALK", '1') ? 1 : 0) : -1;
  k.rpkt_coop = !first_is("ARTIS_GPU_RPKT_COOP", '0');
  k.rpkt_occ = first_is("ARTIS_GPU_RPKT_OCC", '1') ? 1 : first_is("ARTIS_GPU_RPKT_OCC", '3') ? 3 : 2;
  k.ma_pre_on = !first_is("ARTIS_GPU_MA_PRE", '0');
  k.mf_rec_on = !first_is("ARTIS_GPU_MF_REC", '0');
  k.bin_push_on = !first_is("ARTIS_GPU_BIN_PUSH", '0');
  k.ma_bin_blk = !first_is("ARTIS_GPU_MA_BIN_BLK", '0');
  k.refill_min = lanes("ARTIS_GPU_REFILL", 32);
  k.refill_ma = lanes("ARTIS_GPU_REFILL_MA", 12);
  if (const char *e = getenv("ARTIS_GPU_MA_PARK")) k.ma_park = std::max(0, std::min(64, atoi(e)));
  k.fin_gather = !first_is("ARTIS_GPU_FIN_GATHER", '0');
  k.ma_occ = first_is("ARTIS_GPU_MA_OCC", '8') ? 8 : 1;
  if (const char *e = getenv("ARTIS_GPU_MA_WAVES")) {
    const int v = atoi(e);
    k.ma_waves = (v >= 1 && v <= 8) ? v : 4;
  }
  k.coop_max = lanes("ARTIS_GPU_MA_COOP_MAX", 64);
  k.ma_level_coop = first_is("ARTIS_GPU_MA_LEVEL_COOP", '1');
  if (const char *e = getenv("ARTIS_GPU_MA_BUILD_SMALL")) k.ma_build_small = std::max<int64_t>(0, atoll(e));
  k.no_est_lds = first_is("ARTIS_GPU_NO_EST_LDS", '1');
  if (const char *sm = getenv("ARTIS_GPU_MAREC_SCRATCH_MB")) k.marec_scratch_doubles = (int64_t)(atof(sm) * (1 << 20) / 8);
  if (const char *mx = getenv("ARTIS_GPU_MACACHE_MAX_GB")) {
    k.have_macache_max = true;
    k.macache_max_bytes = atof(mx) * (double)(1ull << 30);
  }
  if (const char *mr = getenv("ARTIS_GPU_MACACHE_ROWS")) {
    k.have_macache_rows = true;
    k.macache_rows = atoll(mr);
  }
  k.no_macache = first_is("ARTIS_GPU_NO_MACACHE", '1');
  if (const char *mx = getenv("ARTIS_GPU_LINECOEF_MAX_GB")) {
    k.have_linecoef_max = true;
    k.linecoef_max_bytes = atof(mx) * (double)(1ull << 30);
  }
  if (const char *lr = getenv("ARTIS_GPU_LINECOEF_ROWS")) {
    k.have_linecoef_rows = true;
    k.linecoef_rows = atoi(lr);
  }
  k.no_linecoef = first_is("ARTIS_GPU_NO_LINECOEF", '1');
  const char *lcg = getenv("ARTIS_GPU_LINECOEF_GATHER");
  k.linecoef_gather = lcg && atoi(lcg);
  if (const char *ev = getenv("ARTIS_GPU_TE_LANES")) {
    const int v = atoi(ev);
    if (v >= 1 && v <= 64) k.te_lanes = v;
  }
  if (const char *v = getenv("ARTIS_GPU_SF_BATCH_GB")) k.sf_batch_gb = std::max(0.0, atof(v));
  const char *vo = getenv("ARTIS_VPKT_OCC");
  const int occ = vo ? atoi(vo) : VPKT_OCC_DEFAULT;
  k.vpkt_occ = (occ == 2 || occ == 3) ? occ : 1;
  k.vpkt_lconly = !first_is("ARTIS_VPKT_LCONLY", '0');
  k.vpkt_sort = !first_is("ARTIS_VPKT_SORT", '0');
  return k;
}

// =============================================================================================== device memory
// Every device allocation of the engine goes through dmalloc: ARTIS_GPU_FAIL_ALLOC_ABOVE=<bytes> makes any single
// request above that size fail as out-of-memory, so the error paths can be tested.
inline hipError_t dmalloc(void **p, size_t bytes) {
  *p = nullptr;
  if (const char *lim = getenv("ARTIS_GPU_FAIL_ALLOC_ABOVE"))
    if (bytes > (size_t)strtoull(lim, nullptr, 10)) return hipErrorOutOfMemory;
  return hipMalloc(p, bytes);
}

template <typename T>
void dfree(T *&p) {
  if (p) (void)hipFree((void *)p);
  p = nullptr;
}

// Owner of a set of allocations released together.  The engine holds three (Engine::mem and the two sets that can
// be made again, mem_vpkt and mem_gamma); DevBufs is the call-scoped form.  The buffers that grow on demand (packet
// store, vpkt spawn and sort buffers, snapshot, reduce block) are named pointers instead, released by
// release_engine().
struct Arena {
  std::vector<void *> p;
  hipError_t raw(void **d, size_t bytes) {
    const hipError_t e = dmalloc(d, bytes);
    if (e == hipSuccess) p.push_back(*d);
    return e;
  }
  void release() {
    for (void *q : p) (void)hipFree(q);
    p.clear();
  }
};

struct Engine {
  bool initialised = false;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
  Knobs knob;
  Arena mem;        // engine lifetime
  Arena mem_vpkt;   // the parameter set of the last artis_gpu_vpkt_init
  Arena mem_gamma;  // the tables of the last artis_gpu_init_gamma
  Ctx K{};
  artis_run_params params{};
  // sizes
  int npts_model = 0, nelements = 0, maxnions = 0, nions_total = 0, nlines = 0, ngrid = 0, ntstep = 0;
  EstLayout est{};  // the estimator block as laid out at init (est_block.h)
  int64_t ma_key_stride = 0;          // 16-bit keys per cell block of the macro-atom cache
  bool ma_cache_ok = true;             // the atomic data fit the cache's record layout (engine_dev.h ma_layout)
  std::vector<int64_t> h_dbl_off;     // per level: offset (doubles) of its exact sums in the k_marates scratch
  std::vector<MaMeta> h_ma_meta;      // host copy of DevTab::ma_meta (artis_gpu_cell_ma_keys decodes records with it)
  double *d_marec_scratch = nullptr;  // k_marates output, [position][cell] per level (k_mapack input)
  // macro-atom key records (DevCells::ma_row / ma_bin): row of each cell (row mode), the cell of each bin
  int32_t *d_ma_row = nullptr, *d_ma_bin = nullptr, *d_ma_bincell = nullptr;
  // level mode (DevCells::ma_lptr): pool capacity, record size per level in 128-byte lines (0: never recorded),
  // the activity histogram of the walks since the last placement, and the placement's bookkeeping
  uint32_t *d_ma_lptr = nullptr, *d_ma_lhist = nullptr, *d_lvl_ctr = nullptr;
  const uint32_t *d_rec_lines = nullptr, *d_rl_off = nullptr;
  uint32_t row_lines = 0;  // pool lines of one whole cell's records (the initial placement)
  unsigned long long *d_lvl_buckets = nullptr;
  int2 *d_build_list = nullptr;
  int64_t build_list_cap = 0;
  int64_t ma_level_small = 0, ma_level_large = 0;  // the build list's front (small levels) and back (large) parts
  uint64_t ma_pool_lines = 0;
  std::vector<uint32_t> h_rec_lines;
  int64_t ma_build_lds_doubles = 0;
  bool ma_lhist_ready = false;
  bool ma_initial_placement = false;  // the current placement had no activity to go by (whole cells)
  int64_t ma_level_records = 0, ma_level_lines = 0;  // records / pool lines of the current placement
  // level mode: sampled jumps on pairs that had a record / on all pairs, over the transports before the last placement
  int64_t ma_acts_cached = 0, ma_acts_total = 0;
  int64_t marec_scratch_doubles = 0;
  double *d_estblock = nullptr;
  int32_t *d_target_ul = nullptr, *d_target_t = nullptr;
  bool have_cells = false;
  int cellstate_nts = -1;
  int cap_nonempty = 0;
  // cell-state device buffers
  float *d_cellf = nullptr;  // packed float arrays
  int16_t *d_thick = nullptr;
  float *d_abund = nullptr, *d_glp = nullptr, *d_pf = nullptr;
  double *d_totcool = nullptr, *d_ccion = nullptr, *d_renorm = nullptr;
  // nebular inputs (device copies, npts_model-indexed) and the NO_LUT integration workspace
  double *d_nltepops = nullptr, *d_ntdep = nullptr, *d_ntY = nullptr;
  float *d_rfTR = nullptr, *d_rfW = nullptr, *d_bfest = nullptr, *d_ntprob = nullptr, *d_ntionen = nullptr;
  QagWs qag{};
  int32_t *d_bfcol = nullptr;  // bflist index -> element * maxnions + ion (spectra emission columns)
  int qag_waves = 0;
  int32_t *d_ne_index = nullptr, *d_ne_mgi = nullptr;
  // packets
  uint64_t *d_soa = nullptr, *d_aos = nullptr, *d_snapshot = nullptr;
  int64_t cap_pkts = 0, npkts = 0;
  bool have_snapshot = false;
  // wavefront engine (wavefront.h)
  WaveState W{};
  uint32_t *h_ctr = nullptr;  // pinned [2][NQUEUES * 2]
  hipEvent_t ev_round[2] = {nullptr, nullptr};
  int wave_grid = 2048;
  Ctx *d_ctx = nullptr;           // device copy of K for the transport kernels
  uint32_t *d_binoffs = nullptr;  // exclusive prefix sums of W.bins
  void *d_scan_tmp = nullptr;
  size_t scan_tmp_bytes = 0;
  int64_t last_rounds = 0;
  // per kernel class (rpkt, ma, kpkt, classify+bookkeeping): summed device time and launch count of the last
  // transport, from events bracketing every launch
  std::vector<hipEvent_t> tev;
  std::vector<int> tev_class;
  size_t tev_used = 0;
  double last_kernel_ms[ARTIS_KCLASS_COUNT] = {0};
  int64_t last_kernel_launches[ARTIS_KCLASS_COUNT] = {0};
  double last_transport_ms = 0., last_precompute_ms = 0.;
  int64_t last_work[ARTIS_WORK_COUNT] = {0};
  // virtual packets (vpkt.h): device accumulators and the spawn buffer (sized per update)
  int64_t vpkt_cap_param = 0;
  std::vector<int32_t> h_anumber;  // artis_atomic_tables.elem_anumber
  std::vector<double> h_ion_ionpot;  // artis_atomic_tables.ion_ionpot (get_mean_binding_energy)
  double last_nlte_ms = 0.;
  std::vector<int32_t> h_line_elem;  // artis_atomic_tables.line_elementindex (virtual-packet line masks)
  double *d_vpkt_spawn = nullptr;
  uint32_t vpkt_spawn_cap = 0;
  uint32_t *d_qsnap = nullptr;    // queue count when the current k_rpkt / k_kpkt launch started (vpkt_drain)
  // spawn sort (DevVpkt::perm): keys / indices in and out, hipcub temp storage, sized for vpkt_spawn_cap
  uint32_t *d_vkey = nullptr, *d_vkey2 = nullptr, *d_vidx = nullptr, *d_vperm = nullptr;
  void *d_vsort_tmp = nullptr;
  size_t vsort_tmp_bytes = 0;
  uint32_t *h_vcount = nullptr;   // pinned: spawn count before a flush
  uint32_t *h_vfull = nullptr;    // pinned: DevVpkt::full after a launch
  int64_t vpkt_drains = 0;        // launches resumed after a full spawn buffer (last update_packets)
  std::vector<hipEvent_t> vev;  // (start, end) pairs around the k_vpkt launches of the last update
  size_t vev_used = 0;
  double last_vpkt_ms = 0.;
  int64_t last_vpkt_work[4] = {0, 0, 0, 0};
  int64_t last_vpkt_spawns = 0, last_vpkt_traces = 0;
  // RCCL communicator of this rank (artis_gpu_comm_init) and the packed block it all-reduces
  ncclComm_t comm = nullptr;
  int comm_ranks = 0;
  double *d_redblock = nullptr;
  double last_te_ms = 0.;
  std::string last_error;
};
Engine G;

#define HIPCHK(x)                                                                             \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess) {                                                                   \
      G.last_error = std::string(#x) + ": " + hipGetErrorString(e_);                          \
      return ARTIS_ERR_HIP;                                                                   \
    }                                                                                         \
  } while (0)

// count elements (at least one) in arena A; dupload also copies src into them (host-synchronous: a pageable
// source may be a temporary, and an asynchronous copy queued behind running kernels would read it after it is gone)
template <typename T>
int dalloc(Arena &A, T **p, size_t count) {
  if (count == 0) count = 1;
  HIPCHK(A.raw((void **)p, count * sizeof(T)));
  return 0;
}
template <typename T>
int dupload(Arena &A, const T **dst, const T *src, size_t count) {
  T *d = nullptr;
  if (dalloc(A, &d, count)) return ARTIS_ERR_HIP;
  if (count && src) HIPCHK(hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice));
  *dst = d;
  return 0;
}
// ... in the engine-lifetime arena
template <typename T>
int dalloc(T **p, size_t count) {
  return dalloc(G.mem, p, count);
}
template <typename T>
int dupload(const T **dst, const T *src, size_t count) {
  return dupload(G.mem, dst, src, count);
}
template <typename T>
int dupload(const T **dst, const std::vector<T> &src) {
  return dupload(G.mem, dst, src.data(), src.size());
}

// call-scoped scratch: released when the call returns, on every path
struct DevBufs : Arena {
  DevBufs() = default;
  DevBufs(const DevBufs &) = delete;
  ~DevBufs() { release(); }
  template <typename T>
  int get(T **d, size_t count, const T *src) {
    if (dalloc(*this, d, count)) return ARTIS_ERR_HIP;
    if (src) HIPCHK(hipMemcpy(*d, src, count * sizeof(T), hipMemcpyHostToDevice));
    return 0;
  }
};

// The caller's arrays of one entry point, each listed once with its device slot, element count and host pointer:
// allocated in B and uploaded (a NULL host pointer only allocates, which also serves for scratch), and -- io() with
// a host pointer and a non-zero count -- noted for download(), which copies every noted array back with the size of
// its listing.  A failed listing shows in rc.
struct CallerArrays {
  struct Back {
    const void *dev;
    void *host;
    size_t bytes;
  };
  DevBufs &B;
  std::vector<Back> back;
  int rc = 0;
  explicit CallerArrays(DevBufs &b) : B(b) {}
  template <typename T>
  void in(const T **d, size_t count, const T *host) {
    rc |= B.get((T **)d, count, host);
  }
  template <typename T>
  void io(T **d, size_t count, T *host) {
    rc |= B.get(d, count, (const T *)host);
    if (host && count) back.push_back({*d, host, count * sizeof(T)});
  }
  int download() const {
    for (const Back &b : back) HIPCHK(hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
    return 0;
  }
};

}  // namespace
