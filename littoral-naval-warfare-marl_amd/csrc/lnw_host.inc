// lnw_host.inc — the host side of liblnw: error handling, lnw_handle, the
// kernel tables and launch planning (STEP_KERNELS, OBS_KERNELS, plan_step,
// plan_observe, choose_epw), the kernel launches and the C-ABI of include/lnw.h
// (lnw_create .. lnw_copy, state snapshots). Included last by lnw_kernels.hip,
// still inside the anonymous namespace the kernels opened: the kernel templates
// are launched from here, so it is the same translation unit.

// ===========================================================================
// host side
// ===========================================================================
thread_local std::string g_err;

int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess)                                                             \
      return fail(LNW_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));    \
  } while (0)

void host_constants(KParams &k) {
  const double base = std::sqrt((4.0 / 3.0) * 6370.0 * 2.0);
  const int masts[2] = {15, 30};
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 2; j++) {
      double d = base * (std::sqrt((double)masts[i] / 1000.0) + std::sqrt((double)masts[j] / 1000.0));
      k.d5[i][j] = d / 5.0;
    }
  for (int i = 0; i < 2; i++)
    k.den[i] = (base * (std::sqrt((double)masts[i] / 1000.0) + std::sqrt(15.0 / 1000.0))) / 5.0;
  k.det_q[0] = 0.345 - 0.1;
  k.det_q[1] = 0.345 + 0.1;
  const double ps[2] = {0.45, 0.63};
  for (int h = 0; h < 2; h++)
    for (int n = 0; n < 9; n++) {
      k.hit64[h][n] = 1.0 - std::pow(1.0 - ps[h], (double)n);
      float pn = powf((float)(1.0 - ps[h]), (float)n);
      k.hit32[h][n] = 1.0f - pn;
    }
}

}  // namespace

// The environment knobs of a handle. Constructing one reads them: once, as
// lnw_create makes the handle. (LNW_EPW_RT alone is read where it acts, in choose_epw.)
struct Knobs {
  static bool on(const char *name) { return getenv(name) != nullptr; }
  int dbg_skip = on("LNW_DEBUG_SKIP") ? atoi(getenv("LNW_DEBUG_SKIP")) : 0;  // (checked by lnw_create)
  bool prof = on("LNW_PROF");                    // per-workgroup phase timestamps and their report
  bool force_generic = on("LNW_FORCE_GENERIC");  // the runtime-size kernels for every team shape
  bool no_group = on("LNW_NO_GROUP");            // runtime team sizes on the one-lane-per-env kernel (A/B tests)
  bool force_group = on("LNW_FORCE_GROUP");      // (A/B) the group kernel for templated team sizes too
  bool no_split_rows = on("LNW_NO_SPLIT_ROWS");  // (A/B) row-writing contact steps keep phase S on one wave
  bool no_units = on("LNW_NO_UNITS");            // one 64-env unit per workgroup for the headline shape (A/B tests)
  bool no_prod = on("LNW_NO_PROD");              // the generic units kernel where the production one would run (A/B tests)
  bool no_slab = on("LNW_NO_SLAB");              // no two-slab direct rows (A/B)
  bool no_xcd_remap = on("LNW_NO_XCD_REMAP");    // KParams.xcd_remap off (A/B)
  // LNW_GROUP_MARCH=1: the group kernel marches its pair LOS over the LDS
  // terrain mask instead of loading LOS-table words (A/B)
  bool group_march = on("LNW_GROUP_MARCH");
  bool no_store_wt = on("LNW_NO_STORE_WT");      // non-temporal observation stores kept (A/B)
};

struct lnw_handle {
  int device = 0;
  Knobs knobs;
  lnw_params params{};
  KParams kp{};
  // device copies of every distinct cold block this handle has launched with,
  // each written once and kept until lnw_destroy (cold_commit)
  struct ColdSlot { KCold host; KCold *dev; };
  std::vector<ColdSlot> cold_slots;
  int E = 0, nb = 0, nr = 0, A = 0, T = 0, nmax = 0;
  long long env_base = 0;
  int G = 0, W16 = 0;
  bool terrain = false;
  // device buffers
  uint8_t *d_grid = nullptr;
  float *d_gridf = nullptr, *d_winf = nullptr, *d_dummy = nullptr;
  unsigned long long *d_prof = nullptr;  // LNW_PROF phase timestamps
  size_t prof_cap = 0;                   // d_prof capacity in slots (grown to the launch grid)
  lnw_analytics ana{};                   // bound analytics buffers (lnw_set_analytics)
  unsigned long long *ctr = nullptr;     // bound work counters (lnw_set_counters)
  bool store_wt = false;
  // fixed by lnw_load_terrain (the LDS sizes depend on the grid):
  bool group_fits = false;  // the group kernel's required LDS parts fit (else runtime sizes stay on step_kernel<0, 0>)
  GroupLds group_lds{};     // the group kernel's dynamic LDS (total bytes, which optional parts are staged)
  bool units_fit = false;   // UNITS blocks of the step layout fit one workgroup
  bool contact = false;  // lnw_set_variant: contact-heavy phase-S code in the templated kernels
  int last_kernel = LNW_KERNEL_NONE;     // lnw_step_kernel: what the last lnw_step launched
  bool last_prod = false;                // lnw_step_kernel_prod: it was step_units_prod_kernel
  bool has_medium = false;               // the spawn spec has medium ships (runtime-size kernels only)
  unsigned long long terrain_hash = 0;   // FNV-1a of the loaded grid (state snapshots name their terrain)
  uint32_t *d_mask2 = nullptr, *d_mvtab = nullptr, *d_lostab = nullptr;
  uint32_t *pos = nullptr;
  int32_t *radar = nullptr, *steps = nullptr, *envi = nullptr;
  uint8_t *miss = nullptr, *mkind = nullptr, *alive = nullptr, *type = nullptr;
  double *dist_lz = nullptr, *duct = nullptr, *bear_val = nullptr, *d_atan = nullptr;
  uint8_t *bear_ship = nullptr;
  uint16_t *tl_cnt = nullptr, *tl = nullptr;
  unsigned long long *rng = nullptr;
  uint32_t *err = nullptr;
  int32_t *sp_types = nullptr, *sp_pos = nullptr, *sp_randls = nullptr, *sp_pos_env = nullptr;
  bool sp_pos_env_on = false;  // auto-reset respawns on the per-env cells of the last lnw_reset
  const double *tape = nullptr;
  const long long *tape_off = nullptr;
  std::vector<void *> allocs;
};

namespace {

template <class T>
int dalloc(lnw_handle *h, T **p, size_t n) {
  void *q = nullptr;
  hipError_t e = hipMalloc(&q, n * sizeof(T) + 16);
  if (e != hipSuccess) return fail(LNW_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  (void)hipMemset(q, 0, n * sizeof(T) + 16);
  h->allocs.push_back(q);
  *p = (T *)q;
  return 0;
}

KState make_state(lnw_handle *h) {
  KState s{};
  s.pos = h->pos; s.radar = h->radar; s.miss = h->miss; s.mkind = h->mkind; s.alive = h->alive;
  s.type = h->type; s.steps = h->steps; s.dist_lz = h->dist_lz; s.tl_cnt = h->tl_cnt; s.tl = h->tl;
  s.duct = h->duct; s.envi = h->envi; s.rng = h->rng; s.err = h->err;
  s.atan_deg = h->d_atan;
  s.grid = h->d_grid; s.gridf = h->d_gridf; s.winf = h->d_winf; s.dummy = h->d_dummy; s.prof = nullptr; s.cold = nullptr; s.mask2 = h->d_mask2; s.mvtab = h->d_mvtab; s.lostab = h->d_lostab;
  s.nmax = h->nmax;
  return s;
}

// The device block holding the handle's current cold values (KCold), for the
// launch about to be made. Blocks are versioned, never rewritten: a set of
// values not seen before gets a block of its own, written (a blocking copy)
// before this returns, and launches made from now on point to it; launches
// already queued, and captured graphs, keep reading the block they were given,
// which stays as it was until lnw_destroy. So no setter has to wait for the
// device, and a value set back to an earlier one (counters or analytics
// toggled) reuses that block. Every entry point that launches a kernel taking KState goes
// through here (launch_state), so whatever changed the handle (a setter,
// lnw_reset's spawn spec, lnw_set_state) is picked up; the setters also commit
// at once, so that a step captured into a graph right after them finds its
// block ready (no allocation while capturing).
int cold_commit(lnw_handle *h, ColdPtr *out) {
  KCold c;
  memset(&c, 0, sizeof c);
  c.ana = h->ana;
  c.tape = h->tape; c.tape_off = h->tape_off;
  c.sp_types = h->sp_types; c.sp_pos = h->sp_pos; c.sp_randls = h->sp_randls;
  c.sp_pos_env = h->sp_pos_env_on ? h->sp_pos_env : nullptr;
  c.bear_val = h->bear_val; c.bear_ship = h->bear_ship;
  c.ctr = h->ctr;
  // newest first: the current block is almost always the last one made
  for (size_t i = h->cold_slots.size(); i-- > 0;)
    if (memcmp(&h->cold_slots[i].host, &c, sizeof c) == 0) {
      if (out) *out = (ColdPtr)h->cold_slots[i].dev;
      return 0;
    }
  KCold *d = nullptr;
  HIPCHK(hipSetDevice(h->device));
  if (int rc = dalloc(h, &d, 1)) return rc;
  HIPCHK(hipMemcpy(d, &c, sizeof c, hipMemcpyHostToDevice));
  h->cold_slots.push_back({c, d});
  if (out) *out = (ColdPtr)d;
  return 0;
}

// A launch's KState: the handle's arrays and the cold block's pointer.
int launch_state(lnw_handle *h, KState &s) {
  s = make_state(h);
  return cold_commit(h, &s.cold);
}

// compute units of a device (cached per device; the one place that asks the runtime)
int device_ncu(int dev) {
  static int cache[64] = {0};
  int &c = cache[dev & 63];
  if (c == 0) {
    int n = 0;
    c = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
  }
  return c;
}

// ===========================================================================
// launch planning: which kernel, grid, block and LDS a step or observe launch
// takes (plan_step, plan_observe), and the envs per workgroup (choose_epw).
// The plans read the handle only; nothing here makes a HIP call but device_ncu.
// ===========================================================================
using StepFn = void (*)(KParams, KState, void *, const uint8_t *, float *, float *, float *, float *, int32_t *,
                        float *);
using ObsFn = void (*)(KParams, KState, int, float *, float *);

// One kernel the host can launch: its public code (LNW_KERNEL_*; for an observe
// kernel, that of the step kernel it pairs with), its threads per workgroup
// (the kernel's __launch_bounds__) and the dynamic LDS lnw_load_terrain opts it
// in for. A kernel is launched only through its row, so it cannot miss the opt-in.
template <class Fn>
struct KernelRow { Fn fn; int code, threads, lds_cap; };

constexpr int TEAM_THREADS = EPW == WAVE ? 2 * WAVE : WAVE;  // step_kernel<N, N> with N > 0

// rows of STEP_KERNELS; the plain n-v-n kernels sit at SK_2V2 + 2 * (n - 2) + contact
enum StepK {
  SK_GENERIC, SK_REFLOS, SK_GROUP, SK_2V2, SK_2V2_CONTACT, SK_3V3, SK_3V3_CONTACT, SK_4V4, SK_4V4_CONTACT,
  SK_4V4_SPLIT, SK_4V4_SLAB, SK_UNITS, SK_UNITS_PROD, SK_COUNT
};
const KernelRow<StepFn> STEP_KERNELS[] = {
    {step_kernel<0, 0>, LNW_KERNEL_GENERIC, WAVE, GROUP_LDS_MAX},
    {step_kernel<0, 0, false, true>, LNW_KERNEL_REFLOS, WAVE, GROUP_LDS_MAX},  // diagnostics: the reference's LOS work
    {step_group_kernel, LNW_KERNEL_GROUP, GEPW * GL, GROUP_LDS_MAX},  // runtime team sizes: GL lanes per env (lnw_group.inc)
    {step_kernel<2, 2>, LNW_KERNEL_TEAM, TEAM_THREADS, GROUP_LDS_MAX},
    {step_kernel<2, 2, true>, LNW_KERNEL_TEAM_CONTACT, TEAM_THREADS, GROUP_LDS_MAX},
    {step_kernel<3, 3>, LNW_KERNEL_TEAM, TEAM_THREADS, GROUP_LDS_MAX},
    {step_kernel<3, 3, true>, LNW_KERNEL_TEAM_CONTACT, TEAM_THREADS, GROUP_LDS_MAX},
    {step_kernel<4, 4>, LNW_KERNEL_TEAM, TEAM_THREADS, GROUP_LDS_MAX},
    {step_kernel<4, 4, true>, LNW_KERNEL_TEAM_CONTACT, TEAM_THREADS, GROUP_LDS_MAX},
    // the contact variant with phase S split by side (step_kernel PS)
    {step_kernel<4, 4, true, false, 1, true>, LNW_KERNEL_TEAM_CONTACT, TEAM_THREADS, GROUP_LDS_MAX},
    // two-slab direct rows (step_kernel SL, step_qdirect)
    {step_kernel<4, 4, false, false, 1, false, true>, LNW_KERNEL_TEAM, TEAM_THREADS, GROUP_LDS_MAX},
    // 4 units of 64 envs per workgroup, one workgroup per CU (step_kernel UN)
    {step_kernel<4, 4, false, false, UNITS>, LNW_KERNEL_UNITS, TEAM_THREADS * UNITS, UNITS_LDS_MAX},
    // the same compiled for the production configuration (ProdCfg, prod_config)
    {step_units_prod_kernel, LNW_KERNEL_UNITS, TEAM_THREADS * UNITS, UNITS_LDS_MAX},
};
static_assert(sizeof STEP_KERNELS / sizeof STEP_KERNELS[0] == SK_COUNT, "one row per StepK");

// the runtime-size kernel, then the n-v-n kernels at 1 + 2 * (n - 2) + contact
// (two waves for the contact shapes only: blue's calls on wave 0, red's on wave 1)
const KernelRow<ObsFn> OBS_KERNELS[] = {
    {observe_kernel<0, 0, false>, LNW_KERNEL_GENERIC, WAVE, GROUP_LDS_MAX},
    {observe_kernel<2, 2, false>, LNW_KERNEL_TEAM, WAVE, GROUP_LDS_MAX},
    {observe_kernel<2, 2, true>, LNW_KERNEL_TEAM_CONTACT, 2 * WAVE, GROUP_LDS_MAX},
    {observe_kernel<3, 3, false>, LNW_KERNEL_TEAM, WAVE, GROUP_LDS_MAX},
    {observe_kernel<3, 3, true>, LNW_KERNEL_TEAM_CONTACT, 2 * WAVE, GROUP_LDS_MAX},
    {observe_kernel<4, 4, false>, LNW_KERNEL_TEAM, WAVE, GROUP_LDS_MAX},
    {observe_kernel<4, 4, true>, LNW_KERNEL_TEAM_CONTACT, 2 * WAVE, GROUP_LDS_MAX},
};

// The team-shape test, written once: equal sides of 2..4 ships have kernels with
// compile-time sizes and two waves per workgroup. Each user adds its own further
// conditions where it applies this; they differ (DESIGN.md, "Kernel variants").
bool team_shape(const lnw_handle *h) {
  return !h->knobs.force_generic && h->nb == h->nr && h->nb >= 2 && h->nb <= 4 && EPW == WAVE;
}

// LDS of the step layout, with row stages for `rows` rows per side (lds_layout's qbig)
size_t step_lds_bytes(const lnw_handle *h, int rows = 0) {
  return (size_t)lds_layout(h->A, h->nb, h->nr, h->nmax, h->G * h->W16, h->G, rows).total;
}

// Quiet workgroups' direct rows (quiet_step_t): a workgroup of up to 64 / nb envs
// stages both sides' rows whole (qbig) and wave 1 builds and stores every row
// from registers; up to 128 / nb envs it does so in two slabs of 64 / nb envs,
// for the non-contact kernels and only when the larger LDS still holds the whole
// grid at once (config 3 at N = 4: 16 384 envs, 32 per workgroup). Larger
// workgroups stream their rows in staged passes (quiet_emit_t).
bool step_qdirect(const lnw_handle *h, int epw) {
  // LOS-table mode and no medium ships only; LNW_FORCE_GROUP is not looked at
  // (the group kernel is still passed this value in KParams)
  if (!team_shape(h) || h->has_medium || h->params.los_mode != 0) return false;
  if (epw * h->nb <= WAVE) return true;
  // (4v4 only: step_kernel<4, 4, .., SL> is the one two-slab instantiation)
  if (h->nb != 4 || h->contact || h->knobs.no_slab || epw * h->nb > 2 * WAVE) return false;
  int per_cu = (int)((160 * 1024) / (step_lds_bytes(h, WAVE) + 1024));
  if (per_cu > 4) per_cu = 4;  // 256 VGPRs: two waves per SIMD
  return (h->E + epw - 1) / epw <= (long long)device_ncu(h->device) * per_cu;
}

// the step launch's LDS: step_lds_bytes plus the whole-side row stages of
// small quiet workgroups (the same condition step_kernel evaluates)
size_t step_launch_lds_bytes(const lnw_handle *h, int epw) {
  return step_lds_bytes(h, step_qdirect(h, epw) ? (epw * h->nb < WAVE ? epw * h->nb : WAVE) : 0);
}

// The production configuration, checked value by value against the launch about
// to be made. What ProdCfg (lnw_kernels.hip) compiles into
// step_units_prod_kernel: grid side 100; float32 action rows without row
// kinds; table LOS and moves; no LNW_DEBUG_SKIP bit; no LNW_PROF buffer (team
// sizes, 7x7 windows and 64-env units are the units kernel's own conditions,
// plan_step); a group that a measurement build leaves runtime
// (LNW_PROD_GROUPS) is not checked. And what the kernel still reads at run time
// but a production launch has: no work counters or analytics channels, Philox
// draws, float32 rewards, write-through rows. Those keep the kernel to the
// configuration its tests run it in.
bool prod_config(const lnw_handle *h, int act_dtype, bool row_kind) {
  const lnw_analytics &an = h->ana;
  const bool ana = an.heatmap || an.coldmap || an.launch || an.eng_log || an.ew_log;
  auto ok = [](int group, bool holds) { return !(ProdCfg::GROUPS & group) || holds; };
  return ok(PG_GRID, h->G == PROD_G && h->W16 == (PROD_G + 15) / 16) &&
         ok(PG_ACTIONS, act_dtype == LNW_ACT_F32 && !row_kind) &&
         ok(PG_MODES, h->params.los_mode == 0 && h->params.move_mode == 0) &&
         ok(PG_DEBUG, h->knobs.dbg_skip == 0) && ok(PG_PROF, !h->knobs.prof) &&
         // the rest of the production configuration, which the kernel reads at run time
         !h->ctr && !ana && h->kp.rng_mode == LNW_RNG_PHILOX && !h->kp.rew_f64 && h->store_wt;
}

// One step launch, decided: the kernel's table row, its launch shape, KParams'
// qdirect and the number of LNW_PROF records the launch writes (nwg).
struct StepPlan {
  const KernelRow<StepFn> *row;
  unsigned grid, block, nwg;
  size_t lds;
  bool qdirect;
};

StepPlan plan_step(const lnw_handle *h, int epw, bool no_obs, int act_dtype, bool row_kind) {
  const Knobs &kn = h->knobs;
  const int los = h->params.los_mode;
  const bool cw = h->contact;
  // compile-time sizes: not the reference's LOS work, not medium ships (5x5
  // windows and shorter rows, the runtime-size kernels only), and not under
  // LNW_FORCE_GROUP where the group kernel can run
  const bool templated = team_shape(h) && los != 2 && !h->has_medium && !(kn.force_group && h->group_fits);
  const bool group = los != 2 && !templated && !kn.force_generic && !kn.no_group && h->group_fits;
  // 4v4 at 64 envs per workgroup in LOS-table mode, whole units (the headline):
  // the units kernel (LNW_NO_UNITS keeps one unit per workgroup)
  const bool units = templated && h->nb == 4 && !cw && !kn.no_units && h->units_fit && epw == EPW && los == 0 &&
                     h->E % (EPW * UNITS) == 0 && !(kn.dbg_skip & (1 | 2 | 512));
  StepPlan p;
  p.qdirect = step_qdirect(h, epw);
  int r = group ? SK_GROUP : SK_GENERIC;
  // (LNW_NO_PROD keeps the generic units kernel, beside LNW_NO_UNITS)
  if (units) r = !kn.no_prod && prod_config(h, act_dtype, row_kind) ? SK_UNITS_PROD : SK_UNITS;
  else if (los == 2) r = SK_REFLOS;
  // the contact variant with phase S split by side (LNW_NO_SPLIT_ROWS: only for steps without rows, A/B)
  else if (templated && h->nb == 4 && cw && los == 0 && (no_obs || !kn.no_split_rows)) r = SK_4V4_SPLIT;
  else if (templated && h->nb == 4 && !cw && p.qdirect && epw * 4 > WAVE) r = SK_4V4_SLAB;
  else if (templated) r = SK_2V2 + 2 * (h->nb - 2) + (cw ? 1 : 0);
  p.row = &STEP_KERNELS[r];
  p.block = (unsigned)p.row->threads;
  // one LNW_PROF record per unit of epw envs, or per workgroup of the group kernel
  p.grid = p.nwg = (unsigned)((h->E + epw - 1) / epw);
  p.lds = step_launch_lds_bytes(h, epw);
  if (units) {
    p.grid = (unsigned)(h->E / (EPW * UNITS));
    p.lds = (size_t)UNITS * ((p.lds + 15) & ~(size_t)15);
  } else if (group) {
    p.grid = p.nwg = (unsigned)((h->E + GEPW - 1) / GEPW);
    p.lds = (size_t)h->group_lds.total;
  }
  return p;
}

// lnw_observe's launch: the step layout without row stages, at the handle's
// epw. Unlike plan_step it does not look at LNW_FORCE_GROUP (there is no group
// observe kernel).
struct ObsPlan {
  const KernelRow<ObsFn> *row;
  unsigned grid, block;
  size_t lds;
};

ObsPlan plan_observe(const lnw_handle *h) {
  const bool templated = team_shape(h) && !h->has_medium && h->params.los_mode != 2;
  const KernelRow<ObsFn> *row = &OBS_KERNELS[templated ? 1 + 2 * (h->nb - 2) + (h->contact ? 1 : 0) : 0];
  return {row, (unsigned)((h->E + h->kp.epw - 1) / h->kp.epw), (unsigned)row->threads, step_lds_bytes(h)};
}

// Environments per workgroup: EPW (one env per lane) unless that leaves the GPU
// with fewer workgroups than it can hold at once; then halve it (down to 16 for
// the two-wave kernels, 1 otherwise) until the grid fills every resident slot. A step is a per-lane latency chain, so a
// workgroup with fewer live lanes takes about as long as a full one, and more
// workgroups in flight finish the batch in fewer rounds (config 4: 8 192 envs
// -> 512 workgroups of 16 instead of 128 of 64). LNW_EPW_RT overrides.
int choose_epw(const lnw_handle *h) {
  if (const char *e = getenv("LNW_EPW_RT")) {
    int v = atoi(e);
    if (v >= 1 && v <= EPW) return v;
  }
  const int ncu = device_ncu(h->device);
  // epw is chosen (lnw_load_terrain) before a reset can set has_medium or
  // lnw_set_variant the contact flag, and LNW_FORCE_GROUP is not looked at: the
  // shape counts as two-wave unless the reference's LOS work excludes it
  const bool two_wave = team_shape(h) && h->params.los_mode != 2;
  const int by_waves = two_wave ? 4 : 8;  // 256 VGPRs: two waves per SIMD
  // resident workgroups at a given epw (the launch's LDS depends on it: small
  // quiet workgroups carry whole-side row stages)
  auto slots = [&](int e) {
    const size_t lds = step_launch_lds_bytes(h, e) + 1024;
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > by_waves) per_cu = by_waves;
    if (per_cu < 1) per_cu = 1;
    return (long long)ncu * per_cu;
  };
  // two-wave kernels stop at 16 envs per workgroup: below that each workgroup's
  // fixed head (terrain mask staging, state columns) outweighs the shorter
  // chain (8 192 envs: 20.2 us at 16, 20.5 at 8, 22.3 at 32, 29.0 at 64)
  const int min_epw = two_wave ? 16 : 1;
  int epw = EPW;
  while (epw > min_epw && (h->E + epw - 1) / epw < slots(epw)) epw /= 2;
  if ((h->E + epw - 1) / epw > slots(epw) && epw < EPW) epw *= 2;  // never more rounds than EPW needs
  return epw;
}

}  // namespace

extern "C" {

int lnw_abi_version(void) { return LNW_ABI_VERSION; }
const char *lnw_last_error(void) { return g_err.c_str(); }

int lnw_set_analytics(lnw_handle *h, const lnw_analytics *a) {
  if (!h) return fail(LNW_EINVAL, "null handle");
  if (!a) { h->ana = lnw_analytics{}; return cold_commit(h, nullptr); }
  if ((a->eng_log && (!a->eng_count || a->eng_cap < 0)) || (a->ew_log && (!a->ew_count || a->ew_cap < 0)))
    return fail(LNW_EINVAL, "analytics log without a counter or with a negative capacity");
  h->ana = *a;
  return cold_commit(h, nullptr);
}

int lnw_hit_tables(double *tab64, float *tab32) {
  KParams k{};
  host_constants(k);
  for (int h = 0; h < 2; h++)
    for (int n = 0; n < 9; n++) {
      if (tab64) tab64[h * 9 + n] = k.hit64[h][n];
      if (tab32) tab32[h * 9 + n] = k.hit32[h][n];
    }
  return 0;
}

int lnw_create(const lnw_params *params, int32_t n_envs, int32_t nb, int32_t nr, int32_t device,
               int64_t env_id_base, lnw_handle **out) {
  if (!params || !out) return fail(LNW_EINVAL, "null argument");
  if (n_envs <= 0) return fail(LNW_EINVAL, "n_envs must be > 0");
  if (nb < 1 || nr < 1 || nb > 16 || nr > 16)
    return fail(LNW_EUNSUPPORTED, "need 1 <= nb, nr <= 16 ships per side");
  HIPCHK(hipSetDevice(device));
  lnw_handle *h = new lnw_handle();  // (reads the environment knobs)
  h->device = device;
  const Knobs &kn = h->knobs;
#ifndef LNW_DIAG
  // the shipped library honours only the knobs that change the launch shape or
  // code path, never the results (bit 9: no quiet path, 15: the group kernel's
  // fire loop entry by entry, 17: per-lane bearing loop, 22/23: where the
  // head's loads are issued (22: the staged quiet forms' first pass only), 28: the per-env quiet test in small workgroups,
  // 29: their env counters loaded in phase Q); section skips and
  // replaced arithmetic exist only in the diagnostics build (-DLNW_DIAG,
  // lnw.build.build_diag)
  constexpr int kResultPreserving = 512 | 32768 | 131072 | 4194304 | 8388608 | (1 << 28) | (1 << 29);
  if (kn.dbg_skip & ~kResultPreserving) {
    const int bad = kn.dbg_skip & ~kResultPreserving;
    delete h;
    return fail(LNW_EINVAL, "LNW_DEBUG_SKIP bits " + std::to_string(bad) +
                                " change results; they exist only in the diagnostics build (-DLNW_DIAG)");
  }
#endif
  h->kp.xcd_remap = kn.no_xcd_remap ? 0 : 1;
  h->kp.group_march = kn.group_march ? 1 : 0;
  // write-through observation stores (st_obs4) while a side's output fits the
  // 32-bit buffer offsets
  {
    const int ns = nb > nr ? nb : nr;
    const double side_bytes = (double)n_envs * ns * (4 * ns + 52) * 4.0;
    h->store_wt = !kn.no_store_wt && side_bytes < 2147483648.0;
  }
  h->params = *params;
  h->E = n_envs; h->nb = nb; h->nr = nr; h->A = nb + nr;
  h->nmax = nb > nr ? nb : nr;
  h->T = h->nmax + h->nmax * h->nmax;
  h->env_base = env_id_base;
  const size_t E = (size_t)n_envs, A = (size_t)h->A;
  int rc = 0;
  rc |= dalloc(h, &h->pos, A * E);
  rc |= dalloc(h, &h->radar, A * E);
  rc |= dalloc(h, &h->miss, A * E);
  rc |= dalloc(h, &h->mkind, A * E);
  rc |= dalloc(h, &h->alive, A * E);
  rc |= dalloc(h, &h->type, A * E);
  rc |= dalloc(h, &h->steps, A * E);
  rc |= dalloc(h, &h->dist_lz, A * E);
  rc |= dalloc(h, &h->tl_cnt, A * E);
  rc |= dalloc(h, &h->tl, A * (size_t)h->T * E);
  rc |= dalloc(h, &h->duct, E);
  rc |= dalloc(h, &h->envi, 8 * E);
  rc |= dalloc(h, &h->rng, E);
  rc |= dalloc(h, &h->err, E);
  rc |= dalloc(h, &h->bear_val, (size_t)h->nmax * h->nmax * E);
  rc |= dalloc(h, &h->bear_ship, (size_t)h->nmax * h->nmax * E);
  rc |= dalloc(h, &h->sp_types, 64);
  rc |= dalloc(h, &h->sp_pos, 128);
  rc |= dalloc(h, &h->sp_randls, 64);
  rc |= dalloc(h, &h->d_dummy, 4 * 64);
  rc |= dalloc(h, &h->d_atan, (size_t)LOS_W * LOS_W);
  if (rc) {
    std::string m = g_err;
    lnw_destroy(h);
    return fail(LNW_ENOMEM, m);
  }
  {  // EW bearing table: math.degrees(math.atan2(dy, dx)) for integer offsets in
     // [-R_LOS, R_LOS]^2, computed by the host libm as the reference does
     // (combatant.py:253), so the device needs no atan2 of its own in range
    std::vector<double> at((size_t)LOS_W * LOS_W);
    for (int dy = -R_LOS; dy <= R_LOS; dy++)
      for (int dx = -R_LOS; dx <= R_LOS; dx++)
        at[(size_t)(dy + R_LOS) * LOS_W + (dx + R_LOS)] = atan2((double)dy, (double)dx) * (180.0 / PY_PI);
    HIPCHK(hipMemcpy(h->d_atan, at.data(), at.size() * sizeof(double), hipMemcpyHostToDevice));
    // odd in dy (glibc's atan2 is; checked, not assumed): the group kernel then
    // keeps only the dy >= 0 rows in LDS and negates for dy < 0
    bool odd = true;
    for (int dy = 1; dy <= R_LOS; dy++)
      for (int dx = -R_LOS; dx <= R_LOS; dx++)
        odd = odd && at[(size_t)(R_LOS - dy) * LOS_W + (dx + R_LOS)] == -at[(size_t)(R_LOS + dy) * LOS_W + (dx + R_LOS)];
    h->kp.atan_odd = odd ? 1 : 0;
  }
  KParams &k = h->kp;
  k.discrete = params->discrete; k.landing_ops = params->landing_ops;
  k.aggressive = params->aggressive; k.side_blue = params->side_blue;
  k.trained_red = params->trained_red; k.move_thr = params->move_thr; k.ew_thr = params->ew_thr;
  k.lz_x = params->lz_x; k.lz_y = params->lz_y; k.red_aggression = params->red_aggression;
  k.episode_steps = params->episode_steps; k.auto_reset = params->auto_reset;
  k.los_mode = params->los_mode; k.move_mode = params->move_mode;
  k.E = n_envs; k.nb = nb; k.nr = nr; k.A = h->A; k.T = h->T;
  k.env_base = env_id_base;
  k.rng_mode = LNW_RNG_PHILOX;
  k.seed = 0;
  k.epw = EPW;  // refined by lnw_load_terrain (choose_epw) once the LDS size is known
  k.wc[0] = k.wc[1] = 49;  // 7x7 windows until a reset spawns a side of medium ships
  host_constants(k);
  *out = h;
  return 0;
}

int lnw_destroy(lnw_handle *h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  for (void *p : h->allocs) (void)hipFree(p);
  if (h->d_prof) (void)hipFree(h->d_prof);
  delete h;
  return 0;
}

int lnw_load_terrain(lnw_handle *h, const uint8_t *grid_host, int32_t G) {
  if (!h || !grid_host) return fail(LNW_EINVAL, "null argument");
  if (G < 8 || G > 1024) return fail(LNW_EINVAL, "grid size out of range");
  HIPCHK(hipSetDevice(h->device));
  h->G = G;
  h->W16 = (G + 15) / 16;
  int rc = 0;
  if (h->d_grid) {  // re-load: release the previous terrain structures
    HIPCHK(hipDeviceSynchronize());
    void *old[6] = {h->d_grid, h->d_gridf, h->d_winf, h->d_mask2, h->d_mvtab, h->d_lostab};
    for (void *p : old) {
      for (size_t i = 0; i < h->allocs.size(); i++)
        if (h->allocs[i] == p) { (void)hipFree(p); h->allocs.erase(h->allocs.begin() + i); break; }
    }
  }
  rc |= dalloc(h, &h->d_grid, (size_t)G * G);
  rc |= dalloc(h, &h->d_gridf, (size_t)G * G);
  // the float records, then the byte records (win_bytes_at: in 16-byte units)
  rc |= dalloc(h, &h->d_winf, (size_t)win_bytes_at(G) * 4 + (size_t)LNW_WIN_CLASSES * G * G * LNW_WIN_REC / 4);
  rc |= dalloc(h, &h->d_mask2, (size_t)G * h->W16);
  rc |= dalloc(h, &h->d_mvtab, (size_t)MV_CLASSES * G * G * MV_WORDS);
  rc |= dalloc(h, &h->d_lostab, (size_t)G * G * LOS_CELL_WORDS);
  if (rc) return rc;
  HIPCHK(hipMemcpy(h->d_grid, grid_host, (size_t)G * G, hipMemcpyHostToDevice));
  {
    unsigned long long fh = 1469598103934665603ull ^ (unsigned long long)G;
    for (size_t i = 0; i < (size_t)G * G; i++) fh = (fh ^ grid_host[i]) * 1099511628211ull;
    h->terrain_hash = fh;
  }
  {  // observation window values grid/255 (combatant.py:177), float64 quotient -> float32
    std::vector<float> gf((size_t)G * G);
    for (size_t i = 0; i < gf.size(); i++) gf[i] = (float)((double)grid_host[i] / 255.0);
    HIPCHK(hipMemcpy(h->d_gridf, gf.data(), gf.size() * sizeof(float), hipMemcpyHostToDevice));
    // per-cell observation windows, one record per cell and class (lnw_window.h:
    // [0] Combatant 7x7 around the ship, [1] LandingShip 5x5 rows/cols
    // pos-1..pos+3, [2] medium Combatant 5x5 around the ship; cells outside the
    // hard-coded 0..99 are 0): packed once as 64-byte records of raw grid bytes,
    // which the units kernel's stream converts where it builds a row, and from
    // those the 52-float (13 x float4) records of the other readers
    std::vector<uint8_t> wb((size_t)LNW_WIN_CLASSES * G * G * LNW_WIN_REC);
    win_pack_records(grid_host, G, wb.data());
    const size_t nrec = wb.size() / LNW_WIN_REC;
    std::vector<float> wf(nrec * 52, 0.0f);
    for (size_t r = 0; r < nrec; r++)
      for (int j = 0; j < 49; j++) wf[r * 52 + j] = (float)((double)wb[r * LNW_WIN_REC + j] / 255.0);
    HIPCHK(hipMemcpy(h->d_winf, wf.data(), wf.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy((char *)h->d_winf + (size_t)win_bytes_at(G) * 16, wb.data(), wb.size(), hipMemcpyHostToDevice));
  }
  KParams &k = h->kp;
  k.G = G;
  k.W16 = h->W16;
  int n = G * h->W16;
  build_mask_kernel<<<(n + 255) / 256, 256>>>(h->d_grid, G, h->W16, k.move_thr, k.ew_thr, h->d_mask2);
  HIPCHK(hipGetLastError());
  long long nm = (long long)MV_CLASSES * G * G * MV_W * MV_W;
  build_move_table_kernel<<<(unsigned)((nm + WAVE - 1) / WAVE), WAVE>>>(h->d_mask2, G, h->W16, h->d_mvtab);
  HIPCHK(hipGetLastError());
  long long nl = (long long)G * G * LOS_W;
  const int mwords = G * h->W16 * 4 <= 64 * 1024 ? G * h->W16 : 0;  // terrain mask staged in LDS
  {  // a few resident rounds of workgroups, each looping over its items
    const long long need = (nl + 255) / 256, cap = (long long)device_ncu(h->device) * 8;
    build_los_table_kernel<<<(unsigned)(need < cap ? need : cap), 256, (size_t)mwords * 4>>>(
        h->d_mask2, G, h->W16, h->d_lostab, mwords);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  h->terrain = true;
  // dynamic LDS above the 64 KiB default needs an explicit opt-in
  {
    // the largest step launch (64 / nb envs per workgroup: the biggest row stages)
    const size_t need = step_launch_lds_bytes(h, WAVE / h->nb);
    // the same bound the launch attribute below grants
    if (need > (size_t)GROUP_LDS_MAX) return fail(LNW_EUNSUPPORTED, "agent count needs more LDS than a CU has");
    // the group kernel's LDS, fixed from here on (plan_step reads it)
    h->group_lds = group_lds(lds_layout(h->A, h->nb, h->nr, h->nmax, h->G * h->W16, h->G), h->G * h->W16, h->A,
                             h->nb * h->nr, h->kp.atan_odd != 0);
    const size_t gneed = (size_t)h->group_lds.total + 1024;
    // (else runtime sizes stay on step_kernel<0, 0>)
    h->group_fits = h->group_lds.ms >= 0;
    // the limit is per kernel function and device, shared by every handle of
    // the process on that device: set to GROUP_LDS_MAX once per device, so a
    // smaller handle never lowers it under a larger one's launch (the launch's
    // own size sets the occupancy); hipSetDevice(h->device) above selects it
    static unsigned long long lds_opt_in = 0;  // bit d: device d done
    const unsigned long long dbit = 1ull << (h->device & 63);
    const size_t uneed = (size_t)UNITS * ((step_lds_bytes(h) + 15) & ~(size_t)15);
    h->units_fit = uneed <= (size_t)UNITS_LDS_MAX;
    if (!(lds_opt_in & dbit) && (need > 64 * 1024 || gneed > 64 * 1024 || uneed > 64 * 1024)) {
      for (const auto &row : STEP_KERNELS)
        HIPCHK(hipFuncSetAttribute((const void *)row.fn, hipFuncAttributeMaxDynamicSharedMemorySize, row.lds_cap));
      for (const auto &row : OBS_KERNELS)
        HIPCHK(hipFuncSetAttribute((const void *)row.fn, hipFuncAttributeMaxDynamicSharedMemorySize, row.lds_cap));
      lds_opt_in |= dbit;
    }
  }
  (void)hipGetLastError();
  h->kp.epw = choose_epw(h);
  return 0;
}

int lnw_set_rng(lnw_handle *h, int32_t mode, uint64_t seed, const double *tape_dev,
                const int64_t *tape_off_dev) {
  if (!h) return fail(LNW_EINVAL, "null handle");
  if (mode != LNW_RNG_PHILOX && mode != LNW_RNG_TAPE) return fail(LNW_EINVAL, "bad rng mode");
  if (mode == LNW_RNG_TAPE && (!tape_dev || !tape_off_dev))
    return fail(LNW_EINVAL, "tape mode needs tape and offsets");
  HIPCHK(hipSetDevice(h->device));
  h->kp.rng_mode = mode;
  h->kp.seed = seed;
  h->tape = tape_dev;
  h->tape_off = (const long long *)tape_off_dev;
  HIPCHK(hipMemset(h->rng, 0, sizeof(unsigned long long) * h->E));
  return cold_commit(h, nullptr);
}

// Validate a spawn spec's ship types (blue then red) and derive what the
// kernels key on: each side's window cells (wc) and whether the runtime-size
// kernels must run (has_medium). Shared by lnw_reset and lnw_set_state, so a
// snapshot restored into any handle selects the same kernels and row lengths
// as the handle it was taken from. apply = false only validates.
static int apply_side_types(lnw_handle *h, const int32_t *types, bool apply) {
  int nmed[2] = {0, 0};
  for (int a = 0; a < h->A; a++) {
    const int t = types[a];
    if (t != LNW_SMALL && t != LNW_LARGE && t != LNW_LS && t != LNW_MEDIUM)
      return fail(LNW_EUNSUPPORTED, "ship type must be small, large, ls or medium");
    if (t == LNW_MEDIUM) nmed[a >= h->nb]++;
    if (h->params.discrete && t == LNW_LS)
      return fail(LNW_EUNSUPPORTED, "LandingShip has no value_to_coordinates (DISCRETE mode)");
  }
  // a side's row length follows its fastest ship (game.py:595-610), and a
  // medium ship's get_obs row has a 5x5 window (combatant.py:165-181): a side
  // of medium ships only has 4 n + 28-float rows; medium ships beside speed-3
  // ships make the reference's row assignment raise (game.py:344, 381)
  for (int sd = 0; sd < 2; sd++) {
    const int ns = sd ? h->nr : h->nb;
    if (nmed[sd] && nmed[sd] != ns)
      return fail(LNW_EUNSUPPORTED, "medium ships need a side of medium ships only (the reference's "
                                    "rows are sized by the fastest ship, game.py:595-610)");
  }
  if (apply) {
    h->kp.wc[0] = nmed[0] ? 25 : 49;
    h->kp.wc[1] = nmed[1] ? 25 : 49;
    h->has_medium = nmed[0] || nmed[1];
  }
  return 0;
}

int lnw_reset(lnw_handle *h, const uint8_t *env_mask_dev, const lnw_spawn *spawn,
              const int32_t *pos_dev, void *stream) {
  if (!h || !spawn) return fail(LNW_EINVAL, "null argument");
  if (!h->terrain) return fail(LNW_ESTATE, "lnw_load_terrain must be called first");
  HIPCHK(hipSetDevice(h->device));
  if (int rc = apply_side_types(h, spawn->types, false)) return rc;
  for (int a = 0; a < h->A; a++)
    if (!spawn->rand_ls[a] && (spawn->pos[a][0] < 0 || spawn->pos[a][0] >= h->G ||
                               spawn->pos[a][1] < 0 || spawn->pos[a][1] >= h->G))
      return fail(LNW_EINVAL, "spawn position outside the grid");
  apply_side_types(h, spawn->types, true);
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemcpy(h->sp_types, spawn->types, sizeof(int32_t) * h->A, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->sp_pos, spawn->pos, sizeof(int32_t) * 2 * h->A, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->sp_randls, spawn->rand_ls, sizeof(int32_t) * h->A, hipMemcpyHostToDevice));
  h->kp.box_lo[0] = spawn->box_lo[0]; h->kp.box_lo[1] = spawn->box_lo[1];
  h->kp.box_hi[0] = spawn->box_hi[0]; h->kp.box_hi[1] = spawn->box_hi[1];
  // per-env spawn cells: kept in the handle for the in-kernel auto-reset
  if (pos_dev) {
    const size_t n = (size_t)h->E * h->A * 2;
    if (!h->sp_pos_env && dalloc(h, &h->sp_pos_env, n)) return LNW_ENOMEM;
    HIPCHK(hipMemcpyAsync(h->sp_pos_env, pos_dev, n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  }
  h->sp_pos_env_on = pos_dev != nullptr;
  KState s;
  if (int rc = launch_state(h, s)) return rc;
  reset_kernel<<<(h->E + 255) / 256, 256, 0, st>>>(h->kp, s, env_mask_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

// One step launch (lnw_step_seq makes one per step)
int lnw_step(lnw_handle *h, void *actions_dev, int32_t action_dtype, const uint8_t *row_kind_dev,
             float *obs_blue_dev, float *obs_red_dev, float *rew_blue_dev, float *rew_red_dev,
             int32_t *done_dev, float *cog_dev, void *stream) {
  if (!h || !actions_dev) return fail(LNW_EINVAL, "null argument");
  if (!h->terrain) return fail(LNW_ESTATE, "lnw_load_terrain must be called first");
  if (action_dtype != LNW_ACT_F32 && action_dtype != LNW_ACT_F64 && action_dtype != LNW_ACT_I32)
    return fail(LNW_EINVAL, "bad action dtype");
  if (action_dtype == LNW_ACT_I32 && !h->params.discrete)
    return fail(LNW_EINVAL, "integer actions go with DISCRETE mode only");
  if (action_dtype == LNW_ACT_F32 && h->params.discrete)
    return fail(LNW_EINVAL, "DISCRETE mode takes int32 (ndarray) or float64 (list rows) actions");
  if ((obs_blue_dev == nullptr) != (obs_red_dev == nullptr))
    return fail(LNW_EINVAL, "observation outputs: both or neither");
  KParams k = h->kp;
  k.act_dtype = action_dtype;
  k.no_obs = obs_blue_dev == nullptr ? 1 : 0;
  k.dbg_skip = h->knobs.dbg_skip;
  k.store_wt = h->store_wt;
  KState s;
  if (int rc = launch_state(h, s)) return rc;
  const StepPlan p = plan_step(h, k.epw, k.no_obs != 0, action_dtype, row_kind_dev != nullptr);
  k.qdirect = p.qdirect ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (h->knobs.prof) {
    const size_t slots = (size_t)p.nwg * PROF_SLOTS;
    if (slots > h->prof_cap) {
      HIPCHK(hipStreamSynchronize(st));
      if (h->d_prof) { (void)hipFree(h->d_prof); h->d_prof = nullptr; h->prof_cap = 0; }
      HIPCHK(hipMalloc(&h->d_prof, slots * sizeof(unsigned long long)));
      h->prof_cap = slots;
    }
    HIPCHK(hipMemsetAsync(h->d_prof, 0, slots * sizeof(unsigned long long), st));
    s.prof = h->d_prof;
    if (p.row->code == LNW_KERNEL_GROUP) {
      const GroupLds &gl = h->group_lds;
      fprintf(stderr, "[lnw prof] group kernel LDS %zu B (staged: target lists %d, dist_lz %d, bearing half table %d, pooled slopes %d)\n",
              p.lds, (int)(gl.tls >= 0), (int)(gl.dlz >= 0), (int)(gl.atab >= 0), (int)(gl.ms >= 0));
    }
  }
  h->last_kernel = p.row->code;
  h->last_prod = p.row == &STEP_KERNELS[SK_UNITS_PROD];
  p.row->fn<<<dim3(p.grid), dim3(p.block), p.lds, st>>>(k, s, actions_dev, row_kind_dev, obs_blue_dev, obs_red_dev,
                                                         rew_blue_dev, rew_red_dev, done_dev, cog_dev);
  HIPCHK(hipGetLastError());
  if (s.prof) prof_report(h->d_prof, st, (int)p.nwg);
  return 0;
}

int lnw_step_seq(lnw_handle *h, const lnw_seq *seq, void *actions_dev, int32_t action_dtype,
                 const uint8_t *row_kind_dev, float *obs_blue_dev, float *obs_red_dev, float *rew_blue_dev,
                 float *rew_red_dev, int32_t *done_dev, float *cog_dev, void *stream) {
  if (!h || !seq) return fail(LNW_EINVAL, "null argument");
  if (seq->steps < 1) return fail(LNW_EINVAL, "seq->steps must be >= 1");
  if (seq->act_step < 0 || seq->kind_step < 0 || seq->obs_blue_step < 0 || seq->obs_red_step < 0 ||
      seq->rew_blue_step < 0 || seq->rew_red_step < 0 || seq->done_step < 0 || seq->cog_step < 0)
    return fail(LNW_EINVAL, "negative step stride");
  // K launches back to back on the caller's stream. (Round 5 measured one launch
  // in which each workgroup ran its envs through the K steps: parity with K
  // launches at best, DESIGN.md "Action sequences in one call"; removed.)
  const long long asz = action_dtype == LNW_ACT_F64 ? 8 : 4, rsz = h->kp.rew_f64 ? 8 : 4;
  for (int k = 0; k < seq->steps; k++) {
    auto adv = [&](const void *p, long long stride, long long sz) {
      return p ? (void *)((char *)p + (long long)k * stride * sz) : nullptr;
    };
    if (int e = lnw_step(h, adv(actions_dev, seq->act_step, asz), action_dtype,
                         (const uint8_t *)adv(row_kind_dev, seq->kind_step, 1),
                         (float *)adv(obs_blue_dev, seq->obs_blue_step, 4),
                         (float *)adv(obs_red_dev, seq->obs_red_step, 4),
                         (float *)adv(rew_blue_dev, seq->rew_blue_step, rsz),
                         (float *)adv(rew_red_dev, seq->rew_red_step, rsz),
                         (int32_t *)adv(done_dev, seq->done_step, 4), (float *)adv(cog_dev, seq->cog_step, rsz),
                         stream))
      return e;
  }
  return 0;
}

int lnw_observe(lnw_handle *h, int32_t agent, float *obs_blue_dev, float *obs_red_dev, void *stream) {
  return lnw_observe_ex(h, agent, obs_blue_dev, 0, obs_red_dev, 0, stream);
}

int lnw_observe_ex(lnw_handle *h, int32_t agent, float *obs_blue_dev, int64_t blue_env_stride,
                   float *obs_red_dev, int64_t red_env_stride, void *stream) {
  if (!h) return fail(LNW_EINVAL, "null handle");
  if (!h->terrain) return fail(LNW_ESTATE, "lnw_load_terrain must be called first");
  if (agent >= h->A || agent < LNW_OBS_RED) return fail(LNW_EINVAL, "bad agent selector");
  const int64_t row_b = (int64_t)h->nb * side_D(h->kp, 0), row_r = (int64_t)h->nr * side_D(h->kp, 1);
  if (blue_env_stride < 0 || red_env_stride < 0 || (blue_env_stride && (blue_env_stride < row_b || blue_env_stride % 4)) ||
      (red_env_stride && (red_env_stride < row_r || red_env_stride % 4)))
    return fail(LNW_EINVAL, "env stride: 0, or a multiple of 4 floats of at least the side's n * D");
  if (((uintptr_t)obs_blue_dev | (uintptr_t)obs_red_dev) & 15) return fail(LNW_EINVAL, "rows must be 16-B aligned");
  KState s;
  if (int rc = launch_state(h, s)) return rc;
  const ObsPlan p = plan_observe(h);
  KParams k = h->kp;
  k.obs_stride[0] = blue_env_stride;
  k.obs_stride[1] = red_env_stride;
  p.row->fn<<<dim3(p.grid), dim3(p.block), p.lds, (hipStream_t)stream>>>(k, s, agent, obs_blue_dev, obs_red_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int lnw_state_field(lnw_handle *h, int32_t field, void **dev_ptr, int64_t *nbytes) {
  if (!h || !dev_ptr || !nbytes) return fail(LNW_EINVAL, "null argument");
  const int64_t E = h->E, A = h->A;
  switch (field) {
    case LNW_F_POS: *dev_ptr = h->pos; *nbytes = 4 * A * E; break;
    case LNW_F_RADAR: *dev_ptr = h->radar; *nbytes = 4 * A * E; break;
    case LNW_F_MISSILES: *dev_ptr = h->miss; *nbytes = A * E; break;
    case LNW_F_MKIND: *dev_ptr = h->mkind; *nbytes = A * E; break;
    case LNW_F_ALIVE: *dev_ptr = h->alive; *nbytes = A * E; break;
    case LNW_F_TYPE: *dev_ptr = h->type; *nbytes = A * E; break;
    case LNW_F_STEPS: *dev_ptr = h->steps; *nbytes = 4 * A * E; break;
    case LNW_F_DIST_LZ: *dev_ptr = h->dist_lz; *nbytes = 8 * A * E; break;
    case LNW_F_TL_CNT: *dev_ptr = h->tl_cnt; *nbytes = 2 * A * E; break;
    case LNW_F_TL: *dev_ptr = h->tl; *nbytes = 2 * A * h->T * E; break;
    case LNW_F_DUCT: *dev_ptr = h->duct; *nbytes = 8 * E; break;
    case LNW_F_ENV: *dev_ptr = h->envi; *nbytes = 4 * 8 * E; break;
    case LNW_F_RNG: *dev_ptr = h->rng; *nbytes = 8 * E; break;
    case LNW_F_ERR: *dev_ptr = h->err; *nbytes = 4 * E; break;
    default: return fail(LNW_EINVAL, "unknown state field");
  }
  return 0;
}

int lnw_tlist_cap(lnw_handle *h) { return h ? h->T : LNW_EINVAL; }

int lnw_step_kernel(lnw_handle *h) { return h ? h->last_kernel : LNW_EINVAL; }

int lnw_step_kernel_prod(lnw_handle *h) { return h ? (h->last_prod ? 1 : 0) : LNW_EINVAL; }

// ---- whole-state snapshots (lnw_state_bytes / lnw_get_state / lnw_set_state)
// Snapshot layout: a 128-byte header (below), then the LNW_NFIELDS state
// fields in field order, then the spawn spec the in-kernel auto-reset reads
// (types, cells, randint flags: 64 x i32, 64 x 2 x i32, 64 x i32) and the
// per-env spawn cells ([E][A][2] i32, zeros when the last reset had none);
// every section starts on a 256-byte boundary.
namespace {
struct StateHeader {
  char magic[8];            // "LNWSTATE"
  uint32_t version;         // 1
  int32_t E, nb, nr, T, G;
  int32_t rng_mode;         // LNW_RNG_*
  int32_t pos_env_on;       // the auto-reset respawns on per-env cells
  uint64_t seed;
  uint64_t terrain_hash;    // FNV-1a of the grid loaded when the snapshot was taken
  int64_t total;            // snapshot bytes
  int32_t box_lo[2], box_hi[2];
  int32_t abi;              // LNW_ABI_VERSION
  uint8_t pad[128 - 8 - 4 - 7 * 4 - 3 * 8 - 4 * 4 - 4];
};
static_assert(sizeof(StateHeader) == 128, "state header is 128 bytes");

struct Section { void *dev; int64_t bytes; };

int state_sections(lnw_handle *h, std::vector<Section> &out) {
  out.clear();
  for (int f = 0; f < LNW_NFIELDS; f++) {
    void *p = nullptr;
    int64_t n = 0;
    if (int rc = lnw_state_field(h, f, &p, &n)) return rc;
    out.push_back({p, n});
  }
  out.push_back({h->sp_types, 64 * 4});
  out.push_back({h->sp_pos, 128 * 4});
  out.push_back({h->sp_randls, 64 * 4});
  out.push_back({h->sp_pos_env, (int64_t)h->E * h->A * 2 * 4});  // (may not be allocated yet)
  return 0;
}

inline int64_t sec_align(int64_t v) { return (v + 255) & ~(int64_t)255; }
}  // namespace

int64_t lnw_state_bytes(lnw_handle *h) {
  if (!h) return fail(LNW_EINVAL, "null handle");
  std::vector<Section> s;
  if (int rc = state_sections(h, s)) return rc;
  int64_t o = 256;
  for (const Section &x : s) o += sec_align(x.bytes);
  return o;
}

int lnw_get_state(lnw_handle *h, void *dst, int64_t nbytes, void *stream) {
  if (!h || !dst) return fail(LNW_EINVAL, "null argument");
  if (!h->terrain) return fail(LNW_ESTATE, "lnw_load_terrain must be called first");
  const int64_t total = lnw_state_bytes(h);
  if (nbytes < total) return fail(LNW_EINVAL, "snapshot buffer smaller than lnw_state_bytes()");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  StateHeader hd;
  memset(&hd, 0, sizeof hd);
  memcpy(hd.magic, "LNWSTATE", 8);
  hd.version = 1;
  hd.E = h->E; hd.nb = h->nb; hd.nr = h->nr; hd.T = h->T; hd.G = h->G;
  hd.rng_mode = h->kp.rng_mode;
  hd.pos_env_on = h->sp_pos_env_on ? 1 : 0;
  hd.seed = h->kp.seed;
  hd.terrain_hash = h->terrain_hash;
  hd.total = total;
  for (int i = 0; i < 2; i++) { hd.box_lo[i] = h->kp.box_lo[i]; hd.box_hi[i] = h->kp.box_hi[i]; }
  hd.abi = LNW_ABI_VERSION;
  std::vector<Section> s;
  if (int rc = state_sections(h, s)) return rc;
  char *d = (char *)dst;
  char hbuf[256] = {0};
  memcpy(hbuf, &hd, sizeof hd);
  HIPCHK(hipMemcpy(d, hbuf, sizeof hbuf, hipMemcpyDefault));
  int64_t o = 256;
  for (const Section &x : s) {
    if (x.dev) {
      HIPCHK(hipMemcpy(d + o, x.dev, (size_t)x.bytes, hipMemcpyDefault));
    } else {  // per-env spawn cells never given: zeros (host or device destination)
      const std::vector<char> z((size_t)x.bytes, 0);
      HIPCHK(hipMemcpy(d + o, z.data(), (size_t)x.bytes, hipMemcpyDefault));
    }
    o += sec_align(x.bytes);
  }
  return 0;
}

int lnw_set_state(lnw_handle *h, const void *src, int64_t nbytes, void *stream) {
  if (!h || !src) return fail(LNW_EINVAL, "null argument");
  if (!h->terrain) return fail(LNW_ESTATE, "lnw_load_terrain must be called first");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  if (nbytes < (int64_t)sizeof(StateHeader)) return fail(LNW_EINVAL, "snapshot too short");
  StateHeader hd;
  HIPCHK(hipMemcpy(&hd, src, sizeof hd, hipMemcpyDefault));
  if (memcmp(hd.magic, "LNWSTATE", 8) != 0 || hd.version != 1)
    return fail(LNW_EINVAL, "not an lnw state snapshot (bad magic or version)");
  if (hd.abi != LNW_ABI_VERSION)
    return fail(LNW_EINVAL, "snapshot was taken by a library of another ABI version");
  const int64_t total = lnw_state_bytes(h);
  if (hd.E != h->E || hd.nb != h->nb || hd.nr != h->nr || hd.T != h->T || hd.G != h->G || hd.total != total)
    return fail(LNW_EINVAL, "snapshot shape (envs, team sizes, grid) differs from this handle");
  if (hd.terrain_hash != h->terrain_hash) return fail(LNW_EINVAL, "snapshot was taken on another terrain");
  if (nbytes < total) return fail(LNW_EINVAL, "snapshot shorter than its header says");
  if (hd.rng_mode == LNW_RNG_TAPE && (!h->tape || !h->tape_off))
    return fail(LNW_ESTATE, "snapshot is in tape mode: bind the tape (lnw_set_rng) before restoring");
  if (hd.pos_env_on && !h->sp_pos_env && dalloc(h, &h->sp_pos_env, (size_t)h->E * h->A * 2)) return LNW_ENOMEM;
  std::vector<Section> s;
  if (int rc = state_sections(h, s)) return rc;
  const char *p = (const char *)src;
  // the spawn types decide the kernels and the row lengths (wc, has_medium):
  // validate them before anything is overwritten, apply them after
  int32_t types[64];
  {
    int64_t ot = 256;
    for (int i = 0; i < LNW_NFIELDS; i++) ot += sec_align(s[i].bytes);
    HIPCHK(hipMemcpy(types, p + ot, sizeof types, hipMemcpyDefault));
    if (int rc = apply_side_types(h, types, false)) return rc;
  }
  int64_t o = 256;
  for (const Section &x : s) {
    if (x.dev) HIPCHK(hipMemcpy(x.dev, p + o, (size_t)x.bytes, hipMemcpyDefault));
    o += sec_align(x.bytes);
  }
  apply_side_types(h, types, true);
  h->kp.rng_mode = hd.rng_mode;
  if (hd.rng_mode == LNW_RNG_PHILOX) h->kp.seed = hd.seed;
  for (int i = 0; i < 2; i++) { h->kp.box_lo[i] = hd.box_lo[i]; h->kp.box_hi[i] = hd.box_hi[i]; }
  h->sp_pos_env_on = hd.pos_env_on != 0;
  return cold_commit(h, nullptr);
}

int lnw_set_counters(lnw_handle *h, uint64_t *counters_dev) {
  if (!h) return fail(LNW_EINVAL, "null handle");
  h->ctr = (unsigned long long *)counters_dev;
  return cold_commit(h, nullptr);
}

int lnw_set_reward_dtype(lnw_handle *h, int32_t f64) {
  if (!h) return fail(LNW_EINVAL, "null handle");
  h->kp.rew_f64 = f64 != 0;
  return 0;
}

int lnw_set_variant(lnw_handle *h, int32_t contact) {
  if (!h) return fail(LNW_EINVAL, "null handle");
  h->contact = contact != 0;
  return 0;
}

int lnw_set_epw(lnw_handle *h, int32_t epw) {
  if (!h) return fail(LNW_EINVAL, "null handle");
  if (epw < 0 || epw > EPW) return fail(LNW_EINVAL, "epw must be 0 (automatic) or 1..64");
  if (!h->terrain) return fail(LNW_ESTATE, "lnw_load_terrain must be called first");
  h->kp.epw = epw ? epw : choose_epw(h);
  return h->kp.epw;
}

int lnw_los_batch(const uint8_t *grid_dev, int32_t G, const int16_t *pairs_dev, int64_t n,
                  int32_t move_thr, int32_t ew_thr, uint8_t *out_dev, void *stream) {
  if (!grid_dev || !pairs_dev || !out_dev) return fail(LNW_EINVAL, "null argument");
  if (n <= 0) return 0;
  const size_t lds = (size_t)G * ((G + 15) / 16) * 4;
  if (lds <= 64 * 1024 && ((uintptr_t)pairs_dev & 7) == 0) {  // (the LDS kernel reads a pair as 8 bytes)
    const long long per_block = (long long)(LB_THREADS / WAVE) * LB_RAYS_PER_WAVE;
    los_batch_kernel<<<(unsigned)((n + per_block - 1) / per_block), LB_THREADS, lds, (hipStream_t)stream>>>(
        grid_dev, G, pairs_dev, n, move_thr, ew_thr, out_dev);
  } else {
    los_batch_global_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        grid_dev, G, pairs_dev, n, move_thr, ew_thr, out_dev);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int lnw_astar_batch(const uint8_t *grid_dev, int32_t G, int32_t move_thr, const int8_t *types_dev,
                    const int16_t *start_dev, const int16_t *target_dev, int64_t n,
                    int16_t *plen_dev, int8_t *kind_dev, uint8_t *feasible_dev, void *stream) {
  if (!grid_dev || !types_dev || !start_dev || !target_dev || !plen_dev || !kind_dev || !feasible_dev)
    return fail(LNW_EINVAL, "null argument");
  if (n <= 0) return 0;
  astar_batch_kernel<<<(unsigned)((n + WAVE - 1) / WAVE), WAVE, 0, (hipStream_t)stream>>>(
      grid_dev, G, move_thr, types_dev, start_dev, target_dev, n, plen_dev, kind_dev, feasible_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int lnw_move_batch(lnw_handle *h, const int8_t *types_dev, const int16_t *pos_dev,
                   const double *act_dev, const uint8_t *is_f32_dev, int64_t n, int32_t *rounded_dev,
                   uint8_t *ok_dev, void *stream) {
  if (!h || !types_dev || !pos_dev || !act_dev || !is_f32_dev || !rounded_dev || !ok_dev)
    return fail(LNW_EINVAL, "null argument");
  if (!h->terrain) return fail(LNW_ESTATE, "lnw_load_terrain must be called first");
  if (n <= 0) return 0;
  KState s;
  if (int rc = launch_state(h, s)) return rc;
  move_batch_kernel<<<(unsigned)((n + WAVE - 1) / WAVE), WAVE, 0, (hipStream_t)stream>>>(
      h->kp, s, types_dev, pos_dev, act_dev, is_f32_dev, n, rounded_dev, ok_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int lnw_path_query(lnw_handle *h, const int8_t *types_dev, const int16_t *start_dev,
                   const int16_t *target_dev, int64_t n, uint8_t *out_dev, void *stream) {
  if (!h || !types_dev || !start_dev || !target_dev || !out_dev) return fail(LNW_EINVAL, "null argument");
  if (!h->terrain) return fail(LNW_ESTATE, "lnw_load_terrain must be called first");
  if (n <= 0) return 0;
  KState s;
  if (int rc = launch_state(h, s)) return rc;
  path_query_kernel<<<(unsigned)((n + WAVE - 1) / WAVE), WAVE, 0, (hipStream_t)stream>>>(
      h->kp, s, types_dev, start_dev, target_dev, n, out_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int lnw_los_query(lnw_handle *h, const int16_t *pairs_dev, int64_t n, uint8_t *out_dev, void *stream) {
  if (!h || !pairs_dev || !out_dev) return fail(LNW_EINVAL, "null argument");
  if (!h->terrain) return fail(LNW_ESTATE, "lnw_load_terrain must be called first");
  if (n <= 0) return 0;
  KState s;
  if (int rc = launch_state(h, s)) return rc;
  los_query_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(h->kp, s, pairs_dev, n, out_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int lnw_copy(void *dst, const void *src, int64_t nbytes, void *stream) {
  if (nbytes <= 0) return 0;
  if (!dst || !src) return fail(LNW_EINVAL, "null argument");
  HIPCHK(hipMemcpyAsync(dst, src, (size_t)nbytes, hipMemcpyDefault, (hipStream_t)stream));
  return 0;
}

int lnw_fill_uniform_f32(float *out_dev, int64_t n, uint64_t seed, uint64_t offset, void *stream) {
  if (!out_dev) return fail(LNW_EINVAL, "null argument");
  if (n <= 0) return 0;
  if (offset & 3) return fail(LNW_EINVAL, "offset must be a multiple of 4");
  long long nt = (n + 3) / 4;
  fill_uniform_kernel<<<(unsigned)((nt + 255) / 256), 256, 0, (hipStream_t)stream>>>(out_dev, n, seed, offset);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
