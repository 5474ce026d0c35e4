// lnw_group.inc — the group kernel: runtime team sizes (config 4's 8 blue vs
// 8 + 2 landing ships, and any size outside 2v2..4v4) with GL lanes per
// environment. Included by lnw_kernels.hip inside its anonymous namespace,
// after step_kernel (uses Cols, Ctx, move_phase, fire_dev, reward_dev,
// env_tail from there).
//
// One lane per env (step_kernel<0, 0>) leaves config 4's 8 192 envs as 256
// half-full single-wave workgroups on 1 024 SIMDs, each lane walking 80 (own,
// opponent) pairs per get_obs in series. Here an env owns a group of GL = 16
// lanes of a wave (4 envs per wave, GEPW = 32 envs = 8 waves per workgroup):
//   L, M  the state load and phase M's (env, agent) pairs spread over all the
//         workgroup's lanes;
//   S     first each lane of a group evaluates, for one opponent of each
//         side, every pair condition get_obs can ask for during the step
//         (group_pair_tables: ranges and LOS for both cells of every own ship,
//         in registers); then every lane of the group runs its env's sequential
//         agent loop (take_action, reward, tail: identical values and identical
//         stores; only the group's first lane makes the analytics side effects),
//         except get_obs (get_obs_group): the walk over the pair tables by
//         ballots, then one lane per opponent evaluates that opponent's EW
//         bearings, fix and fix targets;
//   O     each group writes its env's observation rows from the LDS state, four
//         floats per lane per store (group_rows).
// Results are bit-identical to step_kernel<0, 0> (tests/test_gpu_group.py).

// Section timers of the diagnostics build (-DLNW_GROUP_PROF, tools/gpu/sections.sh):
// per-lane sums in registers, one atomic per wave at the end of phase S into
// the LNW_PROF record slots 16..23 (take_action, reward, tail, pair
// tables, get_obs column bits, walk, bearings + fixes, target list).
#ifdef LNW_GROUP_PROF
#define GPROF_MARK(t) unsigned long long t = __builtin_amdgcn_s_memrealtime()
#define GPROF_SET(t) (t) = __builtin_amdgcn_s_memrealtime()
#define GPROF_ADD(X, k, t)                                                   \
  do {                                                                       \
    const unsigned long long _n = __builtin_amdgcn_s_memrealtime();          \
    (X).gp[k] += _n - (t);                                                   \
    (t) = _n;                                                                \
  } while (0)
#define GPROF_FLUSH(X)                                                       \
  do {                                                                       \
    if ((X).S.prof && (threadIdx.x & (WAVE - 1)) == 0)                        \
      for (int _k = 0; _k < 8; _k++)                                         \
        atomicAdd(&(X).S.prof[(size_t)blockIdx.x * PROF_SLOTS + 16 + _k], (X).gp[_k]); \
  } while (0)
#else
#define GPROF_MARK(t) (void)0
#define GPROF_SET(t) (void)0
#define GPROF_ADD(X, k, t) (void)0
#define GPROF_FLUSH(X) (void)0
#endif

constexpr int GL = 16;           // lanes per environment
constexpr int GEPW = 32;         // environments per workgroup (GEPW * GL threads)
constexpr int GNW = GEPW * GL / WAVE;  // waves per workgroup
constexpr int GROUP_LDS_MAX = 158 * 1024;  // dynamic LDS: the CU's 160 KiB less the kernels' static LDS
constexpr int GTL = 16;          // target-list entries per agent staged in LDS (one chunk of the fire loop)
constexpr int ATAN_HALF_BYTES = (R_LOS + 1) * LOS_W * 8;

// Dynamic LDS of the group kernel: the step layout (lds_layout) up to the end of
// the terrain mask — the quiet-path stages, emission stage and x/G table past it
// are never used here —, then (in this order):
//   tls  then, each only if it fits, the first GTL entries of every agent's target list [A][GTL][GEPW]
//        u16, staged in phase L, so take_action's reads never wait (in issue
//        order) behind the target-list stores earlier get_obs calls issued;
//   dlz  the landing ships' dist_lz [A][GEPW] f64, for calculate_reward alike;
//   atab the dy >= 0 half of the bearing-angle table (degrees(atan2), host libm,
//        KState.atan_deg; odd in dy, checked by the host: KParams.atan_odd).
//   ms   (first) the EW bearing slopes of one get_obs call by pair [nb * nr][GEPW]
//        f64, where the lanes that evaluate them (pooled over the group) leave
//        them for the opponent lanes that fix;
// (config 4: 85.5 KB + 18.4 + 4.6 + 26.6 + 20.5 = 156 KB)
struct GroupLds {
  int tls = -1, dlz = -1, atab = -1, ms = -1, total = 0;
};
// (ms is required: without it the runtime sizes stay on step_kernel<0, 0>)
__host__ __device__ inline GroupLds group_lds(const LdsLayout &L, int mask_words, int A, int npair, bool atan_odd) {
  GroupLds g;
  int o = (L.mask + mask_words * 4 + 15) & ~15;
  if (o + GEPW * npair * 8 <= GROUP_LDS_MAX) { g.ms = o; o += GEPW * npair * 8; }
  if (o + A * GTL * GEPW * 2 <= GROUP_LDS_MAX) { g.tls = o; o = (o + A * GTL * GEPW * 2 + 15) & ~15; }
  if (o + A * GEPW * 8 <= GROUP_LDS_MAX) { g.dlz = o; o += A * GEPW * 8; }
  if (atan_odd && o + ATAN_HALF_BYTES <= GROUP_LDS_MAX) { g.atab = o; o += ATAN_HALF_BYTES; }
  g.total = o;
  return g;
}
__host__ __device__ inline int group_base(const LdsLayout &L, int mask_words) { return L.mask + mask_words * 4; }

// math.degrees(math.atan2(dy, dx)) (combatant.py:253) in the +-R_LOS window:
// from the LDS half table (rows dy >= 0, negated for dy < 0) or the HBM table;
// the device atan2 outside it
__device__ __forceinline__ double bearing_tab(const KParams &P, const double *atab, bool half, int dx, int dy) {
  const bool tab = !(P.dbg_skip & 4096) && dx >= -R_LOS && dx <= R_LOS && dy >= -R_LOS && dy <= R_LOS;
  if (!tab) return atan2((double)dy, (double)dx) * RAD2DEG;
  if (!half) return atab[(dy + R_LOS) * LOS_W + (dx + R_LOS)];
  const double v = atab[(dy < 0 ? -dy : dy) * LOS_W + (dx + R_LOS)];
  return dy < 0 ? -v : v;
}

// OR of v over the GL lanes of this lane's group (aligned lanes of one wave)
__device__ __forceinline__ uint32_t group_or(uint32_t v) {
#pragma unroll
  for (int o = GL / 2; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o);
  return v;
}

// np.mean of m < 16 fix points in numpy's order: a plain left-to-right sum
// below 8 terms; from 8 on (pairwise summation, one 8-wide block) the first 8
// points as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the rest added in order.
// Points arrive in order, so the tree forms when point 8 comes in.
struct FixAcc16 {
  double sx = 0, sy = 0;
  double r0x = 0, r1x = 0, r2x = 0, r3x = 0, r4x = 0, r5x = 0, r6x = 0, r7x = 0;
  double r0y = 0, r1y = 0, r2y = 0, r3y = 0, r4y = 0, r5y = 0, r6y = 0, r7y = 0;
  __device__ void add(int k, int m, double x3, double y3) {
    if (m < 8 || k >= 8) {
      if (k == 8) {
        sx = ((r0x + r1x) + (r2x + r3x)) + ((r4x + r5x) + (r6x + r7x));
        sy = ((r0y + r1y) + (r2y + r3y)) + ((r4y + r5y) + (r6y + r7y));
      }
      sx += x3;
      sy += y3;
      return;
    }
#define LNW_PUT8(i)                \
    r##i##x = k == i ? x3 : r##i##x; \
    r##i##y = k == i ? y3 : r##i##y;
    LNW_PUT8(0) LNW_PUT8(1) LNW_PUT8(2) LNW_PUT8(3) LNW_PUT8(4) LNW_PUT8(5) LNW_PUT8(6) LNW_PUT8(7)
#undef LNW_PUT8
  }
  __device__ void mean(int m, double &mx, double &my) {
    if (m == 8) {  // exactly one block: the tree alone
      sx = ((r0x + r1x) + (r2x + r3x)) + ((r4x + r5x) + (r6x + r7x));
      sy = ((r0y + r1y) + (r2y + r3y)) + ((r4y + r5y) + (r6y + r7y));
    }
    mx = sx / (double)m;
    my = sy / (double)m;
  }
};

// The pair tables of one side (GSide): everything get_obs's pair conditions
// read is fixed for the whole step except two things, which ship observes
// (its radar state) and which of its own side's ships have already taken their
// turn (their new cell). Opponents are seen at one cell per side (SURVEY §9
// Q1: blue sees red's old cells, red sees blue's final cells) with one radar
// state (red's before the step, blue's as set by take_action: rint(a0), 0 for a
// non-finite a0), hit ships stay in place until the tail (alive0) and the
// ducting is per env. So lane jj of the env's group takes opponent jj of the
// side and, for every own ship i, both cells i can stand on (v = 0 its cell at
// the start of the step, v = 1 its new cell when it moved), evaluates once per
// step: radar-detect possible (in radar range, radar LOS clear), close (d < 4,
// radar LOS clear), EW candidate (in EW range, the opponent's radar on, both
// LOS clear). Bit i of each word is the start-cell value, bit 16 + i the
// new-cell value. get_obs then selects per own ship by the turn order, in
// registers. Also per side: the opponent's cell and the mask of opponents on the
// same cell (lanes of the group).
struct GSide {
  uint32_t r = 0, c = 0, w = 0;  // radar-detect / close / EW bits [v * 16 + i]
  uint32_t mates = 0;            // lanes (opponents) sharing jj's cell, jj included
  uint32_t pos = 0xffffffffu;    // opponent jj's cell as this side sees it
  bool shared = false;           // some opponents of the side share a cell (uniform in the group)
};

// 16-lane slice of a wave ballot: lane g of this lane's group at bit g
__device__ __forceinline__ uint32_t group_ballot(bool p, int gsh) {
  return (uint32_t)(__ballot(p) >> gsh) & 0xffffu;
}

// take_action's fire loop (combatant.py:548-549 -> fire_missile, :587-668) over
// one chunk of the target list, entries q0 .. q0 + nq - 1, lane sub of the
// env's group holding entry q0 + sub (x | y << 8) in `mine`: the same results,
// draws and side effects as fire_dev<true> entry by entry, with the entries
// side by side. What ties the entries together is only the missile count (and
// its value kind): a shot needs missiles left and spends n of them, and each
// missile shot takes the next two draws. check_target reads the step's start
// cells and alive flags (hits sink ships only in the tail), so every lane
// finds its entry's target at once; the missile recurrence then runs over the
// chunk's missile shots in list order (a few integer steps each, every lane of
// the group the same), giving each shot its salvo n and its draw number; each
// lane then draws and tests its own shot. Hits are counted and flagged by
// ballots (order-free: a count and a mask). Returns the chunk's hits.
// (The analytics maps and engagement log keep fire_dev's entry-by-entry order:
// the caller uses it when they are on.)
__device__ __forceinline__ int fire_group_chunk(Ctx &X, int a, int mine, int nq, double salvo, int ksalvo,
                                                Neut &N) {
  const KParams &P = X.P;
  Cols &c = X.c;
  const int lane = X.lane;  // the env's LDS column (COLW / COLB)
  const int side = a >= P.nb;
  int t = -1;
  if (X.gsub < nq) t = check_target_dev<false>(X, side, mine & 0xff, mine >> 8);
  const uint32_t pa = COLW(c.pos_cur, a);
  const uint32_t pt = t >= 0 ? COLW(c.pos_cur, t) : pa;
  const int dx = pos_x(pt) - pos_x(pa), dy = pos_y(pt) - pos_y(pa);
  const bool gun = t >= 0 && dx * dx + dy * dy < 4;  // main gun, no draw
  uint32_t msm = group_ballot(t >= 0 && !gun, X.gsh);
  int miss = COLB(c.miss_cur, a), mk = COLB(c.mkind, a);
  int my_n = 0, my_kn = 0, my_k = -1, k = 0;
  while (msm) {  // missile shots in list order (uniform over the group)
    const int u = __builtin_ctz(msm);
    msm &= msm - 1;
    if (miss == 0) break;  // no missiles: this shot and every later one return without a draw
    int kn;
    const double num = missiles_fired(P.discrete, COLB(c.type, a), salvo, ksalvo, miss, mk, kn);
    int n = (int)num;
    miss = (miss - n) & 0xff;  // (the uint8 column)
    mk = kind_promote(mk, kn);
    if (n < 0 || n > 8) { X.rng.err |= LNW_ERRF_MISSILES; n = n < 0 ? 0 : 8; }
    if (u == X.gsub) { my_n = n; my_kn = kn; my_k = k; }
    k++;
  }
  COLB(c.miss_cur, a) = (uint8_t)miss;
  COLB(c.mkind, a) = (uint8_t)mk;
  bool hit = gun;
  if (my_k >= 0) {
    const unsigned long long c0 = X.rng.ctr + 2ull * (unsigned long long)my_k;
    const double u1 = X.rng.uniform_at(c0), u2 = X.rng.uniform_at(c0 + 1);
    const bool detected = !(u1 < (COLW(c.radar_cur, t) == 1 ? P.det_q[0] : P.det_q[1]));
    const int hp = detected ? 0 : 1;
    hit = my_kn == K_F32 ? (float)u2 < hit_sel(P.hit32, hp, my_n) : u2 < hit_sel(P.hit64, hp, my_n);
  }
  // the cursor after the chunk's 2k draws (a tape stops at its end, flagging it)
  if (X.rng.mode == 1) {
    const unsigned long long len = (unsigned long long)(X.rng.tape_hi - X.rng.tape_lo);
    const unsigned long long e = X.rng.ctr + 2ull * (unsigned long long)k;
    if (e > len) { X.rng.err |= 4u; X.rng.ctr = len > X.rng.ctr ? len : X.rng.ctr; }
    else X.rng.ctr = e;
  } else {
    X.rng.ctr += 2ull * (unsigned long long)k;
  }
  const bool tr = t >= P.nb;
  N.cnt[0] += __popc(group_ballot(hit && !tr, X.gsh));
  N.cnt[1] += __popc(group_ballot(hit && tr, X.gsh));
  N.mask[0] |= group_or(hit && !tr ? 1u << t : 0u);
  N.mask[1] |= group_or(hit && tr ? 1u << (t - P.nb) : 0u);
  return __popc(group_ballot(hit, X.gsh));
}

// The pair tables of both sides (see GSide) for lane sub of the env's group,
// and the env's moved-ship mask (bit a: agent a has a new cell). LOS words of
// four own ships (both cells each) are in flight together; pairs beyond the
// env's largest sensor reach load nothing. Out-of-window pairs (very long
// sensor ranges) and LOS march mode march the ray.
__device__ __forceinline__ void group_pair_tables(Ctx &X, int sub, GSide (&gs)[2], uint32_t &movedm) {
  const KParams &P = X.P;
  const KState &S = X.S;
  Cols &c = X.c;
  const int lane = X.lane;
  const int nb = P.nb, A = P.A;
  const double duct = X.duct();
  const int gsh = (int)(threadIdx.x & (WAVE - 1)) & ~(GL - 1);
  uint32_t mv = 0;
  for (int a = sub; a < A; a += GL) mv |= ((COLW(c.pos_new, a) & 0x80000000u) ? 1u : 0u) << a;
  movedm = group_or(mv);
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const int own0 = s ? nb : 0, nown = s ? A - nb : nb, opp0 = s ? 0 : nb, nopp = s ? nb : A - nb;
    GSide g;
    const bool mine = sub < nopp;
    const int j = opp0 + (mine ? sub : 0);
    const bool alj = mine && COLB(c.alive0, j) != 0;
    uint32_t pj = COLW(c.pos_cur, j);
    int radj = COLW(c.radar_cur, j);
    if (s) {  // blue as red sees it: after every blue turn
      const uint32_t qn = COLW(c.pos_new, j);
      if (qn & 0x80000000u) pj = qn & 0x7fffffffu;
      const double a0 = COLW(c.act0, j);
      radj = isfinite(a0) ? radar_setting(a0) : 0;
    }
    g.pos = mine ? pj : 0xffffffffu;
    {
      uint32_t m = 0;
#pragma unroll
      for (int q = 0; q < GL; q++) m |= ((uint32_t)__shfl((int)g.pos, gsh + q) == g.pos ? 1u : 0u) << q;
      g.mates = mine ? m : 0u;
      g.shared = group_or(__builtin_popcount(g.mates) > 1 ? 1u : 0u) != 0;
    }
    const int tj = COLB(c.type, j);
    if (alj) {
      for (int i0 = 0; i0 < nown; i0 += 4) {
        uint32_t wi[8], tabm = 0, marchm = 0, fl = 0;  // fl: 3 range bits per (u, v) slot q = 2u + v
#pragma unroll
        for (int u = 0; u < 4; u++) {
          wi[2 * u] = wi[2 * u + 1] = 0;
          const int i = i0 + u;
          if (i >= nown || !COLB(c.alive0, own0 + i)) continue;
          const int ti = COLB(c.type, own0 + i);
          const int rr = radar_r(P, duct, ti, tj), re = ew_r(P, duct, ti, tj);
          const uint32_t pio = COLW(c.pos_cur, own0 + i), pin = COLW(c.pos_new, own0 + i);
#pragma unroll
          for (int v = 0; v < 2; v++) {
            if (v && !(pin & 0x80000000u)) continue;
            const uint32_t pi = v ? (pin & 0x7fffffffu) : pio;
            const int dx = pos_x(pj) - pos_x(pi), dy = pos_y(pj) - pos_y(pi);
            const int d2 = dx * dx + dy * dy;
            if (d2 >= X.r2max) continue;  // beyond every radar / EW / close range
            const uint32_t f = (d2 < rr * rr ? 1u : 0u) | (d2 < 16 ? 2u : 0u) |
                               (d2 < re * re && radj == 1 ? 4u : 0u);
            if (!f) continue;  // the LOS result would be unused
            const int q = 2 * u + v;
            fl |= f << (3 * q);
            if (P.los_mode != 1 && !P.group_march && dx >= -R_LOS && dx <= R_LOS && dy >= -R_LOS &&
                dy <= R_LOS) {
              tabm |= 1u << q;
              wi[q] = ((uint32_t)(pos_x(pi) * P.G + pos_y(pi)) * LOS_CELL_WORDS + (dx + R_LOS) * LOS_ROW_WORDS) *
                          32u + (dy + R_LOS) * 2;
            } else {
              marchm |= 1u << q;
            }
          }
        }
        uint32_t lb = 0;  // 2 LOS bits (radar clear | EW clear) per slot
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const uint32_t w = (tabm >> q) & 1u ? S.lostab[wi[q] >> 5] : 0u;
          lb |= ((w >> (wi[q] & 31)) & 3u) << (2 * q);
        }
        while (marchm) {
          const int q = __builtin_ctz(marchm);
          marchm &= marchm - 1;
          const int o = own0 + i0 + (q >> 1);
          const uint32_t pi = (q & 1) ? (COLW(c.pos_new, o) & 0x7fffffffu) : COLW(c.pos_cur, o);
          lb |= los_march_c(S, X.mask, P.W16, pos_x(pi), pos_y(pi), pos_x(pj), pos_y(pj)) << (2 * q);
        }
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const uint32_t f = (fl >> (3 * q)) & 7u, l = (lb >> (2 * q)) & 3u;
          const int bit = (q & 1) * 16 + i0 + (q >> 1);
          g.r |= ((f & 1u) && (l & 1u) ? 1u : 0u) << bit;
          g.c |= ((f & 2u) && (l & 1u) ? 1u : 0u) << bit;
          g.w |= ((f & 4u) && l == 3u ? 1u : 0u) << bit;
        }
      }
    }
    gs[s] = g;
  }
}

// get_obs (combatant.py:90-161 / landingship.py:94-165) of agent `me` by the
// GL lanes of its env's group, from the pair tables (group_pair_tables): lane
// jj holds opponent jj's column of pairs (i, jj), pair number b = i * nopp + jj
// in the reference's loop order (own ships outer, opponents inner).
//   column bits: D (detects: radar on and radar-detect possible, or close) and
//   E (EW candidate) over own ships i, each from the cell i stands on now
//   (new once its turn has come and it moved);
//   the pair-order walk, as ballots over own-ship rows: the observed list
//   appends opponent jj's cell at the first detecting pair of any opponent on
//   that cell (g = min over jj's cell-mates of their first detecting pair; jj
//   represents its cell when g is its own), and pair (i, jj) yields a bearing
//   iff it is an EW candidate and b < g (the cell not yet observed); bearing k
//   of the call (pair order) takes gauss draw base + k;
//   lane jj then evaluates opponent jj's bearings (two at a time: independent
//   f64 chains) when it has at least two, the consecutive-pair fixes in own-ship
//   order (calculate_fixed_position, combatant.py:265-277), their np.mean, the
//   rounded fix and its targets (every live opponent within 2 cells,
//   combatant.py:156-161).
// The target list is the observed cells followed by the fix targets of the
// opponents in order of their first bearing.
__device__ __forceinline__ void get_obs_group(Ctx &X, int me, int sub, const GSide (&gs)[2],
                                              uint32_t movedm, const double *atab, bool half, double *ms) {
  const KParams &P = X.P;
  const KState &S = X.S;
  Cols &c = X.c;
  const int lane = X.lane;
  const long long E = X.E;
  const int env = X.env;
  const int nb = P.nb, A = P.A;
  const int side = me >= nb;
  const int own0 = side ? nb : 0, own1 = side ? A : nb;
  const int opp0 = side ? 0 : nb, opp1 = side ? nb : A;
  const int nown = own1 - own0, nopp = opp1 - opp0;
  GSide g;  // (field-wise select: a runtime index into gs would put it in scratch)
  g.r = side ? gs[1].r : gs[0].r;
  g.c = side ? gs[1].c : gs[0].c;
  g.w = side ? gs[1].w : gs[0].w;
  g.mates = side ? gs[1].mates : gs[0].mates;
  g.pos = side ? gs[1].pos : gs[0].pos;
  g.shared = side ? gs[1].shared : gs[0].shared;
  const int jj = sub;
  const uint32_t posj = g.pos;
  const int gsh = (int)(threadIdx.x & (WAVE - 1)) & ~(GL - 1);
  GPROF_MARK(tq);
  // ---- column bits: own ships that took their turn stand on their new cell
  const int ml = me - own0;
  const uint32_t vm = (movedm >> own0) & ((2u << ml) - 1u) & 0xffffu;
  auto sel = [&](uint32_t b) { return ((b & 0xffffu) & ~vm) | ((b >> 16) & vm); };
  const bool myradar = COLW(c.radar_cur, me) == 1;
  const bool nowalk = P.dbg_skip & 8192;  // diagnostics: no walk
  const uint32_t dcol = nowalk ? 0u : (sel(g.c) | (myradar ? sel(g.r) : 0u));
  const uint32_t ecol = nowalk ? 0u : sel(g.w);
  GPROF_ADD(X, 4, tq);
  // ---- the walk: first detecting row of jj's cell-mates, then bearings ------
  const int INF = 0x7fffffff;
  const int ij = dcol ? __builtin_ctz(dcol) : -1;  // first detecting row of jj's own column
  int gj = ij >= 0 ? ij * nopp + jj : INF;
  if (g.shared) {  // opponents share cells: over the rows any lane detects in, ascending
    int grow = -1, gcol = 0;
    for (uint32_t rows = group_or(dcol); rows; rows &= rows - 1) {
      const int i = __builtin_ctz(rows);
      const uint32_t m = group_ballot((dcol >> i) & 1u, gsh) & g.mates;
      if (grow < 0 && m) { grow = i; gcol = __builtin_ctz(m); }
    }
    gj = grow >= 0 ? grow * nopp + gcol : INF;
  }
  const bool rep = ij >= 0 && ij * nopp + jj == gj;
  const uint32_t low = (1u << jj) - 1u;
  const unsigned long long base = X.rng.ctr;  // bearing k of the call (pair order) takes draw base + k
  // ---- the bearings' slopes -------------------------------------------------
  // bearing of own ship i on opponent j (cell pj) with draw rank r:
  // calculate_bearing (combatant.py:249-263), then the slope tan(radians(bearing))
  // the fix uses; only opponents with two or more bearings get a fix (single
  // bearings only consume their draw)
  auto slope_at = [&](int i, uint32_t pj, int r) {
    const uint32_t pi = COLW(c.pos_cur, own0 + i);
    const double a0 = bearing_tab(P, atab, half, pos_x(pj) - pos_x(pi), pos_y(pj) - pos_y(pi));
    const double gd = (P.dbg_skip & 262144) ? (double)(r & 7) * 0.25 - 1.0  // diagnostics
                                            : X.rng.gauss_at(base + (unsigned long long)r);
    const double bearing = a0 + gd < 0 ? a0 + gd + 360.0 : a0 + gd;
    return (P.dbg_skip & 524288) ? bearing * 0.01 : tan_fd(bearing * DEG2RAD);
  };

  int nbear = 0, obs_n = 0, orank = 0, n = 0;
  uint32_t colb = 0;
  // the bearings this lane evaluates for the group: ranks r = sub (mod GL),
  // at most one per own-ship row; (i | jj << 4 | r << 8) in 16 bits, up to 8
  // kept for after the walk (fix opponents only), any further ones evaluated
  // at once
  uint64_t it0 = 0, it1 = 0;
  int ni = 0;
  // (rows with no EW candidate and no first detection of any lane add nothing)
  for (uint32_t rows = group_or(ecol | (rep ? 1u << ij : 0u)); rows; rows &= rows - 1) {
    const int i = __builtin_ctz(rows);
    const bool bb = ((ecol >> i) & 1u) && i * nopp + jj < gj;
    const uint32_t brow = group_ballot(bb, gsh);
    if (bb) {
      n++;
      colb |= 1u << i;
    }
    {  // rank nbear + t of this row (t-th set lane of brow) is this lane's when t = (sub - nbear) mod GL
      const int cnt = __builtin_popcount(brow), t = (sub - nbear) & (GL - 1);
      if (t < cnt) {
        uint32_t mm = brow;
        int pos = 0, kk = t, cc = __builtin_popcount(mm & 0xffu);
        if (kk >= cc) { kk -= cc; mm >>= 8; pos += 8; }
        cc = __builtin_popcount(mm & 0xfu);
        if (kk >= cc) { kk -= cc; mm >>= 4; pos += 4; }
        cc = __builtin_popcount(mm & 0x3u);
        if (kk >= cc) { kk -= cc; mm >>= 2; pos += 2; }
        if (kk >= (int)(mm & 1u)) pos += 1;
        const uint64_t item = (uint64_t)(i | pos << 4 | ((nbear + t) & 0xff) << 8);
        if (ni < 4) it0 |= item << (16 * ni);
        else if (ni < 8) it1 |= item << (16 * (ni - 4));
        else ms[(i * nopp + pos) * GEPW] = slope_at(i, COLW(c.pos_cur, opp0 + pos), nbear + t);
        ni++;
      }
    }
    nbear += __builtin_popcount(brow);
    const bool rr = rep && ij == i;
    const uint32_t rrow = group_ballot(rr, gsh);
    if (rr) orank = obs_n + __builtin_popcount(rrow & low);
    obs_n += __builtin_popcount(rrow);
  }
  if (X.rng.mode == 1) {  // tape: a draw past the end sets the flag and does not advance
    const long long avail = X.rng.tape_hi - X.rng.tape_lo - (long long)base;
    if (nbear > avail) X.rng.err |= 4u;
    X.rng.ctr += (unsigned long long)(nbear < avail ? nbear : (avail > 0 ? avail : 0));
  } else {
    X.rng.ctr += (unsigned long long)nbear;
  }
  GPROF_ADD(X, 5, tq);
  const uint32_t fixm = group_ballot(n >= 2, gsh);  // opponents with a fix
  if (S.cold->ctr && n >= 2) X.pooled += (unsigned)n;     // work counter: this column's pooled bearings
  // pooled: the group's fix bearings spread over its lanes by rank (ceil(k / GL)
  // slopes per lane, two at a time) into ms, read back by the opponent lanes
  if (fixm && !(P.dbg_skip & 16384)) {
    auto item = [&](int q) { return (uint32_t)((q < 4 ? it0 >> (16 * q) : it1 >> (16 * (q - 4))) & 0xffffu); };
    for (int q = 0; q < ni; q += 2) {
      const uint32_t u1 = item(q), u2 = q + 1 < ni ? item(q + 1) : 0u;
      const bool f1 = (fixm >> ((u1 >> 4) & 15u)) & 1u, f2 = q + 1 < ni && ((fixm >> ((u2 >> 4) & 15u)) & 1u);
      if (!f1 && !f2) continue;
      const uint32_t v1 = f1 ? u1 : u2, v2 = f1 && f2 ? u2 : v1;
      const double m1 = slope_at((int)(v1 & 15u), COLW(c.pos_cur, opp0 + ((v1 >> 4) & 15u)), (int)(v1 >> 8));
      const double m2 = slope_at((int)(v2 & 15u), COLW(c.pos_cur, opp0 + ((v2 >> 4) & 15u)), (int)(v2 >> 8));
      ms[((v1 & 15u) * nopp + ((v1 >> 4) & 15u)) * GEPW] = m1;
      if (f1 && f2) ms[((v2 & 15u) * nopp + ((v2 >> 4) & 15u)) * GEPW] = m2;
    }
    wave_lds_sync();  // the group's slopes written (one wave: its LDS ops complete in order)
  }
  // ---- lane jj: opponent jj's fix and fix targets ---------------------------
  const int fb = colb ? __builtin_ctz(colb) * nopp + jj : INF;  // first bearing pair
  int nt = 0, fxi = 0, fyi = 0;
  uint32_t err = 0;
  if (n >= 2 && !(P.dbg_skip & 16384)) {
    auto slope = [&](int i, double &x1, double &y1) {
      const uint32_t pi = COLW(c.pos_cur, own0 + i);
      x1 = pos_x(pi);
      y1 = pos_y(pi);
      return ms[(i * nopp + jj) * GEPW];
    };
    const int m = n - 1;  // < 16: at most 16 own ships
    FixAcc16 f;
    bool zero = false;
    double mprev = 0.0, xprev = 0.0, yprev = 0.0;
    uint32_t bits = colb;
    int k = 0;
    auto take = [&](double mt, double x1, double y1) {  // bearing k in order
      if (k > 0 && !zero) {
        if (mprev - mt == 0.0) {
          zero = true;
        } else {
          double x3, y3;
          fix_pair(mprev, mt, xprev, yprev, x1, y1, x3, y3);
          f.add(k - 1, m, x3, y3);
        }
      }
      k++;
      mprev = mt;
      xprev = x1;
      yprev = y1;
    };
    while (bits && !zero) {
      const int i1 = __builtin_ctz(bits);
      bits &= bits - 1;
      const bool two = bits != 0;
      const int i2 = two ? __builtin_ctz(bits) : i1;
      if (two) bits &= bits - 1;
      double x1, y1, x2, y2;
      const double m1 = slope(i1, x1, y1), m2 = slope(i2, x2, y2);
      take(m1, x1, y1);
      if (two) take(m2, x2, y2);
    }
    {
      double mx = 0.0, my = 0.0;
      if (zero) {
        err |= LNW_ERRF_ZERODIV;
      } else {
        f.mean(m, mx, my);
        if (!isfinite(mx) || !isfinite(my)) {
          err |= LNW_ERRF_NAN_ROUND;
        } else {
          const double rx = rint(mx), ry = rint(my);
          if (S.cold->ana.ew_log) {  // combatant.py:146-150: (observer position, rounded fix)
            const int ax = (int)fmin(fmax(rx, -32768.0), 32767.0), ay = (int)fmin(fmax(ry, -32768.0), 32767.0);
            ana_record(S.cold->ana.ew_log, S.cold->ana.ew_count, S.cold->ana.ew_cap, (uint32_t)(P.env_base + env),
                       (uint32_t)X.step | (uint32_t)side << 16, COLW(c.pos_cur, me),
                       (uint32_t)(uint16_t)ax | (uint32_t)(uint16_t)ay << 16);
          }
          if (rx >= 0.0 && rx < (double)P.G && ry >= 0.0 && ry < (double)P.G) {
            fxi = (int)rx;
            fyi = (int)ry;
            for (int q = opp0; q < opp1; q++) {
              if (!COLB(c.alive0, q)) continue;
              const uint32_t pq = COLW(c.pos_cur, q);
              const int ddx = pos_x(pq) - fxi, ddy = pos_y(pq) - fyi;
              nt += ddx * ddx + ddy * ddy < 4 ? 1 : 0;
            }
          }
        }
      }
    }
  }
  GPROF_ADD(X, 6, tq);
  // ---- the target list: observed cells, then the fix targets of the
  // opponents in order of their first bearing (combatant.py:152-161)
  int off = obs_n, tot = obs_n;
#pragma unroll
  for (int q = 0; q < GL; q++) {
    const int fbg = __shfl(fb, gsh + q), ntg = __shfl(nt, gsh + q);
    tot += ntg;
    off += fbg < fb ? ntg : 0;
  }
  uint16_t *tl = S.tl + (size_t)me * P.T * E + env;
  const bool tls = !(P.dbg_skip & 1048576);  // (bit 20: diagnostics, no target-list stores)
  if (rep && tls) tl[(size_t)orank * E] = (uint16_t)(pos_x(posj) | (pos_y(posj) << 8));
  if (nt > 0 && tls) {
    for (int q = opp0; q < opp1; q++) {
      if (!COLB(c.alive0, q)) continue;
      const uint32_t pq = COLW(c.pos_cur, q);
      const int ddx = pos_x(pq) - fxi, ddy = pos_y(pq) - fyi;
      if (ddx * ddx + ddy * ddy < 4) {
        tl[(size_t)off * E] = (uint16_t)(fxi | (fyi << 8));
        off++;
      }
    }
  }
  COLW(c.tcnt, me) = (uint32_t)tot;
  X.rng.err |= group_or(err);
  GPROF_ADD(X, 7, tq);
}

// Phase O of the group kernel: the env's observation rows, one side's block
// [ns rows][D] contiguous in the output; lane sub builds and stores float4
// chunks sub, sub + GL, ... (window floats straight from the per-cell record).
__device__ __forceinline__ void group_rows(const KParams &P, const KState &S, const Cols &c,
                                           const double *duct_col, int el, long long env, int sub,
                                           float *obs_b, float *obs_r) {
  for (int sd = 0; sd < 2; sd++) {
    float *out = sd ? obs_r : obs_b;
    if (!out) continue;
    const int own0 = sd ? P.nb : 0, ns = sd ? P.nr : P.nb;
    const int D = side_D(P, sd), D4 = D / 4;  // (4 ns + 52, or 4 ns + 28 for a side of medium ships)
    f32x4 *base = (f32x4 *)(out + (size_t)env * ns * D);
    for (int ch = sub; ch < ns * D4; ch += GL) {
      const int kl = ch / D4, c4 = ch - kl * D4, k = own0 + kl;
      f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (c.alive0[k * PADB + el]) {
        const int tk = c.type[k * PADB + el];
        const uint32_t p = c.pos_cur[k * PAD + el];
        const int wlen = win_len(tk);
        const float *rec = S.winf + ((size_t)win_cls(tk) * P.G * P.G +
                                     (size_t)(pos_x(p) * P.G + pos_y(p))) * 52;
        const int f0 = 4 * c4;
        if (f0 + 4 <= wlen) {
          v = *(const f32x4 *)(rec + f0);
        } else {
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const int f = f0 + q;
            v[q] = f < wlen ? rec[f] : row_tail(P, c, duct_col, el, k, tk, p, own0, ns, kl, f - wlen);
          }
        }
      }
      base[ch] = v;  // (plain: write-through measured no faster here, st_obs4)
    }
  }
}

template <int DT>
__device__ __forceinline__ bool group_move_phase(const KParams &P, const KState &S, Cols &c,
                                                 const void *actions, const uint8_t *row_kind,
                                                 const uint32_t *mask, int env0, int nenv, int A,
                                                 int wid) {
  return move_phase<DT, GNW>(P, S, c, actions, row_kind, mask, env0, nenv, A, wid);
}

// Game.step (game.py:298-525) for runtime team sizes, GL lanes per env.
__global__ __launch_bounds__(GEPW * GL) void step_group_kernel(
    KParams P, KState S, void *actions, const uint8_t *row_kind, float *obs_b, float *obs_r,
    float *rew_b, float *rew_r, int32_t *done_out, float *cog_out) {
  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int slot = tid / GL, sub = tid - (tid / GL) * GL;
  const int env0 = xcd_chunk(P, (int)blockIdx.x, (int)gridDim.x) * GEPW;
  const long long E = P.E;
  const int nenv = (E - env0) < GEPW ? (int)(E - env0) : GEPW;
  const int env = env0 + slot;
  const bool valid = slot < nenv;
  const int nb = P.nb, nr = P.nr, A = nb + nr;
  LdsLayout L = lds_layout(A, nb, nr, S.nmax, P.G * P.W16, P.G);
  Cols c = carve(lds_dyn, L);
  __shared__ double duct_col[WAVE];
  __shared__ int r2col[WAVE];
  const GroupLds GL_ = group_lds(L, P.G * P.W16, A, nb * nr, P.atan_odd != 0);
  uint16_t *tls = GL_.tls >= 0 ? (uint16_t *)(lds_dyn + GL_.tls) : nullptr;
  double *dlz = GL_.dlz >= 0 ? (double *)(lds_dyn + GL_.dlz) : nullptr;
  const bool half = GL_.atab >= 0;
  double *atab_l = half ? (double *)(lds_dyn + GL_.atab) : nullptr;
  const double *atab = half ? atab_l : S.atan_deg;
  double *ms = GL_.ms >= 0 ? (double *)(lds_dyn + GL_.ms) + slot : nullptr;  // [nb * nr][GEPW]

  // ---- phase L: terrain mask, bearing table and the SoA state -------------
  if (tid == 0) prof_stamp(S, 0);
  if (half) {  // 26.6 KB, 16-B loads, all of a thread's issued before any store
    typedef double f64x2 __attribute__((ext_vector_type(2)));  // (HIP's double2 would sit in scratch)
    const f64x2 *src = (const f64x2 *)(S.atan_deg + R_LOS * LOS_W);  // rows dy = 0..R_LOS
    f64x2 *dst = (f64x2 *)atab_l;
    constexpr int NH = (R_LOS + 1) * LOS_W, N2 = NH / 2, U = (N2 + GEPW * GL - 1) / (GEPW * GL);
    f64x2 v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int i = tid + u * GEPW * GL;
      if (i < N2) v[u] = src[i];
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int i = tid + u * GEPW * GL;
      if (i < N2) dst[i] = v[u];
    }
    if ((NH & 1) && tid == 0) atab_l[NH - 1] = S.atan_deg[R_LOS * LOS_W + NH - 1];  // odd count
  }
  stage_mask<GNW>(P, S, c.mask);
  for (int q = tid; q < A * GEPW; q += GEPW * GL) {  // (agent, env) pairs, env fastest
    const int a = q / GEPW, e = q - (q / GEPW) * GEPW;
    if (e < nenv) {
      const size_t ai = (size_t)a * E + env0 + e;
      const uint32_t p = S.pos[ai];
      c.pos_cur[a * PAD + e] = p;
      c.pos_old[a * PAD + e] = p;
      c.pos_new[a * PAD + e] = p;
      const int rd = S.radar[ai];
      c.radar_cur[a * PAD + e] = rd;
      c.radar_old[a * PAD + e] = rd;
      const uint8_t m = S.miss[ai];
      c.miss_cur[a * PADB + e] = m;
      c.miss_old[a * PADB + e] = m;
      c.type[a * PADB + e] = S.type[ai];
      c.alive0[a * PADB + e] = S.alive[ai];
      const int tc = S.tl_cnt[ai];
      c.tcnt[a * PAD + e] = tc;
      if (tls) {  // the list take_action fires over (its first GTL entries)
        const int nq = min(tc, min(GTL, P.T));
        const uint16_t *src = S.tl + (size_t)a * P.T * E + env0 + e;
        for (int k = 0; k < nq; k++) tls[(a * GTL + k) * GEPW + e] = src[(size_t)k * E];
      }
      if (dlz && S.type[ai] == T_LS) dlz[a * GEPW + e] = S.dist_lz[ai];
      c.steps[a * PAD + e] = S.steps[ai];
      c.eng[a * PADB + e] = 0;
      c.mkind[a * PADB + e] = S.mkind[ai];
      c.obsd[a * PADB + e] = 0;
    } else {
      c.alive0[a * PADB + e] = 0;
      c.type[a * PADB + e] = 0;
    }
  }
  if (tid < GEPW) {
    const double d = tid < nenv ? S.duct[env0 + tid] : 1.0;
    duct_col[tid] = d;
    r2col[tid] = max_range2(P, d);
  }
  __syncthreads();
  if (tid == 0) prof_stamp(S, 4);

  // ---- phase M: move targets and feasibility, pair passes over the waves --
  const int dt = P.act_dtype;
  bool pend = false;
  if (dt == LNW_ACT_F32)
    pend = group_move_phase<LNW_ACT_F32>(P, S, c, actions, row_kind, c.mask, env0, nenv, A, wid);
  else if (dt == LNW_ACT_F64)
    pend = group_move_phase<LNW_ACT_F64>(P, S, c, actions, row_kind, c.mask, env0, nenv, A, wid);
  else
    pend = group_move_phase<LNW_ACT_I32>(P, S, c, actions, row_kind, c.mask, env0, nenv, A, wid);
  if (__syncthreads_or(pend)) {  // the rare A* fallback (open lists sized for one wave)
    if (wid == 0) move_astar_pass(P, S, c, nenv, A);
    __syncthreads();
  }

  // ---- phase S: the sequential agent loop, one env per lane group ---------
  if (tid == 0) prof_stamp(S, 1);
  if (valid) {
    Ctx X{P, S, c, slot, env, duct_col, make_rng(P, S, env), c.mask, E, r2col[slot], 0};
    X.leader = sub == 0;
    X.gsub = sub;
    X.gsh = (int)(threadIdx.x & (WAVE - 1)) & ~(GL - 1);
    GSide gs[2];
    uint32_t movedm;
    GPROF_MARK(tp);
    group_pair_tables(X, sub, gs, movedm);
    GPROF_ADD(X, 3, tp);
    Neut N{{0, 0}, {0u, 0u}};
    int ev[8];
#pragma unroll
    for (int q = 0; q < 8; q++) ev[q] = S.envi[q * E + env];
    X.step = ev[2];
    int hits[2] = {0, 0};
    int bsx = 0, bsy = 0, rsx = 0, rsy = 0;  // exact integer sums
    int nbp = 0, nrp = 0;
    GPROF_MARK(t0);
    for (int a = 0; a < A; a++) {
      const int lane = slot;  // LDS column of the env (COLW / COLB)
      const bool al = COLB(c.alive0, a) != 0;  // sunk ships skip their turn (reward 0)
      const int side = a >= nb;
      bool engage = false, moved = false;
      int destroyed = 0;
      if (al) {
        const uint32_t p0 = COLW(c.pos_cur, a);
        if (!side) {
          if (P.side_blue) { bsx += pos_x(p0); bsy += pos_y(p0); nbp++; }
        } else {
          rsx += pos_x(p0); rsy += pos_y(p0); nrp++;
        }
        const size_t row = ((size_t)env * A + a) * 4;
        const double a0 = COLW(c.act0, a);
        double a1 = COLW(c.act1, a);
        const int kind = COLB(c.akind, a);
        // untrained red: random salvo (game.py:375-379), written back in place
        if (side && !P.trained_red) {
          if (X.rng.uniform() < P.red_aggression) {
            double v = X.rng.uniform();
            if (dt == LNW_ACT_F32) { float f = (float)v; ((float *)actions)[row + 1] = f; a1 = f; }
            else if (dt == LNW_ACT_F64) {
              if (kind == K_F32) v = (double)(float)v;
              ((double *)actions)[row + 1] = v; a1 = v;
            } else { ((int32_t *)actions)[row + 1] = 0; a1 = 0.0; }
          }
        }
        // take_action (combatant.py:501-565)
        const double engagement = P.discrete ? rint(a1) : a1;
        const int keng = P.discrete ? K_PYINT : kind;
        const int mk = COLB(c.mkind, a);
        double thr_v = salvo_size(engagement, keng, &COLB(c.miss_cur, a), mk);
        // round(nan/inf) of engagement * missiles raises (combatant.py:528): flagged, no engagement
        if (!isfinite(thr_v)) { X.rng.err |= LNW_ERRF_NAN_ROUND; thr_v = 0.0; }
        engage = thr_v > 0.0;
        const int tn = (int)COLW(c.tcnt, a);
        if (engage && tn > 0 && !(P.dbg_skip & 65536)) {  // (bit 16: diagnostics, no fire)
          // the list read GL entries at a time, one per lane of the group (the
          // loads of a chunk in flight together), each entry taken by shuffle
          const uint16_t *tl = S.tl + (size_t)a * P.T * E + env;
          const int gsh = (int)(threadIdx.x & (WAVE - 1)) & ~(GL - 1);
          // entries side by side unless an analytics map or the engagement log
          // wants fire_dev's per-hit records in list order (LNW_DEBUG_SKIP bit 15:
          // entry by entry always)
          const bool par = !S.cold->ana.heatmap && !S.cold->ana.coldmap && !S.cold->ana.launch && !S.cold->ana.eng_log &&
                           !(P.dbg_skip & 32768);
          for (int q0 = 0; q0 < tn; q0 += GL) {
            const int q = q0 + sub;
            const int mine = q >= tn ? 0 : (tls && q < GTL) ? (int)tls[(a * GTL + q) * GEPW + slot]
                                                           : (int)tl[(size_t)q * E];
            const int nq = tn - q0 < GL ? tn - q0 : GL;
            if (par) {
              destroyed += fire_group_chunk(X, a, mine, nq, engagement, keng, N);
              continue;
            }
            for (int u = 0; u < nq; u++) {
              const uint16_t tg = (uint16_t)__shfl(mine, gsh + u);
              if (fire_dev<true>(X, a, tg & 0xff, tg >> 8, engagement, keng, N)) destroyed++;
            }
          }
        }
        if (side) ev[6] += destroyed; else ev[5] += destroyed;
        if (!isfinite(a0)) { X.rng.err |= LNW_ERRF_NAN_ROUND; COLW(c.radar_cur, a) = 0; }
        else COLW(c.radar_cur, a) = radar_setting(a0);
        const uint32_t pn = COLW(c.pos_new, a);
        moved = (pn & 0x80000000u) != 0;
        if (moved) COLW(c.pos_cur, a) = pn & 0x7fffffffu;
        GPROF_ADD(X, 0, t0);
        if (!(P.dbg_skip & 128)) get_obs_group(X, a, sub, gs, movedm, atab, half, ms);
        GPROF_SET(t0);
      }
      double r = 0.0;
      if (al && !(P.dbg_skip & 256))
        r = reward_core(P, S, c, slot, E, env, a, moved, engage, destroyed, dlz ? dlz + slot : nullptr, GEPW);
      GPROF_ADD(X, 1, t0);
      COLW(c.reward, a) = r;
      if (al) {
        if (!side) {
          if (P.side_blue ? destroyed > 0 : engage) COLB(c.eng, a) = 1;
        } else {
          if (!P.trained_red ? engage : destroyed > 1) COLB(c.eng, a) = 1;
        }
        if (side) hits[1] += destroyed; else hits[0] += destroyed;  // (constant indices: no scratch)
      }
    }
    env_tail(P, S, c, slot, env, nb, A, N, ev, hits, nbp, nrp, bsx, bsy, rsx, rsy, X.rng, rew_b,
             rew_r, done_out, cog_out);
    if (S.cold->ctr && X.pooled) atomicAdd(&S.cold->ctr[3], (unsigned long long)X.pooled);
    GPROF_ADD(X, 2, t0);
    GPROF_FLUSH(X);
  }
  // ---- phase O: observation rows ----------------------------------------
  if (valid && !(P.dbg_skip & 1) && !P.no_obs) group_rows(P, S, c, duct_col, slot, env, sub, obs_b, obs_r);
}
