// lnw_quiet.inc — the quiet-workgroup path of step_kernel, included by
// lnw_kernels.hip inside its anonymous namespace (uses Cols, row_regs_t,
// copy_side_t, reward_core, env_tail from there).
//
// Quiet workgroups (templated equal team sizes, two-wave workgroups of up to
// 64 envs, LOS table mode; lanes past a partial workgroup's last env count as
// quiet and idle).
// An env is quiet this step when no live agent holds a target
// list (so nobody fires: combatant.py:535-548 loops over an empty list), every
// radar action is finite, and no blue/red pair is within the largest sensor
// reach r2max (max over ship classes of radar^2, EW^2 and the d < 4 close
// range) for any combination of either ship's old and new position — the
// positions get_obs can see during the agent loop (SURVEY §9 Q1). Then every
// get_obs of the step returns an empty target list with no bearing and no draw
// (combatant.py:106-161), and Game.step splits into per-agent work (radar,
// move, calculate_reward with no targets and no hits: game.py:214-295) plus
// the per-env tail (game.py:409-520): bit-identical to phase S, without its
// sequential chain. An untrained (scripted) red's random salvo (game.py:375-379)
// is the only draw such a step makes before the tail: its engagement value
// cannot fire (empty target lists) and with no hits the team bonus it gates
// is zero, so phase Q replays just the draws and the in-place action write.
// When all envs of a workgroup are quiet, phase Q sets
// every agent's radar and cell with both waves; wave 1 then streams whole env
// blocks of observation rows while wave 0 computes the rewards and the tail
// before joining it.

template <int NB, int NR>
__device__ __forceinline__ bool env_quiet_t(const KParams &P, const Cols &c, int lane, int r2) {
  constexpr int A = NB + NR;
  int xs[A][2], ys[A][2];
  uint32_t alive = 0, bad = 0;
  // every LDS column of the test read up front, without a branch between the
  // reads (a short-circuit && here made one LDS round trip per agent: ~1 us of
  // the 8 192-env shard's chain)
  uint32_t alb[A], po[A], pn[A], tc[A];
  double a0[A], a1[A];
#pragma unroll
  for (int a = 0; a < A; a++) {
    alb[a] = c.alive0[a * PADB + lane];
    po[a] = c.pos_old[a * PAD + lane];
    pn[a] = c.pos_new[a * PAD + lane];
    tc[a] = c.tcnt[a * PAD + lane];
    a0[a] = c.act0[a * PAD + lane];
    a1[a] = c.act1[a * PAD + lane];
  }
#pragma unroll
  for (int a = 0; a < A; a++) {
    const uint32_t al = alb[a] != 0 ? 1u : 0u;
    alive |= al << a;
    const uint32_t pm = (pn[a] & 0x80000000u) ? (pn[a] & 0x7fffffffu) : po[a];
    xs[a][0] = pos_x(po[a]); ys[a][0] = pos_y(po[a]);
    xs[a][1] = pos_x(pm); ys[a][1] = pos_y(pm);
    // a radar action round() can take, and an engagement whose threshold
    // round(a1 * missiles) is finite (|a1| < 1e30 implies it for <= 8 missiles in
    // f32 and f64): other rows raise in the reference (combatant.py:528, 558),
    // which phase S flags
    const uint32_t fin = (isfinite(a0[a]) ? 1u : 0u) & (fabs(a1[a]) < 1e30 ? 1u : 0u);
    bad |= al & ((tc[a] != 0 ? 1u : 0u) | (fin ^ 1u));
  }
  // bounding boxes of each side's live ships over old and new cells: their gap
  // bounds every pair distance from below, so fleets that stay apart (the
  // common case) skip the pair test
  int bx0 = 0x7fff, bx1 = -1, by0 = 0x7fff, by1 = -1, rx0 = 0x7fff, rx1 = -1, ry0 = 0x7fff, ry1 = -1;
#pragma unroll
  for (int a = 0; a < A; a++) {
    const bool al = (alive >> a) & 1u;
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int x = xs[a][u], y = ys[a][u];
      if (a < NB) {
        bx0 = al ? min(bx0, x) : bx0; bx1 = al ? max(bx1, x) : bx1;
        by0 = al ? min(by0, y) : by0; by1 = al ? max(by1, y) : by1;
      } else {
        rx0 = al ? min(rx0, x) : rx0; rx1 = al ? max(rx1, x) : rx1;
        ry0 = al ? min(ry0, y) : ry0; ry1 = al ? max(ry1, y) : ry1;
      }
    }
  }
  const int gx = max(0, max(rx0 - bx1, bx0 - rx1)), gy = max(0, max(ry0 - by1, by0 - ry1));
  if (bad != 0 || gx * gx + gy * gy >= r2) return bad == 0;  // (no live ship: empty box, gap huge)
  // branch-free: nearest of the four old/new position combinations per pair
  if (P.G <= 128) {
    // two combinations per packed 16-bit instruction: a ship's old / new
    // coordinate in the two halves (and swapped), so X[j] - X[i] holds
    // (old - old, new - new) and Xs[j] - X[i] (new - old, old - new); exact
    // while a squared distance fits in 15 bits (coordinates below 128)
    typedef short s16x2 __attribute__((ext_vector_type(2)));
    s16x2 X[A], Y[A], Xs[A], Ys[A];
#pragma unroll
    for (int a = 0; a < A; a++) {
      X[a] = s16x2{(short)xs[a][0], (short)xs[a][1]};
      Y[a] = s16x2{(short)ys[a][0], (short)ys[a][1]};
      Xs[a] = s16x2{(short)xs[a][1], (short)xs[a][0]};
      Ys[a] = s16x2{(short)ys[a][1], (short)ys[a][0]};
    }
#pragma unroll
    for (int i = 0; i < NB; i++)
#pragma unroll
      for (int j = NB; j < A; j++) {
        const s16x2 dx = X[j] - X[i], dy = Y[j] - Y[i], ex = Xs[j] - X[i], ey = Ys[j] - Y[i];
        const s16x2 m = __builtin_elementwise_min(dx * dx + dy * dy, ex * ex + ey * ey);
        const int dmin = min((int)m.x, (int)m.y);
        bad |= (alive >> i) & (alive >> j) & (dmin < r2 ? 1u : 0u);
      }
    return bad == 0;
  }
#pragma unroll
  for (int i = 0; i < NB; i++)
#pragma unroll
    for (int j = NB; j < A; j++) {
      int dmin = 0x7fffffff;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int dx = xs[j][u & 1] - xs[i][u >> 1], dy = ys[j][u & 1] - ys[i][u >> 1];
        dmin = min(dmin, dx * dx + dy * dy);
      }
      bad |= (alive >> i) & (alive >> j) & (dmin < r2 ? 1u : 0u);
    }
  return bad == 0;
}

// The same predicate for a whole small workgroup (epw * NB <= 64 lanes, equal
// team sizes), spread over (ship, env) lanes instead of one env per lane: lane
// (g, e) = (lane / epw, lane % epw) checks blue ship g and red ship NB + g of env
// e (alive with a target list or a non-finite action row) and the NR pairs
// (g, NB + j). A single wave per SIMD issues every instruction of the per-env
// version at 4 cycles each (~900 of them: 1.7 us of the 8 192-env shard's
// chain); spread, each lane does a quarter of the pairs and two of the eight
// ships. Returns true when no env of the workgroup has anything in reach.
template <int NB, int NR>
__device__ __forceinline__ bool wg_quiet_spread_t(const KParams &P, const Cols &c, int lane, const int *r2col) {
  static_assert(NB == NR, "the spread test pairs blue ship g with red ship NB + g");
  const int g = lane / P.epw, e = lane - g * P.epw;
  uint32_t bad = 0;
  if (g < NB) {
    uint32_t al[1 + NR], po[1 + NR], pn[1 + NR], tc[2];
    double a0[2], a1[2];
    // [0]: blue ship g, [1 + j]: red ship NB + j
#pragma unroll
    for (int k = 0; k <= NR; k++) {
      const int a = k == 0 ? g : NB + k - 1;
      al[k] = c.alive0[a * PADB + e];
      po[k] = c.pos_old[a * PAD + e];
      pn[k] = c.pos_new[a * PAD + e];
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {  // ships g and NB + g
      const int a = h * NB + g;
      tc[h] = c.tcnt[a * PAD + e];
      a0[h] = c.act0[a * PAD + e];
      a1[h] = c.act1[a * PAD + e];
    }
    const int r2 = r2col[e];
    uint32_t alg[2];
    alg[0] = c.alive0[g * PADB + e] != 0 ? 1u : 0u;
    alg[1] = c.alive0[(NB + g) * PADB + e] != 0 ? 1u : 0u;
#pragma unroll
    for (int h = 0; h < 2; h++) {  // (as env_quiet_t: combatant.py:528, 558)
      const uint32_t fin = (isfinite(a0[h]) ? 1u : 0u) & (fabs(a1[h]) < 1e30 ? 1u : 0u);
      bad |= alg[h] & ((tc[h] != 0 ? 1u : 0u) | (fin ^ 1u));
    }
    int x[1 + NR][2], y[1 + NR][2];
#pragma unroll
    for (int k = 0; k <= NR; k++) {
      const uint32_t pm = (pn[k] & 0x80000000u) ? (pn[k] & 0x7fffffffu) : po[k];
      x[k][0] = pos_x(po[k]); y[k][0] = pos_y(po[k]);
      x[k][1] = pos_x(pm); y[k][1] = pos_y(pm);
    }
    const uint32_t ali = al[0] != 0 ? 1u : 0u;
#pragma unroll
    for (int j = 1; j <= NR; j++) {
      int dmin = 0x7fffffff;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int dx = x[j][u & 1] - x[0][u >> 1], dy = y[j][u & 1] - y[0][u >> 1];
        dmin = min(dmin, dx * dx + dy * dy);
      }
      bad |= ali & (al[j] != 0 ? 1u : 0u) & (dmin < r2 ? 1u : 0u);
    }
  }
  return !__any(bad != 0);
}

// Whole env blocks of a quiet workgroup's observation rows: the 16 passes
// (8 envs x one side each, rows staged in LDS at the phase-O stride, then one
// contiguous 8.5 KB copy-out) are claimed from an LDS counter by whichever wave
// is free; each wave owns one stage. Lanes 0..8*NS-1 build one row each
// (row_regs_t: same content as the phase-S emission and phase O).
// pass0 >= 0: the caller took that pass without claiming it and has already
// loaded its window records into v / w48 (wave 1's pass 0, loaded before the
// phase-Q barrier so the stream starts without an L2 round trip).
template <int NB, int NR>
__device__ __forceinline__ void quiet_emit_t(const KParams &P, const KState &S, const Cols &c,
                                             const double *duct_col, int *claim, float *stage,
                                             float *obs_b, float *obs_r, int env0, int nenv,
                                             f32x4 (&v)[12], float &w48, int pass0) {
  static_assert(NB == NR, "templated obs rows assume equal team sizes");
  constexpr int NS = NB, ROWS = QEPG * NS;
  const int NPASS = 2 * ((nenv + QEPG - 1) / QEPG);  // a partial last group copies fewer envs
  constexpr int N4 = ROWS * (4 * NS + 52) / 4;
  const int lane = threadIdx.x & (WAVE - 1);
  const int G = P.G;
  const f32x4 *wtab = (const f32x4 *)S.winf;
  const int my_e = lane / NS, kl = lane - my_e * NS;
  const bool builder = lane < ROWS;
  auto next_pass = [&]() {
    int p = 0;
    if (lane == 0) p = atomicAdd(claim, 1);
    return __shfl(p, 0);
  };
  auto prefetch = [&](int pass) {  // the row's window record (dead rows read cell 0's, ignored)
    int off = 0;
    if (builder) {
      const int el = (pass >> 1) * QEPG + my_e, k = (pass & 1) * NB + kl;
      if (c.alive0[k * PADB + el]) {
        const uint32_t p = c.pos_cur[k * PAD + el];
        off = ((c.type[k * PADB + el] == T_LS ? G * G : 0) + pos_x(p) * G + pos_y(p)) * 13;
      }
    }
    if (P.dbg_skip & 1024) {  // diagnostics: no window-record reads
#pragma unroll
      for (int q = 0; q < 12; q++) v[q] = f32x4{0.f, 0.f, 0.f, (float)off};
      return;
    }
#pragma unroll
    for (int q = 0; q < 12; q++) v[q] = wtab[off + q];
    w48 = ((const float *)(wtab + off))[48];
  };
  int pass = pass0;
  if (pass < 0) {
    pass = next_pass();
    if (pass < NPASS) prefetch(pass);
  }
  while (pass < NPASS) {
    const int side = pass & 1, g = pass >> 1;
    if (builder)
      row_regs_t<NS>(c, duct_col, g * QEPG + my_e, side * NB + kl, side * NB, v, w48,
                     stage + lane * stage_stride(NS), c.qlut);
    wave_lds_sync();
    const int next = next_pass();
    if (next < NPASS) prefetch(next);  // before this pass's stores (vmcnt is in issue order)
    float *out = side ? obs_r : obs_b;
    const int ne = min(QEPG, nenv - g * QEPG);
    if (out) copy_side_t<NS, N4, false>(stage, out, S.dummy, ne, (long long)env0 + g * QEPG, P.store_wt);
    wave_lds_sync();
    pass = next;
  }
}

// centre of gravity of the pre-move positions (game.py:326-331): the sums over
// the live ships of each side (blue's only when blue is the trained side), every
// column read before any is used
template <int NB, int NR>
__device__ __forceinline__ void quiet_cog_sums_t(const KParams &P, const Cols &c, int lane, int &bsx, int &bsy,
                                                 int &rsx, int &rsy, int &nbp, int &nrp) {
  constexpr int A = NB + NR;
  uint32_t al[A], p0[A];
#pragma unroll
  for (int a = 0; a < A; a++) {
    al[a] = COLB(c.alive0, a);
    p0[a] = COLW(c.pos_old, a);
  }
  bsx = bsy = rsx = rsy = nbp = nrp = 0;
  const bool sb = P.side_blue;
#pragma unroll
  for (int a = 0; a < A; a++) {
    const bool on = al[a] != 0 && (a >= NB || sb);
    const int x = on ? pos_x(p0[a]) : 0, y = on ? pos_y(p0[a]) : 0, n = on ? 1 : 0;
    if (a < NB) { bsx += x; bsy += y; nbp += n; }
    else { rsx += x; rsy += y; nrp += n; }
  }
}

// Phase Q, part 1, for the agents a = W, W+2, ... (compile-time, so every LDS
// column read of the wave's agents is issued up front): what take_action does
// for an agent whose get_obs finds nothing — radar = round(a0)
// (combatant.py:558) and the move. Everything an observation row reads is then
// final.
template <int NB, int NR, int W>
__device__ __forceinline__ void quiet_moves_t(Cols &c, int lane) {
  constexpr int A = NB + NR, N = (A - W + 1) / 2;
  bool al[N];
  double a0[N];
  uint32_t pn[N];
#pragma unroll
  for (int k = 0; k < N; k++) {
    const int a = W + 2 * k;
    al[k] = COLB(c.alive0, a) != 0;
    a0[k] = COLW(c.act0, a);
    pn[k] = COLW(c.pos_new, a);
  }
#pragma unroll
  for (int k = 0; k < N; k++) {
    const int a = W + 2 * k;
    if (!al[k]) continue;
    COLW(c.radar_cur, a) = radar_setting(a0[k]);
    if (pn[k] & 0x80000000u) COLW(c.pos_cur, a) = pn[k] & 0x7fffffffu;
  }
}

// Wave 0's part of a small quiet workgroup's step (epw * NB <= 64, the direct
// mode of quiet_step_t), spread over the wave's lanes instead of one env per
// lane: lane (g, e) = (lane / epw, lane % epw) computes calculate_reward for
// agents g and NB + g of env e; the env lanes (lane = e) then play the
// scripted red's salvo draws, the shared tail (env_tail_core), the per-env
// outputs, counters and the auto-reset; last the pair lanes store their
// agents' rewards and state (phase W) for envs that do not reset. Per wave
// that is two copies of the reward code and two of the state stores instead
// of eight of each, with the same values and stores as env_tail.
// calculate_reward of agents h * NB + g, h in [H0, H1), for env e by pair lane
// (g, e) = (lane / epw, lane % epw) of a small quiet workgroup
// calculate_reward (game.py:214-295) of an agent whose get_obs found nothing and
// who fired nothing: reward_core with tl_n = 0, engage = false, n_hit = 0, from
// columns the caller read up front (steps already counted); a landing ship's
// dist_lz store only for a live agent
__device__ __forceinline__ double quiet_reward(const KParams &P, const KState &S, long long E, int env, int a,
                                               int t, uint32_t p, int steps, bool moved, bool live) {
  double r = moved ? 1.0 : 0.0;  // 0.0 + 1.0, or fmax(0.0 - 0.5, 0.0); + 0 * 10 hits
  const int x = pos_x(p), y = pos_y(p);
  const bool red = a >= P.nb;
  if (red && t != T_LS && !P.aggressive && steps > 14) {
    if (x < 19 || x > 55 || y < 40 || y > 70) r = fmax(r - 2.0, 0.0);
    else r += 1.0;
  }
  if (red && P.aggressive && t != T_LS) {
    const int dx = x - 15, dy = y - 60;
    const double nom = fmax(sqrt((double)(dx * dx + dy * dy)), 1.0);
    r += (1.0 / (nom / (mast_cls(t) ? P.den[1] : P.den[0]))) * 1.0;
  }
  if (t == T_LS) {
    const size_t ai = (size_t)a * E + env;
    const int dx = x - P.lz_x, dy = y - P.lz_y;
    const double dl = sqrt((double)(dx * dx + dy * dy));
    if (dl > 0) {
      const double cur = (P.dbg_skip & 2097152) ? 1e9 : S.dist_lz[ai];  // (bit 21: diagnostics)
      if (dl < cur) {
        r += 1.0;
        if (live) S.dist_lz[ai] = dl;
      } else {
        r -= 1.0;
      }
    } else {
      r += 100.0;
    }
    if (dl == 0) r += 100.0;
    else r += log10(100.0 / dl) * 5.0;
  }
  return r;
}

template <int NB, int NR, int H0, int H1>
__device__ __forceinline__ void quiet_rewards_spread_t(const KParams &P, const KState &S, Cols &c, int lane,
                                                       int env0, int nenv) {
  const long long E = P.E;
  const int g = lane / P.epw, e = lane - g * P.epw;
  if (g < NB && e < nenv) {
    constexpr int H = H1 - H0;
    uint32_t al[H], pc[H], pn[H], ty[H];
    int st[H];
#pragma unroll
    for (int k = 0; k < H; k++) {  // every column read before the first use
      const int a = (H0 + k) * NB + g;
      al[k] = c.alive0[a * PADB + e];
      pc[k] = c.pos_cur[a * PAD + e];
      pn[k] = c.pos_new[a * PAD + e];
      ty[k] = c.type[a * PADB + e];
      st[k] = c.steps[a * PAD + e];
    }
#pragma unroll
    for (int k = 0; k < H; k++) {
      const int a = (H0 + k) * NB + g;
      const bool live = al[k] != 0;
      // (+ 0.0: the team bonus of a step without hits, game.py:425-433, folded in;
      // env_tail_core(.., bonus_folded))
      const double r = quiet_reward(P, S, E, env0 + e, a, (int)ty[k], pc[k], st[k] + 1,
                                    (pn[k] & 0x80000000u) != 0, live) + 0.0;
      if (live) c.steps[a * PAD + e] = st[k] + 1;
      c.reward[a * PAD + e] = live ? r : 0.0;
    }
  }
}

template <int NB, int NR>
__device__ __forceinline__ void quiet_tail_spread_t(const KParams &P, const KState &S, Cols &c, int lane,
                                                    int env0, int nenv, int (&ev)[8], Rng &rng,
                                                    uint32_t kinds, void *actions, float *rew_b,
                                                    float *rew_r, int32_t *done_out, float *cog_out) {
  constexpr int A = NB + NR;
  __shared__ uint8_t qreset[WAVE];
  const long long E = P.E;
  const int g = lane / P.epw, e = lane - g * P.epw;
  const bool pl = g < NB && e < nenv;
  quiet_rewards_spread_t<NB, NR, 0, 2>(P, S, c, lane, env0, nenv);
  wave_lds_sync();
  prof_stamp(S, 10);
  if (lane < nenv) {  // env lanes: column = lane
    const int env = env0 + lane;
    if (!P.trained_red) {
      // untrained red: random salvo (game.py:375-379) for each live red ship in
      // turn order, written back in place as phase S does
#pragma unroll
      for (int a = NB; a < A; a++) {
        if (!COLB(c.alive0, a)) continue;
        if (rng.uniform() < P.red_aggression) {
          double v = rng.uniform();
          const size_t row = ((size_t)env * A + a) * 4;
          if (P.act_dtype == LNW_ACT_F32) ((float *)actions)[row + 1] = (float)v;
          else if (P.act_dtype == LNW_ACT_F64) {
            if ((COLB(c.akind, a) & 3u) == K_F32) v = (double)(float)v;
            ((double *)actions)[row + 1] = v;
          } else {
            ((int32_t *)actions)[row + 1] = 0;
          }
        }
      }
    }
    int bsx, bsy, rsx, rsy, nbp, nrp;
    quiet_cog_sums_t<NB, NR>(P, c, lane, bsx, bsy, rsx, rsy, nbp, nrp);
    const Neut N{{0, 0}, {0u, 0u}};
    const int hits[2] = {0, 0};
    double cog;
    const int done = env_tail_core(P, c, lane, NB, A, N, ev, hits, nbp, nrp, bsx, bsy, rsx, rsy, &cog, true);
    if (P.rew_f64) {
      if (cog_out) ((double *)cog_out)[env] = cog;
    } else if (cog_out) {
      cog_out[env] = (float)cog;
    }
    if (done_out) done_out[env] = done;
    const bool do_reset = env_resets(P, done, ev[2]);
    qreset[lane] = do_reset ? 1 : 0;
    // a quiet step changes the step counter and, when it ends the episode, the
    // victory counters; ship counts, engagements and the reset count stay
    S.envi[2 * E + env] = ev[2];
    if (done == 0) {
      S.envi[3 * E + env] = ev[3];
      S.envi[4 * E + env] = ev[4];
    }
    if (do_reset) reset_env_dev(P, S, env, rng);  // writes every agent's state itself
    if (!P.trained_red || do_reset) S.rng[env] = rng.ctr;  // (else this step drew nothing)
    if (rng.err) S.err[env] |= rng.err;
  }
  wave_lds_sync();
  prof_stamp(S, 11);
  if (pl) {
    const int env = env0 + e;
    const bool rs = qreset[e] != 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int a = h * NB + g;
      const double r = c.reward[a * PAD + e];
      float *out = h ? rew_r : rew_b;
      if (out) {
        if (P.rew_f64) ((double *)out)[(size_t)env * NB + g] = r;
        else out[(size_t)env * NB + g] = (float)r;
      }
      if (rs) continue;
      // phase W: a quiet step fires nothing, sinks nothing and leaves every
      // target list empty, so missiles, their kind, alive and the list length keep
      // their values
      const size_t ai = (size_t)a * E + env;
      S.pos[ai] = c.pos_cur[a * PAD + e];
      S.radar[ai] = c.radar_cur[a * PAD + e];
      S.steps[ai] = c.steps[a * PAD + e];
    }
  }
  prof_stamp(S, 2);
}

// Wave 0 of a quiet workgroup after phase Q, one env per lane: the scripted
// red's salvo draws (game.py:375-379), every agent's calculate_reward (no
// targets, no hits: game.py:214-295), the cog of the pre-move positions and
// the shared tail with outputs and phase W (env_tail).
template <int NB, int NR>
__device__ __forceinline__ void quiet_tail_env_t(const KParams &P, const KState &S, Cols &c, int lane,
                                                 int env, int (&ev)[8], Rng &rng, uint32_t moved,
                                                 uint32_t kinds, void *actions, float *rew_b,
                                                 float *rew_r, int32_t *done_out, float *cog_out) {
  constexpr int A = NB + NR;
  const long long E = P.E;
  if (!P.trained_red) {
    // untrained red: random salvo (game.py:375-379) for each live red ship in
    // turn order, written back in place as phase S does
#pragma unroll
    for (int a = NB; a < A; a++) {
      if (!COLB(c.alive0, a)) continue;
      if (rng.uniform() < P.red_aggression) {
        double v = rng.uniform();
        const size_t row = ((size_t)env * A + a) * 4;
        if (P.act_dtype == LNW_ACT_F32) ((float *)actions)[row + 1] = (float)v;
        else if (P.act_dtype == LNW_ACT_F64) {
          if (((kinds >> (2 * a)) & 3u) == K_F32) v = (double)(float)v;
          ((double *)actions)[row + 1] = v;
        } else {
          ((int32_t *)actions)[row + 1] = 0;
        }
      }
    }
  }
  {
    uint32_t al[A], pc[A], ty[A];
    int st[A];
#pragma unroll
    for (int a = 0; a < A; a++) {  // every column read before the first use
      al[a] = COLB(c.alive0, a);
      pc[a] = COLW(c.pos_cur, a);
      ty[a] = COLB(c.type, a);
      st[a] = COLW(c.steps, a);
    }
#pragma unroll
    for (int a = 0; a < A; a++) {
      const bool live = al[a] != 0;
      // (+ 0.0: the zero team bonus folded in, as above)
      const double r = quiet_reward(P, S, E, env, a, (int)ty[a], pc[a], st[a] + 1, (moved >> a) & 1u, live) + 0.0;
      if (live) COLW(c.steps, a) = st[a] + 1;
      COLW(c.reward, a) = live ? r : 0.0;
    }
  }
  prof_stamp(S, 10);
  const Neut N{{0, 0}, {0u, 0u}};
  const int hits[2] = {0, 0};
  int bsx, bsy, rsx, rsy, nbp, nrp;
  quiet_cog_sums_t<NB, NR>(P, c, lane, bsx, bsy, rsx, rsy, nbp, nrp);
  prof_stamp(S, 11);
  env_tail(P, S, c, lane, env, NB, A, N, ev, hits, nbp, nrp, bsx, bsy, rsx, rsy, rng, rew_b,
           rew_r, done_out, cog_out, true);
  }

// A quiet workgroup's step after phase M (see above): phase Q part 1 (both
// waves split the agents), one barrier, then wave 1 starts the observation
// stream at once while wave 0 computes every agent's calculate_reward (no
// targets, no hits: game.py:214-295, the same reward_core phase S calls), the
// per-env tail and phase W, and then joins the stream. The move flags the
// rewards need are read before the barrier: wave 1's stage aliases pos_new.
template <int NB, int NR, bool SL = false>
__device__ __forceinline__ void quiet_step_t(const KParams &P, const KState &S, Cols &c, int lane,
                                             int env, int wid, const double *duct_col, int *claim,
                                             void *actions, float *obs_b, float *obs_r, float *rew_b,
                                             float *rew_r, int32_t *done_out, float *cog_out, int env0,
                                             int nenv, bool valid, bool evpre, const int (&evp)[8],
                                             const Rng &rngp) {
  constexpr int A = NB + NR;
  const long long E = P.E;
  uint32_t moved = 0, kinds = 0;
  int ev[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  Rng rng{};
  // wave 1 takes pass 0 (envs 0..7, blue rows) and loads its window records now,
  // from the final cells phase M left (pos_new when it moved, else pos_old: the
  // cells quiet_moves_t commits), so they are in flight across phase Q
  // (LNW_DEBUG_SKIP bit 22: in the staged forms, claimed and loaded after the barrier instead)
  const bool early = !(P.dbg_skip & 4194304);
  // small workgroups (nenv * NB <= 64 lanes: config 2 and config 3's per-GPU
  // shard run 16 envs per workgroup): wave 1 builds every row itself, lane
  // (env, k) the blue row of agent k and the red row of agent NB + k, both
  // window records loaded before the barrier and the rows stored straight from
  // registers, so the stream costs one L2 round trip instead of a chain of
  // staged passes while wave 0 runs the tail
  // (the same condition that gave the launch its whole-side stages, c.qbig)
  // (two slabs of 64 / NB envs when the host gave the launch qbig stages for
  // wider workgroups: step_qdirect, P.qdirect; the pair-lane tail needs the
  // narrow form, spread)
  // (not a matter of `early`: bit 22 moves the staged forms' first pass only. A
  // direct form that it turned into a staged one kept spread, skipped the moved /
  // kinds fill below and paid every moved ship reward 0 instead of 1)
  const bool direct = (SL ? P.qdirect != 0 : P.epw * NB <= WAVE) && P.los_mode == 0;
  const bool spread = P.epw * NB <= WAVE;
  f32x4 v[12], vr[12];
  float w48 = 0.0f, wr48 = 0.0f;
  if (wid == 1 && direct && !P.no_obs) {
    const int my_e = lane / NB, kl = lane - my_e * NB;  // (slab 0)
    const bool mine = my_e < nenv;
    load_window(S, mine ? window_rec(P, c, kl, my_e) : 0, v, w48);
    load_window(S, mine ? window_rec(P, c, NB + kl, my_e) : 0, vr, wr48);
  } else if (wid == 1 && early && !P.no_obs) {
    const int my_e = lane / NB, kl = lane - my_e * NB;
    const int off = lane < QEPG * NB && my_e < nenv ? window_rec(P, c, kl, my_e) : 0;
    if (P.dbg_skip & 1024) {  // diagnostics: no window-record reads (as quiet_emit_t's prefetch)
#pragma unroll
      for (int q = 0; q < 12; q++) v[q] = f32x4{0.f, 0.f, 0.f, (float)off};
    } else {
      load_window(S, off, v, w48);
    }
  }
  if (wid == 0) {
    quiet_moves_t<NB, NR, 0>(c, lane);
    if (!spread) {  // (the pair-lane tail reads them after the barrier: wave 1's stages do not alias them)
#pragma unroll
      for (int a = 0; a < A; a++) {
        moved |= (COLW(c.pos_new, a) & 0x80000000u ? 1u : 0u) << a;
        // row value kinds (scratch dies below); phase M writes them for live ships
        // only, so a sunk ship's byte is stale LDS: masked to its 2-bit field
        kinds |= ((uint32_t)COLB(c.akind, a) & 3u) << (2 * a);
      }
    }
    if (valid && evpre) {  // loaded at launch (step_body)
#pragma unroll
      for (int q = 0; q < 8; q++) ev[q] = evp[q];
      rng = rngp;
    } else if (valid) {
#pragma unroll
      for (int q = 0; q < 8; q++) ev[q] = S.envi[q * E + env];  // in flight across the barrier
      rng = make_rng(P, S, env);                                 // (the draw counter too)
    }
    if (lane == 0) *claim = early ? 1 : 0;  // pass 0 is wave 1's (above)
  } else {
    quiet_moves_t<NB, NR, 1>(c, lane);
    for (int x = lane; x < P.G; x += WAVE) c.qlut[x] = (float)((double)x / (double)P.G);
  }
  prof_stamp(S, wid ? 15 : 27);  // each wave's phase-Q work done (LNW_PROF)
  __syncthreads();
  if (wid == 0) {
    prof_stamp(S, 9);
    prof_stamp(S, 14);
    prof_stamp(S, 1);
  }
  if (wid == 1 && (direct || P.no_obs)) {  // (no rows wanted: wave 1 is done)
    if (P.no_obs) return;
    // both sides' rows into their whole-slab stages, then each side's block
    // (the slab's envs, contiguous in HBM) leaves as full coalesced lines; the
    // next slab's window records are loaded before this slab's stores
    constexpr int SS = stage_stride(NB), SE = WAVE / NB;
    const int my_l = lane / NB, kl = lane - my_l * NB;
    float *st_b = c.qbig, *st_r = c.qbig + (SL ? SE : P.epw) * NB * SS;  // (lds_layout's qbig_rows)
    constexpr int N4 = WAVE * (4 * NB + 52) / 4;
    // slab 0 (every launch of this mode), then slab 1 (64 / NB < nenv): written
    // out, not as a loop, so no window-record array is carried around one
    const int ns0 = SL ? min(SE, nenv) : nenv;
    if (my_l < ns0) {
      row_regs_t<NB>(c, duct_col, my_l, kl, 0, v, w48, st_b + lane * SS, c.qlut);
      row_regs_t<NB>(c, duct_col, my_l, NB + kl, NB, vr, wr48, st_r + lane * SS, c.qlut);
    }
    wave_lds_sync();
    prof_stamp(S, 28);  // rows staged (LNW_PROF)
    const bool two = SL && nenv > SE;  // (SL: the two-slab instantiation)
    if (SL && two) {  // slab 1's window records, in flight across slab 0's stores
      const int my_e = SE + my_l;
      const bool mine = my_e < nenv;
      load_window(S, mine ? window_rec(P, c, kl, my_e) : 0, v, w48);
      load_window(S, mine ? window_rec(P, c, NB + kl, my_e) : 0, vr, wr48);
    }
    if (obs_b) copy_side_t<NB, N4, false>(st_b, obs_b, S.dummy, ns0, env0, P.store_wt);
    if (obs_r) copy_side_t<NB, N4, false>(st_r, obs_r, S.dummy, ns0, env0, P.store_wt);
    if (SL && two) {
      wave_lds_sync();  // (slab 1's rows overwrite the stages)
      const int ns1 = nenv - SE;
      if (my_l < ns1) {
        row_regs_t<NB>(c, duct_col, SE + my_l, kl, 0, v, w48, st_b + lane * SS, c.qlut);
        row_regs_t<NB>(c, duct_col, SE + my_l, NB + kl, NB, vr, wr48, st_r + lane * SS, c.qlut);
      }
      wave_lds_sync();
      if (obs_b) copy_side_t<NB, N4, false>(st_b, obs_b, S.dummy, ns1, (long long)env0 + SE, P.store_wt);
      if (obs_r) copy_side_t<NB, N4, false>(st_r, obs_r, S.dummy, ns1, (long long)env0 + SE, P.store_wt);
    }
    prof_stamp(S, 5);
    return;
  }
  if (wid == 0 && direct && spread) {
    quiet_tail_spread_t<NB, NR>(P, S, c, lane, env0, nenv, ev, rng, kinds, actions, rew_b, rew_r,
                                done_out, cog_out);
    prof_stamp(S, 3);
    return;
  }
  if (wid == 0 && valid)  // lanes past the last env of a partial workgroup idle here
    quiet_tail_env_t<NB, NR>(P, S, c, lane, env, ev, rng, moved, kinds, actions, rew_b, rew_r, done_out,
                             cog_out);
  if (wid == 0) prof_stamp(S, 3);
  if (direct || P.no_obs) return;  // wave 1 has stored every row (or none is wanted)
  quiet_emit_t<NB, NR>(P, S, c, duct_col, claim, wid ? c.qstage0 : c.qstage1, obs_b, obs_r, env0,
                       nenv, v, w48, wid == 1 && early ? 0 : -1);
  if (wid == 1) prof_stamp(S, 5);
}

// UN units per workgroup (step_kernel<.., UN>, full 64-env units): the quiet
// units' observation passes (16 per unit: 8 envs x one side each) are served
// from one workgroup-wide counter by every wave of every quiet unit, the row
// inputs read from the pass's own unit's LDS block (final after the phase-Q
// barrier; the tails running meanwhile touch none of them), each wave staging
// through its own unit's stage.
template <int NB, int NR, int UN>
__device__ __forceinline__ void quiet_emit_units_t(const KParams &P, const KState &S, char *lds_base,
                                                   const LdsLayout &L, int lstride, int *ushare,
                                                   double (*duct_all)[WAVE], float *stage, float *obs_b,
                                                   float *obs_r, int envbase) {
  static_assert(NB == NR, "templated obs rows assume equal team sizes");
  constexpr int NS = NB, ROWS = QEPG * NS, NPU = 2 * (WAVE / QEPG);
  constexpr int N4 = ROWS * (4 * NS + 52) / 4;
  const int lane = threadIdx.x & (WAVE - 1);
  const uint32_t qm = (uint32_t)ushare[0];
  const int total = __popc(qm) * NPU;
  const int G = P.G;
  const int my_e = lane / NS, kl = lane - my_e * NS;
  const bool builder = lane < ROWS;
  WinRec v;  // the row's byte record: 16 registers live across the copy-out
  auto unit_of = [&](int p, int &lp) {
    const int k = p / NPU;
    lp = p - k * NPU;
    uint32_t m = qm;
    for (int i = 0; i < k; i++) m &= m - 1;
    return __ffs((int)m) - 1;
  };
  auto next_pass = [&]() {
    int p = 0;
    if (lane == 0) p = atomicAdd(&ushare[1], 1);
    return __shfl(p, 0);
  };
  auto prefetch = [&](int pass) {  // the row's window record (dead rows read cell 0's, ignored)
    int lp;
    const int u = unit_of(pass, lp);
    const Cols cu = carve(lds_base + u * lstride, L);
    int off = 0;
    if (builder) {
      const int el = (lp >> 1) * QEPG + my_e, k = (lp & 1) * NB + kl;
      if (cu.alive0[k * PADB + el]) {
        const uint32_t p = cu.pos_cur[k * PAD + el];
        off = ((cu.type[k * PADB + el] == T_LS ? G * G : 0) + pos_x(p) * G + pos_y(p));
      }
    }
    load_win(S.winf, G, off, v);
  };
  int pass = next_pass();
  if (pass < total) prefetch(pass);
  while (pass < total) {
    int lp;
    const int u = unit_of(pass, lp);
    const Cols cu = carve(lds_base + u * lstride, L);
    const int side = lp & 1, g = lp >> 1;
    if (builder)
      row_regs_bytes_t<NS>(cu, duct_all[u], g * QEPG + my_e, side * NB + kl, side * NB, v,
                           stage + lane * stage_stride(NS), cu.qlut);
    wave_lds_sync();
    const int next = next_pass();
    if (next < total) prefetch(next);  // before this pass's stores (vmcnt is in issue order)
    float *out = side ? obs_r : obs_b;
    if (out) copy_side_t<NS, N4, false>(stage, out, S.dummy, QEPG, (long long)envbase + u * WAVE + g * QEPG, P.store_wt);
    wave_lds_sync();
    pass = next;
  }
}

// A quiet unit's step (UN > 1): phase Q split over the unit's two waves, the
// unit marked quiet, the workgroup-wide barrier (loud units pass it right
// after their quiet test), wave 0's tail, then the shared stream.
template <int NB, int NR, int UN>
__device__ __forceinline__ void quiet_step_units_t(const KParams &P, const KState &S, Cols &c, char *lds_base,
                                                   const LdsLayout &L, int lstride, int unit, int lane,
                                                   int env, int wid, double (*duct_all)[WAVE], int *ushare,
                                                   void *actions, float *obs_b, float *obs_r, float *rew_b,
                                                   float *rew_r, int32_t *done_out, float *cog_out, int env0,
                                                   bool valid) {
  constexpr int A = NB + NR;
  const long long E = P.E;
  uint32_t moved = 0, kinds = 0;
  int ev[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  Rng rng{};
  if (wid == 0) {
    quiet_moves_t<NB, NR, 0>(c, lane);
#pragma unroll
    for (int a = 0; a < A; a++) {
      moved |= (COLW(c.pos_new, a) & 0x80000000u ? 1u : 0u) << a;
      kinds |= ((uint32_t)COLB(c.akind, a) & 3u) << (2 * a);  // (wave 1's stage aliases both; sunk: stale)
    }
    if (valid) {
#pragma unroll
      for (int q = 0; q < 8; q++) ev[q] = S.envi[q * E + env];
      rng = make_rng(P, S, env);
    }
    if (lane == 0) atomicOr(&ushare[0], 1 << unit);
  } else {
    quiet_moves_t<NB, NR, 1>(c, lane);
    for (int x = lane; x < P.G; x += WAVE) c.qlut[x] = (float)((double)x / (double)P.G);
  }
  __syncthreads();
  if (wid == 0) {
    prof_stamp(S, 9);
    prof_stamp(S, 14);
    prof_stamp(S, 1);
    if (valid)
      quiet_tail_env_t<NB, NR>(P, S, c, lane, env, ev, rng, moved, kinds, actions, rew_b, rew_r, done_out,
                               cog_out);
    prof_stamp(S, 3);
  }
  if (!P.no_obs)
    quiet_emit_units_t<NB, NR, UN>(P, S, lds_base, L, lstride, ushare, duct_all, wid ? c.qstage0 : c.qstage1,
                                 obs_b, obs_r, env0 - unit * WAVE);
  if (wid == 1) prof_stamp(S, 5);
}
