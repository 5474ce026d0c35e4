// lnw_turn.inc — one ship's turn of step_body's phase S (Game.step's agent loop,
// game.py:338-381: take_action, get_obs, calculate_reward), included as text at
// the two places that play it: the body of the `turn` lambda of the split
// contact kernel, and the body of the agent loop of every other instantiation.
// It is a fragment, not a function: as a __forceinline__ function template the
// same statements compile, but the scalar register allocation moves and four
// step kernels pass the spill bounds the tests pin (DESIGN.md, "Where the game
// rules live").
//
// Names it expects in scope:
//   template parameters  ST, CW, REFW, NB, NR
//   constants            P (KParams), S (KState), E, A, nb, dt (P.act_dtype),
//                        env, lane, actions
//   the ship             a (its index in turn order)
//   the view             X (Ctx: rng, step, the pair tables) and c (the Cols it
//                        plays on: X.c)
//   the env's totals     N (Neut), ev[8], hits[2], bsx, bsy, nbp, rsx, rsy, nrp
//   LNW_PROF             tp[4], t0
// The lambda's parameters and locals shadow the loop state of the same names on
// purpose, so that this text updates whichever of the two is in scope.
// LNW_DEBUG_SKIP bits tested here: 16 (no fire), 7 (no get_obs), 8 (no reward).
const bool al = COLB(c.alive0, a) != 0;  // sunk ships skip their turn (reward 0)
const int side = a >= nb;
bool engage = false, moved = false;
int destroyed = 0;
t0 = prof_now(S);
if (al) {
  uint32_t p0 = COLW(c.pos_cur, a);
  if (!side) {
    if (P.side_blue) { bsx += pos_x(p0); bsy += pos_y(p0); nbp++; }
  } else {
    rsx += pos_x(p0); rsy += pos_y(p0); nrp++;
  }
  size_t row = ((size_t)env * A + a) * 4;
  double a0 = COLW(c.act0, a), a1 = COLW(c.act1, a);
  int kind = COLB(c.akind, a);
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
  double engagement = P.discrete ? rint(a1) : a1;
  int keng = P.discrete ? K_PYINT : kind;
  int mk = COLB(c.mkind, a);
  // the salvo threshold, salvo_size's rule (combatant.py:528) spelled out: through
  // the helper the 4v4 contact kernel without the split measured slower (DESIGN.md,
  // "Where the game rules live"); a change to the rule is made there and here
  double thr_v;
  if (kind_promote(keng, mk) == K_F32)
    thr_v = (double)rintf((float)engagement * (float)COLB(c.miss_cur, a));
  else
    thr_v = rint(engagement * (double)COLB(c.miss_cur, a));
  // round(nan/inf) of engagement * missiles raises (combatant.py:528): flagged, no engagement
  if (!isfinite(thr_v)) { X.rng.err |= LNW_ERRF_NAN_ROUND; thr_v = 0.0; }
  engage = thr_v > 0.0;
  int tn = (int)COLW(c.tcnt, a);
  if (engage && tn > 0 && !(P.dbg_skip & 65536)) {  // (bit 16: diagnostics, no fire)
    const uint16_t *tl = S.tl + (size_t)a * P.T * E + env;
    if constexpr (CW) {
      // contact variant: the list read 8 entries at a time, the loads of a
      // chunk in flight together (packed in a register pair: a runtime index
      // into a register array would put it in scratch)
      for (int q0 = 0; q0 < tn; q0 += 8) {
        uint64_t pk0 = 0, pk1 = 0;
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const uint64_t v = q0 + u < tn ? (uint64_t)tl[(size_t)(q0 + u) * E] : 0ull;
          if (u < 4) pk0 |= v << (16 * u);
          else pk1 |= v << (16 * (u - 4));
        }
        const int nq = tn - q0 < 8 ? tn - q0 : 8;
        for (int u = 0; u < nq; u++) {
          const uint16_t tg = (uint16_t)((u < 4 ? pk0 : pk1) >> (16 * (u & 3)));
          if (fire_dev(X, a, tg & 0xff, tg >> 8, engagement, keng, N)) destroyed++;
        }
      }
    } else {
      uint16_t nx = tl[0];  // the next target's load is in flight while one fires
      for (int q = 0; q < tn; q++) {
        const uint16_t tg = nx;
        if (q + 1 < tn) nx = tl[(size_t)(q + 1) * E];
        if (fire_dev(X, a, tg & 0xff, tg >> 8, engagement, keng, N)) destroyed++;
      }
    }
  }
  if (side) ev[6] += destroyed; else ev[5] += destroyed;
  if (!isfinite(a0)) { X.rng.err |= LNW_ERRF_NAN_ROUND; COLW(c.radar_cur, a) = 0; }
  else {  // (two statements: as one, three kernels swap an s_and_b64's operands)
    int rr = radar_setting(a0);
    COLW(c.radar_cur, a) = rr;
  }
  uint32_t pn = COLW(c.pos_new, a);
  moved = (pn & 0x80000000u) != 0;
  if (moved) COLW(c.pos_cur, a) = pn & 0x7fffffffu;
}
tp[0] += prof_now(S) - t0;
t0 = prof_now(S);
if (al && !(P.dbg_skip & 128)) {
  if constexpr (REFW) march_pairs_ref(X, a);
  if constexpr (ST) {
    if (!side) get_obs_t<NB, NR, CW>(X, a, 0, NB);
    else get_obs_t<NR, NB, CW>(X, a, NB, 0);
  } else {
    get_obs_dev(X, a);
  }
}
tp[2] += prof_now(S) - t0;
t0 = prof_now(S);
double r = 0.0;
if (al && !(P.dbg_skip & 256)) r = reward_dev(X, a, moved, engage, destroyed);
COLW(c.reward, a) = r;
if (al) {
  if (!side) {
    if (P.side_blue ? destroyed > 0 : engage) COLB(c.eng, a) = 1;
  } else {
    if (!P.trained_red ? engage : destroyed > 1) COLB(c.eng, a) = 1;
  }
  hits[side] += destroyed;
}
tp[3] += prof_now(S) - t0;
