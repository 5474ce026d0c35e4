/*
 * lnw.h — C-ABI of the MI355X-native batched littoral-warfare environment step.
 *
 * Drop-in boundary for the reference's environment API
 * (valauri/Littoral-Naval-Warfare-MARL):
 *
 *   lnw_create / lnw_load_terrain   replace Game.__init__ (game.py:107-158) and
 *                                   Game.define_grid_from_image (game.py:616-626)
 *   lnw_reset                       replaces Game.reset (game.py:528-613)
 *   lnw_step                        replaces Game.step (game.py:298-525) with
 *                                   Combatant/LandingShip.take_action
 *                                   (combatant.py:501-565, landingship.py:508-572)
 *                                   and Game.calculate_reward (game.py:214-295)
 *   lnw_observe                     replaces ship.get_obs() (combatant.py:90-233,
 *                                   landingship.py:94-239) as called by
 *                                   main.py:282, ppo.py:500, ddqn.py:296
 *   lnw_los_batch                   check_line_of_sight (combatant.py:436-456)
 *   lnw_move_batch                  continuous_to_discrete / value_to_coordinates +
 *                                   check_path / astar (combatant.py:289-489,689-704)
 *
 * Conventions
 *  - Every pointer argument named *_dev is a device pointer (HIP, gfx950); the
 *    caller owns action/observation/reward buffers, the handle owns the
 *    environment state and the terrain.
 *  - Work is enqueued on the caller's stream (hipStream_t passed as void*; NULL
 *    = the default stream). Nothing synchronises except lnw_create,
 *    lnw_load_terrain and lnw_destroy.
 *  - Every function returns 0 on success or a negative LNW_E* code; the message
 *    of the last failure on the calling thread is available from
 *    lnw_last_error(). Reference crash modes (ZeroDivisionError in an EW fix,
 *    round(nan), tape exhaustion) do not abort: they set per-environment bits in
 *    the err-flags array (LNW_ERRF_*).
 *  - A handle is not thread-safe; use one handle per device (per process).
 *
 * Layouts (E = n_envs, nb/nr = blue/red slots, A = nb+nr, D_side = 4*n_side+52,
 * or 4*n_side+28 for a side of medium ships: game.py:609-610 sizes a side's rows
 * by its fastest ship, (2*speed+1)^2 window cells):
 *  actions   [E][A][4]  f32 or f64 (continuous), or [E][A][4] i32 (discrete:
 *                       radar, salvo, move-index 0..49, unused) — mutated in
 *                       place where the reference mutates it (game.py:379)
 *  obs_blue  [E][nb][Db] f32, obs_red [E][nr][Dr] f32 (float32 of the reference's
 *                       float64 value; dead slots are zeros)
 *  rew_blue  [E][nb] f32, rew_red [E][nr] f32, done [E] i32 (1 running, 0 over),
 *  cog       [E] f32 (NaN where the reference returns None)
 *  rew_* and cog are float64 instead after lnw_set_reward_dtype(h, 1)
 */
#ifndef LNW_H
#define LNW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LNW_ABI_VERSION 5

/* status codes */
#define LNW_OK 0
#define LNW_EINVAL (-1)
#define LNW_ENOMEM (-2)
#define LNW_EDEVICE (-3)
#define LNW_ESTATE (-4)
#define LNW_EUNSUPPORTED (-5)

/* ship types (Combatant "small"/"large"/"medium", LandingShip "ls";
 * combatant.py:60-88, landingship.py:61-92, game.py:184-212) */
#define LNW_SMALL 0
#define LNW_LARGE 1
#define LNW_LS 2
#define LNW_MEDIUM 3   /* speed 2, 8 missiles, mast 30, rcs 1, 5x5 observation window */

/* action dtypes / per-row value kinds (NumPy NEP 50 semantics) */
#define LNW_ACT_F32 0      /* whole buffer float32 (np.float32 rows)            */
#define LNW_ACT_F64 1      /* whole buffer float64 (np.float64 rows)            */
#define LNW_ACT_I32 2      /* discrete integer actions (DISCRETE=true)         */
#define LNW_KIND_PYFLOAT 1 /* row_kind values for an F64 buffer: python floats */
#define LNW_KIND_F32 2     /*   np.float32 row stored widened to f64           */
#define LNW_KIND_F64 3     /*   np.float64 row                                 */

/* rng modes */
#define LNW_RNG_PHILOX 0   /* production: Philox4x32-10 keyed by (seed, global env id) */
#define LNW_RNG_TAPE 1     /* parity: per-env recorded draws                           */

/* per-env error bits */
#define LNW_ERRF_ZERODIV 1u    /* combatant.py:274 ZeroDivisionError (fix skipped) */
#define LNW_ERRF_NAN_ROUND 2u  /* round(nan/inf) in a fix or a radar action        */
#define LNW_ERRF_TAPE 4u       /* tape exhausted                                   */
#define LNW_ERRF_MISSILES 8u   /* missile count outside the 0..8 hit table         */

/* observe selectors */
#define LNW_OBS_ALL (-1)   /* every live ship, blue then red (main.py:280-333) */
#define LNW_OBS_BLUE (-2)
#define LNW_OBS_RED (-3)

typedef struct lnw_handle lnw_handle;

/* Scenario flags: the reference's config.json keys (game.py:41-53,
 * combatant.py:33-38) that change step semantics. */
typedef struct lnw_params {
    int32_t discrete;        /* overall.discrete                       */
    int32_t landing_ops;     /* overall.landing_ops                    */
    int32_t aggressive;      /* overall.tactics == "aggressive"        */
    int32_t side_blue;       /* environment_setup.side == "blue"       */
    int32_t trained_red;     /* environment_setup.trained_red          */
    int32_t move_thr;        /* environment_setup.movement_threshold   */
    int32_t ew_thr;          /* environment_setup.ew_threshold         */
    int32_t lz_x, lz_y;      /* landing zone (game.py:590): (14, 82)   */
    double red_aggression;   /* environment_setup.red_aggression       */
    /* build-side knobs (not in the reference) */
    int32_t episode_steps;   /* auto-reset horizon (0 = never)          */
    int32_t auto_reset;      /* reset an env in-kernel when done==0 or at the horizon */
    int32_t los_mode;        /* 0 = precomputed LOS table, 1 = ray march,
                                2 = table + the reference's LOS work: every
                                own x opponent ray marched in full at each
                                get_obs and discarded (diagnostics)        */
    int32_t move_mode;       /* 0 = precomputed move table, 1 = direct A*  */
} lnw_params;

/* Spawn description used by lnw_reset and by in-kernel auto-reset.
 * types[A]: LNW_SMALL/LARGE/LS/MEDIUM (medium ships only as a whole side: the
 * reference's row assignment raises for a medium ship beside speed-3 ships,
 * game.py:344 / 381, so lnw_reset refuses that with LNW_EUNSUPPORTED);
 * pos[A][2]: spawn cell; rand_ls[A] != 0 draws the
 * cell with random.randint(98,99), random.randint(48,56) (game.py:589).
 * If box_lo/box_hi are set (box_hi[0] > box_lo[0]) every agent instead spawns on
 * a random water cell of that box (a build-side "melee" scenario, drawn from a
 * separate Philox stream so the game stream is unchanged). */
typedef struct lnw_spawn {
    int32_t types[64];
    int32_t pos[64][2];
    int32_t rand_ls[64];
    int32_t box_lo[2], box_hi[2];
} lnw_spawn;

/* ---- lifecycle ---------------------------------------------------------- */
int lnw_abi_version(void);
const char *lnw_last_error(void);

/* env_id_base: global id of this handle's first env (multi-GPU sharding keys the
 * RNG by global env id so trajectories do not depend on the GPU count). */
int lnw_create(const lnw_params *params, int32_t n_envs, int32_t nb, int32_t nr, int32_t device,
               int64_t env_id_base, lnw_handle **out);
int lnw_destroy(lnw_handle *h);

/* Upload the uint8 terrain (row-major [G][G], grid[x][y]) and build the device
 * structures: radar/EW bitmask, move-feasibility table, LOS table. Synchronous.
 * Team sizes: each side 1..16 ships, except that a side of 16 against 10 or
 * more (16 v 10..16, 10..16 v 16; at G = 100 and 200 alike) is refused with
 * LNW_EUNSUPPORTED "agent count needs more LDS than a CU has": the one-lane
 * runtime kernel's step layout, which every runtime size must be able to fall
 * back to, then passes the 158 KiB (161 792 B) of dynamic LDS a workgroup can
 * have (at G = 100 / 200: 16 v 9 160 192 / 160 592 B and 15 v 15 160 960 /
 * 161 360 B load, 16 v 10 needs 161 824 / 162 224 B). The handle stays valid for
 * lnw_destroy. */
int lnw_load_terrain(lnw_handle *h, const uint8_t *grid_host, int32_t G);

int lnw_set_rng(lnw_handle *h, int32_t mode, uint64_t seed, const double *tape_dev,
                const int64_t *tape_off_dev);

/* ---- environment API ---------------------------------------------------- */
/* env_mask_dev: [E] u8, nonzero = reset that env (NULL = all).
 * pos_dev: optional [E][A][2] i32 per-env spawn cells (overrides spawn->pos). It is
 * copied into the handle (stream-ordered), and the in-kernel auto-reset
 * (lnw_params.auto_reset) respawns every env on its own cells from then on; a
 * reset without pos_dev returns all envs to the shared spawn->pos. */
int lnw_reset(lnw_handle *h, const uint8_t *env_mask_dev, const lnw_spawn *spawn,
              const int32_t *pos_dev, void *stream);

/* obs_blue_dev and obs_red_dev both NULL: no observation rows are written
 * (the MAPPO rollout discards step()'s observations, ppo.py:577, and observes
 * afresh); every other effect of the step is unchanged. One NULL alone is
 * LNW_EINVAL. */
int lnw_step(lnw_handle *h, void *actions_dev, int32_t action_dtype, const uint8_t *row_kind_dev,
             float *obs_blue_dev, float *obs_red_dev, float *rew_blue_dev, float *rew_red_dev,
             int32_t *done_dev, float *cog_dev, void *stream);

/* K consecutive Game.step calls whose action arrays the caller has ahead of
 * time (an open-loop action sequence: scripted or replayed agents, benchmark
 * actions) — no reference counterpart beyond K calls of Game.step; results are
 * exactly those of K lnw_step calls, step k reading actions_dev + k *
 * seq->act_step elements (and row kinds + k * kind_step bytes) and writing its
 * outputs at the output pointers + k * the output strides (elements; a stride
 * 0 makes every step write the same rows, each step's outputs replacing the
 * previous step's as K separate calls would). It makes the K lnw_step
 * launches itself, back to back on the caller's stream. */
typedef struct lnw_seq {
  int32_t steps;               /* K >= 1 */
  int64_t act_step, kind_step; /* action elements / row-kind bytes between steps */
  int64_t obs_blue_step, obs_red_step, rew_blue_step, rew_red_step, done_step, cog_step;
} lnw_seq;
int lnw_step_seq(lnw_handle *h, const lnw_seq *seq, void *actions_dev, int32_t action_dtype,
                 const uint8_t *row_kind_dev, float *obs_blue_dev, float *obs_red_dev, float *rew_blue_dev,
                 float *rew_red_dev, int32_t *done_dev, float *cog_dev, void *stream);

/* agent >= 0: that agent (blue 0..nb-1, red nb..A-1) in every env;
 * LNW_OBS_ALL / LNW_OBS_BLUE / LNW_OBS_RED: every live ship of the selection,
 * in list order. Side effects as the reference (target lists, RNG draws). */
int lnw_observe(lnw_handle *h, int32_t agent, float *obs_blue_dev, float *obs_red_dev,
                void *stream);
/* lnw_observe with the rows of env e at obs + e * stride (floats; 0 = the
 * packed n * D; else a multiple of 4, at least n * D) and NULL for a side whose
 * rows nobody reads (its get_obs calls and their side effects still run):
 * the MAPPO rollout observes straight into its buffer (ppo.py:497-575). */
int lnw_observe_ex(lnw_handle *h, int32_t agent, float *obs_blue_dev, int64_t blue_env_stride,
                   float *obs_red_dev, int64_t red_env_stride, void *stream);

/* ---- state access (tests, facade, checkpoint) --------------------------- */
#define LNW_F_POS 0        /* [A][E] u32: x | y<<16                          */
#define LNW_F_RADAR 1      /* [A][E] i32                                     */
#define LNW_F_MISSILES 2   /* [A][E] u8  missile count                       */
#define LNW_F_MKIND 3      /* [A][E] u8  value kind of the missile count     */
#define LNW_F_ALIVE 4      /* [A][E] u8  list slot is not None               */
#define LNW_F_TYPE 5       /* [A][E] u8                                      */
#define LNW_F_STEPS 6      /* [A][E] i32 ship.steps_done                     */
#define LNW_F_DIST_LZ 7    /* [A][E] f64 LandingShip.distance_to_landing_zone */
#define LNW_F_TL_CNT 8     /* [A][E] u16 len(target_list)                    */
#define LNW_F_TL 9         /* [A][T][E] u16 x | y<<8                         */
#define LNW_F_DUCT 10      /* [E] f64                                        */
#define LNW_F_ENV 11       /* [8][E] i32: n_blue_left, n_red_left, steps_done,
                              blue_victory, red_victory, blue_engagements,
                              red_engagements, episode                      */
#define LNW_F_RNG 12       /* [E] u64 Philox counter or tape cursor          */
#define LNW_F_ERR 13       /* [E] u32 LNW_ERRF_* bits                        */
#define LNW_NFIELDS 14

/* Device pointer and byte size of one state field (valid until lnw_destroy). */
int lnw_state_field(lnw_handle *h, int32_t field, void **dev_ptr, int64_t *nbytes);

/* Whole-state snapshot (SURVEY.md §8(b) lnw_get_state / lnw_set_state; the
 * reference has no counterpart: its state is the Game object itself, and
 * checkpointing it means pickling that object). A snapshot holds every state
 * field above, the spawn spec and per-env spawn cells the in-kernel auto-reset
 * reads, the RNG mode and seed, and a header naming the handle's shape and a
 * hash of its terrain. lnw_set_state restores it into any handle of the same
 * shape (envs, team sizes, grid) and terrain — the same one later, or a fresh
 * one — after which stepping continues exactly as the saved handle would have.
 * A tape-mode snapshot restores the tape cursors only: bind the same tape with
 * lnw_set_rng first. dst / src: host or device memory of at least
 * lnw_state_bytes(h) bytes. Both wait for `stream` and copy synchronously. */
int64_t lnw_state_bytes(lnw_handle *h);
int lnw_get_state(lnw_handle *h, void *dst, int64_t nbytes, void *stream);
int lnw_set_state(lnw_handle *h, const void *src, int64_t nbytes, void *stream);

/* The step kernel the last lnw_step launched (build-side launch shape, no
 * reference counterpart; tests use it to know which code path they checked). */
#define LNW_KERNEL_NONE 0
#define LNW_KERNEL_GENERIC 1       /* one lane per env, runtime team sizes         */
#define LNW_KERNEL_TEAM 2          /* 2v2/3v3/4v4, one unit (<= 64 envs) per workgroup */
#define LNW_KERNEL_TEAM_CONTACT 3  /* the same, contact variant (lnw_set_variant)  */
#define LNW_KERNEL_UNITS 4         /* 4v4 headline: four 64-env units per workgroup */
#define LNW_KERNEL_GROUP 5         /* runtime team sizes, 16 lanes per env         */
#define LNW_KERNEL_REFLOS 6        /* los_mode 2 (the reference's LOS work)        */
int lnw_step_kernel(lnw_handle *h);
/* 1 when the last lnw_step launched the units kernel compiled for the
 * production configuration (step_units_prod_kernel: grid side 100, float32
 * actions without row kinds, table LOS and moves, Philox draws, float32
 * rewards, write-through rows, no diagnostics bound), 0 when it launched any
 * other kernel. lnw_step_kernel reports LNW_KERNEL_UNITS for both units
 * kernels; their results are the same bit for bit. */
int lnw_step_kernel_prod(lnw_handle *h);
/* Target-list capacity T per agent (= max(nb,nr) + max(nb,nr)^2, never overflows). */
int lnw_tlist_cap(lnw_handle *h);
/* Environments per workgroup of the step / observe launches (build-side launch
 * shape, no reference counterpart). epw = 0 restores the automatic choice made
 * by lnw_load_terrain: 64 (one env per lane) unless E is too small to fill the
 * GPU, then fewer per workgroup. 1 <= epw <= 64 forces it (results do not depend
 * on it; tests use it to cover both launch shapes). Every value in 1..64 is
 * supported, powers of two or not (the automatic choice only makes powers of
 * two); no value in that range is refused, anything else is LNW_EINVAL. The
 * quiet path's form follows from it: rows written directly by wave 1 up to
 * 64 / nb envs (4v4: up to 128 / nb in two slabs), staged passes above, the
 * units kernel at 64 ("The quiet predicate at sensor reach"). The
 * LNW_EPW_RT environment variable (1..64) overrides the automatic choice the
 * same way. Returns the epw in force, or a negative LNW_E* code. */
int lnw_set_epw(lnw_handle *h, int32_t epw);

/* Step-kernel code variant for 2v2 / 3v3 / 4v4 (build-side, no reference
 * counterpart; results are identical either way). contact = 0 (default): the
 * variant tuned for envs whose fleets are mostly out of sensor range (the
 * quiet-workgroup path, BASELINE's reference spawns). contact = 1: get_obs
 * pair walk as bit masks over registers and two EW bearings per iteration,
 * faster when fleets are in contact every step (melee, MAPPO rollouts against
 * a closing red) but slower on the quiet path, which shares the kernel. */
int lnw_set_variant(lnw_handle *h, int32_t contact);

/* Work counters (diagnostics, no reference counterpart): while bound, the step
 * and observe kernels add to counters_dev[0] the LOS rays they ray-march
 * (queries outside the LOS table, or every query with los_mode = 1), to [1] the
 * Bresenham cells those rays visit (combatant.py:411-456) and to [2] the A*
 * searches they run (targets outside the move table, or move_mode = 1;
 * combatant.py:289-408), to [3] the EW bearings evaluated pooled across lanes:
 * by the contact variant in wave-pooled rounds (get_obs calls whose busiest
 * lane has more than two), by the group kernel (runtime team sizes) every
 * bearing of an opponent that gets a fix (spread over the env's 16 lanes).
 * counters_dev: [4] uint64 device array, or NULL to unbind. Costs one uniform
 * branch per march / search / pooled get_obs while unbound. */
int lnw_set_counters(lnw_handle *h, uint64_t *counters_dev);

/* Reward / cog output type of lnw_step. f64 = 0 (default): rew_blue, rew_red and
 * cog are float32 arrays; f64 = 1: they are float64 arrays (pass double* cast to
 * float*), the exact values the reference returns as Python floats
 * (game.py:214-295, 507-525) rather than their float32 rounding. */
int lnw_set_reward_dtype(lnw_handle *h, int32_t f64);

/* ---- unit kernels (parity tests, standalone use) ------------------------ */
/* LOS (radar thr = move_thr; EW thr): out[i] = bit0 radar clear | bit1 EW clear
 * for pairs[i] = (x1, y1, x2, y2), traced from (x1,y1) to (x2,y2); every cell of
 * the pairs must lie on the G x G grid. Rays march from the grid's 2-bit mask
 * staged in LDS per workgroup (G <= 512, pairs_dev 8-byte aligned), else from
 * HBM. */
int lnw_los_batch(const uint8_t *grid_dev, int32_t G, const int16_t *pairs_dev, int64_t n,
                  int32_t move_thr, int32_t ew_thr, uint8_t *out_dev, void *stream);
/* A*: plen[i] (-1 = None), kind[i] (0 goal, 1 timeout, 2 none), feasible[i]
 * (check_path) for ship type types[i] from start[i] to target[i]. */
int lnw_astar_batch(const uint8_t *grid_dev, int32_t G, int32_t move_thr, const int8_t *types_dev,
                    const int16_t *start_dev, const int16_t *target_dev, int64_t n,
                    int16_t *plen_dev, int8_t *kind_dev, uint8_t *feasible_dev, void *stream);
/* Continuous move target: rounded (x,y) and feasibility (can_move_to && check_path)
 * through the handle's structures (table or direct A* per params.move_mode). */
int lnw_move_batch(lnw_handle *h, const int8_t *types_dev, const int16_t *pos_dev,
                   const double *act_dev /* [n][2] */, const uint8_t *is_f32_dev, int64_t n,
                   int32_t *rounded_dev, uint8_t *ok_dev, void *stream);
/* check_path(start, target) through the handle's move table (params.move_mode 0,
 * targets within +-4) or the A* replica. start must lie inside the grid. */
int lnw_path_query(lnw_handle *h, const int8_t *types_dev, const int16_t *start_dev,
                   const int16_t *target_dev, int64_t n, uint8_t *out_dev, void *stream);
/* The handle's LOS query (table or march per params.los_mode). Together with
 * params.los_mode = 1 (every query marched) and 2 (the reference's full
 * own x opponent LOS work inside the step), this is what SURVEY.md §8(b)'s
 * lnw_debug_los (the full unpruned LOS matrix) was to provide: any pair set
 * can be queried through the step's own LOS path, bit-exact with
 * check_line_of_sight (combatant.py:436-456). */
int lnw_los_query(lnw_handle *h, const int16_t *pairs_dev, int64_t n, uint8_t *out_dev,
                  void *stream);

/* Stream-ordered byte copy (device<->device/host), for state access. */
int lnw_copy(void *dst, const void *src, int64_t nbytes, void *stream);

/* Philox U[0,1) float32 fill keyed by (seed, offset + i): synthetic actions. */
int lnw_fill_uniform_f32(float *out_dev, int64_t n, uint64_t seed, uint64_t offset,
                         void *stream);

/* ---- analytics side channels ----------------------
 * Device counterparts of Game.heatmap / coldmap / launch_sites / engagements /
 * blue_ew / red_ew (game.py:119-154; written at combatant.py:640-657 and
 * 146-150), accumulated over every env and step while bound. Each pointer may
 * be NULL (that channel is off); lnw_set_analytics(h, NULL) turns all off.
 * Maps are indexed [x * 100 + y] like the reference's 100x100 arrays (cells
 * outside them are skipped). Log records are 4 x uint32:
 *   engagement: env, step | side << 16 | missiles << 24, shooter x | y << 16,
 *               target x | y << 16          (every hit; missiles 0 = main gun)
 *   EW fix:     env, step | side << 16, observer x | y << 16,
 *               (uint16)fix_x | (uint16)fix_y << 16   (every finite EW fix)
 * with env the global env id, step the episode step (0-based) and side 0 blue /
 * 1 red. *_count are incremented atomically per record; records past *_cap are
 * counted but not stored. */
typedef struct lnw_analytics {
  uint32_t *heatmap;   /* [100*100] shooter cells of missile hits by the params.side side */
  uint32_t *coldmap;   /* [100*100] target cells of those hits */
  uint32_t *launch;    /* [2][100*100] missile-hit launch cells (blue, red) */
  uint32_t *eng_log;   /* [eng_cap][4] */
  uint32_t *eng_count; /* [1] */
  int64_t eng_cap;
  uint32_t *ew_log;    /* [ew_cap][4] */
  uint32_t *ew_count;  /* [1] */
  int64_t ew_cap;
} lnw_analytics;
int lnw_set_analytics(lnw_handle *h, const lnw_analytics *a);

/* ---- batched policy forward -------------------------
 * The convolutional head and LayerNorm of the reference actor (network.py:70-85:
 * conv 1->5, BatchNorm, ReLU, 2x2 max pool, conv 5->8, BatchNorm, ReLU, pool,
 * linear 8->12, LayerNorm over [head, obs[49:]]) for B observation rows of
 * obs_dim floats (the first 49 are the 7x7 window): out[B][n_in], n_in =
 * obs_dim - 37 (<= 64). params: 578 + 2 n_in floats packed by
 * lnw.rollout.BatchedActor.packed_features(). bn_running 0: per-row BatchNorm
 * statistics (the reference's training-mode one-state calls), 1: running. */
int lnw_actor_features(const float *params_dev, int32_t obs_dim, const float *obs_dev, int64_t B,
                       int32_t bn_running, float *out_dev /* [B][n_in] */, void *stream);

/* ---- fused rollout step of the MAPPO caller -----
 * lnw_policy_act replaces, per step and side, the reference rollout's actor
 * calls (ppo.py:497-575: MLP.forward per live ship, network.py:70-115, or
 * MLP.get_dist :117-152 for given actions) and the assembly of the action
 * array (ppo.py:515-577), for every env at once: conv head + LayerNorm + tanh
 * MLP + Normal heads, a keyed Philox sample clamped to [0, 1] (+ N(0, noise)),
 * its log-probability, then the f64 rows lnw_step takes (sunk ships 0), the
 * rollout buffer rows, scripted red rows (red_steps*.csv, ppo.py:560-566) and
 * the rows' value kinds (np.asarray of the step's rows, ppo.py:577).
 * params: BatchedActor.packed_policy() (lnw/rollout.py). One launch. */
typedef struct lnw_policy_args {
  const float *obs;            /* [E][n][D] this side's observation rows (16-B aligned) */
  int64_t E;
  int32_t n, D, own0, A;       /* ships of the side, row length, first agent slot, agents per env */
  const float *params;
  int32_t bn_running;          /* 0: per-row BatchNorm statistics (training-mode batch-1 calls) */
  int32_t forced;              /* 1: log-probabilities of forced_act (get_dist), no sampling */
  const float *forced_act;     /* rows of 4 floats: env e ship i at [e * fa_env_stride + 4 i] */
  int64_t fa_env_stride;
  float noise;                 /* > 0: + noise * N(0, 1) before the clamp */
  uint64_t seed;               /* keyed draws: Philox(seed) at slot (call * T + t) * 4 + which */
  const int64_t *call_dev;     /* rollout index, read on the device (NULL = 0) */
  int32_t T, t, which;
  int64_t row_base;            /* global id of row 0 (env_id_base * n) */
  const uint8_t *alive;        /* [A][E] the handle's LNW_F_ALIVE field */
  const uint8_t *live;         /* [E] episode still running (NULL: all) */
  float *obs_out;              /* NULL, or rollout rows: env e at obs_out + e * obs_env_stride */
  int64_t obs_env_stride;
  float *act_out, *logp_out;   /* NULL, or rollout rows of 4: env e ship i at e * act_env_stride + 4 i */
  int64_t act_env_stride;
  double *full;                /* [E][A][4] action array of lnw_step (this side's rows), or NULL */
  const double *script;        /* NULL, or scripted rows [script_n][script_steps][4] */
  int32_t script_n, script_steps, script_own0, script_cnt;
  uint8_t *kinds;              /* NULL, or [E][A] row kinds for lnw_step */
  int32_t kinds_f32_all_alive; /* 1: LNW_KIND_F32 rows when every ship is alive, else F64 */
  uint8_t *f32_out;            /* NULL, or env e at f32_out[e * f32_env_stride]: the rows are F32 */
  int64_t f32_env_stride;
  int64_t obs_in_env_stride;   /* floats between envs' rows in obs (0: n * D). obs_out == obs with
                                  obs_env_stride == this stride: the rows already sit in the rollout
                                  buffer (lnw_observe_ex wrote them there), and only the rows of
                                  envs whose episode ended (live == 0) are zeroed in place */
  int32_t script_self;         /* != 0: this launch's own rows are scripted (the reference's warm-up
                                  of a learning red side, ppo.py:552-557). Ship i takes the row
                                  script[(i * script_steps + t) * 4 ..]; a row past the table (i >=
                                  script_n or t >= script_steps) is zeros. full gets the float64 row
                                  as it stands in the table (zeros for a sunk ship), act_out the row
                                  rounded to float32 and logp_out its log-probability under params
                                  (get_dist, as forced: no NaN guard), both zeros for rows not kept
                                  (!alive or !live). No keyed draw is consumed and T is not read.
                                  Needs script (32-B aligned); LNW_EINVAL together with forced.
                                  script_own0 / script_cnt keep their meaning (the other side's rows,
                                  written by the lane of ship 0) and may be used in the same launch;
                                  obs_out, kinds, f32_out, live and alive behave as without it.
                                  Appended last: zero-initialised callers see no change */
} lnw_policy_args;
int lnw_policy_act(const lnw_policy_args *args, void *stream);

/* ---- parameter-noise exploration: a population of actors in one rollout ------
 * The reference explores by parameter noise (ppo.py:452-482, 669): every rollout
 * episode reloads the noiseless actor and adds clamp(N(0, noise_ratio), -clip,
 * +clip) to each actor parameter whose name holds none of norm1, norm2,
 * layernorm; the episode's actions and old log-probabilities come from that
 * actor. Here the envs of a rollout are split into members of G consecutive
 * global envs (member m = global envs [m G, (m + 1) G); G = 1 is the reference:
 * one noised actor per episode), lnw_actor_perturb writes every member's packed
 * parameter set once per rollout, and lnw_policy_act_pop acts for each env with
 * its member's set.
 *
 * Flat actor vector (P = lnw_ppolearn_args' actor layout, P = 7139 + 66 n_in
 * floats, n_in = D - 37): the conv head / LayerNorm block in
 * BatchedActor.packed_features()'s order, then fc1 w [64][n_in], b; fc2 w, b;
 * fc3 w, b; normal_head w [4][32]; log_std_head w [4][32]; logstd.
 * Packed set (lnw_policy_packed_floats(D) floats, what lnw_policy_act reads and
 * BatchedActor.packed_policy() produces): that block zero-padded to a multiple
 * of 4 floats; b1 [64], b2 [64], b3 [32]; then per layer (fc1 with n_in zero-
 * padded to 32 columns, 64 when n_in > 32; fc2; fc3; the heads: normal rows
 * 0-3, log-std rows 4-7, zero rows to 16) three planes hi, mid, lo of bfloat16
 * x 8 [n-tile][k-pair p][lane], element j = W[16 nt + lane % 16][32 p + 16 (j /
 * 4) + 4 (lane / 16) + j % 4], w = hi + mid + lo exactly (each term rounded to
 * nearest).
 *
 * Member m's parameters: theta_m = theta + mask * clamp(sigma * z_m, -clip,
 * +clip), in float32 in that order (ppo.py:474-475).
 *   mask: 1 on conv1, conv2, convhead, fc1, fc2, fc3 weights and biases and on
 *     the two head weights; 0 on norm1.*, norm2.* (running statistics included),
 *     layernorm.* and the logstd slot (the reference noises logstd too; nothing
 *     ever reads it, and the packed set does not hold it).
 *   z_m[k], k < P: the keyed standard normal of flat index k (masked ones are
 *     drawn and discarded), keyed_normal(row0 = m, rows = 1, cols = P, seed, slot)
 *     of lnw/rollout.py: the uniforms lnw_fill_uniform_f32(seed) holds at
 *     (slot << 40) + 2 P m + k and + P + k, through Box-Muller.
 *   slot = (call * T) * 4 + 3, call read from call_dev (NULL = 0): a rollout's
 *     action draws use slots (call * T + t) * 4 + which with which 0 (blue
 *     sample), 1 (blue action noise) and 2 (red sample), and which = 3 only for
 *     the action noise of a learning red actor (noise > 0 at which = 2), which
 *     lnw.rollout.Rollout refuses at step 0 beside parameter noise: which = 3 of
 *     step 0 is free. (member0 + members) * 2 P must stay below 2^40.
 *   sigma = noise_dev[0], clip = noise_dev[1], read on the device, so a captured
 *     graph follows in-place updates of the schedule. noise_dev == NULL or sigma
 *     == 0: theta_m = theta bit for bit (an exact repack, no draws).
 * theta_member_stride != 0: member k (local) reads its own vector at theta + k *
 * theta_member_stride instead of sharing one. One launch, no atomics, no host
 * synchronisation, bitwise reproducible; 0 B of scratch. */
typedef struct lnw_actor_perturb_args {
  const float *theta;          /* flat actor vector(s), see above */
  int64_t theta_member_stride; /* floats between the members' vectors (>= P), or 0: one for all */
  int32_t D;                   /* observation row length (limits as lnw_policy_act) */
  int32_t T;                   /* rollout steps (the slot); > 0 with noise_dev */
  int64_t member0, members;    /* global id of the first member written, how many */
  float *packed_out;           /* member member0 + k at packed_out + k * member_stride (16-B aligned) */
  int64_t member_stride;       /* floats, >= lnw_policy_packed_floats(D), a multiple of 4 */
  const float *noise_dev;      /* NULL, or [2] = sigma, clip on the device */
  uint64_t seed;
  const int64_t *call_dev;     /* rollout index, read on the device (NULL = 0) */
} lnw_actor_perturb_args;
int64_t lnw_policy_packed_floats(int32_t D); /* 0 for unsupported D */
int lnw_actor_perturb(const lnw_actor_perturb_args *args, void *stream);

/* lnw_policy_act for a population: the E local envs in members of
 * envs_per_member consecutive envs (the last may hold fewer), member k acting
 * with the packed set at args->params + k * member_stride (args->params: the
 * set of the member that owns local env 0; 16-B aligned). A workgroup serves
 * rows of one member: grid = members x ceil(envs_per_member n / 512), most
 * efficient where envs_per_member n is a multiple of 512. Everything else — the
 * keyed sample by global row, forced actions, scripted rows, kinds, rollout
 * rows, live / alive — is lnw_policy_act's, bit for bit what lnw_policy_act
 * computes for the member's envs alone with the member's set.
 * By design: a row whose heads are NaN takes lnw_policy_act's guard (mean 0, std
 * 1); the reference reloads the noiseless actor for the rest of the episode
 * (ppo.py:505-507). */
typedef struct lnw_policy_pop {
  int64_t envs_per_member;     /* G > 0 */
  int64_t member_stride;       /* floats, >= lnw_policy_packed_floats(D), a multiple of 4 */
} lnw_policy_pop;
int lnw_policy_act_pop(const lnw_policy_args *args, const lnw_policy_pop *pop, void *stream);

/* After lnw_step: the rollout's bookkeeping of step t (ppo.py:598-641) and the
 * critic (Value, network.py:154-172) on the rows the actor saw: value (0 after
 * the episode ended), rewards (ditto), running flag, and live &= done != 0. */
typedef struct lnw_rollout_post_args {
  const float *obs;            /* rollout rows of step t: env e at obs + e * obs_env_stride, [n][D] */
  int64_t obs_env_stride, E;
  int32_t n, D;
  const float *critic;         /* BatchedCritic.packed(), or NULL (no value) */
  float *val;                  /* env e at val[e * val_env_stride] */
  int64_t val_env_stride;
  const void *rew;             /* [E][n_rew] lnw_step rewards (float32, or float64 if rew_f64) */
  int32_t rew_f64, n_rew;
  double *rew_out;             /* NULL, or env e at rew_out + e * rew_env_stride */
  int64_t rew_env_stride;
  const int32_t *done;         /* [E] lnw_step done */
  uint8_t *live;               /* [E] in/out */
  uint8_t *running;            /* NULL, or env e at running[e * running_env_stride] */
  int64_t running_env_stride;
  int32_t stop_at_done;        /* mask values / rewards after the episode ended, update live */
} lnw_rollout_post_args;
int lnw_rollout_post(const lnw_rollout_post_args *args, void *stream);

/* ---- fused acting step of the DDQN caller (DISCRETE mode) -------------------
 * lnw_qnet_act replaces, per step and side, the reference DDQN loop's acting
 * (ddqn.py:286-387): per live ship one batch-1 DMLP forward (network.py:246-305:
 * the actor's conv head, x = [head(12), obs[49:]] with no LayerNorm, then the
 * linear heads radar 2 / attack 5 / movement 50, each with bias and ReLU), three
 * argmax().item() calls and Python `random` for epsilon-greedy
 * (ddqn.py:299-308), for every env at once and written as the int32 rows lnw_step
 * takes with LNW_ACT_I32. params: BatchedQNet.packed() (lnw/qlearn.py). One
 * launch.
 *  - LNW_QNET_EPS_GREEDY: with the four keyed uniforms u0..u3 of the row, explore
 *    iff u0 < eps; the random row is [(int)(u1*2), (int)(u2*5), (int)(u3*50)]
 *    (ddqn.py:300), else [argmax radar, argmax attack, argmax movement] with
 *    torch.argmax's order (first maximal index; NaN above every number).
 *    target_net is never put in eval() there, so its batch-1 calls normalise
 *    with the row's own statistics: bn_running = 0.
 *  - LNW_QNET_RED_RANDOM: untrained red (ddqn.py:316-328), no network: t < 20:
 *    [(int)(u0*2), (int)(u1*2), 2 + (int)(u2*3)]; else [(int)(u0*2),
 *    (u1 < red_aggression && tl_cnt > 0) ? 1 + (int)(u2*4) : 0, (int)(u3*50)].
 *  - Rows of sunk ships (ddqn.py:312) and of envs with live == 0 are 0, 0, 0, 0;
 *    column 3 is always 0.
 *  - Keyed draws (as lnw_policy_act's): the uniforms of global row g = row_base +
 *    e * n + i are lnw_fill_uniform_f32(seed, offset = (slot << 40) + 4 g), one
 *    Philox block, so a shard draws what one call over all envs draws.
 * The trained-red branch of the reference (ddqn.py:331) feeds the red network
 * the last blue ship's state; here each side's network sees its own rows. */
#define LNW_QNET_EPS_GREEDY 0
#define LNW_QNET_RED_RANDOM 1
typedef struct lnw_qnet_args {
  const float *obs;            /* [E][n][D] this side's rows, 16-B aligned (RED_RANDOM: unread) */
  int64_t E;
  int32_t n, D, own0, A;       /* ships of the side, row length, first agent slot, agents per env */
  int64_t obs_in_env_stride;   /* floats between envs' rows in obs (0: n * D) */
  const float *params;         /* BatchedQNet.packed(): conv head 578 floats in lnw_actor_features'
                                  order, then W [57][n_in] (radar, attack, movement rows), b [57] */
  int32_t bn_running;          /* 0: per-row BatchNorm statistics, 1: running */
  int32_t mode;                /* LNW_QNET_EPS_GREEDY, or LNW_QNET_RED_RANDOM (params may be NULL) */
  float eps;
  const float *eps_env;        /* NULL, or per-env epsilon [E] (eps unused) */
  uint64_t seed, slot;         /* keyed draws: one slot per (step, side) */
  int64_t row_base;            /* global id of row 0 (env_id_base * n) */
  int32_t t;                   /* episode step (RED_RANDOM's < 20 switch) */
  float red_aggression;
  const uint16_t *tl_cnt;      /* RED_RANDOM: [A][E] the handle's LNW_F_TL_CNT field */
  const uint8_t *alive;        /* [A][E] the handle's LNW_F_ALIVE field */
  const uint8_t *live;         /* [E] episode still running (NULL: all) */
  int32_t *full;               /* NULL, or [E][A][4] action array of lnw_step (LNW_ACT_I32): only rows
                                  own0 .. own0 + n - 1 are written */
  int32_t *act_out;            /* NULL, or replay rows of 4: env e ship i at e * act_env_stride + 4 i */
  int64_t act_env_stride;
  float *q_out;                /* NULL, or [E * n][57] the ReLU'd Q-values (EPS_GREEDY only) */
  uint8_t *explored;           /* NULL, or [E * n]: 1 where a kept row took the random branch */
} lnw_qnet_args;
int lnw_qnet_act(const lnw_qnet_args *args, void *stream);

/* ---- DDQN learner step ------------------------------------------------------
 * lnw_qnet_grad is the reference's optimize() (ddqn.py:153-247) for one side on
 * `rows` transitions, up to the gradient: the target network's forward on
 * next_state with BatchNorm batch statistics (it is never put in eval()), y =
 * float32(double(float32(gamma * per-head max) * done) + reward); the policy
 * network's forward on state (batch statistics, or the running ones:
 * policy_bn_running, what the reference's red side does), the three Q-values
 * gathered at action[0..2], loss = mean((qs - y)^2) over the 3 * rows elements,
 * and its gradient by every policy parameter — through the ReLU, the linear
 * heads, convhead, both max pools (first maximum of a window in row-major
 * order, as torch), both BatchNorms (with the batch-mean terms under batch
 * statistics) and both convolutions. grad has BatchedQNet.packed()'s layout,
 * zeros in the four running-statistics slots, and is not clamped. Every
 * training-mode forward updates that network's running statistics in its
 * parameter vector (momentum 0.1, unbiased variance) unless freeze_running.
 * A chain of launches on `stream`: no host synchronisation, no allocation, no
 * atomics (bitwise reproducible). workspace: lnw_qlearn_workspace_bytes(rows, D)
 * bytes, 16-B aligned (0 for unsupported shapes).
 * Limits as lnw_qnet_act: 16-B aligned rows, D % 4 == 0, 49 <= D, D - 37 <= 64.
 *
 * lnw_qnet_adam clamps the gradient to [-clamp, clamp] (clamp > 0) and applies
 * one torch.optim.Adam step (no weight decay) to all `count` elements; the step
 * number is *step_dev + 1, a device counter the call advances, so a captured
 * graph replays with the right bias correction. A zero gradient with zero
 * moments leaves the parameter bit-unchanged (the running-statistics slots). */
typedef struct lnw_qlearn_args {
  const float *state;          /* [rows][D], 16-B aligned */
  const float *next_state;     /* [rows][D], 16-B aligned */
  int64_t rows;
  int32_t D;
  int32_t action_stride;       /* int32s between rows of action (>= 3) */
  const int32_t *action;       /* row r: action[r * action_stride + 0..2] = radar, attack, movement */
  const void *reward;          /* [rows] float32, or float64 with reward_f64 */
  const int32_t *done;         /* [rows] 1 while the episode runs */
  int32_t reward_f64;
  int32_t policy_bn_running;   /* 0: policy BatchNorm on batch statistics, 1: running */
  int32_t freeze_running;      /* 1: leave the running statistics alone */
  float gamma;
  float *policy_params;        /* BatchedQNet.packed() layout; running statistics updated in place */
  float *target_params;
  float *grad;                 /* [578 + 57 * n_in + 57] out */
  float *loss;                 /* [1] out */
  float *y_out;                /* NULL, or [rows][3] */
  float *qs_out;               /* NULL, or [rows][3] */
  float *stats_out;            /* NULL, or [2 policy, target][2 mean, biased var][13 channels: conv1 5, conv2 8] */
  void *workspace;
  int64_t workspace_bytes;
} lnw_qlearn_args;
int64_t lnw_qlearn_workspace_bytes(int64_t rows, int32_t D);
int lnw_qnet_grad(const lnw_qlearn_args *args, void *stream);
int lnw_qnet_adam(float *params, const float *grad, float *m, float *v, int64_t count, int64_t *step_dev,
                  float lr, float beta1, float beta2, float eps, float clamp, void *stream);

/* ---- MAPPO learner step ------------------------------------------------------
 * lnw_ppo_grad is one minibatch update of the reference's PPO.learn
 * (ppo.py:321-390) for the blue side on `rows` rows, up to the two gradients.
 * Row r is observation row ri = row_index ? row_index[r] : r of obs
 * [groups][n][D]; its global state is the n * D floats of group ri / n.
 *   evaluate (ppo.py:673-693): the actor on each row with that row's own
 *     BatchNorm statistics (the reference calls it one state at a time in
 *     train()), new_log_probs and entropies [rows][4]; V = critic(global state);
 *   advantage: PPO.gae over the rows as the sequence (gamma, lambda), + V, then
 *     popart_normalize against rtg (unbiased std; std = 0 gives NaN), in double;
 *   actor_loss = -(mean(min(adv ratio, adv clamp(ratio, 1 -+ eps_clip))) +
 *     entropy_coef mean(entropies)); critic_loss = sqrt(mean(max((v - rtg)^2,
 *     (clamp(v, v_old -+ eps_clip) - rtg)^2))); torch's tie and clamp gradient
 *     rules (an in-range element passes the whole gradient);
 *   both gradients, unclipped, in the flat layouts below. Max pool sends the
 *     gradient to the first maximum in row-major order.
 * The actor's running statistics take the `rows` sequential updates of the
 * reference (momentum 0.1, unbiased variance, minibatch order) in actor_params
 * unless freeze_running.
 * Actor layout (floats): conv1 w 45, b 5; norm1 w, b, running mean, var 5 each;
 * conv2 w 360, b 8; norm2 w, b, running mean, var 8 each; convhead w 96, b 12;
 * layernorm w, b [n_in] each (BatchedActor.packed_features(), n_in = D - 37);
 * fc1 w [64][n_in], b 64; fc2 w [64][64], b 64; fc3 w [32][64], b 32;
 * normal_head w [4][32]; log_std_head w [4][32]; logstd 1 (gradient 0).
 * Critic layout: the state_dict order, fc1 w [32][n D], b 32; fc2 w [64][32],
 * b 64; fc3 w [64][64], b 64; fc4 w [64], b 1.
 * A chain of launches on `stream`: no host synchronisation, no allocation, no
 * atomics; bitwise reproducible. workspace: lnw_ppolearn_workspace_bytes(rows,
 * n, D) bytes, 16-B aligned (0 for unsupported shapes). Limits as
 * lnw_policy_act: 16-B aligned rows, D % 4 == 0, 49 <= D, D - 37 <= 64; n <= 16.
 *
 * lnw_ppo_clip_adam is clip_grad_norm_(max_norm) followed by lnw_qnet_adam's
 * Adam step: the global L2 norm of grad (fixed order, double), every gradient
 * multiplied by min(1, max_norm / (norm + 1e-6)) from a device scalar.
 * scale_norm [2] receives that factor and the norm. */
typedef struct lnw_ppolearn_args {
  const float *obs;            /* [groups][n][D], 16-B aligned */
  const int64_t *row_index;    /* NULL (identity), or [rows] rows of obs */
  int64_t rows;
  int32_t n, D;
  const float *actions;        /* [rows][4] */
  const float *old_log_probs;  /* [rows][4] */
  const float *rtg;            /* [rows] */
  const float *old_values;     /* [rows] */
  float eps_clip, entropy_coef, gamma, lambda_;
  int32_t freeze_running;
  float *actor_params;         /* running statistics updated in place */
  const float *critic_params;
  float *actor_grad;           /* [579 + 2 n_in + 64 n_in + 64 + 4160 + 2080 + 256] out */
  float *critic_grad;          /* [32 n D + 32 + 2112 + 4160 + 65] out */
  float *actor_loss;           /* [1] out */
  float *critic_loss;          /* [1] out */
  float *new_log_probs;        /* NULL, or [rows][4] */
  float *entropies;            /* NULL, or [rows][4] */
  float *values;               /* NULL, or [rows] */
  float *advantage;            /* NULL, or [rows] */
  void *workspace;
  int64_t workspace_bytes;
} lnw_ppolearn_args;
int64_t lnw_ppolearn_workspace_bytes(int64_t rows, int32_t n, int32_t D);
int lnw_ppo_grad(const lnw_ppolearn_args *args, void *stream);
int lnw_ppo_clip_adam(float *params, const float *grad, float *m, float *v, int64_t count, int64_t *step_dev,
                      float lr, float beta1, float beta2, float eps, float max_norm, float *scale_norm,
                      void *stream);

/* ---- MAPPO minibatch draw ------------------------------------------------------
 * lnw_ppo_sample draws the learner's prioritised minibatch (ppo.py:311-319:
 * WeightedRandomSampler(|rtg| + 1e-5, batch, replacement=False), i.e.
 * torch.multinomial without replacement) as a keyed draw: sequential weighted
 * sampling without replacement is "the `batch` smallest keys e_r / w_r, e_r ~
 * Exp(1), in ascending order" (Efraimidis-Spirakis), which is what torch does
 * with its own generator. For local row r, global row g = row_base + r, slot =
 * *draw_dev:
 *   w_r = (double)(fabsf(rtg[r]) + 1e-5f)               (the float32 sum first)
 *   u_r = u53(o[0], o[1]), o = Philox4x32-10 under key `seed` of the counter
 *         words {lo32(c), hi32(c), LNW_SAMPLE_CTR2, LNW_SAMPLE_CTR3}, c =
 *         (slot << 40) + g (g < 2^40, slot < 2^24): a domain of its own, no
 *         draw shared with the rollout's or lnw_fill_uniform_f32's
 *   k_r = -p_log(1 - u_r) / w_r in double (portable p_log: the same bits on the
 *         host); a zero key is stored as +0; a row whose rtg is NaN or +-inf
 *         gets k_r = +inf and is counted in status[0]
 * The minibatch is the first `batch` rows of the total order (k_r, g): keys
 * compared as numbers, ties to the lower row. Non-finite rows are therefore
 * drawn only after every finite row, in row order. The key depends on the global
 * row alone, so the first `batch` of the union of two shards' (key_out, row_base
 * + index_out), merged by (key, global row), is what one call over all rows
 * draws. lnw_ppo_sample_merge below is that merge on the device, for any number
 * of shards up to 64.
 * The call's last launch gathers actions, log_probs [rows][4], rtg and values[r
 * / n] of the drawn rows (each where both its input and its output are given)
 * and, with advance, adds 1 to *draw_dev.
 * A chain of launches on `stream`: no host synchronisation, no allocation;
 * integer atomics only in counts and a minimum, which no arrival order changes:
 * bitwise reproducible, also under graph replay. workspace:
 * lnw_ppo_sample_workspace_bytes(rows, batch) bytes, 16-B aligned (0 for
 * unsupported shapes: 1 <= batch <= min(rows, 131072), rows < 2^31). */
#define LNW_SAMPLE_CTR2 0x13198A2Eu
#define LNW_SAMPLE_CTR3 0x03707344u
#define LNW_SAMPLE_MAX_BATCH 131072
typedef struct lnw_ppo_sample_args {
  const float *rtg;            /* [rows] */
  int64_t rows, row_base;      /* 1 <= rows < 2^31; global id of row 0 (0 <= row_base, row_base + rows <= 2^40) */
  int64_t batch;               /* 1 <= batch <= min(rows, 131072) */
  uint64_t seed;
  int64_t *draw_dev;           /* [1] the slot, read on the device (NULL = 0) */
  int32_t advance;             /* 1: the call's last launch adds 1 to *draw_dev */
  const float *actions, *log_probs;  /* NULL, or [rows][4] */
  const float *values;         /* NULL, or [rows / n]: old value of row r is values[r / n] */
  int32_t n;
  int64_t *index_out;          /* [batch] local rows in draw order */
  double  *key_out;            /* NULL, or [batch] */
  float *actions_out, *log_probs_out, *rtg_out, *old_values_out;  /* NULL, or [batch][4] / [batch] */
  int64_t *status;             /* NULL, or [1]: rows with a non-finite rtg */
  void *workspace; int64_t workspace_bytes;
} lnw_ppo_sample_args;
int64_t lnw_ppo_sample_workspace_bytes(int64_t rows, int64_t batch);  /* 0: unsupported */
int lnw_ppo_sample(const lnw_ppo_sample_args *args, void *stream);

/* ---- Training over sharded rollouts ---------------------------------------------
 * Every rank draws `batch` candidates from its own rows (lnw_ppo_sample with its
 * row_base), the ranks exchange the candidate lists, every rank merges them into
 * the one draw over all rows, packs the payload of the slots whose rows it owns,
 * and the packed buffers are summed over the ranks: every rank then holds the
 * same minibatch and runs lnw_ppo_grad / lnw_ppo_clip_adam on it. The collectives
 * are the caller's (lnw/ppodist.py: one all-gather, one integer all-reduce).
 *
 * lnw_ppo_sample_merge: lists [W][stride] int64, stride >= 2 batch + 1, list w is
 * rank w's message: words [0, batch) the bits of its key_out (float64), words
 * [batch, 2 batch) its global rows row_base + index_out, word 2 batch its status
 * count. Each list is ascending in (key, global row), as lnw_ppo_sample leaves it;
 * keys are non-negative (a zero key is +0, a non-finite row +inf), global rows
 * are < 2^40 and distinct across the lists. For slot s in [0, batch) the call
 * writes the s-th element of the union of the lists in the total order (key as a
 * number, global row as a 64-bit value):
 *   key_out[s], row_out[s]           its key and global row
 *   src_rank[s], src_pos[s]          the list it came from and its place there
 *   index_out[s] = s n + row_out[s] % n   its row of lnw_ppo_rows_pack's xobs
 *   status_out[0]                    the sum of the W status words
 * One thread per candidate: its place in the union is its place in its own list
 * plus, for every other list, the number of elements before it (binary search).
 * One launch on `stream`: no host synchronisation, no allocation, no workspace,
 * no atomics, every output written by exactly one thread: bitwise reproducible.
 * 1 <= W <= 64 and 1 <= batch <= LNW_SAMPLE_MAX_BATCH (else LNW_EUNSUPPORTED);
 * n >= 1; int64 / double arrays 8-B aligned. With W = 1 the call copies the list. */
typedef struct lnw_ppo_merge_args {
  const int64_t *lists;        /* [W][stride] */
  int32_t W, n;
  int64_t stride, batch;
  double *key_out;             /* [batch] */
  int64_t *row_out;            /* [batch] global rows */
  int32_t *src_rank, *src_pos; /* [batch] */
  int64_t *index_out;          /* [batch] */
  int64_t *status_out;         /* [1] */
} lnw_ppo_merge_args;
int lnw_ppo_sample_merge(const lnw_ppo_merge_args *args, void *stream);

/* lnw_ppo_rows_pack writes the exchange buffer of rank `rank`, whose rows are the
 * global rows [row_base, row_base + rows): xbuf, 32-bit words, every region
 * starting on a 16-B boundary, in this order:
 *   xobs          [batch][n][D]
 *   actions       [batch][4]
 *   old_log_probs [batch][4]
 *   rtg           [batch], padded to a multiple of 4 words
 *   old_values    [batch], padded to a multiple of 4 words
 * lnw_ppo_pack_words(batch, n, D) words in all (0 for unsupported shapes). Slot s
 * with src_rank[s] == rank and local row r = row_out[s] - row_base holds the n D
 * floats of the row's group obs[r / n] (read in place, as float4), actions[r],
 * log_probs[r], rtg[r] and values[r / n], bit for bit; every other slot, and the
 * padding, is zero words. Every word of xbuf is written on every call. Summed
 * over the ranks as int32, the buffers give every rank each owner's bits (a
 * float sum would lose -0.0 and NaN payloads), and xobs with lnw_ppo_sample_merge's
 * index_out is lnw_ppo_grad's obs / row_index.
 * Two launches on `stream`: no host synchronisation, no allocation, no atomics;
 * bitwise reproducible. Width limits are lnw_ppo_grad's (D % 4 == 0, 49 <= D, D -
 * 37 <= 64, 1 <= n <= 16) and 1 <= batch <= LNW_SAMPLE_MAX_BATCH, else
 * LNW_EUNSUPPORTED; rows % n == 0, row_base % n == 0, 0 <= rank < 64, row_base +
 * rows <= 2^40; obs, actions, log_probs and xbuf 16-B aligned. */
typedef struct lnw_ppo_pack_args {
  const float *obs;            /* [rows / n][n][D], 16-B aligned */
  const float *actions, *log_probs;  /* [rows][4], 16-B aligned */
  const float *rtg;            /* [rows] */
  const float *values;         /* [rows / n] */
  int64_t rows, row_base;
  int32_t n, D, rank;
  int64_t batch;
  const int64_t *row_out;      /* [batch] lnw_ppo_sample_merge's */
  const int32_t *src_rank;     /* [batch] */
  uint32_t *xbuf;              /* [xbuf_words] out, 16-B aligned */
  int64_t xbuf_words;          /* >= lnw_ppo_pack_words(batch, n, D) */
} lnw_ppo_pack_args;
int64_t lnw_ppo_pack_words(int64_t batch, int32_t n, int32_t D);  /* 0: unsupported */
int lnw_ppo_rows_pack(const lnw_ppo_pack_args *args, void *stream);

/* ---- DDQN replay ------------------------------------------------------------------
 * The transitions of QCollector's ring (lnw/qlearn.py), drawn and packed on the
 * device. The ring holds `cap` steps of E envs: state, next_state [cap][E][n][D]
 * float32, action [cap][E][n][4] int32, reward [cap][E][n] float32 or float64,
 * done [cap][E] int32. Beside it lies priority [E][cap] float32, env-major, so
 * that a shard of consecutive envs is a contiguous range of the global rows:
 *   local row  r = e cap + k            (env e of the shard, ring slot k)
 *   global row g = row_base + r,  row_base = (the shard's first global env) cap
 * NaN marks a slot that holds no transition yet.
 *
 * The draw is lnw_ppo_sample above, unchanged, with rtg = priority, rows = E cap,
 * that row_base, n = 1 and every gather column NULL: weight |p| + 1e-5, `batch`
 * distinct transitions in ascending (key, global row) order, a NaN entry drawn
 * only after every real one and counted in status. Equal priorities make it
 * uniform sampling without replacement (random.sample, ddqn.py:74-76). Shards
 * merge with lnw_ppo_sample_merge (n = 1). Its limits hold: E cap < 2^31,
 * row_base + E cap <= 2^40.
 *
 * lnw_replay_mark writes priority[e][k] for every env e after a collector step
 * has filled ring slot k: 1.0f when reward is NULL, else the sum over ships i =
 * 0 .. n-1, in that order, in float32, of fabsf((float)reward[k][e][i]). One
 * launch on `stream`; 0 <= k < cap, 1 <= n <= 16. */
typedef struct lnw_replay_mark_args {
  float *priority;             /* [E][cap] */
  const void *reward;          /* NULL (priority 1), or [cap][E][n] float32 / float64 */
  int32_t reward_f64;
  int32_t n, cap, k;
  int64_t E;
} lnw_replay_mark_args;
int lnw_replay_mark(const lnw_replay_mark_args *args, void *stream);

/* lnw_replay_pack writes the drawn transitions as lnw_qnet_grad's row tensors into
 * xbuf, 32-bit words, every region starting on a 16-B boundary, in this order:
 *   state      [batch][n][D]
 *   next_state [batch][n][D]
 *   action     [batch][n][4]
 *   reward     [batch][n], one word each, or two with reward_f64; padded to a
 *              multiple of 4 words
 *   done       [batch][n], the ring's done[k][e] repeated for each ship; padded
 *              likewise
 * lnw_replay_pack_words(batch, n, D, reward_f64) words in all (0 for unsupported
 * shapes). Slot s is owned when src_rank is NULL or src_rank[s] == rank. An owned
 * slot with local row r = row_out[s] - row_base in [0, E cap), e = r / cap, k = r
 * % cap, holds that transition's words bit for bit (-0.0, NaN payloads and
 * denormals kept). Every slot that is not owned, every owned slot whose r lies
 * outside that range (nothing is read out of range), and all padding are zero
 * words. Every word of xbuf is written on every call. With src_rank NULL the call
 * is the local gather; with lnw_ppo_sample_merge's row_out / src_rank it writes a
 * rank's exchange buffer, and the ranks' buffers summed as int32 give every rank
 * each owner's bits. index_out, if given, receives k E + e per slot (the ring's
 * flat (step, env) index, QCollector.sample()'s convention), -1 for a slot that
 * holds zero words.
 * One launch on `stream`, one thread per 16 B of xbuf (float4 accesses, 64-bit
 * ring offsets): no host synchronisation, no allocation, no workspace, no
 * atomics; bitwise reproducible. D % 4 == 0, 49 <= D <= 101, 1 <= n <= 16, 1 <=
 * batch <= LNW_SAMPLE_MAX_BATCH, 0 <= rank < 64, else LNW_EUNSUPPORTED; state,
 * next_state, action and xbuf 16-B aligned. */
typedef struct lnw_replay_pack_args {
  const float *state, *next_state;  /* [cap][E][n][D], 16-B aligned */
  const int32_t *action;       /* [cap][E][n][4], 16-B aligned */
  const void *reward;          /* [cap][E][n] float32, or float64 with reward_f64 */
  const int32_t *done;         /* [cap][E] */
  int32_t reward_f64;
  int32_t cap, n, D;
  int64_t E;
  int64_t row_base, batch;
  const int64_t *row_out;      /* [batch] global rows */
  const int32_t *src_rank;     /* NULL (every slot owned), or [batch] */
  int32_t rank;
  int64_t *index_out;          /* NULL, or [batch] */
  uint32_t *xbuf;              /* [xbuf_words] out, 16-B aligned */
  int64_t xbuf_words;          /* >= lnw_replay_pack_words(batch, n, D, reward_f64) */
} lnw_replay_pack_args;
int64_t lnw_replay_pack_words(int64_t batch, int32_t n, int32_t D, int32_t reward_f64);  /* 0: unsupported */
int lnw_replay_pack(const lnw_replay_pack_args *args, void *stream);

/* Host-side constants the kernels use (for tests): hit probability tables
 * 1-(1-p)^n for p in {0.45, 0.63}, n = 0..8, in float64 and float32. */
int lnw_hit_tables(double *tab64 /* [2][9] */, float *tab32 /* [2][9] */);

#ifdef __cplusplus
}
#endif
#endif /* LNW_H */
