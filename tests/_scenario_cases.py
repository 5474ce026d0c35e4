"""Scenario options across launch forms: the table of scenarios (each differs
from the default scenario in one or two options, one in several) and of launch
forms per fleet, their inputs, and the CPU oracle's record of them. Host only:
numpy and _oracle.

TEST INFRASTRUCTURE: shared by tests/test_scenario_cases_cpu.py (which shows on
the oracle alone, from its step statistics, that each scenario's inputs reach
the rules it is there for, and that the option changes the result) and
tests/test_gpu_scenario_cases.py (which runs every scenario through every
launch form of its fleet).

Every scenario: Philox, float32 rewards, auto-reset with a 20-step horizon, 25
steps (one reset at the least, and steps_done > 14 in both episodes), 256 envs
in four 64-env blocks, blocks 0 and 2 wholly quiet (the sides out of every
sensor's reach), blocks 1 and 3 in contact. The units forms run all 256 envs,
every other form the first 200 (a partial last workgroup at 64, 32, 16 and 8
envs per workgroup); Philox is keyed by the global env id, so one oracle run of
the 256 envs per scenario serves every form.
"""
import functools

import numpy as np

import _oracle
from _spawns import box_positions, grid as _grid, hash_mult, ref_spawns, water_positions

STEPS, HORIZON, SEED = 25, 20, 23
E, BLOCK, E_PART = 256, 64, 200
SNAP_ENVS = tuple(range(8)) + tuple(range(BLOCK, BLOCK + 8))  # of the first quiet and the first contact block
TYPE = {"small": _oracle.T_SMALL, "large": _oracle.T_LARGE, "ls": _oracle.T_LS}
LZ = (14, 82)  # game.py:590

FLEETS = {
    "4v4": dict(blue=["small"] * 4, red=["large"] * 4, G=100),
    "4v4ls": dict(blue=["small"] * 4, red=["large"] * 3 + ["ls"], G=100),  # team_shape: the 4v4 forms
    "3v3ls": dict(blue=["small"] * 3, red=["large", "large", "ls"], G=100),
    "8v10ls": dict(blue=["small"] * 8, red=["large"] * 8 + ["ls"] * 2, G=200),
}
OPTION_DEFAULTS = dict(discrete=False, landing_ops=False, aggressive=True, side_blue=True, trained_red=True,
                       red_aggression=0.4, move_thr=74, ew_thr=70, lz=LZ)


def _moved_zone():
    """A landing zone away from (14, 82), found on the grid: the water cell
    nearest (80, 45) with nothing above 60 within 8 cells of it."""
    g = _grid(100)
    cells = [(x, y) for x in range(70, 91) for y in range(35, 56) if g[x - 8:x + 9, y - 8:y + 9].max() <= 60]
    return min(cells, key=lambda c: ((c[0] - 80) ** 2 + (c[1] - 45) ** 2, c))


def _sc(fleet, layout, baseline, **options):
    """options: what differs from OPTION_DEFAULTS; baseline: the options put
    back to their defaults for the CPU test's "the option changes the result"."""
    unknown = set(options) - set(OPTION_DEFAULTS)
    assert not unknown and set(baseline) <= set(options), (unknown, baseline)
    return dict(fleet=fleet, layout=layout, options=options, baseline=baseline)


SCENARIOS = {
    # the default scenario: what the debug bits run on, and nothing to put back
    "default": _sc("4v4", "zone", ()),
    "defensive": _sc("4v4", "zone", ("aggressive",), aggressive=False),
    "defensive_untrained": _sc("4v4", "zone", ("aggressive",), aggressive=False, trained_red=False),
    # (the sides' engaging-unit rules, game.py:346 / :355, change a reward only where one blue ship
    # hits and another fires and misses: the skirmish layout's single-missile salvos)
    "side_red": _sc("4v4", "skirmish", ("side_blue",), side_blue=False),
    "aggression_hi": _sc("4v4", "zone", ("red_aggression",), trained_red=False, red_aggression=0.9),
    "aggression_lo": _sc("4v4", "zone", ("red_aggression",), trained_red=False, red_aggression=0.05),
    # (movement above and EW below the defaults: the other way round no EW verdict differs,
    # tests/golden/make_golden.py make_option_episodes)
    "thresholds": _sc("4v4", "coast", ("move_thr", "ew_thr"), move_thr=85, ew_thr=60),
    "discrete_defensive": _sc("4v4", "zone", ("aggressive",), discrete=True, aggressive=False),
    "landing_4v4ls": _sc("4v4ls", "landing", ("landing_ops",), landing_ops=True),
    "landing_moved_zone": _sc("4v4ls", "landing", ("lz",), landing_ops=True, lz=_moved_zone()),
    "landing_3v3ls": _sc("3v3ls", "landing", ("landing_ops",), landing_ops=True),
    "landing_8v10ls_g200": _sc("8v10ls", "landing", ("landing_ops",), landing_ops=True),
    # several at once
    "combined": _sc("4v4ls", "landing", ("aggressive", "side_blue"), landing_ops=True, aggressive=False,
                    side_blue=False, trained_red=False, red_aggression=0.7),
}


def _form(E, epw, kernel, prod=False, contact=False, env=None):
    return dict(E=E, epw=epw, kernel=kernel, prod=prod, contact=contact, env=env or {})


# Launch forms per fleet, each row read against plan_step (csrc/lnw_host.inc):
# the kernel lnw_step_kernel must report and what lnw_step_kernel_prod must.
# int32 rows are outside the production configuration (prod_config): a discrete
# scenario's units_prod row must report the generic units kernel (prod_of).
FORMS_4V4 = {
    "units": _form(E, 64, "units", env={"LNW_NO_PROD": "1"}),
    "units_prod": _form(E, 64, "units", prod=True),
    "epw64_staged": _form(E_PART, 64, "team"),                  # E % 256 != 0: no units
    "epw32_two_slab": _form(E_PART, 32, "team"),
    "epw32_no_slab": _form(E_PART, 32, "team", env={"LNW_NO_SLAB": "1"}),
    "epw16_direct": _form(E_PART, 16, "team"),
    "epw8": _form(E_PART, 8, "team"),
    "contact_epw64": _form(E_PART, 64, "team_contact", contact=True),
    "contact_epw16": _form(E_PART, 16, "team_contact", contact=True),
}
FORMS = {
    "4v4": FORMS_4V4,
    "4v4ls": FORMS_4V4,
    "3v3ls": {
        "epw64": _form(E_PART, 64, "team"),
        "epw16_direct": _form(E_PART, 16, "team"),
        "group": _form(E_PART, None, "group", env={"LNW_FORCE_GROUP": "1"}),
    },
    "8v10ls": {
        "group": _form(E_PART, None, "group"),
        "lane": _form(E_PART, None, "generic", env={"LNW_NO_GROUP": "1"}),
    },
}
CASES = [(s, f) for s in sorted(SCENARIOS) for f in FORMS[SCENARIOS[s]["fleet"]]]

# LNW_DEBUG_SKIP bits the shipped library accepts as result preserving
# (lnw_create, kResultPreserving), on the default scenario's 4v4 forms (any bit
# is outside the production configuration, so without the units_prod row; bit 9
# also keeps the units kernel out: plan_step) and, for the group kernel's bit
# 15, on the 8v10ls forms
DEBUG_BITS = (9, 15, 17, 22, 23, 28, 29)
BIT_CASES = [(b, "default", f) for b in DEBUG_BITS if b != 15 for f in FORMS_4V4 if f != "units_prod"] + \
            [(15, "landing_8v10ls_g200", f) for f in FORMS["8v10ls"]]


def prod_of(name, form):
    return FORMS[SCENARIOS[name]["fleet"]][form]["prod"] and not options(name)["discrete"]


def bit_kernel(bit, form):
    f = FORMS_4V4[form]
    return "team" if bit == 9 and f["kernel"] == "units" else f["kernel"]


def fleet(name):
    return FLEETS[SCENARIOS[name]["fleet"]]


def options(name, baseline=False):
    o = dict(OPTION_DEFAULTS, **SCENARIOS[name]["options"])
    if baseline:
        o.update({k: OPTION_DEFAULTS[k] for k in SCENARIOS[name]["baseline"]})
    return o


def scenario_kwargs(name):
    """lnw.config.Scenario's keywords for the scenario."""
    o = options(name)
    return dict(discrete=o["discrete"], landing_ops=o["landing_ops"],
                tactics="aggressive" if o["aggressive"] else "defensive", side="blue" if o["side_blue"] else "red",
                trained_red=o["trained_red"], red_aggression=o["red_aggression"], movement_threshold=o["move_thr"],
                ew_threshold=o["ew_thr"], landing_zone=tuple(o["lz"]), auto_reset=True, episode_steps=HORIZON)


def quiet_env(e):
    return (np.asarray(e) // BLOCK) % 2 == 0


def types(name):
    f = fleet(name)
    return [TYPE[t] for t in f["blue"] + f["red"]]


def mult(name):
    f = fleet(name)
    nb, nr = len(f["blue"]), len(f["red"])
    return hash_mult(nb * (4 * nb + 52) + nr * (4 * nr + 52), seed=9)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
# constant move columns (a2, a3) that take a landing ship 2 cells a step along
# -x, -y, +y: the reference takes cos / sin of degrees(2 pi a2) as if it were
# radians (landingship.py:466-478), so a2 = theta / 360 heads theta
_HEAD = {(-2, 0): np.pi / 360.0, (0, -2): 1.5 * np.pi / 360.0, (0, 2): 0.5 * np.pi / 360.0}


def _around(g, rng, centre, lo, hi, n, bound=100):
    """n water cells lo..hi cells from centre (below `bound`: no ship moves past 99)."""
    cx, cy = centre
    cells = [(x, y) for x in range(max(cx - hi, 0), min(cx + hi + 1, bound))
             for y in range(max(cy - hi, 0), min(cy + hi + 1, bound))
             if g[x, y] <= 60 and lo * lo <= (x - cx) ** 2 + (y - cy) ** 2 <= hi * hi]
    return [cells[i] for i in rng.integers(0, len(cells), n)]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """pos [E, A, 2] int32 and the action rows [STEPS, E, A, 4]: float32 draws
    of U[0, 1), or a discrete scenario's int32 rows (radar 0..1, salvo 0..4, cell
    0..49, 0: the golden generator's ranges). Layouts:

    zone     quiet blocks: blue on the reference spawns, the reds on water at x
             50..60 (the defensive zone of game.py:260 ends at x = 55), 39 cells
             and more away; contact blocks: adjacent boxes inside the zone.
             In the quiet blocks a ship moves a cell a step at most (the
             distance column scaled by 1/3, a discrete row's cell index within
             the inner 3 x 3), so the gap outlasts the 20 steps.
    skirmish as zone; in the contact blocks blue's salvo column lies in
             0.13..0.30 (one missile while it has two or more) and red's below
             0.06 (none), so fights last and blue ships hit and miss side by side.
    coast    quiet blocks as zone (the reference spawns lie at the shore: moves
             onto cells of 75..85); contact blocks: both sides in boxes along
             the same shore.
    landing  the landing ships 2, 4 or 6 cells from the zone along +x, +y or -y
             with constant rows that head for it 2 cells a step (three envs in
             four; the fourth's rows are random, the ship within 4 cells), the
             other reds 3..8 cells from the zone; quiet blocks: blue 50 cells and
             more away; contact blocks: blue 4..12 cells from the zone."""
    sc, f = SCENARIOS[name], fleet(name)
    g = _grid(f["G"])
    nb, nr = len(f["blue"]), len(f["red"])
    A = nb + nr
    rng = np.random.default_rng([SEED, sorted(SCENARIOS).index(name)])
    quiet = quiet_env(np.arange(E))
    if options(name)["discrete"]:
        acts = np.stack([rng.integers(0, 2, (STEPS, E, A)), rng.integers(0, 5, (STEPS, E, A)),
                         rng.integers(0, 50, (STEPS, E, A)), np.zeros((STEPS, E, A), np.int64)], -1).astype(np.int32)
    else:
        acts = rng.random((STEPS, E, A, 4), dtype=np.float32)
    if sc["layout"] in ("zone", "coast", "skirmish"):
        far = water_positions(g, E, [(50, 61, 42, 72)] * nr, int(rng.integers(1 << 30)))
        pos = np.concatenate([np.tile(np.array(ref_spawns(4)[:nb], np.int32), (E, 1, 1)), far], 1)
        boxes = ((5, 16, 56, 84), (8, 20, 56, 84)) if sc["layout"] == "coast" else ((30, 45, 40, 60), (45, 56, 45, 65))
        pos[~quiet] = box_positions(g, E, nb, nr, int(rng.integers(1 << 30)), *boxes)[~quiet]
        if options(name)["discrete"]:  # the cell index's inner 3 x 3 (combatant.py:689-704: x = v // 7, y = v % 7)
            inner = np.array([7 * x + y for x in (2, 3, 4) for y in (2, 3, 4)], np.int32)
            acts[:, quiet, :, 2] = inner[acts[:, quiet, :, 2] % 9]
        else:
            acts[:, quiet, :, 3] *= np.float32(1.0 / 3.0)
        if sc["layout"] == "skirmish":
            c = ~quiet
            acts[:, c, :nb, 1] = np.float32(0.13) + np.float32(0.17) * acts[:, c, :nb, 1]
            acts[:, c, nb:, 1] *= np.float32(0.06)
        return _frozen(pos, acts)
    lz = tuple(options(name)["lz"])
    if f["G"] == 200:
        far_box = (70, 96, 40, 99)
    else:
        far_box = (66, 90, 38, 60) if lz == LZ else (4, 14, 56, 84)
    pos = np.zeros((E, A, 2), np.int32)
    pos[:, :nb] = water_positions(g, E, [far_box] * nb, int(rng.integers(1 << 30)))
    heads = list(_HEAD)
    for e in range(E):
        if not quiet[e]:
            pos[e, :nb] = _around(g, rng, lz, 4, 12, nb)
        for a in range(nb, A):
            if f["red"][a - nb] != "ls":
                pos[e, a] = _around(g, rng, lz, 3, 8, 1)[0]
            elif e % 4 == 3:
                pos[e, a] = _around(g, rng, lz, 1, 4, 1)[0]
            else:
                dx, dy = heads[(e + a) % 3]
                m = 1 + (e // 4 + a) % 3
                pos[e, a] = (lz[0] - m * dx, lz[1] - m * dy)
                acts[:, e, a, 2], acts[:, e, a, 3] = np.float32(_HEAD[(dx, dy)]), 1.0
                assert g[pos[e, a, 0], pos[e, a, 1]] <= 60
    return _frozen(pos, acts)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_run(name, baseline=False):
    """orc_fullsize_range over the scenario's 256 envs, computed once and
    read-only: hash, rew, done, cog [STEPS, E(, A)], acts_after [STEPS, E, A, 4]
    (float32: a discrete run's integer values) and stats [E, len(STATS)].
    baseline: the same inputs with SCENARIOS' baseline options at their defaults."""
    f, o = fleet(name), options(name, baseline)
    pos, acts = inputs(name)
    h, rew, done, cog, aft, st = _oracle.fullsize(
        _grid(f["G"]), len(f["blue"]), len(f["red"]), types(name), pos, acts.astype(np.float32), mult(name), SEED,
        HORIZON, pos_per_env=True, acts_after=True, stats=True, **o)
    out = dict(hash=h, rew=rew, done=done, cog=cog, acts_after=aft, stats=st)
    _frozen(*out.values())
    return out


def block_stats(name, quiet):
    """The statistics summed over the quiet or over the contact blocks' envs."""
    st = oracle_run(name)["stats"][quiet_env(np.arange(E)) == quiet]
    return dict(zip(_oracle.STATS, st.sum(0).tolist()))


def changed_fraction(name):
    """The share of (step, env) pairs whose observation hash, rewards or done
    differ between the scenario and its baseline."""
    a, b = oracle_run(name), oracle_run(name, True)
    differ = (a["hash"] != b["hash"]) | (a["done"] != b["done"]) | (a["rew"] != b["rew"]).any(-1)
    return float(differ.mean())


def replay(name, envs):
    """The envs stepped one by one (OracleEnv under Philox, auto-reset as the
    device does): per env agents() and env_state() after the last step."""
    f, o = fleet(name), options(name)
    nb, nr = len(f["blue"]), len(f["red"])
    pos, acts = inputs(name)
    kinds = np.full(nb + nr, _oracle.K_PYINT if o["discrete"] else _oracle.K_F32, np.int32)
    out = {}
    for e in envs:
        env = _oracle.OracleEnv(_grid(f["G"]), nb, nr, **o)
        env.set_philox(SEED, e)
        env.reset(types(name), pos[e])
        for s in range(STEPS):
            r = env.step(acts[s, e], kinds)
            if r["done"] == 0 or env.env_state()["steps_done"] >= HORIZON:
                env.reset(types(name), pos[e])
        out[e] = dict(agents=env.agents(), env=env.env_state())
    return out
