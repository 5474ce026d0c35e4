"""Inputs at sensor reach for the quiet-workgroup path (csrc/lnw_quiet.inc), and
the CPU oracle's verdict on them. Host only: numpy and _oracle.

TEST INFRASTRUCTURE: shared by tests/test_quiet_reach_cpu.py (which shows on
the CPU that these inputs can tell a loose predicate from a right one) and
tests/test_gpu_quiet_reach.py (which runs them through every launch form).

A layout is three workgroups of envs (two full, one ragged). Each workgroup
holds exactly one probe env whose fleets of large ships stand `reach + k` cells
apart, k in -2..+3; every other env stands at the reference spawns, 88 cells
apart. A workgroup takes the quiet path only when every env in it is quiet, so
the probe alone decides its branch. An instance is one (step, probe env).
"""
import functools
import math

import numpy as np

import _oracle
from _spawns import grid as _grid, ref_spawns

DUCTS = (1.0, 1.37, 1.99)  # across the reference's 1 <= 1 + Beta(1, 3) < 2
KS = (-2, -1, 0, 1, 2, 3)
DIRS = ("x", "y", "diag")
# the four old / new position combinations of a blue / red pair: (blue, red), 0 = old, 1 = new
COMBOS = ((0, 0), (0, 1), (1, 0), (1, 1))
MUTANTS = ("drop blue-old/red-old", "drop blue-old/red-new", "drop blue-new/red-old",
           "drop blue-new/red-new", "reach one cell short")
TYPE_CODES = {"small": _oracle.T_SMALL, "large": _oracle.T_LARGE, "ls": _oracle.T_LS}


REACH_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)  # the reach test's layouts per form
REACH_STEPS = 6


def _form(nb, G, epw, kernel, direct, **kw):
    return dict(nb=nb, G=G, epw=epw, kernel=kernel, direct=direct, units=kw.pop("units", False),
                contact=kw.pop("contact", False), env=kw.pop("env", None), red=kw.pop("red", None), **kw)


# One table of launch forms, each row read against plan_step / step_qdirect
# (csrc/lnw_host.inc): the kernel lnw_step_kernel must report, and whether
# quiet workgroups write their rows directly (wave 1, whole-side stages; the
# LNW_PROF report's "quiet direct" line) or in staged passes (quiet_emit_t).
FORMS = {
    # 4v4, grid 100
    "4v4_epw64_staged": _form(4, 100, 64, "team", False),       # E % 256 != 0: no units
    "4v4_units": _form(4, 100, 64, "units", False, units=True),  # E = 512
    "4v4_epw32_two_slab": _form(4, 100, 32, "team", True),      # 64 < epw * 4 <= 128: SL
    "4v4_epw32_no_slab": _form(4, 100, 32, "team", False, env="LNW_NO_SLAB"),
    "4v4_epw16": _form(4, 100, 16, "team", True),
    "4v4_epw8": _form(4, 100, 8, "team", True),
    "4v4_contact_epw64": _form(4, 100, 64, "team_contact", False, contact=True),
    "4v4_contact_epw16": _form(4, 100, 16, "team_contact", True, contact=True),
    # 3v3, grid 100 (no two-slab instantiation: direct up to 21 envs)
    "3v3_epw64": _form(3, 100, 64, "team", False),
    "3v3_epw32": _form(3, 100, 32, "team", False),
    "3v3_epw16": _form(3, 100, 16, "team", True),                # 48 lanes
    "3v3_ls_epw64": _form(3, 100, 64, "team", False, red=("large", "large", "ls")),
    "3v3_ls_epw16": _form(3, 100, 16, "team", True, red=("large", "large", "ls")),
    # 2v2, grid 100
    "2v2_epw64": _form(2, 100, 64, "team", False),
    "2v2_epw32": _form(2, 100, 32, "team", True),                # 64 lanes
    "2v2_epw16": _form(2, 100, 16, "team", True),
    # team kernels on the 200 grid: env_quiet_t's 32-bit branch
    "4v4_g200_epw64": _form(4, 200, 64, "team", False),
    "4v4_g200_epw16": _form(4, 200, 16, "team", True),
    # either side of a form switch
    # (epw_rt: the value arrives through LNW_EPW_RT, the others through lnw_set_epw)
    "4v4_epw17": _form(4, 100, 17, "team", True, epw_rt=True),   # second slab of one env
    "4v4_epw33": _form(4, 100, 33, "team", False),
    "3v3_epw21": _form(3, 100, 21, "team", True),                # 63 lanes
    "3v3_epw22": _form(3, 100, 22, "team", False, epw_rt=True),
    "2v2_epw33": _form(2, 100, 33, "team", False),
}


def form_sim(name, seed, steps=REACH_STEPS, **kw):
    f = FORMS[name]
    return simulate(f["nb"], f["epw"], f["G"], seed, steps, units=f["units"], red=f["red"],
                    landing_ops=f["red"] is not None, **kw)


def d5(mast_a, mast_b):
    """radar_range's horizon distance over 5 (combatant.py:235-247; KParams.d5)."""
    return math.sqrt((4.0 / 3.0) * 6370.0 * 2.0) * (math.sqrt(mast_a / 1000.0) + math.sqrt(mast_b / 1000.0)) / 5.0


def reach(duct):
    """The widest sensor reach in cells: EW between two 30 m masts."""
    return int(math.ceil(2.0 * (d5(30, 30) * duct)))


@functools.lru_cache(maxsize=None)
def max_range2(duct):
    """The predicate's bound: the largest squared radar / EW / close range over
    all ship classes, from the oracle's own range functions."""
    L = _oracle.lib()
    m = 16  # the d < 4 close range
    for ti in (_oracle.T_SMALL, _oracle.T_LARGE, _oracle.T_LS):
        for tj in (_oracle.T_SMALL, _oracle.T_LARGE, _oracle.T_LS):
            m = max(m, L.orc_radar_range(duct, ti, tj) ** 2, L.orc_ew_range(duct, ti, tj) ** 2)
    return m


def _water_box(G, direction):
    """Open water of the Baltic grids. On the 200 grid no ship moves to a cell
    past 99 (combatant.py:482-489): fleets apart along x stay where both can
    move, the others straddle y = 99 with blue on the near side, out to cells
    whose squared distances no longer fit 15 bits."""
    if G == 100:
        return (20, 78, 44, 96), 96
    return ((30, 99, 76, 99), 99) if direction == "x" else ((30, 99, 80, 150), 97)


def _probe_fleets(grid, nb, gap, direction, ahead, rng):
    """Two columns of nb water cells whose nearest ships are `gap` cells apart
    along x, along y, or diagonally (where the gap of the bounding boxes is
    smaller than the distance of the nearest pair). ahead: each column runs
    away from the other fleet, ships 2 cells apart, so that only the two lead
    ships come within reach (one EW bearing, no fix, no target list: the next
    step starts from empty lists again); else the columns face each other."""
    G = grid.shape[0]
    (x0, x1, y0, y1), by_max = _water_box(G, direction)
    if direction == "diag":
        dx = int(round(gap * 0.6))
        dy = int(round(math.sqrt(max(gap * gap - dx * dx, 0))))
    else:
        dx, dy = (gap, 0) if direction == "x" else (0, gap)
    ux, uy = (1 if dx else 0), (1 if dy else 0)  # towards red
    if ahead:
        sb, sr = (-2 * ux, -2 * uy), (2 * ux, 2 * uy)
    else:
        sb = sr = (0, 2) if direction != "y" else (2, 0)
    for _ in range(10000):
        bx, by = int(rng.integers(x0, x1)), int(rng.integers(y0, by_max))
        cells = [(bx + sb[0] * i, by + sb[1] * i) for i in range(nb)]
        cells += [(bx + dx + sr[0] * i, by + dy + sr[1] * i) for i in range(nb)]
        if all(x0 <= x <= x1 and y0 <= y <= y1 and grid[x, y] <= 74 for x, y in cells):
            return cells
    raise RuntimeError("no water cells for the probe fleets")


def _steer(toward, axis, sign):
    """Action columns (a2, a3) that move a ship `toward` cells (negative: away)
    along the gap's axis: the reference takes cos / sin of degrees(2 pi a2) as
    if it were radians (combatant.py:459-471), so a2 = theta / 360 heads theta."""
    if toward == 0:
        return 0.0, 0.0  # distance 0: the ship stays
    theta = (0.0 if axis == 0 else math.pi / 2) + (0.0 if sign * toward > 0 else math.pi)
    return theta / 360.0, abs(toward) / 3.0


def _manoeuvre(k, rng):
    """How far blue and red close (a, b; negative: open) in a step that starts
    with the fleets reach + k apart. With whole fleets moving, the combinations
    are k (old/old), k - a (blue new / red old), k - b (blue old / red new) and
    k - a - b (new/new) cells beyond the reach; the choices put exactly one of
    them inside it where k allows, or hold at the boundary."""
    choices = {
        -2: [(-2, -2), (-2, -2), (-1, -1)],                       # only old/old, or still inside
        -1: [(-1, -1), (-2, -1), (-1, -2), (-2, -2)],             # only old/old
        0: [(1, -1), (1, -1), (2, -2), (-1, 1), (0, 0), (0, 0), (1, 0), (0, 1)],  # only blue new, only red new, hold, close
        1: [(1, 1), (1, 1), (2, -1), (2, -1), (0, 0), (1, 0)],    # only new/new, only blue new, hold, up to the boundary
        2: [(2, 2), (1, 2), (2, 1), (1, 1)],                      # only new/new, or up to the boundary
        3: [(2, 2), (2, 1), (1, 2)],
    }.get(k, [(1, 1)] if k > 3 else [(-1, -1)])
    return choices[int(rng.integers(0, len(choices)))]


def layout(nb, epw, seed, grid, units=False):
    """Spawn cells [E, 2 nb, 2], per-env ducting [E] (NaN: keep the reset's
    draw), actions [S, E, 2 nb, 4] float32 (S = 45: the reach test uses the
    first 6) and the probe envs, one per workgroup (units: two per workgroup of
    four 64-env units, in different units).

    A probe's fleets start reach + k cells apart and for the first steps each
    fleet as a whole closes, opens or holds by up to 2 cells, chosen so that the
    gap stays within reach - 2 .. reach + 3 (_manoeuvre): the steps in which
    only one old / new combination of positions is inside the bound. From the
    ninth step on a probe moves at random like the other envs."""
    rng = np.random.default_rng([seed, nb, epw, grid.shape[0], int(units)])
    if units:
        assert epw == 64
        E = 512
        # (unit, lane): units 0 and 2 of workgroup 0, 1 and 3 of workgroup 1
        probes = [0 * 64 + 0, 2 * 64 + 63, 5 * 64 + 31, 7 * 64 + (seed % 64)]
    else:
        E = 2 * epw + max(1, epw // 3)
        lanes = [0, epw - 1, epw // 2]
        probes = [w * epw + lanes[(w + seed) % 3] for w in range(2)] + [E - 1]
    A = 2 * nb
    pos = np.array([ref_spawns(nb)] * E, np.int32)
    duct = np.full(E, np.nan)
    S = 45
    acts = rng.random((S, E, A, 4), dtype=np.float32)
    for i, e in enumerate(probes):
        d = DUCTS[int(rng.integers(0, 3))]
        k = KS[int(rng.integers(0, 6))]
        direction = DIRS[(i + seed) % 3]
        cells = _probe_fleets(grid, nb, reach(d) + k, direction, rng.random() < 0.7, rng)
        if rng.random() < 0.6:
            # blue's nearest ship last in turn order: the others' get_obs see it at
            # its old cell (the first ship's old cell is never looked at)
            cells[:nb] = cells[:nb][::-1]
        pos[e] = cells
        duct[e] = d
        if rng.random() < 0.85:  # EW needs the target's radar on: round(a0) = 1
            acts[:, e, :, 0] = 0.5 + 0.5 * acts[:, e, :, 0]
        axis = 1 if direction == "y" else 0  # (diagonal: along x, one component of the gap)
        for s in range(REACH_STEPS + 2):
            a, b = _manoeuvre(k, rng)
            k -= a + b
            # red lies at larger coordinates: blue closes by moving up, red by moving down
            acts[s, e, :nb, 2:] = np.float32(_steer(a, axis, +1))
            acts[s, e, nb:, 2:] = np.float32(_steer(b, axis, -1))
    return pos, duct, acts, probes


def workgroup_of(e, epw):
    return e // epw


# ---------------------------------------------------------------------------
# the predicate as DESIGN.md and SURVEY §9 Q1 state it, and its mutants
# ---------------------------------------------------------------------------
def combo_d2(before, after, nb):
    """d^2 [blue old/new, red old/new, blue ship, red ship] of a step."""
    P = np.stack([before["pos"], after["pos"]]).astype(np.int64)  # [2, A, 2]
    d = P[:, None, :nb, None, :] - P[None, :, None, nb:, :]
    return (d * d).sum(-1)


def _live_pairs(before, nb):
    al = before["alive"] != 0
    return al[:nb, None] & al[None, nb:]


def _holds_list(before):
    return bool((before["tl_cnt"][before["alive"] != 0] != 0).any())


def min_d2(before, after, nb, live=True):
    """Smallest d^2 over all four combinations of every blue / red pair alive
    before the step (live=False: of every pair with a sunk ship)."""
    m = _live_pairs(before, nb)
    D = combo_d2(before, after, nb)[:, :, m if live else ~m]
    return int(D.min()) if D.size else 1 << 40


def spec_quiet(before, after, duct, nb):
    """No live ship holds a target list, and over all four old / new combinations
    of every live blue / red pair the minimum d^2 is >= max_range2(duct)."""
    return not _holds_list(before) and min_d2(before, after, nb) >= max_range2(duct)


def mutants(before, after, duct, nb):
    """What the predicate says of this step with one old / new combination left
    out (four mutants, in COMBOS' order) and with the reach one cell short."""
    if _holds_list(before):
        return [False] * len(MUTANTS)
    r2 = max_range2(duct)
    D = combo_d2(before, after, nb)[:, :, _live_pairs(before, nb)]  # [2, 2, pairs]
    out = []
    for ub, ur in COMBOS:
        keep = np.ones((2, 2), bool)
        keep[ub, ur] = False
        out.append(bool(D.size == 0 or D[keep].min() >= r2))
    out.append(bool(D.size == 0 or D.min() >= (int(round(math.sqrt(r2))) - 1) ** 2))
    return out


def oracle_loud(before, after, ctr_before, ctr_after):
    """The oracle alone: a trained-red step without a reset drew from the env's
    Philox stream (an EW bearing's distortion), or a ship alive before the step
    holds a target list before or after it (a sunk ship keeps its last list for
    good; nothing reads it)."""
    al = before["alive"] != 0
    return bool(ctr_after != ctr_before or before["tl_cnt"][al].any() or after["tl_cnt"][al].any())


# ---------------------------------------------------------------------------
# the oracle over a layout
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def simulate(nb, epw, G, seed, steps, units=False, red=None, trained_red=True, horizon=0,
             landing_ops=False):
    """The oracle's outputs for a layout, every env and step (ctr: the env's
    Philox draw counter after the step and its reset), and what it says of
    each (step, env): loud, quiet by the stated predicate, by each mutant, the
    nearest live combination and whether a dead ship lies inside the bound.
    horizon > 0: auto-reset after a victory or `horizon` steps, as the device's
    (outputs only: the verdicts are for runs without resets).
    Cached: the tests of one form share it and leave it unchanged."""
    grid = _grid(G)
    pos, duct, acts, probes = layout(nb, epw, seed, grid, units)
    E, A = pos.shape[0], 2 * nb
    types = [_oracle.T_LARGE] * nb + [TYPE_CODES[t] for t in (red or ("large",) * nb)]
    kinds = np.full(A, _oracle.K_F32, np.int32)
    out = _oracle.new_record(steps, E, nb, nb)
    out.update(loud=np.zeros((steps, E), bool), quiet=np.zeros((steps, E), bool),
               mutant_quiet=np.zeros((len(MUTANTS), steps, E), bool),
               near2=np.zeros((steps, E), np.int64), r2=np.zeros((steps, E), np.int64),
               dead_inside=np.zeros((steps, E), bool), reset=np.zeros((steps, E), bool),
               err=np.zeros(E, np.int64), ctr=np.zeros((steps, E), np.int64))
    for e in range(E):
        o = _oracle.OracleEnv(grid, nb, nb, trained_red=trained_red, landing_ops=landing_ops)
        o.set_philox(seed, e)
        o.reset(types, pos[e])
        if not np.isnan(duct[e]):
            o.set_ducting(float(duct[e]))
        t = 0  # steps of the episode
        for s in range(steps):
            if not horizon:
                before, st0 = o.agents(), o.env_state()
            r = o.step(acts[s, e], kinds)
            _oracle.record_step(out, s, e, r)
            t += 1
            if horizon:  # (the verdicts below are for runs without resets)
                if r["done"] == 0 or t >= horizon:
                    o.reset(types, pos[e])
                    out["reset"][s, e] = True
                    t = 0
                out["ctr"][s, e] = o.env_state()["ctr"]
                continue
            after, st1 = o.agents(), o.env_state()
            out["ctr"][s, e] = st1["ctr"]
            d = st0["ducting"]
            out["loud"][s, e] = oracle_loud(before, after, st0["ctr"], st1["ctr"])
            out["quiet"][s, e] = spec_quiet(before, after, d, nb)
            out["near2"][s, e] = min_d2(before, after, nb)
            out["r2"][s, e] = max_range2(d)
            if e in probes:
                out["mutant_quiet"][:, s, e] = mutants(before, after, d, nb)
                out["dead_inside"][s, e] = (min_d2(before, after, nb, live=False) < out["r2"][s, e]
                                            <= out["near2"][s, e])
        out["err"][e] = o.env_state()["err"]
    for v in out.values():
        v.setflags(write=False)
    out.update(pos=pos, duct=duct, acts=acts, probes=probes, types=types, E=E)
    return out


def tally(sim, epw):
    """Counts over a simulated layout's probe instances (see the CPU test)."""
    E, probes = sim["E"], sim["probes"]
    S = sim["loud"].shape[0]
    t = dict(unsound=0, isolated=0, near_quiet=0, dead_inside=0, loud=0,
             kills=np.zeros(len(MUTANTS), int), candidates=np.zeros(len(MUTANTS), int))
    for e in probes:
        w = workgroup_of(e, epw)
        others = [x for x in range(w * epw, min(E, (w + 1) * epw)) if x != e]
        for s in range(S):
            loud, quiet = bool(sim["loud"][s, e]), bool(sim["quiet"][s, e])
            t["loud"] += loud
            t["dead_inside"] += bool(sim["dead_inside"][s, e])
            rch = int(round(math.sqrt(sim["r2"][s, e])))
            if quiet and not loud and sim["near2"][s, e] < (rch + 1) ** 2:
                t["near_quiet"] += 1
            # candidates: probe steps where the mutant differs from the predicate
            t["candidates"] += sim["mutant_quiet"][:, s, e] & ~quiet
            if loud and all(sim["quiet"][s, x] for x in others):
                t["isolated"] += 1
                t["kills"] += sim["mutant_quiet"][:, s, e]
    t["unsound"] = int((sim["loud"] & sim["quiet"]).sum())
    return t
