"""Action rows for phase M's float32 path (csrc/lnw_kernels.hip move_stages_f32
and move_batch_t), and the CPU oracle's record of stepping them. Host only:
numpy and _oracle.

TEST INFRASTRUCTURE: shared by tests/test_move_rows_cpu.py (which shows on the
CPU that every class of row is there in numbers, inside single waves, and that
the rows move ships, get refused and raise error flags) and
tests/test_gpu_move_interleave.py (which runs them through the launch forms).

Phase M takes the (env, agent) pairs of a workgroup 64 at a time: pass p, lane l
is pair 64 p + l (env q / A, agent q % A). The float polynomials certify most
rows' target cells (move_cell_f32_fast, csrc/lnw_device.h); the others take the
double sincos. The rows below mix, pair by pair at random and at a rate that
changes every 8 envs (EXOTIC_RATE), every way a row can leave the common path,
so that single lanes of a pass fall back, whole passes do not, and the passes of
one lane go different ways.
"""
import functools

import numpy as np

import _oracle
from _spawns import grid, ref_spawns

STEPS = 12
E_SIM = 512
SEED = 20
# what a 64-env block of the layout holds (the units kernel: one unit each)
BLOCKS = ("ref", "melee", "ref", "mixed", "melee", "ref", "mixed", "ref")
CLASSES = ("plain", "tie", "quarter_tie", "far_deg", "far_dist", "nonfinite", "wide")
# share of rows that are not plain, by (env // 8 + step) % 3: a pass of 64 pairs
# covers 8 envs at 4v4, so there are passes that never leave the common path,
# passes in which a lane or two fall back, and passes in which many do
EXOTIC_RATE = (0.0, 0.03, 0.42)
TEAMS = {
    # name: (blue types, red types, landing_ops)
    "4v4": (("small",) * 4, ("large",) * 4, False),
    "3v3_ls": (("large",) * 3, ("large", "large", "ls"), True),
}
TYPE_CODES = {"small": _oracle.T_SMALL, "large": _oracle.T_LARGE, "ls": _oracle.T_LS}
SPEED = {_oracle.T_SMALL: 3, _oracle.T_LARGE: 3, _oracle.T_LS: 2, _oracle.T_MEDIUM: 2}
RAD2DEG = 180.0 / 3.141592653589793
TIE_BAND = 4e-5  # move_cell_f32_fast's distance from a half-integer
TIE_MARGIN = 4e-6  # the polynomials' error on a coordinate (3e-5 is the proven bound; typical 1e-6)


def types_of(team):
    b, r, _ = TEAMS[team]
    return [TYPE_CODES[t] for t in b + r]


def _melee(g, n, nb, rng):
    """Fleets a few cells apart in open water: they fight from the first step."""
    wb = np.argwhere(g[40:50, 45:60] <= 74) + np.array([40, 45])
    wr = np.argwhere(g[52:62, 45:60] <= 74) + np.array([52, 45])
    return np.concatenate([wb[rng.integers(0, len(wb), (n, nb))], wr[rng.integers(0, len(wr), (n, nb))]],
                          1).astype(np.int32)


def positions(team):
    nb = len(TEAMS[team][0])
    g = grid()
    rng = np.random.default_rng([SEED, nb, 1])
    pos = np.array([ref_spawns(nb)] * E_SIM, np.int32)
    for b, kind in enumerate(BLOCKS):
        e0 = 64 * b
        if kind == "melee":
            pos[e0:e0 + 64] = _melee(g, 64, nb, rng)
        elif kind == "mixed":
            pos[e0 + 32:e0 + 64] = _melee(g, 32, nb, rng)
    return pos


def rows(team):
    """acts [STEPS, E_SIM, A, 4] float32 and each row's class [STEPS, E_SIM, A]
    (index into CLASSES). Columns 0 and 1 (radar, engagement) stay plain, on the
    high side so that fleets in reach fire."""
    types = np.array(types_of(team))
    A = len(types)
    rng = np.random.default_rng([SEED, A, 2])
    shape = (STEPS, E_SIM, A)
    acts = rng.random(shape + (4,), dtype=np.float32)
    acts[..., :2] = 0.5 + 0.5 * acts[..., :2]
    rate = np.array(EXOTIC_RATE)[(np.arange(E_SIM)[None, :] // 8 + np.arange(STEPS)[:, None]) % 3]
    exotic = rng.random(shape) < rate[..., None]
    cls = np.where(exotic, rng.integers(1, len(CLASSES), shape), 0).astype(np.int8)
    a2, a3 = acts[..., 2].copy(), acts[..., 3].copy()
    u = rng.random(shape)
    v = rng.random(shape)
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    # half-integer ties: dist = speed * a3 = 0.5 exactly, heading 0 ...
    half = np.where(types == _oracle.T_LS, np.float32(0.25), np.float32(1.0 / 6.0)).astype(np.float32)
    m = cls == CLASSES.index("tie")
    a2[m] = 0.0
    a3[m] = np.broadcast_to(half, shape)[m]
    # ... and at quarter turns: degrees(2 pi a2) = q pi / 2 to float32's precision
    m = cls == CLASSES.index("quarter_tie")
    quarter = (1 + (u * 3).astype(np.int64)) * (np.pi / 2) / (2 * np.pi * RAD2DEG)
    a2[m] = quarter[m].astype(np.float32)
    a3[m] = np.broadcast_to(half, shape)[m]
    # |deg| >= 1e5: |a2| >= 278
    m = cls == CLASSES.index("far_deg")
    a2[m] = (sign * (300.0 + 5000.0 * u))[m].astype(np.float32)
    # |dist| > 4 for every speed: targets beyond the move table's +-4 window (the A* pass)
    m = cls == CLASSES.index("far_dist")
    a3[m] = (sign * (2.1 + 2.0 * v))[m].astype(np.float32)
    # NaN and +-inf in a2 or a3
    m = cls == CLASSES.index("nonfinite")
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)[(u * 3).astype(np.int64)]
    a2[m & (v < 0.5)] = bad[m & (v < 0.5)]
    a3[m & (v >= 0.5)] = bad[m & (v >= 0.5)]
    # in range but far from [0, 1]: many turns either way, backwards, up to |dist| = 4
    m = cls == CLASSES.index("wide")
    a2[m] = (sign * 250.0 * u)[m].astype(np.float32)
    a3[m] = ((2.0 * v - 1.0) * 1.3)[m].astype(np.float32)
    acts[..., 2], acts[..., 3] = a2, a3
    return acts, cls


def fast_verdict(px, py, speed, a2, a3):
    """move_cell_f32_fast's conditions restated in numpy for float32 rows
    (continuous_to_discrete as move_target_dev has it): +1 where the float
    polynomials certainly certify the cell, -1 where they certainly do not, 0
    within TIE_MARGIN of the band's edge (left out of every count). Also the
    cell (where finite) and whether the row is finite at all."""
    a2 = np.asarray(a2, np.float32)
    a3 = np.asarray(a3, np.float32)
    with np.errstate(all="ignore"):
        course = np.float32(2.0 * 3.141592653589793) * a2
        dist = np.asarray(speed).astype(np.float32) * a3
        deg = course.astype(np.float64) * RAD2DEG
        in_range = (np.abs(deg) < 1.0e5) & (np.abs(dist) <= np.float32(4.0))
        c, s = np.cos(deg).astype(np.float32), np.sin(deg).astype(np.float32)
        fx = np.asarray(px).astype(np.float32) + c * dist
        fy = np.asarray(py).astype(np.float32) + s * dist
        small = (np.abs(fx) < 256) & (np.abs(fy) < 256)
        rx, ry = np.rint(fx), np.rint(fy)
        off = np.minimum(np.abs(np.abs(fx - rx) - np.float32(0.5)), np.abs(np.abs(fy - ry) - np.float32(0.5)))
        finite = np.isfinite(rx) & np.isfinite(ry)
    sure = in_range & small & (off >= TIE_BAND + TIE_MARGIN)
    unsure = ~(in_range & small) | (off < TIE_BAND - TIE_MARGIN)
    verdict = np.where(sure, 1, np.where(unsure, -1, 0)).astype(np.int8)
    big = ~finite | (np.abs(rx) >= 1e6) | (np.abs(ry) >= 1e6)
    cell = np.stack([np.where(big, -1000000, rx), np.where(big, -1000000, ry)], -1).astype(np.int64)
    return verdict, cell, finite


@functools.lru_cache(maxsize=None)
def simulate(team):
    """The oracle over every env and step of the team's rows: outputs, the ships'
    cells and alive flags before and after each step, and the error flags after
    it. Cached: the tests share it and leave it unchanged."""
    g = grid()
    blue, red, landing = TEAMS[team]
    nb, A = len(blue), len(blue) + len(red)
    types = types_of(team)
    pos = positions(team)
    acts, cls = rows(team)
    kinds = np.full(A, _oracle.K_F32, np.int32)
    S, E = STEPS, E_SIM
    out = _oracle.new_record(S, E, nb, nb)
    out.update(pos_before=np.zeros((S, E, A, 2), np.int32), pos_after=np.zeros((S, E, A, 2), np.int32),
               alive_before=np.zeros((S, E, A), bool), err=np.zeros((S, E), np.uint32))
    for e in range(E):
        o = _oracle.OracleEnv(g, nb, nb, landing_ops=landing)
        o.set_philox(SEED, e)
        o.reset(types, pos[e])
        ag = o.agents()
        for s in range(S):
            out["pos_before"][s, e], out["alive_before"][s, e] = ag["pos"], ag["alive"] != 0
            r = o.step(acts[s, e], kinds)
            _oracle.record_step(out, s, e, r)
            ag = o.agents()
            out["pos_after"][s, e] = ag["pos"]
            out["err"][s, e] = o.env_state()["err"]
    out.update(acts=acts, cls=cls, pos=pos)
    for v in out.values():
        v.setflags(write=False)
    out.update(types=types, nb=nb, A=A, landing=landing)
    return out
