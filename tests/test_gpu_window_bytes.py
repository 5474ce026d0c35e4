"""Observation rows of every reader of the window tables (csrc/lnw_window.h:
byte records, converted where the units kernel's stream builds its rows; the
other readers load float records the host derives from the same bytes)
against the CPU oracle, bit for bit.

One case per reader: the units kernel's shared stream (quiet_emit_units_t),
the one-unit quiet path staged, in two slabs and direct (quiet_emit_t,
quiet_step_t), wave 1's phase-S emission line-aligned and by row pieces
(emit_rows_al4_t, emit_rows_t: 2v2 and a 3v3 with a landing ship), phase O
(write_obs_t, under los_mode 1), the runtime-size kernels (build_row under
LNW_FORCE_GENERIC; group_rows with a side of medium Combatants and with
8v10+2LS on the 200 grid).

The terrain is the fixture grid with its cell values dealt again: every cell
keeps its side of the movement (74) and EW (70) thresholds, so the oracle's
trajectory is the fixture's, and the cells that show in some window of the
run are dealt their values first, so that every byte value the thresholds
allow shows in the windows. What the inputs must exercise is asserted from the
oracle's rows alone before the device is touched (_check_conditions): every
byte value of the grid seen, every window class of the fleet, off-grid zeros
beside non-zero cells, ships starting within 3 cells of an edge (on the 200
grid at x >= 97 and x >= 100), sunk ships' rows on both sides in the contact
case. Needs an MI355X."""
import functools

import numpy as np
import pytest

import _device as D
import _oracle
import _quiet_cases as Q
from _spawns import box_positions, grid as _grid

pytestmark = pytest.mark.gpu

CODES = {"small": _oracle.T_SMALL, "large": _oracle.T_LARGE, "ls": _oracle.T_LS, "medium": _oracle.T_MEDIUM}
# a loud arena at the grid's upper edge: water pockets between islands, blue
# from row 0 on (windows leave the grid), red a few cells east of it
BOX_B, BOX_R = (0, 14, 50, 68), (2, 15, 60, 84)
# the 200 grid: no cell past 99 shows in a window, in either direction. Blue
# stands among the islands of the north-west, red in open water on both sides of
# row 99 (the fleets do not meet: this case is about the windows)
BOX_B200, BOX_R200 = (62, 78, 42, 64), (95, 106, 60, 94)


def _case(blue, red, E, *, form=None, epw=None, contact=False, env=(), los_mode=0, G=100, landing_ops=False,
          kernel=None, steps=6):
    return dict(steps=steps, blue=list(blue), red=list(red), E=E, form=form, epw=epw, contact=contact, env=tuple(env),
                los_mode=los_mode, G=G, landing_ops=landing_ops, kernel=kernel)


L4, S4 = ["large"] * 4, ["small"] * 4
CASES = {
    # quiet workgroups: the launch forms of _quiet_cases (layouts, probes and actions from there)
    "4v4_units": _case(L4, L4, 512, form="4v4_units", kernel="UNITS"),
    "4v4_epw64_staged": _case(L4, L4, None, form="4v4_epw64_staged", kernel="TEAM"),
    "4v4_epw32_two_slab": _case(L4, L4, None, form="4v4_epw32_two_slab", kernel="TEAM", steps=8),
    "4v4_epw16": _case(L4, L4, None, form="4v4_epw16", kernel="TEAM"),
    # loud workgroups at 64 envs per workgroup: wave 1 emits the rows during phase S
    "4v4_contact_melee_epw64": _case(S4, L4, 128, epw=64, contact=True, kernel="TEAM_CONTACT"),
    "2v2_epw64": _case(["small"] * 2, ["large"] * 2, 128, epw=64, kernel="TEAM"),
    "3v3_ls_epw64": _case(["small"] * 3, ["large", "large", "ls"], 128, epw=64, kernel="TEAM"),
    # phase O: the ray-march mode writes the rows after phase S
    "4v4_los1_phase_o": _case(S4, L4, 100, epw=64, los_mode=1, kernel="TEAM"),
    # the runtime-size kernels
    "3v3_medium_side": _case(["medium"] * 3, ["large"] * 3, 96, kernel="GROUP"),
    "4v4_force_generic": _case(S4, L4, 72, env=("LNW_FORCE_GENERIC",), kernel="GENERIC"),
    "8v10ls_g200": _case(["small"] * 8, ["large"] * 8 + ["ls"] * 2, 32, G=200, landing_ops=True, kernel="GROUP"),
}


def _classes(grid):
    """Each cell's side of the two thresholds: 0 open (<= 70), 1 (71..74: passable, blocks EW), 2 land."""
    return (grid > 70).astype(np.int8) + (grid > 74)


ALLOWED = (np.arange(0, 71), np.arange(71, 75), np.arange(75, 256))


def redeal(grid, shown):
    """The grid with every cell's value dealt again inside its threshold class:
    the cells of a class take the class's values in turn, the cells that show
    in some window of the run (shown [G, G]: the trajectory does not depend on
    the values) first, so those hold every value if there are enough of them."""
    cls = _classes(grid)
    out = grid.copy()
    for c, vals in enumerate(ALLOWED):
        m = np.flatnonzero(cls.ravel() == c)
        order = m[np.argsort(~shown.ravel()[m], kind="stable")]
        out.ravel()[order] = vals[np.arange(order.size) % vals.size]
    assert np.array_equal(_classes(out), cls)
    return out


@functools.lru_cache(maxsize=None)
def inputs(name):
    """grid (dealt again), pos [E, A, 2], acts [steps, E, A, 4] float32, per-env
    ducting (NaN: the reset's draw) and the seed. Cached and left unchanged."""
    cs = CASES[name]
    nb, nr = len(cs["blue"]), len(cs["red"])
    base = _grid(cs["G"])
    if cs["form"]:
        sim = Q.form_sim(cs["form"], Q.REACH_SEEDS[0])
        pos, duct, acts, seed = sim["pos"], sim["duct"], sim["acts"][:cs["steps"]], Q.REACH_SEEDS[0]
    else:
        seed = 11
        box_b, box_r = (BOX_B200, BOX_R200) if cs["G"] == 200 else (BOX_B, BOX_R)
        pos = box_positions(base, cs["E"], nb, nr, 5, box_b, box_r)
        duct = np.full(cs["E"], np.nan)
        acts = np.random.default_rng(100 + nb).random((cs["steps"], cs["E"], nb + nr, 4), dtype=np.float32)
    # the cells that show in a window, from a run on the fixture's own values
    shown = np.zeros(base.shape, bool)
    for side, rows in zip(("blue", "red"), _oracle_run(cs, base, pos, acts, duct, seed)):
        for k, t in enumerate(cs[side]):
            n, back = WIN[t]
            r = rows[:, :, k].reshape(-1, rows.shape[-1])
            px = np.rint(r[:, n * n].astype(np.float64) * cs["G"]).astype(np.int64)
            py = np.rint(r[:, n * n + 1].astype(np.float64) * cs["G"]).astype(np.int64)
            i, j = np.divmod(np.arange(n * n), n)
            cx, cy = px[:, None] - back + i[None], py[:, None] - back + j[None]
            ok = (cx >= 0) & (cy >= 0) & (cx <= 99) & (cy <= 99) & r.any(axis=1)[:, None]
            shown[cx[ok], cy[ok]] = True
    grid = redeal(base, shown)
    for a in (grid, pos, acts, duct):
        a.setflags(write=False)
    return dict(grid=grid, pos=pos, acts=acts, duct=duct, seed=seed, E=pos.shape[0])


@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    """The oracle's observation rows [steps, E, n, D] per side on the case's inputs."""
    inp = inputs(name)
    ob, orr = _oracle_run(CASES[name], inp["grid"], inp["pos"], inp["acts"], inp["duct"], inp["seed"])
    ob.setflags(write=False)
    orr.setflags(write=False)
    return ob, orr


def _oracle_run(cs, grid, pos, acts, duct, seed):
    inp = dict(grid=grid, pos=pos, acts=acts, duct=duct, seed=seed, E=pos.shape[0])
    nb, nr = len(cs["blue"]), len(cs["red"])
    types = [CODES[t] for t in cs["blue"] + cs["red"]]
    kinds = np.full(nb + nr, _oracle.K_F32, np.int32)
    ob = orr = None
    for e in range(inp["E"]):
        o = _oracle.OracleEnv(inp["grid"], nb, nr, landing_ops=cs["landing_ops"])
        o.set_philox(inp["seed"], e)
        o.reset(types, inp["pos"][e])
        if not np.isnan(inp["duct"][e]):
            o.set_ducting(float(inp["duct"][e]))
        for s in range(acts.shape[0]):
            r = o.step(inp["acts"][s, e], kinds)
            if ob is None:
                ob = np.zeros((acts.shape[0], inp["E"]) + r["obs_blue"].shape, np.float32)
                orr = np.zeros((acts.shape[0], inp["E"]) + r["obs_red"].shape, np.float32)
            ob[s, e], orr[s, e] = r["obs_blue"], r["obs_red"]
        assert o.env_state()["err"] == 0
    return ob, orr


WIN = {"small": (7, 3), "large": (7, 3), "ls": (5, 1), "medium": (5, 2)}  # side, cells behind the ship


def conditions(name):
    """What the case's inputs exercise, from the oracle's rows alone: the byte
    values seen in live rows' windows, the window classes that occur, whether a
    window holds off-grid zeros beside non-zero cells, all-zero rows per side."""
    cs, inp = CASES[name], inputs(name)
    G = cs["G"]
    seen = np.zeros(256, bool)
    classes, edge, zero_rows = set(), 0, []
    for side, rows in zip(("blue", "red"), oracle_rows(name)):
        zero_rows.append(int((~rows.any(axis=-1)).sum()))
        for k, t in enumerate(cs[side]):
            n, back = WIN[t]
            r = rows[:, :, k].reshape(-1, rows.shape[-1])
            r = r[r.any(axis=1)]  # live rows
            if not len(r):
                continue
            classes.add((n, back))
            w = r[:, :n * n].astype(np.float64) * 255.0
            b = np.rint(w).astype(np.int64)
            assert np.array_equal((b / 255.0).astype(np.float32), r[:, :n * n]), (name, side, k)
            seen[np.unique(b)] = True
            # the ship's cell from its own row (x / G, y / G follow the window)
            px = np.rint(r[:, n * n].astype(np.float64) * G).astype(np.int64)
            py = np.rint(r[:, n * n + 1].astype(np.float64) * G).astype(np.int64)
            i, j = np.divmod(np.arange(n * n), n)
            cx, cy = px[:, None] - back + i[None], py[:, None] - back + j[None]
            off = (cx < 0) | (cy < 0) | (cx > 99) | (cy > 99)
            assert not b[off].any(), (name, side, k, "an off-grid window entry is not 0")
            edge += int((off.any(axis=1) & (np.where(off, 0, b) > 0).any(axis=1)).sum())
    return dict(seen=seen, classes=classes, edge=edge, zero_rows=zero_rows)


def _check_conditions(name):
    cs, inp = CASES[name], inputs(name)
    c = conditions(name)
    pos = inp["pos"]
    near = (pos.min(axis=-1) <= 3) | (pos.max(axis=-1) >= 96 if cs["G"] == 100 else (pos[..., 0] >= 96))
    assert near.any(), (name, "no ship starts within 3 cells of a grid edge")
    if cs["G"] == 200:
        assert (pos[..., 0] >= 100).any() and ((pos[..., 0] >= 97) & (pos[..., 0] < 100)).any()
    present = np.zeros(256, bool)
    present[np.unique(inp["grid"][:100, :100])] = True  # (no cell past 99 shows in a window)
    missing = np.flatnonzero(present & ~c["seen"])
    assert missing.size == 0, (name, "byte values never seen in a window", missing.tolist())
    assert present.sum() == 256, name  # every value the thresholds allow is in the grid
    assert c["classes"] == {WIN[t] for t in cs["blue"] + cs["red"]}, (name, c["classes"])
    assert c["edge"] > 0, (name, "no window with off-grid zeros beside non-zero cells")
    if cs["contact"]:
        assert min(c["zero_rows"]) > 0, (name, "a side without a sunk ship's row", c["zero_rows"])


def test_every_window_class_is_covered():
    assert {WIN[t] for cs in CASES.values() for t in cs["blue"] + cs["red"]} == {(7, 3), (5, 1), (5, 2)}


@pytest.mark.parametrize("name", list(CASES))
def test_rows_equal_oracle(name, monkeypatch):
    from lnw.config import Scenario
    cs, inp = CASES[name], inputs(name)
    want = dict(zip(("obs_blue", "obs_red"), oracle_rows(name)))
    _check_conditions(name)  # from the oracle's rows alone, before any device call
    f = Q.FORMS[cs["form"]] if cs["form"] else None
    env = list(cs["env"]) + ([f["env"]] if f and f["env"] else [])
    sc = Scenario(landing_ops=cs["landing_ops"], los_mode=cs["los_mode"])
    g = D.make_game(monkeypatch, inp["E"], cs["blue"], cs["red"], sc, inp["grid"], inp["seed"],
                    env=dict.fromkeys(env, "1"), epw=f["epw"] if f else cs["epw"], contact=cs["contact"])
    D.start(g, inp["pos"], seed=inp["seed"], duct=inp["duct"])
    for s in range(cs["steps"]):
        D.assert_step(D.step(g, inp["acts"][s]), want, s, name)  # the rows alone, bit for bit
    assert g.step_kernel() == D.kernel_code(cs["kernel"])
    assert not g.env_state()["err"].any()
    g.close()
