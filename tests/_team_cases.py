"""Runtime team sizes beyond config 4 (8v10): the table of cases that
tests/test_team_sizes_cpu.py runs on the oracle alone (to show from its step
statistics that each case's inputs reach the code it is built for) and
tests/test_gpu_team_sizes.py runs on the device against the oracle.

Every case: box spawns per env (the two boxes adjacent or overlapping, so the
sides are in contact every step), auto-reset, 25-step episodes, 30 steps, a
number of envs that is no multiple of 32 (the group kernel's last workgroup is
partial), float32 actions unless dtype says "f64".

kernel / form: which step kernel and which LDS form of the group kernel
(csrc/lnw_group.inc group_lds: the staged regions of "ms tls dlz atab") the
case is there for; test_gpu_team_sizes.py reads both back from the device.
"""
import functools

import numpy as np

import _oracle
from _spawns import box_positions, grid as _grid, hash_mult

STEPS, HORIZON = 30, 25
SEED = 11
TYPE = {"small": _oracle.T_SMALL, "large": _oracle.T_LARGE, "ls": _oracle.T_LS}
B100, R100 = (30, 45, 40, 60), (45, 60, 45, 65)
B200, R200 = (30, 45, 90, 120), (45, 60, 95, 125)
ALL = "ms tls dlz atab"


def _case(nb, red, G, E, kernel, form, **kw):
    red = ["large"] * red if isinstance(red, int) else red
    d = dict(blue=["small"] * nb, red=red, G=G, E=E, kernel=kernel, form=form, dtype="f32",
             landing_ops="ls" in red, trained_red=True, no_group=False, acts_after=False,
             box_b=B100 if G == 100 else B200, box_r=R100 if G == 100 else R200)
    d.update(kw)
    return d


CASES = {
    # a side of one ship; every region staged
    "1v7_g100": _case(1, 7, 100, 77, "group", ALL),
    "16v1_g100": _case(16, 1, 100, 71, "group", ALL),
    # the half bearing table no longer fits
    "1v16_g200": _case(1, 16, 200, 70, "group", "ms tls dlz"),
    "10v10_g100": _case(10, 10, 100, 90, "group", "ms tls dlz"),
    # no dist_lz stage while landing ships are in the fleet
    "11v12ls_g100": _case(11, ["large"] * 10 + ["ls"] * 2, 100, 75, "group", "ms tls"),
    # lists from HBM, dist_lz staged; float64 actions
    "12v12_g100_f64": _case(12, 12, 100, 70, "group", "ms dlz", dtype="f64"),
    # the pooled slopes alone
    "13v13_g100": _case(13, 13, 100, 70, "group", "ms"),
    "7v16ls_g200": _case(7, ["large"] * 14 + ["ls"] * 2, 200, 70, "group", "ms"),
    # no room for the pooled slopes: the one-lane kernel, with landing ships and at the largest
    # square fleet that loads
    "8v16ls_g200": _case(8, ["large"] * 14 + ["ls"] * 2, 200, 70, "generic", None),
    "15v15_g100": _case(15, 15, 100, 70, "generic", None),
    # the one-lane kernel by request
    "12v12_g100_lane": _case(12, 12, 100, 70, "generic", None, no_group=True),
    # more blue than red, untrained red: salvo draws written back into the action rows
    "14v9_g100_untrained": _case(14, 9, 100, 70, "group", "ms dlz", trained_red=False, acts_after=True),
}
# the cases whose target lists and env state are compared for the first TLIST_ENVS envs ...
TLIST_CASES = ("12v12_g100_f64", "13v13_g100")
TLIST_ENVS = 8
# ... after this many steps: early in the first episode, one step after the
# horizon's auto-reset (the longest lists: every ship alive again) and at the end
TLIST_STEPS = (3, 26, 30)


def grid(cs):
    return _grid(cs["G"])


def types(cs):
    return [TYPE[t] for t in cs["blue"] + cs["red"]]


def positions(cs):
    return box_positions(grid(cs), cs["E"], len(cs["blue"]), len(cs["red"]), 5, cs["box_b"], cs["box_r"])


def actions(cs):
    """[STEPS, E, A, 4]: float32 draws, or float64 draws that no float32 holds."""
    A = len(cs["blue"]) + len(cs["red"])
    rng = np.random.default_rng(3)
    if cs["dtype"] == "f32":
        return rng.random((STEPS, cs["E"], A, 4), dtype=np.float32)
    return rng.random((STEPS, cs["E"], A, 4))


def mult(cs):
    nb, nr = len(cs["blue"]), len(cs["red"])
    return hash_mult(nb * (4 * nb + 52) + nr * (4 * nr + 52), seed=9)


def _hash(ob, orr, m):
    w = np.concatenate([ob.astype(np.float32).ravel(), orr.astype(np.float32).ravel()])
    return np.sum(w.view(np.uint32).astype(np.uint64) * m.astype(np.uint64), dtype=np.uint64)


def per_env(cs, envs, acts=None, snap=()):
    """The envs `envs` stepped one by one (OracleEnv under Philox, auto-reset
    as the device does), with the action rows' own kind. Returns what
    _oracle.fullsize returns for those envs and, under "snap", per env and per
    step count in `snap` the state that many steps (and their auto-reset) left:
    every agent's target list, agents() and env_state()."""
    nb, nr = len(cs["blue"]), len(cs["red"])
    A = nb + nr
    acts = actions(cs) if acts is None else acts
    kind = np.full(A, _oracle.K_F32 if cs["dtype"] == "f32" else _oracle.K_F64, np.int32)
    pos, ty, m, g = positions(cs), types(cs), mult(cs), grid(cs)
    n = len(envs)
    out = dict(hash=np.zeros((STEPS, n), np.uint64), rew=np.zeros((STEPS, n, A), np.float32),
               done=np.zeros((STEPS, n), np.int32), cog=np.zeros((STEPS, n), np.float32),
               acts_after=np.zeros((STEPS, n, A, 4), acts.dtype), stats=np.zeros((n, len(_oracle.STATS)), np.int64),
               snap=[{} for _ in envs])
    for i, e in enumerate(envs):
        o = _oracle.OracleEnv(g, nb, nr, landing_ops=cs["landing_ops"], trained_red=cs["trained_red"])
        o.set_philox(SEED, e)
        o.reset(ty, pos[e])
        resets = 0
        for s in range(STEPS):
            r = o.step(acts[s, e], kind)
            out["hash"][s, i] = _hash(r["obs_blue"], r["obs_red"], m)
            out["rew"][s, i] = np.concatenate([r["rew_blue"], r["rew_red"]])
            out["done"][s, i] = r["done"]
            out["cog"][s, i] = r["cog"]
            out["acts_after"][s, i] = r["actions_after"]
            if r["done"] == 0 or o.env_state()["steps_done"] >= HORIZON:
                o.reset(ty, pos[e])
                resets += 1
            if s + 1 in snap:
                out["snap"][i][s + 1] = dict(tlists=[[(int(x), int(y)) for x, y in o.tlist(a)] for a in range(A)],
                                             agents=o.agents(), env=o.env_state())
        st = o.stats()
        st["resets"] = resets
        out["stats"][i] = [st[k] for k in _oracle.STATS]
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The oracle's record of a case, computed once: hash, rew, done, cog
    [STEPS, E(, A)], acts_after [STEPS, E, A, 4] and stats [E, len(STATS)]."""
    cs = CASES[name]
    nb, nr = len(cs["blue"]), len(cs["red"])
    if cs["dtype"] == "f64":
        r = per_env(cs, range(cs["E"]))
        del r["snap"]
        return r
    h, rew, done, cog, aft, st = _oracle.fullsize(
        grid(cs), nb, nr, types(cs), positions(cs), actions(cs), mult(cs), SEED, HORIZON, pos_per_env=True,
        landing_ops=cs["landing_ops"], trained_red=cs["trained_red"], acts_after=True, stats=True)
    return dict(hash=h, rew=rew, done=done, cog=cog, acts_after=aft, stats=st)


def stat_sums(name):
    """A case's statistics over its envs: counts summed, tl_max the maximum,
    err the OR."""
    st = oracle_run(name)["stats"]
    d = dict(zip(_oracle.STATS, st.sum(0).tolist()))
    d["tl_max"] = int(st[:, _oracle.STATS.index("tl_max")].max())
    d["err"] = int(np.bitwise_or.reduce(st[:, _oracle.STATS.index("err")]))
    return d
