"""Runtime team sizes beyond config 4 (8v10) against the CPU oracle: the group
kernel (csrc/lnw_group.inc) in each of its LDS forms and the one-lane kernel
step_kernel<0, 0>, on the cases of tests/_team_cases.py.

Above 8v10 three things become live that no smaller fleet reaches: EW fixes
averaged over 8 and more points (numpy's pairwise sum, FixAcc16), target lists
longer than the 16 entries the group kernel stages in LDS, and the LDS forms
in which an optional region (target lists, dist_lz, the half bearing table,
the pooled slopes) no longer fits and its readers go to HBM.
tests/test_team_sizes_cpu.py shows on the oracle alone that every case reaches
what it is there for.

Per case, every env and step: the observation hash, rewards (1e-5), done and
cog as tests/test_gpu_fullsize.py compares them, the env's error flags, and for
the untrained red the action rows after each step. Which kernel ran comes from
step_kernel(), which LDS form from the LNW_PROF report of a one-step handle of
the same shape.

The order in which a fix's points are summed shows in no random episode (a
step holds the fix only as a rounded cell): tests/_fix_order_cases.py builds
the rounding ties that show it, in tape mode. Last, the size limit of
include/lnw.h (a side of 16 against 10 or more is refused). Needs an MI355X."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import _device as D
import _fix_order_cases as F
import _oracle
import _team_cases as T
from _fullsize_util import _compare, _gpu_run
from _spawns import grid as _grid

pytestmark = pytest.mark.gpu

NAMES = sorted(T.CASES)
LDS_LINE = re.compile(r"\[lnw prof\] group kernel LDS (\d+) B \(staged: target lists (\d), dist_lz (\d), "
                      r"bearing half table (\d), pooled slopes (\d)\)")
# every form of the launch for runtime sizes: the group kernel's five LDS forms, and the one-lane kernel
WANTED = {("group", T.ALL), ("group", "ms tls dlz"), ("group", "ms tls"), ("group", "ms dlz"), ("group", "ms"),
          ("generic", None)}


def _game(cs, monkeypatch, E, prof=False):
    """A handle of the case's shape (LNW_NO_GROUP and LNW_PROF are read once, by
    lnw_create: set around it), reset to the case's spawns."""
    from lnw.config import Scenario
    env = {}
    if cs["no_group"]:
        env["LNW_NO_GROUP"] = "1"
    if prof:
        env["LNW_PROF"] = "1"
    sc = Scenario(landing_ops=cs["landing_ops"], auto_reset=True, episode_steps=T.HORIZON,
                  trained_red=cs["trained_red"])
    g = D.make_game(monkeypatch, E, cs["blue"], cs["red"], sc, T.grid(cs), T.SEED, env=env)
    D.start(g, T.positions(cs))
    return g


def _form_ran(cs, monkeypatch, capfd):
    """(kernel, LDS form) of one step of a 33-env handle of the case's shape under LNW_PROF."""
    g = _game(cs, monkeypatch, 33, prof=True)
    capfd.readouterr()
    act = torch.from_numpy(T.actions(cs)[0, :33]).cuda()
    g.step(act)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    kernel = next((k for k in ("group", "generic") if g.step_kernel() == D.kernel_code(k)), g.step_kernel())
    g.close()
    m = LDS_LINE.search(err)
    if kernel != "group":
        assert m is None, err
        return kernel, None
    assert m, err
    tls, dlz, atab, ms = (int(v) for v in m.groups()[1:])
    assert int(m.group(1)) <= 158 * 1024
    return kernel, " ".join(n for n, on in (("ms", ms), ("tls", tls), ("dlz", dlz), ("atab", atab)) if on)


@pytest.mark.parametrize("name", NAMES)
def test_case_matches_oracle(name, monkeypatch, capfd):
    cs = T.CASES[name]
    ran = _form_ran(cs, monkeypatch, capfd)
    assert ran == (cs["kernel"], cs["form"]), (name, ran)
    orc = T.oracle_run(name)
    acts = T.actions(cs)
    g = _game(cs, monkeypatch, cs["E"])
    gpu = _gpu_run(g, acts, T.mult(cs), after=True)
    assert g.step_kernel() == D.kernel_code(cs["kernel"])
    err = g.env_state()["err"]
    g.close()
    _compare(gpu[:4], (orc["hash"], orc["rew"], orc["done"], orc["cog"]), name)
    # equal slopes are legal and set ZERODIV on both sides: equal flags, not zero flags
    want = orc["stats"][:, _oracle.STATS.index("err")]
    assert np.array_equal(err.astype(np.int64), want), (name, "error flags", np.argwhere(err != want)[:4].tolist())
    if cs["acts_after"]:
        bad = (gpu[4] != orc["acts_after"]).any(axis=(2, 3))
        assert not bad.any(), (name, "action rows after the step", np.argwhere(bad)[:4].tolist())
        assert not np.array_equal(gpu[4], acts)


@pytest.mark.parametrize("name", T.TLIST_CASES)
def test_target_lists_and_state(name, monkeypatch):
    """The first envs' state after 3, 26 and all 30 steps: every agent's target
    list (lists of more than 16 entries among them, which no LDS stage holds
    whole) and the env state, against the same envs stepped one by one on the
    oracle."""
    cs = T.CASES[name]
    n = T.TLIST_ENVS
    acts = T.actions(cs)
    one = T.per_env(cs, range(n), acts, snap=T.TLIST_STEPS)
    g = _game(cs, monkeypatch, cs["E"])
    longest = 0
    for s in range(T.STEPS):
        g.step(torch.from_numpy(acts[s]).cuda())
        if s + 1 not in T.TLIST_STEPS:
            continue
        es, ag = g.env_state(), g.agents()
        for e in range(n):
            tag = (name, "after step", s + 1, "env", e)
            ref = one["snap"][e][s + 1]
            lists = g.tlists(e)
            for a, want in enumerate(ref["tlists"]):
                assert lists[a] == want, tag + ("target list of agent", a)
                longest = max(longest, len(want))
            ost, oag = ref["env"], ref["agents"]
            assert np.array_equal(ag["tl_cnt"][e], oag["tl_cnt"]), tag
            assert np.array_equal(np.stack([ag["x"][e], ag["y"][e]], 1), oag["pos"]), tag
            assert np.array_equal(ag["alive"][e], oag["alive"]), tag
            assert np.array_equal(ag["missiles"][e].astype(np.float64), oag["missiles"]), tag
            for dk, ok in (("n_blue_left", "n_blue_left"), ("n_red_left", "n_red_left"), ("steps_done", "steps_done"),
                           ("blue_victory", "blue_victory"), ("red_victory", "red_victory"),
                           ("blue_engagements", "blue_eng"), ("red_engagements", "red_eng")):
                assert es[dk][e] == ost[ok], tag + (dk,)
            assert es["ducting"][e] == ost["ducting"] and es["rng"][e] == ost["ctr"] and es["err"][e] == ost["err"], tag
    g.close()
    assert longest > 16, longest


def test_every_form_ran(monkeypatch, capfd):
    """Over the table, all five LDS forms of the group kernel and the one-lane
    kernel run, each where the table says (test_case_matches_oracle holds each
    case to the oracle in that form)."""
    ran = {name: _form_ran(T.CASES[name], monkeypatch, capfd) for name in NAMES}
    assert ran == {name: (T.CASES[name]["kernel"], T.CASES[name]["form"]) for name in NAMES}, ran
    assert set(ran.values()) >= WANTED, sorted(map(str, ran.values()))


@pytest.mark.parametrize("no_group", [False, True])
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_fix_mean_sums_in_numpy_order(name, no_group, monkeypatch):
    """tests/_fix_order_cases.py: fixes over 8, 9, 12 and 15 points whose cell
    is a target only if the points are summed in numpy's order (FixAcc16 of
    the group kernel, FixAcc of the one-lane kernel). 33 envs on the same
    tape: observations bit for bit, rewards, target-list counts, the tape
    position and the error flags against the oracle's step."""
    from lnw.config import Scenario
    c = F.CASES[name]
    n, E = len(c["blue"]), 33
    r, o = F.oracle_step(c)
    g = D.make_game(monkeypatch, E, ["small"] * n, ["large"], Scenario(landing_ops=False), _grid(100),
                    env={"LNW_NO_GROUP": "1"} if no_group else None)
    tape = F.tape(c)
    D.start(g, np.tile(F.positions(c), (E, 1, 1)),
            tape=(np.tile(tape, E), np.arange(E + 1, dtype=np.int64) * len(tape)))
    out = {k: v.cpu().numpy() for k, v in g.step(torch.zeros((E, n + 1, 4), dtype=torch.float32).cuda()).items()}
    assert g.step_kernel() == D.kernel_code("generic" if no_group else "group")
    es, cnt = g.env_state(), g.agents()["tl_cnt"]
    g.close()
    assert (cnt == np.array([c["want"]] * n + [0])).all(), cnt[:2]
    for k in ("obs_blue", "obs_red"):
        assert (out[k].view(np.int32) == r[k].astype(np.float32).view(np.int32)).all(), k
    assert all(np.abs(out[k] - r[k]).max() <= D.REW_TOL for k in ("rew_blue", "rew_red"))
    ost = o.env_state()
    assert (es["rng"] == ost["tape_pos"]).all() and (es["err"] == ost["err"]).all() and ost["err"] == 0


# --- the size limit ----------------------------------------------------------
LIMIT = [  # (nb, nr, G, loads)
    (16, 16, 100, False), (16, 16, 200, False), (16, 10, 100, False), (10, 16, 200, False),
    (16, 9, 100, True), (9, 16, 200, True), (15, 15, 200, True), (16, 1, 200, True), (1, 16, 100, True),
]


@pytest.mark.parametrize("nb,nr,G,loads", LIMIT)
def test_size_limit(nb, nr, G, loads):
    """include/lnw.h: lnw_load_terrain refuses a fleet whose step layout needs
    more LDS than a CU has, a side of 16 ships against 10 or more, with
    LNW_EUNSUPPORTED and its message, and the handle still closes; every other
    size up to 16 a side loads (15v15, 16v9)."""
    from lnw import _abi
    from lnw.config import Scenario
    L = _abi.load()
    grid = np.ascontiguousarray(_grid(G), np.uint8)
    p = Scenario(landing_ops=False).params()
    h = C.c_void_p()
    _abi.check(L.lnw_create(C.byref(p), 40, nb, nr, 0, 0, C.byref(h)))
    rc = L.lnw_load_terrain(h, grid.ctypes.data_as(C.c_void_p), G)
    msg = L.lnw_last_error().decode()
    assert L.lnw_destroy(h) == 0
    if loads:
        assert rc == 0, msg
    else:
        assert rc == -5 and "agent count needs more LDS than a CU has" in msg, (rc, msg)
