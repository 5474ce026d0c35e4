"""The action rows of tests/_move_rows.py have power (CPU only).

tests/test_gpu_move_interleave.py compares phase M's float32 path with the
oracle on these rows; that says something only if the rows reach every way out
of the common path, inside single waves, and if the moves they ask for matter.
Shown here with a numpy restatement of move_cell_f32_fast's conditions
(_move_rows.fast_verdict: rows within a small margin of the band's edge are
left out of every count) for the presence of each class, and with the oracle
alone for the consequences.
"""
import numpy as np
import pytest

import _move_rows as M

TEAMS = sorted(M.TEAMS)


def _verdicts(sim):
    """Per (step, env, agent): fast_verdict on the cell the ship stands on
    before the step, its target cell, finiteness and whether it is alive."""
    speed = np.array([M.SPEED[t] for t in sim["types"]])
    pb = sim["pos_before"]
    v, cell, finite = M.fast_verdict(pb[..., 0], pb[..., 1], speed, sim["acts"][..., 2], sim["acts"][..., 3])
    return v, cell, finite, sim["alive_before"]


@pytest.mark.parametrize("team", TEAMS)
def test_every_class_is_present(team):
    sim = M.simulate(team)
    v, cell, finite, alive = _verdicts(sim)
    cls = sim["cls"]
    n = {c: int(((cls == i) & alive).sum()) for i, c in enumerate(M.CLASSES)}
    assert min(n.values()) >= 500, n
    ci = M.CLASSES.index
    # plain rows take the polynomials, all but a handful
    plain = (cls == ci("plain")) & alive
    assert (v[plain] == 1).mean() > 0.999
    # ties, turns past 1e5 degrees, |dist| > 4 and non-finite rows never do
    for c in ("tie", "quarter_tie", "far_deg", "nonfinite"):
        m = (cls == ci(c)) & alive
        assert (v[m] == -1).all(), c
    m = (cls == ci("far_dist")) & alive
    assert (v[m] == -1).all()
    # wide rows: in range, many turns: certified, with both signs of k and of dist
    m = (cls == ci("wide")) & alive
    assert (v[m] == 1).mean() > 0.99
    assert (sim["acts"][..., 2][m] < -1).sum() > 100 and (sim["acts"][..., 3][m] < 0).sum() > 100
    # non-finite rows: NaN, +inf and -inf, in a2 and in a3
    m = (cls == ci("nonfinite")) & alive
    for col in (2, 3):
        x = sim["acts"][..., col][m]
        assert np.isnan(x).sum() > 50 and (x == np.inf).sum() > 50 and (x == -np.inf).sum() > 50
    assert (~finite[m]).sum() > 300  # (inf * 0-ish rows aside, they do not round)
    # sunk ships hold rows of every class too
    sunk = ~alive
    assert sunk.sum() > 200 and len(np.unique(cls[sunk])) == len(M.CLASSES)
    # targets: off the grid, on land, in the table's window and beyond it (the A* pass)
    g = M.grid()
    live_t = alive & finite
    x, y = cell[..., 0], cell[..., 1]
    ingrid = live_t & (x >= 0) & (x < 100) & (y >= 0) & (y < 100)
    assert (live_t & ~ingrid).sum() > 300
    land = np.zeros_like(ingrid)
    land[ingrid] = g[x[ingrid], y[ingrid]] > 74
    assert land.sum() > 100
    water = ingrid & ~land
    d = np.abs(cell - sim["pos_before"]).max(-1)
    assert (water & (d <= 4)).sum() > 10000 and (water & (d > 4)).sum() > 300
    if team == "3v3_ls":  # the landing ship: the other dist scale, its own ties
        ls = np.array(sim["types"]) == M._oracle.T_LS
        assert ((cls == ci("tie")) & alive)[..., ls].sum() > 100
        assert (v[..., ls][alive[..., ls]] == 1).sum() > 1000


@pytest.mark.parametrize("team,E,epw", [("4v4", 512, 64), ("4v4", 256, 64), ("4v4", 149, 64), ("4v4", 149, 32),
                                        ("4v4", 149, 16), ("3v3_ls", 149, 64)])
def test_waves_are_mixed(team, E, epw):
    """Inside the 64-lane passes of the launch form (pass p, lane l of a
    workgroup is pair 64 p + l; its two waves take contiguous halves of the
    passes): passes in which one to three lanes fall back, passes in which
    none does, passes in which many do, and lanes whose passes in one wave go
    different ways."""
    sim = M.simulate(team)
    v, _, _, alive = _verdicts(sim)
    A = sim["A"]
    slow = ((v == -1) & alive)[:, :E]
    fast = ((v == 1) & alive)[:, :E]
    few = mixed_lane = none = many = 0
    for e0 in range(0, E, epw):
        nenv = min(epw, E - e0)
        npair = nenv * A
        npass = (npair + 63) // 64
        share = (npass + 1) // 2
        s = np.zeros((M.STEPS, npass * 64), bool)
        f = np.zeros((M.STEPS, npass * 64), bool)
        s[:, :npair] = slow[:, e0:e0 + nenv].reshape(M.STEPS, npair)
        f[:, :npair] = fast[:, e0:e0 + nenv].reshape(M.STEPS, npair)
        s, f = s.reshape(M.STEPS, npass, 64), f.reshape(M.STEPS, npass, 64)
        few += int(((s.sum(-1) >= 1) & (s.sum(-1) <= 3) & (f.sum(-1) >= 8)).sum())
        none += int(((s.sum(-1) == 0) & (f.sum(-1) >= 8)).sum())
        many += int((s.sum(-1) >= 8).sum())  # an eighth of the wave (3v3: a pass spans 10.7 envs, the rates blur)
        for w in range(2):
            ps = slice(w * share, min((w + 1) * share, npass))
            if ps.stop - ps.start >= 2:
                mixed_lane += int((s[:, ps].any(1) & f[:, ps].any(1)).sum())
    assert few >= 20 and none >= 20 and many >= 20, (few, none, many)
    if epw * A >= 256:  # two passes or more per wave
        assert mixed_lane >= 200, mixed_lane
    if E == 149:
        assert E % epw  # the one-unit forms end in a partial workgroup


@pytest.mark.parametrize("team", TEAMS)
def test_rows_have_consequences(team):
    """By the oracle alone: ships move (into the table's window and, through
    the A* pass, not beyond it), moves are refused, non-finite rows of live
    ships raise the error flag and nothing else does."""
    sim = M.simulate(team)
    v, cell, finite, alive = _verdicts(sim)
    moved = (sim["pos_after"] != sim["pos_before"]).any(-1)
    assert (moved & alive).sum() > 10000
    assert not (moved & ~alive).any()
    # a moved ship stands on the cell the restatement gives (where it is sure of it)
    ok = moved & alive & (v == 1)
    assert (sim["pos_after"][ok] == cell[ok]).all()
    # the slow rows move ships too: ties and far turns end on a neighbouring cell
    assert (moved & alive & (v == -1)).sum() > 300
    # refusals: a live ship, a finite target, no move
    assert (~moved & alive & finite & (np.abs(cell - sim["pos_before"]).max(-1) > 0)).sum() > 1000
    # error flags: exactly the envs that have held a live ship's non-finite move row so far
    # (columns 0 and 1 are finite everywhere)
    bad = np.logical_or.accumulate((alive & ~finite).any(-1), axis=0)
    assert bad.sum() > 500 and (~bad).sum() > 500
    assert ((sim["err"] != 0) == bad).all()
    # the fleets in reach fought: ships sank during the run, in melee blocks only
    sunk_end = ~sim["alive_before"][-1]
    for b, kind in enumerate(M.BLOCKS):
        blk = sunk_end[64 * b:64 * b + 64]
        if kind == "ref":
            assert not blk.any(), b
        elif kind == "melee":
            assert blk.sum() >= 10, b
