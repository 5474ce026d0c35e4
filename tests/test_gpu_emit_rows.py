"""Wave 1's row-piece emission for 2- and 3-ship sides (emit_rows_t<2>, <3>)
against the CPU oracle. Needs an MI355X.

The step kernel emits ship a's observation rows during phase S only when a
workgroup holds a full wave of 64 envs; the golden-episode replays run fewer
envs per scenario, and the 4-ship launch-shape test takes the line-aligned
form, so nothing else reaches these two instantiations. The 3v3 case has a
landing ship on red, which puts the landing-ship row layout through the
compile-time row select."""
import numpy as np
import pytest

import _device as D
import _oracle
from _spawns import box_positions, grid as _grid

pytestmark = pytest.mark.gpu

E, S, SEED = 64, 12, 11
CODES = {"small": _oracle.T_SMALL, "large": _oracle.T_LARGE, "ls": _oracle.T_LS}
CASES = {
    "2v2": (["small"] * 2, ["large"] * 2),
    "3v3ls": (["small"] * 3, ["large", "large", "ls"]),
}


def _inputs(name):
    blue, red = CASES[name]
    nb, nr = len(blue), len(red)
    grid = _grid(100)
    pos = box_positions(grid, E, nb, nr, seed=nb)
    rng = np.random.default_rng(100 + nb)
    acts = [rng.random((E, nb + nr, 4)).astype(np.float32) for _ in range(S)]
    return grid, pos, acts


def _oracle_run(name, grid, pos, acts):
    """The oracle's record [S, E] of stepping the same envs."""
    blue, red = CASES[name]
    nb, nr = len(blue), len(red)
    rec = _oracle.new_record(S, E, nb, nr)
    kinds = np.full(nb + nr, _oracle.K_F32, np.int32)
    for e in range(E):
        o = _oracle.OracleEnv(grid, nb, nr)
        o.set_philox(SEED, e)
        o.reset([CODES[t] for t in blue + red], pos[e])
        for s, act in enumerate(acts):
            _oracle.record_step(rec, s, e, o.step(act[e], kinds))
    return rec


@pytest.mark.parametrize("name", sorted(CASES))
def test_philox_emission_vs_oracle(name, monkeypatch):
    from lnw.config import Scenario
    blue, red = CASES[name]
    grid, pos, acts = _inputs(name)
    want = _oracle_run(name, grid, pos, acts)
    # a sunk ship's row is all zeros: each side must show some, or a kernel that
    # never zeroes a dead row would pass
    for side in ("obs_blue", "obs_red"):
        assert (~want[side].any(axis=-1)).sum() > 0, (name, side)
    # one full wave of envs per workgroup: rows leave during phase S
    g = D.make_game(monkeypatch, E, blue, red, Scenario(landing_ops=False), grid, SEED, epw=64)
    D.start(g, pos)
    for s, act in enumerate(acts):
        D.assert_step(D.step(g, act), want, s, name, rew="tol", cog="tol")
    g.close()
