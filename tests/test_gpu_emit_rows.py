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
import torch

import _oracle
from _oracle import load_fixture
from test_gpu_parity import REW_TOL, _melee_positions

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
    grid = load_fixture("grids.npz")["grid100"]
    pos = _melee_positions(grid, E, nb, nr, seed=nb)
    rng = np.random.default_rng(100 + nb)
    acts = [rng.random((E, nb + nr, 4)).astype(np.float32) for _ in range(S)]
    return grid, pos, acts


def _oracle_run(name, grid, pos, acts):
    """[S][E] step results of the oracle stepping the same envs."""
    blue, red = CASES[name]
    A = len(blue) + len(red)
    oracles = []
    for e in range(E):
        o = _oracle.OracleEnv(grid, len(blue), len(red))
        o.set_philox(SEED, e)
        o.reset([CODES[t] for t in blue + red], pos[e])
        oracles.append(o)
    kinds = np.full(A, _oracle.K_F32, np.int32)
    return [[o.step(act[e], kinds) for e, o in enumerate(oracles)] for act in acts]


def _zero_rows(want, side):
    return sum(int((~r[side].any(axis=1)).sum()) for step in want for r in step)


@pytest.mark.parametrize("name", sorted(CASES))
def test_philox_emission_vs_oracle(name):
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    blue, red = CASES[name]
    grid, pos, acts = _inputs(name)
    want = _oracle_run(name, grid, pos, acts)
    # a sunk ship's row is all zeros: each side must show some, or a kernel that
    # never zeroes a dead row would pass
    for side in ("obs_blue", "obs_red"):
        assert _zero_rows(want, side) > 0, (name, side)
    g = BatchedGame(E, blue, red, scenario=Scenario(landing_ops=False), grid=grid, seed=SEED)
    assert g.set_epw(64) == 64  # one full wave of envs per workgroup: rows leave during phase S
    g.reset(positions=pos[0], pos_per_env=torch.from_numpy(pos))
    for s, act in enumerate(acts):
        out = g.step(torch.from_numpy(act).cuda())
        ob, orr = out["obs_blue"].cpu().numpy(), out["obs_red"].cpu().numpy()
        rb, rr = out["rew_blue"].cpu().numpy(), out["rew_red"].cpu().numpy()
        dn = out["done"].cpu().numpy()
        for e in range(E):
            r = want[s][e]
            assert np.array_equal(ob[e], r["obs_blue"].astype(np.float32)), (s, e, "obs_blue")
            assert np.array_equal(orr[e], r["obs_red"].astype(np.float32)), (s, e, "obs_red")
            assert np.allclose(rb[e], r["rew_blue"], rtol=0, atol=REW_TOL), (s, e, "rew_blue")
            assert np.allclose(rr[e], r["rew_red"], rtol=0, atol=REW_TOL), (s, e, "rew_red")
            assert dn[e] == r["done"], (s, e, "done")
    g.close()
