"""Parity at BASELINE.json's full sizes (configs 2, 3 per GPU and 4): every env
of the batch checked against the CPU oracle, in production (Philox) mode, over
45 steps so the 40-step horizon's in-kernel auto-reset is crossed.

Holding 65 536 envs' observations for every step on the host is not needed:
per (step, env) both sides reduce the float32 observations to a 64-bit hash,
sum_k bits(obs[k]) * mult[k] mod 2^64 (mult: random odd 31-bit constants), the
device with torch int64 arithmetic (wrapping), the oracle in C
(oracle/lnw_oracle.c orc_fullsize_range). A single flipped bit anywhere in an
env's rows changes its hash. Rewards (float32, tolerance 1e-5), done and cog are
compared in full. Needs an MI355X.
"""
import numpy as np
import pytest
import torch

import _oracle
from _fullsize_util import _compare, _gpu_run
from _spawns import REF_SPAWNS, grid as _grid, hash_mult, water_positions

pytestmark = pytest.mark.gpu



def test_fullsize_config3_reference_spawns():
    """Config 3 per GPU: 65 536 4v4 envs at the reference spawns (the bench
    workload: quiet workgroups throughout), 45 steps, every env vs the oracle."""
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    grid = _grid(100)
    E, S, seed = 65536, 45, 1234
    sc = Scenario(landing_ops=False, auto_reset=True, episode_steps=40)
    g = BatchedGame(E, ["small"] * 4, ["large"] * 4, scenario=sc, grid=grid, seed=seed)
    g.reset(positions=REF_SPAWNS)
    acts = np.random.default_rng(5).random((S, E, 8, 4), dtype=np.float32)
    mult = hash_mult(4 * 68 + 4 * 68)
    gpu = _gpu_run(g, acts, mult)
    assert int((g.env_state()["err"] != 0).sum()) == 0
    g.close()
    orc = _oracle.fullsize(grid, 4, 4, [0] * 4 + [1] * 4, np.array(REF_SPAWNS), acts, mult, seed, 40)
    _compare(gpu, orc, "config3")
    assert (gpu[2][39] == 1).all()  # horizon reached, envs reset in-kernel after step 40


@pytest.mark.parametrize("contact", [False, True])
def test_fullsize_config2_contact_spawns(contact):
    """Config 2 size (4 096 4v4 envs) with the sides 10-40 cells apart, so
    firing, hits, EW bearings and fixes happen every step (phase S workgroups),
    45 steps, every env vs the oracle."""
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    grid = _grid(100)
    E, S, seed = 4096, 45, 77
    pos = water_positions(grid, E, [(30, 45, 40, 60)] * 4 + [(55, 70, 45, 65)] * 4, seed=3)
    sc = Scenario(landing_ops=False, auto_reset=True, episode_steps=40)
    g = BatchedGame(E, ["small"] * 4, ["large"] * 4, scenario=sc, grid=grid, seed=seed)
    g.set_variant(contact)  # both step-kernel variants (lnw_set_variant)
    g.reset(positions=pos[0], pos_per_env=torch.from_numpy(pos))
    acts = np.random.default_rng(6).random((S, E, 8, 4), dtype=np.float32)
    mult = hash_mult(4 * 68 + 4 * 68, seed=7)
    gpu = _gpu_run(g, acts, mult)
    assert int((g.env_state()["err"] != 0).sum()) == 0
    g.close()
    orc = _oracle.fullsize(grid, 4, 4, [0] * 4 + [1] * 4, pos, acts, mult, seed, 40,
                           pos_per_env=True)
    _compare(gpu, orc, "config2-contact")
    assert (gpu[2] == 0).any()  # some episodes end in a victory (done == 0) and reset


def test_fullsize_config4():
    """Config 4: 8 192 envs, 8 small blue vs 8 large + 2 LandingShip red
    (landing ops, LandingShip spawns drawn by randint as game.py:587-591) on the
    200x200 grid, per-env water spawns in x in [20, 60), y in [80, 140), 42 steps,
    every env vs the oracle."""
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    grid = _grid(200)
    E, S, seed = 8192, 42, 21
    A = 18
    pos = water_positions(grid, E, [(20, 60, 80, 140)] * A, seed=4)
    rand_ls = [0] * 16 + [1, 1]
    sc = Scenario(landing_ops=True, auto_reset=True, episode_steps=40)
    g = BatchedGame(E, ["small"] * 8, ["large"] * 8 + ["ls"] * 2, scenario=sc, grid=grid, seed=seed)
    g.reset(positions=pos[0], rand_ls=rand_ls, pos_per_env=torch.from_numpy(pos))
    acts = np.random.default_rng(8).random((S, E, A, 4), dtype=np.float32)
    mult = hash_mult(8 * 84 + 10 * 92, seed=9)
    gpu = _gpu_run(g, acts, mult)
    assert int((g.env_state()["err"] != 0).sum()) == 0
    g.close()
    orc = _oracle.fullsize(grid, 8, 10, [0] * 8 + [1] * 8 + [2] * 2, pos, acts, mult, seed, 40,
                           pos_per_env=True, rand_ls=rand_ls, landing_ops=True)
    _compare(gpu, orc, "config4")
