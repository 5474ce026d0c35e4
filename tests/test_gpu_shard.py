"""The metric's real per-GPU path at N = 8 and config 2: 8 192 and 4 096 4v4 envs
on one GPU take the small-workgroup quiet direct mode (16 envs per workgroup,
quiet_step_t in csrc/lnw_quiet.inc, DESIGN.md "Direct mode for small
workgroups"); 16 384 envs (config 3's shard at N = 4) take it with 32 envs per
workgroup, the rows written in two slabs of 16 envs. Checked directly against the CPU oracle (orc_fullsize_range,
oracle/lnw_oracle.c) with the default envs-per-workgroup choice:

* "reference": every env at the reference spawns (game.py:560-585), the
  bench's workload: every workgroup quiet every step;
* "mixed": a melee block (sides 10-40 cells apart: fire, hits, EW fixes,
  victories) in every other 16-env workgroup, so quiet direct-mode workgroups
  and phase-S workgroups run side by side in one launch.

45 Philox steps cross the 40-step horizon's in-kernel auto-reset (and, in the
melee blocks, victory resets on the per-env cells), with a trained and an
untrained (scripted-salvo) red. Every env is compared bit for bit:
observation hashes, done and the action rows as the step left them (the
untrained red's salvo write-back, game.py:375-379); rewards and cog within
1e-5. Needs an MI355X."""
import numpy as np
import pytest
import torch

import _oracle
from _fullsize_util import _compare, _gpu_run
from _spawns import REF_SPAWNS, grid as _grid, hash_mult, melee_block

pytestmark = pytest.mark.gpu



@pytest.mark.parametrize("trained_red", [True, False])
@pytest.mark.parametrize("layout", ["reference", "mixed"])
@pytest.mark.parametrize("E", [8192, 4096, 16384])
def test_shard_quiet_direct_vs_oracle(E, layout, trained_red):
    from lnw import _abi
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    grid = _grid(100)
    S, seed = 45, 900 + E // 1024 + 2 * trained_red
    pos = np.array([REF_SPAWNS] * E, np.int32)
    if layout == "mixed":
        blocks = np.arange(E).reshape(-1, 32)[:, 16:].reshape(-1)   # every other 16-env workgroup
        pos[blocks] = melee_block(grid, len(blocks), seed=E)
    sc = Scenario(landing_ops=False, auto_reset=True, episode_steps=40, trained_red=trained_red)
    g = BatchedGame(E, ["small"] * 4, ["large"] * 4, scenario=sc, grid=grid, seed=seed)
    # the default choice: 16 envs per workgroup at 8 192 / 4 096 (one slab), 32 at
    # 16 384 (config 3 at N = 4: wave 1 writes the rows in two slabs of 16 envs)
    assert g.epw == (32 if E == 16384 else 16)
    g.reset(positions=REF_SPAWNS, pos_per_env=torch.from_numpy(pos))
    acts = np.random.default_rng(31 + trained_red).random((S, E, 8, 4), dtype=np.float32)
    mult = hash_mult(2 * 4 * 68, seed=13)
    gpu = _gpu_run(g, acts, mult, after=True, kernel=_abi.KERNEL_TEAM)
    assert int((g.env_state()["err"] != 0).sum()) == 0
    g.close()
    oh, orw, od, oc, oa = _oracle.fullsize(grid, 4, 4, [0] * 4 + [1] * 4, pos, acts, mult, seed, 40,
                                           pos_per_env=True, trained_red=trained_red, acts_after=True)
    gd, ga = gpu[2], gpu[4]
    _compare(gpu[:4], (oh, orw, od, oc), (E, layout))
    assert np.array_equal(ga, oa), np.argwhere((ga != oa).any(-1))[:6].tolist()
    assert (gd[39] == 1).all() if layout == "reference" else (gd == 0).any()
    if not trained_red:  # the scripted salvos were written back
        assert not np.array_equal(ga[:, :, 4:], acts[:, :, 4:])
