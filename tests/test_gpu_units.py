"""The headline units kernel (step_kernel<4, 4, false, false, 4>: four 64-env
units per 512-thread workgroup, DESIGN.md "Units kernel") checked directly
against the CPU oracle, with quiet and loud units mixed inside every workgroup.

The units kernel runs only for 4v4, 64 envs per workgroup, the default variant
and E a multiple of 256 (lnw_kernels.hip lnw_step). Here E = 512 is two
workgroups; each holds units at the reference spawns (quiet: phase Q and the
shared observation-pass queue), units at melee spawns (loud: phase S inside the
same workgroup) and a unit with both kinds of env (loud as a whole). 45 Philox
steps cross the 40-step horizon's in-kernel auto-reset, and melee episodes end
in victories (done == 0) and respawn on their own cells. Every env is compared
with orc_fullsize_range (oracle/lnw_oracle.c) bit for bit: observation hashes,
done, the action rows as the step left them (an untrained red's salvo
write-back, game.py:375-379); rewards and cog within 1e-5. Needs an MI355X.
"""
import numpy as np
import pytest
import torch

import _oracle
from _fullsize_util import _compare, _gpu_run
from _spawns import REF_SPAWNS, grid as _grid, hash_mult, melee_block

pytestmark = pytest.mark.gpu

# unit kinds per workgroup (E = 512: two workgroups of four 64-env units)
LAYOUT = [["ref", "melee", "ref", "mixed"], ["melee", "ref", "mixed", "ref"]]


def _positions(grid):
    pos = np.array([REF_SPAWNS] * 512, np.int32)
    for w, kinds in enumerate(LAYOUT):
        for u, kind in enumerate(kinds):
            e0 = 256 * w + 64 * u
            if kind == "melee":
                pos[e0:e0 + 64] = melee_block(grid, 64, seed=e0)
            elif kind == "mixed":
                pos[e0 + 32:e0 + 64] = melee_block(grid, 32, seed=e0)
    return pos


@pytest.mark.parametrize("trained_red", [True, False])
def test_units_kernel_vs_oracle(trained_red):
    from lnw import _abi
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    grid = _grid(100)
    E, S, seed = 512, 45, 4242
    pos = _positions(grid)
    sc = Scenario(landing_ops=False, auto_reset=True, episode_steps=40, trained_red=trained_red)
    g = BatchedGame(E, ["small"] * 4, ["large"] * 4, scenario=sc, grid=grid, seed=seed)
    assert g.set_epw(64) == 64
    g.reset(positions=REF_SPAWNS, pos_per_env=torch.from_numpy(pos))
    acts = np.random.default_rng(12 + trained_red).random((S, E, 8, 4), dtype=np.float32)
    mult = hash_mult(2 * 4 * 68, seed=5)
    gpu = _gpu_run(g, acts, mult, after=True, kernel=_abi.KERNEL_UNITS)
    assert int((g.env_state()["err"] != 0).sum()) == 0
    g.close()
    oh, orw, od, oc, oa = _oracle.fullsize(grid, 4, 4, [0] * 4 + [1] * 4, pos, acts, mult, seed, 40,
                                           pos_per_env=True, trained_red=trained_red,
                                           acts_after=True)
    gd, ga = gpu[2], gpu[4]
    _compare(gpu[:4], (oh, orw, od, oc), "units")
    assert np.array_equal(ga, oa), np.argwhere((ga != oa).any(-1))[:6].tolist()
    # what the layout is for: loud units fought (victories) and quiet ones ran
    # to the horizon, in both workgroups
    for w in range(2):
        for u, kind in enumerate(LAYOUT[w]):
            blk = gd[:, 256 * w + 64 * u:256 * w + 64 * (u + 1)]
            if kind == "ref":
                assert (blk == 1).all(), (w, u)
            elif kind == "melee":
                assert (blk == 0).any(), (w, u)
    if not trained_red:  # the scripted salvos were written back in both kinds of unit
        assert not np.array_equal(ga[:, :, 4:], acts[:, :, 4:])
