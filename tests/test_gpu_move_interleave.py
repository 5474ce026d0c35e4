"""Phase M's float32 path against the CPU oracle, in every launch form, on rows
that leave its common path in every way (tests/_move_rows.py;
tests/test_move_rows_cpu.py shows on the CPU what those rows hold).

The units kernel takes a wave's four pair passes interleaved, with the rows the
float polynomials cannot certify in one loop after them (move_stages_f32,
csrc/lnw_kernels.hip); the one-unit kernels take them pass after pass
(move_batch_t). Both must leave every row's move, refusal and error flag as the
reference has it. Over 12 steps, every env and step: observation rows, rewards
(float32 of the oracle's sums), done, cog and the action rows after the step
bit for bit, the ships' cells and the error flags. Needs an MI355X.
"""
import numpy as np
import pytest
import torch

import _move_rows as M

pytestmark = pytest.mark.gpu


def _form(team, E, epw, kernel, **kw):
    return dict(team=team, E=E, epw=epw, kernel=kernel, env=kw.pop("env", None), contact=kw.pop("contact", False),
                move_mode=kw.pop("move_mode", 0), **kw)


# E = 149: two workgroups and a partial one at epw 64, partial last workgroups at 32 and 16
FORMS = {
    "units_256": _form("4v4", 256, 64, "units"),
    "units_512": _form("4v4", 512, 64, "units"),
    "units_256_astar": _form("4v4", 256, 64, "units", move_mode=1),  # every target goes to the A* pass
    "4v4_epw64_no_units": _form("4v4", 256, 64, "team", env="LNW_NO_UNITS"),
    "4v4_epw64_ragged": _form("4v4", 149, 64, "team", env="LNW_NO_UNITS"),
    "4v4_epw32": _form("4v4", 149, 32, "team"),
    "4v4_epw16": _form("4v4", 149, 16, "team"),
    "4v4_contact": _form("4v4", 149, 64, "team_contact", contact=True),
    "3v3_ls": _form("3v3_ls", 149, 64, "team"),
}


def _first(bad):
    return np.argwhere(bad)[:4].tolist()


@pytest.mark.parametrize("name", sorted(FORMS))
def test_rows_vs_oracle(name, monkeypatch):
    from lnw import _abi
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    f = FORMS[name]
    sim = M.simulate(f["team"])
    E, nb = f["E"], sim["nb"]
    blue, red, landing = M.TEAMS[f["team"]]
    if f["env"]:
        monkeypatch.setenv(f["env"], "1")  # (read by lnw_create)
    sc = Scenario(landing_ops=landing, move_mode=f["move_mode"])
    g = BatchedGame(E, list(blue), list(red), scenario=sc, grid=M.grid(), seed=M.SEED)
    if f["env"]:
        monkeypatch.delenv(f["env"])
    if f["contact"]:
        g.set_variant(True)
    assert g.set_epw(f["epw"]) == f["epw"]
    g.reset(positions=M.REF_SPAWNS[:nb] + M.REF_SPAWNS[4:4 + nb], pos_per_env=torch.from_numpy(sim["pos"][:E].copy()))
    kernel = {"team": _abi.KERNEL_TEAM, "team_contact": _abi.KERNEL_TEAM_CONTACT, "units": _abi.KERNEL_UNITS}
    for s in range(M.STEPS):
        act = torch.from_numpy(sim["acts"][s, :E].copy()).cuda()
        out = {k: v.cpu().numpy() for k, v in g.step(act).items()}
        assert g.step_kernel() == kernel[f["kernel"]], "the plan chose another kernel than the one under test"
        after = act.cpu().numpy()
        for k in ("obs_blue", "obs_red"):
            bad = (out[k].view(np.int32) != sim[k][s, :E].view(np.int32)).any(axis=(1, 2))
            assert not bad.any(), (name, s, k, "envs", _first(bad))
        for k in ("rew_blue", "rew_red"):
            ref = sim[k][s, :E].astype(np.float32)
            diff = np.abs(out[k].astype(np.float64) - ref)
            print(name, s, k, "max |diff| vs float32(oracle)", diff.max())
            bad = (out[k].view(np.int32) != ref.view(np.int32)).any(axis=1)
            assert not bad.any(), (name, s, k, "envs", _first(bad), float(diff.max()))
        assert np.array_equal(out["done"], sim["done"][s, :E]), (name, s, "done")
        cg, oc = out["cog"], sim["cog"][s, :E].astype(np.float32)
        bad = ~((cg == oc) | (np.isnan(cg) & np.isnan(oc)))
        assert not bad.any(), (name, s, "cog", _first(bad))
        bad = (after.view(np.int32) != sim["acts_after"][s, :E].view(np.int32)).any(axis=(1, 2))
        assert not bad.any(), (name, s, "action rows after the step", _first(bad))
        ag = g.agents()
        pos = np.stack([ag["x"], ag["y"]], -1)
        bad = (pos != sim["pos_after"][s, :E]).any(axis=(1, 2))
        assert not bad.any(), (name, s, "cells", _first(bad))
        err = g.get(_abi.F_ERR).cpu().numpy()
        bad = err.astype(np.uint32) != sim["err"][s, :E]
        assert not bad.any(), (name, s, "error flags", _first(bad))
    g.close()
