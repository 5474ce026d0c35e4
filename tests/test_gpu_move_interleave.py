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

import _device as D
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


@pytest.mark.parametrize("name", sorted(FORMS))
def test_rows_vs_oracle(name, monkeypatch):
    from lnw.config import Scenario
    f = FORMS[name]
    sim = M.simulate(f["team"])
    blue, red, landing = M.TEAMS[f["team"]]
    sc = Scenario(landing_ops=landing, move_mode=f["move_mode"])
    g = D.make_game(monkeypatch, f["E"], blue, red, sc, M.grid(), M.SEED, env={f["env"]: "1"} if f["env"] else None,
                    epw=f["epw"], contact=f["contact"])  # (the knob is read by lnw_create)
    D.start(g, sim["pos"], positions=M.ref_spawns(sim["nb"]))
    for s in range(M.STEPS):
        out = D.step(g, sim["acts"][s, :f["E"]], extra=("pos_after", "err"))
        assert g.step_kernel() == D.kernel_code(f["kernel"]), "the plan chose another kernel than the one under test"
        for k in ("rew_blue", "rew_red"):
            diff = np.abs(out[k].astype(np.float64) - sim[k][s, :f["E"]].astype(np.float32))
            print(name, s, k, "max |diff| vs float32(oracle)", diff.max())
        D.assert_step(out, sim, s, name, rew="bits", cog="exact")
    g.close()
