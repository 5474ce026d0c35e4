"""Which step kernel a launch takes and the envs per workgroup chosen for it
(csrc/lnw_host.inc: plan_step, choose_epw), one case per row of DESIGN.md's
"Kernel variants" selection table: one step each, asserting lnw_step_kernel and,
where epw is left automatic, the epw in force. The expected values are those of
the launch code before the plan existed (the same file passes against that
library through LNW_LIB), so they pin the selection, the kept oddities included:
a 4v4 fleet counts as a two-wave shape for epw (16 at 64 envs) whatever kernel
it is then launched on, unless LNW_FORCE_GENERIC or the reference's LOS work
(los_mode 2) takes it off the team kernels; other shapes go down to 1."""
import numpy as np
import pytest
import torch

import _device as D
from _spawns import grid as _grid

pytestmark = pytest.mark.gpu

S4, L4 = ["small"] * 4, ["large"] * 4

# name: blue, red, knobs (environment), contact, los_mode, E, forced epw (None: automatic) -> kernel, automatic epw
CASES = {
    "4v4_units": (S4, L4, (), False, 0, 256, 64, "UNITS", None),
    "4v4_no_units": (S4, L4, ("LNW_NO_UNITS",), False, 0, 256, 64, "TEAM", None),
    "4v4_small_batch": (S4, L4, (), False, 0, 64, None, "TEAM", 16),
    "4v4_contact": (S4, L4, (), True, 0, 64, None, "TEAM_CONTACT", 16),
    "2v2": (S4[:2], L4[:2], (), False, 0, 64, None, "TEAM", 16),
    "3v3_contact": (S4[:3], L4[:3], (), True, 0, 64, None, "TEAM_CONTACT", 16),
    "5v3_group": (["small"] * 5, L4[:3], (), False, 0, 64, None, "GROUP", 1),
    "5v3_no_group": (["small"] * 5, L4[:3], ("LNW_NO_GROUP",), False, 0, 64, None, "GENERIC", 1),
    "4v4_force_generic": (S4, L4, ("LNW_FORCE_GENERIC",), False, 0, 64, None, "GENERIC", 1),
    "4v4_force_group": (S4, L4, ("LNW_FORCE_GROUP",), False, 0, 64, None, "GROUP", 16),
    "4v4_medium": (["medium"] * 4, L4, (), False, 0, 64, None, "GROUP", 16),
    "4v4_reflos": (S4, L4, (), False, 2, 64, None, "REFLOS", 1),
}


def _positions(grid, nb, nr):
    water = lambda x0, x1, y0, y1: [(x, y) for x in range(x0, x1) for y in range(y0, y1) if grid[x, y] <= 74]
    wb, wr = water(30, 45, 40, 60), water(50, 65, 45, 65)
    return [wb[7 * i] for i in range(nb)] + [wr[7 * i] for i in range(nr)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_plan(name, monkeypatch):
    from lnw.config import Scenario
    blue, red, knobs, contact, los_mode, E, epw, kernel, auto_epw = CASES[name]
    grid = _grid(100)
    g = D.make_game(monkeypatch, E, blue, red, Scenario(landing_ops=False, los_mode=los_mode), grid, 3,
                    env=dict.fromkeys(knobs, "1"), epw=epw, contact=contact)  # (knobs: read once, by lnw_create)
    g.reset(positions=_positions(grid, len(blue), len(red)))
    act = torch.from_numpy(np.random.default_rng(1).random((E, len(blue) + len(red), 4), dtype=np.float32)).cuda()
    g.step(act)
    torch.cuda.synchronize()
    print(name, "kernel", g.step_kernel(), "epw", g.epw)
    assert g.step_kernel() == D.kernel_code(kernel)
    if epw is None:
        assert g.epw == auto_epw
    assert int((g.env_state()["err"] != 0).sum()) == 0
    g.close()
