"""The quiet-workgroup path (csrc/lnw_quiet.inc) at sensor reach, in every
launch form plan_step / step_qdirect (csrc/lnw_host.inc) can give it.

Inputs: tests/_quiet_cases.py. Each workgroup holds one probe env whose fleets
of large ships stand at the widest sensor reach (EW between two 30 m masts)
give or take a few cells, so that env alone decides whether its workgroup
skips phase S; tests/test_quiet_reach_cpu.py shows on the CPU oracle that a
predicate that ignored a position combination or stopped a cell short would
fail here. Every env and step is compared with the oracle: observations bit
for bit, rewards within REW_TOL, done, cog, the action rows after the step
and the env's Philox draw counter. Needs an MI355X."""
import re

import numpy as np
import pytest
import torch

import _device as D
import _quiet_cases as Q
from _spawns import grid, ref_spawns

pytestmark = pytest.mark.gpu

FORMS = sorted(Q.FORMS)


def _make(name, monkeypatch, E, *, auto_reset=False, trained_red=True, prof=False, seed=0):
    """A handle in the row's form. The knobs are read by lnw_create and
    LNW_EPW_RT by the constructor's automatic epw choice."""
    from lnw.config import Scenario
    f = Q.FORMS[name]
    nb = f["nb"]
    env = {f["env"]: "1"} if f["env"] else {}
    if prof:
        env["LNW_PROF"] = "1"
    if f.get("epw_rt"):
        env["LNW_EPW_RT"] = str(f["epw"])
    sc = Scenario(landing_ops=f["red"] is not None, auto_reset=auto_reset, episode_steps=40,
                  trained_red=trained_red)
    g = D.make_game(monkeypatch, E, ["large"] * nb, f["red"] or ["large"] * nb, sc, grid(f["G"]), seed, env=env,
                    contact=f["contact"])
    if f.get("epw_rt"):
        assert g.epw == f["epw"]
    assert g.set_epw(f["epw"]) == f["epw"] and g.epw == f["epw"]
    return g, D.kernel_code(f["kernel"])


def _compare(g, sim, steps, tag):
    """Step the device over the layout's actions; every env and step against
    the oracle's record."""
    for s in range(steps):
        # the env's draw counter: a step wrongly taken as quiet skips the bearings'
        # draws, which with a single bearing (no fix, no target) leave no other
        # trace before the next reset draws its ducting
        D.assert_step(D.step(g, sim["acts"][s], extra=("ctr",)), sim, s, tag, rew="tol", cog="tol")


@pytest.mark.parametrize("name", FORMS)
def test_reach(name, monkeypatch):
    """Six steps without auto-reset over every seed's layout, trained red. The
    workgroups take either branch as their probe env decides (the isolated
    loud instances fail here if the kernel's predicate is loose; the near-quiet
    ones check the quiet path itself right at the bound)."""
    E = Q.form_sim(name, Q.REACH_SEEDS[0])["E"]
    g, kernel = _make(name, monkeypatch, E)
    quiet_wgs = loud_wgs = 0
    for seed in Q.REACH_SEEDS:
        sim = Q.form_sim(name, seed)
        D.start(g, sim["pos"], seed=seed, duct=sim["duct"], positions=ref_spawns(g.nb))
        _compare(g, sim, Q.REACH_STEPS, (name, seed))
        assert g.step_kernel() == kernel
        assert not g.env_state()["err"].any() and not sim["err"].any()
        loud = sim["loud"][:, sim["probes"]]
        quiet_wgs += int((~loud).sum())
        loud_wgs += int(loud.sum())
    assert quiet_wgs >= 10 and loud_wgs >= 10, (quiet_wgs, loud_wgs)  # both branches, by the oracle
    g.close()


@pytest.mark.parametrize("trained_red", [True, False])
@pytest.mark.parametrize("name", FORMS)
def test_forms_45_steps(name, trained_red, monkeypatch):
    """The same layout with auto-reset and 40-step episodes over 45 steps: the
    quiet tails' in-kernel reset (probe envs respawn at their boundary cells
    under a freshly drawn ducting) and, with an untrained red, the salvo draws
    and their write-back into the action rows."""
    seed = Q.REACH_SEEDS[0]
    sim = Q.form_sim(name, seed, steps=45, trained_red=trained_red, horizon=40)
    g, kernel = _make(name, monkeypatch, sim["E"], auto_reset=True, trained_red=trained_red)
    D.start(g, sim["pos"], seed=seed, duct=sim["duct"], positions=ref_spawns(g.nb))
    _compare(g, sim, 45, (name, trained_red))
    assert g.step_kernel() == kernel
    # the 40th step ends every episode no victory ended before: done stays 1
    # (the reference's flag is 0 at a victory) and the env resets
    assert (sim["done"][39] == 1).any() and sim["reset"][39].any()
    assert not g.env_state()["err"].any() and not sim["err"].any()
    if not trained_red:
        assert not np.array_equal(sim["acts_after"], sim["acts"])  # salvos were written back
    g.close()


@pytest.mark.parametrize("name", FORMS)
def test_form_ran(name, monkeypatch, capfd):
    """Proof that the row's form ran: a handle of the same shape under LNW_PROF
    with every env at the far spawns, one step, the report on stderr. Every
    workgroup (every 64-env unit of the units kernel) must report the quiet
    path, and the "quiet direct" line must appear exactly for the direct forms,
    for every workgroup."""
    f = Q.FORMS[name]
    nb, epw = f["nb"], f["epw"]
    E = Q.form_sim(name, Q.REACH_SEEDS[0])["E"]
    g, kernel = _make(name, monkeypatch, E, prof=True, seed=3)
    g.reset(positions=ref_spawns(nb))
    capfd.readouterr()
    g.step(torch.from_numpy(np.random.default_rng(1).random((E, 2 * nb, 4), dtype=np.float32)).cuda())
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert g.step_kernel() == kernel
    g.close()
    nwg = (E + epw - 1) // epw
    m = re.search(r"\[lnw prof\] quiet workgroups (\d+):", err)
    assert m and int(m.group(1)) == nwg, err
    d = re.search(r"\[lnw prof\] quiet direct (\d+):", err)
    if f["direct"]:
        assert d and int(d.group(1)) == nwg, err
    else:
        assert d is None, err


def test_every_epw_is_accepted():
    """lnw_set_epw takes any 1..64 (the LDS columns keep their 64-lane stride and
    every slab, pass and pair-lane index is bounded by the workgroup's envs) and
    refuses the rest."""
    from lnw import _abi
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    g = BatchedGame(40, ["large"] * 4, ["large"] * 4, scenario=Scenario(landing_ops=False), grid=grid(100))
    for epw in range(1, 65):
        assert g.set_epw(epw) == epw
    for epw in (-1, 65, 128):
        with pytest.raises(_abi.LnwError):
            g.set_epw(epw)
    g.close()
