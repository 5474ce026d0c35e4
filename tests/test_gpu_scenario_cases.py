"""Scenario options across launch forms, on the device: every scenario of
tests/_scenario_cases.py through every launch form of its fleet against the
CPU oracle's record of the same 256 envs (tests/test_scenario_cases_cpu.py
shows on the oracle alone that the inputs reach the defensive zone reward, the
landing ending, the distance-0 landing reward, the all-landing-ships-sunk
ending, the neutralised penalty and both outcomes of the scripted red's
aggression draw, in quiet and in contact workgroups of one launch, and that
the option changes the result).

plan_step (csrc/lnw_host.inc) looks at none of these options, so every fast
form runs under every scenario; the rules are restated in the quiet path
(quiet_reward, quiet_cog_sums_t, the aggression draw in both quiet tails) and
in the group kernel beside the one-lane code.

Per case, every env and step: observation hashes, done and the action rows
after the step bit for bit, rewards and cog within _device.REW_TOL / COG_TOL,
no error flag; the kernel lnw_step_kernel reports after every step and what
lnw_step_kernel_prod reports; and for the first 8 envs of the first quiet and
of the first contact block the agents' and the env's state after the last
step against an OracleEnv replay.

Last, the LNW_DEBUG_SKIP bits that the shipped library accepts as result
preserving, one at a time, through the default scenario's forms with the same
comparison. Needs an MI355X."""
import numpy as np
import pytest

import _device as D
import _scenario_cases as C
from _fullsize_util import _compare, _gpu_run
from _spawns import grid as _grid

pytestmark = pytest.mark.gpu

ENV_KEYS = (("n_blue_left", "n_blue_left"), ("n_red_left", "n_red_left"), ("steps_done", "steps_done"),
            ("blue_victory", "blue_victory"), ("red_victory", "red_victory"),
            ("blue_engagements", "blue_eng"), ("red_engagements", "red_eng"))


@pytest.fixture(scope="module")
def replays():
    """OracleEnv replays of the snapshot envs, one per scenario, shared by its forms."""
    cache = {}
    return lambda name: cache.setdefault(name, C.replay(name, C.SNAP_ENVS))


def _run_case(name, form, monkeypatch, replays, *, env=None, kernel=None, prod=None):
    from lnw.config import Scenario
    f, fm = C.fleet(name), C.FORMS[C.SCENARIOS[name]["fleet"]][form]
    n = fm["E"]
    tag = (name, form) + ((env,) if env else ())
    knobs = dict(fm["env"], **(env or {}))
    g = D.make_game(monkeypatch, n, f["blue"], f["red"], Scenario(**C.scenario_kwargs(name)), _grid(f["G"]), C.SEED,
                    env=knobs, epw=fm["epw"], contact=fm["contact"])
    pos, acts = C.inputs(name)
    D.start(g, pos)
    orc = C.oracle_run(name)
    gpu = _gpu_run(g, np.ascontiguousarray(acts[:, :n]), C.mult(name), after=True,
                   kernel=D.kernel_code(fm["kernel"] if kernel is None else kernel))
    assert g.step_kernel_prod() == (C.prod_of(name, form) if prod is None else prod), (tag, "production kernel")
    es, ag = g.env_state(), g.agents()
    g.close()
    _compare(gpu[:4], tuple(orc[k][:, :n] for k in ("hash", "rew", "done", "cog")), tag)
    bad = (gpu[4].astype(np.float32) != orc["acts_after"][:, :n]).any(axis=(2, 3))
    assert not bad.any(), (tag, "action rows after the step", D.first(bad))
    assert not es["err"].any(), (tag, "error flags", D.first(es["err"] != 0))
    ref = replays(name)
    for e in C.SNAP_ENVS:
        oag, ost = ref[e]["agents"], ref[e]["env"]
        for k in ("dist_lz", "steps_done", "alive"):
            assert np.array_equal(ag[k][e].astype(np.float64), oag[k].astype(np.float64)), (tag, "env", e, k)
        assert np.array_equal(np.stack([ag["x"][e], ag["y"][e]], 1), oag["pos"]), (tag, "env", e, "cells")
        for dk, ok in ENV_KEYS:
            assert es[dk][e] == ost[ok], (tag, "env", e, dk)
        assert es["rng"][e] == ost["ctr"], (tag, "env", e, "draw counter")


@pytest.mark.parametrize("name,form", C.CASES)
def test_scenario_in_form(name, form, monkeypatch, replays):
    _run_case(name, form, monkeypatch, replays)


@pytest.mark.parametrize("bit,name,form", C.BIT_CASES)
def test_accepted_debug_bit_preserves_results(bit, name, form, monkeypatch, replays):
    """A bit lnw_create accepts in the shipped library changes where loads are
    issued or which loop runs, never a result."""
    kernel = C.bit_kernel(bit, form) if name == "default" else None
    _run_case(name, form, monkeypatch, replays, env={"LNW_DEBUG_SKIP": str(1 << bit)}, kernel=kernel, prod=False)


def test_every_form_row_is_in_the_table():
    """The forms the issue lists, by fleet (test_scenario_in_form asserts each
    row's kernel after every step of every scenario)."""
    assert set(C.FORMS["4v4"]) == {"units", "units_prod", "epw64_staged", "epw32_two_slab", "epw32_no_slab",
                                   "epw16_direct", "epw8", "contact_epw64", "contact_epw16"}
    assert set(C.FORMS["3v3ls"]) == {"epw64", "epw16_direct", "group"}
    assert set(C.FORMS["8v10ls"]) == {"group", "lane"}
    assert {s for s, _ in C.CASES} == set(C.SCENARIOS)
