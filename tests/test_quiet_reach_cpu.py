"""The power of the quiet-path inputs (tests/_quiet_cases.py), shown on the CPU
oracle alone: for every layout tests/test_gpu_quiet_reach.py steps, over its
seeds, the probe envs sit at sensor reach often enough that a kernel whose
quiet predicate were loose (a position combination ignored, a spread lane on
the wrong env, the reach one cell short) would fail there.

The counts are conditions on the generator, met by the reference alone; the
printed lines are the figures DESIGN.md ("The quiet predicate at sensor
reach") quotes."""
import math

import numpy as np
import pytest

import _oracle
import _quiet_cases as Q


def _layouts():
    seen = {}
    for name, f in Q.FORMS.items():
        seen.setdefault((f["nb"], f["epw"], f["G"], f["units"], f["red"]), name)
    return sorted(seen.values())


def test_reach_formula_is_the_oracles():
    """reach(duct) (the formula of lnw_device.h's d5) against the oracle's own
    ew_range between two 30 m masts, at the probe values and across 1 <= d < 2;
    it is the widest range of all ship classes."""
    L = _oracle.lib()
    for d in list(Q.DUCTS) + list(np.linspace(1.0, 1.999, 250)):
        d = float(d)
        assert Q.reach(d) == L.orc_ew_range(d, _oracle.T_LARGE, _oracle.T_LARGE)
        assert Q.max_range2(d) == Q.reach(d) ** 2
    assert [Q.reach(d) for d in Q.DUCTS] == [19, 25, 36]


def test_layout_shape():
    """Two full workgroups and a ragged one, one probe each: lanes cycling over
    first, last and middle, the ragged one's last valid lane; every other env at
    the reference spawns; all probe cells water."""
    for name in _layouts():
        f = Q.FORMS[name]
        grid = Q._grid(f["G"])
        lanes = set()
        for seed in Q.REACH_SEEDS:
            pos, duct, acts, probes = Q.layout(f["nb"], f["epw"], seed, grid, f["units"])
            E, epw, nb = pos.shape[0], f["epw"], f["nb"]
            assert acts.shape == (45, E, 2 * nb, 4) and acts.dtype == np.float32
            if f["units"]:
                assert E == 512 and len({e // 64 for e in probes}) == 4
                assert sorted({e // 256 for e in probes}) == [0, 1]
            else:
                assert E == 2 * epw + max(1, epw // 3) and E % epw != 0
                assert [e // epw for e in probes] == [0, 1, 2] and probes[2] == E - 1
                lanes |= {e % epw for e in probes[:2]}
            far = np.setdiff1d(np.arange(E), probes)
            assert np.isnan(duct[far]).all() and set(duct[probes]) <= set(Q.DUCTS)
            assert (pos[far] == np.array(Q.ref_spawns(nb))).all()
            for e in probes:
                assert all(grid[x, y] <= 74 for x, y in pos[e]), (name, seed, e)
        if not f["units"]:
            assert lanes == {0, f["epw"] - 1, f["epw"] // 2}, name


@pytest.mark.parametrize("name", _layouts())
def test_inputs_have_power(name):
    f = Q.FORMS[name]
    tot = None
    gaps = set()
    for seed in Q.REACH_SEEDS:
        sim = Q.form_sim(name, seed)
        assert not sim["err"].any()
        t = Q.tally(sim, f["epw"])
        tot = t if tot is None else {k: tot[k] + t[k] for k in t}
        for e in sim["probes"]:
            gaps.add(math.isqrt(int(sim["near2"][0, e])) - math.isqrt(int(sim["r2"][0, e])))
    print(f"[quiet reach] {name}: isolated loud {tot['isolated']}, near-quiet {tot['near_quiet']}, "
          f"dead ship inside the bound {tot['dead_inside']}, first step's nearest combination, cells from the reach: {sorted(gaps)}")
    for m, k, c in zip(Q.MUTANTS, tot["kills"], tot["candidates"]):
        print(f"[quiet reach] {name}: mutant '{m}': killed {k} times, differs from the predicate in {c} instances")
    # soundness of the stated predicate: quiet by it, yet loud in the reference
    assert tot["unsound"] == 0
    assert tot["isolated"] >= 10
    assert tot["near_quiet"] >= 10
    for m, k in zip(Q.MUTANTS, tot["kills"]):
        # a mutant no instance kills is slack in the specification:
        # blue's old cell is never looked at once red has moved
        assert k == 0 or k >= 3, (m, k)
    killable = [m for m, k in zip(Q.MUTANTS, tot["kills"]) if k]
    assert set(killable) >= set(Q.MUTANTS) - {"drop blue-old/red-new"}, killable
