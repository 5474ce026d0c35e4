"""The inputs of tests/test_gpu_team_sizes.py have the power they are there for,
shown on the CPU oracle alone: its mean is numpy's bit for bit, and every case
of tests/_team_cases.py reaches, by the oracle's own step statistics, the code
above config 4 (8v10) that it is built for: EW fixes averaged over 8 and over
9..15 points (numpy sums pairwise from 8 on), firings over target lists longer
than the 16 entries the group kernel stages, landing-ship rewards, bearings
with dy < 0 (the negated half of the bearing table) and an auto-reset."""
import numpy as np
import pytest

import _fix_order_cases as F
import _oracle
import _team_cases as T


def test_oracle_mean_is_numpy_mean():
    """orc_np_mean against numpy.mean of a list of Python floats, bitwise, for
    n = 1..17 and 250 vectors per n whose exponents spread over 2^24, so that
    the order of summation decides the last bits: a plain left-to-right sum
    differs from numpy's for some vector at every n >= 9 (and agrees below 8)."""
    rng = np.random.default_rng(17)
    for n in range(1, 18):
        plain_differs = 0
        for _ in range(250):
            v = rng.standard_normal(n) * 2.0 ** rng.integers(-12, 13, n)
            lst = [float(x) for x in v]
            want = float(np.mean(lst))
            got = _oracle.np_mean(v)
            assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (n, lst)
            s = 0.0
            for x in lst:
                s += x
            plain_differs += (s / n) != want
        if n >= 9:
            assert plain_differs > 0, n
        if n < 8:
            assert plain_differs == 0, n


def _takers(types):
    return sum(t in ("small", "large") for t in types)


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_case_reaches_its_code(name):
    cs = T.CASES[name]
    st = T.stat_sums(name)
    nb, nr = len(cs["blue"]), len(cs["red"])
    far = "bearings outside the +-40 window: %d" % st["bear_far"]
    print(name, st, far)
    assert cs["E"] % 32 != 0 and 70 <= cs["E"] <= 200
    if max(_takers(cs["blue"]), _takers(cs["red"])) >= 9:
        assert st["fix_eq8"] >= 100 and st["fix_gt8"] >= 100, st
    if min(nb, nr) >= 10:
        assert st["tl_past16"] >= 20 and st["tl_max"] > 16, st
    if "ls" in cs["red"]:
        assert st["ls_reward"] > 0, st
    if cs["form"] == T.ALL:
        assert st["bear_dyneg"] > 0, st
    assert (T.oracle_run(name)["stats"][:, _oracle.STATS.index("resets")] > 0).all(), st
    if cs["acts_after"]:
        r = T.oracle_run(name)
        assert not np.array_equal(r["acts_after"], T.actions(cs))  # salvos were written back


def test_stats_driver_matches_per_env():
    """orc_fullsize_range's statistics and records against the same envs stepped
    one by one (OracleEnv.stats), on the first envs of a case with landing ships."""
    name = "11v12ls_g100"
    cs = T.CASES[name]
    full = T.oracle_run(name)
    one = T.per_env(cs, range(5))
    for k in ("hash", "rew", "done", "cog", "acts_after"):
        assert np.array_equal(full[k][:, :5], one[k], equal_nan=True), k
    assert np.array_equal(full["stats"][:5], one["stats"])
    assert one["stats"][:, _oracle.STATS.index("fix_gt8")].sum() > 0


@pytest.mark.parametrize("name", sorted(F.CASES))
def test_fix_order_case_depends_on_the_order(name):
    """tests/_fix_order_cases.py: with numpy's order (the oracle's mean) the
    fix is a target or not as the case says; with a plain left-to-right sum it is
    the opposite. The oracle's step gives every blue ship numpy's outcome and
    consumes the tape to its end, without an error flag."""
    c = F.CASES[name]
    n = len(c["blue"])
    assert F.targets(c, _oracle.np_mean) == c["want"] == F.targets(c, lambda v: float(np.mean(v)))
    assert F.targets(c, F.plain_mean) == 1 - c["want"]
    r, o = F.oracle_step(c)
    assert o.agents()["tl_cnt"].tolist() == [c["want"]] * n + [0]
    assert (r["obs_blue"][:, -3] == c["want"]).all()
    st = o.env_state()
    assert st["tape_pos"] == 1 + n * n and st["err"] == 0
