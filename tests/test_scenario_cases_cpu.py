"""tests/_scenario_cases.py on the CPU oracle alone: each scenario's inputs
reach the rules the scenario is there for (the oracle's step statistics,
counted separately over the quiet and the contact blocks), and the option it
changes shows in the result (against the same inputs under the option's
default). These are conditions on the inputs, not measurements of a kernel:
tests/test_gpu_scenario_cases.py compares the kernels with these records.

The oracle itself is pinned to the reference on the same rules by the episode
fixtures of tests/golden/make_golden.py make_option_episodes
(tests/test_oracle_golden.py)."""
import numpy as np
import pytest

import _oracle
import _scenario_cases as C

NAMES = sorted(C.SCENARIOS)
CHANGED = [n for n in NAMES if C.SCENARIOS[n]["baseline"]]


def test_table_covers_the_issue():
    """Every option of lnw_params differs from its default in some scenario, and
    every fleet's forms name distinct launches."""
    differing = set().union(*(C.SCENARIOS[n]["options"] for n in NAMES))
    assert differing == set(C.OPTION_DEFAULTS), sorted(set(C.OPTION_DEFAULTS) - differing)
    assert C.SCENARIOS["landing_moved_zone"]["options"]["lz"] != C.LZ
    for forms in C.FORMS.values():
        rows = [tuple(sorted((k, str(v)) for k, v in f.items())) for f in forms.values()]
        assert len(set(rows)) == len(rows)
    assert len(C.CASES) >= 70 and sorted(b for b in C.DEBUG_BITS) == sorted({b for b, _, _ in C.BIT_CASES})


@pytest.mark.parametrize("name", NAMES)
def test_inputs_reach_their_rules(name):
    o = C.options(name)
    q, c = C.block_stats(name, True), C.block_stats(name, False)
    st = C.oracle_run(name)["stats"]
    ix = _oracle.STATS.index
    assert q["err"] == 0 and c["err"] == 0
    # every quiet block: no bearing taken, no target list fired over, no loss; every contact block: bearings
    for b in range(C.E // C.BLOCK):
        blk = st[b * C.BLOCK:(b + 1) * C.BLOCK]
        if b % 2 == 0:
            assert blk[:, ix("bearings")].sum() == 0 and blk[:, ix("tl_max")].max() == 0, (name, b)
            assert blk[:, ix("neut_pen")].sum() == 0 and blk[:, ix("ls_sunk_end")].sum() == 0, (name, b)
        else:
            assert blk[:, ix("bearings")].sum() >= 1000, (name, b)
    # one reset at the least in every env (the 20-step horizon inside 25 steps)
    assert (st[:, ix("resets")] >= 1).all()
    if not o["aggressive"] and C.SCENARIOS[name]["layout"] != "landing":
        assert q["def_in"] >= 50 and q["def_out"] >= 50, (name, q)
        assert c["neut_pen"] >= 20, (name, c)
    if o["aggressive"]:
        assert q["def_in"] + q["def_out"] + c["def_in"] + c["def_out"] + q["neut_pen"] + c["neut_pen"] == 0
    if o["landing_ops"]:
        assert q["landings"] >= 8 and c["landings"] >= 4, (name, q, c)
        assert q["ls_dist0"] >= q["landings"] and c["ls_dist0"] >= c["landings"], (name, q, c)
        assert c["ls_sunk_end"] >= 4, (name, c)
        # game.py:484: a landing increments blue_victory, once per landed ship
        assert q["blue_vict"] >= q["landings"] and q["red_vict"] == 0, (name, q)
    else:
        assert q["landings"] + c["landings"] + q["ls_sunk_end"] + c["ls_sunk_end"] == 0
    if name.startswith("aggression"):
        for blocks in (q, c):
            assert blocks["agg_fired"] >= 20 and blocks["agg_held"] >= 20, (name, blocks)
    if o["trained_red"]:
        assert q["agg_fired"] + q["agg_held"] + c["agg_fired"] + c["agg_held"] == 0
    else:  # the draws' write-back shows in the action rows
        aft = C.oracle_run(name)["acts_after"]
        assert (aft != C.inputs(name)[1].astype(np.float32)).any(axis=(0, 2, 3)).sum() >= C.E // 2
    assert c["blue_vict"] + c["red_vict"] >= 20, (name, c)  # contact blocks end episodes by victory too


@pytest.mark.parametrize("name", CHANGED)
def test_option_changes_the_result(name):
    """The same inputs under the default of the scenario's changed option give
    another observation hash, reward or done in 5 % of the (step, env) pairs at
    the least: a kernel that ignored the option, or read its default, fails the
    comparison."""
    frac = C.changed_fraction(name)
    print(name, "changed share", frac)
    assert frac >= 0.05, (name, frac)


def test_units_forms_and_partial_forms_share_envs():
    """The forms of 200 envs read the first 200 of the 256 (Philox is keyed by the
    global env id): both block kinds are in either, and the last workgroup of 200
    is partial at 64, 32 and 16 envs per workgroup (8 divides 200: there the
    last block's boundary at 192 falls inside the run instead)."""
    q = C.quiet_env(np.arange(C.E_PART))
    assert q.sum() >= 64 and (~q).sum() >= 64
    assert [C.E_PART % w for w in (64, 32, 16)] == [8, 8, 8]
    assert set(C.SNAP_ENVS) <= set(range(C.E_PART))


@pytest.mark.parametrize("name", ["landing_4v4ls", "defensive_untrained", "discrete_defensive"])
def test_replay_matches_the_batch_run(name):
    """OracleEnv stepped env by env (what the GPU test reads the final state
    from) gives the batch driver's statistics: same resets, same landings."""
    envs = C.SNAP_ENVS[:2] + C.SNAP_ENVS[8:10]
    st = C.oracle_run(name)["stats"]
    f = C.fleet(name)
    nb, nr = len(f["blue"]), len(f["red"])
    pos, acts = C.inputs(name)
    o = C.options(name)
    kinds = np.full(nb + nr, _oracle.K_PYINT if o["discrete"] else _oracle.K_F32, np.int32)
    from _spawns import grid
    for e in envs:
        env = _oracle.OracleEnv(grid(f["G"]), nb, nr, **o)
        env.set_philox(C.SEED, e)
        env.reset(C.types(name), pos[e])
        rew = []
        for s in range(C.STEPS):
            r = env.step(acts[s, e], kinds)
            rew.append(np.concatenate([r["rew_blue"], r["rew_red"]]))
            if r["done"] == 0 or env.env_state()["steps_done"] >= C.HORIZON:
                env.reset(C.types(name), pos[e])
        one = env.stats()
        for k in ("landings", "ls_dist0", "def_in", "def_out", "neut_pen", "agg_fired", "bearings"):
            assert one[k] == st[e, _oracle.STATS.index(k)], (name, e, k)
        assert np.array_equal(np.array(rew, np.float32), C.oracle_run(name)["rew"][:, e]), (name, e)
