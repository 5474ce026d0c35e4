"""The units kernel compiled for the production configuration
(step_units_prod_kernel, csrc/lnw_kernels.hip ProdCfg; plan_step / prod_config
in csrc/lnw_host.inc) against the CPU oracle, and the generic units kernel in
its place wherever one of the values it fixes differs.

4v4 on the 100 grid, E = 256 (one workgroup of four 64-env units) and E = 512,
12 Philox steps with 5-step episodes, so every env resets in the kernel twice.
Every env and step is compared with the oracle: observations bit for bit,
rewards within REW_TOL (as the quiet tests compare them), done, cog, the action
rows after the step and the env's draw counter; after the last step the error
flags, the env counters, the ducting and every ship's state.

Inputs:
  ref    every env at the reference spawns: all units quiet, with resets
  mixed  tests/_quiet_cases.py's units layout: probe envs at sensor reach in
         units 0 and 2 of workgroup 0 (1 and 3 of workgroup 1), so phase S runs
         inside the new kernel beside quiet units of the same workgroup
  rows   tests/_move_rows.py: rows that leave phase M's common path (non-finite
         actions, targets outside the move table's window and the A* pass,
         far headings, ties), over quiet, melee and mixed units

Fallback: one case per value of the production configuration (the ones ProdCfg
compiles in and the ones prod_config only checks on the host). Each must report
a kernel that is not the production one and still match the oracle. Needs an
MI355X."""
import functools

import numpy as np
import pytest
import torch

import _device as D
import _move_rows as M
import _oracle
import _quiet_cases as Q
from _spawns import REF_SPAWNS, grid as _grid

pytestmark = pytest.mark.gpu

STEPS, HORIZON, SEED = 12, 5, 11
E_SIM = 512
TYPES = [_oracle.T_LARGE] * 8
TAPE_LEN = 400  # per env: far more than 12 steps and two resets draw
ENV_KEYS = (("n_blue_left", "n_blue_left"), ("n_red_left", "n_red_left"), ("steps_done", "steps_done"),
            ("blue_victory", "blue_victory"), ("red_victory", "red_victory"),
            ("blue_engagements", "blue_eng"), ("red_engagements", "red_eng"))


# ---------------------------------------------------------------------------
# inputs and the oracle's record of them (computed once per case, shared, read-only)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(case, G=100):
    """pos [E_SIM, 8, 2], duct [E_SIM] (NaN: the reset's draw), acts [STEPS, E_SIM, 8, 4] float32,
    probes (envs meant to be loud)."""
    grid = _grid(G)
    if case == "ref":
        pos = np.array([REF_SPAWNS] * E_SIM, np.int32)
        acts = np.random.default_rng(SEED).random((STEPS, E_SIM, 8, 4), dtype=np.float32)
        return pos, np.full(E_SIM, np.nan), acts, []
    if case == "mixed":
        pos, duct, acts, probes = Q.layout(4, 64, SEED, grid, units=True)
        assert pos.shape[0] == E_SIM
        return pos, duct, acts[:STEPS], probes
    assert case == "rows" and G == 100
    acts, _ = M.rows("4v4")
    assert acts.shape[:2] == (STEPS, E_SIM)
    return M.positions("4v4"), np.full(E_SIM, np.nan), acts, []


def _tape(E):
    """Per-env tapes of uniform values (offsets [E + 1])."""
    t = np.random.default_rng(SEED + 1).random(E * TAPE_LEN)
    return t, np.arange(E + 1, dtype=np.int64) * TAPE_LEN


@functools.lru_cache(maxsize=None)
def oracle(case, mode="f32", G=100, E=E_SIM):
    """The oracle over envs 0..E-1 of a case's inputs (an env's record depends on
    its own index only, so a run of the first 256 envs reads the first 256).
    mode: f32 rows | f64 rows | i32 DISCRETE rows | tape (f32 rows, tape RNG)."""
    grid = _grid(G)
    pos, duct, acts32, _ = inputs(case, G)
    discrete = mode == "i32"
    if discrete:  # DISCRETE rows: radar, salvo, cell index, unused (the parity test's ranges)
        r = np.random.default_rng(SEED + 2)
        acts = np.stack([r.integers(0, 2, (STEPS, E, 8)), r.integers(0, 2, (STEPS, E, 8)),
                         r.integers(0, 50, (STEPS, E, 8)), np.zeros((STEPS, E, 8), np.int64)], -1).astype(np.int32)
        kind = _oracle.K_PYINT
    elif mode == "f64":
        acts = acts32[:, :E].astype(np.float64) + 2.0 ** -40  # not float32 values
        kind = _oracle.K_F64
    else:
        acts, kind = acts32[:, :E], _oracle.K_F32
    kinds = np.full(8, kind, np.int32)
    tape, offs = _tape(E) if mode == "tape" else (None, None)
    S = STEPS
    out = _oracle.new_record(S, E, 4, 4, acts.dtype)
    out.update(ctr=np.zeros((S, E), np.int64), loud=np.zeros((S, E), bool), reset=np.zeros((S, E), bool),
               err=np.zeros(E, np.int64), ducting=np.zeros(E), pos=np.zeros((E, 8, 2), np.int64))
    for k in ("radar", "missiles", "alive", "steps_done", "dist_lz", "tl_cnt"):
        out[k] = np.zeros((E, 8))
    for _, k in ENV_KEYS:
        out["env_" + k] = np.zeros(E, np.int64)
    for e in range(E):
        o = _oracle.OracleEnv(grid, 4, 4, discrete=discrete)
        if tape is not None:
            o.set_tape(tape[offs[e]:offs[e + 1]])
        else:
            o.set_philox(SEED, e)
        o.reset(TYPES, pos[e])
        if not np.isnan(duct[e]):
            o.set_ducting(float(duct[e]))
        t = 0
        for s in range(S):
            st0 = o.env_state()
            r = o.step(acts[s, e], kinds)
            st1 = o.env_state()
            ctr = "tape_pos" if tape is not None else "ctr"
            # loud by the oracle alone: the step drew (an EW bearing, a shot) or left a target list
            out["loud"][s, e] = st1[ctr] != st0[ctr] or bool(o.agents()["tl_cnt"].any())
            _oracle.record_step(out, s, e, r)
            t += 1
            if r["done"] == 0 or t >= HORIZON:  # the device's auto-reset
                o.reset(TYPES, pos[e])
                out["reset"][s, e] = True
                t = 0
            out["ctr"][s, e] = o.env_state()[ctr]
        st, ag = o.env_state(), o.agents()
        out["err"][e], out["ducting"][e] = st["err"], st["ducting"]
        for _, k in ENV_KEYS:
            out["env_" + k][e] = st[k]
        for k in ("pos", "radar", "missiles", "alive", "steps_done", "dist_lz", "tl_cnt"):
            out[k][e] = ag[k]
    for v in out.values():
        v.setflags(write=False)
    out.update(acts=acts, kind=kind)
    return out


# ---------------------------------------------------------------------------
# the device run
# ---------------------------------------------------------------------------
def _game(E, monkeypatch, *, G=100, env=None, discrete=False, reward_dtype=torch.float32):
    """A 4v4 handle with 5-step episodes; `env`: knobs read by lnw_create."""
    from lnw.config import Scenario
    sc = Scenario(landing_ops=False, auto_reset=True, episode_steps=HORIZON, discrete=discrete)
    return D.make_game(monkeypatch, E, ["large"] * 4, ["large"] * 4, sc, _grid(G), SEED, env=env, epw=64,
                       reward_dtype=reward_dtype)


def _start(g, case, G=100, tape=False):
    pos, duct, _, _ = inputs(case, G)
    D.start(g, pos, seed=SEED, tape=_tape(g.E) if tape else None, duct=duct, positions=REF_SPAWNS)


def _run(g, sim, tag, *, prod, kernels, row_kind=False):
    """Step the device over the case's actions; every env and step against the
    oracle's record `sim`, then the state left behind. Returns the outputs."""
    E = g.E
    kept = []
    rk = torch.full((E, 8), sim["kind"], dtype=torch.uint8).cuda() if row_kind else None
    for s in range(STEPS):
        out = D.step(g, sim["acts"][s, :E], rk, extra=("ctr",))
        assert g.step_kernel() in kernels, (tag, g.step_kernel())
        assert g.step_kernel_prod() == prod, (tag, "production kernel", g.step_kernel_prod())
        D.assert_step(out, sim, s, tag, rew="tol", cog="tol")
        kept.append(out)
    es, ag = g.env_state(), g.agents()
    assert np.array_equal(es["err"].astype(np.int64), sim["err"][:E]), (tag, "error flags")
    assert np.array_equal(es["ducting"], sim["ducting"][:E]), (tag, "ducting")
    for dk, ok in ENV_KEYS:
        assert np.array_equal(es[dk], sim["env_" + ok][:E]), (tag, dk, D.first(es[dk] != sim["env_" + ok][:E]))
    dpos = np.stack([ag["x"], ag["y"]], -1)
    assert np.array_equal(dpos, sim["pos"][:E]), (tag, "cells", D.first((dpos != sim["pos"][:E]).any(-1)))
    for k in ("radar", "missiles", "alive", "steps_done", "dist_lz", "tl_cnt"):
        assert np.array_equal(ag[k].astype(np.float64), sim[k][:E]), (tag, k)
    return kept


def _units():
    from lnw import _abi
    return (_abi.KERNEL_UNITS,)


# ---------------------------------------------------------------------------
# the production kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("E", [256, 512])
@pytest.mark.parametrize("case", ["ref", "mixed", "rows"])
def test_production_kernel_vs_oracle(case, E, monkeypatch):
    sim = oracle(case)
    g = _game(E, monkeypatch)
    _start(g, case)
    _run(g, sim, (case, E), prod=True, kernels=_units())
    g.close()
    assert (sim["reset"][:, :E].sum(0) >= 2).all()  # every env reset inside the run, twice
    unit_loud = sim["loud"][:, :E].reshape(STEPS, E // 64, 64).any(2)  # [step, unit]
    if case == "ref":
        assert not unit_loud.any() and not sim["err"].any()
    elif case == "mixed":
        # a loud unit beside quiet ones, in the same workgroup and step (phase S inside the kernel)
        wg = unit_loud.reshape(STEPS, E // 256, 4)
        assert (wg.any(2) & ~wg.all(2)).any(), "no step with loud and quiet units in one workgroup"
        probes = [e for e in inputs(case)[3] if e < E]
        assert sim["loud"][:, probes].any()
    else:
        assert sim["err"][:E].any(), "no row raised an error flag"  # non-finite rows do
        assert unit_loud.any() and not unit_loud.all()


@pytest.mark.parametrize("case", ["mixed", "rows"])
def test_no_prod_is_bitwise_the_same(case, monkeypatch):
    """LNW_NO_PROD=1: the generic units kernel on the same inputs, every output
    bitwise equal to the production kernel's, the getter telling the two apart."""
    E = 256
    sim = oracle(case)
    runs = []
    for env, prod in ((None, True), ({"LNW_NO_PROD": "1"}, False)):
        g = _game(E, monkeypatch, env=env)
        _start(g, case)
        runs.append(_run(g, sim, (case, "no_prod" if env else "prod"), prod=prod, kernels=_units()))
        g.close()
    for s, (a, b) in enumerate(zip(*runs)):
        for k in a:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (case, s, k)


# ---------------------------------------------------------------------------
# fallback: one case per value the production kernel fixes
# ---------------------------------------------------------------------------
FALLBACK = {
    # name: keyword arguments of _fallback
    "grid_200": dict(G=200),
    "float64_actions": dict(mode="f64"),
    "int32_actions": dict(mode="i32"),
    "row_kind_given": dict(row_kind=True),
    "profile_buffer": dict(env={"LNW_PROF": "1"}),
    "work_counters": dict(counters=True),
    "tape_rng": dict(mode="tape"),
    "float64_rewards": dict(reward_dtype=torch.float64),
    # bit 23: phase M loads its action rows itself (results unchanged)
    "debug_skip_bit": dict(env={"LNW_DEBUG_SKIP": str(1 << 23)}),
}


@pytest.mark.parametrize("name", sorted(FALLBACK))
def test_fallback_takes_the_generic_kernel(name, monkeypatch, capfd):
    from lnw import _abi
    kw = dict(FALLBACK[name])
    G, mode = kw.get("G", 100), kw.get("mode", "f32")
    E = 256
    sim = oracle("mixed", mode, G, E_SIM if (mode, G) == ("f32", 100) else E)
    g = _game(E, monkeypatch, G=G, env=kw.get("env"), discrete=mode == "i32",
              reward_dtype=kw.get("reward_dtype", torch.float32))
    if kw.get("counters"):
        g.count_work(True)
    _start(g, "mixed", G, tape=mode == "tape")
    # (the 200 grid's layout does not fit four units' LDS: one unit per workgroup)
    kernels = (_abi.KERNEL_UNITS, _abi.KERNEL_TEAM) if G != 100 else _units()
    _run(g, sim, name, prod=False, kernels=kernels, row_kind=kw.get("row_kind", False))
    g.close()
    capfd.readouterr()  # (LNW_PROF's report)
    assert sim["loud"].any() and not sim["loud"][:, :E].all()
