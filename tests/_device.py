"""The device side of a parity test: a handle in a given launch form, its start
on a layout, one step's outputs as host arrays, and the one comparison of such
a step with the oracle's record of it (_oracle.new_record / record_step).

TEST INFRASTRUCTURE. What "equals the oracle" means is written here once; a
caller names the strictness of the fields that have more than one mode
(tests/test_helpers_cpu.py shows what each catches)."""
import numpy as np

REW_TOL = 1e-5  # float32 outputs against float64 sums below 1 000
COG_TOL = 1e-5

KERNEL_NAMES = {"team": "KERNEL_TEAM", "team_contact": "KERNEL_TEAM_CONTACT", "units": "KERNEL_UNITS",
                "group": "KERNEL_GROUP", "generic": "KERNEL_GENERIC", "reflos": "KERNEL_REFLOS"}


def kernel_code(name):
    """lnw_step_kernel's value for a kernel as the tests' tables name it."""
    from lnw import _abi
    return getattr(_abi, KERNEL_NAMES[name.lower()])


def make_game(monkeypatch, E, blue, red, scenario, grid, seed=0, *, env=None, epw=None, contact=False, **kw):
    """A handle in a launch form. env {NAME: value}: knobs that lnw_create (or the
    constructor's automatic epw choice) reads once, set around the constructor
    and deleted again; epw: forced, and asserted to be in force; contact: the
    contact variant; kw: further BatchedGame keywords."""
    from lnw.batched import BatchedGame
    env = env or {}
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    g = BatchedGame(E, list(blue), list(red), scenario=scenario, grid=grid, seed=seed, **kw)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    if contact:
        g.set_variant(True)
    if epw:
        assert g.set_epw(epw) == epw and g.epw == epw
    return g


def start(g, pos, *, seed=None, tape=None, duct=None, positions=None):
    """Philox under `seed` or the tape (values, offsets) where given; reset to the
    per-env cells pos [>= E, A, 2] (positions: the spawn spec's cells, env 0's by
    default); then the ducting overwritten where duct [>= E] is not NaN."""
    import torch
    from lnw._abi import F_DUCT
    E = g.E
    if tape is not None:
        g.set_tape(*tape)
    elif seed is not None:
        g.set_rng(seed)
    pos = np.array(pos[:E], np.int32)
    g.reset(positions=pos[0] if positions is None else positions, pos_per_env=torch.from_numpy(pos))
    if duct is not None and not np.isnan(duct[:E]).all():
        d = g.get(F_DUCT).cpu().numpy()
        fixed = ~np.isnan(duct[:E])
        d[fixed] = duct[:E][fixed]
        g.set(F_DUCT, torch.from_numpy(d))


def step(g, acts, row_kind=None, extra=()):
    """One step over the host action rows acts [E, A, 4]: the outputs as host
    arrays by the record's keys, acts_after among them; extra: of "ctr" (the
    env's draw counter), "pos_after" (the ships' cells) and "err"."""
    import torch
    from lnw import _abi
    act = torch.from_numpy(np.array(acts)).cuda()
    out = {k: v.cpu().numpy() for k, v in g.step(act, row_kind).items()}
    out["acts_after"] = act.cpu().numpy()
    if "ctr" in extra:
        out["ctr"] = g.get(_abi.F_RNG).cpu().numpy()
    if "pos_after" in extra:
        ag = g.agents()
        out["pos_after"] = np.stack([ag["x"], ag["y"]], -1)
    if "err" in extra:
        out["err"] = g.get(_abi.F_ERR).cpu().numpy()
    return out


def first(bad):
    return np.argwhere(bad)[:4].tolist()


def _bits_differ(a, b):
    """Per env: a and b differ in some bit (so -0.0 is not 0.0 and a NaN equals only itself)."""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    a, b = (np.ascontiguousarray(x).view(np.uint8).reshape(len(x), -1) for x in (a, b))
    return (a != b).any(axis=1)


NAMES = {"acts_after": "action rows after the step", "ctr": "draw counter", "pos_after": "cells", "err": "error flags"}


def assert_step(got, rec, s, tag, *, rew=None, cog=None):
    """One step's device outputs `got` ([E, ...] host arrays) against step s of the
    oracle's record `rec` ([steps, >= E, ...]). Compared: the record's output
    keys, all of which got must hold, and those of ctr / pos_after / err that
    got holds, which the record then must.
      obs_blue, obs_red, acts_after   bit for bit
      rew_blue, rew_red   rew="tol": within REW_TOL of the float64 record | "bits": its float32, bit for bit
      cog                 cog="tol": within COG_TOL | "exact": the record's float32; NaN = NaN in both
      done, ctr, pos_after, err       equal
    A failure names tag, step, field and the first four envs."""
    def check(key, bad):
        assert not bad.any(), (tag, s, NAMES.get(key, key), "envs", first(bad))

    def ref(key):
        return rec[key][s, :len(got[key])]

    for key in ("obs_blue", "obs_red"):
        if key in rec:
            check(key, _bits_differ(got[key], ref(key)))
    for key in ("rew_blue", "rew_red"):
        if key in rec:
            assert rew in ("tol", "bits"), "rewards: name the mode"
            if rew == "tol":
                check(key, ~(np.abs(got[key] - ref(key)) <= REW_TOL).all(axis=1))
            else:
                check(key, _bits_differ(got[key], ref(key).astype(np.float32)))
    if "done" in rec:
        check("done", got["done"] != ref("done"))
    if "cog" in rec:
        assert cog in ("tol", "exact"), "cog: name the mode"
        cg, oc = got["cog"], ref("cog")
        same = np.abs(cg - oc) <= COG_TOL if cog == "tol" else cg == oc.astype(np.float32)
        check("cog", ~(same | (np.isnan(cg) & np.isnan(oc))))
    if "acts_after" in rec:
        check("acts_after", _bits_differ(got["acts_after"], ref("acts_after")))
    for key in ("ctr", "pos_after", "err"):
        if key in got:
            g, r = got[key], ref(key)
            bad = g.astype(np.uint32) != r if key == "err" else g != r
            check(key, bad.reshape(len(g), -1).any(axis=1))
