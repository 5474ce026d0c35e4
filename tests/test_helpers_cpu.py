"""The tests' shared helpers (CPU): _device.assert_step fails on every kind of
difference it is there to catch and names field, step and env; _spawns'
generators return the arrays the tests have always used (digests taken from the
copies they replace); _codeobj takes the library apart once per process."""
import ast
import hashlib
import os
import subprocess

import numpy as np
import pytest

import _codeobj
import _device as D
import _oracle
import _spawns

S, E, NB = 2, 3, 2
MODES = [(r, c) for r in ("tol", "bits") for c in ("tol", "exact")]
EXTRA = ("ctr", "pos_after", "err")


def _record():
    """A synthetic record of 2 steps, 3 envs, 2v2 (rows of 60 floats): rewards
    that no float32 holds, zeros in the rows, a NaN cog."""
    rng = np.random.default_rng(0)
    rec = _oracle.new_record(S, E, NB, NB)
    assert rec["obs_blue"].shape == (S, E, NB, 60)
    for k in ("obs_blue", "obs_red", "acts_after"):
        rec[k][:] = 1.0 + rng.random(rec[k].shape, dtype=np.float32)
    rec["obs_blue"][..., 7] = 0.0
    for k in ("rew_blue", "rew_red", "cog"):
        rec[k][:] = 1.0 + rng.random(rec[k].shape)
    rec["cog"][1, 2] = np.nan
    rec["done"][:] = rng.integers(0, 3, (S, E))
    rec.update(ctr=rng.integers(0, 99, (S, E)), pos_after=rng.integers(0, 99, (S, E, 2 * NB, 2)),
               err=rng.integers(0, 3, (S, E)).astype(np.uint32))
    return rec


def _device_outputs(rec, s, keys=_oracle.RECORD_KEYS + EXTRA):
    """What a device that equals the oracle returns for step s (float32 rewards and cog)."""
    return {k: rec[k][s].astype(np.float32) if k[:3] in ("rew", "cog") else rec[k][s].copy() for k in keys}


def _fails(got, rec, s, rew, cog, field, env):
    with pytest.raises(AssertionError) as info:
        D.assert_step(got, rec, s, "tag", rew=rew, cog=cog)
    assert info.value.args[0] == ("tag", s, field, "envs", [[env]]), info.value.args[0]


def _ulp(a, idx):
    a[idx] = np.nextafter(a[idx], np.float32(np.inf))


def _flip(a, idx):
    a.view(np.uint32)[idx] ^= 1


def _set(key, idx, f):
    return lambda g: g[key].__setitem__(idx, f(g[key][idx]))


CHANGES = {
    # name: (field in the message, env, the change to step 1's device outputs)
    "obs_one_ulp": ("obs_red", 2, lambda g: _ulp(g["obs_red"], (2, 1, 30))),
    "obs_minus_zero": ("obs_blue", 1, _set("obs_blue", (1, 0, 7), lambda v: -v)),  # (float equality lets it pass)
    "reward_two_tol": ("rew_blue", 0, _set("rew_blue", (0, 1), lambda v: v + 2 * D.REW_TOL)),
    "done": ("done", 2, _set("done", 2, lambda v: v + 1)),
    "cog_nan_for_a_number": ("cog", 0, _set("cog", 0, lambda v: np.nan)),
    "cog_a_number_for_nan": ("cog", 2, _set("cog", 2, lambda v: 0.5)),
    "action_row_bit": ("action rows after the step", 1, lambda g: _flip(g["acts_after"], (1, 3, 2))),
    "draw_counter": ("draw counter", 0, _set("ctr", 0, lambda v: v + 1)),
    "cell": ("cells", 2, _set("pos_after", (2, 3, 1), lambda v: v + 1)),
    "error_flag": ("error flags", 1, _set("err", 1, lambda v: v ^ 2)),
}


@pytest.mark.parametrize("rew,cog", MODES)
def test_equal_outputs_pass(rew, cog):
    rec = _record()
    for s in range(S):  # (step 1: NaN against NaN in cog)
        D.assert_step(_device_outputs(rec, s), rec, s, "tag", rew=rew, cog=cog)


@pytest.mark.parametrize("rew,cog", MODES)
@pytest.mark.parametrize("name", sorted(CHANGES))
def test_a_difference_fails_and_is_named(name, rew, cog):
    rec = _record()
    field, env, change = CHANGES[name]
    got = _device_outputs(rec, 1)
    change(got)
    if name == "obs_minus_zero":
        assert np.signbit(got["obs_blue"][1, 0, 7]) and np.array_equal(got["obs_blue"], rec["obs_blue"][1])
    _fails(got, rec, 1, rew, cog, field, env)


def test_one_ulp_passes_the_tolerance_modes_only():
    rec = _record()
    for key, idx, modes in (("rew_red", (1, 0), ("bits", "tol")), ("cog", 1, ("tol", "exact"))):
        got = _device_outputs(rec, 0)
        _ulp(got[key], idx)
        D.assert_step(got, rec, 0, "tag", rew="tol", cog="tol")
        _fails(got, rec, 0, *modes, key, 1)


def test_modes_are_named_keys_present_and_batches_shorter_than_the_record():
    rec = _record()
    got = _device_outputs(rec, 0)
    for kw in (dict(cog="tol"), dict(rew="tol")):
        with pytest.raises(AssertionError, match="name the mode"):
            D.assert_step(got, rec, 0, "tag", **kw)
    rows = ("obs_blue", "obs_red")  # a record of rows alone needs no mode
    D.assert_step(_device_outputs(rec, 1, rows), {k: rec[k] for k in rows}, 1, "tag")
    del got["done"]
    with pytest.raises(KeyError):  # a field of the record that the device outputs lack is no pass
        D.assert_step(got, rec, 0, "tag", rew="tol", cog="tol")
    got = {k: v[:2] for k, v in _device_outputs(rec, 1).items()}  # the record's first envs
    D.assert_step(got, rec, 1, "tag", rew="bits", cog="exact")
    _ulp(got["obs_blue"], (1, 1, 59))
    _fails(got, rec, 1, "bits", "exact", "obs_blue", 1)


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def test_generators_are_pinned():
    g100, g200 = _spawns.grids()
    assert _spawns.MELEE_BOXES == ((30, 45, 40, 60), (55, 70, 45, 65))
    assert _digest(_spawns.box_positions(g100, 128, 4, 4, 64)) == "11df7d8d05119cfa"
    pos = _spawns.box_positions(g200, 9, 8, 10, 5, (60, 80, 60, 100), (100, 125, 70, 110))
    assert _digest(pos) == "6199c6612d45c570"
    assert _digest(_spawns.melee_block(g100, 64, 0)) == "09ccd9fc35bebe9c"
    assert _digest(_spawns.melee_block(g100, 5, 643, 3, 3)) == "fa41780581b00442"
    assert _digest(_spawns.hash_mult(544, seed=99)) == "75c0350d6cac6608"


def test_grids_are_loaded_once_and_read_only():
    assert _spawns.grid(100) is _spawns.grids()[0] and _spawns.grid(200) is _spawns.grids()[1]
    assert _spawns.grid(100).shape == (100, 100) and _spawns.grid(200).shape == (200, 200)
    with pytest.raises(ValueError):
        _spawns.grid(100)[0, 0] = 1
    assert _spawns.ref_spawns(4) == _spawns.REF_SPAWNS and len(_spawns.ref_spawns(2)) == 4


@_codeobj.needs_lib
@_codeobj.needs_tools
def test_metadata_reader_extracts_once(monkeypatch):
    keys = ("private_segment_fixed_size", "sgpr_spill_count")
    first = _codeobj.kernel_metadata(_codeobj.LIB, keys)
    calls = []
    run = subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda *a, **kw: calls.append(a) or run(*a, **kw))
    assert _codeobj.kernel_metadata(_codeobj.LIB, keys) == first and first
    assert _codeobj.kernel_scratch(_codeobj.LIB) == {k: v["private_segment_fixed_size"] for k, v in first.items()}
    assert calls == []


def _tables(module, *names):
    """Module-level literals of a test file, read from its source (no test module imports another)."""
    tree = ast.parse(open(os.path.join(os.path.dirname(__file__), module + ".py")).read())
    found = {t.id: ast.literal_eval(n.value) for n in tree.body if isinstance(n, ast.Assign)
             for t in n.targets if isinstance(t, ast.Name) and t.id in names}
    return [found[n] for n in names]


@_codeobj.needs_lib
@_codeobj.needs_tools
def test_metadata_reader_finds_every_listed_kernel():
    wanted = ["step_kernel" + f for f in _tables("test_step_args_cpu", "STEP_KERNELS")[0]]
    wanted += _tables("test_units_prod_cpu", "GENERIC", "PROD")
    for module in ("test_kernel", "test_paramnoise", "test_ppo_sample", "test_ppolearn", "test_qlearn", "test_qnet"):
        wanted += list(_tables(module + "_resources_cpu", "LIMITS")[0])
    assert len(wanted) > 50
    names = list(_codeobj.kernel_metadata(_codeobj.LIB, ("private_segment_fixed_size",)))
    for frag in wanted:
        assert any(frag in n for n in names), f"kernel {frag} not found"
