"""Red-side MAPPO training on the GPU: lnw.rollout.Rollout(side="red",
warmup=...) in both implementations and the policy kernels' `script_self` mode.

  1. the reference's own `PPO.rollout` with SIDE == "red" (two recorded 3v3
     rollouts, tests/golden/make_redside_golden.py), replayed in tape mode;
  2. the warm-up rows (scripted actions, the red actor's log-probabilities);
  3. the fused kernels against the torch implementation with keyed sampling;
  4. `script_self` launched directly, plain and over a population;
  5. a rollout sharded by env_id_base; 6. a captured graph; 7. rollout ->
     minibatch -> step with PPOLearner on the red actor and critic.

Tolerances are the project's: log-probabilities 1e-4 (given actions) and 1e-3
(sampled ones, whose action itself carries 1e-5), values 1e-5, rewards 1e-5
against the reference and exact between the implementations."""
import copy
import ctypes as C
import json

import numpy as np
import pytest
import torch

from _oracle import load_fixture
from _spawns import box_positions, grid as _grid

pytestmark = pytest.mark.gpu

NAMES = {0: "small", 1: "large", 2: "ls"}
WARMUP = 15  # the reference's `s > 14`


def bits(t):
    return t.contiguous().view(torch.uint8)


def _actor(D, seed):
    """An actor with its BatchNorm / LayerNorm affines and running statistics
    away from their initial values."""
    from lnw.rollout import BatchedActor
    torch.manual_seed(seed)
    a = BatchedActor.for_obs(D).cuda()
    with torch.no_grad():
        for m in (a.norm1, a.norm2):
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 2.0)
            m.weight.uniform_(0.5, 1.5)
            m.bias.uniform_(-0.1, 0.1)
        a.layernorm.weight.uniform_(0.5, 1.5)
        a.layernorm.bias.uniform_(-0.1, 0.1)
    return a


def _game(E, nb, nr, seed=8, base=0, pos=None, f64=True, side="red"):
    """nb small blue ships against nr large red ones, spawned in the melee boxes
    of tests/_spawns.py (`pos`: the envs' cells, else drawn for E envs)."""
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    grid = _grid(100)
    sc = Scenario(landing_ops=False, trained_red=True, side=side, auto_reset=False)
    g = BatchedGame(E, ["small"] * nb, ["large"] * nr, scenario=sc, grid=grid, seed=seed, env_id_base=base,
                    reward_dtype=torch.float64 if f64 else torch.float32)
    g.set_variant(True)
    if pos is None:
        pos = box_positions(grid, E, nb, nr, 5)
    g.reset(positions=pos[0], pos_per_env=torch.from_numpy(np.ascontiguousarray(pos)))
    return g


def _nets(g, seed=4):
    """(blue actor, red actor, red critic) for a game's fleets."""
    from lnw.rollout import BatchedCritic
    blue, red = _actor(g.Db, seed), _actor(g.Dr, seed + 1)
    torch.manual_seed(seed + 2)
    return blue, red, BatchedCritic(g.Dr * g.nr).cuda()


def _clone(out):
    return {k: v.clone() for k, v in out.items()}


# ---- 1. reference parity -----------------------------------------------------------
@pytest.mark.parametrize("impl", ["hip", "torch"])
@pytest.mark.parametrize("name", ["redside_3v3", "redside_3v3_breaks"])
def test_redside_rollout_matches_reference(name, impl):
    """_rollout_case of test_gpu_rollout_golden.py for the red side. Over all
    steps: the step's action array (float64, the scripted rows exact), its value
    kind, rewards, episode lengths, reward-to-go and the tape's consumption;
    over t >= 15: observations bit for bit, log-probabilities, values (before
    that the reference stores zeros, the blue actor's log-probabilities and the
    critic's value of zeros: Rollout's documented deviations)."""
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    from lnw.rollout import BatchedActor, BatchedCritic, Rollout
    fx = load_fixture(f"rollout_{name}.npz")
    meta = json.loads(str(fx["meta"]))
    eps, R, T, nb, nr = meta["episodes"], meta["R"], meta["T"], meta["nb"], meta["nr"]
    types = eps[0]["types"]
    A = len(types)
    grid = _grid(100)
    sc = Scenario(landing_ops=meta["landing_ops"], trained_red=meta["trained_red"],
                  tactics="aggressive", side="red", auto_reset=False)
    g = BatchedGame(R, [NAMES[t] for t in types[:nb]], [NAMES[t] for t in types[nb:]],
                    scenario=sc, grid=grid, reward_dtype=torch.float64)
    tapes = [fx["tape"][e["tape_start"]:e["tape_end"]] for e in eps]
    offs = np.concatenate([[0], np.cumsum([len(t) for t in tapes])]).astype(np.int64)
    g.set_tape(np.concatenate(tapes), offs)
    pos = np.array([e["spawn"] for e in eps], np.int32)
    g.reset(positions=pos[0], rand_ls=[0] * A, pos_per_env=torch.from_numpy(pos))
    st = g.agents()
    assert np.array_equal(np.stack([st["x"], st["y"]], 2), pos), "spawn cells"
    assert np.array_equal(g.env_state()["ducting"], [e["ducting"] for e in eps]), "ducting"
    assert (g.Db, g.Dr) == (meta["Db"], meta["Dr"])

    def weights(pre):
        return {k[len(pre):]: fx[k] for k in fx if k.startswith(pre)}

    actor = BatchedActor.for_obs(g.Db).load_reference(weights("actor.")).cuda()
    red_actor = BatchedActor.for_obs(g.Dr).load_reference(weights("red_actor.")).cuda()
    red_critic = BatchedCritic(g.Dr * nr).load_reference(weights("red_critic.")).cuda()
    r = Rollout(g, actor, red_critic, steps=T, red_actor=red_actor, gamma=meta["gamma"], impl=impl,
                side="red", warmup=WARMUP)
    r.record_actions = True
    rng_after = []  # every env's draw counter after each step (the tape position)
    out = r.run(forced_actions=torch.from_numpy(fx["act"]).cuda(),
                on_step=lambda t, o: rng_after.append(g.env_state()["rng"].copy()))
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    run = o["running"]
    n_steps = np.array(meta["n_steps"])
    assert np.array_equal(run.sum(1), n_steps)
    assert all(run[e, :n].all() for e, n in enumerate(n_steps))
    # the array handed to step(), float64: the profiles' rows, the replayed actor outputs, zeros for sunk ships
    for e, n in enumerate(n_steps):
        np.testing.assert_array_equal(o["step_actions"][e, :n], fx["act"][e, :n], err_msg=f"step array, env {e}")
    np.testing.assert_array_equal(o["f32_step"] & run, fx["act_f32"].astype(bool))
    np.testing.assert_allclose(o["rewards"], fx["rew"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(o["rtg"], fx["batch_rtg"][..., 0], rtol=1e-5, atol=1e-5)
    used = np.array([rng_after[n - 1][e] for e, n in enumerate(n_steps)])
    assert np.array_equal(used, [len(t) for t in tapes]), (used, [len(t) for t in tapes])
    # t >= 15: what the reference stores
    np.testing.assert_array_equal(o["obs"][:, WARMUP:], fx["batch_obs"][:, WARMUP:])
    d_lp = np.abs(o["log_probs"][:, WARMUP:] - fx["batch_log_probs"][:, WARMUP:]).max()
    d_v = np.abs(o["values"][:, WARMUP:, None, None] - fx["batch_values"][:, WARMUP:]).max()
    print(f"{name} {impl}: t >= {WARMUP} log-probabilities {d_lp:.3e}, values {d_v:.3e}")
    np.testing.assert_allclose(o["log_probs"][:, WARMUP:], fx["batch_log_probs"][:, WARMUP:], rtol=0, atol=1e-4)
    np.testing.assert_allclose(o["values"][:, WARMUP:, None, None].repeat(nr, 2), fx["batch_values"][:, WARMUP:],
                               rtol=0, atol=1e-5)
    np.testing.assert_array_equal(o["sampled"], run & (np.arange(T) >= WARMUP)[None])
    # the warm-up holds the real rows here (a deviation by design), for running envs
    assert all(o["obs"][e, t].any() for e, n in enumerate(n_steps) for t in range(min(n, WARMUP)))
    # rows after a `break` are zeros in every buffer
    for e, n in enumerate(n_steps):
        for k in ("obs", "actions", "log_probs", "rewards", "values", "running", "sampled"):
            assert not o[k][e, n:].any(), (k, e)
    g.close()


# ---- 2. warm-up rows -----------------------------------------------------------------
def test_warmup_rows():
    """For t < warmup the buffers hold the float32 script rows (zeros for ships
    past the table's three profiles, sunk ships and ended envs) and the red
    actor's get_dist of them on the stored observations."""
    from lnw.rollout import Rollout, red_script_table
    E, T, W, nb, nr = 96, 8, 5, 3, 5
    g = _game(E, nb, nr)
    blue, red, critic = _nets(g)
    out = Rollout(g, blue, critic, steps=T, red_actor=red, side="red", warmup=W, keyed_seed=11).run()
    torch.cuda.synchronize()
    table = red_script_table("cuda")
    rows = torch.zeros((T, nr, 4), dtype=torch.float64, device="cuda")
    rows[:, :3] = table[:, :T].transpose(0, 1)
    rows32 = rows.to(torch.float32)[None].expand(E, T, nr, 4)
    run = out["running"]
    # a sunk ship's observation row is zeros (compiled_picture), a live one's is not
    alive = out["obs"].abs().sum(-1) > 0
    keep = (alive & run[:, :, None])[..., None]
    want_a = torch.where(keep, rows32, torch.zeros((), device="cuda"))
    assert torch.equal(out["actions"][:, :W], want_a[:, :W])
    assert (out["actions"][:, :W, 3:] == 0).all() and (out["actions"][:, :W, :3] != 0).any()
    with torch.no_grad():
        lp, _ = red.get_dist(out["obs"][:, :W].reshape(-1, g.Dr), want_a[:, :W].reshape(-1, 4), bn="sample")
    want_lp = torch.where(keep[:, :W], lp.reshape(E, W, nr, 4), torch.zeros((), device="cuda"))
    d = float((out["log_probs"][:, :W] - want_lp).abs().max())
    print(f"warm-up log-probabilities against torch get_dist: {d:.3e}")
    assert d <= 1e-4
    assert bool(keep[:, :W].any()) and bool((out["log_probs"][:, :W] != 0).any())
    assert not out["sampled"][:, :W].any()
    assert torch.equal(out["sampled"][:, W:], run[:, W:])
    assert not out["f32_step"][:, :W].any()
    # sampled steps: other actions than the profiles'
    assert not torch.equal(out["actions"][:, W:], want_a[:, W:])
    g.close()


# ---- 3. HIP against torch, keyed sampling ---------------------------------------------
def _run_pair(E, nb, nr, T, W, pos, **kw):
    outs = {}
    for impl in ("hip", "torch"):
        g = _game(E, nb, nr, pos=pos)
        blue, red, critic = _nets(g)
        r = Rollout_(g, blue, critic, steps=T, red_actor=red, side="red", warmup=W, impl=impl, keyed_seed=21, **kw)
        r.call_index(2)
        outs[impl] = _clone(r.run())
        g.close()
    return outs["hip"], outs["torch"]


def Rollout_(*a, **kw):
    from lnw.rollout import Rollout
    return Rollout(*a, **kw)


def _compare_sampled(h, t, W, tag):
    """Both implementations draw the same keyed normals, so their sampled
    actions agree to 1e-5 (float32 network arithmetic in another order), not
    bit for bit. Ties: an env one of whose actions lies within that distance of
    a decision threshold of the step can take the other branch in one
    implementation (a shot fired or not, a cell further or not), and the two
    envs part ways from there. What a step decides shows in its discrete
    outputs: the rewards, the running flag, the next observations and the row
    kinds. An env is compared through the last step up to which all of these are
    identical, and there the actions, log-probabilities and values have to agree
    within the tolerances; envs that part must stay rare (at 1e-5 per value and
    roughly 10^3 action values per env and rollout, well under one env in ten)."""
    E, T = h["running"].shape
    dev = h["obs"].device
    rew_eq = (h["rewards"] == t["rewards"]).all(2)          # [E, T]
    same = (h["obs"] == t["obs"]).all(3).all(2) & (h["running"] == t["running"]) & (h["f32_step"] == t["f32_step"])
    same[:, 1:] &= rew_eq[:, :-1]                           # step t is reached on the same path
    upto = torch.cumprod(same.long(), 1).bool()            # ... and so was every step before it
    whole = upto[:, -1] & rew_eq[:, -1]
    parted = (~whole).nonzero().flatten().tolist()
    print(f"{tag}: envs identical in every discrete output: {int(whole.sum())} of {E}; parted: "
          f"{[(e, int(upto[e].sum())) for e in parted]} (env, first differing step)")
    assert float(whole.float().mean()) >= 0.9
    assert upto[:, 0].all()
    m = upto[:, :, None, None]
    z = torch.zeros((), device=dev)
    d_a = float(torch.where(m, (h["actions"] - t["actions"]).abs(), z).max())
    samp = (torch.arange(T, device=dev) >= W)[None, :, None, None]
    d_lp_s = float(torch.where(m & samp, (h["log_probs"] - t["log_probs"]).abs(), z).max())
    d_lp_w = float(torch.where(m & ~samp, (h["log_probs"] - t["log_probs"]).abs(), z).max())
    d_v = float(torch.where(upto, (h["values"] - t["values"]).abs(), z).max())
    print(f"{tag}: actions {d_a:.3e}, log-probabilities sampled {d_lp_s:.3e} scripted {d_lp_w:.3e}, values {d_v:.3e}")
    assert d_a <= 1e-5 and d_lp_s <= 1e-3 and d_lp_w <= 1e-4 and d_v <= 1e-5
    # scripted actions carry no arithmetic: exact
    assert torch.equal(torch.where(m[:, :W], h["actions"][:, :W], z), torch.where(m[:, :W], t["actions"][:, :W], z))
    assert torch.equal(h["sampled"] & upto, t["sampled"] & upto)
    # envs that never part: every buffer that holds no network arithmetic is identical
    for k in ("obs", "running", "rewards", "f32_step", "rtg", "sampled"):
        assert torch.equal(h[k][whole], t[k][whole]), k


@pytest.mark.parametrize("nb,nr,E", [(3, 3, 171),   # 513 red rows: a second block of one row
                                     (3, 5, 103)])  # Dr = 72, n_in = 35: the 64-wide kernel; ships 3, 4 past the table
def test_fused_redside_matches_torch_impl(nb, nr, E):
    T, W = 20, 3
    pos = box_positions(_grid(100), E, nb, nr, 5)
    h, t = _run_pair(E, nb, nr, T, W, pos)
    # the inputs reach what the test is about (on the torch implementation's own output)
    run, obs = t["running"], t["obs"]
    zero_row = (obs == 0).all(3)                                   # [E, T, nr]: a sunk ship's row (or an ended env's)
    lost = zero_row[:, 1:] & ~zero_row[:, :-1] & run[:, 1:, None]   # first zero row of a ship in a running env
    late = lost[:, W - 1:]                                          # at steps t >= W
    print(f"{nb}v{nr}: red ships lost at t >= {W} in running envs: {int(late.sum())}, "
          f"envs ended early: {int((~run[:, -1]).sum())} of {E}")
    assert late.any(), "no env loses a red ship after the warm-up"
    assert (~run[:, -1]).any() and run[:, -1].any(), "no env ends early (or all do)"
    if nr > 3:
        assert (t["actions"][:, :W, 3:] == 0).all() and (h["actions"][:, :W, 3:] == 0).all()
    _compare_sampled(h, t, W, f"{nb}v{nr} warmup {W}")
    # no warm-up at all, and nothing but warm-up
    for w in (0, T):
        h, t = _run_pair(E, nb, nr, T, w, pos)
        _compare_sampled(h, t, w, f"{nb}v{nr} warmup {w}")
        assert torch.equal(h["sampled"], h["running"] & (w == 0))
        assert (not h["f32_step"].any()) if w == T else bool(h["f32_step"][:, 0].all())


# ---- 4. script_self, launched directly -------------------------------------------------
def _direct_case(E, nb, n, D, seed, sets=1):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    A = nb + n
    obs = torch.rand((E, n, D), generator=gen, device="cuda")
    obs[:, :, :49] = torch.randint(0, 256, (E, n, 49), generator=gen, device="cuda") / 255.0
    alive = (torch.rand((A, E), generator=gen, device="cuda") > 0.15).to(torch.uint8)
    live = (torch.rand(E, generator=gen, device="cuda") > 0.2).to(torch.uint8)
    script = torch.rand((3, 40, 4), generator=gen, device="cuda", dtype=torch.float64)
    actors = [_actor(D, seed + k) for k in range(sets)]
    params = torch.stack([a.packed_policy() for a in actors]).contiguous()
    return dict(E=E, nb=nb, n=n, D=D, A=A, obs=obs, alive=alive, live=live, script=script, actors=actors,
                params=params)


def _outputs(c):
    E, n, D, A = c["E"], c["n"], c["D"], c["A"]
    return dict(obs=torch.full((E, n, D), -1.0, device="cuda"), act=torch.full((E, n, 4), -1.0, device="cuda"),
                logp=torch.full((E, n, 4), -1.0, device="cuda"),
                full=torch.full((E, A, 4), -1.0, dtype=torch.float64, device="cuda"),
                kinds=torch.full((E, A), 9, dtype=torch.uint8, device="cuda"),
                f32=torch.full((E,), 9, dtype=torch.uint8, device="cuda"))


def _launch(c, out, lo, hi, t, script_self, pop=None, member=0, other_rows=False):
    """One launch over envs [lo, hi) of case c at step t: the side's own rows
    scripted (script_self) or sampled at slot (call 2, T 7, t, which 2)."""
    from lnw import _abi
    L = _abi.load()
    n, D, A, nb = c["n"], c["D"], c["A"], c["nb"]
    alive = c["alive"][:, lo:hi].contiguous()
    call = torch.tensor([2], dtype=torch.int64, device="cuda")
    pa = _abi.PolicyArgs()
    pa.obs, pa.E, pa.n, pa.D, pa.own0, pa.A = c["obs"][lo:].data_ptr(), hi - lo, n, D, nb, A
    pa.params = c["params"][member].data_ptr()
    pa.seed, pa.call_dev, pa.t, pa.which = 99, call.data_ptr(), t, 2
    pa.T = 0 if script_self else 7  # (T is not needed by the mode)
    pa.row_base = (1000 + lo) * n
    pa.alive, pa.live = alive.data_ptr(), c["live"][lo:].data_ptr()
    pa.obs_out, pa.obs_env_stride = out["obs"][lo:].data_ptr(), n * D
    pa.act_out, pa.logp_out, pa.act_env_stride = out["act"][lo:].data_ptr(), out["logp"][lo:].data_ptr(), n * 4
    pa.full = out["full"][lo:].data_ptr()
    pa.kinds, pa.kinds_f32_all_alive = out["kinds"][lo:].data_ptr(), 0 if script_self else 1
    pa.f32_out, pa.f32_env_stride = out["f32"][lo:].data_ptr(), 1
    if script_self:
        pa.script_self = 1
    if script_self or other_rows:
        pa.script, pa.script_n, pa.script_steps = c["script"].data_ptr(), 3, 40
    if other_rows:  # the other side's rows by the lane of ship 0, in the same launch
        pa.script_own0, pa.script_cnt = 0, nb
    if pop is not None:
        pp = _abi.PolicyPop(pop, c["params"].shape[1])
        _abi.check(L.lnw_policy_act_pop(C.byref(pa), C.byref(pp), None))
    else:
        _abi.check(L.lnw_policy_act(C.byref(pa), None))
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,D", [(3, 64), (5, 72)])
def test_script_self_direct(n, D):
    """The mode's outputs against their definition, and that it consumes no
    draw: a sampled launch at the same slot gives the same bits whether or not
    a script_self launch ran before it."""
    E, nb, t = 400, 3, 6
    c = _direct_case(E, nb, n, D, 13 + n)
    got = _outputs(c)
    _launch(c, got, 0, E, t, True, other_rows=True)
    alive = c["alive"].t().bool()                  # [E, A]
    own = alive[:, nb:, None]
    keep = own & c["live"].bool()[:, None, None]
    rows = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    rows[:3] = c["script"][:, t]
    rows = rows[None].expand(E, n, 4)
    z64 = torch.zeros((), dtype=torch.float64, device="cuda")
    z32 = torch.zeros((), device="cuda")
    # the step's array: the table's float64 rows themselves, zeros for sunk ships
    assert torch.equal(got["full"][:, nb:], torch.where(own, rows, z64))
    assert (rows.float().double() != rows).any()
    # the other side's rows of the same launch
    other = c["script"][:, t][None].expand(E, 3, 4)
    assert torch.equal(got["full"][:, :nb], torch.where(alive[:, :nb, None], other, z64))
    assert torch.equal(got["act"], torch.where(keep, rows.float(), z32))
    with torch.no_grad():
        lp, _ = c["actors"][0].get_dist(c["obs"].reshape(E * n, D), rows.float().reshape(E * n, 4), bn="sample")
    want = torch.where(keep, lp.reshape(E, n, 4), z32)
    d = float((got["logp"] - want).abs().max())
    print(f"script_self n={n} D={D}: log-probabilities against torch get_dist {d:.3e}")
    assert d <= 1e-4 and bool(keep.any()) and bool((~keep).any())
    assert (got["kinds"] == 3).all() and (got["f32"] == 0).all()  # LNW_KIND_F64
    lv = c["live"].bool()[:, None, None]
    assert torch.equal(got["obs"], torch.where(lv, c["obs"], z32))
    # a step past the table: zero rows
    late = _outputs(c)
    _launch(c, late, 0, E, 40, True)
    assert (late["full"][:, nb:] == 0).all() and (late["act"] == 0).all()
    # no draw consumed
    a, b = _outputs(c), _outputs(c)
    _launch(c, a, 0, E, t, False)
    _launch(c, b, 0, E, t, True)
    _launch(c, b, 0, E, t, False)
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert not torch.equal(a["act"], got["act"])


def test_script_self_population_equals_member_launches():
    """lnw_policy_act_pop with script_self against lnw_policy_act on each
    member's envs with the member's set: G n = 600 rows per member, so every
    member straddles a 512-row block and the last one holds fewer envs."""
    E, nb, n, D, G, t = 450, 3, 3, 64, 200, 4
    c = _direct_case(E, nb, n, D, 29, sets=3)
    pop, one = _outputs(c), _outputs(c)
    _launch(c, pop, 0, E, t, True, pop=G, other_rows=True)
    for k in range(3):
        _launch(c, one, k * G, min((k + 1) * G, E), t, True, member=k, other_rows=True)
    for key in pop:
        assert torch.equal(bits(pop[key]), bits(one[key])), key
    # the members' sets matter
    assert not torch.equal(pop["logp"][G:2 * G], _member0(c, G, t)["logp"][G:2 * G])


def _member0(c, G, t):
    c2 = dict(c, params=c["params"][:1].expand(3, -1).contiguous())
    out = _outputs(c2)
    _launch(c2, out, 0, c["E"], t, True, pop=G)
    return out


# ---- 5. sharding -------------------------------------------------------------------------
def test_sharded_redside_rollout():
    """One game of 128 envs against two of 64 with env_id_base 0 and 64."""
    E, T, W, G = 128, 8, 3, 32
    pos = box_positions(_grid(100), E, 3, 3, 5)
    kw = dict(steps=T, side="red", warmup=W, keyed_seed=13, noise=0.05, param_noise=(0.05, 0.05), envs_per_member=G)

    def run(lo, hi):
        g = _game(hi - lo, 3, 3, seed=77, base=lo, pos=pos[lo:hi])
        blue, red, critic = _nets(g)
        r = Rollout_(g, blue, critic, red_actor=red, **kw)
        r.call_index(3)
        out = _clone(r.run())
        g.close()
        return out

    whole, lo, hi = run(0, E), run(0, 64), run(64, E)
    assert torch.equal(whole["member"].cpu(), torch.arange(E) // G)
    for k, v in whole.items():
        assert torch.equal(bits(torch.cat([lo[k], hi[k]])), bits(v)), k
    assert not whole["running"].all() and whole["sampled"].any()
    # the members act with different actors: the noise is there
    assert not torch.equal(whole["log_probs"][:G, :W], whole["log_probs"][G:2 * G, :W])


# ---- 6. graph ------------------------------------------------------------------------------
def test_redside_graph_replay_matches_eager():
    E, T, W = 512, 10, 4
    g = _game(E, 3, 3, seed=5)
    blue, red, critic = _nets(g)
    r = Rollout_(g, blue, critic, steps=T, red_actor=red, side="red", warmup=W, noise=0.05, seed=99)
    r.capture()
    pos = box_positions(_grid(100), E, 3, 3, 5)
    g.reset(positions=pos[0], pos_per_env=torch.from_numpy(pos))
    snap = g.get_state(device="cuda")  # incl. RNG counters
    r.call_index(7)
    eager = _clone(r.run())
    assert r.call_index() == 8
    g.set_state(snap)
    r.call_index(7)
    out = r.replay()
    torch.cuda.synchronize()
    assert r.call_index() == 8
    for k, v in eager.items():
        assert torch.equal(bits(out[k]), bits(v)), k
    first = out["actions"][:, W].clone()
    g.set_state(snap)
    out2 = r.replay()  # rollout index 8: other draws
    torch.cuda.synchronize()
    assert torch.equal(out2["obs"][:, 0], eager["obs"][:, 0])
    assert torch.equal(out2["actions"][:, 0], eager["actions"][:, 0])  # (scripted)
    assert not torch.equal(out2["actions"][:, W], first)
    g.close()


# ---- 7. end to end -----------------------------------------------------------------------
def test_redside_rollout_minibatch_step():
    """Rollout(side="red") acting from the learner's vector with parameter
    noise -> minibatch -> step, the kernels against the torch restatement of the
    learner; the next rollout, without export(), acts with the updated vector;
    and minibatch_dist's merge over two shards equals minibatch on their union
    (one process playing the ranks, as tests/test_gpu_ppo_dist.py does)."""
    from _ppo_dist_cases import SEED, SLOT, bits as nbits, check_rank, play
    from _ppolearn_util import ACTOR_GRAD_NAMES, CRITIC_GRAD_NAMES, NOISE, close_loss, segs
    from lnw.ppolearn import PPOLearner
    E, T, W, G, B = 32, 10, 3, 16, 64
    nb = nr = 4
    pos = box_positions(_grid(100), E, nb, nr, 5)
    g = _game(E, nb, nr, seed=3, pos=pos, f64=False)
    blue, red, critic = _nets(g)
    red_t, critic_t = copy.deepcopy(red), copy.deepcopy(critic)
    H = PPOLearner(red, critic, sample_seed=5)
    Tm = PPOLearner(red_t, critic_t, impl="torch", device="cuda")
    assert (H.n, H.D) == (nr, g.Dr)
    snap = g.get_state(device="cuda")
    r = Rollout_(g, blue, critic, steps=T, red_actor=red, side="red", warmup=W, seed=5, theta=H.theta_actor,
                 param_noise=(0.05, 0.05), envs_per_member=G)
    out = _clone(r.run())
    assert tuple(out["obs"].shape) == (E, T, nr, g.Dr) and out["sampled"].any()
    batch = H.minibatch(out, B)
    assert batch["obs"].data_ptr() == out["obs"].data_ptr() and len(set(batch["index"].tolist())) == B
    solid = H.grad(batch, update_running=False)  # (where a gradient is more than rounding noise)
    before = H.theta_actor.clone()
    lh, lt = H.step(batch), Tm.step(batch)
    assert all(bool(x.isfinite()) for x in lh)
    close_loss("actor loss", lh[0], lt[0], 1e-4)
    close_loss("critic loss", lh[1], lt[1], 1e-4)
    assert not torch.equal(before, H.theta_actor)
    for th, tt, sl, names, gr in ((H.theta_actor, Tm.theta_actor, H.actor_sl, ACTOR_GRAD_NAMES, solid["actor_grad"]),
                                  (H.theta_critic, Tm.theta_critic, H.critic_sl, CRITIC_GRAD_NAMES,
                                   solid["critic_grad"])):
        a, b_, gs = segs(th, sl, names), segs(tt, sl, names), segs(gr, sl, names)
        for nm in names:
            if nm in NOISE:
                continue
            ok = gs[nm].abs() > 1e-6
            d = (a[nm] - b_[nm]).abs()
            worst = float(d[ok].max() if ok.any() else 0.0)
            assert worst <= 0.02 * H.lr, (nm, worst)
    # the next rollout reads the updated vector (no export): same envs, same rollout index, same noise
    g.set_state(snap)
    r.call_index(0)
    out2 = r.run()
    assert torch.equal(out2["obs"][:, 0], out["obs"][:, 0])
    assert not torch.equal(out2["log_probs"][:, 0], out["log_probs"][:, 0])
    g.close()
    # two shards of 16 envs (env_id_base 0 and 16) against their union
    shards = []
    for lo in (0, 16):
        gs_ = _game(16, nb, nr, seed=3, base=lo, pos=pos[lo:lo + 16], f64=False)
        rs = Rollout_(gs_, blue, critic, steps=T, red_actor=red, side="red", warmup=W, seed=5, theta=H.theta_actor,
                      param_noise=(0.05, 0.05), envs_per_member=G)
        shards.append(_clone(rs.run()))
        gs_.close()
    rows = 16 * T * nr  # rows per shard: row_base = env_id_base * T * nr
    flat = dict(obs=torch.cat([s["obs"] for s in shards]).reshape(-1, nr, g.Dr).contiguous(),
                rtg=torch.cat([s["rtg"] for s in shards]).reshape(-1).float().contiguous(),
                actions=torch.cat([s["actions"] for s in shards]).reshape(-1, 4).contiguous(),
                log_probs=torch.cat([s["log_probs"] for s in shards]).reshape(-1, 4).contiguous(),
                values=torch.cat([s["values"] for s in shards]).reshape(-1).contiguous())
    H.draw.fill_(SLOT)
    one = _clone({k: v for k, v in H.minibatch(flat, B, seed=SEED, row_base=0, advance=False).items() if k != "obs"})
    want_rows = one["index"].cpu().numpy()
    got, _, _, _ = play(H, flat, [(0, rows), (rows, 2 * rows)], B, nr, 0, "hip")
    for gk in got:
        check_rank(gk, flat, want_rows, nbits(one["key"]), nr, 0)
    assert (want_rows < rows).any() and (want_rows >= rows).any()
