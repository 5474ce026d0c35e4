"""The actor, critic and rollout kernels of csrc/lnw_actor.hip at every fleet
size, against a float64 oracle (tests/_net_oracle.py).

A side's rows have D = 4 n + 52 floats, the network input n_in = D - 37; from
five ships on, n_in passes 32 and features_kernel / policy_act_kernel run their
<64> instantiation (68-float tile rows over a smaller pooled-map area, two fc1
k-pairs, a 14-quad clamped tail, weights read from global memory), and
rollout_post_kernel launches one wave per ship, so its fc2 / fc3 tile dealing
and its LDS layout change with every n. The tolerances are the project's own
(features rtol 1e-4 atol 2e-5, log-probabilities 1e-4, values 1e-5), applied
against float64; every comparison prints err_hip and err_ref (the float32 host
arm), both max-abs against float64."""
import pytest
import torch

import _net_oracle as O
from _spawns import box_positions, grid as _grid

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


# ---------------------------------------------------------------- 1: features
@pytest.mark.parametrize("bn", ["sample", "running"])
@pytest.mark.parametrize("n", [2, 5, 8, 12])
def test_features_kernel_against_float64(n, bn):
    """lnw_actor_features on 333 rows (one 256-row block plus 77): n = 2 is
    features_kernel<32>, n = 5 / 8 / 12 (n_in 35 / 47 / 63) are <64>."""
    import copy
    c = O.features_case(n, bn)
    with torch.no_grad():
        got = copy.deepcopy(c["actor"]).cuda().features(c["obs"].cuda(), bn)
    assert got.shape == c["want"].shape == (333, c["D"] - 37)
    O.report(f"features n={n} D={c['D']} {bn}", got, c["ref"], c["want"], O.FEAT_ATOL, O.FEAT_RTOL)


# ---------------------------------------------------------------- 2: policy, direct ABI
@pytest.mark.parametrize("bn", ["sample", "running"])
@pytest.mark.parametrize("n", [4, 5, 8, 12])
def test_policy_act_forced_against_float64(n, bn):
    """lnw_policy_act with forced actions on 150 envs of n ships (600 / 750 /
    1200 / 1800 rows: full 512-row blocks and a ragged one whose last wave is
    partial), own0 = 2, sunk ships, ended episodes and strided, sentinel-filled
    outputs. n = 4 is policy_act_kernel<32>, the others <64>."""
    c = O.policy_case(n, bn)
    E, own0, A = c["E"], c["own0"], c["A"]
    assert (E * n) % 512 and (E * n) % 64
    print(f"policy n={n} D={c['D']} {bn}: float64 oracle moves by",
          ", ".join(f"{v:.2f} ({k})" for k, v in c["moved"].items()))
    out = O.policy_call(c, c["actor"].packed_policy().cuda())
    keep, own_alive = c["keep"], c["own_alive"]
    lp = out["logp"][:, :4 * n].reshape(E, n, 4).cpu()
    ao = out["act"][:, :4 * n].reshape(E, n, 4).cpu()
    full = out["full"].cpu()
    O.report(f"log-probabilities n={n} D={c['D']} {bn}", lp[keep], c["ref"][keep], c["want"][keep], O.LOGP_ATOL)
    assert not lp[~keep].any()  # (zeros, not the sentinel: written)
    assert torch.equal(ao, torch.where(keep[:, :, None], c["act"], torch.zeros(())))
    assert torch.equal(full[:, own0:], torch.where(own_alive[:, :, None], c["act"].double(),
                                                   torch.zeros((), dtype=torch.float64)))
    assert (full[:, :own0] == O.SENTINEL).all()  # the other side's rows
    assert (out["logp"][:, 4 * n:] == O.SENTINEL).all() and (out["act"][:, 4 * n:] == O.SENTINEL).all()


# ---------------------------------------------------------------- 3: layout invariants
@pytest.mark.parametrize("n,bn", [(5, "sample"), (12, "running")])
def test_policy_act_layout_invariants(n, bn):
    """policy_act_kernel<64> computes every row on its own, bit for bit: rows
    read through an env stride with NaN padding equal the packed call, envs
    [40, 111) run alone equal those rows of the whole call, and a second
    identical call equals the first."""
    c = O.policy_case(n, bn)
    params = c["actor"].packed_policy().cuda()
    base = O.policy_call(c, params)
    again = O.policy_call(c, params)
    strided = O.policy_call(c, params, in_stride=n * c["D"] + 8)
    lo, hi = 40, 111
    part = O.policy_call(c, params, lo=lo, hi=hi)
    assert torch.isfinite(base["logp"]).all()
    for k in ("logp", "act", "full"):
        assert torch.equal(bits(again[k]), bits(base[k])), ("second call", k)
        assert torch.equal(bits(strided[k]), bits(base[k])), ("strided rows", k)
        assert torch.equal(bits(part[k]), bits(base[k][lo:hi])), ("envs alone", k)


# ---------------------------------------------------------------- 4: rollout_post, direct ABI
POST_SHAPES = [(1, 56), (2, 60), (3, 64), (4, 68), (5, 72), (8, 84), (12, 100), (16, 100)]


@pytest.mark.parametrize("n,D", POST_SHAPES)
def test_rollout_post_against_float64(n, D):
    """lnw_rollout_post on 100 envs (the second workgroup holds 36) with one
    wave per ship: values against the float64 critic, the masking of ended
    episodes, the live update, strided outputs around sentinels, rewards in
    both dtypes, and the call without a critic."""
    c = O.critic_case(n, D)
    E = c["E"]
    if c["moved"] is not None:
        print(f"critic n={n} D={D}: float64 oracle moves by {c['moved']:.2f} with ships 0 and {n - 1} exchanged")
    packed = c["critic"].packed(n, D).cuda()
    lv, dn = c["live"].bool(), c["done"] != 0
    zero = torch.zeros((), dtype=torch.float64)
    for stop in (1, 0):
        for rew_f64 in (False, True):
            out = {k: v.cpu() for k, v in O.post_call(c, packed, stop, rew_f64).items()}
            val, tag = out["val"][:, 0], f"values n={n} D={D} stop_at_done={stop} rew_f64={int(rew_f64)}"
            if stop:
                O.report(tag, val[lv], c["ref"][lv], c["want"][lv], O.VALUE_ATOL)
                assert not val[~lv].any()
                assert torch.equal(out["rew"][:, :n], torch.where(lv[:, None], c["rew"], zero))
                assert torch.equal(out["live"].bool(), lv & dn)
            else:
                O.report(tag, val, c["ref"], c["want"], O.VALUE_ATOL)
                assert torch.equal(out["rew"][:, :n], c["rew"])
                assert torch.equal(out["live"], c["live"])
            assert torch.equal(out["running"][:, 0].bool(), lv) and out["running"][:, 0].max() == 1
            assert (out["val"][:, 1:] == O.SENTINEL).all() and (out["rew"][:, n:] == O.SENTINEL).all()
            assert (out["running"][:, 1] == 9).all()
    out = {k: v.cpu() for k, v in O.post_call(c, None, 1, True).items()}
    assert (out["val"] == O.SENTINEL).all()
    assert torch.equal(out["rew"][:, :n], torch.where(lv[:, None], c["rew"], zero))
    assert torch.equal(out["running"][:, 0].bool(), lv) and torch.equal(out["live"].bool(), lv & dn)


# ---------------------------------------------------------------- 5: whole rollouts
GAMES = {
    # spawn boxes of test_gpu_group.py's 5v3_g100 / 12v12_g100 cases on grid100
    "5v3_script": dict(blue=["small"] * 5, red=["large"] * 3, red_mode="script",
                       box_b=(30, 45, 40, 60), box_r=(50, 65, 45, 65)),
    "12v12_actor": dict(blue=["small"] * 12, red=["large"] * 12, red_mode="actor",
                        box_b=(30, 45, 40, 60), box_r=(45, 60, 45, 65)),
}


@pytest.mark.parametrize("name", sorted(GAMES))
def test_fused_rollout_matches_torch_impl_large_fleets(name):
    """test_fused_rollout_matches_torch_impl (test_gpu_rollout.py) at 5 and 12
    blue ships, where the policy's n_in is 35 and 63: with forced actor outputs
    every buffer of Rollout(impl="hip") agrees with impl="torch" —
    observations, actions, running flags, rewards, row kinds and reward-to-go
    exactly, log-probabilities within 1e-4, values within 1e-5 — and one step
    of keyed sampling with exploration noise agrees within 1e-5."""
    from lnw import _abi
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    from lnw.rollout import Rollout
    cs = GAMES[name]
    red = cs["red_mode"]
    E, T = 96, 6
    nb, nr = len(cs["blue"]), len(cs["red"])
    A = nb + nr
    grid = _grid(100)
    pos = torch.from_numpy(box_positions(grid, E, nb, nr, 5, cs["box_b"], cs["box_r"]))
    sc = Scenario(landing_ops=False, trained_red=red != "script", auto_reset=False)

    def game(**kw):
        g = BatchedGame(E, cs["blue"], cs["red"], scenario=sc, grid=grid, seed=8, **kw)
        g.set_variant(True)
        g.reset(positions=pos[0].numpy(), pos_per_env=pos)
        return g

    Db, Dr = O.obs_dim(nb), O.obs_dim(nr)
    actor = O.make_actor(Db, 11).cuda()
    critic = O.make_critic(nb, Db, 12).cuda()
    red_actor = O.make_actor(Dr, 13).cuda() if red == "actor" else None
    assert actor.layernorm.normalized_shape[0] > 32
    gen = torch.Generator(device="cuda").manual_seed(3)
    forced = torch.rand((E, T, A, 4), generator=gen, device="cuda")
    outs = {}
    for impl in ("hip", "torch"):
        g = game(reward_dtype=torch.float64)
        assert (g.Db, g.Dr) == (Db, Dr)
        r = Rollout(g, actor, critic, steps=T, red=red, red_actor=red_actor, impl=impl)
        outs[impl] = {k: v.clone() for k, v in r.run(forced_actions=forced).items()}
        outs[impl]["alive"] = g.get(_abi.F_ALIVE).clone()
        g.close()
    h, t = outs["hip"], outs["torch"]
    for k in ("obs", "actions", "running", "rewards", "f32_step", "rtg", "alive"):
        assert torch.equal(h[k], t[k]), k
    assert not h["running"].all()  # episodes ended inside the rollout: masking exercised
    # the alive masking at n > 4: a blue ship sunk while its env was still running
    sunk = (h["actions"] == 0).all(3) & h["running"][:, :, None]
    print(f"{name}: blue ships sunk at the end {int((h['alive'][:nb] == 0).sum())}, "
          f"masked (env, step, ship) rows of running envs {int(sunk.sum())}")
    assert (h["alive"][:nb] == 0).any() and sunk.any()
    print(f"{name}: hip against torch: log-probabilities {O.max_abs(h['log_probs'], t['log_probs']):.3e}, "
          f"values {O.max_abs(h['values'], t['values']):.3e}")
    torch.testing.assert_close(h["log_probs"], t["log_probs"], rtol=0, atol=1e-4)
    torch.testing.assert_close(h["values"], t["values"], rtol=0, atol=1e-5)
    # keyed sampling, one step from the same state
    samp = {}
    for impl in ("hip", "torch"):
        g = game()
        r = Rollout(g, actor, None, steps=1, red=red, red_actor=red_actor, impl=impl, keyed_seed=21, noise=0.05)
        samp[impl] = {k: v.clone() for k, v in r.run().items()}
        g.close()
    print(f"{name}: keyed step, hip against torch: actions "
          f"{O.max_abs(samp['hip']['actions'], samp['torch']['actions']):.3e}, log-probabilities "
          f"{O.max_abs(samp['hip']['log_probs'], samp['torch']['log_probs']):.3e}")
    torch.testing.assert_close(samp["hip"]["actions"], samp["torch"]["actions"], rtol=0, atol=1e-5)
    torch.testing.assert_close(samp["hip"]["log_probs"], samp["torch"]["log_probs"], rtol=0, atol=1e-3)
