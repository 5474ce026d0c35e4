"""lnw_qnet_act and lnw.qlearn on the GPU: the fused DDQN acting kernel against
the reference's recorded DMLP outputs (tests/golden/qnet.npz), against its own
Q-values, against the torch restatement of its keyed random branches, and the
on-device transition collector replayed on a second game."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qnet.npz")
HEADS = ((0, 2), (2, 7), (7, 57))
SENTINEL = -7


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def load_net(gold, prefix):
    from lnw.qlearn import BatchedQNet
    D = gold[f"{prefix}_obs"].shape[1]
    sd = {k[len(prefix) + 1:]: gold[k] for k in gold.files if k.startswith(prefix + ".")}
    return BatchedQNet.for_obs(D).load_reference(sd).cuda()


def random_net(D, seed):
    from lnw.qlearn import BatchedQNet
    torch.manual_seed(seed)
    net = BatchedQNet.for_obs(D)
    with torch.no_grad():
        for m in (net.norm1, net.norm2):
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 2.0)
    return net.cuda()


def random_obs(E, n, D, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand((E, n, D), generator=g)
    obs[..., :49] = torch.randint(0, 256, (E, n, 49), generator=g) / 255.0
    return obs.cuda()


def call(net, obs, own0=0, A=None, alive=None, live=None, eps=0.0, eps_env=None, seed=5, slot=3,
         row_base=0, bn="sample", obs_stride=0, mode=0, t=0, ra=0.4, tl_cnt=None, act_stride=None,
         want_q=True, shape=None):
    """One raw lnw_qnet_act call. obs [E, n, D] (or a strided buffer with
    `shape`); alive / tl_cnt [A, E]. Returns full [E, A, 4] (pre-filled with
    SENTINEL), act [E, act_stride] (ditto), q [E*n, 57], explored [E*n]."""
    from lnw import _abi
    L = _abi.load()
    E, n, D = shape or obs.shape
    A = A or own0 + n
    a = _abi.QnetArgs()
    if obs is not None:
        a.obs = obs.data_ptr()
    a.E, a.n, a.D, a.own0, a.A, a.obs_in_env_stride = E, n, D, own0, A, obs_stride
    params = net.packed() if net is not None else None
    if params is not None:
        a.params = params.data_ptr()
    a.bn_running, a.mode, a.eps = int(bn == "running"), mode, float(eps)
    if eps_env is not None:
        a.eps_env = eps_env.data_ptr()
    a.seed, a.slot, a.row_base, a.t, a.red_aggression = seed, slot, row_base, t, ra
    alive = torch.ones((A, E), dtype=torch.uint8, device="cuda") if alive is None else alive
    a.alive = alive.data_ptr()
    if tl_cnt is not None:
        a.tl_cnt = tl_cnt.data_ptr()
    if live is not None:
        a.live = live.data_ptr()
    act_stride = act_stride or 4 * n
    out = dict(full=torch.full((E, A, 4), SENTINEL, dtype=torch.int32, device="cuda"),
               act=torch.full((E, act_stride), SENTINEL, dtype=torch.int32, device="cuda"),
               explored=torch.full((E * n,), 9, dtype=torch.uint8, device="cuda"))
    a.full, a.act_out, a.act_env_stride = out["full"].data_ptr(), out["act"].data_ptr(), act_stride
    a.explored = out["explored"].data_ptr()
    if want_q and mode == 0:
        out["q"] = torch.full((E * n, 57), float("nan"), device="cuda")
        a.q_out = out["q"].data_ptr()
    rc = L.lnw_qnet_act(C.byref(a), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def first_argmax(q):
    """[B, 3]: first maximal index per head (numpy argmax returns the first)."""
    q = q.cpu().numpy()
    return np.stack([q[:, lo:hi].argmax(1) for lo, hi in HEADS], 1)


# ---------------------------------------------------------------- reference parity
@pytest.mark.parametrize("prefix,n", [("net", 4), ("dead", 4), ("wide", 8)])
@pytest.mark.parametrize("mode,bn", [("tr", "sample"), ("ev", "running")])
def test_kernel_matches_reference(gold, prefix, n, mode, bn):
    net = load_net(gold, prefix)
    obs = torch.from_numpy(gold[f"{prefix}_obs"]).cuda()
    B, D = obs.shape
    out = call(net, obs.reshape(B // n, n, D).contiguous(), bn=bn)
    ref_q, ref_arg, tie = (gold[f"{prefix}_{mode}_{k}"] for k in ("q", "arg", "tie"))
    q = out["q"].cpu().numpy()
    err = np.abs(q - ref_q)
    print(f"{prefix} {mode}: max |q - ref| = {err.max():.3e}, max rel = "
          f"{(err / np.maximum(np.abs(ref_q), 1e-6)).max():.3e}")
    np.testing.assert_allclose(q, ref_q, rtol=1e-4, atol=2e-5)
    act = out["full"].cpu().numpy().reshape(B, 4)
    assert (act[:, 3] == 0).all()
    assert np.array_equal(act[:, :3][~tie], ref_arg[~tie])
    # inside the near-tie mask: an index whose reference Q is within 1e-3 of the maximum
    for r, h in zip(*np.nonzero(tie)):
        lo, hi = HEADS[h]
        assert ref_q[r, lo + act[r, h]] >= ref_q[r, lo:hi].max() - 1e-3, (r, h)
    if prefix == "dead":
        assert (q[:, :7] == 0).all() and (act[:, :2] == 0).all()
    # lnw.qlearn's device path is this kernel
    assert torch.equal(net.q(obs, bn=bn), out["q"])


# ---------------------------------------------------------------- self-consistency
# ragged wave; blocks + tail; NI = 64; then the 64-wide path's edges: n_in = 35 (the smallest
# width on it) and n_in = 63 (the largest accepted)
SHAPES = [(37, 3, 64), (300, 4, 68), (5, 8, 84), (70, 5, 72), (9, 12, 100)]


@pytest.mark.parametrize("E,n,D", SHAPES)
@pytest.mark.parametrize("bn", ["sample", "running"])
def test_actions_are_first_argmax_of_own_q(E, n, D, bn):
    net, obs = random_net(D, 1), random_obs(E, n, D, 2)
    a, b = call(net, obs, bn=bn), call(net, obs, bn=bn)
    assert torch.isfinite(a["q"]).all() and (a["q"] >= 0).all()
    assert torch.equal(a["q"].view(torch.int32), b["q"].view(torch.int32))
    act = a["full"].cpu().numpy().reshape(E * n, 4)
    assert np.array_equal(act[:, :3], first_argmax(a["q"])) and (act[:, 3] == 0).all()
    assert torch.equal(a["full"], b["full"]) and not a["explored"].any()
    with torch.no_grad():  # and the torch path agrees on the values
        want = net.q_torch(obs.reshape(E * n, D), bn)
    np.testing.assert_allclose(a["q"].cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=2e-5)


def test_nonfinite_parameters_follow_torch():
    """relu keeps a NaN and argmax ranks it above every number (the first one
    wins), as BatchedQNet's torch path on the CPU does."""
    net, obs = random_net(68, 3), random_obs(9, 4, 68, 4)
    with torch.no_grad():
        net.attack.bias[3] = float("nan")
        net.movement.bias[[10, 20]] = float("nan")
        net.radar.bias[1] = float("inf")
    out = call(net, obs)
    with torch.no_grad():
        want = net.cpu().q_torch(obs.cpu().reshape(36, 68), "sample")
    arg = torch.stack([want[:, lo:hi].argmax(1) for lo, hi in HEADS], 1).numpy()
    act = out["full"].cpu().numpy().reshape(36, 4)
    assert np.array_equal(act[:, :3], arg)
    assert (act[:, :3] == [1, 3, 10]).all()
    assert torch.equal(torch.isnan(out["q"]).cpu(), torch.isnan(want))


# ---------------------------------------------------------------- epsilon-greedy
def masks(E, n, seed):
    g = torch.Generator().manual_seed(seed)
    alive = (torch.rand((E, n), generator=g) > 0.2)
    live = (torch.rand((E,), generator=g) > 0.15)
    return alive.cuda(), live.cuda()


def in_range(act):
    a = act.reshape(-1, 4)
    return bool((a >= 0).all() and (a[:, 0] < 2).all() and (a[:, 1] < 5).all() and (a[:, 2] < 50).all()
                and (a[:, 3] == 0).all())


@pytest.mark.parametrize("E,n,D", SHAPES)
def test_epsilon_one_equals_restatement(E, n, D):
    net, obs = random_net(D, 5), random_obs(E, n, D, 6)
    alive, live = masks(E, n, 7)
    kw = dict(eps=1.0, alive=alive, live=live, seed=11, slot=6, row_base=40)
    hip, ref = net.act(obs, impl="hip", **kw), net.act(obs, impl="torch", **kw)
    assert torch.equal(hip["actions"], ref["actions"]) and torch.equal(hip["explored"], ref["explored"])
    keep = alive & live[:, None]
    assert torch.equal(hip["explored"], keep) and in_range(hip["actions"])
    assert not hip["actions"][~keep].any()
    # every value of every column turns up (300 x 4 rows draw 0..49 many times over)
    if E * n >= 1000:
        a = hip["actions"][keep]
        assert a[:, 0].unique().numel() == 2 and a[:, 1].unique().numel() == 5 and a[:, 2].unique().numel() == 50


@pytest.mark.parametrize("per_env", [False, True])
def test_epsilon_half_mixes_branches(per_env):
    from lnw.qlearn import keyed_uniform4
    E, n, D = 300, 4, 68
    net, obs = random_net(D, 8), random_obs(E, n, D, 9)
    alive, live = masks(E, n, 10)
    keep = alive & live[:, None]
    kw = dict(alive=alive, live=live, seed=21, slot=2, row_base=8)
    if per_env:
        eps = torch.tensor([0.0, 0.3, 0.5, 1.0], device="cuda")[torch.arange(E, device="cuda") % 4]
    else:
        eps = 0.5
    mix = net.act(obs, eps=eps, impl="hip", **kw)
    greedy = net.act(obs, eps=0.0, impl="hip", **kw)
    rand = net.act(obs, eps=1.0, impl="torch", **kw)
    u0 = keyed_uniform4(8, E * n, 21, 2, "cuda")[:, 0].reshape(E, n)
    thr = eps[:, None] if per_env else torch.tensor(0.5, device="cuda")
    want = (u0 < thr) & keep
    assert torch.equal(mix["explored"], want) and not greedy["explored"].any()
    assert 0.2 < want.float().mean().item() < 0.6
    assert torch.equal(mix["actions"][want], rand["actions"][want])
    assert torch.equal(mix["actions"][~want], greedy["actions"][~want])
    assert in_range(mix["actions"])
    if per_env:
        assert not mix["explored"][0::4].any() and torch.equal(mix["explored"][3::4], keep[3::4])


# ---------------------------------------------------------------- masks and layout
def test_masks_sentinels_and_strides():
    E, n, D, own0, A = 70, 4, 68, 4, 8
    net, obs = random_net(D, 12), random_obs(E, n, D, 13)
    g = torch.Generator().manual_seed(14)
    alive = (torch.rand((A, E), generator=g) > 0.25).to(torch.uint8).cuda()
    live = (torch.rand((E,), generator=g) > 0.2).to(torch.uint8).cuda()
    kw = dict(own0=own0, A=A, alive=alive, live=live, eps=0.5, seed=3, slot=9)
    base = call(net, obs, **kw)
    keep = (alive[own0:].t().bool() & live.bool()[:, None])
    assert keep.any() and (~keep).any()
    own = base["full"][:, own0:]
    assert not own[~keep].any() and in_range(own)
    assert (base["full"][:, :own0] == SENTINEL).all()          # the other side's rows untouched
    assert torch.equal(base["act"].reshape(E, n, 4), own)       # replay rows = step rows
    assert torch.equal(base["explored"].bool().reshape(E, n) & ~keep, torch.zeros_like(keep))
    # rows read through an env stride larger than n * D
    stride = n * D + 20
    buf = torch.full((E, stride), float("nan"), device="cuda")
    buf[:, :n * D] = obs.reshape(E, n * D)
    strided = call(net, buf, obs_stride=stride, shape=(E, n, D), **kw)
    for k in ("full", "act", "explored"):
        assert torch.equal(strided[k], base[k]), k
    assert torch.equal(strided["q"].view(torch.int32), base["q"].view(torch.int32))
    # replay rows written through an env stride
    wide = call(net, obs, act_stride=4 * n + 8, **kw)
    assert torch.equal(wide["act"][:, :4 * n].reshape(E, n, 4), own)
    assert (wide["act"][:, 4 * n:] == SENTINEL).all()
    assert torch.equal(wide["full"], base["full"])


def test_shard_invariance():
    E, n, D, lo, hi = 300, 4, 68, 100, 229
    net, obs = random_net(D, 15), random_obs(E, n, D, 16)
    alive, live = masks(E, n, 17)
    whole = net.act(obs, eps=0.5, alive=alive, live=live, seed=31, slot=4, row_base=1000 * n, want_q=True)
    part = net.act(obs[lo:hi].contiguous(), eps=0.5, alive=alive[lo:hi], live=live[lo:hi], seed=31, slot=4,
                   row_base=(1000 + lo) * n, want_q=True)
    assert torch.equal(part["actions"], whole["actions"][lo:hi])
    assert torch.equal(part["explored"], whole["explored"][lo:hi])
    assert torch.equal(part["q"].view(torch.int32), whole["q"][lo * n:hi * n].view(torch.int32))


# ---------------------------------------------------------------- untrained red
@pytest.mark.parametrize("t", [5, 25])
def test_red_random_equals_restatement(t):
    from lnw import _abi
    from lnw.qlearn import keyed_uniform4, red_random_rows
    E, n, own0, A = 300, 4, 4, 8
    g = torch.Generator().manual_seed(18)
    alive = (torch.rand((A, E), generator=g) > 0.2).to(torch.uint8).cuda()
    tl = (torch.randint(0, 4, (A, E), generator=g) * (torch.rand((A, E), generator=g) > 0.4)).to(torch.int16).cuda()
    out = call(None, None, own0=own0, A=A, alive=alive, seed=77, slot=13, row_base=4 * 50, t=t, ra=0.4,
               tl_cnt=tl, mode=_abi.LNW_QNET_RED_RANDOM, shape=(E, n, 68))
    u = keyed_uniform4(4 * 50, E * n, 77, 13, "cuda")
    tl_rows = tl[own0:].t().reshape(-1)
    want = red_random_rows(u, t, 0.4, tl_rows).reshape(E, n, 3)
    keep = alive[own0:].t().bool()
    want = torch.where(keep[:, :, None], want, torch.zeros_like(want))
    own = out["full"][:, own0:]
    assert torch.equal(own[:, :, :3], want) and not own[:, :, 3].any()
    assert (out["full"][:, :own0] == SENTINEL).all()
    assert torch.equal(out["act"].reshape(E, n, 4), own)
    a = own[keep]
    if t < 20:
        assert a[:, 1].max() == 1 and a[:, 2].min() == 2 and a[:, 2].max() == 4
    else:
        fired = a[:, 1] > 0
        assert fired.any() and (~fired).any() and a[:, 1].max() == 4 and a[:, 2].max() == 49
        assert not (own[:, :, 1].bool() & (tl[own0:].t() == 0)).any()  # no targets, no salvo


# ---------------------------------------------------------------- collector
def melee_game(E, seed):
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    sc = Scenario(discrete=True, landing_ops=False, trained_red=False, auto_reset=False)
    g = BatchedGame(E, ["small"] * 4, ["large"] * 4, scenario=sc, seed=seed)
    g.reset(positions=[(6, 61), (10, 81), (8, 70), (11, 58), (98, 48), (98, 52), (98, 56), (96, 52)],
            box=((40, 40), (57, 65)))
    return g


def test_collector_ring_replays():
    """The ring's state rows are what observe returned, and stepping a second
    game of the same seed with the recorded actions (red's rows from the torch
    restatement of its keyed draws) reproduces reward, next_state and done."""
    from lnw import _abi
    from lnw.qlearn import QCollector, keyed_uniform4, red_random_rows
    E, cap, seed = 64, 12, 5
    net = random_net(68, 19)
    g1, g2, g3 = melee_game(E, 9), melee_game(E, 9), melee_game(E, 9)
    c1, c3 = QCollector(g1, net, red="random", capacity=cap, seed=seed), \
        QCollector(g3, net, red="random", capacity=cap, seed=seed)
    for k in range(cap):
        assert c1.step(eps=0.3) == k and c3.step(eps=0.3) == k
    assert c1.filled == cap
    for name in ("state", "action", "reward", "next_state", "done"):
        assert torch.equal(getattr(c1, name), getattr(c3, name)), name  # equal seeds, equal rings
    assert in_range(c1.action) and c1.action[..., 2].unique().numel() > 10
    for k in range(cap):
        ob, _ = g2.observe(-1)
        assert torch.equal(ob, c1.state[k]), k
        alive = g2.get(_abi.F_ALIVE).t().bool()                # [E, A]
        assert not c1.action[k][~alive[:, :4]].any()
        full = torch.zeros((E, 8, 4), dtype=torch.int32, device="cuda")
        full[:, :4] = c1.action[k]
        u = keyed_uniform4(0, E * 4, seed, 2 * k + 1, "cuda")
        tl = g2.get(_abi.F_TL_CNT)[4:].t().reshape(-1)
        red = red_random_rows(u, k, g2.sc.red_aggression, tl).reshape(E, 4, 3)
        full[:, 4:, :3] = torch.where(alive[:, 4:, None], red, torch.zeros_like(red))
        o = g2.step(full)
        assert torch.equal(o["rew_blue"], c1.reward[k]), k
        assert torch.equal(o["obs_blue"], c1.next_state[k]), k
        assert torch.equal(o["done"], c1.done[k]), k
    # the melee spawns are in contact: rewards differ between envs
    assert c1.reward.unique().numel() > 2
    s = c1.sample(50, generator=torch.Generator(device="cuda").manual_seed(1))
    idx = s["index"]
    assert idx.shape == (50,) and int(idx.max()) < cap * E
    kk, ee = idx // E, idx % E
    for name in ("state", "action", "reward", "next_state", "done"):
        assert torch.equal(s[name], getattr(c1, name)[kk, ee]), name
    # the ring wraps: step cap overwrites slot 0
    before = c1.state[0].clone()
    assert c1.step(eps=0.3) == 0 and c1.filled == cap and not torch.equal(c1.state[0], before)
    for g in (g1, g2, g3):
        g.close()


def test_collector_trained_red_and_requirements():
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    from lnw.qlearn import QCollector
    E = 64
    blue, red = random_net(68, 20), random_net(68, 21)
    g = melee_game(E, 4)
    c = QCollector(g, blue, red=red, capacity=4, seed=2)
    for _ in range(3):
        c.step(eps=torch.full((E,), 0.25, device="cuda"))
    assert in_range(c.action[:3])
    # red acts greedily on its own rows (left in the game's buffer by the observe)
    greedy = red.act(g.obs_red, eps=0.0)["actions"]
    assert greedy.shape == (E, 4, 4)
    g.close()
    cont = BatchedGame(8, ["small"] * 4, ["large"] * 4, scenario=Scenario(landing_ops=False), seed=1)
    with pytest.raises(ValueError):
        QCollector(cont, blue)
    cont.close()


def test_collector_red_side_replays():
    """side="red" (ddqn.py:343-384): both networks act epsilon-greedily on their
    own rows and red's transitions fill the ring; mirrored step by step on a
    second game through BatchedQNet.act."""
    from lnw import _abi
    from lnw.qlearn import QCollector
    E, seed, eps = 64, 3, 0.3
    blue, red = random_net(68, 22), random_net(68, 23)
    g1, g2 = melee_game(E, 6), melee_game(E, 6)
    c = QCollector(g1, blue, red=red, capacity=4, seed=seed, side="red")
    for k in range(4):
        c.step(eps=eps)
        ob, orr = g2.observe(-1)
        assert torch.equal(orr, c.state[k]), k
        alive = g2.get(_abi.F_ALIVE).t().bool()
        full = torch.zeros((E, 8, 4), dtype=torch.int32, device="cuda")
        full[:, :4] = blue.act(ob, eps=eps, alive=alive[:, :4], seed=seed, slot=2 * k)["actions"]
        full[:, 4:] = red.act(orr, eps=eps, alive=alive[:, 4:], seed=seed, slot=2 * k + 1)["actions"]
        assert torch.equal(full[:, 4:], c.action[k]), k
        o = g2.step(full)
        assert torch.equal(o["rew_red"], c.reward[k]) and torch.equal(o["obs_red"], c.next_state[k]), k
        assert torch.equal(o["done"], c.done[k]), k
    with pytest.raises(ValueError):
        QCollector(g1, blue, red="random", side="red")
    g1.close()
    g2.close()
