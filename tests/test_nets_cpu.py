"""lnw.nets without a GPU: the module form and the flat-vector form of each
network are one function (bit for bit, in float32 and float64, at the narrow and
the wide head, on one to three rows, in every BatchNorm mode each form has), the
actor's and the Q-net's trunks are the same trunk, a seeded constructor draws
what the reference's layer list draws, the names that moved are still importable
from where they were, and an unknown BatchNorm mode is refused."""
import copy
import functools
from collections import OrderedDict
from operator import attrgetter

import pytest
import torch
import torch.nn as nn

from lnw import layout, nets, ppolearn, qlearn, rollout
from lnw.nets import BatchedActor, BatchedCritic, BatchedQNet

SHIPS = {56: 1, 68: 4, 100: 12}  # row length D: ships n (D = 52 + 4 n; 100: n_in = 63 > 32, the wide head)
CASES = [(D, B, dt) for D in SHIPS for B in (1, 2, 3) for dt in (torch.float32, torch.float64)]


@functools.lru_cache(maxsize=None)
def networks(D, dtype):
    """(actor, critic, Q-net) for rows of D floats in `dtype`, every BatchNorm
    affine parameter and running statistic drawn away from its default."""
    torch.manual_seed(D)
    actor, critic, q = BatchedActor.for_obs(D).to(dtype), BatchedCritic(SHIPS[D] * D).to(dtype), BatchedQNet.for_obs(D).to(dtype)
    with torch.no_grad():
        for net in (actor, q):
            for m in (net.norm1, net.norm2):
                m.weight.normal_(1.0, 0.3)
                m.bias.normal_(0.0, 0.3)
                m.running_mean.normal_(0.0, 0.3)
                m.running_var.uniform_(0.5, 2.0)
        actor.layernorm.weight.normal_(1.0, 0.3)
        actor.layernorm.bias.normal_(0.0, 0.3)
    return actor, critic, q


def flat(module, sl):
    """layout.pack() in the module's own dtype."""
    sd = module.state_dict()
    return torch.cat([sd[name].detach().reshape(-1) for name in sl])


def rows(B, D, dtype, seed=0):
    g = torch.Generator().manual_seed(1000 * D + 10 * B + seed)
    return torch.rand((B, D), generator=g, dtype=dtype), torch.rand((B, 4), generator=g, dtype=dtype)


@pytest.mark.parametrize("D,B,dtype", CASES)
def test_module_and_flat_vector_are_one_function(D, B, dtype):
    actor, critic, q = networks(D, dtype)
    obs, act = rows(B, D, dtype)
    sl = layout.packed_slices(q.n_in)
    theta = flat(q, sl)
    if dtype == torch.float32:
        assert torch.equal(theta, q.packed())
    for bn in ("batch", "running"):
        got, stats = nets.q_forward(theta, obs, bn, sl)
        assert got.dtype == dtype and stats.shape == (2, 13)
        assert torch.equal(q.q_torch(obs, bn), got), bn
    sl = layout.actor_slices(q.n_in)
    lp, ent, stats = nets.actor_forward(flat(actor, sl), obs, act, sl)
    want = actor.get_dist(obs, act, "sample")
    assert lp.dtype == dtype and stats.shape == (B, 26)
    assert torch.equal(want[0], lp) and torch.equal(want[1], ent)
    n = SHIPS[D]
    gs = rows(B, n * D, dtype, seed=1)[0]
    sl = layout.critic_slices(n, D)
    assert torch.equal(critic(gs.reshape(B, n, D))[:, 0], nets.critic_forward(flat(critic, sl), gs, sl))


@pytest.mark.parametrize("D,B,dtype", CASES)
def test_actor_and_qnet_share_the_trunk(D, B, dtype):
    actor, _, q = networks(D, dtype)
    q = copy.deepcopy(q)
    q.load_state_dict({name: actor.state_dict()[name] for name, _ in layout.CONV_HEAD}, strict=False)
    obs = rows(B, D, dtype)[0]
    for bn in ("sample", "running"):
        a = nets.trunk(lambda name: attrgetter(name)(actor), obs, bn)[0]
        b = nets.trunk(lambda name: attrgetter(name)(q), obs, bn)[0]
        assert a.shape == (B, q.n_in) and torch.equal(a[:, :12], b[:, :12]), bn
        assert torch.equal(a[:, 12:], obs[:, 49:])
        # and the modules' own paths run that trunk
        assert torch.equal(q.q_torch(obs, bn), nets.q_heads(lambda name: attrgetter(name)(q), b))
        ln = actor.layernorm
        assert torch.equal(actor.features(obs, bn), nn.functional.layer_norm(a, (q.n_in,), ln.weight, ln.bias, ln.eps))


def restated(kind, D):
    """The state_dict a seeded constructor must give, from plain nn layers in
    network.py's order: the trunk (conv1, norm1, conv2, norm2, convhead; the
    pools draw nothing), the network's own layers, then its xavier passes."""
    L, n_in = nn.Linear, D - 49 + 12
    if kind == "critic":
        layers = [("fc1", L(SHIPS[D] * D, 32)), ("fc2", L(32, 64)), ("fc3", L(64, 64)), ("fc4", L(64, 1))]
        xavier = ("fc1", "fc2", "fc3", "fc4")
    else:
        layers = [("conv1", nn.Conv2d(1, 5, 3, 1, padding=1)), ("norm1", nn.BatchNorm2d(5)),
                  ("conv2", nn.Conv2d(5, 8, 3, 1, padding=1)), ("norm2", nn.BatchNorm2d(8)), ("convhead", L(8, 12))]
        if kind == "actor":
            layers += [("layernorm", nn.LayerNorm(n_in)), ("fc1", L(n_in, 64)), ("fc2", L(64, 64)), ("fc3", L(64, 32)),
                       ("normal_head", L(32, 4, bias=False)), ("log_std_head", L(32, 4, bias=False))]
            xavier = ("fc1", "fc2", "fc3", "normal_head", "log_std_head")
        else:
            layers += [("movement", L(n_in, 50)), ("attack", L(n_in, 5)), ("radar", L(n_in, 2))]
            xavier = ("convhead", "movement", "attack", "radar")
    net = nn.Sequential(OrderedDict(layers))
    for name in xavier:
        nn.init.xavier_uniform_(getattr(net, name).weight)
    own = [("logstd", torch.zeros(()))] if kind == "actor" else []  # (a module's own parameters come first)
    return OrderedDict(own + list(net.state_dict().items()))


@pytest.mark.parametrize("D", list(SHIPS))
@pytest.mark.parametrize("kind", ["actor", "critic", "qnet"])
def test_seeded_constructor_draws_the_reference_layer_list(kind, D):
    make = dict(actor=lambda: BatchedActor.for_obs(D), critic=lambda: BatchedCritic(SHIPS[D] * D),
                qnet=lambda: BatchedQNet.for_obs(D))[kind]
    torch.manual_seed(11)
    got = make().state_dict()
    torch.manual_seed(11)
    want = restated(kind, D)
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


MOVED = {
    rollout: ("BatchedActor", "BatchedCritic", "NOISE_FREE", "flat_n_in", "noise_mask", "unpack_policy"),
    qlearn: ("BatchedQNet", "N_Q", "HEADS", "random_rows", "q_forward"),
    ppolearn: ("actor_forward", "critic_forward"),
}
STAYED = {
    rollout: ("Rollout", "perturbed_theta", "red_script_table", "red_script_actions", "reference_rtg",
              "discounted_rtg", "gae", "STRIDED_POLICY_INPUT", "DATA", "keyed_normal", "keyed_uniform"),
    qlearn: ("epsilon", "red_random_rows", "red_random_act", "QCollector", "QLearner", "keyed_uniform4",
             "packed_slices", "PACKED_NAMES", "CONV_PARAMS"),
    ppolearn: ("gae_rows", "popart", "losses", "running_after", "PPOLearner", "sample_keys", "actor_slices",
               "critic_slices", "flat_size", "pack", "RUNNING"),
}


def test_moved_names_are_importable_from_where_they_were():
    for old, names in MOVED.items():
        for name in names:
            assert getattr(old, name) is getattr(nets, name), (old.__name__, name)
    assert qlearn._flat_forward is nets.q_forward
    for mod, names in STAYED.items():
        for name in names:
            assert hasattr(mod, name), (mod.__name__, name)


def test_modules_deep_copy():
    actor, critic, q = networks(68, torch.float32)
    obs, act = rows(4, 68, torch.float32)
    for net, f in ((actor, lambda m: m.get_dist(obs, act)[0]), (critic, lambda m: m(obs.reshape(1, -1))),
                   (q, lambda m: m.q_torch(obs))):
        assert torch.equal(f(copy.deepcopy(net)), f(net))


def test_unknown_batchnorm_mode_is_refused():
    actor, _, q = networks(56, torch.float32)
    obs, act = rows(2, 56, torch.float32)
    msg = "bn must be 'sample', 'running' or 'batch'"
    for bn in ("batch", "x"):  # the actor has no "batch": lnw_actor_features cannot compute it
        for call in (lambda: actor.features(obs, bn), lambda: actor.heads(obs, bn), lambda: actor(obs, bn=bn),
                     lambda: actor.get_dist(obs, act, bn)):
            with pytest.raises(ValueError, match=msg):
                call()
    for call in (lambda: q.q_torch(obs, "x"), lambda: q.q(obs, "x"), lambda: q.td_target(obs, act[:, 0], act[:, 0], 0.9, "x"),
                 lambda: nets.q_forward(q.packed(), obs, "x", layout.packed_slices(q.n_in))):
        with pytest.raises(ValueError, match=msg):
            call()
