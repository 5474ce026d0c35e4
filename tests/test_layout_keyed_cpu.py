"""lnw.layout and lnw.keyed without a GPU: the old import paths give the new
objects, the modules' imports form no cycle, the flat layouts equal tables
written out here, pack and unpack_ move every parameter and running statistic
bit for bit in the order written out here, and the host arm of the keyed draw
equals its definition with and without a payload."""
import ast
import glob
import os

import numpy as np
import pytest
import torch

from lnw import keyed, layout, ppodist, ppolearn, qlearn, replay, rollout
from lnw.layout import CONV_PARAMS, actor_slices, critic_slices, flat_size, pack, packed_slices, unpack_
from lnw.qlearn import BatchedQNet
from lnw.rollout import BatchedActor, BatchedCritic

LNW = os.path.dirname(os.path.abspath(layout.__file__))
OLD_PATHS = {
    rollout: dict(WINDOW=layout, keyed_normal=keyed, keyed_uniform=keyed),
    qlearn: dict(keyed_uniform4=keyed, packed_slices=layout, PACKED_NAMES=layout, CONV_PARAMS=layout),
    ppolearn: dict(sample_keys=keyed, _p_log=keyed, _philox10=keyed, actor_slices=layout, critic_slices=layout,
                   flat_size=layout, pack=layout, CONV_PARAMS=layout),
    replay: dict(draw=keyed, draw_buffers=keyed),
}


def test_old_paths_are_the_new_objects():
    for old, names in OLD_PATHS.items():
        for name, new in names.items():
            assert getattr(old, name) is getattr(new, name), (old.__name__, name)


def lnw_imports(path):
    """The lnw modules a source file imports, anywhere in it (functions too)."""
    found = set()
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.ImportFrom):
            mod = node.module or ""
            if node.level == 1:
                found |= {mod.split(".")[0]} if mod else {a.name for a in node.names}
            elif mod == "lnw":
                found |= {a.name for a in node.names}
            elif mod.startswith("lnw."):
                found.add(mod.split(".")[1])
            else:
                assert node.level == 0, (path, "an import from above the package")
        elif isinstance(node, ast.Import):
            found |= {a.name.split(".")[1] for a in node.names if a.name.startswith("lnw.")}
            assert not any(a.name == "lnw" for a in node.names), (path, "import lnw")
    return found


def test_import_graph_has_no_cycle():
    graph = {os.path.basename(p)[:-3]: lnw_imports(p) for p in glob.glob(os.path.join(LNW, "*.py"))}
    assert graph["layout"] == set()
    assert graph["keyed"] <= {"_abi", "layout"}
    assert graph["nets"] == {"_abi", "layout", "keyed"}
    ring = ("layout", "keyed", "nets", "rollout", "ppolearn", "qlearn", "ppodist", "replay")
    assert set(ring) <= set(graph)
    done, path = set(), []

    def visit(m):
        assert m not in path, "cycle: " + " -> ".join(path[path.index(m):] + [m])
        if m in done:
            return
        path.append(m)
        for d in sorted(graph[m] & set(ring)):
            visit(d)
        path.pop()
        done.add(m)

    for m in ring:
        visit(m)
    assert "ppolearn" not in graph["rollout"] and "rollout" not in graph["ppolearn"] | graph["qlearn"]
    assert "ppolearn" not in graph["replay"]


# ---- the layouts: {name: (offset, shape)}, written out -------------------------------
CONV_TABLE = {
    "conv1.weight": (0, (5, 1, 3, 3)), "conv1.bias": (45, (5,)), "norm1.weight": (50, (5,)), "norm1.bias": (55, (5,)),
    "norm1.running_mean": (60, (5,)), "norm1.running_var": (65, (5,)), "conv2.weight": (70, (8, 5, 3, 3)),
    "conv2.bias": (430, (8,)), "norm2.weight": (438, (8,)), "norm2.bias": (446, (8,)),
    "norm2.running_mean": (454, (8,)), "norm2.running_var": (462, (8,)), "convhead.weight": (470, (12, 8)),
    "convhead.bias": (566, (12,))}


def actor_table(n):
    return dict(CONV_TABLE, **{
        "layernorm.weight": (578, (n,)), "layernorm.bias": (578 + n, (n,)), "fc1.weight": (578 + 2 * n, (64, n)),
        "fc1.bias": (578 + 66 * n, (64,)), "fc2.weight": (642 + 66 * n, (64, 64)), "fc2.bias": (4738 + 66 * n, (64,)),
        "fc3.weight": (4802 + 66 * n, (32, 64)), "fc3.bias": (6850 + 66 * n, (32,)),
        "normal_head.weight": (6882 + 66 * n, (4, 32)), "log_std_head.weight": (7010 + 66 * n, (4, 32)),
        "logstd": (7138 + 66 * n, ())})


def critic_table(n, D):
    k = 32 * n * D
    return {"fc1.weight": (0, (32, n * D)), "fc1.bias": (k, (32,)), "fc2.weight": (k + 32, (64, 32)),
            "fc2.bias": (k + 2080, (64,)), "fc3.weight": (k + 2144, (64, 64)), "fc3.bias": (k + 6240, (64,)),
            "fc4.weight": (k + 6304, (1, 64)), "fc4.bias": (k + 6368, (1,))}


def packed_table(n):
    return dict(CONV_TABLE, **{
        "radar.weight": (578, (2, n)), "attack.weight": (578 + 2 * n, (5, n)), "movement.weight": (578 + 7 * n, (50, n)),
        "radar.bias": (578 + 57 * n, (2,)), "attack.bias": (580 + 57 * n, (5,)), "movement.bias": (585 + 57 * n, (50,))})


def same_table(got, want):
    return list(got.items()) == list(want.items())  # (names in order, offsets, shapes as tuples)


@pytest.mark.parametrize("n_in", [12, 63])
def test_actor_and_packed_tables(n_in):
    assert same_table(actor_slices(n_in), actor_table(n_in))
    assert same_table(packed_slices(n_in), packed_table(n_in))
    assert flat_size(actor_slices(n_in)) == 7139 + 66 * n_in and rollout.flat_n_in(7139 + 66 * n_in) == n_in
    assert flat_size(packed_slices(n_in)) == 635 + 57 * n_in
    assert CONV_PARAMS == 578 == actor_slices(n_in)["layernorm.weight"][0] == packed_slices(n_in)["radar.weight"][0]
    assert layout.ACTOR_NAMES == tuple(actor_table(n_in)) and layout.PACKED_NAMES == tuple(packed_table(n_in))


@pytest.mark.parametrize("n,D", [(1, 49), (4, 100)])
def test_critic_table(n, D):
    assert same_table(critic_slices(n, D), critic_table(n, D))
    assert flat_size(critic_slices(n, D)) == 32 * n * D + 6369
    assert layout.CRITIC_NAMES == tuple(critic_table(n, D))


# ---- pack / unpack_ ----------------------------------------------------------------------
def seeded(make, seed):
    """A network with seeded parameters, running statistics and batch counters."""
    torch.manual_seed(seed)
    net = make()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_()
                m.running_var.uniform_(0.5, 2.0)
                m.num_batches_tracked.fill_(seed + 3)
        if hasattr(net, "logstd"):
            net.logstd.fill_(0.25 * seed)
    return net


def conv_parts(m):
    return [m.conv1.weight, m.conv1.bias, m.norm1.weight, m.norm1.bias, m.norm1.running_mean, m.norm1.running_var,
            m.conv2.weight, m.conv2.bias, m.norm2.weight, m.norm2.bias, m.norm2.running_mean, m.norm2.running_var,
            m.convhead.weight, m.convhead.bias]


def qnet_parts(m):
    return conv_parts(m) + [m.radar.weight, m.attack.weight, m.movement.weight, m.radar.bias, m.attack.bias,
                            m.movement.bias]


def feature_parts(m):
    return conv_parts(m) + [m.layernorm.weight, m.layernorm.bias]


def actor_parts(m):
    return feature_parts(m) + [m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.fc3.weight, m.fc3.bias,
                               m.normal_head.weight, m.log_std_head.weight, m.logstd]


def critic_parts(m):
    return [m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.fc3.weight, m.fc3.bias, m.fc4.weight, m.fc4.bias]


def cat(parts):
    return torch.cat([p.detach().reshape(-1).float() for p in parts]).contiguous()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32),
                                                                                      b.view(torch.int32))


NETS = {
    "qnet": (lambda: BatchedQNet(100), qnet_parts, lambda m: packed_slices(m.n_in)),
    "actor": (lambda: BatchedActor.for_obs(100), actor_parts, lambda m: actor_slices(63)),
    "critic": (lambda: BatchedCritic(400), critic_parts, lambda m: critic_slices(4, 100)),
}


@pytest.mark.parametrize("name", list(NETS))
def test_pack_and_unpack_bit_for_bit(name):
    make, parts, slices = NETS[name]
    a, b = seeded(make, 1), seeded(make, 2)
    sl = slices(a)
    flat = pack(a, sl)
    assert same_bits(flat, cat(parts(a))) and flat.numel() == flat_size(sl)
    assert not same_bits(pack(b, sl), flat)
    counters = [int(m.num_batches_tracked) for m in b.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert unpack_(b, flat, sl) is b
    assert same_bits(pack(b, sl), flat) and same_bits(cat(parts(b)), flat)
    # the layouts hold no batch counter: unpack_ leaves it alone
    assert counters == [int(m.num_batches_tracked) for m in b.modules() if isinstance(m, torch.nn.BatchNorm2d)]


def test_qnet_and_actor_methods():
    q, q2, actor = seeded(NETS["qnet"][0], 1), seeded(NETS["qnet"][0], 2), seeded(NETS["actor"][0], 1)
    assert same_bits(q.packed(), cat(qnet_parts(q)))
    assert same_bits(actor.packed_features(), cat(feature_parts(actor)))
    assert actor.packed_features().numel() == 578 + 2 * 63
    assert q2.unpack_(q.packed()) is q2 and same_bits(q2.packed(), q.packed())
    with pytest.raises(ValueError):
        q2.unpack_(q.packed()[:-1])
    assert same_bits(q2.packed(), q.packed())


# ---- the draw's host arm -------------------------------------------------------------------
WEIGHTS = np.array([0.5, -2.0, np.nan, 0.0, 3.0, np.inf, 1.0, -0.25, 1.0], np.float32)
BASE, SEED, SLOT = 2 ** 33 + 1, 77, 4


def payload(n=3):
    g = torch.Generator().manual_seed(5)
    return dict(actions=torch.rand((9, 4), generator=g), log_probs=torch.randn((9, 4), generator=g),
                values=torch.randn(9 // n, generator=g), n=n)


@pytest.mark.parametrize("advance", [True, False])
@pytest.mark.parametrize("B", [1, 9])
def test_draw_host_arm(B, advance):
    key = keyed.sample_keys(WEIGHTS, SEED, SLOT, BASE)
    order = np.lexsort((np.arange(9), key))[:B]
    w = torch.from_numpy(WEIGHTS)
    results = []
    for pl in (None, payload()):
        counter, status = torch.tensor([SLOT]), torch.tensor([-5])
        b = keyed.draw(w, B, SEED, counter, status, row_base=BASE, advance=advance, impl="torch", payload=pl)
        assert b["index"].dtype == torch.int64 and np.array_equal(b["index"].numpy(), order)
        assert b["key"].dtype == torch.float64
        assert np.array_equal(b["key"].numpy().view(np.uint64), key[order].view(np.uint64))
        assert int(status) == 2 and int(counter) == SLOT + int(advance)
        results.append(b)
    plain, full = results
    assert set(plain) == {"index", "key"}
    assert set(full) == {"index", "key", "actions", "old_log_probs", "rtg", "old_values"}
    pl, idx = payload(), torch.from_numpy(order)
    assert torch.equal(full["actions"], pl["actions"][idx]) and torch.equal(full["old_log_probs"], pl["log_probs"][idx])
    assert torch.equal(full["old_values"], pl["values"][idx // 3])
    assert np.array_equal(full["rtg"].numpy().view(np.uint32), WEIGHTS[order].view(np.uint32))
    if B == 9:  # the rows that are not finite come last, in row order
        assert order[-2:].tolist() == [2, 5]


@pytest.mark.parametrize("B", [0, 10])
@pytest.mark.parametrize("with_payload", [False, True])
def test_draw_refuses_a_batch_out_of_range(B, with_payload):
    counter, status = torch.tensor([SLOT]), torch.tensor([-5])
    with pytest.raises(ValueError, match="batch must be in 1 .. min\\(rows, 131072\\)"):
        keyed.draw(torch.from_numpy(WEIGHTS), B, SEED, counter, status, row_base=BASE, impl="torch",
                   payload=payload() if with_payload else None)
    assert int(counter) == SLOT and int(status) == -5


def test_cached_makes_once_per_key():
    cache, made = {}, []
    make = lambda: made.append(1) or object()  # noqa: E731
    first = keyed.cached(cache, ("local", 4), make)
    assert keyed.cached(cache, ("local", 4), make) is first and len(made) == 1
    assert keyed.cached(None, ("local", 4), make) is not first and len(made) == 2
