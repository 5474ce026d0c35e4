"""lnw.qlearn without a GPU: BatchedQNet's torch path against the reference's
recorded DMLP outputs (tests/golden/make_qnet_golden.py), its packed parameter
block, the epsilon schedule and lnw_qnet_act's argument checks."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from lnw import _abi
from lnw.build import build
from lnw.qlearn import CONV_PARAMS, HEADS, N_Q, BatchedQNet, epsilon

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qnet.npz")
SETS = ("net", "dead", "wide")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def load_net(gold, prefix):
    D = gold[f"{prefix}_obs"].shape[1]
    sd = {k[len(prefix) + 1:]: gold[k] for k in gold.files if k.startswith(prefix + ".")}
    return BatchedQNet.for_obs(D).load_reference(sd), sd


@pytest.mark.parametrize("prefix", SETS)
@pytest.mark.parametrize("mode,bn", [("tr", "sample"), ("ev", "running")])
def test_host_q_matches_reference(gold, prefix, mode, bn):
    """The reference's one-state-at-a-time outputs for every row at once: the
    Q-values to fp32 reordering (test_features_kernel_matches_torch's bound),
    the argmaxes exactly outside the recorded near-tie mask."""
    net, _ = load_net(gold, prefix)
    with torch.no_grad():
        q = net.q(torch.from_numpy(gold[f"{prefix}_obs"]), bn=bn)
    ref = gold[f"{prefix}_{mode}_q"]
    assert q.shape == ref.shape == (ref.shape[0], N_Q)
    np.testing.assert_allclose(q.numpy(), ref, rtol=1e-4, atol=2e-5)
    arg = np.stack([q[:, lo:hi].argmax(1).numpy() for lo, hi in HEADS], 1)
    clear = ~gold[f"{prefix}_{mode}_tie"]
    assert np.array_equal(arg[clear], gold[f"{prefix}_{mode}_arg"][clear])
    if prefix == "dead":  # radar and attack are all zero: the first index
        assert (q[:, :7] == 0).all() and (arg[:, :2] == 0).all()


def test_batch_mode_is_train_mode_batch_call(gold):
    """bn="batch" is what a train-mode module computes for the whole batch
    (optimize()'s calls, ddqn.py:175, 185), and it carries gradients."""
    net, _ = load_net(gold, "net")
    obs = torch.from_numpy(gold["net_obs"])
    q = net.q(obs, bn="batch")
    z = obs[:, :49].reshape(-1, 1, 7, 7)
    bn1 = torch.nn.BatchNorm2d(5)
    bn1.load_state_dict(net.norm1.state_dict())
    bn2 = torch.nn.BatchNorm2d(8)
    bn2.load_state_dict(net.norm2.state_dict())
    z = net.pool(torch.relu(bn1(net.conv1(z))))
    z = net.pool2(torch.relu(bn2(net.conv2(z))))
    x = torch.cat((net.convhead(torch.flatten(z, 1)), obs[:, 49:]), 1)
    ref = torch.cat((torch.relu(net.radar(x)), torch.relu(net.attack(x)), torch.relu(net.movement(x))), 1)
    torch.testing.assert_close(q, ref, rtol=1e-5, atol=1e-6)
    q.sum().backward()
    assert net.movement.weight.grad is not None and net.conv1.weight.grad is not None


@pytest.mark.parametrize("prefix", SETS)
def test_load_reference_round_trips_and_packed_layout(gold, prefix):
    net, sd = load_net(gold, prefix)
    back = net.state_dict()
    assert set(back) == set(sd)
    for k, v in sd.items():
        assert np.array_equal(back[k].numpy(), v.reshape(back[k].shape)), k
    n_in = gold[f"{prefix}_obs"].shape[1] - 37
    p = net.packed().numpy()
    assert p.dtype == np.float32 and p.shape == (CONV_PARAMS + N_Q * n_in + N_Q,)
    assert np.array_equal(p[:45], sd["conv1.weight"].reshape(-1))
    assert np.array_equal(p[470:566], sd["convhead.weight"].reshape(-1))
    w = p[CONV_PARAMS:CONV_PARAMS + N_Q * n_in].reshape(N_Q, n_in)
    assert np.array_equal(w[0:2], sd["radar.weight"])
    assert np.array_equal(w[2:7], sd["attack.weight"])
    assert np.array_equal(w[7:57], sd["movement.weight"])
    b = p[CONV_PARAMS + N_Q * n_in:]
    assert np.array_equal(b, np.concatenate([sd["radar.bias"], sd["attack.bias"], sd["movement.bias"]]))


def test_td_target_formula(gold):
    """ddqn.py:175-193: per-head max of the network on next_state, then
    gamma * max * done + reward."""
    net, _ = load_net(gold, "net")
    obs = torch.from_numpy(gold["net_obs"][:16])
    rew = torch.arange(16, dtype=torch.float32) - 5
    done = torch.tensor([1, 0] * 8, dtype=torch.int32)
    y = net.td_target(obs, rew, done, 0.9)
    with torch.no_grad():
        q = net.q(obs, bn="batch")
    mx = torch.stack([q[:, :2].max(1).values, q[:, 2:7].max(1).values, q[:, 7:].max(1).values], 1)
    torch.testing.assert_close(y, 0.9 * mx * done[:, None].float() + rew[:, None])
    assert y.shape == (16, 3) and torch.equal(y[1::2], rew[1::2, None].expand(8, 3))


def test_epsilon_is_get_epsilon():
    for t in (0, 1, 17, 400, 100000):
        for start, end, decay in ((1.0, 0.05, 200.0), (0.9, 0.1, 1000)):
            assert epsilon(t, start, end, decay) == end + (start - end) * math.exp(-1. * t / decay)
    assert epsilon(0, 0.9, 0.1, 1000) == 0.9


@pytest.fixture(scope="module")
def L():
    build()
    return _abi.load()


def _valid_args(keep):
    """QnetArgs that pass every check (E = 1 row; fake aligned pointers: the
    calls below must fail before any device call)."""
    buf = (ctypes.c_float * 1024)()
    keep.append(buf)
    p = (ctypes.addressof(buf) + 15) & ~15
    a = _abi.QnetArgs()
    a.obs, a.params, a.alive, a.full = p, p, p, p
    a.E, a.n, a.D, a.own0, a.A = 1, 4, 68, 0, 8
    return a


def test_qnet_act_validates_arguments(L):
    keep = []
    assert L.lnw_qnet_act(None, None) == -1
    assert L.lnw_qnet_act(ctypes.byref(_abi.QnetArgs()), None) == -1  # no obs / params / alive
    a = _valid_args(keep)
    a.D = 48          # shorter than the 7x7 window (a medium side)
    assert L.lnw_qnet_act(ctypes.byref(a), None) == -5
    a = _valid_args(keep)
    a.D = 49 + 56     # n_in = 68 > 64
    assert L.lnw_qnet_act(ctypes.byref(a), None) == -5
    a = _valid_args(keep)
    a.E = (1 << 31) // 4   # rows >= 2^31
    assert L.lnw_qnet_act(ctypes.byref(a), None) == -5
    a = _valid_args(keep)
    a.obs += 4        # misaligned rows
    assert L.lnw_qnet_act(ctypes.byref(a), None) == -1
    a = _valid_args(keep)
    a.own0 = 5        # own0 + n > A
    assert L.lnw_qnet_act(ctypes.byref(a), None) == -1
    a = _valid_args(keep)
    a.mode = 2
    assert L.lnw_qnet_act(ctypes.byref(a), None) == -1
    a = _valid_args(keep)
    a.mode = _abi.LNW_QNET_RED_RANDOM   # needs the target-list counts
    assert L.lnw_qnet_act(ctypes.byref(a), None) == -1
    a = _valid_args(keep)
    a.obs_in_env_stride = 4 * 68 - 4    # rows of consecutive envs would overlap
    assert L.lnw_qnet_act(ctypes.byref(a), None) == -1
    a = _valid_args(keep)
    a.E = 0
    assert L.lnw_qnet_act(ctypes.byref(a), None) == 0


def test_struct_matches_header_size(L):
    """QnetArgs mirrors lnw_qnet_args field by field (25 fields; the C side's
    layout is natural alignment, as ctypes')."""
    assert [f[0] for f in _abi.QnetArgs._fields_] == [
        "obs", "E", "n", "D", "own0", "A", "obs_in_env_stride", "params", "bn_running", "mode", "eps",
        "eps_env", "seed", "slot", "row_base", "t", "red_aggression", "tl_cnt", "alive", "live", "full",
        "act_out", "act_env_stride", "q_out", "explored"]
    assert ctypes.sizeof(_abi.QnetArgs) == 168
