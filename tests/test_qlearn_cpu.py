"""The DDQN learner step without a GPU: QLearner(impl="torch") on the host
against what the reference's own DDQN.optimize() left behind
(tests/golden/make_qlearn_golden.py), and the argument checks of lnw_qnet_grad /
lnw_qnet_adam."""
import ctypes

import numpy as np
import pytest
import torch

from _qlearn_util import (GRAD_NAMES, NOISE, RUNNING, SETS, U, assert_grads_within, err, bound, gold, load_set,
                          oracle64, ref_grad_flat, segs)
from lnw import _abi
from lnw.build import build
from lnw.qlearn import PACKED_NAMES, BatchedQNet, QLearner


def learner(prefix, policy_bn, **kw):
    g = gold()
    pol, tgt, batch = load_set(prefix)
    return QLearner(pol, tgt, lr=float(g[f"{prefix}_lr"]), gamma=float(g[f"{prefix}_gamma"]), policy_bn=policy_bn,
                    impl="torch", device="cpu", **kw), batch


@pytest.mark.parametrize("prefix,policy_bn", SETS)
def test_torch_arm_reproduces_reference_gradients(prefix, policy_bn):
    """Loss, y, qs and every gradient tensor of the reference's optimize(): the
    gradients under the bound of the GPU tests (8 x the reference's own error
    against float64 autograd, floored at one ulp), the rest to the same rule."""
    g = gold()
    L, batch = learner(prefix, policy_bn)
    theta0, target0 = L.theta.clone(), L.theta_target.clone()
    out = L.grad(batch)
    o64 = oracle64(theta0, target0, batch, float(g[f"{prefix}_gamma"]), policy_bn)
    assert out["loss"].dim() == 0
    for name, got, ref in (("loss", out["loss"], g[f"{prefix}_loss"]), ("y", out["y"], g[f"{prefix}_y"]),
                           ("qs", out["qs"], g[f"{prefix}_qs"])):
        e, er = err(got, o64[name]), err(ref, o64[name])
        assert e <= bound(er), (name, e, er)
    assert_grads_within(out["grad"], ref_grad_flat(prefix, L.n_in), o64, L.n_in, policy_bn, prefix)
    # the running-statistics slots of the gradient vector are zero
    for n, v in segs(out["grad"], L.n_in, RUNNING).items():
        assert (v == 0).all(), n


@pytest.mark.parametrize("prefix,policy_bn", SETS)
def test_torch_arm_reproduces_reference_step(prefix, policy_bn):
    """One .step(): the running statistics and num_batches_tracked of both
    networks ("unchanged" for red's policy), and the post-step parameters.
    A parameter may differ from the reference's by what Adam's first step makes
    of the (separately bounded) gradient difference, lr * |u(g) - u(g_ref)| with
    u(g) = g / (|g| + eps), plus 2 ulp. conv1.bias and conv2.bias under batch
    statistics are compared on the gradient only: their gradient is rounding
    noise, which Adam turns into a +-lr step."""
    g = gold()
    L, batch = learner(prefix, policy_bn)
    lr = float(g[f"{prefix}_lr"])
    grad = L.grad(batch, update_running=False)["grad"]
    loss = L.step(batch)
    assert loss.dim() == 0 and abs(float(loss) - float(g[f"{prefix}_loss"])) <= 1e-5 * float(g[f"{prefix}_loss"])
    pol, tgt = BatchedQNet.for_obs(L.D), BatchedQNet.for_obs(L.D)
    L.policy, L.target = pol, tgt
    L.export()
    gsegs, rsegs = segs(grad, L.n_in), segs(ref_grad_flat(prefix, L.n_in), L.n_in)
    for net, which in ((pol, "policy"), (tgt, "target")):
        sd = net.state_dict()
        for k in sd:
            ref, ref0 = g[f"{prefix}.{which}.after.{k}"], g[f"{prefix}.{which}.before.{k}"]
            got = sd[k].numpy()
            if "num_batches_tracked" in k:
                assert int(got) == int(ref), (which, k)
            elif k in RUNNING:
                if which == "policy" and policy_bn == "running":
                    assert np.array_equal(got, ref0) and np.array_equal(ref, ref0), (which, k)
                else:
                    assert not np.array_equal(ref, ref0)
                    np.testing.assert_allclose(got, ref, rtol=2e-6, atol=1e-7, err_msg=f"{which} {k}")
            elif which == "target":
                assert np.array_equal(got, ref) and np.array_equal(ref, ref0), (which, k)
            elif policy_bn == "batch" and k in NOISE:
                continue
            else:
                u = lambda x: x / (x.abs() + 1e-8)  # noqa: E731
                tol = lr * (u(gsegs[k]) - u(rsegs[k])).abs().numpy().reshape(ref.shape) * 1.001 + 2 * np.spacing(np.abs(ref))
                assert (np.abs(got - ref) <= tol).all(), (which, k, np.abs(got - ref).max())
                assert not np.array_equal(ref, ref0), k


def test_unpack_is_the_inverse_of_packed():
    pol, _, _ = load_set("wide")
    flat = pol.packed()
    other = BatchedQNet.for_obs(pol.obs_dim).unpack_(flat)
    assert torch.equal(other.packed(), flat)
    for k, v in pol.state_dict().items():
        if "num_batches_tracked" not in k:
            assert torch.equal(other.state_dict()[k], v), k
    with pytest.raises(ValueError):
        other.unpack_(flat[:-1])
    assert tuple(PACKED_NAMES[:2]) == ("conv1.weight", "conv1.bias") and len(GRAD_NAMES) == 16


def test_sync_target_copies_everything():
    L, batch = learner("blue", "batch")
    L.step(batch)
    assert not torch.equal(L.params, L.target_params)
    L.sync_target()
    assert torch.equal(L.params, L.target_params) and int(L.nbt[0]) == int(L.nbt[1]) == 1


def test_batch_of_collector_shape_is_flattened():
    """[B, n, ...] batches (QCollector.sample) become rows, done repeated per ship."""
    L, batch = learner("blue", "batch")
    b3 = dict(state=batch["state"].reshape(16, 4, -1), next_state=batch["next_state"].reshape(16, 4, -1),
              action=torch.cat([batch["action"], torch.zeros(64, 1, dtype=torch.long)], 1).reshape(16, 4, 4),
              reward=batch["reward"].reshape(16, 4), done=torch.ones(16, dtype=torch.int32))
    flat = dict(batch, done=torch.ones(64, dtype=torch.int32))
    a = L.grad(b3, update_running=False)
    b = L.grad(flat, update_running=False)
    assert torch.equal(a["grad"], b["grad"]) and torch.equal(a["y"], b["y"])


# ---- the C ABI's argument checks (no GPU: every call fails before a device call) ----
@pytest.fixture(scope="module")
def lib():
    build()
    return _abi.load()


def _valid_args(lib, keep, D=68, rows=4):
    buf = (ctypes.c_float * 4096)()
    keep.append(buf)
    p = (ctypes.addressof(buf) + 15) & ~15
    a = _abi.QlearnArgs()
    for f in ("state", "next_state", "action", "reward", "done", "policy_params", "target_params", "grad", "loss",
              "workspace"):
        setattr(a, f, p)
    a.rows, a.D, a.action_stride, a.gamma = rows, D, 4, 0.99
    a.workspace_bytes = max(lib.lnw_qlearn_workspace_bytes(rows, D), 0)
    return a


def test_workspace_bytes(lib):
    assert lib.lnw_qlearn_workspace_bytes(64, 68) > 0
    assert lib.lnw_qlearn_workspace_bytes(131072, 68) > lib.lnw_qlearn_workspace_bytes(64, 68)
    assert lib.lnw_qlearn_workspace_bytes(64, 84) > lib.lnw_qlearn_workspace_bytes(64, 68)
    for rows, D in ((0, 68), (64, 48), (64, 70), (64, 49 + 56), (1 << 31, 68)):
        assert lib.lnw_qlearn_workspace_bytes(rows, D) == 0, (rows, D)


def test_qnet_grad_validates_arguments(lib):
    keep = []
    assert lib.lnw_qnet_grad(None, None) == -1
    assert lib.lnw_qnet_grad(ctypes.byref(_abi.QlearnArgs()), None) == -1
    for f in ("state", "next_state", "action", "reward", "done", "policy_params", "target_params", "grad", "loss",
              "workspace"):
        a = _valid_args(lib, keep)
        setattr(a, f, None)
        assert lib.lnw_qnet_grad(ctypes.byref(a), None) == -1, f
    for f in ("state", "next_state"):
        a = _valid_args(lib, keep)
        setattr(a, f, getattr(a, f) + 4)  # misaligned rows
        assert lib.lnw_qnet_grad(ctypes.byref(a), None) == -1, f
    a = _valid_args(lib, keep)
    a.D = 70          # D % 4 != 0
    assert lib.lnw_qnet_grad(ctypes.byref(a), None) == -5
    a = _valid_args(lib, keep)
    a.D = 48          # shorter than the 7x7 window
    assert lib.lnw_qnet_grad(ctypes.byref(a), None) == -5
    a = _valid_args(lib, keep)
    a.D = 49 + 56     # n_in = 68 > 64
    assert lib.lnw_qnet_grad(ctypes.byref(a), None) == -5
    a = _valid_args(lib, keep)
    a.rows = 0
    assert lib.lnw_qnet_grad(ctypes.byref(a), None) == -1
    a = _valid_args(lib, keep)
    a.action_stride = 2
    assert lib.lnw_qnet_grad(ctypes.byref(a), None) == -1
    a = _valid_args(lib, keep)
    a.workspace_bytes -= 1
    assert lib.lnw_qnet_grad(ctypes.byref(a), None) == -1


def test_qnet_adam_validates_arguments(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ok = [p, p, p, p, 0, p, 1e-4, 0.9, 0.999, 1e-8, 1.0, None]
    assert lib.lnw_qnet_adam(*ok) == 0  # (count 0: nothing to do)
    for i in (0, 1, 2, 3, 5):
        bad = list(ok)
        bad[i] = None
        assert lib.lnw_qnet_adam(*bad) == -1, i
    for i, val in ((4, -1), (6, -1.0), (7, 1.0), (8, 1.5), (9, -1e-8)):
        bad = list(ok)
        bad[i] = val
        assert lib.lnw_qnet_adam(*bad) == -1, i


def test_struct_matches_header():
    """QlearnArgs mirrors lnw_qlearn_args field by field (natural alignment on
    both sides)."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lnw.h")).read()
    body = src[src.index("typedef struct lnw_qlearn_args {"):src.index("} lnw_qlearn_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"([^;{]+);", body) for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _abi.QlearnArgs._fields_]
    assert ctypes.sizeof(_abi.QlearnArgs) == 144
