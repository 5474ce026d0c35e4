"""Shared helpers of the DDQN learner tests (test_qlearn_cpu.py,
test_gpu_qlearn.py, and through _learner_cases.py test_learner_cases_cpu.py and
test_gpu_learner_hyper.py): the recorded sets of tests/golden/qlearn.npz, the float64
oracle, the error measure and bound of the gradient checks, generated networks
and transition rows, and lnw_qnet_adam alone."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from lnw.qlearn import HEADS, PACKED_NAMES, BatchedQNet, _flat_forward, packed_slices

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qlearn.npz")
SETS = (("blue", "batch"), ("red", "running"), ("wide", "batch"))
RUNNING = ("norm1.running_mean", "norm1.running_var", "norm2.running_mean", "norm2.running_var")
GRAD_NAMES = tuple(n for n in PACKED_NAMES if n not in RUNNING)
# under batch statistics these two have a mathematically zero gradient (the
# batch mean cancels the bias): their float32 value is rounding noise, measured
# against the conv's weight-gradient scale
NOISE = {"conv1.bias": "conv1.weight", "conv2.bias": "conv2.weight"}
U = 2.0 ** -23

_gold = None


def gold():
    global _gold
    if _gold is None:
        _gold = np.load(GOLD)
    return _gold


def load_set(prefix, when="before"):
    """(policy, target) BatchedQNets of a recorded set and its batch as row
    tensors (reward float64)."""
    g = gold()
    D = g[f"{prefix}_state"].shape[1]
    nets = []
    for n in ("policy", "target"):
        pre = f"{prefix}.{n}.{when}."
        nets.append(BatchedQNet.for_obs(D).load_reference({k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}))
    batch = dict(state=torch.from_numpy(g[f"{prefix}_state"]), next_state=torch.from_numpy(g[f"{prefix}_next_state"]),
                 action=torch.from_numpy(g[f"{prefix}_action"]), reward=torch.from_numpy(g[f"{prefix}_reward"]),
                 done=torch.from_numpy(g[f"{prefix}_done"]))
    return nets[0], nets[1], batch


def ref_grad_flat(prefix, n_in):
    """The reference's recorded gradients as a flat vector in packed() layout."""
    g = gold()
    sl = packed_slices(n_in)
    flat = np.zeros(max(k + int(np.prod(s)) for k, s in sl.values()), np.float32)
    for name in GRAD_NAMES:
        k, shp = sl[name]
        flat[k:k + int(np.prod(shp))] = g[f"{prefix}.grad.{name}"].reshape(-1)
    return torch.from_numpy(flat)


def segs(flat, n_in, names=GRAD_NAMES):
    sl = packed_slices(n_in)
    flat = flat.detach().cpu()
    return {n: flat[sl[n][0]:sl[n][0] + int(np.prod(sl[n][1]))] for n in names}


def oracle64(theta, theta_target, batch, gamma, policy_bn):
    """Float64 CPU autograd of the learner step's loss: dict(y, qs, stats, loss,
    grad), all float64."""
    n_in = batch["state"].shape[1] - 37
    sl = packed_slices(n_in)
    st, ns = batch["state"].detach().cpu().double(), batch["next_state"].detach().cpu().double()
    with torch.no_grad():
        qt, st_t = _flat_forward(theta_target.detach().cpu().double(), ns, "batch", sl)
        nxt = torch.stack([qt[:, lo:hi].max(1).values for lo, hi in HEADS], 1)
        y = gamma * nxt * batch["done"].cpu().double()[:, None] + batch["reward"].cpu().double()[:, None]
    th = theta.detach().cpu().double().clone().requires_grad_(True)
    q, st_p = _flat_forward(th, st, policy_bn, sl)
    act = batch["action"].cpu().long()
    qs = torch.stack([q[:, lo:hi].gather(1, act[:, h:h + 1])[:, 0] for h, (lo, hi) in enumerate(HEADS)], 1)
    loss = F.mse_loss(qs, y)
    loss.backward()
    return dict(y=y, qs=qs.detach(), stats=torch.stack([st_p, st_t]), loss=loss.detach(), grad=th.grad)


def err(got, g64, scale=None):
    """max |got - g64| / max |g64| (or / scale)."""
    got, g64 = torch.as_tensor(got).detach().cpu().double().reshape(-1), g64.reshape(-1)
    d = float(g64.abs().max()) if scale is None else scale
    return float((got - g64).abs().max()) / d if d > 0 else float((got - g64).abs().max())


def grad_errors(flat, o64, n_in, policy_bn):
    """{tensor name: err} of a flat gradient against the oracle's."""
    a, b = segs(flat, n_in), segs(o64["grad"], n_in)
    out = {}
    for n in GRAD_NAMES:
        scale = float(b[NOISE[n]].abs().max()) if (policy_bn == "batch" and n in NOISE) else None
        out[n] = err(a[n], b[n], scale)
    return out


def bound(e_ref):
    """The gradient bound: 8 x the reference float32 arm's own error against the
    float64 oracle, floored at one float32 ulp (the factor for the different
    summation order over B x 49 terms)."""
    return 8.0 * max(e_ref, U)


def assert_grads_within(flat, flat_ref, o64, n_in, policy_bn, what, report=None):
    e, er = grad_errors(flat, o64, n_in, policy_bn), grad_errors(flat_ref, o64, n_in, policy_bn)
    bad = []
    for n in GRAD_NAMES:
        if report is not None:
            report.append((what, n, e[n], er[n]))
        print(f"{what} {n}: err {e[n]:.3e} ref {er[n]:.3e} bound {bound(er[n]):.3e}")
        if not e[n] <= bound(er[n]):
            bad.append((n, e[n], er[n]))
    assert not bad, (what, bad)


def check(name, got, ref, o64):
    e, er = err(got, o64), err(ref, o64)
    print(f"{name}: err {e:.3e} ref {er:.3e} bound {bound(er):.3e}")
    assert e <= bound(er), (name, e, er)


def random_net(D, seed):
    from lnw.qlearn import BatchedQNet
    torch.manual_seed(seed)
    net = BatchedQNet.for_obs(D)
    with torch.no_grad():
        for m in (net.norm1, net.norm2):
            m.weight.add_(0.1 * torch.randn_like(m.weight))
            m.bias.add_(0.1 * torch.randn_like(m.bias))
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 2.0)
    return net


def random_batch(B, D, seed, device="cuda"):
    """Random transition rows. The rewards are centred at -2: the Q-values are
    >= 0, so the residual q - y of a row is not a difference of nearly equal
    numbers. err() is relative to the gradient's scale, and a residual that
    cancels multiplies the float32 rounding of q and y themselves (which no
    float32 arm avoids) by |q| / |q - y|; with two or three rows per radar
    output that alone can pass the 8 x 2^-23 floor."""
    g = torch.Generator().manual_seed(seed)

    def obs():
        o = torch.rand((B, D), generator=g)
        o[:, :49] = torch.randint(0, 256, (B, 49), generator=g) / 255.0
        return o

    act = torch.stack([torch.randint(0, 2, (B,), generator=g), torch.randint(0, 5, (B,), generator=g),
                       torch.randint(0, 50, (B,), generator=g), torch.zeros(B, dtype=torch.long)], 1)
    return dict(state=obs().to(device), next_state=obs().to(device), action=act.to(device, torch.int32),
                reward=(torch.randn(B, generator=g).mul(0.5) - 2.0).to(device),
                done=(torch.rand(B, generator=g) > 0.1).to(device, torch.int32))


def _adam(theta, grad, m, v, step, lr=1e-4, clamp=1.0, betas=(0.9, 0.999), eps=1e-8):
    import ctypes as C
    from lnw import _abi
    L = _abi.load()
    _abi.check(L.lnw_qnet_adam(theta.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), theta.numel(),
                               step.data_ptr(), lr, betas[0], betas[1], eps, clamp,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
