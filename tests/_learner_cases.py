"""Shared inputs of the learner hyperparameter tests (test_learner_cases_cpu.py,
test_gpu_learner_hyper.py): the tables of cases that take lnw_ppo_grad /
lnw_ppo_clip_adam and lnw_qnet_grad / lnw_qnet_adam off the reference's default
hyperparameters and to the ends of the shapes their code distinguishes, each
case's inputs built once per process from seeds, and a float64 Adam in numpy.

TEST INFRASTRUCTURE: the table in DESIGN.md ("MAPPO learner", "DDQN learner")
says which path of which kernel each case is there for."""
import functools

import numpy as np
import torch

import _ppolearn_util as P
import _qlearn_util as Q

PPO_DEFAULTS = dict(eps_clip=0.2, entropy_coef=0.2, gamma=0.99, lambda_=0.95)
Q_GAMMA = 0.99
ADAM_DEFAULTS = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8)

# ---- MAPPO, gradient cases: (B, n, D, hyper), every one with a shuffled index -------------------
# B = 1025: the advantage scan's Lb = 2, 513 threads used, a last block of one row; B = 4097: Lb = 5, 819 full
# blocks and one of 2 rows, 17 weight-gradient chunks, the last short. gamma lambda_ = 1: a block's carry reaches
# every earlier row undamped. gamma = 0: no bootstrap term. lambda_ = 0: pow(0, Lb) = 0 and pow(0, 0) = 1.
# (1, 56), (16, 100), (4, 52): the ABI's fleet limits (n = 1; the widest critic fc1; n_in = 15 < one K tile).
PPO_CASES = {
    "clip0.1-noent-c1": (129, 4, 68, dict(eps_clip=0.1, entropy_coef=0.0, gamma=1.0, lambda_=1.0)),
    "clip0.3-ent0.01-c0.72": (129, 4, 68, dict(eps_clip=0.3, entropy_coef=0.01, gamma=0.9, lambda_=0.8)),
    "gamma0": (129, 4, 68, dict(gamma=0.0)),
    "lambda0": (129, 4, 68, dict(lambda_=0.0)),
    "1025": (1025, 4, 68, {}),
    "1025-c1": (1025, 4, 68, dict(gamma=1.0, lambda_=1.0)),
    "4097-c1": (4097, 4, 68, dict(gamma=1.0, lambda_=1.0)),
    "n1": (129, 1, 56, {}),
    "n16-D100": (129, 16, 100, {}),
    "D52": (129, 4, 52, {}),
}
# running statistics (update_running=True): pl_running_kernel's second trip (B > 256) and tail cut (B > 2048)
PPO_RUNNING_CASES = {"300": (300, 4, 68, {}), "4097": PPO_CASES["4097-c1"]}


@functools.lru_cache(maxsize=None)
def _ppo_generated(B, n, D, hyper):
    return P.generated(B, n, D, "shuffled", hyper=dict(hyper))


def ppo_case(B, n, D, hyper):
    """generated()'s (actor, critic, batch, o64, ref) of a case, built once per
    process (equal cases share it); read-only."""
    return _ppo_generated(B, n, D, tuple(sorted(hyper.items())))


# ---- DDQN, gradient cases: policy_bn, B, D, gamma and what is done to the generated rows --------
Q_CASES = {
    "gamma0": dict(policy_bn="batch", B=600, D=68, gamma=0.0),
    "gamma1": dict(policy_bn="batch", B=600, D=68, gamma=1.0),
    "running-gamma0.9": dict(policy_bn="running", B=600, D=84, gamma=0.9),
    "done-all-1": dict(policy_bn="batch", B=64, D=68, done=1),
    "done-all-0": dict(policy_bn="batch", B=64, D=68, done=0),
    "reward-f64": dict(policy_bn="batch", B=64, D=68, reward_f64=True),
    "action-3-columns": dict(policy_bn="batch", B=64, D=68, columns=3),
    "action-6-columns": dict(policy_bn="batch", B=64, D=68, columns=6),
}


@functools.lru_cache(maxsize=None)
def q_case(name):
    """(policy, target, batch on the host, gamma, policy_bn) of a DDQN case:
    test_shapes_against_torch_arm's networks and rows with the case's change."""
    c = Q_CASES[name]
    B, D = c["B"], c["D"]
    pol, tgt = Q.random_net(D, 100 + D), Q.random_net(D, 200 + D)
    batch = Q.random_batch(B, D, 7 * B + D, device="cpu")
    if "done" in c:
        batch["done"] = torch.full_like(batch["done"], c["done"])
    if c.get("reward_f64"):
        # rewards that no float32 holds: the float32 draw plus a float64 fraction below its last bit
        g = torch.Generator().manual_seed(B + D)
        batch["reward"] = batch["reward"].double() + 1e-8 * torch.rand(B, generator=g, dtype=torch.float64)
    if "columns" in c:
        k = c["columns"]
        act = torch.full((B, k), 7, dtype=torch.int32)  # (columns past the third are never read)
        act[:, :3] = batch["action"][:, :3]
        batch["action"] = act.contiguous()
    return pol, tgt, batch, c.get("gamma", Q_GAMMA), c["policy_bn"]


# ---- Adam, both entry points -------------------------------------------------------------------------
# steps: gradients drawn per step (0.3 randn); t0: the step counter before the first step; preload: moments
# m = 0.1 randn, v = 0.01 U(0.5, 2) instead of zeros
ADAM_COUNTS = (3000, 257, 1)
ADAM_CASES = {
    "A1": dict(lr=3e-4, betas=(0.5, 0.9), eps=1e-3, steps=3),
    "A2": dict(betas=(0.0, 0.999), steps=2),
    "A3-999": dict(t0=999, preload=True, steps=1),
    "A3-1e6": dict(t0=10 ** 6 - 1, preload=True, steps=1),
    "A4": dict(lr=0.0, steps=1),
    # a schedule's values (lr 1e-4 decayed by 0.97 per epoch, as float32): the shortest decimal that rounds to the
    # float has 7 digits after 7 epochs and 9, as_decimal's last trip, after 63
    "A5": dict(lr=float(np.float32(1e-4 * 0.97 ** 7)), steps=2),
    "A5-63": dict(lr=float(np.float32(1e-4 * 0.97 ** 63)), steps=2),
}


def adam_hyper(name):
    c = ADAM_CASES[name]
    return {k: c.get(k, v) for k, v in ADAM_DEFAULTS.items()}


def adam_inputs(name, count):
    """(theta, m, v, t0, [gradient per step]) of an Adam case, float32 on the
    host. The parameters are 0.05 randn, a network weight's size: the bound's 2
    ulp of a parameter near 1 would hide what eps = 1e-3 does to one element."""
    c = ADAM_CASES[name]
    g = torch.Generator().manual_seed(1000 * sorted(ADAM_CASES).index(name) + count)
    theta = 0.05 * torch.randn(count, generator=g)
    if c.get("preload"):
        m, v = 0.1 * torch.randn(count, generator=g), 0.01 * (0.5 + 1.5 * torch.rand(count, generator=g))
    else:
        m, v = torch.zeros(count), torch.zeros(count)
    return theta, m, v, c.get("t0", 0), [0.3 * torch.randn(count, generator=g) for _ in range(c["steps"])]


def adam64(theta, m, v, t0, grads, lr, betas, eps, clamp=0.0, max_norm=None):
    """torch.optim.Adam's steps (no weight decay) in float64 numpy, after the
    entry point's own treatment of the gradient: lnw_qnet_adam's clamp (> 0), or
    lnw_ppo_clip_adam's clip_grad_norm_(max_norm). Returns (theta, m, v, t)."""
    p, m, v = (np.asarray(x, np.float64).copy() for x in (theta, m, v))
    t = int(t0)
    for g in grads:
        g = np.asarray(g, np.float64)
        if clamp > 0:
            g = np.clip(g, -clamp, clamp)
        if max_norm is not None:
            g = g * min(1.0, max_norm / (np.sqrt((g * g).sum()) + 1e-6))
        t += 1
        m = betas[0] * m + (1.0 - betas[0]) * g
        v = betas[1] * v + (1.0 - betas[1]) * g * g
        p = p - lr / (1.0 - betas[0] ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - betas[1] ** t) + eps)
    return p, m, v, t


def adam_bound(p_before, p_after, lr):
    """|theta - p_after| <= 2 ulp(p_after) + 2^-21 max(lr, |p_after - p_before|),
    the rule of test_adam_three_steps_and_clamp with its rounding term scaled by
    the update's size where that exceeds lr (float32 arrays from the torch arm)."""
    p_before, p_after = np.asarray(p_before, np.float32), np.asarray(p_after, np.float32)
    upd = np.abs(p_after.astype(np.float64) - p_before)
    return 2 * np.spacing(np.abs(p_after)).astype(np.float64) + 2.0 ** -21 * np.maximum(lr, upd)


# ---- end to end: every hyperparameter off its default at once ------------------------------------
PPO_E2E = dict(lr=3e-4, eps_clip=0.3, entropy_coef=0.01, gamma=0.9, lambda_=0.8, max_grad_norm=0.5,
               betas=(0.8, 0.99), eps=1e-6)
Q_E2E = dict(lr=3e-4, gamma=0.9, betas=(0.8, 0.99), eps=1e-6, clamp=0.5)
E2E_ROWS, E2E_STEPS = 129, 3


def q_steps64(pol, tgt, batches, K, lr, gamma, betas, eps, clamp, policy_bn="batch"):
    """K DDQN updates in float64 on the host: the oracle's gradient, the clamp
    and torch.optim.Adam on a float64 vector (the target is not synchronised:
    its parameters stay, and its running statistics take no part)."""
    p = torch.nn.Parameter(pol.packed().double())
    target = tgt.packed().double()
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    for k in range(K):
        g = Q.oracle64(p, target, batches[k % len(batches)], gamma, policy_bn)["grad"]
        for name in Q.RUNNING:  # (the running statistics have no gradient; autograd leaves zeros there)
            assert not Q.segs(g, pol.n_in, (name,))[name].any()
        p.grad = g.clamp(-clamp, clamp) if clamp > 0 else g.clone()
        opt.step()
    return p.detach()


@functools.lru_cache(maxsize=None)
def ppo_e2e():
    """The MAPPO end-to-end run's inputs and both host runs of its E2E_STEPS
    updates: dict(actor, critic, batches, T the float32 torch arm after the
    steps, clips its [actor, critic][factor, norm] per step, a64, c64 the float64
    run's vectors)."""
    n, D = 4, 68
    actor, critic = P.random_nets(n, D, 51)
    batches = [P.random_batch(actor, critic, E2E_ROWS, n, D, 510 + k, index="shuffled",
                              eps_clip=PPO_E2E["eps_clip"]) for k in range(E2E_STEPS)]
    T = P.PPOLearner(actor, critic, impl="torch", device="cpu", **PPO_E2E)
    clips = []
    for b in batches:
        T.step(b)
        clips.append(T.clip.clone())
    a64, c64 = P.steps64(actor, critic, batches, E2E_STEPS, n, D, **PPO_E2E)
    return dict(actor=actor, critic=critic, batches=batches, T=T, clips=torch.stack(clips), a64=a64, c64=c64)


@functools.lru_cache(maxsize=None)
def q_e2e():
    """The DDQN end-to-end run likewise: dict(policy, target, batches, T, t64)."""
    from lnw.qlearn import QLearner
    D = 68
    pol, tgt = Q.random_net(D, 61), Q.random_net(D, 62)
    batches = [Q.random_batch(E2E_ROWS, D, 610 + k, device="cpu") for k in range(E2E_STEPS)]
    T = QLearner(pol, tgt, impl="torch", device="cpu", **Q_E2E)
    for b in batches:
        T.step(b)
    return dict(policy=pol, target=tgt, batches=batches, T=T, t64=q_steps64(pol, tgt, batches, E2E_STEPS, **Q_E2E))


def e2e_deviations(theta, theta_ref, theta64, tensors, noise):
    """Per parameter tensor outside `noise`: (name, the largest deviation of theta
    from the float64 run, the float32 reference arm's own, the bound 8 x max(that,
    2^-23 of the tensor's scale))."""
    rows = []
    for name in tensors(theta):
        if name in noise:
            continue
        a, b, c = tensors(theta)[name], tensors(theta_ref)[name], tensors(theta64)[name]
        dh, dt = float((a.double() - c).abs().max()), float((b.double() - c).abs().max())
        rows.append((name, dh, dt, 8 * max(dt, 2.0 ** -23 * float(c.abs().max()))))
    return rows
