"""Shared helpers of the MAPPO learner tests (test_ppolearn_cpu.py,
test_gpu_ppolearn.py, and through _learner_cases.py test_learner_cases_cpu.py and
test_gpu_learner_hyper.py): the recorded sets of tests/golden/ppolearn*.npz, the
float64 oracle, generated inputs with their preconditions, the gradient check
(the measure and bound of _qlearn_util), a generated case and its comparison
against the kernels, lnw_ppo_clip_adam alone, and the float64 run of K updates."""
import ctypes as C
import os

import numpy as np
import torch

from _qlearn_util import U, bound, err  # noqa: F401
from lnw.ppolearn import (RUNNING, PPOLearner, actor_forward, actor_slices, critic_forward, critic_slices, flat_size,
                          losses, popart)
from lnw.rollout import BatchedActor, BatchedCritic, gae

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = (os.path.join(HERE, "golden", "ppolearn.npz"), os.path.join(HERE, "golden", "ppolearn_wide.npz"))
SETS = ("base", "small", "two", "wide")
ACTOR_GRAD_NAMES = tuple(n for n in actor_slices(31) if n not in RUNNING and n != "logstd")
CRITIC_GRAD_NAMES = tuple(critic_slices(4, 68))
# under per-row statistics these two have a mathematically zero gradient (the
# row's mean cancels the bias): their float32 value is rounding noise, measured
# against the conv's weight-gradient scale
NOISE = {"conv1.bias": "conv1.weight", "conv2.bias": "conv2.weight"}
# per-row tolerances: log-probabilities and entropies 1e-4 absolute, values 1e-5
# absolute, advantage 1e-5 relative to max |adv|
TOL_LP, TOL_V, TOL_ADV = 1e-4, 1e-5, 1e-5

_gold = None


def gold():
    global _gold
    if _gold is None:
        _gold = {}
        for p in GOLD:
            with np.load(p) as z:
                _gold.update({k: z[k] for k in z.files})
    return _gold


def hyper(prefix):
    g = gold()
    return dict(lr=float(g[f"{prefix}_lr"]), eps_clip=float(g[f"{prefix}_eps_clip"]),
                entropy_coef=float(g[f"{prefix}_entropy_coef"]), gamma=float(g[f"{prefix}_gamma"]))


def load_set(prefix, when="before"):
    """(actor, critic) of a recorded set and its minibatch in the order
    evaluate() received it: obs [groups, n, D] with index = the recorded
    permutation, the other tensors permuted."""
    g = gold()
    obs = g[f"{prefix}_obs"]
    n, D = int(g[f"{prefix}_n"]), obs.shape[1]
    nets = []
    for nm, net in (("actor", BatchedActor.for_obs(D)), ("critic", BatchedCritic(n * D))):
        pre = f"{prefix}.{nm}.{when}."
        nets.append(net.load_reference({k[len(pre):]: g[k] for k in g if k.startswith(pre)}))
    perm = torch.from_numpy(g[f"{prefix}_perm"])
    t = lambda k: torch.from_numpy(g[f"{prefix}_{k}"])[perm]  # noqa: E731
    batch = dict(obs=torch.from_numpy(obs).reshape(-1, n, D), index=perm, actions=t("actions"),
                 old_log_probs=t("old_log_probs"), rtg=t("rtg"), old_values=t("old_values"))
    return nets[0], nets[1], batch


def ref_flat(prefix, which, sl, what="grad"):
    """The reference's recorded gradients (or a state_dict: what = "before" /
    "after") of a network as a flat vector in the layout sl (zeros where nothing
    was recorded: the running statistics and logstd have no gradient)."""
    g = gold()
    flat = np.zeros(flat_size(sl), np.float32)
    for name, (k, shp) in sl.items():
        key = f"{prefix}.{which}.{what}.{name}"
        if key in g:
            flat[k:k + int(np.prod(shp))] = np.asarray(g[key], np.float32).reshape(-1)
    return torch.from_numpy(flat)


def segs(flat, sl, names):
    flat = flat.detach().cpu()
    return {n: flat[sl[n][0]:sl[n][0] + int(np.prod(sl[n][1]))] for n in names}


def gather(batch, n, D, dtype=torch.float64):
    """(rows [B, D], global states [B, n D]) of a batch, on the host."""
    obs = batch["obs"].detach().cpu().to(dtype)
    idx = batch.get("index")
    if idx is None:
        return obs.reshape(-1, D), obs.reshape(-1, n * D).repeat_interleave(n, 0)
    idx = idx.cpu()
    return obs.reshape(-1, D)[idx], obs.reshape(-1, n * D)[torch.div(idx, n, rounding_mode="floor")]


def oracle64(theta_actor, theta_critic, batch, n, D, eps_clip=0.2, entropy_coef=0.2, gamma=0.99, lambda_=0.95,
             grad=True, **_):
    """Float64 CPU autograd of the update's two losses, the reference's own
    sequence of operations (the sequential gae of lnw.rollout): dict(new_log_probs,
    entropies, values, advantage, stats, actor_loss, critic_loss, actor_grad,
    critic_grad), all float64."""
    asl, csl = actor_slices(D - 37), critic_slices(n, D)
    d = lambda t: t.detach().cpu().double()  # noqa: E731
    rows, gs = gather(batch, n, D)
    tha, thc = d(theta_actor).clone().requires_grad_(grad), d(theta_critic).clone().requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        lp, ent, stats = actor_forward(tha, rows, d(batch["actions"]), asl)
        v = critic_forward(thc, gs, csl)
        rtg, old_v = d(batch["rtg"]), d(batch["old_values"])
        with torch.no_grad():
            adv = popart(gae(rtg, v.detach(), gamma, lambda_), rtg)
        al, cl = losses(lp, ent, v, adv, d(batch["old_log_probs"]), rtg, old_v, eps_clip, entropy_coef)
    out = dict(new_log_probs=lp.detach(), entropies=ent.detach(), values=v.detach(), advantage=adv, stats=stats,
               actor_loss=al.detach(), critic_loss=cl.detach())
    if grad:
        al.backward()
        cl.backward()
        out["actor_grad"], out["critic_grad"] = tha.grad, thc.grad
    return out


def branch_report(o, batch, eps_clip):
    """Element counts of the six actor and three critic branches and the
    smallest distances of a ratio / a value step to the clip boundaries, from an
    oracle's tensors."""
    d = lambda t: t.detach().cpu().double()  # noqa: E731
    ratio = torch.exp(o["new_log_probs"] - d(batch["old_log_probs"]))
    a = o["advantage"][:, None].expand_as(ratio)
    cnt = {}
    for rn, rm in (("in", (ratio >= 1 - eps_clip) & (ratio <= 1 + eps_clip)), ("above", ratio > 1 + eps_clip),
                   ("below", ratio < 1 - eps_clip)):
        for an, am in (("pos", a > 0), ("neg", a < 0)):
            cnt[f"actor_{rn}_{an}"] = int((rm & am).sum())
    v, ov, r = o["values"], d(batch["old_values"]), d(batch["rtg"])
    inr = (v - ov).abs() <= eps_clip
    t1, t2 = (v - r) ** 2, (torch.clamp(v, ov - eps_clip, ov + eps_clip) - r) ** 2
    cnt.update(critic_in=int(inr.sum()), critic_first=int((~inr & (t1 > t2)).sum()),
               critic_second=int((~inr & (t1 < t2)).sum()))
    margin_a = float(torch.minimum((ratio - (1 - eps_clip)).abs(), (ratio - (1 + eps_clip)).abs()).min())
    margin_c = float(((v - ov).abs() - eps_clip).abs().min())
    return cnt, margin_a, margin_c


def random_nets(n, D, seed):
    torch.manual_seed(seed)
    actor, critic = BatchedActor.for_obs(D), BatchedCritic(n * D)
    with torch.no_grad():
        for m in (actor.norm1, actor.norm2, actor.layernorm):
            m.weight.add_(0.1 * torch.randn_like(m.weight))
            m.bias.add_(0.1 * torch.randn_like(m.bias))
        for m in (actor.norm1, actor.norm2):
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 2.0)
    return actor, critic


def random_batch(actor, critic, B, n, D, seed, index="identity", sigma=2.0, eps_clip=0.2):
    """A generated minibatch on the host, built like the recorded sets: old
    log-probabilities the actor's own + N(0, 0.3), old values the critic's own +
    N(0, 0.3), rtg ~ N(1, sigma). (The recorded sets draw rtg around 0, where the
    values are: fc4.bias's gradient is then sum(v - rtg) / (2 B loss), a sum that
    cancels to about 1 / sqrt(B) of its terms, and err(), relative to that one
    number, multiplies the float32 rounding of the values themselves, which no
    float32 arm avoids, by sqrt(B); one generated case missed the 8 x 2^-23 floor
    by 0.7 % that way. Centred at 1 the sum is its terms' size.) index: "identity" (B a multiple of n: None),
    or "shuffled" (B rows drawn from a larger buffer in random order, groups
    repeating). An element whose ratio or value step falls within 1e-3 of a clip
    boundary has its old value moved by 0.01, so the 1e-4 margin the tests
    assert holds by construction."""
    g = torch.Generator().manual_seed(seed)
    if index == "identity":
        assert B % n == 0
        G, idx = B // n, None
    else:
        G = max(2, (B + n - 1) // n)
        idx = torch.randint(0, G * n, (B,), generator=g)
    obs = torch.rand((G * n, D), generator=g)
    obs[:, :49] = torch.randint(0, 256, (G * n, 49), generator=g) / 255.0
    batch = dict(obs=obs.reshape(G, n, D), index=idx, actions=torch.rand((B, 4), generator=g),
                 old_log_probs=torch.zeros(B, 4), rtg=1.0 + sigma * torch.randn(B, generator=g), old_values=torch.zeros(B))
    from lnw.ppolearn import pack
    tha, thc = pack(actor, actor_slices(D - 37)), pack(critic, critic_slices(n, D))
    o = oracle64(tha, thc, batch, n, D, grad=False)
    noise_lp, noise_v = 0.3 * torch.randn((B, 4), generator=g), 0.3 * torch.randn(B, generator=g)
    old_lp = o["new_log_probs"] + noise_lp.double()
    old_v = o["values"] + noise_v.double()
    ratio = torch.exp(o["new_log_probs"] - old_lp)
    near = torch.minimum((ratio - (1 - eps_clip)).abs(), (ratio - (1 + eps_clip)).abs()) < 1e-3
    old_lp = torch.where(near, old_lp + 0.01, old_lp)
    near = ((o["values"] - old_v).abs() - eps_clip).abs() < 1e-3
    old_v = torch.where(near, old_v + 0.01, old_v)
    batch["old_log_probs"], batch["old_values"] = old_lp.float(), old_v.float()
    return batch


def grad_errors(flat, flat64, sl, names):
    a, b = segs(flat, sl, names), segs(flat64, sl, names)
    return {n: err(a[n], b[n], float(b[NOISE[n]].abs().max()) if n in NOISE else None) for n in names}


def assert_grads_within(flat, flat_ref, flat64, sl, names, what, report=None):
    """Every tensor of a flat gradient within 8 x max(err_ref, 2^-23) of the
    float64 oracle's, err_ref the float32 reference arm's own error."""
    e, er = grad_errors(flat, flat64, sl, names), grad_errors(flat_ref, flat64, sl, names)
    bad = []
    for n in names:
        if report is not None:
            report.append((what, n, e[n], er[n]))
        print(f"{what} {n}: err {e[n]:.3e} ref {er[n]:.3e} bound {bound(er[n]):.3e}")
        if not e[n] <= bound(er[n]):
            bad.append((n, e[n], er[n]))
    assert not bad, (what, bad)


def assert_rows_within(out, o64, what):
    """The per-row tensors within the project's tolerances of the oracle's."""
    for k, tol in (("new_log_probs", TOL_LP), ("entropies", TOL_LP), ("values", TOL_V)):
        d = float((out[k].detach().cpu().double() - o64[k]).abs().max())
        print(f"{what} {k}: max abs {d:.3e} (tolerance {tol:.0e})")
        assert d <= tol, (what, k, d)
    e = err(out["advantage"], o64["advantage"])
    print(f"{what} advantage: err {e:.3e} (tolerance {TOL_ADV:.0e})")
    assert e <= TOL_ADV, (what, "advantage", e)


def ulps(a, b):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    return np.abs(a.astype(np.float64) - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))


def close_loss(name, got, want, rel=1e-5):
    got, want = float(got), float(want)
    print(f"{name}: {got!r} against {want!r}")
    assert abs(got - want) <= rel * abs(want), (name, got, want)


def _clip_adam(theta, grad, m, v, step, clip, lr=1e-4, max_norm=1.0, betas=(0.9, 0.999), eps=1e-8):
    from lnw import _abi
    L = _abi.load()
    _abi.check(L.lnw_ppo_clip_adam(theta.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), theta.numel(),
                                   step.data_ptr(), lr, betas[0], betas[1], eps, max_norm, clip.data_ptr(),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def generated(B, n, D, index, seed=None, sigma=2.0, hyper=None):
    """Nets, the batch on the host, the float64 oracle and the float32 host arm's
    result of a generated case, its preconditions asserted. hyper: the loss
    hyperparameters off their defaults (eps_clip, entropy_coef, gamma, lambda_),
    for the batch's margins, the host arm and the oracle alike."""
    hyper = dict(hyper or {})
    eps_clip = hyper.get("eps_clip", 0.2)
    seed = 1000 * n + 7 * B + D if seed is None else seed
    actor, critic = random_nets(n, D, seed)
    batch = random_batch(actor, critic, B, n, D, seed + 1, index=index, sigma=sigma, eps_clip=eps_clip)
    T = PPOLearner(actor, critic, impl="torch", device="cpu", **hyper)
    o64 = oracle64(T.theta_actor, T.theta_critic, batch, n, D, **hyper)
    cnt, margin_a, margin_c = branch_report(o64, batch, eps_clip)
    print(f"B={B} n={n} D={D} {index}: {cnt} margins {margin_a:.2e} {margin_c:.2e}")
    assert margin_a >= 1e-4 and margin_c >= 1e-4, (margin_a, margin_c)
    if B >= 63:
        assert min(v for k, v in cnt.items() if k.startswith("actor")) >= 8, cnt
        assert min(v for k, v in cnt.items() if k.startswith("critic")) >= 4, cnt
    ref = T.grad(batch, update_running=False)
    assert_rows_within(ref, o64, "float32 host arm")
    return actor, critic, batch, o64, ref


def check_case(actor, critic, batch, o64, ref, what, hyper=None, **kw):
    H = PPOLearner(actor, critic, **dict(hyper or {}), **kw)
    out = H.grad(batch, update_running=False)
    assert_rows_within(out, o64, what)
    for k in ("actor_loss", "critic_loss"):
        close_loss(f"{what} {k}", out[k], o64[k])
    assert_grads_within(out["actor_grad"], ref["actor_grad"], o64["actor_grad"], H.actor_sl, ACTOR_GRAD_NAMES,
                        what + " actor")
    assert_grads_within(out["critic_grad"], ref["critic_grad"], o64["critic_grad"], H.critic_sl, CRITIC_GRAD_NAMES,
                        what + " critic")
    return H, out


def steps64(actor, critic, batches, K, n, D, lr, max_grad_norm=1.0, betas=(0.9, 0.999), eps=1e-8, eps_clip=0.2,
            entropy_coef=0.2, gamma=0.99, lambda_=0.95):
    """K updates in float64 on the host: the oracle's gradients, clip_grad_norm_
    and torch.optim.Adam on float64 vectors."""
    T = PPOLearner(actor, critic, impl="torch", device="cpu")
    pa = torch.nn.Parameter(T.theta_actor.double())
    pc = torch.nn.Parameter(T.theta_critic.double())
    opts = [torch.optim.Adam([p], lr=lr, betas=betas, eps=eps) for p in (pa, pc)]
    for k in range(K):
        o = oracle64(pa, pc, batches[k % len(batches)], n, D, eps_clip=eps_clip, entropy_coef=entropy_coef,
                     gamma=gamma, lambda_=lambda_)
        for p, g, opt in ((pa, o["actor_grad"], opts[0]), (pc, o["critic_grad"], opts[1])):
            p.grad = g.clone()
            torch.nn.utils.clip_grad_norm_([p], max_grad_norm)
            opt.step()
    return pa.detach(), pc.detach()
