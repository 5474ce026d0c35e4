#!/usr/bin/env python3
"""Golden vectors for the MAPPO learner step of lnw.ppolearn (PPOLearner).

Drives the reference's own PPO.learn (ppo.py:190-419) through the stub harness
of make_golden.py (this container only): SIDE = "blue", WANDA off, a PPO over
an env stub with K_epochs = 1, `rollout` replaced by a function that returns
prepared tensors of n_rollouts * n_rollout_steps * n = BATCH_SIZE = 64 rows, so
the no-replacement sampler yields one minibatch that is a permutation of all
rows, and learn(total_timesteps = 64) runs exactly one update.
Recorded per set: both state_dicts before and after; the minibatch in the order
evaluate() received it (the permutation of the prepared rows); evaluate()'s
new_log_probs, entropies and V; the popart advantage; both losses; both
networks' gradients before the clip and the norm clip_grad_norm_ returned;
gamma, eps_clip and lr.
Inputs: make_policy_golden.random_obs rows, six of them with constant terrain
windows (exact ties inside every pool window); global states the concatenation
of the group's rows; old log-probabilities the actor's own + N(0, 0.3), old
values the critic's own + N(0, 0.3). Sets:
  base   n = 4, D = 68, rtg ~ N(0, 2)
  small  n = 4, D = 68, rtg ~ N(0, 0.05): the actor's norm below 1, clip inactive
  two    n = 2, D = 60
  wide   n = 8, D = 84 (the 64-wide fc1 input)
Conditions asserted here (the first seed that meets them is taken): each of the
six actor branches (ratio in range / above / below x advantage sign) holds at
least 8 elements and each of the three critic branches (in range; clamped with
the first term larger; clamped with the second larger) at least 4 rows; no ratio
within 1e-4 of 1 +- eps and no |v - v_old| within 1e-4 of eps; at least 4 rows
with an exact positive pool tie; over the sets, an actor norm below 1 and one
above 1.
Writes tests/golden/ppolearn.npz (base, small, two) and ppolearn_wide.npz (wide:
its critic's 32 x 672 fc1 would take one file past the size limit of a
committed file).

usage: python tests/golden/make_ppolearn_golden.py
"""
import copy
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402
from make_policy_golden import random_obs  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = {"wide": os.path.join(HERE, "ppolearn_wide.npz")}
OUT_DEFAULT = os.path.join(HERE, "ppolearn.npz")
B = 64
SETS = (("base", 4, 68, 2.0), ("small", 4, 68, 0.05), ("two", 2, 60, 2.0), ("wide", 8, 84, 2.0))


def tie_rows(torch, F, net, obs):
    """Rows whose first ReLU map (the row's own statistics) has a pool window
    with an exact tie at a positive maximum."""
    with torch.no_grad():
        z = net.conv1(torch.tensor(obs[:, :49]).reshape(-1, 1, 7, 7))
        z = F.instance_norm(z, weight=net.norm1.weight, bias=net.norm1.bias, eps=1e-5)
        a = F.relu(z)[:, :, :6, :6].reshape(-1, 5, 3, 2, 3, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 5, 9, 4)
        mx = a.max(-1, keepdim=True).values
        tie = ((a == mx).sum(-1) > 1) & (mx[..., 0] > 0)
        return tie.any(-1).any(-1).numpy()


def branches(torch, lp, old_lp, adv, v, old_v, rtg, eps):
    """Element counts of the six actor and three critic branches, and the
    smallest distances to the clip boundaries."""
    ratio = torch.exp(lp - old_lp)
    a = adv.reshape(-1, 1).expand_as(ratio)
    cnt = {}
    for rn, rm in (("in", (ratio >= 1 - eps) & (ratio <= 1 + eps)), ("above", ratio > 1 + eps),
                   ("below", ratio < 1 - eps)):
        for an, am in (("pos", a > 0), ("neg", a < 0)):
            cnt[f"actor_{rn}_{an}"] = int((rm & am).sum())
    inr = (v - old_v).abs() <= eps
    t1 = (v - rtg) ** 2
    t2 = (torch.clamp(v, old_v - eps, old_v + eps) - rtg) ** 2
    cnt["critic_in"] = int(inr.sum())
    cnt["critic_first"] = int((~inr & (t1 > t2)).sum())
    cnt["critic_second"] = int((~inr & (t1 < t2)).sum())
    margin_a = float(torch.minimum((ratio - (1 - eps)).abs(), (ratio - (1 + eps)).abs()).min())
    margin_c = float(((v - old_v).abs() - eps).abs().min())
    return cnt, margin_a, margin_c


def one_set(torch, ppo, prefix, n, D, sigma, seed, out):
    """Record one set; None (nothing recorded) if this seed's inputs miss a
    condition, else the actor's gradient norm."""
    import torch.nn.functional as F
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    ppo.SIDE, ppo.WANDA = "blue", False
    assert ppo.BATCH_SIZE == B
    env = types.SimpleNamespace(observation_space=D, red_observation_space=D, action_space=4,
                                blue_ships=[None] * n, red_ships=[None] * n)
    agent = ppo.PPO(env, torch.device("cpu"), K_epochs=1)
    G = B // n
    agent.n_rollouts, agent.n_rollout_steps = G // 8, 8
    with torch.no_grad():
        for m in (agent.actor.norm1, agent.actor.norm2, agent.actor.layernorm):
            m.weight.add_(0.1 * torch.randn_like(m.weight))
            m.bias.add_(0.1 * torch.randn_like(m.bias))
    obs = random_obs(rng, B, D)
    for i in range(6):  # constant terrain windows: exact ties inside every pool window
        obs[i, :49] = np.float32((40 + 35 * i) / 255.0)
    ties = tie_rows(torch, F, agent.actor, obs)
    if ties.sum() < 4:
        return None
    acts = rng.random((B, 4)).astype(np.float32)
    gs = np.repeat(obs.reshape(G, n * D), n, axis=0)
    rtg = rng.normal(0.0, sigma, B).astype(np.float32)
    probe = copy.deepcopy(agent.actor).train()
    with torch.no_grad():
        own_lp = torch.stack([probe.get_dist(torch.tensor(obs[i]), torch.tensor(acts[i]))[0] for i in range(B)])
        own_v = agent.critic(torch.tensor(gs)).reshape(-1)
    old_lp = (own_lp + 0.3 * torch.randn(B, 4)).numpy()
    old_v = (own_v + 0.3 * torch.randn(B)).numpy()
    R, T = agent.n_rollouts, agent.n_rollout_steps
    t = torch.tensor
    prepared = (t(obs).reshape(R, T, n, D), t(acts).reshape(R, T, n, 4), t(old_lp).reshape(R, T, n, 4),
                t(rtg).reshape(R, T, n, 1), B, t(gs).reshape(R, T, n, n * D), t(old_v).reshape(R, T, n, 1))
    agent.rollout = lambda *a, **k: prepared
    before = {nm: {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
              for nm, net in (("actor", agent.actor), ("critic", agent.critic))}
    rec = {"clip": []}
    real_eval, real_pop, real_clip = agent.evaluate, agent.popart_normalize, torch.nn.utils.clip_grad_norm_

    def evaluate(states, global_states, actions):
        v, lp, en = real_eval(states, global_states, actions)
        rec.update(states=states.detach().numpy().copy(), lp=lp.detach().clone(), ent=en.detach().clone(),
                   v=v.detach().reshape(-1).clone())
        return v, lp, en

    def popart_normalize(values, targets):
        r = real_pop(values, targets)
        rec["adv"] = r.detach().reshape(-1).clone()
        return r

    def clip_grad_norm_(params, max_norm, *a, **k):
        params = list(params)
        grads = [None if p.grad is None else p.grad.detach().numpy().copy() for p in params]
        norm = real_clip(params, max_norm, *a, **k)
        rec["clip"].append((grads, float(norm)))
        return norm

    agent.evaluate, agent.popart_normalize = evaluate, popart_normalize
    torch.nn.utils.clip_grad_norm_ = clip_grad_norm_
    try:
        with make_golden.quiet():
            agent.learn(total_timesteps=B)
    finally:
        torch.nn.utils.clip_grad_norm_ = real_clip
    assert len(rec["clip"]) == 2
    # the permutation: minibatch row i is prepared row perm[i]
    perm = np.array([int(np.flatnonzero((obs == rec["states"][i]).all(1))[0]) for i in range(B)])
    assert sorted(perm) == list(range(B))
    eps = float(agent.eps_clip)
    cnt, margin_a, margin_c = branches(torch, rec["lp"], t(old_lp[perm]), rec["adv"], rec["v"], t(old_v[perm]),
                                       t(rtg[perm]), eps)
    print(prefix, "seed", seed, cnt, "margins", margin_a, margin_c, "ties", int(ties.sum()),
          "norms", rec["clip"][0][1], rec["clip"][1][1])
    if min(v for k, v in cnt.items() if k.startswith("actor")) < 8:
        return None
    if min(v for k, v in cnt.items() if k.startswith("critic")) < 4:
        return None
    if margin_a < 1e-4 or margin_c < 1e-4:
        return None
    # the losses as learn() computes them, from the recorded tensors
    with torch.no_grad():
        ratio = torch.exp(rec["lp"] - t(old_lp[perm]))
        adv = rec["adv"].reshape(-1, 1)
        s1, s2 = adv * ratio, torch.clamp(ratio, 1 - agent.eps_clip, 1 + agent.eps_clip) * adv
        actor_loss = -(torch.min(s1, s2).mean() + agent.epsilon * rec["ent"].mean())
        val, rew, ov = rec["v"], t(rtg[perm]), t(old_v[perm])
        critic_loss = torch.sqrt(torch.max((val - rew) ** 2, (torch.clamp(val, ov - agent.eps_clip,
                                                                          ov + agent.eps_clip) - rew) ** 2).mean())
    assert abs(float(actor_loss) - agent.actor_loss_log[-1]) <= 1e-6 * max(1.0, abs(float(actor_loss)))
    after = {nm: {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
             for nm, net in (("actor", agent.actor), ("critic", agent.critic))}
    out.update({f"{prefix}_obs": obs, f"{prefix}_actions": acts, f"{prefix}_old_log_probs": old_lp,
                f"{prefix}_rtg": rtg, f"{prefix}_old_values": old_v, f"{prefix}_perm": perm.astype(np.int64),
                f"{prefix}_n": np.int64(n), f"{prefix}_new_log_probs": rec["lp"].numpy(),
                f"{prefix}_entropies": rec["ent"].numpy(), f"{prefix}_values": rec["v"].numpy(),
                f"{prefix}_advantage": rec["adv"].numpy(), f"{prefix}_actor_loss": np.float32(float(actor_loss)),
                f"{prefix}_critic_loss": np.float32(float(critic_loss)),
                f"{prefix}_actor_norm": np.float32(rec["clip"][0][1]),
                f"{prefix}_critic_norm": np.float32(rec["clip"][1][1]),
                f"{prefix}_gamma": np.float64(agent.gamma), f"{prefix}_eps_clip": np.float64(eps),
                f"{prefix}_entropy_coef": np.float64(agent.epsilon), f"{prefix}_lr": np.float64(agent.learning_rate),
                f"{prefix}_tie_rows": ties, f"{prefix}_seed": np.int64(seed)})
    for k, nm, net in ((0, "actor", agent.actor), (1, "critic", agent.critic)):
        out.update({f"{prefix}.{nm}.before.{key}": v for key, v in before[nm].items()})
        out.update({f"{prefix}.{nm}.after.{key}": v for key, v in after[nm].items()})
        for (key, _), g in zip(net.named_parameters(), rec["clip"][k][0]):
            if g is not None:
                out[f"{prefix}.{nm}.grad.{key}"] = g
    return rec["clip"][0][1]


def main():
    make_golden.import_reference()
    import torch
    import ppo
    out, norms = {}, []
    for prefix, n, D, sigma in SETS:
        for seed in range(1, 64):
            norm = one_set(torch, ppo, prefix, n, D, sigma, seed, out)
            if norm is not None:
                norms.append(norm)
                break
        else:
            raise AssertionError(f"no seed met the conditions of set {prefix}")
    assert min(norms) < 1.0 < max(norms), norms
    for path in sorted(set(OUT.values()) | {OUT_DEFAULT}):
        keep = {k: v for k, v in out.items() if OUT.get(k.split("_")[0].split(".")[0], OUT_DEFAULT) == path}
        np.savez_compressed(path, **keep)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
