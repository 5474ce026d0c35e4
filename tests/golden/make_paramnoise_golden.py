#!/usr/bin/env python3
"""Golden vectors for parameter-noise exploration (lnw.rollout.Rollout with
`member_thetas`, lnw.rollout.noise_mask) taken from the reference's own
`PPO.rollout` (ppo.py:421-671) with its default exploration on
(`add_param_noise = True`, `NETWORK_NOISE = True`, std 0.5, clip 0.05:
config.json). TEST INFRASTRUCTURE ONLY: runs where the reference is mounted,
through the stub harness and the recording tape of make_rollout_golden.py /
make_golden.py.

What runs is the reference loop as written, with make_rollout_golden.py's
substitutions (the loop observes the env it steps; the env's draws come from a
recording tape). Recorded, beside everything make_rollout_golden.py records:
  per episode  the noised actor's state_dict, captured at the episode's first
               actor call (`ep_actor.<name>` [R, ...]): ppo.py:466-482 reloads
               the noiseless actor and adds clamp(N(0, std), -clip, +clip) to
               every parameter whose name holds none of norm1, norm2, layernorm;
  names        the actor's state_dict names (`names`) and, per name, whether any
               episode's tensor differs from the noiseless one (`changed`).

usage: python tests/golden/make_paramnoise_golden.py   (writes rollout_paramnoise.npz)
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
TYPE_CODE = make_golden.TYPE_CODE


def run(name, *, n_blue, n_red, R, T, seed, std, clip):
    game, combatant, landingship = make_golden.import_reference()
    import torch
    import network  # noqa: F401
    import ppo
    game.N_RED_LANDINGSHIP = 0
    game.LANDING_OPS = False
    game.TRAINED_RED = False
    game.SIDE = "blue"
    game.TACTICS = "aggressive"
    game.DISCRETE = combatant.DISCRETE = landingship.DISCRETE = False
    combatant.CUR_SIDE = landingship.CUR_SIDE = "blue"
    ppo.TRAINED_RED = False
    ppo.SIDE = "blue"
    ppo.WANDA = False
    ppo.NETWORK_NOISE = True
    tape = make_golden.TapeRNG(seed)
    game.random = combatant.random = landingship.random = tape
    np_beta = np.random.beta
    np.random.beta = tape.beta
    try:
        env = game.Game()
        marks, rec = [], dict(act=[], f32=[], rew=[], done=[], cog=[], ep=[])
        eps, ep_actors = [], []
        real_reset, real_step = env.reset, env.step
        fresh = [False]  # an episode began and its actor has not been called yet

        def reset(*a, **k):
            marks.append(len(tape.vals))
            out = real_reset(*a, **k)
            ships = list(env.blue_ships) + list(env.red_ships)
            eps.append(dict(tape_start=marks[-1], ducting=env.ducting_factor,
                            spawn=[tuple(int(v) for v in s.position) for s in ships],
                            types=[TYPE_CODE[s.ship_type] for s in ships]))
            fresh[0] = True
            return out

        def step(action):
            arr = np.asarray(action)
            rec["act"].append(np.array(arr, np.float64))
            rec["f32"].append(arr.dtype == np.float32)
            obs, reward, done, cog = real_step(action)
            rec["rew"].append([float(r) for r in reward])
            rec["done"].append(int(done))
            rec["cog"].append(np.nan if cog is None else float(cog))
            # eps[0]: the reset before PPO(env); eps[1]: rollout()'s pre-loop reset
            rec["ep"].append(len(eps) - 3)
            return obs, reward, done, cog

        env.reset, env.step = reset, step
        with make_golden.quiet():
            env.reset(n_blue, n_red)
        torch.manual_seed(seed)
        agent = ppo.PPO(env, torch.device("cpu"))
        agent.add_param_noise = True
        agent.param_noise_clip_factor = clip
        weights = {}
        for pre, net in (("actor.", agent.actor), ("critic.", agent.critic)):
            weights.update({pre + k: v.detach().cpu().numpy().copy()
                            for k, v in net.state_dict().items()})

        def first_call(module, args):
            if fresh[0]:
                fresh[0] = False
                ep_actors.append({k: v.detach().cpu().numpy().copy()
                                  for k, v in module.state_dict().items()})

        hook = agent.actor.register_forward_pre_hook(first_call)
        ppo.Game = lambda: env
        with make_golden.quiet():
            b_obs, b_act, b_lp, b_rtg, lens, b_gs, b_val = agent.rollout(R, T, std)
        hook.remove()
        end = len(tape.vals)
        nb = len(env.blue_ships)
    finally:
        np.random.beta = np_beta
    eps = eps[2:]
    assert len(eps) == R and len(ep_actors) == R, (len(eps), len(ep_actors))
    for i, e in enumerate(eps):
        e["tape_end"] = eps[i + 1]["tape_start"] if i + 1 < len(eps) else end
    A = len(eps[0]["types"])
    steps = np.array(rec["ep"])
    n_steps = [int((steps == i).sum()) for i in range(R)]
    act = np.zeros((R, T, A, 4))
    f32 = np.zeros((R, T), np.uint8)
    rew = np.zeros((R, T, nb))
    done = np.ones((R, T), np.int32)
    cog = np.full((R, T), np.nan)
    k = 0
    for i in range(R):
        for t in range(n_steps[i]):
            act[i, t], f32[i, t] = rec["act"][k], rec["f32"][k]
            rew[i, t], done[i, t], cog[i, t] = rec["rew"][k], rec["done"][k], rec["cog"][k]
            k += 1
    names = list(ep_actors[0])
    stacked = {"ep_actor." + n: np.stack([ea[n] for ea in ep_actors]) for n in names}
    changed = [bool(any(not np.array_equal(ea[n], weights["actor." + n]) for ea in ep_actors)) for n in names]
    meta = dict(name=name, n_blue=n_blue, n_red=n_red, n_ls=0, landing_ops=False, trained_red=False,
                R=R, T=T, nb=nb, A=A, episodes=eps, n_steps=n_steps, gamma=float(agent.gamma),
                Db=env.observation_space, Dr=env.red_observation_space, std=std, clip=clip)
    out = dict(meta=np.array(json.dumps(meta)), tape=np.array(tape.vals, np.float64),
               act=act, act_f32=f32, rew=rew, done=done, cog=cog,
               batch_obs=b_obs.detach().cpu().numpy(), batch_act=np.asarray(b_act.detach().cpu().numpy()),
               batch_log_probs=b_lp.detach().cpu().numpy(),
               batch_values=b_val.detach().cpu().numpy(), batch_rtg=b_rtg.detach().cpu().numpy(),
               names=np.array(names), changed=np.array(changed), **weights, **stacked)
    path = os.path.join(OUT, f"rollout_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {R} episodes, steps {n_steps}, {len(tape.vals)} draws, changed "
          f"{[n for n, c in zip(names, changed) if c]}, unchanged {[n for n, c in zip(names, changed) if not c]}")


def main():
    if not os.path.isdir(make_golden.REF):
        print("reference not present; nothing to do")
        return
    # the reference's default exploration on a scripted-red 3v3 at its own spawns
    run("paramnoise", n_blue=3, n_red=3, R=3, T=6, seed=71, std=0.5, clip=0.05)


if __name__ == "__main__":
    main()
