#!/usr/bin/env python3
"""Golden vectors for the red-side MAPPO rollout (lnw.rollout.Rollout(side="red"))
taken from the reference's own `PPO.rollout` (ppo.py:421-671) with `SIDE ==
"red"`. TEST INFRASTRUCTURE ONLY: runs in the build container, where the
reference is mounted, through the stub harness of make_golden.py.

The harness is make_rollout_golden.run's (the env the loop steps is the one it
observes, the `random` modules and np.random.beta are a recording tape,
parameter noise is off), restated here with the four side settings on "red"
(game.SIDE, combatant.CUR_SIDE, landingship.CUR_SIDE, ppo.SIDE) and the side's
ship count taken from env.red_ships. What the reference's loop does then:
  * blue acts with `self.actor` in eval mode (ppo.py:519-526), nothing stored;
  * steps s <= 14: red takes its scripted rows (ppo.py:552-557) and stores only
    a log-probability (of the *blue* actor's get_dist on the red row); the
    observation, action and critic input rows stay zeros;
  * steps s > 14: red is sampled from `self.red_actor` in training mode and
    stored; the value is `self.red_critic` on the red rows (ppo.py:602-603).
It runs only 3v3 (ppo.py:556 feeds red rows to the blue actor, the scripted rows
are three) and only while no red ship is sunk after step 14 (ppo.py:547 calls
get_obs() on None).

Recorded as make_rollout_golden.py records, with rew [R, T, n_red] the red
rewards, plus the red critic's weights as `red_critic.*` (`actor.*` is the blue
actor, `red_actor.*` the learning one, `critic.*` the unused blue critic).

Seeds (searched on the CPU for rollouts that complete):
  redside_3v3         seed 31: n_steps [40, 40, 40, 40]; the first float32 step is
                      15 in every episode, 99 of 160 steps are float32
  redside_3v3_breaks  seed 49, boxes below: n_steps [3, 6, 1, 9, 6, 5] (every
                      `break` inside the scripted steps)

usage: python tests/golden/make_redside_golden.py [NAME ...]   (writes rollout_redside_*.npz)
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
TYPE_CODE = make_golden.TYPE_CODE


def run(name, *, n_blue, n_red, n_ls, landing_ops, trained_red, R, T, seed, boxes=None):
    game, combatant, landingship = make_golden.import_reference()
    import torch
    import network  # noqa: F401
    import ppo
    game.N_RED_LANDINGSHIP = n_ls
    game.LANDING_OPS = landing_ops
    game.TRAINED_RED = trained_red
    game.SIDE = "red"
    game.TACTICS = "aggressive"
    game.DISCRETE = combatant.DISCRETE = landingship.DISCRETE = False
    combatant.CUR_SIDE = landingship.CUR_SIDE = "red"
    ppo.TRAINED_RED = trained_red
    ppo.SIDE = "red"
    ppo.WANDA = False
    tape = make_golden.TapeRNG(seed)
    game.random = combatant.random = landingship.random = tape
    np_beta = np.random.beta
    np.random.beta = tape.beta
    try:
        env = game.Game()
        marks, rec = [], dict(act=[], f32=[], rew=[], done=[], cog=[], ep=[])
        eps = []
        real_reset, real_step = env.reset, env.step
        rng = np.random.default_rng(seed)
        grid = np.load(os.path.join(OUT, "grids.npz"))["grid100"]

        def reset(*a, **k):
            marks.append(len(tape.vals))
            if boxes is not None:
                env.grid = grid
                k = dict(k, grid=grid,
                         blue_ships=[combatant.Combatant("blue", "small", p, [], env) for p in
                                     make_golden._water_in_box(grid, rng, boxes[0], n_blue)],
                         red_ships=[combatant.Combatant("red", "large", p, [], env) for p in
                                    make_golden._water_in_box(grid, rng, boxes[1], n_red)])
            out = real_reset(*a, **k)
            ships = list(env.blue_ships) + list(env.red_ships)
            eps.append(dict(tape_start=marks[-1], ducting=env.ducting_factor,
                            spawn=[tuple(int(v) for v in s.position) for s in ships],
                            types=[TYPE_CODE[s.ship_type] for s in ships]))
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
        agent.add_param_noise = False
        weights = {}
        for pre, net in (("actor.", agent.actor), ("critic.", agent.critic),
                         ("red_actor.", agent.red_actor), ("red_critic.", agent.red_critic)):
            weights.update({pre + k: v.detach().cpu().numpy().copy()
                            for k, v in net.state_dict().items()})
        ppo.Game = lambda: env
        with make_golden.quiet():
            b_obs, b_act, b_lp, b_rtg, lens, b_gs, b_val = agent.rollout(R, T, 0.0)
        end = len(tape.vals)
        ns = len(env.red_ships)  # the side's ships
        rtg_flat = b_rtg.reshape(R * T * ns, 1)
        val_flat = b_val.detach().reshape(R * T * ns, 1)
        learner_gae = agent.gae(rtg_flat, val_flat).detach().cpu().numpy()
    finally:
        np.random.beta = np_beta
    eps = eps[2:]
    for i, e in enumerate(eps):
        e["tape_end"] = eps[i + 1]["tape_start"] if i + 1 < len(eps) else end
    A = len(eps[0]["types"])
    steps = np.array(rec["ep"])
    n_steps = [int((steps == i).sum()) for i in range(R)]
    act = np.zeros((R, T, A, 4))
    f32 = np.zeros((R, T), np.uint8)
    rew = np.zeros((R, T, ns))
    done = np.ones((R, T), np.int32)
    cog = np.full((R, T), np.nan)
    k = 0
    for i in range(R):
        for t in range(n_steps[i]):
            act[i, t], f32[i, t] = rec["act"][k], rec["f32"][k]
            rew[i, t], done[i, t], cog[i, t] = rec["rew"][k], rec["done"][k], rec["cog"][k]
            k += 1
    meta = dict(name=name, side="red", n_blue=n_blue, n_red=n_red, n_ls=n_ls, landing_ops=landing_ops,
                boxes=boxes, trained_red=trained_red, R=R, T=T, nb=A - ns, nr=ns, A=A, episodes=eps,
                n_steps=n_steps, warmup=15, gamma=float(agent.gamma), Db=env.observation_space,
                Dr=env.red_observation_space)
    out = dict(meta=np.array(json.dumps(meta)), tape=np.array(tape.vals, np.float64),
               act=act, act_f32=f32, rew=rew, done=done, cog=cog,
               batch_obs=b_obs.detach().cpu().numpy(), batch_actions=b_act.detach().cpu().numpy(),
               batch_log_probs=b_lp.detach().cpu().numpy(),
               batch_values=b_val.detach().cpu().numpy(), batch_rtg=b_rtg.detach().cpu().numpy(),
               learner_gae=learner_gae, **weights)
    path = os.path.join(OUT, f"rollout_{name}.npz")
    np.savez_compressed(path, **out)
    first_f32 = [int(np.argmax(f32[i])) if f32[i].any() else None for i in range(R)]
    print(f"{path}: {R} episodes, steps {n_steps}, {len(tape.vals)} draws, "
          f"float32 steps {int(f32.sum())} / {int(sum(n_steps))}, first float32 step {first_f32}, done at "
          f"{[int(np.argmin(done[i])) if (done[i] == 0).any() else None for i in range(R)]}")


BREAK_BOXES = (((37, 43), (45, 53)), ((51, 57), (47, 55)))


def main(only=None):
    """Both scenarios, or only the names given on the command line."""
    if not os.path.isdir(make_golden.REF):
        print("reference not present; nothing to do")
        return
    # 3v3 at the reference's spawns (game.py:551-585): every episode runs all 40
    # steps, 15 scripted ones and 25 sampled ones, some of the latter float64
    # (a blue ship sunk); no red ship is lost after step 14
    if only is None or "redside_3v3" in only:
        run("redside_3v3", n_blue=3, n_red=3, n_ls=0, landing_ops=False, trained_red=True,
            R=4, T=40, seed=31)
    # fleets 8-20 cells apart: every episode ends inside the scripted steps
    if only is None or "redside_3v3_breaks" in only:
        run("redside_3v3_breaks", n_blue=3, n_red=3, n_ls=0, landing_ops=False, trained_red=True,
            R=6, T=40, seed=49, boxes=BREAK_BOXES)


if __name__ == "__main__":
    main(sys.argv[1:] or None)
