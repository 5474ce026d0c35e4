#!/usr/bin/env python3
"""Device-event timing of parameter-noise exploration in the MAPPO rollout at
config 5's shape (bench.py mappo_rollout: 32 768 envs, 4v4, 40 steps, scripted
red, contact variant, HIP-graph replay): the plain rollout beside
Rollout(param_noise=(0.5, 0.05), envs_per_member=128) — 256 members, one policy
block and one parameter set each — on one game, from the same reset state.

The two captured graphs alternate inside one process: every round resets the
envs (untimed) and times one replay of each between device events, after
`--warmup` untimed rounds. Reported: median and min-max over rounds of a whole
rollout, the difference per step (a step's one blue policy launch is the only
launch that changes), and the one lnw_actor_perturb launch of a rollout on its
own (all members' sets from one flat vector). One JSON line on stdout. The
yardstick is the plain rollout of the same process.

usage: python tools/param_noise_bench.py [--envs 32768] [--steps 40] [--group 128] [--rounds 9] [--warmup 2]
       rocprofv3 --kernel-trace --stats -d <dir> -- python tools/param_noise_bench.py --rounds 2
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "littoral-naval-warfare-marl_amd"))

REF_BLUE = [(6, 61), (10, 81), (8, 70), (11, 58)]
REF_RED = [(98, 48), (98, 52), (98, 56), (96, 52)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--group", type=int, default=128, help="envs per member")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("param_noise_bench needs a GPU: timings are device-event times")
    from lnw import _abi
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    from lnw.ppolearn import actor_slices, pack
    from lnw.rollout import BatchedActor, BatchedCritic, Rollout
    E, T, G = args.envs, args.steps, args.group
    sc = Scenario(landing_ops=False, tactics="aggressive", side="blue", trained_red=False, auto_reset=True,
                  episode_steps=40)
    g = BatchedGame(E, ["small"] * 4, ["large"] * 4, scenario=sc, device=0, seed=77)
    g.set_variant(True)
    torch.manual_seed(0)
    actor = BatchedActor.for_obs(g.Db).cuda()
    critic = BatchedCritic(g.Db * g.nb).cuda()
    arms = {"plain": Rollout(g, actor, critic, steps=T, noise=0.05, seed=5),
            "param_noise": Rollout(g, actor, critic, steps=T, noise=0.05, seed=5, param_noise=(0.5, 0.05),
                                   envs_per_member=G)}
    for r in arms.values():
        g.reset(positions=REF_BLUE + REF_RED)
        r.capture()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for rnd in range(args.warmup + args.rounds):
        for k, r in arms.items():
            g.reset(positions=REF_BLUE + REF_RED)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r.replay()
            e1.record()
            e1.synchronize()
            if rnd >= args.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    # the rollout's one lnw_actor_perturb launch on its own
    L = _abi.load()
    M = -(-E // G)
    floats = int(L.lnw_policy_packed_floats(g.Db))
    theta = pack(actor, actor_slices(g.Db - 37)).cuda()
    sets = torch.empty((M, floats), device="cuda")
    call = torch.zeros(1, dtype=torch.int64, device="cuda")
    pt = _abi.ActorPerturbArgs()
    pt.theta, pt.D, pt.T, pt.member0, pt.members = theta.data_ptr(), g.Db, T, 0, M
    pt.packed_out, pt.member_stride = sets.data_ptr(), floats
    pt.noise_dev, pt.seed, pt.call_dev = arms["param_noise"].param_noise.data_ptr(), 5, call.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    perturb = []
    for rnd in range(args.warmup + args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            _abi.check(L.lnw_actor_perturb(C.byref(pt), stream))
        e1.record()
        e1.synchronize()
        if rnd >= args.warmup:
            perturb.append(e0.elapsed_time(e1) * 1e3 / 10)
    g.close()

    def stat(v):
        return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))

    res = dict(envs=E, steps=T, envs_per_member=G, members=M, set_kb=round(floats * 4 / 1024, 1),
               rounds=args.rounds, device=torch.cuda.get_device_name(0),
               plain_rollout_us=stat(times["plain"]), param_noise_rollout_us=stat(times["param_noise"]),
               extra_us_per_step=round((statistics.median(times["param_noise"]) -
                                        statistics.median(times["plain"])) / T, 2),
               extra_percent=round(100.0 * (statistics.median(times["param_noise"]) /
                                            statistics.median(times["plain"]) - 1.0), 2),
               actor_perturb_us=stat(perturb))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
