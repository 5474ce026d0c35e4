#!/usr/bin/env python3
"""Timing of the DDQN replay minibatch: QCollector.minibatch (lnw_ppo_sample over
the ring's priorities, then lnw_replay_pack: one chain of launches), the same
chain captured once in a torch.cuda.graph and replayed, and the path it stands
next to, learner.rows(c.sample(B)) (torch.randint with replacement, five
advanced-index gathers, the reshapes and copies of rows()), on one synthetic
ring of --envs x --cap transitions; lnw_replay_pack alone with its achieved
bandwidth (bytes read + written over the kernel's time); and QCollector.step()
of a real DISCRETE game with and without priorities (the cost of the
lnw_replay_mark launch).

The arms alternate inside one process: every round times `--iters` calls of each
after `--warmup` untimed ones, with device events around them (for the torch arm
they include whatever host round trips it makes, during which the device
idles). Reported: the median over rounds and the min-max spread over rounds; one
JSON line per batch size on stdout, and one for the collector step.

usage: python tools/replay_bench.py [--envs 65536] [--cap 64] [--batch 64 4096 131072] [--rounds 7] [--iters 10]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "littoral-naval-warfare-marl_amd"))


def timed(arms, rounds, iters, warmup):
    """{arm: [us per call, one per round]} by device events, the arms alternating."""
    for _, f in arms:
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k, _ in arms}
    for _ in range(rounds):
        for k, f in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    return us


def summary(v):
    return dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))


def synthetic_collector(E, cap, n, D, dev):
    """A QCollector over a full synthetic ring, without a game: what sample() and
    minibatch() read."""
    from lnw.qlearn import QCollector
    c = QCollector.__new__(QCollector)
    c.g = types.SimpleNamespace(E=E, device=dev, env_id_base=0)
    c.cap, c.n, c.D, c.steps = cap, n, D, cap
    c.state = torch.zeros((cap, E, n, D), device=dev)
    c.next_state = torch.zeros((cap, E, n, D), device=dev)
    c.action = torch.zeros((cap, E, n, 4), dtype=torch.int32, device=dev)
    c.reward = torch.randn((cap, E, n), device=dev)
    c.done = torch.ones((cap, E), dtype=torch.int32, device=dev)
    c.priority_mode, c.sample_seed, c.impl = "reward", 0, "hip"
    c.priority = c.reward.abs().sum(2).t().contiguous()
    c.draw = torch.zeros(1, dtype=torch.int64, device=dev)
    c.sample_status = torch.zeros(1, dtype=torch.int64, device=dev)
    c._replay_buf = {}
    return c


def step_cost(args, dev):
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    from lnw.qlearn import BatchedQNet, QCollector
    sc = Scenario(discrete=True, landing_ops=False, trained_red=False, auto_reset=True, episode_steps=40)
    arms, games = [], []
    for name, pr in (("step", None), ("step_priority", "reward")):
        g = BatchedGame(args.step_envs, ["small"] * 4, ["large"] * 4, scenario=sc, seed=3)
        g.reset(positions=[(6, 61), (10, 81), (8, 70), (11, 58), (98, 48), (98, 52), (98, 56), (96, 52)])
        torch.manual_seed(1)
        c = QCollector(g, BatchedQNet.for_obs(g.Db).cuda(), red="random", capacity=16, seed=1, priority=pr)
        arms.append((name, lambda c=c: c.step(eps=0.5)))
        games.append(g)
    us = timed(arms, args.rounds, args.iters, args.warmup)
    res = dict(step_envs=args.step_envs, rounds=args.rounds, iters=args.iters)
    res.update({f"{k}_event_us": summary(v) for k, v in us.items()})
    print(json.dumps(res), flush=True)
    for g in games:
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--ships", type=int, default=4)
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 4096, 131072])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-envs", type=int, default=4096, help="envs of the collector-step measurement (0: skip)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("replay_bench needs a GPU")
    from lnw import replay
    from lnw.qlearn import BatchedQNet, QLearner
    dev = torch.device("cuda", 0)
    n = args.ships
    D = 4 * n + 52  # a DISCRETE n v n game's observation row
    c = synthetic_collector(args.envs, args.cap, n, D, dev)
    L = QLearner(BatchedQNet.for_obs(D), device=dev)
    for B in args.batch:
        c.minibatch(B)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            c.minibatch(B)
        buf = c._replay_buf[("local", B)]
        ring = c.ring()
        arms = [("minibatch", lambda: c.minibatch(B)), ("minibatch_graph", graph.replay),
                ("sample_rows", lambda: L.rows(c.sample(B))),
                ("pack", lambda: replay.pack(ring, buf["global_row"], xbuf=buf["xbuf"], index_out=buf["ring_index"]))]
        us = timed(arms, args.rounds, args.iters, args.warmup)
        res = dict(envs=args.envs, cap=args.cap, transitions=args.envs * args.cap, batch=B, ships=n, D=D,
                   rounds=args.rounds, iters=args.iters, device=torch.cuda.get_device_name(0))
        res.update({f"{k}_event_us": summary(v) for k, v in us.items()})
        moved = 2 * 4 * buf["xbuf"].numel()
        res["pack_bytes"] = moved
        res["pack_GBps"] = round(moved / statistics.median(us["pack"]) / 1e3, 1)
        print(json.dumps(res), flush=True)
    if args.step_envs:
        step_cost(args, dev)


if __name__ == "__main__":
    main()
