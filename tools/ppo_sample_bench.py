#!/usr/bin/env python3
"""Timing of the learner's minibatch draw: PPOLearner.minibatch (lnw_ppo_sample:
keys, radix select, compaction, sort, gather, one chain of launches) beside the
path it stands next to, rows(out, sample(out, B)) (torch.multinomial on the
normalised priorities and five torch gathers), on the same rollout-shaped
buffers, and the chain captured once in a torch.cuda.graph and replayed
(minibatch_graph: without the host's launch cost).

The arms alternate inside one process: every round times `--iters` draws of each
after `--warmup` untimed ones. Two clocks: device events around the draws (the
HIP arms; for the torch arm they include whatever host round trips
torch.multinomial makes, during which the device idles), and the wall clock
around a torch.cuda.synchronize() for every arm. Reported per batch size: the
median over rounds and the min-max spread over rounds; one JSON line per batch
size on stdout.

usage: python tools/ppo_sample_bench.py [--rows 5242880] [--batch 64 4096 131072] [--rounds 7] [--iters 10]
       rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ppo_sample_bench.py --batch 64 --rounds 2 --no-torch --no-graph
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "littoral-naval-warfare-marl_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5242880, help="rollout rows: envs x steps x ships")
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 4096, 131072])
    ap.add_argument("--ships", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the rows(out, sample(out, B)) arm")
    ap.add_argument("--no-graph", action="store_true", help="skip the graph-replay arm")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ppo_sample_bench needs a GPU")
    from lnw.ppolearn import PPOLearner
    from lnw.rollout import BatchedActor, BatchedCritic
    dev = torch.device("cuda", 0)
    n, N = args.ships, args.rows
    D = 4 * n + 52
    if N % n:
        raise SystemExit("--rows must be a multiple of --ships")
    torch.manual_seed(0)
    actor, critic = BatchedActor.for_obs(D), BatchedCritic(n * D)
    out = dict(obs=torch.zeros((N // n, n, D), device=dev), rtg=torch.randn(N, device=dev) * 2.0,
               actions=torch.rand((N, 4), device=dev), log_probs=torch.randn((N, 4), device=dev) * 0.3 - 1.0,
               values=torch.randn(N // n, device=dev) * 0.3)
    L = PPOLearner(actor, critic, impl="hip", device=dev)
    for B in args.batch:
        arms = [("minibatch", lambda: L.minibatch(out, B))]
        if not args.no_graph:
            L.minibatch(out, B)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                L.minibatch(out, B)
            arms.append(("minibatch_graph", graph.replay))
        if not args.no_torch:
            arms.append(("sample_rows", lambda: L.rows(out, L.sample(out, B))))
        for _, f in arms:
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
        dev_us, wall_us = {k: [] for k, _ in arms}, {k: [] for k, _ in arms}
        for _ in range(args.rounds):
            for k, f in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                for _ in range(args.iters):
                    f()
                e1.record()
                torch.cuda.synchronize()
                wall_us[k].append((time.perf_counter() - t0) * 1e6 / args.iters)
                dev_us[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        res = dict(rows=N, batch=B, ships=n, rounds=args.rounds, iters=args.iters,
                   device=torch.cuda.get_device_name(0))
        for name, t in (("event_us", dev_us), ("wall_us", wall_us)):
            for k, v in t.items():
                res[f"{k}_{name}"] = dict(median=round(statistics.median(v), 1), min=round(min(v), 1),
                                          max=round(max(v), 1))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
