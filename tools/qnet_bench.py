#!/usr/bin/env python3
"""Device-event timing of the DDQN acting kernel (lnw_qnet_act) beside the MAPPO
policy kernel and the torch restatement, on the same observation rows.

  (a) lnw_qnet_act            conv head + one 57 x n_in layer, argmax, keyed eps-greedy
  (b) lnw_policy_act          conv head + LayerNorm + 64/64/32/8 MLP, keyed sample, log-prob
  (c) BatchedQNet.act(impl="torch")  torch conv / norm / pool / linear / argmax / where
                                      + the keyed uniform fill

The three alternate inside one process: every round times `--iters` launches of
each between device events, after `--warmup` untimed launches of each. Reported
per shape: the median over rounds, the min-max spread over rounds, and the
kernel's algorithmic bytes per row (4 D read; 16 written into the step's action
array, 32 with the replay row). One JSON line per shape on stdout.

usage: python tools/qnet_bench.py [--envs 32768 65536] [--rounds 7] [--iters 20] [--warmup 5]
       rocprofv3 --kernel-trace --stats -d <dir> -- python tools/qnet_bench.py --rounds 2
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[32768, 65536])
    ap.add_argument("--ships", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--no-torch", action="store_true", help="skip (c)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qnet_bench needs a GPU: timings are device-event times")
    from lnw import _abi
    from lnw.qlearn import BatchedQNet
    from lnw.rollout import BatchedActor
    L = _abi.load()
    dev = torch.device("cuda", 0)
    n = args.ships
    D = 4 * n + 52
    torch.manual_seed(0)
    qnet = BatchedQNet.for_obs(D).to(dev)
    actor = BatchedActor.for_obs(D).to(dev)
    qp, pp = qnet.packed(), actor.packed_policy()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for E in args.envs:
        obs = torch.rand((E, n, D), device=dev)
        obs[..., :49] = torch.randint(0, 256, (E, n, 49), device=dev) / 255.0
        alive = torch.ones((n, E), dtype=torch.uint8, device=dev)
        full_i = torch.zeros((E, n, 4), dtype=torch.int32, device=dev)
        act_i = torch.zeros((E, n, 4), dtype=torch.int32, device=dev)
        full_d = torch.zeros((E, n, 4), dtype=torch.float64, device=dev)
        act_f = torch.zeros((E, n, 4), dtype=torch.float32, device=dev)
        logp = torch.zeros((E, n, 4), dtype=torch.float32, device=dev)
        qa = _abi.QnetArgs()
        qa.obs, qa.E, qa.n, qa.D, qa.own0, qa.A = obs.data_ptr(), E, n, D, 0, n
        qa.params, qa.mode, qa.eps, qa.seed = qp.data_ptr(), _abi.LNW_QNET_EPS_GREEDY, args.eps, 1
        qa.alive, qa.full = alive.data_ptr(), full_i.data_ptr()
        qa.act_out, qa.act_env_stride = act_i.data_ptr(), 4 * n
        pa = _abi.PolicyArgs()
        pa.obs, pa.E, pa.n, pa.D, pa.own0, pa.A = obs.data_ptr(), E, n, D, 0, n
        pa.params, pa.seed, pa.T, pa.alive = pp.data_ptr(), 1, 1, alive.data_ptr()
        pa.full, pa.act_out, pa.logp_out = full_d.data_ptr(), act_f.data_ptr(), logp.data_ptr()
        pa.act_env_stride = 4 * n
        step = [0]

        def run_a():
            qa.slot = step[0]
            _abi.check(L.lnw_qnet_act(C.byref(qa), stream))

        def run_b():
            pa.t = 0
            _abi.check(L.lnw_policy_act(C.byref(pa), stream))

        def run_c():
            qnet.act(obs, eps=args.eps, seed=1, slot=step[0], impl="torch")

        arms = [("qnet_act", run_a), ("policy_act", run_b)]
        if not args.no_torch:
            arms.append(("torch", run_c))
        for _, f in arms:
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k, _ in arms}
        for _ in range(args.rounds):
            for k, f in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    f()
                    step[0] += 1
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        res = dict(envs=E, ships=n, obs_dim=D, rows=E * n, rounds=args.rounds, iters=args.iters,
                   bytes_per_row=dict(read=4 * D, written=32), device=torch.cuda.get_device_name(0))
        for k, v in times.items():
            res[k + "_us"] = dict(median=round(statistics.median(v), 2), min=round(min(v), 2),
                                  max=round(max(v), 2))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
