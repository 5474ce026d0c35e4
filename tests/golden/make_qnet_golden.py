#!/usr/bin/env python3
"""Golden vectors for the batched Q-network of lnw.qlearn (DDQN acting).

Imports the reference's network.py through the stub harness of make_golden.py
(this container only) and records, for seeded random weights and inputs, what
network.DMLP (network.py:246-305) returns for one state at a time, the way the
DDQN loop calls it (ddqn.py:303: batch-1 calls of a network that is never put
in eval(), so BatchNorm uses that one sample's statistics) — the 57 ReLU'd
Q-values in radar, attack, movement order and the three torch.argmax indices —
and the same in eval mode (running statistics). Three parameter sets:
  net   DMLP(68) (a 4-ship side), 96 rows, BatchNorm affine parameters and
        running statistics perturbed so that both modes are exercised;
  dead  the same with radar.bias and attack.bias driven to -10: those heads are
        all zero after the ReLU and the expected index is 0 (first maximum);
  wide  DMLP(84) (an 8-ship side, n_in = 47), 32 rows.
A (row, head) pair is a near tie when the reference's own top two ReLU'd values
are less than 1e-3 apart, unless every pre-activation of the head is below
-1e-3 (a head that is robustly all zero: index 0 exactly). The generator
asserts that at most 2 % of the pairs of every set and head are near ties — a
condition on the inputs, not a tolerance — and records the mask.
Writes tests/golden/qnet.npz (weights as arrays keyed by state_dict name).

usage: python tests/golden/make_qnet_golden.py
"""
import copy
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402
from make_policy_golden import random_obs  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "qnet.npz")
TIE = 1e-3
HEADS = ("radar", "attack", "movement")


def record(torch, model, obs):
    """Per-sample outputs of `model` in its current mode: q [n, 57], argmax
    [n, 3] int64, near-tie mask [n, 3]."""
    pre = {}
    hooks = [getattr(model, h).register_forward_hook(lambda m, i, o, h=h: pre.__setitem__(h, o.detach()))
             for h in HEADS]
    q, arg, tie = [], [], []
    with torch.no_grad():
        for i in range(obs.shape[0]):
            out = model(torch.tensor(obs[i]))  # (radar, attack, movement)
            q.append(np.concatenate([o.numpy().reshape(-1) for o in out]))
            arg.append([int(torch.argmax(o).item()) for o in out])
            row = []
            for h, o in zip(HEADS, out):
                top = np.sort(o.numpy().reshape(-1))[::-1]
                row.append(bool(top[0] - top[1] < TIE and pre[h].max().item() > -TIE))
            tie.append(row)
    for h in hooks:
        h.remove()
    return np.stack(q).astype(np.float32), np.asarray(arg, np.int64), np.asarray(tie, bool)


def one_set(torch, model, obs, prefix, out, strict=True):
    """Record one parameter set into `out`; False (nothing recorded) if the rows
    miss the near-tie condition and strict is off."""
    model = copy.deepcopy(model)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    ev = copy.deepcopy(model)
    ev.eval()
    ev_q, ev_arg, ev_tie = record(torch, ev, obs)
    model.train()
    tr_q, tr_arg, tr_tie = record(torch, model, obs)  # (updates the running statistics: sd was taken first)
    for name, tie in (("train", tr_tie), ("eval", ev_tie)):
        frac = tie.mean(0)
        print(prefix, name, "near-tie fraction per head:", frac)
        if not (frac <= 0.02).all():
            assert not strict, (prefix, name, frac)
            return False
    out.update({f"{prefix}_obs": obs, f"{prefix}_tr_q": tr_q, f"{prefix}_tr_arg": tr_arg,
                f"{prefix}_tr_tie": tr_tie, f"{prefix}_ev_q": ev_q, f"{prefix}_ev_arg": ev_arg,
                f"{prefix}_ev_tie": ev_tie})
    out.update({f"{prefix}.{k}": v for k, v in sd.items()})
    return True


def perturb(torch, model):
    """BatchNorm affine parameters and running statistics away from their
    initial 1 / 0 / 0 / 1, so a wrong parameter order or mode shows."""
    with torch.no_grad():
        for m in (model.norm1, model.norm2):
            m.weight.add_(0.1 * torch.randn_like(m.weight))
            m.bias.add_(0.1 * torch.randn_like(m.bias))
            m.running_mean.add_(0.1 * torch.randn_like(m.running_mean))
            m.running_var.copy_(0.5 + torch.rand_like(m.running_var))


def main():
    make_golden.import_reference()
    import torch
    import network
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    out = {}
    net = network.DMLP(68)
    perturb(torch, net)
    obs = random_obs(rng, 96, 68)
    dead = copy.deepcopy(net)
    with torch.no_grad():
        dead.radar.bias.fill_(-10.0)
        dead.attack.bias.fill_(-10.0)
    one_set(torch, net, obs, "net", out)
    one_set(torch, dead, obs, "dead", out)
    assert (out["dead_tr_q"][:, :7] == 0).all() and (out["dead_tr_arg"][:, :2] == 0).all()
    assert (out["dead_ev_q"][:, :7] == 0).all() and (out["dead_ev_arg"][:, :2] == 0).all()
    wide = network.DMLP(84)
    perturb(torch, wide)
    # 32 rows admit no near tie at all under the 2 % condition: rows from their
    # own streams, seeds 1, 2, ... — the first set that meets it is recorded
    for seed in range(1, 64):
        if one_set(torch, wide, random_obs(np.random.default_rng(seed), 32, 84), "wide", out, strict=False):
            out["wide_seed"] = np.int64(seed)
            break
    else:
        raise AssertionError("no wide row set met the near-tie condition")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes",
          {k: v.shape for k, v in out.items() if "." not in k})


if __name__ == "__main__":
    main()
