#!/usr/bin/env python3
"""Golden vectors for the DDQN learner step of lnw.qlearn (QLearner).

Drives the reference's own DDQN.optimize() (ddqn.py:153-247) through the stub
harness of make_golden.py (this container only): a DDQN over an env stub with
observation rows of length D, exactly BATCH_SIZE = 64 transitions pushed into
its replay memory (so the sample is the whole memory, in some order: loss and
gradients do not depend on it beyond rounding), rewards float64, done int.
Three sets:
  blue   SIDE = "blue", D = 68: policy forward and backward on batch statistics;
  red    SIDE = "red", D = 68: the reference leaves red_policy_net in eval()
         (ddqn.py:212, 222), so its forward and backward use the running
         statistics, perturbed here as make_qnet_golden.perturb does;
  wide   SIDE = "blue", D = 84 (n_in = 47).
Per set: both networks' state_dict before and after the call, the 64
transitions, the loss (recomputed from the recorded tensors as the reference
computes it) and the gradients optimize() leaves in .grad (clamped to [-1, 1];
the generator asserts none reaches 1).
Conditions on the inputs, asserted here: every one of the 57 outputs is chosen
by at least one row's action; at least 4 rows have a terrain window in which a
pool window of the policy's first ReLU map holds an exact tie at a positive
maximum (constant windows), so max pool's first-maximum rule runs; a few rows
have done = 0.
Writes tests/golden/qlearn.npz.

usage: python tests/golden/make_qlearn_golden.py
"""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402
from make_policy_golden import random_obs  # noqa: E402
from make_qnet_golden import perturb  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "qlearn.npz")
B = 64


def perturb_affine(torch, model):
    with torch.no_grad():
        for m in (model.norm1, model.norm2):
            m.weight.add_(0.1 * torch.randn_like(m.weight))
            m.bias.add_(0.1 * torch.randn_like(m.bias))


def tie_rows(torch, F, net, state, running):
    """Rows whose first ReLU map has a pool window with an exact tie at a
    positive maximum."""
    with torch.no_grad():
        z = net.conv1(torch.tensor(state[:, :49]).reshape(-1, 1, 7, 7))
        if running:
            z = F.batch_norm(z, net.norm1.running_mean, net.norm1.running_var, net.norm1.weight, net.norm1.bias,
                             False, 0.0, 1e-5)
        else:
            z = F.batch_norm(z, None, None, net.norm1.weight, net.norm1.bias, True, 0.0, 1e-5)
        a = F.relu(z)[:, :, :6, :6].reshape(-1, 5, 3, 2, 3, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 5, 9, 4)
        mx = a.max(-1, keepdim=True).values
        tie = ((a == mx).sum(-1) > 1) & (mx[..., 0] > 0)
        return tie.any(-1).any(-1).numpy()


def one_set(torch, ddqn, side, D, seed, prefix, out):
    """Record one set; False (nothing recorded) if a gradient element reaches
    the clamp with this seed's inputs."""
    import torch.nn.functional as F
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    ddqn.WANDA = False
    ddqn.SIDE = side
    assert ddqn.BATCH_SIZE == B
    env = types.SimpleNamespace(observation_space=D, red_observation_space=D)
    agent = ddqn.DDQN(env, torch.device("cpu"))
    pol, tgt = ((agent.policy_net, agent.target_net) if side == "blue"
                else (agent.red_policy_net, agent.red_target_net))
    for net in (pol, tgt):
        if side == "red":
            perturb(torch, net)
        else:
            perturb_affine(torch, net)
    state, nxt = random_obs(rng, B, D), random_obs(rng, B, D)
    for i in range(6):  # constant terrain windows: exact ties inside every pool window
        state[i, :49] = np.float32((40 + 35 * i) / 255.0)
    action = np.stack([np.arange(B) % 2, np.arange(B) % 5, rng.permutation(B) % 50], 1).astype(np.int64)
    assert len(set(action[:, 0])) == 2 and len(set(action[:, 1])) == 5 and len(set(action[:, 2])) == 50
    reward = rng.normal(0.0, 0.5, B)
    done = np.ones(B, np.int64)
    done[rng.choice(B, 5, replace=False)] = 0
    ties = tie_rows(torch, F, pol, state, side == "red")
    print(prefix, "rows with a positive exact pool tie:", int(ties.sum()))
    assert ties.sum() >= 4, ties.sum()
    for i in range(B):
        agent.memory.push(torch.tensor(state[i:i + 1]), torch.tensor(action[i:i + 1]), torch.tensor(nxt[i:i + 1]),
                          torch.tensor(reward[i:i + 1], dtype=torch.float64), torch.tensor(done[i:i + 1]))
    before = {n: {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
              for n, net in (("policy", pol), ("target", tgt))}
    # the loss as optimize() computes it, from the recorded tensors and the state before the call
    import copy
    p2, t2 = copy.deepcopy(pol), copy.deepcopy(tgt)
    t2.train()
    p2.train(side == "blue")
    with torch.no_grad():
        rad, msl, mov = t2(torch.tensor(nxt))
        nv = torch.stack([rad.max(1).values, msl.max(1).values, mov.max(1).values], 1)
        y = (ddqn.GAMMA * nv * torch.tensor(done).unsqueeze(1) + torch.tensor(reward).unsqueeze(1)).type(torch.float32)
        rad, msl, mov = p2(torch.tensor(state))
        a = torch.tensor(action)
        qs = torch.cat((rad.gather(1, a[:, 0:1]), msl.gather(1, a[:, 1:2]), mov.gather(1, a[:, 2:3])), 1)
        loss = torch.nn.MSELoss()(qs, y)
    agent.optimize()
    assert pol.training == (side == "blue")
    grads = {k: p.grad.detach().numpy().copy() for k, p in pol.named_parameters()}
    gmax = max(float(np.abs(g).max()) for g in grads.values())
    print(prefix, "loss", float(loss), "largest |grad|", gmax,
          {k: float(np.abs(g).max()) for k, g in grads.items() if np.abs(g).max() > 0.5})
    if not gmax < 1.0:  # the clamp must be inactive: .grad is then the raw gradient
        return False
    after = {n: {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
             for n, net in (("policy", pol), ("target", tgt))}
    if side == "red":
        for k in ("norm1.running_mean", "norm1.running_var", "norm2.running_mean", "norm2.running_var",
                  "norm1.num_batches_tracked"):
            assert np.array_equal(before["policy"][k], after["policy"][k]), k
    out.update({f"{prefix}_state": state, f"{prefix}_next_state": nxt, f"{prefix}_action": action,
                f"{prefix}_reward": reward, f"{prefix}_done": done, f"{prefix}_loss": np.float32(loss.item()),
                f"{prefix}_gamma": np.float64(ddqn.GAMMA), f"{prefix}_lr": np.float64(agent.lr),
                f"{prefix}_y": y.numpy(), f"{prefix}_qs": qs.numpy(), f"{prefix}_tie_rows": ties})
    for n in ("policy", "target"):
        out.update({f"{prefix}.{n}.before.{k}": v for k, v in before[n].items()})
        out.update({f"{prefix}.{n}.after.{k}": v for k, v in after[n].items()})
    out.update({f"{prefix}.grad.{k}": v for k, v in grads.items()})
    out[f"{prefix}_seed"] = np.int64(seed)
    return True


def main():
    make_golden.import_reference()
    import torch
    import ddqn
    out = {}
    # seeds 1, 2, ...: the first whose gradients all stay inside the clamp is recorded
    for side, D, prefix in (("blue", 68, "blue"), ("red", 68, "red"), ("blue", 84, "wide")):
        for seed in range(1, 64):
            if one_set(torch, ddqn, side, D, seed, prefix, out):
                break
        else:
            raise AssertionError(f"no seed kept the {prefix} gradients inside the clamp")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
