"""One rank of the sharded-training test (tests/test_gpu_ppo_dist.py::
test_two_ranks_train_as_one): a Rollout over this rank's env_range share of the
global envs (env_id_base = its first global env, keyed sampling, acting from the
learner's flat vector), then rollout -> 3 x (minibatch_dist(64) -> step) ->
rollout -> 2 more steps; saves the learner's state, the losses and the drawn
global rows for the parent. With WORLD_SIZE=1 the same sequence on all envs
through the plain minibatch(): the one-rank run the others must equal.
Child process: WORLD_SIZE / RANK / MASTER_* in the environment, every rank on
cuda:0; backend gloo, or nccl (RCCL: one rank under torch.distributed.run, the
collectives on device tensors). minibatch_dist runs whenever there is a
process group.

usage: _ppo_dist_rank.py OUT.npz TOTAL_ENVS plain|noise [gloo|nccl]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "littoral-naval-warfare-marl_amd")]

BLUE = [(6, 61), (10, 81), (8, 70), (11, 58)]
RED = [(98, 48), (98, 52), (98, 56), (96, 52)]
T, BATCH = 8, 64


def main():
    out, total, mode = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    import torch
    from lnw import dist
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    from lnw.ppolearn import PPOLearner
    from lnw.rollout import BatchedActor, BatchedCritic, Rollout
    ws, rank, _ = dist.init(sys.argv[4] if len(sys.argv) > 4 else "gloo")
    grouped = dist.size() is not None
    torch.cuda.set_device(0)
    lo, hi = dist.env_range(total, ws, rank)
    sc = Scenario(landing_ops=False, tactics="aggressive", side="blue", trained_red=False, auto_reset=True,
                  episode_steps=40)
    g = BatchedGame(hi - lo, ["small"] * 4, ["large"] * 4, scenario=sc, device=0, seed=77, env_id_base=lo,
                    reward_dtype=torch.float64)
    g.set_variant(True)
    torch.manual_seed(0)
    actor = BatchedActor.for_obs(g.Db).cuda()
    critic = BatchedCritic(g.Db * g.nb).cuda()
    learner = PPOLearner(actor, critic, lr=1e-3, sample_seed=19)
    kw = dict(param_noise=(0.5, 0.05), envs_per_member=11) if mode == "noise" else {}
    r = Rollout(g, actor, critic, steps=T, noise=0.05, keyed_seed=11, theta=learner.theta_actor, **kw)
    # melee-box spawns: contact and fire inside the 8 steps
    g.reset(positions=BLUE + RED, box=((40, 40), (57, 65)))
    row_base = lo * T * g.nb
    losses, rows = [], []
    for steps in (3, 2):
        learner.export()  # (the rollout's values come from the critic module)
        o = r.run()
        for _ in range(steps):
            if grouped:
                b = learner.minibatch_dist(o, BATCH, row_base=row_base)
                rows.append(b["global_row"].cpu().numpy())
            else:
                b = learner.minibatch(o, BATCH)
                rows.append(b["index"].cpu().numpy())
            losses.append(torch.stack(learner.step(b)).cpu().numpy())
    torch.cuda.synchronize()
    state = {k: getattr(learner, k).cpu().numpy() for k in (
        "theta_actor", "theta_critic", "m_actor", "v_actor", "m_critic", "v_critic", "step_actor", "step_critic",
        "draw", "nbt", "sample_status")}
    dist.barrier()
    np.savez(out, lo=lo, hi=hi, backend=str(dist.backend()), losses=np.stack(losses), rows=np.stack(rows), **state)
    g.close()
    dist.finalize()


if __name__ == "__main__":
    main()
