"""Shared by the tests that compare a whole batch with orc_fullsize_range
(test_gpu_fullsize.py, test_gpu_team_sizes.py): the device-side run that
reduces every (step, env) to the observation hash sum_k bits(obs[k]) * mult[k]
mod 2^64 (_spawns.hash_mult), and the comparison, with _device's tolerances."""
import numpy as np

from _device import COG_TOL, REW_TOL


def _gpu_run(g, acts, mult, after=False, kernel=None):
    """Step g through acts [S, E, A, 4]; per step the observation hashes, rewards,
    done and cog as host arrays; with after=True also the action rows as each
    step left them. kernel: what lnw_step_kernel must report after every step."""
    import torch
    S, E = acts.shape[:2]
    mt = torch.from_numpy(mult).cuda()
    hs, rews, dones, cogs, afts = [], [], [], [], []
    for s in range(S):
        act = torch.from_numpy(acts[s]).cuda()
        out = g.step(act)
        assert kernel is None or g.step_kernel() == kernel, "the plan chose another kernel than the one under test"
        w = torch.cat([out["obs_blue"].reshape(E, -1), out["obs_red"].reshape(E, -1)], 1)
        w = w.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        hs.append((w * mt).sum(1).cpu().numpy().view(np.uint64))
        rews.append(torch.cat([out["rew_blue"].reshape(E, -1), out["rew_red"].reshape(E, -1)],
                              1).cpu().numpy())
        dones.append(out["done"].cpu().numpy().copy())
        cogs.append(out["cog"].cpu().numpy().copy())
        if after:
            afts.append(act.cpu().numpy())
    torch.cuda.synchronize()
    res = (np.stack(hs), np.stack(rews), np.stack(dones), np.stack(cogs))
    return res + (np.stack(afts),) if after else res


def _compare(gpu, orc, label):
    gh, gr, gd, gc = gpu
    oh, orw, od, oc = orc
    bad = np.argwhere(gh != oh)
    assert bad.size == 0, f"{label}: {len(bad)} (step, env) observation hashes differ, first {bad[:4].tolist()}"
    assert np.array_equal(gd, od), f"{label}: done differs at {np.argwhere(gd != od)[:4].tolist()}"
    assert np.allclose(gr, orw, rtol=0, atol=REW_TOL), \
        f"{label}: rewards differ at {np.argwhere(~np.isclose(gr, orw, rtol=0, atol=REW_TOL))[:4].tolist()}"
    assert np.allclose(gc, oc, rtol=0, atol=COG_TOL, equal_nan=True), f"{label}: cog differs"
