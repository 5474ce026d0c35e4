"""Shared by the tests that compare a whole batch with orc_fullsize_range
(test_gpu_fullsize.py, test_gpu_team_sizes.py): the multipliers of the
observation hash sum_k bits(obs[k]) * mult[k] mod 2^64, the device-side run
that reduces every (step, env) to that hash, and the comparison."""
import numpy as np

import _oracle

REW_TOL = 1e-5


def _mult(n, seed=99):
    return (np.random.default_rng(seed).integers(0, 1 << 30, n, dtype=np.int64) * 2 + 1)


def _gpu_run(g, acts, mult, after=False):
    """Step g through acts [S, E, A, 4]; per step the observation hashes, rewards,
    done and cog as host arrays; with after=True also the action rows as each
    step left them."""
    import torch
    S, E = acts.shape[:2]
    mt = torch.from_numpy(mult).cuda()
    hs, rews, dones, cogs, afts = [], [], [], [], []
    for s in range(S):
        act = torch.from_numpy(acts[s]).cuda()
        out = g.step(act)
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
    assert np.allclose(gc, oc, rtol=0, atol=1e-5, equal_nan=True), f"{label}: cog differs"


def _grids():
    g = _oracle.load_fixture("grids.npz")
    return g["grid100"], g["grid200"]


def _water_positions(grid, E, boxes, seed):
    """Per env, per agent a water cell drawn uniformly from that agent's box."""
    rng = np.random.default_rng(seed)
    out = np.zeros((E, len(boxes), 2), np.int32)
    for a, (x0, x1, y0, y1) in enumerate(boxes):
        cells = np.argwhere(grid[x0:x1, y0:y1] <= 74) + np.array([x0, y0])
        out[:, a] = cells[rng.integers(0, len(cells), E)]
    return out
