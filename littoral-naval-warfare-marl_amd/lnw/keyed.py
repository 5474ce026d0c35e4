"""Everything keyed by (seed, slot, global row): the Philox uniforms and normals
the rollouts and the DDQN acting draw (lnw_fill_uniform_f32), and the keyed draw
without replacement behind PPOLearner.minibatch and the DDQN replay
(lnw_ppo_sample, csrc/lnw_pposample.hip) with its restatement on the host. Each
is a pure function of its key, so a shard of the rows draws what one call over
all rows draws for them.
"""
import ctypes as C

import numpy as np
import torch

from . import _abi
from ._abi import LNW_SAMPLE_CTR2, LNW_SAMPLE_CTR3, LNW_SAMPLE_MAX_BATCH


def keyed_normal(row0, rows, cols, seed, slot, device):
    """Standard-normal draws [rows, cols] for global rows row0 .. row0+rows-1,
    a pure function of (seed, slot, global row, column): Philox uniforms
    (lnw_fill_uniform_f32, the bench's action generator) at absolute counter
    slot * 2^40 + row * 2 * cols + k, then Box-Muller. A rank holding global
    envs [lo, hi) draws exactly the values one rank holding all envs draws for
    them, so a sharded rollout samples what an unsharded one does."""
    u = keyed_uniform(row0, rows, cols, seed, slot, device)
    r = torch.sqrt(-2.0 * torch.log1p(-u[:, :cols]))  # 1 - u in (0, 1]
    return r * torch.cos((2.0 * np.pi) * u[:, cols:])


def keyed_uniform(row0, rows, cols, seed, slot, device):
    """The uniforms [rows, 2 cols] under keyed_normal's draws: row r holds the
    Philox stream's values at slot * 2^40 + (row0 + r) * 2 * cols + k (radii for
    k < cols, then angles). The fill starts at a multiple of 4 (one Philox block
    holds four values); an offset that is none (row0 * 2 * cols odd pairs: the
    parameter-noise rows, cols = the flat actor size) is filled from the block
    below and cut. The seed is taken modulo 2^64; no rows launch nothing."""
    per = 2 * cols
    off = (int(slot) << 40) + int(row0) * per
    lead = off & 3
    u = torch.empty(lead + rows * per, dtype=torch.float32, device=device)
    if rows:
        _abi.check(_abi.load().lnw_fill_uniform_f32(u.data_ptr(), u.numel(), int(seed) & (2 ** 64 - 1), off - lead,
                                                    _abi.stream(device)))
    return u[lead:].reshape(rows, per)


def keyed_uniform4(row0, rows, seed, slot, device):
    """The four keyed uniforms [rows, 4] of global rows row0 .. row0+rows-1 that
    lnw_qnet_act draws: Philox (lnw_fill_uniform_f32) at absolute offset
    slot * 2^40 + 4 * row — keyed_normal's convention, so a shard of the envs
    draws what one call over all envs draws for them."""
    return keyed_uniform(row0, rows, 2, seed, slot, device)


def _philox10(c, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words (lnw_device.h)."""
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = c
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def _p_log(x):
    """lnw_device.h's portable ln in float64 array operations: the same bits."""
    m, e = np.frexp(x)
    low = m < 0.70710678118654752
    m = np.where(low, m * 2.0, m)
    e = e - low
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = np.full_like(z, 1.0 / 19.0)
    for d in (17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0, 1.0):
        p = p * z + 1.0 / d
    return 2.0 * s * p + e.astype(np.float64) * 0.6931471805599453


def sample_keys(rtg, seed, slot, row_base=0):
    """lnw_ppo_sample's keys (include/lnw.h) of a float32 reward-to-go vector on
    the host: float64 [rows], +inf where rtg is not finite."""
    rtg = np.ascontiguousarray(rtg, np.float32).reshape(-1)
    m32 = np.uint64(0xFFFFFFFF)
    ctr = np.uint64(int(slot) << 40) + np.uint64(int(row_base)) + np.arange(rtg.shape[0], dtype=np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    o = _philox10((ctr & m32, ctr >> np.uint64(32), np.full_like(ctr, LNW_SAMPLE_CTR2),
                   np.full_like(ctr, LNW_SAMPLE_CTR3)), np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    u = ((o[0] >> np.uint64(5)).astype(np.float64) * 67108864.0
         + (o[1] >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0
    with np.errstate(all="ignore"):
        w = (np.abs(rtg) + np.float32(1e-5)).astype(np.float64)
        key = -_p_log(1.0 - u) / w + 0.0
    return np.where(np.isfinite(rtg), key, np.inf)


def check_batch(batch, rows, noun="rows"):
    """int(batch), or the draw's ValueError: a caller that keeps buffers per
    batch size asks before it makes them, draw() itself always."""
    B = int(batch)
    if not 1 <= B <= min(int(rows), LNW_SAMPLE_MAX_BATCH):
        raise ValueError(f"batch must be in 1 .. min({noun}, {LNW_SAMPLE_MAX_BATCH})")
    return B


def cached(cache, key, make):
    """cache[key], made by make() on first use; cache None: a new make()."""
    if cache is None:
        return make()
    if key not in cache:
        cache[key] = make()
    return cache[key]


def draw_buffers(rows, batch, device, impl="hip", payload=False):
    """The outputs (and, for the kernels, the workspace) of one draw shape;
    payload: also those of the gathered rows."""
    e = lambda *s, dtype=torch.float32: torch.empty(s, dtype=dtype, device=device)  # noqa: E731
    buf = dict(index=e(batch, dtype=torch.int64), key=e(batch, dtype=torch.float64))
    if payload:
        buf.update(actions=e(batch, 4), old_log_probs=e(batch, 4), rtg=e(batch), old_values=e(batch))
    if impl == "hip":
        need = _abi.load().lnw_ppo_sample_workspace_bytes(rows, batch)
        if need <= 0:
            raise _abi.LnwError(f"lnw_ppo_sample does not support rows={rows}, batch={batch}")
        buf["ws"] = e(need, dtype=torch.uint8)
    return buf


def draw(weights, batch, seed, counter, status, row_base=0, advance=True, impl="hip", buf=None, payload=None):
    """The keyed draw (lnw_ppo_sample, include/lnw.h) over the flattened
    weights, a float32 tensor of reward-to-go values or replay priorities [E,
    cap]: `batch` distinct rows by priorities |w| + 1e-5 in ascending (key,
    row) order, the reference sampler's distribution in draw order, as a pure
    function of (seed, counter, global row = row_base + index): dict(index [B]
    int64 local rows (of the priorities: e * cap + k) in draw order, key [B]
    float64). counter: int64 [1], the slot of the draw, read where it lives
    and advanced by one unless advance is False; status: int64 [1], receives
    the count of non-finite weights (drawn last, in row order: a replay's
    empty slots, unless the caller planted others). buf: draw_buffers to write,
    else new ones. payload: None, or dict(actions, log_probs [rows, 4], values
    [rows / n], n) of a rollout's rows (PPOLearner.rollout_rows) to gather
    with the draw: the result also holds actions, old_log_probs [B, 4], rtg
    and old_values [B] (the group's value for each of its n ships).

    impl="hip": one chain of launches on the current stream with no host
    synchronisation. impl="torch": the same draw from the definition with
    NumPy on the host (sample_keys and np.lexsort; it reads the counter, so it
    synchronises), the same index bit for bit."""
    _abi.check_impl(impl)
    w = weights.reshape(-1)
    N = w.shape[0]
    B = check_batch(batch, N)
    seed = int(seed) & (2 ** 64 - 1)
    if buf is None:
        buf = draw_buffers(N, B, w.device, impl, payload is not None)
    if impl == "hip":
        a = _abi.PpoSampleArgs()
        a.rtg, a.rows, a.row_base, a.batch, a.seed = w.data_ptr(), N, int(row_base), B, seed
        a.draw_dev, a.advance, a.n = counter.data_ptr(), int(bool(advance)), 1
        if payload is not None:
            a.actions, a.log_probs = payload["actions"].data_ptr(), payload["log_probs"].data_ptr()
            a.values, a.n = payload["values"].data_ptr(), payload["n"]
            a.actions_out, a.log_probs_out = buf["actions"].data_ptr(), buf["old_log_probs"].data_ptr()
            a.rtg_out, a.old_values_out = buf["rtg"].data_ptr(), buf["old_values"].data_ptr()
        a.index_out, a.key_out, a.status = buf["index"].data_ptr(), buf["key"].data_ptr(), status.data_ptr()
        a.workspace, a.workspace_bytes = buf["ws"].data_ptr(), buf["ws"].numel()
        _abi.check(_abi.load().lnw_ppo_sample(C.byref(a), _abi.stream(w.device)))
        return buf
    h = w.detach().cpu().numpy()
    key = sample_keys(h, seed, int(counter), int(row_base))
    # ascending key, ties to the lower row (keys compare as numbers: sample_keys holds no -0)
    order = np.lexsort((np.arange(N), key))[:B]
    buf["index"].copy_(torch.from_numpy(order.astype(np.int64)))
    buf["key"].copy_(torch.from_numpy(key[order]))
    status.fill_(int((~np.isfinite(h)).sum()))
    if advance:
        counter += 1
    if payload is not None:
        index = buf["index"]
        buf["actions"].copy_(payload["actions"][index])
        buf["old_log_probs"].copy_(payload["log_probs"][index])
        buf["rtg"].copy_(w[index])
        buf["old_values"].copy_(payload["values"][torch.div(index, payload["n"], rounding_mode="floor")])
    return buf
