"""DDQN replay on the device: the priorities beside QCollector's ring, the
keyed draw without replacement over them, and the pack of the drawn transitions
into the learner's row tensors, alone or as a rank's exchange buffer for
training on the union of sharded collectors (include/lnw.h "DDQN replay" has
the device contracts; QCollector.minibatch / minibatch_dist run the pieces).

Every piece works on plain tensors. A ring is dict(state, next_state [cap, E, n,
D] float32, action [cap, E, n, 4] int32, reward [cap, E, n] float32 or float64,
done [cap, E] int32); its priorities are float32 [E, cap], env-major: local row
r = e * cap + k, global row = row_base + r with row_base = (first global env) *
cap, NaN for a slot that holds no transition yet.

  new_priority  the NaN-filled priority tensor
  mark          priority[:, k] after a collector step wrote slot k: 1, or the
                float32 sum of the ships' |reward| (lnw_replay_mark)
  draw          lnw_ppo_sample over the flattened priorities: `batch` distinct
                rows by weights |p| + 1e-5 in ascending (key, row) order; equal
                priorities make it uniform sampling without replacement
                (lnw.keyed.draw, the learner's draw without the payload)
  pack          the drawn transitions as 32-bit words: state, next_state,
                action, reward, done per ship, zero words in the slots another
                rank owns (lnw_replay_pack)
  unpack        the learner's row tensors as views of that buffer
  minibatch     draw, then pack with every slot owned
  minibatch_dist  the local draw, lnw.ppodist's message / all-gather / merge,
                pack of the owned slots, one int32 SUM all-reduce, unpack

impl="hip" runs on the device on the current stream with no host
synchronisation; impl="torch" is the same definition without the library (the
draw from lnw.keyed.sample_keys and np.lexsort, the pack by torch indexing on
int32 views), on the host or the device, and gives the same bits.
"""
import ctypes as C

import torch

from . import _abi, ppodist
from ._abi import check_impl
from .keyed import cached, check_batch, draw, draw_buffers

ROW_KEYS = ("state", "next_state", "action", "reward", "done")


def ring_shape(ring):
    """(cap, E, n, D, reward_f64) of a ring."""
    cap, E, n, D = ring["state"].shape
    return cap, E, n, D, ring["reward"].dtype == torch.float64


def new_priority(E, cap, device):
    """The priorities of an empty ring: float32 [E, cap], all NaN."""
    return torch.full((int(E), int(cap)), float("nan"), dtype=torch.float32, device=device)


def mark(priority, reward, k, mode, impl="hip"):
    """priority[:, k] for the transitions of ring slot k. mode "uniform": 1.0;
    "reward": sum over ships i = 0 .. n-1, in that order, in float32, of
    |float32(reward[k, e, i])|."""
    check_impl(impl)
    if mode not in ("uniform", "reward"):
        raise ValueError("priority must be 'uniform' or 'reward'")
    E, cap = priority.shape
    n = reward.shape[2]
    if impl == "hip":
        L = _abi.load()
        a = _abi.ReplayMarkArgs()
        a.priority, a.E, a.cap, a.k, a.n = priority.data_ptr(), E, cap, int(k), n
        if mode == "reward":
            a.reward, a.reward_f64 = reward.data_ptr(), int(reward.dtype == torch.float64)
        _abi.check(L.lnw_replay_mark(C.byref(a), _abi.stream(priority.device)))
        return priority
    if mode == "uniform":
        priority[:, k] = 1.0
        return priority
    mag = reward[k].to(torch.float32).abs()
    p = torch.zeros(E, dtype=torch.float32, device=priority.device)
    for i in range(n):
        p = p + mag[:, i]
    priority[:, k] = p
    return priority


def _regions(batch, n, D, reward_f64):
    bn = batch * n
    o_next = bn * D
    o_act = 2 * bn * D
    o_rew = o_act + 4 * bn
    o_done = o_rew + ((bn * (2 if reward_f64 else 1) + 3) & ~3)
    return o_next, o_act, o_rew, o_done, o_done + ((bn + 3) & ~3)


def pack_words(batch, n, D, reward_f64):
    """Words of the packed buffer (lnw_replay_pack_words): state and next_state
    [B][n][D], action [B][n][4], reward [B][n] of one or two words and done
    [B][n], the last two padded to a multiple of 4 words."""
    return _regions(int(batch), n, D, bool(reward_f64))[-1]


def pack(ring, global_row, src_rank=None, rank=0, row_base=0, impl="hip", xbuf=None, index_out=None):
    """The packed buffer, int32 [pack_words]: the transitions of the slots this
    rank owns (all of them with src_rank None, else those whose src_rank is
    `rank`) at local rows global_row - row_base of its ring, zero words in every
    other slot, in a slot whose row lies outside the ring, and in the padding.
    xbuf: the buffer to write, else a new one. index_out: int64 [B] to receive
    ring step * E + env per slot (-1 for a slot of zeros)."""
    check_impl(impl)
    cap, E, n, D, f64 = ring_shape(ring)
    B = global_row.shape[0]
    dev = ring["state"].device
    if impl == "hip":
        L = _abi.load()
        words = L.lnw_replay_pack_words(B, n, D, int(f64))
        if words <= 0:
            raise _abi.LnwError(f"lnw_replay_pack does not support batch={B}, n={n}, D={D}")
        if xbuf is None:
            xbuf = torch.empty(words, dtype=torch.int32, device=dev)
        a = _abi.ReplayPackArgs()
        a.state, a.next_state, a.action = ring["state"].data_ptr(), ring["next_state"].data_ptr(), ring["action"].data_ptr()
        a.reward, a.done, a.reward_f64 = ring["reward"].data_ptr(), ring["done"].data_ptr(), int(f64)
        a.cap, a.E, a.n, a.D, a.row_base, a.batch = cap, E, n, D, int(row_base), B
        a.row_out, a.rank = global_row.data_ptr(), int(rank)
        if src_rank is not None:
            a.src_rank = src_rank.data_ptr()
        if index_out is not None:
            a.index_out = index_out.data_ptr()
        a.xbuf, a.xbuf_words = xbuf.data_ptr(), xbuf.numel()
        _abi.check(L.lnw_replay_pack(C.byref(a), _abi.stream(dev)))
        return xbuf
    o_next, o_act, o_rew, o_done, words = _regions(B, n, D, f64)
    if xbuf is None:
        xbuf = torch.empty(words, dtype=torch.int32, device=dev)
    xbuf.zero_()
    r = global_row - int(row_base)
    own = (r >= 0) & (r < E * cap)
    if src_rank is not None:
        own &= src_rank == int(rank)
    r = r[own]
    at = (r % cap) * E + torch.div(r, cap, rounding_mode="floor")  # ring step * E + env
    bits = lambda t, w: t.reshape(cap * E, -1).view(torch.int32).reshape(cap * E, w)  # noqa: E731
    rw = 2 if f64 else 1
    xbuf[:o_next].view(B, n * D)[own] = bits(ring["state"], n * D)[at]
    xbuf[o_next:o_act].view(B, n * D)[own] = bits(ring["next_state"], n * D)[at]
    xbuf[o_act:o_rew].view(B, n * 4)[own] = bits(ring["action"], n * 4)[at]
    xbuf[o_rew:o_rew + B * n * rw].view(B, n * rw)[own] = bits(ring["reward"], n * rw)[at]
    xbuf[o_done:o_done + B * n].view(B, n)[own] = ring["done"].reshape(-1)[at][:, None].expand(-1, n)
    if index_out is not None:
        index_out.fill_(-1)
        index_out[own] = at
    return xbuf


def unpack(xbuf, batch, n, D, reward_f64):
    """The learner's row tensors as views of a packed (or summed) buffer:
    dict(state, next_state [B n, D] float32, action [B n, 4] int32, reward [B n]
    float32 or float64, done [B n] int32)."""
    B = int(batch)
    o_next, o_act, o_rew, o_done, _ = _regions(B, n, D, bool(reward_f64))
    f = xbuf.view(torch.float32)
    rew = xbuf[o_rew:o_rew + 2 * B * n].view(torch.float64) if reward_f64 else f[o_rew:o_rew + B * n]
    return dict(state=f[:o_next].view(B * n, D), next_state=f[o_next:o_act].view(B * n, D),
                action=xbuf[o_act:o_rew].view(B * n, 4), reward=rew, done=xbuf[o_done:o_done + B * n])


def minibatch(ring, priority, batch, filled, seed, counter, status, row_base=0, advance=True, impl="hip",
              cache=None):
    """Draw, then pack with every slot owned: the dict QLearner.step() / grad()
    take as row tensors (unpack's), plus key [B] float64, index [B] int64 = ring
    step * E + env, and global_row [B] int64. filled: the ring slots that hold
    transitions; batch > filled * E raises ValueError before anything runs, so no
    empty slot is drawn. cache: a dict that keeps the buffers per batch size (the
    next call of that size overwrites them); None allocates new ones."""
    check_impl(impl)
    cap, E, n, D, f64 = ring_shape(ring)
    B = check_batch(batch, int(filled) * E, "filled * E")
    dev = priority.device

    def make():
        buf = draw_buffers(E * cap, B, dev, impl)
        buf["global_row"] = torch.empty(B, dtype=torch.int64, device=dev)
        buf["ring_index"] = torch.empty(B, dtype=torch.int64, device=dev)
        buf["xbuf"] = torch.empty(pack_words(B, n, D, f64), dtype=torch.int32, device=dev)
        return buf

    buf = cached(cache, ("local", B), make)
    draw(priority, B, seed, counter, status, row_base, advance, impl, buf)
    torch.add(buf["index"], int(row_base), out=buf["global_row"])
    pack(ring, buf["global_row"], None, 0, row_base, impl, buf["xbuf"], buf["ring_index"])
    out = unpack(buf["xbuf"], B, n, D, f64)
    out.update(key=buf["key"], index=buf["ring_index"], global_row=buf["global_row"])
    return out


def minibatch_dist(ring, priority, batch, filled, seed, counter, status, row_base, advance=True, group=None,
                   impl="hip", cache=None):
    """minibatch() over the union of the ranks' rings (QCollector.minibatch_dist
    has the contract): dict of unpack's row tensors, key and global_row. status
    receives the count over all ranks."""
    check_impl(impl)
    cap, E, n, D, f64 = ring_shape(ring)
    B = check_batch(batch, int(filled) * E, "filled * E")  # raises before any collective
    dev = priority.device
    buf = cached(cache, ("dist", B), lambda: dict(
        draw=draw_buffers(E * cap, B, dev, impl), merge=ppodist.merge_buffers(B, dev),
        xbuf=torch.empty(pack_words(B, n, D, f64), dtype=torch.int32, device=dev)))
    local = draw(priority, B, seed, counter, status, row_base, advance, impl, buf["draw"])
    merged, xbuf = ppodist.exchange(local, status, row_base, B, 1, impl, group, buf["merge"],
                                    lambda m, rank: pack(ring, m["global_row"], m["src_rank"], rank, row_base, impl,
                                                         buf["xbuf"]))
    out = unpack(xbuf, B, n, D, f64)
    out.update(key=merged["key"], global_row=merged["global_row"])
    return out
