"""Training over sharded rollouts: every rank draws its candidates from its own
rows, the ranks assemble the one minibatch a single rank would draw over all the
rows, identically everywhere, and every rank runs the unchanged learner step on
it. The kernels are bitwise reproducible, so the ranks' parameters never
diverge and an N-rank run equals the one-rank run bit for bit; no gradient is
exchanged.

The protocol (PPOLearner.minibatch_dist runs it; include/lnw.h has the device
contracts) has three pieces, each callable on its own so that one process can
play W ranks:

  message  a rank's local draw as [2 B + 1] int64: the keys' bits, the global
           rows, the count of non-finite rows. One all-gather makes [W][2 B + 1].
  merge    the first B of the union in the order (key, global row): for every
           slot its key, global row, source rank and position, and its row of
           the packed observations (lnw_ppo_sample_merge).
  pack     the payload of the slots a rank owns into an exchange buffer of
           32-bit words, zeros elsewhere (lnw_ppo_rows_pack). One all-reduce of
           the buffer as int32 with SUM returns every owner's bits on every
           rank: an integer sum keeps -0.0 and NaN payloads, a float sum would
           not.

impl="hip" runs merge and pack on the device on the current stream;
impl="torch" is the same protocol with NumPy / torch indexing, on the host or
the device. The collectives are lnw.dist.all_gather / all_reduce_sum_.
"""
import ctypes as C

import numpy as np
import torch

from . import _abi, dist
from .keyed import cached

MAX_RANKS = 64  # include/lnw.h: lnw_ppo_sample_merge


def pack_words(batch, n, D):
    """Words of the exchange buffer (lnw_ppo_pack_words): xobs [B][n][D],
    actions [B][4], old_log_probs [B][4], rtg [B] and old_values [B], the last
    two padded to a multiple of 4 words."""
    pad = (batch + 3) & ~3
    return batch * n * D + 8 * batch + 2 * pad


def _regions(batch, n, D):
    pad = (batch + 3) & ~3
    o_act = batch * n * D
    return o_act, o_act + 4 * batch, o_act + 8 * batch, o_act + 8 * batch + pad


def message(b, row_base, status):
    """A rank's candidate list from its local draw b (PPOLearner.minibatch with
    this row_base) and its count of non-finite rows (a 1-element int64 tensor):
    [2 B + 1] int64 on b's device, a copy."""
    return torch.cat([b["key"].view(torch.int64), b["index"] + int(row_base),
                      status.to(b["index"].device, torch.int64).reshape(1)])


def merge_buffers(batch, device):
    e = lambda dtype: torch.empty(batch, dtype=dtype, device=device)  # noqa: E731
    return dict(key=e(torch.float64), global_row=e(torch.int64), src_rank=e(torch.int32), src_pos=e(torch.int32),
                index=e(torch.int64), status=torch.empty(1, dtype=torch.int64, device=device))


def merge(lists, batch, n, impl="hip", out=None):
    """The merged draw of the W ranks' messages `lists` [W, stride] int64:
    dict(key [B] float64, global_row [B] int64, src_rank, src_pos [B] int32,
    index [B] int64 = s n + global_row % n, status [1] int64). out: buffers to
    write (merge_buffers), else new ones."""
    W, stride = lists.shape
    B = int(batch)
    if not 1 <= W <= MAX_RANKS:
        raise ValueError(f"1 .. {MAX_RANKS} ranks")
    if stride < 2 * B + 1 or n < 1:
        raise ValueError("a message holds 2 batch + 1 words; n >= 1")
    m = merge_buffers(B, lists.device) if out is None else out
    if impl == "hip":
        L = _abi.load()
        lists = lists.contiguous()
        a = _abi.PpoMergeArgs()
        a.lists, a.W, a.n, a.stride, a.batch = lists.data_ptr(), W, n, stride, B
        a.key_out, a.row_out, a.index_out = m["key"].data_ptr(), m["global_row"].data_ptr(), m["index"].data_ptr()
        a.src_rank, a.src_pos, a.status_out = m["src_rank"].data_ptr(), m["src_pos"].data_ptr(), m["status"].data_ptr()
        _abi.check(L.lnw_ppo_sample_merge(C.byref(a), _abi.stream(lists.device)))
        return m
    h = lists.detach().cpu().numpy()
    key = np.ascontiguousarray(h[:, :B]).view(np.float64).reshape(-1)
    row = h[:, B:2 * B].reshape(-1)
    order = np.lexsort((row, key))[:B]
    t = lambda v, dtype: torch.from_numpy(np.ascontiguousarray(v.astype(dtype))).to(lists.device)  # noqa: E731
    m["key"].copy_(t(key[order], np.float64))
    m["global_row"].copy_(t(row[order], np.int64))
    m["src_rank"].copy_(t(order // B, np.int32))
    m["src_pos"].copy_(t(order % B, np.int32))
    m["index"].copy_(t(np.arange(B) * n + row[order] % n, np.int64))
    m["status"].copy_(t(h[:, 2 * B].sum(keepdims=True), np.int64))
    return m


def pack(ro, merged, rank, row_base, impl="hip", xbuf=None):
    """Rank `rank`'s exchange buffer, int32 [pack_words]: the payload of the
    slots whose src_rank is `rank` from its rollout tensors ro (PPOLearner.
    rollout_rows: rows [row_base, row_base + rows) of the whole), zeros
    elsewhere. xbuf: the buffer to write, else a new one."""
    n, D, obs = ro["n"], ro["D"], ro["obs"]
    B, N = merged["global_row"].shape[0], ro["rtg"].shape[0]
    if row_base % n:
        raise ValueError("row_base must be a whole number of groups")
    if impl == "hip":
        L = _abi.load()
        words = L.lnw_ppo_pack_words(B, n, D)
        if words <= 0:
            raise _abi.LnwError(f"lnw_ppo_rows_pack does not support batch={B}, n={n}, D={D}")
        if xbuf is None:
            xbuf = torch.empty(words, dtype=torch.int32, device=obs.device)
        a = _abi.PpoPackArgs()
        a.obs, a.actions, a.log_probs = obs.data_ptr(), ro["actions"].data_ptr(), ro["log_probs"].data_ptr()
        a.rtg, a.values, a.rows, a.row_base = ro["rtg"].data_ptr(), ro["values"].data_ptr(), N, int(row_base)
        a.n, a.D, a.rank, a.batch = n, D, int(rank), B
        a.row_out, a.src_rank = merged["global_row"].data_ptr(), merged["src_rank"].data_ptr()
        a.xbuf, a.xbuf_words = xbuf.data_ptr(), xbuf.numel()
        _abi.check(L.lnw_ppo_rows_pack(C.byref(a), _abi.stream(obs.device)))
        return xbuf
    words = pack_words(B, n, D)
    if xbuf is None:
        xbuf = torch.empty(words, dtype=torch.int32, device=obs.device)
    xbuf.zero_()
    o_act, o_lp, o_rtg, o_val = _regions(B, n, D)
    own = merged["src_rank"] == int(rank)
    r = (merged["global_row"] - int(row_base))[own]
    grp = torch.div(r, n, rounding_mode="floor")
    bits = lambda v: v.view(torch.int32)  # noqa: E731
    xbuf[:o_act].view(B, n * D)[own] = bits(obs.reshape(-1, n * D))[grp]
    xbuf[o_act:o_lp].view(B, 4)[own] = bits(ro["actions"])[r]
    xbuf[o_lp:o_rtg].view(B, 4)[own] = bits(ro["log_probs"])[r]
    xbuf[o_rtg:o_rtg + B][own] = bits(ro["rtg"])[r]
    xbuf[o_val:o_val + B][own] = bits(ro["values"])[grp]
    return xbuf


def unpack(xbuf, merged, n, D):
    """The learner's batch from a summed exchange buffer and the merged draw:
    views of xbuf, and the merge's key, index and global_row."""
    B = merged["global_row"].shape[0]
    o_act, o_lp, o_rtg, o_val = _regions(B, n, D)
    f = xbuf.view(torch.float32)
    return dict(obs=f[:o_act].view(B, n, D), index=merged["index"], actions=f[o_act:o_lp].view(B, 4),
                old_log_probs=f[o_lp:o_rtg].view(B, 4), rtg=f[o_rtg:o_rtg + B], old_values=f[o_val:o_val + B],
                key=merged["key"], global_row=merged["global_row"])


def exchange(local, status, row_base, batch, n, impl, group, merge_out, pack_owned):
    """The ranks' part of a sharded draw, after the local draw `local` (its
    count of non-finite rows in `status`): one all-gather of the messages, the
    merge into merge_out (merge_buffers; its status becomes `status`, so the
    count over all ranks replaces the local one), pack_owned(merged, rank) ->
    this rank's exchange buffer, and one int32 SUM all-reduce of it. Returns
    (merged, the summed buffer)."""
    merge_out["status"] = status
    rank, _ = dist.rank_size(group)
    lists = dist.all_gather(message(local, row_base, status), group)
    merged = merge(lists, batch, n, impl, out=merge_out)
    xbuf = pack_owned(merged, rank)
    dist.all_reduce_sum_(xbuf, group)
    return merged, xbuf


def minibatch_dist(learner, out, batch, row_base, seed=None, rtg=None, advance=True, group=None):
    """PPOLearner.minibatch_dist (its docstring has the contract)."""
    B = int(batch)
    if int(row_base) % out["obs"].shape[-2]:
        raise ValueError("row_base must be a whole number of groups")
    # the local draw: raises on batch > local rows, before any collective
    local = learner.minibatch(out, B, seed=seed, rtg=rtg, row_base=row_base, advance=advance)
    ro = learner.rollout_rows(out, rtg)
    n, D, dev = ro["n"], ro["D"], learner.device
    buf = cached(learner._dist_buf, (B, n, D), lambda: dict(
        merge_buffers(B, dev), xbuf=torch.empty(pack_words(B, n, D), dtype=torch.int32, device=dev)))
    merged, xbuf = exchange(local, learner.sample_status, row_base, B, n, learner.impl, group, buf,
                            lambda m, rank: pack(ro, m, rank, row_base, learner.impl, xbuf=buf["xbuf"]))
    return unpack(xbuf, merged, n, D)
