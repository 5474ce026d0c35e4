"""DDQN replay without a GPU: lnw/replay.py's torch arm (no library)
against plain indexing of the ring at the rows a direct sample_keys / lexsort
gives; the priorities against their float32 restatement; one process playing
the ranks of a sharded draw; the statistics of the draw under fixed seeds;
minibatch_dist in two gloo processes against minibatch over all envs; and the
host-side argument checks of lnw_replay_pack and lnw_replay_mark, which run
before anything is launched."""
import math
import os
import queue
import socket
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from _replay_cases import (CASES, SEED, SLOT, bits, build, check_rows, counters, direct_rows, expected, play,
                           priority_restated, same, shard)
from lnw import replay


def one_minibatch(case, **kw):
    ring, pr, filled, ranges = build(case)
    ctr, status = counters("cpu")
    got = replay.minibatch(ring, pr, CASES[case]["B"], filled, SEED, ctr, status, impl="torch", **kw)
    return ring, pr, filled, ranges, ctr, status, got


@pytest.mark.parametrize("case", list(CASES))
def test_minibatch_is_plain_indexing_at_the_direct_draw(case):
    c = CASES[case]
    ring, pr, filled, _, ctr, status, got = one_minibatch(case)
    cap, E, n, D, f64 = replay.ring_shape(ring)
    rows, keys = direct_rows(pr, c["B"], SEED, SLOT)
    check_rows(got, ring, rows, keys)
    B = c["B"]
    assert got["state"].shape == (B * n, D) and got["action"].shape == (B * n, 4) and got["done"].shape == (B * n,)
    assert got["reward"].dtype == (torch.float64 if f64 else torch.float32) and got["action"].dtype == torch.int32
    assert int(ctr) == SLOT + 1 and int(status) == E * (cap - filled)
    assert np.isfinite(keys).all() and (rows % cap < filled).all() and len(set(rows.tolist())) == B
    assert np.all((keys[1:] > keys[:-1]) | ((keys[1:] == keys[:-1]) & (rows[1:] > rows[:-1])))
    # done is the transition's, repeated per ship; index is sample()'s convention ring step * E + env
    k, e = rows % cap, rows // cap
    assert np.array_equal(got["done"].numpy().reshape(B, n), np.repeat(ring["done"].numpy()[k, e][:, None], n, 1))
    assert np.array_equal(got["index"].numpy(), k * E + e)
    flat = lambda t: t.reshape((cap * E,) + tuple(t.shape[2:]))  # noqa: E731  (QCollector.sample's indexing)
    assert same(flat(ring["state"])[got["index"]].reshape(B * n, D), got["state"])
    # the planted bit patterns arrive
    st, ns = bits(got["state"]).reshape(B, n, D), bits(got["next_state"]).reshape(B, n, D)
    assert (st[:, 0, 0] == -0x80000000).all() and (st[:, n - 1, D - 1] == 0x7FC12345).all()
    assert (ns[:, 0, 1] == 1).all() and (ns[:, n - 1, D - 2] == 0x7FC12346).all()
    if case == "all":
        assert sorted(rows.tolist()) == list(range(15))  # every transition exactly once
    if case == "part":
        words = replay.pack_words(B, n, D, True)
        assert words == 2 * B * n * D + 4 * B * n + 44 + 24 and words % 4 == 0
        assert not np.array_equal(got["reward"].numpy().astype(np.float32).astype(np.float64), got["reward"].numpy())


def test_padding_is_zero_and_every_word_is_written():
    ring, pr, filled, _ = build("part")
    rows, _ = direct_rows(pr, 7, SEED, SLOT)
    xbuf = torch.full((replay.pack_words(7, 3, 100, True),), -1515870811, dtype=torch.int32)
    replay.pack(ring, torch.from_numpy(rows), impl="torch", xbuf=xbuf)
    o_rew = 2 * 7 * 300 + 84
    assert not bool(xbuf[o_rew + 42:o_rew + 44].any()) and not bool(xbuf[o_rew + 44 + 21:].any())
    assert not bool((xbuf[:o_rew + 42] == -1515870811).any())


@pytest.mark.parametrize("case", ["part", "wrap", "wide"])
def test_reward_priorities_equal_the_float32_restatement(case):
    ring, pr, filled, _ = build(case)
    assert np.array_equal(bits(pr), priority_restated(ring, filled).view(np.int32))
    u = build(case, mode="uniform")[1].numpy()
    assert (u[:, :filled] == 1.0).all() and np.isnan(u[:, filled:]).all()


def test_wrapped_slots_carry_the_new_priorities():
    """7 steps into 4 slots: slots 0..2 were overwritten, and their priorities are
    those of steps 4..6, not of steps 0..2."""
    from _replay_cases import fill, history
    c = CASES["wrap"]
    hist = history(4, c["n"], c["D"], 7, False, 100 + c["D"] + 4)
    ring, pr = fill(hist, 4, "reward")
    early = fill({k: v[:4] for k, v in hist.items()}, 4, "reward")[1]
    assert same(ring["reward"][:3], hist["reward"][4:7]) and same(ring["reward"][3], hist["reward"][3])
    assert np.array_equal(bits(pr), priority_restated(ring, 4).view(np.int32))
    assert not (pr[:, :3] == early[:, :3]).any() and same(pr[:, 3], early[:, 3])


def test_counter_and_seed():
    ring, pr, filled, _, ctr, status, a = one_minibatch("wrap")
    a = {k: v.clone() for k, v in a.items()}
    b = replay.minibatch(ring, pr, 5, filled, SEED, ctr, status, advance=False, impl="torch")
    assert int(ctr) == SLOT + 1 and not np.array_equal(a["global_row"].numpy(), b["global_row"].numpy())
    c = {k: v.clone() for k, v in replay.minibatch(ring, pr, 5, filled, SEED, ctr, status, impl="torch").items()}
    assert int(ctr) == SLOT + 2
    for k in b:
        assert same(b[k], c[k]), k
    d = replay.minibatch(ring, pr, 5, filled, SEED + 1, ctr, status, advance=False, impl="torch")
    assert not np.array_equal(bits(c["key"]), bits(d["key"]))
    # a cache keeps the buffers per batch size: the next call of that size overwrites them
    cache = {}
    e = replay.minibatch(ring, pr, 5, filled, SEED, ctr, status, impl="torch", cache=cache)
    f = replay.minibatch(ring, pr, 5, filled, SEED, ctr, status, impl="torch", cache=cache)
    assert e["state"].data_ptr() == f["state"].data_ptr() and int(ctr) == SLOT + 4


def test_batch_larger_than_the_filled_ring_raises():
    ring, pr, filled, _ = build("part")
    ctr, status = counters("cpu")
    for B in (0, 11, -1):  # filled * E = 10
        with pytest.raises(ValueError):
            replay.minibatch(ring, pr, B, filled, SEED, ctr, status, impl="torch")
        with pytest.raises(ValueError):
            replay.minibatch_dist(ring, pr, B, filled, SEED, ctr, status, 0, impl="torch")
    assert int(ctr) == SLOT and int(status) == -7
    replay.minibatch(ring, pr, 10, filled, SEED, ctr, status, impl="torch")
    with pytest.raises(ValueError):
        replay.minibatch(ring, pr, 5, filled, SEED, ctr, status, impl="cuda")


def test_rows_tensors_pass_through_the_learner_unchanged():
    """QLearner.rows() on a minibatch is a no-op: the same storage."""
    from lnw.qlearn import BatchedQNet, QLearner
    *_, got = one_minibatch("ranks")
    L = QLearner(BatchedQNet.for_obs(60), impl="torch", device="cpu")
    r = L.rows(got)
    for k in replay.ROW_KEYS:
        assert r[k].data_ptr() == got[k].data_ptr() and r[k].dtype == got[k].dtype, k


def test_collector_without_priorities_refuses():
    """priority=None: minibatch() raises RuntimeError (the check runs before the
    collector's game is touched, so a bare object shows it)."""
    from lnw.qlearn import QCollector
    c = QCollector.__new__(QCollector)
    c.priority = None
    with pytest.raises(RuntimeError):
        c.minibatch(4)
    with pytest.raises(RuntimeError):
        c.minibatch_dist(4)


@pytest.mark.parametrize("case", ["ranks", "quiet"])
def test_played_ranks_equal_one_collector(case):
    c = CASES[case]
    ring, pr, filled, ranges, ctr, status, one = one_minibatch(case)
    cap, B = c["cap"], c["B"]
    got, own, lists, merged = play(ring, pr, filled, ranges, B, "torch")
    for k in got:
        assert same(got[k], one[k]), k
    rows, keys = direct_rows(pr, B, SEED, SLOT)
    check_rows(got, ring, rows, keys)
    # every word of the summed buffer is non-zero on at most one rank
    assert int(torch.stack([o != 0 for o in own]).sum(0).max()) <= 1
    # a shard's keys are the slice of the whole's
    from lnw.ppolearn import sample_keys
    whole = sample_keys(pr.numpy().reshape(-1), SEED, SLOT, 0)
    for w, (lo, hi) in enumerate(ranges):
        part = sample_keys(shard(ring, pr, lo, hi)[1].numpy().reshape(-1), SEED, SLOT, lo * cap)
        assert np.array_equal(part.view(np.int64), whole[lo * cap:hi * cap].view(np.int64))
        owner = (rows >= lo * cap) & (rows < hi * cap)
        assert np.array_equal(merged["src_rank"].numpy() == w, owner)
    if case == "ranks":
        assert lists.shape == (3, 2 * B + 1) and sorted(lists[1, B:2 * B].tolist()) == [12, 13, 14, 15]
    if case == "quiet":
        q = c["quiet"]
        assert not bool((merged["src_rank"] == q).any()) and not bool(own[q].any())
        assert all(bool(own[w].any()) for w in range(3) if w != q)


def test_world_of_one_without_a_process_group():
    ring, pr, filled, _, ctr, status, one = one_minibatch("part")
    one = {k: v.clone() for k, v in one.items()}
    ctr.fill_(SLOT)
    got = replay.minibatch_dist(ring, pr, 7, filled, SEED, ctr, status, 0, impl="torch")
    assert int(ctr) == SLOT + 1 and int(status) == 10 and "index" not in got
    for k in got:
        assert same(got[k], one[k]), k


# ---- statistics (deterministic under the fixed seeds) ----------------------------------
def test_uniform_inclusion_counts():
    """`uniform`, E = 16, cap = 5 with slot 4 empty, B = 8, seed 5, draws 0 ..
    3999: every one of the 64 transitions is included 500 times within 6 binomial
    standard deviations, and no empty slot is ever drawn."""
    E, cap, B, draws = 16, 5, 8, 4000
    pr = replay.new_priority(E, cap, "cpu")
    pr[:, :4] = 1.0
    ctr, status = counters("cpu", 0)
    count = np.zeros(E * cap, np.int64)
    for _ in range(draws):
        count[replay.draw(pr, B, 5, ctr, status, impl="torch")["index"].numpy()] += 1
    assert int(ctr) == draws and int(status) == E
    count = count.reshape(E, cap)
    assert (count[:, 4] == 0).all() and count.sum() == draws * B
    sigma = math.sqrt(draws * (1 / 8) * (7 / 8))
    dev = np.abs(count[:, :4] - 500) / sigma
    print(f"largest deviation {dev.max():.2f} sigma")
    assert dev.max() <= 6.0


def test_weighted_first_draw_counts():
    """64 rows with priorities alternating 3, 1; seed 9, row_base = 2^33, draws 0
    .. 3999: the first-drawn row's counts are 4000 w_r / sum(w) within 6 binomial
    standard deviations."""
    draws = 4000
    pr = torch.tensor([3.0, 1.0] * 32, dtype=torch.float32).reshape(16, 4)
    ctr, status = counters("cpu", 0)
    count = np.zeros(64, np.int64)
    for _ in range(draws):
        count[int(replay.draw(pr, 1, 9, ctr, status, row_base=2 ** 33, impl="torch")["index"][0])] += 1
    w = (np.abs(pr.numpy().reshape(-1)) + np.float32(1e-5)).astype(np.float64)
    p = w / w.sum()
    dev = np.abs(count - draws * p) / np.sqrt(draws * p * (1 - p))
    print(f"largest deviation {dev.max():.2f} sigma")
    assert int(status) == 0 and count.sum() == draws and dev.max() <= 6.0


# ---- two gloo processes ------------------------------------------------------------------
GLOO = dict(shards=(5, 4), cap=4, n=2, D=60, steps=6, B=8, f64=True)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.join(os.path.dirname(here), "littoral-naval-warfare-marl_amd")]
    from lnw import dist
    dist.init("gloo")
    ring, pr, filled, ranges = build(GLOO)
    lo, hi = ranges[rank]
    r, p = shard(ring, pr, lo, hi)
    ctr, status = counters("cpu")
    raised = False
    try:
        # more than either rank holds (20 and 16): raised before any collective
        replay.minibatch_dist(r, p, 21, filled, SEED, ctr, status, lo * 4, impl="torch")
    except ValueError:
        raised = True
    res, cache = [], {}
    for _ in range(2):
        b = replay.minibatch_dist(r, p, GLOO["B"], filled, SEED, ctr, status, lo * 4, impl="torch", cache=cache)
        res.append({k: v.clone().numpy() for k, v in b.items()})
    q.put((rank, raised, int(ctr), int(status), res))
    dist.barrier()
    dist.finalize()


def test_two_gloo_ranks_equal_one():
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res, deadline = [], time.monotonic() + 120
        while len(res) < 2:  # (a rank that died leaves the other in a collective: do not wait for it)
            try:
                res.append(q.get(timeout=1))
            except queue.Empty:
                assert time.monotonic() < deadline, "the ranks hang"
                assert all(p.is_alive() or p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
        res.sort(key=lambda t: t[0])
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    ring, pr, filled, _ = build(GLOO)
    ctr, status = counters("cpu")
    for rank, raised, draw, stat, _ in res:
        assert (raised, draw, stat) == (True, SLOT + 2, 0), rank
    for k in range(2):
        one = replay.minibatch(ring, pr, GLOO["B"], filled, SEED, ctr, status, impl="torch")
        for rank, *_, got in res:
            for name, v in got[k].items():
                assert same(torch.from_numpy(v), one[name]), (rank, k, name)
        want = expected(ring, one["global_row"].numpy())
        assert same(one["state"], want["state"]) and same(one["reward"], want["reward"])


# ---- argument checks (the library's host side; nothing is launched) -----------------------------
@pytest.fixture(scope="module")
def lib():
    from lnw import _abi
    from lnw.build import build as build_lib
    build_lib()
    return _abi.load()


def test_pack_and_mark_validate_arguments(lib):
    import ctypes
    from lnw import _abi
    some = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(some) + 15) & ~15  # (a 16-B aligned address; never dereferenced)
    ptrs = ("state", "next_state", "action", "reward", "done", "row_out", "xbuf")

    def call(**kw):
        a = _abi.ReplayPackArgs()
        for k in ptrs:
            setattr(a, k, p)
        a.cap, a.E, a.n, a.D, a.batch, a.rank, a.xbuf_words = 64, 1000, 4, 68, 64, 1, 1 << 40
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.lnw_replay_pack(ctypes.byref(a), None)

    words = lib.lnw_replay_pack_words
    assert lib.lnw_replay_pack(None, None) == -1
    bad = [{k: None} for k in ptrs] + [
        dict(batch=0), dict(batch=_abi.LNW_SAMPLE_MAX_BATCH + 1), dict(D=48), dict(D=66), dict(D=104), dict(n=0),
        dict(n=17), dict(rank=-1), dict(rank=64), dict(E=0), dict(cap=0), dict(E=1 << 25), dict(row_base=-1),
        dict(row_base=(1 << 40) - 63999), dict(state=p + 4), dict(next_state=p + 8), dict(action=p + 4),
        dict(xbuf=p + 4), dict(reward=p + 2), dict(reward=p + 4, reward_f64=1), dict(done=p + 2), dict(row_out=p + 4),
        dict(src_rank=p + 2), dict(index_out=p + 4), dict(xbuf_words=words(64, 4, 68, 0) - 1)]
    for kw in bad:
        assert call(**kw) < 0, kw
    assert call(D=48) == call(D=104) == call(D=66) == call(n=17) == call(batch=0) == call(rank=64) == -5
    assert call(E=0) == call(row_base=-1) == -1
    for B, n, D, f64 in ((64, 4, 68, 0), (7, 3, 100, 1), (1, 16, 52, 0), (131072, 16, 100, 1), (15, 1, 52, 0)):
        assert words(B, n, D, f64) == replay.pack_words(B, n, D, f64) and words(B, n, D, f64) % 4 == 0
    assert words(0, 4, 68, 0) == words(64, 4, 66, 0) == words(64, 17, 68, 0) == words(131073, 4, 68, 0) == 0

    def mark(**kw):
        a = _abi.ReplayMarkArgs()
        a.priority, a.reward, a.E, a.cap, a.k, a.n = p, p, 8, 4, 3, 2
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.lnw_replay_mark(ctypes.byref(a), None)

    assert lib.lnw_replay_mark(None, None) == -1
    for kw in (dict(priority=None), dict(k=4), dict(k=-1), dict(E=0), dict(cap=0), dict(n=0), dict(n=17),
               dict(priority=p + 2), dict(reward=p + 4, reward_f64=1), dict(E=1 << 30)):
        assert mark(**kw) < 0, kw
    del some
