"""DDQN replay on the GPU: lnw_replay_mark, the keyed draw and lnw_replay_pack
against lnw/replay.py's torch arm bit for bit (_replay_cases.py), one process
playing the ranks; a real collector whose ring wraps; the learner stepping on a
minibatch against stepping on the torch-gathered rows; minibatch -> step
captured in one graph; two rank processes on cuda:0 over gloo training as one
rank does; and one rank over RCCL."""
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from _replay_cases import (CASES, FILL, SEED, SLOT, bits, build, check_rows, counters, direct_rows, play,
                           priority_restated, same)
from _replay_rank import make_collector
from lnw import replay

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", list(CASES))
def test_mark_draw_and_pack_equal_the_torch_arm(case):
    c = CASES[case]
    B = c["B"]
    ring, pr, filled, _ = build(case, "cuda", "hip")
    tring, tpr, _, _ = build(case, "cpu", "torch")
    assert same(pr, tpr)  # lnw_replay_mark, step by step, wraps included
    for k in ring:
        assert same(ring[k], tring[k]), k
    ctr, status = counters("cuda")
    cache = {}
    replay.minibatch(ring, pr, B, filled, SEED, ctr, status, advance=False, cache=cache)
    xbuf = cache[("local", B)]["xbuf"]
    xbuf.fill_(FILL)
    cache[("local", B)]["ring_index"].fill_(-9)
    got = replay.minibatch(ring, pr, B, filled, SEED, ctr, status, cache=cache)
    tctr, tstatus = counters("cpu")
    tcache = {}
    want = replay.minibatch(tring, tpr, B, filled, SEED, tctr, tstatus, impl="torch", cache=tcache)
    for k in want:
        assert same(got[k], want[k]), k
    # the whole buffer, padding included: every word written, none left at the fill
    assert torch.equal(xbuf.cpu(), tcache[("local", B)]["xbuf"])
    assert got["state"].data_ptr() == xbuf.data_ptr()
    assert int(ctr) == int(tctr) == SLOT + 1 and int(status) == int(tstatus) == sum(c["shards"]) * (c["cap"] - filled)
    rows, keys = direct_rows(tpr, B, SEED, SLOT)
    check_rows(got, ring, rows, keys)


@pytest.mark.parametrize("case", ["ranks", "quiet"])
def test_played_ranks_sum_to_the_whole(case):
    c = CASES[case]
    B = c["B"]
    ring, pr, filled, ranges = build(case, "cuda", "hip")
    ctr, status = counters("cuda")
    one = {k: v.clone() for k, v in replay.minibatch(ring, pr, B, filled, SEED, ctr, status, advance=False).items()}
    got, own, lists, merged = play(ring, pr, filled, ranges, B, "hip")
    tring, tpr, _, _ = build(case, "cpu", "torch")
    tgot, town, tlists, _ = play(tring, tpr, filled, ranges, B, "torch")
    assert torch.equal(lists.cpu(), tlists)
    for k in got:
        assert same(got[k], one[k]) and same(got[k], tgot[k]), k
    for w in range(len(ranges)):
        assert torch.equal(own[w].cpu(), town[w]), w
    assert int(torch.stack([o != 0 for o in own]).sum(0).max()) <= 1
    if "quiet" in c:
        assert not bool(own[c["quiet"]].any()) and not bool((merged["src_rank"] == c["quiet"]).any())


def test_owned_slot_with_a_row_outside_the_ring_is_zeros():
    """An argument check: a valid merge whose slot 0 is given the global row just
    past its owner's ring. The owner writes zero words for it, nothing is read
    there, and every other slot is unchanged."""
    c = CASES["ranks"]
    B, n, D, cap = c["B"], c["n"], c["D"], c["cap"]
    ring, pr, filled, ranges = build("ranks", "cuda", "hip")
    good, *_ = play(ring, pr, filled, ranges, B, "hip")
    good = {k: v.clone() for k, v in good.items()}

    def edit(m):
        w = int(m["src_rank"][0])
        m["global_row"][0] = ranges[w][1] * cap

    got, own, _, merged = play(ring, pr, filled, ranges, B, "hip", edit=edit)
    tring, tpr, _, _ = build("ranks", "cpu", "torch")
    tgot, town, _, _ = play(tring, tpr, filled, ranges, B, "torch", edit=edit)
    for w in range(len(ranges)):
        assert torch.equal(own[w].cpu(), town[w]), w
    for k in replay.ROW_KEYS:
        per = got[k].reshape(B, -1)
        assert not bool(per[0].view(torch.int32).any()), k
        assert same(per[1:], good[k].reshape(B, -1)[1:]), k
    # and with every slot owned (src_rank NULL) the ring index reports it
    idx = torch.full((B,), -9, dtype=torch.int64, device="cuda")
    rows = merged["global_row"].clone()
    rows[1] = -1
    x = replay.pack(ring, rows, index_out=idx)
    whole = replay.unpack(x, B, n, D, True)
    assert idx[1].item() == -1 and not bool(whole["state"].reshape(B, -1)[1].view(torch.int32).any())
    assert (idx[2:] >= 0).all()


# ---- a real collector ---------------------------------------------------------------------
def test_collector_marks_draws_and_packs():
    """DISCRETE 2v2, E = 8, cap = 4, priority="reward", 6 steps: the ring wraps."""
    g, net, c = make_collector(8)
    g0, _, twin = make_collector(8, priority=None)
    assert twin.priority is None and not hasattr(twin, "draw")
    for _ in range(6):
        c.step(eps=0.5)
        twin.step(eps=0.5)
    for k, v in c.ring().items():  # the priorities change nothing in the ring
        assert same(v, twin.ring()[k]), k
    assert bool(c.reward.abs().sum() > 0)
    assert np.array_equal(bits(c.priority), priority_restated(c.ring(), 4).view(np.int32))
    assert c.priority.shape == (8, 4) and c.draw.tolist() == [0]
    b = c.minibatch(8)
    assert c.draw.tolist() == [1] and c.sample_status.tolist() == [0]
    rows, keys = direct_rows(c.priority, 8, 19, 0)
    check_rows(b, c.ring(), rows, keys)
    s = c.sample(8)
    assert s["state"].shape == (8, 2, g.Db) and s["done"].shape == (8,)
    with pytest.raises(RuntimeError):
        twin.minibatch(8)
    with pytest.raises(ValueError):
        c.minibatch(33)
    # a caller's priorities are read at draw time: all weight on one env
    c.priority.fill_(0.0)
    c.priority[5] = 1e6
    b = c.minibatch(4)
    assert sorted(b["global_row"].tolist()) == [20, 21, 22, 23]
    g.close()
    g0.close()


def test_uniform_collector_and_env_id_base():
    g, net, c = make_collector(4, lo=3, priority="uniform")
    for _ in range(2):
        c.step(eps=0.5)
    p = c.priority.cpu().numpy()
    assert (p[:, :2] == 1.0).all() and np.isnan(p[:, 2:]).all()
    b = c.minibatch(8, seed=7)  # every transition, once
    assert sorted(b["global_row"].tolist()) == [12, 13, 16, 17, 20, 21, 24, 25]
    assert c.sample_status.tolist() == [8]
    rows, keys = direct_rows(c.priority, 8, 7, 0, row_base=12)
    check_rows(b, c.ring(), rows, keys, row_base=12)
    g.close()


def test_learner_steps_on_the_minibatch():
    from lnw.qlearn import QLearner
    g, net, c = make_collector(8)
    for _ in range(3):
        c.step(eps=0.5)
    A, B = QLearner(net, lr=1e-3), QLearner(net, lr=1e-3)
    mb = c.minibatch(16)
    r = A.rows(mb)
    for k in replay.ROW_KEYS:
        assert r[k].data_ptr() == mb[k].data_ptr(), k  # rows() is a no-op: the same storage
    idx = mb["index"]
    flat = lambda t: t.reshape((c.cap * g.E,) + tuple(t.shape[2:]))  # noqa: E731
    gathered = dict(state=flat(c.state)[idx], action=flat(c.action)[idx], reward=flat(c.reward)[idx],
                    next_state=flat(c.next_state)[idx], done=flat(c.done)[idx])
    la, lb = A.step(mb), B.step(gathered)
    assert bool(la.isfinite()) and same(la, lb)
    for k in ("theta", "m", "v", "theta_target", "step_count", "nbt"):
        assert same(getattr(A, k), getattr(B, k)), k
    g.close()


def _graph_run(graph):
    from lnw.qlearn import QLearner
    g, net, c = make_collector(8)
    L = QLearner(net, lr=1e-3)
    for _ in range(2):
        c.step(eps=0.5)
    rows, losses = [], []
    if graph:
        mb = c.minibatch(8, advance=False)          # (sizes the buffers and the workspace outside the capture)
        L.grad(mb, update_running=False)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            mb = c.minibatch(8)
            loss = L.step(mb)
    for _ in range(3):
        if graph:
            gr.replay()
        else:
            mb = c.minibatch(8)
            loss = L.step(mb)
        rows.append(mb["global_row"].clone())
        losses.append(loss.clone())
        c.step(eps=0.5)
    torch.cuda.synchronize()
    out = dict(theta=L.theta.clone(), m=L.m.clone(), v=L.v.clone(), target=L.theta_target.clone(),
               rows=torch.stack(rows), losses=torch.stack(losses), draw=c.draw.clone(), steps=L.step_count.clone())
    g.close()
    return out


def test_graph_replay_draws_afresh():
    """One capture of minibatch -> learner.step, replayed three times with eager
    collector steps between, equals the same sequence run eagerly; every replay
    draws afresh and reads the ring as it is then."""
    eager, graph = _graph_run(False), _graph_run(True)
    for k in eager:
        assert same(eager[k], graph[k]), k
    assert eager["draw"].tolist() == [3] and eager["steps"].tolist() == [3]
    r = eager["rows"].tolist()
    assert r[0] != r[1] and r[1] != r[2] and r[0] != r[2]
    assert bool(eager["losses"].isfinite().all())


# ---- rank processes --------------------------------------------------------------------------
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _wait_all(procs, limit):
    """Every child's exit status 0 within `limit` seconds; the first failure or
    the time limit kills the siblings."""
    deadline = time.monotonic() + limit
    try:
        while any(p.poll() is None for p in procs):
            assert time.monotonic() < deadline, "a rank ran into the time limit"
            for p in procs:
                try:
                    p.wait(timeout=0.2)
                except subprocess.TimeoutExpired:
                    pass
            assert all(p.poll() in (None, 0) for p in procs), [p.poll() for p in procs]
        assert all(p.returncode == 0 for p in procs), [p.returncode for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()


SCRIPT = os.path.join(ROOT, "tests", "_replay_rank.py")
STATE = ("theta", "theta_target", "m", "v", "step_count", "nbt", "draw", "sample_status", "losses", "rows")


def _ranks(tmp_path, world, total):
    """`world` rank processes at once (the parent holds the GPU too: at most
    three processes)."""
    port = _port()
    procs = []
    for r in range(world):
        env = dict(os.environ, WORLD_SIZE=str(world), RANK=str(r), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        env.pop("TORCHELASTIC_RUN_ID", None)
        procs.append(subprocess.Popen([sys.executable, SCRIPT, str(tmp_path / f"w{world}_r{r}.npz"), str(total),
                                       "gloo" if world > 1 else "none"], env=env))
    _wait_all(procs, 240)
    return [np.load(tmp_path / f"w{world}_r{r}.npz") for r in range(world)]


def _same(a, b, k):
    assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
    assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    """The one-rank run over 9 envs through minibatch(), made once."""
    return _ranks(tmp_path_factory.mktemp("one"), 1, 9)[0]


def test_two_ranks_train_as_one(tmp_path, one_rank):
    """Two rank processes (gloo, both on cuda:0) with collectors over 5 + 4 of 9
    envs, six iterations of step -> minibatch_dist(8) -> learner.step with one
    sync_target: both end with the parameters, Adam moments, counters, losses and
    drawn global rows, bit for bit, of one rank over 9 envs using minibatch()."""
    two = _ranks(tmp_path, 2, 9)
    assert [(int(d["lo"]), int(d["hi"])) for d in two] == [(0, 5), (5, 9)]
    assert str(one_rank["backend"]) == "None" and all(str(d["backend"]) == "gloo" for d in two)
    for k in STATE:
        _same(two[0], two[1], k)
        _same(two[0], one_rank, k)
    assert one_rank["draw"].tolist() == [6] and one_rank["step_count"].tolist() == [6]
    assert one_rank["sample_status"].tolist() == [0] and one_rank["rows"].shape == (6, 8)
    assert np.isfinite(one_rank["losses"]).all()
    rows = one_rank["rows"]
    assert (rows < 20).any() and (rows >= 20).any()  # both shards' transitions are drawn
    assert not np.array_equal(rows[0], rows[1])


def test_one_rank_over_rccl(tmp_path, one_rank):
    """One rank under torch.distributed.run with the nccl backend: the all-gather
    and the int32 all-reduce run on device tensors through RCCL, and the run
    equals the one-rank run through minibatch() bit for bit."""
    env = {k: v for k, v in os.environ.items() if k not in ("LNW_DIST_BACKEND", "WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "rccl.npz"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", SCRIPT, str(out), "9", "nccl"]
    _wait_all([subprocess.Popen(cmd, env=env, cwd=ROOT)], 240)
    got = np.load(out)
    assert str(got["backend"]) == "nccl"
    for k in STATE:
        _same(got, one_rank, k)
