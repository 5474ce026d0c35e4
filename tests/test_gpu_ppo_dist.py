"""Training over sharded rollouts on the GPU: lnw_ppo_sample_merge and
lnw_ppo_rows_pack with one process playing the ranks (_ppo_dist_cases.py), every
result compared bit for bit with one minibatch() over all rows and plain
indexing of the whole rollout; grad() on the packed batch against grad() on the
in-place batch; two rank processes on cuda:0 over gloo training as one rank
does; and one rank over RCCL (the device-tensor collectives)."""
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from _ppo_dist_cases import CASES, SEED, SLOT, bits, build, check_rank, plant, play, rollout
from _ppolearn_util import random_nets
from lnw import ppodist
from lnw.ppolearn import PPOLearner

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    actor, critic = random_nets(4, 68, 1)
    return PPOLearner(actor, critic, sample_seed=5)


def whole_draw(H, whole, B, base):
    H.draw.fill_(SLOT)
    one = H.minibatch(whole, B, seed=SEED, row_base=base, advance=False)
    return {k: v.clone() for k, v in one.items() if k != "obs"}, int(H.sample_status)


@pytest.mark.parametrize("name", list(CASES))
def test_played_ranks_equal_one_minibatch(H, name):
    case = CASES[name]
    whole, ranges, B, n, D, base = build(case, "cuda")
    one, status = whole_draw(H, whole, B, base)
    rows = one["index"].cpu().numpy() + base
    if case.get("planted"):
        spots = plant(whole, [int(rows[0] - base), int(rows[1] - base)], n)
        one, status = whole_draw(H, whole, B, base)
        assert np.array_equal(one["index"].cpu().numpy() + base, rows)
    got, own, lists, stat = play(H, whole, ranges, B, n, base, "hip")
    assert int(H.draw) == SLOT
    for w, g in enumerate(got):
        check_rank(g, whole, rows, bits(one["key"]), n, base)
        for k in ("actions", "old_log_probs", "rtg", "old_values"):
            assert np.array_equal(bits(g[k]), bits(one[k])), k
        assert stat[w] == status
        for k in g:  # all played ranks hold identical results
            assert np.array_equal(bits(g[k]), bits(got[0][k])), (w, k)
        assert own[w].numel() == ppodist.pack_words(B, n, D)
    # every word of the sum comes from exactly one played rank, and each rank's buffer is its own slots only
    assert int(torch.stack([o != 0 for o in own]).sum(0).max()) <= 1
    src = torch.zeros(B, dtype=torch.int64)
    for w, (lo, hi) in enumerate(ranges):
        src[torch.from_numpy((rows - base >= lo) & (rows - base < hi))] = w
    m = ppodist.merge(lists, B, n, "hip")
    assert torch.equal(m["src_rank"].cpu().long(), src)
    pos = m["src_pos"].cpu().long()
    assert torch.equal(lists.cpu()[src, B + pos], torch.from_numpy(rows))
    for w in range(len(ranges)):
        theirs = ppodist.unpack(own[w], m, n, D)
        other = (src != w).cuda()
        for k in ("obs", "actions", "old_log_probs", "rtg", "old_values"):
            assert not bool(theirs[k].view(torch.int32)[other].any()), (w, k)
    if "quiet" in case:
        q = case["quiet"]
        assert not bool((src == q).any())  # the quiet shard owns no winner ...
        assert not bool(own[q].any())      # ... and its exchange buffer is all zero words
        assert all(bool(own[w].any()) for w in range(len(ranges)) if w != q)
    if case.get("nonfinite"):
        k = one["key"].cpu().numpy()
        assert np.isfinite(k[:60]).all() and np.isinf(k[60:]).all() and status == 220
        assert np.isinf(lists[0, :B].view(torch.float64).cpu().numpy()).sum() == 80  # +inf keys in both lists
        assert (src[60:] == 1).all() and np.array_equal(rows[60:], np.sort(rows[60:]))
    if case.get("planted"):
        for name_, pos_, b in spots:
            flat = bits(got[1]["obs" if name_ == "obs" else "actions"]).reshape(-1)
            assert b in flat.tolist(), (name_, pos_)
    if "same_group" in case:
        grp, s0, s1 = case["same_group"]
        where = {int(r): s for s, r in enumerate(rows - base)}
        a, b = where[grp * n + s0], where[grp * n + s1]
        assert torch.equal(got[0]["obs"][a].view(torch.int32), got[0]["obs"][b].view(torch.int32))
    if case.get("base"):
        assert int(rows.min()) > 2 ** 33


def test_torch_arm_equals_kernels_on_the_device(H):
    """impl="torch" on device tensors: the same merge and the same buffer."""
    whole, ranges, B, n, D, base = build(CASES["batch_70"], "cuda")
    gh, oh, lists, _ = play(H, whole, ranges, B, n, base, "hip")
    gt, ot, _, _ = play(H, whole, ranges, B, n, base, "torch")
    for w in range(len(ranges)):
        assert torch.equal(oh[w], ot[w])
        for k in gh[w]:
            assert np.array_equal(bits(gh[w][k]), bits(gt[w][k])), k


@pytest.mark.parametrize("n,D", [(4, 68), (2, 60)])
def test_grad_on_the_packed_batch(n, D):
    """grad() on minibatch_dist's packed batch equals grad() on rows(out,
    global_row), the in-place batch: gradients, losses and per-row outputs."""
    actor, critic = random_nets(n, D, 3)
    P, Q = PPOLearner(actor, critic, sample_seed=7), PPOLearner(actor, critic, sample_seed=7)
    whole = rollout(60 * n, n, D, 41, "cuda")
    packed = P.minibatch_dist(whole, 64, row_base=0)  # no process group: a world of one
    a = P.grad(packed)
    b = Q.grad(Q.rows(whole, packed["global_row"]))
    assert packed["obs"].data_ptr() != whole["obs"].data_ptr() and packed["obs"].shape == (64, n, D)
    for k in ("actor_grad", "critic_grad", "actor_loss", "critic_loss", "new_log_probs", "entropies", "values",
              "advantage"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert bool(a["actor_loss"].isfinite()) and bool(a["critic_loss"].isfinite())
    assert torch.equal(P.theta_actor, Q.theta_actor)  # (the running statistics' updates)


def test_minibatch_dist_raises_before_it_draws(H):
    whole = rollout(400, 4, 68, 43, "cuda")
    H.draw.fill_(2)
    with pytest.raises(ValueError):
        H.minibatch_dist(whole, 401, row_base=0)
    with pytest.raises(ValueError):
        H.minibatch_dist(whole, 64, row_base=6)
    assert int(H.draw) == 2


# ---- rank processes ------------------------------------------------------------------
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


def _ranks(tmp_path, world, total, mode):
    port = _port()
    procs = []
    for r in range(world):
        env = dict(os.environ, WORLD_SIZE=str(world), RANK=str(r), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        env.pop("TORCHELASTIC_RUN_ID", None)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_ppo_dist_rank.py"),
                                       str(tmp_path / f"{mode}_w{world}_r{r}.npz"), str(total), mode], env=env))
    _wait_all(procs, 240)
    return [np.load(tmp_path / f"{mode}_w{world}_r{r}.npz") for r in range(world)]


STATE = ("theta_actor", "theta_critic", "m_actor", "v_actor", "m_critic", "v_critic", "step_actor", "step_critic",
         "draw", "nbt", "sample_status", "losses", "rows")


def _same(a, b, k):
    assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
    assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.fixture(scope="module")
def one_rank_plain(tmp_path_factory):
    """The one-rank run over 65 envs through minibatch(), made once."""
    return _ranks(tmp_path_factory.mktemp("one"), 1, 65, "plain")[0]


@pytest.mark.parametrize("total,mode", [(65, "plain"), (66, "noise")])
def test_two_ranks_train_as_one(tmp_path, one_rank_plain, total, mode):
    """rollout -> 3 x (minibatch_dist(64) -> step) -> rollout -> 2 more steps in
    two rank processes (gloo, both on cuda:0; shards of 33 and 32 envs, or 33
    and 33 with parameter noise in members of 11): both ranks end with the
    parameters, Adam moments, counters, losses and drawn global rows, bit for
    bit, of one rank doing the same over all envs with minibatch()."""
    one = one_rank_plain if mode == "plain" else _ranks(tmp_path, 1, total, mode)[0]
    two = _ranks(tmp_path, 2, total, mode)
    assert [(int(d["lo"]), int(d["hi"])) for d in two] == [(0, 33), (33, total)]
    assert str(one["backend"]) == "None" and all(str(d["backend"]) == "gloo" for d in two)
    for k in STATE:
        _same(two[0], two[1], k)
        _same(two[0], one, k)
    assert one["draw"].tolist() == [5] and one["step_actor"].tolist() == [5] and one["rows"].shape == (5, 64)
    assert np.isfinite(one["losses"]).all()
    # rows of both shards are drawn, and the second rollout's draws differ from the first's
    per = 8 * 4 * 33
    assert (one["rows"] < per).any() and (one["rows"] >= per).any()
    assert not np.array_equal(one["rows"][2], one["rows"][3])


def test_one_rank_over_rccl(tmp_path, one_rank_plain):
    """One rank under torch.distributed.run with the nccl backend: the all-gather
    and the int32 all-reduce run on device tensors through RCCL, and the run
    equals the one-rank run through minibatch() bit for bit."""
    one = one_rank_plain
    env = {k: v for k, v in os.environ.items() if k not in ("LNW_DIST_BACKEND", "WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "rccl.npz"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", os.path.join(ROOT, "tests", "_ppo_dist_rank.py"),
           str(out), "65", "plain", "nccl"]
    _wait_all([subprocess.Popen(cmd, env=env, cwd=ROOT)], 240)
    got = np.load(out)
    assert str(got["backend"]) == "nccl"
    for k in STATE:
        _same(got, one, k)
