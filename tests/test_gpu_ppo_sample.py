"""lnw_ppo_sample / PPOLearner.minibatch on the GPU against the NumPy
restatement (_ppo_sample_ref.py): the index, the keys bit for bit and the
gathered tensors, at the base shapes and at every internal boundary of the
kernels (_ppo_sample_cases.py names them), over the rtg patterns; the device
counter, non-finite rows, the shard merge, one captured graph of draw + update
replayed per epoch, and the draw behind a real rollout."""
import copy

import numpy as np
import pytest
import torch

import _ppo_sample_ref as ref
from _ppo_sample_cases import BIG_BASE, BOUNDARY_CASES, BASE_CASES, PATTERNS, make_out, rtg_pattern, ships
from _ppolearn_util import random_nets
from lnw.ppolearn import PPOLearner

pytestmark = pytest.mark.gpu
SEED = 0x123456789ABCDEF


@pytest.fixture(scope="module")
def H():
    actor, critic = random_nets(4, 68, 1)
    return PPOLearner(actor, critic, sample_seed=SEED)


def check(H, rtg, B, base=0, slot=0, n=None, advance=True):
    N = len(rtg)
    n = ships(N) if n is None else n
    out = make_out(rtg, n, "cuda")
    H.draw.fill_(slot)
    b = H.minibatch(out, B, row_base=base, advance=advance)
    idx, key = ref.draw(rtg, B, SEED, slot=slot, row_base=base)
    got = b["index"].cpu().numpy()
    assert b["index"].dtype == torch.int64 and b["key"].dtype == torch.float64
    assert np.array_equal(got, idx), (np.flatnonzero(got != idx)[:5], got[:5], idx[:5])
    assert np.array_equal(b["key"].cpu().numpy().view(np.uint64), key.view(np.uint64))
    want = H.rows(out, b["index"])
    for k in ("actions", "old_log_probs", "rtg", "old_values"):
        assert torch.equal(b[k].view(torch.int32), want[k].view(torch.int32)), k  # (bitwise: NaN rows too)
    assert b["obs"].data_ptr() == out["obs"].data_ptr()
    assert int(H.draw) == slot + int(advance)
    return b


@pytest.mark.parametrize("N,B", BASE_CASES + BOUNDARY_CASES)
def test_equals_restatement(H, N, B):
    b = check(H, rtg_pattern("normal0", N), B, base=BIG_BASE if N % 2 else 0, slot=N % 7)
    if N == B:
        assert sorted(b["index"].tolist()) == list(range(N))  # every row is drawn: a permutation
    assert int(H.sample_status) == 0


@pytest.mark.parametrize("N,B", [(257, 64), (4099, 64), (20000, 1000)])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_patterns(H, pattern, N, B):
    check(H, rtg_pattern(pattern, N), B, base=BIG_BASE if pattern in ("normal1", "zero", "extreme") else 0, slot=5)


@pytest.mark.parametrize("n", [1, 4])
def test_old_values_per_group(H, n):
    check(H, rtg_pattern("normal2", 1024), 100, n=n)


def test_counter(H):
    """Two draws that advance the counter are slots 0 and 1 and leave it at 2;
    a draw that does not advance repeats itself bitwise."""
    rtg = rtg_pattern("normal1", 4099)
    out = make_out(rtg, 1, "cuda")
    H.draw.zero_()
    for slot in (0, 1):
        b = H.minibatch(out, 64)
        idx, key = ref.draw(rtg, 64, SEED, slot=slot)
        assert np.array_equal(b["index"].cpu().numpy(), idx)
        assert np.array_equal(b["key"].cpu().numpy().view(np.uint64), key.view(np.uint64))
    assert int(H.draw) == 2
    first = {k: v.clone() for k, v in H.minibatch(out, 64, advance=False).items()}
    again = H.minibatch(out, 64, advance=False)
    assert int(H.draw) == 2 and not np.array_equal(first["index"].cpu().numpy(), idx)
    for k in first:
        assert torch.equal(first[k], again[k]), k


def test_nonfinite_rows(H):
    rtg = rtg_pattern("normal1", 300)
    bad = [3, 50, 51, 120, 200, 298, 299]
    rtg[bad] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan]
    b = check(H, rtg, 64)
    assert int(H.sample_status) == 7 and not set(b["index"].tolist()) & set(bad)
    b = check(H, rtg, 300)
    assert int(H.sample_status) == 7 and b["index"][-7:].tolist() == bad
    assert sorted(b["index"].tolist()) == list(range(300))
    # every row non-finite: the draw is the first rows, in row order
    b = check(H, np.full(500, np.nan, np.float32), 70)
    assert b["index"].tolist() == list(range(70)) and int(H.sample_status) == 500


@pytest.mark.parametrize("base", [0, BIG_BASE])
def test_shard_merge_on_device(H, base):
    """Two calls over halves of the rows, merged by key_out, equal one call."""
    rtg = rtg_pattern("normal2", 6000)
    whole = check(H, rtg, 256, base=base, slot=4, advance=False)
    widx, wkey = whole["index"].cpu().numpy(), whole["key"].cpu().numpy()
    parts = []
    for lo, hi in ((0, 2600), (2600, 6000)):
        b = check(H, rtg[lo:hi], 256, base=base + lo, slot=4, advance=False)
        parts.append((base + lo, b["index"].cpu().numpy(), b["key"].cpu().numpy()))
    g, k = ref.merge(parts, 256)
    assert np.array_equal(g, base + widx) and np.array_equal(k.view(np.uint64), wkey.view(np.uint64))


def synthetic_rollout(E, T, n, D, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand((E * T, n, D), generator=g)
    obs[..., :49] = torch.randint(0, 256, (E * T, n, 49), generator=g) / 255.0
    return {k: v.cuda() for k, v in dict(
        obs=obs, rtg=1.0 + 2.0 * torch.randn((E, T, n), generator=g), actions=torch.rand((E, T, n, 4), generator=g),
        log_probs=-1.0 + 0.3 * torch.randn((E, T, n, 4), generator=g),
        values=0.3 * torch.randn((E, T), generator=g)).items()}


def test_graph_capture_of_draw_and_update():
    """learner.step(learner.minibatch(out, 64)) captured once and replayed three
    times equals three eager calls on a second learner from the same state:
    both vectors, the Adam moments, the counter (3) and the last index."""
    n, D = 2, 60
    actor, critic = random_nets(n, D, 8)
    out = synthetic_rollout(16, 5, n, D, 9)
    G, E = PPOLearner(actor, critic, lr=1e-3, sample_seed=3), PPOLearner(actor, critic, lr=1e-3, sample_seed=3)
    # (sizes the draw's buffers and the update's workspace outside the capture; changes no state)
    G.grad(G.minibatch(out, 64, advance=False), update_running=False)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        b = G.minibatch(out, 64)
        loss = torch.stack(G.step(b))
    assert int(G.draw) == 0
    glosses, elosses, seen = [], [], []
    for _ in range(3):
        gr.replay()
        glosses.append(loss.clone())
        seen.append(b["index"].clone())
    for _ in range(3):
        eb = E.minibatch(out, 64)
        elosses.append(torch.stack(E.step(eb)))
    torch.cuda.synchronize()
    assert int(G.draw) == int(E.draw) == 3 and int(G.step_actor) == int(E.step_actor) == 3
    assert torch.equal(seen[2], eb["index"]) and not torch.equal(seen[0], seen[1])
    for k in ("theta_actor", "theta_critic", "m_actor", "v_actor", "m_critic", "v_critic"):
        assert torch.equal(getattr(G, k), getattr(E, k)), k
    assert torch.equal(torch.stack(glosses), torch.stack(elosses)) and bool(torch.stack(glosses).isfinite().all())


def test_with_the_rollout():
    """Rollout.run() at 2v2 -> minibatch(out, 16) -> step: the kernels and the
    torch arm draw the same rows, and their losses agree as a step's do
    (test_gpu_ppolearn.py: 1e-4 relative)."""
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    from lnw.rollout import BatchedActor, BatchedCritic, Rollout
    E, T = 8, 5
    REF_BLUE, REF_RED = [(6, 61), (10, 81)], [(98, 48), (98, 52)]

    def close_loss(name, got, want, rel):
        got, want = float(got), float(want)
        print(f"{name}: {got!r} against {want!r}")
        assert abs(got - want) <= rel * abs(want), (name, got, want)

    sc = Scenario(landing_ops=False, auto_reset=False, trained_red=False)
    g = BatchedGame(E, ["small"] * 2, ["large"] * 2, scenario=sc, seed=3)
    g.reset(positions=REF_BLUE + REF_RED, box=((40, 40), (57, 65)))
    torch.manual_seed(4)
    actor, critic = BatchedActor.for_obs(g.Db).cuda(), BatchedCritic(g.Db * g.nb).cuda()
    actor_t, critic_t = copy.deepcopy(actor), copy.deepcopy(critic)
    r = Rollout(g, actor, critic, steps=T, stop_at_done=False, seed=5)
    out = {k: v.clone() for k, v in r.run().items()}
    rtg = torch.randn((E, T, g.nb), generator=torch.Generator().manual_seed(1), dtype=torch.float64).cuda()
    Hl = PPOLearner(actor, critic, sample_seed=6)
    Tm = PPOLearner(actor_t, critic_t, impl="torch", device="cuda", sample_seed=6)
    bh, bt = Hl.minibatch(out, 16, rtg=rtg), Tm.minibatch(out, 16, rtg=rtg)
    assert torch.equal(bh["index"], bt["index"]) and torch.equal(bh["key"], bt["key"])
    assert len(set(bh["index"].tolist())) == 16 and bh["obs"].data_ptr() == out["obs"].data_ptr()
    for k in ("actions", "old_log_probs", "rtg", "old_values"):
        assert torch.equal(bh[k], bt[k]), k
    lh, lt = Hl.step(bh), Tm.step(bt)
    assert all(bool(x.isfinite()) for x in lh)
    close_loss("actor loss", lh[0], lt[0], 1e-4)
    close_loss("critic loss", lh[1], lt[1], 1e-4)
    g.close()
