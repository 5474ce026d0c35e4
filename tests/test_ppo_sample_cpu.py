"""The keyed minibatch draw (lnw_ppo_sample, PPOLearner.minibatch) without a
GPU: the definition's distribution is the reference sampler's (sequential
weighted sampling without replacement, in draw order), shards merge into the
whole draw, p_log is accurate enough for it, the learner's torch arm equals the
NumPy restatement bit for bit, and the entry point validates its arguments
before it launches anything."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _ppo_sample_ref as ref
from _ppo_sample_cases import BIG_BASE, BOUNDARY_CASES, BASE_CASES, PATTERNS, make_out, rtg_pattern, ships
from lnw import _abi
from lnw.build import build
from lnw.ppolearn import PPOLearner

RTG5 = np.array([0.0, -3.0, 1.0, 0.5, 2.0], np.float32)
DRAWS, SEED = 20000, 2024


@pytest.fixture(scope="module")
def pairs():
    """The first two draws of DRAWS minibatches of RTG5 (slots 0 .. DRAWS - 1)."""
    k = ref.keys(RTG5, SEED, slot=np.arange(DRAWS))
    return np.argsort(k, axis=1, kind="stable")[:, :2]


def weights():
    return (np.abs(RTG5) + np.float32(1e-5)).astype(np.float64)


def test_header_constants_match():
    assert (ref.CTR2, ref.CTR3) == (_abi.LNW_SAMPLE_CTR2, _abi.LNW_SAMPLE_CTR3)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "lnw.h")).read()
    assert f"#define LNW_SAMPLE_CTR2 0x{ref.CTR2:08X}u" in src and f"#define LNW_SAMPLE_CTR3 0x{ref.CTR3:08X}u" in src
    # a domain of its own: not philox_u4's counter words
    assert (ref.CTR2, ref.CTR3) != (0x243F6A88, 0x85A308D3)


def test_distribution_of_ordered_pairs(pairs):
    """Every ordered pair (i, j) with an expected count above 5 is drawn T p
    times within 5 sigma, p = w_i / W * w_j / (W - w_i)."""
    w = weights()
    W = w.sum()
    cells = 0
    for i in range(5):
        for j in range(5):
            if i == j:
                continue
            p = w[i] / W * w[j] / (W - w[i])
            if DRAWS * p <= 5:
                continue
            cells += 1
            count = int(((pairs[:, 0] == i) & (pairs[:, 1] == j)).sum())
            sigma = math.sqrt(DRAWS * p * (1 - p))
            print(f"({i}, {j}): {count} drawn, {DRAWS * p:.1f} expected, {(count - DRAWS * p) / sigma:+.2f} sigma")
            assert abs(count - DRAWS * p) <= 5 * sigma, (i, j, count, DRAWS * p)
    assert cells == 12  # (the pairs with row 0, of weight 1e-5, are below 5)


def test_first_row_marginal_is_ascending_key_order(pairs):
    """The first row drawn is row i with probability w_i / W: a descending
    order, or a selection of the largest keys, fails this."""
    w = weights()
    for i in range(5):
        p = w[i] / w.sum()
        if DRAWS * p <= 5:
            continue
        count = int((pairs[:, 0] == i).sum())
        assert abs(count - DRAWS * p) <= 5 * math.sqrt(DRAWS * p * (1 - p)), (i, count, DRAWS * p)


@pytest.mark.parametrize("base", [0, BIG_BASE])
def test_shard_merge(base):
    rtg = rtg_pattern("normal0", 1000)
    idx, key = ref.draw(rtg, 64, 11, slot=3, row_base=base)
    lo = ref.draw(rtg[:400], 64, 11, slot=3, row_base=base)
    hi = ref.draw(rtg[400:], 64, 11, slot=3, row_base=base + 400)
    g, k = ref.merge([(base, *lo), (base + 400, *hi)], 64)
    assert np.array_equal(g, base + idx) and np.array_equal(k.view(np.uint64), key.view(np.uint64))


def test_p_log_accuracy():
    u = np.random.default_rng(0).random(100000)
    got = ref.p_log(1.0 - u)
    want = np.array([math.log1p(-x) for x in u])
    rel = np.abs(got - want) / np.abs(want)
    print("largest relative error of p_log against log1p:", rel.max())
    assert rel.max() <= 2e-15


@pytest.fixture(scope="module")
def learner():
    from _ppolearn_util import random_nets
    actor, critic = random_nets(4, 68, 1)
    return PPOLearner(actor, critic, impl="torch", device="cpu", sample_seed=5)


def check_against_restatement(L, N, B, pattern, base, slot):
    rtg = rtg_pattern(pattern, N)
    n = ships(N)
    out = make_out(rtg, n)
    L.draw.fill_(slot)
    b = L.minibatch(out, B, row_base=base)
    idx, key = ref.draw(rtg, B, L.sample_seed, slot=slot, row_base=base)
    assert int(L.draw) == slot + 1
    assert b["index"].dtype == torch.int64 and np.array_equal(b["index"].numpy(), idx)
    assert np.array_equal(b["key"].numpy().view(np.uint64), key.view(np.uint64))
    want = L.rows(out, torch.from_numpy(idx))
    for k in ("actions", "old_log_probs", "rtg", "old_values"):
        assert torch.equal(b[k], want[k]), k
    assert b["obs"].shape == want["obs"].shape
    return b


@pytest.mark.parametrize("N,B", BASE_CASES + BOUNDARY_CASES)
def test_torch_arm_equals_restatement(learner, N, B):
    check_against_restatement(learner, N, B, "normal0", BIG_BASE if N % 2 else 0, slot=N % 7)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_torch_arm_patterns(learner, pattern):
    b = check_against_restatement(learner, 4099, 64, pattern, 0, slot=2)
    assert len(set(b["index"].tolist())) == 64


def test_torch_arm_nonfinite_rows_come_last(learner):
    rtg = rtg_pattern("normal1", 300)
    bad = [3, 50, 51, 120, 200, 298, 299]
    rtg[bad] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan]
    out = make_out(rtg, 4)
    b = learner.minibatch(out, 64)
    assert int(learner.sample_status) == 7 and not set(b["index"].tolist()) & set(bad)
    b = learner.minibatch(out, 300)
    assert b["index"][-7:].tolist() == bad and sorted(b["index"].tolist()) == list(range(300))
    assert bool(torch.isinf(b["key"][-7:]).all()) and bool(torch.isfinite(b["key"][:-7]).all())


def test_minibatch_feeds_step(learner):
    """minibatch() is rows(out, index) with a key: step() takes it as it is."""
    from _ppolearn_util import random_batch, random_nets
    actor, critic = random_nets(4, 68, 2)
    L = PPOLearner(actor, critic, impl="torch", device="cpu")
    rb = random_batch(actor, critic, 64, 4, 68, 3)
    out = dict(obs=rb["obs"], rtg=rb["rtg"], actions=rb["actions"], log_probs=rb["old_log_probs"],
               values=rb["old_values"].reshape(-1, 4)[:, 0])
    b = L.minibatch(out, 16, seed=9)
    idx, _ = ref.draw(rb["rtg"].numpy(), 16, 9)
    assert np.array_equal(b["index"].numpy(), idx)
    al, cl = L.step(b)
    assert bool(al.isfinite()) and bool(cl.isfinite()) and int(L.draw) == 1
    with pytest.raises(ValueError):
        L.minibatch(out, 65)


def test_entry_point_validates_arguments():
    build()
    L = _abi.load()
    assert L.lnw_ppo_sample(None, None) == -1
    some = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(some) + 15) & ~15  # (a 16-B aligned address inside the buffer; never dereferenced)

    def call(**kw):
        a = _abi.PpoSampleArgs()
        a.rtg = a.index_out = a.workspace = p
        a.rows, a.batch, a.workspace_bytes = 1000, 64, 1 << 40
        for k, v in kw.items():
            setattr(a, k, v)
        return L.lnw_ppo_sample(ctypes.byref(a), None)

    for kw in (dict(batch=1001), dict(batch=0), dict(rows=1 << 20, batch=131073), dict(rows=1 << 31),
               dict(rows=0), dict(rtg=None), dict(index_out=None), dict(workspace=None),
               dict(workspace_bytes=L.lnw_ppo_sample_workspace_bytes(1000, 64) - 1), dict(row_base=-1),
               dict(row_base=(1 << 40) - 999)):
        assert call(**kw) < 0, kw
    ws = L.lnw_ppo_sample_workspace_bytes
    assert ws(1000, 64) >= 8 * 1000 and ws(1000, 64) % 16 == 0
    assert ws(5242880, 131072) > 0 and ws((1 << 31) - 1, 1) > 0
    assert ws(1000, 1001) == 0 and ws(1 << 20, 131073) == 0 and ws(1 << 31, 64) == 0 and ws(0, 0) == 0 == ws(5, 0)
