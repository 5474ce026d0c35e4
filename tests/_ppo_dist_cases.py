"""Cases and the one-process driver shared by the sharded-training tests
(test_ppo_dist_cpu.py on the torch arm, test_gpu_ppo_dist.py on the kernels): a
synthetic rollout over all rows, cut into the played ranks' row ranges; every
played rank draws locally, and merges and packs for itself; the exchange
buffers are summed as int32, which is what the all-reduce does."""
import numpy as np
import torch

from _ppo_sample_cases import BIG_BASE
from lnw import ppodist

NEG_ZERO, NAN_A, NAN_B = -0x80000000, 0x7FC12345, -0x3FEDCB  # int32 bits: -0.0, a quiet NaN and a negative NaN, with payloads
SEED, SLOT = 0x5EED0FD157, 3

# name: ranges = every played rank's (first row, end row) of the whole, in rank
# order (ranks need not own ascending ranges), batch, (n, D), the global id of
# row 0, and what is planted in the whole rollout before the shards are cut
CASES = {
    # the merge of one list
    "one_rank": dict(ranges=[(0, 1200)], batch=64),
    # test_gpu_ppo_sample.test_shard_merge_on_device's split
    "two_unequal": dict(ranges=[(0, 2600), (2600, 6000)], batch=256),
    # a shard whose |rtg| is about 1e-4 against the others' 1: it owns no winner, all its slots are zero words
    "quiet_first": dict(ranges=[(0, 800), (800, 2000), (2000, 3000)], batch=64, quiet=0),
    "quiet_last": dict(ranges=[(0, 800), (800, 2000), (2000, 3000)], batch=64, quiet=2),
    # more lists than any other case: eight ranks, and the 64 the entry point allows (owning descending ranges)
    "eight_ranks": dict(ranges=[(400 * w, 400 * w + 400) for w in range(8)], batch=300),
    "most_ranks": dict(ranges=[(64 * (63 - w), 64 * (64 - w)) for w in range(64)], batch=64),
    # a batch of several workgroups of every kernel, above lnw_ppo_sample's in-LDS sort tile (2048)
    "batch_5000": dict(ranges=[(0, 5200), (5200, 13200), (13200, 19200)], batch=5000),
    "batch_1": dict(ranges=[(0, 400), (400, 1000)], batch=1),
    # not a multiple of the wave (64) or of the 4-word padding of the rtg / old_values regions
    "batch_70": dict(ranges=[(0, 400), (400, 1000), (1000, 1500)], batch=70),
    # the smallest shard's row count: every row of rank 1 is a candidate
    "batch_whole_shard": dict(ranges=[(96, 500), (0, 96), (500, 700)], batch=96),
    # more slots than finite rows: equal +inf keys in both lists, ordered by global row (rank 0 owns the higher rows)
    "nonfinite": dict(ranges=[(160, 280), (0, 160)], batch=100, nonfinite=True),
    # 64-bit rows (BIG_BASE is odd: one ship per group)
    "big_base": dict(ranges=[(0, 2600), (2600, 6000)], batch=256, nD=(1, 56), base=BIG_BASE),
    "n1_D56": dict(ranges=[(0, 300), (300, 700)], batch=48, nD=(1, 56)),
    "n2_D60": dict(ranges=[(0, 300), (300, 700)], batch=48, nD=(2, 60)),
    "n4_D68": dict(ranges=[(0, 300), (300, 700)], batch=48, nD=(4, 68)),
    "n12_D100": dict(ranges=[(0, 360), (360, 840)], batch=48, nD=(12, 100)),
    # -0.0 and NaNs with payloads in two winners' obs and actions: the integer sum keeps the bits
    "planted_bits": dict(ranges=[(0, 400), (400, 1000)], batch=32, planted=True),
    # two ships of one (env, step) both drawn: both slots read the same group in place
    "same_group": dict(ranges=[(0, 400), (400, 1000)], batch=32, same_group=(130, 0, 2)),
}


def rollout(rows, n, D, seed, device="cpu"):
    """A Rollout.run()-shaped result over `rows` rows (groups of n ships), as
    test_gpu_ppo_sample.synthetic_rollout makes it, flat."""
    g = torch.Generator().manual_seed(seed)
    G = rows // n
    assert G * n == rows
    obs = torch.rand((G, n, D), generator=g)
    obs[..., :49] = torch.randint(0, 256, (G, n, 49), generator=g) / 255.0
    return {k: v.to(device) for k, v in dict(
        obs=obs, rtg=1.0 + 2.0 * torch.randn(rows, generator=g), actions=torch.rand((rows, 4), generator=g),
        log_probs=-1.0 + 0.3 * torch.randn((rows, 4), generator=g), values=0.3 * torch.randn(G, generator=g)).items()}


def shard(whole, lo, hi, n):
    """Rows [lo, hi) of a flat rollout: slices, no copies."""
    return dict(obs=whole["obs"][lo // n:hi // n], rtg=whole["rtg"][lo:hi], actions=whole["actions"][lo:hi],
                log_probs=whole["log_probs"][lo:hi], values=whole["values"][lo // n:hi // n])


def build(case, device="cpu"):
    """(whole rollout, ranges, batch, n, D, base) of a case, with its plants
    except `planted` (which needs the draw: plant())."""
    n, D = case.get("nD", (4, 68))
    ranges = case["ranges"]
    rows = max(hi for _, hi in ranges)
    whole = rollout(rows, n, D, 17 + rows + n, device)
    if "quiet" in case:
        lo, hi = ranges[case["quiet"]]
        whole["rtg"][lo:hi] = torch.sign(whole["rtg"][lo:hi]) * 1e-4
    if case.get("nonfinite"):
        # rows [160, 280): 100 of 120 not finite; rows [0, 160): 120 of 160; 60 finite rows in all
        bad = torch.tensor([float("nan"), float("inf"), float("-inf")], device=device)
        hi_rows = torch.arange(160, 280, device=device)
        hi_rows = hi_rows[hi_rows % 6 != 0]
        lo_rows = torch.arange(0, 160, device=device)
        lo_rows = lo_rows[lo_rows % 4 != 1]
        for r in (hi_rows, lo_rows):
            whole["rtg"][r] = bad[r % 3]
    if "same_group" in case:
        grp, s0, s1 = case["same_group"]
        whole["rtg"][grp * n + s0] = 1e6
        whole["rtg"][grp * n + s1] = -1e6
    return whole, ranges, case["batch"], n, D, case.get("base", 0)


def plant(whole, rows, n):
    """-0.0 and NaNs with payloads in the obs of local row rows[0] and the
    actions of rows[1] (rows of the whole, winners of the draw); rtg is left
    alone, so the draw stays what it was. Returns the (tensor name, flat
    position, bits) planted."""
    D = whole["obs"].shape[-1]
    spots = [("obs", rows[0] * D + 50, NEG_ZERO), ("obs", rows[0] * D + 51, NAN_A), ("obs", rows[0] * D + 3, NAN_B),
             ("actions", rows[1] * 4 + 1, NEG_ZERO), ("actions", rows[1] * 4 + 2, NAN_A),
             ("actions", rows[1] * 4 + 3, NAN_B)]
    for name, pos, bits in spots:
        whole[name].view(torch.int32).reshape(-1)[pos] = bits
    return spots


def play(learner, whole, ranges, batch, n, base, impl):
    """One process plays len(ranges) ranks at draw slot SLOT (the counter is
    left there). Returns (per played rank the batch dict minibatch_dist would
    return, per played rank its own exchange buffer before the sum, the messages
    [W, 2 batch + 1], per played rank its sample_status)."""
    msgs, ros = [], []
    for lo, hi in ranges:
        sh = shard(whole, lo, hi, n)
        learner.draw.fill_(SLOT)
        b = learner.minibatch(sh, batch, seed=SEED, row_base=base + lo, advance=False)
        msgs.append(ppodist.message(b, base + lo, learner.sample_status))  # (a copy: the next draw reuses b's buffers)
        ros.append(learner.rollout_rows(sh))
    lists = torch.stack(msgs)
    merged = [ppodist.merge(lists, batch, n, impl) for _ in ranges]
    own = [ppodist.pack(ros[w], merged[w], w, base + lo, impl) for w, (lo, _) in enumerate(ranges)]
    total = torch.stack(own).sum(0, dtype=torch.int32)
    D = whole["obs"].shape[-1]
    return ([ppodist.unpack(total.clone(), m, n, D) for m in merged], own, lists,
            [int(m["status"]) for m in merged])


def bits(t):
    """A tensor's bit pattern as a NumPy integer array (NaN-safe comparisons)."""
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()


def expect_payload(whole, local_rows, n):
    """Plain indexing of the whole rollout at rows `local_rows` (int64 tensor,
    rows of the whole): what every played rank must end up holding."""
    grp = torch.div(local_rows, n, rounding_mode="floor")
    return dict(xobs=whole["obs"][grp], actions=whole["actions"][local_rows], old_log_probs=whole["log_probs"][local_rows],
                rtg=whole["rtg"][local_rows], old_values=whole["values"][grp])


def check_rank(got, whole, want_rows, want_key_bits, n, base):
    """One played rank's batch against the expected global rows and key bits
    (NumPy) and plain indexing of the whole rollout, bit for bit."""
    B = len(want_rows)
    assert got["global_row"].dtype == torch.int64 and got["index"].dtype == torch.int64
    assert got["key"].dtype == torch.float64 and got["obs"].dtype == torch.float32
    assert np.array_equal(got["global_row"].cpu().numpy(), want_rows)
    assert np.array_equal(bits(got["key"]), want_key_bits)
    assert np.array_equal(got["index"].cpu().numpy(), np.arange(B) * n + want_rows % n)
    local = torch.from_numpy(want_rows - base).to(whole["rtg"].device)
    want = expect_payload(whole, local, n)
    assert got["obs"].shape == want["xobs"].shape
    assert np.array_equal(bits(got["obs"]), bits(want["xobs"]))
    for k in ("actions", "old_log_probs", "rtg", "old_values"):
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), k
    # the learner's own view of the packed batch: row index[s] of obs.reshape(-1, D) is the drawn row
    D = whole["obs"].shape[-1]
    assert np.array_equal(bits(got["obs"].reshape(-1, D)[got["index"]]), bits(whole["obs"].reshape(-1, D)[local]))
