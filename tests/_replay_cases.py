"""Shared inputs of the DDQN replay tests (test_replay_cpu.py,
test_gpu_replay.py): synthetic rings filled step by step from a seeded NumPy
generator, with -0.0, a NaN with a payload and a denormal planted in every
transition's state / next_state and odd float64 rewards; the expected minibatch
by plain indexing; one process playing the ranks of a sharded draw; and
comparisons as bits.

TEST INFRASTRUCTURE: the shapes are the smallest at which each piece can still
go wrong (the table in DESIGN.md "DDQN replay")."""
import numpy as np
import torch

from lnw import ppodist, replay
from lnw.ppolearn import sample_keys

SEED, SLOT = 5, 3
NAN_PAYLOAD, DENORMAL, NEG_ZERO = 0x7FC12345, 0x00000001, -0x80000000
FILL = -1515870811  # 0xA5A5A5A5 as int32: an unwritten word of xbuf shows up

# shards: envs per played rank (one entry: a single collector); steps: collector steps taken
CASES = {
    "all": dict(shards=(3,), cap=5, n=1, D=52, steps=5, B=15, f64=False),
    "part": dict(shards=(5,), cap=4, n=3, D=100, steps=2, B=7, f64=True),
    "wrap": dict(shards=(4,), cap=4, n=2, D=60, steps=7, B=5, f64=False),
    "wide": dict(shards=(2,), cap=3, n=16, D=52, steps=3, B=1, f64=False),
    "ranks": dict(shards=(3, 1, 3), cap=4, n=2, D=60, steps=4, B=4, f64=True),
    "quiet": dict(shards=(2, 2, 2), cap=4, n=2, D=52, steps=4, B=6, f64=False, quiet=1),
}
ODD_REWARDS = (-0.0, 1.0 / 3.0, 1e-310, -2.5000000001, 16777217.0, 1e-40)


def bits(t):
    """A tensor's bytes as int32 words where it has them, else uint8."""
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.int32) if a.dtype.itemsize % 4 == 0 else a.view(np.uint8)


def same(a, b):
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and np.array_equal(bits(a), bits(b))


def history(E, n, D, steps, f64, seed):
    """`steps` collector steps of transitions, [steps, E, ...] host tensors."""
    rng = np.random.default_rng(seed)
    st = rng.standard_normal((2, steps, E, n, D)).astype(np.float32)
    w = st.view(np.int32)
    w[:, :, :, 0, 0] = NEG_ZERO
    w[0, :, :, n - 1, D - 1] = NAN_PAYLOAD
    w[1, :, :, 0, 1] = DENORMAL
    w[1, :, :, n - 1, D - 2] = NAN_PAYLOAD + 1
    rew = rng.standard_normal((steps, E, n)) * 3.0
    if f64:
        flat = rew.reshape(-1)
        flat[::7] = np.resize(np.array(ODD_REWARDS), flat[::7].shape[0])
    else:
        rew = rew.astype(np.float32)
    return dict(state=torch.from_numpy(st[0]), next_state=torch.from_numpy(st[1]),
                action=torch.from_numpy(rng.integers(0, 50, (steps, E, n, 4)).astype(np.int32)),
                reward=torch.from_numpy(rew), done=torch.from_numpy(rng.integers(0, 2, (steps, E)).astype(np.int32)))


def empty_ring(cap, E, n, D, f64, device):
    """A ring as QCollector allocates it."""
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device=device)  # noqa: E731
    return dict(state=z(cap, E, n, D), next_state=z(cap, E, n, D), action=z(cap, E, n, 4, dtype=torch.int32),
                reward=z(cap, E, n, dtype=torch.float64 if f64 else torch.float32),
                done=torch.ones((cap, E), dtype=torch.int32, device=device))


def fill(hist, cap, mode, device="cpu", impl="torch"):
    """The ring and priorities after the history's steps, written slot by slot
    and marked after every step, as QCollector.step does."""
    steps, E, n, D = hist["state"].shape
    ring = empty_ring(cap, E, n, D, hist["reward"].dtype == torch.float64, device)
    pr = replay.new_priority(E, cap, device)
    for t in range(steps):
        for k, v in hist.items():
            ring[k][t % cap].copy_(v[t])
        replay.mark(pr, ring["reward"], t % cap, mode, impl)
    return ring, pr


def priority_restated(ring, filled):
    """The "reward" priorities from the definition, with NumPy float32 scalars."""
    cap, E, n = ring["reward"].shape
    rew = ring["reward"].detach().cpu().numpy()
    p = np.full((E, cap), np.nan, np.float32)
    for e in range(E):
        for k in range(filled):
            acc = np.float32(0.0)
            for i in range(n):
                acc = np.float32(acc + np.abs(np.float32(rew[k, e, i])))
            p[e, k] = acc
    return p


def build(case, device="cpu", impl="torch", mode="reward"):
    """(ring, priority, filled, ranges of envs per played rank) of a case."""
    c = CASES[case] if isinstance(case, str) else case
    E = sum(c["shards"])
    hist = history(E, c["n"], c["D"], c["steps"], c["f64"], 100 + c["D"] + E)
    ring, pr = fill(hist, c["cap"], mode, device, impl)
    ranges, lo = [], 0
    for s in c["shards"]:
        ranges.append((lo, lo + s))
        lo += s
    if "quiet" in c:  # (the priorities are public: a caller may rewrite them)
        a, b = ranges[c["quiet"]]
        pr[a:b] = 1e-30
    return ring, pr, min(c["steps"], c["cap"]), ranges


def shard(ring, pr, lo, hi):
    """Envs [lo, hi) as a collector over them holds them."""
    return {k: v[:, lo:hi].contiguous() for k, v in ring.items()}, pr[lo:hi].contiguous()


def direct_rows(pr, B, seed, slot, row_base=0):
    """The draw from its definition: (local rows [B], keys [B]) by sample_keys
    and a lexsort over (key, row)."""
    key = sample_keys(pr.detach().cpu().numpy().reshape(-1), seed, slot, row_base)
    order = np.lexsort((np.arange(key.shape[0]), key))[:B]
    return order.astype(np.int64), key[order]


def expected(ring, rows):
    """Plain indexing of the ring at local rows e * cap + k: the learner's row tensors."""
    cap, E, n, D = ring["state"].shape
    r = torch.as_tensor(rows, device=ring["state"].device)
    e, k = torch.div(r, cap, rounding_mode="floor"), r % cap
    B = r.shape[0]
    return dict(state=ring["state"][k, e].reshape(B * n, D), next_state=ring["next_state"][k, e].reshape(B * n, D),
                action=ring["action"][k, e].reshape(B * n, 4), reward=ring["reward"][k, e].reshape(B * n),
                done=ring["done"][k, e][:, None].expand(B, n).reshape(B * n).contiguous(), index=k * E + e)


def check_rows(got, ring, rows, keys, row_base=0):
    """A minibatch dict against plain indexing at the whole ring's local rows."""
    want = expected(ring, rows)
    for k in replay.ROW_KEYS:
        assert same(got[k], want[k]), k
    assert np.array_equal(got["global_row"].cpu().numpy(), np.asarray(rows) + row_base)
    assert np.array_equal(bits(got["key"]), np.asarray(keys).view(np.int32))
    if "index" in got:
        assert np.array_equal(got["index"].cpu().numpy(), want["index"].cpu().numpy())


def counters(device, slot=SLOT):
    return (torch.full((1,), slot, dtype=torch.int64, device=device),
            torch.full((1,), -7, dtype=torch.int64, device=device))


def play(ring, pr, filled, ranges, B, impl, seed=SEED, slot=SLOT, edit=None):
    """One process plays the ranks of minibatch_dist: the local draws, the
    messages, the merge, every rank's pack into a buffer pre-filled with FILL,
    the integer sum, the unpack. edit(merged): changes the merge in place before
    the packs. Returns (per-rank results, per-rank buffers, lists, merged)."""
    cap, E, n, D, f64 = replay.ring_shape(ring)
    dev = pr.device
    parts, msgs = [], []
    for lo, hi in ranges:
        r, p = shard(ring, pr, lo, hi)
        assert B <= filled * (hi - lo)
        ctr, status = counters(dev, slot)
        local = replay.draw(p, B, seed, ctr, status, lo * cap, False, impl)
        assert int(ctr) == slot
        parts.append(r)
        msgs.append(ppodist.message(local, lo * cap, status))
    lists = torch.stack(msgs)
    merged = ppodist.merge(lists, B, 1, impl)
    if edit is not None:
        edit(merged)
    own = []
    for w, (lo, hi) in enumerate(ranges):
        xbuf = torch.full((replay.pack_words(B, n, D, f64),), FILL, dtype=torch.int32, device=dev)
        own.append(replay.pack(parts[w], merged["global_row"], merged["src_rank"], w, lo * cap, impl, xbuf))
    total = torch.stack(own).sum(0, dtype=torch.int32)
    got = replay.unpack(total, B, n, D, f64)
    got.update(key=merged["key"], global_row=merged["global_row"])
    return got, own, lists, merged
