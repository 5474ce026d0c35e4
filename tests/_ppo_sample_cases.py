"""Shapes and inputs shared by the minibatch-draw tests (test_ppo_sample_cpu.py,
test_gpu_ppo_sample.py)."""
import numpy as np
import torch

# (rows, batch). The base list, then one below, at and one above every
# internal boundary of csrc/lnw_pposample.hip:
#   rows per workgroup: a chunk is 256 rows up to 2048 workgroups (524 288 rows),
#     then grows by 256: 255 / 256 / 257 rows (one or two workgroups) and
#     524 287 / 524 288 / 524 289 (chunk 256 -> 512);
#   the sort's padding to a power of two: batch 63 / 64 / 65;
#   the sort's LDS tile of 2048 candidates (first stride through global
#     memory): batch 2047 / 2048 / 2049;
#   the largest batch, 131 072 (six strides above the tile), and one below.
# A chunk whose smallest key lies above the threshold is skipped after the first
# pass: every case with more rows than 256 x batch has such chunks, and (64, 64),
# (5, 5), (256, 64) have none.
# There is one algorithm for every batch, so no switch point.
BASE_CASES = [(1, 1), (5, 5), (64, 64), (65, 1), (257, 64), (4099, 64), (20000, 1000), (70001, 4096)]
BOUNDARY_CASES = [(255, 63), (256, 64), (257, 65), (524287, 64), (524288, 64), (524289, 64),
                  (5000, 2047), (5000, 2048), (5000, 2049), (140001, 131071), (140000, 131072)]
PATTERNS = ("normal0", "normal1", "normal2", "zero", "equal", "duplicates", "extreme")
BIG_BASE = 2 ** 33 + 5


def rtg_pattern(name, N):
    rng = np.random.default_rng(sum(map(ord, name)) + N)
    if name.startswith("normal"):
        return rng.standard_normal(N).astype(np.float32)
    if name == "zero":
        return np.zeros(N, np.float32)
    if name == "equal":
        return np.full(N, 0.7, np.float32)
    if name == "duplicates":
        return (rng.integers(-2, 3, N) / 2).astype(np.float32)
    r = rng.standard_normal(N).astype(np.float32)  # extreme: +-1e30 and denormals among normal rows
    r[::5] = 1e30
    r[1::7] = -1e30
    r[2::3] = 1e-42
    r[3::11] = -3e-45
    return r


def make_out(rtg, n, device="cpu", seed=0):
    """A Rollout.run()-shaped dict around a reward-to-go vector: N = len(rtg)
    rows of n ships per group (obs has one float per row: minibatch() never
    reads it)."""
    N = len(rtg)
    assert N % n == 0
    g = torch.Generator().manual_seed(seed)
    return {k: v.to(device) for k, v in dict(
        obs=torch.zeros((N // n, n, 1)), rtg=torch.as_tensor(np.asarray(rtg, np.float32)),
        actions=torch.rand((N, 4), generator=g), log_probs=torch.randn((N, 4), generator=g),
        values=torch.randn(N // n, generator=g)).items()}


def ships(N):
    return 4 if N % 4 == 0 else 1
