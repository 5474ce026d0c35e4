"""Inputs the tests share: the terrain grids, the reference spawns and the
spawn generators. Host only: numpy and _oracle. TEST INFRASTRUCTURE; every
generator is pinned by digest in tests/test_helpers_cpu.py."""
import functools

import numpy as np

import _oracle

# the reference's spawn cells, 4 blue then 4 red
REF_SPAWNS = [(6, 61), (10, 81), (8, 70), (11, 58), (98, 48), (98, 52), (98, 56), (96, 52)]
# split spawns on the 100 grid, sides 10-40 cells apart: fire, EW bearings and fixes from the first steps
MELEE_BOXES = ((30, 45, 40, 60), (55, 70, 45, 65))  # (x0, x1, y0, y1) of blue, of red


def ref_spawns(nb):
    """The first nb reference spawns of either side."""
    return REF_SPAWNS[:nb] + REF_SPAWNS[4:4 + nb]


@functools.lru_cache(maxsize=None)
def grids():
    """(grid100, grid200) of tests/golden/grids.npz, read-only."""
    g = _oracle.load_fixture("grids.npz")
    out = g["grid100"], g["grid200"]
    for a in out:
        a.setflags(write=False)
    return out


def grid(G=100):
    return grids()[{100: 0, 200: 1}[G]]


def box_positions(grid, E, nb, nr, seed, box_b=MELEE_BOXES[0], box_r=MELEE_BOXES[1]):
    """[E, nb + nr, 2]: per env, every ship on a water cell of its side's box
    (drawn env by env, blue before red)."""
    rng = np.random.default_rng(seed)
    water = lambda x0, x1, y0, y1: [(x, y) for x in range(x0, x1) for y in range(y0, y1)  # noqa: E731
                                    if grid[x, y] <= 74]
    wb, wr = water(*box_b), water(*box_r)
    return np.array([[wb[i] for i in rng.integers(0, len(wb), nb)] +
                     [wr[i] for i in rng.integers(0, len(wr), nr)] for _ in range(E)], np.int32)


def melee_block(grid, n, seed, nb=4, nr=4):
    """[n, nb + nr, 2]: a block of n envs in MELEE_BOXES (drawn side by side:
    all blue cells, then all red)."""
    rng = np.random.default_rng(seed)
    (bx0, bx1, by0, by1), (rx0, rx1, ry0, ry1) = MELEE_BOXES
    wb = np.argwhere(grid[bx0:bx1, by0:by1] <= 74) + np.array([bx0, by0])
    wr = np.argwhere(grid[rx0:rx1, ry0:ry1] <= 74) + np.array([rx0, ry0])
    return np.concatenate([wb[rng.integers(0, len(wb), (n, nb))], wr[rng.integers(0, len(wr), (n, nr))]],
                          1).astype(np.int32)


def water_positions(grid, E, boxes, seed):
    """Per env, per agent a water cell drawn uniformly from that agent's box."""
    rng = np.random.default_rng(seed)
    out = np.zeros((E, len(boxes), 2), np.int32)
    for a, (x0, x1, y0, y1) in enumerate(boxes):
        cells = np.argwhere(grid[x0:x1, y0:y1] <= 74) + np.array([x0, y0])
        out[:, a] = cells[rng.integers(0, len(cells), E)]
    return out


def hash_mult(n, seed=99):
    """Odd multipliers of the observation hash sum_k bits(obs[k]) * mult[k] mod 2^64."""
    return (np.random.default_rng(seed).integers(0, 1 << 30, n, dtype=np.int64) * 2 + 1)
