"""EW fixes whose cell depends on the order in which the fix points are summed.

A fix averages its m = n - 1 points with numpy.mean of a Python list: a plain
left-to-right sum below 8 points, from 8 on numpy's pairwise sum (the first 8
points as a tree, the rest in order). The two orders differ in the last bits
of the mean, which the step's outputs show only where the mean sits on a
rounding tie. Random episodes never come that close (a step's outputs hold the
fix only as a rounded cell), so these layouts are built to: n small blue ships
around one large red ship, radars off, no fire and no movement (all-zero
actions), ducting 1.9 and the n bearings' distortions given by the parity tape.
The last distortion was bisected to where the mean x of the pairwise sum
crosses red_x + 1.5, and a neighbouring double taken at which the pairwise and
the left-to-right mean round to different cells: one within two cells of the red
ship (the fix becomes a target: want = 1 is the pairwise, i.e. numpy's,
outcome), the other not. Every slope's tangent argument was checked to give the
same bits in the library's own tan (csrc/lnw_device.h tan_fd, compiled for the
host) and in the host libm, so the only freedom left is the order of the sum.
Each of a step's n blue turns takes the same n bearings (nobody moves), so the
tape holds the ducting draw and n times the n distortions.
"""
import math

import numpy as np

import _oracle
from _spawns import grid as _grid

DUCT_DRAW = 0.9  # np.random.beta's tape value: ducting 1.9, EW range small on large 30 cells

CASES = {
    "9v1": dict(red=(59, 46), want=0,
            blue=[(44, 47), (43, 54), (46, 57), (43, 45), (40, 46), (51, 47), (41, 46), (53, 57),
                  (47, 57)],
            d=["-0x1.fbbb98e670cbap+0", "-0x1.b7595470eb064p-2", "-0x1.44aca8a11258fp-2", "-0x1.62597f7ee4e51p-1",
               "0x1.f4cdfb657ba1ap-2", "0x1.15618a5cdd839p-2", "-0x1.cd5830ae44b70p-1", "-0x1.a17d7e95c7f55p-4",
               "-0x1.137aeb590d1afp-1"]),
    "10v1": dict(red=(57, 50), want=1,
            blue=[(43, 53), (43, 56), (51, 60), (44, 48), (44, 45), (47, 53), (39, 51), (43, 54),
                  (39, 48), (47, 49)],
            d=["-0x1.7c8605f39b651p-1", "-0x1.da0e5f1890a5bp-3", "-0x1.d5f641f2507fep-9", "0x1.de048603f440cp-1",
               "-0x1.d9d97698e0edbp-2", "0x1.08b49f5158a77p-2", "-0x1.e2ed53d73683fp-6", "0x1.91b5a4a1cfcd5p-1",
               "-0x1.742db78b1c89ep-2", "-0x1.c2606d4dd334fp-3"]),
    "13v1": dict(red=(51, 60), want=1,
            blue=[(36, 59), (46, 54), (58, 44), (37, 47), (49, 52), (41, 58), (39, 56), (59, 50),
                  (43, 57), (45, 51), (57, 60), (36, 57), (56, 61)],
            d=["-0x1.fc4f6d60cb462p-1", "0x1.0367f3d2f9486p-1", "-0x1.1ce8dd9488099p+0", "-0x1.deadf737fc3a6p-1",
               "-0x1.f3cf5d1dcb8f2p-2", "0x1.2962144c792b9p-2", "0x1.e0ff2efd482c6p-2", "-0x1.2163d34848c00p-2",
               "-0x1.8f6218eb58a1fp-7", "0x1.e91016d6bc379p+0", "0x1.b9ee18b92cf89p-1", "-0x1.fa3b983f69ae7p-2",
               "-0x1.369af68b9c23fp+0"]),
    "16v1": dict(red=(59, 61), want=0,
            blue=[(43, 55), (54, 44), (59, 55), (54, 50), (49, 44), (49, 60), (47, 50), (44, 57),
                  (45, 58), (50, 45), (55, 55), (43, 51), (54, 59), (59, 44), (46, 59), (48, 60)],
            d=["-0x1.5b4d4d3504254p+0", "0x1.c248dc1fc9952p+0", "0x1.c08af3df4ad8fp+0", "0x1.05675bcbc47b6p+1",
               "-0x1.1252c02947867p-1", "0x1.d754dbf2f3479p+0", "0x1.2d6ce5b3ec5bdp+0", "0x1.13c96cbf97ff3p-4",
               "0x1.376047b188ebfp-1", "-0x1.0c183427aa5ccp-1", "-0x1.78f5dc6007342p+0", "0x1.3a679b53f4657p+0",
               "-0x1.40ba520c7f8f3p+0", "0x1.9ed4ce9ae496ap-3", "-0x1.a8d5ae46c78fcp+0", "0x1.547ccc93c67e4p-1"]),
}


def tape(c):
    n = len(c["blue"])
    return np.array([DUCT_DRAW] + [float.fromhex(v) for v in c["d"]] * n)


def positions(c):
    return np.array(list(c["blue"]) + [c["red"]], np.int32)


def _points(c):
    """The fix points of one blue turn (combatant.py:249-277), in Python floats."""
    red, ms = c["red"], []
    for (x, y), h in zip(c["blue"], c["d"]):
        b, d = math.degrees(math.atan2(red[1] - y, red[0] - x)), float.fromhex(h)
        b = b + d + 360.0 if b + d < 0 else b + d
        ms.append(math.tan(math.radians(b)))
    px, py = [], []
    for q in range(len(ms) - 1):
        (x1, y1), (x2, y2), m1, m2 = c["blue"][q], c["blue"][q + 1], ms[q], ms[q + 1]
        x3 = (m1 * x1 - m2 * x2 + y2 - y1) / (m1 - m2)
        px.append(x3)
        py.append(m1 * (x3 - x1) + y1)
    return px, py


def plain_mean(v):
    s = 0.0
    for x in v:
        s += x
    return s / len(v)


def targets(c, mean):
    """1 if the fix, averaged by `mean`, rounds to a cell within two of the red ship."""
    px, py = _points(c)
    rx, ry = round(mean(px)), round(mean(py))  # round(): half to even, as rint
    return int((rx - c["red"][0]) ** 2 + (ry - c["red"][1]) ** 2 < 4)


def oracle_step(c):
    """One step of the layout on the oracle: its step() record and the OracleEnv."""
    n = len(c["blue"])
    o = _oracle.OracleEnv(_grid(100), n, 1, landing_ops=False)
    o.set_tape(tape(c))
    o.reset([_oracle.T_SMALL] * n + [_oracle.T_LARGE], positions(c))
    r = o.step(np.zeros((n + 1, 4), np.float32), np.full(n + 1, _oracle.K_F32, np.int32))
    return r, o
