"""The observation window table's byte records on the CPU (csrc/lnw_window.h:
the record packer lnw_load_terrain runs and the byte -> float conversion the
row builders run), through the stand-alone host program
tools/window_bytes_check.c, which compiles that same header.

The conversion must give float32(float64(b) / 255.0) bit for bit for every
byte (the rows are compared bitwise with the oracle). The packer is compared
with the window rule restated here in numpy (combatant.py:165-181,
landingship.py:178-188): on a 12x12 grid, where every window leaves the grid,
and on a 104x104 grid, where cells with an index >= 100 read as 0 although the
grid holds them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "littoral-naval-warfare-marl_amd", "csrc")
SRC = os.path.join(ROOT, "tools", "window_bytes_check.c")
REC = 64
# class: (window side, cells behind the ship): Combatant, LandingShip, medium Combatant
CLASSES = ((7, 3), (5, 1), (5, 2))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    out = str(tmp_path_factory.mktemp("winbytes") / "window_bytes_check")
    subprocess.check_call([cc, "-O2", "-ffp-contract=off", f"-I{CSRC}", SRC, "-o", out, "-lm"])
    return out


def test_conversion_and_packer_self_check(prog):
    r = subprocess.run([prog], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "conversion mismatches 0 of 256" in r.stdout, r.stdout
    assert r.stdout.strip().endswith("mismatches 0"), r.stdout


def test_plain_product_is_not_enough():
    """Why the helper is not b * (1/255): that form misses for about half the
    bytes (so a test of the helper that passed with it would prove nothing)."""
    b = np.arange(256)
    want = (b.astype(np.float64) / 255.0).astype(np.float32)
    prod = b.astype(np.float32) * np.float32(1.0 / 255.0)
    assert (prod != want).sum() > 100
    assert np.array_equal(b.astype(np.float32) / np.float32(255.0), want)


def _rule(grid):
    """[3, G, G, 64] from the rule: entry (i, j) of the window of a ship at
    (x, y) is grid[x - back + i, y - back + j] inside 0..99 and the grid, else 0."""
    G = grid.shape[0]
    lim = min(G, 100)
    out = np.zeros((3, G, G, REC), np.uint8)
    xs, ys = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    for cls, (n, back) in enumerate(CLASSES):
        for i in range(n):
            for j in range(n):
                cx, cy = xs - back + i, ys - back + j
                ok = (cx >= 0) & (cy >= 0) & (cx < lim) & (cy < lim)
                out[cls, :, :, i * n + j] = np.where(ok, grid[np.clip(cx, 0, G - 1), np.clip(cy, 0, G - 1)], 0)
    return out


@pytest.mark.parametrize("G", [12, 104])
def test_packer_against_the_rule(prog, G, tmp_path):
    rng = np.random.default_rng(G)
    grid = rng.integers(1, 256, (G, G)).astype(np.uint8)  # no zero cell: an off-grid 0 is told apart
    gp, tp = str(tmp_path / "grid.bin"), str(tmp_path / "tab.bin")
    grid.tofile(gp)
    subprocess.check_call([prog, "pack", str(G), gp, tp])
    tab = np.fromfile(tp, np.uint8)
    assert tab.size == 3 * G * G * REC
    tab = tab.reshape(3, G, G, REC)
    want = _rule(grid)
    assert np.array_equal(tab, want), np.argwhere(tab != want)[:5].tolist()
    for cls, (n, back) in enumerate(CLASSES):
        assert not tab[cls, :, :, n * n:].any()  # zero padding
        # corner cells: the window's off-grid part is 0, the rest the grid's bytes
        c = tab[cls, 0, 0, :n * n].reshape(n, n)
        assert not c[:back].any() and not c[:, :back].any() and c[back:, back:].all()
        assert np.array_equal(c[back:, back:], grid[:n - back, :n - back])
        last = min(G, 100) - 1
        c = tab[cls, last, last, :n * n].reshape(n, n)
        assert c[:back + 1, :back + 1].all() and not c[back + 1:].any() and not c[:, back + 1:].any()
    if G > 100:  # cells 100.. exist in the grid and still read as 0
        assert grid[100:, 100:].all()
        c = tab[0, 101, 50, :49].reshape(7, 7)  # rows 98..104
        assert c[:2].all() and not c[2:].any()
        assert not tab[:, 103, 103].any()
