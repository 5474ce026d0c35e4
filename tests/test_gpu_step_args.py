"""What a step launch is told — per call (action dtype, observation outputs)
and through the setters (work counters, analytics, kernel variant, RNG seed,
a masked reset's spawn spec) — reaches the kernel as it stands at that call:
on one handle whose settings change between steps, with the setters called
while steps are still queued, with two handles interleaved on one stream, and
after a snapshot is restored into a handle that was configured differently.

Every comparison is against a fresh handle that had the settings from its
creation and was brought to the same point with get_state / set_state:
observations, done, the written-back actions and the whole state bit for bit,
rewards and cog to 1e-5 (the suite's bound). Every case runs 45 steps or fewer.
Needs an MI355X."""
import numpy as np
import pytest
import torch

from _spawns import grid as _grid

pytestmark = pytest.mark.gpu

# reference-like spawns (the fleets out of each other's reach: quiet steps) ...
FAR = [(6, 61), (10, 81), (8, 70), (11, 58), (98, 48), (98, 52), (98, 56), (96, 52)]
# ... and the spec the masked reset brings in (other cells, still apart)
FAR2 = [(7, 62), (11, 80), (9, 71), (12, 59), (97, 49), (97, 53), (97, 57), (95, 53)]
BOX_B, BOX_R = (30, 45, 40, 60), (55, 70, 45, 65)  # contact spawns (fire, EW fixes, sinkings)

# (E, environments per workgroup: 0 = automatic)
SHAPES = {"units_256": (256, 64), "direct_64": (64, 16), "partial_40": (40, 0)}


def _positions(grid, E, seed=3):
    """The first half of the envs (whole 64-env units at E = 256) on the far
    spawns, the second half in contact: quiet and loud workgroups in one launch."""
    rng = np.random.default_rng(seed)
    water = lambda x0, x1, y0, y1: [(x, y) for x in range(x0, x1) for y in range(y0, y1)  # noqa: E731
                                    if grid[x, y] <= 74]
    wb, wr = water(*BOX_B), water(*BOX_R)
    pos = np.empty((E, 8, 2), np.int32)
    for e in range(E):
        if e < E // 2:
            pos[e] = FAR
        else:
            pos[e] = ([wb[i] for i in rng.integers(0, len(wb), 4)] +
                      [wr[i] for i in rng.integers(0, len(wr), 4)])
    return pos


def _fresh(E, epw, grid, cfg, trained_red=True, episode_steps=40):
    """A handle with every setting of cfg in force from creation."""
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    sc = Scenario(landing_ops=False, auto_reset=True, episode_steps=episode_steps, trained_red=trained_red)
    g = BatchedGame(E, ["small"] * 4, ["large"] * 4, scenario=sc, grid=grid, seed=cfg["seed"])
    if epw:
        assert g.set_epw(epw) == epw
    g.set_variant(cfg["contact"])
    if cfg["count"]:
        g.count_work(True)
    if cfg["ana"]:
        g.enable_analytics(eng_cap=1 << 12, ew_cap=1 << 12)
    return g


def _steps(g, acts, obs=True):
    """Step through acts; every step's outputs and written-back actions, kept on
    the device (no host synchronisation)."""
    out = []
    for a in acts:
        a = a.clone()
        o = g.step(a, obs=obs)
        rec = {k: v.clone() for k, v in o.items() if obs or not k.startswith("obs_")}
        rec["actions"] = a
        out.append(rec)
    return out


def _state(g):
    """Every state field's bytes (lnw_state_field). Not the get_state() blob: that
    also carries the per-env spawn cells of an earlier reset after a later
    reset has turned them off, which a fresh handle never had."""
    from lnw import _abi
    return [g.get(f).contiguous().view(torch.uint8).cpu() for f in range(_abi.LNW_NFIELDS)]


def _same_state(s1, s2, what):
    for f, (a, b) in enumerate(zip(s1, s2)):
        assert torch.equal(a, b), (what, "state field", f)


def _same(t1, t2, what):
    assert len(t1) == len(t2)
    for s, (x, y) in enumerate(zip(t1, t2)):
        assert x.keys() == y.keys()
        for k in x:
            a, b = x[k].cpu().numpy(), y[k].cpu().numpy()
            if k.startswith("rew_") or k == "cog":
                # (cog is nan once a fleet is gone: the same envs in both, the rest to 1e-5)
                assert np.array_equal(np.isnan(a), np.isnan(b)), (what, s, k)
                ok = ~np.isnan(a)
                d = float(np.max(np.abs(a[ok].astype(np.float64) - b[ok].astype(np.float64)))) if ok.any() else 0.0
                assert d <= 1e-5, (what, s, k, d)
            else:
                assert np.array_equal(a, b, equal_nan=True), (what, s, k)


def _side_channels(g, cfg):
    """Totals of the side channels the settings bound (record order is the
    atomics' order, so totals only)."""
    r = {}
    if cfg["count"]:
        r.update(g.work_counts())
    if cfg["ana"]:
        an = g.analytics()
        r.update(eng=an["engagements_total"], ew=an["ew_total"], heat=int(an["heatmap"].sum().item()),
                 launch=int(an["launch"].sum().item()))
    return r


def _segments(E, dev):
    """(name, settings change, actions, observation rows): 40 steps, so the envs
    the masked reset left alone end on their 40-step auto-reset."""
    rng = np.random.default_rng(11)

    def acts(n, dt):
        return [torch.from_numpy(rng.random((E, 8, 4))).to(dt).to(dev) for _ in range(n)]

    return [
        ("start", {}, acts(6, torch.float32), True),
        ("count_work on, float64 rows", {"count": True}, acts(6, torch.float64), True),
        # (count_work again: fresh counters, so this segment's totals stand alone)
        ("analytics on, no rows", {"ana": True, "count": True}, acts(5, torch.float32), False),
        ("contact variant, side channels off", {"contact": True, "count": False, "ana": False},
         acts(5, torch.float32), True),
        ("re-seeded, first variant", {"seed": 99, "contact": False}, acts(5, torch.float64), True),
        ("masked reset, new spawn spec", {"reset": True}, acts(13, torch.float32), True),
    ]


def _apply(g, cfg, change, E):
    """The setters a segment's change calls on a live handle; returns the new cfg."""
    cfg = dict(cfg)
    for k, v in change.items():
        if k == "count":
            g.count_work(v)
        elif k == "ana":
            g.enable_analytics(eng_cap=1 << 12, ew_cap=1 << 12) if v else g.disable_analytics()
        elif k == "contact":
            g.set_variant(v)
        elif k == "seed":
            g.set_rng(v)
        elif k == "reset":
            mask = np.zeros(E, np.uint8)
            mask[::3] = 1
            g.reset(positions=FAR2, env_mask=mask)
            continue
        cfg[k] = v
    return cfg


CFG0 = dict(seed=5, contact=False, count=False, ana=False)


def _run_sequence(name, sync):
    """The whole sequence on one handle. sync: wait for the device before every
    settings change. Returns per-segment (cfg, snapshot before, outputs,
    side-channel totals, state after) and the final state."""
    from lnw import _abi
    E, epw = SHAPES[name]
    grid = _grid()
    g = _fresh(E, epw, grid, CFG0)
    pos = _positions(grid, E)
    g.reset(positions=pos[0], pos_per_env=torch.from_numpy(pos))
    cfg, segs = dict(CFG0), []
    for what, change, acts, obs in _segments(E, g.device):
        if sync:
            torch.cuda.synchronize()
        cfg = _apply(g, cfg, change, E)
        snap = g.get_state(device="cuda") if sync else None
        out = _steps(g, acts, obs)
        if name == "units_256" and not cfg["contact"]:
            assert g.step_kernel() == _abi.KERNEL_UNITS, what
        # (read before the next change rebinds or unbinds them)
        segs.append((what, cfg, snap, acts, obs, out, _side_channels(g, cfg) if sync else None,
                     _state(g) if sync else None))
    end = _state(g)
    env = g.env_state()
    ag = g.agents()
    g.close()
    return segs, end, env, ag


@pytest.fixture(scope="module")
def synced():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run_sequence(name, sync=True)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_settings_changed_on_one_handle(name, synced):
    """(a) every segment equals a fresh handle that had its settings from creation."""
    E, epw = SHAPES[name]
    grid = _grid()
    segs, end, env, ag = synced(name)
    for what, cfg, snap, acts, obs, out, side, after in segs:
        f = _fresh(E, epw, grid, cfg)
        f.set_state(snap)
        ref = _steps(f, acts, obs)
        _same(out, ref, what)
        assert _side_channels(f, cfg) == side, what
        _same_state(_state(f), after, what)
        f.close()
    _same_state(segs[-1][-1], end, "end")
    # the 40th step was the auto-reset of the envs the masked reset left alone
    # (those that had not finished earlier), and they respawned on the new
    # spec's cells, not on the per-env cells of the first reset
    assert int(env["episode"].sum()) > 0
    fresh_now = (env["steps_done"] == 0) & (np.arange(E) % 3 != 0)
    assert fresh_now.any()
    n = int(fresh_now.sum())
    assert np.array_equal(ag["x"][fresh_now], np.tile([p[0] for p in FAR2], (n, 1)))
    assert np.array_equal(ag["y"][fresh_now], np.tile([p[1] for p in FAR2], (n, 1)))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_setters_with_steps_queued(name, synced):
    """(b) the same setters called while earlier steps are still queued."""
    segs, end, _, _ = synced(name)
    qsegs, qend, _, _ = _run_sequence(name, sync=False)
    for (what, _, _, _, _, out, _, _), (_, _, _, _, _, qout, _, _) in zip(segs, qsegs):
        _same(qout, out, what)
    _same_state(qend, end, "queued")


def test_two_handles_interleaved():
    """(c) two handles of different scenarios stepped alternately on one stream."""
    E, epw, grid = 64, 16, _grid()
    pos = _positions(grid, E)
    rng = np.random.default_rng(21)
    acts = [[torch.from_numpy(rng.random((E, 8, 4)).astype(np.float32)).cuda() for _ in range(20)]
            for _ in range(2)]
    kinds = [dict(cfg=dict(CFG0, seed=5), trained_red=True), dict(cfg=dict(CFG0, seed=6), trained_red=False)]

    def make(k):
        g = _fresh(E, epw, grid, k["cfg"], trained_red=k["trained_red"], episode_steps=12)
        g.reset(positions=pos[0], pos_per_env=torch.from_numpy(pos))
        return g

    solo = []
    for k, a in zip(kinds, acts):
        g = make(k)
        solo.append((_steps(g, a), _state(g)))
        g.close()
    gs = [make(k) for k in kinds]
    both = [[], []]
    for s in range(20):
        for i, g in enumerate(gs):
            both[i] += _steps(g, acts[i][s:s + 1])
    for i, g in enumerate(gs):
        _same(both[i], solo[i][0], f"handle {i}")
        _same_state(_state(g), solo[i][1], f"handle {i}")
        g.close()


def test_snapshot_into_differently_configured_handle():
    """(d) a snapshot restored into a handle created under another seed and
    reset on another spawn spec continues as the saved handle, through the
    auto-reset."""
    E, epw, grid = 64, 16, _grid()
    pos = _positions(grid, E)
    rng = np.random.default_rng(31)
    acts = [torch.from_numpy(rng.random((E, 8, 4)).astype(np.float32)).cuda() for _ in range(30)]
    g = _fresh(E, epw, grid, dict(CFG0, seed=5), episode_steps=12)
    g.reset(positions=pos[0], pos_per_env=torch.from_numpy(pos))
    _steps(g, acts[:8])
    snap = g.get_state()
    ref = _steps(g, acts[8:])
    end = _state(g)
    assert int(g.env_state()["episode"].sum()) > 0
    other = _fresh(E, epw, grid, dict(CFG0, seed=777), episode_steps=12)
    other.reset(positions=FAR2)      # another spec, common cells for every env
    _steps(other, acts[:3])
    other.set_state(snap)
    _same(_steps(other, acts[8:]), ref, "restored")
    _same_state(_state(other), end, "restored")
    g.close()
    other.close()
