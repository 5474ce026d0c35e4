"""bench.sample_outputs (what `--dump-outputs` writes) on host tensors: every
env while the arrays fit bench.DUMP_BYTES, else a fixed seeded sample of the
envs in env order; float32, float64 kept."""
import numpy as np
import torch

import bench


def _outputs(E, rdt=torch.float32):
    gen = torch.Generator().manual_seed(1)
    return dict(obs_blue=torch.rand((E, 4, 68), generator=gen), obs_red=torch.rand((E, 4, 68), generator=gen),
                rew_blue=torch.rand((E, 4), generator=gen, dtype=rdt),
                rew_red=torch.rand((E, 4), generator=gen, dtype=rdt),
                done=torch.randint(0, 2, (E,), generator=gen, dtype=torch.int32),
                cog=torch.rand((E,), generator=gen, dtype=rdt))


def test_everything_while_it_fits():
    out = _outputs(37)
    got = bench.sample_outputs(out, 37)
    assert list(got) == list(bench.OUTPUT_NAMES)
    for k in got:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], out[k].numpy().astype(np.float32)), k


def test_seeded_sample_above_the_limit(monkeypatch):
    E, per_env = 301, (2 * 4 * 68 + 4 + 4 + 1 + 1) * 4
    monkeypatch.setattr(bench, "DUMP_BYTES", 100 * per_env + 7)
    out = _outputs(E)
    got, again = bench.sample_outputs(out, E), bench.sample_outputs(out, E)
    assert all(v.shape[0] == 100 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= bench.DUMP_BYTES
    assert all(np.array_equal(got[k], again[k]) for k in got)
    # the sampled envs, identified by their rows of obs_blue: distinct, in env order
    rows = out["obs_blue"].numpy().reshape(E, -1)
    idx = [int(np.flatnonzero((rows == r.reshape(-1)).all(1))[0]) for r in got["obs_blue"]]
    assert idx == sorted(set(idx)) and len(idx) == 100
    for k in got:
        assert np.array_equal(got[k], out[k].numpy()[idx].astype(np.float32)), k


def test_float64_rewards_stay_float64():
    got = bench.sample_outputs(_outputs(5, torch.float64), 5)
    assert got["rew_blue"].dtype == got["rew_red"].dtype == got["cog"].dtype == np.float64
    assert got["obs_blue"].dtype == got["done"].dtype == np.float32
