"""The MAPPO learner step's torch arm (lnw.ppolearn.PPOLearner, impl="torch") on
the host against what the reference's own PPO.learn left behind
(tests/golden/ppolearn*.npz, make_ppolearn_golden.py), and the batch helpers
rows() and sample().

Gradients: err(T) = max |T - T64| / max |T64| against the float64 oracle, and
err(T) <= 8 x max(err_ref(T), 2^-23) with err_ref the same measure of the
reference's recorded gradient (_qlearn_util's measure and bound). conv1.bias
and conv2.bias have a mathematically zero gradient under per-row statistics:
they are compared on the gradient only, relative to the conv's weight-gradient
scale, and left out of the post-step comparison."""
import numpy as np
import pytest
import torch

from _ppolearn_util import (ACTOR_GRAD_NAMES, CRITIC_GRAD_NAMES, NOISE, SETS, TOL_ADV, TOL_LP, TOL_V,
                            assert_grads_within, branch_report, err, gather, gold, hyper, load_set, oracle64, ref_flat,
                            segs)
from lnw.ppolearn import RUNNING, PPOLearner


def make(prefix, **kw):
    actor, critic, batch = load_set(prefix)
    return PPOLearner(actor, critic, impl="torch", device="cpu", **hyper(prefix), **kw), batch


@pytest.mark.parametrize("prefix", SETS)
def test_fixture_conditions(prefix):
    """What the generator asserted of the recorded sets still holds of the
    files: branch counts, margins, pool ties."""
    g = gold()
    L, batch = make(prefix)
    o = dict(new_log_probs=torch.from_numpy(g[f"{prefix}_new_log_probs"]).double(),
             advantage=torch.from_numpy(g[f"{prefix}_advantage"]).double(),
             values=torch.from_numpy(g[f"{prefix}_values"]).double())
    cnt, margin_a, margin_c = branch_report(o, batch, L.eps_clip)
    assert min(v for k, v in cnt.items() if k.startswith("actor")) >= 8, cnt
    assert min(v for k, v in cnt.items() if k.startswith("critic")) >= 4, cnt
    assert margin_a >= 1e-4 and margin_c >= 1e-4
    assert g[f"{prefix}_tie_rows"].sum() >= 4


def test_fixture_covers_both_sides_of_the_clip():
    g = gold()
    norms = [float(g[f"{p}_actor_norm"]) for p in SETS]
    assert min(norms) < 1.0 < max(norms), norms


@pytest.mark.parametrize("prefix", SETS)
def test_torch_arm_reproduces_reference_gradients(prefix):
    g = gold()
    L, batch = make(prefix)
    tha0, thc0 = L.theta_actor.clone(), L.theta_critic.clone()
    out = L.grad(batch)
    o64 = oracle64(tha0, thc0, batch, L.n, L.D, **hyper(prefix))
    for k, tol in (("new_log_probs", TOL_LP), ("entropies", TOL_LP), ("values", TOL_V)):
        d = float(np.abs(out[k].numpy() - g[f"{prefix}_{k}"]).max())
        print(prefix, k, d)
        assert d <= tol, (k, d)
    e = err(out["advantage"], torch.from_numpy(g[f"{prefix}_advantage"]).double())
    assert e <= TOL_ADV, e
    for k in ("actor_loss", "critic_loss"):
        want = float(g[f"{prefix}_{k}"])
        assert abs(float(out[k]) - want) <= 1e-5 * abs(want), (k, float(out[k]), want)
    assert_grads_within(out["actor_grad"], ref_flat(prefix, "actor", L.actor_sl), o64["actor_grad"], L.actor_sl,
                        ACTOR_GRAD_NAMES, prefix + " actor")
    assert_grads_within(out["critic_grad"], ref_flat(prefix, "critic", L.critic_sl), o64["critic_grad"], L.critic_sl,
                        CRITIC_GRAD_NAMES, prefix + " critic")
    for name, v in segs(out["actor_grad"], L.actor_sl, RUNNING + ("logstd",)).items():
        assert (v == 0).all(), name
    for k in ("actor_norm", "critic_norm"):
        want = float(g[f"{prefix}_{k}"])
        assert abs(float(out[k]) - want) <= 1e-4 * want, (k, float(out[k]), want)


@pytest.mark.parametrize("prefix", SETS)
def test_torch_arm_reproduces_reference_step(prefix):
    """One step(): the post-step parameters outside the two noise tensors, the
    running statistics after the 64 sequential updates, num_batches_tracked."""
    g = gold()
    L, batch = make(prefix)
    nbt0 = int(g[f"{prefix}.actor.before.norm1.num_batches_tracked"])
    al, cl = L.step(batch)
    assert abs(float(al) - float(g[f"{prefix}_actor_loss"])) <= 1e-5 * abs(float(g[f"{prefix}_actor_loss"]))
    assert abs(float(cl) - float(g[f"{prefix}_critic_loss"])) <= 1e-5 * abs(float(g[f"{prefix}_critic_loss"]))
    lr = L.lr
    for which, theta, sl, names in (("actor", L.theta_actor, L.actor_sl, ACTOR_GRAD_NAMES),
                                    ("critic", L.theta_critic, L.critic_sl, CRITIC_GRAD_NAMES)):
        want = segs(ref_flat(prefix, which, sl, "after"), sl, names)
        got = segs(theta, sl, names)
        gref = segs(ref_flat(prefix, which, sl), sl, names)
        for n in names:
            if n in NOISE:
                continue
            # Adam's first step moves an element by lr g / (|g| + eps): where the two
            # arms' gradients differ in rounding only, far less than lr apart — except
            # an element whose gradient is itself rounding noise (|g| near eps)
            solid = gref[n].abs() > 1e-6
            d = (got[n] - want[n]).abs()
            print(prefix, which, n, float(d.max()))
            assert float(d[solid].max() if solid.any() else 0.0) <= 0.02 * lr, (which, n, float(d.max()))
            assert float(d.max()) <= 2.0 * lr, (which, n)
    got = segs(L.theta_actor, L.actor_sl, RUNNING)
    for n in RUNNING:
        e = err(got[n], torch.from_numpy(g[f"{prefix}.actor.after.{n}"]).double())
        print(prefix, n, e)
        assert e <= 1e-6, (n, e)
    assert int(L.nbt) == nbt0 + 64 == int(g[f"{prefix}.actor.after.norm1.num_batches_tracked"])
    actor, critic = L.export()
    assert int(actor.norm1.num_batches_tracked) == nbt0 + 64
    assert torch.equal(actor.fc2.weight.detach().reshape(-1),
                       segs(L.theta_actor, L.actor_sl, ("fc2.weight",))["fc2.weight"])
    assert torch.equal(critic.fc4.bias.detach(), segs(L.theta_critic, L.critic_sl, ("fc4.bias",))["fc4.bias"])


def test_row_order_matters():
    """The minibatch order is part of the step: the advantage scans the rows
    and the running statistics take one update per row in order."""
    L, batch = make("base")
    a = L.grad(batch, update_running=False)
    rev = {k: (v.flip(0) if v is not None and k != "obs" else v) for k, v in batch.items()}
    b = L.grad(rev, update_running=False)
    assert not torch.allclose(a["advantage"], b["advantage"].flip(0), rtol=1e-3, atol=1e-3)


def fake_rollout(E, T, n, D, seed):
    g = torch.Generator().manual_seed(seed)
    rtg = torch.randn((E, 1, 1), generator=g, dtype=torch.float64).expand(E, T, n).contiguous()
    rtg[0] = 0.0  # a rollout whose every reward was zero: priority 1e-5
    return dict(obs=torch.rand((E, T, n, D), generator=g), actions=torch.rand((E, T, n, 4), generator=g),
                log_probs=torch.randn((E, T, n, 4), generator=g), values=torch.randn((E, T), generator=g), rtg=rtg)


def test_rows_gathers_the_dense_batch():
    """rows() hands the learner the observation buffer itself; the rows and
    global states read through the index equal the dense [B, n D] concatenation
    the reference materialises (ppo.py:297-302)."""
    L, _ = make("base")
    E, T, n, D = 3, 5, L.n, L.D
    out = fake_rollout(E, T, n, D, 5)
    idx = torch.tensor([7, 0, 59, 13, 13, 2, 31])
    b = L.rows(out, idx)
    assert b["obs"].data_ptr() == out["obs"].data_ptr()  # no copy
    rows, gs = gather(b, n, D, torch.float32)
    dense_rows = out["obs"].reshape(E * T * n, D)
    dense_gs = out["obs"].reshape(E * T, 1, n * D).expand(E * T, n, n * D).reshape(E * T * n, n * D)
    assert torch.equal(rows, dense_rows[idx]) and torch.equal(gs, dense_gs[idx])
    assert torch.equal(b["actions"], out["actions"].reshape(-1, 4)[idx])
    assert torch.equal(b["old_log_probs"], out["log_probs"].reshape(-1, 4)[idx])
    assert torch.equal(b["rtg"], out["rtg"].reshape(-1)[idx].float())
    assert torch.equal(b["old_values"], out["values"].reshape(E * T, 1).expand(E * T, n).reshape(-1)[idx])
    full = L.rows(out)
    assert full["index"] is None and full["old_values"].shape == (E * T * n,)
    assert torch.equal(full["old_values"], out["values"].reshape(E * T, 1).expand(E * T, n).reshape(-1))
    o = L.grad(L.rows(out, idx), update_running=False)
    assert o["new_log_probs"].shape == (7, 4)


def test_sample_draws_distinct_rows_by_priority():
    L, _ = make("base")
    E, T, n, D = 4, 5, L.n, L.D
    out = fake_rollout(E, T, n, D, 9)
    g = torch.Generator().manual_seed(3)
    for _ in range(20):
        idx = L.sample(out, 16, generator=g)
        assert idx.dtype == torch.int64 and idx.shape == (16,)
        assert len(set(idx.tolist())) == 16
        # rollout 0 has priority 1e-5 per row against ~1: never a draw of those rows only
        assert (idx >= T * n).any()
    # every row can be drawn when the batch is the whole buffer
    idx = L.sample(out, E * T * n, generator=g)
    assert sorted(idx.tolist()) == list(range(E * T * n))
