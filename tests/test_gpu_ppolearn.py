"""The MAPPO learner step on the GPU (lnw_ppo_grad, lnw_ppo_clip_adam,
PPOLearner): against what the reference's own PPO.learn left behind
(tests/golden/ppolearn*.npz), against float64 CPU autograd, against the torch
arm over the shapes at which the kernels take another path, engineered rows,
the running statistics' order, run-to-run and graph-replay bit-equality, 20
updates end to end, and the round trip through Rollout.

The bound of every gradient comparison: err(T) = max |T - T64| / max |T64|
against the float64 oracle, and err_hip(T) <= 8 x max(err_ref(T), 2^-23), err_ref
being the same measure of the float32 reference arm (the reference's recorded
gradients, or the torch arm on the host). Per-row tensors: log-probabilities and
entropies 1e-4 absolute, values 1e-5 absolute, advantage 1e-5 of max |adv|.
Every generated case asserts its preconditions on the host before a kernel
runs: no ratio or value step within 1e-4 of a clip boundary (a float32 arm
cannot then take another branch than the oracle), every branch populated where
the batch is large enough to hold them, and the float32 host arm inside the
per-row tolerances."""
import copy

import numpy as np
import pytest
import torch

from _ppolearn_util import (ACTOR_GRAD_NAMES, CRITIC_GRAD_NAMES, NOISE, SETS, _clip_adam, assert_grads_within,
                            assert_rows_within, branch_report, check_case, close_loss, err, generated, gold, hyper,
                            load_set, oracle64, random_batch, random_nets, ref_flat, segs, steps64, ulps)
from lnw.ppolearn import RUNNING, PPOLearner, running_after

pytestmark = pytest.mark.gpu


def make(prefix, impl="hip", device="cuda", **kw):
    actor, critic, batch = load_set(prefix)
    return PPOLearner(actor, critic, impl=impl, device=device, **hyper(prefix), **kw), batch


@pytest.mark.parametrize("prefix", SETS)
def test_grad_matches_reference_and_float64(prefix):
    """lnw_ppo_grad on the recorded sets: the per-row tensors against the
    reference's and the oracle's, both losses, every gradient tensor under the
    bound with err_ref from the reference's recorded gradients, the running
    statistics against what learn() left in the actor."""
    g = gold()
    L, batch = make(prefix)
    tha0, thc0 = L.theta_actor.clone(), L.theta_critic.clone()
    out = L.grad(batch)
    o64 = oracle64(tha0, thc0, batch, L.n, L.D, **hyper(prefix))
    assert_rows_within(out, o64, prefix)
    rec = {k: torch.from_numpy(g[f"{prefix}_{k}"]).double() for k in ("new_log_probs", "entropies", "values",
                                                                       "advantage")}
    assert_rows_within(out, rec, prefix + " recorded")
    for k in ("actor_loss", "critic_loss"):
        close_loss(f"{prefix} {k} recorded", out[k], g[f"{prefix}_{k}"])
        close_loss(f"{prefix} {k} float64", out[k], o64[k])
    assert_grads_within(out["actor_grad"], ref_flat(prefix, "actor", L.actor_sl), o64["actor_grad"], L.actor_sl,
                        ACTOR_GRAD_NAMES, prefix + " actor")
    assert_grads_within(out["critic_grad"], ref_flat(prefix, "critic", L.critic_sl), o64["critic_grad"], L.critic_sl,
                        CRITIC_GRAD_NAMES, prefix + " critic")
    for name, v in segs(out["actor_grad"], L.actor_sl, RUNNING + ("logstd",)).items():
        assert (v == 0).all(), name
    for k in ("actor_norm", "critic_norm"):
        close_loss(f"{prefix} {k}", out[k], g[f"{prefix}_{k}"], 1e-4)
    got = segs(L.theta_actor, L.actor_sl, RUNNING)
    for n in RUNNING:
        e = err(got[n], torch.from_numpy(g[f"{prefix}.actor.after.{n}"]).double())
        print(prefix, n, e)
        assert e <= 1e-6, (n, e)
    # nothing else of either vector moves in grad()
    keep = torch.ones_like(tha0, dtype=torch.bool)
    for n in RUNNING:
        k, shp = L.actor_sl[n]
        keep[k:k + shp[0]] = False
    assert torch.equal(L.theta_actor[keep], tha0[keep]) and torch.equal(L.theta_critic, thc0)
    assert int(L.nbt) == int(g[f"{prefix}.actor.before.norm1.num_batches_tracked"]) + 64


@pytest.mark.parametrize("which", ["actor", "critic"])
@pytest.mark.parametrize("prefix", SETS)
def test_clip_adam_alone_reproduces_reference_step(prefix, which):
    """lnw_ppo_clip_adam on the reference's recorded gradients and pre-step
    parameters: the reference's post-step parameters to 2 ulp on every element
    (sets with the norm above and below 1: clipped and unclipped), the
    running-statistics and logstd slots bit-unchanged."""
    g = gold()
    L, _ = make(prefix)
    sl = L.actor_sl if which == "actor" else L.critic_sl
    names = ACTOR_GRAD_NAMES if which == "actor" else CRITIC_GRAD_NAMES
    theta0 = ref_flat(prefix, which, sl, "before").cuda()
    theta, grad = theta0.clone(), ref_flat(prefix, which, sl).cuda()
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    step, clip = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(2, device="cuda")
    _clip_adam(theta, grad, m, v, step, clip, lr=float(g[f"{prefix}_lr"]))
    assert int(step) == 1
    norm = float(g[f"{prefix}_{which}_norm"])
    close_loss("norm", clip[1], norm, 1e-6)
    assert (float(clip[0]) == 1.0) == (norm + 1e-6 <= 1.0), (float(clip[0]), norm)
    got, want = segs(theta, sl, names), segs(ref_flat(prefix, which, sl, "after"), sl, names)
    for n in names:
        u = ulps(got[n], want[n])
        assert u.max() <= 2, (n, u.max())
    if which == "actor":
        for n in RUNNING + ("logstd",):
            assert torch.equal(segs(theta, sl, (n,))[n], segs(theta0, sl, (n,))[n]), n
    assert not torch.equal(theta, theta0)


def test_clip_adam_against_torch():
    """Three steps with fresh random gradients against clip_grad_norm_ +
    torch.optim.Adam (the device step counter drives the bias correction), the
    third gradient below the norm: 2 ulp of the parameter plus the rounding of
    the update itself (lr * 2^-21)."""
    torch.manual_seed(3)
    n = 3000
    theta = torch.randn(n, device="cuda")
    p = torch.nn.Parameter(theta.clone())
    opt = torch.optim.Adam([p], lr=1e-3)
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    step, clip = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(2, device="cuda")
    for k in range(3):
        grad = torch.randn(n, device="cuda") * (0.3 if k < 2 else 0.001)
        _clip_adam(theta, grad, m, v, step, clip, lr=1e-3, max_norm=1.0)
        p.grad = grad.clone()
        norm = torch.nn.utils.clip_grad_norm_([p], 1.0)
        opt.step()
        assert int(step) == k + 1
        close_loss("norm", clip[1], norm, 1e-6)
        assert (float(clip[0]) == 1.0) == (k == 2)
        d = (theta - p.detach()).abs().cpu().numpy()
        tol = 2 * np.spacing(np.abs(p.detach().cpu().numpy())) + 1e-3 * 2.0 ** -21
        assert (d <= tol).all(), (k, d.max())


SHAPE_CASES = [(B, 4, 68, "shuffled") for B in (2, 63, 64, 65, 129, 257, 4096)]
SHAPE_CASES += [(B, 4, 68, "identity") for B in (64, 260)]
SHAPE_CASES += [(129, n, D, "shuffled") for n, D in ((2, 60), (3, 64), (8, 84), (12, 100))]
SHAPE_CASES += [(12 * 11, 12, 100, "identity"), (2 * 33, 2, 60, "identity")]


@pytest.mark.parametrize("B,n,D,index", SHAPE_CASES, ids=[f"{B}-{n}x{D}-{i}" for B, n, D, i in SHAPE_CASES])
def test_shapes_against_torch_arm(B, n, D, index):
    """.grad of the kernels against the float32 torch arm on the host, both
    under the float64 oracle's bound: B = 2 a partial wave and one 16-row tile,
    63 / 64 / 65 around a wave, 129 and 257 partial and several workgroups and
    (257) a second chunk of the weight-gradient slabs, 4096 the slab reductions
    over 16 chunks and 32 workgroups; (n, D) = (2, 60), (3, 64), (4, 68), (8, 84),
    (12, 100) are n_in 23, 27, 31, 47, 63 on both fc1 widths and critic inputs of
    120 .. 1200 values; identity rows (row_index NULL) and a shuffled row_index
    in which groups repeat."""
    check_case(*generated(B, n, D, index), f"B={B} {n}x{D} {index}")


def test_one_row_gives_nan():
    """B = 1: popart's unbiased std of one element is NaN, as in the reference,
    so the actor's loss is NaN and NaN is left in its gradient. The critic's loss
    does not read the advantage (ppo.py:362): it stays finite and equals the
    torch arm's."""
    actor, critic = random_nets(4, 68, 5)
    batch = random_batch(actor, critic, 1, 4, 68, 6, index="shuffled")
    H = PPOLearner(actor, critic)
    T = PPOLearner(actor, critic, impl="torch", device="cpu")
    out, ref = H.grad(batch), T.grad(batch)
    assert torch.isnan(out["actor_loss"]) and torch.isnan(ref["actor_loss"])
    assert torch.isnan(out["actor_grad"]).any() and torch.isnan(out["advantage"]).all()
    close_loss("critic_loss", out["critic_loss"], ref["critic_loss"])
    assert torch.isfinite(out["critic_grad"]).all()


def test_engineered_rows():
    """16 rows of 4 groups, identity order: every ratio exactly 1 (old
    log-probabilities = the kernel's own new ones: in range, min's tie, whose two
    halves must add up to the whole gradient); row 1's value clamped from above
    and row 2's from below (old value 1 away); row 5 a dead ship's zero row
    inside a live group; group 3 all zeros (a masked step: zero observations,
    actions, old log-probabilities and old value). Each gradient against
    float64."""
    n, D, B = 4, 68, 16
    actor, critic = random_nets(n, D, 77)
    batch = random_batch(actor, critic, B, n, D, 78)
    batch["obs"][1, 1] = 0.0
    batch["obs"][3] = 0.0
    batch["actions"][12:] = 0.0
    H0 = PPOLearner(actor, critic)
    first = H0.grad(batch, update_running=False)
    batch["old_log_probs"] = first["new_log_probs"].cpu().clone()
    batch["old_log_probs"][12:] = 0.0
    v = first["values"].cpu()
    batch["old_values"] = v + 0.05
    batch["old_values"][1] = v[1] - 1.0
    batch["old_values"][2] = v[2] + 1.0
    batch["old_values"][12:] = 0.0
    T = PPOLearner(actor, critic, impl="torch", device="cpu")
    o64 = oracle64(T.theta_actor, T.theta_critic, batch, n, D)
    ratio = torch.exp(o64["new_log_probs"] - batch["old_log_probs"].double())
    assert ((ratio[:12] - 1).abs() < 1e-5).all()
    cnt, margin_a, margin_c = branch_report(o64, batch, 0.2)
    assert margin_a >= 1e-4 and margin_c >= 1e-4 and cnt["critic_first"] + cnt["critic_second"] >= 2, cnt
    ref = T.grad(batch, update_running=False)
    H, out = check_case(actor, critic, batch, o64, ref, "engineered")
    ratio_hip = torch.exp(out["new_log_probs"] - batch["old_log_probs"].cuda())
    assert (ratio_hip[:12] == 1).all()


def test_zero_rows_with_initial_batchnorm():
    """Freshly initialised networks (BatchNorm weight 1, bias 0) on a batch with a
    dead ship's zero row and an all-zero group: conv1 of a zero window is the bias
    everywhere, its BatchNorm output is 0, so conv2's input is constant too and
    both BatchNorms divide by sqrt(0 + eps). Float sums of the statistics leave
    a few ulp there that the two factors of 316 raise to 1e-3 (the float32 host
    arm is 3e-4 off the oracle on such rows, a float-sum kernel was 6e-3 off);
    the kernels sum the statistics in double, get mean and variance of a
    constant map exactly and stay inside the per-row tolerances. The host arm is
    therefore no precondition here; it still sets the gradient bound. (On such
    rows norm1.bias and norm2.bias sit on the ReLU's kink, their pre-activation
    exactly 0: float64 autograd's own last bit decides whether the gradient
    passes, every arm is O(1) apart from it on these two tensors, and the bound,
    set by the host arm, says so.)"""
    from lnw.rollout import BatchedActor, BatchedCritic
    n, D, B = 4, 68, 16
    torch.manual_seed(91)
    actor, critic = BatchedActor.for_obs(D), BatchedCritic(n * D)
    batch = random_batch(actor, critic, B, n, D, 92)
    batch["obs"][1, 1] = 0.0
    batch["obs"][3] = 0.0
    T = PPOLearner(actor, critic, impl="torch", device="cpu")
    o0 = oracle64(T.theta_actor, T.theta_critic, batch, n, D, grad=False)
    gen = torch.Generator().manual_seed(93)  # (old values around the zeroed rows' own outputs)
    batch["old_log_probs"] = (o0["new_log_probs"] + 0.3 * torch.randn((B, 4), generator=gen).double()).float()
    batch["old_values"] = (o0["values"] + 0.3 * torch.randn(B, generator=gen).double()).float()
    o64 = oracle64(T.theta_actor, T.theta_critic, batch, n, D)
    _, margin_a, margin_c = branch_report(o64, batch, 0.2)
    assert margin_a >= 1e-4 and margin_c >= 1e-4, (margin_a, margin_c)
    ref = T.grad(batch, update_running=False)
    check_case(actor, critic, batch, o64, ref, "initial BatchNorm, zero rows")


def test_running_statistics_freeze_and_order():
    """freeze_running leaves the actor's vector bit-unchanged; without it the
    four running slots match the float64 recurrence over the rows in minibatch
    order within 1e-6, and the same rows in another order give other values."""
    n, D, B = 4, 68, 129
    actor, critic, batch, o64, _ = generated(B, n, D, "shuffled")
    H = PPOLearner(actor, critic)
    th0 = H.theta_actor.clone()
    H.grad(batch, update_running=False)
    assert torch.equal(H.theta_actor, th0) and int(H.nbt) == 0
    H.grad(batch)
    assert int(H.nbt) == B
    got = segs(H.theta_actor, H.actor_sl, RUNNING)
    r0 = segs(th0, H.actor_sl, RUNNING)
    for name, lo, hi in (("norm1.running_mean", 0, 5), ("norm2.running_mean", 5, 13),
                         ("norm1.running_var", 13, 18), ("norm2.running_var", 18, 26)):
        want = running_after(r0[name], o64["stats"][:, lo:hi])
        e = err(got[name], want)
        print(name, e)
        assert e <= 1e-6, (name, e)
    rev = dict(batch, index=batch["index"].flip(0), actions=batch["actions"].flip(0),
               old_log_probs=batch["old_log_probs"].flip(0), rtg=batch["rtg"].flip(0),
               old_values=batch["old_values"].flip(0))
    H2 = PPOLearner(actor, critic)
    H2.grad(rev)
    other = segs(H2.theta_actor, H2.actor_sl, RUNNING)
    for name in RUNNING:
        assert err(other[name], got[name].double()) > 1e-4, name


def _steps(L, batches, graph=False):
    losses = []
    if not graph:
        for b in batches:
            losses.append(torch.stack(L.step(b)))
        return torch.stack(losses)
    static = {k: v.clone() for k, v in L._batch(batches[0]).items()}
    L.grad(static, update_running=False)  # (sizes the workspace outside the capture)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        loss = torch.stack(L.step(static))
    for b in batches:
        for k, v in L._batch(b).items():
            static[k].copy_(v)
        gr.replay()
        losses.append(loss.clone())
    return torch.stack(losses)


def test_reproducible_and_graph_replay():
    """grad() twice is bitwise equal; two .step sequences of 4 updates from equal
    state are bitwise equal in both vectors, the moments and the losses; the
    same updates captured once with torch.cuda.graph and replayed equal the
    eager run bitwise, and the device step counters advance under replay."""
    n, D, B = 4, 68, 300
    actor, critic = random_nets(n, D, 21)
    batches = [{k: (v.cuda() if v is not None else None) for k, v in
                random_batch(actor, critic, B, n, D, 30 + k, index="shuffled").items()} for k in range(4)]
    L = PPOLearner(actor, critic)
    a, b = L.grad(batches[0], update_running=False), L.grad(batches[0], update_running=False)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    runs = []
    for graph in (False, False, True):
        L = PPOLearner(actor, critic, lr=1e-3)
        losses = _steps(L, batches, graph)
        torch.cuda.synchronize()
        runs.append((L.theta_actor.clone(), L.theta_critic.clone(), L.m_actor.clone(), L.v_actor.clone(),
                     L.m_critic.clone(), L.v_critic.clone(), losses, int(L.step_actor), int(L.step_critic)))
    for other in runs[1:]:
        for x, y in zip(runs[0][:7], other[:7]):
            assert torch.equal(x, y)
        assert other[7:] == runs[0][7:] == (4, 4)
    assert runs[0][6].isfinite().all() and not torch.equal(runs[0][6][0], runs[0][6][3])


@pytest.mark.parametrize("max_norm", [1.0, 100.0])
def test_step_clip_against_torch_arm(max_norm):
    """One step() of each arm from equal state, max_grad_norm 1 (clipping
    active) and 100 (inactive): the clip factors and norms agree, and so do the
    parameters wherever the gradient is not itself rounding noise."""
    n, D, B = 4, 68, 129
    actor, critic, batch, o64, _ = generated(B, n, D, "shuffled")
    H = PPOLearner(actor, critic, max_grad_norm=max_norm)
    T = PPOLearner(actor, critic, max_grad_norm=max_norm, impl="torch", device="cpu")
    H.step(batch)
    T.step(batch)
    hc, tc = H.clip.cpu(), T.clip
    print("clip factor and norm:", hc.tolist(), tc.tolist())
    assert torch.allclose(hc, tc, rtol=1e-5, atol=0)
    assert bool((hc[:, 0] == 1.0).all()) == (max_norm == 100.0) and bool((hc[:, 0] < 1.0).any()) == (max_norm == 1.0)
    for th, tt, sl, names, g64 in ((H.theta_actor, T.theta_actor, H.actor_sl, ACTOR_GRAD_NAMES, o64["actor_grad"]),
                                   (H.theta_critic, T.theta_critic, H.critic_sl, CRITIC_GRAD_NAMES,
                                    o64["critic_grad"])):
        a, b, g = segs(th, sl, names), segs(tt, sl, names), segs(g64, sl, names)
        for nm in names:
            if nm in NOISE:
                continue
            solid = g[nm].abs() > 1e-6
            d = (a[nm] - b[nm]).abs()
            assert float(d[solid].max() if solid.any() else 0.0) <= 0.02 * H.lr, (nm, float(d.max()))


def test_twenty_steps_against_torch_arm():
    """20 step()s on four fixed batches of 256 rows, the kernels against the
    torch arm on the device and a float64 run of the same 20 steps on the host.
    Per parameter tensor (the two noise-gradient tensors apart), the kernels'
    largest deviation from the float64 run is at most 8 x the torch float32
    arm's own, floored at one float32 ulp of the tensor's scale. The largest
    loss and parameter deviations are printed ("MAPPO learner")."""
    n, D, B, lr = 4, 68, 256, 1e-4
    actor, critic = random_nets(n, D, 11)
    cpu = [random_batch(actor, critic, B, n, D, 300 + k, index="shuffled") for k in range(4)]
    dev = [{k: (v.cuda() if v is not None else None) for k, v in b.items()} for b in cpu]
    H = PPOLearner(actor, critic, lr=lr)
    T = PPOLearner(actor, critic, lr=lr, impl="torch", device="cuda")
    worst = 0.0
    for k in range(20):
        lh, lt = H.step(dev[k % 4]), T.step(dev[k % 4])
        for x, y in zip(lh, lt):
            worst = max(worst, abs(float(x) - float(y)) / abs(float(y)))
    a64, c64 = steps64(actor, critic, cpu, 20, n, D, lr)
    print(f"largest relative loss deviation between the arms over 20 steps: {worst:.3e}")
    assert worst < 1e-3
    bad = []
    for which, th, tt, t64, sl, names in (("actor", H.theta_actor, T.theta_actor, a64, H.actor_sl, ACTOR_GRAD_NAMES),
                                          ("critic", H.theta_critic, T.theta_critic, c64, H.critic_sl,
                                           CRITIC_GRAD_NAMES)):
        a, b, c = segs(th, sl, names), segs(tt, sl, names), segs(t64, sl, names)
        for nm in names:
            if nm in NOISE:
                continue
            dh = float((a[nm].double() - c[nm]).abs().max())
            dt = float((b[nm].double() - c[nm]).abs().max())
            floor = 2.0 ** -23 * float(c[nm].abs().max())
            print(f"{which} {nm}: kernels {dh:.3e} torch arm {dt:.3e} (in lr: {dh / lr:.3f} {dt / lr:.3f})")
            if not dh <= 8 * max(dt, floor):
                bad.append((which, nm, dh, dt))
    assert not bad, bad
    assert int(H.step_actor) == int(T.step_actor) == 20 and int(H.nbt) == int(T.nbt) == 20 * B


REF_BLUE = [(6, 61), (10, 81), (8, 70), (11, 58)]
REF_RED = [(98, 48), (98, 52), (98, 56), (96, 52)]


def test_rollout_round_trip():
    """8 envs x 5 steps of 4v4: Rollout.run() -> sample(64) -> step -> export()
    -> a second Rollout.run(forced_actions=...). The second run's
    log-probabilities are those of the updated actor: they equal the torch arm's
    updated actor on the same rows within 1e-4, and differ from the first
    run's."""
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    from lnw.rollout import BatchedActor, BatchedCritic, Rollout
    E, T = 8, 5
    sc = Scenario(landing_ops=False, auto_reset=False, trained_red=False)
    g = BatchedGame(E, ["small"] * 4, ["large"] * 4, scenario=sc, seed=3)
    g.reset(positions=REF_BLUE + REF_RED, box=((40, 40), (57, 65)))
    torch.manual_seed(4)
    actor, critic = BatchedActor.for_obs(g.Db).cuda(), BatchedCritic(g.Db * g.nb).cuda()
    actor_t, critic_t = copy.deepcopy(actor), copy.deepcopy(critic)
    r = Rollout(g, actor, critic, steps=T, stop_at_done=False, seed=5)
    out = {k: v.clone() for k, v in r.run().items()}
    rtg = torch.randn((E, T, g.nb), generator=torch.Generator().manual_seed(1), dtype=torch.float64).cuda()
    H = PPOLearner(actor, critic)
    Tm = PPOLearner(actor_t, critic_t, impl="torch", device="cuda")
    idx = H.sample(out, 64, generator=torch.Generator(device="cuda").manual_seed(2), rtg=rtg)
    assert len(set(idx.tolist())) == 64
    batch = H.rows(out, idx, rtg=rtg)
    assert batch["obs"].data_ptr() == out["obs"].data_ptr()
    lh, lt = H.step(batch), Tm.step(batch)
    assert lh[0].dim() == 0 and lh[0].is_cuda and all(bool(x.isfinite()) for x in lh)
    close_loss("actor loss", lh[0], lt[0], 1e-4)
    close_loss("critic loss", lh[1], lt[1], 1e-4)
    H.export()
    Tm.export()
    assert actor.fc1.weight.is_cuda and int(actor.norm1.num_batches_tracked) == 64
    assert torch.equal(actor.fc1.weight.detach().reshape(-1).cpu(),
                       segs(H.theta_actor, H.actor_sl, ("fc1.weight",))["fc1.weight"])
    g.reset(positions=REF_BLUE + REF_RED, box=((40, 40), (57, 65)))
    forced = torch.zeros((E, T, g.A, 4), device="cuda")
    forced[:, :, :g.nb] = out["actions"]
    out2 = r.run(forced_actions=forced)
    with torch.no_grad():
        want, _ = actor_t.get_dist(out2["obs"].reshape(-1, g.Db), out2["actions"].reshape(-1, 4), bn="sample")
    got = out2["log_probs"].reshape(-1, 4)
    live = out2["obs"].reshape(-1, g.Db).abs().sum(1) > 0
    assert live.sum() >= E * T  # (ships sink in this close spawn box: their rows are zeros)
    d = float((got - want)[live].abs().max())
    print("second run's log-probabilities against the torch arm's updated actor:", d)
    assert d <= 1e-4, d
    moved = float((got - out["log_probs"].reshape(-1, 4))[live].abs().max())
    print("and against the first run's:", moved)
    assert moved > 5e-4, moved
    g.close()
