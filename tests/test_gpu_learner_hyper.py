"""The learner kernels off the reference's default hyperparameters and at the
ends of their shapes (_learner_cases.py; the inputs' fitness and every case's
ability to fail are asserted on the host in test_learner_cases_cpu.py):
lnw_ppo_grad with eps_clip, entropy_coef, gamma and lambda_ moved, the advantage
scan with 2 and 5 rows per thread and an undamped carry, the running statistics'
second trip and tail cut, n = 1, n = 16 with D = 100 and D = 52; lnw_qnet_grad
with gamma 0, 1 and 0.9, done all set and all clear, float64 rewards and action
rows of 3 and 6 columns; both Adam entry points with other betas, eps and lr,
preset step counters and moments; three step()s of each learner with every
hyperparameter off its default at once.

The bounds are the suites' own (test_gpu_ppolearn.py, test_gpu_qlearn.py).
Every test prints its largest err / bound ratio (DESIGN.md quotes them)."""
import numpy as np
import pytest
import torch

import _learner_cases as LC
import _ppolearn_util as P
import _qlearn_util as Q
from lnw.ppolearn import RUNNING, PPOLearner, running_after
from lnw.qlearn import QLearner

pytestmark = pytest.mark.gpu


def _worst(what, pairs):
    """Prints and returns the largest err / bound of (name, err, bound) rows."""
    name, e, b = max(pairs, key=lambda r: r[1] / r[2])
    print(f"{what}: largest err / bound {e / b:.3f} ({name}: {e:.3e} / {b:.3e})")
    return e / b


def _grad_pairs(out, ref, o64, H):
    rows = []
    for k, sl, names in (("actor_grad", H.actor_sl, P.ACTOR_GRAD_NAMES), ("critic_grad", H.critic_sl,
                                                                         P.CRITIC_GRAD_NAMES)):
        e, er = P.grad_errors(out[k], o64[k], sl, names), P.grad_errors(ref[k], o64[k], sl, names)
        rows += [(f"{k} {n}", e[n], P.bound(er[n])) for n in names]
    return rows


# ---- MAPPO ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LC.PPO_CASES))
def test_ppo_grad_case(name):
    """check_case over PPO_CASES: per-row tensors, both losses and every
    gradient tensor against the float64 oracle, the bound set by the float32
    host arm, both arms and the oracle at the case's hyperparameters."""
    B, n, D, hyper = LC.PPO_CASES[name]
    actor, critic, batch, o64, ref = LC.ppo_case(B, n, D, hyper)
    H, out = P.check_case(actor, critic, batch, o64, ref, f"{name} B={B} {n}x{D}", hyper=hyper)
    assert (H.eps_clip, H.entropy_coef, H.gamma, H.lambda_) == tuple(
        hyper.get(k, v) for k, v in LC.PPO_DEFAULTS.items())
    assert _worst(f"ppo grad {name}", _grad_pairs(out, ref, o64, H)) <= 1.0
    print(f"ppo rows {name}: advantage err / tolerance {P.err(out['advantage'], o64['advantage']) / P.TOL_ADV:.3f}")


@pytest.mark.parametrize("name", list(LC.PPO_RUNNING_CASES))
def test_ppo_running_statistics_case(name):
    """The four running slots after grad() against the float64 recurrence over
    all B rows in minibatch order, within 1e-6: B = 300 is a second trip of
    pl_running_kernel's 256 threads, B = 4097 cuts the sum to the last 2048 rows
    (what it drops weighs 0.9^2048)."""
    B, n, D, hyper = LC.PPO_RUNNING_CASES[name]
    actor, critic, batch, o64, _ = LC.ppo_case(B, n, D, hyper)
    H = PPOLearner(actor, critic, **hyper)
    th0 = H.theta_actor.clone()
    H.grad(batch)
    assert int(H.nbt) == B
    got, r0 = P.segs(H.theta_actor, H.actor_sl, RUNNING), P.segs(th0, H.actor_sl, RUNNING)
    rows = []
    for slot, lo, hi in (("norm1.running_mean", 0, 5), ("norm2.running_mean", 5, 13),
                         ("norm1.running_var", 13, 18), ("norm2.running_var", 18, 26)):
        want = running_after(r0[slot], o64["stats"][:, lo:hi])
        assert not torch.equal(got[slot], r0[slot])
        rows.append((slot, P.err(got[slot], want), 1e-6))
    worst = _worst(f"ppo running {name}", rows)
    assert worst <= 1.0, rows
    keep = torch.ones_like(th0, dtype=torch.bool)
    for slot in RUNNING:
        k, shp = H.actor_sl[slot]
        keep[k:k + shp[0]] = False
    assert torch.equal(H.theta_actor[keep], th0[keep])


# ---- DDQN -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LC.Q_CASES))
def test_q_grad_case(name):
    """test_shapes_against_torch_arm's comparison over Q_CASES, the float32 arm
    on the host."""
    pol, tgt, batch, gamma, bn = LC.q_case(name)
    H = QLearner(pol, tgt, gamma=gamma, policy_bn=bn)
    T = QLearner(pol, tgt, gamma=gamma, policy_bn=bn, impl="torch", device="cpu")
    o64 = Q.oracle64(H.theta, H.theta_target, batch, gamma, bn)
    out, ref = H.grad(batch), T.grad(batch)
    rows = []
    for k in ("y", "qs", "loss"):
        Q.check(k, out[k], ref[k], o64[k])
        rows.append((k, Q.err(out[k], o64[k]), Q.bound(Q.err(ref[k], o64[k]))))
    for i in range(2):
        for j in range(2):
            for lo, hi in ((0, 5), (5, 13)):
                Q.check(f"stats {i} {j} {lo}", out["stats"][i, j, lo:hi], ref["stats"][i, j, lo:hi],
                        o64["stats"][i, j, lo:hi])
    Q.assert_grads_within(out["grad"], ref["grad"], o64, H.n_in, bn, name)
    e, er = Q.grad_errors(out["grad"], o64, H.n_in, bn), Q.grad_errors(ref["grad"], o64, H.n_in, bn)
    rows += [(n, e[n], Q.bound(er[n])) for n in Q.GRAD_NAMES]
    assert _worst(f"q grad {name}", rows) <= 1.0
    for n in Q.RUNNING:
        a, b = Q.segs(H.theta_target, H.n_in, Q.RUNNING)[n], Q.segs(T.theta_target, T.n_in, Q.RUNNING)[n]
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


# ---- Adam ---------------------------------------------------------------------------------------------
def _ulps_of(got, want):
    """|got - want| in ulps of want (float32 device tensors)."""
    g, w = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    return np.abs(g.astype(np.float64) - w) / np.spacing(np.abs(w)).astype(np.float64)


def _adam_case(entry, name, count, max_norm=1e9):
    """An Adam case through one entry point against torch.optim.Adam on the
    device, step by step; returns the largest |theta - p| / bound."""
    c, h = LC.ADAM_CASES[name], LC.adam_hyper(name)
    theta, m, v, t0, grads = (x.cuda() if torch.is_tensor(x) else x for x in LC.adam_inputs(name, count))
    grads = [g.cuda() for g in grads]
    theta0 = theta.clone()
    p = torch.nn.Parameter(theta.clone())
    opt = torch.optim.Adam([p], **h)
    opt.state[p] = {"step": torch.tensor(float(t0)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    step = torch.full((1,), t0, dtype=torch.int64, device="cuda")
    clip = torch.zeros(2, device="cuda")
    clipped = entry == "ppo" and max_norm < 1e9
    worst = 0.0
    for k, g in enumerate(grads):
        before = p.detach().clone()
        if entry == "q":
            Q._adam(theta, g, m, v, step, lr=h["lr"], clamp=0.0, betas=h["betas"], eps=h["eps"])
        else:
            P._clip_adam(theta, g, m, v, step, clip, lr=h["lr"], max_norm=max_norm, betas=h["betas"], eps=h["eps"])
        p.grad = g.clone()
        if clipped:
            norm = torch.nn.utils.clip_grad_norm_([p], max_norm)
            P.close_loss("norm", clip[1], norm, 1e-6)
            P.close_loss("clip factor", clip[0], max_norm / (float(norm) + 1e-6), 1e-6)
            assert float(clip[0]) < 1.0
        elif entry == "ppo":
            assert float(clip[0]) == 1.0
        opt.step()
        assert int(step) == t0 + k + 1 == int(opt.state[p]["step"])
        bound = LC.adam_bound(before.cpu().numpy(), p.detach().cpu().numpy(), h["lr"])
        d = (theta.double() - p.detach().double()).abs().cpu().numpy()
        ratio = float((d / bound).max())
        um, uv = _ulps_of(m, opt.state[p]["exp_avg"]).max(), _ulps_of(v, opt.state[p]["exp_avg_sq"]).max()
        print(f"adam {entry} {name} count {count} step {k + 1}: theta err / bound {ratio:.3f}, m {um:.2f} ulp, "
              f"v {uv:.2f} ulp")
        assert ratio <= 1.0, (k, ratio)
        if clipped:
            # the gradient reaches Adam times a clip factor that is compared to 1e-6 relative above: m is
            # linear in it and v quadratic
            assert um <= 2 + 1e-6 / 2.0 ** -24 and uv <= 2 + 2e-6 / 2.0 ** -24, (k, um, uv)
        else:
            assert um <= 2 and uv <= 2, (k, um, uv)
        worst = max(worst, ratio)
    if h["lr"] == 0.0:
        assert torch.equal(theta, theta0)
    else:
        assert not torch.equal(theta, theta0)
    if "t0" in c:
        assert int(step) in (1000, 10 ** 6)
    return worst


@pytest.mark.parametrize("count", LC.ADAM_COUNTS)
@pytest.mark.parametrize("name", list(LC.ADAM_CASES))
@pytest.mark.parametrize("entry", ["q", "ppo"])
def test_adam_case(entry, name, count):
    """lnw_qnet_adam (clamp 0) and lnw_ppo_clip_adam (max_norm 1e9: inactive)
    over ADAM_CASES: |theta - p| <= 2 ulp(p) + 2^-21 max(lr, |update|) after every
    step, m and v within 2 ulp of torch's, the device counter against torch's
    step (preset 999 reads 1000, preset 10^6 - 1 reads 10^6); lr = 0 leaves the
    parameters bit-unchanged while m, v and the counter move."""
    _adam_case(entry, name, count)


def test_adam_case_a1_with_active_clip():
    """A1 through lnw_ppo_clip_adam with max_norm 1: the gradients' norm is about
    16, so every step is clipped; norm and factor against clip_grad_norm_."""
    _adam_case("ppo", "A1", LC.ADAM_COUNTS[0], max_norm=1.0)


# ---- end to end ---------------------------------------------------------------------------------------
def _e2e_check(what, rows):
    for name, dh, dt, bound in rows:
        print(f"{what} {name}: kernels {dh:.3e} torch arm {dt:.3e} bound {bound:.3e}")
    bad = [r for r in rows if not r[1] <= r[3]]
    _worst(f"e2e {what}", [(name, dh, bound) for name, dh, _, bound in rows])
    assert not bad, bad


def test_ppo_three_steps_every_hyperparameter_moved():
    """Three step()s at B = 129 with lr, eps_clip, entropy_coef, gamma, lambda_,
    max_grad_norm, betas and eps all off their defaults, against the torch arm
    and a float64 run of the same steps (steps64): per parameter tensor outside
    NOISE the kernels' largest deviation from the float64 run is at most 8 x the
    torch arm's own, floored at 2^-23 of the tensor's scale; the clip factors
    agree with the torch arm's to 1e-5 relative at every step and at least one
    is below 1; the step counters read 3."""
    e = LC.ppo_e2e()
    T = e["T"]
    H = PPOLearner(e["actor"], e["critic"], **LC.PPO_E2E)
    for k, b in enumerate(e["batches"]):
        H.step(b)
        hc, tc = H.clip.cpu(), e["clips"][k]
        print(f"step {k + 1} clip factor and norm:", hc.tolist(), tc.tolist())
        assert torch.allclose(hc, tc, rtol=1e-5, atol=0)
    assert bool((e["clips"][:, :, 0] < 1.0).any()) and bool((H.clip[:, 0] <= 1.0).all())
    for which, th, tt, t64, sl, names in (("actor", H.theta_actor, T.theta_actor, e["a64"], H.actor_sl,
                                           P.ACTOR_GRAD_NAMES),
                                          ("critic", H.theta_critic, T.theta_critic, e["c64"], H.critic_sl,
                                           P.CRITIC_GRAD_NAMES)):
        _e2e_check(f"ppo {which}", LC.e2e_deviations(th, tt, t64, lambda x: P.segs(x, sl, names), P.NOISE))
    assert int(H.step_actor) == int(H.step_critic) == int(T.step_actor) == LC.E2E_STEPS
    assert int(H.nbt) == int(T.nbt) == LC.E2E_STEPS * LC.E2E_ROWS


def test_q_three_steps_every_hyperparameter_moved():
    """Three step()s at B = 129 with lr, gamma, betas, eps and clamp all off
    their defaults, against the torch arm and a float64 run of the same steps
    (q_steps64), under the same per-tensor bound; the step counter reads 3."""
    e = LC.q_e2e()
    T = e["T"]
    H = QLearner(e["policy"], e["target"], **LC.Q_E2E)
    for b in e["batches"]:
        H.step(b)
    _e2e_check("q", LC.e2e_deviations(H.theta, T.theta, e["t64"], lambda x: Q.segs(x, H.n_in), Q.NOISE))
    assert int(H.step_count) == int(T.step_count) == LC.E2E_STEPS and H.nbt.tolist() == T.nbt.tolist()
