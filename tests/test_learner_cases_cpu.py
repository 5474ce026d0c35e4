"""The learner hyperparameter cases (_learner_cases.py) on the host: what
test_gpu_learner_hyper.py relies on is asserted here, so the GPU test never
discovers that an input was unfit, and every case is shown able to fail.

Preconditions (generated()'s own, run once per case): margins to every clip
boundary >= 1e-4, every actor branch populated >= 8 and every critic branch >= 4
times, the float32 host arm inside the per-row tolerances. The host arm sets
the GPU test's gradient bound 8 x max(err_ref, 2^-23), so its own error is
capped: err_ref <= REF_CAP = 1.25e-4 per tensor keeps every bound at or below
1e-3 of the tensor's largest element (a kernel inside it has three digits
right), which is 100 bounds below the smallest effect a hyperparameter has on
a gradient (0.1 of its scale, printed by the discrimination tests).

Discrimination: with one hyperparameter that a case moves put back to its
default, the float64 oracle must move some output that the GPU test compares by
>= 100 x the bound it is compared under (advantage 1e-5, a loss 1e-5 relative,
a gradient as a whole vector 8 x max(err_ref, 2^-23); DDQN y, loss, grad
likewise; an Adam parameter 2 ulp + 2^-21 max(lr, |update|))."""
import numpy as np
import pytest
import torch

import _learner_cases as LC
import _ppolearn_util as P
import _qlearn_util as Q
from lnw.ppolearn import PPOLearner
from lnw.qlearn import QLearner

REF_CAP = 1.25e-4
FACTOR = 100.0


def test_tables_reach_the_shapes_they_are_for():
    """The shapes the cases are there for, from the kernels' constants: the
    advantage scan's 1024 threads, the running tail of 2048 rows and its 256
    threads, the ABI's limits on n and D."""
    shapes = [(B, n, D) for B, n, D, _ in LC.PPO_CASES.values()]
    assert len(LC.PPO_CASES) == 10 and {(1025, 4, 68), (4097, 4, 68), (129, 1, 56), (129, 16, 100),
                                        (129, 4, 52)} <= set(shapes)
    for B, Lb, used, last in ((1025, 2, 513, 1), (4097, 5, 820, 2)):
        assert -(-B // 1024) == Lb and -(-B // Lb) == used and B - (used - 1) * Lb == last
    assert [B for B, *_ in LC.PPO_RUNNING_CASES.values()] == [300, 4097] and 256 < 300 < 2048 < 4097
    moved = {k: {h[k] for *_, h in LC.PPO_CASES.values() if k in h} for k in LC.PPO_DEFAULTS}
    assert moved == dict(eps_clip={0.1, 0.3}, entropy_coef={0.0, 0.01}, gamma={1.0, 0.9, 0.0},
                         lambda_={1.0, 0.8, 0.0})
    assert LC.ADAM_COUNTS == (3000, 257, 1) and len(LC.ADAM_CASES) == 7 and len(LC.Q_CASES) == 8


# ---- MAPPO --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LC.PPO_CASES) + ["running-300"])
def test_ppo_case_preconditions_and_host_arm(name):
    """generated() asserts margins, branch counts and the host arm's per-row
    tensors; here the host arm's gradient error per tensor under REF_CAP."""
    B, n, D, hyper = LC.PPO_RUNNING_CASES["300"] if name == "running-300" else LC.PPO_CASES[name]
    actor, critic, batch, o64, ref = LC.ppo_case(B, n, D, hyper)
    assert batch["index"] is not None and batch["rtg"].shape == (B,)
    T = PPOLearner(actor, critic, impl="torch", device="cpu")
    e = P.grad_errors(ref["actor_grad"], o64["actor_grad"], T.actor_sl, P.ACTOR_GRAD_NAMES)
    e.update({"critic " + k: v for k, v in P.grad_errors(ref["critic_grad"], o64["critic_grad"], T.critic_sl,
                                                         P.CRITIC_GRAD_NAMES).items()})
    worst = max(e, key=e.get)
    print(f"{name}: host arm's largest gradient error {e[worst]:.3e} ({worst})")
    assert e[worst] <= REF_CAP, (worst, e[worst])
    assert 0.0 < float(o64["stats"].abs().max()) < float("inf")


PPO_MOVES = [(name, k) for name, (*_, hyper) in LC.PPO_CASES.items() for k in hyper]


@pytest.mark.parametrize("name,key", PPO_MOVES, ids=[f"{n}-{k}" for n, k in PPO_MOVES])
def test_ppo_case_tells_the_default_from_its_value(name, key):
    B, n, D, hyper = LC.PPO_CASES[name]
    actor, critic, batch, o64, ref = LC.ppo_case(B, n, D, hyper)
    T = PPOLearner(actor, critic, impl="torch", device="cpu")
    back = dict(hyper, **{key: LC.PPO_DEFAULTS[key]})
    o = P.oracle64(T.theta_actor, T.theta_critic, batch, n, D, **back)
    ratios = {"advantage": P.err(o["advantage"], o64["advantage"]) / P.TOL_ADV}
    for k in ("actor_loss", "critic_loss"):
        ratios[k] = abs(float(o[k]) - float(o64[k])) / abs(float(o64[k])) / 1e-5
    for k in ("actor_grad", "critic_grad"):
        ratios[k] = P.err(o[k], o64[k]) / P.bound(P.err(ref[k], o64[k]))
    print(f"{name}, {key} back at {LC.PPO_DEFAULTS[key]}: moved, in bounds:",
          {k: f"{v:.3g}" for k, v in ratios.items()})
    assert max(ratios.values()) >= FACTOR, ratios


# ---- DDQN -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LC.Q_CASES))
def test_q_case_host_arm(name):
    """The float32 torch arm on the host, which sets the GPU test's bounds, under
    REF_CAP on every compared output; what each case is there for holds of its
    rows."""
    pol, tgt, batch, gamma, bn = LC.q_case(name)
    c = LC.Q_CASES[name]
    T = QLearner(pol, tgt, gamma=gamma, policy_bn=bn, impl="torch", device="cpu")
    o64 = Q.oracle64(T.theta, T.theta_target, batch, gamma, bn)
    ref = T.grad(batch, update_running=False)
    e = {k: Q.err(ref[k], o64[k]) for k in ("y", "qs", "loss")}
    e.update(Q.grad_errors(ref["grad"], o64, T.n_in, bn))
    worst = max(e, key=e.get)
    print(f"{name}: host arm's largest error {e[worst]:.3e} ({worst})")
    assert e[worst] <= REF_CAP, (worst, e[worst])
    done = batch["done"]
    assert batch["action"].shape == (c["B"], c.get("columns", 4)) and batch["action"].is_contiguous()
    if "done" in c:
        assert bool((done == c["done"]).all())
        if c["done"] == 0:
            assert torch.equal(o64["y"], batch["reward"].double()[:, None].expand(-1, 3))
    else:
        assert 0 < int(done.sum()) < c["B"]
    if c.get("reward_f64"):
        r = batch["reward"]
        assert r.dtype == torch.float64 and bool((r.float().double() != r).all())
    else:
        assert batch["reward"].dtype == torch.float32


Q_MOVES = [name for name, c in LC.Q_CASES.items() if "gamma" in c]


@pytest.mark.parametrize("name", Q_MOVES)
def test_q_case_tells_the_default_gamma_from_its_value(name):
    pol, tgt, batch, gamma, bn = LC.q_case(name)
    T = QLearner(pol, tgt, gamma=gamma, policy_bn=bn, impl="torch", device="cpu")
    o64 = Q.oracle64(T.theta, T.theta_target, batch, gamma, bn)
    ref = T.grad(batch, update_running=False)
    o = Q.oracle64(T.theta, T.theta_target, batch, LC.Q_GAMMA, bn)
    ratios = {k: Q.err(o[k], o64[k]) / Q.bound(Q.err(ref[k], o64[k])) for k in ("y", "loss", "grad")}
    print(f"{name}, gamma back at {LC.Q_GAMMA}: moved, in bounds:", {k: f"{v:.3g}" for k, v in ratios.items()})
    assert max(ratios.values()) >= FACTOR, ratios


# ---- Adam -----------------------------------------------------------------------------------------
def _adam_torch64(theta, m, v, t0, grads, lr, betas, eps):
    p = torch.nn.Parameter(theta.double().clone())
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    opt.state[p] = {"step": torch.tensor(float(t0)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    for g in grads:
        p.grad = g.double()
        opt.step()
    st = opt.state[p]
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), int(st["step"])


@pytest.mark.parametrize("name", list(LC.ADAM_CASES))
def test_numpy_adam_is_torch_s(name):
    """adam64 against torch.optim.Adam on float64 vectors, from the case's preset
    counter and moments: equal to float64 rounding."""
    theta, m, v, t0, grads = LC.adam_inputs(name, 257)
    h = LC.adam_hyper(name)
    want = _adam_torch64(theta, m, v, t0, grads, **h)
    got = LC.adam64(theta, m, v, t0, grads, **h)
    for a, b in zip(got[:3], want[:3]):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-15)
    assert got[3] == want[3] == t0 + len(grads)
    # the entry points' own treatment of the gradient
    big = [g * 100.0 for g in grads]
    a = LC.adam64(theta, m, v, t0, big, clamp=1.0, **h)
    b = _adam_torch64(theta, m, v, t0, [g.clamp(-1.0, 1.0) for g in big], **h)
    np.testing.assert_allclose(a[0], b[0], rtol=1e-12, atol=1e-15)
    a = LC.adam64(theta, m, v, t0, grads[:1], max_norm=1.0, **h)
    scale = min(1.0, 1.0 / (float(grads[0].double().norm()) + 1e-6))
    b = _adam_torch64(theta, m, v, t0, [grads[0].double() * scale], **h)
    np.testing.assert_allclose(a[0], b[0], rtol=1e-12, atol=1e-15)


def _adam_moved(c):
    betas = c.get("betas", LC.ADAM_DEFAULTS["betas"])
    return [k for k in ("lr", "eps", "t0") if k in c] + [f"beta{i + 1}" for i in (0, 1)
                                                         if betas[i] != LC.ADAM_DEFAULTS["betas"][i]]


ADAM_MOVES = [(name, k) for name, c in LC.ADAM_CASES.items() for k in _adam_moved(c)]


@pytest.mark.parametrize("count", LC.ADAM_COUNTS)
@pytest.mark.parametrize("name,key", ADAM_MOVES, ids=[f"{n}-{k}" for n, k in ADAM_MOVES])
def test_adam_case_tells_the_default_from_its_value(name, key, count):
    """beta1, beta2, eps, lr or the step number back at its default moves some
    parameter by >= 100 x the bound the GPU test applies to that parameter."""
    theta, m, v, t0, grads = LC.adam_inputs(name, count)
    h = LC.adam_hyper(name)
    p_case = LC.adam64(theta, m, v, t0, grads, **h)[0]
    back, t_back = dict(h), t0
    if key == "t0":
        t_back = 0
    elif key in ("beta1", "beta2"):
        b = list(h["betas"])
        b[key == "beta2"] = LC.ADAM_DEFAULTS["betas"][key == "beta2"]
        back["betas"] = tuple(b)
    else:
        back[key] = LC.ADAM_DEFAULTS[key]
    p_back = LC.adam64(theta, m, v, t_back, grads, **back)[0]
    # the bound of the last step (the largest: each step is compared on its own)
    before = LC.adam64(theta, m, v, t0, grads[:-1], **h)[0]
    bound = LC.adam_bound(before.astype(np.float32), p_case.astype(np.float32), h["lr"])
    ratio = float((np.abs(p_back - p_case) / bound).max())
    print(f"{name} count {count}, {key} back at its default: moved {ratio:.3g} bounds")
    assert ratio >= FACTOR, ratio


def test_adam_cases_a5_take_the_long_decimal_paths():
    """The shortest decimal that rounds to A5's lr has 7 digits and that of
    A5-63 has 9 (as_decimal's last trip); every other value has a short one."""
    def digits(x):
        x = np.float32(x)
        return next(d for d in range(1, 10) if np.float32(float(f"{float(x):.{d}g}")) == x)

    for name, d in (("A5", 7), ("A5-63", 9)):
        lr = LC.ADAM_CASES[name]["lr"]
        assert digits(lr) == d and float(np.float32(lr)) == lr, name
    assert [digits(x) for x in (1e-4, 3e-4, 0.9, 0.999, 0.5, 1e-8, 1e-3)] == [1, 1, 1, 3, 1, 1, 1]


# ---- end to end ---------------------------------------------------------------------------------------
def test_end_to_end_values_are_all_off_their_defaults():
    import inspect
    for cls, hyper in ((PPOLearner, LC.PPO_E2E), (QLearner, LC.Q_E2E)):
        sig = inspect.signature(cls.__init__).parameters
        for k, v in hyper.items():
            d = sig[k].default
            assert all(a != b for a, b in zip(v, d)) if isinstance(v, tuple) else v != d, k
    assert set(LC.PPO_E2E) == {"lr", "eps_clip", "entropy_coef", "gamma", "lambda_", "max_grad_norm", "betas", "eps"}
    assert set(LC.Q_E2E) == {"lr", "gamma", "betas", "eps", "clamp"}


def test_end_to_end_host_runs_are_fit():
    """What the GPU test asks of the end-to-end inputs holds of the host arms:
    some step is clipped, every deviation from the float64 run is finite, the
    DDQN clamp cuts some gradient element and every step moved the parameters."""
    e = LC.ppo_e2e()
    T = e["T"]
    assert e["clips"].shape == (LC.E2E_STEPS, 2, 2) and bool((e["clips"][:, :, 0] < 1.0).any())
    assert int(T.step_actor) == int(T.step_critic) == LC.E2E_STEPS
    for th, t64, sl, names in ((T.theta_actor, e["a64"], T.actor_sl, P.ACTOR_GRAD_NAMES),
                               (T.theta_critic, e["c64"], T.critic_sl, P.CRITIC_GRAD_NAMES)):
        rows = LC.e2e_deviations(th, th, t64, lambda x: P.segs(x, sl, names), P.NOISE)
        assert rows and all(np.isfinite(r[1]) and r[1] <= 0.02 * T.lr for r in rows), rows
    q = LC.q_e2e()
    T = q["T"]
    rows = LC.e2e_deviations(T.theta, T.theta, q["t64"], lambda x: Q.segs(x, T.n_in), Q.NOISE)
    assert rows and all(np.isfinite(r[1]) and r[1] <= 0.02 * T.lr for r in rows), rows
    g = Q.oracle64(q["policy"].packed(), q["target"].packed(), q["batches"][0], T.gamma, "batch")["grad"]
    assert int((g.abs() > T.clamp).sum()) >= 8
    assert int(T.step_count) == LC.E2E_STEPS and not torch.equal(T.theta, q["policy"].packed())
