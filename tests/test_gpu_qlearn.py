"""The DDQN learner step on the GPU (lnw_qnet_grad, lnw_qnet_adam, QLearner):
against what the reference's own optimize() left behind
(tests/golden/qlearn.npz), against float64 CPU autograd, against the torch arm
on the device over the shapes at which the kernels take another path, an
engineered max-pool tie, run-to-run and graph-replay bit-equality, 20 updates
end to end, and the round trip through QCollector.

The bound of every comparison: err(T) = max |T - T64| / max |T64| against the
float64 oracle, and err_hip(T) <= 8 x max(err_ref(T), 2^-23), err_ref being the
same measure of the float32 reference arm (the reference's recorded tensors, or
the torch arm)."""
import numpy as np
import pytest
import torch

from _qlearn_util import (GRAD_NAMES, NOISE, RUNNING, SETS, _adam, assert_grads_within, bound, check, err, gold,
                          load_set, oracle64, random_batch, random_net, ref_grad_flat, segs)

pytestmark = pytest.mark.gpu


def make(prefix, policy_bn, impl="hip", device="cuda", **kw):
    from lnw.qlearn import QLearner
    g = gold()
    pol, tgt, batch = load_set(prefix)
    kw.setdefault("lr", float(g[f"{prefix}_lr"]))
    return QLearner(pol, tgt, gamma=float(g[f"{prefix}_gamma"]), policy_bn=policy_bn, impl=impl, device=device,
                    **kw), batch


@pytest.mark.parametrize("prefix,policy_bn", SETS)
def test_grad_matches_reference_and_float64(prefix, policy_bn):
    """lnw_qnet_grad on the recorded sets: y, qs, loss and every gradient tensor
    against the float64 oracle under the bound, err_ref taken from the
    reference's recorded tensors; the batch statistics likewise with the torch
    arm on the host as the float32 arm; the running statistics against what
    optimize() left in the networks."""
    g = gold()
    L, batch = make(prefix, policy_bn)
    T, _ = make(prefix, policy_bn, impl="torch", device="cpu")
    theta0, target0 = L.theta.clone(), L.theta_target.clone()
    out = L.grad(batch)
    ref = T.grad(batch)
    o64 = oracle64(theta0, target0, batch, float(g[f"{prefix}_gamma"]), policy_bn)
    check("y", out["y"], g[f"{prefix}_y"], o64["y"])
    check("qs", out["qs"], g[f"{prefix}_qs"], o64["qs"])
    check("loss", out["loss"], g[f"{prefix}_loss"], o64["loss"])
    for i, net in enumerate(("policy", "target")):
        for j, st in enumerate(("mean", "var")):
            for lo, hi, conv in ((0, 5, "conv1"), (5, 13, "conv2")):
                check(f"stats {net} {st} {conv}", out["stats"][i, j, lo:hi], ref["stats"][i, j, lo:hi],
                      o64["stats"][i, j, lo:hi])
    assert_grads_within(out["grad"], ref_grad_flat(prefix, L.n_in), o64, L.n_in, policy_bn, prefix)
    for n, v in segs(out["grad"], L.n_in, RUNNING).items():
        assert (v == 0).all(), n
    # running statistics: the policy's only under batch statistics, the target's always
    for theta, theta_before, which in ((L.theta, theta0, "policy"), (L.theta_target, target0, "target")):
        got, before = segs(theta, L.n_in, RUNNING), segs(theta_before, L.n_in, RUNNING)
        for n in RUNNING:
            want = g[f"{prefix}.{which}.after.{n}"]
            if which == "policy" and policy_bn == "running":
                assert torch.equal(got[n], before[n]) and np.array_equal(want, before[n].numpy()), n
            else:
                np.testing.assert_allclose(got[n].numpy(), want, rtol=2e-6, atol=1e-7, err_msg=f"{which} {n}")
    # nothing else of either vector moves in grad()
    keep = torch.ones_like(theta0, dtype=torch.bool)
    for n in RUNNING:
        k, shp = L.slices[n]
        keep[k:k + shp[0]] = False
    assert torch.equal(L.theta[keep], theta0[keep]) and torch.equal(L.theta_target[keep], target0[keep])
    assert L.nbt.tolist() == [int(policy_bn == "batch"), 1]


def test_freeze_running_leaves_both_vectors():
    L, batch = make("blue", "batch")
    theta0, target0 = L.theta.clone(), L.theta_target.clone()
    a = L.grad(batch, update_running=False)
    assert torch.equal(L.theta, theta0) and torch.equal(L.theta_target, target0) and L.nbt.tolist() == [0, 0]
    b = L.grad(batch, update_running=False)
    assert torch.equal(a["grad"], b["grad"]) and torch.equal(a["loss"], b["loss"])


def ulps(a, b):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    return np.abs(a.astype(np.float64) - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))


@pytest.mark.parametrize("prefix,policy_bn", SETS)
def test_adam_alone_reproduces_reference_step(prefix, policy_bn):
    """lnw_qnet_adam on the reference's recorded gradients and pre-step
    parameters: the reference's post-step parameters to 2 ulp on every element,
    the running-statistics slots bit-unchanged."""
    g = gold()
    pol, _, _ = load_set(prefix)
    after, _, _ = load_set(prefix, "after")
    theta0 = pol.packed().cuda()
    theta, grad = theta0.clone(), ref_grad_flat(prefix, pol.n_in).cuda()
    m, v, step = torch.zeros_like(theta), torch.zeros_like(theta), torch.zeros(1, dtype=torch.int64, device="cuda")
    _adam(theta, grad, m, v, step, lr=float(g[f"{prefix}_lr"]))
    assert int(step) == 1
    want = after.packed()
    names = [n for n in GRAD_NAMES]
    got_s, want_s = segs(theta, pol.n_in, names), segs(want, pol.n_in, names)
    for n in names:
        u = ulps(got_s[n], want_s[n])
        assert u.max() <= 2, (n, u.max())
    for n, s in segs(theta, pol.n_in, RUNNING).items():
        assert torch.equal(s, segs(theta0, pol.n_in, RUNNING)[n]), n
    assert not torch.equal(theta, theta0)


def test_adam_three_steps_and_clamp():
    """Three steps with fresh random gradients against torch.optim.Adam (the
    device step counter drives the bias correction), then gradients scaled x100
    against Adam on the clamped gradient. 2 ulp of the parameter plus the
    rounding of the update itself (lr * 2^-21: torch's device Adam may fuse or
    order the update's float32 operations differently)."""
    torch.manual_seed(3)
    n = 3000
    theta = torch.randn(n, device="cuda")
    p = torch.nn.Parameter(theta.clone())
    opt = torch.optim.Adam([p], lr=1e-3)
    m, v, step = torch.zeros_like(theta), torch.zeros_like(theta), torch.zeros(1, dtype=torch.int64, device="cuda")
    for k in range(4):
        grad = torch.randn(n, device="cuda") * (100.0 if k == 3 else 0.3)
        _adam(theta, grad, m, v, step, lr=1e-3, clamp=1.0)
        p.grad = grad.clamp(-1.0, 1.0)
        opt.step()
        assert int(step) == k + 1
        d = (theta - p.detach()).abs().cpu().numpy()
        tol = 2 * np.spacing(np.abs(p.detach().cpu().numpy())) + 1e-3 * 2.0 ** -21
        assert (d <= tol).all(), (k, d.max())
    # clamp <= 0: no clamping
    t2, m2, v2, s2 = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda"), \
        torch.zeros(1, dtype=torch.int64, device="cuda")
    _adam(t2, torch.full((8,), 50.0, device="cuda"), m2, v2, s2, clamp=0.0)
    assert torch.allclose(m2, torch.full((8,), 5.0, device="cuda"))


SHAPE_CASES = [(bn, B, D) for bn in ("batch", "running") for B in (1, 3, 64, 600) for D in (52, 68, 72, 84, 100)]
SHAPE_CASES.append(("batch", 8321, 68))


@pytest.mark.parametrize("policy_bn,B,D", SHAPE_CASES, ids=[f"{bn}-{B}-{D}" for bn, B, D in SHAPE_CASES])
def test_shapes_against_torch_arm(B, D, policy_bn):
    """.grad of the kernels against the torch arm on the device, both under the
    float64 oracle's bound: B = 600 spans several workgroups with a partial last
    one, D = 52 / 68 / 84 are n_in 15 / 31 / 47 (both head widths), D = 72 and
    100 are n_in 35 and 63, the narrowest and the widest row of the 64-wide
    path (63 of the head-gradient kernel's 64 lanes), B = 1 and 3 the smallest
    batches torch's training-mode BatchNorm accepts. B = 8321 is 66 workgroups,
    the last holding one row: the reduction kernels' loop over the workgroups'
    partials (one per lane) makes a second trip. That case takes its float32
    arm on the host, as test_grad_matches_reference_and_float64 does: the
    device arm's first convolution at a new batch size this large spends about
    20 s in the library's kernel search, the host arm 0.03 s."""
    from lnw.qlearn import QLearner
    pol, tgt = random_net(D, 100 + D), random_net(D, 200 + D)
    batch = random_batch(B, D, 7 * B + D)
    host = {k: v.cpu() for k, v in batch.items()}
    arm = "cuda" if B <= 600 else "cpu"
    H = QLearner(pol, tgt, policy_bn=policy_bn)
    T = QLearner(pol, tgt, policy_bn=policy_bn, impl="torch", device=arm)
    o64 = oracle64(H.theta, H.theta_target, host, 0.99, policy_bn)
    out, ref = H.grad(batch), T.grad(batch if arm == "cuda" else host)
    for name in ("y", "qs", "loss"):
        check(name, out[name], ref[name], o64[name])
    for i in range(2):
        for j in range(2):
            for lo, hi in ((0, 5), (5, 13)):
                check(f"stats {i} {j} {lo}", out["stats"][i, j, lo:hi], ref["stats"][i, j, lo:hi],
                      o64["stats"][i, j, lo:hi])
    assert_grads_within(out["grad"], ref["grad"], o64, H.n_in, policy_bn, f"B={B} D={D} {policy_bn}")
    for n in RUNNING:
        a, b = segs(H.theta_target, H.n_in, RUNNING)[n], segs(T.theta_target, T.n_in, RUNNING)[n]
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def tie_case(policy_bn, last=False):
    """The engineered batch: (policy, target, batch on the host). last: row 0's
    first maximum lowered by 2^-20, so the gradient goes to the last one."""
    D, B = 68, 8
    pol, tgt = random_net(D, 31), random_net(D, 32)
    with torch.no_grad():
        pol.conv1.weight[0].zero_()
        pol.conv1.weight[0, 0, 1, 1] = 1.0
        pol.conv1.bias[0] = 0.0
        pol.norm1.weight[0], pol.norm1.bias[0] = 1.0, 0.5
        pol.norm1.running_mean[0], pol.norm1.running_var[0] = 0.0, 1.0
        pol.radar.bias[1] = pol.attack.bias[4] = pol.movement.bias[49] = -100.0
    batch = random_batch(B, D, 5, device="cpu")
    win = torch.rand(7, 7, generator=torch.Generator().manual_seed(9)) * 0.5
    win[0, 0], win[0, 1], win[1, 0], win[1, 1] = 0.3, 0.75, 0.1, 0.75
    if last:
        win[0, 1] -= 2.0 ** -20
    batch["state"][0, :49] = win.reshape(-1)
    batch["reward"][0] = 20.0  # row 0's residual, and so its share of the conv gradients, dominates
    act = batch["action"]
    act[:, 0], act[:, 1], act[:, 2] = 0, act[:, 1] % 4, act[:, 2] % 49
    act[1, :3] = torch.tensor([1, 4, 49], dtype=torch.int32)
    return pol, tgt, batch


@pytest.mark.parametrize("policy_bn", ["running", "batch"])
def test_engineered_pool_tie_and_dead_row(policy_bn):
    """conv1 channel 0 has only its centre tap: its map is the window itself,
    exactly. Row 0's window has two equal positive maxima inside the first pool
    window, at (0, 1) and (1, 1), with different neighbours, so the conv1 weight
    gradient tells the first maximum from the last (the oracle with the first
    one lowered by 2^-20 differs by more than 1e-3 of the gradient's scale).
    Row 1 chose outputs that are dead (pre-activation < 0) and that no other row
    chose: their W and b gradients are exactly 0."""
    from lnw.qlearn import QLearner
    pol, tgt, batch = tie_case(policy_bn)
    H = QLearner(pol, tgt, policy_bn=policy_bn)
    T = QLearner(pol, tgt, policy_bn=policy_bn, impl="torch", device="cpu")
    o64 = oracle64(H.theta, H.theta_target, batch, 0.99, policy_bn)
    _, _, batch_last = tie_case(policy_bn, last=True)
    o64_last = oracle64(H.theta, H.theta_target, batch_last, 0.99, policy_bn)
    g_first, g_last = o64["grad"][:9], o64_last["grad"][:9]
    apart = float((g_first - g_last).abs().max() / g_first.abs().max())
    assert apart > 1e-3, apart
    out, ref = H.grad(batch), T.grad(batch)
    assert (out["qs"][1] == 0).all()
    assert_grads_within(out["grad"], ref["grad"], o64, H.n_in, policy_bn, f"tie {policy_bn}")
    assert err(out["grad"][:9], g_first) < apart / 100
    s = segs(out["grad"], H.n_in)
    n_in = H.n_in
    for name, row in (("radar.weight", 1), ("attack.weight", 4), ("movement.weight", 49)):
        assert (s[name].reshape(-1, n_in)[row] == 0).all(), name
    assert s["radar.bias"][1] == 0 and s["attack.bias"][4] == 0 and s["movement.bias"][49] == 0


def _five_steps(L, batches, graph=False):
    losses = []
    if not graph:
        for b in batches:
            losses.append(L.step(b))
        return torch.stack(losses)
    static = {k: v.clone() for k, v in L.rows(batches[0]).items()}
    L.grad(static, update_running=False)  # (sizes the workspace outside the capture)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        loss = L.step(static)
    # the capture ran nothing: the state is untouched
    for b in batches:
        for k, v in L.rows(b).items():
            static[k].copy_(v)
        gr.replay()
        losses.append(loss.clone())
    return torch.stack(losses)


def test_reproducible_and_graph_replay():
    """Two .step sequences of 5 updates from equal state are bitwise equal in
    theta, m, v and the losses; the same 5 updates captured once with
    torch.cuda.graph and replayed equal the eager run bitwise (the device step
    counter advances inside the graph)."""
    from lnw.qlearn import QLearner
    D = 68
    batches = [random_batch(200, D, 50 + k) for k in range(5)]
    runs = []
    for graph in (False, False, True):
        L = QLearner(random_net(D, 1), random_net(D, 2), lr=1e-3)
        losses = _five_steps(L, batches, graph)
        torch.cuda.synchronize()
        runs.append((L.theta.clone(), L.m.clone(), L.v.clone(), L.theta_target.clone(), losses, int(L.step_count)))
    for other in runs[1:]:
        for a, b in zip(runs[0][:5], other[:5]):
            assert torch.equal(a, b)
        assert other[5] == runs[0][5] == 5
    assert runs[0][4].isfinite().all() and not torch.equal(runs[0][4][0], runs[0][4][4])


def test_twenty_updates_against_torch_arm():
    """20 updates on fixed batches, kernels against the torch arm on the device.
    Every step's loss is judged on its own under the loss bound: each arm's loss
    against the float64 oracle run from that arm's own pre-step state. The final
    parameters, apart from the noise-gradient tensors, may differ by Adam's
    steps on gradients that differ within rounding: where a gradient's sign is
    itself noise each of the 20 steps can move the two arms lr apart, so 20 lr
    bounds every element. The largest deviations are printed."""
    from lnw.qlearn import QLearner
    D, lr = 68, 1e-4
    pol, tgt = random_net(D, 11), random_net(D, 12)
    H = QLearner(pol, tgt, lr=lr)
    T = QLearner(pol, tgt, lr=lr, impl="torch", device="cuda")
    batches = [random_batch(256, D, 300 + k) for k in range(4)]
    cpu = [{k: v.cpu() for k, v in b.items()} for b in batches]
    worst = traj = 0.0
    for k in range(20):
        b = batches[k % 4]
        l64h = oracle64(H.theta, H.theta_target, cpu[k % 4], 0.99, "batch")["loss"]
        l64t = oracle64(T.theta, T.theta_target, cpu[k % 4], 0.99, "batch")["loss"]
        lh, lt = H.step(b), T.step(b)
        eh, et = err(lh, l64h), err(lt, l64t)
        assert eh <= bound(et), (k, eh, et)
        worst = max(worst, eh)
        traj = max(traj, abs(float(lh) - float(lt)) / abs(float(lt)))
        if k % 5 == 4:
            H.sync_target()
            T.sync_target()
    print(f"largest loss error against float64 over 20 steps: {worst:.3e}; between the arms: {traj:.3e}")
    a, b = segs(H.theta, H.n_in), segs(T.theta, T.n_in)
    dev = {n: float((a[n] - b[n]).abs().max()) for n in GRAD_NAMES if n not in NOISE}
    print("largest parameter deviation:", max(dev.values()), dev)
    assert max(dev.values()) <= 20 * lr * 1.01
    assert int(H.step_count) == int(T.step_count) == 20 and H.nbt.tolist() == T.nbt.tolist()


def test_collector_round_trip():
    """QCollector fills its ring on a small DISCRETE game, sample(64) ->
    learner.step, then the collector acts from learner.target_params after
    sync_target(); export() loads into a fresh BatchedQNet whose q() equals what
    acting computed."""
    from lnw.batched import BatchedGame
    from lnw.config import Scenario
    from lnw.qlearn import BatchedQNet, QCollector, QLearner
    E = 8
    sc = Scenario(discrete=True, landing_ops=False, trained_red=False, auto_reset=False)
    g = BatchedGame(E, ["small"] * 2, ["large"] * 2, scenario=sc, seed=3)
    g.reset(positions=[(6, 61), (10, 81), (98, 48), (98, 52)], box=((40, 40), (57, 65)))
    net = random_net(g.Db, 41).cuda()
    col = QCollector(g, net, red="random", capacity=16, seed=1)
    for _ in range(16):
        col.step(eps=0.5)
    L = QLearner(net, lr=1e-3)
    gen = torch.Generator(device="cuda").manual_seed(0)
    before = L.params.clone()
    loss = L.step(col.sample(64, generator=gen))
    assert loss.dim() == 0 and loss.is_cuda and bool(loss.isfinite())
    assert not torch.equal(L.params, before) and torch.equal(L.target_params[:45], before[:45])
    L.sync_target()
    assert torch.equal(L.params, L.target_params)
    col.refresh_params(params=L.target_params)
    assert col._bp.data_ptr() == L.target_params.data_ptr()
    k = col.step(eps=0.0)
    fresh = BatchedQNet.for_obs(g.Db)
    L.policy, L.target = fresh, None
    L.export()
    fresh = fresh.cuda()
    assert torch.equal(fresh.packed(), L.params)
    obs = col.state[k]
    q = fresh.q(obs.reshape(-1, g.Db))
    o = fresh._launch(obs, torch.ones((2, E), dtype=torch.uint8, device="cuda"), 0, 2, want_q=True,
                      params=L.target_params)
    assert torch.equal(q, o["q"])
    assert int(fresh.norm1.num_batches_tracked) == 1
    g.close()
