"""Float64 oracle, inputs and preconditions for the tests of the actor, critic
and rollout kernels at every fleet size (tests/test_gpu_net_shapes.py).

The oracle is the torch network itself, deep-copied to the host in float64: on
host tensors BatchedActor.features / heads / get_dist and BatchedCritic.forward
are plain torch ops, so it shares no code with the kernels. Every case built
here also carries the float32 host arm of the same network ("ref"), and asserts
on the host alone, before any kernel runs,
  * that the float32 arm meets the tolerance on these inputs (a later failure
    then points at the kernel, not at the inputs), and
  * the sensitivity preconditions: a wrongly wired float64 network (a tail
    column dropped, the first input only the 64-wide path has dropped, two fc1
    columns past 32 exchanged, two ships exchanged in the critic's input)
    differs from the right one by more than 100 x the tolerance, so such a
    fault cannot hide under it.
Nothing here needs a GPU; the cases are cached, so the tests that share one
compute it once and must not modify it.
"""
import copy
import functools

import torch

WINDOW = 49
# the project's tolerances (test_gpu_rollout.py, test_gpu_rollout_golden.py)
FEAT_RTOL, FEAT_ATOL = 1e-4, 2e-5
LOGP_ATOL = 1e-4
VALUE_ATOL = 1e-5
SENSITIVITY = 100.0  # a wiring fault moves the oracle by more than this many tolerances
SENTINEL = -7.0


def obs_dim(n):
    """Row length of a side of n small / large ships (lnw.batched.side_obs_dim)."""
    return 4 * n + 52


def f64(net):
    """The float64 host copy of a network: the oracle."""
    return copy.deepcopy(net).cpu().double()


def make_actor(D, seed):
    """A BatchedActor for rows of D floats with non-trivial norm parameters and
    running statistics. The log-std head is scaled by 0.25: with the stock
    initialisation the log-scale reaches -2.3 and |log p| 54, where the float32
    arm's own error against float64 (2.8e-5) is a quarter of the tolerance;
    scaled, it is <= 1e-6 with |log p| <= 3.5."""
    from lnw.rollout import BatchedActor
    torch.manual_seed(seed)
    a = BatchedActor.for_obs(D)
    with torch.no_grad():
        for m in (a.norm1, a.norm2):
            m.weight.add_(0.1 * torch.randn_like(m.weight))
            m.bias.add_(0.1 * torch.randn_like(m.bias))
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 2.0)
        a.layernorm.weight.add_(0.1 * torch.randn_like(a.layernorm.weight))
        a.layernorm.bias.add_(0.1 * torch.randn_like(a.layernorm.bias))
        a.log_std_head.weight.mul_(0.25)
    return a


def make_critic(n, D, seed):
    from lnw.rollout import BatchedCritic
    torch.manual_seed(seed)
    return BatchedCritic(n * D)


def random_rows(shape, seed):
    """Observation rows [..., D]: uniform values, the 49 window cells bytes / 255."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand(shape, generator=g)
    obs[..., :WINDOW] = torch.randint(0, 256, tuple(shape[:-1]) + (WINDOW,), generator=g) / 255.0
    return obs


def max_abs(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


def within(got, want, atol, rtol=0.0):
    """Every element within atol + rtol |want| (numpy's assert_allclose rule)."""
    d = (got.double() - want.double()).abs()
    return bool((d <= atol + rtol * want.double().abs()).all())


def report(name, got, ref, want, atol, rtol=0.0):
    """Print err_hip and err_ref (max-abs against float64), then assert the
    kernel's values within the tolerance. The float32 arm was asserted when
    the case was built; it is asserted again on exactly the compared elements."""
    assert within(ref, want, atol, rtol), f"{name}: the float32 host arm misses the tolerance"
    e_hip, e_ref = max_abs(got.cpu(), want), max_abs(ref, want)
    print(f"{name}: err_hip {e_hip:.3e} err_ref {e_ref:.3e} (atol {atol:g} rtol {rtol:g})")
    assert within(got.cpu(), want, atol, rtol), (name, e_hip, e_ref)
    return e_hip, e_ref


# ---------------------------------------------------------------- features
@functools.lru_cache(maxsize=None)
def features_case(n, bn, B=333):
    """Rows for lnw_actor_features at fleet size n: obs, the float64 features
    and the float32 host arm's."""
    D = obs_dim(n)
    actor = make_actor(D, 100 + n)
    obs = random_rows((B, D), 200 + n)
    with torch.no_grad():
        want = f64(actor).features(obs.double(), bn)
        ref = actor.features(obs, bn)
    assert within(ref, want, FEAT_ATOL, FEAT_RTOL), max_abs(ref, want)
    return dict(D=D, actor=actor, obs=obs, want=want, ref=ref)


# ---------------------------------------------------------------- policy
def _logp64(actor64, obs, act, bn):
    with torch.no_grad():
        return actor64.get_dist(obs.double(), act.double(), bn)[0]


def actor_preconditions(actor, obs, act, bn, want):
    """The float64 log-probabilities of a wrongly wired network against the
    right ones (want): {fault: largest change}, each asserted to exceed
    SENSITIVITY x LOGP_ATOL."""
    D = obs.shape[1]
    n_in = D - WINDOW + 12
    a64 = f64(actor)
    moved = {}
    x = obs.clone()
    x[:, D - 1] = 0.0
    moved["last tail column dropped"] = max_abs(_logp64(a64, x, act, bn), want)
    if n_in > 33:  # the 64-wide path only
        x = obs.clone()
        x[:, WINDOW + 20] = 0.0  # network input 32
        moved["network input 32 dropped"] = max_abs(_logp64(a64, x, act, bn), want)
        b64 = f64(actor)
        with torch.no_grad():
            b64.fc1.weight[:, [32, 33]] = b64.fc1.weight[:, [33, 32]]
        moved["fc1 columns 32 and 33 exchanged"] = max_abs(_logp64(b64, obs, act, bn), want)
    for k, v in moved.items():
        assert v > SENSITIVITY * LOGP_ATOL, (k, v)
    return moved


@functools.lru_cache(maxsize=None)
def policy_case(n, bn, E=150, own0=2):
    """Inputs and expected outputs of one forced-actions lnw_policy_act call at
    fleet size n (host tensors): obs [E, n, D], act [E, n, 4], alive [A, E] and
    live [E] with about 15 % zeros, the float64 log-probabilities `want` and
    the float32 host arm's `ref` [E, n, 4], keep [E, n] (alive and live)."""
    D, A = obs_dim(n), n + own0
    actor = make_actor(D, 300 + n)
    obs = random_rows((E, n, D), 400 + n)
    g = torch.Generator().manual_seed(500 + n)
    act = torch.rand((E, n, 4), generator=g)
    alive = (torch.rand((A, E), generator=g) > 0.15).to(torch.uint8)
    live = (torch.rand((E,), generator=g) > 0.15).to(torch.uint8)
    rows, arows = obs.reshape(E * n, D), act.reshape(E * n, 4)
    want = _logp64(f64(actor), rows, arows, bn)
    with torch.no_grad():
        ref = actor.get_dist(rows, arows, bn)[0]
    assert within(ref, want, LOGP_ATOL), max_abs(ref, want)
    moved = actor_preconditions(actor, rows, arows, bn, want)
    own_alive = alive[own0:own0 + n].t().bool()
    keep = own_alive & live.bool()[:, None]
    assert keep.any() and (~own_alive).any() and (own_alive & ~live.bool()[:, None]).any()
    return dict(n=n, D=D, E=E, own0=own0, A=A, bn=bn, actor=actor, obs=obs, act=act, alive=alive, live=live,
                want=want.reshape(E, n, 4), ref=ref.reshape(E, n, 4), own_alive=own_alive, keep=keep, moved=moved)


def policy_call(case, params, lo=0, hi=None, in_stride=0, pad=8):
    """One forced-actions lnw_policy_act launch on envs [lo, hi) of a
    policy_case through the C ABI. Outputs are pre-filled with SENTINEL:
    logp / act [E', 4 n + pad] (act_env_stride = 4 n + pad), full [E', A, 4]
    float64. in_stride > n D: the rows are read from a buffer with that env
    stride whose padding is NaN."""
    import ctypes as C
    from lnw import _abi
    L = _abi.load()
    n, D, own0, A = case["n"], case["D"], case["own0"], case["A"]
    hi = case["E"] if hi is None else hi
    E = hi - lo
    dev = "cuda"
    obs = case["obs"][lo:hi].reshape(E, n * D)
    if in_stride:
        buf = torch.full((E, in_stride), float("nan"))
        buf[:, :n * D] = obs
        obs = buf
    obs = obs.contiguous().to(dev)
    act = case["act"][lo:hi].contiguous().to(dev)
    alive = case["alive"][:, lo:hi].contiguous().to(dev)
    live = case["live"][lo:hi].contiguous().to(dev)
    stride = 4 * n + pad
    out = dict(logp=torch.full((E, stride), SENTINEL, device=dev), act=torch.full((E, stride), SENTINEL, device=dev),
               full=torch.full((E, A, 4), SENTINEL, dtype=torch.float64, device=dev))
    pa = _abi.PolicyArgs()
    pa.obs, pa.E, pa.n, pa.D, pa.own0, pa.A = obs.data_ptr(), E, n, D, own0, A
    pa.obs_in_env_stride = in_stride
    pa.params, pa.bn_running = params.data_ptr(), int(case["bn"] == "running")
    pa.forced, pa.forced_act, pa.fa_env_stride = 1, act.data_ptr(), n * 4
    pa.alive, pa.live = alive.data_ptr(), live.data_ptr()
    pa.act_out, pa.logp_out, pa.act_env_stride = out["act"].data_ptr(), out["logp"].data_ptr(), stride
    pa.full = out["full"].data_ptr()
    _abi.check(L.lnw_policy_act(C.byref(pa), None))
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------- critic
@functools.lru_cache(maxsize=None)
def critic_case(n, D, E=100):
    """Inputs of lnw_rollout_post for n ships of D floats (host tensors): obs
    [E, n, D], the float64 values `want` [E] and the float32 host arm's `ref`,
    rewards [E, n] float64 (exactly representable in float32), live and done
    [E] with zeros."""
    critic = make_critic(n, D, 600 + n)
    obs = random_rows((E, n, D), 700 + n)
    g = torch.Generator().manual_seed(800 + n)
    rew = torch.randn((E, n), generator=g).double()  # float32 draws: both reward dtypes hold them exactly
    live = (torch.rand((E,), generator=g) > 0.3).to(torch.uint8)
    done = (torch.rand((E,), generator=g) > 0.3).to(torch.int32)
    c64 = f64(critic)
    with torch.no_grad():
        want = c64(obs.reshape(E, n * D).double()).reshape(E)
        ref = critic(obs.reshape(E, n * D)).reshape(E)
        moved = None
        if n >= 2:
            perm = list(range(n))
            perm[0], perm[n - 1] = n - 1, 0
            swapped = c64(obs[:, perm].reshape(E, n * D).double()).reshape(E)
            moved = max_abs(swapped, want)
            assert moved > SENSITIVITY * VALUE_ATOL, moved
    assert within(ref, want, VALUE_ATOL), max_abs(ref, want)
    lv, dn = live.bool(), done != 0
    assert (lv & dn).any() and (lv & ~dn).any() and (~lv & dn).any() and (~lv & ~dn).any()
    return dict(n=n, D=D, E=E, critic=critic, obs=obs, want=want, ref=ref, rew=rew, live=live, done=done, moved=moved)


def post_call(case, packed, stop_at_done, rew_f64, pad=8):
    """One lnw_rollout_post launch on a critic_case (packed: the critic's
    parameters on the device, or None). The rows sit in a buffer with env
    stride n D + pad whose padding is NaN; val [E, 3], rew_out [E, n + 2]
    float64, running [E, 2] are pre-filled with SENTINEL / 9 and written
    through their env strides (column 0 / the first n columns); live is the
    in/out flag vector."""
    import ctypes as C
    from lnw import _abi
    L = _abi.load()
    n, D, E = case["n"], case["D"], case["E"]
    dev = "cuda"
    buf = torch.full((E, n * D + pad), float("nan"))
    buf[:, :n * D] = case["obs"].reshape(E, n * D)
    buf = buf.to(dev)
    rew = case["rew"].to(dev, torch.float64 if rew_f64 else torch.float32).contiguous()
    out = dict(val=torch.full((E, 3), SENTINEL, device=dev),
               rew=torch.full((E, n + 2), SENTINEL, dtype=torch.float64, device=dev),
               running=torch.full((E, 2), 9, dtype=torch.uint8, device=dev), live=case["live"].clone().to(dev))
    done = case["done"].to(dev)
    pp = _abi.RolloutPostArgs()
    pp.obs, pp.obs_env_stride, pp.E, pp.n, pp.D = buf.data_ptr(), n * D + pad, E, n, D
    if packed is not None:
        pp.critic = packed.data_ptr()
    pp.val, pp.val_env_stride = out["val"].data_ptr(), 3
    pp.rew, pp.rew_f64, pp.n_rew = rew.data_ptr(), int(rew_f64), n
    pp.rew_out, pp.rew_env_stride = out["rew"].data_ptr(), n + 2
    pp.done, pp.live = done.data_ptr(), out["live"].data_ptr()
    pp.running, pp.running_env_stride = out["running"].data_ptr(), 2
    pp.stop_at_done = int(stop_at_done)
    _abi.check(L.lnw_rollout_post(C.byref(pp), None))
    torch.cuda.synchronize()
    return out
