"""On-device MAPPO rollout pieces around the batched step (SURVEY.md §8(f) rows
1-3): the reference's actor / critic (lnw/nets.py) acting for every (env, ship)
at once, rollout storage as [E, T, ...] device tensors, the reference's
reward-to-go and GAE as batched tensor ops, and the scripted red action
profiles as a device table. Observations never leave the GPU.

Reference: ppo.py:421-671 (rollout), ppo.py:452-482 (parameter noise),
ppo.py:645-659 (reward-to-go), ppo.py:695-714 (gae), game.py:173-182 and
536-542 (red_steps*.csv profiles).
"""
import os

import numpy as np
import torch

from . import _abi, layout
from .batched import BatchedGame
from .keyed import keyed_normal, keyed_uniform
from .layout import ACTOR_NAMES, CONV_PARAMS, WINDOW, actor_slices, flat_size  # noqa: F401
from .nets import (NOISE_FREE, BatchedActor, BatchedCritic, flat_n_in, noise_mask,  # noqa: F401
                   unpack_policy)

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def perturbed_theta(theta, member0, members, std, clip, seed, call, T, dtype=torch.float32):
    """What lnw_actor_perturb computes, restated with torch ops: the flat vectors
    [members, P] of population members member0 .. member0 + members - 1,
    theta_m = theta + mask * clamp(std * z_m, -clip, +clip) (ppo.py:474-475) with
    z_m = keyed_normal(row0 = m, rows = 1, cols = P, seed, slot = call * T * 4 + 3):
    slot 3 of the rollout's first step, which no action draw uses (0: blue
    sample, 1: blue action noise, 2: red sample; 3 is a learning red actor's
    action noise, which Rollout refuses at step 0 beside parameter noise).
    std == 0 returns theta itself.
    dtype=torch.float64 evaluates the same uniforms in double (tests)."""
    theta = theta.reshape(-1)
    P = theta.numel()
    base = theta.to(dtype)[None].expand(members, P)
    if float(std) == 0.0:
        return base.clone()
    mask = noise_mask(flat_n_in(P), theta.device) != 0
    u = keyed_uniform(member0, members, P, seed, (int(call) * int(T)) * 4 + 3, theta.device).to(dtype)
    z = torch.sqrt(-2.0 * torch.log1p(-u[:, :P])) * torch.cos((2.0 * np.pi) * u[:, P:])
    nz = torch.clamp(std * z, -clip, clip)
    return base + torch.where(mask[None], nz, torch.zeros((), dtype=dtype, device=theta.device))


def red_script_table(device="cuda", dtype=torch.float64):
    """The scripted red profiles (red_steps.csv, red_steps2.csv, red_steps3.csv;
    game.py:173-182) as a device tensor [3, 40, 4] = [red ship, step, action].
    float64: the reference's CSV rows are Python floats (game.py:181), so a step
    that contains one runs in float64 (np.asarray upcast, ppo.py:577)."""
    return torch.as_tensor(np.load(os.path.join(DATA, "red_steps.npy")), dtype=dtype, device=device)


def red_script_actions(table, step, n_red):
    """Red actions of one step for untrained red (ppo.py:560-565): profile i for
    red ship i < 3; ships beyond the three profiles, and steps past the 40 rows,
    get zero actions (the reference indexes past its lists there)."""
    out = torch.zeros((n_red, 4), dtype=table.dtype, device=table.device)
    if step < table.shape[1]:
        k = min(n_red, table.shape[0])
        out[:k] = table[:k, step]
    return out


def reference_rtg(rewards, gamma):
    """ppo.py:645-659 reward-to-go for rollouts rewards [R, T, n] (one rollout
    per leading index), as the reference computes it. The loop walks the steps
    in reverse and the ships in order, `discounted_reward += gamma * r`, and
    appends the accumulator after every term; the reward buffer has a trailing
    dim of 1, so after the first term the accumulator is a 1-element ndarray
    updated in place and every appended entry is that same array. Every element
    of the result is therefore gamma * (sum of the rollout's rewards), summed in
    that order. Returned as float64 [R, T, n], like the reference's buffer."""
    R, T, n = rewards.shape
    rev = torch.flip(rewards.to(torch.float64), dims=[1]).reshape(R, T * n)
    total = torch.cumsum(gamma * rev, dim=1)[:, -1]
    return total[:, None, None].expand(R, T, n).contiguous()


def discounted_rtg(rewards, gamma):
    """Per-ship discounted return G_t = r_t + gamma * G_{t+1} over [R, T, n]
    (what the reference's loop is meant to compute; not used by it)."""
    out = torch.zeros_like(rewards, dtype=torch.float64)
    acc = torch.zeros_like(rewards[:, 0], dtype=torch.float64)
    for t in reversed(range(rewards.shape[1])):
        acc = rewards[:, t].to(torch.float64) + gamma * acc
        out[:, t] = acc
    return out


def gae(rewards, values, gamma, lambda_=0.95):
    """ppo.py:695-714 `PPO.gae`, batched over leading dims (the sequence runs
    along the last dim), same operation order. The reference learner calls it
    on the reward-to-go and critic values of a minibatch, treating the sampled
    rows as the sequence (ppo.py:336)."""
    returns = torch.zeros_like(rewards)
    n = rewards.shape[-1]
    g = torch.zeros_like(rewards[..., 0])
    for i in reversed(range(n)):
        if i < n - 1:
            delta = rewards[..., i] + gamma * values[..., i + 1] - values[..., i]
            g = delta + gamma * lambda_ * g
        else:
            delta = rewards[..., i] - values[..., i]
            g = delta
        returns[..., i] = g + values[..., i]
    return returns


# The rollout's fast path observes into the buffer directly and the policy
# reads the rows there (obs_in_env_stride); off: the rows go to the game's
# packed observation buffer and the policy copies them.
STRIDED_POLICY_INPUT = True


class Rollout:
    """Batched MAPPO rollout (ppo.py:421-671; the side being trained is blue,
    or red with side="red", below): env e plays one rollout episode; all E envs
    advance together. Every step t (told for side="blue"):

      1. observe (ppo.py:497-575): `ship.get_obs()` of every live ship, blue
         then red, with its side effects (target lists, EW gauss draws) — one
         lnw_observe launch; rows of sunk ships are zeros (compiled_picture);
      2. the actor acts for every live blue ship (training-mode BatchNorm on a
         batch-1 call = per-row statistics, bn="sample"); red acts from the
         scripted profiles (untrained red, ppo.py:563-566) or the red actor in
         eval mode (ppo.py:569-572, red_bn="running"); sunk ships act
         np.zeros(4) (ppo.py:515, 574);
      3. the step runs on what `np.asarray(actions_for_step)` makes of those
         rows (ppo.py:577): a float32 array when every row is an actor output
         (all ships alive, red actor-driven), else float64 (a CSV row of Python
         floats or a np.zeros(4) row upcasts it) — per env, through a float64
         buffer with per-row value kinds (include/lnw.h);
      4. the critic scores the concatenated blue observations (ppo.py:598-605).

    impl="hip" (default) runs a step as four launches: lnw_observe, the fused
    policy kernel (lnw_policy_act: conv head, MLP, heads, keyed sample, log-
    probability, the action array with scripted red rows and row kinds, and
    the rollout rows; a second launch for a red actor), lnw_step, and
    lnw_rollout_post (critic, rewards, running / live flags). impl="torch" is
    the same rollout as batched torch ops (the features kernel + hipBLASLt
    GEMMs + ~45 small kernels per step), kept as the reference implementation
    the fused path is tested against.

    Rewards are kept in float64 (the reference's floats). With `stop_at_done`
    an env's steps after its first done == 0 are masked out (observations,
    actions, log-probabilities, values and rewards zero, `running` False), as
    the reference `break`s and leaves its buffers at zero.

    Differences from the reference loop, by design:
      * it observes the env it steps; ppo.py:497 calls get_obs on self.env, a
        Game that rollout() never steps (a reference bug);
      * exploration: `noise` adds a fixed N(0, noise) term like MLP.forward's
        `noise` argument; parameter noise is below; the noise ratio's schedule
        and its in-rollout adaptation (ppo.py:586-596) stay with the caller;
      * a noised actor whose heads are NaN for a row acts N(0, 1) for that row
        (lnw_policy_act's guard); the reference reloads the noiseless actor for
        the rest of the episode (ppo.py:505-507);
      * sunk ships' action rows are stored as zeros (the reference stores the
        previous ship's `action` variable there, ppo.py:516-517).

    Sampling: keyed draws (keyed_normal: Philox keyed by the seed, the global
    row, the rollout index and the step), so a rollout sharded over ranks by
    env_id_base samples exactly what one rank over all envs samples. The
    rollout index lives in a device counter (`call_index`) that every rollout
    advances — inside a captured graph too, so each replay draws fresh values.
    The hip impl always samples this way (seed `keyed_seed`, else `seed`); the
    torch impl does when `keyed_seed` is given, else it draws from the torch
    `generator` passed to run().

    `observe="step"` reuses the step's own output rows instead of a fresh
    observe (one launch less per step, but not the reference's draw order).
    `run(forced_actions=...)` replays given actor outputs [E, T, A, 4] instead of
    sampling (log-probabilities from get_dist): parity against recorded
    reference rollouts (tests/golden/make_rollout_golden.py).

    Parameter noise (ppo.py:452-482, the reference's default exploration): a
    population of noised actors inside one rollout. `envs_per_member=G` splits
    the global envs into members of G consecutive envs (member m = global envs
    [m G, (m + 1) G), so game.env_id_base must be a multiple of G); each member
    acts for the whole rollout with its own copy of the blue actor, theta_m =
    theta + mask * clamp(std * z_m, -clip, +clip) (perturbed_theta, noise_mask).
    G = 1 is the reference: one noised actor per episode. The log-probabilities
    returned are the noised actor's, the critic and the red actor are not noised.
      * `param_noise=(std, clip)` creates `self.param_noise`, a float32 [2]
        device tensor read on the device at every run: rewrite it in place
        between runs and graph replays (std 0: no noise). Every run / replay
        draws fresh noise (keyed by the seed, `call_index` and the global member).
      * `theta`: the blue actor as a flat device vector in the learner's layout
        (PPOLearner.theta_actor), read at run time, not copied: the rollout acts
        from the learner's current weights with no export() and no repack by
        torch ops. None: packed from the module, as without these arguments.
      * `member_thetas` [M, P]: explicit per-member vectors (M >= the game's
        members), no draws: parity against recorded reference actors.
    The hip impl runs lnw_actor_perturb once per run (inside a captured graph
    too) and every blue policy launch through lnw_policy_act_pop; the returned
    buffers hold "member" [E] int64, the global member of each env. With none
    of these arguments the rollout issues exactly the launches it did.

    Red-side training (ppo.py's rollout with SIDE == "red"): `side="red"` on a
    game whose scenario plays red (game.sc.side: the step's rewards and
    engagement rules follow it) collects the red side instead. `red_actor` is
    the learning actor, `actor` the frozen blue one (both required; red="script"
    is refused), `critic` the red critic BatchedCritic(Dr * nr). The buffers are
    the red rows' ([E, T, nr, Dr], [E, T, nr, 4], rewards from rew_red,
    reference_rtg over nr); `param_noise`, `envs_per_member`, `theta` and
    `member_thetas` apply to the red actor (the flat layout for Dr). Blue acts
    with running BatchNorm statistics and stores nothing (ppo.py:519-526).
      * `warmup` (default 15, the reference's `s > 14`; 0 <= warmup <= steps; only
        with side="red"): for t < warmup red takes its scripted profiles
        (ppo.py:552-557; lnw_policy_act's script_self) and the step's rows are
        float64; from t >= warmup red is sampled from the red actor, and the
        rows are float32 when every ship is alive. The returned buffers hold
        "sampled" [E, T] bool, True where the rows came from the actor (t >=
        warmup and the episode running): a caller can leave the scripted rows
        out of a minibatch with it.
      * `bn` / `red_bn` None (the default) resolve to "sample" for the learning
        side's actor and "running" for the other's; explicit strings keep their
        meaning by colour.
      * keyed draws: the blue sample is slot `which` 0 (rows env_id_base * nb),
        the red sample 2 (rows env_id_base * nr), the learning red actor's
        action noise 3. lnw_actor_perturb uses slot 3 of step 0, so side="red"
        with `noise`, `param_noise` and warmup == 0 together is refused.
      * `forced_actions` [E, T, A, 4] replays both sides; in the warm-up the red
        rows come from the profiles.
    Differences from the reference's red-side loop, by design, all in the
    warm-up: the observation rows and the scripted actions are stored (the
    reference stores zeros); the log-probabilities are the red actor's (the
    reference stores the blue actor's get_dist of the red rows); the value is
    taken on the real rows (the reference's critic sees zeros). A red ship sunk
    after the warm-up stores zero rows, as a sunk blue ship does (the reference
    raises there, ppo.py:547). Pinned to recordings of the reference's loop
    (tests/golden/make_redside_golden.py), which runs only 3v3 and only while
    no red ship is lost after step 14.
    """

    def __init__(self, game: BatchedGame, actor=None, critic=None, steps=40, red=None,
                 red_actor=None, noise=None, bn=None, red_bn=None, gamma=0.99,
                 stop_at_done=True, observe="fresh", keyed_seed=None, impl="hip", seed=0,
                 param_noise=None, envs_per_member=None, theta=None, member_thetas=None,
                 side="blue", warmup=None):
        if observe not in ("fresh", "step"):
            raise ValueError("observe must be 'fresh' or 'step'")
        _abi.check_impl(impl)
        if side not in ("blue", "red"):
            raise ValueError("side must be 'blue' or 'red'")
        if red is None:  # blue trains against the scripted profiles, red against the blue actor
            red = "script" if side == "blue" else "actor"
        if side == "blue":
            if warmup is not None:
                raise ValueError("warmup needs side='red'")
            warmup = 0
        else:
            if game.sc.side != side:
                raise ValueError(f"the game's scenario plays side {game.sc.side!r}: the step's rewards and "
                                 "engagement rules follow it, so Rollout(side='red') needs Scenario(side='red')")
            if red == "script":
                raise ValueError("side='red' trains the red actor: red='script' is refused")
            if red_actor is None:
                raise ValueError("side='red' needs red_actor, the learning actor")
            if actor is None:
                raise ValueError("side='red' needs actor, the frozen blue actor")
            if warmup is None:
                warmup = min(15, int(steps))  # the reference's `s > 14` (ppo.py:552)
            if int(warmup) != warmup or not 0 <= warmup <= int(steps):
                raise ValueError("warmup must be an integer in [0, steps]")
            if noise is not None and param_noise is not None and warmup == 0:
                raise ValueError("side='red' with noise, param_noise and warmup == 0: the action noise of "
                                 "step 0 and lnw_actor_perturb would share keyed slot 3")
        if envs_per_member is None:
            if param_noise is not None or member_thetas is not None:
                raise ValueError("envs_per_member is required with param_noise or member_thetas")
        else:
            if param_noise is None and member_thetas is None:
                raise ValueError("envs_per_member needs param_noise or member_thetas")
            if int(envs_per_member) != envs_per_member or envs_per_member <= 0:
                raise ValueError("envs_per_member must be a positive integer")
            if game.env_id_base % int(envs_per_member):
                raise ValueError("game.env_id_base must be a multiple of envs_per_member")
        if member_thetas is not None and (param_noise is not None or theta is not None):
            raise ValueError("member_thetas excludes param_noise and theta")
        if param_noise is not None:
            if len(param_noise) != 2 or not (param_noise[0] >= 0 and param_noise[1] >= 0):
                raise ValueError("param_noise must be (std >= 0, clip >= 0)")
        self.G = int(envs_per_member) if envs_per_member is not None else None
        self.theta, self.member_thetas = theta, member_thetas
        n_members = -(-game.E // self.G) if self.G else 1
        if member_thetas is not None and (member_thetas.dim() != 2 or member_thetas.shape[0] < n_members):
            raise ValueError(f"member_thetas must be [M >= {n_members}, P]")
        self.param_noise = None
        if param_noise is not None:
            self.param_noise = torch.tensor([float(param_noise[0]), float(param_noise[1])],
                                            dtype=torch.float32, device=game.device)
        self.keyed_seed, self.impl, self.seed = keyed_seed, impl, int(seed)
        self.g, self.actor, self.critic = game, actor, critic
        self.T, self.red, self.red_actor = int(steps), red, red_actor
        self.side, self.warmup = side, int(warmup)
        # BatchNorm modes: by default the learning side's actor runs in training
        # mode on batch-1 calls (per-row statistics), the other side's in eval mode
        self.bn = bn if bn is not None else ("sample" if side == "blue" else "running")
        self.red_bn = red_bn if red_bn is not None else ("running" if side == "blue" else "sample")
        self.noise = noise
        self.gamma, self.stop_at_done, self.observe = float(gamma), stop_at_done, observe
        self.table = red_script_table(game.device) if red == "script" or self.warmup > 0 else None
        # diagnostics / parity: keep each step's action array and row kinds as
        # the policy wrote them (before the step's in-place salvo write-back)
        # in the returned buffers ("step_actions" [E, T, A, 4] float64,
        # "step_kinds" [E, T, A])
        self.record_actions = False
        # rollout index of the keyed draws, on the device (advanced by run())
        self._call = torch.zeros(1, dtype=torch.int64, device=game.device)

    def call_index(self, value=None):
        """The device rollout counter the keyed draws are keyed by (read, or set
        to `value`)."""
        if value is not None:
            self._call.fill_(int(value))
        return int(self._call.item())

    def _learning(self):
        """The side being trained: (its actor, ships n, row length D, first agent
        slot, keyed-draw slot `which` of its sample, its BatchNorm mode)."""
        g = self.g
        if self.side == "red":
            return self.red_actor, g.nr, g.Dr, g.nb, 2, self.red_bn
        return self.actor, g.nb, g.Db, 0, 0, self.bn

    @torch.no_grad()
    def run(self, generator=None, forced_actions=None, on_step=None):
        """One rollout of T steps from the envs' current state. `on_step(t, out)`
        is called after step t's launch with the step outputs (device tensors),
        where ppo.py:620-638 does its per-step bookkeeping and logging; it must
        not be given while capturing a graph if it synchronises."""
        if self.impl == "hip":
            return self._run_hip(forced_actions, on_step)
        return self._run_torch(generator, forced_actions, on_step)

    def _buffers(self, fill=True):
        """The rollout's storage. fill=False (the HIP path): uninitialised, since
        every element is written each step — the observe writes every ship's row
        (a sunk ship's as zeros), the policy zeroes the rows, actions and
        log-probabilities of envs whose episode ended and writes each env's
        float32 flag, lnw_rollout_post writes every value, reward and running
        flag (masked ones as zeros) — so the 1.4 GB observation buffer of a
        32 768-env rollout is not zero-filled first (≈7 µs per step)."""
        g = self.g
        _, nb, D, _, _, _ = self._learning()  # (the learning side's ships and row length)
        E, T, dev = g.E, self.T, g.device
        z = torch.zeros if fill else torch.empty
        return dict(obs=z((E, T, nb, D), dtype=torch.float32, device=dev),
                    actions=z((E, T, nb, 4), dtype=torch.float32, device=dev),
                    log_probs=z((E, T, nb, 4), dtype=torch.float32, device=dev),
                    rewards=z((E, T, nb), dtype=torch.float64, device=dev),
                    values=z((E, T), dtype=torch.float32, device=dev),
                    running=(torch.ones if fill else torch.empty)((E, T), dtype=torch.bool, device=dev),
                    f32_step=z((E, T), dtype=torch.bool, device=dev))

    def _flat_source(self):
        """The flat actor vector(s) of this run on the game's device: the
        explicit member vectors [M, P], else `theta` [P] as it stands now, else
        the module's parameters packed into the flat layout."""
        dev = self.g.device
        actor = self._learning()[0]
        sl = actor_slices(actor.layernorm.normalized_shape[0])
        P = flat_size(sl)
        if self.member_thetas is not None:
            src = self.member_thetas.to(device=dev, dtype=torch.float32).contiguous()
        elif self.theta is not None:
            src = self.theta
            if src.dtype != torch.float32 or src.device != dev or not src.is_contiguous() or src.dim() != 1:
                raise ValueError("theta must be a contiguous float32 vector on the game's device")
        else:
            src = layout.pack(actor, sl).to(dev)
        if src.shape[-1] != P:
            raise ValueError(f"the flat actor vector holds {P} floats, not {src.shape[-1]}")
        return src

    def _member_actors(self, seed):
        """torch impl: None, or (G, the members' actors as modules) — scratch
        copies of the learning side's actor loaded from the members' flat vectors."""
        import copy
        if self.G is None and self.theta is None:
            return None
        g = self.g
        G = self.G if self.G else g.E
        M = -(-g.E // G)
        src = self._flat_source()
        if src.dim() == 1:
            std, clip = self.param_noise.tolist() if self.param_noise is not None else (0.0, 0.0)
            src = perturbed_theta(src, g.env_id_base // G, M, std, clip, seed, int(self._call.item()), self.T)
        actor = self._learning()[0]
        sl = actor_slices(actor.layernorm.normalized_shape[0])
        return G, [layout.unpack_(copy.deepcopy(actor), src[k], sl) for k in range(M)]

    def _run_hip(self, forced_actions, on_step):
        import ctypes as C
        from ._abi import F_ALIVE, PolicyArgs, RolloutPostArgs
        L = _abi.load()
        g = self.g
        E, nb, nr, A, Db, Dr, T = g.E, g.nb, g.nr, g.A, g.Db, g.Dr, self.T
        dev = g.device
        red_side = self.side == "red"
        # the learning side: its rows fill the buffers, its launch writes the kinds
        lactor, n, D, own0, which, lbn = self._learning()
        b = self._buffers(fill=False)
        obs, acts, logp, rew, val, running, f32s = (b[k] for k in ("obs", "actions", "log_probs", "rewards",
                                                                "values", "running", "f32_step"))
        full = torch.zeros((E, A, 4), dtype=torch.float64, device=dev)
        kinds = torch.full((E, A), _abi.LNW_KIND_F64, dtype=torch.uint8, device=dev)
        live = torch.ones(E, dtype=torch.bool, device=dev)
        # the other side's rows from an actor: a blue rollout's red actor, a red
        # rollout's frozen blue actor (its launch writes action rows only)
        other_rows = red_side or (self.red != "script" and self.red_actor is not None)
        seed = int(self.keyed_seed if self.keyed_seed is not None else self.seed) & (2**64 - 1)
        stream = _abi.stream(dev)
        pop = None
        if self.G is not None or self.theta is not None:
            # the members' packed sets [M, floats] from the flat vector(s), on the device
            src = self._flat_source()
            M = -(-E // self.G) if self.G else 1
            floats = int(L.lnw_policy_packed_floats(D))
            if floats <= 0:
                raise _abi.LnwError(f"the policy kernel does not support rows of {D} floats")
            ap = torch.empty((M, floats), dtype=torch.float32, device=dev)
            pt = _abi.ActorPerturbArgs()
            pt.theta, pt.theta_member_stride = src.data_ptr(), (src.shape[1] if src.dim() == 2 else 0)
            pt.D, pt.T = D, T
            pt.member0, pt.members = (g.env_id_base // self.G if self.G else 0), M
            pt.packed_out, pt.member_stride = ap.data_ptr(), floats
            pt.noise_dev = self.param_noise.data_ptr() if self.param_noise is not None else None
            pt.seed, pt.call_dev = seed, self._call.data_ptr()
            _abi.check(L.lnw_actor_perturb(C.byref(pt), stream))
            if self.G is not None:
                pop = _abi.PolicyPop(self.G, floats)
                b["member"] = torch.arange(E, dtype=torch.int64, device=dev) // self.G + pt.member0
        else:
            ap = lactor.packed_policy()
        cp = self.critic.packed(n, D) if self.critic is not None else None
        if cp is None:  # (no critic: nothing writes the values, which are zeros)
            val.zero_()
        if red_side:
            oactor, on, oD, oown0, owhich, obn, obuf, lbuf = self.actor, nb, Db, 0, 0, self.bn, g.obs_blue, g.obs_red
        else:
            oactor, on, oD, oown0, owhich, obn, obuf, lbuf = (self.red_actor, nr, Dr, nb, 2, self.red_bn,
                                                             g.obs_red, g.obs_blue)
        oap = oactor.packed_policy() if other_rows else None
        fa = None
        if forced_actions is not None:
            fa = forced_actions.to(device=dev, dtype=torch.float32).contiguous()
            assert fa.shape == (E, T, A, 4)
        alive_p, _ = g._field(F_ALIVE)
        if self.record_actions:
            b["step_actions"] = torch.zeros((E, T, A, 4), dtype=torch.float64, device=dev)
            b["step_kinds"] = torch.zeros((E, T, A), dtype=torch.uint8, device=dev)
        P = lambda t_: t_.data_ptr()  # noqa: E731
        f4, f8 = 4, 8
        table = self.table.contiguous() if self.table is not None else None
        rew_side = g.rew_red if red_side else g.rew_blue
        rew_f64 = int(rew_side.dtype == torch.float64)
        # fresh observations with no per-step callback: the learning side's rows go
        # straight into the rollout buffer (lnw_observe_ex; the policy zeroes ended
        # envs' rows in place), the other side's only where an actor reads them,
        # and the step writes none (ppo.py:577 discards them). The game's packed
        # buffer of the learning side (g.obs_blue, or g.obs_red) is not updated then.
        direct = self.observe == "fresh" and on_step is None
        # (STRIDED_POLICY_INPUT: the policy reads the rows in the buffer itself)
        strided = direct and STRIDED_POLICY_INPUT
        if self.observe == "step":
            g.observe(-1)
        for t in range(T):
            row_t = P(obs) + t * n * D * f4  # the rollout buffer's rows of step t
            if direct:
                lrows, lstride = (row_t, T * n * D) if strided else (P(lbuf), 0)
                orows = P(obuf) if other_rows else None
                if red_side:
                    g.observe_into(-1, orows, 0, lrows, lstride)
                else:
                    g.observe_into(-1, lrows, lstride, orows, 0)
            elif self.observe == "fresh":
                g.observe(-1)
            scripted = t < self.warmup  # the learning side's warm-up (side red): its own rows scripted
            pa = PolicyArgs()
            pa.obs, pa.E, pa.n, pa.D, pa.own0, pa.A = (row_t if strided else P(lbuf)), E, n, D, own0, A
            pa.obs_in_env_stride = T * n * D if strided else 0
            pa.params, pa.bn_running = P(ap), int(lbn == "running")
            if scripted:
                pa.script_self = 1
                pa.script, pa.script_n, pa.script_steps = P(table), table.shape[0], table.shape[1]
            elif fa is not None:
                pa.forced, pa.forced_act, pa.fa_env_stride = 1, P(fa) + (t * A + own0) * 4 * f4, T * A * 4
            pa.noise = float(self.noise) if self.noise is not None else 0.0
            pa.seed, pa.call_dev, pa.T, pa.t, pa.which = seed, P(self._call), T, t, which
            pa.row_base = g.env_id_base * n
            pa.alive = alive_p
            pa.live = P(live) if self.stop_at_done else None
            pa.obs_out, pa.obs_env_stride = row_t, T * n * D
            pa.act_out, pa.logp_out = P(acts) + t * n * 4 * f4, P(logp) + t * n * 4 * f4
            pa.act_env_stride = T * n * 4
            pa.full = P(full)
            if self.red == "script":  # (side blue) the lane of ship 0 writes red's scripted rows
                pa.script, pa.script_n, pa.script_steps = P(table), table.shape[0], table.shape[1]
                pa.script_own0, pa.script_cnt = nb, nr
            pa.kinds, pa.kinds_f32_all_alive = P(kinds), int(other_rows and not scripted)
            pa.f32_out, pa.f32_env_stride = P(f32s) + t, T
            if pop is not None:
                _abi.check(L.lnw_policy_act_pop(C.byref(pa), C.byref(pop), stream))
            else:
                _abi.check(L.lnw_policy_act(C.byref(pa), stream))
            if other_rows:
                ra = PolicyArgs()
                ra.obs, ra.E, ra.n, ra.D, ra.own0, ra.A = P(obuf), E, on, oD, oown0, A
                ra.params, ra.bn_running = P(oap), int(obn == "running")
                if fa is not None:
                    ra.forced, ra.forced_act, ra.fa_env_stride = 1, P(fa) + (t * A + oown0) * 4 * f4, T * A * 4
                ra.seed, ra.call_dev, ra.T, ra.t, ra.which = seed, P(self._call), T, t, owhich
                ra.row_base, ra.alive, ra.full = g.env_id_base * on, alive_p, P(full)
                _abi.check(L.lnw_policy_act(C.byref(ra), stream))
            if self.record_actions:
                b["step_actions"][:, t] = full
                b["step_kinds"][:, t] = kinds
            out = g.step(full, kinds, obs=not direct)
            pp = RolloutPostArgs()
            pp.obs, pp.obs_env_stride, pp.E, pp.n, pp.D = pa.obs_out, T * n * D, E, n, D
            if cp is not None:
                pp.critic, pp.val, pp.val_env_stride = P(cp), P(val) + t * f4, T
            pp.rew, pp.rew_f64, pp.n_rew = P(rew_side), rew_f64, n
            pp.rew_out, pp.rew_env_stride = P(rew) + t * n * f8, T * n
            pp.done, pp.live = P(out["done"]), P(live)
            pp.running, pp.running_env_stride = P(running) + t, T
            pp.stop_at_done = int(bool(self.stop_at_done))
            _abi.check(L.lnw_rollout_post(C.byref(pp), stream))
            if on_step is not None:
                on_step(t, out)
        self._call += 1
        rtg = reference_rtg(rew, self.gamma)
        b["rtg"] = rtg
        if red_side:
            b["sampled"] = running & (torch.arange(T, device=dev) >= self.warmup)[None]
        return b

    def _run_torch(self, generator, forced_actions, on_step):
        from ._abi import F_ALIVE, LNW_KIND_F32, LNW_KIND_F64
        g = self.g
        E, nb, nr, A = g.E, g.nb, g.nr, g.A
        dev = g.device
        T = self.T
        red_side = self.side == "red"
        # the learning side: its ships n, row length D, agent slots [own0, own0 + n)
        _, n, D, own0, which, lbn = self._learning()
        b = self._buffers()
        obs, acts, logp, rew, val, running, f32_step = (b[k] for k in (
            "obs", "actions", "log_probs", "rewards", "values", "running", "f32_step"))
        full = torch.zeros((E, A, 4), dtype=torch.float64, device=dev)
        other_rows = red_side or (self.red != "script" and self.red_actor is not None)
        if self.observe == "step":
            g.observe(-1)
        live = torch.ones(E, dtype=torch.bool, device=dev)
        base = g.env_id_base
        call = self._call  # device counter; keyed draws read it on the host here

        def draws(t, which, n_side):
            """keyed draws for this step: which 0/1 blue sample / noise, 2/3 red"""
            if self.keyed_seed is None:
                return None
            slot = ((int(call.item()) * T + t) * 4 + which)
            return keyed_normal(base * n_side, E * n_side, 4, self.keyed_seed, slot, dev)

        # the learning actor of every row: the module, or each member's own copy
        # for the member's rows (a population / a flat `theta`)
        members = self._member_actors(int(self.keyed_seed if self.keyed_seed is not None else self.seed))

        def learner(fn, *rows):
            """fn(actor, *rows) -> tuple of [rows, ...] tensors, over the members"""
            if members is None:
                return fn(self._learning()[0], *rows)
            Gm, nets = members
            parts = [fn(net, *[None if x is None else x[k * Gm * n:(k + 1) * Gm * n] for x in rows])
                     for k, net in enumerate(nets)]
            return tuple(torch.cat(c) for c in zip(*parts))

        if self.G is not None:
            b["member"] = torch.arange(E, dtype=torch.int64, device=dev) // self.G + base // self.G
        if self.record_actions:
            b["step_actions"] = torch.zeros((E, T, A, 4), dtype=torch.float64, device=dev)
            b["step_kinds"] = torch.zeros((E, T, A), dtype=torch.uint8, device=dev)
        zero = torch.zeros((), device=dev)
        for t in range(T):
            if self.observe == "fresh":
                g.observe(-1)
            cur, cur_other = (g.obs_red, g.obs_blue) if red_side else (g.obs_blue, g.obs_red)
            alive = g.get(F_ALIVE).t().bool()  # [E, A], slots not None
            al = alive[:, own0:own0 + n, None]
            # rows an env fills after its episode ended stay zero, as the
            # reference's buffers do after its `break` (ppo.py:640-641)
            keep = al & live[:, None, None] if self.stop_at_done else al
            obs[:, t] = torch.where(live[:, None, None], cur, zero) if self.stop_at_done else cur
            scripted = t < self.warmup  # (side red) the learning side's own rows from the profiles
            rows64 = None
            if scripted:
                rows64 = red_script_actions(self.table, t, n)  # [n, 4] float64
                a = rows64.to(torch.float32)[None].expand(E, n, 4)
                lp, _ = learner(lambda net, x, fa: net.get_dist(x, fa, bn=lbn),
                                cur.reshape(E * n, D), a.reshape(E * n, 4))
            elif forced_actions is not None:
                a = forced_actions[:, t, own0:own0 + n].to(torch.float32)
                lp, _ = learner(lambda net, x, fa: net.get_dist(x, fa, bn=lbn),
                                cur.reshape(E * n, D), a.reshape(E * n, 4))
            else:
                a, lp, _ = learner(lambda net, x, eps, neps: net(x, noise=self.noise, bn=lbn, generator=generator,
                                                                 eps=eps, noise_eps=neps),
                                   cur.reshape(E * n, D), draws(t, which, n),
                                   draws(t, which + 1, n) if self.noise is not None else None)
            a = torch.where(al, a.reshape(E, n, 4), zero)
            acts[:, t] = torch.where(keep, a, zero)
            logp[:, t] = torch.where(keep, lp.reshape(E, n, 4), zero)
            # the step takes the profiles' float64 rows themselves, not the rounded ones
            full[:, own0:own0 + n] = a if rows64 is None else torch.where(
                al, rows64, torch.zeros((), dtype=torch.float64, device=dev))
            if red_side:  # the frozen blue actor
                ab = alive[:, :nb, None]
                if forced_actions is not None:
                    ba = forced_actions[:, t, :nb].to(torch.float32)
                else:
                    ba, _, _ = self.actor(cur_other.reshape(E * nb, g.Db), bn=self.bn,
                                          generator=generator, eps=draws(t, 0, nb))
                full[:, :nb] = torch.where(ab, ba.reshape(E, nb, 4), zero).double()
            else:
                ar = alive[:, nb:, None]
                if self.red == "script":
                    full[:, nb:] = torch.where(ar, red_script_actions(self.table, t, nr),
                                               torch.zeros((), dtype=torch.float64, device=dev))
                elif self.red_actor is not None:
                    if forced_actions is not None:
                        ra = forced_actions[:, t, nb:].to(torch.float32)
                    else:
                        ra, _, _ = self.red_actor(cur_other.reshape(E * nr, g.Dr), bn=self.red_bn,
                                                  generator=generator, eps=draws(t, 2, nr))
                    full[:, nb:] = torch.where(ar, ra.reshape(E, nr, 4), zero).double()
                else:
                    full[:, nb:] = 0
            # np.asarray(actions_for_step): float32 only if every row is float32
            f32 = alive.all(1) if other_rows and not scripted else torch.zeros(E, dtype=torch.bool, device=dev)
            f32_step[:, t] = f32
            kinds = torch.where(f32, LNW_KIND_F32, LNW_KIND_F64).to(torch.uint8)[:, None]
            if self.critic is not None:
                v = self.critic(cur.reshape(E, n * D)).reshape(E)
                val[:, t] = torch.where(live, v, zero) if self.stop_at_done else v
            if self.record_actions:
                b["step_actions"][:, t] = full
                b["step_kinds"][:, t] = kinds
            out = g.step(full, kinds.expand(E, A).contiguous())
            running[:, t] = live
            r = out["rew_red" if red_side else "rew_blue"].to(torch.float64)
            rew[:, t] = torch.where(live[:, None], r, torch.zeros_like(r)) if self.stop_at_done else r
            if self.stop_at_done:
                live = live & (out["done"] != 0)
            if on_step is not None:
                on_step(t, out)
        self._call += 1
        # the learner's advantage is gae(rtg, values) on a sampled minibatch
        # (ppo.py:336), left to the caller as in the reference
        b["rtg"] = reference_rtg(rew, self.gamma)
        if red_side:
            b["sampled"] = running & (torch.arange(T, device=dev) >= self.warmup)[None]
        return b

    def capture(self, generator=None):
        """Record one whole rollout (T steps of actor, red, critic, step kernel,
        buffer writes and reward-to-go) as a HIP graph, so `replay()` launches
        its kernels without host work in between. One eager rollout runs first
        on a side stream (lazy initialisation, GEMM heuristics) and advances the
        envs; reset before replaying. The graph freezes the step launch's
        parameters (scenario, spawn spec) and the buffers it returns: `replay()`
        overwrites them in place. The rollout counter the keyed draws read is a
        device tensor the graph advances, so every replay draws fresh values;
        the torch impl with a `generator` registers it with the graph instead
        (torch's graph-safe generator offsets). The torch impl with
        `keyed_seed` cannot be captured (its keyed draws take the counter on the
        host) and refuses."""
        if self.impl == "torch" and self.keyed_seed is not None:
            raise RuntimeError("Rollout(impl='torch', keyed_seed=...) cannot be captured: its keyed "
                               "draws would be frozen at the capture's rollout index; use impl='hip'")
        dev = self.g.device
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self.run(generator)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        if generator is not None and self.impl == "torch":
            graph.register_generator_state(generator)
        with torch.cuda.graph(graph):
            out = self.run(generator)
        self._graph, self._graph_out = graph, out
        return out

    def replay(self):
        """One rollout from the envs' current state through the captured graph."""
        self._graph.replay()
        return self._graph_out
