"""On-device DDQN around the batched step (DISCRETE mode), acting with the
reference's Q-network (BatchedQNet and q_forward, lnw/nets.py): the epsilon
schedule, untrained red's random actions from keyed Philox draws, and a
transition collector that fills a device replay ring. Observations never leave
the GPU.

Reference: ddqn.py:149-151 (get_epsilon), ddqn.py:286-387 (acting),
ddqn.py:153-247 (optimize(): QLearner, the TD loss, its gradient and the
clamped Adam step as HIP kernels, csrc/lnw_qlearn.hip).
QCollector.minibatch / minibatch_dist draw the replay minibatch on the device,
without replacement, uniformly or by priorities kept beside the ring
(lnw/replay.py, csrc/lnw_replay.hip).
"""
import ctypes as C
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _abi
from .batched import BatchedGame
from .keyed import keyed_uniform4  # noqa: F401
from .layout import CONV_PARAMS, N_ATTACK, N_MOVE, N_RADAR, PACKED_NAMES, WINDOW, packed_slices  # noqa: F401
from .nets import HEADS, N_Q, BatchedQNet, q_forward, random_rows  # noqa: F401

_flat_forward = q_forward  # (its name before lnw/nets.py)


def epsilon(t, start, end, decay):
    """ddqn.py:149-151 `get_epsilon`: end + (start - end) * exp(-t / decay)."""
    return end + (start - end) * math.exp(-1. * t / decay)


def red_random_rows(u, t, red_aggression, tl_cnt):
    """Untrained red's rows (ddqn.py:316-328) from uniforms u [B, 4]; tl_cnt [B]
    target-list lengths; t the episode step."""
    rad = (u[:, 0] * 2.0).to(torch.int32)
    if t < 20:
        return torch.stack([rad, (u[:, 1] * 2.0).to(torch.int32), 2 + (u[:, 2] * 3.0).to(torch.int32)], 1)
    fire = (u[:, 1] < torch.tensor(red_aggression, dtype=torch.float32, device=u.device)) & (tl_cnt > 0)
    msl = torch.where(fire, 1 + (u[:, 2] * 4.0).to(torch.int32), torch.zeros_like(rad))
    return torch.stack([rad, msl, (u[:, 3] * 50.0).to(torch.int32)], 1)


def red_random_act(game, full, t, seed, slot, live=None, act_out=None, act_env_stride=0, explored=None):
    """Untrained red's rows (ddqn.py:316-328) of every env, one lnw_qnet_act
    launch (LNW_QNET_RED_RANDOM) into `full` [E, A, 4] int32."""
    L = _abi.load()
    g = game
    a = _abi.QnetArgs()
    a.E, a.n, a.D, a.own0, a.A = g.E, g.nr, g.Dr, g.nb, g.A
    a.mode, a.t, a.red_aggression = _abi.LNW_QNET_RED_RANDOM, int(t), float(g.sc.red_aggression)
    a.seed, a.slot, a.row_base = int(seed) & (2**64 - 1), int(slot), g.env_id_base * g.nr
    a.tl_cnt, a.alive = g._field(_abi.F_TL_CNT)[0], g._field(_abi.F_ALIVE)[0]
    if live is not None:
        a.live = live.data_ptr()
    a.full = full.data_ptr() if full is not None else None
    if act_out is not None:
        a.act_out, a.act_env_stride = act_out, int(act_env_stride)
    if explored is not None:
        a.explored = explored.data_ptr()
    _abi.check(L.lnw_qnet_act(C.byref(a), g._stream()))


class QCollector:
    """On-device transition collector of the DDQN loop (ddqn.py:282-420) for a
    DISCRETE BatchedGame: every env advances together, and the learning side's
    transitions go into a ring of `capacity` steps on the device —

      state      [cap, E, n, D] float32   the rows get_obs returned (ddqn.py:296)
      action     [cap, E, n, 4] int32     what was passed to Game.step (sunk ships 0)
      reward     [cap, E, n]              Game.step's rewards of the side
      next_state [cap, E, n, D] float32   Game.step's observations (ddqn.py:387)
      done       [cap, E]      int32      1 while the episode runs (ddqn.py:282)

    Per step: lnw_observe_ex writes the side's rows straight into the ring slot
    (the other side's into the game's buffer, or nowhere when no network reads
    them); lnw_qnet_act acts for blue, then for red, into one [E, A, 4] int32
    array (the learning side's rows also into the ring); lnw_step; reward,
    next-state and done are copied with torch ops. Nothing synchronises with the
    host. With an `auto_reset` scenario it runs indefinitely.

    red: "random" — untrained red (ddqn.py:316-328; its `steps_done < 20` switch
    takes the collector's step count since the last `new_episode()`); a
    BatchedQNet — trained red acting greedily on its own rows (the reference
    feeds it the last blue ship's state, ddqn.py:331: a bug not reproduced);
    None — red rows stay zero. side="red" stores red's transitions instead
    (needs a red BatchedQNet, which then acts epsilon-greedily like blue,
    ddqn.py:343-384).

    Draws are keyed by (seed, step, side, global row): kernel slot 2 * step +
    (0 blue, 1 red), `step` advancing once per step(), so two collectors with
    equal seeds over equal games fill equal rings, however the envs are sharded.

    priority: None — the collector above and nothing more (minibatch() raises).
    "uniform" or "reward" — `priority`, a float32 [E, cap] device tensor beside
    the ring (env-major: local row e * cap + k for ring slot k, global row
    (env_id_base + e) * cap + k; NaN while the slot holds no transition), which
    one lnw_replay_mark launch per step() fills for the slot just written: 1.0,
    or the float32 sum over the ships of |reward|. minibatch() and
    minibatch_dist() draw from it with lnw_ppo_sample's keyed draw without
    replacement (weights |p| + 1e-5; equal priorities are uniform sampling
    without replacement, the reference's random.sample, ddqn.py:74-76). The
    tensor is public and is read at draw time: a caller may rewrite entries in
    place with any finite values, for example TD errors from QLearner.grad's
    `y` and `qs`. `draw` (int64 [1]) is the draw counter on the device,
    `sample_status` (int64 [1]) the last draw's count of non-finite priorities,
    E * (cap - filled) unless the caller planted some; sample_seed the default
    seed of the draws; impl "hip" (the kernels) or "torch" (lnw/replay.py's
    restatement, the same bits).
    """

    def __init__(self, game: BatchedGame, blue_net, red="random", capacity=64, seed=0, side="blue",
                 bn="sample", priority=None, sample_seed=0, impl="hip"):
        if not game.sc.discrete:
            raise ValueError("QCollector needs a DISCRETE BatchedGame (Scenario(discrete=True))")
        if side not in ("blue", "red"):
            raise ValueError("side must be 'blue' or 'red'")
        if not (red is None or red == "random" or isinstance(red, BatchedQNet)):
            raise ValueError("red must be 'random', a BatchedQNet or None")
        if side == "red" and not isinstance(red, BatchedQNet):
            raise ValueError("side='red' needs a red BatchedQNet")
        if priority not in (None, "uniform", "reward"):
            raise ValueError("priority must be None, 'uniform' or 'reward'")
        _abi.check_impl(impl)
        g = self.g = game
        self.blue_net, self.red, self.side, self.bn = blue_net, red, side, bn
        self.cap, self.seed = int(capacity), int(seed)
        self.n, self.D = (g.nb, g.Db) if side == "blue" else (g.nr, g.Dr)
        dev, E, cap = g.device, g.E, self.cap
        self.state = torch.zeros((cap, E, self.n, self.D), dtype=torch.float32, device=dev)
        self.next_state = torch.zeros_like(self.state)
        self.action = torch.zeros((cap, E, self.n, 4), dtype=torch.int32, device=dev)
        self.reward = torch.zeros((cap, E, self.n), dtype=g.rew_blue.dtype, device=dev)
        self.done = torch.ones((cap, E), dtype=torch.int32, device=dev)
        self.full = torch.zeros((E, g.A, 4), dtype=torch.int32, device=dev)
        self.steps = 0      # steps taken (slot of the keyed draws, ring position)
        self.t = 0          # episode step of untrained red's switch
        self._bp = self._rp = None
        self.priority_mode, self.sample_seed, self.impl = priority, int(sample_seed), impl
        self.priority = None
        if priority is not None:
            from . import replay
            self.priority = replay.new_priority(E, cap, dev)
            self.draw = torch.zeros(1, dtype=torch.int64, device=dev)
            self.sample_status = torch.zeros(1, dtype=torch.int64, device=dev)
            self._replay_buf = {}  # minibatch(), minibatch_dist(): the buffers per batch size

    def refresh_params(self, params=None):
        """Re-pack the networks' parameters (after a learner update). params: a
        flat device vector in packed() layout for the learning side's network
        (QLearner.target_params, what the reference acts with, ddqn.py:303): it
        is read in place at every step, so later updates need no repack."""
        self._bp = self.blue_net.packed()
        self._rp = self.red.packed() if isinstance(self.red, BatchedQNet) else None
        if params is not None:
            if self.side == "blue":
                self._bp = params
            else:
                self._rp = params

    def new_episode(self):
        """Restart untrained red's episode-step count (after a reset())."""
        self.t = 0

    @property
    def filled(self):
        return min(self.steps, self.cap)

    @torch.no_grad()
    def step(self, eps=0.0):
        """One step of every env; eps: a float or a per-env tensor [E]. Returns
        the ring slot written."""
        from ._abi import F_ALIVE
        g = self.g
        if self._bp is None:
            self.refresh_params()
        k = self.steps % self.cap
        f4 = 4
        blue_side = self.side == "blue"
        red_net = isinstance(self.red, BatchedQNet)
        slot_ptr = self.state.data_ptr() + k * g.E * self.n * self.D * f4
        if blue_side:
            g.observe_into(-1, slot_ptr, g.nb * g.Db, g.obs_red.data_ptr() if red_net else None, 0)
            bobs, robs = slot_ptr, g.obs_red.data_ptr()
        else:
            g.observe_into(-1, g.obs_blue.data_ptr(), 0, slot_ptr, g.nr * g.Dr)
            bobs, robs = g.obs_blue.data_ptr(), slot_ptr
        alive_p = g._field(F_ALIVE)[0]
        act_p = self.action.data_ptr() + k * g.E * self.n * 4 * 4
        eps_env = eps if torch.is_tensor(eps) else None
        eps_f = 0.0 if eps_env is not None else float(eps)
        slot = 2 * self.steps
        self.blue_net._launch((bobs, (g.E, g.nb, g.Db), g.device), alive_p, 0, g.A, eps=eps_f,
                              eps_env=eps_env, seed=self.seed, slot=slot, row_base=g.env_id_base * g.nb,
                              bn=self.bn, full=self.full, act_out=act_p if blue_side else None,
                              act_env_stride=self.n * 4, params=self._bp)
        if red_net:
            self.red._launch((robs, (g.E, g.nr, g.Dr), g.device), alive_p, g.nb, g.A,
                             eps=0.0 if blue_side else eps_f, eps_env=None if blue_side else eps_env,
                             seed=self.seed, slot=slot + 1, row_base=g.env_id_base * g.nr, bn=self.bn,
                             full=self.full, act_out=None if blue_side else act_p,
                             act_env_stride=self.n * 4, params=self._rp)
        elif self.red == "random":
            red_random_act(g, self.full, self.t, self.seed, slot + 1)
        out = g.step(self.full)
        self.reward[k].copy_(out["rew_blue"] if blue_side else out["rew_red"])
        self.next_state[k].copy_(out["obs_blue"] if blue_side else out["obs_red"])
        self.done[k].copy_(out["done"])
        if self.priority is not None:
            from . import replay
            replay.mark(self.priority, self.reward, k, self.priority_mode, self.impl)
        self.steps += 1
        self.t += 1
        return k

    def sample(self, batch, generator=None):
        """`batch` transitions drawn uniformly from the filled part of the ring:
        dict(state [B, n, D], action [B, n, 4], reward [B, n], next_state
        [B, n, D], done [B], index [B] = ring step * E + env). generator: a
        torch.Generator on the ring's device (or None)."""
        if self.filled == 0:
            raise RuntimeError("the ring is empty")
        dev, E = self.g.device, self.g.E
        idx = torch.randint(0, self.filled * E, (int(batch),), generator=generator, device=dev)
        flat = lambda t: t.reshape((self.cap * E,) + tuple(t.shape[2:]))  # noqa: E731
        return dict(state=flat(self.state)[idx], action=flat(self.action)[idx], reward=flat(self.reward)[idx],
                    next_state=flat(self.next_state)[idx], done=flat(self.done)[idx], index=idx)


    def ring(self):
        """The ring's tensors as lnw.replay takes them."""
        return dict(state=self.state, next_state=self.next_state, action=self.action, reward=self.reward,
                    done=self.done)

    def _replay_args(self, seed):
        if self.priority is None:
            raise RuntimeError("the collector keeps no priorities: QCollector(..., priority='uniform' or 'reward')")
        return (self.filled, self.sample_seed if seed is None else int(seed), self.draw, self.sample_status,
                self.g.env_id_base * self.cap)

    def minibatch(self, batch, seed=None, advance=True):
        """`batch` distinct transitions drawn by the priorities and packed on the
        device (lnw_ppo_sample, then lnw_replay_pack), as the row tensors
        QLearner.step() / grad() take: dict(state, next_state [B n, D], action
        [B n, 4] int32, reward [B n] in the ring's dtype, done [B n] int32 (the
        transition's, repeated per ship), key [B] float64, index [B] int64 in
        sample()'s convention ring step * E + env, global_row [B] int64), in
        ascending (key, global row) order. The draw is a pure function of (seed,
        draw counter, global row): bitwise reproducible, and independent of how
        the envs are sharded. seed: None for sample_seed. `draw` advances by one
        unless advance is False. 1 <= batch <= min(filled * E, 131072), else
        ValueError before anything runs: no empty slot is drawn.

        A chain of launches on the current stream with no host synchronisation
        (impl="hip"), capturable with QLearner.step in one torch.cuda.graph:
        every replay draws afresh, the counter living on the device, and reads
        the ring and the priorities as they are then. The row tensors are views
        of a buffer kept per batch size that the next call of that size
        overwrites; QLearner.rows() passes them through without a copy."""
        from . import replay
        filled, seed, draw, status, row_base = self._replay_args(seed)
        return replay.minibatch(self.ring(), self.priority, batch, filled, seed, draw, status, row_base,
                                bool(advance), self.impl, self._replay_buf)

    def minibatch_dist(self, batch, seed=None, advance=True, group=None):
        """minibatch() over the union of the ranks' collectors: every rank gets
        the minibatch that one collector over all envs would draw with
        minibatch(), bit for bit (the same dict without `index`, which has no
        meaning across rings). Every rank draws `batch` candidates from its own
        ring (batch <= its filled * E, else ValueError before any collective),
        one all-gather exchanges the candidate lists (lnw.ppodist.message),
        lnw_ppo_sample_merge merges them, lnw_replay_pack packs the slots this
        rank owns, and one int32 SUM all-reduce assembles the buffer. group: the
        process group (None: the default one; with none initialised, a world of
        one). On "nccl" (RCCL) nothing synchronises with the host; "gloo" stages
        through it. sample_status holds the count over all ranks.

        Preconditions, not checked: every rank has the same cap, steps,
        sample_seed (or seed) and `draw`, and the ranks' envs are disjoint ranges
        of the global envs (env_id_base)."""
        from . import replay
        filled, seed, draw, status, row_base = self._replay_args(seed)
        return replay.minibatch_dist(self.ring(), self.priority, batch, filled, seed, draw, status, row_base,
                                     bool(advance), group, self.impl, self._replay_buf)



class QLearner:
    """The learner half of the DDQN loop: ddqn.py:153-247 `optimize()` for one
    side, on flat device vectors in BatchedQNet.packed() layout.

    `theta` (`.params`) and `theta_target` (`.target_params`) hold the policy and
    target networks, `m`, `v` and a device step counter the Adam state. `target`
    None starts the target as a copy of the policy. policy_bn: "batch" — the
    policy forward and backward on batch statistics (the reference's blue side);
    "running" — on the running statistics (what the reference's red side does:
    ddqn.py:212 puts red_policy_net in eval() and ddqn.py:222 calls train() on
    the other network). The target network always runs on batch statistics, and
    every training-mode forward updates that network's running statistics.

    impl="hip": lnw_qnet_grad + lnw_qnet_adam (csrc/lnw_qlearn.hip), a chain of
    launches on the current stream with no host synchronisation; capturable in
    a torch.cuda.graph. impl="torch": the same steps with torch ops, autograd and
    torch.optim.Adam on the same flat state, on the host or the device — the arm
    the kernels are tested and timed against.

    batch: what QCollector.sample() returns ([B, n, ...] is flattened to rows and
    `done` repeated per ship), or a dict of row tensors state [B, D], action
    [B, >= 3], reward [B] (float32 or float64), next_state [B, D], done [B]."""

    def __init__(self, policy, target=None, lr=1e-4, gamma=0.99, betas=(0.9, 0.999), eps=1e-8, clamp=1.0,
                 policy_bn="batch", impl="hip", device=None):
        if policy_bn not in ("batch", "running"):
            raise ValueError("policy_bn must be 'batch' or 'running'")
        _abi.check_impl(impl)
        if device is None:
            device = "cuda" if impl == "hip" else next(policy.parameters()).device
        self.device = dev = torch.device(device)
        if impl == "hip" and dev.type != "cuda":
            raise ValueError("impl='hip' needs a GPU device")
        self.policy, self.target = policy, target
        self.lr, self.gamma, self.betas, self.eps, self.clamp = float(lr), float(gamma), tuple(betas), float(eps), float(clamp)
        self.policy_bn, self.impl = policy_bn, impl
        self.D, self.n_in = policy.obs_dim, policy.n_in
        self.slices = packed_slices(self.n_in)
        self.theta = policy.packed().to(dev)
        self.theta_target = (policy if target is None else target).packed().to(dev)
        self.m, self.v = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        self.step_count = torch.zeros(1, dtype=torch.int64, device=dev)
        # num_batches_tracked of [policy, target]
        src_t = policy if target is None else target
        self.nbt = torch.tensor([int(policy.norm1.num_batches_tracked), int(src_t.norm1.num_batches_tracked)],
                                dtype=torch.int64, device=dev)
        self._nbt_inc = torch.tensor([int(policy_bn == "batch"), 1], dtype=torch.int64, device=dev)
        self._grad = torch.zeros_like(self.theta)
        self._loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self._ws = None
        self._opt = None

    @property
    def params(self):
        return self.theta

    @property
    def target_params(self):
        return self.theta_target

    def rows(self, batch):
        """The batch as contiguous row tensors on the learner's device."""
        dev = self.device
        st, ns = batch["state"], batch["next_state"]
        ac, rw, dn = batch["action"], batch["reward"], batch["done"]
        if st.dim() == 3:
            n = st.shape[1]
            dn = dn[:, None].expand(dn.shape[0], n).reshape(-1)
            st, ns = st.reshape(-1, st.shape[-1]), ns.reshape(-1, ns.shape[-1])
            ac, rw = ac.reshape(-1, ac.shape[-1]), rw.reshape(-1)
        if rw.dtype != torch.float64:
            rw = rw.float()
        return dict(state=st.to(dev, torch.float32).contiguous(), next_state=ns.to(dev, torch.float32).contiguous(),
                    action=ac.to(dev, torch.int32).contiguous(), reward=rw.to(dev).contiguous(),
                    done=dn.to(dev, torch.int32).contiguous())

    # ---- HIP arm ---------------------------------------------------------------
    def _grad_hip(self, r, want, freeze):
        L = _abi.load()
        dev = self.device
        B, D = r["state"].shape
        need = L.lnw_qlearn_workspace_bytes(B, D)
        if need <= 0:
            raise _abi.LnwError(f"lnw_qnet_grad does not support rows={B}, D={D}")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        a = _abi.QlearnArgs()
        a.state, a.next_state, a.rows, a.D = r["state"].data_ptr(), r["next_state"].data_ptr(), B, D
        a.action, a.action_stride = r["action"].data_ptr(), r["action"].shape[1]
        a.reward, a.reward_f64 = r["reward"].data_ptr(), int(r["reward"].dtype == torch.float64)
        a.done = r["done"].data_ptr()
        a.policy_bn_running, a.freeze_running, a.gamma = int(self.policy_bn == "running"), int(freeze), self.gamma
        a.policy_params, a.target_params = self.theta.data_ptr(), self.theta_target.data_ptr()
        a.grad, a.loss = self._grad.data_ptr(), self._loss.data_ptr()
        out = {}
        if want:
            out["y"] = torch.empty((B, 3), dtype=torch.float32, device=dev)
            out["qs"] = torch.empty((B, 3), dtype=torch.float32, device=dev)
            out["stats"] = torch.empty((2, 2, 13), dtype=torch.float32, device=dev)
            a.y_out, a.qs_out, a.stats_out = out["y"].data_ptr(), out["qs"].data_ptr(), out["stats"].data_ptr()
        a.workspace, a.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        _abi.check(L.lnw_qnet_grad(C.byref(a), _abi.stream(dev)))
        return out

    def _adam_hip(self):
        L = _abi.load()
        _abi.check(L.lnw_qnet_adam(self.theta.data_ptr(), self._grad.data_ptr(), self.m.data_ptr(),
                                   self.v.data_ptr(), self.theta.numel(), self.step_count.data_ptr(),
                                   self.lr, self.betas[0], self.betas[1], self.eps, self.clamp,
                                   _abi.stream(self.device)))

    # ---- torch arm ---------------------------------------------------------------
    def _update_running(self, theta, stats, B):
        with torch.no_grad():
            for pre, lo, hi, n in (("norm1", 0, 5, 49 * B), ("norm2", 5, 13, 9 * B)):
                for name, val in ((pre + ".running_mean", stats[0, lo:hi]),
                                  (pre + ".running_var", stats[1, lo:hi] * (n / (n - 1.0)))):
                    k, shp = self.slices[name]
                    seg = theta[k:k + shp[0]]
                    seg.copy_(0.1 * val + 0.9 * seg)

    def _grad_torch(self, r, freeze):
        B = r["state"].shape[0]
        sl = self.slices
        with torch.no_grad():
            qt, st_t = q_forward(self.theta_target, r["next_state"], "batch", sl)
            nxt = torch.stack([qt[:, lo:hi].max(1).values for lo, hi in HEADS], 1)
            t = (self.gamma * nxt) * r["done"][:, None]
            y = (t + r["reward"][:, None]).float()  # (float64 rewards: the sum in float64, then float32)
        th = self.theta.detach().clone().requires_grad_(True)
        q, st_p = q_forward(th, r["state"], self.policy_bn, sl)
        act = r["action"].long()
        qs = torch.stack([q[:, lo:hi].gather(1, act[:, h:h + 1].clamp(0, hi - lo - 1))[:, 0]
                          for h, (lo, hi) in enumerate(HEADS)], 1)
        loss = F.mse_loss(qs, y)
        loss.backward()
        self._grad.copy_(th.grad)
        self._loss.copy_(loss.detach().reshape(1))
        if not freeze:
            self._update_running(self.theta_target, st_t, B)
            if self.policy_bn == "batch":
                self._update_running(self.theta, st_p, B)
        return dict(y=y, qs=qs.detach(), stats=torch.stack([st_p, st_t]))

    def _adam_torch(self):
        if self._opt is None:
            self._p = nn.Parameter(self.theta)  # (shares theta's storage)
            self._opt = torch.optim.Adam([self._p], lr=self.lr, betas=self.betas, eps=self.eps)
            st = self._opt.state[self._p]
            st["step"], st["exp_avg"], st["exp_avg_sq"] = torch.tensor(0.0), self.m, self.v
        g = self._grad.clone()
        if self.clamp > 0:
            g.clamp_(-self.clamp, self.clamp)
        self._p.grad = g
        self._opt.step()
        self.step_count += 1

    # ---- public ----------------------------------------------------------------
    def grad(self, batch, update_running=True):
        """Loss and gradient of one batch, without the optimiser step: dict(loss
        0-d, grad [P] unclamped in packed() layout, y [B, 3], qs [B, 3], stats
        [2 policy / target, 2 mean / biased variance, 13 channels]). The
        training-mode forwards update the running statistics (and the batch
        counters) as the reference's do, unless update_running is False."""
        r = self.rows(batch)
        if self.impl == "hip":
            out = self._grad_hip(r, True, not update_running)
        else:
            out = self._grad_torch(r, not update_running)
        if update_running:
            self.nbt += self._nbt_inc
        out["loss"], out["grad"] = self._loss.reshape(()).clone(), self._grad.clone()
        return out

    def step(self, batch):
        """One optimize(): gradient, clamp, Adam. Returns the loss, a 0-d device
        tensor (nothing synchronises with the host)."""
        r = self.rows(batch)
        if self.impl == "hip":
            self._grad_hip(r, False, False)
            self._adam_hip()
        else:
            self._grad_torch(r, False)
            self._adam_torch()
        self.nbt += self._nbt_inc
        return self._loss.reshape(()).clone()

    @torch.no_grad()
    def sync_target(self):
        """target.load_state_dict(policy.state_dict()) (ddqn.py:442): parameters,
        running statistics and the batch counter."""
        self.theta_target.copy_(self.theta)
        self.nbt[1:2] = self.nbt[0:1]

    @torch.no_grad()
    def export(self):
        """Write the vectors and num_batches_tracked back into the BatchedQNet
        modules (the target only if one was given); returns (policy, target)."""
        nbt = self.nbt.cpu()
        for net, flat, k in ((self.policy, self.theta, 0), (self.target, self.theta_target, 1)):
            if net is None:
                continue
            net.unpack_(flat.detach().cpu())
            for nm in (net.norm1, net.norm2):
                nm.num_batches_tracked.fill_(int(nbt[k]))
        return self.policy, self.target
