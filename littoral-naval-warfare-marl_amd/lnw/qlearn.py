"""On-device DDQN acting around the batched step (DISCRETE mode): the
reference's Q-network evaluated for every (env, ship) at once, epsilon-greedy
and untrained-red random actions from keyed Philox draws, and a transition
collector that fills a device replay ring. Observations never leave the GPU.

Reference: network.py:246-305 (DMLP), ddqn.py:149-151 (get_epsilon),
ddqn.py:286-387 (acting), ddqn.py:175-193 (the TD target of optimize()).
The optimiser step and replay prioritisation stay with the caller.
"""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .batched import BatchedGame
from .rollout import WINDOW

N_RADAR, N_ATTACK, N_MOVE = 2, 5, 50          # DMLP's heads (network.py:261-263)
N_Q = N_RADAR + N_ATTACK + N_MOVE             # 57, in radar, attack, movement order
HEADS = ((0, N_RADAR), (N_RADAR, N_RADAR + N_ATTACK), (N_RADAR + N_ATTACK, N_Q))
CONV_PARAMS = 578                             # the conv head's packed floats (csrc/lnw_convhead.inc)


def epsilon(t, start, end, decay):
    """ddqn.py:149-151 `get_epsilon`: end + (start - end) * exp(-t / decay)."""
    return end + (start - end) * math.exp(-1. * t / decay)


def keyed_uniform4(row0, rows, seed, slot, device):
    """The four keyed uniforms [rows, 4] of global rows row0 .. row0+rows-1 that
    lnw_qnet_act draws: Philox (lnw_fill_uniform_f32) at absolute offset
    slot * 2^40 + 4 * row — keyed_normal's convention (lnw/rollout.py), so a
    shard of the envs draws what one call over all envs draws for them."""
    from . import _abi
    L = _abi.load()
    u = torch.empty((rows, 4), dtype=torch.float32, device=device)
    if rows:
        _abi.check(L.lnw_fill_uniform_f32(u.data_ptr(), rows * 4, int(seed) & (2**64 - 1),
                                          (int(slot) << 40) + 4 * int(row0),
                                          torch.cuda.current_stream(device).cuda_stream))
    return u


def random_rows(u):
    """The random rows [B, 3] of ddqn.py:300 from uniforms u [B, 4] (u0 decides
    whether a row explores, u0 < eps): [(int)(u1*2), (int)(u2*5), (int)(u3*50)],
    float32 multiply then truncate."""
    return torch.stack([(u[:, 1] * 2.0).to(torch.int32), (u[:, 2] * 5.0).to(torch.int32),
                        (u[:, 3] * 50.0).to(torch.int32)], 1)


def red_random_rows(u, t, red_aggression, tl_cnt):
    """Untrained red's rows (ddqn.py:316-328) from uniforms u [B, 4]; tl_cnt [B]
    target-list lengths; t the episode step."""
    rad = (u[:, 0] * 2.0).to(torch.int32)
    if t < 20:
        return torch.stack([rad, (u[:, 1] * 2.0).to(torch.int32), 2 + (u[:, 2] * 3.0).to(torch.int32)], 1)
    fire = (u[:, 1] < torch.tensor(red_aggression, dtype=torch.float32, device=u.device)) & (tl_cnt > 0)
    msl = torch.where(fire, 1 + (u[:, 2] * 4.0).to(torch.int32), torch.zeros_like(rad))
    return torch.stack([rad, msl, (u[:, 3] * 50.0).to(torch.int32)], 1)


class BatchedQNet(nn.Module):
    """network.py:246-305 `DMLP` for a [B, D] batch of observations.

    Same submodules, parameter names and initialisation as the reference, so a
    reference `state_dict` loads as is (`load_reference`). The DDQN loop calls
    `target_net` one state at a time and never puts it in eval()
    (ddqn.py:303), i.e. with BatchNorm statistics of that single sample:
    `bn="sample"` reproduces that for every row, `bn="running"` is the eval-mode
    network, `bn="batch"` normalises with the statistics of the whole batch as
    optimize()'s train-mode calls do (ddqn.py:175, 185; torch ops only, and the
    mode to differentiate through). Running statistics are not updated.
    """

    def __init__(self, n_inputs):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 5, 3, 1, padding=1)
        self.norm1 = nn.BatchNorm2d(5)
        self.pool = nn.MaxPool2d(2, 2)
        self.conv2 = nn.Conv2d(5, 8, 3, 1, padding=1)
        self.norm2 = nn.BatchNorm2d(8)
        self.pool2 = nn.MaxPool2d(2, 2)
        self.convhead = nn.Linear(8, 12, bias=True)
        n_in = n_inputs - WINDOW + 12
        self.movement = nn.Linear(n_in, N_MOVE, bias=True)
        self.attack = nn.Linear(n_in, N_ATTACK, bias=True)
        self.radar = nn.Linear(n_in, N_RADAR, bias=True)
        for m in (self.convhead, self.movement, self.attack, self.radar):
            nn.init.xavier_uniform_(m.weight)
        self.obs_dim, self.n_in = int(n_inputs), int(n_in)

    @classmethod
    def for_obs(cls, obs_dim):
        """The reference sizing: DMLP(n_inputs = observation row length)."""
        return cls(obs_dim)

    def load_reference(self, state_dict):
        """Load a reference DMLP state_dict (tensors or arrays)."""
        own = self.state_dict()
        self.load_state_dict({k: torch.as_tensor(np.asarray(v)).reshape(own[k].shape)
                              for k, v in state_dict.items()})
        return self

    def packed(self):
        """Every parameter lnw_qnet_act reads (csrc/lnw_qnet.hip), in its order:
        the conv head in lnw_actor_features' order (578 floats), then W [57][n_in]
        with the rows in radar, attack, movement order, then b [57]."""
        parts = [self.conv1.weight, self.conv1.bias, self.norm1.weight, self.norm1.bias,
                 self.norm1.running_mean, self.norm1.running_var, self.conv2.weight,
                 self.conv2.bias, self.norm2.weight, self.norm2.bias, self.norm2.running_mean,
                 self.norm2.running_var, self.convhead.weight, self.convhead.bias,
                 self.radar.weight, self.attack.weight, self.movement.weight,
                 self.radar.bias, self.attack.bias, self.movement.bias]
        return torch.cat([p.detach().reshape(-1).float() for p in parts]).contiguous()

    @staticmethod
    def _bn(m, z, bn):
        if bn == "sample":
            return F.instance_norm(z, weight=m.weight, bias=m.bias, eps=m.eps)
        if bn == "batch":
            return F.batch_norm(z, None, None, m.weight, m.bias, True, 0.0, m.eps)
        if bn == "running":
            return F.batch_norm(z, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)
        raise ValueError("bn must be 'sample', 'running' or 'batch'")

    def q_torch(self, obs, bn="sample"):
        """DMLP.forward as torch ops (host or device): [B, 57] = [radar,
        attack, movement] after the ReLU."""
        B = obs.shape[0]
        z = obs[:, :WINDOW].reshape(B, 1, 7, 7)
        z = self.pool(F.relu(self._bn(self.norm1, self.conv1(z), bn)))
        z = self.pool2(F.relu(self._bn(self.norm2, self.conv2(z), bn)))
        x = torch.cat((self.convhead(torch.flatten(z, 1)), obs[:, WINDOW:]), 1)
        return torch.cat((F.relu(self.radar(x)), F.relu(self.attack(x)), F.relu(self.movement(x))), 1)

    def q(self, obs, bn="sample"):
        """The ReLU'd Q-values [B, 57] of obs [B, D]: the HIP kernel
        (lnw_qnet_act's q_out) for device tensors, torch ops for host tensors
        and for bn="batch"."""
        if not obs.is_cuda or bn == "batch":
            return self.q_torch(obs, bn)
        if bn not in ("sample", "running"):
            raise ValueError("bn must be 'sample', 'running' or 'batch'")
        B = obs.shape[0]
        alive = torch.ones(B, dtype=torch.uint8, device=obs.device)
        return self._launch(obs.reshape(B, 1, -1), alive, 0, 1, bn=bn, want_q=True, want_act=False)["q"]

    def _launch(self, obs, alive, own0, A, eps=0.0, eps_env=None, live=None, seed=0, slot=0,
                row_base=0, bn="sample", full=None, act_out=None, act_env_stride=0,
                obs_in_env_stride=0, want_q=False, want_act=True, want_explored=False, params=None):
        """One lnw_qnet_act launch (EPS_GREEDY) for this side's rows: obs a
        tensor [E, n, D], or (device pointer, (E, n, D), device) for rows in
        caller memory (env e at pointer + e * obs_in_env_stride floats); alive:
        [A][E] uint8 tensor or a device pointer."""
        from . import _abi
        L = _abi.load()
        if torch.is_tensor(obs):
            obs = obs.contiguous().float()
            obs_ptr, (E, n, D), dev = obs.data_ptr(), obs.shape, obs.device
        else:
            obs_ptr, (E, n, D), dev = obs
        a = _abi.QnetArgs()
        a.obs, a.E, a.n, a.D, a.own0, a.A = obs_ptr, E, n, D, own0, A
        a.obs_in_env_stride = int(obs_in_env_stride)
        params = self.packed() if params is None else params
        a.params, a.bn_running, a.mode = params.data_ptr(), int(bn == "running"), _abi.LNW_QNET_EPS_GREEDY
        if eps_env is not None:
            eps_env = eps_env.to(device=dev, dtype=torch.float32).contiguous()
            a.eps_env = eps_env.data_ptr()
        a.eps = float(eps)
        a.seed, a.slot, a.row_base = int(seed) & (2**64 - 1), int(slot), int(row_base)
        a.alive = alive.data_ptr() if torch.is_tensor(alive) else alive
        if live is not None:
            live = live.to(device=dev).contiguous()
            a.live = live.data_ptr()
        out = {}
        if want_act and full is None and act_out is None:
            out["actions"] = torch.empty((E, n, 4), dtype=torch.int32, device=dev)
            a.act_out, a.act_env_stride = out["actions"].data_ptr(), n * 4
        if full is not None:
            a.full = full.data_ptr() if torch.is_tensor(full) else full
        if act_out is not None:
            a.act_out, a.act_env_stride = act_out, int(act_env_stride)
        if want_q:
            out["q"] = torch.empty((E * n, N_Q), dtype=torch.float32, device=dev)
            a.q_out = out["q"].data_ptr()
        if want_explored:
            out["explored"] = torch.empty((E * n,), dtype=torch.uint8, device=dev)
            a.explored = out["explored"].data_ptr()
        _abi.check(L.lnw_qnet_act(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return out

    @torch.no_grad()
    def act(self, obs, eps=0.0, alive=None, live=None, seed=0, slot=0, row_base=0, bn="sample",
            impl="hip", want_q=False):
        """Epsilon-greedy actions (ddqn.py:294-312) for one side's rows obs
        [E, n, D] on the device: dict(actions [E, n, 4] int32 (column 3 zero),
        explored [E, n] bool, q [E*n, 57] if want_q). eps: a float, or a per-env
        tensor [E]. alive: [E, n] (rows of sunk ships act 0, 0, 0); live: [E].
        impl="hip": one lnw_qnet_act launch. impl="torch": the same as torch ops
        with the same keyed draws (keyed_uniform4) — the restatement the kernel's
        random branch is tested against; its greedy rows come from q_torch, so
        they may differ from the kernel's where two Q-values are within
        rounding."""
        E, n, D = obs.shape
        dev = obs.device
        eps_env = eps if torch.is_tensor(eps) else None
        al = torch.ones((E, n), dtype=torch.bool, device=dev) if alive is None else alive.to(dev).bool()
        if impl == "hip":
            o = self._launch(obs, al.t().contiguous().to(torch.uint8), 0, n, eps=0.0 if eps_env is not None else eps,
                             eps_env=eps_env, live=None if live is None else live.to(torch.uint8),
                             seed=seed, slot=slot, row_base=row_base, bn=bn, want_q=want_q, want_explored=True)
            o["explored"] = o["explored"].bool().reshape(E, n)
            return o
        if impl != "torch":
            raise ValueError("impl must be 'hip' or 'torch'")
        q = self.q_torch(obs.reshape(E * n, D).float(), bn)
        greedy = torch.stack([q[:, lo:hi].argmax(1) for lo, hi in HEADS], 1).to(torch.int32)
        u = keyed_uniform4(row_base, E * n, seed, slot, dev)
        e = (eps_env.to(dev).float()[:, None].expand(E, n).reshape(-1) if eps_env is not None
             else torch.tensor(float(eps), dtype=torch.float32, device=dev))
        explore = u[:, 0] < e
        rows = torch.where(explore[:, None], random_rows(u), greedy)
        keep = al.reshape(-1) if live is None else (al & live.to(dev).bool()[:, None]).reshape(-1)
        act = torch.zeros((E * n, 4), dtype=torch.int32, device=dev)
        act[:, :3] = torch.where(keep[:, None], rows, torch.zeros_like(rows))
        out = dict(actions=act.reshape(E, n, 4), explored=(explore & keep).reshape(E, n))
        if want_q:
            out["q"] = q
        return out

    @torch.no_grad()
    def td_target(self, next_obs, reward, done, gamma, bn="batch"):
        """ddqn.py:175-193: per-head max of this (target) network on next_obs
        [B, D], then gamma * max * done + reward -> [B, 3] float32 (done is 1
        while the episode runs, as lnw_step returns it)."""
        q = self.q(next_obs, bn)
        nxt = torch.stack([q[:, lo:hi].max(1).values for lo, hi in HEADS], 1)
        return (gamma * nxt * done.to(nxt.dtype)[:, None] + reward.to(nxt.dtype)[:, None]).float()


def red_random_act(game, full, t, seed, slot, live=None, act_out=None, act_env_stride=0, explored=None):
    """Untrained red's rows (ddqn.py:316-328) of every env, one lnw_qnet_act
    launch (LNW_QNET_RED_RANDOM) into `full` [E, A, 4] int32."""
    from . import _abi
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
    """

    def __init__(self, game: BatchedGame, blue_net, red="random", capacity=64, seed=0, side="blue",
                 bn="sample"):
        if not game.sc.discrete:
            raise ValueError("QCollector needs a DISCRETE BatchedGame (Scenario(discrete=True))")
        if side not in ("blue", "red"):
            raise ValueError("side must be 'blue' or 'red'")
        if not (red is None or red == "random" or isinstance(red, BatchedQNet)):
            raise ValueError("red must be 'random', a BatchedQNet or None")
        if side == "red" and not isinstance(red, BatchedQNet):
            raise ValueError("side='red' needs a red BatchedQNet")
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

    def refresh_params(self):
        """Re-pack the networks' parameters (after a learner update)."""
        self._bp = self.blue_net.packed()
        self._rp = self.red.packed() if isinstance(self.red, BatchedQNet) else None

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
