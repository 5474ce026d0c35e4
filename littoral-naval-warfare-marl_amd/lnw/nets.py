"""The reference's actor `MLP`, critic `Value` (network.py:38-172) and Q-network
`DMLP` (network.py:246-305), each forward pass stated once: as a function of a
parameter lookup p(name) -> tensor, `name` a state_dict key (trunk,
actor_features, actor_mlp, critic_value, q_heads; any dtype, any device). The
modules (BatchedActor, BatchedCritic, BatchedQNet: what acts in a rollout and
what a reference checkpoint loads into) look up their own attributes, the
flat-vector forms the learners' torch arms differentiate (actor_forward,
critic_forward, q_forward) the segments of lnw/layout.py's layouts, so the two
are one function. The modules' device paths (lnw_actor_features, lnw_qnet_act)
and the parameter formats the kernels read are here as well.
"""
import ctypes as C
from functools import partial
from operator import attrgetter

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.distributions import Normal

from . import _abi, layout
from .keyed import keyed_uniform4  # (BatchedQNet.act's torch arm draws what lnw_qnet_act draws)
from .layout import ACTOR_NAMES, CONV_PARAMS, N_ATTACK, N_MOVE, N_RADAR, WINDOW, actor_slices, flat_size, packed_slices

N_Q = N_RADAR + N_ATTACK + N_MOVE             # 57, in radar, attack, movement order
HEADS = ((0, N_RADAR), (N_RADAR, N_RADAR + N_ATTACK), (N_RADAR + N_ATTACK, N_Q))
EPS = 1e-5  # of both BatchNorms and the LayerNorm (torch's default, the reference's)
BN_MODES = "bn must be 'sample', 'running' or 'batch'"


def trunk(p, obs, bn):
    """The conv head of every row of obs [B, D] (network.py:74-87, 280-299)
    joined with the row's tail: ([B, 12 + D - 49], conv1's output, conv2's
    output: what the BatchNorms normalise, for a caller's statistics). bn:
    "sample", each row's own statistics (a training-mode call on one row);
    "batch", the whole batch's; "running", the running ones, as constants."""
    def norm(z, pre):
        w, b = p(pre + ".weight"), p(pre + ".bias")
        if bn == "sample":
            return F.instance_norm(z, weight=w, bias=b, eps=EPS)
        if bn == "batch":
            return F.batch_norm(z, None, None, w, b, True, 0.0, EPS)
        if bn == "running":
            mean, var = p(pre + ".running_mean").detach(), p(pre + ".running_var").detach()
            return F.batch_norm(z, mean, var, w, b, False, 0.0, EPS)
        raise ValueError(BN_MODES)

    z1 = F.conv2d(obs[:, :WINDOW].reshape(obs.shape[0], 1, 7, 7), p("conv1.weight"), p("conv1.bias"), padding=1)
    z = F.max_pool2d(F.relu(norm(z1, "norm1")), 2, 2)
    z2 = F.conv2d(z, p("conv2.weight"), p("conv2.bias"), padding=1)
    z = F.max_pool2d(F.relu(norm(z2, "norm2")), 2, 2)
    x = F.linear(torch.flatten(z, 1), p("convhead.weight"), p("convhead.bias"))
    return torch.cat((x, obs[:, WINDOW:]), 1), z1, z2


def actor_features(p, obs, bn):
    """network.py:74-89, the trunk and the LayerNorm (what lnw_actor_features
    computes): ([B, n_in], conv1's output, conv2's output)."""
    x, z1, z2 = trunk(p, obs, bn)
    return F.layer_norm(x, (x.shape[1],), p("layernorm.weight"), p("layernorm.bias"), EPS), z1, z2


def actor_mlp(p, x):
    """network.py:91-96 on the features [B, n_in]: (normal mean, normal std)."""
    for fc in ("fc1", "fc2", "fc3"):
        x = torch.tanh(F.linear(x, p(fc + ".weight"), p(fc + ".bias")))
    return torch.tanh(F.linear(x, p("normal_head.weight"))), torch.exp(F.linear(x, p("log_std_head.weight")))


def critic_value(p, x):
    """Value.forward (network.py:168-175) on global states [B, n D]: [B, 1]."""
    for fc in ("fc1", "fc2", "fc3"):
        x = torch.tanh(F.linear(x, p(fc + ".weight"), p(fc + ".bias")))
    return F.linear(x, p("fc4.weight"), p("fc4.bias"))


def q_heads(p, x):
    """network.py:301-305 on the trunk's output: [B, 57] = [radar, attack, movement] after the ReLU."""
    return torch.cat([F.relu(F.linear(x, p(h + ".weight"), p(h + ".bias"))) for h in ("radar", "attack", "movement")], 1)


def actor_forward(theta, obs, actions, sl):
    """MLP.get_dist (network.py:117-152) of every row with the row's own
    BatchNorm statistics, from a flat parameter vector (differentiable in
    theta): log-probabilities [B, 4], entropies [B, 4], and the rows'
    statistics [B, 26] (13 channel means, then their unbiased variances)."""
    p = partial(layout.seg, theta, sl)
    x, z1, z2 = actor_features(p, obs, "sample")
    with torch.no_grad():
        stats = torch.cat([z1.mean((2, 3)), z2.mean((2, 3)), z1.var((2, 3), unbiased=True),
                           z2.var((2, 3), unbiased=True)], 1)
    dist = Normal(*actor_mlp(p, x), validate_args=False)
    return dist.log_prob(actions), dist.entropy(), stats


def critic_forward(theta, gs, sl):
    """Value.forward (network.py:168-175) from a flat parameter vector: [B]."""
    return critic_value(partial(layout.seg, theta, sl), gs)[:, 0]


def q_forward(theta, obs, bn, sl):
    """DMLP.forward from a flat parameter vector (differentiable in theta):
    q [B, 57] after the ReLU, and the batch mean / biased variance of the 13
    BatchNorm channels [2, 13]. bn: "batch" or "running" (the running slots are
    constants then)."""
    p = partial(layout.seg, theta, sl)
    x, z1, z2 = trunk(p, obs, bn)
    with torch.no_grad():
        st = torch.stack([torch.cat([z1.mean((0, 2, 3)), z2.mean((0, 2, 3))]),
                          torch.cat([z1.var((0, 2, 3), unbiased=False), z2.var((0, 2, 3), unbiased=False)])])
    return q_heads(p, x), st


class _Net(nn.Module):
    def _p(self):
        """The forwards' lookup over this module's own attributes (built per
        call: a module that kept one would not deep-copy)."""
        return lambda name: attrgetter(name)(self)

    def load_reference(self, state_dict):
        """Load the reference network's state_dict (tensors or arrays)."""
        own = self.state_dict()
        sd = {k: torch.as_tensor(np.asarray(v)).reshape(own[k].shape) for k, v in state_dict.items()}
        if "logstd" in own:  # (the actor's unused parameter, which a checkpoint may lack)
            sd.setdefault("logstd", torch.zeros(()))
        self.load_state_dict(sd)
        return self


class _ConvNet(_Net):
    """The conv trunk's submodules, declared first and in the reference's order
    (network.py:39-47, 251-259): the draws of a seeded constructor and the
    state_dict's order are the reference's."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 5, 3, 1, padding=1)
        self.norm1 = nn.BatchNorm2d(5)
        self.pool = nn.MaxPool2d(2, 2)
        self.conv2 = nn.Conv2d(5, 8, 3, 1, padding=1)
        self.norm2 = nn.BatchNorm2d(8)
        self.pool2 = nn.MaxPool2d(2, 2)
        self.convhead = nn.Linear(8, 12, bias=True)


class BatchedActor(_ConvNet):
    """network.py:38-152 `MLP` for a [B, D] batch of observations.

    Same submodules, parameter names and initialisation as the reference, so a
    reference `state_dict` loads as is (`load_reference`). The reference is a
    batch-1 network: it flattens the conv head over the batch and concatenates
    along dim 0 (network.py:83), and the PPO rollout calls it one state at a time
    with BatchNorm in training mode (ppo.py:504-512), i.e. with statistics of that
    single sample. `bn="sample"` reproduces exactly that for every row (instance
    statistics with the BatchNorm affine parameters); `bn="running"` is the
    eval-mode network (running statistics). Any other mode is a ValueError
    ("batch" too: lnw_actor_features has no such mode). Running statistics are
    not updated.
    """

    def __init__(self, n_inputs, n_outputs):
        super().__init__()
        self.layernorm = nn.LayerNorm(n_inputs)
        self.fc1 = nn.Linear(n_inputs, 64, bias=True)
        self.fc2 = nn.Linear(64, 64, bias=True)
        self.fc3 = nn.Linear(64, 32, bias=True)
        self.normal_head = nn.Linear(32, n_outputs, bias=False)
        self.log_std_head = nn.Linear(32, n_outputs, bias=False)
        for m in (self.fc1, self.fc2, self.fc3, self.normal_head, self.log_std_head):
            nn.init.xavier_uniform_(m.weight)
        self.logstd = nn.Parameter(torch.zeros(()))  # present in the reference, unused there too

    @classmethod
    def for_obs(cls, obs_dim, n_outputs=4):
        """The reference sizing: n_inputs = obs_dim - 7*7 + 12 (ppo.py:78, 446)."""
        return cls(obs_dim - WINDOW + 12, n_outputs)

    def packed_features(self):
        """Parameters in lnw_actor_features' order (csrc/lnw_actor.hip): conv1
        w, b; norm1 w, b, running mean, var; conv2 w, b; norm2 w, b, running
        mean, var; convhead w, b; layernorm w, b (578 + 2 n_in floats)."""
        return layout.pack(self, ACTOR_NAMES[:16])

    def packed_policy(self):
        """Every parameter lnw_policy_act reads (csrc/lnw_actor.hip), in its order:
        packed_features() zero-padded to a multiple of 4 floats; the biases b1
        [64], b2 [64], b3 [32]; then the MFMA A-operand fragments of fc1 (n_in
        zero-padded to 32 columns, 64 when n_in > 32), fc2, fc3 and the heads
        (normal_head rows 0-3, log_std_head rows 4-7, zero rows to 16) for
        v_mfma_f32_16x16x32_bf16 with each weight split exactly into three
        bfloat16 terms (w = hi + mid + lo, round-to-nearest each): per layer three
        planes (hi, mid, lo) of bf16x8 [n-tile][k-pair p][lane], element j =
        W[16 nt + lane % 16][32 p + 16 (j // 4) + 4 (lane // 16) + j % 4] (the k
        order the kernel's chained layers sum in), stored as raw bits, two per
        float."""
        n_in = self.layernorm.normalized_shape[0]
        dev = self.fc1.weight.device

        def frags(w, k_pad, n_pad):
            wp = torch.zeros((n_pad, k_pad), dtype=torch.float32, device=dev)
            wp[:w.shape[0], :w.shape[1]] = w.detach().float()
            nt, qp = n_pad // 16, k_pad // 32
            # [nt][m][p][half][g][v] -> [nt][p][lane = 16 g + m][j = 4 half + v]
            x = wp.reshape(nt, 16, qp, 2, 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(nt, qp, 64, 8)
            hi = x.to(torch.bfloat16)
            r = x - hi.float()
            mid = r.to(torch.bfloat16)
            lo = (r - mid.float()).to(torch.bfloat16)
            return torch.stack([hi, mid, lo]).contiguous().reshape(-1).view(torch.float32)

        conv = self.packed_features()
        conv = torch.cat([conv, torch.zeros((-conv.numel()) % 4, device=dev)])
        k1 = 32 if n_in <= 32 else 64
        heads = torch.cat([self.normal_head.weight, self.log_std_head.weight], 0)
        parts = [conv, self.fc1.bias, self.fc2.bias, self.fc3.bias,
                 frags(self.fc1.weight, k1, 64), frags(self.fc2.weight, 64, 64),
                 frags(self.fc3.weight, 64, 32), frags(heads, 32, 16)]
        return torch.cat([p.detach().reshape(-1).float() for p in parts]).contiguous()

    def features(self, obs, bn="sample"):
        """network.py:70-85 up to the LayerNorm -> [B, n_in]: the HIP kernel
        for device tensors (lnw_actor_features), torch ops for host tensors."""
        if bn not in ("sample", "running"):
            raise ValueError(BN_MODES)
        if not obs.is_cuda:
            return actor_features(self._p(), obs, bn)[0]
        L = _abi.load()
        B = obs.shape[0]
        obs = obs.contiguous().float()
        n_in = self.layernorm.normalized_shape[0]
        out = torch.empty((B, n_in), dtype=torch.float32, device=obs.device)
        params = self.packed_features()
        _abi.check(L.lnw_actor_features(params.data_ptr(), obs.shape[1], obs.data_ptr(), B,
                                        int(bn == "running"), out.data_ptr(),
                                        _abi.stream(obs.device)))
        return out

    def heads(self, obs, bn="sample"):
        """(normal mean, normal std) for every row of obs [B, D]."""
        return actor_mlp(self._p(), self.features(obs, bn))

    def forward(self, obs, noise=None, bn="sample", generator=None, eps=None, noise_eps=None):
        """network.py:70-115 for every row: sample N(mean, std), add N(0, noise)
        exploration noise, clamp to [0, 1], log-probabilities of the clamped
        actions. Returns (actions, log_probs, ok) where ok marks rows without
        NaN heads (the reference returns (None, None) for those). `eps` /
        `noise_eps`: given standard-normal draws [B, n_outputs] instead of
        drawing from `generator` (keyed_normal: shard-invariant rollouts)."""
        mean, std = self.heads(obs, bn)
        ok = ~(torch.isnan(mean).any(1) | torch.isnan(std).any(1))
        mean_s = torch.where(ok[:, None], mean, torch.zeros_like(mean))
        std_s = torch.where(ok[:, None], std, torch.ones_like(std))
        dist = Normal(mean_s, std_s, validate_args=False)  # no host sync (graph capture)
        if eps is None:
            eps = torch.randn(mean.shape, generator=generator, device=mean.device, dtype=mean.dtype)
        actions = mean_s + std_s * eps
        if noise is not None:
            if noise_eps is None:
                noise_eps = torch.randn(mean.shape, generator=generator, device=mean.device,
                                        dtype=mean.dtype)
            actions = actions + noise * noise_eps
        actions = torch.clamp(actions, 0, 1)
        return actions, dist.log_prob(actions), ok

    def get_dist(self, obs, actions, bn="sample"):
        """network.py:117-152: (log_probs, entropies) of given actions."""
        mean, std = self.heads(obs, bn)
        dist = Normal(mean, std)
        return dist.log_prob(actions), dist.entropy()


class BatchedCritic(_Net):
    """network.py:154-172 `Value` (already batched in the reference): the
    centralised critic over the concatenated observations of one side."""

    def __init__(self, n_inputs):
        super().__init__()
        self.fc1 = nn.Linear(n_inputs, 32, bias=True)
        self.fc2 = nn.Linear(32, 64, bias=True)
        self.fc3 = nn.Linear(64, 64, bias=True)
        self.fc4 = nn.Linear(64, 1)
        for m in (self.fc1, self.fc2, self.fc3, self.fc4):
            nn.init.xavier_uniform_(m.weight)

    def packed(self, n_ships, obs_dim):
        """Parameters in lnw_rollout_post's order (csrc/lnw_actor.hip): the MFMA
        A-operand fragments of fc1 per ship (its obs_dim inputs zero-padded to
        a multiple of 16), b1; fc2 fragments, b2; fc3 fragments, b3; fc4 w
        [64], b (+ 3 zeros). Fragments: float4 [n-tile][k-quad][lane] =
        W[16 nt + lane % 16][16 q + 4 (lane // 16) + 0..3] (BatchedActor.packed_policy)."""
        dev = self.fc1.weight.device

        def frags(w, k_pad, n_pad):
            wp = torch.zeros((n_pad, k_pad), dtype=torch.float32, device=dev)
            wp[:w.shape[0], :w.shape[1]] = w.detach().float()
            return wp.reshape(n_pad // 16, 16, k_pad // 16, 4, 4).permute(0, 2, 3, 1, 4).reshape(-1)

        dq = (obs_dim + 15) // 16
        w1 = self.fc1.weight.detach().float().reshape(32, n_ships, obs_dim)
        f1 = torch.cat([frags(w1[:, i], 16 * dq, 32) for i in range(n_ships)])
        parts = [f1, self.fc1.bias, frags(self.fc2.weight, 32, 64), self.fc2.bias,
                 frags(self.fc3.weight, 64, 64), self.fc3.bias, self.fc4.weight.reshape(-1),
                 self.fc4.bias, torch.zeros(3, device=dev)]
        return torch.cat([p.detach().reshape(-1).float() for p in parts]).contiguous()

    def forward(self, x):
        return critic_value(self._p(), torch.flatten(x, 1))


def random_rows(u):
    """The random rows [B, 3] of ddqn.py:300 from uniforms u [B, 4] (u0 decides
    whether a row explores, u0 < eps): [(int)(u1*2), (int)(u2*5), (int)(u3*50)],
    float32 multiply then truncate."""
    return torch.stack([(u[:, 1] * 2.0).to(torch.int32), (u[:, 2] * 5.0).to(torch.int32),
                        (u[:, 3] * 50.0).to(torch.int32)], 1)


class BatchedQNet(_ConvNet):
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

    def packed(self):
        """Every parameter lnw_qnet_act reads (csrc/lnw_qnet.hip), in its order:
        the conv head in lnw_actor_features' order (578 floats), then W [57][n_in]
        with the rows in radar, attack, movement order, then b [57]."""
        return layout.pack(self, packed_slices(self.n_in))

    @torch.no_grad()
    def unpack_(self, flat):
        """The inverse of packed(): load a flat vector in its layout into the
        parameters and running statistics, in place."""
        sl = packed_slices(self.n_in)
        if flat.numel() != layout.flat_size(sl):
            raise ValueError("flat vector length does not match packed()")
        return layout.unpack_(self, flat, sl)

    def q_torch(self, obs, bn="sample"):
        """DMLP.forward as torch ops (host or device): [B, 57] = [radar,
        attack, movement] after the ReLU."""
        p = self._p()
        return q_heads(p, trunk(p, obs, bn)[0])

    def q(self, obs, bn="sample"):
        """The ReLU'd Q-values [B, 57] of obs [B, D]: the HIP kernel
        (lnw_qnet_act's q_out) for device tensors, torch ops for host tensors
        and for bn="batch"."""
        if not obs.is_cuda or bn == "batch":
            return self.q_torch(obs, bn)
        if bn not in ("sample", "running"):
            raise ValueError(BN_MODES)
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
        _abi.check(L.lnw_qnet_act(C.byref(a), _abi.stream(dev)))
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
        _abi.check_impl(impl)
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


# ---- parameter noise (ppo.py:452-482): flat and packed actor vectors -----------
# The flat layout is the learner's (layout.actor_slices, include/lnw.h), the
# packed one what lnw_policy_act reads (BatchedActor.packed_policy()).
NOISE_FREE = ("norm1", "norm2", "layernorm")  # name parts the reference leaves alone (ppo.py:470-473)


def flat_n_in(P):
    """n_in of a flat actor vector of P floats (P = 7139 + 66 n_in)."""
    n_in, rem = divmod(int(P) - 7139, 66)
    if rem or n_in < 12:
        raise ValueError(f"{P} floats is no flat actor vector")
    return n_in


def noise_mask(n_in, device=None):
    """float32 [P], 1 where parameter noise is added, in the flat layout: every
    weight and bias of conv1, conv2, convhead, fc1, fc2, fc3 and the two heads; 0
    on norm1.*, norm2.* (running statistics included), layernorm.* and the logstd
    slot (which the reference noises, and nothing reads)."""
    sl = actor_slices(n_in)
    m = torch.zeros(flat_size(sl), dtype=torch.float32)
    for name, (k, shp) in sl.items():
        if name != "logstd" and not any(s in name for s in NOISE_FREE):
            m[k:k + int(np.prod(shp))] = 1.0
    return m.to(device) if device is not None else m


def unpack_policy(packed, n_in):
    """The inverse of BatchedActor.packed_policy(): packed sets [..., floats] to
    flat vectors [..., P], bit for bit (hi + mid + lo of a weight's three
    bfloat16 terms is exact in float32). The logstd slot, which the packed set
    does not hold, is 0."""
    sl = actor_slices(n_in)
    P = flat_size(sl)
    x = packed.reshape(-1, packed.shape[-1])
    M = x.shape[0]
    out = torch.zeros((M, P), dtype=torch.float32, device=x.device)
    n_par = CONV_PARAMS + 2 * n_in
    out[:, :n_par] = x[:, :n_par]
    o = (n_par + 3) & ~3
    for name, cnt in (("fc1.bias", 64), ("fc2.bias", 64), ("fc3.bias", 32)):
        out[:, sl[name][0]:sl[name][0] + cnt] = x[:, o:o + cnt]
        o += cnt
    for name, k_pad, n_pad, rows, cols in (("fc1.weight", 32 if n_in <= 32 else 64, 64, 64, n_in),
                                           ("fc2.weight", 64, 64, 64, 64), ("fc3.weight", 64, 32, 32, 64),
                                           ("normal_head.weight", 32, 16, 8, 32)):  # (+ log_std_head, adjacent)
        nt, qp = n_pad // 16, k_pad // 32
        cnt = 3 * nt * qp * 64 * 4
        pl = x[:, o:o + cnt].contiguous().view(torch.bfloat16).reshape(M, 3, nt, qp, 64, 8).float()
        o += cnt
        w = (pl[:, 0] + pl[:, 1]) + pl[:, 2]
        # [nt][p][lane = 16 g + m][j = 4 half + v] -> [nt][m][p][half][g][v]
        w = w.reshape(M, nt, qp, 4, 16, 2, 4).permute(0, 1, 4, 2, 5, 3, 6).reshape(M, n_pad, k_pad)
        out[:, sl[name][0]:sl[name][0] + rows * cols] = w[:, :rows, :cols].reshape(M, -1)
    return out.reshape(packed.shape[:-1] + (P,))
