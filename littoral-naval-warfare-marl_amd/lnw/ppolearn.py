"""The learner half of the MAPPO loop: one minibatch update of the reference's
PPO.learn (ppo.py:321-390) for one side, on flat device vectors: the side whose
actor and critic it is given (n ships and rows of D floats follow from their
shapes), blue, or red from a Rollout(side="red").

Reference: ppo.py:673-693 (evaluate), ppo.py:695-714 (gae, over the minibatch
rows as the sequence), ppo.py:716-729 (popart_normalize), ppo.py:342-362 (the
two losses), ppo.py:371-380 (clip_grad_norm_ and Adam per network),
ppo.py:311-319 (the prioritised sampler). The kernels are csrc/lnw_ppolearn.hip
(lnw_ppo_grad, lnw_ppo_clip_adam), csrc/lnw_pposample.hip (lnw_ppo_sample,
the keyed minibatch draw behind PPOLearner.minibatch: lnw/keyed.py, with its
host restatement sample_keys) and csrc/lnw_ppodist.hip (the merge and the row
exchange behind PPOLearner.minibatch_dist, which trains on rollouts sharded
over ranks: lnw/ppodist.py). The flat layouts are lnw/layout.py's
(actor_slices, critic_slices, pack), the torch arm's forwards lnw/nets.py's
(actor_forward, critic_forward). learn()'s outer schedule
(noise ratio, lr halving on victories, epoch count) stays with the caller;
parameter noise is the rollout's (lnw.rollout.Rollout(param_noise=..., theta=
learner.theta_actor) acts from this learner's flat vector).
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _abi, keyed, layout
from .keyed import _p_log, _philox10, sample_keys  # noqa: F401  (the draw's host restatement lives there)
from .layout import (ACTOR_NAMES, CONV_PARAMS, CRITIC_NAMES, RUNNING, WINDOW, actor_slices,  # noqa: F401
                     critic_slices, flat_size, pack)
from .nets import actor_forward, critic_forward


def gae_rows(rtg, values, gamma, lambda_, block=512):
    """PPO.gae (ppo.py:695-714) over the rows of a minibatch as the sequence,
    returns = gae + values: g_i = delta_i + gamma lambda g_{i+1}, delta_i = rtg_i
    + gamma v_{i+1} - v_i (no v term after the last row). The recurrence runs in
    blocks (a triangular matrix of powers per block, a carry between blocks), in
    the dtype of rtg."""
    B = rtg.shape[0]
    nxt = torch.cat([values[1:], torch.zeros_like(values[:1])])
    delta = rtg + gamma * nxt - values
    c = gamma * lambda_
    k = torch.arange(block, device=rtg.device, dtype=rtg.dtype)
    e = k[None, :] - k[:, None]
    tri = torch.where(e >= 0, torch.pow(torch.as_tensor(c, dtype=rtg.dtype, device=rtg.device), e.clamp(min=0)),
                      torch.zeros((), dtype=rtg.dtype, device=rtg.device))
    g = torch.empty_like(delta)
    carry = torch.zeros((), dtype=rtg.dtype, device=rtg.device)
    for hi in range(B, 0, -block):
        lo = max(hi - block, 0)
        m = hi - lo
        # g[lo + i] = sum_{j >= i} c^(j - i) delta[lo + j] + c^(m - i) carry
        g[lo:hi] = tri[:m, :m] @ delta[lo:hi] + torch.pow(torch.as_tensor(c, dtype=rtg.dtype, device=rtg.device),
                                                           m - k[:m]) * carry
        carry = g[lo]
    return g + values


def popart(adv, rtg):
    """ppo.py:716-729 `popart_normalize` (unbiased std; NaN where it is 0)."""
    return (adv - adv.mean()) / adv.std() * rtg.std() + rtg.mean()


def losses(lp, ent, v, adv, old_lp, rtg, old_v, eps_clip, entropy_coef):
    """ppo.py:342-362: (actor_loss, critic_loss)."""
    ratio = torch.exp(lp - old_lp)
    a = adv[:, None]
    surr1 = a * ratio
    surr2 = torch.clamp(ratio, 1 - eps_clip, 1 + eps_clip) * a
    actor_loss = -(torch.min(surr1, surr2).mean() + entropy_coef * ent.mean())
    critic_loss = torch.sqrt(torch.max((v - rtg) ** 2,
                                       (torch.clamp(v, old_v - eps_clip, old_v + eps_clip) - rtg) ** 2).mean())
    return actor_loss, critic_loss


def running_after(r0, stats, momentum=0.1):
    """The running statistics after one BatchNorm update per row of stats
    [B, C], rows in order: (1 - m)^B r0 + m sum_i (1 - m)^(B - 1 - i) stat_i, in
    float64."""
    B = stats.shape[0]
    wgt = torch.pow(torch.as_tensor(1.0 - momentum, dtype=torch.float64, device=stats.device),
                    torch.arange(B - 1, -1, -1, device=stats.device, dtype=torch.float64))
    return (1.0 - momentum) ** B * r0.double() + momentum * (wgt[:, None] * stats.double()).sum(0)


class PPOLearner:
    """PPO.learn's minibatch update (ppo.py:321-390) for one side (blue, or red
    given the red actor and critic and a Rollout(side="red")'s buffers) on flat
    device vectors: `theta_actor` (actor_slices layout) and `theta_critic`
    (critic_slices layout), each with Adam moments `m`, `v` and a device step
    counter.

    One update on B rows, each one (rollout, step, ship), in the order given (the
    order matters: the reference's gae scans the minibatch rows, and the actor's
    running statistics take one update per row): the actor row by row with the
    row's own BatchNorm statistics (BatchedActor's bn="sample"), the critic on
    the rows' global states, advantage = popart(gae(rtg, V) , rtg), the clipped
    surrogate with the entropy bonus, the clipped RMSE value loss, and per
    network clip_grad_norm_(max_grad_norm) and Adam.

    impl="hip": lnw_ppo_grad + lnw_ppo_clip_adam (csrc/lnw_ppolearn.hip), a chain
    of launches on the current stream with no host synchronisation; capturable
    in a torch.cuda.graph. impl="torch": the same step with torch ops, autograd,
    clip_grad_norm_ and torch.optim.Adam on the same flat state, on the host or
    the device — the arm the kernels are tested and timed against.

    batch (what rows() and minibatch() return): dict(obs [groups, n, D] float32,
    index [B] int64 rows of obs.reshape(-1, D) or None for all rows in order,
    actions [B, 4], old_log_probs [B, 4], rtg [B], old_values [B]). minibatch()
    draws the reference's prioritised minibatch on the device (lnw_ppo_sample);
    minibatch_dist() draws it over the rollouts of every rank of a process group;
    sample() is the same distribution through torch.multinomial."""

    def __init__(self, actor, critic, lr=1e-4, eps_clip=0.2, entropy_coef=0.2, gamma=0.99, lambda_=0.95,
                 max_grad_norm=1.0, betas=(0.9, 0.999), eps=1e-8, impl="hip", device=None, sample_seed=0):
        _abi.check_impl(impl)
        if device is None:
            device = "cuda" if impl == "hip" else next(actor.parameters()).device
        self.device = dev = torch.device(device)
        if impl == "hip" and dev.type != "cuda":
            raise ValueError("impl='hip' needs a GPU device")
        self.actor, self.critic, self.impl = actor, critic, impl
        self.lr, self.eps_clip, self.entropy_coef = float(lr), float(eps_clip), float(entropy_coef)
        self.gamma, self.lambda_, self.max_grad_norm = float(gamma), float(lambda_), float(max_grad_norm)
        self.betas, self.eps = tuple(betas), float(eps)
        self.n_in = actor.layernorm.normalized_shape[0]
        self.D = self.n_in - 12 + WINDOW
        k1 = critic.fc1.weight.shape[1]
        if k1 % self.D:
            raise ValueError("the critic's input is not a whole number of actor observation rows")
        self.n = k1 // self.D
        self.actor_sl, self.critic_sl = actor_slices(self.n_in), critic_slices(self.n, self.D)
        self.theta_actor = pack(actor, self.actor_sl).to(dev)
        self.theta_critic = pack(critic, self.critic_sl).to(dev)
        z = torch.zeros_like
        self.m_actor, self.v_actor = z(self.theta_actor), z(self.theta_actor)
        self.m_critic, self.v_critic = z(self.theta_critic), z(self.theta_critic)
        self.step_actor = torch.zeros(1, dtype=torch.int64, device=dev)
        self.step_critic = torch.zeros(1, dtype=torch.int64, device=dev)
        self.nbt = torch.tensor([int(actor.norm1.num_batches_tracked)], dtype=torch.int64, device=dev)
        self._grad_actor, self._grad_critic = z(self.theta_actor), z(self.theta_critic)
        self._loss = torch.zeros(2, dtype=torch.float32, device=dev)
        # [actor, critic][clip factor, gradient norm] of the last step()
        self.clip = torch.zeros((2, 2), dtype=torch.float32, device=dev)
        self._ws = None
        self._opt = None
        # minibatch(): the default seed, the draw counter (the slot of the next draw), the last draw's count of
        # rows with a non-finite rtg, and the output buffers and workspace per (rows, batch)
        self.sample_seed = int(sample_seed)
        self.draw = torch.zeros(1, dtype=torch.int64, device=dev)
        self.sample_status = torch.zeros(1, dtype=torch.int64, device=dev)
        self._sample_buf = {}
        self._dist_buf = {}  # minibatch_dist(): the merge's outputs and the exchange buffer per (batch, n, D)

    # ---- batches -------------------------------------------------------------------
    def rows(self, out, index=None, rtg=None):
        """A Rollout.run() result as the learner's batch, without copying `obs`:
        row r = (env, step, ship) of obs.reshape(-1, D); index: the rows of the
        minibatch in order (None: every row). rtg: a reward-to-go [E, T, n]
        instead of out["rtg"]; old values are out["values"] repeated per ship."""
        dev = self.device
        obs = out["obs"]
        n, D = obs.shape[-2], obs.shape[-1]
        obs = obs.reshape(-1, n, D).to(dev, torch.float32).contiguous()
        rtg = (out["rtg"] if rtg is None else rtg).reshape(-1).to(dev, torch.float32)
        acts = out["actions"].reshape(-1, 4).to(dev, torch.float32)
        lps = out["log_probs"].reshape(-1, 4).to(dev, torch.float32)
        vals = out["values"].reshape(-1).to(dev, torch.float32)
        if index is None:
            old_v = vals[:, None].expand(vals.shape[0], n).reshape(-1)
            return dict(obs=obs, index=None, actions=acts.contiguous(), old_log_probs=lps.contiguous(),
                        rtg=rtg.contiguous(), old_values=old_v.contiguous())
        index = index.to(dev, torch.int64).contiguous()
        return dict(obs=obs, index=index, actions=acts[index].contiguous(), old_log_probs=lps[index].contiguous(),
                    rtg=rtg[index].contiguous(), old_values=vals[torch.div(index, n, rounding_mode="floor")].contiguous())

    def sample(self, out, batch, generator=None, rtg=None):
        """ppo.py:311-319: `batch` distinct rows drawn with priorities |rtg| +
        1e-5 (torch.multinomial without replacement, on the learner's device);
        the row index [batch] int64 in draw order, for rows()."""
        rtg = (out["rtg"] if rtg is None else rtg).reshape(-1).to(self.device, torch.float32)
        pr = torch.abs(rtg) + 1e-5
        return torch.multinomial(pr / pr.sum(), int(batch), replacement=False, generator=generator)

    def minibatch(self, out, batch, seed=None, rtg=None, row_base=0, advance=True):
        """The prioritised minibatch of a Rollout.run() result, drawn and
        gathered on the device: what rows(out, sample(out, batch)) returns, ready
        for step() / grad(), plus `key` [batch] float64. The draw is
        lnw_ppo_sample's (include/lnw.h): the reference sampler's distribution
        (`batch` distinct rows by priorities |rtg| + 1e-5, in draw order) as a
        pure function of (seed, draw counter, global row), so it is bitwise
        reproducible, shards of the rows merge by `key` into the draw over all
        of them (global row = row_base + index), and a captured graph draws
        fresh rows at every replay. seed: None for self.sample_seed. The counter
        self.draw advances by one unless advance is False; self.sample_status
        counts the rows whose rtg is not finite (drawn last, in row order).

        impl="hip": a chain of launches on the current stream with no host
        synchronisation, capturable with step() in one torch.cuda.graph; the
        returned tensors are buffers kept per (rows, batch) that the next call
        of the same shape overwrites. impl="torch": the same draw from the
        definition with NumPy on the host (it reads the counter, so it
        synchronises), the same index bit for bit."""
        ro = self.rollout_rows(out, rtg)
        N = ro["rtg"].shape[0]
        B = keyed.check_batch(batch, N)
        buf = None  # (the torch arm returns new tensors)
        if self.impl == "hip":
            buf = keyed.cached(self._sample_buf, (N, B),
                               lambda: keyed.draw_buffers(N, B, self.device, "hip", payload=True))
        b = keyed.draw(ro["rtg"], B, self.sample_seed if seed is None else seed, self.draw, self.sample_status,
                       row_base, advance, self.impl, buf, payload=ro)
        return dict(obs=ro["obs"], index=b["index"], actions=b["actions"], old_log_probs=b["old_log_probs"],
                    rtg=b["rtg"], old_values=b["old_values"], key=b["key"])

    def rollout_rows(self, out, rtg=None):
        """The tensors of a Rollout.run() result as the draw reads them, on the
        learner's device, without a copy where they already are float32 and
        contiguous: dict(obs [groups, n, D], rtg [N], actions, log_probs [N, 4],
        values [groups], n, D), N = groups * n rows of (env, step, ship)."""
        dev = self.device
        obs = out["obs"]
        n, D = obs.shape[-2], obs.shape[-1]
        obs = obs.reshape(-1, n, D).to(dev, torch.float32).contiguous()
        rtg = (out["rtg"] if rtg is None else rtg).reshape(-1).to(dev, torch.float32).contiguous()
        acts = out["actions"].reshape(-1, 4).to(dev, torch.float32).contiguous()
        lps = out["log_probs"].reshape(-1, 4).to(dev, torch.float32).contiguous()
        vals = out["values"].reshape(-1).to(dev, torch.float32).contiguous()
        N = rtg.shape[0]
        if acts.shape[0] != N or lps.shape[0] != N or vals.shape[0] * n != N:
            raise ValueError("rtg, actions and log_probs need one row per (env, step, ship), values one per (env, step)")
        return dict(obs=obs, rtg=rtg, actions=acts, log_probs=lps, values=vals, n=n, D=D)

    def minibatch_dist(self, out, batch, row_base, seed=None, rtg=None, advance=True, group=None):
        """minibatch() over rollouts sharded across the ranks of a process group:
        `out` holds this rank's rows, global rows [row_base, row_base + rows) of
        the job's (row_base a multiple of n; the ranks' ranges are disjoint), and
        every rank gets the minibatch that one minibatch() over all the rows
        would draw, with its payload: the dict step() / grad() take, obs = the
        drawn rows' groups packed as [batch, n, D], index their rows of it,
        actions, old_log_probs, rtg, old_values, key, and global_row [batch]
        int64. Same seed, counter and learner state on every rank give bitwise
        equal results on every rank, so the ranks' step() stay equal to each
        other and to one rank training on all rows.

        Every rank draws `batch` candidates locally (batch <= its own rows, else
        ValueError before any collective), one all-gather exchanges the
        candidate lists, lnw_ppo_sample_merge merges them, lnw_ppo_rows_pack
        packs the rows this rank owns, and one int32 SUM all-reduce assembles
        the buffer (lnw.ppodist). group: the process group (None: the default
        one; with none initialised, a world of one). On "nccl" (RCCL) nothing
        synchronises with the host; "gloo" stages through it. self.draw advances
        as in minibatch(); self.sample_status holds the count over all ranks.
        The returned tensors are buffers the next call of the same shape
        overwrites. impl="torch": the same protocol with NumPy / torch indexing."""
        from . import ppodist
        return ppodist.minibatch_dist(self, out, batch, row_base, seed=seed, rtg=rtg, advance=advance, group=group)

    def _batch(self, b):
        dev = self.device
        f = lambda t: t.to(dev, torch.float32).contiguous()  # noqa: E731
        obs = f(b["obs"])
        if obs.dim() != 3 or obs.shape[1] != self.n or obs.shape[2] != self.D:
            raise ValueError(f"obs must be [groups, {self.n}, {self.D}]")
        idx = b.get("index")
        if idx is not None:
            idx = idx.to(dev, torch.int64).contiguous()
        return dict(obs=obs, index=idx, actions=f(b["actions"]).reshape(-1, 4),
                    old_log_probs=f(b["old_log_probs"]).reshape(-1, 4), rtg=f(b["rtg"]).reshape(-1),
                    old_values=f(b["old_values"]).reshape(-1))

    # ---- HIP arm ---------------------------------------------------------------------
    def _grad_hip(self, b, want, freeze):
        L = _abi.load()
        dev = self.device
        B = b["rtg"].shape[0]
        need = L.lnw_ppolearn_workspace_bytes(B, self.n, self.D)
        if need <= 0:
            raise _abi.LnwError(f"lnw_ppo_grad does not support rows={B}, n={self.n}, D={self.D}")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        a = _abi.PpolearnArgs()
        a.obs, a.rows, a.n, a.D = b["obs"].data_ptr(), B, self.n, self.D
        a.row_index = b["index"].data_ptr() if b["index"] is not None else None
        a.actions, a.old_log_probs = b["actions"].data_ptr(), b["old_log_probs"].data_ptr()
        a.rtg, a.old_values = b["rtg"].data_ptr(), b["old_values"].data_ptr()
        a.eps_clip, a.entropy_coef, a.gamma, a.lambda_ = self.eps_clip, self.entropy_coef, self.gamma, self.lambda_
        a.freeze_running = int(freeze)
        a.actor_params, a.critic_params = self.theta_actor.data_ptr(), self.theta_critic.data_ptr()
        a.actor_grad, a.critic_grad = self._grad_actor.data_ptr(), self._grad_critic.data_ptr()
        a.actor_loss, a.critic_loss = self._loss.data_ptr(), self._loss.data_ptr() + 4
        out = {}
        if want:
            out["new_log_probs"] = torch.empty((B, 4), dtype=torch.float32, device=dev)
            out["entropies"] = torch.empty((B, 4), dtype=torch.float32, device=dev)
            out["values"] = torch.empty(B, dtype=torch.float32, device=dev)
            out["advantage"] = torch.empty(B, dtype=torch.float32, device=dev)
            a.new_log_probs, a.entropies = out["new_log_probs"].data_ptr(), out["entropies"].data_ptr()
            a.values, a.advantage = out["values"].data_ptr(), out["advantage"].data_ptr()
        a.workspace, a.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        _abi.check(L.lnw_ppo_grad(C.byref(a), _abi.stream(dev)))
        return out

    def _adam_hip(self):
        L = _abi.load()
        st = _abi.stream(self.device)
        for k, (th, g, m, v, cnt) in enumerate(((self.theta_actor, self._grad_actor, self.m_actor, self.v_actor,
                                                 self.step_actor),
                                                (self.theta_critic, self._grad_critic, self.m_critic, self.v_critic,
                                                 self.step_critic))):
            _abi.check(L.lnw_ppo_clip_adam(th.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), th.numel(),
                                           cnt.data_ptr(), self.lr, self.betas[0], self.betas[1], self.eps,
                                           self.max_grad_norm, self.clip.data_ptr() + 8 * k, st))

    # ---- torch arm -------------------------------------------------------------------
    def _grad_torch(self, b, freeze):
        n, D = self.n, self.D
        flat = b["obs"].reshape(-1, D)
        gs_all = b["obs"].reshape(-1, n * D)
        if b["index"] is None:
            obs = flat
            gs = gs_all.repeat_interleave(n, 0)
        else:
            obs = flat[b["index"]]
            gs = gs_all[torch.div(b["index"], n, rounding_mode="floor")]
        tha = self.theta_actor.detach().clone().requires_grad_(True)
        thc = self.theta_critic.detach().clone().requires_grad_(True)
        lp, ent, stats = actor_forward(tha, obs, b["actions"], self.actor_sl)
        v = critic_forward(thc, gs, self.critic_sl)
        with torch.no_grad():
            adv = popart(gae_rows(b["rtg"], v.detach(), self.gamma, self.lambda_), b["rtg"])
        al, cl = losses(lp, ent, v, adv, b["old_log_probs"], b["rtg"], b["old_values"], self.eps_clip,
                        self.entropy_coef)
        al.backward()
        cl.backward()
        self._grad_actor.copy_(tha.grad)
        self._grad_critic.copy_(thc.grad)
        self._loss.copy_(torch.stack([al.detach(), cl.detach()]))
        if not freeze:
            with torch.no_grad():
                for name, lo, hi in (("norm1.running_mean", 0, 5), ("norm2.running_mean", 5, 13),
                                     ("norm1.running_var", 13, 18), ("norm2.running_var", 18, 26)):
                    k, shp = self.actor_sl[name]
                    seg = self.theta_actor[k:k + shp[0]]
                    seg.copy_(running_after(seg, stats[:, lo:hi]).float())
        return dict(new_log_probs=lp.detach(), entropies=ent.detach(), values=v.detach(), advantage=adv)

    def _adam_torch(self):
        if self._opt is None:
            self._p, self._opt = [], []
            for th, m, v in ((self.theta_actor, self.m_actor, self.v_actor),
                             (self.theta_critic, self.m_critic, self.v_critic)):
                p = nn.Parameter(th)  # (shares the vector's storage)
                opt = torch.optim.Adam([p], lr=self.lr, betas=self.betas, eps=self.eps)
                st = opt.state[p]
                st["step"], st["exp_avg"], st["exp_avg_sq"] = torch.tensor(0.0), m, v
                self._p.append(p)
                self._opt.append(opt)
        for k, (g, cnt) in enumerate(((self._grad_actor, self.step_actor), (self._grad_critic, self.step_critic))):
            self._p[k].grad = g.clone()
            norm = torch.nn.utils.clip_grad_norm_([self._p[k]], self.max_grad_norm)
            self.clip[k, 0] = torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0)
            self.clip[k, 1] = norm
            self._opt[k].step()
            cnt += 1

    # ---- public ------------------------------------------------------------------------
    def grad(self, batch, update_running=True):
        """Losses and gradients of one minibatch, without the optimiser step:
        dict(actor_loss, critic_loss 0-d; actor_grad, critic_grad unclipped, in
        the flat layouts; actor_norm, critic_norm their L2 norms;
        new_log_probs [B, 4], entropies [B, 4], values [B], advantage [B]). The
        actor's running statistics and batch counter take the B updates of the
        reference's evaluate() unless update_running is False."""
        b = self._batch(batch)
        if self.impl == "hip":
            out = self._grad_hip(b, True, not update_running)
        else:
            out = self._grad_torch(b, not update_running)
        if update_running:
            self.nbt += b["rtg"].shape[0]
        out["actor_loss"], out["critic_loss"] = self._loss[0].clone(), self._loss[1].clone()
        out["actor_grad"], out["critic_grad"] = self._grad_actor.clone(), self._grad_critic.clone()
        out["actor_norm"] = torch.linalg.vector_norm(out["actor_grad"])
        out["critic_norm"] = torch.linalg.vector_norm(out["critic_grad"])
        return out

    def step(self, batch):
        """One minibatch update: gradients, clip_grad_norm_, Adam, for the actor
        and the critic. Returns (actor_loss, critic_loss), 0-d device tensors
        (nothing synchronises with the host)."""
        b = self._batch(batch)
        if self.impl == "hip":
            self._grad_hip(b, False, False)
            self._adam_hip()
        else:
            self._grad_torch(b, False)
            self._adam_torch()
        self.nbt += b["rtg"].shape[0]
        return self._loss[0].clone(), self._loss[1].clone()

    @torch.no_grad()
    def export(self):
        """Write both vectors, the running statistics and num_batches_tracked
        back into the BatchedActor / BatchedCritic modules, on the device they
        live on (device-to-device copies: no host round trip); returns (actor,
        critic). The next Rollout.run() acts with the updated weights."""
        layout.unpack_(self.actor, self.theta_actor, self.actor_sl)
        layout.unpack_(self.critic, self.theta_critic, self.critic_sl)
        for nm in (self.actor.norm1, self.actor.norm2):
            nm.num_batches_tracked.copy_(self.nbt[0])
        return self.actor, self.critic
