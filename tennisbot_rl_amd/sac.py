"""SAC on the batched envs: the gradient step as HIP kernels (csrc/tb_sac.hpp; C ABI tb_sac_* in include/tb_stepper.h).

The rule is SB3 1.8.0's SAC with MlpPolicy as the reference selects it with `-s sac` (train.py:129-130; train_swing.py:93-96 with
batch_size = 1100): actor and two critics are [256, 256] ReLU nets, lr 3e-4 for actor, critic and log_ent_coef, plain Adam (eps
1e-8, no clipping), gamma 0.99, tau 0.005, target_update_interval 1, ent_coef "auto" (log_ent_coef from 0, target entropy -A),
buffer_size 1e6, learning_starts 100 timesteps of uniform actions. One gradient step on a batch (s, a, r, s', d), in SB3's order:

  1. a~, logp = actor(s; eps_pi)                                                             tb_sac_actor_forward
  2. alpha = exp(log_ent_coef) as it is BEFORE this step's update; gradient of log_ent_coef: -mean(logp - A)
  3. y = r + (1 - d) gamma (min(Q1t, Q2t)(s', a') - alpha logp'), a', logp' = actor(s'; eps_next)   tb_sac_targets
  4. critic loss 0.5 (mean (Q1 - y)^2 + mean (Q2 - y)^2); Adam on the critic                 tb_sac_critic_grad, tb_sac_adam
  5. actor loss mean(alpha logp - min(Q1, Q2)(s, a~)) with the UPDATED critic; Adam on the actor  tb_sac_actor_grad, tb_sac_adam
  6. target <- (1 - tau) target + tau critic                                                 (folded into the critic's tb_sac_adam)

The kernels read log_ent_coef on the device, so its Adam step is issued last: steps 3 and 5 see the value of step 2. The noise
is an input (torch.randn, drawn in bulk by the trainer): every stage is deterministic in its inputs, and nothing in a gradient
step synchronises with the host.

Episode ends: the reference registers both envs without a time limit, so every `done` is a true terminal and (1 - d) removes the
bootstrap. With auto-reset the stored s' of a done transition is the next episode's first observation: finite, and selected away.

`FusedSAC` is the learner (flat parameter, gradient and Adam-moment vectors in named_parameters() order; `opt.state` holds views
of them, as `FusedLearner` does), `ReplayBuffer` a device-resident ring, `SACTrainer` the loop around a `BatchedEnv`. There is
no torch fallback for the gradient step: a refused call raises. One rank only.
"""
import copy
import math
import sys
import time

from .learner import flatten_parameters
from .params import ENV_SWING
from .stepper import ACT_DIM, ENV_IDS, OBS_DIM, BatchedEnv, StepperError, _check, load_library

TB_SAC_ACTOR, TB_SAC_CRITIC = 0, 1
HIDDEN = 256
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
SAC_DEFAULTS = dict(learning_rate=3e-4, gamma=0.99, tau=0.005, adam_eps=1e-8)
BATCH_SIZE = {"SwingRacket-v0": 1100, "Tennisbot-v0": 256}   # train_swing.py:93-96 / train.py:129-130 (SB3's default)
# launches of one gradient_step: actor forward 5 (gather, three tile launches, sample), targets 9 (gather, actor 4, the two targets'
# three layers in 3, y), critic gradient 10 (gather, forward 3, loss, backward 2, weight gradients 3), its Adam + Polyak 1, actor
# gradient 13 (critics forward 3, loss, their backward 3, the head's backward, the actor's backward 2 and weight gradients 3), Adam 2
LAUNCHES_PER_STEP = 40
EVAL_FORMS = ("torch", "fused")   # SACTrainer.evaluate_episodes: the torch actor between env steps / one tb_sac_evaluate launch
COLLECT_FORMS = ("torch", "fused")   # SACTrainer.vector_step: the torch actor between single env steps / tb_sac_collect launches into the ring
SWING_EPISODE_STEPS = 26
ACTOR_NAMES = ("latent_pi.0.weight", "latent_pi.0.bias", "latent_pi.2.weight", "latent_pi.2.bias", "mu.weight", "mu.bias", "log_std.weight", "log_std.bias")
CRITIC_NAMES = tuple("qf%d.%d.%s" % (q, layer, w) for q in (0, 1) for layer in (0, 2, 4) for w in ("weight", "bias"))


def build_sac_modules(obs_dim, act_dim):
    """(actor, critic, critic_target): torch modules whose named_parameters() are SB3's SAC MlpPolicy names and shapes. The actor
    has `sample(obs, eps) -> (action, logp)` and `mean_action(obs)`; the critic `forward(obs, action) -> (q0, q1)`, each [n]."""
    import torch
    from torch import nn

    class Actor(nn.Module):
        def __init__(self):
            super().__init__()
            self.latent_pi = nn.Sequential(nn.Linear(obs_dim, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, HIDDEN), nn.ReLU())
            self.mu = nn.Linear(HIDDEN, act_dim)
            self.log_std = nn.Linear(HIDDEN, act_dim)

        def heads(self, obs):
            h = self.latent_pi(obs)
            return self.mu(h), self.log_std(h).clamp(LOG_STD_MIN, LOG_STD_MAX)

        def sample(self, obs, eps):
            mu, log_std = self.heads(obs)
            a = torch.tanh(mu + log_std.exp() * eps)
            logp = (-0.5 * eps * eps - log_std - 0.5 * math.log(2.0 * math.pi)).sum(1) - torch.log(1.0 - a * a + 1e-6).sum(1)
            return a, logp

        def mean_action(self, obs):
            return torch.tanh(self.heads(obs)[0])

    class Critic(nn.Module):
        def __init__(self):
            super().__init__()
            for q in (0, 1):
                setattr(self, "qf%d" % q, nn.Sequential(nn.Linear(obs_dim + act_dim, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, 1)))

        def forward(self, obs, action):
            x = torch.cat([obs, action], 1)
            return self.qf0(x)[:, 0], self.qf1(x)[:, 0]

    actor, critic = Actor(), Critic()
    target = copy.deepcopy(critic)
    for p in target.parameters():
        p.requires_grad_(False)
    return actor, critic, target


def flatten_actor(state_dict):
    """a SAC / TQC trainer checkpoint's `actor` state dict as the flat TB_SAC_ACTOR vector (ACTOR_NAMES order)"""
    import torch
    return torch.cat([state_dict[k].detach().reshape(-1).float() for k in ACTOR_NAMES]).contiguous()


class _Flat:
    """one module's flat parameter vector with its gradient and Adam moments, and the optimiser whose state views them"""

    def __init__(self, torch, params, flat, opt, what):
        self.params, self.flat, self.opt, self.n = params, flat, opt, int(flat.numel())
        if opt is not None:
            g = opt.param_groups
            if type(opt) is not torch.optim.Adam or len(g) != 1 or [id(p) for p in g[0]["params"]] != [id(p) for p in params]:
                raise StepperError("FusedSAC: the %s's optimiser must be a plain torch.optim.Adam over its parameters in named_parameters() order, in one group" % what)
            if g[0].get("amsgrad") or g[0].get("weight_decay") or g[0].get("maximize"):
                raise StepperError("FusedSAC: plain Adam only (no amsgrad, weight decay or maximize) for the %s" % what)
            z = lambda: torch.zeros(self.n, dtype=torch.float32, device=flat.device)  # noqa: E731
            self.grad, self.exp_avg, self.exp_avg_sq = z(), z(), z()
            self.views, off = [], 0
            for p in params:
                k = p.numel()
                self.views.append(tuple(b[off:off + k].view(p.shape) for b in (self.grad, self.exp_avg, self.exp_avg_sq)))
                off += k

    def adopt(self, torch):
        """the moments as the optimiser holds them now into the flat buffers, the buffers' views into opt.state; the step count"""
        step = None
        for p, (gv, mv, vv) in zip(self.params, self.views):
            st = self.opt.state[p]
            if len(st) == 0:
                mv.zero_(); vv.zero_()
                st["step"] = torch.tensor(0.0)
            else:
                if st["exp_avg"].data_ptr() != mv.data_ptr():
                    mv.copy_(st["exp_avg"])
                if st["exp_avg_sq"].data_ptr() != vv.data_ptr():
                    vv.copy_(st["exp_avg_sq"])
            st["exp_avg"], st["exp_avg_sq"] = mv, vv
            k = int(st["step"])
            if step is not None and k != step:
                raise StepperError("FusedSAC: an optimiser's parameters have taken different numbers of steps")
            step = k
        return step

    def publish(self, torch, step):
        for p, (gv, mv, vv) in zip(self.params, self.views):
            st = self.opt.state[p]
            st["step"] = torch.tensor(float(step), dtype=st["step"].dtype, device=st["step"].device)
            p.grad = gv


class FusedSAC:
    """SAC's gradient step on the device for (actor, critic, critic_target, log_ent_coef) and their three Adam optimisers
    `optimisers = (actor_opt, critic_opt, ent_opt)`. hp: gamma, tau (SAC_DEFAULTS); lr, betas and eps are the optimisers' own.
    hp stays the CALLER'S dict (missing keys are filled in place, as FusedLearner does): a later change of trainer.hp reaches the learner.
    What another algorithm on the same actor and stages changes is in the class attributes (tqc.FusedTQC)."""

    ABI = "tb_sac_"   # the C entry points of the stages and the two queries are ABI + their names
    DEFAULTS = SAC_DEFAULTS
    Y_SHAPE = ()      # the trailing shape of y [B, ...]: one target per row
    NET, NET_SHAPE = "SB3's SAC MlpPolicy", "[256, 256] ReLU"   # the words of the architecture message

    def __init__(self, kind, actor, critic, critic_target, log_ent_coef, optimisers, hp, device):
        import torch
        name = type(self).__name__
        self.torch, self.kind, self.hp = torch, int(kind), hp
        self.actor, self.critic, self.critic_target, self.log_ent_coef = actor, critic, critic_target, log_ent_coef
        for k, v in self.DEFAULTS.items():
            hp.setdefault(k, v)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise StepperError("%s needs a GPU (there is no CPU fallback)" % name)
        self.lib = load_library()
        self.O, self.A = OBS_DIM[self.kind], ACT_DIM[self.kind]
        want = {"actor": ACTOR_NAMES, "critic": CRITIC_NAMES, "critic_target": CRITIC_NAMES}
        sets = {}
        for what, module, which in (("actor", actor, TB_SAC_ACTOR), ("critic", critic, TB_SAC_CRITIC), ("critic_target", critic_target, TB_SAC_CRITIC)):
            named = list(module.named_parameters())
            n = self._query("param_floats", self.kind, which)
            if tuple(k for k, _ in named) != want[what] or sum(p.numel() for _, p in named) != n:
                raise StepperError("%s: the %s is not %s net for this env kind (%d parameters in %d tensors; the kernels take %d: %s)"
                                   % (name, what, self.NET, sum(p.numel() for _, p in named), len(named), n, self.NET_SHAPE))
            if any(p.device != self.device and p.device.type != "cuda" for _, p in named):
                raise StepperError("%s: the %s is not on a GPU" % (name, what))
            sets[what] = [p for _, p in named]
        if tuple(log_ent_coef.shape) != (1,) or log_ent_coef.dtype != torch.float32 or log_ent_coef.device.type != "cuda":
            raise StepperError("%s: log_ent_coef must be a float32 tensor of shape [1] on the GPU" % name)
        actor_opt, critic_opt, ent_opt = optimisers
        self.pi = _Flat(torch, sets["actor"], flatten_parameters(actor), actor_opt, "actor")
        self.q = _Flat(torch, sets["critic"], flatten_parameters(critic), critic_opt, "critic")
        self.qt = _Flat(torch, sets["critic_target"], flatten_parameters(critic_target), None, "critic_target")
        self.ent = _Flat(torch, [log_ent_coef], log_ent_coef.data, ent_opt, "entropy coefficient")
        self.stats = torch.zeros(4, dtype=torch.float64, device=self.device)  # critic loss, actor loss, mean logp, d log_ent_coef
        self.step = 0
        self._ws = self._batch = self._pi_batch = None   # _pi_batch: the batch whose actor activations the workspace holds
        self.adopt()

    def _query(self, what, *args):
        """a count from this algorithm's C query `what`; a refusal raises"""
        n = getattr(self.lib, self.ABI + what)(*args)
        if n < 0:
            _check(self.lib, int(n), self.ABI + what)
        return n

    def _call(self, stage, *args):
        """this algorithm's C entry point of a stage; a refusal raises"""
        _check(self.lib, getattr(self.lib, self.ABI + stage)(*args), self.ABI + stage)

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _dev(self):
        return self.device.index if self.device.index is not None else self.torch.cuda.current_device()

    def _float(self, x, name, shape=None):
        t = self.torch
        if x.dtype != t.float32 or x.device.type != "cuda" or not x.is_contiguous() or (shape is not None and tuple(x.shape) != tuple(shape)):
            raise ValueError("%s: contiguous float32 tensor%s on the GPU expected" % (name, "" if shape is None else " of shape %s" % (tuple(shape),)))
        return x

    def _index(self, idx):
        if idx.dtype != self.torch.int64 or idx.device.type != "cuda" or not idx.is_contiguous() or idx.dim() != 1 or idx.numel() < 1:
            raise ValueError("idx: contiguous int64 vector of at least one entry on the GPU expected")
        return idx

    def workspace(self, batch):
        need = self._query("workspace_bytes", self.kind, int(batch))
        if self._ws is None or self._ws.numel() * 8 < need:
            self._ws = self.torch.zeros((need + 7) // 8, dtype=self.torch.float64, device=self.device)
        if self._batch != int(batch):   # the regions' offsets scale with the batch: what an earlier stage kept is gone
            B = self._batch = int(batch)
            self._pi_batch = None
            e = lambda *s: self.torch.empty(s, dtype=self.torch.float32, device=self.device)  # noqa: E731
            self.act_pi, self.logp_pi, self.y = e(B, self.A), e(B), e(B, *self.Y_SHAPE)
        return self._ws

    def adopt(self):
        """take over what the optimisers and modules hold now (after a load_state_dict); returns the step count"""
        t = self.torch
        for f, m in ((self.pi, self.actor), (self.q, self.critic), (self.qt, self.critic_target)):
            f.flat = flatten_parameters(m)
        steps = {f.adopt(t) for f in (self.pi, self.q, self.ent)}
        if len(steps) != 1:
            raise StepperError("FusedSAC: the three optimisers have taken different numbers of steps (%s)" % sorted(steps))
        self.step = steps.pop()
        return self.step

    def publish(self):
        """the step count and the gradients' views into the optimisers' state (what a checkpoint reads)"""
        for f in (self.pi, self.q, self.ent):
            f.publish(self.torch, self.step)

    # --------------------------------------------------------------------------------------------------------------- the stages
    def actor_forward(self, obs, idx, eps, act_out=None, logp_out=None):
        """(a~ [B, A], logp [B]) of the actor on obs[idx] with the noise eps [B, A]; keeps the activations for actor_gradient"""
        B = int(self._index(idx).numel())
        ws = self.workspace(B)
        act_out, logp_out = self.act_pi if act_out is None else act_out, self.logp_pi if logp_out is None else logp_out
        obs, eps = self._float(obs, "obs"), self._float(eps, "eps", (B, self.A))
        self._call("actor_forward", self.kind, self._dev(), self._stream(), obs.data_ptr(), int(obs.shape[0]), idx.data_ptr(), B, self.pi.flat.data_ptr(), eps.data_ptr(),
                   self._float(act_out, "act_out", (B, self.A)).data_ptr(), self._float(logp_out, "logp_out", (B,)).data_ptr(), ws.data_ptr(), ws.numel() * 8)
        self._pi_batch = B
        return act_out, logp_out

    def targets(self, next_obs, reward, done, idx, eps_next, y=None):
        """y [B, *Y_SHAPE]: SAC's target of every row, or TQC's truncated target distribution [B, 46]"""
        B = int(self._index(idx).numel())
        ws = self.workspace(B)
        y = self.y if y is None else y
        next_obs, n = self._float(next_obs, "next_obs"), int(next_obs.shape[0])
        self._call("targets", self.kind, self._dev(), self._stream(), next_obs.data_ptr(), self._float(reward, "reward", (n,)).data_ptr(), self._float(done, "done", (n,)).data_ptr(),
                   n, idx.data_ptr(), B, self.pi.flat.data_ptr(), self.qt.flat.data_ptr(), self.log_ent_coef.data_ptr(), self._float(eps_next, "eps_next", (B, self.A)).data_ptr(),
                   float(self.hp["gamma"]), self._float(y, "y", (B,) + self.Y_SHAPE).data_ptr(), ws.data_ptr(), ws.numel() * 8)
        return y

    def critic_gradient(self, obs, action, idx, y):
        """the critic's gradient into self.q.grad; stats[0] = the critic loss"""
        B = int(self._index(idx).numel())
        ws = self.workspace(B)
        obs, n = self._float(obs, "obs"), int(obs.shape[0])
        self._call("critic_grad", self.kind, self._dev(), self._stream(), obs.data_ptr(), self._float(action, "action", (n, self.A)).data_ptr(), n, idx.data_ptr(), B,
                   self.q.flat.data_ptr(), self._float(y, "y", (B,) + self.Y_SHAPE).data_ptr(), self.q.grad.data_ptr(), self.stats.data_ptr(), ws.data_ptr(), ws.numel() * 8)
        return self.q.grad

    def actor_gradient(self, batch, eps):
        """the actor's gradient into self.pi.grad and log_ent_coef's into self.ent.grad, on the batch of the last actor_forward"""
        B = int(batch)
        if B != self._pi_batch:
            raise ValueError("actor_gradient: the workspace holds %s, not an actor_forward of %d rows (a stage at another batch size in between overwrites it)"
                             % ("no actor_forward" if self._pi_batch is None else "an actor_forward of %d rows" % self._pi_batch, B))
        ws = self.workspace(B)
        self._call("actor_grad", self.kind, self._dev(), self._stream(), B, self.pi.flat.data_ptr(), self.q.flat.data_ptr(), self.log_ent_coef.data_ptr(),
                   self._float(eps, "eps", (B, self.A)).data_ptr(), self.pi.grad.data_ptr(), self.ent.grad.data_ptr(), self.stats.data_ptr(), ws.data_ptr(), ws.numel() * 8)
        return self.pi.grad, self.ent.grad

    def adam(self, f, step, target=None):
        """one Adam step of the flat set f (self.pi, self.q or self.ent) with ITS optimiser's lr, betas and eps; target: a flat
        vector that follows by the Polyak update in the same launch"""
        g = f.opt.param_groups[0]
        _check(self.lib, self.lib.tb_sac_adam(self._dev(), self._stream(), f.flat.data_ptr(), f.grad.data_ptr(), f.exp_avg.data_ptr(), f.exp_avg_sq.data_ptr(), f.n, float(g["lr"]),
                                              float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), int(step), None if target is None else target.data_ptr(),
                                              float(self.hp["tau"])), "tb_sac_adam")

    def polyak(self, params, target, tau):
        _check(self.lib, self.lib.tb_sac_adam(self._dev(), self._stream(), params.data_ptr(), None, None, None, int(params.numel()), 0.0, 0.0, 0.0, 0.0, 1, target.data_ptr(),
                                              float(tau)), "tb_sac_adam")

    def gradient_step(self, replay_arrays, idx, eps_pi, eps_next):
        """one SAC gradient step on the rows idx of replay_arrays = (obs, next_obs, action, reward, done); no host synchronisation"""
        obs, next_obs, action, reward, done = replay_arrays
        B = int(idx.numel())
        self.step += 1
        self.actor_forward(obs, idx, eps_pi)
        y = self.targets(next_obs, reward, done, idx, eps_next)
        self.critic_gradient(obs, action, idx, y)
        self.adam(self.q, self.step, target=self.qt.flat)
        self.actor_gradient(B, eps_pi)
        self.adam(self.pi, self.step)
        self.adam(self.ent, self.step)  # last: the kernels above read log_ent_coef as it was before this step


class ReplayBuffer:
    """a device-resident ring of transitions; takes whole vector steps, samples an int64 index vector on the device"""

    def __init__(self, obs_dim, act_dim, capacity, device):
        import torch
        self.torch, self.capacity, self.device = torch, int(capacity), torch.device(device)
        if self.capacity < 1:
            raise ValueError("ReplayBuffer: capacity must be >= 1")
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.device)  # noqa: E731
        self.obs, self.next_obs, self.action = z(self.capacity, obs_dim), z(self.capacity, obs_dim), z(self.capacity, act_dim)
        self.reward, self.done = z(self.capacity), z(self.capacity)
        self.pos, self.size = 0, 0

    def arrays(self):
        return self.obs, self.next_obs, self.action, self.reward, self.done

    def add(self, obs, next_obs, action, reward, done):
        """n transitions [n, ...] at the cursor (wrapping); done may be uint8 or bool"""
        n = int(obs.shape[0])
        if n > self.capacity:
            raise ValueError("ReplayBuffer.add: %d transitions do not fit a capacity of %d" % (n, self.capacity))
        first = min(n, self.capacity - self.pos)
        for dst, src in zip(self.arrays(), (obs, next_obs, action, reward, done)):
            dst[self.pos:self.pos + first].copy_(src[:first])
            if first < n:
                dst[:n - first].copy_(src[first:])
        self.pos = (self.pos + n) % self.capacity
        self.size = min(self.capacity, self.size + n)

    def reserve(self, n_steps, n_envs):
        """views of the next n_steps * n_envs rows of (obs, next_obs, action, reward, done) for a producer that writes whole vector
        steps in place (tb_sac_collect); the cursor and the fill advance as add() of as many rows would move them. The ring must
        hold whole vector steps (capacity % n_envs == 0, the cursor on a step boundary) and the rows must not cross the wrap:
        plan_collect_chunks cuts a request there."""
        n_steps, n_envs = int(n_steps), int(n_envs)
        if n_steps < 1 or n_envs < 1:
            raise ValueError("ReplayBuffer.reserve: n_steps and n_envs must be >= 1")
        if self.capacity % n_envs or self.pos % n_envs:
            raise ValueError("ReplayBuffer.reserve: capacity %d and cursor %d must be multiples of n_envs = %d" % (self.capacity, self.pos, n_envs))
        rows = n_steps * n_envs
        if self.pos + rows > self.capacity:
            raise ValueError("ReplayBuffer.reserve: %d rows from row %d would cross the wrap at %d" % (rows, self.pos, self.capacity))
        views = tuple(a[self.pos:self.pos + rows] for a in self.arrays())
        self.pos = (self.pos + rows) % self.capacity
        self.size = min(self.capacity, self.size + rows)
        return views

    def sample(self, n):
        if self.size < 1:
            raise ValueError("ReplayBuffer.sample: the buffer is empty")
        return self.torch.randint(0, self.size, (int(n),), device=self.device, dtype=self.torch.int64)

    def state_dict(self):
        return {"pos": self.pos, "size": self.size, "capacity": self.capacity, "arrays": [a[:self.size].cpu() for a in self.arrays()]}

    def load_state_dict(self, sd):
        if int(sd["capacity"]) != self.capacity:
            raise ValueError("ReplayBuffer: the checkpoint's capacity is %d, this buffer's %d" % (sd["capacity"], self.capacity))
        self.pos, self.size = int(sd["pos"]), int(sd["size"])
        for dst, src in zip(self.arrays(), sd["arrays"]):
            dst[:self.size].copy_(src)


def plan_collect_chunks(pos_rows, capacity_rows, n_steps, swing_phase_or_None, steps_to_learning_starts):
    """The launch sizes, in env steps, of a fused collect of n_steps env steps. Rows are VECTOR steps here: the ring's cursor and
    capacity divided by num_envs. A launch ends at the ring's wrap (its rows are contiguous), at SwingRacket's episode end (26 -
    phase: the launch that ends the episodes parks them; None for Tennisbot) and at the step where num_timesteps reaches
    learning_starts (steps_to_learning_starts env steps from now, <= 0 or None: already past), so that uniform and actor
    launches change over at the timestep where the torch form does. Pure: no device, no trainer."""
    pos, cap, left = int(pos_rows), int(capacity_rows), int(n_steps)
    if cap < 1 or not 0 <= pos < cap:
        raise ValueError("plan_collect_chunks: the cursor %d is not inside a ring of %d vector steps" % (pos, cap))
    if left < 1:
        raise ValueError("plan_collect_chunks: n_steps must be >= 1")
    phase = None if swing_phase_or_None is None else int(swing_phase_or_None)
    if phase is not None and not 0 <= phase < SWING_EPISODE_STEPS:
        raise ValueError("plan_collect_chunks: SwingRacket's episode phase must be in [0, %d), not %d (envs out of lockstep?)" % (SWING_EPISODE_STEPS, phase))
    to_ls = 0 if steps_to_learning_starts is None else max(0, int(steps_to_learning_starts))
    chunks = []
    while left > 0:
        c = min(left, cap - pos)
        if phase is not None:
            c = min(c, SWING_EPISODE_STEPS - phase)
        if to_ls > 0:
            c = min(c, to_ls)
            to_ls -= c
        if phase is not None:
            phase = (phase + c) % SWING_EPISODE_STEPS
        chunks.append(c)
        left -= c
        pos = (pos + c) % cap
    return chunks


class SACTrainer:
    """SAC over a BatchedEnv. Collect: one BatchedEnv.step of every env with the torch actor (uniform actions in [-1, 1] while
    num_timesteps < learning_starts), the transitions into the replay ring; then `gradient_steps` fused gradient steps (default
    num_envs: one per collected transition, the update-to-data ratio of the reference's single env). The env is not pipelined, so
    SwingRacket's terminal reward is complete when its transition is stored. hp: learning_rate, gamma, tau (SAC_DEFAULTS).
    collect_form "fused" (default "torch"): a vector step is collect_steps env steps in tb_sac_collect launches, the learner's flat
    actor vector inside, every row written in place into the ring (its capacity rounded down to whole vector steps; SwingRacket's
    env pipelined; noise keyed by the trainer's seed, not drawn from torch's RNG), then gradient_steps * collect_steps gradient steps.
    What another algorithm with the same loop changes is in the class attributes (tqc.TQCTrainer)."""

    LEARNER, DEFAULTS = FusedSAC, SAC_DEFAULTS
    build_modules = staticmethod(build_sac_modules)
    default_batch = staticmethod(BATCH_SIZE.__getitem__)   # of an env id
    ALGO, NETS = "SAC", "SB3's MlpPolicy [256, 256]"          # the words of the two messages

    def __init__(self, env_id="SwingRacket-v0", num_envs=256, batch_size=None, gradient_steps=None, buffer_size=1_000_000, learning_starts=100, seed=0, params=None,
                 device=None, eval_form="torch", collect_form="torch", collect_steps=1, **hp):
        import torch
        self.torch = torch
        if eval_form not in EVAL_FORMS:
            raise ValueError("%s: eval_form must be one of %s, not %r" % (type(self).__name__, EVAL_FORMS, eval_form))
        self.eval_form = eval_form
        if collect_form not in COLLECT_FORMS:
            raise ValueError("%s: collect_form must be one of %s, not %r" % (type(self).__name__, COLLECT_FORMS, collect_form))
        if int(collect_steps) < 1:
            raise ValueError("%s: collect_steps must be >= 1, not %r" % (type(self).__name__, collect_steps))
        self.collect_form, self.collect_steps = collect_form, int(collect_steps)
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("%s runs on one rank (world size %d): multi-rank %s is not provided" % (type(self).__name__, dist.get_world_size(), self.ALGO))
        unknown = set(hp) - set(self.DEFAULTS)
        if unknown:
            raise ValueError("%s: unknown hyper-parameters %s (the nets are %s: the kernels are instantiated for that architecture)" % (type(self).__name__, sorted(unknown), self.NETS))
        kind = ENV_IDS[env_id]
        self.env_id, self.kind, self.num_envs = env_id, kind, int(num_envs)
        self.hp = dict(self.DEFAULTS, **hp)
        self.batch_size = int(batch_size or self.default_batch(env_id))
        self.gradient_steps = self.num_envs if gradient_steps is None else int(gradient_steps)
        self.learning_starts = int(learning_starts)
        fused = collect_form == "fused"
        if fused:   # the ring holds whole vector steps: tb_sac_collect writes [S][N] rows in place
            rounded = int(buffer_size) // self.num_envs * self.num_envs
            if rounded < self.num_envs:
                raise ValueError("%s: collect_form='fused' needs a buffer_size of at least num_envs = %d, not %d" % (type(self).__name__, self.num_envs, buffer_size))
            if rounded != int(buffer_size):
                print("%s: collect_form='fused' rounds buffer_size %d down to %d, a multiple of num_envs = %d" % (type(self).__name__, buffer_size, rounded, self.num_envs),
                      file=sys.stderr)
            buffer_size = rounded
        # fused collect on SwingRacket: the launch that ends the episodes parks them for the pipeline's fast-forward
        self.env = BatchedEnv(kind, self.num_envs, device=device, seed=seed, params=params, track_terminal_obs=False, pipeline=fused and kind == ENV_SWING)
        # the fused collect's noise key: from the trainer's seed alone (episode and step live in the env's state words, which a checkpoint holds)
        self._collect_seed = (int(seed) * 0x9E3779B97F4A7C15 + 0x53414343) & 0xFFFFFFFFFFFFFFFF
        self.device = self.env.device
        O, A = self.env.obs_dim, self.env.act_dim
        torch.manual_seed(seed)
        self.actor, self.critic, self.critic_target = (m.to(self.device) for m in self.build_modules(O, A))
        self.log_ent_coef = torch.zeros(1, dtype=torch.float32, device=self.device, requires_grad=True)  # ent_coef "auto": starts at 0
        lr, eps = self.hp["learning_rate"], self.hp["adam_eps"]
        self.opts = (torch.optim.Adam(self.actor.parameters(), lr=lr, eps=eps), torch.optim.Adam(self.critic.parameters(), lr=lr, eps=eps),
                     torch.optim.Adam([self.log_ent_coef], lr=lr, eps=eps))
        self._learner = self.LEARNER(kind, self.actor, self.critic, self.critic_target, self.log_ent_coef, self.opts, self.hp, self.device)
        self.replay = ReplayBuffer(O, A, buffer_size, self.device)
        self.obs = self.env.reset()
        self.num_timesteps = 0
        self.rank = 0
        self._ep_return = torch.zeros(self.num_envs, device=self.device)
        self._ep_stats = torch.zeros(2, dtype=torch.float64, device=self.device)   # finished episodes, the sum of their returns

    # ------------------------------------------------------------------------------------------------------------------ collect
    def collect(self):
        """one step of every env into the replay ring; returns (action, obs, reward, done) of that step"""
        t = self.torch
        with t.no_grad():
            if self.num_timesteps < self.learning_starts:
                a = t.rand((self.num_envs, self.env.act_dim), device=self.device) * 2.0 - 1.0
            else:
                a, _ = self.actor.sample(self.obs, t.randn((self.num_envs, self.env.act_dim), device=self.device))
            a = a.contiguous()
            obs, r, d = self.env.step(a)    # not pipelined: r holds SwingRacket's terminal reward already
            if self.env.pipeline:            # (this form on a trainer built for the fused one: the terminal reward is written late)
                self.env.flush()
            df = d.float()
            self.replay.add(self.obs, obs, a, r, df)   # (a done row's obs is the next episode's first: its bootstrap is selected away)
            self._ep_return += r
            self._ep_stats[0] += df.sum()
            self._ep_stats[1] += (self._ep_return * df).sum()
            self._ep_return *= 1.0 - df
            self.obs = obs
        self.num_timesteps += self.num_envs
        return a, obs, r, d

    def collect_fused(self, n_steps=None):
        """`n_steps` (default: collect_steps) steps of every env in as few tb_sac_collect launches as plan_collect_chunks allows, the
        actor inside (uniform actions while num_timesteps < learning_starts), every row written straight into the replay ring:
        no torch forward, no copy, nothing drawn from torch's RNG. Returns (action, obs, reward, done) of the last step, done as
        0.0 / 1.0 (views of the ring)."""
        t, N, O, A = self.torch, self.num_envs, self.env.obs_dim, self.env.act_dim
        S = self.collect_steps if n_steps is None else int(n_steps)
        phase = self.env.phase() if self.kind == ENV_SWING else None
        to_ls = -(-(self.learning_starts - self.num_timesteps) // N)   # env steps until num_timesteps >= learning_starts (ceil)
        out = None
        for c in plan_collect_chunks(self.replay.pos // N, self.replay.capacity // N, S, phase, to_ls):
            uniform = self.num_timesteps < self.learning_starts
            views = self.replay.reserve(c, N)
            self.env.sac_collect(None if uniform else self._learner.pi.flat, c, views, seed=self._collect_seed, uniform=uniform)   # (the vector the kernels train)
            obs, next_obs, action, reward, done = views
            reward, done = reward.view(c, N), done.view(c, N)
            with t.no_grad():
                for k in range(c):   # collect()'s float sums, step by step
                    r, df = reward[k], done[k]
                    self._ep_return += r
                    self._ep_stats[0] += df.sum()
                    self._ep_stats[1] += (self._ep_return * df).sum()
                    self._ep_return *= 1.0 - df
            self.obs = next_obs.view(c, N, O)[c - 1].clone()   # (a copy: the ring's row is overwritten one lap later)
            self.num_timesteps += c * N
            out = (action.view(c, N, A)[c - 1], self.obs, reward[c - 1], done[c - 1])
        return out

    def train(self, gradient_steps=None):
        """`gradient_steps` fused steps on fresh samples; indices and noise are drawn in bulk. Returns the number of steps issued."""
        t, L = self.torch, self._learner
        G, B, A = self.gradient_steps if gradient_steps is None else int(gradient_steps), self.batch_size, self.env.act_dim
        if G < 1:
            return 0
        idx = self.replay.sample(G * B).view(G, B)
        eps = t.randn((G, 2, B, A), device=self.device)
        arrays = self.replay.arrays()
        for k in range(G):
            L.gradient_step(arrays, idx[k], eps[k, 0], eps[k, 1])
        L.publish()
        return G

    def vector_step(self):
        """collect one step of every env, then (past learning_starts) the gradient steps; returns collect's (action, obs, reward, done).
        collect_form "fused": collect_steps env steps (collect_fused), then gradient_steps * collect_steps gradient steps --
        gradient_steps stays "per env step"."""
        if self.collect_form == "fused":
            out = self.collect_fused()
            if self.num_timesteps > self.learning_starts:
                self.train(self.gradient_steps * self.collect_steps)
            return out
        out = self.collect()
        if self.num_timesteps > self.learning_starts:
            self.train()
        return out

    def learn(self, total_timesteps, log=print, log_every=10, schedule=None):
        """vector steps until num_timesteps >= total_timesteps. One read of the device per vector step (losses, entropy
        coefficient, episode statistics); a progress line every `log_every` vector steps. schedule: an evaluation.EvalSchedule,
        asked after every vector step whether an evaluation or a checkpoint is due."""
        history, k = [], 0
        t0, steps0 = time.perf_counter(), self._learner.step
        while self.num_timesteps < total_timesteps:
            self.vector_step()
            k += 1
            row = self.torch.cat([self._learner.stats, self.log_ent_coef.detach().double(), self._ep_stats]).tolist()  # the one read
            self._ep_stats.zero_()
            c = self.env.counters()
            if c["nonfinite_states"]:
                raise StepperError("vector step %d: %d env states went non-finite" % (k, c["nonfinite_states"]))
            stats = {"timesteps": self.num_timesteps, "critic_loss": row[0], "actor_loss": row[1], "mean_logp": row[2], "ent_coef": math.exp(row[4]),
                     "episodes": row[5], "mean_episode_reward": row[6] / max(row[5], 1.0), "gradient_steps": self._learner.step}
            history.append(stats)
            if k % max(1, int(log_every)) == 0 or self.num_timesteps >= total_timesteps:
                now = time.perf_counter()
                recent = history[-max(1, int(log_every)):]
                ep = sum(h["episodes"] for h in recent)
                rew = sum(h["mean_episode_reward"] * h["episodes"] for h in recent) / max(ep, 1.0)
                stats["gradient_steps_per_s"] = (self._learner.step - steps0) / max(now - t0, 1e-9)
                if log:
                    log("timesteps %10d  episodes %7d  mean episode reward %8.3f  ent_coef %.4f  critic loss %.4g  actor loss %.4g  %.0f gradient steps/s"
                        % (self.num_timesteps, ep, rew, stats["ent_coef"], stats["critic_loss"], stats["actor_loss"], stats["gradient_steps_per_s"]))
                t0, steps0 = now, self._learner.step
            if schedule is not None:
                schedule.after_rollout(self)
        return history

    def evaluate(self, n_steps=None, deterministic=False):
        """mean episode reward over n_steps more steps of the same envs (default: 26, one SwingRacket episode; 1000 on Tennisbot)"""
        t = self.torch
        n_steps = n_steps or (26 if self.kind == ENV_SWING else 1000)
        total, eps = t.zeros((), device=self.device), t.zeros((), device=self.device)
        with t.no_grad():
            for _ in range(int(n_steps)):
                if deterministic:
                    a = self.actor.mean_action(self.obs)
                else:
                    a, _ = self.actor.sample(self.obs, t.randn((self.num_envs, self.env.act_dim), device=self.device))
                self.obs, r, d = self.env.step(a.contiguous())
                if self.env.pipeline:   # (a trainer built for the fused collect: SwingRacket's terminal reward is written late)
                    self.env.flush()
                total += r.sum(); eps += d.float().sum()
        self._ep_return.zero_()
        return float(total) / max(float(eps), 1.0)

    def evaluate_episodes(self, n_episodes=64, deterministic=False, n_envs=64, form=None):
        """Mean return over n_episodes WHOLE episodes of the current actor: {episodes, mean, std, min, max, mean_length}.
        form (default: the constructor's eval_form) "torch": evaluation.evaluate_actor_episodes. A separate, unpipelined env batch
        with the trainer's engine parameters is stepped by the torch actor until every env has finished its first episode;
        the noise comes from a torch.Generator of its own. "fused": evaluation.ActorEvaluator, every episode of a batch in ONE
        launch with the learner's flat actor vector inside (tb_sac_evaluate), the noise keyed in the kernel. Either way the
        training envs, self.obs and torch's global RNG are not touched."""
        from .evaluation import EVAL_ENV_ID_BASE, ActorEvaluator, evaluate_actor_episodes
        t = self.torch
        form = self.eval_form if form is None else form
        if form not in EVAL_FORMS:
            raise ValueError("evaluate_episodes: form must be one of %s, not %r" % (EVAL_FORMS, form))
        if form == "fused":
            fe = getattr(self, "_eval_fused", None)
            if fe is None or fe.n_envs != int(n_envs):
                if fe is not None:
                    fe.close()
                fe = self._eval_fused = ActorEvaluator(self.kind, int(n_envs), seed=self.env.seed + 1000003, params=self.env.params, device=self.device)
            if fe.env.params.racket_scale != self.env.params.racket_scale:
                fe.set_racket_scale(self.env.params.racket_scale)
            return fe.evaluate(self._learner.pi.flat, n_episodes, deterministic=deterministic)   # (the vector the kernels train: nothing to repack)
        ev = getattr(self, "_eval_env", None)
        if ev is None or ev.num_envs != int(n_envs):
            ev = self._eval_env = BatchedEnv(self.kind, int(n_envs), device=self.device, seed=self.env.seed + 1000003, env_id_base=EVAL_ENV_ID_BASE,
                                             params=self.env.params, track_terminal_obs=False, pipeline=False)
            self._eval_gen = t.Generator(device=self.device)
            self._eval_gen.manual_seed(self.env.seed + 1000003)
        if ev.params.racket_scale != self.env.params.racket_scale:
            ev.set_racket_scale(self.env.params.racket_scale)
        if deterministic:
            act = self.actor.mean_action
        else:
            act = lambda obs: self.actor.sample(obs, t.randn((ev.num_envs, ev.act_dim), device=self.device, generator=self._eval_gen))[0]  # noqa: E731
        return evaluate_actor_episodes(ev, act, n_episodes)

    def save(self, path):
        """the nets, the three optimisers, log_ent_coef, num_timesteps, the env batch's state words and the replay ring with its cursor"""
        self._learner.publish()
        w, d = self.env.get_state_words()
        self.torch.save({"actor": self.actor.state_dict(), "critic": self.critic.state_dict(), "critic_target": self.critic_target.state_dict(),
                         "optimizers": [o.state_dict() for o in self.opts], "log_ent_coef": self.log_ent_coef.detach().cpu(), "num_timesteps": self.num_timesteps,
                         "env_words": w.cpu(), "env_done": d.cpu(), "replay": self.replay.state_dict(), "ep_return": self._ep_return.cpu(), "hp": self.hp}, path)

    def load(self, path):
        t = self.torch
        ck = t.load(path, map_location=self.device, weights_only=True)
        self.actor.load_state_dict(ck["actor"]); self.critic.load_state_dict(ck["critic"]); self.critic_target.load_state_dict(ck["critic_target"])
        for o, sd in zip(self.opts, ck["optimizers"]):
            o.load_state_dict(sd)
        with t.no_grad():
            self.log_ent_coef.copy_(ck["log_ent_coef"].to(self.device))
        self._learner.adopt()
        self.num_timesteps = int(ck["num_timesteps"])
        self.env.set_state_words(ck["env_words"].to(self.device), ck["env_done"].to(self.device))
        self.obs = self.env.observe().clone()
        self.replay.load_state_dict(ck["replay"])
        self._ep_return.copy_(ck["ep_return"].to(self.device))
        return self
