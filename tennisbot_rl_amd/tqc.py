"""TQC on the batched envs: the gradient step as HIP kernels (csrc/tb_tqc.hpp on csrc/tb_sac.hpp; C ABI tb_tqc_* in include/tb_stepper.h).

The rule is sb3_contrib 1.8.0's TQC with MlpPolicy at its defaults, which is what the reference's `train_swing.py -s tqc` selects
(train_swing.py:98-99): SAC's actor; two critics [256, 256] ReLU with 25 quantile outputs each; the 2 largest quantiles per net
dropped from the sorted 50 of the targets, 46 kept; lr 3e-4 for actor, critic and log_ent_coef, plain Adam (eps 1e-8), gamma 0.99,
tau 0.005, ent_coef "auto" (log_ent_coef from 0, target entropy -A), batch_size 256, buffer_size 1e6, learning_starts 100. One
gradient step on a batch (s, a, r, s', d), in sb3_contrib's order:

  1. a~, logp = actor(s; eps_pi)                                                             tb_tqc_actor_forward
  2. alpha = exp(log_ent_coef) as it is BEFORE this step's update; gradient of log_ent_coef: -mean(logp - A)
  3. z = sort(concat(Q1t, Q2t)(s', a'))[:46], y[b][j] = r + (1 - d) gamma (z[j] - alpha logp')       tb_tqc_targets
  4. critic loss: the mean over (b, n, i, j) of |tau_i - [delta < 0]| H(delta), delta = y[b][j] - Q_n(s, a)[i],
     tau_i = (i + 0.5) / 25, H the Huber loss at 1; Adam on the critic                       tb_tqc_critic_grad, tb_sac_adam
  5. actor loss mean(alpha logp - Qbar(s, a~)) with the UPDATED critic, Qbar the mean over 25 quantiles and 2 critics;
     Adam on the actor                                                                       tb_tqc_actor_grad, tb_sac_adam
  6. target <- (1 - tau) target + tau critic                                                 (folded into the critic's tb_sac_adam)

Everything else is sac.py's: the kernels read log_ent_coef on the device, so its Adam step is issued last; the noise is an input;
nothing in a gradient step synchronises with the host; every `done` is a true terminal. `FusedTQC` is `FusedSAC` with TQC's
stages (it inherits the flat vectors, adopt / publish, adam, polyak and gradient_step), `TQCTrainer` is `SACTrainer` around it.
There is no torch fallback for the gradient step: a refused call raises. One rank only.
"""
import copy

from .learner import flatten_parameters
from .sac import ACTOR_NAMES, CRITIC_NAMES, HIDDEN, SAC_DEFAULTS, TB_SAC_ACTOR, TB_SAC_CRITIC, FusedSAC, ReplayBuffer, SACTrainer, _Flat, build_sac_modules
from .stepper import ACT_DIM, ENV_IDS, OBS_DIM, BatchedEnv, StepperError, _check, load_library

N_QUANTILES, N_CRITICS, TOP_QUANTILES_TO_DROP_PER_NET = 25, 2, 2
N_TARGETS = N_CRITICS * (N_QUANTILES - TOP_QUANTILES_TO_DROP_PER_NET)   # 46
TQC_DEFAULTS = dict(SAC_DEFAULTS)
BATCH_SIZE = 256   # train_swing.py:98-99 passes none: sb3_contrib's default (unlike the reference's SAC line, which sets 1100)
# launches of one gradient_step: actor forward 5 (gather, three tile launches, sample), targets 9 (gather, actor 4, the two targets'
# three layers in 3, sort and y), critic gradient 11 (gather, forward 3, loss, the loss's sum, backward 2, weight gradients 3), its
# Adam + Polyak 1, actor gradient 13 (critics forward 3, loss, their backward 3, the head's backward, the actor's backward 2 and
# weight gradients 3), Adam 2
LAUNCHES_PER_STEP = 41


def build_tqc_modules(obs_dim, act_dim, n_quantiles=N_QUANTILES, n_critics=N_CRITICS):
    """(actor, critic, critic_target): torch modules whose named_parameters() are sb3_contrib's TQC MlpPolicy names and shapes.
    The actor is build_sac_modules'; the critic's `forward(obs, action)` returns the quantiles [n, n_critics, n_quantiles]."""
    import torch
    from torch import nn

    class Critic(nn.Module):
        def __init__(self):
            super().__init__()
            for q in range(n_critics):
                setattr(self, "qf%d" % q, nn.Sequential(nn.Linear(obs_dim + act_dim, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, n_quantiles)))

        def forward(self, obs, action):
            x = torch.cat([obs, action], 1)
            return torch.stack([getattr(self, "qf%d" % q)(x) for q in range(n_critics)], 1)

    actor, critic = build_sac_modules(obs_dim, act_dim)[0], Critic()
    target = copy.deepcopy(critic)
    for p in target.parameters():
        p.requires_grad_(False)
    return actor, critic, target


class FusedTQC(FusedSAC):
    """TQC's gradient step on the device for (actor, critic, critic_target, log_ent_coef) and their three Adam optimisers
    `optimisers = (actor_opt, critic_opt, ent_opt)`. hp: gamma, tau (TQC_DEFAULTS); lr, betas and eps are the optimisers' own; hp
    stays the CALLER'S dict, as in FusedSAC. The kernels are instantiated for 25 quantiles, 2 critics and 2 dropped per net."""

    def __init__(self, kind, actor, critic, critic_target, log_ent_coef, optimisers, hp, device, n_quantiles=N_QUANTILES, n_critics=N_CRITICS,
                 top_quantiles_to_drop_per_net=TOP_QUANTILES_TO_DROP_PER_NET):
        import torch
        if (int(n_quantiles), int(n_critics), int(top_quantiles_to_drop_per_net)) != (N_QUANTILES, N_CRITICS, TOP_QUANTILES_TO_DROP_PER_NET):
            raise StepperError("FusedTQC: n_quantiles = %s, n_critics = %s, top_quantiles_to_drop_per_net = %s; the kernels take %d quantiles, %d critics and %d dropped per net"
                               % (n_quantiles, n_critics, top_quantiles_to_drop_per_net, N_QUANTILES, N_CRITICS, TOP_QUANTILES_TO_DROP_PER_NET))
        self.torch, self.kind, self.hp = torch, int(kind), hp
        self.actor, self.critic, self.critic_target, self.log_ent_coef = actor, critic, critic_target, log_ent_coef
        for k, v in TQC_DEFAULTS.items():
            hp.setdefault(k, v)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise StepperError("FusedTQC needs a GPU (there is no CPU fallback)")
        self.lib = load_library()
        self.O, self.A = OBS_DIM[self.kind], ACT_DIM[self.kind]
        want = {"actor": ACTOR_NAMES, "critic": CRITIC_NAMES, "critic_target": CRITIC_NAMES}
        sets = {}
        for what, module, which in (("actor", actor, TB_SAC_ACTOR), ("critic", critic, TB_SAC_CRITIC), ("critic_target", critic_target, TB_SAC_CRITIC)):
            named = list(module.named_parameters())
            n = self.lib.tb_tqc_param_floats(self.kind, which)
            if n < 0:
                _check(self.lib, n, "tb_tqc_param_floats")
            if tuple(k for k, _ in named) != want[what] or sum(p.numel() for _, p in named) != n:
                raise StepperError("FusedTQC: the %s is not sb3_contrib's TQC MlpPolicy net for this env kind (%d parameters in %d tensors; the kernels take %d: [256, 256] ReLU, "
                                   "%d critics of %d quantiles)" % (what, sum(p.numel() for _, p in named), len(named), n, N_CRITICS, N_QUANTILES))
            if any(p.device != self.device and p.device.type != "cuda" for _, p in named):
                raise StepperError("FusedTQC: the %s is not on a GPU" % what)
            sets[what] = [p for _, p in named]
        if tuple(log_ent_coef.shape) != (1,) or log_ent_coef.dtype != torch.float32 or log_ent_coef.device.type != "cuda":
            raise StepperError("FusedTQC: log_ent_coef must be a float32 tensor of shape [1] on the GPU")
        actor_opt, critic_opt, ent_opt = optimisers
        self.pi = _Flat(torch, sets["actor"], flatten_parameters(actor), actor_opt, "actor")
        self.q = _Flat(torch, sets["critic"], flatten_parameters(critic), critic_opt, "critic")
        self.qt = _Flat(torch, sets["critic_target"], flatten_parameters(critic_target), None, "critic_target")
        self.ent = _Flat(torch, [log_ent_coef], log_ent_coef.data, ent_opt, "entropy coefficient")
        self.stats = torch.zeros(4, dtype=torch.float64, device=self.device)  # critic loss, actor loss, mean logp, d log_ent_coef
        self.step = 0
        self._ws = self._batch = self._pi_batch = None   # _pi_batch: the batch whose actor activations the workspace holds
        self.adopt()

    def workspace(self, batch):
        need = self.lib.tb_tqc_workspace_bytes(self.kind, int(batch))
        if need < 0:
            _check(self.lib, int(need), "tb_tqc_workspace_bytes")
        if self._ws is None or self._ws.numel() * 8 < need:
            self._ws = self.torch.zeros((need + 7) // 8, dtype=self.torch.float64, device=self.device)
        if self._batch != int(batch):   # the regions' offsets scale with the batch: what an earlier stage kept is gone
            B = self._batch = int(batch)
            self._pi_batch = None
            e = lambda *s: self.torch.empty(s, dtype=self.torch.float32, device=self.device)  # noqa: E731
            self.act_pi, self.logp_pi, self.y = e(B, self.A), e(B), e(B, N_TARGETS)
        return self._ws

    # --------------------------------------------------------------------------------------------------------------- the stages
    def actor_forward(self, obs, idx, eps, act_out=None, logp_out=None):
        """(a~ [B, A], logp [B]) of the actor on obs[idx] with the noise eps [B, A]; keeps the activations for actor_gradient"""
        B = int(self._index(idx).numel())
        ws = self.workspace(B)
        act_out, logp_out = self.act_pi if act_out is None else act_out, self.logp_pi if logp_out is None else logp_out
        obs, eps = self._float(obs, "obs"), self._float(eps, "eps", (B, self.A))
        _check(self.lib, self.lib.tb_tqc_actor_forward(self.kind, self._dev(), self._stream(), obs.data_ptr(), int(obs.shape[0]), idx.data_ptr(), B, self.pi.flat.data_ptr(),
                                                       eps.data_ptr(), self._float(act_out, "act_out", (B, self.A)).data_ptr(), self._float(logp_out, "logp_out", (B,)).data_ptr(),
                                                       ws.data_ptr(), ws.numel() * 8), "tb_tqc_actor_forward")
        self._pi_batch = B
        return act_out, logp_out

    def targets(self, next_obs, reward, done, idx, eps_next, y=None):
        """y [B, 46]: the truncated target distribution of every row"""
        B = int(self._index(idx).numel())
        ws = self.workspace(B)
        y = self.y if y is None else y
        next_obs, n = self._float(next_obs, "next_obs"), int(next_obs.shape[0])
        _check(self.lib, self.lib.tb_tqc_targets(self.kind, self._dev(), self._stream(), next_obs.data_ptr(), self._float(reward, "reward", (n,)).data_ptr(),
                                                 self._float(done, "done", (n,)).data_ptr(), n, idx.data_ptr(), B, self.pi.flat.data_ptr(), self.qt.flat.data_ptr(),
                                                 self.log_ent_coef.data_ptr(), self._float(eps_next, "eps_next", (B, self.A)).data_ptr(), float(self.hp["gamma"]),
                                                 self._float(y, "y", (B, N_TARGETS)).data_ptr(), ws.data_ptr(), ws.numel() * 8), "tb_tqc_targets")
        return y

    def critic_gradient(self, obs, action, idx, y):
        """the critic's gradient into self.q.grad; stats[0] = the critic loss"""
        B = int(self._index(idx).numel())
        ws = self.workspace(B)
        obs, n = self._float(obs, "obs"), int(obs.shape[0])
        _check(self.lib, self.lib.tb_tqc_critic_grad(self.kind, self._dev(), self._stream(), obs.data_ptr(), self._float(action, "action", (n, self.A)).data_ptr(), n, idx.data_ptr(),
                                                     B, self.q.flat.data_ptr(), self._float(y, "y", (B, N_TARGETS)).data_ptr(), self.q.grad.data_ptr(), self.stats.data_ptr(),
                                                     ws.data_ptr(), ws.numel() * 8), "tb_tqc_critic_grad")
        return self.q.grad

    def actor_gradient(self, batch, eps):
        """the actor's gradient into self.pi.grad and log_ent_coef's into self.ent.grad, on the batch of the last actor_forward"""
        B = int(batch)
        if B != self._pi_batch:
            raise ValueError("actor_gradient: the workspace holds %s, not an actor_forward of %d rows (a stage at another batch size in between overwrites it)"
                             % ("no actor_forward" if self._pi_batch is None else "an actor_forward of %d rows" % self._pi_batch, B))
        ws = self.workspace(B)
        _check(self.lib, self.lib.tb_tqc_actor_grad(self.kind, self._dev(), self._stream(), B, self.pi.flat.data_ptr(), self.q.flat.data_ptr(), self.log_ent_coef.data_ptr(),
                                                    self._float(eps, "eps", (B, self.A)).data_ptr(), self.pi.grad.data_ptr(), self.ent.grad.data_ptr(), self.stats.data_ptr(),
                                                    ws.data_ptr(), ws.numel() * 8), "tb_tqc_actor_grad")
        return self.pi.grad, self.ent.grad


class TQCTrainer(SACTrainer):
    """TQC over a BatchedEnv: SACTrainer's loop (collect, train, vector_step, learn, evaluate, save, load) around a FusedTQC.
    hp: learning_rate, gamma, tau (TQC_DEFAULTS)."""

    def __init__(self, env_id="SwingRacket-v0", num_envs=256, batch_size=None, gradient_steps=None, buffer_size=1_000_000, learning_starts=100, seed=0, params=None,
                 device=None, **hp):
        import torch
        self.torch = torch
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("TQCTrainer runs on one rank (world size %d): multi-rank TQC is not provided" % dist.get_world_size())
        unknown = set(hp) - set(TQC_DEFAULTS)
        if unknown:
            raise ValueError("TQCTrainer: unknown hyper-parameters %s (the nets are sb3_contrib's MlpPolicy [256, 256] with 25 quantiles, 2 critics, 2 dropped per net: the "
                             "kernels are instantiated for that architecture)" % sorted(unknown))
        kind = ENV_IDS[env_id]
        self.env_id, self.kind, self.num_envs = env_id, kind, int(num_envs)
        self.hp = dict(TQC_DEFAULTS, **hp)
        self.batch_size = int(batch_size or BATCH_SIZE)
        self.gradient_steps = self.num_envs if gradient_steps is None else int(gradient_steps)
        self.learning_starts = int(learning_starts)
        self.env = BatchedEnv(kind, self.num_envs, device=device, seed=seed, params=params, track_terminal_obs=False, pipeline=False)
        self.device = self.env.device
        O, A = self.env.obs_dim, self.env.act_dim
        torch.manual_seed(seed)
        self.actor, self.critic, self.critic_target = (m.to(self.device) for m in build_tqc_modules(O, A))
        self.log_ent_coef = torch.zeros(1, dtype=torch.float32, device=self.device, requires_grad=True)  # ent_coef "auto": starts at 0
        lr, eps = self.hp["learning_rate"], self.hp["adam_eps"]
        self.opts = (torch.optim.Adam(self.actor.parameters(), lr=lr, eps=eps), torch.optim.Adam(self.critic.parameters(), lr=lr, eps=eps),
                     torch.optim.Adam([self.log_ent_coef], lr=lr, eps=eps))
        self._learner = FusedTQC(kind, self.actor, self.critic, self.critic_target, self.log_ent_coef, self.opts, self.hp, self.device)
        self.replay = ReplayBuffer(O, A, buffer_size, self.device)
        self.obs = self.env.reset()
        self.num_timesteps = 0
        self.rank = 0
        self._ep_return = torch.zeros(self.num_envs, device=self.device)
        self._ep_stats = torch.zeros(2, dtype=torch.float64, device=self.device)   # finished episodes, the sum of their returns
