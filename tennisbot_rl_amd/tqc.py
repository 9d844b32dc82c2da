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
nothing in a gradient step synchronises with the host; every `done` is a true terminal. There is one learner and one trainer:
`FusedTQC` is `FusedSAC` with the tb_tqc_ entry points, y of shape [B, 46] and the words of TQC's nets in its class attributes,
and a check of the three counts before anything else; the stages, the workspace, the flat vectors, adopt / publish, adam, polyak
and gradient_step are FusedSAC's own code. `TQCTrainer` is `SACTrainer` with FusedTQC, build_tqc_modules and batch 256 as its
attributes. There is no torch fallback for the gradient step: a refused call raises. One rank only.
"""
import copy

from .sac import ACTOR_NAMES, CRITIC_NAMES, HIDDEN, SAC_DEFAULTS, FusedSAC, ReplayBuffer, SACTrainer, _Flat, build_sac_modules  # noqa: F401  (tests and tools import the names from here)
from .stepper import StepperError

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

    ABI, DEFAULTS, Y_SHAPE = "tb_tqc_", TQC_DEFAULTS, (N_TARGETS,)
    NET, NET_SHAPE = "sb3_contrib's TQC MlpPolicy", "[256, 256] ReLU, %d critics of %d quantiles" % (N_CRITICS, N_QUANTILES)

    def __init__(self, kind, actor, critic, critic_target, log_ent_coef, optimisers, hp, device, n_quantiles=N_QUANTILES, n_critics=N_CRITICS,
                 top_quantiles_to_drop_per_net=TOP_QUANTILES_TO_DROP_PER_NET):
        if (int(n_quantiles), int(n_critics), int(top_quantiles_to_drop_per_net)) != (N_QUANTILES, N_CRITICS, TOP_QUANTILES_TO_DROP_PER_NET):
            raise StepperError("FusedTQC: n_quantiles = %s, n_critics = %s, top_quantiles_to_drop_per_net = %s; the kernels take %d quantiles, %d critics and %d dropped per net"
                               % (n_quantiles, n_critics, top_quantiles_to_drop_per_net, N_QUANTILES, N_CRITICS, TOP_QUANTILES_TO_DROP_PER_NET))
        super().__init__(kind, actor, critic, critic_target, log_ent_coef, optimisers, hp, device)


class TQCTrainer(SACTrainer):
    """TQC over a BatchedEnv: SACTrainer's loop (collect, train, vector_step, learn, evaluate, save, load) around a FusedTQC.
    hp: learning_rate, gamma, tau (TQC_DEFAULTS)."""

    LEARNER, DEFAULTS = FusedTQC, TQC_DEFAULTS
    build_modules = staticmethod(build_tqc_modules)
    default_batch = staticmethod(lambda env_id: BATCH_SIZE)
    ALGO, NETS = "TQC", "sb3_contrib's MlpPolicy [256, 256] with %d quantiles, %d critics, %d dropped per net" % (N_QUANTILES, N_CRITICS, TOP_QUANTILES_TO_DROP_PER_NET)
