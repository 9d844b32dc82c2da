"""Evolution strategies on the GPU: the counterpart of the reference's `train_es.py` / `evaluate_es.py` /
`tennisbot/ES/*` (default multi-process path, `--threads -1`).

The population's episodes run in ONE kernel launch (tb_es_evaluate, csrc/tb_es.hpp): every env steps its whole episode with its
member's GatedCNN and a fresh float64 observation normaliser inside the loop, exactly what `fitness_static`
(tennisbot/ES/fitness_functions.py:17-159) computes per episode. Around it, in torch on the device: the noise, the population
(`pack_population`), the mean over repeats and the update of `evolution_strategy_static.py:124-250`. Nothing syncs with the host
but the log line.

Two defined deviations from the reference's update:
  1. a generation whose elite fitness has std == 0 leaves the weights as they are and reports it (`skipped`); the reference
     divides by zero and writes NaN weights;
  2. NaN fitness differences rank below every number (the reference's argsort puts NaN first in descending order).
Noise comes from a seeded torch generator on the device: the reference's np.random stream is not reproduced.
"""
import math

import numpy as np

from .params import ACT_DIM, ENV_SWING, OBS_DIM
from .stepper import ENV_IDS, BatchedEnv

HISTORY = 8  # fitness_functions.py HISTORY_LEN: the network sees the last 8 normalised observations


def es_floats(obs_dim, act_dim):
    """GatedCNN parameter count: 766 for SwingRacket-v0 (O = A = 6), 858 for Tennisbot-v0 (O = 12, A = 2)"""
    return 2 * (8 * obs_dim * 2 + 8) + 2 * (12 * 8 * 2 + 12) + act_dim * 12 * 2 + act_dim


def _module():
    import torch
    from torch import nn

    class GatedCNN(nn.Module):
        """tennisbot/ES/policies.py:59-130: three dilated kernel-2 convolutions, the first two gated (tanh * sigmoid).
        Input (..., O, 8) -- the last 8 normalised observations as channels x time -- output (..., A). Parameter order
        (nn.utils.parameters_to_vector) is the C ABI's: conv_0, conv_gate_0, conv_1, conv_gate_1, conv_2, weight then bias."""

        def __init__(self, obs_dim, act_dim):
            super().__init__()
            self.obs_dim, self.act_dim = obs_dim, act_dim
            self.conv_0 = nn.Conv1d(obs_dim, 8, kernel_size=2, dilation=1)
            self.conv_gate_0 = nn.Conv1d(obs_dim, 8, kernel_size=2, dilation=1)
            self.conv_1 = nn.Conv1d(8, 12, kernel_size=2, dilation=2)
            self.conv_gate_1 = nn.Conv1d(8, 12, kernel_size=2, dilation=2)
            self.conv_2 = nn.Conv1d(12, act_dim, kernel_size=2, dilation=4)

        def forward(self, x):
            lead = x.shape[:-2]
            x = x.reshape((-1,) + tuple(x.shape[-2:]))
            h = torch.tanh(self.conv_0(x)) * torch.sigmoid(self.conv_gate_0(x))
            h = torch.tanh(self.conv_1(h)) * torch.sigmoid(self.conv_gate_1(h))
            return self.conv_2(h)[..., 0].reshape(tuple(lead) + (self.act_dim,))

        def get_weights(self):
            return nn.utils.parameters_to_vector(self.parameters()).detach()

        def set_weights(self, w):
            nn.utils.vector_to_parameters(torch.as_tensor(w, dtype=self.conv_0.weight.dtype), self.parameters())
            return self

    return GatedCNN


def GatedCNN(obs_dim, act_dim):  # noqa: N802 (a class, built on first use so that importing this module does not import torch)
    return _module()(obs_dim, act_dim)


def initial_weights(env_kind, seed=0):
    """torch's default Conv1d initialisation of GatedCNN(O, A) under a seeded CPU generator, as a float32 vector"""
    import torch
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        return GatedCNN(OBS_DIM[env_kind], ACT_DIM[env_kind]).get_weights().float()


def pack_population(w, eps, sigma, stride=None):
    """Members [w + sigma eps_0, ..., w + sigma eps_{p-1}, w - sigma eps_0, ..., w - sigma eps_{p-1}] as rows of a [2p, stride]
    float32 tensor on w's device (zero-padded; stride: a multiple of 4, default the smallest >= P) -- tb_es_evaluate's layout."""
    import torch
    p, P = eps.shape
    stride = (P + 3) // 4 * 4 if stride is None else int(stride)
    if stride < P or stride % 4:
        raise ValueError("stride must be a multiple of 4 and >= %d" % P)
    out = torch.zeros((2 * p, stride), dtype=torch.float32, device=w.device)
    d = eps.to(torch.float32) * float(sigma)
    out[:p, :P] = w + d
    out[p:, :P] = w - d
    return out


def elite_order(diff, k):
    """indices of the top k of `diff` in descending order: a stable sort (ties keep index order), NaN below every number"""
    import torch
    nan = torch.isnan(diff)
    key = torch.where(nan, torch.full_like(diff, -math.inf), diff)
    idx = torch.sort(key, descending=True, stable=True).indices
    idx = idx[torch.sort(nan[idx].to(torch.int8), stable=True).indices]
    return idx[:k]


def es_update(w, eps, r_pos, r_neg, lr, elite):
    """evolution_strategy_static.py:124-250: the elite pairs by r_pos - r_neg, std (ddof 0) of their r_neg and r_pos together,
    w + lr / (std K) E^T (r_pos - r_neg). std == 0 leaves w as it is (deviation 1). Returns (w, info) without a host sync;
    info: elite indices, std, skipped (0-d bool tensor)."""
    import torch
    idx = elite_order(r_pos - r_neg, elite)
    rp, rn = r_pos[idx], r_neg[idx]
    std = torch.cat([rn, rp]).std(unbiased=False)
    skipped = std == 0
    step = (eps[idx].to(torch.float32).t() @ (rp - rn)) * (float(lr) / (std * float(elite)))
    return torch.where(skipped, w, w + step), dict(elite=idx, std=std, skipped=skipped)


def fitness(returns):
    """a member's fitness: the mean of its repeats' float64 returns [M, R], cast to float32"""
    import torch
    return returns.mean(dim=1).to(torch.float32)


def schedule(lr, sigma, decay):
    """evolution_strategy_static.py: lr *= decay while lr > 0.001; sigma *= 0.999 while sigma > 0.01"""
    if lr > 0.001:
        lr *= decay
    if sigma > 0.01:
        sigma *= 0.999
    return lr, sigma


class ESTrainer:
    """The reference's EvolutionStrategyStatic on one GPU. Each generation evaluates 2 popsize members x `repeats` episodes in one
    BatchedEnv of 2 popsize repeats envs (SwingRacket-v0 with the pipeline on); member m's episodes are envs
    [m repeats, (m + 1) repeats)."""

    def __init__(self, env_id, popsize=200, repeats=10, elite=66, sigma=0.1, lr=0.2, decay=0.995, seed=0, options=None, device=None,
                 params=None, weights=None):
        import torch
        self.torch = torch
        self.env_id = env_id
        self.kind = ENV_IDS[env_id] if isinstance(env_id, str) else int(env_id)
        self.popsize, self.repeats, self.elite = int(popsize), int(repeats), int(elite)
        if not 1 <= self.elite <= self.popsize:
            raise ValueError("elite must be in [1, popsize]")
        self.sigma, self.lr, self.decay = float(sigma), float(lr), float(decay)
        self.seed = int(seed)
        self.params, self.options = params, options
        self.env = BatchedEnv(self.kind, 2 * self.popsize * self.repeats, device=device, seed=self.seed, params=params,
                              pipeline=self.kind == ENV_SWING, options=options)
        self.device = self.env.device
        self.P = self.env.es_floats()
        self.stride = (self.P + 3) // 4 * 4
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(self.seed)
        w = initial_weights(self.kind, self.seed) if weights is None else torch.as_tensor(weights, dtype=torch.float32)
        self.w = w.to(self.device).reshape(self.P).clone()
        self.generation = 0
        self.last = None
        self._eval_envs = {}

    def step(self):
        """one generation; returns the info dict (device tensors: fitness [2p], lengths [2p, R], elite, std, skipped)"""
        t = self.torch
        eps = t.randn((self.popsize, self.P), generator=self.gen, device=self.device, dtype=t.float32)
        pop = pack_population(self.w, eps, self.sigma, self.stride)
        ret, length = self.env.es_evaluate(pop, self.repeats)
        fit = fitness(ret)
        self.w, info = es_update(self.w, eps, fit[:self.popsize], fit[self.popsize:], self.lr, self.elite)
        self.lr, self.sigma = schedule(self.lr, self.sigma, self.decay)
        self.generation += 1
        info.update(fitness=fit, lengths=length, eps=eps)
        self.last = info
        return info

    def log(self):
        """the log line's numbers (this is the one host sync)"""
        i = self.last
        f = i["fitness"].double()
        return dict(generation=self.generation, mean=float(f.mean()), max=float(f.max()), elite_std=float(i["std"]),
                    skipped=bool(i["skipped"]), steps=int(i["lengths"].sum()), lr=self.lr, sigma=self.sigma)

    def evaluate(self, weights=None, episodes=100):
        """evaluate_es.py: `episodes` episodes of one weight vector (default: the current one), each with a fresh normaliser.
        Returns the float64 returns [episodes] on the device."""
        t = self.torch
        w = self.w if weights is None else t.as_tensor(weights, dtype=t.float32).to(self.device).reshape(self.P)
        episodes = int(episodes)
        env = self._eval_envs.get(episodes)
        if env is None:
            env = BatchedEnv(self.kind, episodes, device=self.device, seed=self.seed + 1, params=self.params,
                             pipeline=self.kind == ENV_SWING, options=self.options)
            self._eval_envs[episodes] = env
        pop = t.zeros((1, self.stride), dtype=t.float32, device=self.device)
        pop[0, :self.P] = w
        return env.es_evaluate(pop, episodes)[0][0]

    def save(self, path):
        np.savez(path, weights=self.w.cpu().numpy(), env_id=str(self.env_id), generation=self.generation, lr=self.lr, sigma=self.sigma,
                 popsize=self.popsize, repeats=self.repeats, elite=self.elite, decay=self.decay, seed=self.seed)

    def load(self, path):
        z = np.load(path, allow_pickle=False)
        w = z["weights"].astype(np.float32)
        if w.shape != (self.P,):
            raise ValueError("%s holds %s weights, this env needs (%d,)" % (path, w.shape, self.P))
        self.w = self.torch.from_numpy(w).to(self.device)
        self.generation, self.lr, self.sigma = int(z["generation"]), float(z["lr"]), float(z["sigma"])
        return self

    def close(self):
        for env in [self.env] + list(self._eval_envs.values()):
            env.close()
