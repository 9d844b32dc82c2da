"""Evolution strategies on the MlpPolicy actor: es.py's update on the network that PPO / TRPO train, a whole population per launch.

es.py evolves the reference's GatedCNN, whose members cannot share a matrix-core tile. The fused MlpPolicy
kernels are that tile: 16 envs against one weight fragment. tb_policy_evaluate_members (csrc/tb_kernels.hpp,
tb_policy_evaluate_members_kernel) runs every env's whole episode with its MEMBER's blob, so a generation of 2 popsize members x
`repeats` episodes is one launch, and a run can start from a trained checkpoint.

What evolves is the ACTOR: the parameters on the pi path (`actor_parameters`). The value tower and log_std are carried along
unchanged from the template policy -- ES has no use for a critic, and with deterministic=True (the default) none for log_std.
The update, the elite order, the fitness, the schedule, the population order [w + sigma eps_0 ..., w - sigma eps_0 ...] and the two
deviations from the reference (a zero elite std skips the update; NaN ranks last) are es.py's own functions.

This is the project's actor, not the reference's unused 128-64 `MLP` class (tennisbot/ES/policies.py).
"""
import os

from .es import es_update, fitness, pack_population, schedule
from .params import ACT_DIM, ENV_SWING, ENV_TENNIS, NET_DEFAULT, NET_MLP64, NET_NAMES, NET_TUNED, OBS_DIM
from .stepper import ENV_IDS, BatchedEnv

ACTOR_PREFIXES = ("features_extractor.", "policy_net.", "action_net.")  # the pi path; value_net_body / value_net / log_std are not on it
MEMBER_GRANULE = 16  # tb_policy_member_granule(): the envs of one tower wave (checked against the library when an env exists)


def actor_parameters(policy):
    """The parameters on the pi path, in named_parameters() order: the tuned net's shared extractor (once), then policy_net, then
    action_net. log_std and the value tower are not part of it."""
    return [p for name, p in policy.named_parameters() if name.startswith(ACTOR_PREFIXES)]


def actor_flat(policy):
    """the actor as one float32 vector [Pa] on the policy's device (a copy)"""
    import torch
    return torch.cat([p.detach().reshape(-1).float() for p in actor_parameters(policy)])


def set_actor_flat(policy, vec):
    """write a [Pa] vector back into the actor's parameters, in place; returns the policy"""
    import torch
    params = actor_parameters(policy)
    vec = torch.as_tensor(vec, dtype=torch.float32).reshape(-1)
    if vec.numel() != sum(p.numel() for p in params):
        raise ValueError("the actor has %d parameters, got %d" % (sum(p.numel() for p in params), vec.numel()))
    off = 0
    with torch.no_grad():
        for p in params:
            p.copy_(vec[off:off + p.numel()].reshape(p.shape).to(p.device))
            off += p.numel()
    return policy


def _members_index(policy):
    """pack_policy's gather index, re-aimed: a blob position whose source is an actor parameter points into the member's row
    [0, Pa), every other (value tower, log_std, the padding zero) into the template's source behind it, at Pa + its old place."""
    import torch
    from .ppo import _blob_layers, pack_policy
    dev = policy.log_std.device
    cache = getattr(policy, "_pack_members_index", None)
    if cache is not None and cache.device == dev:
        return cache
    base = getattr(policy, "_pack_index", None)
    if base is None or base.device != dev:
        pack_policy(policy)   # (builds and caches the index)
        base = policy._pack_index
    flat_off, off = {}, 0
    for p in actor_parameters(policy):
        flat_off[id(p)] = off
        off += p.numel()
    pa = off
    n_src = sum(m.out_features * (m.in_features + 1) for m, _ in _blob_layers(policy)) + policy.log_std.numel() + 1
    remap = torch.arange(n_src, dtype=torch.long) + pa
    off = 0
    for m, _ in _blob_layers(policy):   # the source's order: per layer [bias, weight (out x in) row-major]
        for t in (m.bias, m.weight):
            if id(t) in flat_off:
                remap[off:off + t.numel()] = torch.arange(t.numel(), dtype=torch.long) + flat_off[id(t)]
            off += t.numel()
    cache = remap.to(dev)[base]
    policy._pack_members_index = cache
    return cache


def pack_policy_members(policy, flat, out=None):
    """[M, B] float32 on flat's device: row m is bit for bit `ppo.pack_policy` of `policy` with its actor set to flat[m] ([M, Pa]);
    the value tower and log_std are `policy`'s. ONE batched gather with a cached index (pack_policy's, re-aimed: _members_index),
    whatever M is. `out`: a preallocated [M, B] tensor to refresh in place."""
    import torch
    from .ppo import _blob_layers
    if flat.dim() != 2:
        raise ValueError("flat must be [M, Pa]")
    idx = _members_index(policy)
    dev = policy.log_std.device
    if flat.device != dev:
        raise ValueError("flat is on %s, the policy on %s" % (flat.device, dev))
    pa = sum(p.numel() for p in actor_parameters(policy))
    if flat.shape[1] != pa:
        raise ValueError("flat must have %d columns (the actor's parameters), got %d" % (pa, flat.shape[1]))
    with torch.no_grad():
        layers = [m for m, _ in _blob_layers(policy)]
        src = torch.cat([t.detach().float().reshape(-1) for m in layers for t in (m.bias, m.weight)] + [policy.log_std.detach().float().reshape(-1), torch.zeros(1, device=dev)])
        both = torch.cat([flat.float(), src.unsqueeze(0).expand(flat.shape[0], -1)], dim=1)
        if out is None:
            return both.index_select(1, idx)
        torch.index_select(both, 1, idx, out=out)
    return out


def build_policy(kind, net=NET_DEFAULT, seed=0):
    """the torch module of (kind, net) with the trainers' architecture defaults, initialised under a seeded CPU generator (the
    global RNG is left alone)"""
    import torch
    from .ppo import SB3_SWING_DEFAULTS, SWING_DEFAULTS, TENNIS_DEFAULTS, TUNED_TENNIS_DEFAULTS, build_actor_critic, build_tuned_actor_critic
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        if net == NET_TUNED:
            return build_tuned_actor_critic(OBS_DIM[kind], ACT_DIM[kind], tuple(TUNED_TENNIS_DEFAULTS["net_arch"]), TUNED_TENNIS_DEFAULTS["extractor_hidden"])
        arch = SB3_SWING_DEFAULTS if net == NET_MLP64 else SWING_DEFAULTS if kind == ENV_SWING else TENNIS_DEFAULTS
        return build_actor_critic(OBS_DIM[kind], ACT_DIM[kind], tuple(arch["net_arch"]))


def load_init(policy, init):
    """init: a state dict; a checkpoint written by the PPO / TRPO trainers or by PolicyESTrainer.save (its "policy" entry); or an
    .npz of SB3-named arrays (tools/export_reference_policy.py, e.g. tests/golden/ppo_swing_policy.npz)"""
    import numpy as np
    import torch
    if isinstance(init, dict):
        policy.load_state_dict(init)
    elif str(init).endswith(".npz"):
        policy.load_sb3_arrays(dict(np.load(init)))
    else:
        policy.load_state_dict(torch.load(init, map_location="cpu", weights_only=True)["policy"])
    return policy


def check_repeats(repeats, granule=MEMBER_GRANULE):
    if int(repeats) < 1 or int(repeats) % granule:
        raise ValueError("repeats must be a positive multiple of the member granule %d (a workgroup's 16 envs share one member's weights), got %d"
                         % (granule, int(repeats)))
    return int(repeats)


class PolicyESTrainer:
    """es.ESTrainer on the MlpPolicy actor. Each generation evaluates 2 popsize members x `repeats` episodes in one BatchedEnv of
    2 popsize repeats envs (SwingRacket-v0 with the pipeline on) by one policy_evaluate_members launch; member m's episodes are
    envs [m repeats, (m + 1) repeats). deterministic=True: members act on their mean (fitness then differs by the weights and the
    episodes' starts alone); False: they sample with the template's log_std. Noise for the population comes from a generator of
    the trainer's own: torch's global RNG is never drawn from."""

    def __init__(self, env_id, net="default", popsize=200, repeats=16, elite=66, sigma=0.1, lr=0.2, decay=0.995, seed=0, deterministic=True, init=None,
                 options=None, device=None, params=None):
        self.repeats = check_repeats(repeats)   # (before any device use)
        self.env_id = env_id
        self.kind = ENV_IDS[env_id] if isinstance(env_id, str) else int(env_id)
        names = {v: k for k, v in NET_NAMES.items()}
        if net not in names:
            raise ValueError("net must be one of %s, not %r" % (sorted(names), net))
        self.net = names[net]
        if (self.net == NET_TUNED and self.kind != ENV_TENNIS) or (self.net == NET_MLP64 and self.kind != ENV_SWING):
            raise ValueError("net %r is not built for %s (tuned: Tennisbot-v0, mlp64: SwingRacket-v0)" % (net, env_id))
        self.popsize, self.elite = int(popsize), int(elite)
        if not 1 <= self.elite <= self.popsize:
            raise ValueError("elite must be in [1, popsize]")
        self.sigma, self.lr, self.decay = float(sigma), float(lr), float(decay)
        self.seed, self.deterministic = int(seed), bool(deterministic)
        self.params, self.options = params, options
        import torch
        self.torch = torch
        self.env = BatchedEnv(self.kind, 2 * self.popsize * self.repeats, device=device, seed=self.seed, params=params, track_terminal_obs=False,
                              pipeline=self.kind == ENV_SWING, options=options)
        check_repeats(self.repeats, self.env.policy_member_granule())
        self.device = self.env.device
        policy = build_policy(self.kind, self.net, self.seed)
        if init is not None:
            load_init(policy, init)
        self.policy = policy.to(self.device)   # the template: its value tower and log_std travel in every member's blob
        self.w = actor_flat(self.policy)
        self.P = int(self.w.numel())
        self.blob_floats = self.env.policy_floats(self.net)
        self._blobs = torch.empty((2 * self.popsize, self.blob_floats), dtype=torch.float32, device=self.device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(self.seed)
        self.noise_seed = (self.seed * 1000003 + 0x4D4C50) & 0xFFFFFFFFFFFFFFFF
        self.generation = 0
        self.last = None
        self._evaluators = {}

    def sample_noise(self):
        """eps [popsize, Pa] from the trainer's generator"""
        t = self.torch
        return t.randn((self.popsize, self.P), generator=self.gen, device=self.device, dtype=t.float32)

    def population(self, eps):
        """the 2 popsize members' blobs [2p, B] for this noise, es.py's order: [w + sigma eps_0 ..., w - sigma eps_0 ...]"""
        pop = pack_population(self.w, eps, self.sigma)
        return pack_policy_members(self.policy, pop[:, :self.P], out=self._blobs)

    def step(self):
        """one generation; returns the info dict (device tensors: fitness [2p], lengths [2p, R], eps, elite, std, skipped)"""
        eps = self.sample_noise()
        ret, length = self.env.policy_evaluate_members(self.population(eps), self.repeats, seed=self.noise_seed, deterministic=self.deterministic, net=self.net)
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

    def current_policy(self):
        """the template with the current actor written into it"""
        return set_actor_flat(self.policy, self.w)

    def evaluate(self, n_episodes=256, deterministic=None, n_envs=64):
        """{episodes, mean, std, min, max, mean_length} of the CURRENT actor over n_episodes whole episodes on a separate batch
        (evaluation.PolicyEvaluator); deterministic: default the trainer's own"""
        from .evaluation import PolicyEvaluator
        from .ppo import pack_policy
        ev = self._evaluators.get(int(n_envs))
        if ev is None:
            ev = self._evaluators[int(n_envs)] = PolicyEvaluator(self.kind, n_envs=n_envs, seed=self.seed + 1000003, params=self.params, options=self.options,
                                                                 device=self.device, net=self.net)
        return ev.evaluate(pack_policy(self.current_policy()), n_episodes, deterministic=self.deterministic if deterministic is None else deterministic)

    def save(self, path):
        """{"policy": state_dict, "net": name, "es": {...}}: "policy" and "net" as the PPO / TRPO trainers write them, so whatever
        reads a checkpoint's policy reads this one. There is no optimizer and no env state to save: ES has neither."""
        es = dict(env_id=str(self.env_id), generation=self.generation, lr=self.lr, sigma=self.sigma, popsize=self.popsize, repeats=self.repeats, elite=self.elite,
                  decay=self.decay, seed=self.seed, deterministic=self.deterministic, generator=self.gen.get_state())
        d = os.path.dirname(os.path.abspath(path))
        os.makedirs(d, exist_ok=True)
        self.torch.save({"policy": self.current_policy().state_dict(), "net": NET_NAMES[self.net], "es": es}, path)

    def load(self, path):
        ck = self.torch.load(path, map_location=self.device, weights_only=True)
        if ck.get("net", NET_NAMES[self.net]) != NET_NAMES[self.net]:
            raise ValueError("%s holds a checkpoint of the %r network; this trainer's network is %r" % (path, ck["net"], NET_NAMES[self.net]))
        self.policy.load_state_dict(ck["policy"])
        self.w = actor_flat(self.policy)
        es = ck.get("es")
        if es is not None:   # (a PPO / TRPO checkpoint has none: the run starts at generation 0 from its policy)
            self.generation, self.lr, self.sigma = int(es["generation"]), float(es["lr"]), float(es["sigma"])
            self.gen.set_state(es["generator"].cpu())
        return self

    def close(self):
        self.env.close()
        for ev in self._evaluators.values():
            ev.close()
