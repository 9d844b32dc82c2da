"""A population of PPO learners on one GPU: M policies, each with its own hyper-parameters, trained side by side.

A sweep over seeds, learning rates, entropy coefficients or clip ranges is M runs; as M `PPOTrainer`s they are M times the launches,
one after another, each far too small for the device. `PopulationPPO` runs them as ONE batch of M x R envs:

  collect     tb_policy_rollout_members: env i runs with member i // R's blob, one launch per episode cut whatever M is
  advantages  tb_ppo_gae over all envs at once (it is per env)
  update      tb_ppo_grad_members + tb_ppo_apply_members per minibatch: three launches whatever M is. The flat rollout arrays are
              shared; member m's rows (t N + m R + j) are picked by its row of the index tensor

State on the device: flat [M, P] in named_parameters() order (learner.flatten_parameters' order), both Adam moments [M, P],
hp [M, 4] (clip_range, vf_coef, ent_coef, lr: TbPpoMemberHp) and the packed blobs [M, B]. Per member the kernels leave what
`PPOTrainer(learner="fused")` leaves given that member's rows and scalars, bit for bit (include/tb_stepper.h).

`pbt_exploit` is the exploit / explore step of population-based training on those tensors; `export_member` writes a checkpoint
`PPOTrainer.load` reads.
"""
import math
import os
import time

from .learner import current_stream, device_index, gae, grown_workspace
from .params import ENV_SWING, ENV_TENNIS, NET_MLP64, NET_NAMES, NET_TUNED
from .rollout import RolloutBuffer
from .stepper import ENV_IDS, BatchedEnv, StepperError, _check, load_library

HP_COLUMNS = ("clip_range", "vf_coef", "ent_coef", "lr")   # TbPpoMemberHp's fields, hp [M, 4]
MEMBER_HP_KEYS = {"clip_range": 0, "vf_coef": 1, "ent_coef": 2, "lr": 3, "learning_rate": 3}
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-5                  # PPOTrainer's optimiser


def net_of_name(kind, net):
    """"default" / "tuned" / "mlp64" -> NET_*, under PPOTrainer's rules (tuned is Tennisbot-v0's, mlp64 SwingRacket-v0's)"""
    names = {v: k for k, v in NET_NAMES.items()}
    if net not in names:
        raise ValueError("net must be one of %s, not %r" % (sorted(names), net))
    net = names[net]
    if net == NET_TUNED and kind != ENV_TENNIS:
        raise ValueError("net 'tuned' is Tennisbot-v0's network (the reference's train.py -s tuned_ppo)")
    if net == NET_MLP64 and kind != ENV_SWING:
        raise ValueError("net 'mlp64' (NET_MLP64) is SwingRacket-v0's; on Tennisbot-v0 net='default' is that net: pi = vf = [64, 64], tanh")
    return net


def arch_defaults(kind, net):
    from .ppo import SB3_SWING_DEFAULTS, SWING_DEFAULTS, TENNIS_DEFAULTS, TUNED_TENNIS_DEFAULTS
    return TUNED_TENNIS_DEFAULTS if net == NET_TUNED else SB3_SWING_DEFAULTS if net == NET_MLP64 else SWING_DEFAULTS if kind == ENV_SWING else TENNIS_DEFAULTS


def policy_flat(policy):
    """the module's parameters as one float32 vector in named_parameters() order (a copy)"""
    import torch
    return torch.cat([p.detach().reshape(-1).float() for _, p in policy.named_parameters()])


def flat_pack_index(policy):
    """pack_policy's gather index (`_pack_index`), re-aimed at the flat order, in the manner of policy_es._members_index: blob
    position k takes [flat row | 0.0][index[k]]. pack_policy's source is [bias, weight] per layer in blob order, then log_std, then
    one 0.0; here every parameter is found at its named_parameters() offset and the 0.0 at P."""
    import torch
    from .learner import parameter_offsets
    from .ppo import _blob_layers, pack_policy
    dev = policy.log_std.device
    cache = getattr(policy, "_pack_flat_index", None)
    if cache is not None and cache.device == dev:
        return cache
    base = getattr(policy, "_pack_index", None)
    if base is None or base.device != dev:
        pack_policy(policy)   # (builds and caches the index)
        base = policy._pack_index
    offsets = parameter_offsets(policy)
    by_id = {id(p): offsets[name][0] for name, p in policy.named_parameters()}
    total = sum(n for _, n in offsets.values())
    pieces = []
    for m, _ in _blob_layers(policy):
        for t in (m.bias, m.weight):
            pieces.append(torch.arange(t.numel(), dtype=torch.long) + by_id[id(t)])
    pieces.append(torch.arange(policy.log_std.numel(), dtype=torch.long) + by_id[id(policy.log_std)])
    pieces.append(torch.tensor([total], dtype=torch.long))
    cache = torch.cat(pieces).to(dev)[base]
    policy._pack_flat_index = cache
    return cache


def pack_members(policy, flat, out=None):
    """[M, B]: row m is bit for bit `ppo.pack_policy` of a module holding flat[m] ([M, P], named_parameters() order). ONE batched
    gather with a cached index, whatever M is; `policy` only names the architecture. `out`: a preallocated [M, B] tensor."""
    import torch
    idx = flat_pack_index(policy)
    if flat.dim() != 2 or flat.device != idx.device:
        raise ValueError("flat must be [M, P] on %s" % idx.device)
    with torch.no_grad():
        src = torch.cat([flat, torch.zeros((flat.shape[0], 1), dtype=flat.dtype, device=flat.device)], dim=1)
        if out is None:
            return src.index_select(1, idx)
        torch.index_select(src, 1, idx, out=out)
    return out


def members_value(policy, flat, obs):
    """The value path of M networks at once: flat [M, P], obs [M, R, O] -> values [M, R], one batched matrix product per layer
    (torch.baddbmm). `policy` names the architecture (its own parameters are not read): the tuned net's shared extractor first."""
    import torch
    from .learner import parameter_offsets
    offsets = parameter_offsets(policy)
    names = {id(p): name for name, p in policy.named_parameters()}
    M = flat.shape[0]

    def linear(layer, h):
        wo, wn = offsets[names[id(layer.weight)]]
        bo, bn = offsets[names[id(layer.bias)]]
        W = flat[:, wo:wo + wn].view(M, layer.out_features, layer.in_features)
        return torch.baddbmm(flat[:, bo:bo + bn].unsqueeze(1), h, W.transpose(1, 2))

    def body(seq, h):
        for layer in seq:
            h = linear(layer, h) if isinstance(layer, torch.nn.Linear) else layer(h)
        return h

    with torch.no_grad():
        h = obs
        if hasattr(policy, "features_extractor"):
            h = body(policy.features_extractor.layers, h)
        return linear(policy.value_net, body(policy.value_net_body, h)).squeeze(-1)


def pbt_exploit(scores, flat, exp_avg, exp_avg_sq, hp, generator, frac=0.25, factors=(0.8, 1.25)):
    """Population-based training's exploit / explore step, in place on the population's tensors. The floor(frac M) worst members by
    `scores` (NaN ranks worst) copy parameters, both moments and hp from the equally many best, k-th worst from k-th best; then
    the copies' lr and ent_coef are each multiplied by a factor drawn from `factors` with `generator` (clip_range and vf_coef are
    copied unchanged). Returns [(loser, winner)]; nothing happens, and nothing is drawn, when floor(frac M) is 0."""
    import torch
    M = int(flat.shape[0])
    k = int(math.floor(frac * M))
    if k < 1:
        return []
    s = torch.as_tensor(scores, dtype=torch.float64).detach().cpu().reshape(-1)
    if s.numel() != M:
        raise ValueError("scores must have one entry per member (%d), got %d" % (M, s.numel()))
    s = torch.where(torch.isnan(s), torch.full_like(s, -math.inf), s)
    order = torch.argsort(s, descending=True, stable=True).tolist()   # best first; NaN last
    best, worst = order[:k], order[::-1][:k]
    draws = torch.randint(len(factors), (k, 2), generator=generator, device=generator.device).cpu().tolist()
    pairs = []
    with torch.no_grad():
        for j, (lo, hi) in enumerate(zip(worst, best)):
            for x in (flat, exp_avg, exp_avg_sq, hp):
                x[lo].copy_(x[hi])
            hp[lo, 3] *= float(factors[draws[j][0]])   # lr
            hp[lo, 2] *= float(factors[draws[j][1]])   # ent_coef
            pairs.append((lo, hi))
    return pairs


def member_hp_rows(M, base, member_hp):
    """hp [M, 4] as nested lists: `base` (clip_range, vf_coef, ent_coef, lr) for everyone, then member_hp's columns -- a dict of
    clip_range / vf_coef / ent_coef / lr (or learning_rate) -> one value, or a sequence of 1 or M values"""
    rows = [list(base) for _ in range(M)]
    for key, vals in (member_hp or {}).items():
        if key not in MEMBER_HP_KEYS:
            raise ValueError("member_hp: %r is not one of %s" % (key, sorted(MEMBER_HP_KEYS)))
        vals = [float(vals)] if isinstance(vals, (int, float)) else [float(v) for v in vals]
        if len(vals) not in (1, M):
            raise ValueError("member_hp[%r] must hold 1 or %d values, got %d" % (key, M, len(vals)))
        for m in range(M):
            rows[m][MEMBER_HP_KEYS[key]] = vals[m % len(vals)]
    return rows


# ---------------------------------------------------------------------------------------- the scripts' flags (train.py, train_swing.py)
MEMBER_GRANULE = 16  # tb_policy_member_granule() (checked against the library when an env exists)


def add_population_arguments(ap):
    ap.add_argument("--population", type=int, default=0, help="train this many PPO learners side by side on one GPU (tennisbot_rl_amd/population.py); "
                    "--num-envs stays the total and num_envs / population must be a multiple of 16")
    ap.add_argument("--member-lr", type=str, default=None, help="population: learning rates, a comma list of 1 or M values")
    ap.add_argument("--member-ent-coef", type=str, default=None, help="population: entropy coefficients, a comma list of 1 or M values")
    ap.add_argument("--member-clip-range", type=str, default=None, help="population: clip ranges, a comma list of 1 or M values")
    ap.add_argument("--pbt-every", type=int, default=0, help="population: exploit / explore (pbt_exploit) every this many rollouts; 0: never")


def population_keywords(args, select, ppo_selects=("ppo", "tuned_ppo")):
    """PopulationPPO's keywords (members, envs_per_member, member_hp, pbt_every) from the command line, or None without
    --population. Raises ValueError with the message the script exits with."""
    lists = {"lr": args.member_lr, "ent_coef": args.member_ent_coef, "clip_range": args.member_clip_range}
    M = int(args.population)
    if M <= 0:
        if M < 0 or args.pbt_every or any(v is not None for v in lists.values()):
            raise ValueError("--member-lr, --member-ent-coef, --member-clip-range and --pbt-every belong to --population M (M >= 1)")
        return None
    if select not in ppo_selects:
        raise ValueError("--population trains PPO learners (-s ppo / -s tuned_ppo), not -s %s" % select)
    if args.num_envs % M or (args.num_envs // M) % MEMBER_GRANULE or args.num_envs < M:
        raise ValueError("--num-envs %d over --population %d: the envs per member must be a positive multiple of the member granule %d"
                         % (args.num_envs, M, MEMBER_GRANULE))
    member_hp = {}
    for key, text in lists.items():
        if text is None:
            continue
        try:
            vals = [float(x) for x in text.split(",")]
        except ValueError:
            raise ValueError("--member-%s: a comma list of numbers expected, got %r" % (key.replace("_", "-"), text))
        if len(vals) not in (1, M):
            raise ValueError("--member-%s must hold 1 or %d values (--population), got %d" % (key.replace("_", "-"), M, len(vals)))
        member_hp[key] = vals
    if args.pbt_every < 0:
        raise ValueError("--pbt-every must be >= 0")
    return dict(members=M, envs_per_member=args.num_envs // M, member_hp=member_hp, pbt_every=args.pbt_every)


def run_population(pop, total, path, save_freq=0, log=print):
    """the scripts' run: learn to `total` timesteps; at the end and every save_freq timesteps the population checkpoint at `path`
    and best_model.pt beside it = export_member(argmax score). Returns the history."""
    best_path = os.path.join(os.path.dirname(os.path.abspath(path)), "best_model.pt")

    def write():
        pop.save(path)
        sc = pop.torch.nan_to_num(pop.scores(), nan=-math.inf)
        best = int(sc.argmax())
        pop.export_member(best, best_path)
        log("saved %s and %s (member %d, mean episode reward %.3f)" % (path, best_path, best, float(sc[best])))

    history, next_save = [], save_freq or math.inf
    while pop.num_timesteps < total:
        history += pop.learn(min(total, pop.num_timesteps + pop.n_steps * pop.num_envs), log=log)
        if pop.num_timesteps >= next_save and pop.num_timesteps < total:
            write()
            next_save += save_freq
    write()
    return history


class PopulationPPO:
    """M PPO learners on one BatchedEnv of M x envs_per_member envs; member m starts from policy_es.build_policy(kind, net, seed + m).
    hp: PPOTrainer's hyper-parameters, shared (gamma, gae_lambda, n_epochs, max_grad_norm) or every member's default (clip_range,
    vf_coef, ent_coef, learning_rate); member_hp: per-member columns (member_hp_rows). pbt_every=K: pbt_exploit every K rollouts."""

    def __init__(self, env_id="SwingRacket-v0", members=4, envs_per_member=256, n_steps=104, net="default", device=None, seed=0, batch_size=None,
                 member_hp=None, pbt_every=0, pbt_frac=0.25, pbt_factors=(0.8, 1.25), params=None, options=None, **hp):
        import torch
        from .policy_es import build_policy
        from .ppo import COMMON
        self.torch = torch
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("PopulationPPO runs on one GPU: torch.distributed is initialised with world size %d" % dist.get_world_size())
        self.env_id = env_id
        self.kind = kind = ENV_IDS[env_id]
        self.net = net_of_name(kind, net)
        self.M, self.R, self.n_steps = int(members), int(envs_per_member), int(n_steps)
        if self.M < 1:
            raise ValueError("members must be >= 1")
        d = dict(arch_defaults(kind, self.net))
        d.update(COMMON)
        d.update(hp)
        self.hp = d
        if tuple(d["net_arch"]) != tuple(arch_defaults(kind, self.net)["net_arch"]):
            raise ValueError("PopulationPPO trains the architectures the kernels are built for: net_arch %s" % (tuple(arch_defaults(kind, self.net)["net_arch"]),))
        rows = member_hp_rows(self.M, (d["clip_range"], d["vf_coef"], d["ent_coef"], d["learning_rate"]), member_hp)
        self.seed = int(seed)
        self.num_envs = self.M * self.R
        self.env = BatchedEnv(kind, self.num_envs, device=device, seed=self.seed, params=params, track_terminal_obs=False, pipeline=kind == ENV_SWING,
                              options=dict({"ff_defer": "all"}, **(options or {})))
        if self.R % self.env.policy_member_granule():
            raise ValueError("envs_per_member must be a multiple of the member granule %d, got %d" % (self.env.policy_member_granule(), self.R))
        self.device = self.env.device
        self.lib = load_library()
        M, N, T, O, A = self.M, self.num_envs, self.n_steps, self.env.obs_dim, self.env.act_dim
        self.buf = RolloutBuffer(kind, T, N, self.device).bind(self.env)
        # (build_policy seeds under fork_rng(devices=[]), and torch.manual_seed reaches the GPU's generator too: fork that one as well)
        with torch.random.fork_rng(devices=[self.device]):
            self.template = build_policy(kind, self.net, self.seed).to(self.device)   # names the architecture; member 0's initial weights
            self.flat = torch.stack([policy_flat(build_policy(kind, self.net, self.seed + m)) for m in range(M)]).to(self.device).contiguous()
        self.P = int(self.flat.shape[1])
        if self.P != self.lib.tb_ppo_param_floats_net(kind, self.net):
            raise StepperError("the policy has %d parameters, the learner kernels take %d" % (self.P, self.lib.tb_ppo_param_floats_net(kind, self.net)))
        f = dict(dtype=torch.float32, device=self.device)
        self.grad, self.exp_avg, self.exp_avg_sq = (torch.zeros((M, self.P), **f) for _ in range(3))
        self.hp_rows = torch.tensor(rows, **f)
        self.stats = torch.zeros((M, 3), **f)
        self.blobs = torch.empty((M, self.env.policy_floats(self.net)), **f)
        assert self.blobs.shape[1] % 4 == 0 and self.blobs.data_ptr() % 16 == 0
        self.batch_size = int(batch_size or min(T * self.R, 65536))
        self.values, self.logps = torch.zeros((T, N), **f), torch.zeros((T, N), **f)
        self.obs_seq, self._raw_actions = torch.zeros((T, N, O), **f), torch.zeros((T, N, A), **f)
        self.last_value = torch.zeros(N, **f)
        self.obs_in = self.env.reset().clone()
        # member m's global rows of the flat rollout [T N]: t N + m R + j, as [M, T R]
        tt, jj = torch.arange(T, device=self.device).view(1, T, 1), torch.arange(self.R, device=self.device).view(1, 1, self.R)
        self.member_rows = (tt * N + torch.arange(M, device=self.device).view(M, 1, 1) * self.R + jj).reshape(M, T * self.R).contiguous()
        self.gen = torch.Generator(device=self.device)   # minibatch permutations and PBT's factors: the global RNG is left alone
        self.gen.manual_seed(self.seed)
        self.noise_seed = (self.seed * 1000003 + 7919) & 0xFFFFFFFF
        self.pbt_every, self.pbt_frac, self.pbt_factors = int(pbt_every), float(pbt_frac), tuple(pbt_factors)
        self.num_timesteps, self.step_count, self._rollouts = 0, 0, 0
        self._ws = None

    # ------------------------------------------------------------------------------------------------------------ plumbing
    _stream, _dev, _grow = current_stream, device_index, grown_workspace

    def pack(self):
        """flat -> blobs, one batched gather"""
        return pack_members(self.template, self.flat, out=self.blobs)

    def members_value(self, flat, obs):
        return members_value(self.template, flat, obs)

    # ------------------------------------------------------------------------------------------------------------- collect
    def collect(self):
        """n_steps of every env with its member's policy inside the kernel (eagerly: whole episodes per launch); the obs_seq /
        last_value bookkeeping is PPOTrainer._collect_fused's"""
        t, buf, env = self.torch, self.buf, self.env
        with t.no_grad():
            self.pack()
            self.obs_seq[0].copy_(self.obs_in)
            rec = buf.record
            env.policy_rollout_members_ptrs(self.n_steps, self.blobs.data_ptr(), self.M, self.blobs.shape[1], self.R, self.obs_in.data_ptr(),
                                            buf.actions[0].data_ptr(), self._raw_actions.data_ptr(), self.logps.data_ptr(), self.values.data_ptr(),
                                            buf.obs[0].data_ptr(), buf.rewards[0].data_ptr(), buf.dones[0].data_ptr(), (rec, 0, 0, 0, rec, rec, rec),
                                            self.noise_seed, net=self.net)
            env.flush()
            self.obs_seq[1:].copy_(buf.obs[:-1])
            last = buf.obs[self.n_steps - 1]
            self.last_value.copy_(self.members_value(self.flat, last.view(self.M, self.R, -1)).reshape(-1))
            self.obs_in.copy_(last)
        self.num_timesteps += self.n_steps * self.num_envs
        self._rollouts += 1
        return self.last_value

    def advantages(self, last_value):
        """(adv, returns) [T, N]: one tb_ppo_gae call over all envs"""
        return gae(self, self.buf.rewards, self.buf.dones, self.values, last_value)

    # -------------------------------------------------------------------------------------------------------------- update
    def draw_indices(self):
        """one epoch's index rows [M, T R] int64: per member a permutation of its own global rows, all M drawn at once from the
        trainer's generator"""
        t = self.torch
        perm = t.argsort(t.rand(self.member_rows.shape, generator=self.gen, device=self.device), dim=1)
        return self.member_rows.gather(1, perm).contiguous()

    def workspace(self, batch):
        stride = int(self.lib.tb_ppo_members_workspace_stride_bytes(self.kind, self.net, int(batch)))
        self._ws = self._grow(self._ws, stride if stride < 0 else stride * self.M, "tb_ppo_members_workspace_stride_bytes")
        return self._ws

    def minibatch(self, arrays, n_rows, idx, offset, batch, step):
        """one gradient step of every member on rows idx[m, offset : offset + batch]: three launches"""
        L, hp, dev, s = self.lib, self.hp, self._dev(), self._stream()
        obs, act, old_logp, adv, returns = arrays
        ws = self.workspace(batch)
        wb = ws.numel() * 8
        _check(L, L.tb_ppo_grad_members(self.kind, self.net, dev, s, obs.data_ptr(), act.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), returns.data_ptr(), n_rows,
                                        idx.data_ptr() + 8 * offset, idx.stride(0), batch, self.M, self.flat.data_ptr(), self.flat.stride(0), self.P,
                                        self.hp_rows.data_ptr(), ws.data_ptr(), wb), "tb_ppo_grad_members")
        _check(L, L.tb_ppo_apply_members(self.kind, self.net, dev, s, ws.data_ptr(), wb, batch, self.M, self.flat.data_ptr(), self.grad.data_ptr(),
                                         self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.flat.stride(0), self.P, self.stats.data_ptr(), self.hp_rows.data_ptr(),
                                         float(hp["max_grad_norm"]), ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, int(step)), "tb_ppo_apply_members")

    def update(self, adv, returns):
        """n_epochs over every member's own rows in minibatches of batch_size (a ragged tail is a smaller batch for every member
        alike). One device-to-host read at the end: the [M, 3] statistics of the last minibatch."""
        n = self.n_steps * self.num_envs
        arrays = (self.obs_seq.reshape(n, -1), self._raw_actions.reshape(n, -1), self.logps.reshape(n), adv.reshape(n), returns.reshape(n))
        per_member = self.n_steps * self.R
        for _ in range(int(self.hp["n_epochs"])):
            idx = self.draw_indices()
            for s in range(0, per_member, self.batch_size):
                self.step_count += 1
                self.minibatch(arrays, n, idx, s, min(self.batch_size, per_member - s), self.step_count)
        rows = self.stats.tolist()   # the one device-to-host read
        return [{"policy_loss": r[0], "value_loss": r[1], "entropy": r[2]} for r in rows]

    # ---------------------------------------------------------------------------------------------------------- the run
    def scores(self):
        """[M] float64 on the device: each member's mean episode reward over the last rollout (its slice of dones and rewards)"""
        t = self.torch
        ep = self.buf.dones.unflatten(1, (self.M, self.R)).sum(dim=(0, 2), dtype=t.float64)
        rew = self.buf.rewards.unflatten(1, (self.M, self.R)).sum(dim=(0, 2), dtype=t.float64)
        return rew / ep.clamp(min=1.0)

    def learn(self, total_timesteps, log=print):
        history = []
        while self.num_timesteps < total_timesteps:
            t0 = time.perf_counter()
            last_value = self.collect()
            self.torch.cuda.synchronize(self.device)
            t1 = time.perf_counter()
            adv, returns = self.advantages(last_value)
            stats = self.update(adv, returns)
            self.torch.cuda.synchronize(self.device)
            t2 = time.perf_counter()
            c = self.env.counters()
            if c["nonfinite_states"] or c["lockstep_violations"]:
                raise StepperError("rollout %d: %d env states went non-finite, %d episode ends fell outside the pipelined launches' slots"
                                   % (len(history), c["nonfinite_states"], c["lockstep_violations"]))
            sc = self.scores().cpu()
            order = self.torch.argsort(self.torch.nan_to_num(sc, nan=-math.inf), descending=True).tolist()
            best, med, worst = order[0], order[len(order) // 2], order[-1]
            rec = dict(timesteps=self.num_timesteps, scores=sc.tolist(), best=best, median=med, worst=worst, members=stats,
                       collect_steps_per_s=self.n_steps * self.num_envs / (t1 - t0), update_s=t2 - t1)
            if self.pbt_every and self._rollouts % self.pbt_every == 0:
                rec["pbt"] = pbt_exploit(sc, self.flat, self.exp_avg, self.exp_avg_sq, self.hp_rows, self.gen, self.pbt_frac, self.pbt_factors)
            history.append(rec)
            if log:
                log("timesteps %10d  mean episode reward: best %8.3f (member %d)  median %8.3f (%d)  worst %8.3f (%d)  collect %.1f M steps/s  update %.2f s"
                    % (self.num_timesteps, sc[best], best, sc[med], med, sc[worst], worst, rec["collect_steps_per_s"] / 1e6, rec["update_s"]))
        return history

    # ------------------------------------------------------------------------------------------------------ members, files
    def member_policy(self, m):
        """a torch module (on the trainer's device) holding member m's parameters, a copy"""
        import copy
        policy = copy.deepcopy(self.template)
        for name in ("_pack_index", "_pack_flat_index", "_flat_params"):   # (caches that belong to the template's own tensors)
            policy.__dict__.pop(name, None)
        off = 0
        with self.torch.no_grad():
            for _, p in policy.named_parameters():
                p.copy_(self.flat[m, off:off + p.numel()].view(p.shape))
                off += p.numel()
        return policy

    def member_hp(self, m):
        row = self.hp_rows[m].tolist()
        return dict(self.hp, clip_range=row[0], vf_coef=row[1], ent_coef=row[2], learning_rate=row[3])

    def export_member(self, m, path):
        """member m as a checkpoint in PPOTrainer.save's format: its policy, an Adam state holding its moments and step count, its
        slice of the env batch and its hyper-parameters. PPOTrainer(num_envs=envs_per_member).load reads it unchanged."""
        t = self.torch
        policy, hp = self.member_policy(m), self.member_hp(m)
        opt = t.optim.Adam(policy.parameters(), lr=hp["learning_rate"], eps=ADAM_EPS)
        off = 0
        for p in policy.parameters():
            n = p.numel()
            opt.state[p] = {"step": t.tensor(float(self.step_count)), "exp_avg": self.exp_avg[m, off:off + n].view(p.shape).clone(),
                            "exp_avg_sq": self.exp_avg_sq[m, off:off + n].view(p.shape).clone()}
            off += n
        w, d = self.env.get_state_words()
        lo, hi = m * self.R, (m + 1) * self.R
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        t.save({"policy": policy.state_dict(), "optimizer": opt.state_dict(), "num_timesteps": self.num_timesteps // self.M,
                "env_words": w[:, lo:hi].contiguous().cpu(), "env_done": d[lo:hi].contiguous().cpu(), "hp": hp, "net": NET_NAMES[self.net]}, path)

    def save(self, path):
        """the whole population: flat, moments, hp, step count, timesteps, the generator's state, and the env batch"""
        w, d = self.env.get_state_words()
        pop = dict(flat=self.flat.cpu(), exp_avg=self.exp_avg.cpu(), exp_avg_sq=self.exp_avg_sq.cpu(), hp=self.hp_rows.cpu(), step=self.step_count,
                   num_timesteps=self.num_timesteps, rollouts=self._rollouts, generator=self.gen.get_state(), members=self.M, envs_per_member=self.R)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.torch.save({"population": pop, "net": NET_NAMES[self.net], "env_words": w.cpu(), "env_done": d.cpu(), "hp": self.hp}, path)

    def load(self, path):
        ck = self.torch.load(path, map_location="cpu", weights_only=True)
        pop = ck.get("population")
        if pop is None:
            raise ValueError("%s is not a population checkpoint (a member's file goes to PPOTrainer.load)" % path)
        if ck["net"] != NET_NAMES[self.net] or int(pop["members"]) != self.M or int(pop["envs_per_member"]) != self.R:
            raise ValueError("%s holds %d x %d members of the %r network; this population is %d x %d of %r"
                             % (path, pop["members"], pop["envs_per_member"], ck["net"], self.M, self.R, NET_NAMES[self.net]))
        for dst, key in ((self.flat, "flat"), (self.exp_avg, "exp_avg"), (self.exp_avg_sq, "exp_avg_sq"), (self.hp_rows, "hp")):
            dst.copy_(pop[key])
        self.step_count, self.num_timesteps, self._rollouts = int(pop["step"]), int(pop["num_timesteps"]), int(pop["rollouts"])
        self.gen.set_state(pop["generator"].cpu())
        self.env.set_state_words(ck["env_words"].to(self.device), ck["env_done"].to(self.device))
        self.obs_in.copy_(self.env.observe())
        return self

    def close(self):
        self.env.close()
