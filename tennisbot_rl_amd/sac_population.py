"""A population of SAC (or TQC) learners on one GPU: M learners, each with its own learning rates, gamma and tau, trained in the
launches of ONE learner's gradient step (C ABI tb_sac_*_members / tb_tqc_*_members in include/tb_stepper.h; the member axis of
csrc/tb_sac.hpp). `population.py` is PPO's; this is its off-policy counterpart.

One fused SAC gradient step is LAUNCHES_PER_STEP = 40 launches (sac.py), launch-bound at SB3's batch sizes: M `SACTrainer`s one
after another pay M x 40 launch gaps on a device that is mostly empty. Here the member is one more grid axis of the same kernels:
`FusedSACMembers.gradient_step` is 40 launches whatever M is (TQC: 41), in SAC's order, with no host synchronisation inside:

  actor forward 5 | targets 9 | critic gradient 10 (TQC 11) | the critics' Adam with Polyak folded in 1 | actor gradient 13 |
  the actors' Adam 1 | log_ent_coef's Adam 1 -- last: the kernels above read log_ent_coef as it was before this step

Per member the stages leave, bit for bit, what `FusedSAC`'s stages leave given that member's rows and scalars.

`PopulationSAC` is the loop: one BatchedEnv of M x R envs, ONE shared replay ring that holds whole vector steps (row = slot * N +
m * R + j, N = M R), member m's batches drawn from its own columns (`sample_member_indices`), the torch collect with one batched
actor forward for all members (`members_sample`). `pbt_exploit_sac` is the exploit / explore step; `export_member` writes a
checkpoint `SACTrainer.load` / `TQCTrainer.load` reads. One rank only; there is no torch fallback for the gradient step.
"""
import math
import os
import time

from .learner import current_stream, device_index, grown_workspace
from .sac import ACTOR_NAMES, HIDDEN, LAUNCHES_PER_STEP, LOG_STD_MAX, LOG_STD_MIN, SAC_DEFAULTS, TB_SAC_ACTOR, TB_SAC_CRITIC, ReplayBuffer
from .stepper import ACT_DIM, ENV_IDS, OBS_DIM, BatchedEnv, StepperError, _check, load_library

HP_COLUMNS = ("lr_actor", "lr_critic", "lr_ent", "gamma", "tau")   # TbSacMemberHp's fields; hp is [M, 8], columns 5 .. 7 padding
HP_WIDTH = 8
LR_ACTOR, LR_CRITIC, LR_ENT = 0, 1, 2                              # TB_SAC_LR_*: which learning rate a tb_sac_adam_members call takes
MEMBER_HP_KEYS = {"lr": (0, 1, 2), "learning_rate": (0, 1, 2), "lr_actor": (0,), "lr_critic": (1,), "lr_ent": (2,), "gamma": (3,), "tau": (4,)}
ADAM_BETAS = (0.9, 0.999)
MAX_MEMBERS = 32767        # TB_SAC_MAX_MEMBERS: (member, net) is the grid's z axis
MAX_ENVS = 1 << 25         # what one BatchedEnv holds (tb_create)
ALGOS = ("sac", "tqc")
# launches of one FusedSACMembers / FusedTQCMembers gradient_step, whatever M is: sac.LAUNCHES_PER_STEP and tqc.LAUNCHES_PER_STEP
MEMBERS_LAUNCHES_PER_STEP = {"sac": LAUNCHES_PER_STEP, "tqc": LAUNCHES_PER_STEP + 1}
assert MEMBERS_LAUNCHES_PER_STEP == {"sac": 5 + 9 + 10 + 1 + 13 + 2, "tqc": 5 + 9 + 11 + 1 + 13 + 2}


def _algo(algo):
    """(C prefix, y's trailing shape, the modules' builder, the trainer class) of "sac" / "tqc\""""
    if algo == "sac":
        from .sac import SACTrainer, build_sac_modules
        return "tb_sac_", (), build_sac_modules, SACTrainer
    if algo == "tqc":
        from .tqc import N_TARGETS, TQCTrainer, build_tqc_modules
        return "tb_tqc_", (N_TARGETS,), build_tqc_modules, TQCTrainer
    raise ValueError("algo must be one of %s, not %r" % (ALGOS, algo))


# ------------------------------------------------------------------------------------------------------------- pure functions
def sample_member_indices(generator, M, R, filled_slots, G, B):
    """int64 [G, M, B]: G batches of B replay rows for each of M members, from a ring that holds `filled_slots` whole vector steps
    of N = M R envs (row = slot * N + m * R + j). Member m's entries lie in its own columns [m R, (m + 1) R) of a filled slot,
    drawn uniformly WITH replacement (as ReplayBuffer.sample draws): a batch may exceed what the columns hold. Everything is drawn
    from `generator`, on its device; torch's global RNG is not touched."""
    import torch
    M, R, S, G, B = int(M), int(R), int(filled_slots), int(G), int(B)
    if min(M, R, S, G, B) < 1:
        raise ValueError("sample_member_indices: M, R, filled_slots, G and B must all be >= 1")
    dev = generator.device
    slot = torch.randint(0, S, (G, M, B), generator=generator, device=dev, dtype=torch.int64)
    col = torch.randint(0, R, (G, M, B), generator=generator, device=dev, dtype=torch.int64)
    return (slot * (M * R) + torch.arange(M, device=dev, dtype=torch.int64).view(1, M, 1) * R + col).contiguous()


def actor_offsets(obs_dim, act_dim):
    """name -> (offset, shape) of the flat TB_SAC_ACTOR vector (ACTOR_NAMES order)"""
    shapes = ((HIDDEN, obs_dim), (HIDDEN,), (HIDDEN, HIDDEN), (HIDDEN,), (act_dim, HIDDEN), (act_dim,), (act_dim, HIDDEN), (act_dim,))
    out, off = {}, 0
    for name, shape in zip(ACTOR_NAMES, shapes):
        out[name] = (off, shape)
        off += math.prod(shape)
    return out


def members_sample(flat, obs, eps):
    """The actors of M members at once: flat [M, P] (TB_SAC_ACTOR vectors; a row stride above P is fine), obs [M, R, O], eps
    [M, R, A] -> (action [M, R, A], logp [M, R]): `Actor.sample` of sac.build_sac_modules per member, one torch.baddbmm per layer
    on views of the stacked flat vector (as population.members_value does). Pure torch, any device."""
    import torch
    M, _, O = obs.shape
    A = eps.shape[2]
    off = actor_offsets(O, A)

    def linear(prefix, h):
        (wo, ws), (bo, bs) = off[prefix + ".weight"], off[prefix + ".bias"]
        W = flat[:, wo:wo + ws[0] * ws[1]].view(M, ws[0], ws[1])
        return torch.baddbmm(flat[:, bo:bo + bs[0]].unsqueeze(1), h, W.transpose(1, 2))

    with torch.no_grad():
        h = torch.relu(linear("latent_pi.0", obs))
        h = torch.relu(linear("latent_pi.2", h))
        mu, log_std = linear("mu", h), linear("log_std", h).clamp(LOG_STD_MIN, LOG_STD_MAX)
        a = torch.tanh(mu + log_std.exp() * eps)
        logp = (-0.5 * eps * eps - log_std - 0.5 * math.log(2.0 * math.pi)).sum(2) - torch.log(1.0 - a * a + 1e-6).sum(2)
    return a, logp


def pbt_exploit_sac(scores, vectors, hp, generator, frac=0.25, factors=(0.8, 1.25)):
    """Population-based training's exploit / explore step, in place on the population's tensors. The floor(frac M) worst members by
    `scores` (NaN ranks worst) copy from the equally many best, k-th worst from k-th best: every tensor of `vectors` (leading
    dimension M: actor, critic, target, log_ent_coef and every Adam moment) and the hp row. Then the copy's three learning rates
    are multiplied by ONE factor drawn uniformly from the open interval `factors` with `generator`; gamma and tau are copied
    unchanged. Replay columns are NOT copied: SAC is off-policy, so the transitions the old member collected stay usable for the
    new parameters, and the copy goes on collecting into the same columns. Returns [(loser, winner)]; nothing happens, and nothing
    is drawn, when floor(frac M) is 0."""
    import torch
    M = int(hp.shape[0])
    k = int(math.floor(frac * M))
    if k < 1:
        return []
    s = torch.as_tensor(scores, dtype=torch.float64).detach().cpu().reshape(-1)
    if s.numel() != M:
        raise ValueError("scores must have one entry per member (%d), got %d" % (M, s.numel()))
    s = torch.where(torch.isnan(s), torch.full_like(s, -math.inf), s)
    order = torch.argsort(s, descending=True, stable=True).tolist()   # best first; NaN last
    best, worst = order[:k], order[::-1][:k]
    lo_f, hi_f = float(factors[0]), float(factors[1])
    u = torch.rand(k, generator=generator, device=generator.device, dtype=torch.float64).cpu().tolist()
    pairs = []
    with torch.no_grad():
        for j, (lo, hi) in enumerate(zip(worst, best)):
            for x in tuple(vectors) + (hp,):
                x[lo].copy_(x[hi])
            hp[lo, 0:3] *= lo_f + (hi_f - lo_f) * (0.001 + 0.998 * u[j])   # strictly inside the interval
            pairs.append((lo, hi))
    return pairs


def member_hp_rows(M, base, member_hp):
    """hp [M, 8] as nested lists: `base` (lr_actor, lr_critic, lr_ent, gamma, tau) for everyone, then member_hp's columns -- a dict
    of lr (or learning_rate: all three optimisers) / lr_actor / lr_critic / lr_ent / gamma / tau -> one value, or 1 or M values"""
    rows = [list(base) + [0.0] * (HP_WIDTH - len(base)) for _ in range(M)]
    for key, vals in (member_hp or {}).items():
        if key not in MEMBER_HP_KEYS:
            raise ValueError("member_hp: %r is not one of %s" % (key, sorted(MEMBER_HP_KEYS)))
        vals = [float(vals)] if isinstance(vals, (int, float)) else [float(v) for v in vals]
        if len(vals) not in (1, M):
            raise ValueError("member_hp[%r] must hold 1 or %d values, got %d" % (key, M, len(vals)))
        for m in range(M):
            for c in MEMBER_HP_KEYS[key]:
                rows[m][c] = vals[m % len(vals)]
    return rows


def member_checkpoint(algo, obs_dim, act_dim, actor, critic, target, log_ent_coef, moments, hp_row, step, adam_eps=SAC_DEFAULTS["adam_eps"]):
    """One member as the dict SACTrainer.save / TQCTrainer.save writes, without the env and replay entries: `actor`, `critic`,
    `critic_target` state dicts, the three `optimizers` (plain Adam holding the member's moments and step count), `log_ent_coef`
    [1] and `hp`. actor / critic / target: the member's flat vectors; moments = ((m, v) of the actor, of the critic, of
    log_ent_coef); hp_row: its TbSacMemberHp row. Pure torch on CPU copies: no device is needed."""
    import torch
    build = _algo(algo)[2]
    hp_row = [float(x) for x in hp_row]
    mods = build(obs_dim, act_dim)
    lec = torch.nn.Parameter(torch.as_tensor(log_ent_coef, dtype=torch.float32).detach().cpu().reshape(1).clone())
    sets = ([p for _, p in mods[0].named_parameters()], [p for _, p in mods[1].named_parameters()], [lec])
    with torch.no_grad():
        for module, flat in zip(mods, (actor, critic, target)):
            flat, off = flat.detach().cpu(), 0
            for _, p in module.named_parameters():
                p.copy_(flat[off:off + p.numel()].view(p.shape))
                off += p.numel()
    opts = []
    for params, (m1, m2), lr in zip(sets, moments, hp_row[:3]):
        opt = torch.optim.Adam(params, lr=lr, eps=adam_eps)
        m1, m2, off = m1.detach().cpu().reshape(-1), m2.detach().cpu().reshape(-1), 0
        for p in params:
            n = p.numel()
            opt.state[p] = {"step": torch.tensor(float(step)), "exp_avg": m1[off:off + n].view(p.shape).clone(), "exp_avg_sq": m2[off:off + n].view(p.shape).clone()}
            off += n
        opts.append(opt.state_dict())
    return {"actor": mods[0].state_dict(), "critic": mods[1].state_dict(), "critic_target": mods[2].state_dict(), "optimizers": opts, "log_ent_coef": lec.detach().clone(),
            "hp": dict(learning_rate=hp_row[0], gamma=hp_row[3], tau=hp_row[4], adam_eps=adam_eps)}


# ------------------------------------------------------------------------------------------------------------------ the learner
class _Rows:
    """[M, n] parameters with their gradient and both Adam moments (optimised=False: parameters alone, the target's form)"""

    def __init__(self, torch, flat, optimised=True):
        self.flat = flat
        self.grad, self.exp_avg, self.exp_avg_sq = (torch.zeros_like(flat) if optimised else None for _ in range(3))

    def tensors(self):
        return self.flat, self.exp_avg, self.exp_avg_sq


class FusedSACMembers:
    """SAC's gradient step for M members at once. State on the device, one row per member: pi / q / qt (`_Rows`: flat [M, P] with
    gradient and moments; qt the target, parameters only), ent (log_ent_coef [M, 1] likewise), hp [M, 8] (HP_COLUMNS), stats
    [M, 4] float64 (critic loss, actor loss, mean logp, d log_ent_coef), step. Every array is passed with its row stride
    (tensor.stride(0)), so rows may be views of wider storage. Member m starts from the modules built under seed + m; its rows are
    then what FusedSAC holds for those modules. Adam is torch's plain Adam (betas 0.9 / 0.999, eps adam_eps), shared."""

    ALGO = "sac"

    def __init__(self, kind, members, device, seed=0, hp_rows=None, adam_eps=SAC_DEFAULTS["adam_eps"]):
        import torch
        self.torch, self.kind, self.M = torch, int(kind), int(members)
        if not 1 <= self.M <= MAX_MEMBERS:
            raise ValueError("%s: members must be in [1, %d], not %d" % (type(self).__name__, MAX_MEMBERS, self.M))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise StepperError("%s needs a GPU (there is no CPU fallback)" % type(self).__name__)
        self.ABI, self.Y_SHAPE, build, _ = _algo(self.ALGO)
        self.lib = load_library()
        self.O, self.A, self.adam_eps = OBS_DIM[self.kind], ACT_DIM[self.kind], float(adam_eps)
        pis, qs = [], []
        with torch.random.fork_rng(devices=[self.device]):   # (torch.manual_seed reaches the GPU's generator too)
            for m in range(self.M):
                torch.manual_seed(int(seed) + m)
                actor, critic, _ = build(self.O, self.A)
                pis.append(torch.cat([p.detach().reshape(-1) for _, p in actor.named_parameters()]))
                qs.append(torch.cat([p.detach().reshape(-1) for _, p in critic.named_parameters()]))
        f = dict(dtype=torch.float32, device=self.device)
        self.pi, self.q = _Rows(torch, torch.stack(pis).to(**f).contiguous()), _Rows(torch, torch.stack(qs).to(**f).contiguous())
        self.qt = _Rows(torch, self.q.flat.clone(), optimised=False)   # follows q by the Polyak update: no gradient, no moments
        self.ent = _Rows(torch, torch.zeros((self.M, 1), **f))   # ent_coef "auto": log_ent_coef starts at 0
        for rows, which in ((self.pi, TB_SAC_ACTOR), (self.q, TB_SAC_CRITIC)):
            n = int(getattr(self.lib, self.ABI + "param_floats")(self.kind, which))
            if rows.flat.shape[1] != n:
                raise StepperError("%s: the modules hold %d parameters, the kernels take %d" % (type(self).__name__, rows.flat.shape[1], n))
        d = SAC_DEFAULTS
        base = member_hp_rows(self.M, (d["learning_rate"],) * 3 + (d["gamma"], d["tau"]), None)
        self.hp = torch.tensor(base if hp_rows is None else hp_rows, **f).contiguous()
        if tuple(self.hp.shape) != (self.M, HP_WIDTH):
            raise ValueError("hp_rows must be [%d, %d]" % (self.M, HP_WIDTH))
        self.stats = torch.zeros((self.M, 4), dtype=torch.float64, device=self.device)
        self.step = 0
        self._ws = self._batch = self._pi_batch = None   # _pi_batch: the batch whose actor activations the workspace holds

    _stream, _dev, _grow = current_stream, device_index, grown_workspace

    @property
    def log_ent_coef(self):
        return self.ent.flat

    def vectors(self):
        """every tensor pbt_exploit_sac copies: actor, critic, target, log_ent_coef and every moment"""
        return self.pi.tensors() + self.q.tensors() + (self.qt.flat,) + self.ent.tensors()

    def workspace(self, batch):
        what = self.ABI + "members_workspace_stride_bytes"
        stride = int(getattr(self.lib, what)(self.kind, int(batch)))
        self._ws = self._grow(self._ws, stride if stride < 0 else stride * self.M, what)
        if self._batch != int(batch):   # the regions' offsets scale with the batch: what an earlier stage kept is gone
            B = self._batch = int(batch)
            self._pi_batch = None
            e = lambda *s: self.torch.empty(s, dtype=self.torch.float32, device=self.device)  # noqa: E731
            self.act_pi, self.logp_pi, self.y = e(self.M, B, self.A), e(self.M, B), e(self.M, B, *self.Y_SHAPE)
        return self._ws

    def _rows(self, x, name, inner, dtype=None):
        """x [M, *inner] of float32 (or dtype) on the device, the inner dimensions contiguous: (pointer, row stride in elements)"""
        t = self.torch
        dtype = t.float32 if dtype is None else dtype
        ok = x.dtype == dtype and x.device.type == "cuda" and tuple(x.shape) == (self.M,) + tuple(inner) and x[0].is_contiguous()
        if not ok or (self.M > 1 and x.stride(0) < max(1, x[0].numel())):
            raise ValueError("%s: a %s tensor of shape %s on the GPU with contiguous rows expected" % (name, dtype, (self.M,) + tuple(inner)))
        return x.data_ptr(), int(x.stride(0)) if self.M > 1 else max(1, int(x[0].numel()))

    def _shared(self, x, name, shape):
        if x.dtype != self.torch.float32 or x.device.type != "cuda" or not x.is_contiguous() or tuple(x.shape) != tuple(shape):
            raise ValueError("%s: contiguous float32 tensor of shape %s on the GPU expected" % (name, tuple(shape)))
        return x.data_ptr()

    def _call(self, stage, *args):
        _check(self.lib, getattr(self.lib, self.ABI + stage)(*args), self.ABI + stage)

    def _per_member(self, x, name, dtype=None):
        """x [M] or [M, 1]: one CONTIGUOUS entry per member (the kernels index these by the member alone); its pointer"""
        t = self.torch
        if x.dtype != (t.float32 if dtype is None else dtype) or x.device.type != "cuda" or x.numel() != self.M or not x.is_contiguous():
            raise ValueError("%s: one contiguous entry per member on the GPU expected" % name)
        return x.data_ptr()

    # --------------------------------------------------------------------------------------------------------------- the stages
    def actor_forward(self, obs, idx, eps):
        B = int(idx.shape[1])
        ws = self.workspace(B)
        n = int(obs.shape[0])
        self._call("actor_forward_members", self.kind, self._dev(), self._stream(), self._shared(obs, "obs", (n, self.O)), n, *self._rows(idx, "idx", (B,), self.torch.int64), B,
                   self.M, *self._rows(self.pi.flat, "actor", (self.pi.flat.shape[1],)), *self._rows(eps, "eps", (B, self.A)), *self._rows(self.act_pi, "act_out", (B, self.A)),
                   *self._rows(self.logp_pi, "logp_out", (B,)), ws.data_ptr(), ws.numel() * 8)
        self._pi_batch = B
        return self.act_pi, self.logp_pi

    def targets(self, next_obs, reward, done, idx, eps_next):
        B = int(idx.shape[1])
        ws = self.workspace(B)
        n = int(next_obs.shape[0])
        self._call("targets_members", self.kind, self._dev(), self._stream(), self._shared(next_obs, "next_obs", (n, self.O)), self._shared(reward, "reward", (n,)),
                   self._shared(done, "done", (n,)), n, *self._rows(idx, "idx", (B,), self.torch.int64), B, self.M, *self._rows(self.pi.flat, "actor", (self.pi.flat.shape[1],)),
                   *self._rows(self.qt.flat, "target", (self.qt.flat.shape[1],)), self._per_member(self.ent.flat, "log_ent_coef"), *self._rows(eps_next, "eps_next", (B, self.A)),
                   self.hp.data_ptr(), *self._rows(self.y, "y", (B,) + self.Y_SHAPE), ws.data_ptr(), ws.numel() * 8)
        return self.y

    def critic_gradient(self, obs, action, idx):
        B = int(idx.shape[1])
        ws = self.workspace(B)
        n = int(obs.shape[0])
        qp, qs = self._rows(self.q.flat, "critic", (self.q.flat.shape[1],))
        if self._rows(self.q.grad, "critic gradient", (self.q.flat.shape[1],))[1] != qs:
            raise ValueError("the critic's gradient must have the critic's row stride")
        self._call("critic_grad_members", self.kind, self._dev(), self._stream(), self._shared(obs, "obs", (n, self.O)), self._shared(action, "action", (n, self.A)), n,
                   *self._rows(idx, "idx", (B,), self.torch.int64), B, self.M, qp, qs, *self._rows(self.y, "y", (B,) + self.Y_SHAPE), self.q.grad.data_ptr(),
                   self.stats.data_ptr(), ws.data_ptr(), ws.numel() * 8)
        return self.q.grad

    def actor_gradient(self, batch, eps):
        """every member's actor gradient and log_ent_coef's, on the batch of the last actor_forward"""
        B = int(batch)
        if B != self._pi_batch:
            raise ValueError("actor_gradient: the workspace holds %s, not an actor_forward of %d rows (a stage at another batch size in between overwrites it)"
                             % ("no actor_forward" if self._pi_batch is None else "an actor_forward of %d rows" % self._pi_batch, B))
        ws = self.workspace(B)
        pp, ps = self._rows(self.pi.flat, "actor", (self.pi.flat.shape[1],))
        if self._rows(self.pi.grad, "actor gradient", (self.pi.flat.shape[1],))[1] != ps:
            raise ValueError("the actor's gradient must have the actor's row stride")
        self._call("actor_grad_members", self.kind, self._dev(), self._stream(), B, self.M, pp, ps, *self._rows(self.q.flat, "critic", (self.q.flat.shape[1],)),
                   self._per_member(self.ent.flat, "log_ent_coef"), *self._rows(eps, "eps", (B, self.A)), self.pi.grad.data_ptr(),
                   self._per_member(self.ent.grad, "ent_grad"), self.stats.data_ptr(), ws.data_ptr(), ws.numel() * 8)
        return self.pi.grad, self.ent.grad

    def adam(self, rows, which_lr, target=None):
        """one Adam step of every member's row of `rows` with hp's learning rate `which_lr`; target: rows that follow by the Polyak
        update (hp's tau) in the same launch"""
        n = int(rows.flat.shape[1])
        p, stride = self._rows(rows.flat, "params", (n,))
        for x, name in ((rows.grad, "grad"), (rows.exp_avg, "exp_avg"), (rows.exp_avg_sq, "exp_avg_sq")) + (() if target is None else ((target, "target"),)):
            if self._rows(x, name, (n,))[1] != stride:
                raise ValueError("%s must have its parameters' row stride" % name)
        _check(self.lib, self.lib.tb_sac_adam_members(self._dev(), self._stream(), p, rows.grad.data_ptr(), rows.exp_avg.data_ptr(), rows.exp_avg_sq.data_ptr(), n, stride, self.M,
                                                      self.hp.data_ptr(), int(which_lr), ADAM_BETAS[0], ADAM_BETAS[1], self.adam_eps, int(self.step),
                                                      None if target is None else target.data_ptr()), "tb_sac_adam_members")

    def polyak(self, params, target):
        """every member's target row <- (1 - tau) target + tau params with ITS tau, alone (one launch)"""
        n = int(params.shape[1])
        p, stride = self._rows(params, "params", (n,))
        if self._rows(target, "target", (n,))[1] != stride:
            raise ValueError("target must have its parameters' row stride")
        _check(self.lib, self.lib.tb_sac_adam_members(self._dev(), self._stream(), p, None, None, None, n, stride, self.M, self.hp.data_ptr(), LR_CRITIC, 0.0, 0.0, 0.0, 1,
                                                      target.data_ptr()), "tb_sac_adam_members")

    def gradient_step(self, replay_arrays, idx, eps_pi, eps_next):
        """one gradient step of every member on ITS rows idx[m] of the shared replay_arrays = (obs, next_obs, action, reward, done),
        idx [M, B] int64, eps_pi / eps_next [M, B, A]. MEMBERS_LAUNCHES_PER_STEP launches (40; TQC 41) whatever M is, SAC's stages in
        SAC's order; nothing here synchronises with the host."""
        obs, next_obs, action, reward, done = replay_arrays
        self.step += 1
        self.actor_forward(obs, idx, eps_pi)                  # 5
        self.targets(next_obs, reward, done, idx, eps_next)   # 9
        self.critic_gradient(obs, action, idx)                # 10 (TQC: 11)
        self.adam(self.q, LR_CRITIC, target=self.qt.flat)     # 1, Polyak folded in
        self.actor_gradient(int(idx.shape[1]), eps_pi)        # 13
        self.adam(self.pi, LR_ACTOR)                          # 1
        self.adam(self.ent, LR_ENT)                           # 1, last: the kernels above read log_ent_coef as it was before this step


class FusedTQCMembers(FusedSACMembers):
    """TQC's gradient step for M members at once: FusedSACMembers with the tb_tqc_ entry points and y [M, B, 46]"""

    ALGO = "tqc"


# -------------------------------------------------------------------------------------------------------------------- the loop
class PopulationSAC:
    """M SAC (algo="tqc": TQC) learners on one BatchedEnv of M x envs_per_member envs and ONE replay ring. Member m behaves like a
    `SACTrainer(num_envs=envs_per_member)`: learning_starts counts ITS timesteps (slots x R), gradient_steps defaults to R, its
    batches come from its own columns of the ring. buffer_size is the ring's rows over all members, rounded down to whole vector
    steps (a multiple of N = M R, as collect_form="fused" rounds). batch_size may exceed what a member's columns hold: sampling is
    with replacement, as ReplayBuffer.sample's is, so nothing is refused for it. hp: learning_rate, gamma, tau, adam_eps
    (SAC_DEFAULTS), every member's default; member_hp: per-member columns (member_hp_rows). Noise, uniform actions, batch indices and
    PBT's factors come from the trainer's own device generator.

    A member's score (`scores()`, the progress line, PBT, the scripts' best member) is the mean reward of its last score_episodes to
    2 score_episodes finished episodes, kept on the device in two windows per member: it does not depend on when the progress lines
    fall, and it is NaN only for a member that has finished no episode yet. pbt_every=K: every K vector steps of learn(),
    pbt_exploit_sac -- but only once EVERY member has a score, so that no member is copied over, or copied from, on no evidence (on
    SwingRacket-v0 all envs end together every 26 steps: before step 26 nobody has one). A copy's windows are cleared: the episodes
    in them were the old parameters', so the next exploit waits until the copy has finished an episode of its own."""

    def __init__(self, env_id="SwingRacket-v0", members=4, envs_per_member=16, algo="sac", batch_size=None, gradient_steps=None, buffer_size=1_000_000, learning_starts=100,
                 seed=0, member_hp=None, pbt_every=0, pbt_frac=0.25, pbt_factors=(0.8, 1.25), score_episodes=100, params=None, device=None, **hp):
        import torch
        self.torch = torch
        name = type(self).__name__
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("%s runs on one rank (world size %d): multi-GPU populations are not provided" % (name, dist.get_world_size()))
        self.algo = algo
        _, _, _, self.trainer_class = _algo(algo)
        unknown = set(hp) - set(SAC_DEFAULTS)
        if unknown:
            raise ValueError("%s: unknown hyper-parameters %s" % (name, sorted(unknown)))
        self.hp = dict(SAC_DEFAULTS, **hp)
        self.env_id, self.kind = env_id, ENV_IDS[env_id]
        self.M, self.R = int(members), int(envs_per_member)
        if not 1 <= self.M <= MAX_MEMBERS or self.R < 1:
            raise ValueError("%s: members must be in [1, %d] and envs_per_member >= 1, not %d x %d" % (name, MAX_MEMBERS, self.M, self.R))
        self.num_envs = N = self.M * self.R
        if N > MAX_ENVS:
            raise ValueError("%s: members x envs_per_member = %d x %d = %d envs; one BatchedEnv holds at most %d" % (name, self.M, self.R, N, MAX_ENVS))
        from .sac import BATCH_SIZE
        from .tqc import BATCH_SIZE as TQC_BATCH
        self.batch_size = int(batch_size or (BATCH_SIZE[env_id] if algo == "sac" else TQC_BATCH))
        self.gradient_steps = self.R if gradient_steps is None else int(gradient_steps)
        self.learning_starts = int(learning_starts)
        rounded = int(buffer_size) // N * N
        if rounded < N:
            raise ValueError("%s: buffer_size %d holds no whole vector step of %d envs" % (name, buffer_size, N))
        d = self.hp
        rows = member_hp_rows(self.M, (d["learning_rate"],) * 3 + (d["gamma"], d["tau"]), member_hp)
        self.seed = int(seed)
        self.env = BatchedEnv(self.kind, N, device=device, seed=self.seed, params=params, track_terminal_obs=False, pipeline=False)
        self.device = self.env.device
        learner = FusedSACMembers if algo == "sac" else FusedTQCMembers
        self._learner = learner(self.kind, self.M, self.device, seed=self.seed, hp_rows=rows, adam_eps=d["adam_eps"])
        self.replay = ReplayBuffer(self.env.obs_dim, self.env.act_dim, rounded, self.device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(self.seed)
        self.obs = self.env.reset()
        self.num_timesteps = 0   # over all members; a member's own: member_timesteps
        self.pbt_every, self.pbt_frac, self.pbt_factors = int(pbt_every), float(pbt_frac), tuple(pbt_factors)
        self._ep_return = torch.zeros(N, device=self.device)
        self._ep_stats = torch.zeros((self.M, 2), dtype=torch.float64, device=self.device)   # per member: finished episodes, the sum of their returns (since the last progress line)
        self.score_episodes = int(score_episodes)
        if self.score_episodes < 1:
            raise ValueError("%s: score_episodes must be >= 1" % name)
        self._score = torch.zeros((2, self.M, 2), dtype=torch.float64, device=self.device)   # the same two sums in [the last full window, the one being filled]
        self._vector_steps = 0

    @property
    def member_timesteps(self):
        return self.num_timesteps // self.M

    @property
    def filled_slots(self):
        return self.replay.size // self.num_envs

    # ------------------------------------------------------------------------------------------------------------------ collect
    def collect(self):
        """one step of every env into the ring: uniform actions while a member's timesteps < learning_starts, afterwards ONE batched
        actor forward for all members (members_sample). Returns (action, obs, reward, done) of that step."""
        t, M, R, A = self.torch, self.M, self.R, self.env.act_dim
        with t.no_grad():
            if self.member_timesteps < self.learning_starts:
                a = t.rand((self.num_envs, A), device=self.device, generator=self.gen) * 2.0 - 1.0
            else:
                eps = t.randn((M, R, A), device=self.device, generator=self.gen)
                a = members_sample(self._learner.pi.flat, self.obs.view(M, R, -1), eps)[0].reshape(self.num_envs, A)
            a = a.contiguous()
            obs, r, d = self.env.step(a)
            df = d.float()
            self.replay.add(self.obs, obs, a, r, df)   # a whole vector step: row = slot * N + m * R + j
            self._ep_return += r
            ended = t.stack((df.view(M, R).sum(1), (self._ep_return * df).view(M, R).sum(1)), 1).double()   # [M, 2]
            self._ep_stats += ended
            self._score[1] += ended
            full = self._score[1, :, 0:1] >= self.score_episodes   # a member's window that is full becomes its last full one (no read of the device)
            self._score[0] = t.where(full, self._score[1], self._score[0])
            self._score[1] = t.where(full, t.zeros_like(ended), self._score[1])
            self._ep_return *= 1.0 - df
            self.obs = obs
        self.num_timesteps += self.num_envs
        return a, obs, r, d

    def draw_batches(self, G):
        """(idx [G, M, B] int64, eps [G, 2, M, B, A]) of G gradient steps, from the trainer's generator: first the indices, then the noise"""
        B, A = self.batch_size, self.env.act_dim
        idx = sample_member_indices(self.gen, self.M, self.R, self.filled_slots, G, B)
        return idx, self.torch.randn((G, 2, self.M, B, A), device=self.device, generator=self.gen)

    def train(self, gradient_steps=None):
        """`gradient_steps` fused steps of every member on fresh samples of its own columns. Returns the number of steps issued."""
        G = self.gradient_steps if gradient_steps is None else int(gradient_steps)
        if G < 1:
            return 0
        idx, eps = self.draw_batches(G)
        arrays = self.replay.arrays()
        for k in range(G):
            self._learner.gradient_step(arrays, idx[k], eps[k, 0], eps[k, 1])
        return G

    def vector_step(self):
        out = self.collect()
        self._vector_steps += 1
        if self.member_timesteps > self.learning_starts:
            self.train()
        return out

    def scores(self):
        """[M] float64 on the device: each member's mean episode reward over its last score_episodes .. 2 score_episodes finished
        episodes (both windows); NaN for a member that has finished none since it was created or last copied over by PBT"""
        s = self._score.sum(0)
        return s[:, 1] / s[:, 0]

    def learn(self, total_timesteps, log=print, log_every=10):
        """vector steps until every member has seen total_timesteps of its own. One progress line with per-member scores every
        log_every vector steps and at every PBT point (one read of the device per line). A record's `episodes` are those finished
        since the line before; its `scores` are scores(), which no line clears. At a PBT point the record has `pbt`: the
        (loser, winner) pairs, or [] where the exploit was skipped because some member had no score yet."""
        L = self._learner
        history, k, t0, steps0 = [], 0, time.perf_counter(), L.step
        while self.member_timesteps < total_timesteps:
            self.vector_step()
            k += 1
            pbt = bool(self.pbt_every) and self._vector_steps % self.pbt_every == 0
            if not (pbt or k % max(1, int(log_every)) == 0 or self.member_timesteps >= total_timesteps):
                continue
            c = self.env.counters()
            if c["nonfinite_states"]:
                raise StepperError("vector step %d: %d env states went non-finite" % (k, c["nonfinite_states"]))
            row = self.torch.cat([L.stats.reshape(-1), L.ent.flat.reshape(-1).double(), self._ep_stats[:, 0], self.scores()]).tolist()   # the one read
            M = self.M
            ep, sc = row[5 * M:6 * M], row[6 * M:7 * M]
            now = time.perf_counter()
            rec = dict(timesteps=self.member_timesteps, scores=sc, episodes=ep, critic_loss=row[0:4 * M:4], actor_loss=row[1:4 * M:4],
                       ent_coef=[math.exp(x) for x in row[4 * M:5 * M]], gradient_steps=L.step, gradient_steps_per_s=(L.step - steps0) / max(now - t0, 1e-9))
            if pbt:
                rec["pbt"] = []
                if self.member_timesteps > self.learning_starts and all(math.isfinite(s) for s in sc):
                    rec["pbt"] = pbt_exploit_sac(sc, L.vectors(), L.hp, self.gen, self.pbt_frac, self.pbt_factors)
                    for loser, _ in rec["pbt"]:
                        self._score[:, loser] = 0.0   # those episodes were the old parameters'
            history.append(rec)
            if log:
                log("member timesteps %9d  mean episode reward per member [%s]  episodes %d  %.0f population gradient steps/s%s"
                    % (self.member_timesteps, " ".join("%.3f" % s for s in sc), int(sum(ep)), rec["gradient_steps_per_s"],
                       "  pbt %s" % (" ".join("%d<-%d" % p for p in rec["pbt"]) or "skipped (a member has no score yet, or pbt_frac x members < 1)") if pbt else ""))
            self._ep_stats.zero_()
            t0, steps0 = now, L.step
        return history

    # ------------------------------------------------------------------------------------------------------------ members, files
    def member_replay_state(self, m):
        """member m's columns of the ring as a ReplayBuffer.state_dict of capacity (capacity / N) * R"""
        N, R, rp = self.num_envs, self.R, self.replay
        slots = rp.size // N
        arrays = [a[:slots * N].unflatten(0, (slots, N))[:, m * R:(m + 1) * R].flatten(0, 1).contiguous().cpu() for a in rp.arrays()]
        return {"pos": rp.pos // N * R, "size": slots * R, "capacity": rp.capacity // N * R, "arrays": arrays}

    def export_member(self, m, path):
        """member m as a checkpoint in SACTrainer.save's (TQCTrainer.save's) format: its nets, three Adam states holding its moments
        and the step count, log_ent_coef, its slice of the env batch, its columns of the replay ring and its hyper-parameters (hp's
        learning_rate is the actor's). `SACTrainer(env_id, num_envs=envs_per_member, buffer_size=(ring rows / N) * envs_per_member)
        .load(path)` reads the file as it is, as do tools/validate.py and tools/rank_checkpoints.py with -s sac / -s tqc. What
        survives the load: the member's three learning rates do, inside the optimisers' state dicts. Its gamma and tau do NOT:
        the trainers' load() ignores the file's `hp`, so a trainer that is to go on training as the member did takes them in its
        constructor (SACTrainer(..., gamma=ck["hp"]["gamma"], tau=ck["hp"]["tau"]))."""
        L, m = self._learner, int(m)
        ck = member_checkpoint(self.algo, self.env.obs_dim, self.env.act_dim, L.pi.flat[m], L.q.flat[m], L.qt.flat[m], L.ent.flat[m],
                               ((L.pi.exp_avg[m], L.pi.exp_avg_sq[m]), (L.q.exp_avg[m], L.q.exp_avg_sq[m]), (L.ent.exp_avg[m], L.ent.exp_avg_sq[m])),
                               L.hp[m].tolist(), L.step, adam_eps=L.adam_eps)
        w, d = self.env.get_state_words()
        lo, hi = m * self.R, (m + 1) * self.R
        ck.update(num_timesteps=self.member_timesteps, env_words=w[:, lo:hi].contiguous().cpu(), env_done=d[lo:hi].contiguous().cpu(),
                  replay=self.member_replay_state(m), ep_return=self._ep_return[lo:hi].cpu())
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.torch.save(ck, path)

    def save(self, path):
        """the whole population: every vector and moment, log_ent_coef, hp, the step count, timesteps, the generator's state, the ring
        with its cursor, the env batch and the episode statistics"""
        L = self._learner
        w, d = self.env.get_state_words()
        names = ("pi", "pi_m", "pi_v", "q", "q_m", "q_v", "qt", "ent", "ent_m", "ent_v")
        pop = dict({k: v.cpu() for k, v in zip(names, L.vectors())}, hp=L.hp.cpu(), step=L.step, num_timesteps=self.num_timesteps, vector_steps=self._vector_steps,
                   generator=self.gen.get_state(), members=self.M, envs_per_member=self.R, algo=self.algo, ep_return=self._ep_return.cpu(), ep_stats=self._ep_stats.cpu(),
                   score=self._score.cpu())
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.torch.save({"population": pop, "env_words": w.cpu(), "env_done": d.cpu(), "replay": self.replay.state_dict(), "hp": self.hp}, path)

    def load(self, path):
        ck = self.torch.load(path, map_location="cpu", weights_only=True)
        pop = ck.get("population")
        if pop is None:
            raise ValueError("%s is not a population checkpoint (a member's file goes to %s.load)" % (path, self.trainer_class.__name__))
        if pop["algo"] != self.algo or int(pop["members"]) != self.M or int(pop["envs_per_member"]) != self.R:
            raise ValueError("%s holds %d x %d members of %s; this population is %d x %d of %s" % (path, pop["members"], pop["envs_per_member"], pop["algo"], self.M, self.R, self.algo))
        L = self._learner
        names = ("pi", "pi_m", "pi_v", "q", "q_m", "q_v", "qt", "ent", "ent_m", "ent_v")
        for dst, key in zip(L.vectors() + (L.hp, self._ep_return, self._ep_stats, self._score), names + ("hp", "ep_return", "ep_stats", "score")):
            dst.copy_(pop[key])
        L.step, self.num_timesteps, self._vector_steps = int(pop["step"]), int(pop["num_timesteps"]), int(pop["vector_steps"])
        self.gen.set_state(pop["generator"].cpu())
        self.env.set_state_words(ck["env_words"].to(self.device), ck["env_done"].to(self.device))
        self.obs = self.env.observe().clone()
        self.replay.load_state_dict(ck["replay"])
        return self

    def close(self):
        self.env.close()


# ---------------------------------------------------------------------------------------- the scripts' flags (train_sac.py, train_tqc.py)
def add_population_arguments(ap):
    ap.add_argument("--population", type=int, default=0, help="train this many learners side by side on one GPU (tennisbot_rl_amd/sac_population.py); "
                    "--num-envs stays the total and must be a multiple of it")
    ap.add_argument("--member-lr", type=str, default=None, help="population: learning rates (all three optimisers), a comma list of 1 or M values")
    ap.add_argument("--member-gamma", type=str, default=None, help="population: discount factors, a comma list of 1 or M values")
    ap.add_argument("--member-tau", type=str, default=None, help="population: Polyak coefficients, a comma list of 1 or M values")
    ap.add_argument("--pbt-every", type=int, default=0, help="population: exploit / explore (pbt_exploit_sac) every this many vector steps; 0: never")


def population_keywords(args):
    """PopulationSAC's keywords (members, envs_per_member, member_hp, pbt_every) from the command line, or None without
    --population. Raises ValueError with the message the script exits with."""
    lists = {"lr": args.member_lr, "gamma": args.member_gamma, "tau": args.member_tau}
    M = int(args.population)
    if M <= 0:
        if M < 0 or args.pbt_every or any(v is not None for v in lists.values()):
            raise ValueError("--member-lr, --member-gamma, --member-tau and --pbt-every belong to --population M (M >= 1)")
        return None
    if args.num_envs % M or args.num_envs < M:
        raise ValueError("--num-envs %d is not a positive multiple of --population %d" % (args.num_envs, M))
    member_hp = {}
    for key, text in lists.items():
        if text is None:
            continue
        try:
            vals = [float(x) for x in text.split(",")]
        except ValueError:
            raise ValueError("--member-%s: a comma list of numbers expected, got %r" % (key, text))
        if len(vals) not in (1, M):
            raise ValueError("--member-%s must hold 1 or %d values (--population), got %d" % (key, M, len(vals)))
        member_hp[key] = vals
    if args.pbt_every < 0:
        raise ValueError("--pbt-every must be >= 0")
    return dict(members=M, envs_per_member=args.num_envs // M, member_hp=member_hp, pbt_every=args.pbt_every)


def run_population(pop, total, path, save_freq=0, log=print, log_every=10):
    """the scripts' run: learn until every member has `total` timesteps; at the end and every save_freq member timesteps the
    population checkpoint at `path` and best_model.pt beside it = export_member(the member with the highest pop.scores()). Members
    without a score (NaN) are not candidates. While no member has one, a best_model.pt this run wrote earlier is kept; if there is
    none yet, member 0 is written, so that the file exists, and the line says that no episode has finished. Returns the history."""
    best_path = os.path.join(os.path.dirname(os.path.abspath(path)), "best_model.pt")
    written = [False]

    def write():
        pop.save(path)
        sc = [float(s) for s in pop.scores().tolist()]
        scored = [m for m in range(pop.M) if math.isfinite(sc[m])]
        if scored:
            best = max(scored, key=sc.__getitem__)   # the first of equals
            pop.export_member(best, best_path)
            log("saved %s and %s (member %d, mean episode reward %.3f)" % (path, best_path, best, sc[best]))
        elif written[0]:
            log("saved %s; %s stays as it is: no member has a score" % (path, best_path))
        else:
            pop.export_member(0, best_path)
            log("saved %s and %s (member 0: no member has finished an episode, so there is no best one yet)" % (path, best_path))
        written[0] = True

    history, next_save = [], save_freq or math.inf
    while pop.member_timesteps < total:
        history += pop.learn(min(total, pop.member_timesteps + max(pop.R * max(1, int(log_every)), int(save_freq or 0))), log=log, log_every=log_every)
        if pop.member_timesteps >= next_save and pop.member_timesteps < total:
            write()
            next_save += save_freq
    write()
    return history
