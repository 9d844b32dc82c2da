"""Plain float64 restatement of the SAC gradient step (tennisbot_rl_amd/sac.py; kernels csrc/tb_sac.hpp): numpy only.

The rule is SB3 1.8.0's SAC with MlpPolicy as the reference scripts select it (train.py:129-130, train_swing.py:93-96):
  * actor  latent_pi.0 (O -> 256), ReLU, latent_pi.2 (256 -> 256), ReLU, then mu (256 -> A) and log_std (256 -> A) clamped to [-20, 2];
    g = mu + exp(log_std) eps, a = tanh(g), logp = sum(-eps^2 / 2 - log_std - ln sqrt(2 pi)) - sum log(1 - a^2 + 1e-6), the
    squash term from a itself;
  * critics qf0, qf1 (and two targets): (O + A) -> 256 -> 256 -> 1, ReLU, on cat(obs, action);
  * one gradient step, in SB3's order: sample on s; alpha = exp(log_ent_coef) BEFORE its update, whose gradient is
    -mean(logp + target_entropy), target_entropy = -A; y = r + (1 - d) gamma (min(Q1t, Q2t)(s', a') - alpha logp'); critic loss
    0.5 (mean (Q1 - y)^2 + mean (Q2 - y)^2) and Adam; actor loss mean(alpha logp - min(Q1, Q2)(s, a~)) with the UPDATED critic,
    its gradient to the actor only, Adam; target <- (1 - tau) target + tau critic. Adam is torch's with eps 1e-8; no clipping.
Gradients come from a hand-written backward pass. Every function takes a `dtype`: with np.float32 it is the float32 twin of itself
(the scheme of tests/ppo_reference.py, whose twin_scale / check_tensors / MULTIPLE set the tolerances).

Parameters are dicts name -> array with SB3's names (ACTOR_NAMES, CRITIC_NAMES: named_parameters() order)."""
import numpy as np

from ppo_reference import BETAS, MULTIPLE, adam_init, adam_step, check_tensors, param_change, twin_scale  # noqa: F401
from policy_reference import LN_SQRT_2PI

HIDDEN = 256
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
SQUASH_EPS = 1e-6
ADAM_EPS = 1e-8
GAMMA, TAU, LR = 0.99, 0.005, 3e-4
DIMS = {0: (6, 6), 1: (12, 2)}     # env kind -> (O, A): SwingRacket-v0, Tennisbot-v0
ACTOR_NAMES = ("latent_pi.0.weight", "latent_pi.0.bias", "latent_pi.2.weight", "latent_pi.2.bias", "mu.weight", "mu.bias", "log_std.weight", "log_std.bias")
CRITIC_NAMES = tuple("qf%d.%d.%s" % (q, layer, w) for q in (0, 1) for layer in (0, 2, 4) for w in ("weight", "bias"))


def actor_shapes(O, A):
    return {"latent_pi.0.weight": (HIDDEN, O), "latent_pi.0.bias": (HIDDEN,), "latent_pi.2.weight": (HIDDEN, HIDDEN), "latent_pi.2.bias": (HIDDEN,),
            "mu.weight": (A, HIDDEN), "mu.bias": (A,), "log_std.weight": (A, HIDDEN), "log_std.bias": (A,)}


def critic_shapes(O, A):
    out = {}
    for q in (0, 1):
        out.update({"qf%d.0.weight" % q: (HIDDEN, O + A), "qf%d.0.bias" % q: (HIDDEN,), "qf%d.2.weight" % q: (HIDDEN, HIDDEN), "qf%d.2.bias" % q: (HIDDEN,),
                    "qf%d.4.weight" % q: (1, HIDDEN), "qf%d.4.bias" % q: (1,)})
    return out


def n_floats(shapes):
    return int(sum(np.prod(s) for s in shapes.values()))


def cast(P, dtype):
    return {k: np.asarray(v).astype(dtype) for k, v in P.items()}


def join_flat(P, names, dtype=np.float32):
    return np.concatenate([np.asarray(P[k], dtype).ravel() for k in names])


def split_flat(flat, shapes):
    out, off = {}, 0
    for k, s in shapes.items():
        n = int(np.prod(s))
        out[k] = np.asarray(flat[off:off + n]).reshape(s)
        off += n
    assert off == len(flat)
    return out


class Pass:
    """one forward pass with what the backward pass and the kink margins need"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _relu(z):
    return np.maximum(z, z.dtype.type(0))


def actor_forward(PA, obs, eps, dtype=np.float64):
    dt = np.dtype(dtype).type
    P, x, eps = cast(PA, dtype), np.asarray(obs).astype(dtype), np.asarray(eps).astype(dtype)
    z1 = x @ P["latent_pi.0.weight"].T + P["latent_pi.0.bias"]
    h1 = _relu(z1)
    z2 = h1 @ P["latent_pi.2.weight"].T + P["latent_pi.2.bias"]
    h2 = _relu(z2)
    mu = h2 @ P["mu.weight"].T + P["mu.bias"]
    raw = h2 @ P["log_std.weight"].T + P["log_std.bias"]
    ls = np.clip(raw, dt(LOG_STD_MIN), dt(LOG_STD_MAX))
    g = mu + np.exp(ls) * eps
    a = np.tanh(g)
    gauss = (dt(-0.5) * eps * eps - ls - dt(LN_SQRT_2PI)).sum(-1, dtype=dtype)
    squash = np.log(dt(1) - a * a + dt(SQUASH_EPS)).sum(-1, dtype=dtype)
    return Pass(x=x, eps=eps, z1=z1, h1=h1, z2=z2, h2=h2, mu=mu, raw=raw, ls=ls, g=g, a=a, logp=gauss - squash)


def critic_forward(PC, q, x, dtype=np.float64):
    P, x = cast(PC, dtype), np.asarray(x).astype(dtype)
    n = "qf%d." % q
    z1 = x @ P[n + "0.weight"].T + P[n + "0.bias"]
    h1 = _relu(z1)
    z2 = h1 @ P[n + "2.weight"].T + P[n + "2.bias"]
    h2 = _relu(z2)
    qv = (h2 @ P[n + "4.weight"].T + P[n + "4.bias"])[:, 0]
    return Pass(x=x, z1=z1, h1=h1, z2=z2, h2=h2, q=qv)


def cat(obs, act, dtype):
    return np.concatenate([np.asarray(obs).astype(dtype), np.asarray(act).astype(dtype)], 1)


def targets(PA, PT, log_ent_coef, next_obs, reward, done, eps_next, gamma=GAMMA, dtype=np.float64, full=False):
    """y [B]; full=True: (y, the actor's pass on s', the two targets' passes)"""
    dt = np.dtype(dtype).type
    pi = actor_forward(PA, next_obs, eps_next, dtype)
    t = [critic_forward(PT, q, cat(next_obs, pi.a, dtype), dtype) for q in (0, 1)]
    alpha = np.exp(dt(log_ent_coef))
    r, d = np.asarray(reward).astype(dtype), np.asarray(done).astype(dtype)
    y = r + (dt(1) - d) * (dt(gamma) * (np.minimum(t[0].q, t[1].q) - alpha * pi.logp))
    return (y, pi, t) if full else y


def _critic_backward(P, q, c, dq, grads=None):
    """dq [B] back through critic q's pass c; fills grads (when given) and returns the gradient of the input rows [B, O + A]"""
    n = "qf%d." % q
    dh2 = dq[:, None] * P[n + "4.weight"]
    dz2 = dh2 * (c.z2 > 0)
    dh1 = dz2 @ P[n + "2.weight"]
    dz1 = dh1 * (c.z1 > 0)
    if grads is not None:
        grads[n + "4.weight"], grads[n + "4.bias"] = (dq[None, :] @ c.h2), dq.sum(keepdims=True, dtype=dq.dtype)
        grads[n + "2.weight"], grads[n + "2.bias"] = dz2.T @ c.h1, dz2.sum(0, dtype=dq.dtype)
        grads[n + "0.weight"], grads[n + "0.bias"] = dz1.T @ c.x, dz1.sum(0, dtype=dq.dtype)
    return dz1 @ P[n + "0.weight"]


def critic_loss_and_grads(PC, obs, act, y, dtype=np.float64, full=False):
    """(loss, grads over CRITIC_NAMES); full=True adds the two passes"""
    dt = np.dtype(dtype).type
    P, y = cast(PC, dtype), np.asarray(y).astype(dtype)
    B = dt(len(y))
    x = cat(obs, act, dtype)
    grads, loss, passes = {}, dt(0), []
    for q in (0, 1):
        c = critic_forward(P, q, x, dtype)
        d = c.q - y
        loss = loss + dt(0.5) * ((d * d).sum(dtype=dtype) / B)
        _critic_backward(P, q, c, d / B, grads)
        passes.append(c)
    grads = {k: grads[k] for k in CRITIC_NAMES}
    return (loss, grads, passes) if full else (loss, grads)


class ActorGrad:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def actor_loss_and_grads(PA, PC, log_ent_coef, obs, eps, dtype=np.float64):
    """loss = mean(alpha logp - min(Q1, Q2)(s, a~)) and its gradient over ACTOR_NAMES (the critic receives none: it is not in
    `grads`), ent_grad = -mean(logp + target_entropy), mean_logp, the actor's pass `pi`, the critics' passes `c`"""
    dt = np.dtype(dtype).type
    PAc, PCc = cast(PA, dtype), cast(PC, dtype)
    pi = actor_forward(PAc, obs, eps, dtype)
    A = pi.a.shape[1]
    B = dt(pi.a.shape[0])
    alpha = np.exp(dt(log_ent_coef))
    c = [critic_forward(PCc, q, cat(obs, pi.a, dtype), dtype) for q in (0, 1)]
    first = c[0].q <= c[1].q
    qmin = np.where(first, c[0].q, c[1].q)
    loss = (alpha * pi.logp - qmin).sum(dtype=dtype) / B
    mean_logp = pi.logp.sum(dtype=dtype) / B
    ent_grad = -((pi.logp + dt(-A)).sum(dtype=dtype) / B)
    O = pi.x.shape[1]
    da = np.zeros_like(pi.a)
    for q, mask in ((0, first), (1, ~first)):
        dq = np.where(mask, dt(-1) / B, dt(0)).astype(dtype)
        da = da + _critic_backward(PCc, q, c[q], dq)[:, O:]
    cc = alpha / B
    one = dt(1) - pi.a * pi.a
    dg = da * one + cc * ((dt(2) * pi.a) * one / (one + dt(SQUASH_EPS)))
    dmu = dg
    dls = np.where((pi.raw < dt(LOG_STD_MIN)) | (pi.raw > dt(LOG_STD_MAX)), dt(0), dg * (np.exp(pi.ls) * pi.eps) - cc).astype(dtype)
    g = {}
    g["mu.weight"], g["mu.bias"] = dmu.T @ pi.h2, dmu.sum(0, dtype=dtype)
    g["log_std.weight"], g["log_std.bias"] = dls.T @ pi.h2, dls.sum(0, dtype=dtype)
    dh2 = dmu @ PAc["mu.weight"] + dls @ PAc["log_std.weight"]
    dz2 = dh2 * (pi.z2 > 0)
    g["latent_pi.2.weight"], g["latent_pi.2.bias"] = dz2.T @ pi.h1, dz2.sum(0, dtype=dtype)
    dz1 = (dz2 @ PAc["latent_pi.2.weight"]) * (pi.z1 > 0)
    g["latent_pi.0.weight"], g["latent_pi.0.bias"] = dz1.T @ pi.x, dz1.sum(0, dtype=dtype)
    return ActorGrad(loss=loss, grads={k: g[k] for k in ACTOR_NAMES}, ent_grad=ent_grad, mean_logp=mean_logp, pi=pi, c=c, first=first)


def polyak(target, params, tau=TAU, dtype=np.float64):
    """SB3's polyak_update: target.mul_(1 - tau), then target += tau * param"""
    dt = np.dtype(dtype).type
    return {k: np.asarray(target[k]).astype(dtype) * dt(1.0 - tau) + dt(tau) * np.asarray(params[k]).astype(dtype) for k in target}


class State:
    """everything a gradient step reads and writes"""

    def __init__(self, actor, critic, target, log_ent_coef=0.0, dtype=np.float64):
        self.dtype = dtype
        self.actor, self.critic, self.target = cast(actor, dtype), cast(critic, dtype), cast(target, dtype)
        self.ent = {"log_ent_coef": np.full(1, log_ent_coef, dtype)}
        self.adam = {"actor": adam_init(self.actor, dtype), "critic": adam_init(self.critic, dtype), "ent": adam_init(self.ent, dtype)}


class Step:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def gradient_step(S, batch, eps_pi, eps_next, gamma=GAMMA, tau=TAU, lr=LR):
    """one SAC gradient step on batch = (obs, next_obs, action, reward, done) in S.dtype; S is updated in place. Returns the
    step's intermediate results."""
    dtype = S.dtype
    obs, next_obs, action, reward, done = batch
    log_alpha = S.ent["log_ent_coef"][0]                                       # alpha of steps 3 and 5: before this step's update
    y, pi_next, t = targets(S.actor, S.target, log_alpha, next_obs, reward, done, eps_next, gamma, dtype, full=True)
    closs, cgrads, cpass = critic_loss_and_grads(S.critic, obs, action, y, dtype, full=True)
    S.critic = adam_step(S.critic, cgrads, S.adam["critic"], lr, eps=ADAM_EPS, dtype=dtype)
    ag = actor_loss_and_grads(S.actor, S.critic, log_alpha, obs, eps_pi, dtype)
    S.actor = adam_step(S.actor, ag.grads, S.adam["actor"], lr, eps=ADAM_EPS, dtype=dtype)
    S.ent = adam_step(S.ent, {"log_ent_coef": np.full(1, ag.ent_grad, dtype)}, S.adam["ent"], lr, eps=ADAM_EPS, dtype=dtype)
    S.target = polyak(S.target, S.critic, tau, dtype)
    return Step(y=y, critic_loss=closs, critic_grads=cgrads, actor=ag, pi_next=pi_next, targets=t, critics=cpass)


# ------------------------------------------------------------------------------------------------------------------------ kinks
def kink_margins(step_or_parts):
    """per row, over the eight passes of a gradient step: (the smallest |hidden pre-activation|, |Q1 - Q2|(s, a~), the distance
    of log_std from its clamp, the largest |g|). `step_or_parts`: a Step, or (actor passes, critic passes, ActorGrad)"""
    if isinstance(step_or_parts, Step):
        s = step_or_parts
        actors, critics, ag = [s.actor.pi, s.pi_next], list(s.critics) + list(s.actor.c) + list(s.targets), s.actor
    else:
        actors, critics, ag = step_or_parts
    relu = np.min([np.minimum(np.abs(p.z1).min(1), np.abs(p.z2).min(1)) for p in actors + critics], 0)
    qgap = np.abs(ag.c[0].q - ag.c[1].q)
    clamp = np.min([np.minimum(p.raw - LOG_STD_MIN, LOG_STD_MAX - p.raw).min(1) for p in actors], 0)
    gmax = np.max([np.abs(p.g).max(1) for p in actors], 0)
    return relu, qgap, clamp, gmax


def sides(step):
    """which side of every kink a step took: the ReLU masks of its eight passes, the smaller critic, the clamp's state"""
    s = step
    out = [p.z1 > 0 for p in [s.actor.pi, s.pi_next] + list(s.critics) + list(s.actor.c) + list(s.targets)]
    out += [p.z2 > 0 for p in [s.actor.pi, s.pi_next] + list(s.critics) + list(s.actor.c) + list(s.targets)]
    out += [s.actor.first] + [(p.raw < LOG_STD_MIN) | (p.raw > LOG_STD_MAX) for p in (s.actor.pi, s.pi_next)]
    return out


def same_sides(a, b):
    return all(np.array_equal(x, y) for x, y in zip(sides(a), sides(b)))
