"""Plain float64 restatement of the TQC gradient step (tennisbot_rl_amd/tqc.py; kernels csrc/tb_tqc.hpp): numpy only.

The rule is sb3_contrib 1.8.0's TQC with MlpPolicy at its defaults, as the reference's train_swing.py:98-99 selects it:
  * the actor is SAC's (sac_reference.actor_forward), and so are Adam and the Polyak update;
  * critics qf0, qf1 (and two targets): (O + A) -> 256 -> 256 -> 25, ReLU, on cat(obs, action): 25 quantiles each;
  * one gradient step: sample on s; alpha = exp(log_ent_coef) BEFORE its update, whose gradient is -mean(logp - A);
    z = sort(concat(Q1t, Q2t)(s', a')) ascending, the first 46 of 50 kept, y[b][j] = r + (1 - d) gamma (z[j] - alpha logp'), a
    terminal row selected (y = r bit for bit); critic loss = the mean over (b, n, i, j) of |tau_i - [delta < 0]| H(delta) with
    delta = y[b][j] - theta[b][n][i], tau_i = (i + 0.5) / 25, H(delta) = |delta| - 0.5 where |delta| > 1, delta^2 / 2 elsewhere,
    and Adam; actor loss mean(alpha logp - Qbar(s, a~)) with the UPDATED critic, Qbar the mean over the 25 quantiles and the 2
    critics, its gradient to the actor only, Adam; target <- (1 - tau) target + tau critic.
Gradients come from a hand-written backward pass: d loss / d theta[b][n][i] = -(1 / (B 2300)) sum_j |tau_i - [delta < 0]|
clamp(delta, -1, 1), and -1 / (50 B) for each of a row's 50 head outputs under the actor loss. Every function takes a `dtype`:
with np.float32 it is the float32 twin of itself (the scheme of tests/ppo_reference.py).

Parameters are dicts name -> array with sb3_contrib's names (ACTOR_NAMES, CRITIC_NAMES: named_parameters() order)."""
import numpy as np

from sac_reference import (ACTOR_NAMES, ADAM_EPS, CRITIC_NAMES, DIMS, GAMMA, HIDDEN, LOG_STD_MAX, LOG_STD_MIN, LR, SQUASH_EPS, TAU, Pass, _relu, actor_forward,  # noqa: F401
                           actor_shapes, adam_init, adam_step, cast, cat, join_flat, n_floats, param_change, polyak, split_flat)

N_QUANTILES, N_CRITICS, DROP_PER_NET = 25, 2, 2
N_ALL = N_CRITICS * N_QUANTILES                     # 50
N_TARGETS = N_ALL - N_CRITICS * DROP_PER_NET        # 46


def critic_shapes(O, A):
    out = {}
    for q in range(N_CRITICS):
        out.update({"qf%d.0.weight" % q: (HIDDEN, O + A), "qf%d.0.bias" % q: (HIDDEN,), "qf%d.2.weight" % q: (HIDDEN, HIDDEN), "qf%d.2.bias" % q: (HIDDEN,),
                    "qf%d.4.weight" % q: (N_QUANTILES, HIDDEN), "qf%d.4.bias" % q: (N_QUANTILES,)})
    return out


def critic_forward(PC, q, x, dtype=np.float64):
    """critic q on the rows x: Pass.q [B, 25]"""
    P, x = cast(PC, dtype), np.asarray(x).astype(dtype)
    n = "qf%d." % q
    z1 = x @ P[n + "0.weight"].T + P[n + "0.bias"]
    h1 = _relu(z1)
    z2 = h1 @ P[n + "2.weight"].T + P[n + "2.bias"]
    h2 = _relu(z2)
    return Pass(x=x, z1=z1, h1=h1, z2=z2, h2=h2, q=h2 @ P[n + "4.weight"].T + P[n + "4.bias"])


def targets(PA, PT, log_ent_coef, next_obs, reward, done, eps_next, gamma=GAMMA, dtype=np.float64, full=False):
    """y [B, 46]; full=True: (y, the actor's pass on s', the two targets' passes). np.sort puts a NaN last, as torch.sort does."""
    dt = np.dtype(dtype).type
    pi = actor_forward(PA, next_obs, eps_next, dtype)
    t = [critic_forward(PT, q, cat(next_obs, pi.a, dtype), dtype) for q in range(N_CRITICS)]
    z = np.sort(np.concatenate([c.q for c in t], 1), 1)[:, :N_TARGETS]
    alpha = np.exp(dt(log_ent_coef))
    r, d = np.asarray(reward).astype(dtype)[:, None], np.asarray(done).astype(dtype)[:, None]
    y = np.where(d != 0, np.broadcast_to(r, z.shape), r + dt(gamma) * (z - (alpha * pi.logp)[:, None])).astype(dtype)
    return (y, pi, t) if full else y


def _critic_backward(P, q, c, dq, grads=None):
    """dq [B, 25] back through critic q's pass c; fills grads (when given) and returns the gradient of the input rows [B, O + A]"""
    n = "qf%d." % q
    dz2 = (dq @ P[n + "4.weight"]) * (c.z2 > 0)
    dz1 = (dz2 @ P[n + "2.weight"]) * (c.z1 > 0)
    if grads is not None:
        grads[n + "4.weight"], grads[n + "4.bias"] = dq.T @ c.h2, dq.sum(0, dtype=dq.dtype)
        grads[n + "2.weight"], grads[n + "2.bias"] = dz2.T @ c.h1, dz2.sum(0, dtype=dq.dtype)
        grads[n + "0.weight"], grads[n + "0.bias"] = dz1.T @ c.x, dz1.sum(0, dtype=dq.dtype)
    return dz1 @ P[n + "0.weight"]


def quantile_huber(theta, y, dtype=np.float64):
    """theta [B, 25], y [B, 46]: (the sum of the B 25 46 loss terms, the sum over j of |tau_i - [delta < 0]| clamp(delta, -1, 1) [B, 25])"""
    dt = np.dtype(dtype).type
    tau = ((np.arange(N_QUANTILES).astype(dtype) + dt(0.5)) / dt(N_QUANTILES))[None, :, None]
    delta = y[:, None, :] - theta[:, :, None]
    w = np.where(delta < 0, dt(1) - tau, tau).astype(dtype)
    ad = np.abs(delta)
    huber = np.where(ad > 1, ad - dt(0.5), dt(0.5) * delta * delta).astype(dtype)
    return (w * huber).sum(dtype=dtype), (w * np.clip(delta, dt(-1), dt(1))).sum(2, dtype=dtype)


def critic_loss_and_grads(PC, obs, act, y, dtype=np.float64, full=False):
    """(loss, grads over CRITIC_NAMES); full=True adds the two passes. y [B, 46]."""
    dt = np.dtype(dtype).type
    P, y = cast(PC, dtype), np.asarray(y).astype(dtype)
    terms = dt(len(y) * N_ALL * N_TARGETS)
    x = cat(obs, act, dtype)
    grads, loss, passes = {}, dt(0), []
    for q in range(N_CRITICS):
        c = critic_forward(P, q, x, dtype)
        total, g = quantile_huber(c.q, y, dtype)
        loss = loss + total / terms
        _critic_backward(P, q, c, -g / terms, grads)
        passes.append(c)
    grads = {k: grads[k] for k in CRITIC_NAMES}
    return (loss, grads, passes) if full else (loss, grads)


class ActorGrad:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def actor_loss_and_grads(PA, PC, log_ent_coef, obs, eps, dtype=np.float64):
    """loss = mean(alpha logp - Qbar(s, a~)) and its gradient over ACTOR_NAMES (the critic receives none: it is not in `grads`),
    ent_grad = -mean(logp + target_entropy), mean_logp, the actor's pass `pi`, the critics' passes `c`"""
    dt = np.dtype(dtype).type
    PAc, PCc = cast(PA, dtype), cast(PC, dtype)
    pi = actor_forward(PAc, obs, eps, dtype)
    A, O = pi.a.shape[1], pi.x.shape[1]
    B = dt(pi.a.shape[0])
    alpha = np.exp(dt(log_ent_coef))
    c = [critic_forward(PCc, q, cat(obs, pi.a, dtype), dtype) for q in range(N_CRITICS)]
    qbar = np.concatenate([p.q for p in c], 1).sum(1, dtype=dtype) / dt(N_ALL)
    loss = (alpha * pi.logp - qbar).sum(dtype=dtype) / B
    mean_logp = pi.logp.sum(dtype=dtype) / B
    ent_grad = -((pi.logp + dt(-A)).sum(dtype=dtype) / B)
    da = np.zeros_like(pi.a)
    for q in range(N_CRITICS):
        dq = np.full_like(c[q].q, dt(-1) / (dt(N_ALL) * B))
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
    return ActorGrad(loss=loss, grads={k: g[k] for k in ACTOR_NAMES}, ent_grad=ent_grad, mean_logp=mean_logp, pi=pi, c=c)


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
    """one TQC gradient step on batch = (obs, next_obs, action, reward, done) in S.dtype; S is updated in place. Returns the
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
# ReLU and the log_std clamp are TQC's kinks. The sort and the truncation are continuous in their inputs, the quantile weight's
# jump at delta = 0 multiplies clamp(delta) = 0, and the Huber gradient is continuous at |delta| = 1: no condition on those.
def kink_margins(step_or_parts):
    """per row, over the eight passes of a gradient step: (the smallest |hidden pre-activation|, the distance of log_std from its
    clamp, the largest |g|). `step_or_parts`: a Step, or (actor passes, critic passes)"""
    if isinstance(step_or_parts, Step):
        s = step_or_parts
        actors, critics = [s.actor.pi, s.pi_next], list(s.critics) + list(s.actor.c) + list(s.targets)
    else:
        actors, critics = step_or_parts[:2]
    relu = np.min([np.minimum(np.abs(p.z1).min(1), np.abs(p.z2).min(1)) for p in actors + critics], 0)
    clamp = np.min([np.minimum(p.raw - LOG_STD_MIN, LOG_STD_MAX - p.raw).min(1) for p in actors], 0)
    gmax = np.max([np.abs(p.g).max(1) for p in actors], 0)
    return relu, clamp, gmax


def sides(step):
    """which side of every kink a step took: the ReLU masks of its eight passes and the clamp's state"""
    s = step
    passes = [s.actor.pi, s.pi_next] + list(s.critics) + list(s.actor.c) + list(s.targets)
    return [p.z1 > 0 for p in passes] + [p.z2 > 0 for p in passes] + [(p.raw < LOG_STD_MIN) | (p.raw > LOG_STD_MAX) for p in (s.actor.pi, s.pi_next)]


def same_sides(a, b):
    return all(np.array_equal(x, y) for x, y in zip(sides(a), sides(b)))
