"""Plain float64 restatement of the TRPO policy step (tennisbot_rl_amd/trpo.py; csrc/tb_trpo.hpp): numpy only, generic in the
layer widths (any tanh MLP in the naming of build_actor_critic).

The rule is the reference's agent.py (TRPOAgent), with the deviations listed in tennisbot_rl_amd/trpo.py:
  * theta = log_std, policy_net.*, action_net.* (THETA picks them out of a parameter dict)
  * the KL of agent.py:92-97 and the surrogate mean(ratio A_hat) of agent.py:99-107, A_hat normalised over the rows given
  * the Fisher-vector product by an explicit JVP (tangent forward pass), the head's scaling by sigma^-2, and the VJP of
    ppo_reference._tower_backward: F v = (1/m) sum_rows J^T diag(sigma^-2) J v on the network, 2 v on log_std, + damping v.
    tests/test_trpo_reference.py holds it against torch's float64 double backprop of the KL (agent.py:144-167).
  * conjugate gradient of agent.py:169-191 (x, r and the scalars float64 in both precisions, p rounded to `dtype`)
  * the line search's table (L_k, KL_k) for theta + beta decay^-k x and the selection rule of agent.py:132

Every function takes a `dtype` and is its own float32 twin, as in tests/ppo_reference.py; tolerances are that file's
`check_tensors` and MULTIPLE. tanh is exact in both precisions (the kernels' fast_tanh is held against it, as there).
"""
import numpy as np

import ppo_reference as ref
from ppo_reference import ADV_EPS, LN_SQRT_2PI, MULTIPLE, cast_params, check_tensors, tensor_ratios, twin_scale  # noqa: F401

KL_DELTA, CG_ITERATIONS, CG_DAMPING, CG_TOLERANCE, CG_STATE_PERCENT = 0.01, 10, 0.001, 1e-10, 0.1   # agent.py:17-18
CANDIDATES, DECAY = 10, 1.5                                                                         # agent.py:112-113


def is_theta(name):
    return name == "log_std" or name.startswith("policy_net.") or name.startswith("action_net.")


def theta_of(d):
    return {k: v for k, v in d.items() if is_theta(k)}


def split_flat(vec, template):
    """a flat vector in the order of `template` (a dict in named_parameters() order) -> dict of arrays shaped like it"""
    out, off = {}, 0
    vec = np.asarray(vec)
    for k, v in template.items():
        n = int(np.size(v))
        out[k] = vec[off:off + n].reshape(np.shape(v))
        off += n
    assert off == vec.size
    return out


def join_flat(d, template, dtype=np.float64):
    """the inverse; names missing from d are zeros"""
    return np.concatenate([np.asarray(d[k], dtype).reshape(-1) if k in d else np.zeros(int(np.size(v)), dtype) for k, v in template.items()])


def mean_of(P, obs, dtype=np.float64):
    """(hidden activations, mean) of the policy tower"""
    return ref._tower(cast_params(theta_of(P), dtype), "policy_net", "action_net", np.asarray(obs).astype(dtype))


def normalise(adv, dtype=np.float64):
    adv = np.asarray(adv).astype(dtype)
    return (adv - adv.mean(dtype=dtype)) / (adv.std(ddof=1, dtype=dtype) + np.dtype(dtype).type(ADV_EPS))


def kl(P, P2, obs, dtype=np.float64):
    """mean over rows of sum_a [(ls' - ls) + (sigma^2 + (mu - mu')^2) / (2 sigma'^2) - 1/2], agent.py:92-97"""
    dt = np.dtype(dtype).type
    _, mu = mean_of(P, obs, dtype)
    _, mu2 = mean_of(P2, obs, dtype)
    ls, ls2 = np.asarray(P["log_std"]).astype(dtype), np.asarray(P2["log_std"]).astype(dtype)
    m = (ls2 - ls) + dt(0.5) * (np.exp(ls) ** 2 + (mu - mu2) ** 2) / np.exp(ls2) ** 2 - dt(0.5)
    return float(m.sum(-1, dtype=dtype).mean(dtype=dtype))


def surrogate(P2, obs, act, old_logp, adv_norm, dtype=np.float64):
    """mean(ratio A_hat), agent.py:99-107; adv_norm: already normalised"""
    dt = np.dtype(dtype).type
    _, mu = mean_of(P2, obs, dtype)
    ls = np.asarray(P2["log_std"]).astype(dtype)
    zeta = (np.asarray(act).astype(dtype) - mu) * np.exp(-ls)
    logp = (dt(-0.5) * zeta * zeta - ls - dt(LN_SQRT_2PI)).sum(-1, dtype=dtype)
    ratio = np.exp(logp - np.asarray(old_logp).astype(dtype))
    return float((ratio * np.asarray(adv_norm).astype(dtype)).mean(dtype=dtype))


def surrogate_gradient(P, obs, act, old_logp, adv, dtype=np.float64):
    """g = grad_theta mean(ratio A_hat) at P (adv: raw, normalised here): minus the policy part of the PPO loss's gradient with
    a clip that never binds and no entropy term"""
    hp = dict(clip_range=np.inf, vf_coef=0.0, ent_coef=0.0)
    res = ref.loss_and_grads(P, obs, act, old_logp, adv, np.zeros(len(np.asarray(adv))), hp, dtype)
    return {k: -v for k, v in res.grads.items() if is_theta(k)}


def fvp(P, obs, v, damping=CG_DAMPING, dtype=np.float64):
    """F v + damping v over the rows of obs; v and the result: dicts over theta"""
    dt = np.dtype(dtype).type
    Pt, V = cast_params(theta_of(P), dtype), cast_params(theta_of(v), dtype)
    hs, _ = ref._tower(Pt, "policy_net", "action_net", np.asarray(obs).astype(dtype))
    m = hs[0].shape[0]
    hd = None                                      # the tangent of the layer's input (the observation has none)
    for i in range(len(hs) - 1):
        W, name = Pt["policy_net.%d.weight" % (2 * i)], "policy_net.%d" % (2 * i)
        zd = hs[i] @ V[name + ".weight"].T + V[name + ".bias"]
        if hd is not None:
            zd = zd + hd @ W.T
        hd = (dt(1) - hs[i + 1] * hs[i + 1]) * zd
    mud = hs[-1] @ V["action_net.weight"].T + V["action_net.bias"] + hd @ Pt["action_net.weight"].T
    d_out = mud * np.exp(dt(-2) * Pt["log_std"]) / dt(m)
    out = {}
    ref._tower_backward(Pt, "policy_net", "action_net", hs, d_out, out)
    out["log_std"] = dt(2) * V["log_std"]
    return {k: out[k] + dt(damping) * V[k] for k in Pt}


def dot(a, b):
    return float(sum((np.asarray(a[k], np.float64) * np.asarray(b[k], np.float64)).sum() for k in a))


def conjugate_gradient(apply, b, iterations=CG_ITERATIONS, tolerance=CG_TOLERANCE, dtype=np.float64):
    """agent.py:169-191: x ~ A^-1 b for `apply`(p) = A p on dicts. x, r and the scalars are float64 in both precisions; p is
    rounded to `dtype` before every product, and the product is what `apply` returns. Stops once rdotr < tolerance."""
    p = {k: np.asarray(v).astype(dtype) for k, v in b.items()}
    r = {k: np.asarray(v).astype(dtype).astype(np.float64) for k, v in b.items()}
    x = {k: np.zeros_like(v) for k, v in r.items()}
    rdotr = dot(r, r)
    for _ in range(iterations):
        f = {k: np.asarray(v, np.float64) for k, v in apply(p).items()}
        pd = {k: v.astype(np.float64) for k, v in p.items()}
        alpha = rdotr / dot(pd, f)
        x = {k: x[k] + alpha * pd[k] for k in x}
        r = {k: r[k] - alpha * f[k] for k in r}
        new = dot(r, r)
        p = {k: (r[k] + (new / rdotr) * pd[k]).astype(dtype) for k in r}
        rdotr = new
        if rdotr < tolerance:
            break
    return x


def step_size(x, Fx, delta=KL_DELTA):
    """beta = sqrt(2 delta / x^T F x), agent.py:110-111"""
    return float(np.sqrt(2.0 * delta / dot(x, Fx)))


def moved(P, x, step, dtype=np.float64):
    """theta + step x (the value tower as it is)"""
    dt = np.dtype(dtype).type
    return {k: (np.asarray(v).astype(dtype) + dt(step) * np.asarray(x[k]).astype(dtype)) if is_theta(k) else np.asarray(v).astype(dtype) for k, v in P.items()}


def search_table(P, x, steps, obs, act, old_logp, adv, dtype=np.float64):
    """[K, 2]: (L_k, KL_k) of theta + steps[k] x over the rows given; adv raw"""
    a = normalise(adv, dtype)
    out = np.zeros((len(steps), 2))
    for k, s in enumerate(steps):
        P2 = moved(P, x, s, dtype)
        out[k] = surrogate(P2, obs, act, old_logp, a, dtype), kl(P, P2, obs, dtype)
    return out


def select(table, delta=KL_DELTA):
    """the first k that is finite with KL_k <= delta and L_k >= 0 (agent.py:132), or -1"""
    for k, (L, KL) in enumerate(np.asarray(table, np.float64)):
        if np.isfinite(L) and np.isfinite(KL) and KL <= delta and L >= 0.0:
            return k
    return -1


def threshold_margins(table, twin_table, delta=KL_DELTA):
    """per candidate: the distance of KL_k from delta and of L_k from 0, in twin errors of that very number (floored at
    u |value| as twin_scale does): [K, 2]"""
    t, w = np.asarray(table, np.float64), np.asarray(twin_table, np.float64)
    scale = np.maximum(np.abs(w - t), ref.U32 * np.maximum(np.abs(t), np.array([0.0, delta])))
    return np.stack([np.abs(t[:, 0]) / scale[:, 0], np.abs(t[:, 1] - delta) / scale[:, 1]], 1)
