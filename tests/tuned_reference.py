"""Plain float64 restatement of the tuned network (the reference's `train.py -s tuned_ppo`, train.py:54-67,112-127; kernels:
TunedTrunk / TunedTower in csrc/tb_policy.hpp), numpy only, with the error bound its float32 kernels are checked to.

    f  = ReLU(W1 ReLU(W0 obs + b0) + b1)            O -> 64 -> A          features_extractor.layers.{0,2}, shared
    pi = A -> 32 -> 64 -> 32 (ReLU) -> action_net   32 -> A               policy_net.{0,2,4}, state-independent log_std
    vf = A -> 32 -> 64 -> 32 (ReLU) -> value_net    32 -> 1               value_net_body.{0,2,4}

A is the action dimension: the reference builds the extractor with output_shape=env.action_space.shape[0] (train.py:116-118),
which is 2 on Tennisbot-v0 (tennisbot_env.py:43-44). Flat parameter order = named_parameters() (`layout`):
    log_std | features_extractor W0 b0 W1 b1 | policy_net | value_net_body | action_net | value_net        9639 floats.

Forward bound. The same per-layer bound as policy_reference (Higham's dot-product bound, one rounding per term for the MFMA's
fmaf chain, the underflow term), composed through ReLU instead of tanh: ReLU is computed exactly (a compare and a select) and is
1-Lipschitz, so a layer's error passes through unchanged and the tanh terms (slope, fast_tanh's own 3e-7) drop out. The zero
padding adds nothing: the extractor's padded output rows are fmaf chains of exact zeros, and the towers' first layer multiplies
them by zero weights -- terms that are exactly 0 and round nothing, so that layer's K is A, not 16.

The minibatch gradient is ppo_reference.loss_and_grads's loss -- the same advantage statistics, clipped surrogate, value error
and entropy, term for term -- with the backward pass written for this net: ReLU' = 1 for z > 0 and 0 for z <= 0 (torch's
convention at the kink), and the extractor's gradient the SUM of what the pi tower and the vf tower send back through the
feature. `parts` keeps the two contributions apart. With dtype=np.float32 every function is its own float32 twin.
"""
import numpy as np

import policy_reference as pr
from ppo_reference import ADV_EPS, LN_SQRT_2PI, Loss, cast_params

EXTRACTOR = "features_extractor.layers"
TRUNK_KEYS = tuple("%s.%d.%s" % (EXTRACTOR, k, w) for k in (0, 2) for w in ("weight", "bias"))
# |z| of every hidden pre-activation of a gradient fixture (tests/test_tuned_reference.py). 1e-4 was planned for a float32 forward
# error below 1e-6; the fixtures' torch float32 twin measures 1.8e-6 (sb3) on pre-activations of size ~10, so the margin is
# 100 x that, rounded up
KINK_MARGIN = 2.5e-4


def layout(obs_dim=12, act_dim=2, net_arch=(32, 64, 32), extractor_hidden=64):
    """[(name, shape, offset)] of the flat parameter vector, and its length"""
    rows = [("log_std", (act_dim,))]
    rows += [(EXTRACTOR + ".0.weight", (extractor_hidden, obs_dim)), (EXTRACTOR + ".0.bias", (extractor_hidden,)),
             (EXTRACTOR + ".2.weight", (act_dim, extractor_hidden)), (EXTRACTOR + ".2.bias", (act_dim,))]
    for body in ("policy_net", "value_net_body"):
        d = act_dim
        for j, h in enumerate(net_arch):
            rows += [("%s.%d.weight" % (body, 2 * j), (h, d)), ("%s.%d.bias" % (body, 2 * j), (h,))]
            d = h
    rows += [("action_net.weight", (act_dim, net_arch[-1])), ("action_net.bias", (act_dim,)), ("value_net.weight", (1, net_arch[-1])), ("value_net.bias", (1,))]
    out, off = [], 0
    for name, shape in rows:
        out.append((name, shape, off))
        off += int(np.prod(shape))
    return out, off


def blob_floats(obs_dim=12, act_dim=2, net_arch=(32, 64, 32), extractor_hidden=64):
    """length of the packed blob: per layer ceil(out / 16) tiles of 16 bias floats + chunks x 64 weight floats; log_std padded to 4"""
    lf = lambda n_in, n_out, first: -(-n_out // 16) * (16 + (-(-n_in // 4) if first else 4 * -(-n_in // 16)) * 64)
    total = lf(obs_dim, extractor_hidden, True) + lf(extractor_hidden, act_dim, False)
    tower, d = 0, act_dim
    for h in net_arch:
        tower += lf(d, h, False)
        d = h
    return total + 2 * (tower + lf(d, 16, False)) + -(-act_dim // 4) * 4


def _bodies(sd, body):
    k = 0
    while "%s.%d.weight" % (body, k) in sd:
        yield sd["%s.%d.weight" % (body, k)], sd["%s.%d.bias" % (body, k)]
        k += 2


def _relu(z, e):
    """ReLU and the error bound behind it: exact and 1-Lipschitz; an infinite pre-activation is not a case the kernels are held
    to (they make the env's outputs NaN: 0 x inf in the padded rows)"""
    return np.maximum(z, 0.0), e


def towers(policy, obs, rounds=1):
    """pr.Towers (mean, value, their forward error bounds, log_std) of the tuned net for obs [n, O] (float32 values);
    also .feature [n, A] and .pre: every hidden pre-activation, [n, units] per layer, for the kink margin"""
    sd = pr.state_dict_arrays(policy)
    x = np.asarray(obs, np.float32).astype(np.float64)
    err, pre = np.zeros_like(x), []
    for j, (W, b) in enumerate(_bodies(sd, EXTRACTOR)):
        z, e = pr._layer(W, b, x, err, rounds, j == 0)
        pre.append(z)
        x, err = _relu(z, e)
    feature, ferr = x, err
    outs = []
    for body, head in (("policy_net", "action_net"), ("value_net_body", "value_net")):
        x, err = feature, ferr
        for W, b in _bodies(sd, body):
            z, e = pr._layer(W, b, x, err, rounds, False)
            pre.append(z)
            x, err = _relu(z, e)
        outs.append(pr._layer(sd[head + ".weight"], sd[head + ".bias"], x, err, rounds, False))
    (mean, mean_bound), (value, value_bound) = outs
    t = pr.Towers(mean, value[:, 0], mean_bound, value_bound[:, 0], sd["log_std"])
    t.feature, t.pre = feature, pre
    return t


def kink_margin(policy, obs):
    """min |z| over every hidden pre-activation of every row, in float64"""
    return min(float(np.abs(z).min()) for z in towers(policy, obs).pre)


# ---------------------------------------------------------------------------------------------------------- loss and gradient
def _forward(P, body, x):
    """ReLU layers of `body`: ([input, h1, ...], [z1, ...])"""
    hs, zs = [x], []
    for W, b in _bodies(P, body):
        zs.append(hs[-1] @ W.T + b)
        hs.append(np.maximum(zs[-1], zs[-1].dtype.type(0)))
    return hs, zs


def _backward(P, body, hs, zs, dh, grads, add=False):
    """dh: the loss's derivative with respect to the body's output; returns it with respect to the body's input"""
    for i in reversed(range(len(zs))):
        dz = np.where(zs[i] > 0, dh, dh.dtype.type(0))   # ReLU' = 0 at z <= 0
        kw, kb = "%s.%d.weight" % (body, 2 * i), "%s.%d.bias" % (body, 2 * i)
        gw, gb = dz.T @ hs[i], dz.sum(0)
        grads[kw], grads[kb] = (grads[kw] + gw, grads[kb] + gb) if add else (gw, gb)
        dh = dz @ P[kw]
    return dh


def loss_and_grads(params, obs, act, old_logp, adv, returns, hp, dtype=np.float64):
    """one minibatch of the shared-trunk net: ppo_reference.loss_and_grads's loss and statistics, the gradient of every parameter,
    and in .parts the extractor's gradient split into what came back through the pi tower and through the vf tower"""
    dt = np.dtype(dtype).type
    P = cast_params(params, dtype)
    obs, act, old_logp, adv, returns = (np.asarray(x).astype(dtype) for x in (obs, act, old_logp, adv, returns))
    B = adv.shape[0]
    c, vf, ent = dt(hp["clip_range"]), dt(hp["vf_coef"]), dt(hp["ent_coef"])
    a = (adv - adv.mean(dtype=dtype)) / (adv.std(ddof=1, dtype=dtype) + dt(ADV_EPS))
    hs_f, zs_f = _forward(P, EXTRACTOR, obs)
    hs_pi, zs_pi = _forward(P, "policy_net", hs_f[-1])
    hs_vf, zs_vf = _forward(P, "value_net_body", hs_f[-1])
    mean = hs_pi[-1] @ P["action_net.weight"].T + P["action_net.bias"]
    value = (hs_vf[-1] @ P["value_net.weight"].T + P["value_net.bias"])[:, 0]
    log_std = P["log_std"]
    inv_std = np.exp(-log_std)
    zeta = (act - mean) * inv_std
    logp = (dt(-0.5) * zeta * zeta - log_std - dt(LN_SQRT_2PI)).sum(-1, dtype=dtype)
    ratio = np.exp(logp - old_logp)
    s1, s2 = a * ratio, a * np.clip(ratio, dt(1) - c, dt(1) + c)
    pg = -np.minimum(s1, s2).mean(dtype=dtype)
    verr = returns - value
    vl = (verr * verr).mean(dtype=dtype)
    entropy = (dt(0.5) + dt(LN_SQRT_2PI) + log_std).sum(dtype=dtype)
    loss = pg + vf * vl - ent * entropy
    active = s1 <= s2
    d_logp = np.where(active, -a * ratio, dt(0)) / dt(B)
    grads, parts = {}, {}
    d_mean = (d_logp[:, None] * zeta) * inv_std
    grads["action_net.weight"], grads["action_net.bias"] = d_mean.T @ hs_pi[-1], d_mean.sum(0)
    grads["log_std"] = (d_logp[:, None] * (zeta * zeta - dt(1))).sum(0, dtype=dtype) - ent
    df_pi = _backward(P, "policy_net", hs_pi, zs_pi, d_mean @ P["action_net.weight"], grads)
    d_value = (dt(-2) * vf / dt(B) * verr)[:, None]
    grads["value_net.weight"], grads["value_net.bias"] = d_value.T @ hs_vf[-1], d_value.sum(0)
    df_vf = _backward(P, "value_net_body", hs_vf, zs_vf, d_value @ P["value_net.weight"], grads)
    for name, df in (("pi", df_pi), ("vf", df_vf)):
        parts[name] = {}
        _backward(P, EXTRACTOR, hs_f, zs_f, df, parts[name])
    for k in TRUNK_KEYS:
        grads[k] = parts["pi"][k] + parts["vf"][k]
    stats = {"policy_loss": float(pg), "value_loss": float(vl), "entropy": float(entropy)}
    out = Loss(float(loss), grads, stats, ratio, a, active)
    out.parts = parts
    return out


def flat(named, obs_dim=12, act_dim=2):
    """a dict of named tensors as the flat float64 vector of `layout`"""
    rows, total = layout(obs_dim, act_dim)
    v = np.zeros(total)
    for name, shape, off in rows:
        v[off:off + int(np.prod(shape))] = np.asarray(named[name], np.float64).reshape(-1)
    return v


def unflat(vector, obs_dim=12, act_dim=2):
    rows, _ = layout(obs_dim, act_dim)
    return {name: np.asarray(vector)[off:off + int(np.prod(shape))].reshape(shape) for name, shape, off in rows}


def unpack_layer(blob, n_in, n_out, first):
    """W [n_out, n_in], b [n_out] back out of one layer of the packed blob, and the layer's length: the inverse of the fragment
    order stated in include/tb_stepper.h, written from that statement (not from ppo._fragment_indices); every padded slot
    must hold 0"""
    blob = np.asarray(blob)
    n_tiles = -(-n_out // 16)
    if first:
        chunks = [[4 * c + g for g in range(4)] for c in range(-(-n_in // 4))]
    else:
        chunks = [[16 * u + 4 * g + r for g in range(4)] for u in range(-(-n_in // 16)) for r in range(4)]
    W, b = np.zeros((n_out, n_in), blob.dtype), np.zeros(n_out, blob.dtype)
    p = 0
    for t in range(n_tiles):
        for g in range(4):
            for r in range(4):
                o = 16 * t + 4 * g + r
                if o < n_out:
                    b[o] = blob[p]
                else:
                    assert blob[p] == 0
                p += 1
    for t in range(n_tiles):
        for ks in chunks:
            for g in range(4):
                for j in range(16):
                    o, k = 16 * t + j, ks[g]
                    if o < n_out and k < n_in:
                        W[o, k] = blob[p]
                    else:
                        assert blob[p] == 0
                    p += 1
    return W, b, p
