"""Plain float64 restatement of the fused policy half (csrc/tb_policy.hpp), with the error bounds it is checked to.

What tb_policy_step / tb_policy_rollout compute per env and step, from nothing but the torch state dict and the noise key:

  * the towers (SB3 MlpPolicy, separate pi / vf, tanh hidden layers), with the weights rounded to float32 as the blob holds
    them and everything else in float64, plus a forward error bound per output for the kernel's float32 arithmetic;
  * the exploration noise: Philox4x32-10 keyed like policy_noise, Box-Muller in float64 from the kernel's own 24-bit uniforms;
  * the sample: raw = mean + exp(log_std) eps, action = raw clipped to [-1, 1] with NaN kept (np.clip / torch.clamp),
    logp = sum(-eps^2 / 2 - log_std - ln(2 pi) / 2).

Error bound of one layer z = b + sum_k W[k] x[k] (Higham's dot-product bound, any summation order):
    err(z) <= sum |W| err(x) + gamma_m (|b| + sum |W| (|x| + err(x))) + underflow,   gamma_m = m u / (1 - m u),  u = 2^-24,
with m = rounds (K + 1) for K terms and the bias: rounds = 1 for v_mfma_f32_16x16x4_f32 (bit for bit a k-ordered fmaf chain,
one rounding per term), 2 for an emulation that rounds every product and every sum. The underflow term covers subnormal
inputs and products flushed to zero: (K + 1 + sum |W|) 2^-126. After tanh: tanh is 1-Lipschitz and, on [|z| - err, |z| + err],
has slope at most sech^2(max(|z| - err, 0)); fast_tanh adds its own 3e-7 (the bound stated in tb_policy.hpp). A pre-activation
that is infinite (an infinite observation) saturates both tanh's exactly: error 0 after the layer. Observations are exact float32:
the first layer starts from err = 0.
"""
import math

import numpy as np

U32 = 2.0 ** -24
FAST_TANH_ERR = 3e-7
UNDERFLOW = 2.0 ** -126
LN_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
M32 = 0xFFFFFFFF
NOISE_KEY_TAG = 0x504F4C49  # "POLI": xored into the high key word, so the policy noise never repeats the reset draws

# Absolute error of one float32 standard normal of policy_noise against the float64 Box-Muller of the same two uniforms. The
# uniforms themselves are exact (24-bit integers times 2^-24). |eps| <= r_max = sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.77.
#   r = sqrtf(-2 logf(u1)):  logf and sqrtf are correctly rounded to within 1 ulp each; -2 L is exact. A relative error d in
#     L = -2 ln u1 is d / 2 in r, so r carries at most (1 + 1/2 + ...) ~ 2 ulp relative: 2 * 2^-23 * 5.77 = 1.4e-6 absolute.
#   th = 2 pi u2:  the float32 constant 6.2831855f is 1.7e-7 above 2 pi (times u2 < 1), and the product rounds by at most half
#     an ulp of a value below 2 pi (2.4e-7): |dth| <= 4.1e-7, i.e. r |dth| <= 5.77 * 4.1e-7 = 2.4e-6.
#   cosf / sinf: within 2 ulp of a result <= 1 (2.4e-7 relative to 1), times r: 1.4e-6.
#   r * cos(th): half an ulp of a value <= 5.77: 2.4e-7.
# Sum 5.5e-6; the tolerance keeps 8e-6.
EPS_TOL = 8e-6


def gamma(m):
    return m * U32 / (1.0 - m * U32)


def philox4x32(ctr, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11), from the paper. Works on Python ints and, element-wise, on numpy
    uint64 arrays holding 32-bit words (the products of two 32-bit words fit)."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def box_muller(u_a, u_b):
    """two standard normals from two 32-bit Philox words, as policy_noise forms them: the top 24 bits, u1 in (0, 1], u2 in [0, 1)"""
    u1 = ((np.asarray(u_a, np.uint64) >> np.uint64(8)).astype(np.float64) + 1.0) * U32
    u2 = (np.asarray(u_b, np.uint64) >> np.uint64(8)).astype(np.float64) * U32
    r, th = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return r * np.cos(th), r * np.sin(th)


def policy_noise(seed, env_id, episode, step_count, n_act):
    """eps [..., n_act] in float64: counter (env_lo, env_hi, episode, 4 step_count + block), key (seed_lo, seed_hi ^ "POLI");
    env_id, episode, step_count broadcast against each other (step_count taken modulo 2^32 like the kernel's uint32 cast)"""
    env_id, episode, step_count = np.broadcast_arrays(np.asarray(env_id, np.uint64), np.asarray(episode, np.uint64),
                                                      np.asarray(step_count, np.int64).astype(np.uint64) & np.uint64(M32))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (np.uint64(seed & M32), np.uint64((seed >> 32) ^ NOISE_KEY_TAG))
    m = np.uint64(M32)
    eps = []
    for blk in range((n_act + 3) // 4):
        ctr = (env_id & m, env_id >> np.uint64(32), episode & m, (step_count * np.uint64(4) + np.uint64(blk)) & m)
        u = philox4x32(ctr, key)
        for pair in range(2):
            eps += list(box_muller(u[2 * pair], u[2 * pair + 1]))
    return np.stack(eps[:n_act], -1)


def state_dict_arrays(policy):
    """the module's parameters as the blob holds them: float32 values, widened to float64"""
    sd = policy.state_dict() if hasattr(policy, "state_dict") else policy
    out = {}
    for k, v in sd.items():
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v).astype(np.float32).astype(np.float64)
    return out


def _layer(W, b, x, err, rounds, first):
    """one affine layer in float64 and its error bound; x, err [n, K]; W [out, K]"""
    K = W.shape[1]
    if first:
        K = -(-K // 4) * 4  # the first layer's k is padded to a multiple of 4 with zero terms
    aW = np.abs(W)
    with np.errstate(invalid="ignore", over="ignore"):
        z = x @ W.T + b
        prop = err @ aW.T
        mag = np.abs(b) + (np.abs(x) + err) @ aW.T
        e = prop + gamma(rounds * (K + 1)) * mag + (K + 1 + aW.sum(1)) * UNDERFLOW
    return z, e


def _tanh(z, e):
    with np.errstate(invalid="ignore", over="ignore"):
        slope = 1.0 / np.cosh(np.maximum(np.abs(z) - e, 0.0)) ** 2
        e_out = np.minimum(slope * e, 2.0) + FAST_TANH_ERR
    return np.tanh(z), np.where(np.isinf(z), 0.0, e_out)


class Towers:
    """mean [n, A], value [n] in float64; mean_bound, value_bound: the forward error bound of the kernel's float32 towers"""

    def __init__(self, mean, value, mean_bound, value_bound, log_std):
        self.mean, self.value, self.mean_bound, self.value_bound, self.log_std = mean, value, mean_bound, value_bound, log_std


def towers(policy, obs, rounds=1):
    """both towers for obs [n, O] (float32 values); `policy`: an ActorCritic or its state dict"""
    sd = state_dict_arrays(policy)
    x0 = np.asarray(obs, np.float32).astype(np.float64)
    outs = []
    for body, head in (("policy_net", "action_net"), ("value_net_body", "value_net")):
        x, err, k = x0, np.zeros_like(x0), 0
        while "%s.%d.weight" % (body, k) in sd:
            z, e = _layer(sd["%s.%d.weight" % (body, k)], sd["%s.%d.bias" % (body, k)], x, err, rounds, k == 0)
            x, err = _tanh(z, e)
            k += 2
        outs.append(_layer(sd[head + ".weight"], sd[head + ".bias"], x, err, rounds, False))
    (mean, mean_bound), (value, value_bound) = outs
    return Towers(mean, value[:, 0], mean_bound, value_bound[:, 0], sd["log_std"])


FIXED_TOL = 2e-5  # test_gpu_policy.POLICY_TOL: the suite's tolerance for the towers under SB3's init on the envs' own observations


def tower_tol(bound, cap=None):
    """tolerance of a kernel's mean / value: twice the forward error bound, and never looser than `cap` where one applies"""
    tol = 2.0 * np.asarray(bound)
    return tol if cap is None else np.minimum(tol, cap)


def clip_action(raw):
    """np.clip to [-1, 1]: NaN stays NaN (SB3 clips Box actions with np.clip before env.step)"""
    return np.clip(raw, -1.0, 1.0)


def sample(mean, log_std, eps):
    """raw, action, logp of the kernel's sampling in float64"""
    raw = mean + np.exp(log_std) * eps
    logp = (-0.5 * eps ** 2 - log_std - LN_SQRT_2PI).sum(-1)
    return raw, clip_action(raw), logp


def raw_tol(mean_bound, log_std, eps, mean):
    """|raw - (mean + std eps)|: the mean's tolerance, the noise's scaled by std (expf within 2 ulp), the fmaf's rounding"""
    std = np.exp(log_std)
    return 2.0 * mean_bound + std * (EPS_TOL + 2.5e-7 * np.abs(eps)) + 6e-8 * (np.abs(mean) + std * np.abs(eps)) * 1.01


def logp_tol(log_std, eps):
    """|logp - sum(-eps^2/2 - log_std - ln(2 pi)/2)|: eps's tolerance through eps^2 / 2, plus float32 rounding of the
    fmaf, the constant's subtraction and the running sum (3 roundings per action dimension)"""
    A = eps.shape[-1]
    terms = 0.5 * eps ** 2 + np.abs(log_std) + LN_SQRT_2PI
    return (np.abs(eps) * EPS_TOL + EPS_TOL ** 2).sum(-1) + gamma(3 * A + 1) * terms.sum(-1) + A * 3e-8


def excess(got, want, tol):
    """max |got - want| / tol over the finite elements (0 for none), and the index of the worst; NaN where one side is NaN
    and the other is not counts as infinitely far"""
    got, want, tol = np.asarray(got, np.float64), np.asarray(want, np.float64), np.broadcast_to(tol, np.shape(want))
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want)
        both_nan = np.isnan(got) & np.isnan(want)
        d = np.where(both_nan, 0.0, np.where(np.isnan(d), np.inf, d))
        d = np.where(np.isinf(got) & (got == want), 0.0, d)
        r = np.where(d == 0.0, 0.0, d / tol)
        r = np.where(np.isnan(r), np.inf, r)  # a NaN bound only excuses exact agreement
    if r.size == 0:
        return 0.0, None
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), i


def assert_within(name, got, want, tol):
    """every element within its tolerance; returns the largest |error| / tolerance"""
    r, i = excess(got, want, tol)
    if not r <= 1.0:
        g, w, t = np.asarray(got)[i], np.asarray(want)[i], np.broadcast_to(tol, np.shape(want))[i]
        raise AssertionError("%s at %s: got %r, want %r, |error| %.3g > tolerance %.3g (%.3g x)" % (name, i, g, w, abs(g - w), t, r))
    return r


def episode_keys(episode0, step_count0, dones):
    """(episode, step_count) [T, n] that each step's noise is keyed by, from the state before the first step and the done flags:
    an env whose step ends its episode is reset inside it (episode + 1, step_count 0), every other step counts one"""
    dones = np.asarray(dones) != 0
    T, n = dones.shape
    ep, sc = np.empty((T, n), np.int64), np.empty((T, n), np.int64)
    e, s = np.asarray(episode0, np.int64).copy(), np.asarray(step_count0, np.int64).copy()
    for t in range(T):
        ep[t], sc[t] = e, s
        e = np.where(dones[t], e + 1, e)
        s = np.where(dones[t], 0, s + 1)
    return ep, sc, e, s
