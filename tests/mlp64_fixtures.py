"""Shared inputs of the TB_NET_MLP64 tests (SB3's [64, 64] on SwingRacket-v0) and of sb3_contrib's TRPO form: the policy and synthetic
rollout of tests/test_ppo_reference.py on the new architecture, the numpy twin of trpo.select_candidate_sb3, the line search's
fixtures with sb3_contrib's decay and the zero step in front, and their margins from BOTH of its thresholds (KL = delta, L = L_0).
numpy only apart from the policy; everything here is computed once and shared."""
import types

import numpy as np

import ppo_reference as ref
import trpo_reference as tr
from learner_edge_fixtures import logp64
from test_ppo_reference import flat_shard, make_policy

ARCH = (64, 64)
BLOB_FLOATS, PARAM_FLOATS = 11560, 9677          # 2 (576 + 4160 + 1040) + 8;  6 + 2 (64 7 + 64 65) + 6 65 + 65
ORDER = ["log_std", "policy_net.0.weight", "policy_net.0.bias", "policy_net.2.weight", "policy_net.2.bias", "value_net_body.0.weight", "value_net_body.0.bias",
         "value_net_body.2.weight", "value_net_body.2.bias", "action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias"]
# sb3_contrib 1.8.0's TRPO defaults as the issue lists them: the dict in trpo.py is held against THIS copy
SB3 = dict(kl_delta=0.01, cg_iterations=15, cg_damping=0.1, cg_tolerance=1e-10, cg_state_percent=1.0, search_candidates=10, search_decay=1.25,
           n_epochs=10, learning_rate=1e-3, vf_coef=1.0, gae_lambda=0.95, gamma=0.99, max_grad_norm=float("inf"))
MARGIN = 100.0
ROWS = (2, 16, 17, 128, 129, 256, 257, 600)      # the tile, half-share and workgroup edges of tb_trpo_fvp
SEARCH_ROWS = ROWS + (1025,)                     # ... and one past a search workgroup's share
_cache = {}


def policy(seed=11):
    from tennisbot_rl_amd.params import ENV_SWING
    return make_policy(ARCH, ENV_SWING, seed)


def rollout():
    """test_ppo_reference.make_rollout's "swing-52-lockstep" on the [64, 64] net: 52 steps x 300 envs, an episode end every 26 steps"""
    if "ro" in _cache:
        return _cache["ro"]
    import torch
    from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, OBS_DIM
    from tennisbot_rl_amd.ppo import COMMON, SB3_SWING_DEFAULTS
    T, n, kind = 52, 300, ENV_SWING
    hp = dict(SB3_SWING_DEFAULTS)
    assert tuple(hp["net_arch"]) == ARCH
    hp.update(COMMON)
    hp["ent_coef"] = 0.002                                 # (SB3's 0 would leave the entropy term of log_std's gradient untested)
    rng = np.random.default_rng(6464)
    O, A = OBS_DIM[kind], ACT_DIM[kind]
    dones = np.broadcast_to(np.arange(T)[:, None] % 26 == 25, (T, n)).copy()
    dones[:, 0] = False
    dones[:, 1] = False; dones[0, 1] = dones[T - 1, 1] = True
    rewards = rng.normal(0.0, 0.3, (T, n)) + 2.0 * (rng.random((T, n)) < 0.1) + 50.0 * (dones & (rng.random((T, n)) < 0.3))
    obs = rng.normal(0.0, 1.5, (T, n, O)).astype(np.float32)
    pol = policy()
    with torch.no_grad():
        mean, v_pred = pol(torch.from_numpy(obs.reshape(T * n, O)))
        raw = mean + pol.log_std.exp() * torch.from_numpy(rng.normal(size=(T * n, A)).astype(np.float32))
        _, logp, _ = pol.evaluate(torch.from_numpy(obs.reshape(T * n, O)), raw)
    old_logp = logp.numpy().reshape(T, n) + rng.normal(0.0, 0.25, (T, n))
    values = 12.0 + 8.0 * rng.normal(size=(T, n)) + v_pred.numpy().reshape(T, n)
    f = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    ro = types.SimpleNamespace(name="swing64-52-lockstep", kind=kind, arch=ARCH, T=T, n=n, O=O, A=A, hp=hp, batch=7500, dones=dones.astype(np.uint8), rewards=f(rewards),
                               obs=obs, raw=f(raw.numpy().reshape(T, n, A)), old_logp=f(old_logp), values=f(values), v_pred=f(v_pred.numpy().reshape(T, n)),
                               last_value=f(12.0 + 8.0 * rng.normal(size=n)))
    ro.gae = ref.gae(ro.rewards, ro.values, ro.dones, ro.last_value, hp["gamma"], hp["gae_lambda"])
    for a in (ro.gae.adv, ro.gae.returns):
        a.setflags(write=False)
    _cache["ro"] = ro
    return ro


def index_vector(N, m, seed):
    """m rows with a repeat and two entries outside [0, N), which the kernels clamp (tests/test_gpu_trpo.py's)"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N, m).astype(np.int64)
    if m > 2:
        idx[0] = idx[m - 1]
        idx[1], idx[m // 2] = -5, N + 7
    return idx, np.clip(idx, 0, N - 1)


# --------------------------------------------------------------------------------------------------------- sb3_contrib's rule
def select_sb3(table, delta=SB3["kl_delta"]):
    """numpy twin of trpo.select_candidate_sb3: table[0] = (L_0, 0.0) of the zero step; the first candidate k (0-based) that is finite
    with KL_k < delta and L_k > L_0, both strict, or -1"""
    t = np.asarray(table, np.float64)
    for k, (L, KL) in enumerate(t[1:]):
        if np.isfinite(L) and np.isfinite(KL) and KL < delta and L > t[0, 0]:
            return k
    return -1


def sb3_steps(beta):
    """the zero step, then beta 0.8^k, k = 0 .. 9, float32"""
    return np.concatenate([[0.0], beta * SB3["search_decay"] ** -np.arange(SB3["search_candidates"])]).astype(np.float32)


def sb3_margins(table, twin_table, delta=SB3["kl_delta"]):
    """per candidate (rows 1 ..): the distance of L_k from L_0 and of KL_k from delta in float32-twin errors. KL_k: the twin error of
    that very number, floored at u max(|KL_k|, delta) as trpo_reference.threshold_margins does. L_k - L_0: the two numbers come out of
    different workgroups with errors of their own, so the scale is the SUM of their twin errors, floored at u (|L_k| + |L_0|)."""
    t, w = np.asarray(table, np.float64), np.asarray(twin_table, np.float64)
    e = np.abs(w - t)
    sl = np.maximum(e[1:, 0] + e[0, 0], ref.U32 * (np.abs(t[1:, 0]) + abs(t[0, 0])))
    sk = np.maximum(e[1:, 1], ref.U32 * np.maximum(np.abs(t[1:, 1]), delta))
    return np.stack([np.abs(t[1:, 0] - t[0, 0]) / sl, np.abs(t[1:, 1] - delta) / sk], 1)


def search_fixture(ro, P, rows, which):
    """learner_edge_fixtures.search_direction with sb3_contrib's steps. 'kl': along the surrogate's gradient, first candidate at
    KL about 3 delta (KL_k = KL_0 0.64^k re-enters the region at k = 3); 'none': against the gradient from a behaviour policy that IS
    theta (L_0 = 0 up to rounding, every L_k < L_0); 'random': a random direction. Returns (obs, act, old_logp, adv), x, steps [11]"""
    obs, act, old_logp, adv = (x[rows] for x in flat_shard(ro, ro.gae.adv, ro.gae.returns)[:4])
    theta = tr.theta_of(P)
    if which == "none":
        old_logp = logp64(P, obs, act).astype(np.float32)
    if which == "random":
        rng = np.random.default_rng(len(rows))
        x = {k: rng.normal(size=np.shape(v)) for k, v in theta.items()}
    else:
        g = tr.surrogate_gradient(P, obs, act, old_logp, adv)
        x = {k: (-v if which == "none" else v) for k, v in g.items()}
    x = {k: v.astype(np.float32).astype(np.float64) for k, v in x.items()}
    probe = 1e-3 / max(np.abs(v).max() for v in x.values())
    c = tr.kl(P, tr.moved(P, x, probe), obs) / probe ** 2                      # KL(s) ~ c s^2
    beta = np.sqrt({"kl": 3.0, "none": 0.5, "random": 1.2}[which] * SB3["kl_delta"] / c)
    return (obs, act, old_logp, adv), x, sb3_steps(beta)


def search_case(m, which):
    """one search fixture with its float64 table, the float32 twin's and the margins: computed once per (m, which), shared by the CPU
    test that asserts the margins and the GPU test that runs the kernel"""
    key = ("search", m, which)
    if key not in _cache:
        from policy_reference import state_dict_arrays
        ro = rollout()
        P = state_dict_arrays(policy())
        idx, rows = index_vector(ro.T * ro.n, m, 200 + m)
        data, x, steps = search_fixture(ro, P, rows, which)
        s64 = steps.astype(np.float64)
        want, twin = tr.search_table(P, x, s64, *data), tr.search_table(P, x, s64, *data, np.float32)
        _cache[key] = types.SimpleNamespace(m=m, which=which, P=P, idx=idx, rows=rows, data=data, x=x, steps=steps, want=want, twin=twin,
                                            margins=sb3_margins(want, twin), k=select_sb3(want))
    return _cache[key]
