"""Shared by the population tests: member blobs as tests/test_gpu_policy_members.py builds them (its helpers, copied: a module per
member, packed one by one with pack_policy), env makers, and seeded valid rollout rows for the learner kernels."""
import os

import numpy as np

from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, NET_DEFAULT, NET_MLP64, NET_TUNED, OBS_DIM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NOISE_SEED = 0x5EED1234ABCD
ENV_SEED, ID_BASE = 21, 1 << 33   # (env ids beyond 32 bits: the noise key's high word is in use)
PERTURBATION = 0.1
# The tuned net's seed is chosen, not arbitrary (tests/test_gpu_policy_members.py explains): under most N(0, 0.1^2) perturbations its
# 2-wide ReLU feature is dead for every observation and two members cannot be told apart; with 96 both members move the racket.
PERTURBATION_SEED = {(ENV_SWING, NET_DEFAULT): 77, (ENV_SWING, NET_MLP64): 79, (ENV_TENNIS, NET_DEFAULT): 87, (ENV_TENNIS, NET_TUNED): 96}
M_MAX = 4
PAIRS = [(ENV_SWING, NET_DEFAULT), (ENV_SWING, NET_MLP64), (ENV_TENNIS, NET_DEFAULT), (ENV_TENNIS, NET_TUNED)]
NET_WORD = {NET_DEFAULT: "default", NET_MLP64: "mlp64", NET_TUNED: "tuned"}

_BLOBS, _POLICIES = {}, {}


def base_policy(torch, kind, net):
    """tests/test_gpu_policy_evaluate.py's weights: SwingRacket -- the reference's shipped policy (NET_MLP64: the [64, 64] student fitted
    to it); Tennisbot -- seeded random weights with an action head that moves the racket and unequal log_std"""
    from tennisbot_rl_amd.policy_es import build_policy
    policy = build_policy(kind, net, seed=1234)
    if kind == ENV_SWING and net == NET_DEFAULT:
        policy.load_sb3_arrays(dict(np.load(os.path.join(GOLDEN, "ppo_swing_policy.npz"))))
    elif kind == ENV_SWING:
        policy.load_state_dict({k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "mlp64_swing_student.npz")).items()})
    else:
        with torch.no_grad():
            policy.action_net.weight.mul_(30.0)
            policy.log_std.copy_(torch.linspace(-1.0, 0.2, ACT_DIM[kind]))
    return policy


def member_policies(torch, kind, net):
    """M_MAX CPU modules, built once per (kind, net): member m is the base actor plus a seeded N(0, 0.1^2) perturbation, with a
    log_std row of its own"""
    from tennisbot_rl_amd.policy_es import actor_flat, set_actor_flat
    key = (kind, net)
    if key not in _POLICIES:
        g = torch.Generator().manual_seed(PERTURBATION_SEED[key])
        out = []
        for m in range(M_MAX):
            policy = base_policy(torch, kind, net)
            base = actor_flat(policy)
            set_actor_flat(policy, base + PERTURBATION * torch.randn(base.numel(), generator=g))
            with torch.no_grad():
                policy.log_std.add_(0.15 * m * torch.linspace(-1.0, 1.0, ACT_DIM[kind]))
            out.append(policy)
        _POLICIES[key] = out
    return _POLICIES[key]


def member_blobs(torch, kind, net):
    """[M_MAX, B] on the GPU: each row is pack_policy of that member's module"""
    import copy
    from tennisbot_rl_amd.ppo import pack_policy
    key = (kind, net)
    if key not in _BLOBS:
        _BLOBS[key] = torch.stack([pack_policy(copy.deepcopy(p).to("cuda:0")) for p in member_policies(torch, kind, net)])
    return _BLOBS[key]


def case_params(extended=False):
    from tennisbot_rl_amd.params import F_DEFAULT, F_RACKET_GROUND, default_params, reference_rolling_friction
    if extended:  # the reference's full contact set: racket<->court contact + the rolling-friction rows
        return default_params(flags=F_DEFAULT | F_RACKET_GROUND, **reference_rolling_friction())
    return default_params()


def make_env(kind, n, params, pipeline=None, base=ID_BASE, policy_slices=0):
    from tennisbot_rl_amd.stepper import BatchedEnv
    return BatchedEnv(kind, n, device="cuda:0", seed=ENV_SEED, env_id_base=base, params=params, pipeline=kind == ENV_SWING if pipeline is None else pipeline,
                      track_terminal_obs=False, options={"policy_slices": policy_slices} if policy_slices else None)


def padded(torch, w, extra):
    """the rows `extra` floats further apart, NaN in between: floats the kernel must never read"""
    out = torch.full((w.shape[0], w.shape[1] + extra), float("nan"), dtype=torch.float32, device=w.device)
    out[:, :w.shape[1]] = w
    return out


def golden_observations(kind, n):
    """n observation rows [n, O] float32 from the golden trajectories"""
    z = np.load(os.path.join(GOLDEN, "swing_trajectories.npz" if kind == ENV_SWING else "tennis_trajectories.npz"))
    obs = np.asarray(z["obs"], dtype=np.float32).reshape(-1, OBS_DIM[kind])
    obs = obs[np.all(np.isfinite(obs), axis=1)]
    step = max(1, len(obs) // n)
    return np.ascontiguousarray(obs[::step][:n])


def learner_rows(kind, n, seed=5):
    """seeded valid rows for the learner kernels: observations from the golden trajectories, raw actions, old log-probs,
    advantages and returns of plausible scale. float32 numpy arrays (obs [n, O], act [n, A], old_logp, adv, returns [n])."""
    rng = np.random.default_rng(seed)
    obs = golden_observations(kind, n)
    obs = obs[rng.integers(0, len(obs), n)]
    act = rng.normal(0.0, 0.7, (n, ACT_DIM[kind])).astype(np.float32)
    old_logp = (-0.5 * (act.astype(np.float64) ** 2).sum(1) - 0.9189385332046727 * ACT_DIM[kind] + rng.normal(0.0, 0.1, n)).astype(np.float32)
    adv = rng.normal(0.0, 1.5, n).astype(np.float32)
    returns = rng.normal(0.5, 1.0, n).astype(np.float32)
    return obs, act, old_logp, adv, returns
