"""Plain float64 restatement of tb_trpo_returns (include/tb_stepper.h; csrc/tb_trpo.hpp), numpy only, written from its definition:

  row (t, e) of a rollout [T][n] has flat index t n + e; L_e is the last step of env e with done != 0, or -1;
  the row is FINISHED iff t <= L_e (its episode ended inside this rollout, wherever it began);
  on finished rows R[t] = r[t] where done[t], else r[t] + discount R[t + 1], in float64, the product and the sum rounded separately;
  `returns` is R rounded to float32 once, 0.0 on unfinished rows; idx = the finished rows' flat indices, ascending.

The rule is the reference's agent.py: the backward discounting of agent.py:264-268 per episode (`episode_returns` restates that loop
operation for operation), `completed_rewards` holding finished episodes only (agent.py:193-203), rounded to float32 by torch.tensor (agent.py:200).
`patterns` and `strided` build the inputs of tests/test_gpu_trpo_returns.py.
"""
import numpy as np

DISCOUNT = 0.98   # agent.py:17


def returns_reference(rewards, dones, discount=DISCOUNT):
    """(R float64 [T, n] -- 0 on unfinished rows --, mask bool [T, n], idx int64 [count]) from the definition"""
    rewards, dones = np.asarray(rewards), np.asarray(dones) != 0
    T, n = rewards.shape
    R, mask = np.zeros((T, n), np.float64), np.zeros((T, n), bool)
    discount = float(discount)
    for e in range(n):
        ends = np.flatnonzero(dones[:, e])
        last = int(ends[-1]) if len(ends) else -1
        nxt = 0.0
        for t in range(last, -1, -1):
            r = float(rewards[t, e])
            nxt = r if dones[t, e] else r + discount * nxt     # two float64 roundings: the product, then the sum
            R[t, e], mask[t, e] = nxt, True
    return R, mask, np.flatnonzero(mask.reshape(-1)).astype(np.int64)


def episode_returns(episode_reward, discount=DISCOUNT):
    """the arithmetic of agent.py:264-268, operation for operation: a copy of one finished episode's rewards (Python floats), walked
    from the last-but-one entry down, each entry += discount * the entry behind it, in place"""
    out = [float(r) for r in episode_reward]
    k = len(out) - 2
    while k >= 0:
        out[k] += discount * out[k + 1]
        k -= 1
    return out


def agent_py_returns(rewards, dones, discount=DISCOUNT):
    """agent.py's train loop (agent.py:253-279) run over every env of a rollout [T][n] on its own: rewards are appended step by step,
    an episode's returns are computed when it ends, an unfinished tail yields nothing. {flat index: return} of the finished rows."""
    rewards, dones = np.asarray(rewards), np.asarray(dones) != 0
    T, n = rewards.shape
    out = {}
    for e in range(n):
        episode, steps = [], []
        for t in range(T):
            episode.append(float(rewards[t, e]))
            steps.append(t)
            if dones[t, e]:
                for s, R in zip(steps, episode_returns(episode, discount)):
                    out[s * n + e] = R
                episode, steps = [], []
    return out


PATTERNS = ("none", "last-step", "step-0", "one-env-every-step", "bernoulli")


def patterns(T, n, which, seed=0):
    """the done patterns of the GPU test: uint8 [T, n]"""
    d = np.zeros((T, n), np.uint8)
    if which == "last-step":
        d[T - 1] = 1
    elif which == "step-0":
        d[0] = 1
    elif which == "one-env-every-step":
        d[:, n // 2] = 1
    elif which == "bernoulli":
        d[:] = np.random.default_rng(seed).random((T, n)) < 0.05
    else:
        assert which == "none", which
    return d


def rollout_rewards(T, n, seed=0):
    """float32 rewards of mixed sign and size, none of them a short binary fraction: every product and every sum rounds"""
    rng = np.random.default_rng(1000 + seed)
    return (rng.normal(0.0, 1.0, (T, n)) * np.exp(rng.normal(0.0, 2.0, (T, n)))).astype(np.float32)


def strided(a, pad, fill):
    """a [T, n] as a view into a wider [T, n + pad] array filled with `fill`: (view, step stride in bytes)"""
    T, n = a.shape
    wide = np.full((T, n + pad), fill, a.dtype)
    wide[:, :n] = a
    return wide, wide.strides[0]
