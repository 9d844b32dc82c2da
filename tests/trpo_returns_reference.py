"""Plain float64 restatement of tb_trpo_returns (include/tb_stepper.h; csrc/tb_trpo.hpp), numpy only, written from its definition:

  row (t, e) of a rollout [T][n] has flat index t n + e; L_e is the last step of env e with done != 0, or -1;
  the row is FINISHED iff t <= L_e (its episode ended inside this rollout, wherever it began);
  on finished rows R[t] = r[t] where done[t], else r[t] + discount R[t + 1], in float64, the product and the sum rounded separately;
  `returns` is R rounded to float32 once, 0.0 on unfinished rows; idx = the finished rows' flat indices, ascending.

The rule is the reference's agent.py: the backward discounting of agent.py:264-268 per episode (`episode_returns` restates that loop
operation for operation), `completed_rewards` holding finished episodes only (agent.py:193-203), rounded to float32 by torch.tensor (agent.py:200).
`patterns` and `strided` build the inputs of tests/test_gpu_trpo_returns.py.

For tests/test_gpu_trpo_returns_edges.py (numpy and `fractions` only):
  `compact_by_table` restates the three index-list launches: the count table, its scan `pass_entries` at a time, the scatter;
  `kernel_reference` restates the four launches as they run (backwards from the last step, one float32 store per row) and gives
  what the device gives: (returns float32 [T, n], idx, count). tests/test_trpo_returns_reference.py holds it against
  `returns_reference`, the definition. `Mutant(name)` is `kernel_reference` with one line changed: a kernel that is subtly wrong;
  `tie_fixture` and `value_fixtures` are the inputs on which each mutant's bits differ from the reference's.
"""
import functools
from fractions import Fraction

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


# ------------------------------------------------------------------------------------------- the launches, restated; the mutants
MUTANTS = ("no_carry", "fused", "float32_carry", "first_done", "done_is_one", "flush_subnormal", "unfinished_keep")
F32_MAX = float(np.finfo(np.float32).max)
F32_TINY = float(np.finfo(np.float32).tiny)    # 2^-126: below it a float32 is subnormal
SCAN_PASS = 1024                               # table entries per pass of tb_trpo_finished_scan_kernel


def compact_by_table(mask, pass_entries=SCAN_PASS, carry=True):
    """the index list as the count, scan and scatter launches build it. table[t][c] = the set rows of step t in the 64-env chunk c;
    its exclusive scan in row-major order, `pass_entries` at a time, a running carry handing every pass the total of the passes
    before it; row (t, e) goes to idx[offset[t][c] + the set rows of its chunk below e]. carry=True: np.flatnonzero(mask).
    carry=False (a kernel without the carry): every pass starts at 0 again and the count is the last pass's total."""
    mask = np.asarray(mask, bool)
    T, n = mask.shape
    chunks = (n + 63) // 64
    padded = np.zeros((T, chunks * 64), bool)
    padded[:, :n] = mask
    table = padded.reshape(T * chunks, 64).sum(1).astype(np.int64)
    offsets, run, count = np.zeros_like(table), 0, 0
    for base in range(0, len(table), pass_entries):
        own = table[base:base + pass_entries]
        offsets[base:base + pass_entries] = (run if carry else 0) + np.cumsum(own) - own
        run += int(own.sum())
        count = run if carry else int(own.sum())
    idx = np.full(T * n, -1, np.int64)
    for w in np.flatnonzero(table):
        t, c = divmod(int(w), chunks)
        e = c * 64 + np.flatnonzero(padded[t, c * 64:(c + 1) * 64])
        idx[offsets[w] + np.arange(len(e))] = t * n + e
    return idx[:count]


def _store(R, flush=False):
    """the one float32 rounding, at the store"""
    out = np.float32(R)
    if flush and out != 0 and abs(float(out)) < F32_TINY:
        out = np.float32(np.copysign(0.0, float(out)))
    return out


def kernel_reference(rewards, dones, discount=DISCOUNT, mutant=None):
    """(returns float32 [T, n], idx int64 [count], count) as tb_trpo_returns leaves them, restated launch by launch; `mutant`: one of
    MUTANTS, the line it names changed"""
    assert mutant is None or mutant in MUTANTS, mutant
    rewards, dones = np.asarray(rewards), np.asarray(dones)
    done = (dones == 1) if mutant == "done_is_one" else (dones != 0)
    T, n = rewards.shape
    discount = float(discount)
    out, last = np.zeros((T, n), np.float32), np.full(n, -1)
    with np.errstate(all="ignore"):
        for e in range(n):
            R, L = 0.0, -1
            for t in range(T - 1, -1, -1):
                r, d = float(rewards[t, e]), bool(done[t, e])
                if d:
                    R = r
                elif mutant == "fused":
                    R = float(Fraction(discount) * Fraction(R) + Fraction(r))    # the exact product and sum, one float64 rounding
                else:
                    R = r + discount * R                                         # two float64 roundings: the product, then the sum
                if mutant == "float32_carry":
                    R = float(np.float32(R))
                if d and (L < 0 or mutant == "first_done"):
                    L = t
                if L >= 0 or mutant == "unfinished_keep":
                    out[t, e] = _store(R, mutant == "flush_subnormal")
            last[e] = L
    mask = np.arange(T)[:, None] <= last[None, :]
    if mutant == "first_done":
        out[~mask] = 0.0
    idx = compact_by_table(mask, carry=mutant != "no_carry")
    return out, idx, len(idx)


class Mutant:
    """kernel_reference with one line changed (MUTANTS): called as kernel_reference is"""

    def __init__(self, name):
        assert name in MUTANTS, name
        self.name = name

    def __call__(self, rewards, dones, discount=DISCOUNT):
        return kernel_reference(rewards, dones, discount, self.name)


def differs(a, b):
    """two (returns, idx, count) results: is there a bit of difference? (NaN payloads included: the callers compare finite results)"""
    return not (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and a[2] == b[2])


# ---------------------------------------------------------------------------------------------------- where the rounding shows
@functools.lru_cache(maxsize=None)
def _tie_cases():
    """two-step episodes (r0, r1 done) whose float32 result tells r0 + fl(discount r1) from fl(r0 + discount r1). discount r1 is
    1 +- 2^-29 to within a float64 rounding, r0 = 2^24 + 2 k is even with a float64 ulp of 2^-28 and a float32 ulp of 2: the
    separate product rounds to 1 +- 2^-29, the sum is a float64 tie that goes to the even neighbour, and where that is r0 + 1
    exactly the float32 store ties to even again; the fused sum keeps the product's error and falls off both ties.
    [(discount, r1, [r0 ...])], every discount whose differing r0 fill more than a wave."""
    out = []
    for r1 in (5, 7, 11, 13):
        for sign in (1, -1):
            centre = float((1 + sign * Fraction(1, 2 ** 29)) / r1)
            for discount in (float(np.nextafter(centre, 0.0)), centre, float(np.nextafter(centre, 1.0))):
                r0s = []
                for k in range(200):
                    r0 = float(2 ** 24 + 2 * k)
                    separate = np.float32(r0 + discount * r1)
                    fused = np.float32(float(Fraction(discount) * r1 + Fraction(r0)))
                    if separate != fused:
                        r0s.append(r0)
                if len(r0s) >= 65:
                    out.append((discount, float(r1), r0s))
    return out


def tie_discounts():
    return len(_tie_cases())


def tie_fixture(discount_index):
    """(rewards float32 [2, n], dones uint8 [2, n], discount): one env per r0, done at step 1; n >= 65 crosses a wave edge"""
    discount, r1, r0s = _tie_cases()[discount_index]
    rewards = np.array([r0s, [r1] * len(r0s)], np.float32)
    assert np.array_equal(rewards[0].astype(np.float64), r0s)
    dones = np.zeros(rewards.shape, np.uint8)
    dones[1] = 1
    return rewards, dones, discount


# --------------------------------------------------------------------------------------------------------- where the values show
VALUE_T, VALUE_N = 27, 65
FINITE_VALUE_FIXTURES = ("overflow", "overflow_and_back", "subnormal", "signed_zero", "done_bytes", "discount_1")
VALUE_FIXTURES = FINITE_VALUE_FIXTURES + ("nonfinite", "discount_0")


def value_fixtures():
    """{name: (rewards float32 [27, 65], dones uint8 [27, 65], discount)}. Every env has episodes over steps 0 .. 8 and 9 .. 17; an odd
    env has a third over 18 .. 26, an even env an unfinished tail there. The values of each fixture sit in the MIDDLE episode of the
    envs e with e % 3 != 2; the envs with e % 3 == 2 are clean."""
    T, n = VALUE_T, VALUE_N
    e = np.arange(n)
    special, sign = e % 3 != 2, np.where(e % 2 == 0, 1.0, -1.0).astype(np.float32)
    sub = np.float32(2.0 ** -149)                  # the smallest float32 subnormal

    def base(seed):
        dones = np.zeros((T, n), np.uint8)
        dones[8] = dones[17] = 1
        dones[26, 1::2] = 1
        return rollout_rewards(T, n, seed), dones

    out = {}
    big = np.float32(3e38)
    for name, back in (("overflow", False), ("overflow_and_back", True)):
        r, d = base(20 + back)
        r[12, special] = r[13, special] = (big * sign)[special]        # R[12] ~ 5.9e38 and the rows before it: above float32's 3.4e38
        if back:
            r[11, special] = (-big * sign)[special]                    # R[11] ~ 2.8e38: finite in float32 again, from a float64 carry
        out[name] = (r, d, DISCOUNT)
    r, d = base(22)
    k = np.random.default_rng(5).integers(1, 2 ** 20, (9, n)).astype(np.float32)
    r[9:18] = np.where(special, k * sub * sign, r[9:18])
    r[17, special] = (-sub * sign)[special]                            # the done row: R = -+2^-149
    r[16, special] = (sub * sign)[special]                             # R = +-0.02 x 2^-149: below 2^-150, a zero of either sign
    out["subnormal"] = (r, d, DISCOUNT)
    r, d = base(23)
    z = np.float32(-0.0)
    r[17, special], r[16, special], r[15, special], r[14, special] = z, z, 0.0, z   # -0 at the done row, -0 + -0, +0 + -0, -0 + +0
    r[8, special] = z                                                                # ... and a one-row -0 behind an ordinary episode
    r[20:, 0::2] = z                                                                 # -0 rewards on unfinished rows: +0 is stored
    # (a zero of either sign by underflow: the `subnormal` fixture, step 16)
    out["signed_zero"] = (r, d, DISCOUNT)
    r, d = base(24)
    nan, inf = np.float32("nan"), np.float32("inf")
    r[13, e % 6 == 0] = nan
    r[13, e % 6 == 1] = inf
    r[13, e % 6 == 3] = -inf
    r[14, e % 6 == 4], r[13, e % 6 == 4] = inf, -inf                   # inf - inf
    d[26] = 1                                                          # (here every env has a later episode, except env 2:)
    d[26, 2], r[20, 2] = 0, nan                                        # a NaN on an unfinished row, which nothing reads
    out["nonfinite"] = (r, d, DISCOUNT)
    r, d = base(25)
    d[8, e % 3 == 0], d[8, e % 3 == 1], d[8, e % 3 == 2] = 2, 0x80, 0xFF
    d[26, 1::2] = 0xFF
    out["done_bytes"] = (r, d, DISCOUNT)
    r, d = base(26)
    r[13, special] = (inf * sign)[special]                             # 0 x inf = NaN on the rows before it
    out["discount_0"] = (r, d, 0.0)
    out["discount_1"] = base(27) + (1.0,)
    return out
