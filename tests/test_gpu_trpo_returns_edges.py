"""tb_trpo_returns and the finished-rows update where tests/test_gpu_trpo_returns.py does not reach.

  * the scan past one pass of 1024 table entries: 1025 and 2048 entries of one env, 1056 entries with a ragged last chunk of 16 envs,
    1105 with a last chunk of one env, and the training shape's 6656 -- the running carry, the barrier between two passes;
  * the rounding contract: two-step episodes on which r + fl(discount R') and fl(r + discount R') give other float32 bits on
    EVERY env (trpo_returns_reference.tie_fixture), five discounts;
  * the values: the float32 store's overflow, a float64 carry that leaves float32's range and comes back, subnormal inputs and
    results, zeros of both signs, NaN / +-inf rewards held inside their episode, done bytes 2, 0x80, 0xFF, discount 0.0 and 1.0;
  * the finished-rows update on 2 .. 20 rows (tb_trpo_fvp on m = 1 row, tb_ppo_grad / tb_trpo_search on 2, 3, ... rows) and on
    returns that are all equal.

Which fixture rejects which wrong kernel is asserted on the CPU, on the mutants of tests/trpo_returns_reference.py:
no_carry: a shape past 1024 entries; fused: tie_fixture; float32_carry: overflow_and_back; first_done: bernoulli; done_is_one:
done_bytes; flush_subnormal: subnormal; unfinished_keep: last-step minus one env.
Tolerances: bits for the kernel; ppo_reference.MULTIPLE float32-twin errors for the learner's tensors, as everywhere. Nothing new.
Measured on an MI355X: every test passed as written, no kernel was changed. Largest ratios on 2 .. 20 finished rows: g 1.78, F v 5.24
(17 rows, m = 1), search 2.35 twin errors; update_finished on two rows rejected all ten candidates (every L_k < 0), theta unmoved.
Two scratch builds of the library, not kept: the scan without its carry fails every case of test_scan_takes_more_than_one_pass and
test_trainer_past_one_scan_pass, fma(discount, R', r) in the recurrence fails all five cases of
test_rounding_is_two_float64_roundings_and_one_float32; both pass all of tests/test_gpu_trpo_returns.py.
"""
import numpy as np
import pytest

import learner_edge_fixtures as lf
import ppo_reference as ref
import trpo_reference as tr
import trpo_returns_reference as rr
from policy_reference import state_dict_arrays
from test_gpu_trpo_returns import SENTINEL_B, SENTINEL_F, SENTINEL_I, bits, dev, h, make_trpo, run_returns, snapshot
from test_ppo_reference import rollout

pytestmark = pytest.mark.gpu

MULTIPLE = ref.MULTIPLE
DEV = "cuda:0"
SCAN_SHAPES = [(1025, 1), (2048, 1), (33, 2000), (17, 4097)]   # 1025, 2048, 33 x 32 = 1056 and 17 x 65 = 1105 table entries
WORKLOAD = (104, 4096)                                           # 6656 entries: six passes and a half
SMALL_COUNTS = (2, 3, 16, 17, 19, 20)
RATIOS = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def lib(torch):
    from tennisbot_rl_amd.stepper import load_library
    return load_library()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print("trpo returns edges (gpu): largest %s = %.3g" % (k, RATIOS[k]))


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def definition(rewards, dones, discount=rr.DISCOUNT):
    """(returns float32 [T, n], idx) of the float64 reference"""
    with np.errstate(all="ignore"):
        R, mask, idx = rr.returns_reference(rewards, dones, discount)
        return np.where(mask, R, 0.0).astype(np.float32), idx


def check_kernel(torch, lib, rewards, dones, discount, want, what, layouts=("contiguous", "strided")):
    """the assertions of test_returns_mask_and_index_list on one input: the returns' bits (NaN where the reference is NaN), idx, the
    exact count, the sentinels behind every output, the same bytes from a second run"""
    T, n = rewards.shape
    N = T * n
    want_ret, want_idx = want
    nan = np.isnan(want_ret).reshape(-1)
    for layout in layouts:
        if layout == "contiguous":
            r_d, d_d, rs, ds = dev(torch, rewards), dev(torch, dones), 0, 0
        else:  # record strides larger than n; what lies between the records must not be read as data
            rw, rs = rr.strided(rewards, 5, np.float32("nan"))
            dw, ds = rr.strided(dones, 3, np.uint8(1))
            r_d, d_d = dev(torch, rw), dev(torch, dw)
        first = run_returns(torch, lib, r_d, d_d, rs, ds, T, n, discount)
        ret, idx, count, tail = first
        tag = "%s %s" % (what, layout)
        assert count[1] == len(want_idx), "%s: count %d, want %d" % (tag, count[1], len(want_idx))
        assert count[0] == SENTINEL_I and count[2] == SENTINEL_I, tag + ": count's neighbours were written"
        assert np.array_equal(np.isnan(ret[:N]), nan), tag + ": NaN where the reference has none, or none where it has one"
        assert np.array_equal(bits(ret[:N])[~nan], bits(want_ret.reshape(-1))[~nan]), tag + ": returns differ from the float64 reference rounded to float32"
        assert np.array_equal(idx[:len(want_idx)], want_idx), tag + ": idx"
        assert (idx[len(want_idx):] == SENTINEL_I).all(), tag + ": idx was written past count"
        assert (ret[N:] == SENTINEL_F).all() and (tail == SENTINEL_B).all(), tag + ": an output or the workspace was written past its end"
        second = run_returns(torch, lib, r_d, d_d, rs, ds, T, n, discount)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(first, second)), tag + ": a second run gave other bits"


# -------------------------------------------------------------------------------------------------------------------- the scan
@pytest.mark.parametrize("T,n", SCAN_SHAPES + [WORKLOAD])
def test_scan_takes_more_than_one_pass(torch, lib, T, n):
    assert T * ((n + 63) // 64) > rr.SCAN_PASS
    for p, which in enumerate(rr.PATTERNS):
        if (T, n) == WORKLOAD and which not in ("bernoulli", "last-step"):
            continue
        rewards, dones = rr.rollout_rewards(T, n, seed=p), rr.patterns(T, n, which, seed=7 + p)
        want = definition(rewards, dones)
        if which == "last-step":
            assert np.array_equal(want[1], np.arange(T * n))
        if which == "bernoulli" and (T, n) != (1025, 1):      # (one env, one entry behind the pass: "last-step" has a row there)
            entry = want[1] // n * ((n + 63) // 64) + want[1] % n // 64
            assert (entry < rr.SCAN_PASS).any() and (entry >= rr.SCAN_PASS).any(), "no finished row behind the first pass"
        check_kernel(torch, lib, rewards, dones, rr.DISCOUNT, want, "(%d, %d) %s" % (T, n, which), ("contiguous",) if (T, n) == WORKLOAD else ("contiguous", "strided"))


# ---------------------------------------------------------------------------------------------------------------- the rounding
@pytest.mark.parametrize("i", range(rr.tie_discounts()))
def test_rounding_is_two_float64_roundings_and_one_float32(torch, lib, i):
    rewards, dones, discount = rr.tie_fixture(i)
    want = definition(rewards, dones, discount)
    assert rewards.shape[1] >= 65 and len(want[1]) == rewards.size
    # (that the fused form's bits are others on every env of row 0: tests/test_trpo_returns_reference.py)
    check_kernel(torch, lib, rewards, dones, discount, want, "tie fixture %d (discount %r)" % (i, discount))


# ------------------------------------------------------------------------------------------------------------------ the values
@pytest.mark.parametrize("name", rr.VALUE_FIXTURES)
def test_value_edges(torch, lib, name):
    rewards, dones, discount = rr.value_fixtures()[name]
    want = definition(rewards, dones, discount)
    assert np.isnan(want[0]).any() == (name in ("nonfinite", "discount_0")) and 0 < len(want[1]) < rewards.size
    check_kernel(torch, lib, rewards, dones, discount, want, name)


# ---------------------------------------------------------------------------------------------------- a handful of finished rows
def small_rollout(count):
    """T = 8, n = 65 of rollout("tennis-70-ragged"), done bytes placed for `count` finished rows; count = 2: both in the ragged last chunk"""
    ro = rollout("tennis-70-ragged")
    T, n = 8, 65
    dones = np.zeros((T, n), np.uint8)
    rows = 0
    for e, t in ((64, 1), (64, 2), (64, 7), (3, 7), (10, 0), (20, 1), (30, 0)):   # (env, its done step): rows 2, 3, 8, 16, 17, 19, 20
        if rows < count:
            dones[:, e] = 0
            dones[t, e] = 1
            rows = int(sum(np.flatnonzero(dones[:, k])[-1] + 1 for k in range(n) if dones[:, k].any()))
    assert rows == count, (rows, count)
    c = lambda a: np.ascontiguousarray(a[:T, :n]).reshape((T * n,) + a.shape[2:])  # noqa: E731
    return ro, T, n, np.ascontiguousarray(ro.rewards[:T, :n]), dones, c(ro.obs), c(ro.raw), c(ro.old_logp)


def test_small_finished_counts(torch):
    from tennisbot_rl_amd.trpo import select_candidate
    ro = rollout("tennis-70-ragged")
    L = make_trpo(torch, ro)
    P = state_dict_arrays(L.policy)
    assert L.hp["cg_damping"] == tr.CG_DAMPING and L.hp["cg_state_percent"] == tr.CG_STATE_PERCENT and L.hp["kl_delta"] == tr.KL_DELTA
    d32 = float(np.float32(tr.CG_DAMPING))
    vec, v = lf.fvp_vector(P)
    vec_d = dev(torch, vec)
    theta = h(L.mask) != 0
    ms = []
    for count in SMALL_COUNTS:
        ro, T, n, rewards, dones, obs, act, old_logp = small_rollout(count)
        N = T * n
        ret, idx, cnt = L.returns_to_go(dev(torch, rewards), dev(torch, dones))
        R, mask, rows = rr.returns_reference(rewards, dones)
        assert int(cnt.item()) == count == len(rows) and np.array_equal(h(idx)[:count], rows)
        assert np.array_equal(bits(h(ret)), bits(np.where(mask, R, 0.0)))
        if count == 2:
            assert (rows % n == 64).all()
        adv64 = R.reshape(-1)[rows]
        adv32 = adv64.astype(np.float32)
        assert adv64.std() > 0.0
        arrays = (dev(torch, obs), dev(torch, act), dev(torch, old_logp), ret.reshape(N), ret.reshape(N))
        # g on the finished rows, the raw returns as `adv`
        got = h(L.surrogate_gradient(arrays, N, idx.data_ptr(), count))
        assert np.isfinite(got).all() and not got[~theta].any() and got[theta].any()
        want = tr.surrogate_gradient(P, obs[rows], act[rows], old_logp[rows], adv64)
        twin = tr.surrogate_gradient(P, obs[rows], act[rows], old_logp[rows], adv32, np.float32)
        r_g = note("g error / twin error", ref.check_tensors("%d rows: surrogate gradient" % count, tr.theta_of(tr.split_flat(got, P)), want, twin, MULTIPLE))
        # F v on m rows of the shuffled list, as update_finished draws them
        m = max(1, int(tr.CG_STATE_PERCENT * count))
        ms.append(m)
        cg_rows = rows[np.random.default_rng(count).permutation(count)]
        cg_d = dev(torch, cg_rows)
        out = [torch.full((L.n_params,), 7.0, device=DEV) for _ in range(2)]
        L.fvp(arrays[0], cg_d.data_ptr(), m, vec_d, out[0])
        L.fvp(arrays[0], cg_d.data_ptr(), m, vec_d, out[1])
        assert torch.equal(out[0], out[1]), "%d rows, m = %d: a second run gave other bits" % (count, m)
        got = h(out[0])
        assert np.isfinite(got).all() and not got[~theta].any()
        want, twin = tr.fvp(P, obs[cg_rows[:m]], v, d32), tr.fvp(P, obs[cg_rows[:m]], v, d32, np.float32)
        r_f = note("FVP error / twin error", ref.check_tensors("%d rows: fvp on m = %d" % (count, m), tr.theta_of(tr.split_flat(got, P)), want, twin, MULTIPLE))
        # the line search's table on the finished rows
        data = (obs[rows], act[rows], old_logp[rows])
        _, x, steps = lf.search_direction(P, data + (adv64,), "kl")
        got_t = L.search(arrays, N, idx.data_ptr(), count, dev(torch, tr.join_flat(x, P, np.float32)), dev(torch, steps))
        got = h(got_t)
        s64 = steps.astype(np.float64)
        want, twin = tr.search_table(P, x, s64, *data, adv64), tr.search_table(P, x, s64, *data, adv32, np.float32)
        r_s = note("search error / twin error", ref.check_tensors("%d rows: search" % count, lf.columns(got), lf.columns(want), lf.columns(twin), MULTIPLE))
        margins = tr.threshold_margins(want, twin)
        k_dev = int(select_candidate(torch, got_t, tr.KL_DELTA))
        if margins.min() > 100.0:       # (the margin of tests/test_gpu_trpo.py: the fixture decides the selection)
            assert k_dev == tr.select(want) == tr.select(got), (count, got, want)
        print("%2d finished rows, m = %d: g %.3g, FVP %.3g, search %.3g twin errors; accepted %d (smallest margin %.3g)" % (count, m, r_g, r_f, r_s, k_dev, margins.min()))
    assert ms == [1, 1, 1, 1, 1, 2]
    # one whole update on two rows: theta moves by the accepted candidate, bit for bit, or not at all; nothing else moves
    ro, T, n, rewards, dones, obs, act, old_logp = small_rollout(2)
    ret, idx, cnt = L.returns_to_go(dev(torch, rewards), dev(torch, dones))
    before = [h(x) for x in (L.flat, L.grad, L.exp_avg, L.exp_avg_sq)]
    flat0_t = L.flat.clone()
    stats = L.update_finished(dev(torch, obs), dev(torch, act), dev(torch, old_logp), ret.reshape(T * n), idx, cnt)
    after = [h(x) for x in (L.flat, L.grad, L.exp_avg, L.exp_avg_sq)]
    k = stats["accepted_k"]
    assert stats["finished_rows"] == 2 and stats["finished_share"] == 2 / (T * n) and -1 <= k < tr.CANDIDATES, stats
    assert np.isfinite(after[0]).all()
    if k >= 0:
        assert torch.equal(L.flat, flat0_t + L.steps[k] * L.direction) and not np.array_equal(after[0][theta], before[0][theta])
    else:
        assert np.array_equal(bits(after[0]), bits(before[0]))
    assert np.array_equal(bits(after[0][~theta]), bits(before[0][~theta]))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before[1:], after[1:])), "the gradient buffer or a moment was written"
    print("update_finished on 2 rows: %s\n%s" % (stats, h(L.table)))


# ------------------------------------------------------------------------------------------------------------- equal returns
@pytest.mark.parametrize("reward", [0.0, 0.25])
def test_equal_returns_reject_the_step(torch, reward):
    """every finished row's return the same: std = 0, A_hat = 0, g = 0, conjugate gradient's 0 / 0. Reward 0: SwingRacket's own episodes
    (a ball that drops straight down); reward 0.25: with a done at every step, so that R = r on every row"""
    from tennisbot_rl_amd.trpo import TRPOTrainer
    t = TRPOTrainer("SwingRacket-v0", num_envs=64, n_steps=26, device=DEV, seed=4, form="agent_returns")
    n = 64 * 26
    t.collect()
    t.buf.rewards.fill_(reward)
    if reward:
        t.buf.dones.fill_(1)
    ret, _ = t.advantages(None)
    torch.cuda.synchronize()
    assert (h(ret) == np.float32(reward)).all() and h(t.buf.dones)[-1].all()
    before = snapshot(t)
    stats = t.update(ret, ret)
    assert stats["accepted_k"] == -1 and stats["finished_rows"] == n, stats
    after = snapshot(t)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, after)), "a rejected step wrote something"
    assert all(np.isfinite(h(p)).all() for p in t.policy.parameters())
    # whatever NaN the rejected step left in the learner's vectors and its table: the next update does not see it
    ret, _ = t.advantages(t.collect())
    stats = t.update(ret, ret)
    assert 0 <= stats["accepted_k"] < tr.CANDIDATES and stats["finished_rows"] == n, (stats, h(t._learner.table))
    assert all(np.isfinite(v) for k, v in stats.items() if k != "value_loss"), stats
    assert np.isfinite(snapshot(t)[0]).all() and not np.array_equal(snapshot(t)[0], before[0])
    t.env.close()


# ------------------------------------------------------------------------------------------- a trainer past one pass of the scan
def test_trainer_past_one_scan_pass(torch):
    from tennisbot_rl_amd.trpo import TRPOTrainer
    num_envs, n_steps = 1100, 78                  # 18 chunks x 78 steps = 1404 table entries, a last chunk of 12 envs
    t = TRPOTrainer("SwingRacket-v0", num_envs=num_envs, n_steps=n_steps, device=DEV, seed=4, form="agent_returns")
    n = num_envs * n_steps
    ret, _ = t.advantages(t.collect())
    torch.cuda.synchronize()
    want, want_idx = definition(h(t.buf.rewards), h(t.buf.dones))
    assert np.array_equal(bits(h(ret)), bits(want)), "advantages() is not the reference on the trainer's own buffers"
    _, idx, count = t._finished
    assert int(count.item()) == n == 85800 and np.array_equal(h(idx), np.arange(n)) and np.array_equal(want_idx, np.arange(n))
    before = snapshot(t)[0]
    stats = t.update(ret, ret)
    assert stats["finished_rows"] == 85800 and stats["finished_share"] == 1.0 and 0 <= stats["accepted_k"] < tr.CANDIDATES, (stats, h(t._learner.table))
    assert np.isfinite(snapshot(t)[0]).all() and not np.array_equal(snapshot(t)[0], before)
    t.env.close()
