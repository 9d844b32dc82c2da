"""Tennisbot with the extended contact set (racket<->court manifold + rolling-friction rows) in the kernels that step envs in a loop
with a network in front -- tb_policy_rollout_kernel, tb_policy_evaluate_kernel, tb_sac_evaluate_kernel, tb_sac_collect_kernel --
on a real MI355X. Those kernels keep Tennisbot's three static contact rows in registers also with the extended set compiled in
(policy_rollout_rows_in_registers; SF_RG | SF_REGROWS | SF_COLD), a form tb_step does not have (step_rows_in_registers: LDS with RG)
and that tb_es_evaluate gave up after it stepped a ball-court bounce differently. Everywhere else in the suite they start from
tb_reset with a racket of scale 1 that the ball rarely reaches and that never comes down to the court.

Here they start on forced contact states: helpers.low_racket_batch -- the ball on a randomly oriented, randomly scaled racket, half
of the rackets with hull vertices on or under the court (what that batch reaches is pinned on the oracle alone in
tests/test_tennis_contact_states.py) -- loaded with set_state_words into the handle under test, a twin BatchedEnv and a float32
OracleBatch; and on whole episodes at the shape that exposed the ES difference (208 envs, racket scale 3). Every comparison is
bit for bit.

  a. the yardstick: tb_step (its RG instantiation) against the oracle on the low rackets, every output and the whole state after
     every step, and the state again four steps later (the handle has no reader for its contact cache: a cache that differed
     shows in the steps that warm-start from it);
  b. tb_policy_rollout_net, one launch of 12 steps: default and tuned network, policy_slices 1 and 3 (3 is the non-wide form with
     RG), 2047 envs too (dummy lanes in the last workgroup) -- its reported actions replayed through tb_step and the oracle;
  c. tb_sac_collect, one launch of 12 steps, actor and uniform mode, replayed the same way;
  d. whole episodes at scale 3: policy_evaluate, sac_evaluate, policy_rollout (1001 steps, policy_slices 3), sac_collect (1001);
  e. in b and c the handle's counters are the oracle's, and its final state differs from a twin without F_RACKET_GROUND and from one
     without the rolling rows in at least as many envs as test_tennis_contact_states.py asserts for the oracle: the rows ran."""
import time

import numpy as np
import pytest

import test_gpu_policy_evaluate as pe
import test_gpu_sac_collect as sc
import test_gpu_sac_evaluate as ev
from helpers import LOW_RACKET_STEPS, low_racket_batch, low_racket_params, same_bits
from oracle import OracleBatch
from test_gpu_parity import compare_state, same
from test_tennis_contact_states import AT_LEAST
from tennisbot_rl_amd.params import COUNTER_NAMES, ENV_TENNIS, F_AUTO_RESET, F_RACKET_GROUND, NET_DEFAULT, NET_TUNED

pytestmark = pytest.mark.gpu

DEV, NOISE_SEED, ENV_SEED, ID_BASE = ev.DEV, ev.NOISE_SEED, ev.ENV_SEED, ev.ID_BASE
T = LOW_RACKET_STEPS
N_EPISODES = 208            # 13 slices of 16 envs: the size at which tb_es_evaluate's register form left tb_step
SCALE = 3.0


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def make_env(n, params, slices=0):
    from tennisbot_rl_amd.stepper import BatchedEnv
    return BatchedEnv(ENV_TENNIS, n, device=DEV, seed=ENV_SEED, env_id_base=ID_BASE, params=params, options=dict(policy_slices=slices))


def make_oracle(n, params, threads=8):
    pf = params.copy()
    pf.flags |= F_AUTO_RESET
    return OracleBatch(pf, ENV_TENNIS, n, seed=ENV_SEED, env_id_base=ID_BASE, precision="f32", threads=threads)


def without(params, what):
    p = params.copy()
    if what == "rg":
        p.flags &= ~F_RACKET_GROUND
    else:
        p.roll_racket = p.roll_court = p.roll_goal = 0.0
    return p


def load(env, words, done):
    if isinstance(env, OracleBatch):
        env.set_state_words(words, done)
    else:
        env.set_state_words(words.view(np.int32), done)


def replay(torch, twin, ref, actions, what):
    """actions [S, n, 2] (numpy) through twin.step and the oracle from where both stand: obs, reward, done, substeps and the whole
    state equal after every step. Returns the steps' (obs, reward, done) as numpy [S, ...]."""
    obs, rew, done = [], [], []
    a_dev = torch.from_numpy(np.ascontiguousarray(actions)).to(DEV)
    for t in range(len(actions)):
        o, r, d = twin.step(a_dev[t].clone())   # (a row of its own: step() wants 16-byte aligned rows)
        o2, r2, d2, s2 = ref.step(actions[t])
        tag = "%s, tb_step against the oracle, step %d" % (what, t)
        same(d.cpu().numpy(), d2, tag + " done")
        same(twin.last_substeps().cpu().numpy(), s2, tag + " substeps")
        same(o.cpu().numpy(), o2, tag + " obs")
        same(r.cpu().numpy(), r2, tag + " reward")
        compare_state(twin, ref, tag)
        obs.append(o2); rew.append(r2); done.append(d2)
    return np.stack(obs), np.stack(rew), np.stack(done)


def counters_of(ref):
    return dict(zip(COUNTER_NAMES, [int(x) for x in ref.counters()]))


def envs_that_differ(torch, env, params, what, words, done, actions):
    """how many envs' final state words differ between env and a twin without `what` ("rg": F_RACKET_GROUND, "roll": the rolling
    rows) stepped from the same words with the same actions"""
    plain = make_env(words.shape[1], without(params, what))
    load(plain, words, done)
    a_dev = torch.from_numpy(np.ascontiguousarray(actions)).to(DEV)
    for t in range(len(actions)):
        plain.step(a_dev[t].clone())
    differ = int((env.get_state_words()[0] != plain.get_state_words()[0]).any(0).sum())
    plain.close()
    return differ


def check_loop_kernel_on_low_rackets(torch, env, words, done, params, actions, obs, rew, dn, what):
    """b / c / e: the loop kernel's steps (actions it reports, next observations, rewards, done flags [T, n, ...] on the host) and
    the state and counters it left in env, against tb_step on a twin and the oracle driven with those actions"""
    n = env.num_envs
    twin, ref = make_env(n, params), make_oracle(n, params)
    load(twin, words, done); load(ref, words, done)
    o2, r2, d2 = replay(torch, twin, ref, actions, what)
    for t in range(len(actions)):
        same(obs[t], o2[t], "%s step %d obs" % (what, t))
        same(rew[t], r2[t], "%s step %d reward" % (what, t))
        same(dn[t] != 0, d2[t] != 0, "%s step %d done" % (what, t))
    compare_state(env, ref, what + " final state")
    wa, da = env.get_state_words(); wb, db = twin.get_state_words()
    assert torch.equal(wa, wb) and torch.equal(da, db), what + ": the handle is not where tb_step left the twin"
    got, want = env.counters(), counters_of(ref)
    assert got == want and twin.counters() == want, (what, got, want, twin.counters())   # all nine
    assert got["nonfinite_states"] == 0 and got["lockstep_violations"] == 0 and got["substeps"] == len(actions) * n
    assert got["racket_ball_contact_substeps"] > 0 and got["episodes_finished"] > 0
    twin.close(); ref.close()
    # e. the racket<->court rows and the rolling rows ran on the device
    no_rg = envs_that_differ(torch, env, params, "rg", words, done, actions)
    no_roll = envs_that_differ(torch, env, params, "roll", words, done, actions)
    print("%s: counters %s; final state differs from a twin without F_RACKET_GROUND in %d envs, without the rolling rows in %d" % (what, got, no_rg, no_roll))
    assert no_rg >= AT_LEAST["differ_without_rg"] and no_roll >= AT_LEAST["differ_without_rolling"], (no_rg, no_roll)


# ------------------------------------------------------------------------------------------------------------------- a.
def test_tb_step_on_low_rackets_matches_the_oracle(torch):
    t0 = time.perf_counter()
    n, params = 2048, low_racket_params()
    words, done, actions = low_racket_batch(n)
    twin, ref = make_env(n, params), make_oracle(n, params)
    load(twin, words, done); load(ref, words, done)
    same(twin.observe().cpu().numpy(), words[[0, 1, 2, 7, 8, 9, 13, 14, 15, 16, 17, 18]].view(np.float32).T, "observe() of the loaded words")
    replay(torch, twin, ref, actions, "low rackets")
    # the handle has no reader for its contact cache: four further steps warm-start from it
    more = np.random.default_rng(2).uniform(-1, 1, (4, n, 2)).astype(np.float32)
    replay(torch, twin, ref, more, "low rackets, four steps on")
    got, want = twin.counters(), counters_of(ref)
    assert got == want, (got, want)
    assert got["racket_ball_contact_substeps"] >= AT_LEAST["racket_ball_contact_substeps"] and got["episodes_finished"] >= AT_LEAST["episodes_restarted"]
    no_rg = envs_that_differ(torch, twin, params, "rg", words, done, np.concatenate([actions, more]))
    no_roll = envs_that_differ(torch, twin, params, "roll", words, done, np.concatenate([actions, more]))
    twin.close(); ref.close()
    print("tb_step on low rackets: counters %s; differs without F_RACKET_GROUND in %d envs, without rolling rows in %d; %.2f s"
          % (got, no_rg, no_roll, time.perf_counter() - t0))
    assert no_rg > 0 and no_roll > 0


# ------------------------------------------------------------------------------------------------------------------- b.
@pytest.mark.parametrize("net,slices,n", [(NET_DEFAULT, 1, 2048), (NET_DEFAULT, 3, 2047), (NET_TUNED, 1, 2047), (NET_TUNED, 3, 2048)])
def test_policy_rollout_on_low_rackets(torch, net, slices, n):
    t0 = time.perf_counter()
    params = low_racket_params()
    words, done, _ = low_racket_batch(n)
    w = pe.blob(torch, ENV_TENNIS, net)
    env = make_env(n, params, slices)
    load(env, words, done)
    (obs, rew, dn), (act, raw, logp, value) = env.policy_rollout(w, env.observe(), T, seed=NOISE_SEED, net=net)
    torch.cuda.synchronize()
    assert torch.equal(act, raw.clamp(-1.0, 1.0)) and bool(torch.isfinite(logp).all()) and bool(torch.isfinite(value).all())
    what = "policy_rollout net=%d slices=%d n=%d" % (net, slices, n)
    check_loop_kernel_on_low_rackets(torch, env, words, done, params, act.cpu().numpy(), obs.cpu().numpy(), rew.cpu().numpy(), dn.cpu().numpy(), what)
    env.close()
    print("%s: %.2f s" % (what, time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------------------------- c.
@pytest.mark.parametrize("uniform,n", [(False, 2048), (True, 2047)])
def test_sac_collect_on_low_rackets(torch, uniform, n):
    t0 = time.perf_counter()
    params = low_racket_params()
    words, done, _ = low_racket_batch(n)
    act = ev.actor(torch, ENV_TENNIS, "plain")
    env = make_env(n, params)
    load(env, words, done)
    obs0 = env.observe().cpu().numpy()
    rec = sc.collect(torch, env, act.flat, (T,), uniform=uniform)
    what = "sac_collect %s n=%d" % ("uniform" if uniform else "actor", n)
    assert not any(np.isnan(rec[k]).any() for k in rec), what + ": a row was not written"
    assert same_bits(rec["obs"][0], obs0) and same_bits(rec["obs"][1:], rec["next_obs"][:-1])
    assert set(np.unique(rec["done"])) <= {0.0, 1.0} and np.abs(rec["action"]).max() <= 1.0
    check_loop_kernel_on_low_rackets(torch, env, words, done, params, rec["action"], rec["next_obs"], rec["reward"], rec["done"], what)
    env.close()
    print("%s: %.2f s" % (what, time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------------------------- d.
def episode_params():
    return pe.case_params(extended=True, scale=SCALE)


def oracle_episode_counters(params, actions, length, reward=None):
    """the nine counters the oracle books for exactly one episode per env (episode 0), env i stepped length[i] times with
    actions[:, i] on a batch of its own (a twin handle goes on stepping the envs that finished early: its counters hold more);
    reward [T, n]: those steps' rewards, compared bit for bit on the way"""
    total = np.zeros(len(COUNTER_NAMES), np.int64)
    for i in range(len(length)):
        pf = params.copy()
        pf.flags |= F_AUTO_RESET
        ref = OracleBatch(pf, ENV_TENNIS, 1, seed=ENV_SEED, env_id_base=ID_BASE + i, precision="f32")
        ref.reset()
        for t in range(int(length[i])):
            _, r, d, _ = ref.step(np.ascontiguousarray(actions[t, i:i + 1]))
            if reward is not None:
                assert same_bits(r, reward[t, i:i + 1]), "env %d step %d: the oracle's reward differs" % (i, t)
            assert bool(d[0]) == (t + 1 == length[i]), "env %d: the oracle's episode ends at another step" % i
        total += np.array([int(x) for x in ref.counters()], np.int64)
        ref.close()
    return dict(zip(COUNTER_NAMES, [int(x) for x in total]))


def check_episode_counters(c, want, length, what):
    n = len(length)
    print("%s: lengths %d .. %d, counters %s" % (what, length.min(), length.max(), c))
    assert c == want, (what, c, want)
    assert c["episodes_finished"] == n and c["substeps"] == int(length.sum()) and c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0
    assert c["racket_ball_contact_substeps"] > 0, what + ": no racket contact"
    assert len(set(length.tolist())) > 8, what + ": hardly any spread of episode lengths"


@pytest.mark.parametrize("net,deterministic", [(NET_DEFAULT, False), (NET_TUNED, True)])
def test_policy_evaluate_whole_episodes_at_scale_3(torch, net, deterministic):
    t0 = time.perf_counter()
    n, params, w = N_EPISODES, episode_params(), pe.blob(torch, ENV_TENNIS, net)
    a, b = pe.make_env(ENV_TENNIS, n, params, False), pe.make_env(ENV_TENNIS, n, params, False)
    ret, length = pe.evaluate(torch, a, w, deterministic, net)
    # the yardstick of test_gpu_policy_evaluate.step_loop -- policy_step after policy_step on a stepped twin -- with its steps kept
    obs = b.reset()
    acts, rews = [], []
    want_ret = torch.zeros(n, dtype=torch.float64, device=DEV)
    want_len = torch.zeros(n, dtype=torch.int32, device=DEV)
    active = torch.ones(n, dtype=torch.bool, device=DEV)
    for t in range(1001):
        (obs, r, d), (ac, _, _, _) = b.policy_step(w, obs, seed=NOISE_SEED, deterministic=deterministic, net=net)
        acts.append(ac); rews.append(r)
        want_ret += torch.where(active, r.double(), torch.zeros_like(want_ret))
        want_len += active.int()
        active &= d == 0
        if (t + 1) % 16 == 0 and not bool(active.any()):
            break
    assert not bool(active.any()), "an episode outlasted the step limit"
    what = "policy_evaluate net=%d det=%s" % (net, deterministic)
    assert np.array_equal(length, want_len.cpu().numpy()), what
    assert np.array_equal(ret, want_ret.cpu().numpy()), what
    assert np.any(ret != 0.0)
    want = oracle_episode_counters(params, torch.stack(acts).cpu().numpy(), length, torch.stack(rews).cpu().numpy())
    check_episode_counters(a.counters(), want, length, what)
    a.close(); b.close()
    print("%s: %.2f s" % (what, time.perf_counter() - t0))


def test_sac_evaluate_whole_episodes_at_scale_3(torch):
    t0 = time.perf_counter()
    n, params, act = N_EPISODES, episode_params(), ev.actor(torch, ENV_TENNIS, "plain")
    env = ev.make_env(ENV_TENNIS, n, params, False)
    ret, length, tr = ev.run(torch, env, act.flat)
    c = env.counters()
    env.close()
    what = "sac_evaluate"
    ev.check_env(torch, ENV_TENNIS, n, params, tr, ret, length, what)   # the trace replayed through tb_step on a twin
    check_episode_counters(c, oracle_episode_counters(params, tr["actions"], length, tr["reward"]), length, what)
    assert np.any(ret >= 25.0), "a racket contact that no return shows"
    print("%s: %.2f s" % (what, time.perf_counter() - t0))


def check_steps_from_reset(torch, env, params, actions, obs, rew, dn, what):
    """1001 steps from a common reset: the loop kernel's rows against tb_step on a twin and the oracle, then states and counters"""
    n = env.num_envs
    twin, ref = make_env(n, params), make_oracle(n, params)
    same(twin.reset().cpu().numpy(), ref.reset(), what + " reset obs")
    a_dev = torch.from_numpy(np.ascontiguousarray(actions)).to(DEV)
    outs = []
    for t in range(len(actions)):
        outs.append(twin.step(a_dev[t].clone()))
        o2, r2, d2, _ = ref.step(actions[t])
        same(obs[t], o2, "%s step %d obs against the oracle" % (what, t))
        same(rew[t], r2, "%s step %d reward against the oracle" % (what, t))
        same(dn[t] != 0, d2 != 0, "%s step %d done against the oracle" % (what, t))
    for k, name in enumerate(("obs", "reward", "done")):
        got = torch.stack([o[k] for o in outs]).cpu().numpy()
        same(got != 0 if k == 2 else got, (dn != 0) if k == 2 else (obs, rew)[k], "%s %s against tb_step" % (what, name))
    compare_state(env, ref, what + " final state")
    compare_state(twin, ref, what + " twin's final state")
    c, want = env.counters(), counters_of(ref)
    first = np.where((dn != 0).any(0), (dn != 0).argmax(0), len(dn))
    print("%s: first episodes end at steps %d .. %d, counters %s" % (what, first.min(), first.max(), c))
    assert c == want and twin.counters() == want, (what, c, want)
    assert c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0 and c["episodes_finished"] >= n
    assert c["racket_ball_contact_substeps"] > 0, what + ": no racket contact"
    assert len(set(first.tolist())) > 8, what + ": hardly any spread of episode lengths"
    twin.close(); ref.close()


def test_policy_rollout_1001_steps_at_scale_3(torch):
    t0 = time.perf_counter()
    n, params, w = N_EPISODES, episode_params(), pe.blob(torch, ENV_TENNIS, NET_DEFAULT)
    env = make_env(n, params, slices=3)
    (obs, rew, dn), (act, raw, _, _) = env.policy_rollout(w, env.reset(), 1001, seed=NOISE_SEED)
    torch.cuda.synchronize()
    check_steps_from_reset(torch, env, params, act.cpu().numpy(), obs.cpu().numpy(), rew.cpu().numpy(), dn.cpu().numpy(), "policy_rollout T=1001 slices=3")
    env.close()
    print("policy_rollout T=1001: %.2f s" % (time.perf_counter() - t0))


def test_sac_collect_1001_steps_at_scale_3(torch):
    t0 = time.perf_counter()
    n, params, act = N_EPISODES, episode_params(), ev.actor(torch, ENV_TENNIS, "plain")
    env = make_env(n, params)
    obs0 = env.reset().cpu().numpy()
    rec = sc.collect(torch, env, act.flat, (1001,))
    assert not any(np.isnan(rec[k]).any() for k in rec)
    assert same_bits(rec["obs"][0], obs0) and same_bits(rec["obs"][1:], rec["next_obs"][:-1])
    check_steps_from_reset(torch, env, params, rec["action"], rec["next_obs"], rec["reward"], rec["done"], "sac_collect 1001 steps")
    assert (rec["reward"] >= 25.0).any(), "a racket contact that no reward shows"
    env.close()
    print("sac_collect 1001 steps: %.2f s" % (time.perf_counter() - t0))
