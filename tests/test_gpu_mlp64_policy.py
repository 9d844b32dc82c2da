"""TB_NET_MLP64 inside the fused policy kernels (SB3's [64, 64] on SwingRacket-v0: tb_policy_step_net, tb_policy_rollout_net,
tb_policy_evaluate; TowerRegs<TB_ENV_SWING, TB_NET_MLP64> in csrc/tb_policy.hpp). The one-step kernel against the float64 towers,
sample and logp of tests/policy_reference.py with the checks of test_gpu_policy_reference.py; the rollout kernel, in both
policy_slices forms and with the extended contact set, bit for bit against 52 one-step calls; the evaluation kernel bit for bit
against the stepped twin of test_gpu_policy_evaluate.py; and TB_NET_DEFAULT around a TB_NET_MLP64 call on one handle. Batch sizes:
one env, and both sides of the 16-env slice and of the 48-env workgroup.
Two weight sets. "crafted": mlp64_fixtures.policy (action head x 30, unequal stds, non-zero biases) -- its rackets flail and never meet
a ball, every return is 0. "student": tests/golden/mlp64_swing_student.npz, a [64, 64] net fitted to the action means and values of the
reference's shipped ppo_swing policy (tests/golden/ppo_swing_policy.npz) with that policy's log_std: it strikes the ball in every
episode, so rollouts and evaluations go through racket contacts, goal hits and fast-forwards that differ from env to env."""
import os

import numpy as np
import pytest

import mlp64_fixtures as fx
import policy_reference as pr
from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, NET_DEFAULT, NET_MLP64
from test_gpu_policy_evaluate import case_params, evaluate, make_env, step_loop
from test_gpu_policy_reference import NOISE_SEED, _bits_equal, check_outputs, crafted, keys_of

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 48, 49)
A = ACT_DIM[ENV_SWING]
T = 52                                  # two SwingRacket episodes
STUDENT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp64_swing_student.npz")
_made = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def packed(torch, name="crafted"):
    """a weight set's policy and its blob, built once"""
    if name not in _made:
        from tennisbot_rl_amd.ppo import build_actor_critic, pack_policy
        if name == "student":
            policy = build_actor_critic(6, 6, fx.ARCH)
            policy.load_state_dict({k: torch.from_numpy(v) for k, v in np.load(STUDENT).items()})
        else:
            policy = fx.policy()
        policy = policy.to("cuda:0")
        _made[name] = policy, pack_policy(policy)
        assert _made[name][1].numel() == fx.BLOB_FLOATS
    return _made[name]


@pytest.mark.parametrize("n", SIZES)
def test_policy_step_matches_the_float64_reference(torch, n):
    from tennisbot_rl_amd.stepper import BatchedEnv
    policy, blob = packed(torch)
    det = BatchedEnv(ENV_SWING, n, device="cuda:0", seed=13)
    sto = BatchedEnv(ENV_SWING, n, device="cuda:0", seed=13)
    assert det.policy_floats(NET_MLP64) == fx.BLOB_FLOATS
    obs = det.reset()
    sto.reset()
    obs_in, _ = crafted(obs.cpu().numpy())
    episode, step_count = keys_of(sto)
    x = torch.from_numpy(obs_in).to("cuda:0")
    _, (act_d, raw_d, logp_d, val_d) = det.policy_step(blob, x, seed=NOISE_SEED, deterministic=True, net=NET_MLP64)
    _, (act_s, raw_s, logp_s, val_s) = sto.policy_step(blob, x, seed=NOISE_SEED, net=NET_MLP64)
    torch.cuda.synchronize()
    ref = pr.towers(policy, obs_in)
    eps = pr.policy_noise(NOISE_SEED, np.arange(n, dtype=np.uint64), episode, step_count, A)
    h = lambda t: t.cpu().numpy()  # noqa: E731
    check_outputs("mlp64 n=%d deterministic" % n, ref, None, h(act_d), h(raw_d), h(logp_d), h(val_d), True)
    check_outputs("mlp64 n=%d stochastic" % n, ref, eps, h(act_s), h(raw_s), h(logp_s), h(val_s), False)
    assert np.array_equal(h(val_d).view(np.uint32), h(val_s).view(np.uint32))          # the value does not depend on the noise
    ep1, sc1 = keys_of(sto)
    assert np.array_equal(ep1, episode) and np.array_equal(sc1, step_count + 1)
    det.close(); sto.close()


ROLLOUTS = [(n, s, False) for s in (1, 3) for n in SIZES] + [(49, 1, True), (17, 3, True)]   # n, policy_slices, the extended contact set


@pytest.mark.parametrize("n,slices,extended", ROLLOUTS)
def test_policy_rollout_equals_repeated_policy_steps(torch, n, slices, extended):
    from tennisbot_rl_amd.stepper import BatchedEnv
    _, blob = packed(torch, "student" if n >= 16 else "crafted")
    prm = case_params(True) if extended else None
    a = BatchedEnv(ENV_SWING, n, device="cuda:0", seed=8, pipeline=True, track_terminal_obs=False, params=prm, options=dict(policy_slices=slices))
    b = BatchedEnv(ENV_SWING, n, device="cuda:0", seed=8, pipeline=True, track_terminal_obs=False, params=prm)
    oa, ob = a.reset(), b.reset()
    (obs, rew, done), pol = a.policy_rollout(blob, oa, T, seed=NOISE_SEED, net=NET_MLP64)
    a.flush()
    steps = []
    for t in range(T):
        (ob, r, d), p1 = b.policy_step(blob, ob, seed=NOISE_SEED, net=NET_MLP64)
        steps.append((ob, r, d) + tuple(p1))
    b.flush()
    torch.cuda.synchronize()
    for t, row in enumerate(steps):
        for name, x, y in zip(("obs", "reward", "done", "actions", "raw", "logp", "value"), (obs[t], rew[t], done[t]) + tuple(p[t] for p in pol), row):
            assert _bits_equal(x, y), "step %d: %s differs between tb_policy_rollout_net and tb_policy_step_net" % (t, name)
    assert int(done.sum()) == 2 * n and bool(done[25].all()) and bool(done[51].all())
    wa, da = a.get_state_words(); wb, db = b.get_state_words()
    assert torch.equal(wa, wb) and torch.equal(da, db) and a.counters() == b.counters()
    c = a.counters()
    assert c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0, c
    if n >= 16:
        assert c["racket_ball_contact_substeps"] > 0 and float(rew.abs().sum()) > 0.0, "the student struck no ball"
    a.close(); b.close()


EVALUATIONS = [(n, False, False) for n in SIZES] + [(17, True, False), (49, True, False), (17, False, True)]   # n, deterministic, extended


@pytest.mark.parametrize("n,deterministic,extended", EVALUATIONS)
def test_policy_evaluate_equals_the_stepped_twin(torch, n, deterministic, extended):
    """tb_policy_evaluate has no action output: returns (float64 sums of every step's reward) and lengths are what it reports, and they are
    compared bit for bit with a tb_policy_step_net loop on a twin env, as tests/test_gpu_policy_evaluate.py does. The actions are covered
    through the returns: the student strikes the ball in every episode, so each return is a contact bonus per substep of contact plus
    a terminal reward of the flight the racket gave the ball -- one differing action bit moves them. (The rollout test above compares
    the actions themselves, from the same sampling code.)"""
    _, blob = packed(torch, "student")
    params = case_params(extended)
    a, b = make_env(ENV_SWING, n, params, True), make_env(ENV_SWING, n, params, False)
    obs = b.reset()
    ret, length = evaluate(torch, a, blob, deterministic, NET_MLP64)
    want_ret, want_len = step_loop(torch, b, obs, blob, deterministic, NET_MLP64)
    assert np.array_equal(length, want_len) and np.all(length == 26)
    assert np.array_equal(ret, want_ret), (ret, want_ret)
    print("mlp64 evaluate n=%d det=%s ext=%s: returns %g .. %g, %d of them non-zero" % (n, deterministic, extended, ret.min(), ret.max(), int((ret != 0).sum())))
    assert np.any(ret != 0.0), "every return is 0: the student struck no ball"
    c = a.counters()
    assert c["episodes_finished"] == n and c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0
    assert a.phase() == 0
    a.close(); b.close()


def test_the_default_net_around_an_mlp64_call_gives_its_usual_bits(torch):
    """the net is an argument of the call: TB_NET_DEFAULT before and after TB_NET_MLP64 on one handle gives what a handle that never saw
    the new net gives, in the one-step and the rollout form; the pairs that are not built are refused"""
    from tennisbot_rl_amd.evaluation import PolicyEvaluator
    from tennisbot_rl_amd.ppo import SWING_DEFAULTS, build_actor_critic, pack_policy
    from tennisbot_rl_amd.stepper import BatchedEnv, StepperError
    _, blob64 = packed(torch)
    torch.manual_seed(2)
    default = build_actor_critic(6, 6, tuple(SWING_DEFAULTS["net_arch"])).to("cuda:0")
    with torch.no_grad():
        default.action_net.weight.mul_(20.0)
    default_blob = pack_policy(default)
    n = 49
    mk = lambda: BatchedEnv(ENV_SWING, n, device="cuda:0", seed=6, pipeline=True, track_terminal_obs=False)  # noqa: E731
    used, fresh = mk(), mk()
    o = used.reset(); fresh.reset()
    before = used.policy_step(default_blob, o, seed=NOISE_SEED, net=NET_DEFAULT), fresh.policy_step(default_blob, o, seed=NOISE_SEED)
    for x, y in zip(before[0][0] + before[0][1], before[1][0] + before[1][1]):
        assert _bits_equal(x, y)
    o1 = before[0][0][0]
    w, d = fresh.get_state_words()
    used.policy_step(blob64, o1, seed=NOISE_SEED, net=NET_MLP64)
    used.policy_rollout(blob64, o1, 3, seed=NOISE_SEED, net=NET_MLP64)
    used.flush()
    used.set_state_words(w, d)                       # the same env state again: only the handle's history differs
    for form in ("step", "rollout"):
        if form == "step":
            ra, rb = used.policy_step(default_blob, o1, seed=NOISE_SEED, net=NET_DEFAULT), fresh.policy_step(default_blob, o1, seed=NOISE_SEED)
        else:
            ra, rb = used.policy_rollout(default_blob, o1, 5, seed=NOISE_SEED, net=NET_DEFAULT), fresh.policy_rollout(default_blob, o1, 5, seed=NOISE_SEED)
        used.flush(); fresh.flush()
        for x, y in zip(ra[0] + ra[1], rb[0] + rb[1]):
            assert _bits_equal(x, y), form
        o1 = ra[0][0] if form == "step" else ra[0][0][-1]
    with pytest.raises(ValueError):
        used.policy_step(default_blob, o1, net=NET_MLP64)       # the default net's blob is not the new net's length
    tennis = BatchedEnv(ENV_TENNIS, 16, device="cuda:0", seed=6)
    to = tennis.reset()
    with pytest.raises(ValueError, match="NET_DEFAULT"):
        tennis.policy_floats(NET_MLP64)
    z = torch.zeros(16384, device="cuda:0")
    rc = tennis.L.tb_policy_step_net(tennis._h, NET_MLP64, z.data_ptr(), to.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                     z.data_ptr(), z.data_ptr(), 0, 0, None)
    assert rc == -3 and b"TB_NET_DEFAULT is that net" in tennis.L.tb_last_error()     # TB_E_PARAMS, before anything is launched
    with pytest.raises(StepperError, match="Tennisbot"):
        used.policy_floats(1)
    ev = PolicyEvaluator(ENV_SWING, n_envs=16, seed=3, net=NET_MLP64)
    stats = ev.evaluate(blob64, 16)
    assert stats["episodes"] == 16 and stats["mean_length"] == 26.0 and np.isfinite(stats["mean"])
    ev.close()
    for e in (used, fresh, tennis):
        e.close()
