"""Whole-episode evaluation of the fused policy (tb_policy_evaluate, tb_policy_evaluate_kernel in csrc/tb_kernels.hpp) on a real
MI355X. The yardstick is the existing one-step kernel, not the new one: a twin handle driven through policy_step
(tb_policy_step_net) with the same seed, env ids, parameters, noise seed and network must give every env the same float64 return
and the same length, bit for bit. Then the episode contract (call k is episode k; the handle is left freshly reset), the
trainers' evaluate_episodes and EvalSchedule leaving training bit-identical, and the refusals on a real handle.

Handle A is fresh, so its policy_evaluate call -- which resets first -- runs episode 0; handle B is reset once and stepped.
(With one env the batch's lengths cannot differ from one another: that assertion starts at two envs.)"""
import os

import numpy as np
import pytest

from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, NET_DEFAULT, NET_TUNED, OBS_DIM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE_SEED = 0x5EED1234ABCD
ENV_SEED, ID_BASE = 21, 1 << 33   # (env ids beyond 32 bits: the noise key's high word is in use)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_BLOBS = {}


def blob(torch, kind, net):
    """the packed weights of a case, built once: SwingRacket -- the reference's shipped policy (balls are struck); Tennisbot --
    seeded random weights with an action head that moves the racket (SB3's init is near zero) and unequal log_std"""
    from tennisbot_rl_amd.ppo import (SWING_DEFAULTS, TENNIS_DEFAULTS, TUNED_TENNIS_DEFAULTS, build_actor_critic, build_tuned_actor_critic, pack_policy)
    key = (kind, net)
    if key not in _BLOBS:
        torch.manual_seed(1234)
        if kind == ENV_SWING:
            policy = build_actor_critic(OBS_DIM[kind], ACT_DIM[kind], tuple(SWING_DEFAULTS["net_arch"]))
            policy.load_sb3_arrays(dict(np.load(os.path.join(ROOT, "tests", "golden", "ppo_swing_policy.npz"))))
        else:
            if net == NET_TUNED:
                policy = build_tuned_actor_critic(OBS_DIM[kind], ACT_DIM[kind], tuple(TUNED_TENNIS_DEFAULTS["net_arch"]), TUNED_TENNIS_DEFAULTS["extractor_hidden"])
            else:
                policy = build_actor_critic(OBS_DIM[kind], ACT_DIM[kind], tuple(TENNIS_DEFAULTS["net_arch"]))
            with torch.no_grad():
                policy.action_net.weight.mul_(30.0)
                policy.log_std.copy_(torch.linspace(-1.0, 0.2, ACT_DIM[kind]))
        _BLOBS[key] = pack_policy(policy.to("cuda:0"))
    return _BLOBS[key]


def case_params(extended=False, scale=1.0):
    from tennisbot_rl_amd.params import F_DEFAULT, F_RACKET_GROUND, default_params, reference_rolling_friction
    if extended:  # the reference's full contact set: racket<->court contact + the rolling-friction rows
        return default_params(racket_scale=scale, flags=F_DEFAULT | F_RACKET_GROUND, **reference_rolling_friction())
    return default_params(racket_scale=scale)


def make_env(kind, n, params, pipeline, seed=ENV_SEED):
    from tennisbot_rl_amd.stepper import BatchedEnv
    return BatchedEnv(kind, n, device="cuda:0", seed=seed, env_id_base=ID_BASE, params=params, pipeline=pipeline, track_terminal_obs=False)


def evaluate(torch, env, w, deterministic, net):
    ret, length = env.policy_evaluate(w, seed=NOISE_SEED, deterministic=deterministic, net=net)
    torch.cuda.synchronize()
    return ret.cpu().numpy(), length.cpu().numpy()


def step_loop(torch, env, obs, w, deterministic, net):
    """the yardstick: policy_step after policy_step from the freshly reset env (obs: what that reset returned); float64(reward)
    summed per env in step order through its first done, its steps counted"""
    n, swing = env.num_envs, env.kind == ENV_SWING
    ret = torch.zeros(n, dtype=torch.float64, device=env.device)
    length = torch.zeros(n, dtype=torch.int32, device=env.device)
    active = torch.ones(n, dtype=torch.bool, device=env.device)
    for t in range(26 if swing else 1001):
        (obs, r, d), _ = env.policy_step(w, obs, seed=NOISE_SEED, deterministic=deterministic, net=net)
        ret += torch.where(active, r.double(), torch.zeros_like(ret))
        length += active.int()
        active &= d == 0
        if not swing and (t + 1) % 16 == 0 and not bool(active.any()):
            break
    assert not bool(active.any()), "an episode outlasted the step limit"
    return ret.cpu().numpy(), length.cpu().numpy()


TENNIS_CASES = [  # n, deterministic, net, extended contact set, racket scale
    (1, False, NET_DEFAULT, False, 1.0),     # one live lane
    (15, True, NET_DEFAULT, False, 1.0),
    (16, False, NET_TUNED, False, 1.0),      # the slice's edge
    (17, False, NET_DEFAULT, False, 1.0),    # a second workgroup that holds a single env
    (33, False, NET_DEFAULT, False, 1.0),    # workgroups that finish at different steps
    (33, True, NET_TUNED, False, 1.0),
    (33, False, NET_DEFAULT, False, 3.0),    # a racket big enough to be hit under random weights: reward 25 + tier
    (33, False, NET_DEFAULT, True, 1.0),     # F_RACKET_GROUND + rolling friction
]


@pytest.mark.parametrize("n,deterministic,net,extended,scale", TENNIS_CASES)
def test_tennisbot_twin_replay_bit_for_bit(torch, n, deterministic, net, extended, scale):
    w, params = blob(torch, ENV_TENNIS, net), case_params(extended, scale)
    a, b = make_env(ENV_TENNIS, n, params, False), make_env(ENV_TENNIS, n, params, False)
    obs = b.reset()
    ret, length = evaluate(torch, a, w, deterministic, net)
    want_ret, want_len = step_loop(torch, b, obs, w, deterministic, net)
    print("Tennisbot n=%d det=%s net=%d ext=%s scale=%g: lengths %d .. %d, returns %g .. %g" % (n, deterministic, net, extended, scale, length.min(), length.max(), ret.min(), ret.max()))
    assert length.dtype == np.int32 and ret.dtype == np.float64 and ret.shape == (n,) and length.shape == (n,)
    assert np.array_equal(length, want_len), (length, want_len)
    assert np.array_equal(ret, want_ret), (ret, want_ret)
    assert np.all((length >= 1) & (length <= 1001))
    if n > 1:
        assert len(set(length.tolist())) > 1, "every episode of the batch has the same length"
    assert np.any(ret != 0.0)
    c = a.counters()
    assert c["episodes_finished"] == n and c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0
    if scale != 1.0:
        assert c["racket_ball_contact_substeps"] > 0, "no racket contact in this case"
    a.close(); b.close()


SWING_CASES = [  # n, deterministic, extended contact set
    (1, False, False), (16, True, False), (17, False, False), (48, False, False), (48, True, False), (17, False, True),
]


@pytest.mark.parametrize("n,deterministic,extended", SWING_CASES)
def test_swingracket_twin_replay_bit_for_bit(torch, n, deterministic, extended):
    w, params = blob(torch, ENV_SWING, NET_DEFAULT), case_params(extended)
    a, b = make_env(ENV_SWING, n, params, True), make_env(ENV_SWING, n, params, False)
    obs = b.reset()
    ret, length = evaluate(torch, a, w, deterministic, NET_DEFAULT)
    want_ret, want_len = step_loop(torch, b, obs, w, deterministic, NET_DEFAULT)
    print("SwingRacket n=%d det=%s ext=%s: returns %g .. %g" % (n, deterministic, extended, ret.min(), ret.max()))
    assert np.array_equal(length, want_len) and np.all(length == 26)
    assert np.array_equal(ret, want_ret), (ret, want_ret)
    assert np.any(ret != 0.0)
    c = a.counters()
    assert c["episodes_finished"] == n and c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0
    assert a.phase() == 0
    a.close(); b.close()


@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
def test_call_k_is_episode_k_and_the_handle_is_left_freshly_reset(torch, kind):
    n, swing = 17, kind == ENV_SWING
    w, params = blob(torch, kind, NET_DEFAULT), case_params()
    a, twin, plain = (make_env(kind, n, params, swing) for _ in range(3))
    r0, l0 = evaluate(torch, a, w, False, NET_DEFAULT)
    r1, l1 = evaluate(torch, a, w, False, NET_DEFAULT)
    assert not np.array_equal(r0, r1), "two calls on one handle returned the same episodes"
    t0, tl0 = evaluate(torch, twin, w, False, NET_DEFAULT)
    assert np.array_equal(t0, r0) and np.array_equal(tl0, l0)       # a fresh twin's first call repeats the first
    # after call 1 the handle holds what a plain reset leaves at episode 1 ...
    plain.reset()
    obs1 = plain.reset()
    wa, da = a.get_state_words()
    wp, dp = plain.get_state_words()
    assert torch.equal(wa, wp) and torch.equal(da, dp)
    assert int(wa[-1].min()) == 1 and int(wa[-1].max()) == 1       # (the episode word)
    # ... so the step loop from there reproduces call 1, and a reset followed by a call is the episode after it
    s1, sl1 = step_loop(torch, plain, obs1, w, False, NET_DEFAULT) if not swing else (r1, l1)
    assert np.array_equal(s1, r1) and np.array_equal(sl1, l1)
    twin.reset()                                                   # twin: call 0, a reset (episode 1), then a call: episode 2
    t2, _ = evaluate(torch, twin, w, False, NET_DEFAULT)
    r2, _ = evaluate(torch, a, w, False, NET_DEFAULT)
    assert np.array_equal(t2, r2) and not np.array_equal(r2, r1)
    for e in (a, twin, plain):
        e.close()


def test_policy_evaluator_statistics_and_racket_scale(torch):
    """PolicyEvaluator: ceil(n_episodes / n_envs) calls, the surplus dropped, float64 statistics of exactly those episodes"""
    from tennisbot_rl_amd.evaluation import PolicyEvaluator
    w = blob(torch, ENV_SWING, NET_DEFAULT)
    ev = PolicyEvaluator(ENV_SWING, n_envs=16, seed=4, device="cuda:0")
    twin = PolicyEvaluator(ENV_SWING, n_envs=16, seed=4, device="cuda:0")
    state = torch.cuda.get_rng_state("cuda:0").clone()
    out = ev.evaluate(w, 40)
    r, ln = twin.episodes(w, 40)
    assert torch.equal(torch.cuda.get_rng_state("cuda:0"), state), "the evaluation drew from torch's RNG"
    r = r.cpu().numpy()
    assert r.shape == (40,) and out["episodes"] == 40 and out["mean_length"] == 26.0
    assert out["mean"] == pytest.approx(r.mean(), rel=1e-12) and out["std"] == pytest.approx(r.std(), rel=1e-12)
    assert out["min"] == r.min() and out["max"] == r.max()
    assert ev.env.env_id_base != 0 and ev.env.pipeline and ev.env.phase() == 0
    ev.close(); twin.close()


def test_schedule_leaves_ppo_training_bit_identical(torch, tmp_path):
    """three rollouts (eager, capture, replay) with an evaluation and a best-model save after every one, against the same run
    without: the weights, the training envs and the captured graph do not notice"""
    from tennisbot_rl_amd.evaluation import EvalSchedule
    from tennisbot_rl_amd.ppo import PPOTrainer
    mk = lambda: PPOTrainer("SwingRacket-v0", num_envs=64, n_steps=26, device="cuda:0", seed=3, learner="fused", graph=True)  # noqa: E731
    sched = EvalSchedule(eval_freq=1, n_eval_episodes=32, best_model_save_path=str(tmp_path), save_freq=2 * 26 * 64, save_path=str(tmp_path))
    total = 3 * 26 * 64
    a = mk()   # (each trainer is built right before its run: the constructor seeds torch's RNG, which the update's randperm draws from)
    a.learn(total, log=None, schedule=sched)
    b = mk()
    b.learn(total, log=None)
    torch.cuda.synchronize()
    assert [h["timesteps"] for h in sched.history] == [26 * 64, 2 * 26 * 64, 3 * 26 * 64] and all(h["episodes"] == 32 and h["mean_length"] == 26.0 for h in sched.history)
    sa, sb = a.policy.state_dict(), b.policy.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k].view(torch.int32), sb[k].view(torch.int32)), "%s differs between the run with and the run without the schedule" % k
    wa, da = a.env.get_state_words()
    wb, db = b.env.get_state_words()
    assert torch.equal(wa, wb) and torch.equal(da, db)
    assert a._graph is not None and a._graph.valid() and b._graph is not None
    best = os.path.join(str(tmp_path), "best_model.pt")
    assert os.path.exists(best) and sched.best_mean == max(h["mean"] for h in sched.history)
    assert [os.path.basename(p) for p in sched.checkpoints] == ["rl_model_%d_steps.pt" % (2 * 26 * 64)]
    ck = torch.load(best, map_location="cpu", weights_only=True)
    assert set(ck["policy"].keys()) == set(sa.keys())
    b.load(best)                                                   # ... and it loads
    assert b.num_timesteps in (26 * 64, 2 * 26 * 64, 3 * 26 * 64)
    # the trainer's own call, outside a schedule
    out = a.evaluate_episodes(20)
    assert out["episodes"] == 20 and out["mean_length"] == 26.0 and out["min"] <= out["mean"] <= out["max"]


def test_sac_evaluate_episodes_and_schedule_leave_training_alone(torch):
    from tennisbot_rl_amd.evaluation import EvalSchedule
    from tennisbot_rl_amd.sac import SACTrainer
    mk = lambda: SACTrainer("Tennisbot-v0", num_envs=16, batch_size=32, gradient_steps=2, buffer_size=4096, learning_starts=16, seed=3, device="cuda:0")  # noqa: E731
    a = mk()   # (each trainer is built right before its run: the constructor seeds torch's RNG, which collect and train draw from)
    w0, d0 = a.env.get_state_words()
    obs0 = a.obs.clone()
    state = torch.cuda.get_rng_state("cuda:0").clone()
    out = a.evaluate_episodes(20, n_envs=16)
    assert out["episodes"] == 20 and 1.0 <= out["mean_length"] <= 1001.0 and out["min"] <= out["mean"] <= out["max"]
    assert a.evaluate_episodes(5, deterministic=True, n_envs=16)["episodes"] == 5
    w1, d1 = a.env.get_state_words()
    assert torch.equal(w0, w1) and torch.equal(d0, d1) and torch.equal(a.obs, obs0)
    assert torch.equal(torch.cuda.get_rng_state("cuda:0"), state), "the evaluation drew from torch's global RNG"
    sched = EvalSchedule(eval_freq=32, n_eval_episodes=16)
    a.learn(5 * 16, log=None, schedule=sched)
    b = mk()
    b.learn(5 * 16, log=None)
    torch.cuda.synchronize()
    assert [h["timesteps"] for h in sched.history] == [32, 64] and a._learner.step == b._learner.step and a._learner.step > 0
    sa, sb = a.actor.state_dict(), b.actor.state_dict()
    for k in sa:
        assert torch.equal(sa[k].view(torch.int32), sb[k].view(torch.int32)), k
    assert not torch.equal(sa[next(iter(sa))], mk().actor.state_dict()[next(iter(sa))]), "the five vector steps trained nothing"


def test_refusals_on_a_real_handle_launch_nothing(torch):
    from tennisbot_rl_amd.stepper import StepperError
    w = blob(torch, ENV_SWING, NET_DEFAULT)
    ret = torch.zeros(16, dtype=torch.float64, device="cuda:0")
    length = torch.zeros(16, dtype=torch.int32, device="cuda:0")
    # SwingRacket without the pipeline: TB_E_UNSUPPORTED
    plain = make_env(ENV_SWING, 16, case_params(), False)
    plain.reset()
    w0, d0 = plain.get_state_words()
    with pytest.raises(StepperError, match="tb_set_pipeline"):
        plain.policy_evaluate(w)
    rc = plain.L.tb_policy_evaluate(plain._h, NET_DEFAULT, w.data_ptr(), ret.data_ptr(), length.data_ptr(), 1, 0, None)
    assert rc == -4
    w1, d1 = plain.get_state_words()
    assert torch.equal(w0, w1) and torch.equal(d0, d1)
    # the tuned network is Tennisbot's: TB_E_PARAMS, on a handle that could otherwise evaluate
    piped = make_env(ENV_SWING, 16, case_params(), True)
    piped.reset()
    w0, d0 = piped.get_state_words()
    rc = piped.L.tb_policy_evaluate(piped._h, NET_TUNED, w.data_ptr(), ret.data_ptr(), length.data_ptr(), 1, 0, None)
    assert rc == -3 and b"Tennisbot" in piped.L.tb_last_error() and b"tb_policy_evaluate" in piped.L.tb_last_error()
    with pytest.raises(StepperError):
        piped.policy_evaluate(w, net=NET_TUNED)
    rc = piped.L.tb_policy_evaluate(piped._h, NET_DEFAULT, None, ret.data_ptr(), length.data_ptr(), 1, 0, None)
    assert rc == -1
    w1, d1 = piped.get_state_words()
    assert torch.equal(w0, w1) and torch.equal(d0, d1) and piped.phase() == 0
    torch.cuda.synchronize()
    assert float(ret.abs().sum()) == 0.0 and int(length.abs().sum()) == 0   # nothing was written
    # ... and the handle still evaluates
    r, ln = piped.policy_evaluate(w, seed=NOISE_SEED)
    assert bool((ln == 26).all())
    plain.close(); piped.close()
