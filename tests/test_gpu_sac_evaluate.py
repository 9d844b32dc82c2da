"""Whole-episode evaluation of the SAC / TQC actor in one launch (tb_sac_evaluate, tb_sac_evaluate_kernel in csrc/tb_sac.hpp) on
a real MI355X. Everything is checked from the per-step trace of a fresh handle, every traced row with t < length, none left out:

  1. the actor: the traced obs / eps rows through the EXISTING tb_sac_actor_forward (FusedSAC.actor_forward, idx = arange, chunks
     of 2048 rows) give the traced actions bit for bit; and, independently of that kernel, the actions are within
     ppo_reference.MULTIPLE float32-twin errors of sac_reference.actor_forward in float64 (test_gpu_sac.py's measure);
  2. the env: an unpipelined twin handle (same seed, id base, parameters), reset once and stepped by BatchedEnv.step with the traced
     actions, gives the traced obs[t + 1], reward and done bit for bit; the return is the float64 sum of the float32 rewards
     through the first done, bit for bit, and the length that step count;
  3. the noise keys, 4. both loop exits, 5. the episode contract and the refusals, 6. trace neutrality with guard words,
  7. the trainers' fused evaluate_episodes leaving training bit-identical.

Actors: `plain` -- seeded torch-default init with the mu head scaled so that the racket moves; `edge` -- the log_std head's bias
spread from -25 to 4 (both clamps bind) and mu scaled until tanh saturates to +-1 in float32."""
import ctypes
import os

import numpy as np
import pytest

import ppo_reference as ref
import sac_reference as sr
from helpers import same_bits
from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, OBS_DIM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NOISE_SEED = 0x5EED1234ABCD
ENV_SEED, ID_BASE = 21, 1 << 33   # (env ids beyond 32 bits: the noise key's high word is in use)
# seeds of the torch-default init, picked from a measurement so that the cases below see both loop exits, a racket contact at scale 3
# and struck balls on SwingRacket (most seeds give a racket that runs away from every ball: every episode at the cap, every return 0)
ACTOR_SEED = {(ENV_SWING, "plain"): 3, (ENV_SWING, "edge"): 1235, (ENV_TENNIS, "plain"): 1235, (ENV_TENNIS, "edge"): 1235}
MU_SCALE = {"plain": 30.0, "edge": 3000.0}
CHUNK = 2048
T_MAX = {ENV_SWING: 26, ENV_TENNIS: 1001}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


# ------------------------------------------------------------------------------------------------------------------- the actors
_ACTORS = {}


class Actor:
    """one case's actor: the FusedSAC that owns the flat vector (and tb_sac_actor_forward), and the arrays by name"""

    def __init__(self, torch, kind, which):
        from tennisbot_rl_amd.sac import FusedSAC, build_sac_modules
        O, A = OBS_DIM[kind], ACT_DIM[kind]
        torch.manual_seed(ACTOR_SEED[(kind, which)])
        mods = build_sac_modules(O, A)
        with torch.no_grad():
            mods[0].mu.weight.mul_(MU_SCALE[which])
            if which == "edge":
                mods[0].log_std.bias.copy_(torch.linspace(-25.0, 4.0, A))
        for m in mods:
            m.to(DEV)
        lec = torch.zeros(1, dtype=torch.float32, device=DEV, requires_grad=True)
        opts = (torch.optim.Adam(mods[0].parameters(), lr=sr.LR, eps=sr.ADAM_EPS), torch.optim.Adam(mods[1].parameters(), lr=sr.LR, eps=sr.ADAM_EPS),
                torch.optim.Adam([lec], lr=sr.LR, eps=sr.ADAM_EPS))
        self.learner = FusedSAC(kind, mods[0], mods[1], mods[2], lec, opts, {}, torch.device(DEV))
        self.flat = self.learner.pi.flat
        self.arrays = {k: p.detach().cpu().numpy().copy() for k, p in mods[0].named_parameters()}
        assert tuple(self.arrays) == sr.ACTOR_NAMES and self.flat.numel() == sr.n_floats(sr.actor_shapes(O, A))


def actor(torch, kind, which):
    key = (kind, which)
    if key not in _ACTORS:
        _ACTORS[key] = Actor(torch, kind, which)
    return _ACTORS[key]


def case_params(extended=False, scale=1.0):
    from tennisbot_rl_amd.params import F_DEFAULT, F_RACKET_GROUND, default_params, reference_rolling_friction
    if extended:  # the reference's full contact set: racket<->court contact + the rolling-friction rows
        return default_params(racket_scale=scale, flags=F_DEFAULT | F_RACKET_GROUND, **reference_rolling_friction())
    return default_params(racket_scale=scale)


def make_env(kind, n, params, pipeline, seed=ENV_SEED):
    from tennisbot_rl_amd.stepper import BatchedEnv
    return BatchedEnv(kind, n, device=DEV, seed=seed, env_id_base=ID_BASE, params=params, pipeline=pipeline, track_terminal_obs=False)


def host(x):
    return x.detach().cpu().numpy().copy()


def same_trace(a, b, rows=slice(None)):
    """two traces, bit for bit (done is uint8: compared as it is)"""
    return all(np.array_equal(a[k], b[k][rows]) if a[k].dtype == np.uint8 else same_bits(a[k], b[k][rows]) for k in a)


def run(torch, env, flat, deterministic=False, trace=True, max_steps=None):
    out = env.sac_evaluate(flat, seed=NOISE_SEED, deterministic=deterministic, trace=trace, max_steps=max_steps)
    torch.cuda.synchronize()
    ret, length = host(out[0]), host(out[1])
    return (ret, length, {k: host(v) for k, v in out[2].items()}) if trace else (ret, length)


# ------------------------------------------------------------------------------------------------------------------- the checks
def live_rows(tr, length):
    T = tr["reward"].shape[0]
    return np.arange(T)[:, None] < length[None, :]   # [T, n]: the env's episode ran step t


def check_actor(torch, act, kind, tr, length, deterministic, name):
    live = live_rows(tr, length)
    obs, eps, got = (np.ascontiguousarray(tr[k][live]) for k in ("obs", "eps", "actions"))   # [R, .]: every traced row
    R = len(obs)
    assert R == int(length.sum()) and R > 0
    if deterministic:
        assert not eps.any() and not tr["eps"].any(), "a deterministic run traced noise"
    else:
        assert np.all(np.abs(eps).max(axis=1) > 0), "a stochastic row drew no noise"
    # (a) the existing kernel, bit for bit; every chunk has CHUNK rows (the last one padded with row 0) so the workspace is built once
    L = act.learner
    idx = torch.arange(CHUNK, dtype=torch.int64, device=DEV)
    bits = np.empty_like(got)
    for s in range(0, R, CHUNK):
        m = min(CHUNK, R - s)
        o, e = np.repeat(obs[:1], CHUNK, 0), np.repeat(eps[:1], CHUNK, 0)
        o[:m], e[:m] = obs[s:s + m], eps[s:s + m]
        a_t, _ = L.actor_forward(torch.from_numpy(o).to(DEV), idx, torch.from_numpy(e).to(DEV))
        bits[s:s + m] = host(a_t)[:m]
    assert same_bits(bits, got), "%s: %d of %d traced action rows differ from tb_sac_actor_forward on the traced obs / eps" % (
        name, int((bits.view(np.uint32) != got.view(np.uint32)).any(axis=1).sum()), R)
    # (b) the float64 reference, independently of that kernel
    want, twin = (sr.actor_forward(act.arrays, obs, eps, dt) for dt in (np.float64, np.float32))
    r = ref.check_tensors("%s actions" % name, {"a": got}, {"a": want.a}, {"a": twin.a}, ref.MULTIPLE)
    assert np.all(np.abs(got) <= 1.0)
    return r, want


def check_env(torch, kind, n, params, tr, ret, length, name, episode=0):
    """the twin: unpipelined, reset episode + 1 times (so it is at the start of that episode), stepped with the traced actions"""
    T = tr["reward"].shape[0]
    live = live_rows(tr, length)
    assert length.min() >= 1 and length.max() <= T_MAX[kind]
    twin = make_env(kind, n, params, False)
    for _ in range(episode + 1):
        obs0 = twin.reset()
    assert same_bits(host(obs0), tr["obs"][0]), "%s: the first traced observation is not the reset's" % name
    obs_r, rew_r, done_r = [], [], []
    for t in range(int(length.max())):
        o, r, d = twin.step(torch.from_numpy(np.ascontiguousarray(tr["actions"][t])).to(DEV))
        obs_r.append(host(o)); rew_r.append(host(r)); done_r.append(host(d))
    c = twin.counters()
    twin.close()
    Tl = len(obs_r)
    obs_r, rew_r, done_r = np.stack(obs_r), np.stack(rew_r), np.stack(done_r)
    a = live[:Tl]
    assert not live[Tl:].any()
    assert same_bits(rew_r[a], tr["reward"][:Tl][a]), "%s: rewards differ from the twin's" % name
    assert np.array_equal(done_r[a] != 0, tr["done"][:Tl][a] != 0), "%s: done flags differ from the twin's" % name
    nxt = live[1:Tl]   # obs[t + 1] was recorded: step t was not the env's last
    assert same_bits(obs_r[:Tl - 1][nxt], tr["obs"][1:Tl][nxt]), "%s: observations differ from the twin's" % name
    # the return: float64 sum in step order through the first done; the length: that step count
    done = tr["done"] != 0
    first = np.where(done.any(0), done.argmax(0), -1)
    assert np.array_equal(first + 1, length), "%s: length is not the first done + 1" % name
    s = np.zeros(n)
    for t in range(T):
        s = np.where(live[t], s + tr["reward"][t].astype(np.float64), s)
    assert same_bits(s, ret), "%s: the return is not the float64 sum of the traced rewards" % name
    # rows after an env's last step were not written
    for k in ("obs", "eps", "actions", "reward", "done"):
        assert not tr[k][~live].any(), "%s: %s has rows written after an env's last step" % (name, k)
    return c


_CASES = {}


def case(torch, kind, n, deterministic=False, which="plain", extended=False, scale=1.0):
    """one case, run and checked once: (ret, length, trace, counters, float64 pass)"""
    key = (kind, n, deterministic, which, extended, scale)
    if key in _CASES:
        return _CASES[key]
    name = "%s n=%d det=%s actor=%s ext=%s scale=%g" % ("SwingRacket" if kind == ENV_SWING else "Tennisbot", n, deterministic, which, extended, scale)
    act, params = actor(torch, kind, which), case_params(extended, scale)
    env = make_env(kind, n, params, kind == ENV_SWING)
    ret, length, tr = run(torch, env, act.flat, deterministic)
    c = env.counters()
    assert env.phase() == 0
    env.close()
    assert ret.dtype == np.float64 and length.dtype == np.int32 and ret.shape == (n,) and length.shape == (n,)
    ratio, want = check_actor(torch, act, kind, tr, length, deterministic, name)
    check_env(torch, kind, n, params, tr, ret, length, name)
    print("%s: lengths %d .. %d, returns %g .. %g, actions %.3g twin errors from float64, racket contacts %d"
          % (name, length.min(), length.max(), ret.min(), ret.max(), ratio, c["racket_ball_contact_substeps"]))
    assert c["episodes_finished"] == n and c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0
    _CASES[key] = (ret, length, tr, c, want)
    return _CASES[key]


TENNIS_CASES = [  # n, deterministic, actor, extended contact set, racket scale
    (1, False, "plain", False, 1.0),     # one live lane
    (15, True, "plain", False, 1.0),
    (16, False, "plain", False, 1.0),    # the slice's edge
    (17, False, "plain", False, 1.0),    # a second workgroup that holds a single env
    (33, False, "plain", False, 1.0),    # workgroups that finish at different steps
    (33, True, "plain", False, 1.0),
    (33, False, "plain", False, 3.0),    # a racket big enough to be hit: reward 25 + tier
    (33, False, "plain", True, 1.0),     # F_RACKET_GROUND + rolling friction
    (17, False, "edge", False, 1.0),     # both log_std clamps bind, tanh saturates
    (17, True, "edge", False, 1.0),
]
SWING_CASES = [  # n, deterministic, actor, extended contact set
    (1, False, "plain", False), (16, True, "plain", False), (17, False, "plain", False), (48, False, "plain", False), (48, True, "plain", False),
    (17, False, "plain", True), (16, False, "edge", False), (16, True, "edge", False),
]


@pytest.mark.parametrize("n,deterministic,which,extended,scale", TENNIS_CASES)
def test_tennisbot_trace_against_the_actor_kernel_the_reference_and_the_twin(torch, n, deterministic, which, extended, scale):
    ret, length, tr, c, want = case(torch, ENV_TENNIS, n, deterministic, which, extended, scale)
    assert np.all((length >= 1) & (length <= 1001))
    if scale != 1.0:
        assert c["racket_ball_contact_substeps"] > 0, "no racket contact in this case"
        assert np.any(ret >= 25.0), "a racket contact that no return shows"


@pytest.mark.parametrize("n,deterministic,which,extended", SWING_CASES)
def test_swingracket_trace_against_the_actor_kernel_the_reference_and_the_twin(torch, n, deterministic, which, extended):
    ret, length, tr, c, want = case(torch, ENV_SWING, n, deterministic, which, extended)
    assert np.all(length == 26)
    if (n, deterministic, which, extended) == (48, False, "plain", False):
        assert c["racket_ball_contact_substeps"] > 0 and np.any(ret != 0.0), "no ball was struck in this case"


@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
def test_edge_actor_binds_both_clamps_and_saturates_tanh(torch, kind):
    n = 16 if kind == ENV_SWING else 17
    ret, length, tr, c, want = case(torch, kind, n, False, "edge")
    live = live_rows(tr, length)
    assert (want.raw < sr.LOG_STD_MIN).any() and (want.raw > sr.LOG_STD_MAX).any(), "a log_std clamp never binds"
    a = tr["actions"][live]
    assert (a == 1.0).any() and (a == -1.0).any(), "tanh never saturates to +-1 in float32"


def test_noise_is_keyed_by_env_id_not_by_lane_or_workgroup(torch):
    _, l17, t17, _, _ = case(torch, ENV_TENNIS, 17)
    _, l33, t33, _, _ = case(torch, ENV_TENNIS, 33)
    assert np.array_equal(l17, l33[:17])
    T = int(l17.max())
    assert same_bits(t17["eps"][:T], t33["eps"][:T, :17]) and same_bits(t17["actions"][:T], t33["actions"][:T, :17])
    first = t33["eps"][0]
    assert len({first[i].tobytes() for i in range(33)}) == 33, "two envs drew the same noise at step 0"
    assert not same_bits(t33["eps"][0], t33["eps"][1])
    # two fresh handles: identical results
    act, params = actor(torch, ENV_TENNIS, "plain"), case_params()
    env = make_env(ENV_TENNIS, 33, params, False)
    r, ln, tr = run(torch, env, act.flat)
    env.close()
    ret, length, t0, _, _ = case(torch, ENV_TENNIS, 33)
    assert same_bits(r, ret) and np.array_equal(ln, length) and same_trace(tr, t0)


def test_both_loop_exits_are_taken(torch):
    """across the Tennisbot cases some env ends before step 1001 (the workgroup leaves by s_go, or idles the lane) and some env
    reaches the cap (the loop ends at T_MAX)"""
    lengths = np.concatenate([case(torch, ENV_TENNIS, *c)[1] for c in TENNIS_CASES])
    print("Tennisbot lengths over all cases: min %d, max %d, %d of %d at the cap" % (lengths.min(), lengths.max(), int((lengths == 1001).sum()), len(lengths)))
    assert (lengths < 1001).any(), "no episode ended before the cap"
    assert (lengths == 1001).any(), "no episode reached the cap"
    # a workgroup that left by s_go before the cap: every env of the N = 1 .. 16 cases' single workgroup, if all are short
    per_wg = [case(torch, ENV_TENNIS, *c)[1] for c in TENNIS_CASES]
    assert any(ln[g:g + 16].max() < 1001 for ln in per_wg for g in range(0, len(ln), 16)), "no workgroup left the loop by s_go"


@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
def test_call_k_is_episode_k_and_the_handle_is_left_freshly_reset(torch, kind):
    n, swing = 17, kind == ENV_SWING
    act, params = actor(torch, kind, "plain"), case_params()
    a, plain = make_env(kind, n, params, swing), make_env(kind, n, params, swing)
    r0, l0, t0 = run(torch, a, act.flat)
    want = case(torch, kind, n)
    assert same_bits(r0, want[0]) and np.array_equal(l0, want[1])
    r1, l1, t1 = run(torch, a, act.flat)
    assert not same_bits(r0, r1), "two calls on one handle returned the same episodes"
    # call 1 is episode 1: the twin stepped through it
    check_env(torch, kind, n, params, t1, r1, l1, "call 1", episode=1)
    # after call 1 the handle holds what a plain reset leaves at episode 1
    plain.reset()
    plain.reset()
    wa, da = a.get_state_words()
    wp, dp = plain.get_state_words()
    assert torch.equal(wa, wp) and torch.equal(da, dp)
    assert int(wa[-1].min()) == 1 and int(wa[-1].max()) == 1       # (the episode word)
    assert a.phase() == 0
    r2, l2, t2 = run(torch, a, act.flat)
    check_env(torch, kind, n, params, t2, r2, l2, "call 2", episode=2)
    a.close(); plain.close()


def raw_call(torch, env, flat, T, deterministic=0, struct_size=None, guard=64, fill=0x5A):
    """tb_sac_evaluate with caller-owned trace arrays of exactly [T][n][.] elements, `guard` sentinel bytes-elements behind each"""
    from tennisbot_rl_amd.stepper import TbSacEvalTrace
    n, O, A = env.num_envs, env.obs_dim, env.act_dim
    ret = torch.zeros(n, dtype=torch.float64, device=DEV)
    length = torch.zeros(n, dtype=torch.int32, device=DEV)
    sizes = {"obs": T * n * O, "eps": T * n * A, "actions": T * n * A, "reward": T * n, "done": T * n}
    bufs = {k: torch.full((4 * (m + guard) if k != "done" else m + guard,), fill, dtype=torch.uint8, device=DEV) for k, m in sizes.items()}
    tr = TbSacEvalTrace(ctypes.sizeof(TbSacEvalTrace) if struct_size is None else struct_size, T, *(bufs[k].data_ptr() for k in ("obs", "eps", "actions", "reward", "done")))
    rc = env.L.tb_sac_evaluate(env._h, flat.data_ptr(), ret.data_ptr(), length.data_ptr(), NOISE_SEED, deterministic, ctypes.byref(tr), env._stream())
    torch.cuda.synchronize()
    body = {k: host(bufs[k][:(4 if k != "done" else 1) * m]) for k, m in sizes.items()}
    tail = {k: host(bufs[k][(4 if k != "done" else 1) * m:]) for k, m in sizes.items()}
    return rc, host(ret), host(length), body, tail


@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
def test_trace_changes_no_result_and_stays_inside_its_arrays(torch, kind):
    n, swing = 33 if kind == ENV_TENNIS else 17, kind == ENV_SWING
    act, params = actor(torch, kind, "plain"), case_params()
    ret, length, tr, _, _ = case(torch, kind, n)
    short = 7
    assert short < length.max()
    env = make_env(kind, n, params, swing)
    r, ln = run(torch, env, act.flat, trace=False)
    env.close()
    assert same_bits(r, ret) and np.array_equal(ln, length), "the results without the trace differ"
    env = make_env(kind, n, params, swing)
    r, ln, ts = run(torch, env, act.flat, max_steps=short)
    env.close()
    assert same_bits(r, ret) and np.array_equal(ln, length), "the results with a short trace differ"
    assert same_trace(ts, tr, slice(0, short)), "the short trace is not the long one's first rows"
    for T in (short, T_MAX[kind]):
        env = make_env(kind, n, params, swing)
        rc, r, ln, body, tail = raw_call(torch, env, act.flat, T)
        env.close()
        assert rc == 0 and same_bits(r, ret) and np.array_equal(ln, length)
        for k in tail:
            assert (tail[k] == 0x5A).all(), "T = %d: the words behind %s were written" % (T, k)
        live = live_rows({"reward": np.zeros((T, n))}, length)
        got = body["reward"].view(np.float32).reshape(T, n)
        assert same_bits(got[live], tr["reward"][:T][live])
        assert (body["reward"].reshape(T, n, 4)[~live] == 0x5A).all(), "T = %d: reward rows after an env's last step were written" % T


def test_refusals_on_a_real_handle_launch_nothing(torch):
    from tennisbot_rl_amd.stepper import StepperError
    act = actor(torch, ENV_SWING, "plain")
    ret = torch.zeros(16, dtype=torch.float64, device=DEV)
    length = torch.zeros(16, dtype=torch.int32, device=DEV)
    # SwingRacket without the pipeline: TB_E_UNSUPPORTED
    plain = make_env(ENV_SWING, 16, case_params(), False)
    plain.reset()
    w0, d0 = plain.get_state_words()
    c0 = plain.counters()
    with pytest.raises(StepperError, match="tb_set_pipeline"):
        plain.sac_evaluate(act.flat)
    rc = plain.L.tb_sac_evaluate(plain._h, act.flat.data_ptr(), ret.data_ptr(), length.data_ptr(), 1, 0, None, None)
    assert rc == -4 and b"tb_sac_evaluate" in plain.L.tb_last_error()
    w1, d1 = plain.get_state_words()
    assert torch.equal(w0, w1) and torch.equal(d0, d1) and plain.counters() == c0
    # null arguments and a trace of another size: TB_E_INVAL, on a handle that could otherwise evaluate
    piped = make_env(ENV_SWING, 16, case_params(), True)
    piped.reset()
    w0, d0 = piped.get_state_words()
    c0 = piped.counters()
    f, r, ln = act.flat.data_ptr(), ret.data_ptr(), length.data_ptr()
    for args in ((None, r, ln), (f, None, ln), (f, r, None)):
        assert piped.L.tb_sac_evaluate(piped._h, *args, 1, 0, None, None) == -1
        assert b"tb_sac_evaluate" in piped.L.tb_last_error()
    rc, r2, l2, body, tail = raw_call(torch, piped, act.flat, 26, struct_size=8)
    assert rc == -1 and b"struct_size" in piped.L.tb_last_error()
    assert all((body[k] == 0x5A).all() for k in body) and not r2.any() and not l2.any()
    with pytest.raises(ValueError):
        piped.sac_evaluate(act.flat[:-1])
    w1, d1 = piped.get_state_words()
    assert torch.equal(w0, w1) and torch.equal(d0, d1) and piped.phase() == 0 and piped.counters() == c0
    torch.cuda.synchronize()
    assert float(ret.abs().sum()) == 0.0 and int(length.abs().sum()) == 0   # nothing was written
    # ... and the handle still evaluates
    out = piped.sac_evaluate(act.flat, seed=NOISE_SEED)
    assert bool((out[1] == 26).all())
    plain.close(); piped.close()


def test_actor_evaluator_statistics(torch):
    """ActorEvaluator: ceil(n_episodes / n_envs) calls, the surplus dropped, float64 statistics of exactly those episodes"""
    from tennisbot_rl_amd.evaluation import ActorEvaluator
    act = actor(torch, ENV_SWING, "plain")
    ev, twin = (ActorEvaluator(ENV_SWING, n_envs=16, seed=4, device=DEV) for _ in range(2))
    state = torch.cuda.get_rng_state(DEV).clone()
    out = ev.evaluate(act.flat, 40)
    r, ln = twin.episodes(act.flat, 40)
    assert torch.equal(torch.cuda.get_rng_state(DEV), state), "the evaluation drew from torch's RNG"
    r = host(r)
    assert r.shape == (40,) and out["episodes"] == 40 and out["mean_length"] == 26.0
    assert out["mean"] == pytest.approx(r.mean(), rel=1e-12) and out["std"] == pytest.approx(r.std(), rel=1e-12)
    assert out["min"] == r.min() and out["max"] == r.max()
    assert ev.env.env_id_base != 0 and ev.env.pipeline and ev.env.phase() == 0
    ev.close(); twin.close()


def trainer_state(torch, tr):
    """everything a fused evaluation must not move: the nets, the optimisers' moments, log_ent_coef, the env words, obs"""
    tr._learner.publish()
    out = {}
    for name, m in (("actor", tr.actor), ("critic", tr.critic), ("target", tr.critic_target)):
        out.update({"%s.%s" % (name, k): v for k, v in m.state_dict().items()})
    for f, name in ((tr._learner.pi, "pi"), (tr._learner.q, "q"), (tr._learner.ent, "ent")):
        out["%s.exp_avg" % name], out["%s.exp_avg_sq" % name] = f.exp_avg, f.exp_avg_sq
    out["log_ent_coef"] = tr.log_ent_coef.detach()
    out["env_words"], out["env_done"] = tr.env.get_state_words()
    out["obs"] = tr.obs
    return {k: v.detach().clone() for k, v in out.items()}


@pytest.mark.parametrize("algo,env_id", [("sac", "Tennisbot-v0"), ("tqc", "SwingRacket-v0")])
def test_fused_evaluation_and_saves_leave_training_bit_identical(torch, tmp_path, algo, env_id):
    """five vector steps with a fused evaluation and a best-model save after each, against the same run without"""
    if algo == "sac":
        from tennisbot_rl_amd.sac import SACTrainer as Trainer
    else:
        from tennisbot_rl_amd.tqc import TQCTrainer as Trainer
    mk = lambda **kw: Trainer(env_id, num_envs=16, batch_size=32, gradient_steps=2, buffer_size=4096, learning_starts=16, seed=3, device=DEV, **kw)  # noqa: E731
    a = mk(eval_form="fused")   # (each trainer is built right before its run: the constructor seeds torch's RNG, which collect and train draw from)
    best = os.path.join(str(tmp_path), "best_model.pt")
    state = None
    for k in range(5):
        a.vector_step()
        state = torch.cuda.get_rng_state(DEV).clone()
        out = a.evaluate_episodes(16, n_envs=16)        # the constructor's form: fused
        assert torch.equal(torch.cuda.get_rng_state(DEV), state), "the evaluation drew from torch's global RNG"
        assert out["episodes"] == 16 and 1.0 <= out["mean_length"] <= 1001.0 and out["min"] <= out["mean"] <= out["max"]
        a.save(best)
    assert a._eval_fused.env.pipeline == (env_id == "SwingRacket-v0") and getattr(a, "_eval_env", None) is None
    b = mk()
    assert b.eval_form == "torch"
    for k in range(5):
        b.vector_step()
    torch.cuda.synchronize()
    assert a._learner.step == b._learner.step and a._learner.step > 0
    sa, sb = trainer_state(torch, a), trainer_state(torch, b)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k].view(torch.uint8), sb[k].view(torch.uint8)), "%s differs between the run with and the run without the fused evaluation" % k
    fresh = mk()
    assert not torch.equal(sa["actor.mu.weight"], fresh.actor.state_dict()["mu.weight"]), "the five vector steps trained nothing"
    # form= per call, deterministic, n_episodes no multiple of n_envs: summarise's keys
    out = a.evaluate_episodes(20, deterministic=True, n_envs=16, form="fused")
    assert set(out) == {"episodes", "mean", "std", "min", "max", "mean_length"} and out["episodes"] == 20
    # the fused form evaluates the CURRENT flat vector: the same numbers from an ActorEvaluator fed the published actor
    from tennisbot_rl_amd.evaluation import ActorEvaluator
    ev = ActorEvaluator(a.kind, 16, seed=a.env.seed + 1000003, params=a.env.params, device=DEV)
    for _ in range(7):   # (the trainer's evaluation handle has run 5 + 2 launches so far: the next one is its episode 7)
        ev.episodes(a._learner.pi.flat, 16)
    flat = torch.cat([p.detach().reshape(-1) for p in a.actor.parameters()])
    assert torch.equal(flat, a._learner.pi.flat)
    again = a.evaluate_episodes(16, deterministic=True, n_envs=16, form="fused")
    assert ev.evaluate(flat, 16, deterministic=True) == again
    ev.close()
    with pytest.raises(ValueError, match="form"):
        a.evaluate_episodes(4, form="eager")
    b.load(best)                                                    # ... and the best model loads, and evaluates fused
    assert b.evaluate_episodes(5, n_envs=16, form="fused")["episodes"] == 5
