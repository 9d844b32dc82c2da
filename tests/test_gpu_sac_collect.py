"""SAC / TQC transitions collected in one launch, straight into the replay ring (tb_sac_collect, tb_sac_collect_kernel in
csrc/tb_sac.hpp) on a real MI355X. Every comparison covers every row of every call, none left out:

  1. the actor: the obs / eps rows through the EXISTING tb_sac_actor_forward give the action rows bit for bit, and the actions are
     within ppo_reference.MULTIPLE float32-twin errors of sac_reference.actor_forward in float64;
  2. the noise keys: eps against policy_reference.policy_noise with the keys that follow the done rows; env i's rows at N = 17 and 33;
  3. the env twin: a second handle (same seed, id base, parameters, pipeline setting), reset once and stepped by BatchedEnv.step with
     the collected actions, gives next_obs, reward and done bit for bit, obs[0] is the reset's, obs[t + 1] == next_obs[t] across call
     boundaries, and after the last call the two handles hold the same state words and done bytes;
  4. uniform mode against its numpy restatement, 5. refusals behind guard words, 6. eps_or_null changes nothing,
  7. the trainers' ring against a torch-form ReplayBuffer.add of the twin's transitions, 8. the trainers' loop, change-over and
     save / load.

The actors, seeds and parameter sets are test_gpu_sac_evaluate.py's: with its noise seed the first episode of every env is the one
that file traces (racket contacts at scale 3, struck balls on SwingRacket, both episode endings)."""
import ctypes

import numpy as np
import pytest

import policy_reference as pr
import sac_collect_reference as cr
import test_gpu_sac_evaluate as ev
from helpers import same_bits
from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, OBS_DIM

pytestmark = pytest.mark.gpu

DEV, NOISE_SEED, ID_BASE = ev.DEV, ev.NOISE_SEED, ev.ID_BASE
assert ID_BASE == 1 << 33
ROWS = ("obs", "next_obs", "action", "reward", "done", "eps")
# Tennisbot: 1100 steps as calls of 1, 7, 64 and the remainder, the remainder cut once more so that a call ends with step 1001, where
# an episode that reaches the step limit ends (the launches' last steps: 1, 8, 72, 1001, 1100)
TENNIS_SPLIT = (1, 7, 64, 929, 99)
SWING_SPLITS = ((26, 26), (13, 13, 13, 13), (25, 1, 25, 1), (1,) * 52)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def host(x):
    return x.detach().cpu().numpy().copy()


def collect(torch, env, flat, splits, uniform=False, with_eps=True, seed=NOISE_SEED):
    """one sac_collect call per entry of splits (an entry may be (S, uniform)); the rows of all calls [T, n, .] on the host"""
    n, O, A = env.num_envs, env.obs_dim, env.act_dim
    parts = []
    for s in splits:
        S, uni = (s, uniform) if isinstance(s, int) else s
        f = dict(dtype=torch.float32, device=DEV)
        out = [torch.full((S, n, O), np.nan, **f), torch.full((S, n, O), np.nan, **f), torch.full((S, n, A), np.nan, **f), torch.full((S, n), np.nan, **f),
               torch.full((S, n), np.nan, **f)]
        eps = torch.full((S, n, A), np.nan, **f) if with_eps else None
        env.sac_collect(None if uni else flat, S, tuple(out), seed=seed, uniform=uni, eps=eps)
        parts.append(out + ([eps] if with_eps else []))
    torch.cuda.synchronize()
    return {k: np.concatenate([host(p[j]) for p in parts]) for j, k in enumerate(ROWS[:6 if with_eps else 5])}


_TWINS = {}


def twin_run(torch, kind, n, params, pipeline, actions, key):
    """the twin's (obs0, obs, reward, done, state words, done bytes, counters) for these actions: computed once per key and reused
    while the actions are the same bits"""
    hit = _TWINS.get(key)
    if hit is not None and hit[0].shape == actions.shape and same_bits(hit[0], actions):
        return hit[1]
    twin = ev.make_env(kind, n, params, pipeline)
    obs0 = host(twin.reset())
    a_dev = torch.from_numpy(np.ascontiguousarray(actions)).to(DEV)
    o, r, d = [], [], []
    for t in range(len(actions)):
        ot, rt, dt = twin.step(a_dev[t].clone())   # (a row of its own: step() wants 16-byte aligned rows)
        o.append(ot); r.append(rt); d.append(dt)
    if pipeline:
        twin.flush()
    torch.cuda.synchronize()
    w, db = twin.get_state_words()
    res = (obs0, host(torch.stack(o)), host(torch.stack(r)), host(torch.stack(d)), host(w), host(db), twin.counters(), twin.phase())
    twin.close()
    _TWINS[key] = (actions.copy(), res)
    return res


def check_twin(torch, env, kind, n, params, pipeline, rec, key, name):
    """3. of the module docstring, every row; returns the twin's counters"""
    T = len(rec["action"])
    assert not any(np.isnan(rec[k]).any() for k in rec), "%s: a row was not written (or a NaN was computed)" % name
    obs0, obs_r, rew_r, done_r, words, dbytes, c, phase = twin_run(torch, kind, n, params, pipeline, rec["action"], key)
    assert same_bits(obs0, rec["obs"][0]), "%s: obs[0] of the first call is not the reset's observation" % name
    assert same_bits(rec["obs"][1:], rec["next_obs"][:-1]), "%s: obs[t + 1] is not next_obs[t]" % name
    assert same_bits(obs_r, rec["next_obs"]), "%s: next_obs differs from the twin's in %d of %d rows" % (
        name, int((obs_r.view(np.uint32) != rec["next_obs"].view(np.uint32)).any(-1).sum()), T * n)
    assert same_bits(rew_r, rec["reward"]), "%s: rewards differ from the twin's" % name
    assert np.array_equal(done_r.astype(np.float32), rec["done"]) and set(np.unique(rec["done"])) <= {0.0, 1.0}, "%s: done differs from the twin's" % name
    w, d = env.get_state_words()
    assert np.array_equal(host(w), words) and np.array_equal(host(d), dbytes), "%s: the handle is not where the twin's steps left it" % name
    assert env.phase() == phase
    return c


def check_keys(rec, n, A, uniform_rows=None):
    """2.: eps of every actor row against policy_noise at the keys the done rows give; returns the keys"""
    ep, sc, _, _ = pr.episode_keys(np.zeros(n, np.int64), np.zeros(n, np.int64), rec["done"])
    ids = (ID_BASE + np.arange(n, dtype=np.uint64))[None, :]
    want = pr.policy_noise(NOISE_SEED, ids, ep, sc, A)
    actor_rows = np.ones(len(rec["done"]), bool) if uniform_rows is None else ~uniform_rows
    err = np.abs(rec["eps"].astype(np.float64) - want)[actor_rows]
    assert err.size and err.max() <= pr.EPS_TOL, "eps is %.3g from policy_noise at its (seed, id, episode, step) key (allowed %.3g)" % (err.max(), pr.EPS_TOL)
    return ids, ep, sc


def launch_ends(splits):
    return np.cumsum([s if isinstance(s, int) else s[0] for s in splits]) - 1


_CASES = {}


def case(torch, kind, n, which="plain", extended=False, scale=1.0, splits=None):
    key = (kind, n, which, extended, scale, splits)
    if key in _CASES:
        return _CASES[key]
    swing = kind == ENV_SWING
    splits = splits or (SWING_SPLITS[0] if swing else TENNIS_SPLIT)
    name = "%s n=%d actor=%s ext=%s scale=%g calls=%s" % ("SwingRacket" if swing else "Tennisbot", n, which, extended, scale, splits if len(splits) < 8 else "%d x %d" % (len(splits), splits[0]))
    act, params = ev.actor(torch, kind, which), ev.case_params(extended, scale)
    env = ev.make_env(kind, n, params, swing)
    env.reset()
    rec = collect(torch, env, act.flat, splits)
    T = len(rec["action"])
    assert T == sum(splits) and rec["obs"].shape == (T, n, OBS_DIM[kind]) and rec["action"].shape == (T, n, ACT_DIM[kind])
    c = env.counters()
    ct = check_twin(torch, env, kind, n, params, swing, rec, (kind, n, which, extended, scale), name)
    env.close()
    assert c == ct, "%s: the counters differ from the twin's: %s / %s" % (name, c, ct)
    assert c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0 and c["substeps"] >= T * n
    # 1. the actor: test_gpu_sac_evaluate's check on every row (a "trace" whose every row is live)
    length = np.full(n, T, np.int32)
    ratio, _ = ev.check_actor(torch, act, kind, {"obs": rec["obs"], "eps": rec["eps"], "actions": rec["action"], "reward": rec["reward"]}, length, False, name)
    check_keys(rec, n, ACT_DIM[kind])
    ends = launch_ends(splits)
    done_t = np.nonzero(rec["done"].any(1))[0]
    print("%s: %d episodes finished at steps %s ..., launches end at %s, actions %.3g twin errors from float64, racket contacts %d"
          % (name, int(rec["done"].sum()), done_t[:12].tolist(), ends.tolist()[:8], ratio, c["racket_ball_contact_substeps"]))
    assert c["episodes_finished"] == int(rec["done"].sum())
    _CASES[key] = (rec, c, ends)
    return _CASES[key]


TENNIS_CASES = [  # n, actor, extended contact set, racket scale
    (1, "plain", False, 1.0), (15, "plain", False, 1.0), (16, "plain", False, 1.0), (17, "plain", False, 1.0), (33, "plain", False, 1.0),
    (33, "plain", False, 3.0), (33, "plain", True, 1.0), (17, "edge", False, 1.0),
]
SWING_CASES = [(n, "plain", False, s) for n in (1, 16, 17, 48) for s in SWING_SPLITS] + [(17, "plain", True, s) for s in SWING_SPLITS] + [(16, "edge", False, SWING_SPLITS[1])]


@pytest.mark.parametrize("n,which,extended,scale", TENNIS_CASES)
def test_tennisbot_rows_against_the_actor_kernel_the_reference_and_the_twin(torch, n, which, extended, scale):
    rec, c, ends = case(torch, ENV_TENNIS, n, which, extended, scale)
    assert len(rec["done"]) == 1100
    if scale != 1.0:
        assert c["racket_ball_contact_substeps"] > 0, "the twin's counters show no racket contact in this case"
        assert (rec["reward"] >= 25.0).any(), "a racket contact that no reward shows"


def test_tennisbot_episodes_end_inside_launches_and_on_their_last_steps(torch):
    inside = last = 0
    for cs in TENNIS_CASES:
        rec, c, ends = case(torch, ENV_TENNIS, *cs)
        at_end = np.zeros(len(rec["done"]), bool)
        at_end[ends] = True
        last += int(rec["done"][at_end].sum())
        inside += int(rec["done"][~at_end].sum())
    print("Tennisbot: %d episodes finished inside a launch, %d on a launch's last step" % (inside, last))
    assert inside > 0, "no env finished inside a launch: the in-loop restart never ran"
    assert last > 0, "no env finished on a launch's last step: a restarted state was never written back"


@pytest.mark.parametrize("n,which,extended,splits", SWING_CASES)
def test_swingracket_rows_against_the_actor_kernel_the_reference_and_the_twin(torch, n, which, extended, splits):
    rec, c, ends = case(torch, ENV_SWING, n, which, extended, splits=splits)
    T = sum(splits)
    done = np.zeros((T, n), np.float32)
    done[25::26] = 1.0
    assert np.array_equal(rec["done"], done), "SwingRacket episodes are 26 steps"
    assert c["episodes_finished"] == n * (T // 26)
    if n == 48 and which == "plain" and not extended:
        assert c["racket_ball_contact_substeps"] > 0 and (rec["reward"][25::26] != 0.0).any(), "no terminal reward row is nonzero in this case"
    # the same rows however the calls cut the episodes
    base = case(torch, ENV_SWING, n, which, extended, splits=SWING_SPLITS[0] if which == "plain" else splits)[0]
    assert all(same_bits(rec[k], base[k]) for k in ROWS)


def test_env_rows_do_not_depend_on_the_batch_size(torch):
    r17, r33 = case(torch, ENV_TENNIS, 17)[0], case(torch, ENV_TENNIS, 33)[0]
    assert all(same_bits(r17[k], r33[k][:, :17]) for k in ROWS), "env i's rows differ between N = 17 and N = 33"
    first = r33["eps"][0]
    assert len({first[i].tobytes() for i in range(33)}) == 33, "two envs drew the same noise at step 0"
    s17, s48 = case(torch, ENV_SWING, 17, splits=SWING_SPLITS[0])[0], case(torch, ENV_SWING, 48, splits=SWING_SPLITS[0])[0]
    assert all(same_bits(s17[k], s48[k][:, :17]) for k in ROWS)


@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
def test_uniform_mode_is_its_numpy_restatement_and_the_actor_takes_over_the_same_episodes(torch, kind):
    n, swing, A = 17, kind == ENV_SWING, ACT_DIM[kind]
    act, params = ev.actor(torch, kind, "plain"), ev.case_params(scale=1.0 if swing else 3.0)
    splits = ((13, True), (13, True), (20, False), (6, False)) if swing else ((3, True), (40, True), (30, False), (400, False))
    uni = np.concatenate([np.full(s, u) for s, u in splits])
    env = ev.make_env(kind, n, params, swing)
    env.reset()
    rec = collect(torch, env, act.flat, splits)          # (uniform calls pass actor_dev = NULL)
    name = "uniform %s" % ("SwingRacket" if swing else "Tennisbot")
    check_twin(torch, env, kind, n, params, swing, rec, ("uniform", kind), name)
    env.close()
    ids, ep, sc = check_keys(rec, n, A, uniform_rows=uni)   # the actor rows' eps: the keys go on from where the uniform calls left them
    want = cr.uniform_actions(NOISE_SEED, ids, ep, sc, A)
    assert uni.sum() > 0 and same_bits(rec["action"][uni], want[uni]), "uniform actions are not the numpy restatement's"
    assert not rec["eps"][uni].any(), "a uniform row reported noise"
    a = rec["action"][uni]
    assert a.min() >= -1.0 and a.max() < 1.0 and a.min() < -0.9 and a.max() > 0.9
    assert not same_bits(rec["action"][~uni], want[~uni])
    # the actor rows are the actor's: the existing kernel on their obs / eps, bit for bit
    sub = {"obs": rec["obs"][~uni], "eps": rec["eps"][~uni], "actions": rec["action"][~uni], "reward": rec["reward"][~uni]}
    ev.check_actor(torch, act, kind, sub, np.full(n, int((~uni).sum()), np.int32), False, name)
    if not swing:
        assert rec["done"][uni].any() or rec["done"][~uni].any(), "no episode ended in this case"


def raw_collect(torch, env, actor_ptr, S, mode=0, struct_size=None, null=None, with_eps=True, guard=64, fill=0x5A):
    """tb_sac_collect with caller-owned arrays of exactly [S][n][.] floats, `guard` sentinel floats behind each"""
    from tennisbot_rl_amd.stepper import TbSacCollectOut
    n, O, A = env.num_envs, env.obs_dim, env.act_dim
    S_alloc = max(S, 1)
    sizes = {"obs": S_alloc * n * O, "next_obs": S_alloc * n * O, "action": S_alloc * n * A, "reward": S_alloc * n, "done": S_alloc * n, "eps": S_alloc * n * A}
    bufs = {k: torch.full((4 * (m + guard),), fill, dtype=torch.uint8, device=DEV) for k, m in sizes.items()}
    ptr = lambda k: None if k == null or (k == "eps" and not with_eps) else bufs[k].data_ptr()  # noqa: E731
    out = TbSacCollectOut(ctypes.sizeof(TbSacCollectOut) if struct_size is None else struct_size, *(ptr(k) for k in ROWS))
    rc = env.L.tb_sac_collect(env._h, actor_ptr, S, mode, NOISE_SEED, ctypes.byref(out), env._stream())
    err = env.L.tb_last_error()
    torch.cuda.synchronize()
    body = {k: host(bufs[k][:4 * m]) for k, m in sizes.items()}
    tail = {k: host(bufs[k][4 * m:]) for k, m in sizes.items()}
    return rc, err, body, tail


def test_refusals_launch_nothing(torch):
    act_s, act_t = ev.actor(torch, ENV_SWING, "plain"), ev.actor(torch, ENV_TENNIS, "plain")
    plain = ev.make_env(ENV_SWING, 16, ev.case_params(), False)
    piped = ev.make_env(ENV_SWING, 16, ev.case_params(), True)
    tennis = ev.make_env(ENV_TENNIS, 17, ev.case_params(), False)
    f_s, f_t = act_s.flat.data_ptr(), act_t.flat.data_ptr()
    refusals = [  # env, what, the call's keywords, the code, a word of the message
        (plain, "SwingRacket without the pipeline", dict(actor_ptr=f_s, S=3), -4, b"tb_set_pipeline"),
        (piped, "phase + n_steps > 26", dict(actor_ptr=f_s, S=27), -1, b"phase + n_steps"),
        (piped, "n_steps < 1", dict(actor_ptr=f_s, S=0), -1, b"n_steps"),
        (tennis, "n_steps < 1", dict(actor_ptr=f_t, S=-3), -1, b"n_steps"),
        (tennis, "a wrong struct_size", dict(actor_ptr=f_t, S=2, struct_size=48), -1, b"struct_size"),
        (tennis, "a null actor in actor mode", dict(actor_ptr=None, S=2), -1, b"actor_dev"),
        (tennis, "an unknown mode", dict(actor_ptr=f_t, S=2, mode=2), -1, b"mode"),
    ] + [(tennis, "a null %s" % k, dict(actor_ptr=f_t, S=2, null=k), -1, b"null") for k in ROWS[:5]] + [
        (piped, "a null reward", dict(actor_ptr=f_s, S=2, null="reward"), -1, b"null")]
    for env in (plain, piped, tennis):
        env.reset()
    # phase 20 + 7 > 26 too: a handle in mid-episode
    rec = collect(torch, piped, act_s.flat, (20,))
    assert piped.phase() == 20
    refusals.append((piped, "phase 20 + 7 steps", dict(actor_ptr=f_s, S=7), -1, b"phase + n_steps"))
    state = {id(e): (e.get_state_words(), e.counters(), e.phase()) for e in (plain, piped, tennis)}
    for env, what, kw, code, word in refusals:
        rc, err, body, tail = raw_collect(torch, env, **kw)
        assert rc == code and b"tb_sac_collect" in err and word in err, "%s: rc %d, %r" % (what, rc, err)
        assert all((body[k] == 0x5A).all() and (tail[k] == 0x5A).all() for k in body), "%s: an output was written" % what
        (w0, d0), c0, p0 = state[id(env)]
        w1, d1 = env.get_state_words()
        assert torch.equal(w0, w1) and torch.equal(d0, d1) and env.counters() == c0 and env.phase() == p0, "%s: the handle moved" % what
    # ... and the handles still collect: the six steps that end the episodes, the terminal reward in place without a flush
    rc, err, body, tail = raw_collect(torch, piped, f_s, 6)
    assert rc == 0 and piped.phase() == 0 and all((tail[k] == 0x5A).all() for k in tail)
    done = body["done"].view(np.float32).reshape(6, 16)
    assert not done[:5].any() and (done[5] == 1.0).all()
    rc, err, body, tail = raw_collect(torch, tennis, None, 5, mode=1)
    assert rc == 0 and all((tail[k] == 0x5A).all() for k in tail) and not (body["obs"] == 0x5A).all()
    from tennisbot_rl_amd.stepper import StepperError
    with pytest.raises(StepperError, match="tb_set_pipeline"):
        collect(torch, plain, act_s.flat, (1,))
    with pytest.raises(ValueError):
        tennis.sac_collect(act_t.flat[:-1], 1, tuple(torch.zeros(s, device=DEV) for s in ((1, 17, 12), (1, 17, 12), (1, 17, 2), (1, 17), (1, 17))))
    with pytest.raises(ValueError):
        tennis.sac_collect(act_t.flat, 2, tuple(torch.zeros(s, device=DEV) for s in ((1, 17, 12), (1, 17, 12), (1, 17, 2), (1, 17), (1, 17))))
    for env in (plain, piped, tennis):
        env.close()


@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
def test_eps_or_null_changes_no_result_and_every_array_stays_inside_its_rows(torch, kind):
    n, swing = 17, kind == ENV_SWING
    act, params = ev.actor(torch, kind, "plain"), ev.case_params()
    S = 26 if swing else 90
    got = []
    for with_eps in (True, False):
        env = ev.make_env(kind, n, params, swing)
        env.reset()
        rc, err, body, tail = raw_collect(torch, env, act.flat.data_ptr(), S, with_eps=with_eps)
        assert rc == 0, err
        assert all((tail[k] == 0x5A).all() for k in tail), "the words behind an array were written"
        if not with_eps:
            assert (body["eps"] == 0x5A).all()
        w, d = env.get_state_words()
        got.append((body, host(w), host(d), env.counters()))
        env.close()
    (b0, w0, d0, c0), (b1, w1, d1, c1) = got
    assert all(np.array_equal(b0[k], b1[k]) for k in ROWS[:5]) and np.array_equal(w0, w1) and np.array_equal(d0, d1) and c0 == c1
    # ... and they are the rows of the case above (Tennisbot: its first 90 steps; SwingRacket: its first episode)
    base = case(torch, kind, n, splits=SWING_SPLITS[0] if swing else None)[0]
    for k in ROWS:
        assert same_bits(b0[k].view(np.float32).reshape(base[k][:S].shape), base[k][:S]), k


# ------------------------------------------------------------------------------------------------------------------- the trainers
def trainer_class(algo):
    if algo == "sac":
        from tennisbot_rl_amd.sac import SACTrainer
        return SACTrainer
    from tennisbot_rl_amd.tqc import TQCTrainer
    return TQCTrainer


def spy_on_collect(torch, tr):
    """record every sac_collect launch of the trainer's env: (num_timesteps before it, steps, uniform, copies of its rows)"""
    calls, inner = [], tr.env.sac_collect

    def sac_collect(actor_flat, n_steps, out_views, seed=0, uniform=False, eps=None):
        before = tr.num_timesteps
        inner(actor_flat, n_steps, out_views, seed=seed, uniform=uniform, eps=eps)
        calls.append((before, int(n_steps), bool(uniform), [v.clone() for v in out_views], actor_flat is not None and actor_flat.data_ptr() == tr._learner.pi.flat.data_ptr()))
    tr.env.sac_collect = sac_collect
    return calls


@pytest.mark.parametrize("algo,env_id,collect_steps", [("sac", "Tennisbot-v0", 2), ("tqc", "SwingRacket-v0", 6)])
def test_ring_holds_what_a_torch_form_add_of_the_twins_transitions_holds(torch, capsys, algo, env_id, collect_steps):
    from tennisbot_rl_amd.sac import ReplayBuffer
    from tennisbot_rl_amd.stepper import BatchedEnv
    N, S = 16, collect_steps
    tr = trainer_class(algo)(env_id, num_envs=N, batch_size=32, gradient_steps=1, buffer_size=50, learning_starts=40, seed=5, device=DEV, collect_form="fused", collect_steps=S)
    assert "rounds buffer_size 50 down to 48" in capsys.readouterr().err
    assert tr.replay.capacity == 48 and tr.env.pipeline == (env_id == "SwingRacket-v0")
    calls = spy_on_collect(torch, tr)
    obs0 = tr.obs.clone()
    for k in range(5):   # vector_step's body, with torch's RNG read around the collect
        state = torch.cuda.get_rng_state(DEV).clone()
        cpu_state = torch.get_rng_state().clone()
        tr.collect_fused()
        assert torch.equal(torch.cuda.get_rng_state(DEV), state) and torch.equal(torch.get_rng_state(), cpu_state), "the fused collect drew from torch's global RNG"
        if tr.num_timesteps > tr.learning_starts:
            tr.train(tr.gradient_steps * S)
    torch.cuda.synchronize()
    T = 5 * S
    assert tr.num_timesteps == T * N and sum(c[1] for c in calls) == T and tr._learner.step > 0
    assert all(c[1] * N <= 48 for c in calls) and all(c[4] for c in calls if not c[2]), "an actor launch was not fed the learner's flat vector"
    if env_id == "SwingRacket-v0":
        assert any(float(c[3][4].sum()) > 0 for c in calls), "no launch crossed an episode end"
    # the twin: the trainer's env parameters, stepped with the collected actions; its transitions through add()
    twin = BatchedEnv(tr.kind, N, device=DEV, seed=5, params=tr.env.params, track_terminal_obs=False, pipeline=False)
    ring = ReplayBuffer(tr.env.obs_dim, tr.env.act_dim, 48, DEV)
    obs = twin.reset()
    assert torch.equal(obs, obs0)
    for before, steps, uniform, rows, _ in calls:
        actions = rows[2].view(steps, N, -1)
        for t in range(steps):
            nxt, r, d = twin.step(actions[t].clone())
            ring.add(obs, nxt, actions[t], r, d.float())
            obs = nxt
    torch.cuda.synchronize()
    assert (ring.pos, ring.size) == (tr.replay.pos, tr.replay.size) and ring.size == 48
    for name, x, y in zip(ROWS, ring.arrays(), tr.replay.arrays()):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "the ring's %s rows are not the twin's" % name
    assert torch.equal(tr.obs, obs), "self.obs is not the last next_obs row"
    wa, da = tr.env.get_state_words()
    wb, db = twin.get_state_words()
    assert torch.equal(wa, wb) and torch.equal(da, db)
    twin.close()


def learner_bits(torch, tr):
    out = ev.trainer_state(torch, tr)
    for name, a in zip(ROWS, tr.replay.arrays()):
        out["ring." + name] = a.detach().clone()
    out["ep_return"] = tr._ep_return.detach().clone()
    return out


@pytest.mark.parametrize("algo,env_id", [("sac", "Tennisbot-v0"), ("tqc", "SwingRacket-v0")])
def test_fused_trainer_changes_over_where_the_torch_form_does_and_repeats_after_a_load(torch, tmp_path, algo, env_id):
    N, S, LS = 16, 4, 40   # learning_starts falls inside the first request: 3 uniform steps (timesteps 0, 16, 32), then the actor
    mk = lambda: trainer_class(algo)(env_id, num_envs=N, batch_size=32, gradient_steps=1, buffer_size=4096, learning_starts=LS, seed=7, device=DEV,  # noqa: E731
                                     collect_form="fused", collect_steps=S)
    a = mk()
    calls = spy_on_collect(torch, a)
    for k in range(4):
        a.vector_step()
    assert a.num_timesteps == 4 * S * N and a._learner.step == 4 * S   # gradient_steps per ENV step; the first vector step trains too (64 > 40)
    for before, steps, uniform, rows, _ in calls:
        for t in range(steps):   # the torch form's rule, step by step: uniform while num_timesteps < learning_starts
            assert uniform == (before + t * N < LS), "a launch at timestep %d (+%d steps) is %s" % (before, t, "uniform" if uniform else "the actor's")
    assert [c[1] for c in calls[:2]] == [3, 1] and calls[0][2] and not calls[1][2]
    path = str(tmp_path / "ck.pt")
    a.save(path)
    torch.manual_seed(99)   # (train() draws its indices and noise from torch's global RNG, which a checkpoint does not hold)
    a.vector_step()
    torch.cuda.synchronize()
    want = learner_bits(torch, a)
    b = mk().load(path)
    torch.manual_seed(99)
    b.vector_step()
    torch.cuda.synchronize()
    got = learner_bits(torch, b)
    assert got.keys() == want.keys() and b.num_timesteps == a.num_timesteps and (b.replay.pos, b.replay.size) == (a.replay.pos, a.replay.size)
    for k in want:
        assert torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)), "%s differs after save / load and one more vector step" % k
    fresh = mk()
    assert not torch.equal(want["actor.mu.weight"], fresh.actor.state_dict()["mu.weight"]), "the vector steps trained nothing"


def test_default_collect_form_is_the_torch_form(torch):
    from tennisbot_rl_amd.sac import SACTrainer
    kw = dict(num_envs=16, batch_size=32, gradient_steps=2, buffer_size=4096, learning_starts=16, seed=3, device=DEV)
    runs = []
    for extra in ({}, {"collect_form": "torch"}):
        tr = SACTrainer("Tennisbot-v0", **kw, **extra)   # (built right before its run: the constructor seeds torch's RNG)
        assert tr.collect_form == "torch" and tr.collect_steps == 1 and not tr.env.pipeline and tr.replay.capacity == 4096
        for _ in range(3):
            tr.vector_step()
        torch.cuda.synchronize()
        runs.append(learner_bits(torch, tr))
    for k in runs[0]:
        assert torch.equal(runs[0][k].view(torch.uint8), runs[1][k].view(torch.uint8)), k
