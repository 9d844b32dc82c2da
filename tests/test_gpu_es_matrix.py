"""The fused ES evaluation (tb_es_evaluate, csrc/tb_es.hpp) across the engine-parameter space, the fast-forward forms, batch sizes,
weight layouts and handle states that the other kernel families are pinned across. Every evaluation is held to the strict trace
check of test_gpu_es.py (helpers.check_es_trace): oracle reset, bit-exact replay through BatchedEnv.step, bit-exact normaliser,
the network within twice its float64 forward bound, bit-exact float64 returns. On top of it:
  * the nine counters of an evaluation equal what the float32 oracle books for exactly those episodes;
  * every case names the path it claims: pipeline_form(), the staging path of each wave, racket-ball contacts that ran;
  * returns do not depend on the fast-forward form, the weights' row stride or their staging;
  * a truncated trace is the prefix of the full one and changes no result;
  * an evaluation on a handle that was stepped (pending pool stragglers, mid-episode Tennisbot) evaluates each env's next episode
    and leaves the env where the oracle's reset of that episode is, for eager steps and for graphs captured before it."""
import numpy as np
import pytest

from helpers import (check_es_trace, draw_engine_params, es_env, es_evaluate, es_member_weights, es_oracle_counters, es_params,
                     es_population, es_run, same_bits)
from outlines import with_outline
from tennisbot_rl_amd.params import COUNTER_NAMES, ENV_SWING, ENV_TENNIS, F_AUTO_RESET, reference_rolling_friction

pytestmark = pytest.mark.gpu

LDS_MEMBERS = 8  # csrc/tb_es.hpp TB_ES_LDS_MEMBERS


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def wave_members(n, epm):
    """members spanned by each 64-env wave of tb_es_rollout_kernel (a wave stages its rows in LDS iff it spans <= LDS_MEMBERS)"""
    first = np.arange(0, n, 64)
    last = np.minimum(first + 63, n - 1)
    return last // epm - first // epm + 1


def sample_members(M, k=16):
    """a fixed sample of at least k members, the first and the last among them"""
    return sorted(set(np.linspace(0, M - 1, k).astype(int).tolist()) | {0, M - 1})


def evaluate_counted(torch, env, epm, W, stride=None):
    env.counters_reset()
    ret, length, tr = es_run(torch, env, epm, es_population(torch, W, stride))
    return ret, length, tr, env.counters()


# ------------------------------------------------------------------ 1. engine parameters, outlines, racket scales
def matrix_params(kind, case):
    """(params, racket scale to set through set_racket_scale after creation or None). Tennisbot's rackets are scaled up where the case
    does not scale them itself (a curriculum-sized racket is hit by many more balls), and its random draws are ones under which the
    balls reach the racket at all (many draws -- heavy balls, strong gravity -- drop every ball short of it): every case reaches the
    contact solver"""
    big = 3.0 if kind == ENV_TENNIS else 1.0
    if case.startswith("random"):
        k = int(case[-1])
        rng = np.random.default_rng((400, 101)[k] if kind == ENV_TENNIS else 4321 + k)
        over = draw_engine_params(rng, rolling=k == 1)
        if k == 0:  # the Magnus and spin extensions on (quadratic damping is drawn non-zero)
            over.update(magnus_k=float(rng.choice([1e-4, 5e-4])), ball_spin_max=float(rng.choice([50.0, 200.0])))
            assert over["lin_damp_quad"] > 0 and over["ang_damp_quad"] > 0
        return es_params(racket_scale=big, **over), None
    if case == "full-contact":
        return es_params(rg=True, racket_scale=big, **reference_rolling_friction()), None
    if case.startswith("outline"):  # (SwingRacket: an outline inside the ball's radius, so that the ball resting at the face's
        e = int(case[len("outline"):])  # centre touches its rim and the edges decide the strike)
        p = with_outline(es_params(), e) if kind == ENV_TENNIS else with_outline(es_params(), e, radius_y=0.02, radius_z=0.03)
        p.racket_scale = big
        return p, None
    if case == "scale-params":
        return es_params(racket_scale=2.3), None
    if case == "scale-set":
        return es_params(), 3.0
    raise ValueError(case)


MATRIX = ([(ENV_SWING, c) for c in ("random0", "random1", "full-contact", "outline3", "outline4", "outline63", "outline64")]
          + [(ENV_TENNIS, c) for c in ("random0", "random1", "full-contact", "outline3", "outline4", "outline63", "outline64",
                                       "scale-params", "scale-set")])


@pytest.mark.parametrize("kind,case", MATRIX)
def test_engine_parameter_matrix(torch, kind, case):
    params, set_scale = matrix_params(kind, case)
    n, epm = (1000, 10) if kind == ENV_TENNIS and case.startswith("random") else (200, 10)  # (contacts are rare under those draws)
    W = es_member_weights(kind, "golden" if kind == ENV_SWING else "default", n // epm)
    env = es_env(kind, n, params)
    if set_scale is not None:
        env.set_racket_scale(set_scale)
    ret, length, tr, c = evaluate_counted(torch, env, epm, W)
    used = env.params.copy()  # (set_racket_scale updates it: what the evaluation's resets built their rackets with)
    env.close()
    check_es_trace(torch, kind, n, epm, W, ret, length, tr, used, members=sample_members(n // epm, 20))
    assert c["lockstep_violations"] == 0 and c["episodes_finished"] == n, c
    print(kind, case, c)
    if case.startswith("outline"):  # the outline changed the episodes: the evaluation did not step the product's
        base = es_params(racket_scale=params.racket_scale, rg=False)
        assert not same_bits(ret, es_evaluate(torch, kind, n, epm, W, base, trace=False)[0])
    if kind == ENV_TENNIS:
        assert c["racket_ball_contact_substeps"] > 0, c  # the contact solver ran inside the evaluation


# ------------------------------------------------------------------ 2. counters
COUNTER_CASES = [
    # kind, n, envs per member, weights, racket-ground, options
    (ENV_SWING, 200, 10, "golden", False, dict(ff_defer="all")),
    (ENV_SWING, 200, 10, "golden", False, dict(ff_defer="all", ff_seal=False)),
    (ENV_SWING, 200, 10, "saturating", False, dict(ff_defer="all")),
    (ENV_SWING, 100, 10, "golden", True, None),
    (ENV_SWING, 70, 7, "nan", False, None),
    (ENV_TENNIS, 60, 10, "default", False, None),
    (ENV_TENNIS, 60, 10, "default", True, None),
    (ENV_TENNIS, 77, 11, "nan", False, None),
]


@pytest.mark.parametrize("kind,n,epm,wset,rg,options", COUNTER_CASES)
def test_counters_equal_the_oracles(torch, kind, n, epm, wset, rg, options):
    params = es_params(rg)
    W = es_member_weights(kind, wset, n // epm)
    env = es_env(kind, n, params, options=options)
    ret, length, tr, got = evaluate_counted(torch, env, epm, W)
    sealed = env.sealed_substeps()
    env.close()
    want = es_oracle_counters(kind, n, params, tr, length)
    print(kind, wset, rg, options, "sealed", sealed, got)
    assert list(got.values()) == want, (got, dict(zip(COUNTER_NAMES, want)))
    assert got["lockstep_violations"] == 0 and got["episodes_finished"] == n
    if wset == "nan":
        assert got["nonfinite_states"] > 0
    if options and options.get("ff_seal") is False:
        assert sealed == 0
    assert sealed <= got["substeps"]


def test_sealed_fate_exit_books_the_full_flights(torch):
    """the pool's sealed-fate exit under ES: the substeps it books without running them (sealed_substeps) leave every counter as the
    full flights give it, and the returns as those of the run without the exit"""
    n, epm = 200, 10
    params = es_params()
    W = es_member_weights(ENV_SWING, "golden", n // epm)  # (struck balls that leave the court: flights the exit ends early)
    res = {}
    for seal in (True, False):
        env = es_env(ENV_SWING, n, params, options=dict(ff_defer="all", ff_seal=seal))
        assert env.pipeline_form() == "pool"
        ret, length, tr, c = evaluate_counted(torch, env, epm, W)
        res[seal] = (ret, c, env.sealed_substeps())
        env.close()
    print("sealed substeps", res[True][2], "of", res[True][1]["substeps"])
    assert same_bits(res[True][0], res[False][0])
    assert res[True][1] == res[False][1]
    assert res[False][2] == 0 and res[True][2] > 0


# ------------------------------------------------------------------ 3. fast-forward forms and sizes
def test_swing_small_batch_forms_agree(torch):
    n, epm = 200, 10
    params = es_params()
    W = es_member_weights(ENV_SWING, "golden", n // epm)
    forms = [(dict(ff_defer=False), "slots"), (dict(ff_defer="all"), "pool"), (dict(ff_defer="all", ff_seal=False), "pool"),
             (dict(ff_defer=True, ff_defer_margin=4), "slots+pool")]
    rets = []
    for opts, form in forms:
        env = es_env(ENV_SWING, n, params, options=opts)
        assert env.pipeline_form() == form, (opts, env.pipeline_form())
        ret, length, tr, c = evaluate_counted(torch, env, epm, W)
        env.close()
        check_es_trace(torch, ENV_SWING, n, epm, W, ret, length, tr, params)
        assert c["lockstep_violations"] == 0 and c["episodes_finished"] == n
        rets.append(ret)
    for r in rets[1:]:
        assert same_bits(rets[0], r)


@pytest.mark.parametrize("n,rg,options,form", [
    (20000, False, None, "slots"),
    (20000, True, None, "slots+pool"),
    (20000, False, dict(ff_defer="all"), "pool"),
    (131072, False, None, "slots"),               # the BIG fast-forward, one phase
    (131072, False, dict(ff_phases=3), "slots"),  # the BIG fast-forward in phases, its first one the ESC instantiation
], ids=["20k-slots", "20k-rg-slots+pool", "20k-pool", "131k-big", "131k-big-esc"])
def test_swing_large_batch_forms(torch, n, rg, options, form):
    epm = 10 if n == 20000 else 64
    params = es_params(rg)
    M = n // epm
    W = es_member_weights(ENV_SWING, "golden", M)
    env = es_env(ENV_SWING, n, params, options=options)
    assert env.pipeline_form() == form, env.pipeline_form()
    ret, length, tr, c = evaluate_counted(torch, env, epm, W)
    env.close()
    check_es_trace(torch, ENV_SWING, n, epm, W, ret, length, tr, params, members=sample_members(M))
    assert c["lockstep_violations"] == 0 and c["episodes_finished"] == n, c
    other = es_evaluate(torch, ENV_SWING, n, epm, W, params, ff=False, trace=False)
    assert same_bits(ret, other[0]) and np.array_equal(length, other[1]), "the returns depend on the fast-forward form"


def test_tennis_benchmark_shape(torch):
    n, epm = 4000, 10
    params = es_params()
    M = n // epm
    W = es_member_weights(ENV_TENNIS, "default", M)
    env = es_env(ENV_TENNIS, n, params)
    ret, length, tr, c = evaluate_counted(torch, env, epm, W)
    env.close()
    check_es_trace(torch, ENV_TENNIS, n, epm, W, ret, length, tr, params, members=sample_members(M))
    print(c)
    assert c["lockstep_violations"] == 0 and c["episodes_finished"] == n and c["racket_ball_contact_substeps"] > 0, c


# ------------------------------------------------------------------ 4. weight layout and staging
@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
@pytest.mark.parametrize("epm", [10, 1])
def test_weight_row_stride(torch, kind, epm):
    """row stride 1024 passed through, and a non-contiguous view (the Python copy path), staged (10 envs per member) and unstaged
    (1: 64 members per wave): bit-identical to the compact layout"""
    n = 130
    params = es_params()
    M = n // epm
    W = es_member_weights(kind, "golden" if kind == ENV_SWING else "default", M)
    staged = wave_members(n, epm) <= LDS_MEMBERS
    assert staged.all() if epm == 10 else not staged[:-1].any()
    env = es_env(kind, n, params)
    compact = es_run(torch, env, epm, es_population(torch, W), trace=False)
    env.close()
    env = es_env(kind, n, params)
    wide = es_population(torch, W, 1024)
    assert wide.shape[1] == 1024 and wide.is_contiguous()
    ret, length, tr = es_run(torch, env, epm, wide)
    env.close()
    check_es_trace(torch, kind, n, epm, W, ret, length, tr, params)
    assert same_bits(ret, compact[0]) and np.array_equal(length, compact[1])
    env = es_env(kind, n, params)
    view = es_population(torch, np.repeat(W, 2, axis=1), 2 * W.shape[1] + 8)[:, 0:2 * W.shape[1]:2]
    assert not view.is_contiguous() and view.shape[1] == W.shape[1]
    got = es_run(torch, env, epm, view, trace=False)
    env.close()
    assert same_bits(got[0], compact[0]) and np.array_equal(got[1], compact[1])


@pytest.mark.parametrize("kind,n,epm,path", [
    (ENV_SWING, 128, 8, "staged-8"),     # every wave spans exactly 8 members
    (ENV_SWING, 576, 9, "staged-8"),     # 9 envs per member: every wave still spans 8
    (ENV_SWING, 140, 7, "mixed"),        # waves of 10 members (global), the ragged last one 2 (LDS)
    (ENV_TENNIS, 128, 8, "staged-8"),
    (ENV_TENNIS, 126, 7, "unstaged-9+"),
    (ENV_SWING, 100, 100, "single"),     # one member: ESTrainer.evaluate's call
    (ENV_TENNIS, 64, 64, "single"),
])
def test_staging_edges(torch, kind, n, epm, path):
    span = wave_members(n, epm)
    if path == "staged-8":
        assert (span == LDS_MEMBERS).all()
    elif path == "unstaged-9+":
        assert (span > LDS_MEMBERS).all()
    elif path == "mixed":
        assert (span[:-1] > LDS_MEMBERS).all() and span[-1] <= LDS_MEMBERS
    else:
        assert n == epm and (span == 1).all()
    params = es_params()
    W = es_member_weights(kind, "golden" if kind == ENV_SWING else "saturating", n // epm)
    ret, length, tr = es_evaluate(torch, kind, n, epm, W, params)
    check_es_trace(torch, kind, n, epm, W, ret, length, tr, params)


# ------------------------------------------------------------------ 5. trace truncation
@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
def test_trace_truncation(torch, kind):
    n, epm = 130, 10
    params = es_params()
    W = es_member_weights(kind, "golden" if kind == ENV_SWING else "default", n // epm)
    full = es_evaluate(torch, kind, n, epm, W, params)
    bare = es_evaluate(torch, kind, n, epm, W, params, trace=False)
    assert same_bits(full[0], bare[0]) and np.array_equal(full[1], bare[1])
    longest = int(full[1].max())
    cuts = (1, 25, 26) if kind == ENV_SWING else (1, longest // 2, longest - 1)
    for T in cuts:
        env = es_env(kind, n, params)
        ret, length, tr = es_run(torch, env, epm, es_population(torch, W), max_steps=T)
        env.close()
        assert same_bits(ret, full[0]) and np.array_equal(length, full[1]), "max_steps %d changed a result" % T
        for k, v in tr.items():
            assert v.shape[0] == T
            assert (same_bits(v, full[2][k][:T]) if v.dtype != np.uint8 else np.array_equal(v, full[2][k][:T])), (T, k)


# ------------------------------------------------------------------ 6. ES on a used handle
def step_both(torch, env, ref, acts, what):
    """eager steps of env and oracle; compared after a flush (pipelined: the fast-forward writes rewards late)"""
    outs, want = [], []
    for a in acts:
        outs.append(env.step(torch.from_numpy(a).cuda()))
        want.append(ref.step(a))
    if env.pipeline:
        env.flush()
    torch.cuda.synchronize()
    for t, ((o, r, d), w) in enumerate(zip(outs, want)):
        assert same_bits(o.cpu().numpy(), w[0]), "%s obs %d" % (what, t)
        assert same_bits(r.cpu().numpy(), w[1]), "%s reward %d" % (what, t)
        assert np.array_equal(d.cpu().numpy(), w[2]), "%s done %d" % (what, t)


def check_reset_state(env, ref, what):
    w, d = env.get_state_words()
    rw, rd = ref.get_state_words()
    assert np.array_equal(w.cpu().numpy().view(np.uint32), rw), what + ": state words"
    assert np.array_equal(d.cpu().numpy(), rd), what + ": done bytes"


def check_episode_against_oracle(kind, n, params, words, done, ret, length, tr, seed=5):
    """the evaluated episodes follow the oracle from its reset state (words, done): traced rewards, done flags and observations of
    every active step bit for bit, and the returns their float64 sums"""
    from oracle import OracleBatch
    pf = params.copy()
    pf.flags |= F_AUTO_RESET
    ref = OracleBatch(pf, kind, n, seed=seed, precision="f32")
    ref.set_state_words(words, done)
    s = np.zeros(n)
    for t in range(int(length.max())):
        o, r, d, _ = ref.step(np.ascontiguousarray(tr["actions"][t]))
        act = t < length
        assert same_bits(r[act], tr["reward"][t][act]), "reward of step %d" % t
        assert np.array_equal(d[act], tr["done"][t][act]), "done of step %d" % t
        if t + 1 < tr["obs"].shape[0]:
            nxt = t + 1 < length
            assert same_bits(o[nxt], tr["obs"][t + 1][nxt]), "obs after step %d" % t
        s = np.where(act, s + r.astype(np.float64), s)
    ref.close()
    assert same_bits(s, ret)


def test_swing_on_a_used_handle(torch):
    """a pipelined pool-form SwingRacket handle 30 steps in (episode 0 parked in the pool at step 26, its fast-forward pending):
    es_evaluate delivers those rewards, evaluates the next episode and leaves every env at its reset; of two graphs captured
    before it, the one of phase 0 is accepted after it and follows the oracle, the one of phase 4 is refused"""
    from oracle import OracleBatch
    from tennisbot_rl_amd.stepper import StepperError
    n, epm = 192, 12
    params = es_params()
    W = es_member_weights(ENV_SWING, "golden", n // epm)
    rng = np.random.default_rng(17)
    env = es_env(ENV_SWING, n, params, options=dict(ff_defer="all"))
    assert env.pipeline_form() == "pool"
    ref = OracleBatch(params, ENV_SWING, n, seed=5, precision="f32")
    assert same_bits(env.reset().cpu().numpy(), ref.reset())
    K = 5
    a_buf = torch.zeros((n, 6), device="cuda:0")
    outs = [(torch.empty((n, 6), device="cuda:0"), torch.empty(n, device="cuda:0"), torch.empty(n, dtype=torch.uint8, device="cuda:0"))
            for _ in range(K)]

    def body():
        for t in range(K):
            env.step(a_buf, out=outs[t])
    g0 = env.capture(body)  # at phase 0
    step_both(torch, env, ref, [rng.uniform(-1, 1, (n, 6)).astype(np.float32) for _ in range(4)], "before capture")
    g4 = env.capture(body)  # at phase 4
    assert not g0.valid() and g4.valid()
    acts = [rng.uniform(-1, 1, (n, 6)).astype(np.float32) for _ in range(26)]
    pending = [env.step(torch.from_numpy(a).cuda()) for a in acts]  # unflushed: the 26th step parks every env in the pool
    assert env.phase() == 4
    env.counters_reset()
    ret, length, tr = es_run(torch, env, epm, es_population(torch, W))
    c = env.counters()
    assert c["lockstep_violations"] == 0 and c["episodes_finished"] == n, c
    # the evaluation ran the pending pool into the steps' own buffers: those outputs are the oracle's
    for t, a in enumerate(acts):
        o, r, d, _ = ref.step(a)
        assert same_bits(pending[t][1].cpu().numpy(), r), "reward of pending step %d" % t
        assert same_bits(pending[t][0].cpu().numpy(), o) and np.array_equal(pending[t][2].cpu().numpy(), d), "pending step %d" % t
    ep_before = ref.get_state()["episode"].astype(np.int64)
    # the next episode of every env
    assert same_bits(tr["obs"][0], ref.reset())
    assert np.array_equal(env.get_state()["episode"].astype(np.int64), ep_before + 1)
    check_reset_state(env, ref, "after es_evaluate")
    check_episode_against_oracle(ENV_SWING, n, params, *ref.get_state_words(), ret, length, tr)
    assert env.phase() == 0
    assert not g4.valid()
    with pytest.raises(StepperError, match="phase"):
        g4.replay()
    assert g0.valid()
    a = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
    a_buf.copy_(torch.from_numpy(a).cuda())  # (every captured step reads a_buf)
    g0.replay()
    env.flush()
    torch.cuda.synchronize()
    for t in range(K):
        o, r, d, _ = ref.step(a)
        assert same_bits(outs[t][0].cpu().numpy(), o) and same_bits(outs[t][1].cpu().numpy(), r), "replayed step %d" % t
        assert np.array_equal(outs[t][2].cpu().numpy(), d)
    assert env.phase() == K
    step_both(torch, env, ref, [rng.uniform(-1, 1, (n, 6)).astype(np.float32) for _ in range(26 - K + 3)], "after es_evaluate")
    assert env.counters()["lockstep_violations"] == 0
    env.close()
    ref.close()


def test_tennis_on_a_used_handle(torch):
    """Tennisbot 800 steps in (envs in episodes of their own): es_evaluate evaluates each env's next episode and leaves the env at
    its reset; a graph captured before the call is accepted after it and follows the oracle"""
    from oracle import OracleBatch
    n, epm = 128, 8
    params = es_params()
    W = es_member_weights(ENV_TENNIS, "default", n // epm)
    rng = np.random.default_rng(18)
    env = es_env(ENV_TENNIS, n, params)
    ref = OracleBatch(params, ENV_TENNIS, n, seed=5, precision="f32")
    assert same_bits(env.reset().cpu().numpy(), ref.reset())
    K = 3
    a_buf = torch.zeros((n, 2), device="cuda:0")
    outs = [(torch.empty((n, 12), device="cuda:0"), torch.empty(n, device="cuda:0"), torch.empty(n, dtype=torch.uint8, device="cuda:0"))
            for _ in range(K)]

    def body():
        for t in range(K):
            env.step(a_buf, out=outs[t])
    g = env.capture(body)
    step_both(torch, env, ref, [rng.uniform(-1, 1, (n, 2)).astype(np.float32) for _ in range(800)], "before es_evaluate")
    ep_before = env.get_state()["episode"].astype(np.int64)
    assert ep_before.max() > ep_before.min()  # the envs are in different episodes
    ret, length, tr = es_run(torch, env, epm, es_population(torch, W))
    assert same_bits(tr["obs"][0], ref.reset())
    assert np.array_equal(env.get_state()["episode"].astype(np.int64), ep_before + 1)
    check_reset_state(env, ref, "after es_evaluate")
    check_episode_against_oracle(ENV_TENNIS, n, params, *ref.get_state_words(), ret, length, tr)
    assert g.valid()
    a = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    a_buf.copy_(torch.from_numpy(a).cuda())
    g.replay()
    torch.cuda.synchronize()
    for t in range(K):
        o, r, d, _ = ref.step(a)
        assert same_bits(outs[t][0].cpu().numpy(), o) and same_bits(outs[t][1].cpu().numpy(), r), "replayed step %d" % t
        assert np.array_equal(outs[t][2].cpu().numpy(), d)
    step_both(torch, env, ref, [rng.uniform(-1, 1, (n, 2)).astype(np.float32) for _ in range(40)], "after es_evaluate")
    assert env.counters()["lockstep_violations"] == 0
    env.close()
    ref.close()
