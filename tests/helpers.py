"""Shared helpers for the test-suite: state construction in the library's SoA word layout, random engine parameters, and the checks
of the fused ES evaluation against the oracle."""
import os

import numpy as np

from tennisbot_rl_amd.params import (ACT_DIM, COUNTER_NAMES, ENV_SWING, ENV_TENNIS, F_AUTO_RESET, F_DEFAULT, F_RACKET_GROUND, OBS_DIM, STATE_ROWS,
                                     STATE_WORDS, default_params, reference_rolling_friction)

IDENT_Q = (0.0, 0.0, 0.0, 1.0)


def make_words(kind, n, **fields):
    """Build [words, n] uint32 + done[n] from named fields (each scalar, [k] or [n, k]).

    Unspecified rows default to 0 (quaternion: identity; init_dist: 1)."""
    names = STATE_ROWS[kind]
    vals = np.zeros((STATE_WORDS[kind], n), np.float64)
    defaults = {"racket_quat": IDENT_Q, "init_dist": (1.0,), "racket_scale": (1.0,)}
    done = np.asarray(fields.pop("done", np.zeros(n)), np.uint8) * np.ones(n, np.uint8)
    groups = {}
    for i, nm in enumerate(names):
        groups.setdefault(nm, []).append(i)
    for nm, rows in groups.items():
        v = fields.pop(nm, defaults.get(nm, 0.0))
        v = np.asarray(v, np.float64)
        if v.ndim == 0:
            v = np.full((n, len(rows)), float(v))
        elif v.ndim == 1 and v.shape[0] == len(rows):
            v = np.tile(v, (n, 1))
        elif v.ndim == 1 and v.shape[0] == n and len(rows) == 1:
            v = v[:, None]
        vals[rows] = v.reshape(n, len(rows)).T
    assert not fields, "unknown state fields: %s" % sorted(fields)
    words = vals.astype(np.float32).view(np.uint32).copy()
    nw = STATE_WORDS[kind]
    words[nw - 2] = vals[nw - 2].astype(np.int32).view(np.uint32)
    words[nw - 1] = vals[nw - 1].astype(np.uint32)
    return words, done


def racket_contact_states(kind, n, rng, rg=False, low_rackets=False):
    """(words, done) of n forced contact states: the ball anywhere in a thin shell around a randomly oriented (Tennisbot: randomly
    scaled, 1 .. 3) racket that itself hovers close to the court -- faces, rim, handle, corners, grazing and deep overlaps, ball on
    racket AND ground at once. rg: the racket's COM at least its reach above the court (0.52 .. 0.75 x scale), so that no hull
    vertex starts under it. low_rackets (with rg): a seeded half of the envs get a COM height of 0.02 .. 0.52 x scale instead:
    hull vertices on and under the court (vertex_supported: "however deep below it"), the racket<->court rows from the first
    substep on, many of them in one solve with a ball contact. Without low_rackets the draws from rng are those
    test_fuzzed_states_around_the_racket_stay_bit_exact has always made, in its order."""
    p = default_params()
    scale = rng.uniform(1.0, 3.0, n) if kind != ENV_SWING else np.ones(n)
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    rp = np.stack([rng.uniform(8, 12, n), rng.uniform(-4, 4, n), rng.uniform(0.05, 1.2, n) * scale], 1)
    if rg:  # keep every hull vertex above the court (the stateless manifold ignores vertices below it): COM at least its reach up
        rp[:, 2] = rng.uniform(0.52, 0.75, n) * scale
    if low_rackets:
        low = rng.random(n) < 0.5
        rp[low, 2] = (rng.uniform(0.02, 0.52, n) * scale)[low]
    ht, r = float(p.racket_half_thick), float(p.ball_radius)
    pad = r + 0.004
    loc = np.stack([rng.uniform(-(ht * scale + pad), ht * scale + pad), rng.uniform(-0.16 * scale - pad, 0.16 * scale + pad),
                    rng.uniform(-0.51 * scale - pad, 0.21 * scale + pad)], 1)
    # push two thirds of the samples onto the shell (the rest stay inside: deep overlaps)
    k = rng.integers(0, 3, n); sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0); shell = rng.random(n) < 0.67
    ext = np.stack([ht * scale, 0.15 * scale, np.where(sgn > 0, 0.197, 0.5) * scale], 1)
    idx = np.arange(n)
    loc[idx[shell], k[shell]] = (sgn * (ext[idx, k] + r + rng.uniform(-0.004, 0.001, n)))[shell]

    def rot(q, v):
        u, w = q[:, :3], q[:, 3:4]
        t = 2 * np.cross(u, v)
        return v + w * t + np.cross(u, t)
    bp = rp + rot(q, loc)
    bp[:, 2] = np.maximum(bp[:, 2], 0.005 + r - 0.003)  # never (much) under the court
    fields = dict(racket_pos=rp, racket_quat=q, racket_vel=rng.uniform(-4, 4, (n, 3)), racket_angvel=rng.uniform(-6, 6, (n, 3)),
                  ball_pos=bp, ball_vel=rng.uniform(-15, 15, (n, 3)), ball_angvel=rng.uniform(-60, 60, (n, 3)))
    if kind != ENV_SWING:
        fields.update(shoot_force=(30, 0, 20), step_count=50, racket_scale=scale)
    else:
        fields.update(goal=np.stack([rng.uniform(-11, -4, n), rng.uniform(-4, 4, n)], 1), spawn_pos=(9, 0, 0.6), init_dist=rng.uniform(8, 20, n),
                      step_count=rng.integers(0, 24, n))
    return make_words(kind, n, **fields)


# the low-racket batch of tests/test_tennis_contact_states.py (what it reaches, on the oracle) and tests/test_gpu_tennis_extended_loops.py
# (the kernels on it): Tennisbot, 12 steps -- the balls start on the rackets and most envs' episodes end within a few steps
LOW_RACKET_SEED, LOW_RACKET_STEPS = 1207, 12
_LOW_RACKETS = {}


def low_racket_params():
    """Tennisbot's full contact set: racket<->court contact and the reference's rolling-friction rows"""
    return default_params(flags=F_DEFAULT | F_RACKET_GROUND, **reference_rolling_friction())


def low_racket_batch(n=2048):
    """(words [W, n] uint32, done [n], actions [12, n, 2] float32 uniform in [-1, 1) from default_rng(1)): the first n of 2048
    forced Tennisbot contact states with low rackets, built once; callers must not write into them"""
    if not _LOW_RACKETS:
        w, d = racket_contact_states(ENV_TENNIS, 2048, np.random.default_rng(LOW_RACKET_SEED), rg=True, low_rackets=True)
        _LOW_RACKETS["all"] = (w, d, np.random.default_rng(1).uniform(-1, 1, (LOW_RACKET_STEPS, 2048, 2)).astype(np.float32))
    w, d, a = _LOW_RACKETS["all"]
    return np.ascontiguousarray(w[:, :n]), np.ascontiguousarray(d[:n]), np.ascontiguousarray(a[:, :n])


def words_to_f32(kind, words):
    """float view of the float rows + int rows split out."""
    nw = STATE_WORDS[kind]
    f = words[: nw - 2].view(np.float32)
    return f, words[nw - 2].view(np.int32), words[nw - 1]


def far_ball(kind):
    """A ball position that touches nothing (high above the court)."""
    return (0.0, 3.0, 50.0) if kind == ENV_SWING else (0.0, 3.0, 50.0)


# ------------------------------------------------------------------ engine parameters
def draw_engine_params(rng, rolling=False):
    """one random draw of every engine constant recalled from Bullet as default_params() keywords: the ranges
    of the parity tests' randomised-parameter matrix; `rolling` adds the rolling-friction rows"""
    over = dict(
        gravity=rng.uniform(3.0, 15.0), lin_damp=rng.uniform(0.0, 0.1), ang_damp=rng.uniform(0.0, 0.1),
        max_ang_step=rng.uniform(0.3, 1.2), rest_vel_threshold=rng.uniform(0.0, 1.0), erp=rng.uniform(0.02, 0.4),
        contact_threshold=rng.uniform(2e-4, 3e-3), solver_iters=int(rng.integers(4, 80)), solver_tol=10.0 ** rng.uniform(-7, -4),
        racket_mass=rng.uniform(1.0, 8.0), racket_inertia=tuple(rng.uniform(0.02, 0.3, 3)), ball_mass=rng.uniform(0.03, 0.2),
        ball_inertia=10.0 ** rng.uniform(-5, -3), rest_racket=rng.uniform(0.0, 1.0), rest_court=rng.uniform(0.0, 1.0),
        rest_goal=rng.uniform(0.0, 0.9), fric_racket=rng.uniform(0.0, 0.8), fric_court=rng.uniform(0.0, 0.8), fric_goal=rng.uniform(0.0, 0.8),
        magnus_k=rng.choice([0.0, 1e-4, 5e-4]), ball_spin_max=rng.choice([0.0, 50.0, 200.0]),
        lin_damp_quad=rng.uniform(0.0, 0.1), ang_damp_quad=rng.uniform(0.0, 0.1))
    if rolling:
        over.update(roll_racket=rng.uniform(0, 2e-3), roll_court=rng.uniform(0, 2e-3), roll_goal=rng.uniform(0, 2e-3))
    return over


# ------------------------------------------------------------------ the fused ES evaluation (tb_es_evaluate) against the oracle
ES_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "es_swing_policy.npz")


def es_member_weights(kind, name, M):
    """[M, P] float32: torch's default init (a seed per member), the shipped ES policy (+ small noise per member), saturating
    N(0, 2^2), all zero, or the default init with a NaN weight in member 1"""
    import es_reference as er
    from tennisbot_rl_amd import es
    O, A = OBS_DIM[kind], ACT_DIM[kind]
    P = er.es_floats(O, A)
    rng = np.random.default_rng(7)
    if name in ("default", "nan"):
        W = np.stack([es.initial_weights(kind, 100 + m).numpy() for m in range(M)])
        if name == "nan":
            W[min(1, M - 1), 37] = np.nan
    elif name == "golden":
        W = np.load(ES_GOLD)["weights"][None, :] + rng.normal(0.0, 0.02, (M, P)).astype(np.float32)
        W[0] = np.load(ES_GOLD)["weights"]
    elif name == "saturating":
        W = rng.normal(0.0, 2.0, (M, P))
    else:
        W = np.zeros((M, P))
    return np.ascontiguousarray(W, dtype=np.float32)


def same_bits(a, b):
    """bit for bit, any NaN matching any NaN (a NaN's payload is not part of the contract)"""
    a, b = np.asarray(a), np.asarray(b)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def es_params(rg=False, **over):
    """default_params with auto-reset (every ES handle runs with it), racket<->court contact on request, other keywords passed on"""
    return default_params(flags=F_DEFAULT | F_AUTO_RESET | (F_RACKET_GROUND if rg else 0), **over)


def es_env(kind, n, params, seed=5, options=None):
    """a BatchedEnv as tb_es_evaluate needs it (SwingRacket: pipelined); options: make_options() keywords"""
    from tennisbot_rl_amd.stepper import BatchedEnv
    return BatchedEnv(kind, n, device="cuda:0", seed=seed, params=params, pipeline=kind == ENV_SWING, options=options)


def es_population(torch, W, stride=None):
    """W [M, P] -> a zeroed [M, stride] device tensor holding W in its first P columns (stride: ceil4(P) by default)"""
    M, P = W.shape
    pop = torch.zeros((M, stride or (P + 3) // 4 * 4), device="cuda:0")
    pop[:, :P] = torch.from_numpy(W).to("cuda:0")
    return pop


def es_run(torch, env, epm, pop, trace=True, max_steps=None):
    """env.es_evaluate -> [returns [n] float64, lengths [n] int32 (, trace dict of numpy arrays)] on the host"""
    out = env.es_evaluate(pop, epm, trace=trace, max_steps=max_steps)
    torch.cuda.synchronize()
    res = [x.reshape(-1).cpu().numpy() for x in out[:2]]
    if trace:
        res.append({k: v.cpu().numpy() for k, v in out[2].items()})
    return res


def es_evaluate(torch, kind, n, epm, W, params, ff=None, trace=True, seed=5, options=None):
    """one evaluation on a fresh handle (episode 0 of every env); ff: TbOptions.ff_defer (make_options' form)"""
    opts = dict(options or {})
    if ff is not None:
        opts["ff_defer"] = ff
    env = es_env(kind, n, params, seed=seed, options=opts)
    res = es_run(torch, env, epm, es_population(torch, W), trace=trace)
    env.close()
    return res


def check_es_trace(torch, kind, n, epm, W, ret, length, tr, params, seed=5, members=None):
    """the ES trace of a fresh handle (episode 0) against the oracle, the env's own step path and tests/es_reference.py:
    oracle reset bit for bit, replay through BatchedEnv.step bit for bit, net_in the float64 normaliser rounded bit for bit, the
    network within twice its float64 forward bound (members: those of the members, default all), actions the clip of raw, the
    return the float64 sum of the rewards through the first done, the length that step + 1"""
    import es_reference as er
    from oracle import OracleBatch
    from tennisbot_rl_amd.stepper import BatchedEnv
    O, A = OBS_DIM[kind], ACT_DIM[kind]
    pf = params.copy()
    pf.flags |= F_AUTO_RESET
    T = tr["reward"].shape[0]
    assert length.min() >= 1 and length.max() <= T
    if kind == ENV_SWING:
        assert (length == 26).all()
    steps = np.arange(T)[:, None]
    act = steps < length[None, :]  # [T, n] the env's episode ran step t
    # 1. the first observation is the oracle's reset of episode 0
    ref = OracleBatch(pf, kind, n, seed=seed, precision="f32")
    assert np.array_equal(tr["obs"][0].view(np.uint32), ref.reset().view(np.uint32))
    ref.close()
    # 2. replay through the env's own step path
    env = BatchedEnv(kind, n, device="cuda:0", seed=seed, params=pf)
    env.reset()
    obs_r, rew_r, done_r = [], [], []
    for t in range(int(length.max())):
        o, r, d = env.step(torch.from_numpy(np.ascontiguousarray(tr["actions"][t])).to("cuda:0"))
        obs_r.append(o.cpu().numpy()); rew_r.append(r.cpu().numpy()); done_r.append(d.cpu().numpy())
    env.close()
    Tl = len(obs_r)
    obs_r, rew_r, done_r = np.stack(obs_r), np.stack(rew_r), np.stack(done_r)
    a = act[:Tl]
    assert same_bits(rew_r[a], tr["reward"][:Tl][a]), "rewards differ from the replay"
    assert np.array_equal(done_r[a], tr["done"][:Tl][a]), "done flags differ from the replay"
    nxt = (steps[:Tl - 1] + 1) < length[None, :]  # obs[t + 1] recorded: step t was not the last
    assert same_bits(obs_r[:Tl - 1][nxt], tr["obs"][1:Tl][nxt]), "observations differ from the replay"
    # 3. the normaliser, bit for bit
    rows = er.normalised_rows(tr["obs"])
    assert same_bits(rows[act], tr["net_in"][act]), "net_in is not the float64 normaliser rounded"
    # 4. the network within twice its forward error bound; actions = clip(raw), NaN kept
    clipped = np.clip(tr["raw"], -1.0, 1.0)
    assert same_bits(clipped[act], tr["actions"][act])
    M = n // epm
    for m in (range(M) if members is None else members):
        envs = slice(m * epm, (m + 1) * epm)
        p = er.unpack(W[m], O, A)
        Tm = int(length[envs].max())
        want, bound = er.forward_bound(p, er.windows(tr["net_in"][:Tm, envs]))
        got = np.where(act[:Tm, envs, None], tr["raw"][:Tm, envs], want)
        er.assert_within("raw action of member %d" % m, got, want, 2.0 * bound)
    # 5. the return: float64 sum through the first done; the length: that step + 1
    done = tr["done"] != 0
    first = np.where(done.any(0), done.argmax(0), -1)
    assert np.array_equal(first + 1, length), "length is not the first done + 1"
    s = np.zeros(n)
    for t in range(T):
        s = np.where(act[t], s + tr["reward"][t].astype(np.float64), s)
    assert same_bits(s, ret), "return is not the float64 sum of the step rewards"


def es_oracle_counters(kind, n, params, tr, length, seed=5, threads=1):
    """the nine counters the float32 oracle books for exactly the traced episodes (episode 0 of every env): SwingRacket, whose
    episodes are all 26 steps, one auto-reset batch stepped 26 times with the traced actions; Tennisbot one single-env batch per
    env (env_id_base = i), stepped length[i] times, summed"""
    from oracle import OracleBatch
    pf = params.copy()
    pf.flags |= F_AUTO_RESET
    if kind == ENV_SWING:
        ref = OracleBatch(pf, kind, n, seed=seed, precision="f32", threads=threads)
        ref.reset()
        for t in range(26):
            ref.step(np.ascontiguousarray(tr["actions"][t]))
        c = [int(x) for x in ref.counters()]
        ref.close()
        return c
    total = np.zeros(len(COUNTER_NAMES), np.int64)
    for i in range(n):
        ref = OracleBatch(pf, kind, 1, seed=seed, env_id_base=i, precision="f32")
        ref.reset()
        for t in range(int(length[i])):
            ref.step(np.ascontiguousarray(tr["actions"][t, i:i + 1]))
        total += np.array([int(x) for x in ref.counters()], np.int64)
        ref.close()
    return [int(x) for x in total]
