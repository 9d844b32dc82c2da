"""A population of SAC / TQC actors in one launch (tb_sac_evaluate_members; tb_sac_evaluate_kernel's members form in
csrc/tb_sac.hpp) on a real MI355X. The yardstick is the existing single-actor call: resets and noise are keyed by the global env id,
so row m of a members launch over M x R envs at ID_BASE must equal, bit for bit, sac_evaluate with actor m on a fresh handle of R
envs whose env_id_base is ID_BASE + m R -- returns, lengths and every traced row. Then equal members against sac_evaluate on one
handle, the episode contract, trace neutrality with guard words, the refusals on a real handle, and tools/rank_checkpoints.py -s sac
against a direct call.

Actors: the `plain` actor of tests/test_gpu_sac_evaluate.py (seeded torch-default init, the mu head x 30), one seed per member."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, OBS_DIM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NOISE_SEED = 0x5EED1234ABCD
ENV_SEED, ID_BASE = 21, 1 << 33   # (env ids beyond 32 bits: the noise key's high word is in use)
MU_SCALE = 30.0
M_MAX = 3
# One init seed per member, chosen, not arbitrary. On SwingRacket most seeds give a racket that runs away from every ball (every
# return 0, as tests/test_gpu_sac_evaluate.py records), and two such members cannot be told apart by their returns: of the seeds 0..39
# on an MI355X only 3, 14, 23, 25 and 32 strike balls in most 16-env blocks of these env ids (6, 12, 22 and 35 in one or two; the
# other 31 in none), and 14 only when it acts stochastically. 3, 32 and 23 strike some in every block their member owns in the cases
# below, on the mean action too (seed 3 alone fails there: its deterministic return on member 1's block is 0 like most seeds'). On
# Tennisbot 1235, 1236 and 1237 all score in every block. The separation is asserted in the test either way.
MEMBER_SEED = {ENV_SWING: (3, 32, 23), ENV_TENNIS: (1235, 1236, 1237)}
T_MAX = {ENV_SWING: 26, ENV_TENNIS: 1001}
TRACE_KEYS = ("obs", "eps", "actions", "reward", "done")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_ACTORS = {}


def member_state_dict(torch, kind, m):
    from tennisbot_rl_amd.sac import build_sac_modules
    torch.manual_seed(MEMBER_SEED[kind][m])
    actor = build_sac_modules(OBS_DIM[kind], ACT_DIM[kind])[0]
    with torch.no_grad():
        actor.mu.weight.mul_(MU_SCALE)
    return actor.state_dict()


def member_actors(torch, kind):
    """[M_MAX, P] on the GPU, built once per kind and never written: row m is member m's flat TB_SAC_ACTOR vector"""
    from tennisbot_rl_amd.sac import flatten_actor
    if kind not in _ACTORS:
        _ACTORS[kind] = torch.stack([flatten_actor(member_state_dict(torch, kind, m)) for m in range(M_MAX)]).to(DEV)
    return _ACTORS[kind]


def case_params(extended=False):
    from tennisbot_rl_amd.params import F_DEFAULT, F_RACKET_GROUND, default_params, reference_rolling_friction
    if extended:  # the reference's full contact set: racket<->court contact + the rolling-friction rows
        return default_params(flags=F_DEFAULT | F_RACKET_GROUND, **reference_rolling_friction())
    return default_params()


def make_env(kind, n, params, pipeline=None, base=ID_BASE):
    from tennisbot_rl_amd.stepper import BatchedEnv
    return BatchedEnv(kind, n, device=DEV, seed=ENV_SEED, env_id_base=base, params=params, pipeline=kind == ENV_SWING if pipeline is None else pipeline,
                      track_terminal_obs=False)


def members(torch, env, w, R, deterministic=False, trace=False, max_steps=None):
    out = env.sac_evaluate_members(w, R, seed=NOISE_SEED, deterministic=deterministic, trace=trace, max_steps=max_steps)
    torch.cuda.synchronize()
    return out


def single(torch, env, w, deterministic=False, trace=False, max_steps=None):
    out = env.sac_evaluate(w, seed=NOISE_SEED, deterministic=deterministic, trace=trace, max_steps=max_steps)
    torch.cuda.synchronize()
    return out


def same(torch, a, b):
    """two device tensors, bit for bit"""
    word = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(word), b.contiguous().view(word)))


def padded(torch, w, extra):
    """the rows `extra` floats further apart, NaN in between: floats the kernel must never read"""
    out = torch.full((w.shape[0], w.shape[1] + extra), float("nan"), dtype=torch.float32, device=w.device)
    out[:, :w.shape[1]] = w
    return out


TWIN_CASES = [  # kind, M, R, deterministic, extended contact set, NaN-padded stride
    (ENV_TENNIS, 3, 16, False, False, True),
    (ENV_TENNIS, 2, 32, True, False, False),
    (ENV_TENNIS, 2, 16, False, True, False),
    (ENV_SWING, 3, 16, False, False, True),
    (ENV_SWING, 2, 48, False, False, False),
    (ENV_SWING, 2, 16, True, True, False),
]


@pytest.mark.parametrize("kind,M,R,deterministic,extended,pad", TWIN_CASES)
def test_each_member_is_its_twin_handle_bit_for_bit(torch, kind, M, R, deterministic, extended, pad):
    w, params = member_actors(torch, kind)[:M].contiguous(), case_params(extended)
    a = make_env(kind, M * R, params)
    assert R % a.policy_member_granule() == 0
    wa = padded(torch, w, 8) if pad else w
    assert wa.shape[1] == a.sac_actor_floats() + (8 if pad else 0) and wa.data_ptr() % 16 == 0 and wa.is_contiguous()
    ret, length, tr = members(torch, a, wa, R, deterministic, trace=True)
    assert tuple(ret.shape) == (M, R) and tuple(length.shape) == (M, R) and ret.dtype == torch.float64 and length.dtype == torch.int32
    T = T_MAX[kind]
    assert all(tr[k].shape[:2] == (T, M * R) for k in TRACE_KEYS)
    for m in range(M):
        twin = make_env(kind, R, params, base=ID_BASE + m * R)
        want_ret, want_len, want_tr = single(torch, twin, w[m], deterministic, trace=True)
        twin.close()
        print("kind=%d member %d: lengths %d .. %d, returns %g .. %g, %d non-zero" % (kind, m, int(length[m].min()), int(length[m].max()), float(ret[m].min()),
                                                                                    float(ret[m].max()), int((ret[m] != 0).sum())))
        assert torch.equal(length[m], want_len), (m, length[m], want_len)
        assert same(torch, ret[m], want_ret), (m, ret[m], want_ret)
        live = (torch.arange(T, device=DEV)[:, None] < want_len[None, :].long())   # [T, R]: the env's episode ran step t
        assert int(live.sum()) == int(want_len.sum()) > 0
        for k in TRACE_KEYS:
            got, want = tr[k][:, m * R:(m + 1) * R], want_tr[k]
            assert same(torch, got[live], want[live]), "member %d: live %s rows differ" % (m, k)
            assert same(torch, got, want), "member %d: %s rows behind an episode's end differ" % (m, k)
    # the test can tell members apart: member 1's envs under member 0's actor are other episodes
    twin = make_env(kind, R, params, base=ID_BASE + R)
    other_ret, other_len = single(torch, twin, w[0], deterministic)
    twin.close()
    assert not (same(torch, other_ret, ret[1]) and torch.equal(other_len, length[1])), "member 0's actor reproduces member 1's row: the case cannot see a wrong blob"
    assert bool(torch.isfinite(ret).all()) and bool((ret != 0.0).any())
    if kind == ENV_SWING:
        assert bool((length == 26).all())
    else:
        assert bool(((length >= 1) & (length <= 1001)).all())
    c = a.counters()
    assert c["episodes_finished"] == M * R and c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0
    assert a.phase() == 0
    a.close()


@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
@pytest.mark.parametrize("M,R", [(3, 16), (1, 48)])
def test_equal_members_are_sac_evaluate(torch, kind, M, R):
    w1, params = member_actors(torch, kind)[1], case_params()
    a, b = make_env(kind, M * R, params), make_env(kind, M * R, params)
    ret, length = members(torch, a, w1.unsqueeze(0).repeat(M, 1), R)
    want_ret, want_len = single(torch, b, w1)
    assert same(torch, ret.reshape(-1), want_ret) and torch.equal(length.reshape(-1), want_len)
    assert bool((ret != 0.0).any())
    a.close(); b.close()


@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
def test_call_k_is_episode_k_and_the_handle_is_left_freshly_reset(torch, kind):
    M, R = 2, 16
    w, params = member_actors(torch, kind)[:M].contiguous(), case_params()
    a, twin, plain = (make_env(kind, M * R, params) for _ in range(3))
    r0, l0 = members(torch, a, w, R)
    r1, l1 = members(torch, a, w, R)
    assert not same(torch, r0, r1), "two calls on one handle returned the same episodes"
    t0, tl0 = members(torch, twin, w, R)
    assert same(torch, t0, r0) and torch.equal(tl0, l0)            # a fresh twin's first call repeats the first
    plain.reset()
    plain.reset()                                                  # two calls = two resets: episode 1
    wa, da = a.get_state_words()
    wp, dp = plain.get_state_words()
    assert torch.equal(wa, wp) and torch.equal(da, dp)
    assert int(wa[-1].min()) == 1 and int(wa[-1].max()) == 1       # (the episode word)
    assert a.phase() == 0
    for e in (a, twin, plain):
        e.close()


def raw_call(torch, env, ptr, M, stride, R, T, struct_size=None, null=None, guard=64, fill=0x5A):
    """tb_sac_evaluate_members with caller-owned outputs (zero-filled) and trace arrays of exactly [T][n][.] elements, `guard`
    sentinel elements behind each; null: the trace array to hand over as NULL"""
    from tennisbot_rl_amd.stepper import TbSacEvalTrace
    n, O, A = env.num_envs, env.obs_dim, env.act_dim
    ret = torch.zeros(n, dtype=torch.float64, device=DEV)
    length = torch.zeros(n, dtype=torch.int32, device=DEV)
    sizes = {"obs": T * n * O, "eps": T * n * A, "actions": T * n * A, "reward": T * n, "done": T * n}
    width = {k: 1 if k == "done" else 4 for k in sizes}
    bufs = {k: torch.full((width[k] * (m + guard),), fill, dtype=torch.uint8, device=DEV) for k, m in sizes.items()}
    tr = TbSacEvalTrace(ctypes.sizeof(TbSacEvalTrace) if struct_size is None else struct_size, T, *(None if k == null else bufs[k].data_ptr() for k in TRACE_KEYS))
    rc = env.L.tb_sac_evaluate_members(env._h, ptr, M, stride, R, ret.data_ptr(), length.data_ptr(), NOISE_SEED, 0, ctypes.byref(tr), env._stream())
    torch.cuda.synchronize()
    body = {k: bufs[k][:width[k] * m] for k, m in sizes.items()}
    tail = {k: bufs[k][width[k] * m:] for k, m in sizes.items()}
    return rc, ret, length, body, tail


@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
def test_trace_changes_no_result_and_stays_inside_its_arrays(torch, kind):
    M, R, short = 2, 16, 7
    n = M * R
    w, params = member_actors(torch, kind)[:M].contiguous(), case_params()
    P = w.shape[1]
    env = make_env(kind, n, params)
    ret, length, tr = members(torch, env, w, R, trace=True)
    env.close()
    assert short < int(length.max())
    env = make_env(kind, n, params)
    r, ln = members(torch, env, w, R)
    env.close()
    assert same(torch, r, ret) and torch.equal(ln, length), "the results without the trace differ"
    env = make_env(kind, n, params)
    r, ln, ts = members(torch, env, w, R, trace=True, max_steps=short)
    env.close()
    assert same(torch, r, ret) and torch.equal(ln, length), "the results with a short trace differ"
    assert all(same(torch, ts[k], tr[k][:short]) for k in TRACE_KEYS), "the short trace is not the long one's first rows"
    for T in (short, T_MAX[kind]):
        env = make_env(kind, n, params)
        rc, r, ln, body, tail = raw_call(torch, env, w.data_ptr(), M, P, R, T)
        env.close()
        assert rc == 0 and same(torch, r.view(M, R), ret) and torch.equal(ln.view(M, R), length)
        for k in tail:
            assert bool((tail[k] == 0x5A).all()), "T = %d: the words behind %s were written" % (T, k)
        live = torch.arange(T, device=DEV)[:, None] < length.reshape(-1)[None, :].long()   # [T, n]
        got = body["reward"].view(torch.float32).view(T, n)
        assert same(torch, got[live], tr["reward"][:T][live])
        assert bool((body["reward"].view(T, n, 4)[~live] == 0x5A).all()), "T = %d: reward rows after an env's last step were written" % T


def test_refusals_on_a_real_handle_launch_nothing(torch):
    from tennisbot_rl_amd.stepper import StepperError
    n = 48
    w = member_actors(torch, ENV_SWING)
    P = w.shape[1]
    wide = padded(torch, w, 8)
    ret = torch.zeros(n, dtype=torch.float64, device=DEV)
    length = torch.zeros(n, dtype=torch.int32, device=DEV)
    piped, plain = make_env(ENV_SWING, n, case_params(), True), make_env(ENV_SWING, n, case_params(), False)
    assert P == piped.sac_actor_floats() and wide.data_ptr() % 16 == 0

    def call(env, ptr, M, stride, R, r=ret, ln=length):
        return env.L.tb_sac_evaluate_members(env._h, ptr, M, stride, R, None if r is None else r.data_ptr(), None if ln is None else ln.data_ptr(), 1, 0, None, None)

    piped.reset()
    w0, d0 = piped.get_state_words()
    c0 = piped.counters()
    cases = [  # actors, M, stride, R
        (wide.data_ptr(), 6, P + 8, 8),          # R below the granule
        (wide.data_ptr(), 2, P + 8, 24),         # R not a multiple of it
        (wide.data_ptr(), 3, P + 8, 0),          # R not positive
        (wide.data_ptr(), 2, P + 8, 16),         # M R != n
        (wide.data_ptr(), 3, P - 4, 16),         # a stride below the vector
        (wide.data_ptr(), 3, P + 2, 16),         # ... not a multiple of 4
        (wide.data_ptr() + 4, 3, P + 4, 16),     # a misaligned base
        (None, 3, P + 8, 16),
        (wide.data_ptr(), 0, P + 8, 16),         # n_members < 1
    ]
    for ptr, M, stride, R in cases:
        assert call(piped, ptr, M, stride, R) == -1, (M, stride, R)
        assert b"tb_sac_evaluate_members" in piped.L.tb_last_error()
    for r, ln in ((None, length), (ret, None)):
        assert call(piped, wide.data_ptr(), 3, P + 8, 16, r, ln) == -1 and b"tb_sac_evaluate_members" in piped.L.tb_last_error()
    # a malformed TbSacEvalTrace
    rc, r2, l2, body, _ = raw_call(torch, piped, wide.data_ptr(), 3, P + 8, 16, 26, struct_size=8)
    err = piped.L.tb_last_error()
    assert rc == -1 and b"tb_sac_evaluate_members" in err and b"struct_size" in err
    assert all(bool((body[k] == 0x5A).all()) for k in body) and not bool(r2.any()) and not bool(l2.any())
    rc, r2, l2, body, _ = raw_call(torch, piped, wide.data_ptr(), 3, P + 8, 16, 26, null="actions")
    assert rc == -1 and b"tb_sac_evaluate_members" in piped.L.tb_last_error()
    assert all(bool((body[k] == 0x5A).all()) for k in body) and not bool(r2.any()) and not bool(l2.any())
    w1, d1 = piped.get_state_words()
    assert torch.equal(w0, w1) and torch.equal(d0, d1) and piped.phase() == 0 and piped.counters() == c0
    # SwingRacket without the pipeline: TB_E_UNSUPPORTED
    plain.reset()
    p0, q0 = plain.get_state_words()
    assert call(plain, wide.data_ptr(), 3, P + 8, 16) == -4 and b"tb_sac_evaluate_members" in plain.L.tb_last_error()
    with pytest.raises(StepperError, match="tb_set_pipeline"):
        plain.sac_evaluate_members(w, 16)
    p1, q1 = plain.get_state_words()
    assert torch.equal(p0, p1) and torch.equal(q0, q1)
    # the Python side refuses before the library is asked
    with pytest.raises(ValueError, match="granule"):
        piped.sac_evaluate_members(w, 24)
    with pytest.raises(ValueError):
        piped.sac_evaluate_members(w[:2], 16)
    with pytest.raises(ValueError):
        piped.sac_evaluate_members(w[:, :-4], 16)
    torch.cuda.synchronize()
    assert float(ret.abs().sum()) == 0.0 and int(length.abs().sum()) == 0   # nothing was written
    w1, d1 = piped.get_state_words()
    assert torch.equal(w0, w1) and torch.equal(d0, d1)
    # ... and the handle still evaluates; a misaligned non-contiguous view is re-packed, not refused
    r, ln = piped.sac_evaluate_members(w, 16, seed=NOISE_SEED)
    assert bool((ln == 26).all()) and tuple(r.shape) == (3, 16)
    fresh = make_env(ENV_SWING, n, case_params(), True)
    fresh.reset()                                                  # (piped was reset once before its first evaluation)
    buf = torch.full((3 * (P + 4) + 1,), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[1:].view(3, P + 4)[:, :P + 3]                       # rows of P + 3 floats, P + 4 apart, at base + 4 bytes
    view[:, :P] = w
    assert view.data_ptr() % 16 == 4 and not view.is_contiguous()
    r2, ln2 = fresh.sac_evaluate_members(view, 16, seed=NOISE_SEED)
    torch.cuda.synchronize()
    assert same(torch, r, r2) and torch.equal(ln, ln2)
    for e in (piped, plain, fresh):
        e.close()


def test_rank_checkpoints_ranks_saved_actors_as_a_direct_call_does(torch, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rank_checkpoints as rc
    from tennisbot_rl_amd.evaluation import EVAL_ENV_ID_BASE
    from tennisbot_rl_amd.stepper import BatchedEnv
    kind, seed, R = ENV_SWING, 3, 16
    names = ["rl_model_1000_steps.pt", "rl_model_2000_steps.pt", "best_model.pt"]
    paths = [str(tmp_path / f) for f in names]
    for m, p in enumerate(paths):
        torch.save({"actor": member_state_dict(torch, kind, m), "timesteps": 1000 * (m + 1)}, p)
    rows = rc.main(["-s", "sac", "--env", "SwingRacket-v0", "--episodes-per-member", str(R), "--seed", str(seed)] + paths)
    out = capsys.readouterr().out
    env = BatchedEnv(kind, 3 * R, device=DEV, seed=seed, env_id_base=EVAL_ENV_ID_BASE, track_terminal_obs=False, pipeline=True)
    ret, length = env.sac_evaluate_members(member_actors(torch, kind), R, seed=rc.tournament_noise_seed(seed))
    torch.cuda.synchronize()
    env.close()
    mean, sem, mean_len = torch.stack([ret.mean(1), ret.std(1, unbiased=True) / R ** 0.5, length.double().mean(1)]).cpu().tolist()   # (the tool's reductions)
    print(out, mean, sem)
    assert len(rows) == 3 and sorted(r["checkpoint"] for r in rows) == sorted(paths)
    assert [r["mean"] for r in rows] == sorted((r["mean"] for r in rows), reverse=True)
    for r in rows:
        m = paths.index(r["checkpoint"])
        assert r["episodes"] == R and r["mean"] == mean[m] and r["sem"] == sem[m] and r["mean_length"] == mean_len[m] == 26.0
    table = [ln for ln in out.splitlines() if ln.strip().endswith(".pt")]
    assert len(table) == 3 and [ln.split()[-1] for ln in table] == [r["checkpoint"] for r in rows]
    assert [int(ln.split()[0]) for ln in table] == [1, 2, 3]
    assert "3 checkpoints x 16 episodes of SwingRacket-v0 (sac, stochastic)" in out and "members see DIFFERENT episodes" in out
