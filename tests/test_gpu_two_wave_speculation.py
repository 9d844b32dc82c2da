"""The two-wave step kernel speculates past its common-path gate (tb_kernels.hpp, two_wave_step): the racket wave integrates before the
ball wave's verdict on the geometric tests is in, and a launch whose 64 envs are not all on the common path is stepped from the loaded
state by the one-wave code. Each case puts ONE rare lane among 63 common ones (or a non-finite value on one wave's side) into some
workgroups in the middle of the short steps, then runs on through the parking step. The two-wave form (TbOptions.step_waves = 2) is
compared with the float32 oracle bit for bit -- state words, done byte, obs, reward, done, counters (substeps and the non-finite
count among them) -- and with the one-wave form (step_waves = 1) of the same kernel, which must agree to the last bit of every NaN."""
import numpy as np
import pytest

from oracle import OracleBatch
from tennisbot_rl_amd.params import ENV_SWING, F_AUTO_RESET, F_DEFAULT, default_params

pytestmark = pytest.mark.gpu

ROW_RP, ROW_RV, ROW_BP, ROW_BV, ROW_STEP = 0, 7, 13, 16, 28
DONE_PENDING_FORCE, DONE_YES = 1, 2


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def same(a, b, what, nan_equal=False):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        ok = a.view(np.uint32) == b.view(np.uint32)
        if nan_equal:  # the oracle's NaN payloads are the host's
            ok |= np.isnan(a) & np.isnan(b)
    else:
        ok = a == b
    if not ok.all():
        bad = np.argwhere(~ok)
        raise AssertionError("%s: %d mismatches, first at %s" % (what, len(bad), bad[0]))


def put_ball_on_racket(f, d, k):  # the ball's centre on the racket's: past the slab test
    f[ROW_BP:ROW_BP + 3, k] = f[ROW_RP:ROW_RP + 3, k]


def put_ball_near_court(f, d, k):  # under the highest static shape's top: the static-height test
    f[ROW_BP + 2, k] = np.float32(0.05)


def make_last_short_step(f, d, k):  # step_count 25: this step parks the env
    f.view(np.int32)[ROW_STEP, k] = 25


def make_done(f, d, k):
    d[k] = DONE_YES


def make_pending_force(f, d, k):
    d[k] = DONE_PENDING_FORCE


def poison_racket(f, d, k):  # a non-finite value on the racket wave's side
    f[ROW_RV, k] = np.float32(np.inf)


def poison_ball(f, d, k):  # ... and on the ball wave's (its position stays finite: the gate passes it)
    f[ROW_BV + 1, k] = np.float32(-np.inf)


def lockstep(torch, n, seed, edit, edit_at=12, steps=30):
    """n envs, both forms and the oracle from one seed; at step edit_at, `edit` is applied to one env in each of a few workgroups
    (a different lane in each); then on through the parking step (step 26) and a few steps of the next episode"""
    from tennisbot_rl_amd.stepper import BatchedEnv
    p = default_params(flags=F_DEFAULT)
    envs = [BatchedEnv(ENV_SWING, n, device="cuda:0", seed=seed, params=p, pipeline=True, track_terminal_obs=False, options=dict(step_waves=w))
            for w in (2, 1)]
    assert [e.step_waves() for e in envs] == [2, 1]
    pf = p.copy(); pf.flags |= F_AUTO_RESET
    ref = OracleBatch(pf, ENV_SWING, n, seed=seed, precision="f32")
    ref.L.tbo_set_threads(ref.h, 8)
    rng = np.random.default_rng(seed)
    o_ref = ref.reset()
    for e in envs:
        same(e.reset().cpu().numpy(), o_ref, "reset obs")
    groups = (n + 63) // 64
    lanes = [g * 64 + (g * 37) % 64 for g in range(0, groups - 1, 3)] + [n - 1]  # the last (maybe ragged) workgroup's last lane too
    nan_equal = edit in (poison_racket, poison_ball)
    rewards = []
    for t in range(steps):
        if t == edit_at:
            w, d = envs[0].get_state_words()
            w = w.cpu().numpy().view(np.uint32).copy(); d = d.cpu().numpy().copy()
            f = w.view(np.float32)
            for k in lanes:
                edit(f, d, k)
            for e in envs:
                e.set_state_words(w.view(np.int32), d)
            ref.set_state_words(w, d)
        a = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
        outs = [e.step(torch.from_numpy(a).cuda()) for e in envs]
        o2, r2, d2, s2 = ref.step(a)
        (obs, rew, done), (obs1, rew1, done1) = outs
        same(obs.cpu().numpy(), o2, "n=%d step %d obs" % (n, t), nan_equal)
        same(done.cpu().numpy(), d2, "n=%d step %d done" % (n, t))
        same(obs.cpu().numpy(), obs1.cpu().numpy(), "n=%d step %d obs, one-wave form" % (n, t))
        same(done.cpu().numpy(), done1.cpu().numpy(), "n=%d step %d done, one-wave form" % (n, t))
        rewards.append((rew, rew1, r2))  # the terminal rewards arrive with the pool's fast-forward at the join
    for e in envs:
        e.flush()
    for t, (rew, rew1, r2) in enumerate(rewards):
        same(rew.cpu().numpy(), r2, "n=%d step %d reward" % (n, t), nan_equal)
        same(rew.cpu().numpy(), rew1.cpu().numpy(), "n=%d step %d reward, one-wave form" % (n, t))
    w2, d2 = envs[0].get_state_words()
    w1, d1 = envs[1].get_state_words()
    wr, dr = ref.get_state_words()
    w2 = w2.cpu().numpy().view(np.uint32)
    same(w2[:-2].view(np.float32), wr[:-2].view(np.float32), "n=%d state words" % n, nan_equal)
    same(w2[-2:], wr[-2:].view(np.uint32), "n=%d step count, episode" % n)
    same(d2.cpu().numpy(), dr, "n=%d done byte" % n)
    same(w2, w1.cpu().numpy().view(np.uint32), "n=%d state words, one-wave form" % n)
    same(d2.cpu().numpy(), d1.cpu().numpy(), "n=%d done byte, one-wave form" % n)
    got, want = envs[0].counters(), ref.counters()
    assert list(got.values()) == [int(x) for x in want], (got, want)
    assert got == envs[1].counters()
    for e in envs:
        e.close()
    return got, len(lanes)


@pytest.mark.parametrize("edit", [put_ball_on_racket, put_ball_near_court, make_last_short_step, make_done, make_pending_force],
                         ids=lambda f: f.__name__)
def test_one_rare_lane_among_common_ones(torch, edit):
    lockstep(torch, 4096, 300, edit)


@pytest.mark.parametrize("edit", [put_ball_on_racket, make_last_short_step], ids=lambda f: f.__name__)
def test_ragged_final_workgroup(torch, edit):
    lockstep(torch, 1000, 301, edit)
    lockstep(torch, 4096 + 17, 302, edit, edit_at=3)


@pytest.mark.parametrize("edit", [poison_racket, poison_ball], ids=lambda f: f.__name__)
def test_non_finite_state_on_either_wave(torch, edit):
    got, k = lockstep(torch, 3000, 303, edit, steps=20)
    assert got["nonfinite_states"] >= k


def test_parking_step_with_every_lane_rare(torch):
    """no edit: step 26 of every episode is the parking step (every lane fails the cheap first test), twice over"""
    lockstep(torch, 4096, 304, lambda f, d, k: None, steps=26 * 2 + 3)
