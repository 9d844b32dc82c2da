"""tb_swing_trace on the device, bit for bit against the float32 oracle (tests/trace_reference.py cuts copies of each env's step at
every sampled substep) and against the product's own step.

The batches are trace_reference.mixed_batch's: the four hand-built flights (goal hit, 800-limit, court contact, a moving ball's goal
hit), flights after 25 random steps -- some with a racket contact in them -- and, in the same waves, rows that start no flight (step
counts 0, 10 and 24, with the contact bonus where it is due) and rows that enter with a non-zero done byte. test_trace_reference.py
asserts those properties on the oracle, without a GPU; here one case repeats the assertion on the batch it traces."""
import numpy as np
import pytest

import trace_reference as tr
from helpers import same_bits
from tennisbot_rl_amd.params import COUNTER_NAMES, ENV_SWING, ENV_TENNIS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_ROWS = (1, 5, 64, 65, 130)
STRIDES = (1, 7, 8, 775, 10000)
SETS = list(tr.param_sets())


def ample(stride):
    return 2 + 775 // stride


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_cache = {}


def batch(name):
    """(params, words, done, actions, TraceOracle) of a parameter set's 130-row batch, built once"""
    if name not in _cache:
        params, seed = tr.param_sets()[name]
        words, done, actions = tr.mixed_batch(params, seed)
        _cache[name] = (params, words, done, actions, tr.TraceOracle(params, words, done, actions), {})
    return _cache[name][:5]


def reference_frames(name, stride, F):
    refs = _cache[name][5]
    if (stride, F) not in refs:
        refs[(stride, F)] = _cache[name][4].frames(stride, F)
    return refs[(stride, F)]


@pytest.fixture(scope="module")
def envs(torch):
    """one small handle per parameter set, auto-reset on: the trace takes parameters, outline table and device from it, nothing else"""
    from tennisbot_rl_amd.stepper import BatchedEnv
    made = {}

    def get(name):
        if name not in made:
            made[name] = BatchedEnv(ENV_SWING, 7, device=DEV, seed=9, params=batch(name)[0])
            made[name].reset()
        return made[name]
    yield get
    for e in made.values():
        e.close()


def dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def run_trace(torch, env, words, done, actions, stride, F):
    out = env.trace_step(dev(torch, actions), stride=stride, words=dev(torch, words), done=dev(torch, done), max_frames=F)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_outputs(got, o, n):
    assert np.array_equal(got["substeps"], o.substeps[:n]) and np.array_equal(got["done"], o.done[:n])
    assert same_bits(got["reward"], o.reward[:n]) and same_bits(got["obs"], o.obs[:n])


@pytest.mark.parametrize("n", N_ROWS)
@pytest.mark.parametrize("name", SETS)
def test_every_stored_row_is_the_oracles(torch, envs, name, n):
    params, words, done, actions, o = batch(name)
    env = envs(name)
    for stride in STRIDES:
        for F in (1, 2, 3, ample(stride)):
            got = run_trace(torch, env, words[:, :n], done[:n], actions[:n], stride, F)
            fr, nf, steps = reference_frames(name, stride, F)
            check_outputs(got, o, n)
            assert np.array_equal(got["n_frames"], nf[:n]), (stride, F)
            frames = got["frames"].view(np.uint32)
            assert frames.shape == (F, tr.W, n)
            bad = np.argwhere(frames != fr[:, :, :n])
            assert bad.size == 0, "stride %d, max_frames %d: first differing (row, word, env) %s of %d" % (stride, F, bad[0], len(bad))
            # stated on the trace's own output as well: unstored rows equal the final row, which is the last one
            final = steps[:, :n] == o.substeps[None, :n]   # [F, n]
            by_env = frames.transpose(0, 2, 1)             # [F, n, W]
            assert final[-1].all() and np.array_equal(by_env[final], np.broadcast_to(by_env[-1], by_env.shape)[final])


def test_the_traced_batch_holds_every_case(torch, envs):
    """a flight with a racket contact in it, each ending, a contact bonus, done rows, and flights beside non-flights in one wave"""
    params, words, done, actions, o = batch("default")
    got = run_trace(torch, envs("default"), words, done, actions, 8, ample(8))
    c = dict(zip(COUNTER_NAMES, o.counters))
    assert o.flight_contact_substeps() > 0 and c["ball_court_terminations"] > 0 and c["goal_hits"] > 0 and c["timeouts"] > 0
    flight = got["substeps"] > 1
    assert flight[:64].any() and (~flight[:64]).any() and flight[64:].any() and (~flight[64:]).any()
    assert (got["n_frames"][~flight] == 1).all() and (got["reward"][~flight] == 2.0).sum() >= 2
    step0 = words[tr.ROW_STEP].view(np.int32)
    assert set(step0[~flight & (done == 0)]) == {0, 10, 24} and sorted(done[done != 0]) == [1, 2]
    assert got["substeps"].max() == 776 and got["n_frames"].max() == 98 and (got["reward"] == 70.0).any()


@pytest.mark.parametrize("name", ["default", "racket_ground_rolling"])
def test_against_the_products_own_step(torch, envs, name):
    from tennisbot_rl_amd.stepper import BatchedEnv
    params, words, done, actions, o = batch(name)
    n = 130
    got = run_trace(torch, envs(name), words, done, actions, 8, ample(8))
    check_outputs(got, o, n)
    last = got["frames"][-1]
    for auto_reset in (True, False):
        env = BatchedEnv(ENV_SWING, n, device=DEV, seed=4, params=params, auto_reset=auto_reset)
        env.reset()
        env.set_state_words(words, done)
        obs, rew, d = env.step(dev(torch, actions))
        sub = env.last_substeps()
        torch.cuda.synchronize()
        obs, rew, d, sub = obs.cpu().numpy(), rew.cpu().numpy(), d.cpu().numpy(), sub.cpu().numpy()
        state = env.get_state_words()[0].cpu().numpy()
        assert same_bits(rew, got["reward"]) and np.array_equal(sub, got["substeps"]) and np.array_equal(d, got["done"])
        if auto_reset:
            term = env.terminal_obs().cpu().numpy()
            ended = d != 0
            assert ended.any() and (~ended).any()
            assert same_bits(term[ended], got["obs"][ended]) and same_bits(obs[~ended], got["obs"][~ended])
            assert np.array_equal(state[:, ~ended], last[:, ~ended])   # where it did not reset
        else:
            assert same_bits(obs, got["obs"]) and np.array_equal(state, last)
            # the env's own state, words=None: the same trace, and the env is where it was
            env.set_state_words(words, done)
            own = env.trace_step(dev(torch, actions), stride=8)
            torch.cuda.synchronize()
            for k in got:
                assert np.array_equal(own[k].cpu().numpy().view(np.uint8), got[k].view(np.uint8)), k
            w2, d2 = env.get_state_words()
            assert np.array_equal(w2.cpu().numpy().view(np.uint32), words) and np.array_equal(d2.cpu().numpy(), done)
        env.close()


def test_the_handle_is_untouched(torch):
    """a pipelined handle with 26 steps issued and not flushed, traced in between on foreign words, against a twin never traced"""
    from tennisbot_rl_amd.stepper import BatchedEnv
    params, words, done, actions, o = batch("default")
    n = 256
    rng = np.random.default_rng(5)
    acts = [dev(torch, rng.uniform(-1, 1, (n, 6)).astype(np.float32)) for _ in range(26)]
    res = []
    for traced in (True, False):
        env = BatchedEnv(ENV_SWING, n, device=DEV, seed=3, params=params, pipeline=True)
        env.reset()
        rews, traces = [], []
        for t in range(26):
            rews.append(env.step(acts[t])[1])
            if traced and t in (4, 24, 25):
                traces.append(env.trace_step(dev(torch, actions), stride=8, words=dev(torch, words), done=dev(torch, done)))
        env.flush()
        torch.cuda.synchronize()
        for tr_out in traces:   # and the traces themselves are right, whatever the handle was doing
            check_outputs({k: v.cpu().numpy() for k, v in tr_out.items()}, o, 130)
        res.append(dict(rew=np.stack([r.cpu().numpy() for r in rews]), state=[x.cpu().numpy() for x in env.get_state_words()],
                        counters=env.counters(), phase=env.phase(), sealed=env.sealed_substeps()))
        env.close()
    a, b = res
    assert same_bits(a["rew"], b["rew"]) and all(np.array_equal(x, y) for x, y in zip(a["state"], b["state"]))
    assert a["counters"] == b["counters"] and a["phase"] == b["phase"] == 0 and a["sealed"] == b["sealed"]
    assert a["counters"]["episodes_finished"] == n


def test_a_traced_row_renders_as_the_same_words_uploaded_afresh(torch, envs):
    from tennisbot_rl_amd import stepper
    params, words, done, actions, o = batch("default")
    out = envs("default").trace_step(dev(torch, actions), stride=8, words=dev(torch, words), done=dev(torch, done))
    for k in (0, 5, out["frames"].shape[0] - 1):
        row = out["frames"][k]
        fresh = dev(torch, row.cpu().numpy())
        for cam in (stepper.court_camera(), stepper.default_camera(ENV_SWING)):
            a = stepper.render_words(ENV_SWING, params, row, camera=cam, width=32, height=24, layers=True)
            b = stepper.render_words(ENV_SWING, params, fresh, camera=cam, width=32, height=24, layers=True)
            torch.cuda.synchronize()
            for x, y in zip(a, b):
                assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
            assert bool((a[1] != 0).any())   # a picture of the court, not of the sky alone


def test_refusals_write_nothing(torch, envs):
    from tennisbot_rl_amd.stepper import BatchedEnv
    params, words, done, actions, o = batch("default")
    env, n, F = envs("default"), 5, 4
    L = env.L
    w, d, a = dev(torch, words[:, :n]), dev(torch, done[:n]), dev(torch, actions[:n])
    fill = lambda *shape: torch.full(shape, 0x5A, dtype=torch.uint8, device=DEV)  # noqa: E731
    outs = dict(frames=fill(F * tr.W * n * 4 + 8), n_frames=fill(n * 4), reward=fill(n * 4), substeps=fill(n * 4), done=fill(n), obs=fill(n * 24))

    def call(h=env._h, n_rows=n, stride=8, max_frames=F, frames_off=0, **null):
        ptr = {k: (None if k in null else v.data_ptr()) for k, v in outs.items()}
        return L.tb_swing_trace(h, w.data_ptr(), d.data_ptr(), n_rows, a.data_ptr(), stride, max_frames, ptr["frames"] + frames_off, ptr["n_frames"],
                                ptr["reward"], ptr["substeps"], ptr["done"], ptr["obs"], env._stream())

    tennis = BatchedEnv(ENV_TENNIS, 4, device=DEV)
    cases = [(dict(stride=0), ">= 1"), (dict(max_frames=0), ">= 1"), (dict(n_rows=0), ">= 1"), (dict(stride=-3), ">= 1"),
             (dict(frames_off=2), "aligned"), (dict(reward=None), "null argument"), (dict(h=tennis._h), "SwingRacket-v0")]
    for kw, text in cases:
        assert call(**kw) == -1, kw   # TB_E_INVAL
        msg = L.tb_last_error().decode()
        assert msg.startswith("tb_swing_trace:") and text in msg, (kw, msg)
    torch.cuda.synchronize()
    tennis.close()
    for k, v in outs.items():
        assert bool((v == 0x5A).all()), "a refused call wrote %s" % k
    assert call() == 0   # and the same buffers take a good call: every byte of the frames is written
    torch.cuda.synchronize()
    fr = outs["frames"][:F * tr.W * n * 4].cpu().numpy().view(np.uint32).reshape(F, tr.W, n)
    assert np.array_equal(fr, tr.TraceOracle(params, words[:, :n], done[:n], actions[:n]).frames(8, F)[0])
    assert bool((outs["frames"][F * tr.W * n * 4:] == 0x5A).all())   # and none beyond them
