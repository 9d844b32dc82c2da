"""The fused ES evaluation (tb_es_evaluate, csrc/tb_es.hpp) on the GPU, from its trace, against the CPU oracle, the env's own
step path and the float64 restatement of tests/es_reference.py:
  * the first observation is the oracle's reset of episode 0 (a fresh handle's first call evaluates episode 0);
  * replaying the traced actions through BatchedEnv.step from the same reset gives obs / reward / done bit for bit;
  * net_in is the float64 normaliser of the traced observations rounded to float32, bit for bit;
  * raw actions are within twice the forward error bound of the float64 GatedCNN on the traced rows, actions are the clip of raw
    bit for bit (NaN kept);
  * the return is the float64 sum of the traced rewards through the first done, bit for bit, and the length is that step + 1;
  * the return does not depend on the trace, on the SwingRacket fast-forward form or on the run."""
import numpy as np
import pytest

import es_reference as er
from helpers import check_es_trace, es_evaluate, es_member_weights, es_params, same_bits
from tennisbot_rl_amd.params import ENV_SWING, ENV_TENNIS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


member_weights = es_member_weights


def make_params(rg):
    return es_params(rg)


def evaluate(torch, kind, n, epm, W, rg=False, ff=None, trace=True, seed=5):
    return es_evaluate(torch, kind, n, epm, W, make_params(rg), ff=ff, trace=trace, seed=seed)


def check_trace(torch, kind, n, epm, W, ret, length, tr, rg, seed=5):
    check_es_trace(torch, kind, n, epm, W, ret, length, tr, make_params(rg), seed=seed)


CASES = [
    # kind, n, envs per member, weights, racket-ground
    (ENV_SWING, 200, 10, "default", False),
    (ENV_SWING, 130, 1, "golden", False),
    (ENV_SWING, 192, 64, "saturating", False),
    (ENV_SWING, 90, 10, "zero", False),
    (ENV_SWING, 70, 7, "nan", False),
    (ENV_SWING, 100, 10, "golden", True),
    (ENV_TENNIS, 200, 10, "default", False),
    (ENV_TENNIS, 65, 1, "saturating", False),
    (ENV_TENNIS, 128, 64, "zero", False),
    (ENV_TENNIS, 77, 11, "nan", False),
    (ENV_TENNIS, 60, 10, "default", True),
]


@pytest.mark.parametrize("kind,n,epm,wset,rg", CASES)
def test_es_trace(torch, kind, n, epm, wset, rg):
    W = member_weights(kind, wset, n // epm)
    ret, length, tr = evaluate(torch, kind, n, epm, W, rg=rg)
    check_trace(torch, kind, n, epm, W, ret, length, tr, rg)
    if wset == "nan":
        assert np.isnan(tr["raw"][0, epm:2 * epm]).all()  # member 1's envs act NaN from the first step
    ret2, length2 = evaluate(torch, kind, n, epm, W, rg=rg, trace=False)
    assert same_bits(ret, ret2) and np.array_equal(length, length2), "the trace changed a result"


@pytest.mark.parametrize("rg", (False, True))
def test_swing_fast_forward_forms_agree(torch, rg):
    W = member_weights(ENV_SWING, "golden", 20)
    a = evaluate(torch, ENV_SWING, 200, 10, W, rg=rg, ff="all", trace=False)
    b = evaluate(torch, ENV_SWING, 200, 10, W, rg=rg, ff=False, trace=False)
    assert same_bits(a[0], b[0])


def test_repeatable_and_episode_index(torch):
    """two fresh handles give the same returns; a second call on one handle evaluates the next episode (other spawns)"""
    from tennisbot_rl_amd.stepper import BatchedEnv
    W = member_weights(ENV_TENNIS, "default", 8)
    a = evaluate(torch, ENV_TENNIS, 80, 10, W, trace=False)
    b = evaluate(torch, ENV_TENNIS, 80, 10, W, trace=False)
    assert same_bits(a[0], b[0])
    env = BatchedEnv(ENV_TENNIS, 80, device="cuda:0", seed=5, params=make_params(False))
    pop = torch.zeros((8, 860), device="cuda:0")
    pop[:, :858] = torch.from_numpy(W).to("cuda:0")
    r1 = env.es_evaluate(pop, 10)[0].reshape(-1).cpu().numpy()
    r2, _, tr = env.es_evaluate(pop, 10, trace=True, max_steps=1)
    env.close()
    assert same_bits(r1, a[0])
    from oracle import OracleBatch
    ref = OracleBatch(make_params(False), ENV_TENNIS, 80, seed=5, precision="f32")
    ref.reset()
    assert np.array_equal(tr["obs"][0].cpu().numpy().view(np.uint32), ref.reset().view(np.uint32))  # episode 1


def test_swing_needs_pipeline(torch):
    from tennisbot_rl_amd.stepper import BatchedEnv, StepperError
    env = BatchedEnv(ENV_SWING, 64, device="cuda:0", seed=1)
    with pytest.raises(StepperError, match="tb_set_pipeline"):
        env.es_evaluate(torch.zeros((64, 768), device="cuda:0"), 1)
    env.close()


@pytest.mark.parametrize("env_id", ("SwingRacket-v0", "Tennisbot-v0"))
def test_trainer_generations_match_cpu_update(torch, env_id):
    from tennisbot_rl_amd import es
    tr = es.ESTrainer(env_id, popsize=8, repeats=3, elite=3, seed=2, device="cuda:0")
    for _ in range(3):
        w0, lr0 = tr.w.cpu().numpy(), tr.lr
        info = tr.step()
        fit, eps = info["fitness"].cpu().numpy(), info["eps"].cpu().numpy()
        want, idx, std, skipped = er.es_update(w0, eps, fit[:8], fit[8:], lr0, 3)
        got = tr.w.cpu().numpy()
        assert np.isfinite(got).all()
        assert np.array_equal(info["elite"].cpu().numpy(), idx) and bool(info["skipped"]) == skipped
        d = np.abs((fit[:8] - fit[8:])[idx].astype(np.float64))
        mag = np.abs(w0) + (lr0 / (std * 3) if std else 0.0) * (np.abs(eps[idx]).T.astype(np.float64) @ d)
        er.assert_within("updated weights", got, want, er.gamma(16) * mag + 1e-30)
    log = tr.log()
    assert log["generation"] == 3 and log["steps"] > 0
    r = tr.evaluate(episodes=16).cpu().numpy()
    assert r.shape == (16,) and np.isfinite(r).all()
    tr.close()
