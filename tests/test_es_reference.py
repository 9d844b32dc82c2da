"""CPU checks of the evolution-strategies path (tennisbot_rl_amd/es.py) against the float64 restatement of tests/es_reference.py:
the GatedCNN module and its parameter order, the streaming form of the network, the shipped ES policy fixture, and the
generation's update -- elite order with ties and NaN, the two defined deviations, the lr / sigma schedule, the mean over repeats."""
import hashlib
import os

import numpy as np
import pytest
import torch

import es_reference as er
from tennisbot_rl_amd import es
from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, OBS_DIM

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "es_swing_policy.npz")
KINDS = (ENV_SWING, ENV_TENNIS)


def _weights(kind, scale, seed):
    O, A = OBS_DIM[kind], ACT_DIM[kind]
    return np.random.default_rng(seed).normal(0.0, scale, er.es_floats(O, A)).astype(np.float32)


@pytest.mark.parametrize("kind", KINDS)
def test_parameter_count_and_order(kind):
    O, A = OBS_DIM[kind], ACT_DIM[kind]
    assert es.es_floats(O, A) == er.es_floats(O, A) == {ENV_SWING: 766, ENV_TENNIS: 858}[kind]
    net = es.GatedCNN(O, A)
    names = [n for n, _ in net.named_parameters()]
    assert names == ["conv_0.weight", "conv_0.bias", "conv_gate_0.weight", "conv_gate_0.bias", "conv_1.weight", "conv_1.bias",
                     "conv_gate_1.weight", "conv_gate_1.bias", "conv_2.weight", "conv_2.bias"]
    w = net.get_weights().numpy()
    assert w.shape == (er.es_floats(O, A),)
    p = er.unpack(w, O, A)
    for n, t in net.named_parameters():
        assert np.array_equal(p[n], t.detach().double().numpy()), n
    assert len(es.initial_weights(kind, 3)) == w.shape[0]
    assert torch.equal(es.initial_weights(kind, 3), es.initial_weights(kind, 3))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("scale", (0.3, 2.0))
def test_restatement_matches_module(kind, scale):
    O, A = OBS_DIM[kind], ACT_DIM[kind]
    w = _weights(kind, scale, 1)
    net = es.GatedCNN(O, A).set_weights(torch.from_numpy(w)).double()
    X = np.random.default_rng(2).normal(0.0, 1.5, (64, 8, O)).astype(np.float32)
    got = net(torch.from_numpy(X).double().transpose(-1, -2)).detach().numpy()  # the module takes channels x time
    want = er.forward_window(er.unpack(w, O, A), X)
    assert got.shape == (64, A)
    assert np.max(np.abs(got - want)) <= 1e-12


@pytest.mark.parametrize("kind", KINDS)
def test_streaming_equals_window_bit_for_bit(kind):
    O, A = OBS_DIM[kind], ACT_DIM[kind]
    p = er.unpack(_weights(kind, 0.5, 4), O, A)
    rows = np.random.default_rng(5).normal(0.0, 1.0, (30, 16, O)).astype(np.float32)
    stream = er.forward_streaming(p, rows)
    window = er.forward_window(p, er.windows(rows))
    assert stream.shape == window.shape == (30, 16, A)
    assert np.array_equal(stream.view(np.uint64), window.view(np.uint64))


def test_window_of_first_step_repeats_x0():
    rows = np.arange(3 * 2 * 6, dtype=np.float32).reshape(3, 2, 6)
    W = er.windows(rows)
    assert W.shape == (3, 2, 8, 6)
    assert np.array_equal(W[0], np.repeat(rows[0][:, None, :], 8, axis=1))
    assert np.array_equal(W[2][:, -1], rows[2]) and np.array_equal(W[2][:, -3], rows[0])


def test_normaliser_first_row_is_zero_and_nan_kept():
    obs = np.random.default_rng(6).normal(0.0, 3.0, (5, 4, 6)).astype(np.float32)
    rows = er.normalised_rows(obs)
    assert np.array_equal(rows[0], np.zeros_like(rows[0]))
    obs[2, 1, 3] = np.nan
    rows = er.normalised_rows(obs)
    assert np.isnan(rows[2:, 1, 3]).all() and np.isfinite(rows[:, 0]).all()


def test_golden_es_policy_fixture():
    z = np.load(GOLD, allow_pickle=False)
    w = z["weights"]
    assert w.dtype == np.float32 and w.shape == (766,) and np.isfinite(w).all()
    assert hashlib.sha256(w.astype("<f4").tobytes()).hexdigest() == str(z["sha256"])
    assert str(z["member"]).startswith("SwingRacket-v0__")


def _update_case(p=12, P=30, ties=False, nan=False, seed=0):
    rng = np.random.default_rng(seed)
    w = rng.normal(0.0, 0.5, P).astype(np.float32)
    eps = rng.normal(0.0, 1.0, (p, P)).astype(np.float32)
    r_pos = rng.normal(10.0, 5.0, p).astype(np.float32)
    r_neg = rng.normal(10.0, 5.0, p).astype(np.float32)
    if ties:
        r_pos[[1, 4, 7]] = 3.0
        r_neg[[1, 4, 7]] = 1.0  # three equal differences: index order
        r_pos[9], r_neg[9] = r_pos[2], r_neg[2]
    if nan:
        r_pos[[0, 5]] = np.nan
        r_neg[3] = np.nan
        r_pos[6], r_neg[6] = -np.inf, 0.0  # -inf ranks above NaN
    return w, eps, r_pos, r_neg


@pytest.mark.parametrize("case", ("plain", "ties", "nan"))
@pytest.mark.parametrize("k", (1, 5, 12))
def test_update_matches_numpy(case, k):
    w, eps, r_pos, r_neg = _update_case(ties=case == "ties", nan=case == "nan", seed=k)
    lr = 0.2
    idx_t = es.elite_order(torch.from_numpy(r_pos) - torch.from_numpy(r_neg), k).numpy()
    idx_n = er.elite_order(r_pos - r_neg, k)
    assert np.array_equal(idx_t, idx_n)
    if case == "nan":
        order = er.elite_order(r_pos - r_neg, len(r_pos))
        assert set(order[-3:]) == {0, 3, 5} and order[-4] == 6
    got, info = es.es_update(torch.from_numpy(w), torch.from_numpy(eps), torch.from_numpy(r_pos), torch.from_numpy(r_neg), lr, k)
    want, idx, std, skipped = er.es_update(w, eps, r_pos, r_neg, lr, k)
    assert np.array_equal(info["elite"].numpy(), idx) and bool(info["skipped"]) == skipped
    if np.isnan(std):  # a NaN difference in the elite
        assert np.isnan(float(info["std"]))
    else:
        assert abs(float(info["std"]) - std) <= 1e-6 * max(std, 1.0)
    got = got.numpy()
    if not np.isfinite(want).all():
        assert np.array_equal(np.isnan(got), np.isnan(want))
        return
    # float32 rounding of w + step: the step's dot product of k terms and its scale, relative to their magnitudes
    d = np.abs((r_pos - r_neg)[idx].astype(np.float64))
    mag = np.abs(w) + lr / (std * k) * (np.abs(eps[idx]).T.astype(np.float64) @ d)
    er.assert_within("updated weights", got, want, er.gamma(2 * k + 8) * mag + 1e-30)


def test_update_std_zero_is_skipped():
    w, eps, _, _ = _update_case()
    r = np.full(12, 7.5, np.float32)
    got, info = es.es_update(torch.from_numpy(w), torch.from_numpy(eps), torch.from_numpy(r), torch.from_numpy(r.copy()), 0.2, 5)
    assert bool(info["skipped"]) and float(info["std"]) == 0.0
    assert np.array_equal(got.numpy(), w)  # the reference would write NaN weights here


def test_schedule():
    lr, sigma = 0.2, 0.1
    for _ in range(3000):
        lr2, sigma2 = es.schedule(lr, sigma, 0.995)
        assert lr2 == (lr * 0.995 if lr > 0.001 else lr) and sigma2 == (sigma * 0.999 if sigma > 0.01 else sigma)
        lr, sigma = lr2, sigma2
    assert 0.00099 < lr <= 0.001 and 0.00999 < sigma <= 0.01


def test_fitness_is_float32_mean_of_repeats():
    ret = np.random.default_rng(8).normal(20.0, 9.0, (40, 10))
    got = es.fitness(torch.from_numpy(ret)).numpy()
    want = ret.mean(axis=1).astype(np.float32)
    assert got.dtype == np.float32
    assert np.max(np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want))) <= 1.0


def test_pack_population_layout():
    P, p = 766, 3
    w = torch.randn(P)
    eps = torch.randn(p, P)
    pop = es.pack_population(w, eps, 0.1)
    assert pop.shape == (2 * p, 768) and pop.dtype == torch.float32
    assert torch.equal(pop[1, :P], w + eps[1] * 0.1) and torch.equal(pop[p + 1, :P], w - eps[1] * 0.1)
    assert torch.count_nonzero(pop[:, P:]) == 0
    with pytest.raises(ValueError):
        es.pack_population(w, eps, 0.1, stride=770)
