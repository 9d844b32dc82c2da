"""One minibatch step of a population in three launches (tb_ppo_grad_members + tb_ppo_apply_members; the member axis of
csrc/tb_learner.hpp) on a real MI355X. The yardstick is the single-member pair: given member m's index row, parameter, moment rows
and its four scalars, tb_ppo_grad_net + tb_ppo_apply_net(TB_PPO_REDUCE | TB_PPO_STEP, world = 1) must leave the same bits in that
member's gradient, parameter, moment and statistics rows. Rows are seeded valid rows (population_fixtures.learner_rows); moments
are non-zero, step = 2, the hyper-parameter rows and the permutations are distinct, and every row is NaN-padded to P + 4."""
import numpy as np
import pytest

import population_fixtures as fx
from tennisbot_rl_amd.params import NET_DEFAULT

pytestmark = pytest.mark.gpu

N_ROWS, M, STEP, PAD = 1200, 3, 2, 4
HP = [[0.2, 0.5, 0.002, 3e-4], [0.1, 0.7, 0.01, 1e-3], [0.3, 0.25, 0.0, 1e-4]]   # clip_range, vf_coef, ent_coef, lr
MAX_NORM, BETA1, BETA2, EPS = 0.5, 0.9, 0.999, 1e-5
CASES = [(k, n, b) for (k, n) in fx.PAIRS for b in ((2, 255, 257, 600) if n == NET_DEFAULT else (257, 600))]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_ROWS = {}


def device_rows(torch, kind):
    if kind not in _ROWS:
        _ROWS[kind] = tuple(torch.from_numpy(x).to("cuda:0") for x in fx.learner_rows(kind, N_ROWS))
    return _ROWS[kind]


def member_state(torch, kind, net, P):
    """params, exp_avg, exp_avg_sq [M, P] on the GPU: the fixtures' members plus a seeded perturbation of every parameter; seeded
    non-zero moments (exp_avg_sq positive)"""
    from tennisbot_rl_amd.population import policy_flat
    g = torch.Generator().manual_seed(41 + 7 * kind + net)
    flat = torch.stack([policy_flat(p) for p in fx.member_policies(torch, kind, net)[:M]])
    assert flat.shape == (M, P)
    flat = flat + 0.02 * torch.randn(flat.shape, generator=g)
    m1 = 1e-3 * torch.randn(flat.shape, generator=g)
    m2 = 1e-6 * torch.rand(flat.shape, generator=g) + 1e-8
    return tuple(x.to("cuda:0") for x in (flat, m1, m2))


def padded_rows(torch, x):
    out = torch.full((x.shape[0], x.shape[1] + PAD), float("nan"), dtype=torch.float32, device=x.device)
    out[:, :x.shape[1]] = x
    return out


def run_members(torch, lib, kind, net, batch, rows, idx, state, hp):
    """grad_members + apply_members on NaN-padded copies; returns (params, grad, exp_avg, exp_avg_sq, stats) as [M, ..] host arrays
    (the padding cut off, after checking that it is still NaN)"""
    P = state[0].shape[1]
    params, m1, m2 = (padded_rows(torch, x) for x in state)
    grad = padded_rows(torch, torch.zeros_like(state[0]))
    stats = torch.zeros((M, 3), dtype=torch.float32, device="cuda:0")
    hp_dev = torch.tensor(hp, dtype=torch.float32, device="cuda:0")
    stride = lib.tb_ppo_members_workspace_stride_bytes(kind, net, batch)
    ws = torch.zeros(M * stride // 8, dtype=torch.float64, device="cuda:0")
    obs, act, old_logp, adv, ret = rows
    rc = lib.tb_ppo_grad_members(kind, net, 0, None, obs.data_ptr(), act.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), ret.data_ptr(), N_ROWS, idx.data_ptr(),
                                 idx.stride(0), batch, M, params.data_ptr(), P + PAD, P, hp_dev.data_ptr(), ws.data_ptr(), ws.numel() * 8)
    assert rc == 0, lib.tb_last_error()
    rc = lib.tb_ppo_apply_members(kind, net, 0, None, ws.data_ptr(), ws.numel() * 8, batch, M, params.data_ptr(), grad.data_ptr(), m1.data_ptr(), m2.data_ptr(), P + PAD, P,
                                  stats.data_ptr(), hp_dev.data_ptr(), MAX_NORM, BETA1, BETA2, EPS, STEP)
    assert rc == 0, lib.tb_last_error()
    torch.cuda.synchronize()
    for x in (params, grad, m1, m2):
        assert bool(torch.isnan(x[:, P:]).all()), "the floats between rows were written"
    return [x[:, :P].cpu().numpy() for x in (params, grad, m1, m2)] + [stats.cpu().numpy()]


def run_single(torch, lib, kind, net, batch, rows, idx_row, state_m, hp_m):
    """the single-member pair on copies of member m's inputs"""
    P = state_m[0].numel()
    params, m1, m2 = (x.clone().contiguous() for x in state_m)
    grad, stats = torch.zeros(P, dtype=torch.float32, device="cuda:0"), torch.zeros(3, dtype=torch.float32, device="cuda:0")
    idx = idx_row[:batch].clone().contiguous()
    nbytes = lib.tb_ppo_workspace_bytes_net(kind, net, batch)
    ws = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device="cuda:0")
    obs, act, old_logp, adv, ret = rows
    clip, vf, ent, lr = hp_m
    rc = lib.tb_ppo_grad_net(kind, net, 0, None, obs.data_ptr(), act.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), ret.data_ptr(), N_ROWS, idx.data_ptr(), batch,
                             params.data_ptr(), P, clip, vf, ws.data_ptr(), ws.numel() * 8)
    assert rc == 0, lib.tb_last_error()
    rc = lib.tb_ppo_apply_net(kind, net, 0, None, 1 | 2, ws.data_ptr(), ws.numel() * 8, batch, params.data_ptr(), grad.data_ptr(), m1.data_ptr(), m2.data_ptr(), P,
                              stats.data_ptr(), ent, MAX_NORM, 1, lr, BETA1, BETA2, EPS, STEP)
    assert rc == 0, lib.tb_last_error()
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (params, grad, m1, m2, stats)]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("kind,net,batch", CASES)
def test_every_members_rows_are_the_single_member_pairs_bit_for_bit(torch, kind, net, batch):
    from tennisbot_rl_amd.stepper import load_library
    lib = load_library()
    P = lib.tb_ppo_param_floats_net(kind, net)
    rows, state = device_rows(torch, kind), member_state(torch, kind, net, P)
    g = torch.Generator().manual_seed(100 + batch)
    idx = torch.stack([torch.randperm(N_ROWS, generator=g) for _ in range(M)])[:, :batch + 5].contiguous().to("cuda:0")   # rows batch + 5 apart
    assert not torch.equal(idx[0], idx[1]) and not torch.equal(idx[1], idx[2])
    got = run_members(torch, lib, kind, net, batch, rows, idx, state, HP)
    for m in range(M):
        want = run_single(torch, lib, kind, net, batch, rows, idx[m], tuple(x[m] for x in state), HP[m])
        for name, g_, w_ in zip(("params", "grad", "exp_avg", "exp_avg_sq", "stats"), got, want):
            assert np.all(np.isfinite(w_)), (m, name)
            assert np.array_equal(bits(g_[m]), bits(w_)), (m, name, float(np.abs(g_[m] - w_).max()))
        assert np.any(want[0] != state[0][m].cpu().numpy()) and np.any(want[1] != 0.0)      # the step moved the parameters
    # the test can see a wrong hyper-parameter row: member 1 computed with member 0's differs
    wrong = run_single(torch, lib, kind, net, batch, rows, idx[1], tuple(x[1] for x in state), HP[0])
    assert not np.array_equal(bits(wrong[0]), bits(got[0][1])) and not np.array_equal(bits(wrong[1]), bits(got[1][1]))
    # the same call twice gives the same bits
    again = run_members(torch, lib, kind, net, batch, rows, idx, state, HP)
    for g_, a_ in zip(got, again):
        assert np.array_equal(bits(g_), bits(a_))
