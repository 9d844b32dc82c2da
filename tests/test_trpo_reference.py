"""The TRPO reference (tests/trpo_reference.py) against independent constructions, and what of the product needs no GPU.

  * its Fisher-vector product against torch's float64 double backprop of the KL -- the construction of agent.py:144-167 -- on both
    env architectures, log_std block included;
  * its conjugate gradient against np.linalg.solve on the dense F of a 6 -> 8 -> 8 -> 2 policy;
  * its surrogate gradient against torch autograd of mean(ratio A_hat);
  * the line search's selection (the reference's and the product's device-side select_candidate) on hand-made tables;
  * the host side of the C ABI: the tb_trpo_* symbols, the workspace queries, refusals that need no device.
"""
import ctypes
import math

import numpy as np
import pytest

import trpo_reference as tr
from policy_reference import state_dict_arrays
from test_ppo_reference import flat_shard, make_policy, rollout


def torch_kl(torch, policy, old_mean, old_ls, obs):
    """KL(old || new) of diagonal Gaussians as torch ops: the formula of agent.py:92-97, whose double backprop is agent.py:144-167"""
    mean = policy.action_net(policy.policy_net(obs))
    ls = policy.log_std
    return ((ls - old_ls) + 0.5 * (old_ls.exp() ** 2 + (old_mean - mean) ** 2) / ls.exp() ** 2 - 0.5).sum(1).mean()


def theta_params(policy):
    return [(k, p) for k, p in policy.named_parameters() if tr.is_theta(k)]


@pytest.mark.parametrize("name", ["swing-52-lockstep", "tennis-70-ragged"])
def test_fvp_is_the_double_backprop_hessian_of_the_kl(name):
    import torch
    ro = rollout(name)
    policy = make_policy(ro.arch, ro.kind).double()
    rows = np.random.default_rng(3).permutation(ro.T * ro.n)[:257]
    obs = ro.obs.reshape(ro.T * ro.n, -1)[rows]
    P = state_dict_arrays(policy)
    rng = np.random.default_rng(4)
    v = {k: rng.normal(size=np.shape(w)) for k, w in tr.theta_of(P).items()}
    want = tr.fvp(P, obs, v, damping=0.0)
    x = torch.from_numpy(obs.astype(np.float64))
    with torch.no_grad():
        old_mean, old_ls = policy.action_net(policy.policy_net(x)).clone(), policy.log_std.detach().clone()
    names, params = zip(*theta_params(policy))
    grads = torch.autograd.grad(torch_kl(torch, policy, old_mean, old_ls, x), params, create_graph=True)
    gv = sum((g * torch.from_numpy(v[k])).sum() for k, g in zip(names, grads))
    hv = torch.autograd.grad(gv, params)
    for k, h in zip(names, hv):
        scale = max(np.abs(want[k]).max(), 1e-30)
        assert np.abs(h.numpy() - want[k]).max() <= 1e-11 * scale, k
    assert np.array_equal(want["log_std"], 2.0 * v["log_std"])
    damped = tr.fvp(P, obs, v, damping=0.25)
    for k in want:
        np.testing.assert_allclose(damped[k], want[k] + 0.25 * v[k], rtol=1e-14, atol=0)


def small_policy():
    import torch
    from tennisbot_rl_amd.ppo import build_actor_critic
    torch.manual_seed(2)
    policy = build_actor_critic(6, 2, (8, 8)).double()
    with torch.no_grad():
        policy.action_net.weight.mul_(30.0)
        policy.log_std.copy_(torch.tensor([-0.2, 0.3]))
    return policy


def test_conjugate_gradient_solves_the_dense_system():
    policy = small_policy()
    P = state_dict_arrays(policy)
    theta = tr.theta_of(P)
    obs = np.random.default_rng(1).normal(0.0, 1.5, (200, 6))
    n = sum(int(np.size(v)) for v in theta.values())
    assert n == 6 * 8 + 8 + 8 * 8 + 8 + 8 * 2 + 2 + 2
    damping = 0.05
    F = np.stack([tr.join_flat(tr.fvp(P, obs, tr.split_flat(e, theta), damping), theta) for e in np.eye(n)], 1)
    assert np.abs(F - F.T).max() <= 1e-12 * np.abs(F).max() and np.linalg.eigvalsh(0.5 * (F + F.T)).min() > 0.9 * damping
    b = np.random.default_rng(2).normal(size=n)
    want = np.linalg.solve(F, b)
    got = tr.conjugate_gradient(lambda p: tr.fvp(P, obs, p, damping), tr.split_flat(b, theta), iterations=4 * n, tolerance=1e-30)
    assert np.abs(tr.join_flat(got, theta) - want).max() <= 1e-8 * np.abs(want).max()
    # ten iterations, as the learner runs: the same Krylov iterate as a textbook CG on the dense matrix
    x, r = np.zeros(n), b.copy()
    p, rr = r.copy(), r @ r
    for _ in range(10):
        Fp = F @ p
        a = rr / (p @ Fp)
        x, r = x + a * p, r - a * Fp
        p, rr = r + (r @ r / rr) * p, r @ r
    got10 = tr.join_flat(tr.conjugate_gradient(lambda q: tr.fvp(P, obs, q, damping), tr.split_flat(b, theta)), theta)
    assert np.abs(got10 - x).max() <= 1e-9 * np.abs(x).max()
    # the step size puts the quadratic model of the KL on delta
    xd = tr.split_flat(x, theta)
    beta = tr.step_size(xd, tr.fvp(P, obs, xd, damping))
    assert abs(0.5 * beta * beta * (x @ F @ x) - tr.KL_DELTA) <= 1e-12


def test_surrogate_gradient_is_autograd_of_the_surrogate():
    import torch
    ro = rollout("swing-52-lockstep")
    rows = np.random.default_rng(6).permutation(ro.T * ro.n)[:300]
    obs, act, old_logp, adv, _ = (x[rows] for x in flat_shard(ro, ro.gae.adv, ro.gae.returns))
    policy = make_policy(ro.arch, ro.kind).double()
    P = state_dict_arrays(policy)
    got = tr.surrogate_gradient(P, obs, act, old_logp, adv)
    a = torch.from_numpy(tr.normalise(adv))
    _, logp, _ = policy.evaluate(torch.from_numpy(obs.astype(np.float64)), torch.from_numpy(act.astype(np.float64)))
    L = ((logp - torch.from_numpy(old_logp.astype(np.float64))).exp() * a).mean()
    names, params = zip(*theta_params(policy))
    for k, g in zip(names, torch.autograd.grad(L, params)):
        assert np.abs(g.numpy() - got[k]).max() <= 1e-11 * max(np.abs(got[k]).max(), 1e-30), k
    assert abs(float(L.detach()) - tr.surrogate(P, obs, act, old_logp, tr.normalise(adv))) <= 1e-13
    assert tr.kl(P, P, obs) == 0.0


NAN, INF = float("nan"), float("inf")
TABLES = [  # (L_k, KL_k) rows, the k to accept
    ([(0.1, 0.005)] * 10, 0),                                                     # accepted at k = 0
    ([(0.1, 0.02), (0.1, 0.011), (0.05, 0.0099), (0.04, 0.001)], 2),              # k = 0, 1 violate the KL bound
    ([(-0.1, 0.001), (-1e-9, 0.001), (0.0, 0.01), (0.1, 0.001)], 2),              # L >= 0 and KL <= delta include equality
    ([(NAN, 0.001), (0.1, NAN), (INF, 0.001), (0.1, -INF), (0.2, 0.002)], 4),     # non-finite candidates never qualify
    ([(0.1, 0.02)] * 5 + [(-0.1, 0.001)] * 5, -1),                                # all rejected
    ([(NAN, NAN)] * 10, -1),
]


@pytest.mark.parametrize("rows,want", TABLES)
def test_selection_on_hand_made_tables(rows, want):
    import torch
    from tennisbot_rl_amd.trpo import select_candidate
    table = np.array(rows, np.float64)
    assert tr.select(table, 0.01) == want
    got = select_candidate(torch, torch.from_numpy(table), 0.01)
    assert got.dim() == 0 and got.dtype == torch.int64 and int(got) == want


# ------------------------------------------------------------------------------------------------------ the host side of the ABI
@pytest.fixture(scope="module")
def lib():
    from tennisbot_rl_amd.build import build_library
    from tennisbot_rl_amd.stepper import load_library
    build_library()
    return load_library()


def test_trpo_symbols_and_workspace_queries(lib):
    for name in ("tb_trpo_fvp", "tb_trpo_search", "tb_trpo_fvp_workspace_bytes", "tb_trpo_search_workspace_bytes", "tb_trpo_rows_per_workgroup",
                 "tb_trpo_search_rows_per_workgroup"):
        assert hasattr(lib, name), name
    assert lib.tb_abi_version() == 4
    share, sshare = lib.tb_trpo_rows_per_workgroup(), lib.tb_trpo_search_rows_per_workgroup()
    assert share == lib.tb_ppo_rows_per_workgroup() and sshare > 0 and sshare % 64 == 0
    for kind in (0, 1):
        P = lib.tb_ppo_param_floats(kind)
        sizes = [lib.tb_trpo_fvp_workspace_bytes(kind, m) for m in (1, share, share + 1, 40 * share)]
        assert sizes[0] == sizes[1] == 2 * 4 * P and sizes[2] == 2 * sizes[1] and sizes[3] == 40 * sizes[1]
        s = [lib.tb_trpo_search_workspace_bytes(kind, b, 10) for b in (2, sshare, sshare + 1, 100 * sshare)]
        assert 0 < s[0] == s[1] < s[2] < s[3] and s[3] - s[0] == 99 * (s[2] - s[1])
        assert lib.tb_trpo_search_workspace_bytes(kind, sshare, 20) - s[1] == s[2] - s[1]
    for bad in (lib.tb_trpo_fvp_workspace_bytes(7, 100), lib.tb_trpo_fvp_workspace_bytes(0, 0), lib.tb_trpo_search_workspace_bytes(-1, 100, 10),
                lib.tb_trpo_search_workspace_bytes(0, 1, 10), lib.tb_trpo_search_workspace_bytes(0, 100, 0), lib.tb_trpo_search_workspace_bytes(0, 100, 65)):
        assert bad == -1 and b"tb_trpo_" in lib.tb_last_error()


def test_trpo_refusals_need_no_device(lib):
    P = lib.tb_ppo_param_floats(0)
    buf = (ctypes.c_double * 8192)()
    a = ctypes.addressof(buf)
    assert a % 8 == 0
    ws = 1 << 20

    def refused(fn, args, word):
        assert fn(*args) == -1 and word in lib.tb_last_error(), lib.tb_last_error()

    fvp = [0, 0, None, a, 100, a, 50, a, a + 4096, P, 0.001, a + 8192, a, ws]
    for k in (3, 5, 7, 8, 11, 12):
        bad = list(fvp); bad[k] = None
        refused(lib.tb_trpo_fvp, bad, b"null")
    for k in (3, 7, 8, 11):
        bad = list(fvp); bad[k] += 2
        refused(lib.tb_trpo_fvp, bad, b"aligned")
    for k in (5, 12):
        bad = list(fvp); bad[k] += 4
        refused(lib.tb_trpo_fvp, bad, b"aligned")
    bad = list(fvp); bad[9] = P - 1
    refused(lib.tb_trpo_fvp, bad, b"n_params")
    bad = list(fvp); bad[0] = 9
    refused(lib.tb_trpo_fvp, bad, b"env kind")
    bad = list(fvp); bad[6] = 0
    refused(lib.tb_trpo_fvp, bad, b"n_idx")
    bad = list(fvp); bad[13] = 16
    refused(lib.tb_trpo_fvp, bad, b"workspace")
    bad = list(fvp); bad[11] = bad[8]
    refused(lib.tb_trpo_fvp, bad, b"vec_dev")
    search = [0, 0, None, a, a, a, a, 100, a, 100, a, a, P, a, 10, a, a, ws]
    for k in (3, 4, 5, 6, 8, 10, 11, 13, 15, 16):
        bad = list(search); bad[k] = None
        refused(lib.tb_trpo_search, bad, b"null")
    for k in (3, 4, 5, 6, 10, 11, 13):
        bad = list(search); bad[k] += 2
        refused(lib.tb_trpo_search, bad, b"aligned")
    for k in (8, 15, 16):
        bad = list(search); bad[k] += 4
        refused(lib.tb_trpo_search, bad, b"aligned")
    bad = list(search); bad[12] = P + 1
    refused(lib.tb_trpo_search, bad, b"n_params")
    bad = list(search); bad[9] = 1
    refused(lib.tb_trpo_search, bad, b"batch")
    bad = list(search); bad[14] = 65
    refused(lib.tb_trpo_search, bad, b"n_candidates")
    bad = list(search); bad[17] = 64
    refused(lib.tb_trpo_search, bad, b"workspace")
    # the critic-only bit of tb_ppo_apply is a modifier, not a phase of its own
    tail = [a, a, a, a, P, a, 0.0, 0.5, 1, 3e-4, 0.9, 0.999, 1e-5, 1]
    refused(lib.tb_ppo_apply, [0, 0, None, 4, a, ws, 100] + tail, b"phases")
    refused(lib.tb_ppo_apply, [0, 0, None, 8 | 1, a, ws, 100] + tail, b"phases")


def test_trainer_refuses_another_architecture_before_it_touches_a_device():
    from tennisbot_rl_amd.trpo import TRPO_DEFAULTS, TRPOTrainer
    with pytest.raises(ValueError, match="net_arch"):
        TRPOTrainer("SwingRacket-v0", num_envs=64, n_steps=26, net_arch=(64, 64))
    with pytest.raises(ValueError, match="torch learner"):
        TRPOTrainer("Tennisbot-v0", num_envs=64, n_steps=26, learner="torch")
    assert (TRPO_DEFAULTS["kl_delta"], TRPO_DEFAULTS["cg_iterations"], TRPO_DEFAULTS["cg_damping"], TRPO_DEFAULTS["cg_state_percent"]) == (0.01, 10, 0.001, 0.1)
    assert math.isclose(TRPO_DEFAULTS["search_decay"], 1.5) and TRPO_DEFAULTS["search_candidates"] == 10


def test_trainer_refuses_more_than_one_rank(monkeypatch):
    import torch
    from tennisbot_rl_amd.trpo import TRPOTrainer
    monkeypatch.setattr(torch.distributed, "is_available", lambda: True)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True, raising=False)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2, raising=False)
    with pytest.raises(ValueError, match="one rank"):
        TRPOTrainer("SwingRacket-v0", num_envs=64, n_steps=26)


def test_train_swing_options_for_trpo(monkeypatch, capsys):
    import importlib.util
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_swing_for_trpo", os.path.join(root, "train_swing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for argv, word in ((["-s", "trpo", "--learner", "torch"], "no torch learner"), (["-s", "sac"], "only -s ppo and -s trpo")):
        monkeypatch.setattr(sys, "argv", ["train_swing.py"] + argv)
        with pytest.raises(SystemExit) as e:
            mod.main()
        assert word in str(e.value.code)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(sys, "argv", ["train_swing.py", "-s", "trpo"])
    with pytest.raises(SystemExit) as e:
        mod.main()
    assert "one rank" in str(e.value.code)
