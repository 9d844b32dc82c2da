"""TB_NET_MLP64 (SB3's [64, 64] on SwingRacket-v0) and sb3_contrib's TRPO form, as far as no GPU is needed: the sizes and refusals of the
C ABI, the packed blob and the flat parameter order, the preset and the acceptance rule, the float64 references on the new
architecture, the margins of the line search's fixtures that tests/test_gpu_mlp64_trpo.py runs on the device, the script's flags and
the checkpoint's net field."""
import ctypes
import math
import os
import sys
import types

import numpy as np
import pytest

import mlp64_fixtures as fx
import trpo_reference as tr
from policy_reference import state_dict_arrays
from test_ppo_reference import flat_shard
from test_trpo_reference import theta_params, torch_kl
from tennisbot_rl_amd.params import ENV_SWING, ENV_TENNIS, NET_DEFAULT, NET_MLP64, NET_TUNED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB_E_PARAMS = -3


@pytest.fixture(scope="module")
def lib():
    from tennisbot_rl_amd.build import build_library
    from tennisbot_rl_amd.stepper import load_library
    build_library()
    return load_library()


# ------------------------------------------------------------------------------------------------------------ sizes and refusals
def test_sizes_of_the_new_net(lib):
    assert NET_MLP64 == 2
    assert lib.tb_policy_blob_floats(ENV_SWING, NET_MLP64) == fx.BLOB_FLOATS == 11560
    assert lib.tb_ppo_param_floats_net(ENV_SWING, NET_MLP64) == fx.PARAM_FLOATS == 9677 == sum(p.numel() for p in fx.policy().parameters())
    # the other nets are where they were
    assert lib.tb_policy_blob_floats(ENV_SWING, NET_DEFAULT) == lib.tb_policy_floats(ENV_SWING) and lib.tb_ppo_param_floats_net(ENV_SWING, NET_DEFAULT) == 9069
    assert lib.tb_ppo_param_floats_net(ENV_TENNIS, NET_DEFAULT) == 10181 and lib.tb_ppo_param_floats_net(ENV_TENNIS, NET_TUNED) == 9639
    share = lib.tb_ppo_rows_per_workgroup()
    assert lib.tb_ppo_workspace_bytes_net(ENV_SWING, NET_MLP64, share) == 2 * 64 * 8 + 2 * 4 * (9677 + 2)
    assert lib.tb_trpo_fvp_workspace_bytes_net(ENV_SWING, NET_MLP64, share) == 2 * 4 * 9677
    assert lib.tb_trpo_fvp_workspace_bytes_net(ENV_SWING, NET_DEFAULT, share) == lib.tb_trpo_fvp_workspace_bytes(ENV_SWING, share)
    assert lib.tb_trpo_search_workspace_bytes_net(ENV_SWING, NET_MLP64, 5000, 11) == lib.tb_trpo_search_workspace_bytes(ENV_SWING, 5000, 11) > 0


def test_the_tennisbot_pair_is_refused_by_name(lib):
    calls = [lambda: lib.tb_policy_blob_floats(ENV_TENNIS, NET_MLP64), lambda: lib.tb_ppo_param_floats_net(ENV_TENNIS, NET_MLP64),
             lambda: lib.tb_ppo_workspace_bytes_net(ENV_TENNIS, NET_MLP64, 64), lambda: lib.tb_trpo_fvp_workspace_bytes_net(ENV_TENNIS, NET_MLP64, 64),
             lambda: lib.tb_trpo_search_workspace_bytes_net(ENV_TENNIS, NET_MLP64, 64, 10)]
    for call in calls:
        assert call() == TB_E_PARAMS
        assert b"TB_NET_DEFAULT is that net" in lib.tb_last_error(), lib.tb_last_error()
    # the tuned network has no TRPO kernels, as before; SwingRacket has no tuned network
    assert lib.tb_trpo_fvp_workspace_bytes_net(ENV_TENNIS, NET_TUNED, 64) == TB_E_PARAMS and b"TB_NET_TUNED" in lib.tb_last_error()
    assert lib.tb_trpo_search_workspace_bytes_net(ENV_TENNIS, NET_TUNED, 64, 10) == TB_E_PARAMS
    assert lib.tb_policy_blob_floats(ENV_SWING, NET_TUNED) == TB_E_PARAMS and lib.tb_policy_blob_floats(ENV_SWING, 3) == TB_E_PARAMS
    # the Python layer: the same explanation, as a ValueError, before any env exists
    from tennisbot_rl_amd.evaluation import PolicyEvaluator
    from tennisbot_rl_amd.ppo import PPOTrainer
    from tennisbot_rl_amd.stepper import check_net
    from tennisbot_rl_amd.trpo import TRPOTrainer
    assert check_net(ENV_SWING, NET_MLP64) == NET_MLP64 and check_net(ENV_TENNIS, NET_TUNED) == NET_TUNED
    for make in (lambda: check_net(ENV_TENNIS, NET_MLP64), lambda: PolicyEvaluator(ENV_TENNIS, net=NET_MLP64),
                 lambda: PPOTrainer("Tennisbot-v0", num_envs=16, n_steps=8, policy="mlp64"),
                 lambda: TRPOTrainer("Tennisbot-v0", num_envs=16, n_steps=8, policy="mlp64", form="sb3")):
        with pytest.raises(ValueError, match="NET_DEFAULT"):
            make()
    with pytest.raises(ValueError, match="form"):
        TRPOTrainer("SwingRacket-v0", num_envs=16, n_steps=26, form="sb4")
    with pytest.raises(ValueError, match="net_arch"):
        TRPOTrainer("SwingRacket-v0", num_envs=16, n_steps=26, policy="mlp64", net_arch=(32, 64, 32))
    # the name is the architecture: PPOTrainer lets no other net_arch carry it, fused or not
    for kw in (dict(), dict(fused=False), dict(learner="fused")):
        with pytest.raises(ValueError, match=r"policy='mlp64' is net_arch \(64, 64\)"):
            PPOTrainer("SwingRacket-v0", num_envs=16, n_steps=26, policy="mlp64", net_arch=(32, 64, 32), **kw)


def test_trpo_net_calls_refuse_bad_arguments_without_a_device(lib):
    for name in ("tb_trpo_fvp_net", "tb_trpo_search_net", "tb_trpo_fvp_workspace_bytes_net", "tb_trpo_search_workspace_bytes_net"):
        assert hasattr(lib, name), name
    P = fx.PARAM_FLOATS
    buf = (ctypes.c_double * 8192)()
    a = ctypes.addressof(buf)
    assert a % 8 == 0
    ws = 1 << 20

    def refused(fn, args, word, rc=-1):
        assert fn(*args) == rc and word in lib.tb_last_error(), lib.tb_last_error()

    fvp = [ENV_SWING, NET_MLP64, 0, None, a, 100, a, 50, a, a + 4096, P, 0.1, a + 8192, a, ws]
    for k in (4, 6, 8, 9, 12, 13):
        bad = list(fvp); bad[k] = None
        refused(lib.tb_trpo_fvp_net, bad, b"null")
    for k in (4, 8, 9, 12):
        bad = list(fvp); bad[k] += 2
        refused(lib.tb_trpo_fvp_net, bad, b"aligned")
    for k in (6, 13):
        bad = list(fvp); bad[k] += 4
        refused(lib.tb_trpo_fvp_net, bad, b"aligned")
    bad = list(fvp); bad[10] = 9069                                      # the default net's count
    refused(lib.tb_trpo_fvp_net, bad, b"n_params")
    bad = list(fvp); bad[14] = 16
    refused(lib.tb_trpo_fvp_net, bad, b"workspace")
    bad = list(fvp); bad[0] = ENV_TENNIS
    refused(lib.tb_trpo_fvp_net, bad, b"TB_NET_DEFAULT", TB_E_PARAMS)
    bad = list(fvp); bad[0], bad[1] = ENV_TENNIS, NET_TUNED
    refused(lib.tb_trpo_fvp_net, bad, b"TB_NET_TUNED", TB_E_PARAMS)
    search = [ENV_SWING, NET_MLP64, 0, None, a, a, a, a, 100, a, 100, a, a, P, a, 11, a, a, ws]
    for k in (4, 5, 6, 7, 9, 11, 12, 14, 16, 17):
        bad = list(search); bad[k] = None
        refused(lib.tb_trpo_search_net, bad, b"null")
    for k in (4, 5, 6, 7, 11, 12, 14):
        bad = list(search); bad[k] += 2
        refused(lib.tb_trpo_search_net, bad, b"aligned")
    for k in (9, 16, 17):
        bad = list(search); bad[k] += 4
        refused(lib.tb_trpo_search_net, bad, b"aligned")
    bad = list(search); bad[13] = 9069
    refused(lib.tb_trpo_search_net, bad, b"n_params")
    bad = list(search); bad[15] = 65
    refused(lib.tb_trpo_search_net, bad, b"n_candidates")
    bad = list(search); bad[18] = 64
    refused(lib.tb_trpo_search_net, bad, b"workspace")
    bad = list(search); bad[0] = ENV_TENNIS
    refused(lib.tb_trpo_search_net, bad, b"TB_NET_DEFAULT", TB_E_PARAMS)
    # the learner's calls with the new net: the count that belongs to it, and the critic-only modifier is offered
    grad = [ENV_SWING, NET_MLP64, 0, None, 16, 16, 16, 16, 16, 10, 16, 8, 16, 9069, 0.2, 0.5, 16, 1 << 30]
    refused(lib.tb_ppo_grad_net, grad, b"n_params")
    grad[13] = P; grad[5] = 18
    refused(lib.tb_ppo_grad_net, grad, b"aligned")
    tail = [a, a, a, a, P, a, 0.0, 0.5, 1, 3e-4, 0.9, 0.999, 1e-5, 1]
    refused(lib.tb_ppo_apply_net, [ENV_SWING, NET_MLP64, 0, None, 4, a, ws, 100] + tail, b"phases")           # VALUE_ONLY alone is no phase
    refused(lib.tb_ppo_apply_net, [ENV_SWING, NET_MLP64, 0, None, 1 | 4, a + 4, ws, 100] + tail, b"workspace")  # ... but with one it gets as far as the buffers
    refused(lib.tb_ppo_apply_net, [ENV_TENNIS, NET_TUNED, 0, None, 1 | 4, a, ws, 100] + tail, b"VALUE_ONLY", -4)                 # TB_E_UNSUPPORTED, as before


# ------------------------------------------------------------------------------------------------------------ packing and layout
def test_pack_policy_unpacks_to_the_module():
    """the blob of the new net, taken apart by the fragment order stated in include/tb_stepper.h (tuned_reference.unpack_layer: every
    padded slot must hold 0), then a numpy forward pass in float64 against the torch module in float64"""
    import torch
    from tennisbot_rl_amd.ppo import pack_policy, policy_net_of
    from tuned_reference import unpack_layer
    policy = fx.policy()
    assert policy_net_of(policy) == NET_MLP64
    blob = pack_policy(policy).numpy().astype(np.float64)
    assert blob.size == fx.BLOB_FLOATS
    p, towers = 0, []
    for _ in range(2):
        layers = []
        for n_in, n_out, first in ((6, 64, True), (64, 64, False), (64, 6 if not towers else 1, False)):
            W, b, used = unpack_layer(blob[p:], n_in, n_out, first)
            layers.append((W, b))
            p += used
        towers.append(layers)
    assert p == 2 * (576 + 4160 + 1040) and blob.size - p == 8
    log_std = blob[p:p + 6]
    assert not blob[p + 6:].any()
    obs = np.random.default_rng(5).normal(0.0, 1.5, (37, 6))

    def forward(layers):
        h = obs
        for W, b in layers[:-1]:
            h = np.tanh(h @ W.T + b)
        return h @ layers[-1][0].T + layers[-1][1]

    with torch.no_grad():
        mean, value = policy.double()(torch.from_numpy(obs))
    assert np.abs(forward(towers[0]) - mean.numpy()).max() <= 1e-12 and np.abs(forward(towers[1])[:, 0] - value.numpy()).max() <= 1e-12
    assert np.array_equal(log_std, policy.log_std.detach().numpy())


def test_flat_parameter_order_is_named_parameters():
    import torch
    from tennisbot_rl_amd.learner import flatten_parameters, parameter_offsets
    from tennisbot_rl_amd.ppo import SB3_SWING_DEFAULTS, build_actor_critic, policy_net_of
    assert tuple(SB3_SWING_DEFAULTS["net_arch"]) == (64, 64)
    policy = build_actor_critic(6, 6, (64, 64))
    assert [k for k, _ in policy.named_parameters()] == fx.ORDER
    before = {k: v.clone() for k, v in policy.state_dict().items()}
    flat = flatten_parameters(policy)
    assert flat.numel() == fx.PARAM_FLOATS
    assert torch.equal(flat, torch.cat([before[k].reshape(-1) for k in fx.ORDER]))
    off = parameter_offsets(policy)
    # the slot ranges of csrc/tb_learner.hpp's PpoLayout for this net
    body = 64 * 7 + 64 * 65
    assert off["log_std"] == (0, 6) and off["policy_net.0.weight"][0] == 6 and off["value_net_body.0.weight"][0] == 6 + body
    assert off["action_net.weight"][0] == 6 + 2 * body and off["value_net.weight"][0] == 6 + 2 * body + 6 * 65 and off["value_net.bias"] == (fx.PARAM_FLOATS - 1, 1)
    # which module is which net
    assert policy_net_of(policy) == NET_MLP64 and policy_net_of(build_actor_critic(12, 2, (64, 64))) == NET_DEFAULT
    assert policy_net_of(build_actor_critic(6, 6, (32, 64, 32))) == NET_DEFAULT


# -------------------------------------------------------------------------------------------------------------- preset and rule
def test_the_sb3_preset():
    from tennisbot_rl_amd.trpo import SB3_TRPO_DEFAULTS, TRPO_DEFAULTS
    assert SB3_TRPO_DEFAULTS == fx.SB3 and set(TRPO_DEFAULTS) < set(SB3_TRPO_DEFAULTS)
    assert math.isinf(SB3_TRPO_DEFAULTS["max_grad_norm"]) and math.isclose(1.0 / SB3_TRPO_DEFAULTS["search_decay"], 0.8)
    assert TRPO_DEFAULTS["cg_iterations"] == 10 and TRPO_DEFAULTS["search_decay"] == 1.5          # the agent form's: where they were
    text = open(os.path.join(ROOT, "tennisbot_rl_amd", "trpo.py")).read()
    assert "[3P-recalled]" in text[text.index("SB3_TRPO_DEFAULTS") - 600:text.index("SB3_TRPO_DEFAULTS = ")]


NAN, INF = float("nan"), float("inf")
D = 0.01
SB3_TABLES = [  # row 0: the zero step (L_0, 0); then the candidates; the k sb3's rule accepts
    ([(0.3, 0.0)] + [(0.4, 0.005)] * 10, 0),                                              # accepted at the first candidate
    ([(0.3, 0.0), (0.4, D), (0.4, 0.009)], 1),                                            # KL_k == delta: rejected
    ([(0.3, 0.0), (0.3, 0.001), (0.31, 0.001)], 1),                                       # L_k == L_0: rejected
    ([(0.3, 0.0), (NAN, 0.001), (0.4, NAN), (INF, 0.001), (0.4, -INF), (0.35, 0.002)], 4),  # non-finite candidates are skipped
    ([(0.3, 0.0)] + [(0.4, 0.02)] * 5 + [(0.2, 0.001)] * 5, -1),                          # none accepted
    ([(NAN, 0.0)] + [(0.4, 0.001)] * 3, -1),                                              # no L_0 to beat
    ([(-0.2, 0.0), (-0.1, 0.001)], 0),                                                    # L_0 < L_k < 0: sb3 takes it
]


@pytest.mark.parametrize("rows,want", SB3_TABLES)
def test_sb3_selection_on_hand_made_tables(rows, want):
    import torch
    from tennisbot_rl_amd.trpo import select_candidate_sb3
    table = np.array(rows, np.float64)
    assert fx.select_sb3(table, D) == want
    got = select_candidate_sb3(torch, torch.from_numpy(table), D)
    assert got.dim() == 0 and got.dtype == torch.int64 and int(got) == want


def test_the_two_rules_differ_where_they_should():
    import torch
    from tennisbot_rl_amd.trpo import select_candidate, select_candidate_sb3
    both = lambda rows: (int(select_candidate(torch, torch.tensor(rows[1:], dtype=torch.float64), D)),  # noqa: E731
                         int(select_candidate_sb3(torch, torch.tensor(rows, dtype=torch.float64), D)))
    # a candidate that improves on a negative L_0 without reaching 0: sb3 accepts it, agent.py waits for L >= 0
    assert both([(-0.2, 0.0), (-0.1, 0.001), (0.0, 0.0005)]) == (1, 0)
    # a candidate that is positive but below L_0, and one exactly on the KL bound: agent.py accepts them, sb3 does not
    assert both([(0.3, 0.0), (0.2, 0.001), (0.35, D), (0.36, 0.001)]) == (0, 2)
    assert tr.select(np.array([(-0.1, 0.001), (0.0, 0.0005)]), D) == 1 and fx.select_sb3(np.array([(-0.2, 0.0), (-0.1, 0.001), (0.0, 0.0005)]), D) == 0


# ------------------------------------------------------------------------------------------------------------------ references
def test_fvp_reference_is_the_double_backprop_hessian_on_the_new_net():
    import torch
    ro = fx.rollout()
    policy = fx.policy().double()
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
    assert sum(p.numel() for p in params) == 6 + 64 * 7 + 64 * 65 + 6 * 65
    grads = torch.autograd.grad(torch_kl(torch, policy, old_mean, old_ls, x), params, create_graph=True)
    hv = torch.autograd.grad(sum((g * torch.from_numpy(v[k])).sum() for k, g in zip(names, grads)), params)
    for k, h in zip(names, hv):
        assert np.abs(h.numpy() - want[k]).max() <= 1e-11 * max(np.abs(want[k]).max(), 1e-30), k
    assert np.array_equal(want["log_std"], 2.0 * v["log_std"])


def test_surrogate_gradient_reference_is_autograd_on_the_new_net():
    import torch
    ro = fx.rollout()
    rows = np.random.default_rng(6).permutation(ro.T * ro.n)[:300]
    obs, act, old_logp, adv, _ = (x[rows] for x in flat_shard(ro, ro.gae.adv, ro.gae.returns))
    policy = fx.policy().double()
    P = state_dict_arrays(policy)
    got = tr.surrogate_gradient(P, obs, act, old_logp, adv)
    a = torch.from_numpy(tr.normalise(adv))
    _, logp, _ = policy.evaluate(torch.from_numpy(obs.astype(np.float64)), torch.from_numpy(act.astype(np.float64)))
    L = ((logp - torch.from_numpy(old_logp.astype(np.float64))).exp() * a).mean()
    names, params = zip(*theta_params(policy))
    for k, g in zip(names, torch.autograd.grad(L, params)):
        assert np.abs(g.numpy() - got[k]).max() <= 1e-11 * max(np.abs(got[k]).max(), 1e-30), k


@pytest.mark.parametrize("which", ["kl", "none", "random"])
def test_search_fixtures_keep_their_distance_from_both_thresholds(which):
    """what tests/test_gpu_mlp64_trpo.py runs on the device: every candidate of every fixture at least MARGIN float32-twin errors away from
    KL = delta and from L = L_0, so that a kernel within tolerance must pick the reference's k; and the fixtures are of their kinds"""
    picked = set()
    for m in fx.SEARCH_ROWS:
        c = fx.search_case(m, which)
        assert c.steps[0] == 0.0 and c.steps.size == 11 and c.want[0, 1] == 0.0 and c.twin[0, 1] == 0.0
        assert c.margins.min() > fx.MARGIN, "m = %d %s: a candidate sits %.3g twin errors from a threshold" % (m, which, c.margins.min())
        if which == "kl":
            assert c.want[1, 1] > fx.SB3["kl_delta"] and c.k >= 1
        if which == "none":
            assert c.k == -1 and (c.want[1:, 0] < c.want[0, 0]).all() and (c.want[1:, 1] < fx.SB3["kl_delta"]).all()
        picked.add(c.k)
        print("m = %4d %-6s accepted %2d, L_0 %.3g, smallest margin %.3g" % (m, which, c.k, c.want[0, 0], c.margins.min()))
    assert which != "kl" or max(picked) >= 2


# ------------------------------------------------------------------------------------------------------- script and checkpoints
def load_script():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_swing_for_mlp64", os.path.join(ROOT, "train_swing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_an_explicit_flag_beats_the_preset(monkeypatch):
    from tennisbot_rl_amd.trpo import SB3_TRPO_DEFAULTS, TRPO_DEFAULTS
    mod = load_script()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    kw = mod.trpo_keywords(mod.parse_args(["-s", "trpo", "--trpo-form", "sb3", "--net", "mlp64"]))
    assert kw == dict(form="sb3", policy="mlp64")                      # nothing given: everything is the preset's
    hp = dict(SB3_TRPO_DEFAULTS, **{k: v for k, v in kw.items() if k not in ("form", "policy")})
    assert (hp["cg_iterations"], hp["cg_damping"], hp["cg_state_percent"], hp["kl_delta"]) == (15, 0.1, 1.0, 0.01)
    kw = mod.trpo_keywords(mod.parse_args(["-s", "trpo", "--trpo-form", "sb3", "--cg-damping", "0.001", "--cg-iterations", "10", "--cg-state-percent", "0.1", "--kl-delta", "0.02"]))
    assert kw == dict(form="sb3", policy="default", cg_damping=0.001, cg_iterations=10, cg_state_percent=0.1, kl_delta=0.02)
    hp = dict(SB3_TRPO_DEFAULTS, **{k: v for k, v in kw.items() if k not in ("form", "policy")})   # what TRPOTrainer(form="sb3", **kw) does
    assert (hp["cg_iterations"], hp["cg_damping"], hp["cg_state_percent"], hp["kl_delta"], hp["search_decay"]) == (10, 0.001, 0.1, 0.02, 1.25)
    # a flag that names the preset's own value is still "given"; the agent form without flags is today's
    assert mod.trpo_keywords(mod.parse_args(["-s", "trpo", "--cg-damping", "0.1"])) == dict(form="agent", policy="default", cg_damping=0.1)
    assert mod.trpo_keywords(mod.parse_args(["-s", "trpo"])) == dict(form="agent", policy="default")
    assert dict(TRPO_DEFAULTS)["cg_damping"] == 0.001
    for argv, word in ((["--net", "mlp64", "--env", "Tennisbot-v0"], "mlp64"), (["--trpo-form", "sb3"], "-s trpo")):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(argv)
        assert word in str(e.value.code)
    assert mod.parse_args(["--net", "mlp64"]).select == "ppo"         # --net mlp64 also goes with -s ppo
    assert mod.parse_args(["-s", "trpo", "--trpo-form", "sb3", "--env", "Tennisbot-v0"]).net == "default"


def test_a_checkpoint_of_one_net_is_refused_by_a_trainer_of_another(tmp_path):
    """PPOTrainer.save / .load unbound on stand-ins (no device): the net's name travels with the checkpoint, and load() compares it before
    it touches the policy"""
    import torch
    from tennisbot_rl_amd.ppo import PPOTrainer, build_actor_critic

    def stand_in(net, arch):
        policy = build_actor_critic(6, 6, arch)
        env = types.SimpleNamespace(get_state_words=lambda: (torch.zeros(30, 4, dtype=torch.int32), torch.zeros(4, dtype=torch.uint8)),
                                    set_state_words=lambda w, d: None, observe=lambda: torch.zeros(4, 6))
        return types.SimpleNamespace(torch=torch, net=net, policy=policy, opt=torch.optim.Adam(policy.parameters(), lr=1e-3, eps=1e-5), num_timesteps=123, env=env,
                                     hp={"net_arch": arch}, device=torch.device("cpu"), obs_in=torch.zeros(4, 6))

    a = stand_in(NET_MLP64, (64, 64))
    path = str(tmp_path / "mlp64.pt")
    PPOTrainer.save(a, path)
    assert torch.load(path, weights_only=True)["net"] == "mlp64"
    b = stand_in(NET_MLP64, (64, 64))
    PPOTrainer.load(b, path)
    assert b.num_timesteps == 123 and all(torch.equal(p, q) for p, q in zip(a.policy.parameters(), b.policy.parameters()))
    c = stand_in(NET_DEFAULT, (32, 64, 32))
    before = [p.clone() for p in c.policy.parameters()]
    with pytest.raises(ValueError, match="'mlp64'.*'default'"):
        PPOTrainer.load(c, path)
    assert all(torch.equal(p, q) for p, q in zip(before, c.policy.parameters())) and c.num_timesteps == 123
    path2 = str(tmp_path / "default.pt")
    PPOTrainer.save(c, path2)
    with pytest.raises(ValueError, match="'default'.*'mlp64'"):
        PPOTrainer.load(stand_in(NET_MLP64, (64, 64)), path2)


def test_tools_take_the_net():
    import subprocess
    for tool, words in (("validate_swing.py", ("--net",)), ("trpo_rate.py", ("--net", "--form")), ("fit_mlp64_student.py", ("--out",))):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and all(w in out.stdout for w in words), out.stdout + out.stderr


def test_the_student_fixture_is_a_mlp64_state_dict():
    """tests/golden/mlp64_swing_student.npz (tools/fit_mlp64_student.py): the module's own names and shapes, finite, the shipped policy's log_std"""
    from tennisbot_rl_amd.ppo import build_actor_critic
    z = dict(np.load(os.path.join(ROOT, "tests", "golden", "mlp64_swing_student.npz")))
    policy = build_actor_critic(6, 6, fx.ARCH)
    want = {k: tuple(v.shape) for k, v in policy.state_dict().items()}
    assert list(z) == list(want) == fx.ORDER and {k: v.shape for k, v in z.items()} == want
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in z.values()) and sum(v.size for v in z.values()) == fx.PARAM_FLOATS
    teacher = dict(np.load(os.path.join(ROOT, "tests", "golden", "ppo_swing_policy.npz")))
    assert np.array_equal(z["log_std"], teacher["log_std"])
