"""The fused learner (tennisbot_rl_amd/learner.py: tb_ppo_gae, tb_ppo_grad, tb_ppo_apply) alone on the device, driven with the synthetic
rollouts of tests/test_ppo_reference.py (300 envs -- no multiple of a wave -- by 52 / 70 steps) and held to the float64 reference
of tests/ppo_reference.py with that file's own tolerances: GAE within the reference's a-priori bound, everything else within
ppo_reference.MULTIPLE float32-twin errors per tensor in the max norm. The largest ratios are printed at the end of the module
and quoted in DESIGN.md ("The fused learner")."""
import copy
import ctypes
import types

import numpy as np
import pytest

import ppo_reference as ref
from policy_reference import assert_within, state_dict_arrays
from test_ppo_reference import CASES, flat_shard, make_policy, returns_near_the_critic, rollout

pytestmark = pytest.mark.gpu

MULTIPLE = ref.MULTIPLE
DEV = "cuda:0"
RATIOS = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print("fused learner (gpu): largest %s = %.3g" % (k, RATIOS[k]))


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def make_learner(torch, ro, policy=None, opt=None):
    from tennisbot_rl_amd.learner import FusedLearner
    policy = policy if policy is not None else make_policy(ro.arch, ro.kind).to(DEV)
    opt = opt if opt is not None else torch.optim.Adam(policy.parameters(), lr=ro.hp["learning_rate"], eps=1e-5)
    return FusedLearner(ro.kind, policy, opt, dict(ro.hp), torch.device(DEV))


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def h(x):
    return x.detach().cpu().numpy().copy()


# ------------------------------------------------------------------------------------------------------------------------- GAE
@pytest.mark.parametrize("name", list(CASES))
def test_gae_contiguous_and_with_a_record_stride(torch, name):
    from tennisbot_rl_amd.rollout import RolloutBuffer
    ro = rollout(name)
    L = make_learner(torch, ro)
    values, last = dev(torch, ro.values), dev(torch, ro.last_value)
    adv, ret = L.advantages(dev(torch, ro.rewards), values, dev(torch, ro.dones), last)
    assert adv.shape == (ro.T, ro.n) and adv.dtype == torch.float32 and ret.shape == (ro.T, ro.n)
    r = max(assert_within(name + " advantages", h(adv), ro.gae.adv, ro.gae.adv_bound), assert_within(name + " returns", h(ret), ro.gae.returns, ro.gae.returns_bound))
    buf = RolloutBuffer(ro.kind, ro.T, ro.n, DEV)              # one packed record per step: rewards and dones strided over steps
    buf.rewards.copy_(dev(torch, ro.rewards)); buf.dones.copy_(dev(torch, ro.dones))
    assert buf.rewards.stride(0) * 4 == buf.record and buf.dones.stride(0) == buf.record and buf.record > 5 * ro.n
    adv2, ret2 = L.advantages(buf.rewards, values, buf.dones, last)
    assert torch.equal(adv2, adv) and torch.equal(ret2, ret)
    note("GAE |error| / bound", r)
    print("%s: GAE |error| / bound %.3g" % (name, r))


def test_gae_edge_shapes(torch):
    ro = rollout("tennis-70-ragged")
    L = make_learner(torch, ro)
    g, lam = ro.hp["gamma"], ro.hp["gae_lambda"]
    rew, val, don, last = dev(torch, ro.rewards), dev(torch, ro.values), dev(torch, ro.dones), dev(torch, ro.last_value)
    # T = 1: the bootstrap from last_value alone
    want = ref.gae(ro.rewards[:1], ro.values[:1], ro.dones[:1], ro.last_value, g, lam)
    adv, ret = L.advantages(rew[:1], val[:1].contiguous(), don[:1], last)
    assert adv.shape == (1, ro.n)
    note("GAE |error| / bound", max(assert_within("T=1 advantages", h(adv), want.adv, want.adv_bound), assert_within("T=1 returns", h(ret), want.returns, want.returns_bound)))
    # n = 1, 63, 65: column slices (rewards and dones keep the case's row stride; the env that never ends and the one done at 0 and T - 1 are in)
    for n in (1, 63, 65):
        want = ref.gae(ro.rewards[:, :n], ro.values[:, :n], ro.dones[:, :n], ro.last_value[:n], g, lam)
        adv, ret = L.advantages(rew[:, :n], val[:, :n].contiguous(), don[:, :n], last[:n].contiguous())
        assert adv.shape == (ro.T, n)
        note("GAE |error| / bound", max(assert_within("n=%d advantages" % n, h(adv), want.adv, want.adv_bound),
                                        assert_within("n=%d returns" % n, h(ret), want.returns, want.returns_bound)))


# -------------------------------------------------------------------------------------------------------------- one minibatch
def one_minibatch(torch, ro, shard, tag):
    """one epoch, one minibatch over every row of `shard` through the fused learner, against the reference; returns the ratios"""
    L = make_learner(torch, ro)
    P = state_dict_arrays(L.policy)
    N = shard[3].shape[0]
    stats = L.update(*(dev(torch, x) for x in shard), 1, N, 1)
    perms = [[np.arange(N)]]
    want, twin = ref.replay_update(P, [shard], perms, N, L.hp), ref.replay_update(P, [shard], perms, N, L.hp, np.float32)
    grads = ref.named_grads(L.policy)
    gr, sr = ref.tensor_ratios(grads, want.grads, twin.grads), ref.tensor_ratios({k: np.float64(v) for k, v in stats.items()}, want.stats[0], twin.stats[0])
    print("%s: B = %d, pre-clip norm %.3g; gradient %.3g (%s), statistics %.3g twin errors" % (tag, N, want.norms[0], max(gr.values()), max(gr, key=gr.get), max(sr.values())))
    g = note("gradient error / twin error", ref.check_tensors(tag + " gradient", grads, want.grads, twin.grads, MULTIPLE))
    s = note("statistics error / twin error", ref.check_tensors(tag + " statistics", {k: np.float64(v) for k, v in stats.items()}, want.stats[0], twin.stats[0], MULTIPLE))
    # the parameters moved by this one Adam step, too
    lr = L.hp["learning_rate"]
    note("parameter change error / twin error", ref.check_tensors(tag + " parameters", ref.param_change(ref.named_params(L.policy), P, lr), ref.param_change(want.params, P, lr),
                                                                 ref.param_change(twin.params, P, lr), MULTIPLE))
    return want, g, s


@pytest.mark.parametrize("name", list(CASES))
def test_single_minibatch_gradient_and_statistics(torch, name):
    ro = rollout(name)
    want, _, _ = one_minibatch(torch, ro, flat_shard(ro, ro.gae.adv, ro.gae.returns), name + " (norm clip active)")
    assert want.norms[0] > 2 * ro.hp["max_grad_norm"], want.norms
    want, _, _ = one_minibatch(torch, ro, flat_shard(ro, ro.gae.adv, returns_near_the_critic(ro)), name + " (norm clip idle)")
    assert want.norms[0] < 0.8 * ro.hp["max_grad_norm"], want.norms


@pytest.mark.parametrize("name", ["swing-70-midepisode", "tennis-52-ragged"])
def test_minibatch_sizes_at_the_kernels_seams(torch, name):
    from tennisbot_rl_amd.stepper import load_library
    share = load_library().tb_ppo_rows_per_workgroup()
    ro = rollout(name)
    full = flat_shard(ro, ro.gae.adv, returns_near_the_critic(ro))
    rows = np.random.default_rng(9).permutation(ro.T * ro.n)
    for B in (2, 15, 16, 17, share // 2 + 1, share - 1, share + 1, 3 * share + 1):
        one_minibatch(torch, ro, tuple(x[rows[:B]] for x in full), "%s seam" % name)


# ------------------------------------------------------------------------------------------------------ epochs x minibatches
def torch_minibatch_first(torch, ro, adv, returns):
    """a policy and optimiser on the device that have taken ONE minibatch step of the torch learner: moments that are not zero"""
    from tennisbot_rl_amd.ppo import PPOTrainer
    policy = make_policy(ro.arch, ro.kind).to(DEV)
    opt = torch.optim.Adam(policy.parameters(), lr=ro.hp["learning_rate"], eps=1e-5)
    ns = types.SimpleNamespace(torch=torch, hp=dict(ro.hp, n_epochs=1), n_steps=ro.T, num_envs=ro.n, device=torch.device(DEV), world=1, policy=policy, opt=opt,
                               batch_size=ro.T * ro.n, logps=dev(torch, ro.old_logp), obs_seq=dev(torch, ro.obs), _raw_actions=dev(torch, ro.raw))
    PPOTrainer.update(ns, dev(torch, np.asarray(adv, np.float32)), dev(torch, np.asarray(returns, np.float32)))
    return policy, opt


@pytest.mark.parametrize("name", list(CASES))
def test_two_epochs_of_three_minibatches_with_a_ragged_tail(torch, name):
    ro = rollout(name)
    N = ro.T * ro.n
    assert N % ro.batch and N // ro.batch == 2
    shard = flat_shard(ro, ro.gae.adv, ro.gae.returns)
    policy, opt = torch_minibatch_first(torch, ro, ro.gae.adv, ro.gae.returns)
    P0, adam0 = state_dict_arrays(policy), ref.adam_state_of(policy, opt)
    assert adam0["t"] == 1 and min(np.abs(v).max() for v in adam0["m"].values()) > 0.0
    L = make_learner(torch, ro, policy, opt)
    perms = ref.record_permutations(torch, 77, N, 2, DEV)
    stats = L.update(*(dev(torch, x) for x in shard), 2, ro.batch, 1)
    s_want, s_twin = ref.copy_state(adam0), ref.copy_state(adam0)
    want = ref.replay_update(P0, [shard], [perms], ro.batch, L.hp, adam_state=s_want)
    twin = ref.replay_update(P0, [shard], [perms], ro.batch, L.hp, np.float32, adam_state=s_twin)
    assert len(want.norms) == 6
    lr = L.hp["learning_rate"]
    d_want, d_twin, d_got = ref.param_change(want.params, P0, lr), ref.param_change(twin.params, P0, lr), ref.param_change(ref.named_params(policy), P0, lr)
    p = note("parameter change error / twin error", ref.check_tensors(name + " parameters", d_got, d_want, d_twin, MULTIPLE))
    g = note("gradient error / twin error", ref.check_tensors(name + " last gradient", ref.named_grads(policy), want.grads, twin.grads, MULTIPLE))
    s = note("statistics error / twin error", ref.check_tensors(name + " statistics", {k: np.float64(v) for k, v in stats.items()}, want.stats[0], twin.stats[0], MULTIPLE))
    got = ref.adam_state_of(policy, opt)                # what torch.optim.Adam, a checkpoint or the torch learner would find
    assert got["t"] == s_want["t"] == 7
    m = note("Adam moment error / twin error", max(ref.check_tensors(name + " exp_avg", got["m"], s_want["m"], s_twin["m"], MULTIPLE),
                                                   ref.check_tensors(name + " exp_avg_sq", got["v"], s_want["v"], s_twin["v"], MULTIPLE)))
    for q in policy.parameters():
        st = opt.state[q]
        assert float(st["step"]) == 7.0 and st["exp_avg"].shape == q.shape and st["exp_avg_sq"].shape == q.shape and q.grad.shape == q.shape
    print("%s: parameters %.3g, last gradient %.3g, statistics %.3g, moments %.3g twin errors; norms %s" % (name, p, g, s, m, " ".join("%.3g" % x for x in want.norms)))


def test_the_same_update_twice_gives_the_same_bits(torch):
    ro = rollout("swing-52-lockstep")
    shard = tuple(dev(torch, x) for x in flat_shard(ro, ro.gae.adv, ro.gae.returns))
    policy, opt = torch_minibatch_first(torch, ro, ro.gae.adv, ro.gae.returns)
    L = make_learner(torch, ro, policy, opt)
    saved = copy.deepcopy(policy.state_dict()), copy.deepcopy(opt.state_dict())
    runs = []
    for _ in range(2):
        policy.load_state_dict(saved[0]); opt.load_state_dict(copy.deepcopy(saved[1]))
        torch.manual_seed(5)
        L.update(*shard, 2, ro.batch, 1)
        torch.cuda.synchronize()
        runs.append([L.flat.clone(), L.grad.clone(), L.exp_avg.clone(), L.exp_avg_sq.clone(), L.stats.clone()])
    assert not torch.equal(runs[0][0], torch.cat([saved[0][k].reshape(-1) for k, _ in policy.named_parameters()]))
    for a, b in zip(*runs):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_bad_buffers_are_refused_and_nothing_is_written(torch):
    from tennisbot_rl_amd.stepper import StepperError
    ro = rollout("swing-52-lockstep")
    L = make_learner(torch, ro)
    lib, kind, P = L.lib, ro.kind, L.n_params
    N = ro.T * ro.n
    obs, act, old_logp, adv, ret = (dev(torch, x) for x in flat_shard(ro, ro.gae.adv, ro.gae.returns))
    idx = torch.arange(N, device=DEV)
    ws = L.workspace(N)
    ws.fill_(-7.0)
    wb = ws.numel() * 8
    s = torch.cuda.current_stream().cuda_stream
    before = L.flat.clone(), L.grad.clone(), L.exp_avg.clone(), L.exp_avg_sq.clone()
    args = [kind, 0, s, obs.data_ptr(), act.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), ret.data_ptr(), N, idx.data_ptr(), N, L.flat.data_ptr(), P, 0.2, 0.5,
            ws.data_ptr(), wb]

    def refused(fn, a, word):
        assert fn(*a) == -1 and word in lib.tb_last_error(), lib.tb_last_error()

    for k in (3, 4, 7, 11):                                         # obs, raw actions, returns, the parameters: 2 bytes off
        bad = list(args); bad[k] += 2
        refused(lib.tb_ppo_grad, bad, b"aligned")
    bad = list(args); bad[9] += 4                                   # idx: int64
    refused(lib.tb_ppo_grad, bad, b"aligned")
    bad = list(args); bad[12] = P - 1
    refused(lib.tb_ppo_grad, bad, b"n_params")
    bad = list(args); bad[16] = wb - 8 * ws.numel() // 2
    refused(lib.tb_ppo_grad, bad, b"workspace")
    bad = list(args); bad[10] = 1
    refused(lib.tb_ppo_grad, bad, b"batch")
    tail = [L.flat.data_ptr(), L.grad.data_ptr(), L.exp_avg.data_ptr(), L.exp_avg_sq.data_ptr(), P, L.stats.data_ptr(), 0.002, 0.5, 1, 3e-4, 0.9, 0.999, 1e-5, 1]
    refused(lib.tb_ppo_apply, [kind, 0, s, 3, ws.data_ptr(), wb, N] + tail[:4] + [P + 1] + tail[5:], b"n_params")
    refused(lib.tb_ppo_apply, [kind, 0, s, 3, ws.data_ptr(), wb, N, tail[0] + 2] + tail[1:], b"aligned")
    refused(lib.tb_ppo_apply, [kind, 0, s, 0, ws.data_ptr(), wb, N] + tail, b"phases")
    refused(lib.tb_ppo_gae, [kind, 0, s, ro.T, ro.n, adv.data_ptr(), 4 * ro.n - 4, idx.data_ptr(), 0, ret.data_ptr(), ret.data_ptr(), 0.99, 0.95, adv.data_ptr(), ret.data_ptr()], b"stride")
    # ... and through the Python layer a refusal is an error, not a fallback
    with pytest.raises(StepperError):
        L.minibatch((obs, act, old_logp, adv, ret), N, idx.data_ptr() + 4, N, 1)
    with pytest.raises(ValueError):
        L.update(obs, act, old_logp.double(), adv, ret, 1, N, 1)
    torch.cuda.synchronize()
    assert bool((ws == -7.0).all())
    for a, b in zip(before, (L.flat, L.grad, L.exp_avg, L.exp_avg_sq)):
        assert torch.equal(a, b)
    assert ctypes.sizeof(ctypes.c_longlong) == 8
