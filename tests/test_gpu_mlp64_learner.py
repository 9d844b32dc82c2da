"""The learner kernels instantiated for TB_NET_MLP64 (tb_ppo_grad_net, tb_ppo_apply_net: SB3's [64, 64] on SwingRacket-v0) on the device,
against the float64 reference of tests/ppo_reference.py with its own tolerance: ppo_reference.MULTIPLE float32-twin errors per tensor in
the max norm. Minibatch sizes on both sides of the 16-row tile, of a wave's half share (128) and of a workgroup's share (256), through
index vectors with a repeat and two out-of-range entries; the critic-only step; max_grad_norm = inf; PPOTrainer(policy="mlp64") with
the fused learner beside the torch learner on the same rollouts. (tb_ppo_gae does not depend on the net: tests/test_gpu_learner.py.)"""
import numpy as np
import pytest

import mlp64_fixtures as fx
import ppo_reference as ref
import trpo_reference as tr
from policy_reference import state_dict_arrays
from test_ppo_reference import flat_shard

pytestmark = pytest.mark.gpu

MULTIPLE = ref.MULTIPLE
DEV = "cuda:0"
SIZES = (2, 15, 16, 17, 127, 128, 129, 255, 256, 257, 600)
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
        print("mlp64 learner (gpu): largest %s = %.3g" % (k, RATIOS[k]))


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def h(x):
    return x.detach().cpu().numpy().copy()


def make_learner(torch, ro, **hp):
    from tennisbot_rl_amd.learner import FusedLearner
    from tennisbot_rl_amd.params import NET_MLP64
    policy = fx.policy().to(DEV)
    opt = torch.optim.Adam(policy.parameters(), lr=ro.hp["learning_rate"], eps=1e-5)
    L = FusedLearner(ro.kind, policy, opt, dict(ro.hp, **hp), torch.device(DEV))
    assert L.net == NET_MLP64 and L.n_params == fx.PARAM_FLOATS
    return L


@pytest.mark.parametrize("B", SIZES)
def test_three_adam_steps_on_one_minibatch(torch, B):
    ro = fx.rollout()
    N = ro.T * ro.n
    full = flat_shard(ro, ro.gae.adv, ro.gae.returns)
    arrays = tuple(dev(torch, x) for x in full)
    idx, rows = fx.index_vector(N, B, 300 + B)
    idx_d = dev(torch, idx)
    shard = tuple(x[rows] for x in full)
    runs = []
    for _ in range(2):
        L = make_learner(torch, ro)
        P = state_dict_arrays(L.policy)
        for step in (1, 2, 3):
            L.minibatch(arrays, N, idx_d.data_ptr(), B, step)
        torch.cuda.synchronize()
        runs.append([L.flat.clone(), L.grad.clone(), L.exp_avg.clone(), L.exp_avg_sq.clone(), L.stats.clone()])
    for a, b in zip(*runs):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), "B = %d: a second run gave other bits" % B
    perms = [[np.arange(B)] * 3]
    want, twin = ref.replay_update(P, [shard], perms, B, L.hp), ref.replay_update(P, [shard], perms, B, L.hp, np.float32)
    assert len(want.norms) == 3
    grads = tr.split_flat(h(L.grad), P)
    stats = dict(zip(("policy_loss", "value_loss", "entropy"), (np.float64(v) for v in h(L.stats))))
    lr = L.hp["learning_rate"]
    g = note("gradient error / twin error", ref.check_tensors("B = %d gradient" % B, grads, want.grads, twin.grads, MULTIPLE))
    s = note("statistics error / twin error", ref.check_tensors("B = %d statistics" % B, stats, want.stats[0], twin.stats[0], MULTIPLE))
    p = note("parameter change error / twin error", ref.check_tensors("B = %d parameters" % B, ref.param_change(tr.split_flat(h(L.flat).astype(np.float64), P), P, lr),
                                                                     ref.param_change(want.params, P, lr), ref.param_change(twin.params, P, lr), MULTIPLE))
    m = {"m": tr.split_flat(h(L.exp_avg), P), "v": tr.split_flat(h(L.exp_avg_sq), P)}
    s64, s32 = ref.adam_init(P), ref.adam_init(P, np.float32)
    ref.replay_update(P, [shard], perms, B, L.hp, adam_state=s64); ref.replay_update(P, [shard], perms, B, L.hp, np.float32, adam_state=s32)
    a = note("Adam moment error / twin error", max(ref.check_tensors("B = %d exp_avg" % B, m["m"], s64["m"], s32["m"], MULTIPLE),
                                                   ref.check_tensors("B = %d exp_avg_sq" % B, m["v"], s64["v"], s32["v"], MULTIPLE)))
    print("B = %3d: gradient %.3g, statistics %.3g, parameters %.3g, moments %.3g twin errors; pre-clip norms %s" % (B, g, s, p, a, " ".join("%.3g" % x for x in want.norms)))


def test_value_only_and_an_infinite_norm_bound(torch):
    """TB_PPO_VALUE_ONLY is offered for this net (separate towers): the policy slots of parameters, gradient and both moments keep their
    bits, the value slots take the reference's critic-only Adam step. max_grad_norm = inf: the clip factor is exactly 1 -- the bits of a
    bound that cannot bind, and the gradient TB_PPO_REDUCE left is the gradient TB_PPO_STEP leaves."""
    ro = fx.rollout()
    L = make_learner(torch, ro)
    lib, kind, net, Pn = L.lib, ro.kind, L.net, L.n_params
    P = state_dict_arrays(L.policy)
    rows = np.random.default_rng(12).permutation(ro.T * ro.n)[:600]
    shard = tuple(x[rows] for x in flat_shard(ro, ro.gae.adv, ro.gae.returns))
    N = len(rows)
    arrays = tuple(dev(torch, x) for x in shard)
    idx = torch.arange(N, device=DEV)
    rng = np.random.default_rng(13)
    m0, v0 = (rng.normal(0.0, 1e-3, Pn)).astype(np.float32), (rng.random(Pn) * 1e-5 + 1e-8).astype(np.float32)
    g0 = rng.normal(0.0, 1.0, Pn).astype(np.float32)
    flat0 = L.flat.clone()
    value = np.array([not tr.is_theta(k) for k, v in P.items() for _ in range(int(np.size(v)))])
    assert value.sum() == 64 * 7 + 64 * 65 + 65
    s = torch.cuda.current_stream().cuda_stream
    ws = L.workspace(N)
    wb = ws.numel() * 8
    lr, STEP = 1e-3, 4

    def run(phase_list, max_norm):
        L.flat.copy_(flat0); L.grad.copy_(dev(torch, g0)); L.exp_avg.copy_(dev(torch, m0)); L.exp_avg_sq.copy_(dev(torch, v0)); L.stats.zero_()
        rc = lib.tb_ppo_grad_net(kind, net, 0, s, *(a.data_ptr() for a in arrays), N, idx.data_ptr(), N, L.flat.data_ptr(), Pn, 0.2, 1.0, ws.data_ptr(), wb)
        assert rc == 0, lib.tb_last_error()
        for ph in phase_list:
            rc = lib.tb_ppo_apply_net(kind, net, 0, s, ph, ws.data_ptr(), wb, N, L.flat.data_ptr(), L.grad.data_ptr(), L.exp_avg.data_ptr(), L.exp_avg_sq.data_ptr(), Pn,
                                      L.stats.data_ptr(), 0.002, max_norm, 1, lr, 0.9, 0.999, 1e-5, STEP)
            assert rc == 0, lib.tb_last_error()
        torch.cuda.synchronize()
        return [h(x) for x in (L.flat, L.grad, L.exp_avg, L.exp_avg_sq, L.stats)]

    bits = lambda x: x.view(np.uint32)  # noqa: E731
    names = [k for k in P if not tr.is_theta(k)]
    sub = lambda flat: {k: v for k, v in tr.split_flat(flat, P).items() if k in names}  # noqa: E731
    hp = dict(ro.hp, vf_coef=1.0)
    for max_norm in (0.5, float("inf")):
        only = run([1 | 2 | 4], max_norm)
        for got, before in zip(only[:4], (h(flat0), g0, m0, v0)):                  # the policy slots: not written, bit for bit
            assert np.array_equal(bits(got[~value]), bits(before[~value]))
        assert not np.array_equal(only[0][value], h(flat0)[value])
        res = {}
        for dtype in (np.float64, np.float32):
            grads = ref.loss_and_grads(P, *shard, hp, dtype).grads
            gv, norm = ref.clip_global_norm({k: grads[k] for k in names}, max_norm, dtype)
            state = {"t": STEP - 1, "m": {k: tr.split_flat(m0, P)[k].astype(dtype) for k in names}, "v": {k: tr.split_flat(v0, P)[k].astype(dtype) for k in names}}
            new = ref.adam_step({k: P[k] for k in names}, gv, state, lr, dtype=dtype)
            res[dtype] = (ref.param_change(new, {k: P[k] for k in names}, lr), gv, norm)
        got_change = ref.param_change(sub(only[0].astype(np.float64)), {k: P[k] for k in names}, lr)
        note("critic parameter change / twin error", ref.check_tensors("value parameters", got_change, res[np.float64][0], res[np.float32][0], MULTIPLE))
        note("critic gradient / twin error", ref.check_tensors("value gradient", sub(only[1]), res[np.float64][1], res[np.float32][1], MULTIPLE))
        if max_norm == 0.5:
            assert res[np.float64][2] > 2.0 * max_norm, "the critic's own norm clip was meant to be active here"
    # max_grad_norm = inf, every slot: the bits of a bound that cannot bind, and the reduced gradient untouched by the step
    reduced = run([1], float("inf"))
    unbounded, huge = run([1 | 2], float("inf")), run([1 | 2], 1e30)
    for a, b in zip(unbounded, huge):
        assert np.isfinite(a).all() and np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(unbounded[1]), bits(reduced[1])), "max_grad_norm = inf changed the gradient's bits"
    assert not np.array_equal(unbounded[0], h(flat0))
    clipped = run([1 | 2], 0.5)
    assert not np.array_equal(clipped[1], reduced[1])                            # (a bound that binds does change them)


_rollouts = {}


@pytest.mark.parametrize("learner", ["fused", "torch"])
def test_trainer_learners_on_the_same_rollout(torch, learner):
    """PPOTrainer("SwingRacket-v0", policy="mlp64") with learner="fused" and with learner="torch", at the shape of the default net's twin
    tests (tests/test_gpu_learner_trainer.py, tests/test_gpu_ppo_reference.py: 512 envs x 52 steps) and held exactly as those hold their
    trainers -- test_gpu_ppo_reference.check_learner: GAE within the reference's bound, then two updates against the float64 replay,
    a single-minibatch one (every gradient tensor and EACH of the three statistics on its own, ppo_reference.MULTIPLE twin errors) and
    two epochs of three minibatches (every parameter tensor's change). Both trainers have the same seed, so the fused collect hands
    them the same rollout: asserted bit for bit, and both are held to the one float64 reference of it."""
    from tennisbot_rl_amd.learner import FusedLearner
    from tennisbot_rl_amd.params import NET_MLP64
    from tennisbot_rl_amd.ppo import PPOTrainer
    from test_gpu_ppo_reference import check_learner
    tr = PPOTrainer("SwingRacket-v0", num_envs=512, n_steps=52, device=DEV, seed=3, policy="mlp64", n_epochs=2, learner=learner)
    assert tr.net == NET_MLP64 and tr.fused and tr.rollout_launch and tr.packed.numel() == fx.BLOB_FLOATS and tuple(tr.hp["net_arch"]) == (64, 64)
    assert isinstance(tr._learner, FusedLearner) == (learner == "fused")
    tr.collect()
    torch.cuda.synchronize()
    mine = {k: h(getattr(tr, k)) for k in ("obs_seq", "_raw_actions", "logps", "values", "last_value")}
    mine["rewards"], mine["dones"] = h(tr.buf.rewards), h(tr.buf.dones)
    for other in _rollouts.values():
        for k, v in mine.items():
            assert np.array_equal(v.view(np.uint8), other[k].view(np.uint8)), "%s: the two trainers did not collect the same rollout" % k
    _rollouts[learner] = mine
    dones, want = check_learner(torch, tr, "mlp64 %s learner, swing 512 x 52" % learner)
    assert np.array_equal(np.flatnonzero(dones.any(1)), [25, 51]) and dones[[25, 51]].all()
    c = tr.env.counters()
    assert c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0, c
    tr.env.close()
