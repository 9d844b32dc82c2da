"""tb_ppo_grad + TB_PPO_REDUCE (through FusedLearner's buffers, both env kinds) and tb_ppo_grad_net with TB_NET_TUNED on the edge
fixtures of tests/learner_edge_fixtures.py: tanh saturated and overflowing, log_std at -5 / +2, every row of the minibatch cut off
by the clip, every row outside the clip range yet active, ratios of e^+-20, constant advantages and advantages with a large common
offset. B = 17, 129 and 257 through an index vector with a repeat and two out-of-range entries. Every run is held to
ppo_reference.MULTIPLE float32-twin errors per tensor against the float64 reference (learner_edge_fixtures.check: a tensor that is
exactly 0 in the reference and in its twin must be exactly 0 on the device), and to the exact values derived in the fixtures'
docstring. The largest ratios are printed at the end of the module and quoted in DESIGN.md."""
import numpy as np
import pytest

import learner_edge_fixtures as lf
import ppo_reference as ref
import trpo_reference as tr
import tuned_reference as tref
from test_ppo_reference import make_policy

pytestmark = pytest.mark.gpu

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
        print("learner edges (gpu): largest %s = %.3g" % (k, RATIOS[k]))


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def h(x):
    return x.detach().cpu().numpy().copy()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def make_learner(torch, f, **hp):
    from tennisbot_rl_amd.learner import FusedLearner
    policy = make_policy(f.arch, f.kind)
    policy.load_state_dict({k: torch.from_numpy(v.astype(np.float32)) for k, v in f.P.items()})
    policy = policy.to(DEV)
    opt = torch.optim.Adam(policy.parameters(), lr=f.hp["learning_rate"], eps=1e-5)
    return FusedLearner(f.kind, policy, opt, dict(f.hp, **hp), torch.device(DEV))


def device_gradient(torch, L, arrays, idx_d, batch, **hp):
    """tb_ppo_grad_net + TB_PPO_REDUCE into the learner's own buffers: (named gradient, the three statistics)"""
    from tennisbot_rl_amd.learner import TB_PPO_REDUCE
    hp = dict(L.hp, **hp)
    lib, s = L.lib, torch.cuda.current_stream().cuda_stream
    ws = L.workspace(batch)
    wb = ws.numel() * 8
    L.grad.fill_(7.0); L.stats.fill_(7.0)
    rc = lib.tb_ppo_grad_net(L.kind, L.net, 0, s, *(a.data_ptr() for a in arrays), int(arrays[3].shape[0]), idx_d.data_ptr(), batch, L.flat.data_ptr(), L.n_params,
                             float(hp["clip_range"]), float(hp["vf_coef"]), ws.data_ptr(), wb)
    assert rc == 0, lib.tb_last_error()
    rc = lib.tb_ppo_apply_net(L.kind, L.net, 0, s, TB_PPO_REDUCE, ws.data_ptr(), wb, batch, L.flat.data_ptr(), L.grad.data_ptr(), L.exp_avg.data_ptr(), L.exp_avg_sq.data_ptr(),
                              L.n_params, L.stats.data_ptr(), float(hp["ent_coef"]), float(hp["max_grad_norm"]), 1, float(hp["learning_rate"]), 0.9, 0.999, 1e-5, 1)
    assert rc == 0, lib.tb_last_error()
    torch.cuda.synchronize()
    return h(L.grad), h(L.stats)


def policy_net_slots(named):
    return {k: v for k, v in named.items() if tr.is_theta(k) and k != "log_std"}


def exact_claims(tag, which, named, stats, ent_coef):
    """the values derived for the regime, bit for bit"""
    if which == "overflow":
        for body in ("policy_net", "value_net_body"):       # h = +-1 exactly, dz = 0 exactly: units 0 and 1 of the first layer
            assert not bits(named[body + ".0.weight"][:2]).any() and not bits(named[body + ".0.bias"][:2]).any(), "%s: %s units 0 / 1 hold a non-zero bit" % (tag, body)
    if which in ("all_inactive", "constant_adv", "constant_adv_tenth"):
        for k, v in policy_net_slots(named).items():
            assert not np.any(v), "%s: %s must be exactly zero" % (tag, k)
        assert np.array_equal(named["log_std"], np.full_like(named["log_std"], -np.float32(ent_coef))), "%s: log_std's gradient is not -ent_coef" % tag
    if which in ("constant_adv", "constant_adv_tenth"):
        assert stats[0] == 0.0, "%s: policy_loss %r" % (tag, stats[0])


@pytest.mark.parametrize("which", lf.REGIMES)
@pytest.mark.parametrize("kname", list(lf.CASE))
def test_gradient_on_the_edge_fixture(torch, kname, which):
    f = lf.build(kname, which)
    L = make_learner(torch, f)
    arrays = tuple(dev(torch, x[:lf.N_ROWS]) for x in f.data)
    for B in lf.SIZES:
        tag = "%s %s B = %d" % (kname, which, B)
        idx, rows = lf.gpu_rows(f, "grad", B)
        idx_d = dev(torch, idx)
        g, stats = device_gradient(torch, L, arrays, idx_d, B)
        g2, stats2 = device_gradient(torch, L, arrays, idx_d, B)
        assert np.array_equal(bits(g), bits(g2)) and np.array_equal(bits(stats), bits(stats2)), "%s: a second run gave other bits" % tag
        named = tr.split_flat(g, f.P)
        want, twin = (ref.loss_and_grads(f.P, *lf.rows_of(f, rows), f.hp, dt) for dt in (np.float64, np.float32))
        got = dict(named, **dict(zip(("policy_loss", "value_loss", "entropy"), stats.astype(np.float64))))
        r = lf.ratios(got, lf.checked(want), lf.checked(twin))
        worst = max(r, key=r.get)
        print("%s: %.3g twin errors (%s); active %.2f" % (tag, r[worst], worst, want.active.mean()))
        exact_claims(tag, which, named, stats, f.hp["ent_coef"])
        if which == "all_active_outside":       # the clip must change nothing: the same call with clip_range = inf, bit for bit
            gi, si = device_gradient(torch, L, arrays, idx_d, B, clip_range=float("inf"))
            assert np.array_equal(bits(g), bits(gi)) and np.array_equal(bits(stats), bits(si)), "%s: the clip changed a bit" % tag
        note("gradient and statistics error / twin error, %s" % which, lf.check(tag, got, lf.checked(want), lf.checked(twin)))


@pytest.mark.parametrize("kname", list(lf.CASE))
def test_a_step_on_a_zero_gradient_moves_nothing(torch, kname):
    """all_inactive with the value and entropy coefficients 0: the whole gradient is 0, its norm 0, the clip factor 1 and Adam's
    update 0 / (0 + eps) on zero moments: every parameter keeps its bits"""
    f = lf.build(kname, "all_inactive")
    arrays = tuple(dev(torch, x[:lf.N_ROWS]) for x in f.data)
    for B in lf.SIZES:
        L = make_learner(torch, f, vf_coef=0.0, ent_coef=0.0)
        before = h(L.flat)
        idx_d = dev(torch, lf.gpu_rows(f, "grad", B)[0])
        L.minibatch(arrays, lf.N_ROWS, idx_d.data_ptr(), B, 1)
        torch.cuda.synchronize()
        after = h(L.flat)
        assert np.isfinite(after).all() and np.array_equal(bits(after), bits(before)), "%s B = %d: a step on a zero gradient moved a parameter" % (kname, B)
        for x in (L.grad, L.exp_avg, L.exp_avg_sq):
            assert not h(x).any()
        assert np.isfinite(h(L.stats)).all()


# --------------------------------------------------------------------------------------------------------------- the tuned net
@pytest.mark.parametrize("name,which", lf.TUNED_CASES)
def test_tuned_gradient_on_the_edge_fixture(torch, name, which):
    from tennisbot_rl_amd.params import ENV_TENNIS, NET_TUNED
    from tennisbot_rl_amd.stepper import load_library
    from test_gpu_tuned_learner import device_gradient as tuned_gradient
    from test_tuned_reference import N_PARAMS
    lib = load_library()
    P, hp, data, kept, pool = lf.tuned_fixture(name, which)
    assert kept >= max(lf.N_ROWS, pool // 2)
    data = tuple(x[:lf.N_ROWS] for x in data)
    flat = tref.flat(P).astype(np.float32)
    for B in lf.SIZES:
        tag = "tuned %s %s B = %d" % (name, which, B)
        idx, rows = lf.tuned_rows(name, which, B)
        g, stats = tuned_gradient(torch, lib, ENV_TENNIS, NET_TUNED, N_PARAMS, flat, data, idx, hp)
        named = tref.unflat(g)
        batch = tuple(x[rows] for x in data)
        want, twin = tref.loss_and_grads(P, *batch, hp), tref.loss_and_grads(P, *batch, hp, np.float32)
        if which != "constant_adv_tenth":
            assert np.array_equal(want.active, twin.active)
        assert which != "all_inactive" or not want.active.any()
        got = dict(named, **dict(zip(("policy_loss", "value_loss", "entropy"), stats.astype(np.float64))))
        r = lf.ratios(got, lf.checked(want), lf.checked(twin))
        worst = max(r, key=r.get)
        print("%s: %.3g twin errors (%s)" % (tag, r[worst], worst))
        exact_claims(tag, which, named, stats, hp["ent_coef"])
        note("tuned gradient and statistics error / twin error, %s" % which, lf.check(tag, got, lf.checked(want), lf.checked(twin)))
