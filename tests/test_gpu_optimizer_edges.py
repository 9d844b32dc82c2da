"""tb_ppo_step_kernel (behind tb_ppo_apply_net with TB_PPO_STEP and tb_ppo_apply_members) and sac_adam_kernel / sac_polyak_kernel
(behind tb_sac_adam) on a real MI355X, held BIT FOR BIT to their restatement in numpy float32 (tests/optimizer_edge_fixtures.py) at
the edges of their arguments: the step counts where c1 and c2 become 1.0f and one beyond 2^31, clip bounds that put the factor next
to 1.0f, a world that is no power of two, moments and gradients that underflow, go denormal and overflow, and non-finite gradients.
tests/test_optimizer_edges_reference.py holds that restatement to ppo_reference in float64 and to torch, and shows that this
comparison rejects seven one-line mutants of it.

Every launch is one workgroup per member or a few hundred threads. Every device array is NaN-padded past its length and the pad is
checked after each call. Comparisons are of uint32 views; where the restatement holds a NaN the device must hold one (any payload).

The clip rule (include/tb_stepper.h): the factor keeps a NaN, as torch's clamp does. With fminf, which drops it, the
non-finite cases whose factor is NaN fail in every slot but the planted one. Run once on an MI355X against a library built with the
previous fminf line: the twelve (net, case) pairs with a NaN or inf / inf norm and the members test failed ("params differs from
the restatement in 9068 of 9069 slots"), the other 36 tests passed; the fminf_clip mutant shows the same on the CPU."""
import numpy as np
import pytest

import optimizer_edge_fixtures as fx
from tennisbot_rl_amd.params import ENV_SWING, NET_MLP64

pytestmark = pytest.mark.gpu

F = fx.F
DEV = "cuda:0"
PAD = 64
TB_PPO_STEP, TB_PPO_VALUE_ONLY = 2, 4
HP = dict(lr=fx.LR, beta1=fx.BETA1, beta2=fx.BETA2, eps=fx.ADAM_EPS)
ARRAYS = ("params", "grad", "exp_avg", "exp_avg_sq")
CRITIC_NETS = [n for n in fx.NETS if fx.Layout(n).critic]
SAC_SIZES = (1, 255, 256, 257, 1025)
TAUS = (0.005, 0.37, 1.0, 0.0)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def lib(torch):
    from tennisbot_rl_amd.stepper import load_library
    return load_library()


def padded(torch, x):
    out = torch.full((len(x) + PAD,), float("nan"), dtype=torch.float32, device=DEV)
    out[:len(x)].copy_(torch.from_numpy(np.ascontiguousarray(x, F)))
    return out


def unpadded(torch, arrays, n):
    torch.cuda.synchronize()
    host = [a.cpu().numpy() for a in arrays]
    for k, a in enumerate(host):
        assert np.isnan(a[n:]).all() and len(a) == n + PAD, "array %d of the call: the floats past the vector's length were written" % k
    return [a[:n].copy() for a in host]


def device_step(torch, lib, L, vec, *, world, max_norm, step, value_only=False):
    """tb_ppo_apply_net(TB_PPO_STEP) alone on NaN-padded copies of (p, g, m, v): no workspace, no statistics, grad_dev is the input"""
    assert lib.tb_ppo_param_floats_net(L.kind, L.net) == L.P == len(vec[0])
    arrays = [padded(torch, x) for x in vec[:4]]
    s = torch.cuda.current_stream().cuda_stream
    rc = lib.tb_ppo_apply_net(L.kind, L.net, 0, s, TB_PPO_STEP | (TB_PPO_VALUE_ONLY if value_only else 0), None, 0, 0, *(a.data_ptr() for a in arrays), L.P, None,
                              0.0, float(max_norm), world, fx.LR, fx.BETA1, fx.BETA2, fx.ADAM_EPS, step)
    assert rc == 0, lib.tb_last_error()
    return unpadded(torch, arrays, L.P)


def same(tag, got, want, classes=None):
    for name, a, b in zip(ARRAYS, got, want):
        if not fx.same_bits(a, b):
            bad = np.flatnonzero(~((fx.bits(a) == fx.bits(b)) | (np.isnan(a) & np.isnan(b))))
            k = int(bad[0])
            raise AssertionError("%s: %s differs from the restatement in %d of %d slots; first slot %d%s: device %r (0x%08x), restated %r (0x%08x)"
                                 % (tag, name, len(bad), len(b), k, "" if classes is None else " (%s)" % classes[k], a[k], fx.bits(a)[k], b[k], fx.bits(b)[k]))


# -------------------------------------------------------------------------------------------- tb_ppo_apply_net(TB_PPO_STEP) alone
@pytest.mark.parametrize("name", list(fx.NETS))
def test_step_is_the_restatement_at_every_step_count(torch, lib, name):
    L = fx.Layout(name)
    _, vec, bounds = fx.sharpest_case(L.P, 1, L.everything)
    for step in fx.steps():
        kw = dict(world=1, max_norm=bounds["binds"], step=step)
        same("%s step %d" % (name, step), device_step(torch, lib, L, vec, **kw), fx.step_restated(*vec[:4], ranges=L.everything, **kw, **HP), vec[4])


@pytest.mark.parametrize("name", list(fx.NETS))
def test_step_is_the_restatement_at_every_clip_bound(torch, lib, name):
    L = fx.Layout(name)
    seed, vec, bounds = fx.sharpest_case(L.P, 1, L.everything)
    for which, b in bounds.items():
        kw = dict(world=1, max_norm=b, step=7)
        got = device_step(torch, lib, L, vec, **kw)
        same("%s bound %s = %.9g (seed %d)" % (name, which, b, seed), got, fx.step_restated(*vec[:4], ranges=L.everything, **kw, **HP), vec[4])
        if which in ("just_misses", "exact_one", "inf"):          # a clip that misses leaves the gradient's bits alone
            assert np.array_equal(fx.bits(got[1]), fx.bits(vec[1])), which
        else:
            assert not np.array_equal(fx.bits(got[1]), fx.bits(vec[1])), which


@pytest.mark.parametrize("world", (1, 2, 3))
@pytest.mark.parametrize("name", list(fx.NETS))
def test_step_is_the_restatement_at_every_world(torch, lib, name, world):
    L = fx.Layout(name)
    _, vec, bounds = fx.sharpest_case(L.P, world, L.everything)
    for which in ("binds", "just_below", "just_misses"):
        kw = dict(world=world, max_norm=bounds[which], step=7)
        same("%s world %d %s" % (name, world, which), device_step(torch, lib, L, vec, **kw), fx.step_restated(*vec[:4], ranges=L.everything, **kw, **HP), vec[4])


@pytest.mark.parametrize("name", list(fx.NETS))
def test_step_is_the_restatement_on_extreme_magnitudes(torch, lib, name):
    L = fx.Layout(name)
    vec = fx.vectors(L.P, 7, with_extremes=True)
    for world in (1, 3):
        for step in fx.steps():
            kw = dict(world=world, max_norm=np.inf, step=step)
            got = device_step(torch, lib, L, vec, **kw)
            same("%s extremes world %d step %d" % (name, world, step), got, fx.step_restated(*vec[:4], ranges=L.everything, **kw, **HP), vec[4])
            if world == 1:
                fx.class_invariants(vec[4], vec[:4], got, step)
                assert np.array_equal(fx.bits(got[1]), fx.bits(vec[1]))


# ------------------------------------------------------------------------------------------------ TB_PPO_VALUE_ONLY | TB_PPO_STEP
def with_sentinels(L, vec):
    """NaN in every 97th policy slot of the gradient: the critic's norm must not see them, and no array's policy slot may change"""
    p, g, m, v, classes = vec
    g = g.copy()
    policy = np.flatnonzero(fx.mask_of(L.P, L.policy))
    g[policy[::97]] = np.nan
    return p, g, m, v, classes


@pytest.mark.parametrize("name", CRITIC_NETS)
def test_value_only_step_is_the_critics_alone(torch, lib, name):
    L = fx.Layout(name)
    critic = fx.mask_of(L.P, L.critic)
    seed, vec, bounds = fx.sharpest_case(L.P, 1, L.critic)
    cases = [(with_sentinels(L, vec), which, b, 7) for which, b in bounds.items()]
    cases += [(with_sentinels(L, fx.vectors(L.P, 9, with_extremes=True)), "inf, extremes", np.inf, step) for step in (1, fx.step_edges()[1])]
    for v_, which, b, step in cases:
        kw = dict(world=1, max_norm=b, step=step)
        got = device_step(torch, lib, L, v_, value_only=True, **kw)
        tag = "%s value-only %s step %d (seed %d)" % (name, which, step, seed)
        same(tag, got, fx.step_restated(*v_[:4], ranges=L.critic, **kw, **HP), v_[4])
        for arr, a, b0 in zip(ARRAYS, got, v_[:4]):
            assert np.array_equal(fx.bits(a)[~critic], fx.bits(b0)[~critic]), "%s: a policy slot of %s changed" % (tag, arr)
        assert np.isfinite(got[0]).all() and (fx.bits(got[0])[critic] != fx.bits(v_[0])[critic]).any()
        if which in ("just_misses", "exact_one", "inf"):
            assert np.array_equal(fx.bits(got[1]), fx.bits(v_[1])), which


# ------------------------------------------------------------------------------------------------------------ non-finite gradients
@pytest.mark.parametrize("case", fx.NONFINITE_CASES)
@pytest.mark.parametrize("name", list(fx.NETS))
def test_nonfinite_gradient_reaches_every_participating_slot_as_in_torch(torch, lib, name, case):
    L = fx.Layout(name)
    p, g0, m, v, classes = fx.vectors(L.P, 21)
    for ranges in (L.everything,) + ((L.critic,) if L.critic else ()):
        g, max_norm = fx.nonfinite_case(case, g0, ranges)
        mask = fx.mask_of(L.P, ranges)
        kw = dict(world=1, max_norm=max_norm, step=7)
        got = device_step(torch, lib, L, (p, g, m, v), value_only=ranges is not L.everything, **kw)
        want = fx.step_restated(p, g, m, v, ranges=ranges, **kw, **HP)
        same("%s %s%s" % (name, case, "" if ranges is L.everything else " value-only"), got, want, classes)
        for arr, before, a, b in zip(ARRAYS, (p, g, m, v), got, want):
            assert np.array_equal(fx.pattern(before, a), fx.pattern(before, b)), arr
            nan = int(np.isnan(a).sum())
            assert nan == (1 if case == "inf_slot" else int(mask.sum())), (arr, nan)         # torch: every slot, or [0, nan, 0, 0]
            assert np.array_equal(fx.bits(a)[~mask], fx.bits(before)[~mask]), arr


# --------------------------------------------------------------------------------------------------------- tb_ppo_apply_members
def test_a_diverged_member_leaves_its_neighbours_rows_alone(torch, lib):
    """(swing, mlp64), three members at the smallest batch of test_gpu_learner_members' cases; member 1 carries one NaN weight"""
    import test_gpu_learner_members as tm
    kind, net = ENV_SWING, NET_MLP64
    batch = min(b for k, n, b in tm.CASES if (k, n) == (kind, net))
    P = lib.tb_ppo_param_floats_net(kind, net)
    L = fx.Layout("swing-mlp64")
    assert P == L.P and tm.M == 3
    rows = tm.device_rows(torch, kind)
    state = tuple(x.clone() for x in tm.member_state(torch, kind, net, P))
    state[0][1, L.policy[0][0] + 16] = float("nan")          # a first-layer weight of member 1's policy tower
    g = torch.Generator().manual_seed(100 + batch)
    idx = torch.stack([torch.randperm(tm.N_ROWS, generator=g) for _ in range(tm.M)])[:, :batch + 5].contiguous().to(DEV)
    got = tm.run_members(torch, lib, kind, net, batch, rows, idx, state, tm.HP)      # (checks that the floats between rows are still NaN)
    names = ARRAYS + ("stats",)
    for m in range(tm.M):
        want = tm.run_single(torch, lib, kind, net, batch, rows, idx[m], tuple(x[m] for x in state), tm.HP[m])
        for name, g_, w_ in zip(names, got, want):
            if m != 1:
                assert np.isfinite(w_).all() and np.array_equal(fx.bits(g_[m]), fx.bits(w_)), (m, name)
            else:
                assert fx.same_bits(g_[m], w_), (m, name)
        if m != 1:
            assert np.any(want[0] != state[0][m].cpu().numpy())
    # the critic's tower never sees the NaN weight; the norm does, and the rule sends it to every slot of member 1's four rows
    for name, g_ in zip(ARRAYS, got):
        assert np.isnan(g_[1]).all(), name


# ------------------------------------------------------------------------------------------------------------------- tb_sac_adam
def device_adam(torch, lib, n, p, g, m, v, step, target=None, tau=0.0):
    """tb_sac_adam on NaN-padded copies; g, m, v None: the Polyak update alone. Returns [p, (m, v,) (target)] as the call took them."""
    arrays = [padded(torch, x) if x is not None else None for x in (p, g, m, v, target)]
    ptr = [a.data_ptr() if a is not None else None for a in arrays]
    s = torch.cuda.current_stream().cuda_stream
    rc = lib.tb_sac_adam(0, s, ptr[0], ptr[1], ptr[2], ptr[3], n, fx.LR, fx.BETA1, fx.BETA2, fx.ADAM_EPS, step, ptr[4], float(tau))
    assert rc == 0, lib.tb_last_error()
    out = unpadded(torch, [a for a in arrays if a is not None], n)
    return dict(zip([k for k, a in zip(("p", "g", "m", "v", "target"), arrays) if a is not None], out))


@pytest.mark.parametrize("n", SAC_SIZES)
def test_sac_adam_and_polyak_are_the_restatement(torch, lib, n):
    p, g, m, v, classes = fx.vectors(n, 30 + n, with_extremes=True)
    t0 = np.random.default_rng(n).normal(0.0, 1.0, n).astype(F)
    assert t0.all()
    for step in fx.steps():
        pn, mn, vn = fx.adam_restated(p, g, m, v, step=step, **HP)
        assert np.isfinite(pn).all()
        if n >= 256:        # (every class has 16 slots or more)
            fx.class_invariants(classes, (p, g, m, v), (pn, g, mn, vn), step)
        for tau in (None,) + TAUS:
            got = device_adam(torch, lib, n, p, g, m, v, step, None if tau is None else t0, 0.0 if tau is None else tau)
            tag = "n = %d step %d tau %s" % (n, step, tau)
            same(tag, (got["p"], got["g"], got["m"], got["v"]), (pn, g, mn, vn), classes)
            if tau is not None:
                assert fx.same_bits(got["target"], fx.polyak_restated(pn, t0, tau)), tag
                if tau == 0.0:
                    assert np.array_equal(fx.bits(got["target"]), fx.bits(t0)), tag
                if tau == 1.0:
                    assert np.array_equal(fx.bits(got["target"]), fx.bits(pn)), tag
    # the Polyak update alone: the same target bits on parameters it leaves unchanged
    for tau in TAUS:
        got = device_adam(torch, lib, n, p, None, None, None, 1, t0, tau)
        assert np.array_equal(fx.bits(got["p"]), fx.bits(p)) and fx.same_bits(got["target"], fx.polyak_restated(p, t0, tau)), (n, tau)
