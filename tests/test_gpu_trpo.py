"""The TRPO kernels (tb_trpo_fvp, tb_trpo_search, the critic-only tb_ppo_apply) and a real TRPOTrainer on the device, held to the
float64 reference of tests/trpo_reference.py with the tolerances of tests/ppo_reference.py: ppo_reference.MULTIPLE float32-twin
errors per tensor in the max norm. Both env kinds; the policy of test_ppo_reference.make_policy (log_std from -0.3 to 0.4, one
value per action; a mean that depends on the observation); vectors that are non-zero in every slot. The largest ratios are
printed at the end of the module."""
import numpy as np
import pytest

import ppo_reference as ref
import trpo_reference as tr
from learner_edge_fixtures import search_fixture
from policy_reference import state_dict_arrays
from test_ppo_reference import flat_shard, make_policy, rollout

pytestmark = pytest.mark.gpu

MULTIPLE = ref.MULTIPLE
DEV = "cuda:0"
CASE = {"swing": "swing-52-lockstep", "tennis": "tennis-70-ragged"}
ROWS = (2, 16, 17, 128, 129, 256, 257, 600)      # the tile, half-share and workgroup edges of tb_trpo_fvp
MARGIN = 100.0                                   # twin errors between every candidate's L / KL and its threshold
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
        print("trpo (gpu): largest %s = %.3g" % (k, RATIOS[k]))


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def h(x):
    return x.detach().cpu().numpy().copy()


def make_trpo(torch, ro, **hp):
    from tennisbot_rl_amd.trpo import FusedTRPO
    policy = make_policy(ro.arch, ro.kind).to(DEV)
    opt = torch.optim.Adam(policy.parameters(), lr=ro.hp["learning_rate"], eps=1e-5)
    return FusedTRPO(ro.kind, policy, opt, dict(ro.hp, **hp), torch.device(DEV))


def index_vector(N, m, seed):
    """m rows with repeats and entries outside [0, N), which the kernels clamp"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N, m).astype(np.int64)
    if m > 2:                                # (two rows stay two different rows: the advantages' std must not vanish)
        idx[0] = idx[m - 1]                  # a repeat
        idx[1], idx[m // 2] = -5, N + 7      # clamped to rows 0 and N - 1
    return idx, np.clip(idx, 0, N - 1)


# ------------------------------------------------------------------------------------------------------ Fisher-vector product
@pytest.mark.parametrize("kname", list(CASE))
def test_fvp_against_the_reference(torch, kname):
    ro = rollout(CASE[kname])
    L = make_trpo(torch, ro)
    P = state_dict_arrays(L.policy)
    N = ro.T * ro.n
    obs = ro.obs.reshape(N, -1)
    obs_d = dev(torch, obs)
    vec = np.random.default_rng(8).normal(0.0, 1.0, L.n_params).astype(np.float32)
    vec[np.abs(vec) < 1e-3] = 0.5
    vec_d, v = dev(torch, vec), tr.theta_of(tr.split_flat(vec.astype(np.float64), P))
    d32 = np.float32(tr.CG_DAMPING)
    mask = h(L.mask) != 0
    for m in ROWS:
        idx, rows = index_vector(N, m, 100 + m)
        idx_d = dev(torch, idx)
        out = [torch.full((L.n_params,), 7.0, device=DEV) for _ in range(3)]
        L.fvp(obs_d, idx_d.data_ptr(), m, vec_d, out[0])
        L.fvp(obs_d, idx_d.data_ptr(), m, vec_d, out[1])
        L.fvp(obs_d, idx_d.data_ptr(), m, vec_d, out[2], damping=0.0)
        assert torch.equal(out[0], out[1]), "m = %d: a second run gave other bits" % m
        got, plain = h(out[0]), h(out[2])
        assert np.isfinite(got).all() and not got[~mask].any() and not plain[~mask].any()          # the value slots: 0
        net = mask.copy(); net[:ro.A] = False
        assert np.array_equal(got[net], plain[net] + d32 * vec[net]), "m = %d: the damping term is not exact" % m
        assert np.array_equal(got[:ro.A], np.float32(2.0) * vec[:ro.A] + d32 * vec[:ro.A]) and np.array_equal(plain[:ro.A], np.float32(2.0) * vec[:ro.A])
        want, twin = tr.fvp(P, obs[rows], v, float(d32)), tr.fvp(P, obs[rows], v, float(d32), np.float32)
        gd = tr.theta_of(tr.split_flat(got, P))
        r = note("FVP error / twin error", ref.check_tensors("%s fvp m = %d" % (kname, m), gd, want, twin, MULTIPLE))
        print("%s: m = %3d, FVP %.3g twin errors" % (kname, m, r))


# ------------------------------------------------------------------------------------- the surrogate's gradient and the CG solve
@pytest.mark.parametrize("kname", list(CASE))
def test_gradient_and_conjugate_gradient_against_the_reference(torch, kname):
    """FusedTRPO.surrogate_gradient (tb_ppo_grad with a clip that never binds, negated, masked) against the reference's g, and
    FusedTRPO.conjugate_gradient (ten tb_trpo_fvp products, torch vector ops) against the reference's CG on the same rows"""
    ro = rollout(CASE[kname])
    L = make_trpo(torch, ro)
    P = state_dict_arrays(L.policy)
    N = ro.T * ro.n
    mask = h(L.mask) != 0
    rows = np.random.default_rng(21).permutation(N)[:1500]                  # six workgroups of the gradient kernel
    full = flat_shard(ro, ro.gae.adv, ro.gae.returns)
    arrays = tuple(dev(torch, f) for f in full)
    obs, act, old_logp, adv, _ = (f[rows] for f in full)
    rows_d = dev(torch, rows.astype(np.int64))
    g_t = L.surrogate_gradient(arrays, N, rows_d.data_ptr(), len(rows))
    got = h(g_t)
    assert g_t.dtype == torch.float32 and np.isfinite(got).all() and not got[~mask].any() and got[mask].any()
    want, twin = tr.surrogate_gradient(P, obs, act, old_logp, adv), tr.surrogate_gradient(P, obs, act, old_logp, adv, np.float32)
    r = note("g error / twin error", ref.check_tensors(kname + " surrogate gradient", tr.theta_of(tr.split_flat(got, P)), want, twin, MULTIPLE))
    # the sign, outright: g is the ascent direction of the surrogate
    step = 1e-3 / max(np.abs(v).max() for v in want.values())
    an = tr.normalise(adv)
    gain = tr.surrogate(tr.moved(P, tr.theta_of(tr.split_flat(got.astype(np.float64), P)), step), obs, act, old_logp, an) - tr.surrogate(P, obs, act, old_logp, an)
    assert gain > 0.5 * step * tr.dot(want, want), (gain, step * tr.dot(want, want))
    print("%s: g %.3g twin errors, |g| = %.3g" % (kname, r, np.sqrt(tr.dot(want, want))))
    # CG on 600 index entries (repeats, clamped entries), from the float32 g the device holds
    idx, cg_rows = index_vector(N, 600, 300)
    idx_d = dev(torch, idx)
    b = tr.theta_of(tr.split_flat(got.astype(np.float64), P))
    all_obs = full[0]
    x_t = L.conjugate_gradient(g_t, arrays[0], idx_d.data_ptr(), len(idx))
    x = h(x_t)
    assert x_t.dtype == torch.float64 and np.isfinite(x).all() and not x[~mask].any()
    damping = float(np.float32(tr.CG_DAMPING))
    history = []

    def product(dtype):
        def apply(p):
            history.append(tr.dot(p, p))
            return tr.fvp(P, all_obs[cg_rows], p, damping, dtype)
        return apply

    want_x = tr.conjugate_gradient(product(np.float64), b)
    assert len(history) == tr.CG_ITERATIONS, "the reference left its loop early: the device's freeze and it are not on the same path"
    twin_x = tr.conjugate_gradient(product(np.float32), b, dtype=np.float32)
    assert len(history) == 2 * tr.CG_ITERATIONS
    r = note("CG error / twin error", ref.check_tensors(kname + " conjugate gradient", tr.theta_of(tr.split_flat(x, P)), want_x, twin_x, MULTIPLE))
    # what the ten iterations bought: the residual of the solve, by the reference's own product
    res = tr.fvp(P, all_obs[cg_rows], tr.theta_of(tr.split_flat(x, P)), damping)
    xd = tr.theta_of(tr.split_flat(x, P))
    rel = np.sqrt(sum(((res[k] - b[k]) ** 2).sum() for k in b) / tr.dot(b, b))
    print("%s: CG %.3g twin errors, |F x - g| / |g| = %.3g" % (kname, r, rel))
    assert 0.5 * tr.dot(xd, res) - tr.dot(b, xd) < 0.0 < tr.dot(b, xd)      # every CG iterate lowers x^T F x / 2 - g^T x below its value at 0
    # the freeze: with a tolerance no residual reaches, x stays at 0 + the first iterate
    frozen = make_trpo(torch, ro, cg_tolerance=1e30)
    x1 = h(frozen.conjugate_gradient(g_t, arrays[0], idx_d.data_ptr(), len(idx)))
    one = tr.conjugate_gradient(lambda p: tr.fvp(P, all_obs[cg_rows], p, damping), b, iterations=1)
    one32 = tr.conjugate_gradient(lambda p: tr.fvp(P, all_obs[cg_rows], p, damping, np.float32), b, iterations=1, dtype=np.float32)
    note("CG (frozen after one iteration) error / twin error", ref.check_tensors(kname + " frozen CG", tr.theta_of(tr.split_flat(x1, P)), one, one32, MULTIPLE))


# ----------------------------------------------------------------------------------------------------------------- line search
@pytest.mark.parametrize("kname", list(CASE))
def test_search_against_the_reference(torch, kname):
    ro = rollout(CASE[kname])
    L = make_trpo(torch, ro)
    from tennisbot_rl_amd.trpo import select_candidate
    P = state_dict_arrays(L.policy)
    N = ro.T * ro.n
    share = L.lib.tb_trpo_search_rows_per_workgroup()
    picked = {}
    for m in ROWS + (share + 1,):
        idx, rows = index_vector(N, m, 200 + m)
        for which in ("kl", "none", "random"):
            (obs, act, old_logp, adv), x, steps = search_fixture(ro, P, rows, which)
            # the kernel gathers through idx from the full-size arrays; only old_logp may differ from the rollout's on these rows
            full = list(flat_shard(ro, ro.gae.adv, ro.gae.returns)[:4])
            full[2] = full[2].copy(); full[2][rows] = old_logp
            arrays = tuple(dev(torch, f) for f in full)
            xflat = tr.join_flat(x, P, np.float32)
            idx_d = dev(torch, idx)
            got_t = L.search(arrays, N, idx_d.data_ptr(), m, dev(torch, xflat), dev(torch, steps))
            got = h(got_t)
            s64 = steps.astype(np.float64)
            want, twin = tr.search_table(P, x, s64, obs, act, old_logp, adv), tr.search_table(P, x, s64, obs, act, old_logp, adv, np.float32)
            margins = tr.threshold_margins(want, twin)
            assert margins.min() > MARGIN, "%s m = %d %s: a candidate sits %.3g twin errors from its threshold: the fixture decides nothing" % (kname, m, which, margins.min())
            # one tensor per column, in the max norm over k: the float32 error of KL_k does not fall with KL_k (every row's
            # sigma^2 / (2 sigma'^2) - 1/2 cancels at the size of 1, so all ten candidates carry about the same absolute
            # error), and a single number's twin error scatters over orders of magnitude: no scale for one candidate
            t = lambda a: {"L": a[:, 0], "KL": a[:, 1]}  # noqa: E731
            r = note("search error / twin error", ref.check_tensors("%s search m = %d %s" % (kname, m, which), t(got), t(want), t(twin), MULTIPLE))
            k_want = tr.select(want)
            assert int(select_candidate(torch, got_t, tr.KL_DELTA)) == k_want == tr.select(got), (kname, m, which, got, want)
            if which == "kl":
                assert want[0, 1] > tr.KL_DELTA and k_want != 0
            if which == "none":
                assert k_want == -1
            picked.setdefault(which, set()).add(k_want)
            print("%s: m = %4d %-6s accepted %2d, search %.3g twin errors, smallest margin %.3g" % (kname, m, which, k_want, r, margins.min()))
            # a zero step: mu' == mu, KL exactly 0
            zero = h(L.search(arrays, N, idx_d.data_ptr(), m, dev(torch, xflat), dev(torch, np.zeros(tr.CANDIDATES, np.float32))))
            assert np.array_equal(zero[:, 1], np.zeros(tr.CANDIDATES)) and (zero[:, 0] == zero[0, 0]).all() and abs(zero[0, 0] - want[-1, 0]) < 0.1 + abs(want[-1, 0])
    assert picked["none"] == {-1} and max(picked["kl"]) >= 1, picked


# ------------------------------------------------------------------------------------------------------- the critic-only step
@pytest.mark.parametrize("kname", list(CASE))
def test_value_only_step(torch, kname):
    ro = rollout(CASE[kname])
    L = make_trpo(torch, ro)
    lib, kind, Pn = L.lib, ro.kind, L.n_params
    P = state_dict_arrays(L.policy)
    rows = np.random.default_rng(12).permutation(ro.T * ro.n)[:1500]
    shard = tuple(x[rows] for x in flat_shard(ro, ro.gae.adv, ro.gae.returns))
    N = len(rows)
    arrays = tuple(dev(torch, x) for x in shard)
    idx = torch.arange(N, device=DEV)
    rng = np.random.default_rng(13)
    m0, v0 = (rng.normal(0.0, 1e-3, Pn)).astype(np.float32), (rng.random(Pn) * 1e-5 + 1e-8).astype(np.float32)
    g0 = rng.normal(0.0, 1.0, Pn).astype(np.float32)
    flat0 = L.flat.clone()
    value = ~(h(L.mask) != 0)
    s = torch.cuda.current_stream().cuda_stream
    ws = L.workspace(N)
    wb = ws.numel() * 8
    lr, STEP = 3e-4, 4

    def run(phase_list, max_norm):
        L.flat.copy_(flat0); L.grad.copy_(dev(torch, g0)); L.exp_avg.copy_(dev(torch, m0)); L.exp_avg_sq.copy_(dev(torch, v0)); L.stats.zero_()
        rc = lib.tb_ppo_grad(kind, 0, s, *(a.data_ptr() for a in arrays), N, idx.data_ptr(), N, L.flat.data_ptr(), Pn, 0.2, 0.5, ws.data_ptr(), wb)
        assert rc == 0, lib.tb_last_error()
        for ph in phase_list:
            rc = lib.tb_ppo_apply(kind, 0, s, ph, ws.data_ptr(), wb, N, L.flat.data_ptr(), L.grad.data_ptr(), L.exp_avg.data_ptr(), L.exp_avg_sq.data_ptr(), Pn,
                                  L.stats.data_ptr(), 0.002, max_norm, 1, lr, 0.9, 0.999, 1e-5, STEP)
            assert rc == 0, lib.tb_last_error()
        torch.cuda.synchronize()
        return [h(x) for x in (L.flat, L.grad, L.exp_avg, L.exp_avg_sq, L.stats)]

    for max_norm in (0.5, 1e9):
        only = run([1 | 2 | 4], max_norm)
        for got, before in zip(only[:4], (h(flat0), g0, m0, v0)):                  # the policy slots: not written, bit for bit
            assert np.array_equal(got[~value].view(np.uint32), before[~value].view(np.uint32))
        assert not np.array_equal(only[0][value], h(flat0)[value])
        split = run([1 | 4, 2 | 4], max_norm)
        assert all(np.array_equal(a, b) for a, b in zip(only, split))
        # the reference: the value tensors' gradient, clipped by ITS OWN norm, one Adam step from the moments given
        names = [k for k in P if not tr.is_theta(k)]
        res = {}
        for dtype in (np.float64, np.float32):
            grads = ref.loss_and_grads(P, *shard, dict(ro.hp), dtype).grads
            gv, norm = ref.clip_global_norm({k: grads[k] for k in names}, max_norm, dtype)
            state = {"t": STEP - 1, "m": {k: tr.split_flat(m0, P)[k].astype(dtype) for k in names}, "v": {k: tr.split_flat(v0, P)[k].astype(dtype) for k in names}}
            new = ref.adam_step({k: P[k] for k in names}, gv, state, lr, dtype=dtype)
            res[dtype] = (ref.param_change(new, {k: P[k] for k in names}, lr), gv, state["m"], state["v"], norm)
        sub = lambda flat: {k: v for k, v in tr.split_flat(flat, P).items() if k in names}  # noqa: E731
        got_change = ref.param_change(sub(only[0].astype(np.float64)), {k: P[k] for k in names}, lr)
        note("critic parameter change / twin error", ref.check_tensors(kname + " value parameters", got_change, res[np.float64][0], res[np.float32][0], MULTIPLE))
        note("critic gradient / twin error", ref.check_tensors(kname + " value gradient", sub(only[1]), res[np.float64][1], res[np.float32][1], MULTIPLE))
        note("critic moments / twin error", max(ref.check_tensors(kname + " exp_avg", sub(only[2]), res[np.float64][2], res[np.float32][2], MULTIPLE),
                                                ref.check_tensors(kname + " exp_avg_sq", sub(only[3]), res[np.float64][3], res[np.float32][3], MULTIPLE)))
        # the phases that existed before: both at once == one after the other, and where no clip binds (in either norm) the
        # value slots of a full step are the critic-only step's, bit for bit
        full = run([1 | 2], max_norm)
        both = run([1, 2], max_norm)
        assert all(np.array_equal(a, b) for a, b in zip(full, both))
        assert not np.array_equal(full[0][~value], h(flat0)[~value])
        if max_norm == 1e9:
            for a, b in zip(full[:4], only[:4]):
                assert np.array_equal(a[value].view(np.uint32), b[value].view(np.uint32))
        else:
            assert res[np.float64][4] > 2.0 * max_norm, "the critic's own norm clip was meant to be active here"


# --------------------------------------------------------------------------------------------------------------- whole updates
@pytest.mark.parametrize("env_id,num_envs,n_steps", [("SwingRacket-v0", 64, 26), ("Tennisbot-v0", 64, 40)])
def test_three_updates_of_a_trainer(torch, tmp_path, env_id, num_envs, n_steps):
    from tennisbot_rl_amd.stepper import StepperError
    from tennisbot_rl_amd.trpo import FusedTRPO, TRPOTrainer
    t = TRPOTrainer(env_id, num_envs=num_envs, n_steps=n_steps, device=DEV, seed=4)
    assert isinstance(t._learner, FusedTRPO) and t.fused
    assert t._learner.hp is t.hp, "a later change of the trainer's hyper-parameters would not reach the learner"
    n = num_envs * n_steps
    delta = t.hp["kl_delta"]
    theta = h(t._learner.mask) != 0
    seen, ends = [], []
    # a Tennisbot episode ends when the ball passes the racket, or after 1000 steps (tennisbot_env.py:104-207): every env starts
    # at step 0, so rollouts of 40 steps see no episode end until the envs have run apart. 25 rollouts are those 1000 steps.
    warm = 25 if env_id == "Tennisbot-v0" else 0
    for _ in range(warm):
        t.collect()
    for u in range(3):
        last = t.collect()
        adv, ret = t.advantages(last)
        torch.cuda.synchronize()
        ends.append(h(t.buf.dones) != 0)
        before, flat0 = state_dict_arrays(t.policy), h(t.policy._flat_params)
        obs, act, old_logp, a = h(t.obs_seq).reshape(n, -1), h(t._raw_actions).reshape(n, -1), h(t.logps).reshape(n), h(adv).reshape(n)
        stats = t.update(adv, ret)
        after, flat1 = state_dict_arrays(t.policy), h(t.policy._flat_params)
        assert np.isfinite(flat1).all() and all(np.isfinite(v) for v in stats.values()), stats
        assert not np.array_equal(flat1[~theta], flat0[~theta])                                           # the critic learned
        k = stats["accepted_k"]
        seen.append(k)
        # x is an ascent direction of the surrogate (g . x > 0 for every CG iterate of a positive definite F) and the smallest
        # candidate's KL is 1.5^-18 of the first one's: on an on-policy rollout a step is always found
        assert 0 <= k < tr.CANDIDATES, "update %d: no candidate was accepted (%s)" % (u, stats)
        assert not np.array_equal(flat1[theta], flat0[theta])
        kl64, kl32 = tr.kl(before, after, obs), tr.kl(before, after, obs, np.float32)
        an = tr.normalise(a)
        l64, l32 = tr.surrogate(after, obs, act, old_logp, an), tr.surrogate(after, obs, act, old_logp, tr.normalise(a, np.float32), np.float32)
        e_kl, e_l = max(abs(kl32 - kl64), ref.U32 * max(abs(kl64), delta)), max(abs(l32 - l64), ref.U32 * abs(l64))
        print("%s update %d: accepted k = %d, KL %.6g (reported %.6g), L %.6g (reported %.6g); twin errors %.3g / %.3g" % (env_id, u, k, kl64, stats["kl"], l64, stats["surrogate"], e_kl, e_l))
        assert kl64 <= delta + MULTIPLE * e_kl and l64 >= -MULTIPLE * e_l
        assert kl64 > 0.0 and l64 > 0.0, "the step did not raise the surrogate"
        note("reported KL error / twin error", abs(stats["kl"] - kl64) / e_kl)
        note("reported L error / twin error", abs(stats["surrogate"] - l64) / e_l)
        c = t.env.counters()
        assert c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0, c
    at = [np.unique(np.nonzero(d)[0]) for d in ends]
    print("%s: accepted candidates %s; episode ends per rollout %s, at steps %s" % (env_id, seen, [int(d.sum()) for d in ends], [list(s) for s in at]))
    assert all(d.any() for d in ends), "a rollout without an episode end: GAE's resets are not covered"
    if env_id == "Tennisbot-v0":
        assert all(len(s) > 1 for s in at) and not any(d.all(1).any() for d in ends), "the episode ends are not ragged"
    with pytest.raises(StepperError, match="one rank"):
        t._learner.update(t.obs_seq.reshape(n, -1), t._raw_actions.reshape(n, -1), t.logps.reshape(n), adv.reshape(n), ret.reshape(n), 1, n, world=2)
    # a rollout that says nothing (every advantage alike: A_hat = 0, g = 0, CG's 0 / 0) is a rejected update: theta as it was
    adv, ret = t.advantages(t.collect())
    torch.cuda.synchronize()
    flat0 = h(t.policy._flat_params)
    stats = t.update(torch.full_like(adv, 0.25), ret)
    flat1 = h(t.policy._flat_params)
    assert stats["accepted_k"] == -1, stats
    assert np.array_equal(flat1[theta].view(np.uint32), flat0[theta].view(np.uint32)), "a rejected step moved theta"
    assert np.isfinite(flat1).all() and not np.array_equal(flat1[~theta], flat0[~theta])
    path = str(tmp_path / "trpo.pt")
    t.save(path)
    other = TRPOTrainer(env_id, num_envs=num_envs, n_steps=n_steps, device=DEV, seed=77).load(path)
    assert other.num_timesteps == t.num_timesteps == (warm + 4) * n
    assert all(torch.equal(p, q) for p, q in zip(t.policy.parameters(), other.policy.parameters()))
    for p, q in zip(t.policy.parameters(), other.policy.parameters()):
        assert torch.equal(t.opt.state[p]["exp_avg_sq"], other.opt.state[q]["exp_avg_sq"]) and float(t.opt.state[p]["step"]) == float(other.opt.state[q]["step"])
    assert torch.equal(t.env.get_state_words()[0], other.env.get_state_words()[0])
    stats = other.update(*other.advantages(other.collect()))
    assert np.isfinite(list(stats.values())).all()
    for x in (t, other):
        x.env.close()
