"""The TRPO kernels instantiated for TB_NET_MLP64 (tb_trpo_fvp_net, tb_trpo_search_net: SB3's [64, 64] on SwingRacket-v0) and sb3_contrib's
form of the update (TRPOTrainer(form="sb3")) on the device. The kernels against the float64 reference of tests/trpo_reference.py with
the tolerance of tests/ppo_reference.py -- ppo_reference.MULTIPLE float32-twin errors per tensor in the max norm -- at row counts on
both sides of the 16-row tile, a wave's half share, a workgroup's share and, for the search, its 1024-row share, through index vectors
with a repeat and two out-of-range entries. The search runs sb3_contrib's eleven entries, the zero step in front; its fixtures and
their margins are those tests/test_mlp64_reference.py asserts on the CPU. Then whole updates of real trainers on both env ids."""
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
DELTA = fx.SB3["kl_delta"]
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
        print("mlp64 trpo (gpu): largest %s = %.3g" % (k, RATIOS[k]))


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def h(x):
    return x.detach().cpu().numpy().copy()


def make_trpo(torch, ro):
    from tennisbot_rl_amd.params import NET_MLP64
    from tennisbot_rl_amd.trpo import FusedTRPO
    policy = fx.policy().to(DEV)
    opt = torch.optim.Adam(policy.parameters(), lr=fx.SB3["learning_rate"], eps=1e-5)
    hp = dict(ro.hp, **{k: v for k, v in fx.SB3.items() if k not in ("cg_damping", "search_candidates")})
    L = FusedTRPO(ro.kind, policy, opt, hp, torch.device(DEV), form="sb3")
    assert L.net == NET_MLP64 and L.n_params == fx.PARAM_FLOATS and L.table.shape == (11, 2)
    assert L.hp["cg_damping"] == 0.1 and L.hp["search_candidates"] == 10          # left out above: the form's preset fills them in
    return L


def test_fvp_against_the_reference(torch):
    ro = fx.rollout()
    L = make_trpo(torch, ro)
    P = state_dict_arrays(L.policy)
    N = ro.T * ro.n
    obs = ro.obs.reshape(N, -1)
    obs_d = dev(torch, obs)
    vec = np.random.default_rng(8).normal(0.0, 1.0, L.n_params).astype(np.float32)
    vec[np.abs(vec) < 1e-3] = 0.5
    vec_d, v = dev(torch, vec), tr.theta_of(tr.split_flat(vec.astype(np.float64), P))
    d32 = np.float32(fx.SB3["cg_damping"])
    mask = h(L.mask) != 0
    assert mask.sum() == 6 + 64 * 7 + 64 * 65 + 6 * 65
    for m in fx.ROWS:
        idx, rows = fx.index_vector(N, m, 100 + m)
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
        r = note("FVP error / twin error", ref.check_tensors("fvp m = %d" % m, tr.theta_of(tr.split_flat(got, P)), want, twin, MULTIPLE))
        print("m = %3d, FVP %.3g twin errors" % (m, r))


@pytest.mark.parametrize("which", ["kl", "none", "random"])
def test_search_with_the_zero_step_in_front(torch, which):
    from tennisbot_rl_amd.trpo import select_candidate_sb3
    ro = fx.rollout()
    L = make_trpo(torch, ro)
    N = ro.T * ro.n
    picked = set()
    for m in fx.SEARCH_ROWS:
        c = fx.search_case(m, which)
        obs, act, old_logp, adv = c.data
        assert c.margins.min() > fx.MARGIN
        # the kernel gathers through idx from the full-size arrays; only old_logp may differ from the rollout's on these rows
        full = list(flat_shard(ro, ro.gae.adv, ro.gae.returns)[:4])
        full[2] = full[2].copy(); full[2][c.rows] = old_logp
        arrays = tuple(dev(torch, f) for f in full)
        idx_d = dev(torch, c.idx)
        got_t = L.search(arrays, N, idx_d.data_ptr(), m, dev(torch, tr.join_flat(c.x, c.P, np.float32)), dev(torch, c.steps))
        got = h(got_t)
        assert got.shape == (11, 2)
        assert got[0, 1] == 0.0, "the zero step's KL is %r, not exactly 0" % got[0, 1]
        t = lambda a: {"L": a[:, 0], "KL": a[:, 1]}  # noqa: E731
        r = note("search error / twin error", ref.check_tensors("search m = %d %s" % (m, which), t(got), t(c.want), t(c.twin), MULTIPLE))
        l0 = note("L_0 error / twin error", abs(got[0, 0] - c.want[0, 0]) / max(abs(c.twin[0, 0] - c.want[0, 0]), ref.U32 * np.abs(c.want[:, 0]).max()))
        assert l0 <= MULTIPLE
        k_dev = int(select_candidate_sb3(torch, got_t, DELTA))
        assert k_dev == c.k == fx.select_sb3(got), (m, which, k_dev, c.k, got, c.want)
        picked.add(c.k)
        print("m = %4d %-6s accepted %2d, search %.3g twin errors, L_0 %.6g (%.3g twin errors), smallest margin %.3g" % (m, which, c.k, r, got[0, 0], l0, c.margins.min()))
    if which == "none":
        assert picked == {-1}
    if which == "kl":
        assert min(picked) >= 1


# --------------------------------------------------------------------------------------------------------------- whole updates
TRAINERS = [("SwingRacket-v0", "mlp64", 64, 52), ("Tennisbot-v0", "default", 64, 64)]


@pytest.mark.parametrize("env_id,policy,num_envs,n_steps", TRAINERS)
def test_updates_of_an_sb3_form_trainer(torch, tmp_path, env_id, policy, num_envs, n_steps):
    from tennisbot_rl_amd.params import NET_DEFAULT, NET_MLP64
    from tennisbot_rl_amd.trpo import SB3_TRPO_DEFAULTS, FusedTRPO, TRPOTrainer
    kw = dict(num_envs=num_envs, n_steps=n_steps, device=DEV, seed=4, policy=policy, form="sb3", batch_size=1024)
    t = TRPOTrainer(env_id, **kw)
    assert isinstance(t._learner, FusedTRPO) and t.fused and t.form == t._learner.form == "sb3" and t._learner.hp is t.hp
    assert t.net == (NET_MLP64 if policy == "mlp64" else NET_DEFAULT) and t._learner.net == t.net
    assert all(t.hp[k] == v for k, v in SB3_TRPO_DEFAULTS.items()) and t.opt.param_groups[0]["lr"] == 1e-3
    n = num_envs * n_steps
    theta = h(t._learner.mask) != 0
    seen = []
    for u in range(3):
        adv, ret = t.advantages(t.collect())
        torch.cuda.synchronize()
        before, flat0 = state_dict_arrays(t.policy), h(t.policy._flat_params)
        obs, act, old_logp, a = h(t.obs_seq).reshape(n, -1), h(t._raw_actions).reshape(n, -1), h(t.logps).reshape(n), h(adv).reshape(n)
        stats = t.update(adv, ret)
        after, flat1 = state_dict_arrays(t.policy), h(t.policy._flat_params)
        table = h(t._learner.table)
        assert np.isfinite(flat1).all() and all(np.isfinite(v) for v in stats.values()), stats
        assert not np.array_equal(flat1[~theta], flat0[~theta])                                           # the critic learned
        k = stats["accepted_k"]
        seen.append(k)
        if not 0 <= k < 10:
            print("%s update %d rejected; (L, KL) of the zero step and the ten candidates:\n%s" % (env_id, u, table))
        assert 0 <= k < 10, "update %d: no candidate was accepted (%s)" % (u, stats)
        assert table[0, 1] == 0.0 and stats["surrogate"] == table[k + 1, 0] and stats["kl"] == table[k + 1, 1]
        assert not np.array_equal(flat1[theta], flat0[theta])
        an = tr.normalise(a)
        kl64 = tr.kl(before, after, obs)
        l0, l64 = tr.surrogate(before, obs, act, old_logp, an), tr.surrogate(after, obs, act, old_logp, an)
        print("%s update %d: accepted k = %d, KL %.6g (reported %.6g), L %.6g (reported %.6g), L_0 %.6g (the launch's %.6g)" % (env_id, u, k, kl64, stats["kl"], l64, stats["surrogate"],
                                                                                                                    l0, table[0, 0]))
        assert 0.0 < kl64 < DELTA and l64 > l0
        e_l0 = max(abs(tr.surrogate(before, obs, act, old_logp, tr.normalise(a, np.float32), np.float32) - l0), ref.U32 * max(abs(l0), abs(l64)))
        note("trainer L_0 error / twin error", abs(table[0, 0] - l0) / e_l0)
        assert abs(table[0, 0] - l0) <= MULTIPLE * e_l0
        c = t.env.counters()
        assert c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0, c
    print("%s: accepted candidates %s" % (env_id, seen))
    # a rollout that says nothing (every advantage alike: A_hat = 0, g = 0, CG's 0 / 0) is a rejected update: theta as it was
    adv, ret = t.advantages(t.collect())
    torch.cuda.synchronize()
    flat0 = h(t.policy._flat_params)
    stats = t.update(torch.full_like(adv, 0.25), ret)
    flat1 = h(t.policy._flat_params)
    assert stats["accepted_k"] == -1, stats
    assert np.array_equal(flat1[theta].view(np.uint32), flat0[theta].view(np.uint32)), "a rejected step moved theta"
    assert np.isfinite(flat1).all() and not np.array_equal(flat1[~theta], flat0[~theta])                 # ... and the critic still moves
    # a checkpoint, loaded into a second trainer: its next update repeats the original's, bit for bit
    path = str(tmp_path / "trpo_sb3.pt")
    t.save(path)
    assert torch.load(path, weights_only=True)["net"] == policy
    other = TRPOTrainer(env_id, **kw).load(path)
    assert other.num_timesteps == t.num_timesteps == 4 * n
    assert all(torch.equal(p, q) for p, q in zip(t.policy.parameters(), other.policy.parameters()))
    assert torch.equal(t.env.get_state_words()[0], other.env.get_state_words()[0])
    results = []
    for x in (t, other):
        adv, ret = x.advantages(x.collect())
        torch.manual_seed(99)
        stats = x.update(adv, ret)
        torch.cuda.synchronize()
        results.append((stats, x.policy._flat_params.clone(), x._learner.exp_avg_sq.clone()))
    assert results[0][0] == results[1][0], (results[0][0], results[1][0])
    assert torch.equal(results[0][1], results[1][1]) and torch.equal(results[0][2], results[1][2]), "the loaded trainer's update is not the original's"
    if policy == "mlp64":   # the other net's trainer refuses this checkpoint by name
        plain = TRPOTrainer(env_id, num_envs=num_envs, n_steps=n_steps, device=DEV, seed=4)
        with pytest.raises(ValueError, match="'mlp64'.*'default'"):
            plain.load(path)
        plain.env.close()
    for x in (t, other):
        x.env.close()
