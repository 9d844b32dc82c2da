"""tb_trpo_returns and TRPOTrainer(form="agent_returns") on the device.

The kernel: returns bit for bit the float64 reference of tests/trpo_returns_reference.py rounded to float32, the index list equal to
np.flatnonzero of the reference's mask, the count exact, nothing written past idx[count] or past any output's end, the same bits on a
second run -- on shapes at the wave and workgroup edges (one env; 63, 64, 65 envs; 130 envs over 53 steps: 159 table entries, a ragged
last workgroup of the count / scatter kernels; 4097 envs: 65 chunks, 195 entries) and five done patterns, each contiguous and with
record strides larger than n whose padding holds NaN rewards and set done flags.

The trainer: ppo_reference.MULTIPLE = 24 float32-twin errors, the tolerance of the other TRPO tests; nothing new.
Measured on an MI355X (seed 4, 512 envs), the finished share of the three updates: SwingRacket-v0, n_steps 52: 1, 1, 1 (asserted);
Tennisbot-v0, n_steps 128 after three rollouts of warm-up (the first episode of an untrained policy ends after 350 .. 1000 steps):
0.132523, 0.160400, 0.108627 (8685, 10512 and 7119 of 65536 rows), each asserted to lie strictly between 0 and 1; accepted
candidates k = 1, 0, 1 on both envs. Largest ratios seen: g on the finished rows 0.99, the reported KL 1.7 and L 1.5 twin errors.
"""
import numpy as np
import pytest

import ppo_reference as ref
import trpo_reference as tr
import trpo_returns_reference as rr
from policy_reference import state_dict_arrays
from test_ppo_reference import flat_shard, make_policy, rollout

pytestmark = pytest.mark.gpu

MULTIPLE = ref.MULTIPLE
DEV = "cuda:0"
SHAPES = [(1, 1), (2, 63), (27, 64), (27, 65), (53, 130), (3, 4097)]
SENTINEL_F, SENTINEL_I, SENTINEL_B = -7.5, -99, 0x5A
RATIOS = {}


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


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print("trpo returns (gpu): largest %s = %.3g" % (k, RATIOS[k]))


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def h(x):
    return x.detach().cpu().numpy().copy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------- the kernel
def run_returns(torch, lib, rewards, dones, r_stride, d_stride, T, n, discount):
    """one tb_trpo_returns call into sentinel-filled buffers; (returns [T n + 64], idx [T n + 64], count [3], workspace bytes)"""
    N = T * n
    ws_bytes = lib.tb_trpo_returns_workspace_bytes(T, n)
    assert ws_bytes > 0
    ret = torch.full((N + 64,), SENTINEL_F, dtype=torch.float32, device=DEV)
    idx = torch.full((N + 64,), SENTINEL_I, dtype=torch.int64, device=DEV)
    count = torch.full((3,), SENTINEL_I, dtype=torch.int64, device=DEV)
    ws = torch.full((ws_bytes + 64,), SENTINEL_B, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 8 == 0
    rc = lib.tb_trpo_returns(0, 0, torch.cuda.current_stream().cuda_stream, T, n, rewards.data_ptr(), r_stride, dones.data_ptr(), d_stride, discount,
                             ret.data_ptr(), idx.data_ptr(), count.data_ptr() + 8, ws.data_ptr(), ws_bytes)
    assert rc == 0, lib.tb_last_error()
    torch.cuda.synchronize()
    return h(ret), h(idx), h(count), h(ws)[ws_bytes:]


@pytest.mark.parametrize("T,n", SHAPES)
def test_returns_mask_and_index_list(torch, lib, T, n):
    N = T * n
    for p, which in enumerate(rr.PATTERNS):
        rewards, dones = rr.rollout_rewards(T, n, seed=p), rr.patterns(T, n, which, seed=7 + p)
        R, mask, want_idx = rr.returns_reference(rewards, dones)
        want = np.where(mask, R, 0.0).astype(np.float32)
        if which == "none":
            assert len(want_idx) == 0
        if which == "last-step":
            assert len(want_idx) == N
        if which == "step-0":
            assert np.array_equal(want_idx, np.arange(n))
        if which == "one-env-every-step":
            assert np.array_equal(want_idx, np.arange(T) * n + n // 2)
        for layout in ("contiguous", "strided"):
            if layout == "contiguous":
                r_d, d_d, rs, ds = dev(torch, rewards), dev(torch, dones), 0, 0
            else:  # record strides larger than n; what lies between the records must not be read as data
                rw, rs = rr.strided(rewards, 5, np.float32("nan"))
                dw, ds = rr.strided(dones, 3, np.uint8(1))
                r_d, d_d = dev(torch, rw), dev(torch, dw)
                assert rs == 4 * (n + 5) and ds == n + 3
            first = run_returns(torch, lib, r_d, d_d, rs, ds, T, n, rr.DISCOUNT)
            ret, idx, count, tail = first
            what = "(%d, %d) %s %s" % (T, n, which, layout)
            assert count[1] == len(want_idx), what
            assert count[0] == SENTINEL_I and count[2] == SENTINEL_I, what + ": count's neighbours were written"
            assert np.array_equal(bits(ret[:N]), bits(want.reshape(-1))), what + ": returns differ from the float64 reference rounded to float32"
            assert np.array_equal(idx[:len(want_idx)], want_idx), what
            assert (idx[len(want_idx):] == SENTINEL_I).all(), what + ": idx was written past count"
            assert (ret[N:] == SENTINEL_F).all() and (tail == SENTINEL_B).all(), what + ": an output or the workspace was written past its end"
            second = run_returns(torch, lib, r_d, d_d, rs, ds, T, n, rr.DISCOUNT)
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(first, second)), what + ": a second run gave other bits"
    # another discount is another result (the argument is read), and the stride refusals are tb_ppo_gae's
    rewards, dones = rr.rollout_rewards(T, n, seed=3), rr.patterns(T, n, "last-step")
    r_d, d_d = dev(torch, rewards), dev(torch, dones)
    half = run_returns(torch, lib, r_d, d_d, 0, 0, T, n, 0.5)[0][:N]
    R, mask, _ = rr.returns_reference(rewards, dones, 0.5)
    assert np.array_equal(bits(half), bits(R.reshape(-1)))
    if n > 1:
        s = torch.cuda.current_stream().cuda_stream
        scratch = torch.zeros(N + 8, dtype=torch.int64, device=DEV)
        for rs, ds, word in ((4 * n - 4, 0, b"rewards' step stride"), (0, n - 1, b"dones' step stride")):
            rc = lib.tb_trpo_returns(0, 0, s, T, n, r_d.data_ptr(), rs, d_d.data_ptr(), ds, 0.98, scratch.data_ptr(), scratch.data_ptr(), scratch.data_ptr(),
                                     scratch.data_ptr(), 8 * scratch.numel())
            assert rc == -1 and word in lib.tb_last_error()


def test_returns_to_go_takes_the_rollout_buffers_views(torch):
    """FusedTRPO.returns_to_go on strided views (a packed rollout buffer's), bool dones and a transposed array: the same outputs"""
    ro = rollout("tennis-70-ragged")
    L = make_trpo(torch, ro)
    R, mask, want_idx = rr.returns_reference(ro.rewards, ro.dones)
    want = np.where(mask, R, 0.0).astype(np.float32)
    wide_r = torch.full((ro.T, ro.n + 9), float("nan"), device=DEV)
    wide_d = torch.ones((ro.T, ro.n + 9), dtype=torch.uint8, device=DEV)
    wide_r[:, :ro.n], wide_d[:, :ro.n] = dev(torch, ro.rewards), dev(torch, ro.dones)
    inputs = [(dev(torch, ro.rewards), dev(torch, ro.dones)), (wide_r[:, :ro.n], wide_d[:, :ro.n]), (dev(torch, ro.rewards), dev(torch, ro.dones).bool()),
              (dev(torch, ro.rewards.T.copy()).T, dev(torch, ro.dones.T.copy()).T)]
    for r_t, d_t in inputs:
        ret, idx, count = L.returns_to_go(r_t, d_t)
        assert ret.shape == (ro.T, ro.n) and idx.dtype == torch.int64 and idx.numel() == ro.T * ro.n and count.dtype == torch.int64 and count.numel() == 1
        c = int(count.item())
        assert c == len(want_idx) and np.array_equal(h(idx)[:c], want_idx) and np.array_equal(bits(h(ret)), bits(want))
    assert 0 < len(want_idx) < ro.T * ro.n


# ------------------------------------------------------------------------------------------------- the gradient on finished rows
def make_trpo(torch, ro, form="agent_returns", **hp):
    from tennisbot_rl_amd.trpo import FusedTRPO
    policy = make_policy(ro.arch, ro.kind).to(DEV)
    opt = torch.optim.Adam(policy.parameters(), lr=ro.hp["learning_rate"], eps=1e-5)
    return FusedTRPO(ro.kind, policy, opt, dict(ro.hp, **hp), torch.device(DEV), form=form)


@pytest.mark.parametrize("name", ["swing-52-lockstep", "tennis-70-ragged"])
def test_surrogate_gradient_on_the_finished_rows(torch, name):
    """tb_ppo_grad given the raw returns as `adv`, idx[0 .. count) as its rows: g against the reference's, whose A_hat is built in
    float64 from the reference returns (normalised over the finished rows: mean, unbiased std)"""
    ro = rollout(name)
    L = make_trpo(torch, ro)
    assert L.hp["discount"] == rr.DISCOUNT and L.hp["log_std_step"] == "raw" and L.hp["step_rows"] == "all"
    P = state_dict_arrays(L.policy)
    N = ro.T * ro.n
    ret, idx, count = L.returns_to_go(dev(torch, ro.rewards), dev(torch, ro.dones))
    c = int(count.item())
    R, mask, rows = rr.returns_reference(ro.rewards, ro.dones)
    assert c == len(rows) and 1000 < c < N and np.array_equal(h(idx)[:c], rows)
    obs, act, old_logp = (x for x in flat_shard(ro, ret.cpu().numpy(), ret.cpu().numpy())[:3])
    arrays = (dev(torch, obs), dev(torch, act), dev(torch, old_logp), ret.reshape(N), ret.reshape(N))
    g_t = L.surrogate_gradient(arrays, N, idx.data_ptr(), c)
    got = h(g_t)
    theta = h(L.mask) != 0
    assert np.isfinite(got).all() and not got[~theta].any() and got[theta].any()
    adv64 = R.reshape(-1)[rows]
    want = tr.surrogate_gradient(P, obs[rows], act[rows], old_logp[rows], adv64)
    twin = tr.surrogate_gradient(P, obs[rows], act[rows], old_logp[rows], adv64.astype(np.float32), np.float32)
    r = note("g (finished rows) error / twin error", ref.check_tensors(name + " surrogate gradient on finished rows", tr.theta_of(tr.split_flat(got, P)), want, twin, MULTIPLE))
    print("%s: %d of %d rows finished, g %.3g twin errors" % (name, c, N, r))


# --------------------------------------------------------------------------------------------------------------- whole updates
def snapshot(t):
    L = t._learner
    return [h(x) for x in (t.policy._flat_params, L.grad, L.exp_avg, L.exp_avg_sq)]


@pytest.mark.parametrize("env_id,n_steps,warm", [("SwingRacket-v0", 52, 0), ("Tennisbot-v0", 128, 3)])
def test_updates_of_an_agent_returns_trainer(torch, tmp_path, env_id, n_steps, warm):
    import math
    from tennisbot_rl_amd.stepper import StepperError
    from tennisbot_rl_amd.trpo import AGENT_PY_DEFAULTS, FusedTRPO, TRPOTrainer
    num_envs = 512
    kw = dict(num_envs=num_envs, n_steps=n_steps, device=DEV, seed=4, form="agent_returns")
    t = TRPOTrainer(env_id, **kw)
    L = t._learner
    assert isinstance(L, FusedTRPO) and t.fused and t.form == L.form == "agent_returns" and L.hp is t.hp
    assert all(t.hp[k] == v for k, v in AGENT_PY_DEFAULTS.items())
    A = t.env.act_dim
    assert np.array_equal(bits(h(t.policy.log_std)), bits(np.full(A, math.exp(-1))))            # agent.py:39-42
    n = num_envs * n_steps
    delta = t.hp["kl_delta"]
    theta = h(L.mask) != 0
    assert theta[:A].all() and not theta.all()
    # Tennisbot: every env starts at step 0 and no episode of an untrained policy ends in the first 128 steps -- a rollout without a
    # finished row: the update is skipped, theta stays bit for bit, the device's state is as it was
    for w in range(warm):
        last = t.collect()
        if w:
            continue         # (theta has not moved: the later warm-up rollouts only let the envs run apart, as in tests/test_gpu_trpo.py)
        ret, ret2 = t.advantages(last)
        assert ret is ret2
        before = snapshot(t)
        stats = t.update(ret, ret2)
        assert stats["accepted_k"] == -1 and stats["finished_rows"] == 0 and stats["finished_share"] == 0.0, stats
        assert not h(t.buf.dones).any() and not h(ret).any()
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(before, snapshot(t))), "a skipped update wrote something"
    seen, shares = [], []
    for u in range(3):
        ret, _ = t.advantages(t.collect())
        torch.cuda.synchronize()
        rewards, dones = h(t.buf.rewards), h(t.buf.dones)
        R, mask, rows = rr.returns_reference(rewards, dones)
        assert np.array_equal(bits(h(ret)), bits(np.where(mask, R, 0.0)))                      # the trainer's estimator IS the kernel's
        before, snap0 = state_dict_arrays(t.policy), snapshot(t)
        flat0_t = t.policy._flat_params.clone()
        obs, act, old_logp = h(t.obs_seq).reshape(n, -1)[rows], h(t._raw_actions).reshape(n, -1)[rows], h(t.logps).reshape(n)[rows]
        stats = t.update(ret, ret)
        after, snap1 = state_dict_arrays(t.policy), snapshot(t)
        flat0, flat1 = snap0[0], snap1[0]
        assert stats["finished_rows"] == len(rows) and stats["finished_share"] == len(rows) / n, stats
        shares.append(stats["finished_share"])
        if env_id == "SwingRacket-v0":
            assert stats["finished_share"] == 1.0                                                # 52 steps: two whole episodes of every env
        else:
            assert 0.0 < stats["finished_share"] < 1.0, stats
        assert math.isnan(stats["value_loss"]) and all(np.isfinite(v) for k, v in stats.items() if k != "value_loss"), stats
        k = stats["accepted_k"]
        seen.append(k)
        assert 0 <= k < tr.CANDIDATES, "update %d: no candidate was accepted (%s)\n%s" % (u, stats, h(L.table))
        # no critic: the value slots of the parameters, the whole gradient buffer and both moments, bit for bit; no optimiser state
        assert np.array_equal(flat1[~theta].view(np.uint32), flat0[~theta].view(np.uint32))
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(snap0[1:], snap1[1:]))
        assert not any(len(t.opt.state[p]) for p in t.policy.parameters())
        assert not np.array_equal(flat1[theta], flat0[theta]) and np.isfinite(flat1).all()
        # log_std_step="raw": log_std moved by fl(step_k g_logstd), added as policy_step adds the step -- bit for bit
        step = L.steps[k]
        assert torch.equal(t.policy._flat_params[:A], flat0_t[:A] + step * L.gradient[:A]) and h(L.gradient[:A]).any()
        assert torch.equal(L.direction[:A], L.gradient[:A]) and not h(L.direction)[~theta].any()
        assert torch.equal(t.policy._flat_params, flat0_t + step * L.direction)
        # the trust region, re-measured in float64 on the finished rows between the parameters before and after
        adv64 = R.reshape(-1)[rows]
        an = tr.normalise(adv64)
        kl64, kl32 = tr.kl(before, after, obs), tr.kl(before, after, obs, np.float32)
        l64, l32 = tr.surrogate(after, obs, act, old_logp, an), tr.surrogate(after, obs, act, old_logp, tr.normalise(adv64.astype(np.float32), np.float32), np.float32)
        e_kl, e_l = max(abs(kl32 - kl64), ref.U32 * max(abs(kl64), delta)), max(abs(l32 - l64), ref.U32 * abs(l64))
        print("%s update %d: %d of %d rows finished (share %.6f), accepted k = %d, KL %.6g (reported %.6g), L %.6g (reported %.6g); twin errors %.3g / %.3g"
              % (env_id, u, len(rows), n, stats["finished_share"], k, kl64, stats["kl"], l64, stats["surrogate"], e_kl, e_l))
        assert kl64 <= delta + MULTIPLE * e_kl and l64 >= -MULTIPLE * e_l
        assert kl64 > 0.0 and l64 > 0.0, "the step did not raise the surrogate"
        note("reported KL error / twin error", abs(stats["kl"] - kl64) / e_kl)
        note("reported L error / twin error", abs(stats["surrogate"] - l64) / e_l)
        assert abs(stats["kl"] - kl64) <= MULTIPLE * e_kl and abs(stats["surrogate"] - l64) <= MULTIPLE * e_l
        c = t.env.counters()
        assert c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0, c
    print("%s: accepted candidates %s, finished shares %s" % (env_id, seen, shares))
    # the generic update has no meaning here, and update() takes what advantages() gave
    with pytest.raises(StepperError, match="update_finished"):
        L.update(t.obs_seq.reshape(n, -1), t._raw_actions.reshape(n, -1), t.logps.reshape(n), ret.reshape(n), ret.reshape(n), 1, n)
    with pytest.raises(StepperError, match="advantages"):
        t.update(ret, ret.clone())
    # a checkpoint, loaded into a second trainer: its next update repeats the original's, bit for bit
    path = str(tmp_path / "trpo_agent_returns.pt")
    t.save(path)
    other = TRPOTrainer(env_id, **kw).load(path)
    assert other.num_timesteps == t.num_timesteps == (warm + 3) * n and other.hp["log_std_step"] == "raw"
    assert all(torch.equal(p, q) for p, q in zip(t.policy.parameters(), other.policy.parameters()))
    assert torch.equal(t.env.get_state_words()[0], other.env.get_state_words()[0])
    results = []
    for x in (t, other):
        ret, _ = x.advantages(x.collect())
        torch.manual_seed(99)
        stats = x.update(ret, ret)
        torch.cuda.synchronize()
        results.append((stats, x.policy._flat_params.clone(), ret.clone()))
    assert results[0][0]["accepted_k"] >= 0 and str(results[0][0]) == str(results[1][0]), (results[0][0], results[1][0])
    assert torch.equal(results[0][2], results[1][2]) and torch.equal(results[0][1], results[1][1]), "the loaded trainer's update is not the original's"
    for x in (t, other):
        x.env.close()


def test_an_agent_form_trainer_is_not_disturbed(torch):
    """form="agent" before and after a form="agent_returns" trainer lived in the process: the same rollout, the same update, bit for bit"""
    from tennisbot_rl_amd.trpo import TRPOTrainer

    def agent_run():
        t = TRPOTrainer("SwingRacket-v0", num_envs=64, n_steps=26, device=DEV, seed=4)
        assert t.form == "agent" and t.hp["log_std_step"] == "natural" and t.hp["step_rows"] == "cg" and "discount" not in t.hp and not h(t.policy.log_std).any()
        out = []
        for _ in range(2):
            adv, ret = t.advantages(t.collect())
            torch.manual_seed(5)
            stats = t.update(adv, ret)
            out.append((stats, h(t.policy._flat_params), h(t._learner.exp_avg_sq), h(adv)))
        t.env.close()
        return out

    alone = agent_run()
    other = TRPOTrainer("SwingRacket-v0", num_envs=64, n_steps=26, device=DEV, seed=4, form="agent_returns")
    ret, _ = other.advantages(other.collect())
    stats = other.update(ret, ret)
    assert stats["finished_share"] == 1.0
    # the new hyper-parameters from form="agent": raw log_std step and all rows behind beta, with GAE and the critic as they are
    mixed = TRPOTrainer("SwingRacket-v0", num_envs=64, n_steps=26, device=DEV, seed=4, log_std_step="raw", step_rows="all")
    adv, ret = mixed.advantages(mixed.collect())
    torch.manual_seed(5)
    flat0 = mixed.policy._flat_params.clone()
    ms = mixed.update(adv, ret)
    assert ms["accepted_k"] >= 0 and np.isfinite(ms["value_loss"])
    A, Lm = mixed.env.act_dim, mixed._learner
    assert torch.equal(mixed.policy._flat_params[:A], flat0[:A] + Lm.steps[ms["accepted_k"]] * Lm.gradient[:A])
    assert np.array_equal(h(adv), alone[0][3]) and not np.array_equal(h(mixed.policy._flat_params), alone[0][1])
    other.env.close(); mixed.env.close()
    again = agent_run()
    for (s0, f0, v0, a0), (s1, f1, v1, a1) in zip(alone, again):
        assert str(s0) == str(s1), (s0, s1)
        assert np.array_equal(f0.view(np.uint32), f1.view(np.uint32)) and np.array_equal(v0.view(np.uint32), v1.view(np.uint32)) and np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
