"""A population of SAC / TQC learners on the device (tb_sac_*_members / tb_tqc_*_members; tennisbot_rl_amd/sac_population.py), held
BIT FOR BIT to the single-member stages, which tests/test_gpu_sac.py and tests/test_gpu_tqc.py hold to the float64 reference:

  stage bits    one members gradient step at M = 3 against FusedSAC / FusedTQC on copies of member m's rows and scalars. B = 1 (a
                one-row tile), 16 / 17 (a tile edge), 65 (a second workgroup of rows; the weight gradient's tail past two 32-row
                chunks), 257 (the row kernels' second block; the loss kernels' strided loop). Distinct parameters, moments,
                log_ent_coef and hyper-parameter rows (one member with tau = 0), step = 2, index rows with a repeat and two
                out-of-range entries that clamp onto terminal rows, every strided per-member array NaN-padded by 4 floats.
  trainer bits  PopulationSAC.train(3) against three FusedSAC.gradient_steps per member on its index and noise rows
  loop          30 vector steps: the ring's rows are what BatchedEnv.step returned, member by member; episode counts; a save /
                load round trip repeats the next train(1)'s bits; an exported member loads into SACTrainer and evaluates
  learn         learn() with pbt_every on SwingRacket-v0 across three episode ends: the exploit acts on scores that hold episodes,
                and waits where a member has none
  guard         actor_gradient refuses a batch other than the last actor_forward's, as FusedSAC's does
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = {"swing": 0, "tennis": 1}
ENV_ID = {"swing": "SwingRacket-v0", "tennis": "Tennisbot-v0"}
DIMS = {0: (6, 6), 1: (12, 2)}
N_ROWS, M, PAD = 300, 3, 4
HP = [[1.0e-4, 2.0e-4, 3.0e-4, 0.99, 0.005], [2.5e-4, 1.5e-4, 0.5e-4, 0.95, 0.0], [3.0e-4, 4.0e-4, 6.0e-4, 0.90, 0.02]]   # member 1: tau = 0
LOG_ENT_COEF = [-0.7, 0.2, -1.3]
IDX_PAD = 1 << 60


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def bits(x):
    x = x.detach().cpu().contiguous()
    return x.numpy().view({4: np.uint32, 8: np.uint64}[x.element_size()])


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def replay_rows(torch, kind):
    """seeded finite replay rows in test_sac_reference.fixture's recipe; rows 0 and N_ROWS - 1 (where out-of-range indices clamp to) terminal"""
    O, A = DIMS[kind]
    rng = np.random.default_rng(70 + kind)
    done = (rng.random(N_ROWS) < 0.2).astype(np.float32)
    done[0] = done[-1] = 1.0
    host = (rng.normal(0.0, 3.0, (N_ROWS, O)).astype(np.float32), rng.normal(0.0, 3.0, (N_ROWS, O)).astype(np.float32), rng.uniform(-1.0, 1.0, (N_ROWS, A)).astype(np.float32),
            rng.normal(0.0, 1.0, N_ROWS).astype(np.float32), done)
    return tuple(torch.from_numpy(x).to(DEV) for x in host), done


def index_rows(B, seed):
    """[M, B] with, per member, a repeat and two out-of-range entries (B = 1: one out-of-range entry, or a terminal row): every member
    reads a terminal row, because the out-of-range entries clamp to rows 0 and N_ROWS - 1"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N_ROWS, (M, B)).astype(np.int64)
    if B > 2:
        idx[:, 0] = idx[:, B - 1]
        idx[:, 1], idx[:, B // 2] = -5, N_ROWS + 7
    else:
        idx[:, 0] = [-5, N_ROWS + 7, N_ROWS - 1][:M]
    return idx


def padded(torch, x, pad_value=math.nan):
    """x [M, ...] as a view of storage whose rows lie PAD elements further apart, the padding set to pad_value; (view, storage)"""
    n = x[0].numel()
    big = torch.full((x.shape[0], n + PAD), pad_value, dtype=x.dtype, device=DEV)
    big[:, :n] = x.reshape(x.shape[0], n).to(DEV)
    view = big[:, :n] if x.dim() == 2 else big[:, :n].unflatten(1, tuple(x.shape[1:]))
    return view, big


def padding_intact(torch, big, n, pad_value=math.nan):
    tail = big[:, n:]
    return bool(torch.isnan(tail).all()) if isinstance(pad_value, float) else bool((tail == pad_value).all())


def single_learner(torch, algo, kind, ck, hp_row):
    """FusedSAC / FusedTQC on modules and optimisers loaded from a member's checkpoint dict, with that member's gamma and tau"""
    from tennisbot_rl_amd import sac_population as sp
    from tennisbot_rl_amd.sac import FusedSAC
    from tennisbot_rl_amd.tqc import FusedTQC
    O, A = DIMS[kind]
    actor, critic, target = (m.to(DEV) for m in sp._algo(algo)[2](O, A))
    lec = torch.zeros(1, dtype=torch.float32, device=DEV, requires_grad=True)
    opts = tuple(torch.optim.Adam(p, lr=lr, eps=1e-8) for p, lr in ((actor.parameters(), hp_row[0]), (critic.parameters(), hp_row[1]), ([lec], hp_row[2])))
    actor.load_state_dict(ck["actor"]); critic.load_state_dict(ck["critic"]); target.load_state_dict(ck["critic_target"])
    for o, sd in zip(opts, ck["optimizers"]):
        o.load_state_dict(sd)
    with torch.no_grad():
        lec.copy_(ck["log_ent_coef"].to(DEV))
    return (FusedSAC if algo == "sac" else FusedTQC)(kind, actor, critic, target, lec, opts, dict(gamma=hp_row[3], tau=hp_row[4]), torch.device(DEV))


def member_ck(sp, L, algo, kind, m):
    O, A = DIMS[kind]
    return sp.member_checkpoint(algo, O, A, L.pi.flat[m], L.q.flat[m], L.qt.flat[m], L.ent.flat[m],
                                ((L.pi.exp_avg[m], L.pi.exp_avg_sq[m]), (L.q.exp_avg[m], L.q.exp_avg_sq[m]), (L.ent.exp_avg[m], L.ent.exp_avg_sq[m])),
                                L.hp[m].tolist(), L.step, adam_eps=L.adam_eps)


def member_state(L, m):
    """what a gradient step leaves of member m: parameters, moments, target, log_ent_coef with its moments"""
    return dict(pi=L.pi.flat[m], pi_m=L.pi.exp_avg[m], pi_v=L.pi.exp_avg_sq[m], q=L.q.flat[m], q_m=L.q.exp_avg[m], q_v=L.q.exp_avg_sq[m], qt=L.qt.flat[m],
                ent=L.ent.flat[m].reshape(1), ent_m=L.ent.exp_avg[m].reshape(1), ent_v=L.ent.exp_avg_sq[m].reshape(1))


def single_state(S):
    return dict(pi=S.pi.flat, pi_m=S.pi.exp_avg, pi_v=S.pi.exp_avg_sq, q=S.q.flat, q_m=S.q.exp_avg, q_v=S.q.exp_avg_sq, qt=S.qt.flat,
                ent=S.log_ent_coef.detach().reshape(1), ent_m=S.ent.exp_avg.reshape(1), ent_v=S.ent.exp_avg_sq.reshape(1))


# ------------------------------------------------------------------------------------------------------------------- stage bits
@pytest.mark.parametrize("B", [1, 16, 17, 65, 257])
@pytest.mark.parametrize("kname", list(KINDS))
@pytest.mark.parametrize("algo", ["sac", "tqc"])
def test_a_members_step_leaves_every_members_single_step_bit_for_bit(torch, algo, kname, B):
    from tennisbot_rl_amd import sac_population as sp
    kind = KINDS[kname]
    O, A = DIMS[kind]
    arrays, done = replay_rows(torch, kind)
    L = (sp.FusedSACMembers if algo == "sac" else sp.FusedTQCMembers)(kind, M, DEV, seed=300 + kind, hp_rows=[r + [0.0] * 3 for r in HP])
    g = torch.Generator().manual_seed(1000 + 10 * B + kind)
    stores = {}
    with torch.no_grad():   # distinct parameters come from the seeds; non-zero moments, distinct log_ent_coef, everything strided NaN-padded
        for rows, name in ((L.pi, "pi"), (L.q, "q"), (L.qt, "qt")):
            for attr in ("flat", "grad", "exp_avg", "exp_avg_sq"):
                if name == "qt" and attr != "flat":
                    assert getattr(rows, attr) is None   # the target follows by the Polyak update: parameters alone
                    continue
                x = getattr(rows, attr).cpu()
                if attr == "flat" and name == "qt":
                    x = x + 0.01 * torch.randn(x.shape, generator=g)       # (a target that is not the critic)
                elif attr == "exp_avg":
                    x = 0.01 * torch.randn(x.shape, generator=g)
                elif attr == "exp_avg_sq":
                    x = 1e-4 * torch.rand(x.shape, generator=g)
                elif attr == "grad":
                    x = torch.full(x.shape, math.nan)                         # (every entry must be written)
                view, big = padded(torch, x)
                setattr(rows, attr, view)
                stores[name + "." + attr] = (big, x.shape[1])
        L.ent.flat.copy_(torch.tensor(LOG_ENT_COEF).view(M, 1))
        L.ent.exp_avg.copy_(0.01 * torch.randn((M, 1), generator=g))
        L.ent.exp_avg_sq.copy_(1e-4 * torch.rand((M, 1), generator=g))
    L.step = 1   # the step under test is step 2
    idx_host = index_rows(B, 17 * B + kind)
    idx, idx_big = padded(torch, torch.from_numpy(idx_host), IDX_PAD)
    eps_pi, eps_pi_big = padded(torch, torch.randn((M, B, A), generator=g).clamp(-2.5, 2.5))
    eps_next, eps_next_big = padded(torch, torch.randn((M, B, A), generator=g).clamp(-2.5, 2.5))
    L.workspace(B)
    y_shape = (M, B) + L.Y_SHAPE
    (L.act_pi, act_big), (L.logp_pi, logp_big), (L.y, y_big) = (padded(torch, torch.full(s, math.nan)) for s in ((M, B, A), (M, B), y_shape))
    for m in range(M):
        assert done[np.clip(idx_host[m], 0, N_ROWS - 1)].sum() >= 1, "every member's batch holds a terminal row"
    cks = [member_ck(sp, L, algo, kind, m) for m in range(M)]   # the members' rows BEFORE the step

    L.gradient_step(arrays, idx, eps_pi, eps_next)
    torch.cuda.synchronize()
    assert L.step == 2

    for m in range(M):
        S = single_learner(torch, algo, kind, cks[m], HP[m])
        assert S.step == 1
        S.gradient_step(arrays, idx[m].contiguous(), eps_pi[m].contiguous(), eps_next[m].contiguous())
        torch.cuda.synchronize()
        want = dict(single_state(S), act=S.act_pi, logp=S.logp_pi, y=S.y, q_grad=S.q.grad, pi_grad=S.pi.grad, ent_grad=S.ent.grad.reshape(1), stats=S.stats)
        got = dict(member_state(L, m), act=L.act_pi[m], logp=L.logp_pi[m], y=L.y[m], q_grad=L.q.grad[m], pi_grad=L.pi.grad[m], ent_grad=L.ent.grad[m].reshape(1), stats=L.stats[m])
        for k in want:
            assert same(got[k], want[k]), "%s %s B = %d member %d: %s differs from the single-member stage" % (algo, kname, B, m, k)
        assert bool(torch.isfinite(want["stats"]).all()) and bool(torch.isfinite(want["pi_grad"]).all()) and bool(torch.isfinite(want["q_grad"]).all())
        terminal = torch.from_numpy(done[np.clip(idx_host[m], 0, N_ROWS - 1)] != 0).to(DEV)
        r = arrays[3][torch.from_numpy(np.clip(idx_host[m], 0, N_ROWS - 1)).to(DEV)]
        ym = L.y[m].reshape(B, -1)
        assert same(ym[terminal], r[terminal].unsqueeze(1).expand(-1, ym.shape[1])), "a terminal row's target is its reward"
        if HP[m][4] == 0.0:
            assert same(L.qt.flat[m], torch.cat([v.reshape(-1) for v in cks[m]["critic_target"].values()])), "tau = 0 leaves the target as it was"
    # the case could see a wrong member
    assert not same(L.act_pi[0], L.act_pi[1]) and not same(L.q.grad[0], L.q.grad[1]) and not same(L.pi.flat[0], L.pi.flat[1])
    # nothing between two rows was written
    for name, (big, n) in stores.items():
        assert padding_intact(torch, big, n), name
    for name, big, n in (("eps_pi", eps_pi_big, B * A), ("eps_next", eps_next_big, B * A), ("act", act_big, B * A), ("logp", logp_big, B), ("y", y_big, int(np.prod(y_shape[1:])))):
        assert padding_intact(torch, big, n), name
    assert padding_intact(torch, idx_big, B, IDX_PAD) and np.array_equal(idx.cpu().numpy(), idx_host)


def test_actor_gradient_refuses_a_batch_other_than_the_last_actor_forwards(torch):
    """the workspace's regions scale with the batch, so a stage at another batch size overwrites what actor_forward kept: refused on
    the host, before any launch, as FusedSAC.actor_gradient refuses it"""
    from tennisbot_rl_amd import sac_population as sp
    arrays, _ = replay_rows(torch, 0)
    L = sp.FusedSACMembers(0, M, DEV, seed=2)
    g = torch.Generator().manual_seed(3)
    eps = {B: torch.randn((M, B, 6), generator=g).to(DEV) for B in (16, 17)}
    idx = {B: torch.from_numpy(np.random.default_rng(B).integers(0, N_ROWS, (M, B)).astype(np.int64)).to(DEV) for B in (16, 17)}
    with pytest.raises(ValueError, match="no actor_forward"):
        L.actor_gradient(16, eps[16])
    L.actor_forward(arrays[0], idx[16], eps[16])
    with pytest.raises(ValueError, match="an actor_forward of 16 rows"):
        L.actor_gradient(17, eps[17])
    L.targets(arrays[1], arrays[3], arrays[4], idx[17], eps[17])   # a stage at another batch size in between
    with pytest.raises(ValueError, match="no actor_forward"):
        L.actor_gradient(16, eps[16])
    L.actor_forward(arrays[0], idx[16], eps[16])
    L.actor_gradient(16, eps[16])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(L.pi.grad).all())


def test_the_members_polyak_update_alone_is_each_members_single_update(torch):
    """tb_sac_adam_members without gradient and moments: target <- (1 - tau_m) target + tau_m params per member, the bits of tb_sac_adam's
    Polyak-only call with that member's tau (257 floats: a second block), on NaN-padded rows"""
    from tennisbot_rl_amd import sac_population as sp
    L = sp.FusedSACMembers(0, M, DEV, seed=1, hp_rows=[r + [0.0] * 3 for r in HP])
    g, n = torch.Generator().manual_seed(8), 257
    (params, params_big), (target, target_big) = padded(torch, torch.randn((M, n), generator=g)), padded(torch, torch.randn((M, n), generator=g))
    before = target.clone()
    L.polyak(params, target)
    torch.cuda.synchronize()
    for m in range(M):
        p, t = params[m].clone(), before[m].clone()   # (copies: the single call updates t in place)
        rc = L.lib.tb_sac_adam(0, None, p.data_ptr(), None, None, None, n, 0.0, 0.0, 0.0, 0.0, 1, t.data_ptr(), HP[m][4])
        assert rc == 0, L.lib.tb_last_error()
        torch.cuda.synchronize()
        assert same(target[m], t), m
        assert same(target[m], before[m]) == (HP[m][4] == 0.0)
    assert padding_intact(torch, params_big, n) and padding_intact(torch, target_big, n)


# ----------------------------------------------------------------------------------------------------------------- trainer bits
@pytest.mark.parametrize("algo,kname", [("sac", "swing"), ("sac", "tennis"), ("tqc", "swing")])
def test_population_train_is_three_single_gradient_steps_per_member(torch, algo, kname):
    from tennisbot_rl_amd import sac_population as sp
    kind = KINDS[kname]
    pop = sp.PopulationSAC(ENV_ID[kname], members=3, envs_per_member=16, algo=algo, batch_size=17, buffer_size=4096, seed=5, device=DEV,
                           member_hp=dict(lr_actor=[r[0] for r in HP], lr_critic=[r[1] for r in HP], lr_ent=[r[2] for r in HP], gamma=[r[3] for r in HP], tau=[r[4] for r in HP]))
    try:
        for _ in range(4):
            pop.collect()
        assert pop.filled_slots == 4 and pop.member_timesteps == 64
        L = pop._learner
        cks = [member_ck(sp, L, algo, kind, m) for m in range(3)]
        state = pop.gen.get_state()
        idx, eps = pop.draw_batches(3)
        pop.gen.set_state(state)
        before = torch.get_rng_state()
        assert pop.train(3) == 3 and L.step == 3
        assert torch.equal(torch.get_rng_state(), before), "torch's global RNG was drawn from"
        torch.cuda.synchronize()
        arrays = pop.replay.arrays()
        for m in range(3):
            assert int(idx[:, m].min()) >= 0 and bool(((idx[:, m] % 48) // 16 == m).all()) and int(idx[:, m].max()) < 4 * 48
            S = single_learner(torch, algo, kind, cks[m], L.hp[m].tolist())
            for k in range(3):
                S.gradient_step(arrays, idx[k, m], eps[k, 0, m], eps[k, 1, m])
            torch.cuda.synchronize()
            got, want = member_state(L, m), single_state(S)
            for name in want:
                assert same(got[name], want[name]), "%s %s member %d: %s differs after three steps" % (algo, kname, m, name)
        assert not same(L.pi.flat[0], L.pi.flat[1])
    finally:
        pop.close()


# ------------------------------------------------------------------------------------------------------------------------- loop
@pytest.mark.parametrize("kname", list(KINDS))
def test_the_loop_fills_the_ring_counts_episodes_and_round_trips(torch, kname, tmp_path):
    from tennisbot_rl_amd import sac_population as sp
    from tennisbot_rl_amd.sac import SACTrainer
    Mm, R, SLOTS = 2, 16, 20
    N = Mm * R
    kw = dict(members=Mm, envs_per_member=R, batch_size=16, gradient_steps=2, buffer_size=SLOTS * N + 5, learning_starts=48, seed=3, device=DEV, member_hp=dict(lr=[3e-4, 1e-4]))
    pop = sp.PopulationSAC(ENV_ID[kname], **kw)
    other = loaded = None
    try:
        assert pop.replay.capacity == SLOTS * N   # rounded down to whole vector steps
        steps, episodes = [], torch.zeros(Mm, dtype=torch.float64)
        for t in range(30):
            obs_in = pop.obs.clone()
            a, obs, r, d = pop.vector_step()
            steps.append((obs_in, obs.clone(), a.clone(), r.clone(), d.float()))
            episodes += d.view(Mm, R).sum(1).double().cpu()
            if kname == "swing":
                assert bool(d.all()) == (t % 26 == 25), "SwingRacket-v0 episodes are 26 steps"
        assert pop.member_timesteps == 30 * R and pop._learner.step == 2 * (30 - 3)   # trains once a member's timesteps exceed learning_starts = 48
        torch.cuda.synchronize()
        for t in range(30 - SLOTS, 30):   # what the wrapped ring still holds
            slot = t % SLOTS
            for m in range(Mm):
                lo, hi = slot * N + m * R, slot * N + (m + 1) * R
                for ring, step in zip(pop.replay.arrays(), steps[t]):
                    assert same(ring[lo:hi], step[m * R:(m + 1) * R]), (kname, t, m)
        if kname == "swing":   # the 26th step's reward carries the terminal reward of the fast-forwarded flight, complete when it is stored
            r26 = steps[25][3]
            assert same(pop.replay.reward[(25 % SLOTS) * N:(25 % SLOTS) * N + N], r26) and bool(torch.isfinite(r26).all()) and float(r26.abs().max()) > 0.0
            assert bool((steps[25][4] == 1.0).all())
        assert torch.equal(pop._ep_stats[:, 0].cpu(), episodes), "per-member episode counts"
        assert bool(torch.isfinite(pop._learner.stats).all())

        path = str(tmp_path / "population.pt")
        pop.save(path)
        member_path = str(tmp_path / "member1.pt")
        pop.export_member(1, member_path)
        at_save = member_ck(sp, pop._learner, "sac", KINDS[kname], 1)
        pop.train(1)
        torch.cuda.synchronize()
        want = [{k: v.clone() for k, v in member_state(pop._learner, m).items()} for m in range(Mm)]
        other = sp.PopulationSAC(ENV_ID[kname], **dict(kw, seed=99)).load(path)
        assert other.num_timesteps == 30 * N and other.replay.pos == pop.replay.pos and same(other.obs, steps[-1][1])
        other.train(1)
        torch.cuda.synchronize()
        for m in range(Mm):
            for k, v in member_state(other._learner, m).items():
                assert same(v, want[m][k]), "after save / load, train(1) differs in member %d's %s" % (m, k)

        loaded = SACTrainer(ENV_ID[kname], num_envs=R, buffer_size=SLOTS * R, seed=1, device=DEV).load(member_path)
        assert loaded.num_timesteps == 30 * R and loaded.replay.size == SLOTS * R and loaded._learner.step == 2 * 27
        for flat, key in ((loaded._learner.pi.flat, "actor"), (loaded._learner.q.flat, "critic"), (loaded._learner.qt.flat, "critic_target")):
            assert same(flat, torch.cat([v.reshape(-1) for v in at_save[key].values()])), key   # member 1 as it was at the save
        assert same(loaded.log_ent_coef.detach(), at_save["log_ent_coef"]) and not same(loaded._learner.pi.flat, want[1]["pi"])
        assert same(loaded.replay.obs[:R], pop.replay.obs[R:2 * R]) and same(loaded.obs, steps[-1][1][R:2 * R])
        score = loaded.evaluate(n_steps=5)
        assert math.isfinite(score)
    finally:
        for x in (pop, other):
            if x is not None:
                x.close()
        if loaded is not None:
            loaded.env.close()


# -------------------------------------------------------------------------------------------------- learn(): what PBT acts on
def test_learn_exploits_on_scores_that_hold_episodes_and_waits_for_them(torch):
    """learn() with pbt_every = 10 on SwingRacket-v0, whose envs all end together every 26 steps: most windows of 10 vector steps
    hold no finished episode. At steps 10 and 20 nobody has a score and the exploit is skipped (no row changes); at
    step 30 everybody has one (the episodes that ended at step 26) and the worst member becomes a bit-for-bit copy of the best, its
    learning rates perturbed, its score cleared; at steps 40 and 50 the copy has finished no episode of its own, so the exploit
    waits; at step 60 (episodes ended at 52) it runs again. A score is not tied to the progress lines: a line at step 30 clears
    nothing that step 60 needs."""
    from tennisbot_rl_amd import sac_population as sp
    Mm, R = 4, 8
    pop = sp.PopulationSAC("SwingRacket-v0", members=Mm, envs_per_member=R, batch_size=16, gradient_steps=1, buffer_size=64 * Mm * R, learning_starts=8, seed=5, device=DEV,
                           member_hp=dict(lr=[3e-4, 1e-4, 6e-4, 2e-4], tau=[0.005, 0.01, 0.02, 0.0]), pbt_every=10, pbt_frac=0.25)
    try:
        L = pop._learner
        hp0, lines = L.hp.clone(), []
        history = pop.learn(20 * R, log=lines.append)
        assert [h["timesteps"] for h in history] == [10 * R, 20 * R] and len(lines) == 2
        for h in history:
            assert h["pbt"] == [] and all(math.isnan(s) for s in h["scores"]) and sum(h["episodes"]) == 0
        assert same(L.hp, hp0) and bool(torch.isnan(pop.scores()).all()) and "skipped" in lines[0]

        history = pop.learn(30 * R, log=None)
        assert len(history) == 1
        rec = history[0]
        sc = rec["scores"]
        assert all(math.isfinite(s) for s in sc) and rec["episodes"] == [float(R)] * Mm, "the episodes that ended at step 26"
        assert len(set(sc)) == Mm, "four untrained actors with four different returns"
        worst, best = sc.index(min(sc)), sc.index(max(sc))
        assert rec["pbt"] == [(worst, best)]
        torch.cuda.synchronize()
        for x in L.vectors():
            assert same(x[worst], x[best])
        ratio = (L.hp[worst, 0:3].double() / L.hp[best, 0:3].double()).tolist()
        assert all(0.8 < r < 1.25 for r in ratio) and max(ratio) - min(ratio) < 1e-6 and same(L.hp[worst, 3:], L.hp[best, 3:])
        for m in range(Mm):
            if m != worst:
                assert same(L.hp[m], hp0[m])
        now = pop.scores().tolist()
        assert math.isnan(now[worst]) and all(now[m] == sc[m] for m in range(Mm) if m != worst), "the line at step 30 cleared nobody's score but the copy's"

        hp30 = L.hp.clone()
        history = pop.learn(50 * R, log=None)
        assert [(h["timesteps"], h["pbt"]) for h in history] == [(40 * R, []), (50 * R, [])] and same(L.hp, hp30)
        assert all(math.isnan(h["scores"][worst]) and sum(math.isfinite(s) for s in h["scores"]) == Mm - 1 for h in history)

        history = pop.learn(60 * R, log=None)
        rec = history[-1]
        assert all(math.isfinite(s) for s in rec["scores"]) and len(rec["pbt"]) == 1, "episodes ended at step 52: everybody has a score again"
        lo, hi = rec["pbt"][0]
        assert rec["scores"][lo] == min(rec["scores"]) and rec["scores"][hi] == max(rec["scores"]) and lo != hi
        assert pop._vector_steps == 60 and bool(torch.isfinite(L.stats).all())
    finally:
        pop.close()
