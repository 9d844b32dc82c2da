"""The SAC kernels (tb_sac_actor_forward, tb_sac_targets, tb_sac_critic_grad, tb_sac_actor_grad, tb_sac_adam) and a real SACTrainer
on the device, held to the float64 reference of tests/sac_reference.py with the tolerance of tests/ppo_reference.py:
ppo_reference.MULTIPLE float32-twin errors per tensor in the max norm. Both env kinds; the nets, the pool and the kink-free rows
of test_sac_reference.fixture (no row is left out of any comparison). Batches: 1, 2, the 16-row tile's edges, the edges of a
workgroup's rows (tb_sac_rows_per_workgroup() - 1, equal, + 1, 2 x + 1) and 600; the index vector has a repeat and entries
below 0 and above N - 1. The largest ratios are printed at the end of the module."""
import numpy as np
import pytest

import ppo_reference as ref
import sac_reference as sr
from test_sac_reference import KINDS, ROWS, cached_sequence, fixture

pytestmark = pytest.mark.gpu

MULTIPLE = ref.MULTIPLE
DEV = "cuda:0"
RATIOS = {}
ENV_ID = {"swing": "SwingRacket-v0", "tennis": "Tennisbot-v0"}


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
        print("sac (gpu): largest %s = %.3g" % (k, RATIOS[k]))


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def h(x):
    return x.detach().cpu().numpy().copy()


def make_sac(torch, kname, actor=None, critic=None, target=None, log_ent_coef=None):
    """a FusedSAC on the fixture's nets (or the arrays given)"""
    from tennisbot_rl_amd.sac import FusedSAC, build_sac_modules
    f = fixture(kname)
    mods = build_sac_modules(f.O, f.A)
    for m, P in zip(mods, (actor or f.actor, critic or f.critic, target or f.target)):
        m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in P.items()})
        m.to(DEV)
    lec = torch.full((1,), f.log_ent_coef if log_ent_coef is None else log_ent_coef, dtype=torch.float32, device=DEV, requires_grad=True)
    opts = (torch.optim.Adam(mods[0].parameters(), lr=sr.LR, eps=sr.ADAM_EPS), torch.optim.Adam(mods[1].parameters(), lr=sr.LR, eps=sr.ADAM_EPS),
            torch.optim.Adam([lec], lr=sr.LR, eps=sr.ADAM_EPS))
    return FusedSAC(f.kind, mods[0], mods[1], mods[2], lec, opts, {}, torch.device(DEV))


class Data:
    """the fixture's ROWS kink-free rows as replay arrays on the device (every row a clamped index can reach is one of them)"""

    def __init__(self, torch, f):
        keep = f.keep[:ROWS]
        self.N = len(keep)
        self.host = tuple(x[keep] for x in (f.obs, f.next_obs, f.action, f.reward, f.done))
        self.eps_pi, self.eps_next = f.eps_pi[keep], f.eps_next[keep]
        self.arrays = tuple(dev(torch, x) for x in self.host)


def batches(lib):
    R = lib.tb_sac_rows_per_workgroup()
    return sorted({1, 2, 15, 16, 17, R - 1, R, R + 1, 2 * R + 1, 600})


def index_vector(N, m, seed):
    """m rows with a repeat and entries outside [0, N), which the kernels clamp"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N, m).astype(np.int64)
    if m > 2:
        idx[0] = idx[m - 1]
        idx[1], idx[m // 2] = -5, N + 7
    elif m == 2:
        idx[0], idx[1] = -3, N + 2
    return idx, np.clip(idx, 0, N - 1)


def scalars(**kw):
    return {k: np.asarray(v, np.float64) for k, v in kw.items()}


# -------------------------------------------------------------------------------------------------------------- stages (a), (b)
@pytest.mark.parametrize("kname", list(KINDS))
def test_actor_forward_and_targets_against_the_reference(torch, kname):
    f = fixture(kname)
    L, D = make_sac(torch, kname), Data(torch, fixture(kname))
    for m in batches(L.lib):
        idx, rows = index_vector(D.N, m, 100 + m)
        idx_d = dev(torch, idx)
        obs, nobs, act, rew, done = (x[rows] for x in D.host)
        eps_pi, eps_next = D.eps_pi[rows], D.eps_next[rows]
        a_t, lp_t = L.actor_forward(D.arrays[0], idx_d, dev(torch, eps_pi))
        got = {"a": h(a_t), "logp": h(lp_t)}
        want, twin = (sr.actor_forward(f.actor, obs, eps_pi, dt) for dt in (np.float64, np.float32))
        r1 = note("actor forward error / twin error", ref.check_tensors("%s actor forward B = %d" % (kname, m), got, {"a": want.a, "logp": want.logp},
                                                                        {"a": twin.a, "logp": twin.logp}, MULTIPLE))
        y_t = L.targets(D.arrays[1], D.arrays[3], D.arrays[4], idx_d, dev(torch, eps_next))
        y = h(y_t)
        y64, y32 = (sr.targets(f.actor, f.target, f.log_ent_coef, nobs, rew, done, eps_next, sr.GAMMA, dt) for dt in (np.float64, np.float32))
        r2 = note("targets error / twin error", ref.check_tensors("%s targets B = %d" % (kname, m), {"y": y}, {"y": y64}, {"y": y32}, MULTIPLE))
        end = done != 0
        assert np.array_equal(y[end].view(np.uint32), rew[end].view(np.uint32)), "B = %d: a terminal row's target is not its reward, bit for bit" % m
        if m == 600:
            assert end.any() and not end.all()
        print("%s: B = %3d, actor forward %.3g, targets %.3g twin errors" % (kname, m, r1, r2))


# --------------------------------------------------------------------------------------------------------------------- stage (c)
@pytest.mark.parametrize("kname", list(KINDS))
def test_critic_gradient_against_the_reference(torch, kname):
    f = fixture(kname)
    L, D = make_sac(torch, kname), Data(torch, fixture(kname))
    shapes = sr.critic_shapes(f.O, f.A)
    for m in batches(L.lib):
        idx, rows = index_vector(D.N, m, 200 + m)
        obs, nobs, act, rew, done = (x[rows] for x in D.host)
        y = sr.targets(f.actor, f.target, f.log_ent_coef, nobs, rew, done, D.eps_next[rows]).astype(np.float32)
        L.q.grad.fill_(7.0); L.stats.fill_(7.0)
        g_t = L.critic_gradient(D.arrays[0], D.arrays[2], dev(torch, idx), dev(torch, y))
        got = sr.split_flat(h(g_t), shapes)
        (l64, g64), (l32, g32) = (sr.critic_loss_and_grads(f.critic, obs, act, y, dt) for dt in (np.float64, np.float32))
        r = note("critic gradient error / twin error", ref.check_tensors("%s critic gradient B = %d" % (kname, m), got, g64, g32, MULTIPLE))
        rl = note("critic loss error / twin error", ref.check_tensors("%s critic loss B = %d" % (kname, m), scalars(loss=h(L.stats)[0]), scalars(loss=l64), scalars(loss=l32), MULTIPLE))
        print("%s: B = %3d, critic gradient %.3g, loss %.3g twin errors" % (kname, m, r, rl))


# --------------------------------------------------------------------------------------------------------------------- stage (d)
@pytest.mark.parametrize("kname", list(KINDS))
def test_actor_gradient_against_the_reference(torch, kname):
    f = fixture(kname)
    L, D = make_sac(torch, kname), Data(torch, fixture(kname))
    shapes = sr.actor_shapes(f.O, f.A)
    for m in batches(L.lib):
        idx, rows = index_vector(D.N, m, 300 + m)
        obs, eps = D.host[0][rows], D.eps_pi[rows]
        eps_d = dev(torch, eps)
        L.actor_forward(D.arrays[0], dev(torch, idx), eps_d)
        L.q.grad.fill_(7.0); L.pi.grad.fill_(7.0); L.ent.grad.fill_(7.0); L.stats.fill_(7.0)
        L.actor_gradient(m, eps_d)
        assert bool((L.q.grad == 7.0).all()), "the actor's stage wrote into the critic's gradient vector"
        got = sr.split_flat(h(L.pi.grad), shapes)
        a64, a32 = (sr.actor_loss_and_grads(f.actor, f.critic, f.log_ent_coef, obs, eps, dt) for dt in (np.float64, np.float32))
        r = note("actor gradient error / twin error", ref.check_tensors("%s actor gradient B = %d" % (kname, m), got, a64.grads, a32.grads, MULTIPLE))
        st = h(L.stats)
        assert st[0] == 7.0 and float(h(L.ent.grad)[0]) == float(np.float32(st[3]))
        pick = lambda a: scalars(loss=a.loss, mean_logp=a.mean_logp, ent_grad=a.ent_grad)  # noqa: E731
        rs = note("actor loss, mean logp, entropy-coefficient gradient error / twin error",
                  ref.check_tensors("%s actor statistics B = %d" % (kname, m), scalars(loss=st[1], mean_logp=st[2], ent_grad=st[3]), pick(a64), pick(a32), MULTIPLE))
        print("%s: B = %3d, actor gradient %.3g, statistics %.3g twin errors" % (kname, m, r, rs))


# --------------------------------------------------------------------------------------------------------------------- stage (e)
@pytest.mark.parametrize("kname", list(KINDS))
def test_adam_three_steps_and_polyak(torch, kname):
    f = fixture(kname)
    L = make_sac(torch, kname)
    shapes = sr.critic_shapes(f.O, f.A)
    _, s64, _, _, _ = cached_sequence(kname)
    grads = [{k: np.asarray(v, np.float32) for k, v in s.critic_grads.items()} for s in s64]   # the CPU sequence's critic gradients
    n, pad = L.q.n, 64
    z = lambda fill: torch.full((n + pad,), fill, dtype=torch.float32, device=DEV)  # noqa: E731
    p, g, m, v, tgt = z(0.0), z(3.0), z(0.0), z(0.0), z(5.0)
    p0 = sr.join_flat(f.critic, sr.CRITIC_NAMES)
    p[:n].copy_(dev(torch, p0)); p[n:] = 9.0; m[n:] = 9.0; v[n:] = 9.0
    s = torch.cuda.current_stream().cuda_stream
    for k, gk in enumerate(grads):
        g[:n].copy_(dev(torch, sr.join_flat(gk, sr.CRITIC_NAMES)))
        rc = L.lib.tb_sac_adam(0, s, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, sr.LR, 0.9, 0.999, sr.ADAM_EPS, k + 1, tgt.data_ptr(), 0.0)
        assert rc == 0, L.lib.tb_last_error()
    for x, fill in ((p, 9.0), (m, 9.0), (v, 9.0), (tgt, 5.0), (g, 3.0)):
        assert bool((x[n:] == fill).all()), "the kernel wrote beyond the vector's length"
    assert bool((tgt == 5.0).all()), "tau = 0 changed the target"
    res = {}
    for dt in (np.float64, np.float32):
        cur, state = sr.cast(f.critic, dt), sr.adam_init(f.critic, dt)
        for gk in grads:
            cur = sr.adam_step(cur, gk, state, sr.LR, eps=sr.ADAM_EPS, dtype=dt)
        res[dt] = (sr.param_change(cur, f.critic, sr.LR), state["m"], state["v"])
    got = (sr.param_change(sr.split_flat(h(p)[:n].astype(np.float64), shapes), f.critic, sr.LR), sr.split_flat(h(m)[:n], shapes), sr.split_flat(h(v)[:n], shapes))
    for what, a, b, c in zip(("parameter change", "exp_avg", "exp_avg_sq"), got, res[np.float64], res[np.float32]):
        note("Adam %s error / twin error" % what, ref.check_tensors("%s Adam %s" % (kname, what), a, b, c, MULTIPLE))
    # Polyak: folded into the step and alone, within 4 u (|target| + |param|); tau = 0 leaves the target's bits
    rng = np.random.default_rng(9)
    t0 = rng.normal(0.0, 1.0, n).astype(np.float32)
    for tau in (sr.TAU, 0.37):
        t_d = dev(torch, t0)
        L.polyak(p[:n], t_d, tau)
        pn = h(p)[:n].astype(np.float64)
        want = (1.0 - tau) * t0.astype(np.float64) + tau * pn
        assert (np.abs(h(t_d) - want) <= 4.0 * 2.0 ** -24 * (np.abs(t0) + np.abs(pn))).all(), tau
    t_d = dev(torch, t0)
    L.polyak(p[:n], t_d, 0.0)
    assert np.array_equal(h(t_d).view(np.uint32), t0.view(np.uint32))
    # folded: the target follows the NEW parameters of the same launch
    t_d, p_before = dev(torch, t0), p.clone()
    rc = L.lib.tb_sac_adam(0, s, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, sr.LR, 0.9, 0.999, sr.ADAM_EPS, 4, t_d.data_ptr(), sr.TAU)
    assert rc == 0, L.lib.tb_last_error()
    pn = h(p)[:n].astype(np.float64)
    assert not np.array_equal(h(p)[:n], h(p_before)[:n])
    assert (np.abs(h(t_d) - ((1.0 - sr.TAU) * t0.astype(np.float64) + sr.TAU * pn)) <= 4.0 * 2.0 ** -24 * (np.abs(t0) + np.abs(pn))).all()


# ----------------------------------------------------------------------------------------------------------- the combined step
def snapshot(L):
    return [h(x) for x in (L.pi.flat, L.q.flat, L.qt.flat, L.log_ent_coef, L.pi.exp_avg, L.pi.exp_avg_sq, L.q.exp_avg, L.q.exp_avg_sq, L.ent.exp_avg, L.ent.exp_avg_sq,
                           L.pi.grad, L.q.grad, L.ent.grad, L.stats)]


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("kname", list(KINDS))
def test_gradient_step_is_the_stages_and_repeats_its_bits(torch, kname):
    f = fixture(kname)
    D = Data(torch, f)
    idx, rows = index_vector(D.N, 129, 77)
    idx_d, eps_pi, eps_next = dev(torch, idx), dev(torch, D.eps_pi[rows]), dev(torch, D.eps_next[rows])
    runs = []
    for _ in range(2):
        L = make_sac(torch, kname)
        for _ in range(2):
            L.gradient_step(D.arrays, idx_d, eps_pi, eps_next)
        runs.append(snapshot(L))
    assert same_bits(*runs), "two runs from the same state gave other bits"
    L = make_sac(torch, kname)
    # The five stages one by one, in SB3's own order: the critic's Adam WITHOUT a target, the Polyak update alone at the end of the
    # step. gradient_step folds the Polyak update into the critic's Adam launch instead (the target is not read in between), so
    # equal bits here also pin that the folded and the standalone Polyak kernels compute the same thing.
    for k in (1, 2):
        L.actor_forward(D.arrays[0], idx_d, eps_pi)
        y = L.targets(D.arrays[1], D.arrays[3], D.arrays[4], idx_d, eps_next)
        L.critic_gradient(D.arrays[0], D.arrays[2], idx_d, y)
        L.adam(L.q, k)
        L.actor_gradient(129, eps_pi)
        L.adam(L.pi, k)
        L.adam(L.ent, k)
        L.polyak(L.q.flat, L.qt.flat, sr.TAU)
    assert same_bits(runs[0], snapshot(L)), "gradient_step is not the five stages called one by one"
    before = make_sac(torch, kname)
    assert not any(np.array_equal(a, b) for a, b in zip(runs[0][:4], snapshot(before)[:4])), "a parameter set did not move"
    # every row terminal: the next-state stage has no say in the critic's gradient
    done = torch.ones_like(D.arrays[4])
    grads = []
    for nobs in (D.arrays[1], D.arrays[1].flip(0) * 1.5 + 0.25):
        L = make_sac(torch, kname)
        y = L.targets(nobs.contiguous(), D.arrays[3], done, idx_d, eps_next)
        grads.append(h(L.critic_gradient(D.arrays[0], D.arrays[2], idx_d, y)))
    assert np.array_equal(grads[0].view(np.uint32), grads[1].view(np.uint32)) and grads[0].any()


def test_learner_refuses_another_optimiser_and_another_architecture(torch):
    from tennisbot_rl_amd.sac import FusedSAC, build_sac_modules
    from tennisbot_rl_amd.stepper import StepperError

    def parts(O=6, A=6):
        mods = [m.to(DEV) for m in build_sac_modules(O, A)]
        lec = torch.zeros(1, device=DEV, requires_grad=True)
        return mods, lec

    def adam(ps, **kw):
        return torch.optim.Adam(ps, lr=sr.LR, eps=sr.ADAM_EPS, **kw)

    def build(mods, lec, opts, kind=0):
        return FusedSAC(kind, mods[0], mods[1], mods[2], lec, opts, {}, torch.device(DEV))

    mods, lec = parts()
    good = lambda: (adam(mods[0].parameters()), adam(mods[1].parameters()), adam([lec]))  # noqa: E731
    assert build(mods, lec, good()).step == 0
    for k, bad in ((0, lambda ps: adam(ps, amsgrad=True)), (1, lambda ps: adam(ps, weight_decay=1e-4)), (2, lambda ps: adam(ps, maximize=True)),
                   (0, lambda ps: torch.optim.AdamW(ps, lr=sr.LR)), (1, lambda ps: torch.optim.SGD(ps, lr=sr.LR)),
                   (0, lambda ps: adam(list(ps)[::-1]))):
        opts = list(good())
        opts[k] = bad(list(mods[k].parameters()) if k < 2 else [lec])
        with pytest.raises(StepperError, match="Adam"):
            build(mods, lec, opts)
    with pytest.raises(StepperError, match="MlpPolicy"):          # Tennisbot's nets under SwingRacket's kind
        other, lec2 = parts(12, 2)
        build(other, lec2, (adam(other[0].parameters()), adam(other[1].parameters()), adam([lec2])), kind=0)
    with pytest.raises(StepperError, match="MlpPolicy"):          # an actor of another shape
        narrow = torch.nn.Sequential(torch.nn.Linear(6, 64), torch.nn.Linear(64, 6)).to(DEV)
        build([narrow, mods[1], mods[2]], lec, (adam(narrow.parameters()), adam(mods[1].parameters()), adam([lec])))
    with pytest.raises(StepperError, match="log_ent_coef"):
        wide = torch.zeros(2, device=DEV, requires_grad=True)
        build(mods, wide, (adam(mods[0].parameters()), adam(mods[1].parameters()), adam([wide])))
    # a stage at another batch size between actor_forward and actor_gradient overwrites what was kept: refused, and said so
    L, D = make_sac(torch, "swing"), Data(torch, fixture("swing"))
    idx = dev(torch, np.arange(16, dtype=np.int64))
    eps = dev(torch, D.eps_pi[:16])
    L.actor_forward(D.arrays[0], idx, eps)
    L.targets(D.arrays[1], D.arrays[3], D.arrays[4], idx[:8].contiguous(), dev(torch, D.eps_next[:8]))
    with pytest.raises(ValueError, match="no actor_forward"):
        L.actor_gradient(16, eps)


# --------------------------------------------------------------------------------------------------------------- a real trainer
@pytest.mark.parametrize("kname", list(KINDS))
def test_trainer_thirty_vector_steps_save_and_load(torch, tmp_path, kname):
    from tennisbot_rl_amd.sac import FusedSAC, SACTrainer
    env_id, n = ENV_ID[kname], 64
    t = SACTrainer(env_id, num_envs=n, batch_size=64, gradient_steps=4, learning_starts=64, seed=3, device=DEV, buffer_size=4096)
    assert isinstance(t._learner, FusedSAC) and t._learner.hp is t.hp
    target0, critic0 = h(t._learner.qt.flat), h(t._learner.q.flat)
    assert np.array_equal(target0, critic0)
    A = t.env.act_dim
    ends = []
    for k in range(30):
        prev = t.obs.clone()
        if k == 0:
            torch.manual_seed(123)
        a, obs, r, d = t.vector_step()
        if k == 0:
            torch.manual_seed(123)
            assert torch.equal(a, torch.rand((n, A), device=DEV) * 2.0 - 1.0), "the first step's actions are not the uniform draw"
        assert bool((a.abs() < 1.0).all())
        sl = slice(k * n, (k + 1) * n)
        R = t.replay
        assert torch.equal(R.obs[sl], prev) and torch.equal(R.next_obs[sl], obs) and torch.equal(R.action[sl], a)
        assert torch.equal(R.reward[sl], r) and torch.equal(R.done[sl], d.float())
        ends.append(h(d) != 0)
        assert t._learner.step == 4 * max(0, k)
    torch.cuda.synchronize()
    assert t.num_timesteps == 30 * n and t.replay.size == 30 * n and t.replay.pos == 30 * n
    if kname == "swing":
        assert ends[25].all() and not np.any(ends[:25]), "SwingRacket's episodes end at step 26"
        assert bool((t.replay.reward[25 * n:26 * n] != 0).any()), "the terminal reward is missing from the replay rows"
    L = t._learner
    flats = [h(x) for x in (L.pi.flat, L.q.flat, L.qt.flat)]
    assert all(np.isfinite(x).all() for x in flats) and np.isfinite(h(L.stats)).all()
    assert float(h(t.log_ent_coef)[0]) != 0.0, "ent_coef has not moved"
    assert not np.array_equal(flats[2], flats[1]) and not np.array_equal(flats[2], target0) and not np.array_equal(flats[1], critic0)
    c = t.env.counters()
    assert c["nonfinite_states"] == 0, c
    for p in t.actor.parameters():
        assert float(t.opts[0].state[p]["step"]) == L.step
    path = str(tmp_path / "sac.pt")
    t.save(path)
    other = SACTrainer(env_id, num_envs=n, batch_size=64, gradient_steps=4, learning_starts=64, seed=91, device=DEV, buffer_size=4096).load(path)
    assert other.num_timesteps == t.num_timesteps and other.replay.pos == t.replay.pos and other.replay.size == t.replay.size and other._learner.step == L.step
    assert all(torch.equal(x, y) for x, y in zip(t.replay.arrays(), other.replay.arrays()))
    assert torch.equal(t.env.get_state_words()[0], other.env.get_state_words()[0]) and torch.equal(t.obs, other.obs)
    idx = t.replay.sample(64)
    eps = torch.randn((2, 64, A), device=DEV)
    for x in (t, other):
        x._learner.gradient_step(x.replay.arrays(), idx, eps[0], eps[1])
    assert same_bits(snapshot(t._learner), snapshot(other._learner)), "the loaded trainer's next gradient step gave other bits"
    assert np.isfinite(t.evaluate(n_steps=26))
    for x in (t, other):
        x.env.close()
