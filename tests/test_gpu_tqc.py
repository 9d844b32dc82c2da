"""The TQC kernels (tb_tqc_actor_forward, tb_tqc_targets, tb_tqc_critic_grad, tb_tqc_actor_grad, with tb_sac_adam) and a real
TQCTrainer on the device, held to the float64 reference of tests/tqc_reference.py with the tolerance of tests/ppo_reference.py:
ppo_reference.MULTIPLE float32-twin errors per tensor set in the max norm. Both env kinds; the nets, the pool and the kink-free
rows of test_tqc_reference.fixture (no row is left out of any comparison). Batches: 1, 2, the edges of the 16-row tile (15, 16,
17) and of a workgroup's 64 rows (63, 64, 65), 129 and 600; the index vector has a repeat and entries below 0 and above N - 1.
The head's M = 25 is a partial second column tile and a reduction tail of one at every one of them. The largest ratios are
printed at the end of the module."""
import numpy as np
import pytest

import ppo_reference as ref
import tqc_reference as tr
from test_tqc_reference import KINDS, ROWS, cached_sequence, fixture

pytestmark = pytest.mark.gpu

MULTIPLE = ref.MULTIPLE
DEV = "cuda:0"
RATIOS = {}
ENV_ID = {"swing": "SwingRacket-v0", "tennis": "Tennisbot-v0"}
BATCHES = (1, 2, 15, 16, 17, 63, 64, 65, 129, 600)
GUARD, SENTINEL = 64, -12345.0


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
        print("tqc (gpu): largest %s = %.3g" % (k, RATIOS[k]))


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def h(x):
    return x.detach().cpu().numpy().copy()


def make_tqc(torch, kname, actor=None, critic=None, target=None, log_ent_coef=None):
    """a FusedTQC on the fixture's nets (or the arrays given)"""
    from tennisbot_rl_amd.tqc import FusedTQC, build_tqc_modules
    f = fixture(kname)
    mods = build_tqc_modules(f.O, f.A)
    for m, P in zip(mods, (actor or f.actor, critic or f.critic, target or f.target)):
        m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in P.items()})
        m.to(DEV)
    lec = torch.full((1,), f.log_ent_coef if log_ent_coef is None else log_ent_coef, dtype=torch.float32, device=DEV, requires_grad=True)
    opts = (torch.optim.Adam(mods[0].parameters(), lr=tr.LR, eps=tr.ADAM_EPS), torch.optim.Adam(mods[1].parameters(), lr=tr.LR, eps=tr.ADAM_EPS),
            torch.optim.Adam([lec], lr=tr.LR, eps=tr.ADAM_EPS))
    return FusedTQC(f.kind, mods[0], mods[1], mods[2], lec, opts, {}, torch.device(DEV))


class Data:
    """the fixture's ROWS kink-free rows as replay arrays on the device (every row a clamped index can reach is one of them)"""

    def __init__(self, torch, f):
        keep = f.keep[:ROWS]
        self.N = len(keep)
        self.host = tuple(x[keep] for x in (f.obs, f.next_obs, f.action, f.reward, f.done))
        self.eps_pi, self.eps_next = f.eps_pi[keep], f.eps_next[keep]
        self.arrays = tuple(dev(torch, x) for x in self.host)


def index_vector(N, m, seed):
    """m rows with a repeat and two entries outside [0, N), which the kernels clamp"""
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


def guarded(torch, *shape):
    """(the whole buffer, its first prod(shape) floats as a view of that shape): GUARD sentinel floats follow the view"""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[:n].view(*shape)


def guard_workspace(torch, L, B):
    """the learner's workspace for B rows replaced by one of exactly the queried size with GUARD doubles behind it"""
    L.workspace(B)
    need = L.lib.tb_tqc_workspace_bytes(L.kind, B)
    assert need % 8 == 0
    whole = torch.zeros(need // 8 + GUARD, dtype=torch.float64, device=DEV)
    whole[need // 8:] = SENTINEL
    L._ws = whole[:need // 8]
    return whole, need // 8


# -------------------------------------------------------------------------------------------------------------- stages (a), (b)
@pytest.mark.parametrize("kname", list(KINDS))
def test_actor_forward_and_targets_against_the_reference(torch, kname):
    f = fixture(kname)
    L, D = make_tqc(torch, kname), Data(torch, fixture(kname))
    for m in BATCHES:
        idx, rows = index_vector(D.N, m, 100 + m)
        idx_d = dev(torch, idx)
        obs, nobs, act, rew, done = (x[rows] for x in D.host)
        eps_pi, eps_next = D.eps_pi[rows], D.eps_next[rows]
        whole, n_ws = guard_workspace(torch, L, m)
        a_t, lp_t = L.actor_forward(D.arrays[0], idx_d, dev(torch, eps_pi))
        got = {"a": h(a_t), "logp": h(lp_t)}
        want, twin = (tr.actor_forward(f.actor, obs, eps_pi, dt) for dt in (np.float64, np.float32))
        r1 = note("actor forward error / twin error", ref.check_tensors("%s actor forward B = %d" % (kname, m), got, {"a": want.a, "logp": want.logp},
                                                                        {"a": twin.a, "logp": twin.logp}, MULTIPLE))
        ybuf, yv = guarded(torch, m, 46)
        L.targets(D.arrays[1], D.arrays[3], D.arrays[4], idx_d, dev(torch, eps_next), y=yv)
        y = h(yv)
        assert bool((ybuf[m * 46:] == SENTINEL).all()), "B = %d: the target kernel wrote beyond y" % m
        assert not (y == SENTINEL).any(), "B = %d: a slot of y was not written" % m
        assert bool((whole[n_ws:] == SENTINEL).all()), "B = %d: a kernel wrote beyond the workspace" % m
        y64, y32 = (tr.targets(f.actor, f.target, f.log_ent_coef, nobs, rew, done, eps_next, tr.GAMMA, dt) for dt in (np.float64, np.float32))
        r2 = note("targets error / twin error", ref.check_tensors("%s targets B = %d" % (kname, m), {"y": y}, {"y": y64}, {"y": y32}, MULTIPLE))
        end = done != 0
        assert np.array_equal(y[end].view(np.uint32), np.repeat(rew[end][:, None], 46, 1).view(np.uint32)), "B = %d: a terminal row's targets are not its reward, bit for bit" % m
        assert (np.diff(y[~end], axis=1) >= 0).all(), "B = %d: a row of y is not sorted" % m
        if m == 600:
            assert end.any() and not end.all()
        print("%s: B = %3d, actor forward %.3g, targets %.3g twin errors" % (kname, m, r1, r2))


def _targets_case(torch, kname, target, m=65):
    f = fixture(kname)
    L, D = make_tqc(torch, kname, target=target), Data(torch, f)
    idx, rows = index_vector(D.N, m, 150)
    _, nobs, _, rew, done = (x[rows] for x in D.host)
    ybuf, yv = guarded(torch, m, 46)
    L.targets(D.arrays[1], D.arrays[3], D.arrays[4], dev(torch, idx), dev(torch, D.eps_next[rows]), y=yv)
    y64, y32 = (tr.targets(f.actor, target, f.log_ent_coef, nobs, rew, done, D.eps_next[rows], tr.GAMMA, dt) for dt in (np.float64, np.float32))
    assert bool((ybuf[m * 46:] == SENTINEL).all())
    return h(yv), y64, y32, done != 0


@pytest.mark.parametrize("kname", list(KINDS))
def test_targets_with_every_quantile_twice(torch, kname):
    """the target's qf1 a bitwise copy of qf0: every value occurs twice, and every one of the 46 slots is still written once"""
    f = fixture(kname)
    twice = {k: (f.target["qf0." + k[4:]].copy() if k.startswith("qf1.") else v) for k, v in f.target.items()}
    y, y64, y32, end = _targets_case(torch, kname, twice)
    assert not (y == SENTINEL).any(), "a slot kept the sentinel: two equal quantiles took the same rank"
    assert np.array_equal(y[~end][:, 0:46:2], y[~end][:, 1:46:2]) and (np.diff(y[~end], axis=1) >= 0).all()
    note("targets (ties) error / twin error", ref.check_tensors("%s targets with ties" % kname, {"y": y}, {"y": y64}, {"y": y32}, MULTIPLE))


@pytest.mark.parametrize("kname", list(KINDS))
def test_targets_with_a_nan_quantile(torch, kname):
    """one target head bias NaN: one of the 50 quantiles is NaN in every row, sorts last as in np.sort, and is dropped"""
    f = fixture(kname)
    bad = dict(f.target)
    bad["qf0.4.bias"] = f.target["qf0.4.bias"].copy()
    bad["qf0.4.bias"][7] = np.nan
    y, y64, y32, end = _targets_case(torch, kname, bad)
    assert np.isfinite(y64).all() and np.isfinite(y).all() and not (y == SENTINEL).any()
    note("targets (NaN) error / twin error", ref.check_tensors("%s targets with a NaN" % kname, {"y": y}, {"y": y64}, {"y": y32}, MULTIPLE))


# --------------------------------------------------------------------------------------------------------------------- stage (c)
def head_region(L, B, name):
    """the [2][B][32] head region `name` of the workspace as a host array"""
    from_floats = h(L._ws).view(np.float32)
    at = {"Q": 3280, "DQ": 3344}[name]   # TqcWs::Q, TqcWs::DQ in csrc/tb_tqc.hpp: floats per row before the region
    return from_floats[at * B:(at + 64) * B].reshape(2, B, 32)


@pytest.mark.parametrize("kname", list(KINDS))
def test_critic_gradient_against_the_reference(torch, kname):
    f = fixture(kname)
    L, D = make_tqc(torch, kname), Data(torch, fixture(kname))
    shapes = tr.critic_shapes(f.O, f.A)
    heads = [k for k in tr.CRITIC_NAMES if ".4." in k]
    for m in BATCHES:
        idx, rows = index_vector(D.N, m, 200 + m)
        obs, nobs, act, rew, done = (x[rows] for x in D.host)
        y = tr.targets(f.actor, f.target, f.log_ent_coef, nobs, rew, done, D.eps_next[rows]).astype(np.float32)
        whole, n_ws = guard_workspace(torch, L, m)
        L._ws.view(torch.float32).fill_(3.0)             # stale content, the padding columns included
        gbuf = torch.full((L.q.n + GUARD,), 7.0, dtype=torch.float32, device=DEV)
        L.q.grad = gbuf[:L.q.n]
        L.stats.fill_(7.0)
        g_t = L.critic_gradient(D.arrays[0], D.arrays[2], dev(torch, idx), dev(torch, y))
        assert bool((gbuf[L.q.n:] == 7.0).all()), "B = %d: a kernel wrote beyond the gradient vector" % m
        assert bool((whole[n_ws:] == SENTINEL).all()), "B = %d: a kernel wrote beyond the workspace" % m
        dq = head_region(L, m, "DQ")
        assert (dq[:, :, 25:] == 0.0).all() and (dq[:, :, :25] != 3.0).all(), "B = %d: the gradient region's padding columns are not zero" % m
        got = tr.split_flat(h(g_t), shapes)
        (l64, g64), (l32, g32) = (tr.critic_loss_and_grads(f.critic, obs, act, y, dt) for dt in (np.float64, np.float32))
        r = note("critic gradient error / twin error", ref.check_tensors("%s critic gradient B = %d" % (kname, m), got, g64, g32, MULTIPLE))
        pick = lambda g: {k: g[k] for k in heads}  # noqa: E731
        rh = note("critic head (qf*.4) gradient error / twin error", ref.check_tensors("%s critic head gradient B = %d" % (kname, m), pick(got), pick(g64), pick(g32), MULTIPLE))
        assert all(got[k].shape == ((25, 256) if k.endswith("weight") else (25,)) and got[k][24].any() for k in heads)   # the last quantile's row: the second column tile
        rl = note("critic loss error / twin error", ref.check_tensors("%s critic loss B = %d" % (kname, m), scalars(loss=h(L.stats)[0]), scalars(loss=l64), scalars(loss=l32), MULTIPLE))
        assert (h(L.stats)[1:] == 7.0).all()
        print("%s: B = %3d, critic gradient %.3g (head %.3g), loss %.3g twin errors" % (kname, m, r, rh, rl))


# --------------------------------------------------------------------------------------------------------------------- stage (d)
@pytest.mark.parametrize("kname", list(KINDS))
def test_actor_gradient_against_the_reference(torch, kname):
    f = fixture(kname)
    L, D = make_tqc(torch, kname), Data(torch, fixture(kname))
    shapes = tr.actor_shapes(f.O, f.A)
    for m in BATCHES:
        idx, rows = index_vector(D.N, m, 300 + m)
        obs, eps = D.host[0][rows], D.eps_pi[rows]
        eps_d = dev(torch, eps)
        whole, n_ws = guard_workspace(torch, L, m)
        L._ws.view(torch.float32).fill_(3.0)
        L.actor_forward(D.arrays[0], dev(torch, idx), eps_d)
        gbuf = torch.full((L.pi.n + GUARD,), 7.0, dtype=torch.float32, device=DEV)
        L.pi.grad = gbuf[:L.pi.n]
        L.q.grad.fill_(7.0); L.ent.grad.fill_(7.0); L.stats.fill_(7.0)
        L.actor_gradient(m, eps_d)
        assert bool((L.q.grad == 7.0).all()), "the actor's stage wrote into the critic's gradient vector"
        assert bool((gbuf[L.pi.n:] == 7.0).all()), "B = %d: a kernel wrote beyond the gradient vector" % m
        assert bool((whole[n_ws:] == SENTINEL).all()), "B = %d: a kernel wrote beyond the workspace" % m
        dq = head_region(L, m, "DQ")
        assert (dq[:, :, 25:] == 0.0).all() and (dq[:, :, :25] == np.float32(-1.0) / (np.float32(50.0) * np.float32(m))).all()
        got = tr.split_flat(h(L.pi.grad), shapes)
        a64, a32 = (tr.actor_loss_and_grads(f.actor, f.critic, f.log_ent_coef, obs, eps, dt) for dt in (np.float64, np.float32))
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
    """tb_sac_adam on a vector of the TQC critic's length, with the CPU sequence's critic gradients"""
    f = fixture(kname)
    L = make_tqc(torch, kname)
    shapes = tr.critic_shapes(f.O, f.A)
    _, s64, _, _, _ = cached_sequence(kname)
    grads = [{k: np.asarray(v, np.float32) for k, v in s.critic_grads.items()} for s in s64]
    n, pad = L.q.n, GUARD
    assert n == (151090, 152114)[f.kind]
    z = lambda fill: torch.full((n + pad,), fill, dtype=torch.float32, device=DEV)  # noqa: E731
    p, g, m, v, tgt = z(0.0), z(3.0), z(0.0), z(0.0), z(5.0)
    p0 = tr.join_flat(f.critic, tr.CRITIC_NAMES)
    p[:n].copy_(dev(torch, p0)); p[n:] = 9.0; m[n:] = 9.0; v[n:] = 9.0
    s = torch.cuda.current_stream().cuda_stream
    for k, gk in enumerate(grads):
        g[:n].copy_(dev(torch, tr.join_flat(gk, tr.CRITIC_NAMES)))
        rc = L.lib.tb_sac_adam(0, s, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, tr.LR, 0.9, 0.999, tr.ADAM_EPS, k + 1, tgt.data_ptr(), 0.0)
        assert rc == 0, L.lib.tb_last_error()
    for x, fill in ((p, 9.0), (m, 9.0), (v, 9.0), (tgt, 5.0), (g, 3.0)):
        assert bool((x[n:] == fill).all()), "the kernel wrote beyond the vector's length"
    assert bool((tgt == 5.0).all()), "tau = 0 changed the target"
    res = {}
    for dt in (np.float64, np.float32):
        cur, state = tr.cast(f.critic, dt), tr.adam_init(f.critic, dt)
        for gk in grads:
            cur = tr.adam_step(cur, gk, state, tr.LR, eps=tr.ADAM_EPS, dtype=dt)
        res[dt] = (tr.param_change(cur, f.critic, tr.LR), state["m"], state["v"])
    got = (tr.param_change(tr.split_flat(h(p)[:n].astype(np.float64), shapes), f.critic, tr.LR), tr.split_flat(h(m)[:n], shapes), tr.split_flat(h(v)[:n], shapes))
    for what, a, b, c in zip(("parameter change", "exp_avg", "exp_avg_sq"), got, res[np.float64], res[np.float32]):
        note("Adam %s error / twin error" % what, ref.check_tensors("%s Adam %s" % (kname, what), a, b, c, MULTIPLE))
    # Polyak alone, within 4 u (|target| + |param|); tau = 0 leaves the target's bits
    rng = np.random.default_rng(9)
    t0 = rng.normal(0.0, 1.0, n).astype(np.float32)
    t_d = dev(torch, t0)
    L.polyak(p[:n], t_d, tr.TAU)
    pn = h(p)[:n].astype(np.float64)
    assert (np.abs(h(t_d) - ((1.0 - tr.TAU) * t0.astype(np.float64) + tr.TAU * pn)) <= 4.0 * 2.0 ** -24 * (np.abs(t0) + np.abs(pn))).all()
    t_d = dev(torch, t0)
    L.polyak(p[:n], t_d, 0.0)
    assert np.array_equal(h(t_d).view(np.uint32), t0.view(np.uint32))


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
        L = make_tqc(torch, kname)
        for _ in range(2):
            L.gradient_step(D.arrays, idx_d, eps_pi, eps_next)
        runs.append(snapshot(L))
    assert same_bits(*runs), "two runs from the same state gave other bits"
    L = make_tqc(torch, kname)
    # the stages one by one: the critic's Adam WITHOUT a target, the Polyak update alone at the end of the step (gradient_step folds
    # it into the critic's Adam launch)
    for k in (1, 2):
        L.actor_forward(D.arrays[0], idx_d, eps_pi)
        y = L.targets(D.arrays[1], D.arrays[3], D.arrays[4], idx_d, eps_next)
        L.critic_gradient(D.arrays[0], D.arrays[2], idx_d, y)
        L.adam(L.q, k)
        L.actor_gradient(129, eps_pi)
        L.adam(L.pi, k)
        L.adam(L.ent, k)
        L.polyak(L.q.flat, L.qt.flat, tr.TAU)
    assert same_bits(runs[0], snapshot(L)), "gradient_step is not the stages called one by one"
    before = make_tqc(torch, kname)
    assert not any(np.array_equal(a, b) for a, b in zip(runs[0][:4], snapshot(before)[:4])), "a parameter set did not move"
    # tau = 0 leaves the target's bits
    L = make_tqc(torch, kname)
    L.hp["tau"] = 0.0
    L.gradient_step(D.arrays, idx_d, eps_pi, eps_next)
    assert np.array_equal(h(L.qt.flat).view(np.uint32), snapshot(before)[2].view(np.uint32)) and not np.array_equal(h(L.q.flat), snapshot(before)[1])
    # every row terminal: the next-state stage has no say in the critic's gradient
    done = torch.ones_like(D.arrays[4])
    grads = []
    for nobs in (D.arrays[1], D.arrays[1].flip(0) * 1.5 + 0.25):
        L = make_tqc(torch, kname)
        y = L.targets(nobs.contiguous(), D.arrays[3], done, idx_d, eps_next)
        grads.append(h(L.critic_gradient(D.arrays[0], D.arrays[2], idx_d, y)))
    assert np.array_equal(grads[0].view(np.uint32), grads[1].view(np.uint32)) and grads[0].any()


def test_learner_refuses_another_optimiser_and_another_architecture(torch):
    from tennisbot_rl_amd.stepper import StepperError
    from tennisbot_rl_amd.tqc import FusedTQC, build_tqc_modules

    def parts(O=6, A=6, **kw):
        mods = [m.to(DEV) for m in build_tqc_modules(O, A, **kw)]
        lec = torch.zeros(1, device=DEV, requires_grad=True)
        return mods, lec

    def adam(ps, **kw):
        return torch.optim.Adam(ps, lr=tr.LR, eps=tr.ADAM_EPS, **kw)

    def build(mods, lec, opts, kind=0, **kw):
        return FusedTQC(kind, mods[0], mods[1], mods[2], lec, opts, {}, torch.device(DEV), **kw)

    mods, lec = parts()
    good = lambda: (adam(mods[0].parameters()), adam(mods[1].parameters()), adam([lec]))  # noqa: E731
    assert build(mods, lec, good()).step == 0
    for k, bad in ((0, lambda ps: adam(ps, amsgrad=True)), (1, lambda ps: adam(ps, weight_decay=1e-4)), (2, lambda ps: adam(ps, maximize=True)),
                   (0, lambda ps: torch.optim.AdamW(ps, lr=tr.LR)), (1, lambda ps: torch.optim.SGD(ps, lr=tr.LR)),
                   (0, lambda ps: adam(list(ps)[::-1]))):
        opts = list(good())
        opts[k] = bad(list(mods[k].parameters()) if k < 2 else [lec])
        with pytest.raises(StepperError, match="Adam"):
            build(mods, lec, opts)
    for kw in (dict(n_quantiles=24), dict(n_critics=3), dict(top_quantiles_to_drop_per_net=3)):      # said by the caller ...
        with pytest.raises(StepperError, match="the kernels take 25 quantiles, 2 critics and 2 dropped per net"):
            build(mods, lec, good(), **kw)
    for kw in (dict(n_quantiles=24), dict(n_critics=3)):                                              # ... or only built
        other, lec2 = parts(**kw)
        with pytest.raises(StepperError, match="2 critics of 25 quantiles"):
            build(other, lec2, (adam(other[0].parameters()), adam(other[1].parameters()), adam([lec2])))
    with pytest.raises(StepperError, match="MlpPolicy"):          # Tennisbot's nets under SwingRacket's kind
        other, lec2 = parts(12, 2)
        build(other, lec2, (adam(other[0].parameters()), adam(other[1].parameters()), adam([lec2])), kind=0)
    with pytest.raises(StepperError, match="MlpPolicy"):          # SAC's critic: one output per net
        from tennisbot_rl_amd.sac import build_sac_modules
        sac = [m.to(DEV) for m in build_sac_modules(6, 6)]
        build(sac, lec, (adam(sac[0].parameters()), adam(sac[1].parameters()), adam([lec])))
    with pytest.raises(StepperError, match="log_ent_coef"):
        wide = torch.zeros(2, device=DEV, requires_grad=True)
        build(mods, wide, (adam(mods[0].parameters()), adam(mods[1].parameters()), adam([wide])))
    # a stage at another batch size between actor_forward and actor_gradient overwrites what was kept: refused, and said so
    L, D = make_tqc(torch, "swing"), Data(torch, fixture("swing"))
    idx = dev(torch, np.arange(16, dtype=np.int64))
    eps = dev(torch, D.eps_pi[:16])
    L.actor_forward(D.arrays[0], idx, eps)
    L.targets(D.arrays[1], D.arrays[3], D.arrays[4], idx[:8].contiguous(), dev(torch, D.eps_next[:8]))
    with pytest.raises(ValueError, match="no actor_forward"):
        L.actor_gradient(16, eps)


# --------------------------------------------------------------------------------------------------------------- a real trainer
@pytest.mark.parametrize("kname", list(KINDS))
def test_trainer_thirty_vector_steps_save_and_load(torch, tmp_path, kname):
    from tennisbot_rl_amd.tqc import FusedTQC, TQCTrainer
    env_id, n = ENV_ID[kname], 64
    assert TQCTrainer.__init__.__defaults__[:2] == ("SwingRacket-v0", 256)
    t = TQCTrainer(env_id, num_envs=n, batch_size=64, gradient_steps=4, learning_starts=64, seed=3, device=DEV, buffer_size=4096)
    assert isinstance(t._learner, FusedTQC) and t._learner.hp is t.hp
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
    path = str(tmp_path / "tqc.pt")
    t.save(path)
    other = TQCTrainer(env_id, num_envs=n, batch_size=64, gradient_steps=4, learning_starts=64, seed=91, device=DEV, buffer_size=4096).load(path)
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
