"""What tests/test_gpu_sac_edges.py and tests/test_gpu_tqc_edges.py share: the stages of a learner on the device at the edge fixtures
of tests/edge_fixtures.py, held to the float64 reference with ppo_reference.MULTIPLE float32-twin errors per tensor, exactly as
tests/test_gpu_sac.py and tests/test_gpu_tqc.py hold them at the comfortable fixtures. A `Learner` says what differs."""
import numpy as np

import edge_fixtures as ef
import ppo_reference as ref

MULTIPLE = ref.MULTIPLE
DEV = "cuda:0"
GUARD, SENTINEL = 64, -12345.0


class Learner:
    """name; mod: the reference module; fixture(which, kname); make(torch, kname, actor=...): the sibling's make_sac / make_tqc;
    workspace_bytes: the C ABI's query by name; y_shape(B); index_vector, snapshot, same_bits: the sibling's"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.ratios, self.notes = {}, []

    def note(self, name, r):
        self.ratios[name] = max(self.ratios.get(name, 0.0), r)
        return r

    def report(self):
        for k in sorted(self.ratios):
            print("%s edges (gpu): largest %s = %.3g" % (self.name, k, self.ratios[k]))
        for line in self.notes:
            print("%s edges (gpu): %s" % (self.name, line))


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def h(x):
    return x.detach().cpu().numpy().copy()


def scalars(**kw):
    return {k: np.asarray(v, np.float64) for k, v in kw.items()}


class Data:
    """the fixture's first N_ROWS ordered rows as replay arrays on the device (every row a clamped index can reach is one of them)"""

    def __init__(self, torch, f):
        rows = f.rows[:ef.N_ROWS]
        self.N = len(rows)
        assert self.N == ef.N_ROWS
        self.host = tuple(x[rows] for x in (f.obs, f.next_obs, f.action, f.reward, f.done))
        self.eps_pi, self.eps_next = f.eps_pi[rows], f.eps_next[rows]
        self.arrays = tuple(dev(torch, x) for x in self.host)


def batch(G, D, what, m):
    """the sibling's index vector (a repeat, an entry below 0 and one above N - 1) and the rows it selects; edge_fixtures
    restates that function for the CPU modules: it must be the same"""
    idx, rows = G.index_vector(D.N, m, ef.SEEDS[what] + m)
    idx2, rows2 = ef.index_vector(D.N, m, ef.SEEDS[what] + m)
    assert np.array_equal(idx, idx2) and np.array_equal(rows, rows2)
    assert 0 in rows and D.N - 1 in rows and idx.min() < 0 and idx.max() >= D.N
    return idx, rows


def guarded(torch, *shape, fill=SENTINEL):
    """(the whole buffer, its first prod(shape) floats as a view of that shape): GUARD floats of `fill` follow the view"""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), fill, dtype=torch.float32, device=DEV)
    return buf, buf[:n].view(*shape)


def guard_workspace(torch, G, L, B):
    """the learner's workspace for B rows replaced by one of exactly the queried size, stale 3.0 in every float, with GUARD
    sentinel doubles behind it"""
    L.workspace(B)
    need = getattr(L.lib, G.workspace_bytes)(L.kind, B)
    assert need > 0 and need % 8 == 0
    whole = torch.zeros(need // 8 + GUARD, dtype=torch.float64, device=DEV)
    whole[need // 8:] = SENTINEL
    L._ws = whole[:need // 8]
    L._ws.view(torch.float32).fill_(3.0)
    return whole, need // 8


def actor_forward_and_targets(torch, G, which, kname):
    f = G.fixture(which, kname)
    L, D = G.make(torch, kname, actor=f.actor), Data(torch, f)
    tag = "%s %s" % (which, kname)
    for m in ef.SIZES:
        idx, rows = batch(G, D, "forward", m)
        idx_d = dev(torch, idx)
        obs, nobs, act, rew, done = (x[rows] for x in D.host)
        eps_pi, eps_next = D.eps_pi[rows], D.eps_next[rows]
        whole, n_ws = guard_workspace(torch, G, L, m)
        abuf, av = guarded(torch, m, f.A)
        lbuf, lv = guarded(torch, m)
        L.actor_forward(D.arrays[0], idx_d, dev(torch, eps_pi), act_out=av, logp_out=lv)
        got = {"a": h(av), "logp": h(lv)}
        assert bool((abuf[m * f.A:] == SENTINEL).all()) and bool((lbuf[m:] == SENTINEL).all()), "B = %d: the sample kernel wrote beyond its outputs" % m
        assert np.isfinite(got["a"]).all() and np.isfinite(got["logp"]).all(), "%s B = %d: a non-finite action or logp" % (tag, m)
        assert (np.abs(got["a"]) <= 1.0).all(), "%s B = %d: an action outside [-1, 1]" % (tag, m)
        want, twin = (G.mod.actor_forward(f.actor, obs, eps_pi, dt) for dt in (np.float64, np.float32))
        r1 = G.note("%s: actor forward error / twin error" % which, ref.check_tensors("%s actor forward B = %d" % (tag, m), got, {"a": want.a, "logp": want.logp},
                                                                                     {"a": twin.a, "logp": twin.logp}, MULTIPLE))
        if which == "deep":
            G.notes.append("%s B = %d: |a| exactly 1 in every saturated column: %s" % (tag, m, bool((np.abs(got["a"][:, 1::2]) == 1.0).all())))
        shape = G.y_shape(m)
        ybuf, yv = guarded(torch, *shape)
        L.targets(D.arrays[1], D.arrays[3], D.arrays[4], idx_d, dev(torch, eps_next), y=yv)
        y = h(yv)
        assert bool((ybuf[int(np.prod(shape)):] == SENTINEL).all()), "B = %d: the target kernel wrote beyond y" % m
        assert not (y == SENTINEL).any(), "B = %d: a slot of y was not written" % m
        assert bool((whole[n_ws:] == SENTINEL).all()), "B = %d: a kernel wrote beyond the workspace" % m
        assert np.isfinite(y).all()
        y64, y32 = (G.mod.targets(f.actor, f.target, f.log_ent_coef, nobs, rew, done, eps_next, G.mod.GAMMA, dt) for dt in (np.float64, np.float32))
        r2 = G.note("%s: targets error / twin error" % which, ref.check_tensors("%s targets B = %d" % (tag, m), {"y": y}, {"y": y64}, {"y": y32}, MULTIPLE))
        end = done != 0
        assert end.any() and not end.all()
        want_end = rew[end] if len(shape) == 1 else np.repeat(rew[end][:, None], shape[1], 1)
        assert np.array_equal(y[end].view(np.uint32), want_end.view(np.uint32)), "B = %d: a terminal row's target is not its reward, bit for bit" % m
        if len(shape) == 2:
            assert (np.diff(y[~end], axis=1) >= 0).all(), "B = %d: a row of y is not sorted" % m
        print("%s: B = %3d, actor forward %.3g, targets %.3g twin errors" % (tag, m, r1, r2))


def actor_gradient(torch, G, which, kname):
    f = G.fixture(which, kname)
    L, D = G.make(torch, kname, actor=f.actor), Data(torch, f)
    shapes = G.mod.actor_shapes(f.O, f.A)
    tag = "%s %s" % (which, kname)
    for m in ef.SIZES:
        idx, rows = batch(G, D, "gradient", m)
        obs, eps = D.host[0][rows], D.eps_pi[rows]
        eps_d = dev(torch, eps)
        whole, n_ws = guard_workspace(torch, G, L, m)
        L.actor_forward(D.arrays[0], dev(torch, idx), eps_d)
        gbuf = torch.full((L.pi.n + GUARD,), 7.0, dtype=torch.float32, device=DEV)
        L.pi.grad = gbuf[:L.pi.n]
        qbuf = torch.full((L.q.n + GUARD,), 7.0, dtype=torch.float32, device=DEV)
        L.q.grad = qbuf[:L.q.n]
        L.ent.grad.fill_(7.0); L.stats.fill_(7.0)
        L.actor_gradient(m, eps_d)
        assert bool((qbuf == 7.0).all()), "the actor's stage wrote into the critic's gradient vector"
        assert bool((gbuf[L.pi.n:] == 7.0).all()), "B = %d: a kernel wrote beyond the gradient vector" % m
        assert bool((whole[n_ws:] == SENTINEL).all()), "B = %d: a kernel wrote beyond the workspace" % m
        got = G.mod.split_flat(h(L.pi.grad), shapes)
        a64, a32 = (G.mod.actor_loss_and_grads(f.actor, f.critic, f.log_ent_coef, obs, eps, dt) for dt in (np.float64, np.float32))
        r = G.note("%s: actor gradient error / twin error" % which, ref.check_tensors("%s actor gradient B = %d" % (tag, m), got, a64.grads, a32.grads, MULTIPLE))
        st = h(L.stats)
        assert st[0] == 7.0 and float(h(L.ent.grad)[0]) == float(np.float32(st[3]))
        pick = lambda a: scalars(loss=a.loss, mean_logp=a.mean_logp, ent_grad=a.ent_grad)  # noqa: E731
        rs = G.note("%s: actor loss, mean logp, entropy-coefficient gradient error / twin error" % which,
                    ref.check_tensors("%s actor statistics B = %d" % (tag, m), scalars(loss=st[1], mean_logp=st[2], ent_grad=st[3]), pick(a64), pick(a32), MULTIPLE))
        line = "%s: B = %3d, actor gradient %.3g, statistics %.3g twin errors" % (tag, m, r, rs)
        if which == "deep":      # the saturated columns: the reference is below 1e-8 alpha / B, anything that leaks through shows
            odd = ef.odd_mu(got)
            ro = G.note("deep: gradient of the odd mu rows error / twin error", ref.check_tensors("%s odd mu rows B = %d" % (tag, m), odd, ef.odd_mu(a64.grads), ef.odd_mu(a32.grads), MULTIPLE))
            G.notes.append("%s B = %d: the gradient of the odd mu rows is exactly zero: %s (largest |entry| %.3g)" % (tag, m, all(not v.any() for v in odd.values()), max(np.abs(v).max() for v in odd.values())))
            line += ", odd mu rows %.3g" % ro
        if which == "clamp":
            rl = G.note("clamp: log_std head gradient error / twin error",
                        ref.check_tensors("%s log_std head B = %d" % (tag, m), ef.log_std_head(got), ef.log_std_head(a64.grads), ef.log_std_head(a32.grads), MULTIPLE))
            line += ", log_std head %.3g" % rl
        print(line)


def whole_step(torch, G, which, kname, m=65):
    """two gradient_steps at B = 65: everything finite afterwards, and the bits of the stages called one by one"""
    f = G.fixture(which, kname)
    D = Data(torch, f)
    idx, rows = batch(G, D, "step", m)
    idx_d, eps_pi, eps_next = dev(torch, idx), dev(torch, D.eps_pi[rows]), dev(torch, D.eps_next[rows])
    L = G.make(torch, kname, actor=f.actor)
    before = G.snapshot(L)
    for _ in range(2):
        L.gradient_step(D.arrays, idx_d, eps_pi, eps_next)
    whole = G.snapshot(L)
    assert all(np.isfinite(x).all() for x in whole), "%s %s: a parameter, moment, gradient or statistic is not finite after the step" % (which, kname)
    assert not any(np.array_equal(a, b) for a, b in zip(whole[:4], before[:4])), "a parameter set did not move"
    L = G.make(torch, kname, actor=f.actor)
    for k in (1, 2):
        L.actor_forward(D.arrays[0], idx_d, eps_pi)
        y = L.targets(D.arrays[1], D.arrays[3], D.arrays[4], idx_d, eps_next)
        L.critic_gradient(D.arrays[0], D.arrays[2], idx_d, y)
        L.adam(L.q, k)
        L.actor_gradient(m, eps_pi)
        L.adam(L.pi, k)
        L.adam(L.ent, k)
        L.polyak(L.q.flat, L.qt.flat, G.mod.TAU)
    assert G.same_bits(whole, G.snapshot(L)), "gradient_step is not the stages called one by one"
