"""The TQC reference (tests/tqc_reference.py) against independent constructions, the fixtures the GPU tests share, and what of
the product needs no GPU.

  * the reference's y, logp, both losses and every gradient tensor against torch float64 autograd on both env kinds (B = 5, 1e-11
    relative), the loss built with torch.sort and the broadcast [B, 2, 25, 46] form; the critic receives no gradient from the
    actor loss; names, shapes and counts of build_tqc_modules;
  * the fixtures: ReLU and the log_std clamp are kinks at which a float32 evaluation may take the other branch, and then no
    tolerance means anything (TQC has no min of two critics; sort, truncation and the quantile Huber gradient are continuous).
    Rows are kept by seeded rejection from a pool of 4096 candidates only if every hidden pre-activation of the eight passes
    (actor on s and s', both critics on (s, a) and (s, a~), both targets on (s', a')) has |z| >= KINK, log_std is KINK inside its
    clamp and |g| <= 4. KINK is 100 x the largest float32-twin error of the pre-activations, MEASURED on the pool and asserted;
  * a three-step sequence whose float64 run and float32 twin take the same side of every kink;
  * the host side of the C ABI: symbols, parameter counts, the workspace query, refusals without a device; the script's --help,
    and the trainer's refusal of a second rank.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import tqc_reference as tr

KINDS = {"swing": 0, "tennis": 1}
POOL = 4096
ROWS = 600                 # the largest batch of the GPU stage tests
KINK = 3.0e-4              # >= 100 x the float32-twin error of a hidden pre-activation (asserted below)
G_MAX = 4.0                # |g| <= 4: 1 - tanh(g)^2 >= 1.3e-3, the float32 twin is a meaningful scale for the squash term
EPS_MAX = 2.5
LOG_ENT_COEF = -0.7        # alpha = 0.497: not 1, so a missing alpha shows
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arrays_of(module, dtype=np.float64):
    return {k: p.detach().cpu().numpy().astype(dtype) for k, p in module.named_parameters()}


class Fixture:
    pass


@functools.lru_cache(maxsize=None)
def fixture(kname):
    """nets of torch's default initialisation (the target an independent draw), a log_std head biased so that log_std spans about
    -1.5 .. 0.5 over the rows, and a pool of POOL candidate transitions with their noise: obs, next_obs ~ N(0, 3^2), action uniform in
    (-1, 1), reward ~ N(0, 1), a fifth of the rows terminal, |eps| <= 2.5. `keep`: the rows that pass every kink condition."""
    import torch
    from tennisbot_rl_amd.tqc import build_tqc_modules
    kind = KINDS[kname]
    O, A = tr.DIMS[kind]
    torch.manual_seed(30 + kind)
    actor, critic, _ = build_tqc_modules(O, A)
    _, target, _ = build_tqc_modules(O, A)
    with torch.no_grad():
        actor.log_std.weight.mul_(0.75)
        actor.log_std.bias.copy_(torch.linspace(-0.45, -0.05, A))
    f = Fixture()
    f.kind, f.O, f.A = kind, O, A
    f.actor, f.critic, f.target = arrays_of(actor, np.float32), arrays_of(critic, np.float32), arrays_of(target, np.float32)
    rng = np.random.default_rng(17 + kind)
    f.obs = rng.normal(0.0, 3.0, (POOL, O)).astype(np.float32)
    f.next_obs = rng.normal(0.0, 3.0, (POOL, O)).astype(np.float32)
    f.action = rng.uniform(-1.0, 1.0, (POOL, A)).astype(np.float32)
    f.reward = rng.normal(0.0, 1.0, POOL).astype(np.float32)
    f.done = (rng.random(POOL) < 0.2).astype(np.float32)
    f.eps_pi = np.clip(rng.normal(0.0, 1.0, (POOL, A)), -EPS_MAX, EPS_MAX).astype(np.float32)
    f.eps_next = np.clip(rng.normal(0.0, 1.0, (POOL, A)), -EPS_MAX, EPS_MAX).astype(np.float32)
    f.log_ent_coef = float(np.float32(LOG_ENT_COEF))
    f.parts64, f.parts32 = parts(f, f.actor, f.critic, f.target, np.float64), parts(f, f.actor, f.critic, f.target, np.float32)
    f.keep = np.nonzero(passes_conditions(f.parts64))[0]
    return f


def parts(f, actor, critic, target, dtype, rows=slice(None)):
    """the eight passes of a step's stages on the pool's rows, each stage at the parameters GIVEN (the critic is not stepped):
    (actor passes, critic passes, the actor-loss result)"""
    ag = tr.actor_loss_and_grads(actor, critic, f.log_ent_coef, f.obs[rows], f.eps_pi[rows], dtype)
    nxt = tr.actor_forward(actor, f.next_obs[rows], f.eps_next[rows], dtype)
    csa = [tr.critic_forward(critic, q, tr.cat(f.obs[rows], f.action[rows], dtype), dtype) for q in (0, 1)]
    tgt = [tr.critic_forward(target, q, tr.cat(f.next_obs[rows], nxt.a, dtype), dtype) for q in (0, 1)]
    return [ag.pi, nxt], csa + list(ag.c) + tgt, ag


def passes_conditions(p):
    relu, clamp, gmax = tr.kink_margins(p)
    return (relu >= KINK) & (clamp >= KINK) & (gmax <= G_MAX)


def batch_of(f, rows):
    return f.obs[rows], f.next_obs[rows], f.action[rows], f.reward[rows], f.done[rows]


# ------------------------------------------------------------------------------------------------------ against torch autograd
def torch_critic_loss(torch, quantiles, y):
    """sb3_contrib's quantile_huber_loss: quantiles [B, 2, 25], y [B, 46], the broadcast [B, 2, 25, 46] form"""
    tau = (torch.arange(tr.N_QUANTILES, dtype=quantiles.dtype) + 0.5) / tr.N_QUANTILES
    delta = y[:, None, None, :] - quantiles[:, :, :, None]
    ad = delta.abs()
    huber = torch.where(ad > 1, ad - 0.5, 0.5 * delta ** 2)
    return ((tau[None, None, :, None] - (delta.detach() < 0).to(quantiles.dtype)).abs() * huber).mean()


@pytest.mark.parametrize("kname", list(KINDS))
def test_reference_against_torch_float64_autograd(kname):
    import torch
    from tennisbot_rl_amd.tqc import ACTOR_NAMES, CRITIC_NAMES, N_TARGETS, build_tqc_modules
    kind = KINDS[kname]
    O, A = tr.DIMS[kind]
    torch.manual_seed(3 + kind)
    actor, critic, target = (m.double() for m in build_tqc_modules(O, A))
    with torch.no_grad():
        for p in target.parameters():
            p.add_(0.05 * torch.randn_like(p))
    assert tuple(k for k, _ in actor.named_parameters()) == ACTOR_NAMES == tr.ACTOR_NAMES
    assert tuple(k for k, _ in critic.named_parameters()) == CRITIC_NAMES == tr.CRITIC_NAMES
    assert tuple(k for k, _ in target.named_parameters()) == CRITIC_NAMES and not any(p.requires_grad for p in target.parameters())
    assert {k: tuple(p.shape) for k, p in actor.named_parameters()} == tr.actor_shapes(O, A)
    assert {k: tuple(p.shape) for k, p in critic.named_parameters()} == tr.critic_shapes(O, A)
    assert tr.n_floats(tr.critic_shapes(O, A)) == (151090, 152114)[kind] and N_TARGETS == tr.N_TARGETS == 46
    B = 5
    rng = np.random.default_rng(11 + kind)
    obs, nobs = rng.normal(0, 2.0, (B, O)), rng.normal(0, 2.0, (B, O))
    act, rew, done = rng.uniform(-1, 1, (B, A)), rng.normal(0, 1, B), np.array([0, 1, 0, 0, 1.0])
    eps_pi, eps_next = rng.normal(0, 1, (B, A)), rng.normal(0, 1, (B, A))
    log_alpha = -0.3
    PA, PC, PT = arrays_of(actor), arrays_of(critic), arrays_of(target)
    T = lambda x: torch.from_numpy(np.asarray(x, np.float64))  # noqa: E731
    rel = lambda got, want: np.abs(np.asarray(got) - np.asarray(want)).max() / max(np.abs(np.asarray(want)).max(), 1e-30)  # noqa: E731
    assert tuple(critic(T(obs), T(act)).shape) == (B, 2, 25)
    # logp and the targets
    with torch.no_grad():
        a_n, lp_n = actor.sample(T(nobs), T(eps_next))
        z, _ = torch.sort(target(T(nobs), a_n).reshape(B, -1))
        y_t = T(rew)[:, None] + (1 - T(done))[:, None] * tr.GAMMA * (z[:, :N_TARGETS] - np.exp(log_alpha) * lp_n[:, None])
    y, pi_n, _ = tr.targets(PA, PT, log_alpha, nobs, rew, done, eps_next, full=True)
    assert y.shape == (B, 46)
    assert rel(pi_n.logp, lp_n.numpy()) <= 1e-11 and rel(pi_n.a, a_n.numpy()) <= 1e-11 and rel(y, y_t.numpy()) <= 1e-11
    assert np.array_equal(y[done == 1], np.repeat(rew[done == 1][:, None], 46, 1))
    assert (np.diff(y[done == 0], axis=1) >= 0).all()
    # the critic loss
    loss_t = torch_critic_loss(torch, critic(T(obs), T(act)), y_t)
    g_t = torch.autograd.grad(loss_t, list(critic.parameters()))
    loss, grads = tr.critic_loss_and_grads(PC, obs, act, y)
    assert abs(loss - float(loss_t.detach())) <= 1e-11 * abs(float(loss_t.detach())) and tuple(grads) == tr.CRITIC_NAMES and len(grads) == 12
    for k, g in zip(tr.CRITIC_NAMES, g_t):
        assert rel(grads[k], g.numpy()) <= 1e-11, k
    # the actor loss: gradients for the actor, none for the critic in the reference's output
    a_pi, lp = actor.sample(T(obs), T(eps_pi))
    aloss_t = (np.exp(log_alpha) * lp - critic(T(obs), a_pi).mean(2).mean(1)).mean()
    ga_t = torch.autograd.grad(aloss_t, list(actor.parameters()))
    ag = tr.actor_loss_and_grads(PA, PC, log_alpha, obs, eps_pi)
    assert abs(ag.loss - float(aloss_t.detach())) <= 1e-11 * abs(float(aloss_t.detach())) and rel(ag.pi.logp, lp.detach().numpy()) <= 1e-11
    assert tuple(ag.grads) == tr.ACTOR_NAMES and len(ag.grads) == 8 and not any(k.startswith("qf") for k in ag.grads)
    for k, g in zip(tr.ACTOR_NAMES, ga_t):
        assert rel(ag.grads[k], g.numpy()) <= 1e-11, k
    la = torch.tensor([log_alpha], dtype=torch.float64, requires_grad=True)
    ent_t = torch.autograd.grad(-(la * (lp.detach() - A)).mean(), la)[0]
    assert abs(ag.ent_grad - float(ent_t)) <= 1e-11 * abs(float(ent_t)) and abs(ag.mean_logp - float(lp.detach().mean())) <= 1e-11 * abs(float(lp.detach().mean()))


def test_reference_sort_keeps_ties_and_puts_nan_last():
    """what the tie and NaN cases of the GPU tests rely on"""
    f = fixture("swing")
    rows = f.keep[:7]
    twice = dict(f.target)
    for k in list(twice):
        if k.startswith("qf1."):
            twice[k] = f.target["qf0." + k[4:]].copy()
    y, _, t = tr.targets(f.actor, twice, f.log_ent_coef, f.next_obs[rows], f.reward[rows], f.done[rows], f.eps_next[rows], full=True)
    live = f.done[rows] == 0
    assert np.array_equal(t[0].q, t[1].q) and np.array_equal(y[live][:, 0:46:2], y[live][:, 1:46:2])
    bad = dict(f.target)
    bad["qf1.4.bias"] = f.target["qf1.4.bias"].copy()
    bad["qf1.4.bias"][3] = np.nan
    y, _, t = tr.targets(f.actor, bad, f.log_ent_coef, f.next_obs[rows], f.reward[rows], f.done[rows], f.eps_next[rows], full=True)
    assert np.isnan(t[1].q[:, 3]).all() and np.isfinite(y).all()


def test_rate_tool_torch_step_is_the_reference_step():
    """tools/tqc_rate.py's torch-autograd form (the baseline of the measured rates) is the rule: one step in float64 against the
    reference's gradient_step, parameters, target and log_ent_coef to 1e-11 of the step's size"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import tqc_rate
    finally:
        sys.path.pop(0)
    from tennisbot_rl_amd.tqc import build_tqc_modules
    O, A, B = 6, 6, 7
    torch.manual_seed(0)
    actor, critic, target = (m.double() for m in build_tqc_modules(O, A))
    with torch.no_grad():
        for p in target.parameters():
            p.add_(0.05 * torch.randn_like(p))
    lec = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    S = tr.State(arrays_of(actor), arrays_of(critic), arrays_of(target), 0.0)
    start = {"actor": S.actor, "critic": S.critic, "target": S.target}
    opts = tuple(torch.optim.Adam(ps, lr=tr.LR, eps=tr.ADAM_EPS) for ps in (actor.parameters(), critic.parameters(), [lec]))
    rng = np.random.default_rng(0)
    batch = (rng.normal(size=(B, O)), rng.normal(size=(B, O)), rng.uniform(-1, 1, (B, A)), rng.normal(size=B), np.array([0, 0, 1, 0, 1, 0, 0.0]))
    eps_pi, eps_next = rng.normal(size=(B, A)), rng.normal(size=(B, A))
    T = lambda x: torch.from_numpy(np.asarray(x, np.float64))  # noqa: E731
    tqc_rate.torch_step(torch, actor, critic, target, lec, opts, tuple(T(x) for x in batch), T(eps_pi), T(eps_next), tr.GAMMA, tr.TAU, A)
    tr.gradient_step(S, batch, eps_pi, eps_next)
    for name, module, after in (("actor", actor, S.actor), ("critic", critic, S.critic), ("target", target, S.target)):
        for k, p in module.named_parameters():
            moved = np.abs(after[k] - start[name][k]).max()
            assert moved > 0 and np.abs(p.detach().numpy() - after[k]).max() <= 1e-11 * moved, (name, k)
    assert abs(float(lec.detach()) - S.ent["log_ent_coef"][0]) <= 1e-11 * abs(S.ent["log_ent_coef"][0])


# ------------------------------------------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("kname", list(KINDS))
def test_fixture_margins_are_measured(kname):
    f = fixture(kname)
    (a64, c64, ag64), (a32, c32, ag32) = f.parts64, f.parts32
    z_err = max(max(np.abs(p.z1 - q.z1).max(), np.abs(p.z2 - q.z2).max()) for p, q in zip(a64 + c64, a32 + c32))
    raw_err = max(np.abs(p.raw - q.raw).max() for p, q in zip(a64, a32))
    print("%s: float32-twin error on the pool: pre-activations %.3g, log_std %.3g; %d of %d rows kept" % (kname, z_err, raw_err, len(f.keep), POOL))
    assert 100.0 * z_err <= KINK and 100.0 * raw_err <= KINK
    assert len(f.keep) >= ROWS, "the pool leaves %d rows, %d are needed" % (len(f.keep), ROWS)
    rows = f.keep[:ROWS]
    relu, clamp, gmax = tr.kink_margins(parts(f, f.actor, f.critic, f.target, np.float64, rows))
    assert relu.min() >= KINK and clamp.min() >= KINK and gmax.max() <= G_MAX
    ls = np.concatenate([p.ls for p in parts(f, f.actor, f.critic, f.target, np.float64, rows)[0]])
    print("%s: log_std over the fixture's rows %.3f .. %.3f" % (kname, ls.min(), ls.max()))
    assert -2.0 < ls.min() < -0.6 and 0.1 < ls.max() < 1.0   # spread well away from 0, far inside the clamp [-20, 2]
    assert np.abs(f.eps_pi).max() <= EPS_MAX and np.abs(f.eps_next).max() <= EPS_MAX
    assert 0 < f.done[rows].sum() < ROWS
    # on those rows the twin took every branch the float64 run took
    p32 = parts(f, f.actor, f.critic, f.target, np.float32, rows)
    p64 = parts(f, f.actor, f.critic, f.target, np.float64, rows)
    for a, b in zip(p64[0] + p64[1], p32[0] + p32[1]):
        assert np.array_equal(a.z1 > 0, b.z1 > 0) and np.array_equal(a.z2 > 0, b.z2 > 0)
    for a, b in zip(p64[0], p32[0]):           # ... and the clamp's side
        side = lambda p: (p.raw < tr.LOG_STD_MIN).astype(int) - (p.raw > tr.LOG_STD_MAX).astype(int)  # noqa: E731
        assert np.array_equal(side(a), side(b))


def sequence(kname, B=64, steps=3):
    """`steps` gradient steps of the float64 reference and of its float32 twin on batches the reference chooses from the pool at
    the parameters it has reached: rows that pass every kink condition there. The critics' passes on (s, a~) run with the STEPPED
    critic, which depends on the batch but not on eps_pi: a row that loses its margin there gets a fresh eps_pi (seeded) until
    the step's own eight passes hold every margin. Returns (per step (rows, eps_pi, eps_next), the float64 steps, the twin's
    steps, the two final states)."""
    import copy
    f = fixture(kname)
    S64, S32 = (tr.State(f.actor, f.critic, f.target, f.log_ent_coef, dt) for dt in (np.float64, np.float32))
    chosen, out64, out32 = [], [], []
    for k in range(steps):
        rng = np.random.default_rng(40 + k)
        cand = np.nonzero(passes_conditions(parts(f, S64.actor, S64.critic, S64.target, np.float64)))[0]
        assert len(cand) >= B
        rows = rng.permutation(cand)[:B]
        eps_pi, eps_next = f.eps_pi[rows].copy(), f.eps_next[rows]
        for _ in range(40):
            st = tr.gradient_step(copy.deepcopy(S64), batch_of(f, rows), eps_pi, eps_next)
            relu, clamp, gmax = tr.kink_margins(st)
            bad = ~((relu >= KINK) & (clamp >= KINK) & (gmax <= G_MAX))
            if not bad.any():
                break
            eps_pi[bad] = np.clip(rng.normal(0.0, 1.0, (int(bad.sum()), f.A)), -EPS_MAX, EPS_MAX).astype(np.float32)
        assert not bad.any()
        chosen.append((rows, eps_pi, eps_next))
        out64.append(tr.gradient_step(S64, batch_of(f, rows), eps_pi, eps_next))
        out32.append(tr.gradient_step(S32, batch_of(f, rows), eps_pi, eps_next))
    return chosen, out64, out32, S64, S32


@functools.lru_cache(maxsize=None)
def cached_sequence(kname):
    return sequence(kname)


@pytest.mark.parametrize("kname", list(KINDS))
def test_three_step_sequence_takes_the_same_side_of_every_kink(kname):
    rows, s64, s32, S64, S32 = cached_sequence(kname)
    for k, (a, b) in enumerate(zip(s64, s32)):
        assert tr.same_sides(a, b), "step %d: the float32 twin took another branch" % k
        relu, clamp, gmax = tr.kink_margins(a)
        assert relu.min() >= KINK and clamp.min() >= KINK and gmax.max() <= G_MAX
    assert S64.adam["critic"]["t"] == S64.adam["actor"]["t"] == S64.adam["ent"]["t"] == 3
    assert S64.ent["log_ent_coef"][0] != np.float32(LOG_ENT_COEF)
    f = fixture(kname)
    assert any(not np.array_equal(S64.target[k], f.target[k]) for k in f.target)


# ------------------------------------------------------------------------------------------------------ the host side of the ABI
@pytest.fixture(scope="module")
def lib():
    from tennisbot_rl_amd.build import build_library
    from tennisbot_rl_amd.stepper import load_library
    build_library()
    return load_library()


def test_tqc_symbols_counts_and_workspace_query(lib):
    for name in ("tb_tqc_param_floats", "tb_tqc_workspace_bytes", "tb_tqc_actor_forward", "tb_tqc_targets", "tb_tqc_critic_grad", "tb_tqc_actor_grad", "tb_sac_adam"):
        assert hasattr(lib, name), name
    assert lib.tb_abi_version() == 4
    assert [lib.tb_tqc_param_floats(k, w) for k in (0, 1) for w in (0, 1)] == [70668, 151090, 70148, 152114]
    for kind in (0, 1):
        O, A = tr.DIMS[kind]
        assert lib.tb_tqc_param_floats(kind, 0) == lib.tb_sac_param_floats(kind, 0) == tr.n_floats(tr.actor_shapes(O, A))
        assert tr.n_floats(tr.critic_shapes(O, A)) == lib.tb_tqc_param_floats(kind, 1)
        sizes = [lib.tb_tqc_workspace_bytes(kind, b) for b in (1, 2, 16, 17, 256, 1100, 4096)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
        assert sizes[0] % 8 == 0 and sizes[0] > lib.tb_sac_workspace_bytes(kind, 1)     # the head regions are wider than SAC's
    for bad in (lib.tb_tqc_param_floats(2, 0), lib.tb_tqc_param_floats(0, 2), lib.tb_tqc_param_floats(-1, 1), lib.tb_tqc_workspace_bytes(5, 16), lib.tb_tqc_workspace_bytes(0, 0)):
        assert bad == -1 and b"tb_tqc_" in lib.tb_last_error()


def test_tqc_refusals_need_no_device(lib):
    buf = (ctypes.c_double * 8192)()
    a = ctypes.addressof(buf)
    assert a % 8 == 0
    ws = lib.tb_tqc_workspace_bytes(0, 4)

    def refused(fn, args, word, code=(-1,)):
        rc = fn(*args)
        assert rc in code and word in lib.tb_last_error() and b"tb_tqc_" in lib.tb_last_error(), (rc, lib.tb_last_error())

    calls = [
        # (arguments, pointer positions, (kind, batch, workspace, workspace bytes) positions)
        (lib.tb_tqc_actor_forward, ([0, 0, None, a, 100, a, 4, a, a, a, a, a, ws], (3, 5, 7, 8, 9, 10), (0, 6, 11, 12))),
        (lib.tb_tqc_targets, ([0, 0, None, a, a, a, 100, a, 4, a, a, a, a, 0.99, a, a, ws], (3, 4, 5, 7, 9, 10, 11, 12, 14), (0, 8, 15, 16))),
        (lib.tb_tqc_critic_grad, ([0, 0, None, a, a, 100, a, 4, a, a, a + 4096, a, a, ws], (3, 4, 6, 8, 9, 10, 11), (0, 7, 12, 13))),
        (lib.tb_tqc_actor_grad, ([0, 0, None, 4, a, a, a, a, a + 4096, a, a, a, ws], (4, 5, 6, 7, 8, 9, 10), (0, 3, 11, 12))),
    ]
    for fn, (args, pointers, (k_kind, k_batch, k_ws, k_bytes)) in calls:
        for k in pointers + (k_ws,):
            bad = list(args); bad[k] = None
            refused(fn, bad, b"null")
        bad = list(args); bad[k_kind] = 7
        refused(fn, bad, b"env kind")
        bad = list(args); bad[k_batch] = 0
        refused(fn, bad, b"batch")
        bad = list(args); bad[k_bytes] = ws - 1
        refused(fn, bad, b"tb_tqc_workspace_bytes", code=(-3,))   # TB_E_PARAMS: a workspace that is too small
        bad = list(args); bad[k_bytes] = lib.tb_sac_workspace_bytes(0, 4)
        refused(fn, bad, b"workspace", code=(-3,))                # ... SAC's size is too small for TQC's head regions
        bad = list(args); bad[k_ws] = a + 4
        refused(fn, bad, b"aligned")
        bad = list(args); bad[pointers[0]] = a + 2
        refused(fn, bad, b"aligned")
    fwd, tgt, cg, ag = ((fn, args) for fn, (args, _, _) in calls)
    for (fn, args), k in ((fwd, 4), (tgt, 6), (cg, 5)):
        bad = list(args); bad[k] = 0
        refused(fn, bad, b"n_rows")
    bad = list(cg[1]); bad[10] = bad[8]
    refused(lib.tb_tqc_critic_grad, bad, b"grad_dev must not be critic_dev")
    bad = list(ag[1]); bad[8] = bad[4]
    refused(lib.tb_tqc_actor_grad, bad, b"actor_grad_dev must not be actor_dev")


# ----------------------------------------------------------------------------------------------------------- script and trainer
def test_train_tqc_help_names_both_envs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train_tqc.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "SwingRacket-v0" in out.stdout and "Tennisbot-v0" in out.stdout
    for flag in ("--total-timesteps", "--batch-size", "--gradient-steps", "--num-envs", "--seed", "--save", "--load", "--curri"):
        assert flag in out.stdout, flag


def test_train_swing_points_to_train_tqc():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train_swing.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "train_tqc.py" in out.stdout


def test_trainer_refuses_more_than_one_rank(monkeypatch):
    import torch
    from tennisbot_rl_amd.tqc import TQCTrainer
    monkeypatch.setattr(torch.distributed, "is_available", lambda: True)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True, raising=False)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2, raising=False)
    with pytest.raises(ValueError, match="one rank"):
        TQCTrainer("SwingRacket-v0", num_envs=64)


def test_learner_refuses_other_counts_and_a_cpu_device():
    """(the counts and the device are checked first; the optimiser and architecture refusals need a device: tests/test_gpu_tqc.py)"""
    import torch
    from tennisbot_rl_amd.stepper import StepperError
    from tennisbot_rl_amd.tqc import FusedTQC, build_tqc_modules
    actor, critic, target = build_tqc_modules(6, 6)
    lec = torch.zeros(1)
    opts = (torch.optim.Adam(actor.parameters()), torch.optim.Adam(critic.parameters()), torch.optim.Adam([lec]))
    with pytest.raises(StepperError, match="GPU"):
        FusedTQC(0, actor, critic, target, lec, opts, {}, "cpu")
    for kw in (dict(n_quantiles=24), dict(n_critics=3), dict(top_quantiles_to_drop_per_net=5)):
        with pytest.raises(StepperError, match="the kernels take 25 quantiles, 2 critics and 2 dropped per net"):
            FusedTQC(0, actor, critic, target, lec, opts, {}, "cpu", **kw)
