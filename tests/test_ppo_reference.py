"""The PPO learner (PPOTrainer.advantages / PPOTrainer.update) against the float64 reference of tests/ppo_reference.py, on CPU.

First the reference itself: its hand-written gradient against central finite differences on every parameter tensor, its GAE
against closed cases, its Adam against torch.optim.Adam in float64. Then the product: `advantages` and `update` only touch
attributes, so they run unbound on a stand-in (types.SimpleNamespace) that holds CPU tensors. Compared: every advantage and
return within the reference's a-priori bound; the clipped gradient a one-minibatch update leaves in p.grad and its three
statistics; the parameters after 2 epochs x 3 minibatches (ragged tail) from recorded permutations, as (p - p0) / lr; two gloo
ranks' averaged-then-clipped gradient. Finally the checker is shown to reject eight wrong learners.

Tolerances. GAE: the reference's a-priori bound itself. Everything else: ppo_reference.MULTIPLE = 24 float32-twin errors per tensor
in the max norm (ppo_reference.check_tensors; the twin is the reference run in float32 on the same inputs; its error is floored at
u max|tensor|), every element included. No element needed an allowance for Adam's ill-conditioned g / (|g| + eps).

Measured, in twin errors (largest over the cases):          CPU (torch)      MI355X (real PPOTrainer, both env ids)
    GAE |error| / bound                                      0.67             0.47
    gradients: weights (batch GEMMs)                         2.1              11.5   (2 .. 12 on every layer's weight)
    gradients: biases, log_std (column sums)                 1.7              1.1    (mostly 0.01 .. 0.3)
    statistics                                               2.9              2.6
    parameter change after six Adam steps                    1.9              2.6
    twin error itself: gradients                             3.2e-7 absolute  3.5e-7 (clipped gradients, norm <= 0.5)
    twin error itself: parameter change                      3.8e-4 lr        1.1e-3 lr
    wrong learners                                           >= 55 (biased std over 21 000 rows: a 2.4e-5 relative change); others 7e4 .. 6e8
GAE on CPU peaks one step before an episode end, a chain of three roundings where a worst-case bound is nearly attained; mean 0.06.

Why 24. The twin's error is not one scale but two, and the twin shows both by itself: its weight gradients come out of a blocked
BLAS GEMM (many partial sums) and err by 4 .. 8 u max|g|, its bias gradients are plain sequential column sums over the same rows
and err by 36 .. 72 u max|g| (26 624 rows of an oracle-stepped SwingRacket rollout) -- a factor of about 9 between two legitimate
float32 summation orders of the same batch. A learner whose GEMM accumulates the batch dimension in long sequential runs, as the
GPU library's does, lands on the second scale for its weights: that is the 2 .. 12 above, while its bias sums (tree reductions)
sit far below 1. On top of that the twin's error is one sample: over 8 row orders of one case it varied 1.4- to 3.9-fold per
multi-element tensor. 24 = 9 x 2.7 covers both, from the reference's own figures; the product's largest is 11.5, the smallest
mistake 55. (The multiple stood at 8 before anything had been measured on the GPU.)
"""
import os
import socket
import types

import numpy as np
import pytest

import ppo_reference as ref
from policy_reference import assert_within, excess, state_dict_arrays

MULTIPLE = ref.MULTIPLE
WORLD = 2
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print("ppo reference (cpu): largest %s = %.3g" % (k, RATIOS[k]))


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


# ----------------------------------------------------------------------------------------------------------------- the inputs
CASES = {  # arch, kind name, T, n, done pattern, batch size of the ragged update (3 minibatches, a small tail)
    "swing-52-lockstep": ((32, 64, 32), "swing", 52, 300, "every26", 7500),
    "swing-70-midepisode": ((32, 64, 32), "swing", 70, 300, "every26+7", 10000),
    "tennis-70-ragged": ((64, 64), "tennis", 70, 300, "ragged", 10000),
    "tennis-52-ragged": ((64, 64), "tennis", 52, 300, "ragged", 7500),
}
_cache = {}


def make_policy(arch, kind, seed=11):
    import torch
    from tennisbot_rl_amd.params import ACT_DIM, OBS_DIM
    from tennisbot_rl_amd.ppo import build_actor_critic
    torch.manual_seed(seed)
    policy = build_actor_critic(OBS_DIM[kind], ACT_DIM[kind], tuple(arch))
    with torch.no_grad():  # off SB3's init: a mean that depends on the observation, unequal stds, non-zero biases
        policy.action_net.weight.mul_(30.0)
        policy.log_std.copy_(torch.linspace(-0.3, 0.4, ACT_DIM[kind]))
        for p in policy.parameters():
            if p.dim() == 1 and p is not policy.log_std:
                p.normal_(0.0, 0.1)
    return policy


def make_rollout(name, rank=0):
    """a synthetic rollout for CASES[name]: float32 arrays, and the hyper-parameters"""
    from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, OBS_DIM
    from tennisbot_rl_amd.ppo import COMMON, SWING_DEFAULTS, TENNIS_DEFAULTS
    import torch
    arch, kname, T, n, pattern, batch = CASES[name]
    kind = ENV_SWING if kname == "swing" else ENV_TENNIS
    hp = dict(SWING_DEFAULTS if kname == "swing" else TENNIS_DEFAULTS)
    assert tuple(hp["net_arch"]) == arch
    hp.update(COMMON)
    rng = np.random.default_rng(1000 * rank + sum(map(ord, name)))
    O, A = OBS_DIM[kind], ACT_DIM[kind]
    k = np.arange(T)[:, None]
    if pattern.startswith("every26"):
        phase = int(pattern[8:] or 0)
        dones = np.broadcast_to((k + phase) % 26 == 25, (T, n)).copy()
    else:  # Tennisbot-like: episodes of 15 .. 60 steps, every env on its own clock
        dones = np.zeros((T, n), bool)
        for e in range(n):
            t = int(rng.integers(0, 40))
            while t < T:
                dones[t, e] = True
                t += int(rng.integers(15, 60))
    dones[:, 0] = False                                   # an env that never finishes
    dones[:, 1] = False; dones[0, 1] = dones[T - 1, 1] = True  # ... and one that is done at steps 0 and T - 1
    rewards = rng.normal(0.0, 0.3, (T, n)) + 2.0 * (rng.random((T, n)) < 0.1) + 50.0 * (dones & (rng.random((T, n)) < 0.3))  # +50: the goal bonus
    obs = rng.normal(0.0, 1.5, (T, n, O)).astype(np.float32)
    policy = make_policy(arch, kind)
    with torch.no_grad():
        mean, v_pred = policy(torch.from_numpy(obs.reshape(T * n, O)))
        raw = mean + policy.log_std.exp() * torch.from_numpy(rng.normal(size=(T * n, A)).astype(np.float32))
        _, logp, _ = policy.evaluate(torch.from_numpy(obs.reshape(T * n, O)), raw)
    # the behaviour policy's logp, shifted: the ratio leaves [0.8, 1.2] on both sides for a good share of the rows
    old_logp = logp.numpy().reshape(T, n) + rng.normal(0.0, 0.25, (T, n))
    values = 12.0 + 8.0 * rng.normal(size=(T, n)) + v_pred.numpy().reshape(T, n)   # a critic at the scale of the returns
    f = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    return types.SimpleNamespace(name=name, kind=kind, arch=arch, T=T, n=n, O=O, A=A, hp=hp, batch=batch, dones=dones.astype(np.uint8), rewards=f(rewards),
                                 obs=obs, raw=f(raw.numpy().reshape(T, n, A)), old_logp=f(old_logp), values=f(values), v_pred=f(v_pred.numpy().reshape(T, n)),
                                 last_value=f(12.0 + 8.0 * rng.normal(size=n)))


def rollout(name):
    if name not in _cache:
        ro = make_rollout(name)
        ro.gae = ref.gae(ro.rewards, ro.values, ro.dones, ro.last_value, ro.hp["gamma"], ro.hp["gae_lambda"])
        for a in (ro.gae.adv, ro.gae.returns, ro.gae.adv_bound, ro.gae.returns_bound):
            a.setflags(write=False)
        _cache[name] = ro
    return _cache[name]


def stand_in(ro, world=1, n_epochs=None, batch_size=None, **hp):
    """what PPOTrainer.advantages / .update touch, on CPU tensors"""
    import torch
    from tennisbot_rl_amd.rollout import RolloutBuffer
    h = dict(ro.hp, **hp)
    if n_epochs is not None:
        h["n_epochs"] = n_epochs
    buf = RolloutBuffer(ro.kind, ro.T, ro.n, "cpu")
    buf.rewards.copy_(torch.from_numpy(ro.rewards)); buf.dones.copy_(torch.from_numpy(ro.dones))
    buf.obs.copy_(torch.from_numpy(np.concatenate([ro.obs[1:], ro.obs[:1]])))
    buf.actions.copy_(torch.from_numpy(ro.raw).clamp(-1.0, 1.0))
    policy = make_policy(ro.arch, ro.kind)
    ns = types.SimpleNamespace(torch=torch, hp=h, buf=buf, n_steps=ro.T, num_envs=ro.n, device=torch.device("cpu"), world=world, policy=policy,
                               opt=torch.optim.Adam(policy.parameters(), lr=h["learning_rate"], eps=1e-5), batch_size=batch_size or ro.T * ro.n,
                               values=torch.from_numpy(ro.values.copy()), logps=torch.from_numpy(ro.old_logp.copy()),
                               obs_seq=torch.from_numpy(ro.obs.copy()), _raw_actions=torch.from_numpy(ro.raw.copy()))
    return ns


def flat_shard(ro, adv, returns):
    N = ro.T * ro.n
    return (ro.obs.reshape(N, -1), ro.raw.reshape(N, -1), ro.old_logp.reshape(N), np.asarray(adv, np.float32).reshape(N), np.asarray(returns, np.float32).reshape(N))


def returns_near_the_critic(ro):
    """returns scaled towards the policy's own value predictions: the value gradient stays small, the norm clip idle"""
    return (ro.v_pred + 0.01 * (ro.gae.returns - ro.v_pred)).astype(np.float32)


# ------------------------------------------------------------------------------------------------- the reference checks itself
@pytest.mark.parametrize("name", ["swing-52-lockstep", "tennis-70-ragged"])
def test_reference_gradient_matches_central_differences(name):
    ro = rollout(name)
    rows = np.random.default_rng(5).permutation(ro.T * ro.n)[:400]
    shard = [x[rows] for x in flat_shard(ro, ro.gae.adv, ro.gae.returns)]
    shard[4] = (shard[4] * 0.05).astype(np.float32)   # the value loss at the size of the others: every gradient is of order 1e-1 .. 1
    P = state_dict_arrays(make_policy(ro.arch, ro.kind))
    res = ref.loss_and_grads(P, *shard, ro.hp)
    share = float(((res.ratio < 0.8) | (res.ratio > 1.2)).mean())
    assert 0.2 < share < 0.8, share                      # clipped and unclipped rows both take part
    rng = np.random.default_rng(6)
    assert set(res.grads) == set(P)
    for k, p in P.items():
        idx = [np.unravel_index(i, p.shape) for i in rng.permutation(p.size)[:12]]
        for i in idx:
            # central differences: truncation h^2 f''' / 6 and rounding eps |loss| / h balance near h = 1e-5 for a loss of order 1 (a
            # row whose ratio crosses the clip inside [p - h, p + h] adds a kink: its share of the gradient, a_i / 400 <= 1e-2, times
            # the chance of a crossing, ~ h |d ratio / d p| ~ 1e-4)
            h = 1e-5
            Pp, Pm = dict(P), dict(P)
            Pp[k], Pm[k] = p.copy(), p.copy()
            Pp[k][i] += h; Pm[k][i] -= h
            fd = (ref.scalar_loss(Pp, *shard, ro.hp) - ref.scalar_loss(Pm, *shard, ro.hp)) / (2 * h)
            assert abs(fd - res.grads[k][i]) <= 1e-6 + 1e-6 * abs(fd), (k, i, fd, res.grads[k][i])


def test_reference_gae_closed_cases():
    ro = rollout("tennis-70-ragged")
    r, V, d, lv = ro.rewards.astype(np.float64), ro.values.astype(np.float64), ro.dones, ro.last_value.astype(np.float64)
    g = 0.99
    T, n = r.shape
    nt = 1.0 - d
    Vn = np.concatenate([V[1:], lv[None]])
    delta = r + g * Vn * nt - V
    assert d.sum() > n and not d[:, 0].any() and d[0, 1] and d[T - 1, 1]
    # lambda = 0: the one-step TD error
    np.testing.assert_allclose(ref.gae(r, V, d, lv, g, 0.0).adv, delta, rtol=0, atol=1e-12)
    # lambda = 1: the discounted return of the rest of the episode (bootstrapped with last_value where it is still running) minus V
    want = np.zeros_like(r)
    for e in range(n):
        for k in range(T):
            ret, disc, l = 0.0, 1.0, k
            while True:
                ret += disc * r[l, e]
                disc *= g
                if d[l, e]:
                    break
                l += 1
                if l == T:
                    ret += disc * lv[e]
                    break
            want[k, e] = ret - V[k, e]
    np.testing.assert_allclose(ref.gae(r, V, d, lv, g, 1.0).adv, want, rtol=0, atol=1e-10)
    # a done at the last step: last_value does not matter (env 1), and it does where the episode is still running (env 0)
    a, b = ref.gae(r, V, d, lv, g, 0.95).adv, ref.gae(r, V, d, lv + 100.0, g, 0.95).adv
    last_done = d[T - 1] != 0
    assert last_done.any() and not last_done.all()
    assert np.array_equal(a[:, last_done], b[:, last_done]) and (np.abs(a - b)[T - 1, ~last_done] > 90.0).all()
    # a done at k: A[k] does not depend on anything after k
    rng = np.random.default_rng(2)
    r2, V2, d2 = r.copy(), V.copy(), d.copy()
    for e in range(2, n):
        ks = np.flatnonzero(d[:, e])
        if ks.size and ks[0] < T - 1:
            k = ks[0]
            r2[k + 1:, e] = rng.normal(size=T - 1 - k); V2[k + 1:, e] = rng.normal(size=T - 1 - k); d2[k + 1:, e] = rng.random(T - 1 - k) < 0.3
    c = ref.gae(r2, V2, d2, lv * 3.0, g, 0.95).adv
    first = np.array([np.flatnonzero(d[:, e])[0] if d[:, e].any() else -1 for e in range(n)])
    assert (first[2:] >= 0).sum() > n // 2
    for e in range(2, n):
        if first[e] >= 0:
            assert np.array_equal(a[:first[e] + 1, e], c[:first[e] + 1, e]), e


def test_reference_adam_matches_torch_in_float64():
    import torch
    rng = np.random.default_rng(3)
    P = {"a": rng.normal(size=(5, 7)), "b": rng.normal(size=3)}
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in P.items()}
    opt = torch.optim.Adam(list(tp.values()), lr=3e-4, eps=1e-5)
    state = ref.adam_init(P)
    for step in range(25):
        G = {k: rng.normal(size=v.shape) * 10.0 ** rng.integers(-7, 1, v.shape) for k, v in P.items()}   # gradients above and below eps
        for k in tp:
            tp[k].grad = torch.tensor(G[k])
        opt.step()
        P = ref.adam_step(P, G, state, 3e-4)
        for k in P:
            np.testing.assert_allclose(P[k], tp[k].detach().numpy(), rtol=0, atol=1e-15)
    G = {k: rng.normal(size=v.shape) for k, v in P.items()}
    for k in tp:
        tp[k].grad = torch.tensor(G[k])
    tn = float(torch.nn.utils.clip_grad_norm_(list(tp.values()), 0.5))
    clipped, norm = ref.clip_global_norm(G, 0.5)
    assert abs(norm - tn) < 1e-12 and all(np.allclose(clipped[k], tp[k].grad.numpy(), rtol=0, atol=1e-15) for k in G)
    small = {k: v * 1e-3 for k, v in G.items()}
    assert all(np.array_equal(ref.clip_global_norm(small, 0.5)[0][k], small[k]) for k in G)   # below the norm: untouched


# ------------------------------------------------------------------------------------------------------ the product on CPU
def check_gae(tag, adv, returns, want):
    r = max(assert_within(tag + " advantages", adv, want.adv, want.adv_bound), assert_within(tag + " returns", returns, want.returns, want.returns_bound))
    return note("GAE |error| / bound", r)


@pytest.mark.parametrize("name", list(CASES))
def test_advantages_match_the_definition_within_the_bound(name):
    from tennisbot_rl_amd.ppo import PPOTrainer
    import torch
    ro = rollout(name)
    ns = stand_in(ro)
    adv, returns = PPOTrainer.advantages(ns, torch.from_numpy(ro.last_value))
    assert adv.shape == (ro.T, ro.n) and adv.dtype == torch.float32
    r = check_gae(name, adv.numpy(), returns.numpy(), ro.gae)
    print("%s: GAE |error| / bound %.3g, largest |A| %.3g, largest bound %.3g" % (name, r, np.abs(ro.gae.adv).max(), ro.gae.adv_bound.max()))
    assert np.abs(ro.gae.adv).max() > 30.0          # the +50 bonus is in there
    # the float32 twin of the definition keeps the bound as well (another evaluation order of the same sum)
    twin = ref.gae(ro.rewards, ro.values, ro.dones, ro.last_value, ro.hp["gamma"], ro.hp["gae_lambda"], np.float32)
    assert twin.adv.dtype == np.float32
    note("GAE twin |error| / bound", assert_within("twin", twin.adv, ro.gae.adv, ro.gae.adv_bound))


def single_minibatch(ro, adv, returns, **hp):
    """one epoch, one minibatch through the product: p.grad as left behind, the statistics, and the reference's float64 and
    float32 answers"""
    from tennisbot_rl_amd.ppo import PPOTrainer
    import torch
    ns = stand_in(ro, n_epochs=1, **hp)
    P = state_dict_arrays(ns.policy)
    stats = PPOTrainer.update(ns, torch.from_numpy(np.asarray(adv, np.float32)), torch.from_numpy(np.asarray(returns, np.float32)))
    shard = flat_shard(ro, adv, returns)
    N = ro.T * ro.n
    perms = [[np.arange(N)]]
    return ns, stats, ref.replay_update(P, [shard], perms, N, ns.hp), ref.replay_update(P, [shard], perms, N, ns.hp, np.float32), shard, P


def check_update(tag, got_grads, got_stats, want, twin):
    r = ref.check_tensors(tag + " gradient", got_grads, want.grads, twin.grads, MULTIPLE)
    note("gradient error / twin error", r)
    note("twin gradient error, absolute", max(np.abs(np.asarray(twin.grads[k], np.float64) - want.grads[k]).max() for k in want.grads))
    s = ref.check_tensors(tag + " statistics", {k: np.float64(v) for k, v in got_stats.items()}, want.stats[0], twin.stats[0], MULTIPLE)
    note("statistics error / twin error", s)
    return r, s


@pytest.mark.parametrize("name", list(CASES))
def test_single_minibatch_gradient_and_statistics(name):
    """norm clip active (returns far from the critic) and idle (returns near it); the ratio clip binds on both sides for both
    signs of the advantage"""
    ro = rollout(name)
    ns, stats, want, twin, shard, P = single_minibatch(ro, ro.gae.adv, ro.gae.returns)
    assert want.norms[0] > 2 * ro.hp["max_grad_norm"], want.norms          # the clip is active ...
    res = ref.loss_and_grads(P, *shard, ns.hp)
    for side, bound in (("low", res.ratio < 0.8), ("high", res.ratio > 1.2)):
        for sign, sel in (("+", res.adv_norm > 0), ("-", res.adv_norm < 0)):
            share = float((bound & sel).mean())
            assert share > 0.05, "ratio clip %s, advantage %s: only %.3g of the rows" % (side, sign, share)
    assert 0.2 < float(res.active.mean()) < 0.9       # ... rows whose surrogate is cut off, and rows whose is not
    r, s = check_update(name + " (norm clip active)", ref.named_grads(ns.policy), stats, want, twin)
    print("%s: clip active: gradient %.3g, statistics %.3g twin errors; pre-clip norm %.3g" % (name, r, s, want.norms[0]))
    near = returns_near_the_critic(ro)
    ns, stats, want, twin, shard, P = single_minibatch(ro, ro.gae.adv, near)
    assert want.norms[0] < 0.8 * ro.hp["max_grad_norm"], want.norms        # ... and idle here
    r, s = check_update(name + " (norm clip idle)", ref.named_grads(ns.policy), stats, want, twin)
    print("%s: clip idle: gradient %.3g, statistics %.3g twin errors; norm %.3g" % (name, r, s, want.norms[0]))


@pytest.mark.parametrize("name", list(CASES))
def test_two_epochs_of_three_minibatches_with_a_ragged_tail(name):
    from tennisbot_rl_amd.ppo import PPOTrainer
    import torch
    ro = rollout(name)
    N = ro.T * ro.n
    assert N % ro.batch and N // ro.batch == 2 and N % ro.batch < ro.batch // 5     # two full minibatches and a much smaller tail
    for tag, returns in (("clip active", ro.gae.returns), ("clip idle", returns_near_the_critic(ro))):
        ns = stand_in(ro, n_epochs=2, batch_size=ro.batch)
        P0 = state_dict_arrays(ns.policy)
        perms = ref.record_permutations(torch, 77, N, 2)
        stats = PPOTrainer.update(ns, torch.from_numpy(np.asarray(ro.gae.adv, np.float32)), torch.from_numpy(np.asarray(returns, np.float32)))
        shard = flat_shard(ro, ro.gae.adv, returns)
        want = ref.replay_update(P0, [shard], [perms], ro.batch, ns.hp)
        twin = ref.replay_update(P0, [shard], [perms], ro.batch, ns.hp, np.float32)
        assert len(want.norms) == 6 and (min(want.norms) > 0.5 if tag == "clip active" else max(want.norms) < 0.5), want.norms
        lr = ns.hp["learning_rate"]
        d_want, d_twin, d_got = ref.param_change(want.params, P0, lr), ref.param_change(twin.params, P0, lr), ref.param_change(ref.named_params(ns.policy), P0, lr)
        assert min(np.abs(v).max() for v in d_want.values()) > 1.0      # six Adam steps moved every tensor by more than one learning rate
        r = note("parameter change error / twin error", ref.check_tensors("%s %s parameters" % (name, tag), d_got, d_want, d_twin, MULTIPLE))
        note("twin parameter change error, in learning rates", max(np.abs(d_twin[k] - d_want[k]).max() for k in d_want))
        g = note("gradient error / twin error", ref.check_tensors("%s %s last gradient" % (name, tag), ref.named_grads(ns.policy), want.grads, twin.grads, MULTIPLE))
        s = note("statistics error / twin error", ref.check_tensors("%s %s statistics" % (name, tag), {k: np.float64(v) for k, v in stats.items()}, want.stats[0], twin.stats[0], MULTIPLE))
        print("%s %s: parameters %.3g, last gradient %.3g, statistics %.3g twin errors" % (name, tag, r, g, s))


# ------------------------------------------------------------------------------------------------- wrong learners are rejected
def torch_learner(ro, adv, returns, wrong=None, shards=1):
    """A learner written with autograd, one minibatch per rank, with one deliberate mistake (`wrong`); None: the rule itself.
    Returns the gradient every rank would hold before the optimiser step."""
    import torch
    policy = make_policy(ro.arch, ro.kind)
    hp = ro.hp
    obs, act, old_lp, adv, returns = (torch.from_numpy(np.ascontiguousarray(x)) for x in flat_shard(ro, adv, returns))
    if wrong == "clipped actions":
        act = act.clamp(-1.0, 1.0)
    if wrong == "whole-batch normalisation":
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    per_rank = []
    for idx in torch.arange(adv.numel()).chunk(shards):
        a = adv[idx]
        if wrong != "whole-batch normalisation":
            a = (a - a.mean()) / (a.std(unbiased=wrong != "biased std") + 1e-8)
        value, logp, entropy = policy.evaluate(obs[idx], act[idx])
        ratio = (logp - old_lp[idx]).exp()
        pg = -torch.min(a * ratio, a * ratio.clamp(1 - hp["clip_range"], 1 + hp["clip_range"])).mean()
        vl = ((returns[idx] - value) ** 2).mean()
        if wrong == "vf_coef on the policy term":
            loss = hp["vf_coef"] * pg + vl - hp["ent_coef"] * entropy
        else:
            loss = pg + hp["vf_coef"] * vl + (hp["ent_coef"] if wrong == "entropy sign" else -hp["ent_coef"]) * entropy
        policy.zero_grad(set_to_none=True)
        loss.backward()
        if wrong == "clip before averaging":
            torch.nn.utils.clip_grad_norm_(policy.parameters(), hp["max_grad_norm"])
        per_rank.append([p.grad.clone() for p in policy.parameters()])
    for p, *gs in zip(policy.parameters(), *per_rank):
        p.grad = sum(gs) / len(gs)
    torch.nn.utils.clip_grad_norm_(policy.parameters(), hp["max_grad_norm"])
    return ref.named_grads(policy)


def test_the_checker_rejects_wrong_learners():
    """each mistake of the list, made on purpose: the comparison that passes the rule itself flags it"""
    from tennisbot_rl_amd.ppo import PPOTrainer
    import torch
    name = "swing-70-midepisode"
    ro = rollout(name)
    # GAE mistakes, made through the product's own inputs: dones shifted by one step, last_value zeroed
    ns = stand_in(ro)
    ns.buf.dones.copy_(torch.from_numpy(np.concatenate([ro.dones[1:], ro.dones[:1]])))
    adv, returns = PPOTrainer.advantages(ns, torch.from_numpy(ro.last_value))
    assert excess(adv.numpy(), ro.gae.adv, ro.gae.adv_bound)[0] > 1e3
    adv, returns = PPOTrainer.advantages(stand_in(ro), torch.zeros(ro.n))
    assert excess(adv.numpy(), ro.gae.adv, ro.gae.adv_bound)[0] > 1e3 and excess(returns.numpy(), ro.gae.returns, ro.gae.returns_bound)[0] > 1e3
    # minibatch mistakes. Two settings: returns near the critic (norm clip idle: nothing rescales the gradient) and the rollout's own
    near = returns_near_the_critic(ro)
    N = ro.T * ro.n
    P = state_dict_arrays(make_policy(ro.arch, ro.kind))
    for returns, world in ((near, 1), (ro.gae.returns, 1), (ro.gae.returns, 2)):
        shard = flat_shard(ro, ro.gae.adv, returns)
        halves = [tuple(x[i * (N // world):(i + 1) * (N // world)] for x in shard) for i in range(world)]
        perms = [[np.arange(N // world)]] * world
        want, twin = ref.replay_update(P, halves, perms, N, ro.hp), ref.replay_update(P, halves, perms, N, ro.hp, np.float32)
        right = ref.tensor_ratios(torch_learner(ro, ro.gae.adv, returns, None, world), want.grads, twin.grads)
        assert max(right.values()) <= MULTIPLE, right       # the rule itself, written with autograd, passes
        wrongs = ["clipped actions", "biased std", "entropy sign", "vf_coef on the policy term"] if world == 1 else \
            ["clip before averaging", "whole-batch normalisation"]
        for wrong in wrongs:
            ratios = ref.tensor_ratios(torch_learner(ro, ro.gae.adv, returns, wrong, world), want.grads, twin.grads)
            worst = max(ratios.values())
            print("%-28s world %d, norm %.3g: %.3g twin errors" % (wrong, world, want.norms[0], worst))
            with pytest.raises(AssertionError):
                ref.check_tensors(wrong, torch_learner(ro, ro.gae.adv, returns, wrong, world), want.grads, twin.grads, MULTIPLE)
            RATIOS["(smallest) wrong learner's error / twin error"] = min(worst, RATIOS.get("(smallest) wrong learner's error / twin error", np.inf))


# ------------------------------------------------------------------------------------------------------------ two gloo ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_shard(ro, rank):
    """rank r's envs: [r n/2, (r + 1) n/2) of the rollout, with its own GAE"""
    n2 = ro.n // WORLD
    sl = slice(rank * n2, (rank + 1) * n2)
    sub = types.SimpleNamespace(**vars(ro))
    for k in ("dones", "rewards", "obs", "raw", "old_logp", "values", "v_pred"):
        setattr(sub, k, np.ascontiguousarray(getattr(ro, k)[:, sl]))
    sub.last_value, sub.n = ro.last_value[sl].copy(), n2
    sub.gae = ref.gae(sub.rewards, sub.values, sub.dones, sub.last_value, ro.hp["gamma"], ro.hp["gae_lambda"])
    return sub


def _rank_worker(rank, port, name, out_dir):
    import torch
    import torch.distributed as dist
    from tennisbot_rl_amd.ppo import PPOTrainer
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    sub = _rank_shard(make_rollout(name), rank)
    for mode in ("active", "idle"):
        ns = stand_in(sub, world=WORLD, n_epochs=1)
        adv, returns = PPOTrainer.advantages(ns, torch.from_numpy(sub.last_value))
        if mode == "idle":
            returns = torch.from_numpy(returns_near_the_critic(sub))
        stats = PPOTrainer.update(ns, adv, returns)
        out = {"grad." + k: v for k, v in ref.named_grads(ns.policy).items()}
        out.update({"param." + k: v for k, v in ref.named_params(ns.policy).items()})
        out.update({"stat." + k: np.float64(v) for k, v in stats.items()})
        np.savez(os.path.join(out_dir, "rank%d_%s.npz" % (rank, mode)), adv=adv.numpy(), returns=returns.numpy(), **out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_average_then_clip():
    """two ranks with different shards: both hold the reference's clipped mean of the two shard gradients (each normalised
    within its own minibatch) and end with identical parameters. Once with the norm clip active -- clipping each rank's gradient
    before the average would show -- and once with it idle: there a sum in place of the mean shows, which the clip would hide."""
    import tempfile
    import torch.multiprocessing as mp
    name = "tennis-52-ragged"
    ro = rollout(name)
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_rank_worker, args=(_free_port(), name, tmp), nprocs=WORLD, join=True)
        results = {mode: [dict(np.load(os.path.join(tmp, "rank%d_%s.npz" % (r, mode)))) for r in range(WORLD)] for mode in ("active", "idle")}
    subs = [_rank_shard(ro, r) for r in range(WORLD)]
    n2 = ro.T * ro.n // WORLD
    perms = [[np.arange(n2)]] * WORLD
    P = state_dict_arrays(make_policy(ro.arch, ro.kind))
    lr = ro.hp["learning_rate"]
    for mode, got in results.items():
        if mode == "active":
            for r in range(WORLD):
                check_gae("rank %d" % r, got[r]["adv"], got[r]["returns"], subs[r].gae)
        # the reference takes the ranks' own float32 advantages and returns, as update did
        shards = [flat_shard(subs[r], got[r]["adv"], got[r]["returns"]) for r in range(WORLD)]
        want, twin = ref.replay_update(P, shards, perms, n2, ro.hp), ref.replay_update(P, shards, perms, n2, ro.hp, np.float32)
        if mode == "active":
            assert want.norms[0] > 2 * ro.hp["max_grad_norm"]
        else:
            assert want.norms[0] < 0.8 * ro.hp["max_grad_norm"]
        alone = ref.replay_update(P, shards[:1], perms[:1], n2, ro.hp)
        assert max(ref.tensor_ratios(alone.grads, want.grads, twin.grads).values()) > 100 * MULTIPLE    # the other rank's shard matters
        for r in range(WORLD):
            grads = {k[5:]: v for k, v in got[r].items() if k.startswith("grad.")}
            note("two-rank gradient error / twin error", ref.check_tensors("rank %d gradient, clip %s" % (r, mode), grads, want.grads, twin.grads, MULTIPLE))
            stats = {k[5:]: v for k, v in got[r].items() if k.startswith("stat.")}
            note("statistics error / twin error", ref.check_tensors("rank %d statistics" % r, stats, want.stats[r], twin.stats[r], MULTIPLE))
        for k in got[0]:
            if k.startswith(("grad.", "param.")):
                assert np.array_equal(got[0][k], got[1][k]), k
        params = {k[6:]: v for k, v in got[0].items() if k.startswith("param.")}
        ref.check_tensors("two-rank parameters", ref.param_change(params, P, lr), ref.param_change(want.params, P, lr), ref.param_change(twin.params, P, lr), MULTIPLE)
