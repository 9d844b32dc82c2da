"""The PPO learner on the device against the float64 reference of tests/ppo_reference.py: a real PPOTrainer for both env ids,
its buffers read back after a collect, then

  * the on-device advantages / returns against `gae`, every element within the reference's a-priori bound;
  * one single-minibatch update's p.grad (the averaged, clipped gradient) and statistics against `loss_and_grads`;
  * a 2-epoch x 3-minibatch update (ragged tail, recorded permutations, the optimiser's moments as they stand) against
    `replay_update`, as (p - p0) / lr;
  * after learn() for one more rollout, that the blob the kernels read is the updated module's.

SwingRacket with n_steps = 52 is the default form (pipelined, one hipGraph, whole episodes per launch): the first, eager collect
and a replayed one, whose terminal rewards the fast-forward wrote late. n_steps = 70 is issued eagerly and starts mid-episode.
Tennisbot runs 900 steps: episodes end at ragged times. Tolerances: see tests/test_ppo_reference.py; the figures measured on an
MI355X are in its docstring and in DESIGN.md ("The learner's reference")."""
import copy

import numpy as np
import pytest

import ppo_reference as ref
from policy_reference import assert_within, state_dict_arrays

pytestmark = pytest.mark.gpu

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
        print("ppo reference (gpu): largest %s = %.3g" % (k, RATIOS[k]))


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def check_learner(torch, tr, tag):
    """the collect that has just run: GAE, a single-minibatch gradient (undone afterwards), a ragged multi-epoch update (kept)"""
    torch.cuda.synchronize()
    h = lambda x: x.detach().cpu().numpy().copy()  # noqa: E731
    T, n = tr.n_steps, tr.num_envs
    N = T * n
    dones = h(tr.buf.dones)
    want = ref.gae(h(tr.buf.rewards), h(tr.values), dones, h(tr.last_value), tr.hp["gamma"], tr.hp["gae_lambda"])
    adv, returns = tr.advantages(tr.last_value)
    r = max(assert_within(tag + " advantages", h(adv), want.adv, want.adv_bound), assert_within(tag + " returns", h(returns), want.returns, want.returns_bound))
    note("GAE |error| / bound", r)
    shard = (h(tr.obs_seq).reshape(N, -1), h(tr._raw_actions).reshape(N, -1), h(tr.logps).reshape(N), h(adv).reshape(N), h(returns).reshape(N))
    lr = tr.hp["learning_rate"]
    saved = copy.deepcopy(tr.policy.state_dict()), copy.deepcopy(tr.opt.state_dict()), tr.hp["n_epochs"], tr.batch_size
    P0, adam0 = state_dict_arrays(tr.policy), ref.adam_state_of(tr.policy, tr.opt)
    try:
        # one epoch, one minibatch
        tr.hp["n_epochs"], tr.batch_size = 1, N
        stats = tr.update(adv, returns)
        perms = [[np.arange(N)]]
        w1 = ref.replay_update(P0, [shard], perms, N, tr.hp, adam_state=ref.copy_state(adam0))
        t1 = ref.replay_update(P0, [shard], perms, N, tr.hp, np.float32, adam_state=ref.copy_state(adam0))
        g = note("gradient error / twin error", ref.check_tensors(tag + " gradient", ref.named_grads(tr.policy), w1.grads, t1.grads, ref.MULTIPLE))
        s = note("statistics error / twin error", ref.check_tensors(tag + " statistics", {k: np.float64(v) for k, v in stats.items()}, w1.stats[0], t1.stats[0], ref.MULTIPLE))
        note("twin gradient error, absolute", max(np.abs(np.asarray(t1.grads[k], np.float64) - w1.grads[k]).max() for k in w1.grads))
        tr.policy.load_state_dict(saved[0]); tr.opt.load_state_dict(saved[1])
        # two epochs of two full minibatches and a tail of about N / 40 rows
        batch = (N - N // 40 + 1) // 2
        assert 0 < N - 2 * batch < batch // 10
        tr.hp["n_epochs"], tr.batch_size = 2, batch
        perms = ref.record_permutations(torch, 4242, N, 2, tr.device)
        tr.update(adv, returns)
        w2 = ref.replay_update(P0, [shard], [perms], batch, tr.hp, adam_state=ref.copy_state(adam0))
        t2 = ref.replay_update(P0, [shard], [perms], batch, tr.hp, np.float32, adam_state=ref.copy_state(adam0))
        d_want, d_twin, d_got = ref.param_change(w2.params, P0, lr), ref.param_change(t2.params, P0, lr), ref.param_change(ref.named_params(tr.policy), P0, lr)
        moved = [np.abs(v).max() for v in d_want.values()]
        assert max(moved) > 1.0 and min(moved) > 0.0                   # the six Adam steps moved every tensor, some by more than a learning rate
        p = note("parameter change error / twin error", ref.check_tensors(tag + " parameters", d_got, d_want, d_twin, ref.MULTIPLE))
        note("twin parameter change error, in learning rates", max(np.abs(d_twin[k] - d_want[k]).max() for k in d_want))
    finally:
        tr.hp["n_epochs"], tr.batch_size = saved[2], saved[3]
    print("%s: GAE %.3g of its bound; gradient %.3g, statistics %.3g, parameters %.3g twin errors; pre-clip norms %.3g / %s"
          % (tag, r, g, s, p, w1.norms[0], " ".join("%.3g" % x for x in w2.norms)))
    return dones, want


def check_learn_repacks(torch, tr):
    """learn() for one more rollout: its collect hands the kernels the module as the update above left it"""
    from tennisbot_rl_amd.ppo import pack_policy
    before = tr.packed.clone()
    updated = pack_policy(tr.policy)
    assert not torch.equal(updated, before)            # the update moved the weights the last collect ran with
    hist = tr.learn(tr.num_timesteps + tr.n_steps * tr.num_envs, log=None)
    torch.cuda.synchronize()
    assert len(hist) == 1 and all(np.isfinite(hist[0][k]) for k in ("policy_loss", "value_loss", "entropy"))
    assert torch.equal(tr.packed, updated), "the rollout kernels did not read the updated module"
    assert not torch.equal(pack_policy(tr.policy), updated)   # ... and learn's own update moved on from there


def test_swing_52_default_form_eager_and_replayed(torch):
    from tennisbot_rl_amd.ppo import PPOTrainer
    tr = PPOTrainer("SwingRacket-v0", num_envs=512, n_steps=52, device="cuda:0", seed=3, n_epochs=2)
    assert tr.env.pipeline and tr.use_graph and tr.rollout_launch and tr.fused
    tr.collect()
    assert tr._graph is not None
    g = tr._graph
    dones, want = check_learner(torch, tr, "swing 52 eager")
    assert np.array_equal(np.flatnonzero(dones.any(1)), [25, 51]) and dones[[25, 51]].all()
    tr.collect()
    tr.collect()
    assert tr._graph is g, "the later collects did not replay the captured graph"
    dones, want = check_learner(torch, tr, "swing 52 replayed")
    assert dones[[25, 51]].all()
    rew = tr.buf.rewards.cpu().numpy()
    assert (rew[[25, 51]] != 0).any()             # the terminal rewards, written by the fast-forward after the step kernels, are in
    assert np.abs(want.adv).max() > 1.0
    check_learn_repacks(torch, tr)
    c = tr.env.counters()
    assert c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0, c
    tr.env.close()


def test_swing_70_eager_from_mid_episode(torch):
    from tennisbot_rl_amd.ppo import PPOTrainer
    tr = PPOTrainer("SwingRacket-v0", num_envs=512, n_steps=70, device="cuda:0", seed=4, n_epochs=2)
    assert not tr.use_graph                          # 70 is no whole number of 26-step episodes: issued eagerly
    for _ in range(5):                               # a few stray steps: the rollout starts at phase 5
        obs, _, _ = tr.env.step(torch.zeros((512, 6), device=tr.device))
    tr.env.flush()
    tr.obs_in.copy_(obs)
    assert tr.env.phase() == 5
    tr.collect()
    dones, _ = check_learner(torch, tr, "swing 70 mid-episode")
    assert np.array_equal(np.flatnonzero(dones.any(1)), [20, 46]) and dones[[20, 46]].all()
    tr.collect()                                     # the next rollout starts at phase 23
    dones, _ = check_learner(torch, tr, "swing 70 second rollout")
    assert np.array_equal(np.flatnonzero(dones.any(1)), [2, 28, 54])
    assert tr._graph is None
    check_learn_repacks(torch, tr)
    tr.env.close()


def test_tennis_900_ragged_episode_ends(torch):
    from tennisbot_rl_amd.ppo import PPOTrainer
    tr = PPOTrainer("Tennisbot-v0", num_envs=64, n_steps=900, device="cuda:0", seed=5, n_epochs=2)
    tr.collect()
    dones, want = check_learner(torch, tr, "tennis 900")
    ends = np.flatnonzero(dones.any(1))
    assert dones.sum() >= 32 and ends.size >= 8, (int(dones.sum()), ends)     # episodes ended, and at ragged times
    assert (dones.sum(0) == 0).any() or dones.sum(0).max() >= 2 or ends.size >= 8
    check_learn_repacks(torch, tr)
    tr.env.close()
