"""The fused learner through a real PPOTrainer(learner="fused"), held to the float64 reference exactly as the torch learner is in
tests/test_gpu_ppo_reference.py (same helpers, shapes and tolerances): SwingRacket-v0 with 512 envs x 52 steps after the eager
collect and after a replayed graph (terminal rewards written late by the fast-forward), Tennisbot-v0 with 64 envs x 900 steps;
then a checkpoint handed to a fresh trainer."""
import numpy as np
import pytest

import ppo_reference as ref
from test_gpu_ppo_reference import check_learn_repacks, check_learner

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def fused_trainer(env_id, **kw):
    from tennisbot_rl_amd.learner import FusedLearner
    from tennisbot_rl_amd.ppo import PPOTrainer
    tr = PPOTrainer(env_id, device="cuda:0", n_epochs=2, learner="fused", **kw)
    assert isinstance(tr._learner, FusedLearner) and tr.fused
    flat = tr.policy._flat_params
    assert flat.numel() == tr._learner.n_params == sum(p.numel() for p in tr.policy.parameters())
    return tr


def test_swing_52_eager_and_replayed_then_a_checkpoint(torch, tmp_path):
    tr = fused_trainer("SwingRacket-v0", num_envs=512, n_steps=52, seed=3)
    assert tr.env.pipeline and tr.use_graph and tr.rollout_launch
    tr.collect()
    assert tr._graph is not None
    g = tr._graph
    dones, want = check_learner(torch, tr, "fused swing 52 eager")
    assert np.array_equal(np.flatnonzero(dones.any(1)), [25, 51]) and dones[[25, 51]].all()
    tr.collect()
    tr.collect()
    assert tr._graph is g, "the later collects did not replay the captured graph"
    dones, want = check_learner(torch, tr, "fused swing 52 replayed")
    rew = tr.buf.rewards.cpu().numpy()
    assert dones[[25, 51]].all() and (rew[[25, 51]] != 0).any()     # the terminal rewards, written by the fast-forward after the step kernels, are in
    assert np.abs(want.adv).max() > 1.0
    check_learn_repacks(torch, tr)
    # save -> a fresh trainer -> load -> one more update from the same recorded permutation: the same bits on both
    path = str(tmp_path / "fused.pt")
    tr.save(path)
    other = fused_trainer("SwingRacket-v0", num_envs=512, n_steps=52, seed=99).load(path)
    assert all(torch.equal(a, b) for a, b in zip(tr.policy.parameters(), other.policy.parameters()))
    N = tr.n_steps * tr.num_envs
    for x in ("obs_seq", "_raw_actions", "logps", "values", "last_value"):     # the rollout the update learns from
        getattr(other, x).copy_(getattr(tr, x))
    other.buf.raw.copy_(tr.buf.raw)
    ends = []
    for t in (tr, other):
        adv, returns = t.advantages(t.last_value)
        ref.record_permutations(torch, 31, N, 2, t.device)
        stats = t.update(adv, returns)
        torch.cuda.synchronize()
        ends.append((t.policy._flat_params.clone(), t._learner.grad.clone(), t._learner.exp_avg.clone(), t._learner.exp_avg_sq.clone(), stats,
                     {int(t.opt.state[p]["step"]) for p in t.policy.parameters()}))
    for a, b in zip(ends[0][:4], ends[1][:4]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert ends[0][4] == ends[1][4] and ends[0][5] == ends[1][5] and len(ends[0][5]) == 1
    for t in (tr, other):
        c = t.env.counters()
        assert c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0, c
        t.env.close()


def test_tennis_900_ragged_episode_ends(torch):
    tr = fused_trainer("Tennisbot-v0", num_envs=64, n_steps=900, seed=5)
    tr.collect()
    dones, want = check_learner(torch, tr, "fused tennis 900")
    ends = np.flatnonzero(dones.any(1))
    assert dones.sum() >= 32 and ends.size >= 8, (int(dones.sum()), ends)     # episodes ended, and at ragged times
    check_learn_repacks(torch, tr)
    c = tr.env.counters()
    assert c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0, c
    tr.env.close()
