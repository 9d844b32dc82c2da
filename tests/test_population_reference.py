"""PopulationPPO's pure parts on the CPU: the batched gather against pack_policy, the batched value forward against float64,
pbt_exploit, and the scripts' flags."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import population_fixtures as fx  # noqa: E402
import ppo_reference as ref  # noqa: E402
from tennisbot_rl_amd.population import members_value, pack_members, pbt_exploit, policy_flat, population_keywords  # noqa: E402


@pytest.mark.parametrize("kind,net", fx.PAIRS)
def test_row_m_of_the_batched_gather_is_pack_policy_of_member_m(kind, net):
    from tennisbot_rl_amd.policy_es import build_policy
    from tennisbot_rl_amd.ppo import pack_policy
    policies = fx.member_policies(torch, kind, net)[:3]
    flat = torch.stack([policy_flat(p) for p in policies])
    assert not torch.equal(flat[0], flat[1]) and not torch.equal(flat[1], flat[2])
    template = build_policy(kind, net, seed=0)           # names the architecture only: its own weights are none of the members'
    blobs = pack_members(template, flat)
    out = torch.full_like(blobs, float("nan"))
    pack_members(template, flat, out=out)
    for m, p in enumerate(policies):
        want = pack_policy(copy.deepcopy(p))
        assert blobs.shape[1] == want.numel()
        assert np.array_equal(blobs[m].numpy().view(np.uint32), want.numpy().view(np.uint32)), m
        assert np.array_equal(out[m].numpy().view(np.uint32), want.numpy().view(np.uint32)), m


@pytest.mark.parametrize("kind,net", fx.PAIRS)
def test_members_value_is_a_float32_twin_of_the_modules_value(kind, net):
    """against a float64 evaluation of the same parameters, members_value may err ppo_reference.MULTIPLE (24) times what the
    member's own float32 module errs: the project's allowance for a float32 twin with another summation order"""
    from tennisbot_rl_amd.policy_es import build_policy
    policies = [copy.deepcopy(p) for p in fx.member_policies(torch, kind, net)[:3]]
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():   # (the fixture's members share one value tower: give each its own)
        for p in policies:
            for name, t in p.named_parameters():
                if name.startswith(("value_net", "features_extractor")):
                    t.add_(0.05 * torch.randn(t.shape, generator=g))
    R = 64
    obs = torch.from_numpy(fx.golden_observations(kind, 3 * R)).view(3, R, -1)
    flat = torch.stack([policy_flat(p) for p in policies])
    got = members_value(build_policy(kind, net, seed=0), flat, obs)
    assert got.shape == (3, R) and got.dtype == torch.float32
    with torch.no_grad():
        for m, p in enumerate(policies):
            want = copy.deepcopy(p).double()(obs[m].double())[1]
            own = (p(obs[m])[1].double() - want).abs().max().item()
            err = (got[m].double() - want).abs().max().item()
            print("kind=%d net=%d member %d: members_value err %.3g, the module's own %.3g" % (kind, net, m, err, own))
            assert own > 0.0 and err <= ref.MULTIPLE * own, (m, err, own)
    # the members differ: row 1 under member 0's parameters is another function
    assert not torch.equal(members_value(build_policy(kind, net, seed=0), flat[[0, 0, 0]], obs)[1], got[1])


def population_tensors(M, P=5):
    flat = torch.arange(M * P, dtype=torch.float32).view(M, P)
    return flat, flat + 1000.0, flat + 2000.0, torch.tensor([[0.2, 0.5, 0.01 * (m + 1), 1e-4 * (m + 1)] for m in range(M)], dtype=torch.float32)


def test_pbt_exploit_who_copies_from_whom_nan_ranks_worst_and_the_moments_travel():
    M = 8
    flat, m1, m2, hp = population_tensors(M)
    before = [x.clone() for x in (flat, m1, m2, hp)]
    scores = torch.tensor([3.0, float("nan"), 9.0, 1.0, 5.0, 7.0, 2.0, 4.0])
    g = torch.Generator().manual_seed(11)
    twin = torch.Generator().manual_seed(11)
    global_state = torch.get_rng_state().clone()
    pairs = pbt_exploit(scores, flat, m1, m2, hp, g, frac=0.25, factors=(0.8, 1.25))
    assert torch.equal(torch.get_rng_state(), global_state), "pbt_exploit drew from the global RNG"
    assert pairs == [(1, 2), (3, 5)]            # the NaN member is the worst and copies the best; the next worst the second best
    draws = torch.randint(2, (2, 2), generator=twin).tolist()   # the factors come from the given generator, and from it alone
    assert torch.equal(g.get_state(), twin.get_state())
    for j, (lo, hi) in enumerate(pairs):
        for x, x0 in zip((flat, m1, m2), before):
            assert torch.equal(x[lo], x0[hi])
        assert hp[lo, 0] == before[3][hi, 0] and hp[lo, 1] == before[3][hi, 1]      # clip_range, vf_coef: copied unchanged
        f = (0.8, 1.25)
        assert hp[lo, 3] == before[3][hi, 3] * f[draws[j][0]] and hp[lo, 2] == before[3][hi, 2] * f[draws[j][1]]
    for m in set(range(M)) - {1, 3}:
        for x, x0 in zip((flat, m1, m2, hp), before):
            assert torch.equal(x[m], x0[m])


def test_pbt_exploit_is_a_no_op_for_three_members():
    flat, m1, m2, hp = population_tensors(3)
    before = [x.clone() for x in (flat, m1, m2, hp)]
    g = torch.Generator().manual_seed(3)
    state = g.get_state().clone()
    assert pbt_exploit(torch.tensor([1.0, 2.0, 3.0]), flat, m1, m2, hp, g, frac=0.25) == []
    assert all(torch.equal(x, x0) for x, x0 in zip((flat, m1, m2, hp), before)) and torch.equal(g.get_state(), state)


def swing_args(argv):
    import train_swing
    return train_swing.parse_args(argv)


def test_flags_lists_of_length_1_or_m():
    kw = swing_args(["--population", "4", "--num-envs", "256", "--member-lr", "1e-4,3e-4,1e-3,3e-3", "--member-ent-coef", "0.002", "--pbt-every", "3"]).population_keywords
    assert kw == dict(members=4, envs_per_member=64, member_hp={"lr": [1e-4, 3e-4, 1e-3, 3e-3], "ent_coef": [0.002]}, pbt_every=3)
    assert swing_args([]).population_keywords is None and swing_args(["-s", "trpo"]).population_keywords is None
    with pytest.raises(SystemExit, match="1 or 4 values"):
        swing_args(["--population", "4", "--num-envs", "256", "--member-clip-range", "0.1,0.2"])
    with pytest.raises(SystemExit, match="belong to --population"):
        swing_args(["--member-lr", "1e-3"])


def test_flags_the_granule_and_the_other_learners():
    with pytest.raises(SystemExit, match="multiple of the member granule 16"):
        swing_args(["--population", "3", "--num-envs", "100"])
    with pytest.raises(SystemExit, match="multiple of the member granule 16"):
        swing_args(["--population", "4", "--num-envs", "96"])      # 24 envs per member
    with pytest.raises(SystemExit, match="not -s trpo"):
        swing_args(["--population", "4", "--num-envs", "256", "-s", "trpo"])
    import train
    with pytest.raises(SystemExit, match="multiple of the member granule 16"):
        train.main(["-s", "tuned_ppo", "--population", "4", "--num-envs", "72"])
    import argparse
    ns = argparse.Namespace(population=2, num_envs=64, member_lr=None, member_ent_coef=None, member_clip_range="0.1,0.3", pbt_every=0)
    assert population_keywords(ns, "tuned_ppo") == dict(members=2, envs_per_member=32, member_hp={"clip_range": [0.1, 0.3]}, pbt_every=0)
    with pytest.raises(ValueError, match="not -s sac"):
        population_keywords(ns, "sac")
