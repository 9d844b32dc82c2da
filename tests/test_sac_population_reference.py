"""The SAC / TQC population's pure functions (tennisbot_rl_amd/sac_population.py) without a GPU: sample_member_indices keeps every
member inside its own columns of the shared ring and draws from its generator alone; members_sample is a float32 twin of each
member's own Actor.sample; pbt_exploit_sac copies the right rows bit for bit and perturbs the learning rates only; a member's
checkpoint round-trips through the state dicts SACTrainer.load / TQCTrainer.load read; run_population picks the best member among
those that have a score and keeps the earlier one when nobody has."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ppo_reference as ref  # noqa: E402
from tennisbot_rl_amd import sac_population as sp  # noqa: E402
from tennisbot_rl_amd.params import ENV_SWING, ENV_TENNIS  # noqa: E402

DIMS = {ENV_SWING: (6, 6), ENV_TENNIS: (12, 2)}


def bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.uint32 if x.dtype == torch.float32 else np.uint64)


# ------------------------------------------------------------------------------------------------------ sample_member_indices
@pytest.mark.parametrize("filled,what", [(5, "a part-filled ring: 5 of 8 slots"), (8, "a full, wrapped ring")])
def test_member_indices_stay_in_the_members_columns_of_filled_slots(filled, what):
    M, R, G, B = 3, 16, 4, 257
    N = M * R
    gen = torch.Generator().manual_seed(11)
    state = gen.get_state()
    global_before = torch.get_rng_state()
    idx = sp.sample_member_indices(gen, M, R, filled, G, B)
    assert torch.equal(torch.get_rng_state(), global_before), "torch's global RNG was drawn from"
    assert idx.shape == (G, M, B) and idx.dtype == torch.int64 and idx.is_contiguous()
    slot, col = idx // N, idx % N
    assert int(slot.min()) >= 0 and int(slot.max()) < filled, what
    sets = []
    for m in range(M):
        assert int(col[:, m].min()) >= m * R and int(col[:, m].max()) < (m + 1) * R, (what, m)
        sets.append(set(idx[:, m].reshape(-1).tolist()))
        assert len(set((col[:, m] - m * R).reshape(-1).tolist())) == R and len(set(slot[:, m].reshape(-1).tolist())) == filled   # (every column and slot is reachable)
    assert not (sets[0] & sets[1]) and not (sets[0] & sets[2]) and not (sets[1] & sets[2])
    gen.set_state(state)
    assert torch.equal(sp.sample_member_indices(gen, M, R, filled, G, B), idx), "the same generator state must give the same tensor"
    assert not torch.equal(sp.sample_member_indices(gen, M, R, filled, G, B), idx)   # (and the state has moved on)


def test_member_indices_refuse_an_empty_ring():
    with pytest.raises(ValueError):
        sp.sample_member_indices(torch.Generator(), 3, 16, 0, 1, 4)


# -------------------------------------------------------------------------------------------------------------- members_sample
def member_actors(kind, M=3):
    from tennisbot_rl_amd.sac import build_sac_modules
    O, A = DIMS[kind]
    actors = []
    with torch.random.fork_rng(devices=[]):
        for m in range(M):
            torch.manual_seed(40 + 10 * kind + m)
            actor = build_sac_modules(O, A)[0]
            with torch.no_grad():   # (log_std away from 0, and different per member)
                actor.log_std.bias.copy_(torch.linspace(-0.6, 0.1, A) - 0.1 * m)
            actors.append(actor)
    return actors


@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
def test_members_sample_is_a_float32_twin_of_each_members_own_sample(kind):
    """against a float64 evaluation of the same parameters, members_sample may err ppo_reference.MULTIPLE (24) times what the
    member's own float32 module errs, per tensor in the max norm: the rule tests/test_population_reference.py holds members_value to"""
    import copy
    O, A = DIMS[kind]
    M, R = 3, 16
    actors = member_actors(kind, M)
    g = torch.Generator().manual_seed(5 + kind)
    obs, eps = 3.0 * torch.randn((M, R, O), generator=g), torch.randn((M, R, A), generator=g).clamp(-2.5, 2.5)
    flat = torch.stack([torch.cat([p.detach().reshape(-1) for _, p in a.named_parameters()]) for a in actors])
    padded = torch.full((M, flat.shape[1] + 4), math.nan)
    padded[:, :flat.shape[1]] = flat
    act, logp = sp.members_sample(padded[:, :flat.shape[1]], obs, eps)   # rows of wider storage: the padding is never read
    assert act.shape == (M, R, A) and logp.shape == (M, R) and act.dtype == logp.dtype == torch.float32
    assert tuple(sp.actor_offsets(O, A)) == sp.ACTOR_NAMES and sum(math.prod(s) for _, s in sp.actor_offsets(O, A).values()) == flat.shape[1]
    with torch.no_grad():
        for m, a in enumerate(actors):
            want_a, want_lp = copy.deepcopy(a).double().sample(obs[m].double(), eps[m].double())
            own_a, own_lp = a.sample(obs[m], eps[m])
            for name, got, own, want in (("action", act[m], own_a, want_a), ("logp", logp[m], own_lp, want_lp)):
                own_err, err = (own.double() - want).abs().max().item(), (got.double() - want).abs().max().item()
                print("kind=%d member %d %s: members_sample err %.3g, the module's own %.3g" % (kind, m, name, err, own_err))
                assert own_err > 0.0 and err <= ref.MULTIPLE * own_err, (m, name, err, own_err)
    # the members differ: member 1's rows under member 0's parameters are another function
    assert not torch.equal(sp.members_sample(flat[[0, 0, 0]], obs, eps)[0][1], act[1])


# ------------------------------------------------------------------------------------------------------------- pbt_exploit_sac
def population_tensors(M):
    f = lambda base, n: base + torch.arange(M * n, dtype=torch.float32).view(M, n)  # noqa: E731
    vectors = tuple(f(1000.0 * k, n) for k, n in enumerate((7, 7, 7, 9, 9, 9, 9, 1, 1, 1)))   # pi, m, v, q, m, v, qt, ent, m, v
    hp = torch.tensor([[1e-4 * (m + 1), 2e-4 * (m + 1), 3e-4 * (m + 1), 0.9 + 0.01 * m, 0.001 * (m + 1), 0.0, 0.0, 0.0] for m in range(M)], dtype=torch.float32)
    return vectors, hp


def test_pbt_copies_the_best_onto_the_worst_and_perturbs_only_the_learning_rates():
    M = 8
    vectors, hp = population_tensors(M)
    before, hp_before = [v.clone() for v in vectors], hp.clone()
    scores = [3.0, math.nan, 9.0, -1.0, 5.0, 7.0, 0.5, 2.0]   # best: 2, 5; worst: 1 (NaN), then 3
    gen = torch.Generator().manual_seed(3)
    global_before = torch.get_rng_state()
    pairs = sp.pbt_exploit_sac(scores, vectors, hp, gen, frac=0.25, factors=(0.8, 1.25))
    assert torch.equal(torch.get_rng_state(), global_before)
    assert pairs == [(1, 2), (3, 5)]
    for lo, hi in pairs:
        for v, b in zip(vectors, before):
            assert np.array_equal(bits(v[lo]), bits(b[hi])), "a copied vector must be bit-equal to its source"
        assert np.array_equal(bits(hp[lo, 3:]), bits(hp_before[hi, 3:])), "gamma, tau and the padding are copied unchanged"
        ratio = (hp[lo, :3].double() / hp_before[hi, :3].double()).tolist()
        assert all(0.8 < r < 1.25 for r in ratio), ratio
        assert max(ratio) - min(ratio) < 1e-6, "one factor for the three learning rates"
    ratios = [float(hp[lo, 0].double() / hp_before[hi, 0].double()) for lo, hi in pairs]
    assert ratios[0] != ratios[1]   # (a draw per copy)
    for m in (0, 2, 4, 5, 6, 7):
        for v, b in zip(vectors, before):
            assert np.array_equal(bits(v[m]), bits(b[m])), "an untouched member must stay bit-identical"
        assert np.array_equal(bits(hp[m]), bits(hp_before[m]))


def test_pbt_does_nothing_and_draws_nothing_below_one_pair():
    vectors, hp = population_tensors(3)
    before, gen = [v.clone() for v in vectors], torch.Generator().manual_seed(3)
    state = gen.get_state()
    assert sp.pbt_exploit_sac([1.0, 2.0, 3.0], vectors, hp, gen, frac=0.25) == []
    assert torch.equal(gen.get_state(), state) and all(torch.equal(v, b) for v, b in zip(vectors, before))
    with pytest.raises(ValueError):
        sp.pbt_exploit_sac([1.0, 2.0], vectors, hp, gen, frac=0.5)


def test_member_hp_rows_and_the_scripts_flags():
    rows = sp.member_hp_rows(3, (3e-4, 3e-4, 3e-4, 0.99, 0.005), {"lr": [1e-4, 2e-4, 3e-4], "tau": 0.0, "gamma": [0.9]})
    assert [r[:5] for r in rows] == [[1e-4, 1e-4, 1e-4, 0.9, 0.0], [2e-4, 2e-4, 2e-4, 0.9, 0.0], [3e-4, 3e-4, 3e-4, 0.9, 0.0]] and all(len(r) == sp.HP_WIDTH for r in rows)
    with pytest.raises(ValueError):
        sp.member_hp_rows(3, (0, 0, 0, 0, 0), {"lr": [1.0, 2.0]})
    with pytest.raises(ValueError):
        sp.member_hp_rows(3, (0, 0, 0, 0, 0), {"clip_range": 0.2})
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=48)
    sp.add_population_arguments(ap)
    assert sp.population_keywords(ap.parse_args([])) is None
    kw = sp.population_keywords(ap.parse_args(["--population", "3", "--member-lr", "1e-4,2e-4,3e-4", "--member-tau", "0.01", "--pbt-every", "50"]))
    assert kw == dict(members=3, envs_per_member=16, member_hp={"lr": [1e-4, 2e-4, 3e-4], "tau": [0.01]}, pbt_every=50)
    for bad in (["--member-lr", "1e-4"], ["--population", "5"], ["--population", "3", "--member-gamma", "0.9,0.8"], ["--population", "3", "--member-lr", "x"]):
        with pytest.raises(ValueError):
            sp.population_keywords(ap.parse_args(bad))


def test_the_launch_counts_are_the_single_learners():
    from tennisbot_rl_amd import sac, tqc
    assert sp.MEMBERS_LAUNCHES_PER_STEP == {"sac": sac.LAUNCHES_PER_STEP, "tqc": tqc.LAUNCHES_PER_STEP}


# ----------------------------------------------------------------------------------------------------------------- checkpoints
@pytest.mark.parametrize("algo", ["sac", "tqc"])
@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
def test_a_members_checkpoint_round_trips_through_the_trainers_state_dicts(tmp_path, algo, kind):
    """member_checkpoint (what export_member writes, less the env and replay entries, which need a device) -> torch.save ->
    torch.load(weights_only=True), as SACTrainer.load reads it -> load_state_dict into the trainer's modules and its three Adam
    optimisers: every parameter, moment, step count and learning rate arrives bit for bit."""
    from tennisbot_rl_amd.learner import flatten_parameters
    build = sp._algo(algo)[2]
    O, A = DIMS[kind]
    g = torch.Generator().manual_seed(9)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(77)
        src = build(O, A)
    n_pi, n_q = (sum(p.numel() for p in m.parameters()) for m in src[:2])
    pi, q, qt = torch.randn(n_pi, generator=g), torch.randn(n_q, generator=g), torch.randn(n_q, generator=g)
    moments = tuple((torch.randn(n, generator=g), torch.rand(n, generator=g)) for n in (n_pi, n_q, 1))
    lec, hp_row, step = torch.tensor([-0.7]), [1e-4, 2e-4, 5e-4, 0.97, 0.01, 0.0, 0.0, 0.0], 5
    ck = sp.member_checkpoint(algo, O, A, pi, q, qt, lec, moments, hp_row, step)
    path = str(tmp_path / "member.pt")
    torch.save(ck, path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    actor, critic, target = build(O, A)
    log_ent_coef = torch.zeros(1, requires_grad=True)
    opts = (torch.optim.Adam(actor.parameters(), lr=3e-4, eps=1e-8), torch.optim.Adam(critic.parameters(), lr=3e-4, eps=1e-8), torch.optim.Adam([log_ent_coef], lr=3e-4, eps=1e-8))
    actor.load_state_dict(ck["actor"]); critic.load_state_dict(ck["critic"]); target.load_state_dict(ck["critic_target"])
    for o, sd in zip(opts, ck["optimizers"]):
        o.load_state_dict(sd)
    with torch.no_grad():
        log_ent_coef.copy_(ck["log_ent_coef"])
    for module, want in ((actor, pi), (critic, q), (target, qt)):
        assert np.array_equal(bits(flatten_parameters(module)), bits(want))
    assert np.array_equal(bits(log_ent_coef), bits(lec))
    for o, params, (m1, m2), lr in zip(opts, (list(actor.parameters()), list(critic.parameters()), [log_ent_coef]), moments, hp_row[:3]):
        assert o.param_groups[0]["lr"] == lr and o.param_groups[0]["eps"] == 1e-8
        assert np.array_equal(bits(torch.cat([o.state[p]["exp_avg"].reshape(-1) for p in params])), bits(m1))
        assert np.array_equal(bits(torch.cat([o.state[p]["exp_avg_sq"].reshape(-1) for p in params])), bits(m2))
        assert all(int(o.state[p]["step"]) == step for p in params)
    assert ck["hp"] == dict(learning_rate=1e-4, gamma=0.97, tau=0.01, adam_eps=1e-8)


# ------------------------------------------------------------------------------------------ run_population: which member is "best"
class StandInPopulation:
    """what run_population uses of a PopulationSAC, with scores that follow a script: one list per learn() call"""

    def __init__(self, script, R=4):
        self.script, self.M, self.R, self.member_timesteps, self.calls, self.exported, self.saved = list(script), len(script[0]), R, 0, 0, [], 0

    def learn(self, total, log=None, log_every=10):
        self.member_timesteps = int(total)
        self.calls += 1
        return [dict(timesteps=self.member_timesteps, scores=self.script[self.calls - 1])]

    def scores(self):
        return torch.tensor(self.script[self.calls - 1], dtype=torch.float64)

    def save(self, path):
        self.saved += 1

    def export_member(self, m, path):
        self.exported.append(m)


def test_run_population_keeps_the_best_member_it_has_evidence_for(tmp_path):
    """best_model.pt is the member with the highest finite score (NaN is no candidate, whatever its index); with no finite score the
    file written before stays; with none written yet member 0 is, and the line says why. save_freq is in a member's timesteps."""
    nan = math.nan
    path = str(tmp_path / "population.pt")
    # chunks of max(R * log_every, save_freq) = 40 member timesteps; a save after every chunk, the last one the final save
    pop, lines = StandInPopulation([[nan, nan, nan], [nan, 1.5, 2.5], [nan, nan, nan], [3.0, nan, 3.0]]), []
    history = sp.run_population(pop, 160, path, save_freq=40, log=lines.append)
    assert pop.calls == 4 and pop.saved == 4 and len(history) == 4
    assert pop.exported == [0, 2, 0] and len(lines) == 4   # the third save exports nothing; a tie goes to the first
    assert "no member has finished an episode" in lines[0] and "member 2" in lines[1] and "stays as it is" in lines[2] and "member 0" in lines[3]
    # without save_freq: one save, at the end
    pop = StandInPopulation([[nan, nan], [0.5, nan], [nan, -1.0]])
    sp.run_population(pop, 120, path, log=lines.append)
    assert pop.saved == 1 and pop.exported == [1]
