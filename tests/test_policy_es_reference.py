"""tennisbot_rl_amd/policy_es.py without a GPU: the actor's flat view, the batched packing of a population against pack_policy row
by row, train_es.py's parser, and the refusals that need no device."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, NET_DEFAULT, NET_MLP64, NET_TUNED, OBS_DIM  # noqa: E402

CASES = [(ENV_SWING, NET_DEFAULT), (ENV_TENNIS, NET_DEFAULT), (ENV_TENNIS, NET_TUNED), (ENV_SWING, NET_MLP64)]
M = 3


def layer_floats(n_in, n_out):
    """csrc/tb_policy.hpp layer_floats: bias tiles + weight fragments of one layer of the blob"""
    return -(-n_out // 16) * (16 + -(-n_in // 4) * 64)


def regions(kind, net):
    """(actor end, value tower [begin, end), log_std begin) in the blob, from the header's layout"""
    O, A = OBS_DIM[kind], ACT_DIM[kind]
    if net == NET_TUNED:
        trunk = layer_floats(O, 64) + layer_floats(64, A)
        tower = layer_floats(16, 32) + layer_floats(32, 64) + layer_floats(64, 32) + layer_floats(32, A)
        return trunk + tower, (trunk + tower, trunk + 2 * tower), trunk + 2 * tower
    arch = (32, 64, 32) if (kind == ENV_SWING and net == NET_DEFAULT) else (64, 64)
    tower, d = 0, O
    for h in arch:
        tower += layer_floats(d, h)
        d = h
    tower += layer_floats(d, A)
    return tower, (tower, 2 * tower), 2 * tower


def template(torch, kind, net):
    from tennisbot_rl_amd.policy_es import build_policy
    policy = build_policy(kind, net, seed=5)
    with torch.no_grad():
        policy.log_std.copy_(torch.linspace(-1.0, 0.2, ACT_DIM[kind]))
        policy.value_net.weight.mul_(3.0)
    return policy


@pytest.mark.parametrize("kind,net", CASES)
def test_pack_policy_members_rows_are_pack_policy_bit_for_bit(kind, net):
    import torch
    from tennisbot_rl_amd.policy_es import actor_flat, actor_parameters, pack_policy_members, set_actor_flat
    from tennisbot_rl_amd.ppo import pack_policy
    policy = template(torch, kind, net)
    base = actor_flat(policy)
    names = [n for n, p in policy.named_parameters() if any(p is q for q in actor_parameters(policy))]
    want = [n for n, _ in policy.named_parameters() if n.startswith(("features_extractor.", "policy_net.", "action_net."))]
    assert names == want and not any(n.startswith(("value_net", "log_std")) for n in names)
    # Pa: the pi path's parameter sizes, the tuned net's extractor once
    pa = sum(p.numel() for n, p in policy.named_parameters() if n in want)
    assert base.numel() == pa
    if net == NET_TUNED:
        assert sum(n.startswith("features_extractor.") for n in names) == 4 and names[0].startswith("features_extractor.")
        assert pa == (12 * 64 + 64) + (64 * 2 + 2) + (2 * 32 + 32) + (32 * 64 + 64) + (64 * 32 + 32) + (32 * 2 + 2)
    g = torch.Generator().manual_seed(9)
    flat = base + 0.1 * torch.randn((M, pa), generator=g)
    blob0 = pack_policy(policy)
    rows = pack_policy_members(policy, flat)
    assert rows.shape == (M, blob0.numel()) and rows.dtype == torch.float32
    actor_end, (v0, v1), ls = regions(kind, net)
    assert blob0.numel() == ls + (ACT_DIM[kind] + 3) // 4 * 4
    for m in range(M):
        twin = template(torch, kind, net)
        set_actor_flat(twin, flat[m])
        assert torch.equal(actor_flat(twin).view(torch.int32), flat[m].view(torch.int32))
        assert torch.equal(rows[m].view(torch.int32), pack_policy(twin).view(torch.int32)), "row %d is not pack_policy of that member" % m
        # the value tower and log_std are the template's; the actor's region is the member's own
        assert torch.equal(rows[m, v0:v1].view(torch.int32), blob0[v0:v1].view(torch.int32))
        assert torch.equal(rows[m, ls:].view(torch.int32), blob0[ls:].view(torch.int32))
        assert not torch.equal(rows[m, :actor_end], blob0[:actor_end])
    # `out`: refreshed in place, the same bits
    out = torch.full_like(rows, float("nan"))
    assert pack_policy_members(policy, flat, out=out) is out and torch.equal(out.view(torch.int32), rows.view(torch.int32))
    # the template itself was not written
    assert torch.equal(actor_flat(policy).view(torch.int32), base.view(torch.int32))
    with pytest.raises(ValueError):
        pack_policy_members(policy, flat[:, :-1])


@pytest.mark.parametrize("kind,net", CASES)
def test_actor_flat_round_trips_bit_for_bit(kind, net):
    import torch
    from tennisbot_rl_amd.policy_es import actor_flat, set_actor_flat
    policy = template(torch, kind, net)
    sd = {k: v.clone() for k, v in policy.state_dict().items()}
    vec = actor_flat(policy)
    g = torch.Generator().manual_seed(2)
    other = torch.randn(vec.numel(), generator=g)
    set_actor_flat(policy, other)
    assert torch.equal(actor_flat(policy).view(torch.int32), other.view(torch.int32))
    for k, v in policy.state_dict().items():   # nothing off the pi path moved
        if k.startswith(("value_net", "log_std")):
            assert torch.equal(v, sd[k]), k
    set_actor_flat(policy, vec)
    for k, v in policy.state_dict().items():
        assert torch.equal(v.view(torch.int32), sd[k].view(torch.int32)), k
    with pytest.raises(ValueError):
        set_actor_flat(policy, vec[:-1])


def test_train_es_parser_defaults_do_not_move():
    import train_es
    args = train_es.parse([])
    assert args.policy == "gatedcnn" and args.repeats == 10 and args.environment == "SwingRacket-v0" and args.popsize == 200 and args.elite == 66
    assert args.init is None and not args.stochastic and args.net == "default"
    mlp = train_es.parse(["--policy", "mlp"])
    assert mlp.policy == "mlp" and mlp.repeats == 16
    assert train_es.parse(["--policy", "mlp", "--repeats", "32"]).repeats == 32
    ref = train_es.parse(["--policy", "mlp", "--init", "reference"])
    assert ref.init == os.path.join(ROOT, "tests", "golden", "ppo_swing_policy.npz") and os.path.exists(ref.init)
    with pytest.raises(SystemExit):
        train_es.parse(["--policy", "transformer"])
    with pytest.raises(SystemExit):
        train_es.parse(["--init", "reference"])                                   # --init belongs to --policy mlp
    with pytest.raises(SystemExit):
        train_es.parse(["--policy", "mlp", "--init", "reference", "--environment", "Tennisbot-v0"])


def test_trainer_refuses_repeats_off_the_granule_before_any_device_use():
    from tennisbot_rl_amd.policy_es import PolicyESTrainer
    with pytest.raises(ValueError, match="multiple of the member granule 16"):
        PolicyESTrainer("SwingRacket-v0", popsize=4, repeats=10, elite=2)
    with pytest.raises(ValueError, match="granule"):
        PolicyESTrainer("Tennisbot-v0", popsize=4, repeats=0, elite=2)


def test_rank_checkpoints_help_states_how_to_read_the_table():
    tool = os.path.join(ROOT, "tools", "rank_checkpoints.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    text = " ".join(out.stdout.split())
    assert "MEMBERS SEE DIFFERENT EPISODES" in text and "STANDARD ERRORS" in text and "--episodes-per-member" in text


def test_rank_checkpoints_plan_covers_the_episodes_in_whole_launches():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rank_checkpoints as rc
    assert rc.plan(3, 256) == (256, 1)
    assert rc.plan(3, 250) == (256, 1)                       # rounded up to the granule
    assert rc.plan(1, 1) == (16, 1)
    per, launches = rc.plan(400, 1024)                       # 400 x 1024 envs do not fit one batch: more launches
    assert per % 16 == 0 and 400 * per <= rc.MAX_ENVS and per * launches >= 1024 and per * (launches - 1) < 1024
