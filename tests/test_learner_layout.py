"""The fused learner's host-side contract, on CPU: `flatten_parameters` re-points a policy's parameters at one flat buffer in the
documented order (named_parameters(), each tensor row-major) without changing anything a user of the module can see; the library
reports the parameter counts the kernels are instantiated for; PPOTrainer refuses an unknown learner."""
import copy

import numpy as np
import pytest

from tennisbot_rl_amd.learner import flatten_parameters, parameter_offsets
from tennisbot_rl_amd.params import ENV_SWING, ENV_TENNIS, OBS_DIM
from tennisbot_rl_amd.ppo import pack_policy
from test_ppo_reference import make_policy

ARCHS = {"swing": ((32, 64, 32), ENV_SWING, 9069), "tennis": ((64, 64), ENV_TENNIS, 10181)}
ORDER = {
    "swing": ["log_std", "policy_net.0.weight", "policy_net.0.bias", "policy_net.2.weight", "policy_net.2.bias", "policy_net.4.weight", "policy_net.4.bias",
              "value_net_body.0.weight", "value_net_body.0.bias", "value_net_body.2.weight", "value_net_body.2.bias", "value_net_body.4.weight",
              "value_net_body.4.bias", "action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias"],
    "tennis": ["log_std", "policy_net.0.weight", "policy_net.0.bias", "policy_net.2.weight", "policy_net.2.bias", "value_net_body.0.weight",
               "value_net_body.0.bias", "value_net_body.2.weight", "value_net_body.2.bias", "action_net.weight", "action_net.bias", "value_net.weight",
               "value_net.bias"],
}


@pytest.mark.parametrize("name", list(ARCHS))
def test_flatten_parameters_changes_nothing_but_the_storage(name):
    import torch
    arch, kind, count = ARCHS[name]
    policy = make_policy(arch, kind)
    obs = torch.from_numpy(np.random.default_rng(1).normal(size=(37, OBS_DIM[kind])).astype(np.float32))
    before = copy.deepcopy(policy.state_dict())
    with torch.no_grad():
        mean0, value0 = policy(obs)
    packed0 = pack_policy(policy).clone()
    policy._pack_index = None
    names0 = [k for k, _ in policy.named_parameters()]
    ids0 = [id(p) for p in policy.parameters()]

    flat = flatten_parameters(policy)
    assert flat.dtype == torch.float32 and flat.dim() == 1 and flat.is_contiguous() and flat.numel() == count == sum(p.numel() for p in policy.parameters())
    assert [k for k, _ in policy.named_parameters()] == names0 == ORDER[name]
    assert [id(p) for p in policy.parameters()] == ids0            # the same Parameter objects: an optimiser built before keeps them
    after = policy.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    # every parameter aliases the buffer at the documented offset: the running sum of numel in named_parameters() order
    off, offsets = 0, parameter_offsets(policy)
    for k, p in policy.named_parameters():
        assert offsets[k] == (off, p.numel())
        assert p.data_ptr() == flat.data_ptr() + 4 * off and p.is_contiguous() and p.requires_grad
        assert torch.equal(flat[off:off + p.numel()], before[k].reshape(-1))      # row-major, as torch holds it
        off += p.numel()
    assert flatten_parameters(policy) is flat                        # a second call finds the aliasing intact
    with torch.no_grad():
        mean1, value1 = policy(obs)
    assert torch.equal(mean1, mean0) and torch.equal(value1, value0)
    assert torch.equal(pack_policy(policy), packed0)

    # load_state_dict writes through to the flat buffer
    other = {k: v + 0.25 for k, v in before.items()}
    policy.load_state_dict(other)
    assert torch.equal(flat, torch.cat([other[k].reshape(-1) for k in ORDER[name]]))
    # ... and so does an optimiser step on the views
    opt = torch.optim.Adam(policy.parameters(), lr=1e-2)
    snapshot = flat.clone()
    mean, value = policy(obs)
    (mean.sum() + value.sum() + policy.log_std.sum()).backward()
    opt.step()
    assert all(p.data_ptr() == flat.data_ptr() + 4 * offsets[k][0] for k, p in policy.named_parameters())
    moved = (flat != snapshot)
    assert moved.all(), "an Adam step on the views left %d elements of the flat buffer where they were" % int((~moved).sum())
    assert torch.equal(flat, torch.cat([p.detach().reshape(-1) for p in policy.parameters()]))


def test_the_library_reports_the_parameter_counts():
    from tennisbot_rl_amd.build import build_library
    from tennisbot_rl_amd.stepper import load_library
    build_library()
    lib = load_library()
    for name, (arch, kind, count) in ARCHS.items():
        assert lib.tb_ppo_param_floats(kind) == count == sum(p.numel() for p in make_policy(arch, kind).parameters())
    assert lib.tb_ppo_param_floats(7) < 0
    share = lib.tb_ppo_rows_per_workgroup()
    assert share >= 16 and share % 16 == 0
    assert lib.tb_ppo_workspace_bytes(ENV_SWING, 2) > 0 and lib.tb_ppo_workspace_bytes(ENV_SWING, 1) < 0 and lib.tb_ppo_workspace_bytes(9, 64) < 0
    assert lib.tb_ppo_workspace_bytes(ENV_SWING, share + 1) > lib.tb_ppo_workspace_bytes(ENV_SWING, share)
    # refused on the host, before a device is looked for
    assert lib.tb_ppo_gae(ENV_SWING, 0, None, 4, 4, None, 0, None, 0, None, None, 0.99, 0.95, None, None) == -1
    assert lib.tb_ppo_grad(ENV_SWING, 0, None, 16, 16, 16, 16, 16, 10, 16, 8, 16, 9068, 0.2, 0.5, 16, 1 << 30) == -1 and b"n_params" in lib.tb_last_error()
    assert lib.tb_ppo_grad(ENV_SWING, 0, None, 16, 18, 16, 16, 16, 10, 16, 8, 16, 9069, 0.2, 0.5, 16, 1 << 30) == -1 and b"aligned" in lib.tb_last_error()


def test_an_unknown_learner_is_refused():
    from tennisbot_rl_amd.ppo import PPOTrainer
    with pytest.raises(ValueError, match="learner"):
        PPOTrainer("SwingRacket-v0", num_envs=16, n_steps=26, learner="nonsense")
