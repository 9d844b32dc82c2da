"""The tuned network (the reference's `train.py -s tuned_ppo`) on the CPU: tests/tuned_reference.py against torch float64 autograd
on `build_tuned_actor_critic`'s module -- forward and the shared-trunk minibatch gradient, to the 1e-11 relative level
test_trpo_reference uses --, the flat layout against named_parameters() and the library's size queries, `pack_policy` undone by
a decoder written from the header's statement of the blob, the refusals that need no device, and the kink margin of the
gradient fixtures the GPU tests use.

Fixtures (`gradient_fixture`). A ReLU net's gradient is discontinuous where a hidden pre-activation crosses 0: a float32 forward
that rounds z = +1e-9 to -1e-9 switches a unit's whole gradient off, and no rounding tolerance covers that. So every fixture's rows
are chosen (on the CPU, by rejection from a seeded stream, until the fixture is full) such that EVERY hidden pre-activation of EVERY
row has |z| >= KINK_MARGIN in float64: at least 100 x the float32 forward error of these fixtures' pre-activations (torch's float32
forward as the twin, asserted here; measured 1.8e-6, so the margin is 2.5e-4 instead of the 1e-4 a twin error below 1e-6 would
have allowed), so no float32 evaluation can flip a sign and no row has to be left out of a comparison.
  sb3        SB3's init, action head x 30: a feature unit is dead on part of the rows and alive on the rest (asserted)
  dead       the same with feature unit 1 dead on ALL rows (bias -4, small weights): its row of W1 and b1, and everything it
             would send upstream, get an exactly zero gradient from both towers (asserted)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import policy_reference as pr
import ppo_reference as ref
import tuned_reference as tref
from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, NET_DEFAULT, NET_TUNED, OBS_DIM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O, A = OBS_DIM[ENV_TENNIS], ACT_DIM[ENV_TENNIS]
N_PARAMS = 9639   # 2 + (12 * 64 + 64 + 64 * 2 + 2) + 2 * (2 * 32 + 32 + 32 * 64 + 64 + 64 * 32 + 32) + (32 * 2 + 2) + (32 + 1)
ORDER = ["log_std"] + ["features_extractor.layers.%d.%s" % (k, w) for k in (0, 2) for w in ("weight", "bias")] \
    + ["%s.%d.%s" % (b, k, w) for b in ("policy_net", "value_net_body") for k in (0, 2, 4) for w in ("weight", "bias")] \
    + ["action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias"]
HP = dict(clip_range=0.2, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5, learning_rate=3e-4)
OBS_SCALE = np.array([6, 3, 1, 2, 2, 2, 6, 3, 2, 4, 4, 4], np.float32)   # racket and ball position / velocity, the envs' order of magnitude
WEIGHT_SETS = ("sb3", "saturating", "tiny", "log_std", "dead")
FIXTURES = {"sb3": dict(seed=101, rows=640), "dead": dict(seed=202, rows=640)}


def make_policy(name, seed=21):
    """weight sets of the tuned net (float32, CPU): sb3 (SB3's init, action head x 30), saturating (N(0, 2^2) hidden weights),
    tiny (pre-activations around 1e-4), log_std (sb3 with log_std at -5 / +2), dead (sb3 with feature unit 1 dead on every input)"""
    import torch
    from tennisbot_rl_amd.ppo import build_tuned_actor_critic
    torch.manual_seed(seed)
    policy = build_tuned_actor_critic(O, A)
    with torch.no_grad():
        policy.action_net.weight.mul_(30.0)
        policy.log_std.copy_(torch.linspace(-1.0, 0.2, A) if name != "log_std" else torch.tensor([-5.0, 2.0]))
        lins = [[m for m in body if isinstance(m, torch.nn.Linear)] for body in (policy.features_extractor.layers, policy.policy_net, policy.value_net_body)]
        for bi, lin in enumerate(lins):
            for j, m in enumerate(lin):
                if name == "saturating":
                    m.weight.normal_(0.0, 2.0); m.bias.normal_(0.0, 1.0)
                elif name == "tiny":
                    m.weight.normal_(0.0, 1e-5 if (bi, j) == (0, 0) else m.in_features ** -0.5); m.bias.normal_(0.0, 1e-4)
        if name == "dead":
            last = policy.features_extractor.layers[2]
            last.weight[1].mul_(0.01); last.bias[1] = -4.0
    return policy


_FIXTURE_CACHE = {}


def gradient_fixture(name):
    """dict(policy, obs [n, O], act [n, A], old_logp, adv, returns [n]) in float32: `rows` rows whose every hidden pre-activation
    keeps KINK_MARGIN (see the module docstring). act is a sample of the policy, old_logp its log-probability under slightly
    different weights (ratios spread around 1, some beyond the clip range), returns near the critic's own scale."""
    if name in _FIXTURE_CACHE:
        return _FIXTURE_CACHE[name]
    spec = FIXTURES[name]
    policy = make_policy(name, seed=spec["seed"])
    rng = np.random.default_rng(spec["seed"])
    kept = []
    while sum(len(k) for k in kept) < spec["rows"]:
        cand = (rng.normal(size=(256, O)) * OBS_SCALE).astype(np.float32)
        t = tref.towers(policy, cand)
        ok = np.all([np.abs(z).min(1) >= tref.KINK_MARGIN for z in t.pre], 0)
        kept.append(cand[ok])
    obs = np.concatenate(kept)[:spec["rows"]]
    t = tref.towers(policy, obs)
    n = len(obs)
    eps = rng.normal(size=(n, A))
    act = (t.mean + np.exp(t.log_std) * eps).astype(np.float32)
    zeta = (act - t.mean) * np.exp(-t.log_std)
    logp = (-0.5 * zeta ** 2 - t.log_std - pr.LN_SQRT_2PI).sum(-1)
    old_logp = (logp + rng.normal(size=n) * 0.15).astype(np.float32)
    adv = (rng.normal(size=n) * 2.0 + 0.3).astype(np.float32)
    returns = (t.value + rng.normal(size=n)).astype(np.float32)
    fx = dict(policy=policy, obs=obs, act=act, old_logp=old_logp, adv=adv, returns=returns)
    _FIXTURE_CACHE[name] = fx
    return fx


def batch_of(fx, idx):
    return tuple(fx[k][idx] for k in ("obs", "act", "old_logp", "adv", "returns"))


def batch_indices(batch, n_rows, seed=5):
    """`batch` row indices into a fixture, with repeats: random rows, the first tenth (at least two) overwritten by copies of row 3;
    a batch of two takes two different rows (the advantage's std of a repeated row is 0)"""
    rng = np.random.default_rng(seed + batch)
    idx = rng.integers(0, n_rows, size=batch)
    if batch > 2:
        idx[: max(2, batch // 10)] = 3
    else:
        idx[:] = (5, 9)
    return idx.astype(np.int64)


def rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


@pytest.mark.parametrize("name", WEIGHT_SETS)
def test_forward_equals_torch_in_float64(name):
    import torch
    policy = make_policy(name)
    rng = np.random.default_rng(3)
    obs = (rng.normal(size=(300, O)) * OBS_SCALE).astype(np.float32)
    t = tref.towers(policy, obs)
    p64 = make_policy(name).double()
    with torch.no_grad():
        mean, value = p64(torch.from_numpy(obs).double())
        feature = p64.features_extractor(torch.from_numpy(obs).double())
    assert rel(mean.numpy(), t.mean) < 1e-11 and rel(value.numpy(), t.value) < 1e-11 and rel(feature.numpy(), t.feature) < 1e-11
    assert np.all(t.mean_bound > 0) and np.all(t.value_bound > 0) and np.all(np.isfinite(t.mean_bound))
    # the bound is a bound: a float32 evaluation that rounds every product and sum (rounds = 2) stays inside its own
    with torch.no_grad():
        m32, v32 = policy(torch.from_numpy(obs))
    b2 = tref.towers(policy, obs, rounds=2)
    pr.assert_within("float32 torch mean", m32.numpy(), t.mean, b2.mean_bound)
    pr.assert_within("float32 torch value", v32.numpy(), t.value, b2.value_bound)
    if name == "dead":
        assert np.all(t.feature[:, 1] == 0.0)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_gradient_equals_torch_autograd_in_float64(name):
    import torch
    fx = gradient_fixture(name)
    idx = batch_indices(257, len(fx["adv"]))
    obs, act, old_logp, adv, returns = batch_of(fx, idx)
    P = pr.state_dict_arrays(fx["policy"])
    for hp in (HP, dict(HP, ent_coef=0.01, vf_coef=0.25)):
        got = tref.loss_and_grads(P, obs, act, old_logp, adv, returns, hp)
        p64 = make_policy(name, seed=FIXTURES[name]["seed"]).double()
        to = lambda x: torch.from_numpy(np.asarray(x, np.float64))  # noqa: E731
        a = to(adv)
        a = (a - a.mean()) / (a.std() + 1e-8)
        value, logp, entropy = p64.evaluate(to(obs), to(act))
        ratio = (logp - to(old_logp)).exp()
        pg = -torch.min(a * ratio, a * ratio.clamp(1 - hp["clip_range"], 1 + hp["clip_range"])).mean()
        vl = ((to(returns) - value) ** 2).mean()
        loss = pg + hp["vf_coef"] * vl - hp["ent_coef"] * entropy
        loss.backward()
        loss = float(loss.detach())
        assert abs(got.loss - loss) <= 1e-12 * max(1.0, abs(loss))
        assert 0.05 < np.mean(~got.active) < 0.95                      # clipped rows and unclipped rows
        scale = max(np.abs(g).max() for g in got.grads.values())
        for k, p in p64.named_parameters():
            assert np.abs(got.grads[k] - p.grad.numpy()).max() <= 1e-11 * scale, k
        for k in tref.TRUNK_KEYS:                                        # the trunk's gradient is the sum of the towers' shares, both non-trivial
            assert np.array_equal(got.grads[k], got.parts["pi"][k] + got.parts["vf"][k])
            assert np.abs(got.parts["pi"][k]).max() > 0 and np.abs(got.parts["vf"][k]).max() > 0
    # the shares alone: vf_coef = 0 leaves the pi share, zero advantages with ent_coef = 0 the vf share
    pi_only = tref.loss_and_grads(P, obs, act, old_logp, adv, returns, dict(HP, vf_coef=0.0))
    base = tref.loss_and_grads(P, obs, act, old_logp, adv, returns, HP)
    for k in tref.TRUNK_KEYS:
        assert np.array_equal(pi_only.grads[k], base.parts["pi"][k])


def test_layout_matches_named_parameters_and_the_library():
    from tennisbot_rl_amd.build import build_library
    from tennisbot_rl_amd.learner import parameter_offsets
    from tennisbot_rl_amd.ppo import pack_policy
    from tennisbot_rl_amd.stepper import load_library
    policy = make_policy("sb3")
    rows, total = tref.layout(O, A)
    assert total == N_PARAMS == sum(p.numel() for p in policy.parameters())
    assert [k for k, _ in policy.named_parameters()] == ORDER == [r[0] for r in rows]
    offsets = parameter_offsets(policy)
    for (name, shape, off), (k, p) in zip(rows, policy.named_parameters()):
        assert tuple(p.shape) == tuple(shape) and offsets[k] == (off, p.numel())
    build_library()
    lib = load_library()
    blob = pack_policy(policy)
    assert lib.tb_policy_blob_floats(ENV_TENNIS, NET_TUNED) == blob.numel() == tref.blob_floats(O, A)
    for kind in (ENV_SWING, ENV_TENNIS):
        assert lib.tb_policy_blob_floats(kind, NET_DEFAULT) == lib.tb_policy_floats(kind) > 0
    assert lib.tb_abi_version() == 4 and lib.tb_ppo_param_floats(7) < 0


@pytest.mark.parametrize("name", ["sb3", "dead"])
def test_pack_policy_round_trip(name):
    """decoding the blob by the header's statement of it gives back every W and b; every padded slot holds 0"""
    from tennisbot_rl_amd.ppo import pack_policy
    policy = make_policy(name)
    blob = pack_policy(policy).numpy()
    sd = {k: v.numpy() for k, v in policy.state_dict().items()}
    p = 0
    plan = [("features_extractor.layers.0", True), ("features_extractor.layers.2", False)]
    for body, head in (("policy_net", "action_net"), ("value_net_body", "value_net")):
        plan += [("%s.%d" % (body, k), False) for k in (0, 2, 4)] + [(head, False)]
    for key, first in plan:
        W = sd[key + ".weight"]
        padded_out = 16 if key in ("action_net", "value_net", "features_extractor.layers.2") else W.shape[0]
        Wb, bb, used = tref.unpack_layer(blob[p:], W.shape[1], W.shape[0], first)
        assert np.array_equal(Wb, W) and np.array_equal(bb, sd[key + ".bias"]), key
        assert used == -(-padded_out // 16) * (16 + (-(-W.shape[1] // 4) if first else 4 * -(-W.shape[1] // 16)) * 64), key
        p += used
    assert np.array_equal(blob[p:p + A], sd["log_std"]) and np.all(blob[p + A:] == 0) and len(blob) == p + 4


def test_refusals_that_need_no_device():
    from tennisbot_rl_amd.build import build_library
    from tennisbot_rl_amd.ppo import PPOTrainer
    from tennisbot_rl_amd.stepper import load_library
    from tennisbot_rl_amd.trpo import TRPOTrainer
    build_library()
    lib = load_library()
    assert lib.tb_policy_blob_floats(ENV_SWING, NET_TUNED) == -3 and b"Tennisbot" in lib.tb_last_error()      # TB_E_PARAMS
    assert lib.tb_policy_blob_floats(ENV_TENNIS, 2) == -3 and lib.tb_policy_blob_floats(5, NET_DEFAULT) == -1
    with pytest.raises(ValueError, match="Tennisbot"):
        PPOTrainer("SwingRacket-v0", num_envs=16, n_steps=26, policy="tuned")
    with pytest.raises(ValueError, match="policy"):
        PPOTrainer("Tennisbot-v0", num_envs=16, n_steps=26, policy="nonsense")
    with pytest.raises(ValueError, match="net_arch"):
        TRPOTrainer("Tennisbot-v0", num_envs=16, n_steps=26, policy="tuned")
    from tennisbot_rl_amd.trpo import FusedTRPO
    with pytest.raises(ValueError, match="net_arch"):
        FusedTRPO(ENV_TENNIS, make_policy("sb3"), None, {}, "cpu")
    assert lib.tb_ppo_param_floats_net(ENV_TENNIS, NET_TUNED) == N_PARAMS and lib.tb_ppo_param_floats_net(ENV_SWING, NET_TUNED) == -3
    assert lib.tb_ppo_param_floats_net(ENV_TENNIS, NET_DEFAULT) == lib.tb_ppo_param_floats(ENV_TENNIS) == 10181
    share = lib.tb_ppo_rows_per_workgroup()
    per_partial = (lib.tb_ppo_workspace_bytes_net(ENV_TENNIS, NET_TUNED, share + 1) - lib.tb_ppo_workspace_bytes_net(ENV_TENNIS, NET_TUNED, share)) // 8
    assert per_partial == N_PARAMS + 2 + 962                                  # gradient, two statistics, the vf waves' extractor share
    assert lib.tb_ppo_workspace_bytes_net(ENV_SWING, NET_TUNED, 64) == -3
    assert lib.tb_ppo_workspace_bytes(ENV_TENNIS, 600) == lib.tb_ppo_workspace_bytes_net(ENV_TENNIS, NET_DEFAULT, 600)
    # TB_PPO_VALUE_ONLY (4) is not offered for the tuned net; refused on the host before a device is looked for
    assert lib.tb_ppo_apply_net(ENV_TENNIS, NET_TUNED, 0, None, 1 | 4, 16, 1 << 30, 64, 16, 16, 16, 16, N_PARAMS, 16, 0.0, 0.5, 1, 3e-4, 0.9, 0.999, 1e-5, 1) == -4
    assert b"TB_PPO_VALUE_ONLY" in lib.tb_last_error()
    for argv in (["-s", "sac"], ["-s", "tuned_ppo", "--bogus"]):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + argv, capture_output=True, text=True)
        assert p.returncode != 0 and (p.stderr + p.stdout).strip(), argv
    p = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-s", "sac"], capture_output=True, text=True)
    assert "ppo" in p.stderr and "tuned_ppo" in p.stderr


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixtures_keep_the_kink_margin(name):
    fx = gradient_fixture(name)
    t = tref.towers(fx["policy"], fx["obs"])
    assert len(fx["obs"]) == FIXTURES[name]["rows"]
    assert min(float(np.abs(z).min()) for z in t.pre) >= tref.KINK_MARGIN
    # the float32 twin of the forward pass: the margin is at least 100 x the error of its pre-activations
    import torch
    with torch.no_grad():
        x, worst, k = torch.from_numpy(fx["obs"]), 0.0, 0
        f = x
        for m in fx["policy"].features_extractor.layers:
            f = m(f)
            if isinstance(m, torch.nn.Linear):
                worst = max(worst, float(np.abs(f.numpy().astype(np.float64) - t.pre[k]).max())); k += 1
        for body in (fx["policy"].policy_net, fx["policy"].value_net_body):
            h = f
            for m in body:
                h = m(h)
                if isinstance(m, torch.nn.Linear):
                    worst = max(worst, float(np.abs(h.numpy().astype(np.float64) - t.pre[k]).max())); k += 1
    assert k == len(t.pre) == 8 and 100.0 * worst <= tref.KINK_MARGIN, worst
    print("fixture %s: float32 twin error of the pre-activations %.3g, margin %.3g" % (name, worst, tref.KINK_MARGIN))
    P = pr.state_dict_arrays(fx["policy"])
    g = tref.loss_and_grads(P, *batch_of(fx, np.arange(len(fx["obs"]))), HP)
    if name == "dead":
        assert np.all(t.pre[1][:, 1] < 0)
        for share in (g.parts["pi"], g.parts["vf"], g.grads):
            assert np.all(share["features_extractor.layers.2.weight"][1] == 0.0) and share["features_extractor.layers.2.bias"][1] == 0.0
        for body in ("policy_net", "value_net_body"):
            assert np.all(g.grads[body + ".0.weight"][:, 1] == 0.0)      # nothing ever arrives through the dead feature
    else:
        dead = np.mean(t.pre[1] < 0, 0)
        assert ((dead > 0.1) & (dead < 0.9)).any(), dead                  # a feature unit dead on part of the rows
        assert np.all(np.abs(g.grads["features_extractor.layers.2.weight"]).max(1) > 0)
