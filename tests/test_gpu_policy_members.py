"""A population of policy networks in one launch (tb_policy_evaluate_members; tb_policy_evaluate_kernel's members form in
csrc/tb_kernels.hpp) on a real MI355X. The yardstick is the existing single-blob call: resets and noise are keyed by the global env
id, so row m of a members launch over M x R envs at ID_BASE must equal, bit for bit, policy_evaluate with blob m on a fresh handle
of R envs whose env_id_base is ID_BASE + m R. Then equal members against policy_evaluate on one handle, the episode contract, the
refusals on a real handle, and PolicyESTrainer's generation against its parts.

The members' blobs here are built one by one with pack_policy (a module per member, its own log_std), not with
pack_policy_members: that one is held against pack_policy in tests/test_policy_es_reference.py."""
import os

import numpy as np
import pytest

from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, NET_DEFAULT, NET_MLP64, NET_TUNED, OBS_DIM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NOISE_SEED = 0x5EED1234ABCD
ENV_SEED, ID_BASE = 21, 1 << 33   # (env ids beyond 32 bits: the noise key's high word is in use)
PERTURBATION = 0.1
# The tuned net's seed is chosen, not arbitrary: its ReLU extractor ends in a 2-wide feature, and under most N(0, 0.1^2) perturbations both
# outputs are dead for every observation -- the action is then a constant, every episode runs 1001 steps to a return of 0, and two such
# members cannot be told apart (seeds 88, 90, 92, 93, 95, 97, 98 of 88..99 on an MI355X). With 96 both members move the racket:
# lengths 329..801 and 412..902. The separation is asserted in the test either way.
PERTURBATION_SEED = {(ENV_SWING, NET_DEFAULT): 77, (ENV_SWING, NET_MLP64): 79, (ENV_TENNIS, NET_DEFAULT): 87, (ENV_TENNIS, NET_TUNED): 96}
M_MAX = 3


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_BLOBS = {}


def base_policy(torch, kind, net):
    """tests/test_gpu_policy_evaluate.py's weights: SwingRacket -- the reference's shipped policy (NET_MLP64: the [64, 64] student fitted
    to it); Tennisbot -- seeded random weights with an action head that moves the racket and unequal log_std"""
    from tennisbot_rl_amd.policy_es import build_policy
    policy = build_policy(kind, net, seed=1234)
    if kind == ENV_SWING and net == NET_DEFAULT:
        policy.load_sb3_arrays(dict(np.load(os.path.join(GOLDEN, "ppo_swing_policy.npz"))))
    elif kind == ENV_SWING:
        policy.load_state_dict({k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "mlp64_swing_student.npz")).items()})
    else:
        with torch.no_grad():
            policy.action_net.weight.mul_(30.0)
            policy.log_std.copy_(torch.linspace(-1.0, 0.2, ACT_DIM[kind]))
    return policy


def member_blobs(torch, kind, net):
    """[M_MAX, B] on the GPU, built once per (kind, net): member m is the base actor plus a seeded N(0, 0.1^2) perturbation, with a
    log_std row of its own; each row is pack_policy of that member's module"""
    from tennisbot_rl_amd.policy_es import actor_flat, set_actor_flat
    from tennisbot_rl_amd.ppo import pack_policy
    key = (kind, net)
    if key not in _BLOBS:
        g = torch.Generator().manual_seed(PERTURBATION_SEED[key])
        rows = []
        for m in range(M_MAX):
            policy = base_policy(torch, kind, net)
            base = actor_flat(policy)
            set_actor_flat(policy, base + PERTURBATION * torch.randn(base.numel(), generator=g))
            with torch.no_grad():
                policy.log_std.add_(0.15 * m * torch.linspace(-1.0, 1.0, ACT_DIM[kind]))
            rows.append(pack_policy(policy.to("cuda:0")))
        _BLOBS[key] = torch.stack(rows)
    return _BLOBS[key]


def case_params(extended=False):
    from tennisbot_rl_amd.params import F_DEFAULT, F_RACKET_GROUND, default_params, reference_rolling_friction
    if extended:  # the reference's full contact set: racket<->court contact + the rolling-friction rows
        return default_params(flags=F_DEFAULT | F_RACKET_GROUND, **reference_rolling_friction())
    return default_params()


def make_env(kind, n, params, pipeline=None, base=ID_BASE):
    from tennisbot_rl_amd.stepper import BatchedEnv
    return BatchedEnv(kind, n, device="cuda:0", seed=ENV_SEED, env_id_base=base, params=params, pipeline=kind == ENV_SWING if pipeline is None else pipeline,
                      track_terminal_obs=False)


def members(torch, env, w, R, deterministic, net):
    ret, length = env.policy_evaluate_members(w, R, seed=NOISE_SEED, deterministic=deterministic, net=net)
    torch.cuda.synchronize()
    return ret.cpu().numpy(), length.cpu().numpy()


def single(torch, env, w, deterministic, net):
    ret, length = env.policy_evaluate(w, seed=NOISE_SEED, deterministic=deterministic, net=net)
    torch.cuda.synchronize()
    return ret.cpu().numpy(), length.cpu().numpy()


def padded(torch, w, extra):
    """the rows `extra` floats further apart, NaN in between: floats the kernel must never read"""
    out = torch.full((w.shape[0], w.shape[1] + extra), float("nan"), dtype=torch.float32, device=w.device)
    out[:, :w.shape[1]] = w
    return out


TWIN_CASES = [  # kind, net, M, R, deterministic, extended contact set, NaN-padded stride
    (ENV_TENNIS, NET_DEFAULT, 3, 16, False, False, True),
    (ENV_TENNIS, NET_TUNED, 2, 32, True, False, False),
    (ENV_TENNIS, NET_DEFAULT, 2, 16, False, True, False),
    (ENV_SWING, NET_DEFAULT, 3, 16, False, False, True),
    (ENV_SWING, NET_MLP64, 2, 48, False, False, False),
    (ENV_SWING, NET_DEFAULT, 2, 16, True, True, False),
]


@pytest.mark.parametrize("kind,net,M,R,deterministic,extended,pad", TWIN_CASES)
def test_each_member_is_its_twin_handle_bit_for_bit(torch, kind, net, M, R, deterministic, extended, pad):
    w, params = member_blobs(torch, kind, net)[:M].contiguous(), case_params(extended)
    a = make_env(kind, M * R, params)
    assert R % a.policy_member_granule() == 0
    wa = padded(torch, w, 8) if pad else w
    assert wa.shape[1] == a.policy_floats(net) + (8 if pad else 0) and wa.data_ptr() % 16 == 0
    ret, length = members(torch, a, wa, R, deterministic, net)
    assert ret.shape == (M, R) and length.shape == (M, R) and ret.dtype == np.float64 and length.dtype == np.int32
    for m in range(M):
        twin = make_env(kind, R, params, base=ID_BASE + m * R)
        want_ret, want_len = single(torch, twin, w[m], deterministic, net)
        twin.close()
        print("kind=%d net=%d member %d: lengths %d .. %d, returns %g .. %g" % (kind, net, m, length[m].min(), length[m].max(), ret[m].min(), ret[m].max()))
        assert np.array_equal(length[m], want_len), (m, length[m], want_len)
        assert np.array_equal(ret[m], want_ret), (m, ret[m], want_ret)
    # the test can tell members apart: member 1's envs under member 0's weights are other episodes
    twin = make_env(kind, R, params, base=ID_BASE + R)
    other_ret, other_len = single(torch, twin, w[0], deterministic, net)
    twin.close()
    assert not (np.array_equal(other_ret, ret[1]) and np.array_equal(other_len, length[1])), "member 0's weights reproduce member 1's row: the case cannot see a wrong blob"
    assert np.all(np.isfinite(ret)) and np.any(ret != 0.0)
    if kind == ENV_SWING:
        assert np.all(length == 26)
    else:
        assert np.all((length >= 1) & (length <= 1001))
    c = a.counters()
    assert c["episodes_finished"] == M * R and c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0
    assert a.phase() == 0
    a.close()


@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
@pytest.mark.parametrize("M,R", [(3, 16), (1, 48)])
def test_equal_members_are_policy_evaluate(torch, kind, M, R):
    w1, params = member_blobs(torch, kind, NET_DEFAULT)[1], case_params()
    a, b = make_env(kind, M * R, params), make_env(kind, M * R, params)
    ret, length = members(torch, a, w1.unsqueeze(0).repeat(M, 1), R, False, NET_DEFAULT)
    want_ret, want_len = single(torch, b, w1, False, NET_DEFAULT)
    assert np.array_equal(ret.reshape(-1), want_ret) and np.array_equal(length.reshape(-1), want_len)
    a.close(); b.close()


@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
def test_call_k_is_episode_k_and_the_handle_is_left_freshly_reset(torch, kind):
    M, R = 2, 16
    w, params = member_blobs(torch, kind, NET_DEFAULT)[:M].contiguous(), case_params()
    a, twin, plain = (make_env(kind, M * R, params) for _ in range(3))
    r0, l0 = members(torch, a, w, R, False, NET_DEFAULT)
    r1, l1 = members(torch, a, w, R, False, NET_DEFAULT)
    assert not np.array_equal(r0, r1), "two calls on one handle returned the same episodes"
    t0, tl0 = members(torch, twin, w, R, False, NET_DEFAULT)
    assert np.array_equal(t0, r0) and np.array_equal(tl0, l0)       # a fresh twin's first call repeats the first
    plain.reset()
    plain.reset()                                                  # two calls = two resets: episode 1
    wa, da = a.get_state_words()
    wp, dp = plain.get_state_words()
    assert torch.equal(wa, wp) and torch.equal(da, dp)
    assert int(wa[-1].min()) == 1 and int(wa[-1].max()) == 1       # (the episode word)
    assert a.phase() == 0
    for e in (a, twin, plain):
        e.close()


def test_refusals_on_a_real_handle_launch_nothing(torch):
    from tennisbot_rl_amd.stepper import StepperError
    n = 48
    w = member_blobs(torch, ENV_SWING, NET_DEFAULT)
    B = w.shape[1]
    wide = padded(torch, w, 8)
    ret = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    length = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    piped, plain = make_env(ENV_SWING, n, case_params(), True), make_env(ENV_SWING, n, case_params(), False)

    def call(env, net, ptr, M, stride, R):
        return env.L.tb_policy_evaluate_members(env._h, net, ptr, M, stride, R, ret.data_ptr(), length.data_ptr(), 1, 0, None)

    piped.reset()
    w0, d0 = piped.get_state_words()
    cases = [  # net, weights, M, stride, R, code
        (NET_DEFAULT, wide.data_ptr(), 6, B + 8, 8, -1),        # R below the granule
        (NET_DEFAULT, wide.data_ptr(), 2, B + 8, 24, -1),       # R not a multiple of it
        (NET_DEFAULT, wide.data_ptr(), 2, B + 8, 16, -1),       # M R != n
        (NET_DEFAULT, wide.data_ptr(), 3, B - 4, 16, -1),       # a stride below the blob
        (NET_DEFAULT, wide.data_ptr(), 3, B + 2, 16, -1),       # ... not a multiple of 4
        (NET_DEFAULT, wide.data_ptr() + 4, 3, B + 4, 16, -1),   # a misaligned base
        (NET_DEFAULT, None, 3, B + 8, 16, -1),
        (NET_DEFAULT, wide.data_ptr(), 0, B + 8, 16, -1),
        (NET_TUNED, wide.data_ptr(), 3, B + 8, 16, -3),         # the tuned network is Tennisbot's
    ]
    for net, ptr, M, stride, R, code in cases:
        assert call(piped, net, ptr, M, stride, R) == code, (net, M, stride, R)
        assert b"tb_policy_evaluate_members" in piped.L.tb_last_error()
    w1, d1 = piped.get_state_words()
    assert torch.equal(w0, w1) and torch.equal(d0, d1) and piped.phase() == 0
    # SwingRacket without the pipeline: TB_E_UNSUPPORTED
    plain.reset()
    p0, q0 = plain.get_state_words()
    assert call(plain, NET_DEFAULT, wide.data_ptr(), 3, B + 8, 16) == -4 and b"tb_policy_evaluate_members" in plain.L.tb_last_error()
    with pytest.raises(StepperError, match="tb_set_pipeline"):
        plain.policy_evaluate_members(w, 16)
    p1, q1 = plain.get_state_words()
    assert torch.equal(p0, p1) and torch.equal(q0, q1)
    # the Python side refuses before the library is asked
    with pytest.raises(ValueError, match="granule"):
        piped.policy_evaluate_members(w, 24)
    with pytest.raises(ValueError):
        piped.policy_evaluate_members(w[:2], 16)
    torch.cuda.synchronize()
    assert float(ret.abs().sum()) == 0.0 and int(length.abs().sum()) == 0   # nothing was written
    # ... and the handle still evaluates; a misaligned view is re-packed, not refused
    r, ln = piped.policy_evaluate_members(w, 16, seed=NOISE_SEED)
    assert bool((ln == 26).all()) and tuple(r.shape) == (3, 16)
    fresh = make_env(ENV_SWING, n, case_params(), True)
    fresh.reset()                                                  # (piped was reset once before its first evaluation)
    buf = torch.full((3 * (B + 4) + 1,), float("nan"), dtype=torch.float32, device="cuda:0")
    view = buf[1:].view(3, B + 4)[:, :B + 3]                       # rows of B + 3 floats, B + 4 apart, at base + 4 bytes
    view[:, :B] = w
    assert view.data_ptr() % 16 == 4 and not view.is_contiguous()
    r2, _ = fresh.policy_evaluate_members(view, 16, seed=NOISE_SEED)
    torch.cuda.synchronize()
    assert torch.equal(r, r2)
    for e in (piped, plain, fresh):
        e.close()


def test_trainer_generation_is_its_parts(torch, tmp_path):
    from tennisbot_rl_amd.es import es_update, fitness
    from tennisbot_rl_amd.policy_es import PolicyESTrainer, actor_flat
    from tennisbot_rl_amd.ppo import PPOTrainer
    reference = os.path.join(GOLDEN, "ppo_swing_policy.npz")
    mk = lambda: PolicyESTrainer("SwingRacket-v0", popsize=4, repeats=16, elite=2, init=reference, device="cuda:0", seed=5)  # noqa: E731
    tr, twin = mk(), mk()
    assert tr.env.num_envs == 2 * 4 * 16 and tr.env.pipeline and tr.deterministic
    state = torch.cuda.get_rng_state("cuda:0").clone()
    w0 = tr.w.clone()
    info = tr.step()
    assert torch.equal(torch.cuda.get_rng_state("cuda:0"), state), "the generation drew from torch's global RNG"
    # the fitness: the mean over repeats of the members launch, on an identically seeded trainer's parts
    eps = twin.sample_noise()
    assert torch.equal(eps, info["eps"])
    ret, length = twin.env.policy_evaluate_members(twin.population(eps), twin.repeats, seed=twin.noise_seed, deterministic=twin.deterministic, net=twin.net)
    assert torch.equal(info["fitness"], fitness(ret)) and torch.equal(info["fitness"], ret.mean(dim=1).float()) and torch.equal(info["lengths"], length)
    assert bool((length == 26).all()) and len(set(info["fitness"].tolist())) > 1
    # the update: es.py's, recomputed on the same device
    p = tr.popsize
    want, _ = es_update(w0, info["eps"], info["fitness"][:p], info["fitness"][p:], 0.2, 2)
    assert torch.equal(tr.w, want) and not torch.equal(tr.w, w0)
    log = tr.log()
    assert log["generation"] == 1 and log["steps"] == 128 * 26 and not log["skipped"]
    # save -> load round-trips, and the file is a checkpoint the PPO trainer's policy reads
    path = str(tmp_path / "es.pt")
    tr.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck.keys()) == {"policy", "net", "es"} and ck["net"] == "default" and ck["es"]["generation"] == 1
    other = mk().load(path)
    assert torch.equal(other.w, tr.w) and other.generation == 1 and other.lr == tr.lr and other.sigma == tr.sigma
    assert torch.equal(other.sample_noise(), tr.sample_noise())   # the generator's state travels too
    ppo = PPOTrainer("SwingRacket-v0", num_envs=64, n_steps=26, device="cuda:0", seed=0, graph=False)
    ppo.policy.load_state_dict(ck["policy"])
    assert torch.equal(actor_flat(ppo.policy), tr.w)
    out = tr.evaluate(32)
    assert out["episodes"] == 32 and out["mean_length"] == 26.0
    for t in (tr, twin, other):
        t.close()
