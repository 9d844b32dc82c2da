"""The float64 policy reference (tests/policy_reference.py) checked on the CPU: its Philox against the oracle's, its Box-Muller at
the edges of the uniforms, its error bound against a float32 emulation of the packed blob's data flow -- and that the checker
built on it rejects blobs that are subtly wrong."""
import numpy as np
import pytest

import policy_reference as pr
from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, OBS_DIM

KINDS = [ENV_SWING, ENV_TENNIS]


def hidden(kind):
    return (32, 64, 32) if kind == ENV_SWING else (64, 64)


def make_policy(kind, seed, hidden_scale=None, bias_scale=0.0, head_scale=None, log_std=None):
    """ActorCritic on the CPU: SB3's init, or N(0, hidden_scale^2) hidden weights and N(0, bias_scale^2) hidden biases; the action
    head's weights x head_scale (SB3 initialises them near zero)"""
    import torch
    from tennisbot_rl_amd.ppo import build_actor_critic
    torch.manual_seed(seed)
    policy = build_actor_critic(OBS_DIM[kind], ACT_DIM[kind], hidden(kind))
    with torch.no_grad():
        for name, p in policy.named_parameters():
            is_head = name.startswith(("action_net", "value_net."))
            if name == "log_std":
                p.copy_(torch.as_tensor(log_std if log_std is not None else np.linspace(-1.0, 0.2, p.numel()), dtype=torch.float32))
            elif name == "action_net.weight" and head_scale is not None:
                p.mul_(head_scale)
            elif not is_head and hidden_scale is not None:
                p.copy_(torch.randn_like(p) * (hidden_scale if name.endswith("weight") else bias_scale))
    return policy


def layer_table(kind):
    """[(tower, layer, bias offset, fragment offset, tiles, chunks)] of the blob (csrc/tb_policy.hpp, layer_floats)"""
    widths = [OBS_DIM[kind]] + list(hidden(kind)) + [16]
    rows, pos = [], 0
    for tower in range(2):
        for li in range(len(widths) - 1):
            nt, nc = widths[li + 1] // 16, (widths[li] + 3) // 4
            rows.append((tower, li, pos, pos + 16 * nt, nt, nc))
            pos += nt * (16 + nc * 64)
    return rows, pos


def emulate_blob_f32(blob, obs, kind):
    """the kernel's data flow (v_mfma_f32_16x16x4_f32, test_ppo._emulate_blob's operand layout) in float32, one k-ordered chain
    per output that rounds every product and every sum: (mean [n, A], value [n], log_std [A]) as float32"""
    blob = np.asarray(blob, np.float32)
    table, end = layer_table(kind)
    n_obs, n_env = OBS_DIM[kind], obs.shape[0]
    heads = []
    for tower in range(2):
        padded = np.concatenate([np.asarray(obs, np.float32), np.zeros((n_env, -n_obs % 4), np.float32)], 1)
        x = padded.T.reshape(-1, 4, n_env)  # [chunk][g][env] = obs[4 chunk + g]
        layers = [r for r in table if r[0] == tower]
        for _, li, bo, fo, nt, nc in layers:
            bias = blob[bo:bo + 16 * nt].reshape(nt, 16)                # [tile][4 g + r] = output row 4 g + r
            frag = blob[fo:fo + nt * nc * 64].reshape(nt, nc, 4, 16)    # [tile][chunk][g][row]
            y = []
            for t in range(nt):
                acc = np.repeat(bias[t][:, None], n_env, 1)              # [row][env]
                for c in range(nc):
                    for g in range(4):
                        acc = (acc + (frag[t, c, g][:, None] * x[c, g][None, :]).astype(np.float32)).astype(np.float32)
                for r in range(4):
                    y.append(acc[[4 * g + r for g in range(4)]])         # register r: [g][env]
            x = np.stack(y, 0).astype(np.float32)
            if li < len(layers) - 1:
                x = np.tanh(x).astype(np.float32)
        heads.append(x)
    mean = np.stack([heads[0][i & 3, i >> 2] for i in range(ACT_DIM[kind])], -1)
    return mean, heads[1][0, 0], blob[end:end + ACT_DIM[kind]]


def sample_f32(mean, log_std, eps):
    """policy_sample in float32: raw = fmaf(std, eps, mean), logp += fmaf(-eps / 2, eps, -log_std) - ln(2 pi) / 2"""
    f = np.float32
    mean, log_std, eps = mean.astype(f), np.asarray(log_std, f), eps.astype(f)
    std = np.exp(log_std).astype(f)
    raw = (std.astype(np.float64) * eps + mean).astype(f)
    logp = np.zeros(mean.shape[0], f)
    for k in range(mean.shape[1]):
        term = ((f(-0.5) * eps[:, k]).astype(np.float64) * eps[:, k] - log_std[k]).astype(f)
        logp = (logp + (term - f(0.9189385332046727)).astype(f)).astype(f)
    return raw, logp


def noise_f32(seed, env_id, episode, step_count, n_act):
    """policy_noise's Box-Muller in float32 from the same words (numpy's float32 log / sqrt / cos / sin)"""
    f = np.float32
    env_id = np.asarray(env_id, np.uint64)
    seed = int(seed)
    key = (np.uint64(seed & pr.M32), np.uint64((seed >> 32) ^ pr.NOISE_KEY_TAG))
    out = []
    for blk in range((n_act + 3) // 4):
        ctr = (env_id & np.uint64(pr.M32), env_id >> np.uint64(32), np.full_like(env_id, episode), np.full_like(env_id, 4 * step_count + blk))
        u = pr.philox4x32(ctr, key)
        for pair in range(2):
            u1 = ((u[2 * pair] >> np.uint64(8)).astype(f) + f(1)) * f(2.0 ** -24)
            u2 = (u[2 * pair + 1] >> np.uint64(8)).astype(f) * f(2.0 ** -24)
            r, th = np.sqrt(f(-2) * np.log(u1)), f(6.283185307179586) * u2
            out += [r * np.cos(th), r * np.sin(th)]
    return np.stack(out[:n_act], -1)


def check_towers(policy, blob, obs, kind):
    """the GPU tests' tower check, against the float32 emulation: largest |error| / (2 x bound) of mean, value"""
    ref = pr.towers(policy, obs, rounds=2)
    mean, value, log_std = emulate_blob_f32(blob, obs, kind)
    r_mean = pr.assert_within("mean", mean, ref.mean, 2 * ref.mean_bound)
    r_value = pr.assert_within("value", value, ref.value, 2 * ref.value_bound)
    assert np.array_equal(log_std.astype(np.float64), ref.log_std), "log_std"
    return r_mean, r_value, log_std


# ---------------------------------------------------------------- noise
def test_philox_matches_the_oracle_with_high_words_set():
    from oracle import philox4x32 as oracle_philox
    rng = np.random.default_rng(5)
    for _ in range(64):
        ctr = [int(x) for x in rng.integers(0, 2 ** 32, 4, dtype=np.uint64)]
        key = [int(x) for x in rng.integers(0, 2 ** 32, 2, dtype=np.uint64)]
        ctr[1] |= 0x80000001; key[1] |= 0x40000003  # the env id's and the seed's high words
        want = [int(x) for x in oracle_philox(ctr, key)]
        assert list(pr.philox4x32(tuple(ctr), tuple(key))) == want
        got = pr.philox4x32(tuple(np.uint64(c) for c in ctr), tuple(np.uint64(k) for k in key))  # the vectorised form
        assert [int(x) for x in got] == want


def test_policy_noise_key_layout():
    """counter (env_lo, env_hi, episode, 4 step_count + block), key (seed_lo, seed_hi ^ 'POLI'): each piece moves the draw"""
    seed, env = 0x0000_0123_89AB_CDEF, 2 ** 32 + 5
    base = pr.policy_noise(seed, env, 3, 7, 6)
    u = pr.philox4x32((env & pr.M32, env >> 32, 3, 28), (seed & pr.M32, (seed >> 32) ^ 0x504F4C49))
    u2 = pr.philox4x32((env & pr.M32, env >> 32, 3, 29), (seed & pr.M32, (seed >> 32) ^ 0x504F4C49))
    want = [x for a, b in ((u[0], u[1]), (u[2], u[3]), (u2[0], u2[1])) for x in pr.box_muller(a, b)]
    assert np.array_equal(base, np.array(want))
    for other in (pr.policy_noise(seed, env - 2 ** 32, 3, 7, 6), pr.policy_noise(seed, env, 4, 7, 6), pr.policy_noise(seed, env, 3, 8, 6),
                  pr.policy_noise(seed & pr.M32, env, 3, 7, 6), pr.policy_noise(seed + 1, env, 3, 7, 6)):
        assert np.abs(other - base).min() > 0
    # vectorised over envs / episodes / steps: the same as element by element
    envs = np.arange(2 ** 32 - 3, 2 ** 32 + 3, dtype=np.uint64)
    many = pr.policy_noise(seed, envs, np.arange(6), np.arange(6) * 5, 2)
    for j in range(6):
        assert np.array_equal(many[j], pr.policy_noise(seed, int(envs[j]), j, 5 * j, 2))


def test_box_muller_edges():
    r_max = np.sqrt(2 * 24 * np.log(2.0))
    a, b = pr.box_muller(0, 0)          # u1 = 2^-24, u2 = 0: the largest radius, at angle 0
    assert a == pytest.approx(r_max, rel=1e-15) and b == 0.0 and r_max < 5.8
    a, b = pr.box_muller(0xFFFFFFFF, 0x12345678)   # u1 = 1: r = 0 whatever the angle
    assert a == 0.0 and b == 0.0
    a, b = pr.box_muller(0, 0x40000000)  # u2 = 1/4: all of the radius on the sine
    assert abs(a) < 1e-15 * r_max and b == pytest.approx(r_max, rel=1e-15)


def test_noise_tolerance_covers_float32_box_muller():
    seed = 0x0000_00C0_FFEE_0042
    envs = np.arange(2 ** 32 - 4000, 2 ** 32 + 4000, dtype=np.uint64)
    worst = 0.0
    for ep, sc in ((0, 0), (1, 25), (7, 300), (2 ** 31, 999)):
        want = pr.policy_noise(seed, envs, ep, sc, 6)
        got = noise_f32(seed, envs, ep, sc, 6)
        worst = max(worst, pr.assert_within("eps", got, want, pr.EPS_TOL))
    assert worst > 0.005  # (float32 does differ: the tolerance is not vacuous)
    # ... and the words of the extreme uniforms
    for u_a, u_b in ((0, 0), (0, 0xFFFFFFFF), (255, 0x80000000), (0xFFFFFFFF, 0)):
        want = np.array(pr.box_muller(u_a, u_b))
        f = np.float32
        u1 = (f(u_a >> 8) + f(1)) * f(2.0 ** -24); u2 = f(u_b >> 8) * f(2.0 ** -24)
        r, th = np.sqrt(f(-2) * np.log(u1)), f(6.283185307179586) * u2
        pr.assert_within("eps edge", np.array([r * np.cos(th), r * np.sin(th)]), want, pr.EPS_TOL)


# ---------------------------------------------------------------- towers
CASES = [  # name, make_policy keywords, observation scale
    ("sb3_head30", dict(head_scale=30.0), 1.0),
    ("sb3_head30_big_obs", dict(head_scale=30.0), 1e3),
    ("random_0.3", dict(hidden_scale=0.3, bias_scale=0.3, head_scale=30.0), 3.0),
    ("saturating", dict(hidden_scale=2.0, bias_scale=1.0, head_scale=30.0), 10.0),
    ("tiny", dict(hidden_scale=1e-5, bias_scale=1e-4), 10.0),
    ("tiny_obs", dict(hidden_scale=0.3, bias_scale=0.0), 1e-6),
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,kw,scale", CASES, ids=[c[0] for c in CASES])
def test_bound_covers_float32_emulation_of_the_blob(kind, name, kw, scale):
    from tennisbot_rl_amd.ppo import pack_policy
    policy = make_policy(kind, 3, **kw)
    blob = pack_policy(policy).numpy()
    rng = np.random.default_rng(1)
    obs = (rng.normal(size=(512, OBS_DIM[kind])) * scale).astype(np.float32)
    obs[:16] *= np.where(np.arange(16) % 2, -1.0, 1.0)[:, None].astype(np.float32)   # mixed signs in one 16-env slice
    obs[16] = 0.0
    obs[17] = np.float32(1e-40)                                                       # subnormal
    ref = pr.towers(policy, obs, rounds=2)
    mean, value, log_std = emulate_blob_f32(blob, obs, kind)
    r_mean = pr.assert_within("mean", mean, ref.mean, ref.mean_bound)
    r_value = pr.assert_within("value", value, ref.value, ref.value_bound)
    assert np.array_equal(log_std.astype(np.float64), ref.log_std)
    assert max(r_mean, r_value) < 1.0 and np.all(np.isfinite(ref.mean_bound))


@pytest.mark.parametrize("kind", KINDS)
def test_tower_tolerance_under_sb3_init_on_reset_observations(kind):
    """SB3's init with the action head x 30 (test_gpu_policy.make) on the oracle's reset observations. The worst-case bound is
    looser than the fixed 2e-5 of test_gpu_policy (measured: mean 1.1e-4 / 4.5e-5, value 2.8e-4 / 1.4e-4, SwingRacket /
    Tennisbot): the first layer's 8e-6 (observations up to 12) is carried through |W| row sums of 5.5 and 9.6 with no
    cancellation. So where the fixed tolerance applies, tower_tol keeps it: the new check is never looser than the old one. And
    the bound stays far from vacuous."""
    from oracle import OracleBatch
    from tennisbot_rl_amd.params import F_AUTO_RESET, F_DEFAULT, default_params
    policy = make_policy(kind, 5, head_scale=30.0)
    ref = OracleBatch(default_params(flags=F_DEFAULT | F_AUTO_RESET), kind, 2048, seed=5, precision="f32")
    t = pr.towers(policy, ref.reset())
    assert 2 * t.mean_bound.max() < 1e-3 and 2 * t.value_bound.max() < 1e-3, (t.mean_bound.max(), t.value_bound.max())
    for b in (t.mean_bound, t.value_bound):
        assert np.all(pr.tower_tol(b, pr.FIXED_TOL) <= pr.FIXED_TOL) and np.array_equal(pr.tower_tol(b), 2 * b)
        assert np.array_equal(pr.tower_tol(b * 1e-3, pr.FIXED_TOL), 2e-3 * b)


@pytest.mark.parametrize("kind", KINDS)
def test_infinite_and_nan_observations(kind):
    """an infinite input saturates the first layer exactly (finite outputs, bound from there on); NaN stays NaN"""
    from tennisbot_rl_amd.ppo import pack_policy
    policy = make_policy(kind, 2, head_scale=30.0)
    obs = np.random.default_rng(0).normal(size=(32, OBS_DIM[kind])).astype(np.float32)
    obs[3, 0], obs[4, 1], obs[5, 2] = np.inf, -np.inf, np.nan
    t = pr.towers(policy, obs)
    assert np.all(np.isfinite(t.mean[[3, 4]])) and np.all(np.isfinite(t.mean_bound[[3, 4]])) and np.all(np.isnan(t.mean[5]))
    mean, value, _ = emulate_blob_f32(pack_policy(policy).numpy(), obs, kind)
    pr.assert_within("mean", mean, t.mean, pr.towers(policy, obs, rounds=2).mean_bound)
    assert np.isnan(value[5]) and np.all(np.isfinite(np.delete(value, 5)))
    raw, act, _ = pr.sample(t.mean, t.log_std, np.zeros_like(t.mean))
    assert np.all(np.isnan(act[5])) and np.all(np.abs(np.delete(act, 5, 0)) <= 1.0)


@pytest.mark.parametrize("kind", KINDS)
def test_sampling_tolerances_cover_float32_sampling(kind):
    A = ACT_DIM[kind]
    rng = np.random.default_rng(2)
    n = 4096
    mean = rng.normal(size=(n, A)) * 3
    for log_std in (np.full(A, -5.0), np.full(A, 2.0), np.linspace(-1.0, 0.2, A)):
        log_std = log_std.astype(np.float32).astype(np.float64)
        eps = pr.policy_noise(77, np.arange(n), 0, 3, A)
        eps32 = noise_f32(77, np.arange(n, dtype=np.uint64), 0, 3, A)
        raw_ref, act_ref, logp_ref = pr.sample(mean.astype(np.float32).astype(np.float64), log_std, eps)
        raw, logp = sample_f32(mean, log_std, eps32)
        pr.assert_within("raw", raw, raw_ref, pr.raw_tol(np.zeros_like(mean), log_std, eps, mean))
        pr.assert_within("logp", logp, logp_ref, pr.logp_tol(log_std, eps))


def test_episode_keys_follow_the_done_flags():
    dones = np.zeros((30, 3), np.uint8)
    dones[25, 0] = 1; dones[10, 1] = 1; dones[11, 1] = 1
    ep, sc, e_end, s_end = pr.episode_keys([4, 0, 9], [0, 3, 990], dones)
    assert list(ep[:, 0][[0, 25, 26]]) == [4, 4, 5] and list(sc[:, 0][[0, 25, 26, 29]]) == [0, 25, 0, 3]
    assert list(ep[:, 1][[10, 11, 12]]) == [0, 1, 2] and list(sc[:, 1][[10, 11, 12]]) == [13, 0, 0]
    assert list(e_end) == [5, 2, 9] and list(s_end) == [4, 18, 1020]


# ---------------------------------------------------------------- teeth
def _corrupt(kind, blob, what):
    table, end = layer_table(kind)
    b = blob.copy()
    pi = [r for r in table if r[0] == 0]
    if what == "swapped_k_chunks":            # two k-chunks of the pi tower's second hidden layer trade places
        _, _, bo, fo, nt, nc = pi[1]
        c0, c1 = fo + 0 * 64, fo + 1 * 64
        b[c0:c0 + 64], b[c1:c1 + 64] = blob[c1:c1 + 64], blob[c0:c0 + 64]
    elif what == "moved_bias_tile":           # the first bias tile of the pi tower's second hidden layer, one tile on
        _, _, bo, fo, nt, nc = pi[1]
        b[bo:bo + 16], b[bo + 16:bo + 32] = blob[bo + 16:bo + 32], blob[bo:bo + 16]
    elif what == "shifted_head_lane_group":   # lane group 0 of the action head's fragments one lane over
        _, _, bo, fo, nt, nc = pi[-1]
        for c in range(nc):
            s = fo + c * 64
            b[s:s + 16] = np.roll(blob[s:s + 16], 1)
    elif what == "log_std_off_by_one":
        b[end:end + ACT_DIM[kind]] = np.roll(blob[end:end + ACT_DIM[kind]], 1)
    return b


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("what", ["swapped_k_chunks", "moved_bias_tile", "shifted_head_lane_group", "log_std_off_by_one"])
def test_checker_rejects_corrupted_blobs(kind, what):
    """the checks the GPU tests make -- towers within 2 x bound, raw / logp within their tolerances -- fail on blobs that are
    wrong in ways a packer or a kernel could be: the clean blob passes the same checks"""
    from tennisbot_rl_amd.ppo import pack_policy
    A = ACT_DIM[kind]
    policy = make_policy(kind, 8, hidden_scale=0.3, bias_scale=0.3, head_scale=30.0, log_std=np.linspace(-1.0, 0.5, A))
    blob = pack_policy(policy).numpy()
    obs = np.random.default_rng(4).normal(size=(64, OBS_DIM[kind])).astype(np.float32) * 2
    ref = pr.towers(policy, obs, rounds=2)
    eps = pr.policy_noise(99, np.arange(64), 0, 0, A)
    eps32 = noise_f32(99, np.arange(64, dtype=np.uint64), 0, 0, A)
    raw_ref, _, logp_ref = pr.sample(ref.mean, ref.log_std, eps)

    def check(bl):
        mean, value, log_std = emulate_blob_f32(bl, obs, kind)
        pr.assert_within("mean", mean, ref.mean, 2 * ref.mean_bound)
        pr.assert_within("value", value, ref.value, 2 * ref.value_bound)
        raw, logp = sample_f32(mean, log_std, eps32)
        pr.assert_within("raw", raw, raw_ref, pr.raw_tol(ref.mean_bound, ref.log_std, eps, ref.mean))
        pr.assert_within("logp", logp, logp_ref, pr.logp_tol(ref.log_std, eps))

    check(blob)
    with pytest.raises(AssertionError):
        check(_corrupt(kind, blob, what))
