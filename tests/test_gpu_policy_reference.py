"""The policy half of the fused kernels (tb_policy_step, tb_policy_rollout; csrc/tb_policy.hpp) against the float64 reference of
tests/policy_reference.py, output by output and element by element: action means and values within twice their forward error
bound, raw actions within the bound of mean + std * eps with eps drawn from the reference's own Philox / Box-Muller, logp within
the tolerance that follows, actions equal to raw clipped to [-1, 1] (NaN kept) bit for bit. Every step's noise key -- episode and
step count -- is derived from the state before the first step and the done flags, and that derivation is checked against the
state after the last step."""
import os

import numpy as np
import pytest

import policy_reference as pr
from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, OBS_DIM, STATE_WORDS

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_swing_policy.npz")
NOISE_SEED = 0x0000_0042_DEAD_BEEF  # a non-zero high word: the key's second word
ID_CARRY = 2 ** 32 - 300            # env_id_base with n = 777: the env ids straddle the carry into the high word
N_STEP = (1, 15, 16, 17, 63, 65, 777, 4096)
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
        print("policy reference: largest |error| / %s = %.3g" % (k, RATIOS[k]))


def check(name, got, want, tol, bound=None):
    r = pr.assert_within(name, got, want, tol)
    RATIOS[name + " tolerance"] = max(RATIOS.get(name + " tolerance", 0.0), r)
    if bound is not None:
        RATIOS[name + " bound"] = max(RATIOS.get(name + " bound", 0.0), pr.excess(got, want, bound)[0])


def make_policy(torch, kind, name):
    """weight sets: sb3 (SB3's init, action head x 30), golden (the reference's trained SwingRacket policy), saturating (N(0, 2^2)
    hidden weights), tiny (pre-activations around 1e-4), log_std (sb3 with log_std at -5 and +2)"""
    from tennisbot_rl_amd.ppo import SWING_DEFAULTS, TENNIS_DEFAULTS, build_actor_critic
    torch.manual_seed(21)
    A = ACT_DIM[kind]
    policy = build_actor_critic(OBS_DIM[kind], A, tuple((SWING_DEFAULTS if kind == ENV_SWING else TENNIS_DEFAULTS)["net_arch"]))
    if name == "golden":
        assert kind == ENV_SWING
        return policy.load_sb3_arrays(dict(np.load(GOLD))).to("cuda:0")
    with torch.no_grad():
        policy.action_net.weight.mul_(30.0)
        policy.log_std.copy_(torch.linspace(-1.0, 0.2, A) if name != "log_std" else torch.tensor([-5.0, 2.0] * (A // 2)))
        for body in (policy.policy_net, policy.value_net_body):
            lin = [m for m in body if isinstance(m, torch.nn.Linear)]
            for j, m in enumerate(lin):
                if name == "saturating":
                    m.weight.normal_(0.0, 2.0); m.bias.normal_(0.0, 1.0)
                elif name == "tiny":  # observations are up to ~12: the first layer's weights ~1e-5, the later ones ~1 / sqrt(in)
                    m.weight.normal_(0.0, 1e-5 if j == 0 else m.in_features ** -0.5); m.bias.normal_(0.0, 1e-4)
    return policy.to("cuda:0")


WEIGHTS = [(ENV_SWING, w) for w in ("sb3", "golden", "saturating", "tiny", "log_std")] + [(ENV_TENNIS, w) for w in ("sb3", "saturating", "tiny", "log_std")]


def crafted(obs):
    """obs_in with crafted rows: by i % 8 -- 1 zeros, 2 +1e3, 3 -1e3, 4 subnormals of both signs; the other rows are the env's own,
    their components' signs alternated in every second group of 8 (mixed signs inside each 16-env slice). Returns obs, natural"""
    o = obs.copy()
    n, O = o.shape
    i = np.arange(n)
    alt = np.where(np.arange(O) % 2, -1.0, 1.0).astype(np.float32)
    o[i % 8 == 1] = 0.0
    o[i % 8 == 2] = 1e3
    o[i % 8 == 3] = -1e3
    o[i % 8 == 4] = np.float32(1e-40) * alt
    natural = np.isin(i % 8, (0, 5, 6, 7))
    flip = natural & ((i // 8) % 2 == 1)
    o[flip] *= alt
    return o, natural & ~flip


def keys_of(env):
    w, _ = env.get_state_words()
    w = w.cpu().numpy()
    nw = STATE_WORDS[env.kind]
    return w[nw - 1].view(np.uint32).astype(np.int64), w[nw - 2].astype(np.int64)  # episode, step_count


def check_outputs(tag, ref, eps, act, raw, logp, value, deterministic, cap_rows=None):
    """one step's outputs (or T steps', flattened) against the reference; eps: the reference noise [rows, A]"""
    mean_tol, value_tol = pr.tower_tol(ref.mean_bound), pr.tower_tol(ref.value_bound)
    if cap_rows is not None:  # SB3's init on the envs' own observations: test_gpu_policy's fixed 2e-5 where it is the tighter one
        mean_tol[cap_rows] = pr.tower_tol(ref.mean_bound[cap_rows], pr.FIXED_TOL)
        value_tol[cap_rows] = pr.tower_tol(ref.value_bound[cap_rows], pr.FIXED_TOL)
    check("value", value, ref.value, value_tol, ref.value_bound)
    if deterministic:
        eps = np.zeros_like(ref.mean)
        check("mean", raw, ref.mean, mean_tol, ref.mean_bound)
    raw_ref, _, logp_ref = pr.sample(ref.mean, ref.log_std, eps)
    check("raw", raw, raw_ref, pr.raw_tol(mean_tol / 2, ref.log_std, eps, ref.mean))  # (raw_tol takes twice the mean's bound)
    check("logp", logp, logp_ref, pr.logp_tol(ref.log_std, eps))
    want_act = pr.clip_action(raw.astype(np.float32))
    assert np.array_equal(act.view(np.uint32), want_act.view(np.uint32)), "%s: actions are not raw clipped to [-1, 1] bit for bit" % tag


@pytest.mark.parametrize("kind,wname", WEIGHTS, ids=["%s-%s" % ("swing" if k == ENV_SWING else "tennis", w) for k, w in WEIGHTS])
def test_policy_step_matches_the_float64_reference(torch, kind, wname):
    """tb_policy_step at batch sizes around the 16-env slice and the 64-env workgroup, on crafted observations, deterministic and
    stochastic: every output of every env"""
    from tennisbot_rl_amd.ppo import pack_policy
    from tennisbot_rl_amd.stepper import BatchedEnv
    policy = make_policy(torch, kind, wname)
    blob = pack_policy(policy)
    A = ACT_DIM[kind]
    for n in N_STEP:
        base = ID_CARRY if n == 777 else 0
        det = BatchedEnv(kind, n, device="cuda:0", seed=13, env_id_base=base)
        sto = BatchedEnv(kind, n, device="cuda:0", seed=13, env_id_base=base)
        obs = det.reset()
        sto.reset()
        obs_in, natural = crafted(obs.cpu().numpy())
        episode, step_count = keys_of(sto)
        x = torch.from_numpy(obs_in).to("cuda:0")
        _, (act_d, raw_d, logp_d, val_d) = det.policy_step(blob, x, seed=NOISE_SEED, deterministic=True)
        _, (act_s, raw_s, logp_s, val_s) = sto.policy_step(blob, x, seed=NOISE_SEED)
        torch.cuda.synchronize()
        ref = pr.towers(policy, obs_in)
        cap = natural if wname == "sb3" else None
        eps = pr.policy_noise(NOISE_SEED, base + np.arange(n, dtype=np.uint64), episode, step_count, A)
        tag = "n=%d %s" % (n, wname)
        h = lambda t: t.cpu().numpy()
        check_outputs(tag + " deterministic", ref, None, h(act_d), h(raw_d), h(logp_d), h(val_d), True, cap)
        check_outputs(tag + " stochastic", ref, eps, h(act_s), h(raw_s), h(logp_s), h(val_s), False, cap)
        assert np.array_equal(h(val_d).view(np.uint32), h(val_s).view(np.uint32)), tag  # the value does not depend on the noise
        ep1, sc1 = keys_of(sto)
        assert np.array_equal(ep1, episode) and np.array_equal(sc1, step_count + 1), tag  # one step inside the episode
        det.close(); sto.close()


ROLLOUTS = [  # kind, n, policy_slices, T, lead steps, weights, deterministic
    (ENV_SWING, 777, 0, 78, 9, "golden", False),
    (ENV_SWING, 777, 0, 60, 9, "golden", True),
    (ENV_SWING, 65, 1, 78, 3, "sb3", False),
    (ENV_SWING, 63, 3, 60, 5, "saturating", False),
    (ENV_SWING, 17, 1, 60, 0, "tiny", True),
    (ENV_SWING, 1000, 3, 60, 2, "log_std", False),
    (ENV_SWING, 5000, 0, 78, 0, "sb3", False),    # auto: 48-env workgroups above 4096 envs
    (ENV_TENNIS, 777, 0, 900, 3, "sb3", False),
    (ENV_TENNIS, 63, 1, 900, 0, "saturating", False),
    (ENV_TENNIS, 15, 3, 900, 0, "sb3", True),
    (ENV_TENNIS, 16, 1, 900, 0, "log_std", False),
]


@pytest.mark.parametrize("kind,n,slices,T,lead,wname,deterministic", ROLLOUTS)
def test_policy_rollout_matches_the_float64_reference(torch, kind, n, slices, T, lead, wname, deterministic):
    """tb_policy_rollout (16- and 48-env forms) on the observations it consumed, [obs_in, obs[:-1]], across episode ends:
    SwingRacket >= 2 per env (the parking step and its fast-forward included), Tennisbot 900 steps with curriculum-sized rackets"""
    from tennisbot_rl_amd.params import default_params
    from tennisbot_rl_amd.ppo import pack_policy
    from tennisbot_rl_amd.stepper import BatchedEnv
    policy = make_policy(torch, kind, wname)
    blob = pack_policy(policy)
    A = ACT_DIM[kind]
    base = ID_CARRY if n == 777 else 0
    swing = kind == ENV_SWING
    params = None if swing else default_params(racket_scale=3.0)
    env = BatchedEnv(kind, n, device="cuda:0", seed=8, env_id_base=base, pipeline=swing, track_terminal_obs=False, params=params,
                     options=dict(policy_slices=slices))
    o = env.reset()
    for _ in range(lead):
        (o, _, _), _ = env.policy_step(blob, o, seed=NOISE_SEED, deterministic=deterministic)
    env.flush()
    episode0, step_count0 = keys_of(env)
    (obs, rew, done), (act, raw, logp, value) = env.policy_rollout(blob, o, T, seed=NOISE_SEED, deterministic=deterministic)
    env.flush()
    torch.cuda.synchronize()
    done_h = done.cpu().numpy()
    ep, sc, ep_end, sc_end = pr.episode_keys(episode0, step_count0, done_h)
    ep1, sc1 = keys_of(env)
    assert np.array_equal(ep1, ep_end) and np.array_equal(sc1, sc_end), "the noise keys derived from the done flags are not the state's"
    if swing:
        assert done_h.sum(0).min() >= 2
    elif n > 100:
        assert done_h.sum() > 0
    consumed = torch.cat([o[None], obs[:-1]]).cpu().numpy().reshape(T * n, -1)
    ids = base + np.arange(n, dtype=np.uint64)
    flat = lambda t: t.cpu().numpy().reshape(T * n, *t.shape[2:])
    act_h, raw_h, logp_h, value_h = flat(act), flat(raw), flat(logp), flat(value)
    chunk = max(1, 200000 // n)  # the reference in slices of steps: bounded host memory
    for t0 in range(0, T, chunk):
        rows = slice(t0 * n, min(T, t0 + chunk) * n)
        ref = pr.towers(policy, consumed[rows])
        eps = None if deterministic else pr.policy_noise(NOISE_SEED, np.tile(ids, min(T, t0 + chunk) - t0), ep[t0:t0 + chunk].ravel(),
                                                         sc[t0:t0 + chunk].ravel(), A)
        check_outputs("steps %d.. of %d" % (t0, T), ref, eps, act_h[rows], raw_h[rows], logp_h[rows], value_h[rows], deterministic)
    c = env.counters()
    assert c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0, c
    env.close()


def _bits_equal(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    both_nan = np.isnan(a) & np.isnan(b) if a.dtype.kind == "f" else np.zeros(a.shape, bool)
    return bool(np.all(both_nan | (a.view(np.uint8 if a.dtype.itemsize == 1 else np.uint32) == b.view(np.uint8 if b.dtype.itemsize == 1 else np.uint32))))


@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_nonfinite_observation_stays_in_its_env(torch, kind, bad):
    """NaN, then +inf, in one env's obs_in inside a full 16-env slice: every other env's outputs bit-identical to the clean run; a
    NaN makes that env's mean and value NaN and its action NaN, as torch's clamp keeps it (a diverged policy then shows in
    nonfinite_states instead of stepping the env with -1); +inf saturates the first layer exactly and matches the reference. The
    env half still equals tb_step driven by the reported actions. Both kernels."""
    from tennisbot_rl_amd.ppo import pack_policy
    from tennisbot_rl_amd.stepper import BatchedEnv
    policy = make_policy(torch, kind, "sb3")
    blob = pack_policy(policy)
    n, k, A = 64, 5, ACT_DIM[kind]
    value = float("nan") if bad == "nan" else float("inf")
    swing = kind == ENV_SWING
    for rollout in (False, True):
        mk = lambda: BatchedEnv(kind, n, device="cuda:0", seed=4, pipeline=rollout and swing, track_terminal_obs=False)
        clean, env, twin = mk(), mk(), mk()
        obs = clean.reset(); env.reset(); twin.reset()
        obs_bad = obs.clone()
        obs_bad[k, 1] = value
        episode, step_count = keys_of(env)
        if rollout:
            (o1, r1, d1), p1 = clean.policy_rollout(blob, obs, 2, seed=NOISE_SEED)
            (o2, r2, d2), p2 = env.policy_rollout(blob, obs_bad, 2, seed=NOISE_SEED)
        else:
            (o1, r1, d1), p1 = clean.policy_step(blob, obs, seed=NOISE_SEED)
            (o2, r2, d2), p2 = env.policy_step(blob, obs_bad, seed=NOISE_SEED)
        env.flush(); clean.flush()
        torch.cuda.synchronize()
        others = [j for j in range(n) if j != k]
        for name, x, y in zip(("obs", "reward", "done", "actions", "raw", "logp", "value"), (o1, r1, d1) + tuple(p1), (o2, r2, d2) + tuple(p2)):
            assert torch.equal(x.index_select(int(rollout), torch.tensor(others, device=x.device)), y.index_select(int(rollout), torch.tensor(others, device=y.device))), \
                "%s of the other envs changed (rollout=%s)" % (name, rollout)
        act, raw, logp, val = (t[0] if rollout else t for t in p2)
        assert _bits_equal(act, raw.clamp(-1.0, 1.0)), "actions are not torch's clamp of raw (rollout=%s): %s from %s" % (rollout, act[k], raw[k])
        ref = pr.towers(policy, obs_bad.cpu().numpy())
        eps = pr.policy_noise(NOISE_SEED, np.arange(n, dtype=np.uint64), episode, step_count, A)
        if bad == "nan":
            assert bool(torch.isnan(val[k])) and bool(torch.isnan(raw[k]).all()) and bool(torch.isnan(act[k]).all())
            assert bool(torch.isfinite(logp[k]))  # (logp depends on the noise only)
        else:
            check_outputs("+inf row", pr.Towers(ref.mean[[k]], ref.value[[k]], ref.mean_bound[[k]], ref.value_bound[[k]], ref.log_std),
                          eps[[k]], act[[k]].cpu().numpy(), raw[[k]].cpu().numpy(), logp[[k]].cpu().numpy(), val[[k]].cpu().numpy(), False)
        if not rollout:
            o3, r3, d3 = twin.step(act.contiguous())
            assert _bits_equal(o3, o2) and _bits_equal(r3, r2) and _bits_equal(d3, d2), "the env half differs from tb_step"
        bad_states = env.counters()["nonfinite_states"]
        assert (bad_states > 0) == (bad == "nan"), env.counters()
        for e in (clean, env, twin):
            e.close()


@pytest.mark.parametrize("env_id,num_envs,n_steps,rollout_launch", [("SwingRacket-v0", 1024, 52, True), ("SwingRacket-v0", 1024, 52, False),
                                                                     ("Tennisbot-v0", 512, 64, True)])
def test_trainer_buffers_match_the_reference_across_replays_and_weight_changes(torch, env_id, num_envs, n_steps, rollout_launch):
    """PPOTrainer's collect, eager, captured and replayed: the stored values match the reference on obs_seq (obs_seq[k] is what
    step k acted on), the raw actions and logps match it under the trainer's noise seed and env ids. Then the weights change in
    place and the next collect -- a replay of the SAME graph -- matches the new weights, not the old ones."""
    from tennisbot_rl_amd.ppo import PPOTrainer
    tr = PPOTrainer(env_id, num_envs=num_envs, n_steps=n_steps, device="cuda:0", seed=3, rollout_launch=rollout_launch)
    A, n = tr.env.act_dim, num_envs
    ids = tr.env.env_id_base + np.arange(n, dtype=np.uint64)

    def collect_and_check(tag):
        ep0, sc0 = keys_of(tr.env)
        tr.collect()
        torch.cuda.synchronize()
        dones = tr.buf.dones.cpu().numpy()
        ep, sc, ep_end, sc_end = pr.episode_keys(ep0, sc0, dones)
        ep1, sc1 = keys_of(tr.env)
        assert np.array_equal(ep1, ep_end) and np.array_equal(sc1, sc_end), tag
        ref = pr.towers(tr.policy, tr.obs_seq.cpu().numpy().reshape(n_steps * n, -1))
        eps = pr.policy_noise(tr.noise_seed, np.tile(ids, n_steps), ep.ravel(), sc.ravel(), A)
        raw = tr._raw_actions.cpu().numpy().reshape(-1, A)
        check_outputs(tag, ref, eps, tr.buf.actions.cpu().numpy().reshape(-1, A), raw, tr.logps.cpu().numpy().ravel(),
                      tr.values.cpu().numpy().ravel(), False)
        return ref

    collect_and_check("eager + capture")
    g = tr._graph
    assert g is not None
    collect_and_check("replay 1")
    collect_and_check("replay 2")
    assert tr._graph is g
    old_weights = pr.state_dict_arrays(tr.policy)
    with torch.no_grad():
        gen = torch.Generator(device=tr.device).manual_seed(17)
        for p in tr.policy.parameters():
            p.add_(torch.randn(p.shape, device=tr.device, generator=gen) * 0.05)
    collect_and_check("replay after the weights changed")
    assert tr._graph is g, "the collect after the weight change captured a new graph instead of replaying"
    # ... and the old weights do not explain that collect's values
    old = pr.towers(old_weights, tr.obs_seq.cpu().numpy().reshape(n_steps * n, -1))
    assert pr.excess(tr.values.cpu().numpy().ravel(), old.value, pr.tower_tol(old.value_bound))[0] > 100
