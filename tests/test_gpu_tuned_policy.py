"""The tuned network inside the fused policy kernels (tb_policy_step_net / tb_policy_rollout_net with TB_NET_TUNED; TunedTrunk /
TunedTower in csrc/tb_policy.hpp) against the float64 reference of tests/tuned_reference.py, with the checks of
test_gpu_policy_reference.py: action means and values within twice their forward error bound, raw actions and logp within the
tolerances that follow from it with the reference's own Philox / Box-Muller noise, actions equal to raw clipped to [-1, 1] bit for
bit, the value independent of the noise, the noise keys derived from the done flags. Then: the one-step and the rollout forms
agree bit for bit, and the default network on a handle that has run the tuned one gives the bits a fresh handle gives."""
import numpy as np
import pytest

import policy_reference as pr
import tuned_reference as tref
from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, NET_DEFAULT, NET_TUNED
from test_gpu_policy_reference import ID_CARRY, NOISE_SEED, _bits_equal, check_outputs, crafted, keys_of
from test_tuned_reference import WEIGHT_SETS, make_policy

pytestmark = pytest.mark.gpu

N_STEP = (1, 15, 16, 17, 63, 65, 777)
A = ACT_DIM[ENV_TENNIS]
LEAD = 560   # agent steps before a checked rollout: Tennisbot episodes under these policies end from ~400 steps on, at ragged times


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def packed(torch, wname):
    from tennisbot_rl_amd.ppo import pack_policy
    policy = make_policy(wname).to("cuda:0")
    blob = pack_policy(policy)
    assert blob.numel() == tref.blob_floats()
    return policy, blob


@pytest.mark.parametrize("wname", WEIGHT_SETS)
def test_policy_step_matches_the_float64_reference(torch, wname):
    """tb_policy_step_net at batch sizes around the 16-env slice and the 64-env workgroup, on crafted observations (zeros, +-1e3,
    subnormals, mixed signs), deterministic and stochastic: every output of every env"""
    from tennisbot_rl_amd.stepper import BatchedEnv
    policy, blob = packed(torch, wname)
    for n in N_STEP:
        base = ID_CARRY if n == 777 else 0
        det = BatchedEnv(ENV_TENNIS, n, device="cuda:0", seed=13, env_id_base=base)
        sto = BatchedEnv(ENV_TENNIS, n, device="cuda:0", seed=13, env_id_base=base)
        obs = det.reset()
        sto.reset()
        obs_in, _ = crafted(obs.cpu().numpy())
        episode, step_count = keys_of(sto)
        x = torch.from_numpy(obs_in).to("cuda:0")
        _, (act_d, raw_d, logp_d, val_d) = det.policy_step(blob, x, seed=NOISE_SEED, deterministic=True, net=NET_TUNED)
        _, (act_s, raw_s, logp_s, val_s) = sto.policy_step(blob, x, seed=NOISE_SEED, net=NET_TUNED)
        torch.cuda.synchronize()
        ref = tref.towers(policy, obs_in)
        eps = pr.policy_noise(NOISE_SEED, base + np.arange(n, dtype=np.uint64), episode, step_count, A)
        tag = "tuned n=%d %s" % (n, wname)
        h = lambda t: t.cpu().numpy()  # noqa: E731
        check_outputs(tag + " deterministic", ref, None, h(act_d), h(raw_d), h(logp_d), h(val_d), True)
        check_outputs(tag + " stochastic", ref, eps, h(act_s), h(raw_s), h(logp_s), h(val_s), False)
        assert np.array_equal(h(val_d).view(np.uint32), h(val_s).view(np.uint32)), tag  # the value does not depend on the noise
        if wname == "dead":                                                             # ... and not on anything the dead feature unit reads
            assert np.all(ref.feature[:, 1] == 0.0)
        ep1, sc1 = keys_of(sto)
        assert np.array_equal(ep1, episode) and np.array_equal(sc1, step_count + 1), tag
        det.close(); sto.close()


ROLLOUTS = [  # n, policy_slices, T, weights, deterministic
    (777, 0, 60, "sb3", False),
    (63, 1, 60, "sb3", False),
    (15, 3, 60, "dead", True),
    (16, 1, 60, "log_std", False),
    (65, 3, 60, "saturating", False),   # (actions pinned at +-1: its episodes outlast the window)
]


@pytest.mark.parametrize("n,slices,T,wname,deterministic", ROLLOUTS)
def test_policy_rollout_matches_the_float64_reference(torch, n, slices, T, wname, deterministic):
    """tb_policy_rollout_net (16- and 48-env forms) on the observations it consumed, [obs_in, obs[:-1]]: 60 steps late enough in the
    episodes (LEAD steps of the same kernel first) that episodes end, restart and shoot their ball inside the checked window"""
    from tennisbot_rl_amd.params import default_params
    from tennisbot_rl_amd.stepper import BatchedEnv
    policy, blob = packed(torch, wname)
    base = ID_CARRY if n == 777 else 0
    env = BatchedEnv(ENV_TENNIS, n, device="cuda:0", seed=8, env_id_base=base, track_terminal_obs=False, params=default_params(racket_scale=3.0),
                     options=dict(policy_slices=slices))
    o = env.reset()
    (lead_obs, _, lead_done), _ = env.policy_rollout(blob, o, LEAD, seed=NOISE_SEED, deterministic=deterministic, net=NET_TUNED)
    o = lead_obs[-1].clone()
    episode0, step_count0 = keys_of(env)
    (obs, rew, done), (act, raw, logp, value) = env.policy_rollout(blob, o, T, seed=NOISE_SEED, deterministic=deterministic, net=NET_TUNED)
    torch.cuda.synchronize()
    done_h = done.cpu().numpy()
    ep, sc, ep_end, sc_end = pr.episode_keys(episode0, step_count0, done_h)
    ep1, sc1 = keys_of(env)
    assert np.array_equal(ep1, ep_end) and np.array_equal(sc1, sc_end), "the noise keys derived from the done flags are not the state's"
    print("tuned rollout n=%d: %d episode ends in the lead, %d in the checked window" % (n, int(lead_done.sum()), int(done_h.sum())))
    if n > 60 and wname == "sb3":
        assert done_h.sum() > 0 and (sc[1:][done_h[:-1] != 0] == 0).all()   # episodes ended inside, and their envs went on from step 0
    consumed = torch.cat([o[None], obs[:-1]]).cpu().numpy().reshape(T * n, -1)
    ids = base + np.arange(n, dtype=np.uint64)
    flat = lambda t: t.cpu().numpy().reshape(T * n, *t.shape[2:])  # noqa: E731
    ref = tref.towers(policy, consumed)
    eps = None if deterministic else pr.policy_noise(NOISE_SEED, np.tile(ids, T), ep.ravel(), sc.ravel(), A)
    check_outputs("tuned rollout n=%d" % n, ref, eps, flat(act), flat(raw), flat(logp), flat(value), deterministic)
    c = env.counters()
    assert c["nonfinite_states"] == 0 and c["lockstep_violations"] == 0, c
    env.close()


@pytest.mark.parametrize("n,slices", [(65, 1), (100, 3)])
def test_one_step_and_rollout_forms_agree_bit_for_bit(torch, n, slices):
    from tennisbot_rl_amd.stepper import BatchedEnv
    _, blob = packed(torch, "sb3")
    T = 40
    mk = lambda: BatchedEnv(ENV_TENNIS, n, device="cuda:0", seed=5, track_terminal_obs=False, options=dict(policy_slices=slices))  # noqa: E731
    a, b = mk(), mk()
    o = a.reset(); b.reset()
    (obs, rew, done), pol = a.policy_rollout(blob, o, T, seed=NOISE_SEED, net=NET_TUNED)
    cur = o
    for t in range(T):
        (o1, r1, d1), p1 = b.policy_step(blob, cur, seed=NOISE_SEED, net=NET_TUNED)
        for name, x, y in zip(("obs", "reward", "done", "actions", "raw", "logp", "value"), (obs[t], rew[t], done[t]) + tuple(p[t] for p in pol), (o1, r1, d1) + tuple(p1)):
            assert _bits_equal(x, y), "step %d: %s differs between tb_policy_rollout_net and tb_policy_step_net" % (t, name)
        cur = o1
    wa, da = a.get_state_words(); wb, db = b.get_state_words()
    assert torch.equal(wa, wb) and torch.equal(da, db)
    a.close(); b.close()


def test_the_default_net_after_the_tuned_one_is_a_fresh_handle_s(torch):
    """the net is an argument of the call, not a state of the handle: TB_NET_DEFAULT after TB_NET_TUNED on one handle gives the bits
    a handle that never saw the tuned net gives, in both forms; and the pairs the kernels are not built for are refused"""
    from tennisbot_rl_amd.ppo import TENNIS_DEFAULTS, build_actor_critic, pack_policy
    from tennisbot_rl_amd.stepper import BatchedEnv, StepperError
    _, tuned_blob = packed(torch, "sb3")
    torch.manual_seed(2)
    default_blob = pack_policy(build_actor_critic(12, A, tuple(TENNIS_DEFAULTS["net_arch"])).to("cuda:0"))
    n = 65
    mk = lambda kind=ENV_TENNIS: BatchedEnv(kind, n, device="cuda:0", seed=6, track_terminal_obs=False)  # noqa: E731
    used, fresh = mk(), mk()
    o = used.reset(); fresh.reset()
    (o_t, _, _), _ = used.policy_step(tuned_blob, o, seed=NOISE_SEED, net=NET_TUNED)
    (o_t2, _, _), _ = used.policy_rollout(tuned_blob, o_t, 3, seed=NOISE_SEED, net=NET_TUNED)
    w, d = fresh.get_state_words()
    used.set_state_words(w, d)                       # the same env state again: only the handle's history differs
    for form in ("step", "rollout"):
        if form == "step":
            ra, rb = used.policy_step(default_blob, o, seed=NOISE_SEED, net=NET_DEFAULT), fresh.policy_step(default_blob, o, seed=NOISE_SEED)
        else:
            ra, rb = used.policy_rollout(default_blob, o, 5, seed=NOISE_SEED, net=NET_DEFAULT), fresh.policy_rollout(default_blob, o, 5, seed=NOISE_SEED)
        for x, y in zip(ra[0] + ra[1], rb[0] + rb[1]):
            assert _bits_equal(x, y), form
        o = ra[0][0] if form == "step" else ra[0][0][-1]
    with pytest.raises(ValueError):
        used.policy_step(default_blob, o, net=NET_TUNED)     # the default net's blob is not the tuned net's length
    swing = mk(ENV_SWING)
    so = swing.reset()
    with pytest.raises(StepperError, match="Tennisbot"):
        swing.policy_floats(NET_TUNED)
    z = torch.zeros(1024, device="cuda:0")
    rc = swing.L.tb_policy_step_net(swing._h, NET_TUNED, z.data_ptr(), so.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                    z.data_ptr(), z.data_ptr(), 0, 0, None)
    assert rc == -3 and b"Tennisbot" in swing.L.tb_last_error()     # TB_E_PARAMS, before anything is launched
    for e in (used, fresh, swing):
        e.close()


def test_trainer_collects_with_the_tuned_net_and_round_trips_a_checkpoint(torch, tmp_path):
    """PPOTrainer(policy="tuned") with the torch learner: the fused rollout's buffers match the reference eager and replayed, three
    updates give finite losses and move the extractor, the checkpoint round trip is bit-exact; default arguments still build the
    default net"""
    from tennisbot_rl_amd.ppo import PPOTrainer, pack_policy
    tr = PPOTrainer("Tennisbot-v0", policy="tuned", num_envs=64, n_steps=32, device="cuda:0", seed=3)
    assert tr.fused and tr.rollout_launch and tr.net == NET_TUNED and sum(p.numel() for p in tr.policy.parameters()) == 9639
    assert tr.hp["ent_coef"] == 0.0 and tr.hp["n_epochs"] == 10 and tr.hp["reference_n_epochs"] == 2000
    n, T = 64, 32
    ids = tr.env.env_id_base + np.arange(n, dtype=np.uint64)
    w0 = {k: v.clone() for k, v in tr.policy.state_dict().items()}
    for k in range(3):
        ep0, sc0 = keys_of(tr.env)
        last_value = tr.collect()
        torch.cuda.synchronize()
        ep, sc, _, _ = pr.episode_keys(ep0, sc0, tr.buf.dones.cpu().numpy())
        ref = tref.towers(tr.policy, tr.obs_seq.cpu().numpy().reshape(T * n, -1))
        eps = pr.policy_noise(tr.noise_seed, np.tile(ids, T), ep.ravel(), sc.ravel(), A)
        check_outputs("tuned trainer collect %d" % k, ref, eps, tr.buf.actions.cpu().numpy().reshape(-1, A), tr._raw_actions.cpu().numpy().reshape(-1, A),
                      tr.logps.cpu().numpy().ravel(), tr.values.cpu().numpy().ravel(), False)
        stats = tr.update(*tr.advantages(last_value))
        assert all(np.isfinite(stats[s]) for s in ("policy_loss", "value_loss", "entropy")), stats
    assert tr._graph is not None
    for k in tref.TRUNK_KEYS:
        assert not torch.equal(tr.policy.state_dict()[k], w0[k]), "%s did not move" % k
    path = str(tmp_path / "tuned.pt")
    tr.save(path)
    tr2 = PPOTrainer("Tennisbot-v0", policy="tuned", num_envs=64, n_steps=32, device="cuda:0", seed=99).load(path)
    for k, v in tr.policy.state_dict().items():
        assert torch.equal(v, tr2.policy.state_dict()[k]), k
    assert torch.equal(pack_policy(tr2.policy), pack_policy(tr.policy)) and tr2.num_timesteps == tr.num_timesteps
    wa, da = tr.env.get_state_words(); wb, db = tr2.env.get_state_words()
    assert torch.equal(wa, wb) and torch.equal(da, db)
    tr.env.close(); tr2.env.close()
    plain = PPOTrainer("Tennisbot-v0", num_envs=64, n_steps=32, device="cuda:0", seed=3)
    assert plain.net == NET_DEFAULT and not hasattr(plain.policy, "features_extractor") and plain.hp["ent_coef"] == 0.01
    plain.env.close()
