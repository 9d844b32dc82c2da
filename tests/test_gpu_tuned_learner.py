"""The fused learner on the tuned network (tb_ppo_grad_net / tb_ppo_apply_net with TB_NET_TUNED; ppo_tuned_tower in
csrc/tb_learner.hpp) against the float64 reference of tests/tuned_reference.py, on the kink-margin fixtures of
tests/test_tuned_reference.py: no hidden pre-activation of any row is within 2.5e-4 of 0, so a float32 forward cannot flip a ReLU
and every row takes part in every comparison.

Tolerance: ppo_reference.MULTIPLE (24) float32-twin errors per parameter tensor in the max norm, the twin being the reference's
own formulas in float32 (tests/ppo_reference.py, check_tensors). The extractor's four tensors are groups of their own, and are
checked three times: the whole gradient, the pi waves' share alone (vf_coef = 0: the vf waves' share is then an exact 0) and the
vf waves' share alone (zero advantages and ent_coef = 0: the pi share is an exact 0), each against the reference's share; and
whole = fl(pi sums + vf sums) against fl(pi sums) + fl(vf sums) within the three roundings that separate them.

The default Tennisbot network's gradient at batch 600 is held bit for bit to a hash recorded from the parent commit on an MI355X
(tests/golden/tennis_default_grad_b600.json): adding a network must not change a bit of the existing kernels' results."""
import hashlib
import json
import os
import socket
import sys

import numpy as np
import pytest

import ppo_reference as ref
import tuned_reference as tref
from policy_reference import U32, state_dict_arrays
from tennisbot_rl_amd.params import ENV_TENNIS, NET_DEFAULT, NET_TUNED
from test_tuned_reference import FIXTURES, HP, N_PARAMS, batch_indices, batch_of, gradient_fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tennis_default_grad_b600.json")
BATCHES = (2, 16, 17, 128, 129, 256, 257, 600)
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
        print("tuned learner: largest %s = %.3g" % (k, RATIOS[k]))


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)


def check_grads(tag, got, want, twin):
    """ppo_reference.check_tensors; a tensor that is exactly zero in the float64 reference AND in its float32 twin (a dead unit's
    row is only part of a tensor; this is a whole tensor: the other tower's in a one-share run) has no rounding scale and must be
    exactly zero on the device too"""
    zero = [k for k in want if not np.any(want[k]) and not np.any(twin[k])]
    for k in zero:
        assert not np.any(got[k]), "%s: %s must be exactly zero" % (tag, k)
    rest = [k for k in want if k not in zero]
    return ref.check_tensors(tag, {k: got[k] for k in rest}, {k: want[k] for k in rest}, {k: twin[k] for k in rest}, ref.MULTIPLE)


def device_gradient(torch, lib, kind, net, n_params, params, data, idx, hp, step=None):
    """tb_ppo_grad_net + TB_PPO_REDUCE (and, with `step`, TB_PPO_STEP on zero moments): (grad, stats[, new params]) as numpy"""
    dev = "cuda:0"
    t = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).to(dev)  # noqa: E731
    obs, act, old_logp, adv, returns = (t(x) for x in data)
    flat, ix = t(params), t(idx, torch.int64)
    batch = len(idx)
    need = lib.tb_ppo_workspace_bytes_net(kind, net, batch)
    assert need > 0
    ws = torch.full(((need + 7) // 8,), float("nan"), dtype=torch.float64, device=dev)   # the kernels must write every slot they read
    grad, stats, m, v = (torch.zeros(k, device=dev) for k in (n_params, 3, n_params, n_params))
    s = torch.cuda.current_stream().cuda_stream
    rc = lib.tb_ppo_grad_net(kind, net, 0, s, obs.data_ptr(), act.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), returns.data_ptr(), obs.shape[0], ix.data_ptr(),
                             batch, flat.data_ptr(), n_params, hp["clip_range"], hp["vf_coef"], ws.data_ptr(), ws.numel() * 8)
    assert rc == 0, lib.tb_last_error()
    phases = 1 if step is None else 3
    rc = lib.tb_ppo_apply_net(kind, net, 0, s, phases, ws.data_ptr(), ws.numel() * 8, batch, flat.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n_params,
                              stats.data_ptr(), hp["ent_coef"], hp["max_grad_norm"], 1, hp["learning_rate"], 0.9, 0.999, 1e-5, step or 1)
    assert rc == 0, lib.tb_last_error()
    torch.cuda.synchronize()
    out = (grad.cpu().numpy(), stats.cpu().numpy())
    return out if step is None else out + (flat.cpu().numpy(),)


@pytest.fixture(scope="module")
def lib(torch):
    from tennisbot_rl_amd.stepper import load_library
    return load_library()


@pytest.mark.parametrize("name", list(FIXTURES))
@pytest.mark.parametrize("batch", BATCHES)
def test_gradient_matches_the_float64_reference(torch, lib, name, batch):
    fx = gradient_fixture(name)
    P = state_dict_arrays(fx["policy"])
    flat = tref.flat(P).astype(np.float32)
    idx = batch_indices(batch, len(fx["adv"]))
    assert batch == 2 or len(np.unique(idx)) < batch                       # repeated rows
    data = tuple(fx[k] for k in ("obs", "act", "old_logp", "adv", "returns"))
    rows = batch_of(fx, idx)
    zero_adv = data[:3] + (np.zeros_like(fx["adv"]),) + data[4:]
    rows_zero_adv = rows[:3] + (np.zeros_like(rows[3]),) + rows[4:]
    cases = {"whole": (HP, data, rows), "pi share": (dict(HP, vf_coef=0.0), data, rows), "vf share": (HP, zero_adv, rows_zero_adv)}
    got = {}
    for tag, (hp, d, r) in cases.items():
        g, stats = device_gradient(torch, lib, ENV_TENNIS, NET_TUNED, N_PARAMS, flat, d, idx, hp)
        g2, stats2 = device_gradient(torch, lib, ENV_TENNIS, NET_TUNED, N_PARAMS, flat, d, idx, hp)
        assert np.array_equal(g.view(np.uint32), g2.view(np.uint32)) and np.array_equal(stats.view(np.uint32), stats2.view(np.uint32)), "a second run gave other bits"
        want, twin = tref.loss_and_grads(P, *r, hp), tref.loss_and_grads(P, *r, hp, np.float32)
        named = tref.unflat(g)
        note("gradient error / twin error (%s)" % tag, check_grads("%s b=%d %s gradient" % (name, batch, tag), named, want.grads, twin.grads))
        note("statistics error / twin error", check_grads("%s b=%d %s statistics" % (name, batch, tag), dict(zip(("policy_loss", "value_loss", "entropy"), stats.astype(np.float64))),
                                                           {k: np.float64(v) for k, v in want.stats.items()}, {k: np.float64(v) for k, v in twin.stats.items()}))
        got[tag] = (named, want)
    whole, want = got["whole"]
    for k in tref.TRUNK_KEYS:
        pi, vf = got["pi share"][0][k].astype(np.float64), got["vf share"][0][k].astype(np.float64)
        # each share alone against the reference's share (the other towers' tensors are checked above: the vf tensors of the pi-share
        # run and the pi tensors of the vf-share run are exact zeros on both sides)
        for tag, share in (("pi", pi), ("vf", vf)):
            scale = max(np.abs(want.parts[tag][k]).max(), 1e-30)
            twin_share = tref.loss_and_grads(P, *rows, HP, np.float32).parts[tag][k]
            tol = ref.MULTIPLE * max(np.abs(twin_share.astype(np.float64) - want.parts[tag][k]).max(), U32 * scale)
            err = np.abs(share - want.parts[tag][k]).max()
            assert err <= tol, "%s b=%d: %s share of %s off by %.3g (allowed %.3g)" % (name, batch, tag, k, err, tol)
        bound = 2.0 * U32 * (np.abs(pi) + np.abs(vf)) + 1e-45
        assert np.all(np.abs(whole[k].astype(np.float64) - (pi + vf)) <= bound), "%s b=%d: %s is not the sum of the two towers' shares" % (name, batch, k)
    if name == "dead":
        assert np.all(whole["features_extractor.layers.2.weight"][1] == 0.0) and whole["features_extractor.layers.2.bias"][1] == 0.0
        assert np.all(whole["policy_net.0.weight"][:, 1] == 0.0) and np.all(whole["value_net_body.0.weight"][:, 1] == 0.0)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_one_clip_and_adam_step_matches_the_reference(torch, lib, name):
    fx = gradient_fixture(name)
    P = state_dict_arrays(fx["policy"])
    flat = tref.flat(P).astype(np.float32)
    idx = batch_indices(257, len(fx["adv"]))
    data = tuple(fx[k] for k in ("obs", "act", "old_logp", "adv", "returns"))
    g, stats, new = device_gradient(torch, lib, ENV_TENNIS, NET_TUNED, N_PARAMS, flat, data, idx, HP, step=1)
    moved = {}
    for dtype in (np.float64, np.float32):
        res = tref.loss_and_grads(P, *batch_of(fx, idx), HP, dtype)
        clipped, norm = ref.clip_global_norm(res.grads, HP["max_grad_norm"], dtype)
        Pd = ref.cast_params(P, dtype)
        moved[dtype] = (ref.param_change(ref.adam_step(Pd, clipped, ref.adam_init(Pd, dtype), HP["learning_rate"], dtype=dtype), P, HP["learning_rate"]), clipped, norm)
    assert moved[np.float64][2] > HP["max_grad_norm"]                      # the clip is active
    note("clipped gradient error / twin error", ref.check_tensors(name + " clipped gradient", tref.unflat(g), moved[np.float64][1], moved[np.float32][1], ref.MULTIPLE))
    d_got = ref.param_change(tref.unflat(new.astype(np.float64)), P, HP["learning_rate"])
    note("parameter change error / twin error", ref.check_tensors(name + " parameters", d_got, moved[np.float64][0], moved[np.float32][0], ref.MULTIPLE))


def default_net_case():
    """the default Tennisbot network's gradient inputs at batch 600: everything from numpy generators with fixed seeds"""
    rng = np.random.default_rng(600)
    n_params, n = 10181, 900
    params = (rng.normal(size=n_params) * 0.1).astype(np.float32)
    obs = (rng.normal(size=(n, 12)) * 3.0).astype(np.float32)
    act = rng.normal(size=(n, 2)).astype(np.float32)
    old_logp = (rng.normal(size=n) * 0.3 - 2.0).astype(np.float32)
    adv = rng.normal(size=n).astype(np.float32)
    returns = rng.normal(size=n).astype(np.float32)
    idx = rng.integers(0, n, size=600).astype(np.int64)
    return n_params, params, (obs, act, old_logp, adv, returns), idx


def gradient_hash(grad, stats):
    return hashlib.sha256(np.ascontiguousarray(grad, np.float32).tobytes() + np.ascontiguousarray(stats, np.float32).tobytes()).hexdigest()


def test_the_default_net_gradient_is_the_parent_commit_s_bit_for_bit(torch, lib):
    n_params, params, data, idx = default_net_case()
    hp = dict(HP, ent_coef=0.01)
    g, stats = device_gradient(torch, lib, ENV_TENNIS, NET_DEFAULT, n_params, params, data, idx, hp)
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    golden = json.load(open(GOLDEN))
    assert gradient_hash(g, stats) == golden["sha256"], "the default Tennisbot net's gradient at batch 600 is not the parent commit's"


def test_trainer_updates_the_tuned_net_with_the_fused_learner(torch, tmp_path):
    from tennisbot_rl_amd.ppo import PPOTrainer, pack_policy
    tr = PPOTrainer("Tennisbot-v0", policy="tuned", learner="fused", num_envs=64, n_steps=32, device="cuda:0", seed=3)
    assert tr.fused and tr._learner is not None and tr._learner.net == NET_TUNED and tr._learner.n_params == N_PARAMS
    w0 = {k: v.clone() for k, v in tr.policy.state_dict().items()}
    hist = tr.learn(3 * 64 * 32, log=None)
    torch.cuda.synchronize()
    assert len(hist) == 3 and all(np.isfinite(h[k]) for h in hist for k in ("policy_loss", "value_loss", "entropy"))
    for k in tref.TRUNK_KEYS:
        assert not torch.equal(tr.policy.state_dict()[k], w0[k]), "%s did not move" % k
    assert torch.equal(pack_policy(tr.policy), pack_policy(tr.policy).clone()) and torch.isfinite(tr._learner.flat).all()
    path = str(tmp_path / "tuned_fused.pt")
    tr.save(path)
    tr2 = PPOTrainer("Tennisbot-v0", policy="tuned", learner="fused", num_envs=64, n_steps=32, device="cuda:0", seed=77).load(path)
    for k, v in tr.policy.state_dict().items():
        assert torch.equal(v, tr2.policy.state_dict()[k]), k
    for p, q in zip(tr.policy.parameters(), tr2.policy.parameters()):
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(tr.opt.state[p][key], tr2.opt.state[q][key])
    # ... and both go on identically from there (the same envs, weights, moments and noise keys; rank-local seeds only seed torch)
    tr2.noise_seed = tr.noise_seed
    torch.manual_seed(5); tr.learn(tr.num_timesteps + 64 * 32, log=None)
    torch.manual_seed(5); tr2.learn(tr2.num_timesteps + 64 * 32, log=None)
    for k, v in tr.policy.state_dict().items():
        assert torch.equal(v, tr2.policy.state_dict()[k]), k
    tr.env.close(); tr2.env.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from tennisbot_rl_amd.ppo import PPOTrainer
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    tr = PPOTrainer("Tennisbot-v0", policy="tuned", learner="fused", num_envs=128, n_steps=32, device="cuda:0", seed=5, batch_size=2048, n_epochs=3)
    assert tr.world == 2 and tr.rank == rank and tr.env.env_id_base == rank * 128 and tr._learner.net == NET_TUNED
    start = torch.cat([p.detach().reshape(-1) for p in tr.policy.parameters()]).cpu().numpy()
    hist = tr.learn(2 * 128 * 32 * 2, log=None)
    flat = torch.cat([p.detach().reshape(-1) for p in tr.policy.parameters()]).cpu().numpy()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), weights=flat, start=start, obs=tr.buf.obs.cpu().numpy(), grad=tr._learner.grad.cpu().numpy(),
             losses=np.array([[x["policy_loss"], x["value_loss"], x["entropy"]] for x in hist]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_end_with_identical_weights(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(_free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert np.array_equal(a["weights"], b["weights"]), "replicas diverged: gradients were not averaged identically"
    assert np.array_equal(a["grad"], b["grad"]) and len(a["weights"]) == N_PARAMS
    assert not np.array_equal(a["obs"], b["obs"]), "both ranks stepped the same envs"
    assert np.isfinite(a["weights"]).all() and np.isfinite(a["losses"]).all() and np.isfinite(b["losses"]).all()
    assert not np.array_equal(a["weights"][2:964], a["start"][2:964])     # the extractor moved
