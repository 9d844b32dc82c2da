"""The on-policy learner kernels of csrc/tb_learner.hpp and csrc/tb_trpo.hpp held BIT FOR BIT to what the commit before their shared
pieces computed (tests/golden/learner_bits_parent.json: per case a sha256 of the input bytes and a sha256 of the output bytes, with
the recording commit and card). The float64 references of the other learner tests allow 24 float32-twin errors; a piece that is
shared by four kernels must not move one rounding in any of them, and only a hash says so.

Cases (every input from the fixture code of learner_edge_fixtures, test_tuned_reference, mlp64_fixtures and population_fixtures; every
index vector has a repeat and two out-of-range entries, which the kernels clamp to the first and the last row):
  grad     tb_ppo_grad_net + TB_PPO_REDUCE on the four built (kind, net) pairs, batches 17 / 129 / 257, a benign fixture and a saturating
           one per pair: the gradient and the three statistics
  value    the same with TB_PPO_VALUE_ONLY, batch 129, the default nets: the policy slots keep what the gradient vector held
  members  tb_ppo_grad_members + tb_ppo_apply_members, three members with hyper-parameter rows of their own, batch 129
  fvp      tb_trpo_fvp_net on its three pairs, m = 17 / 129 / 257, damping 0 and 0.1
  search   tb_trpo_search_net on its three pairs, batches 17 and 1025 (one past a search share), steps (0, 1e-3, 1e-2): the float64
           pairs; the zero step's KL is exactly 0.0

The golden is the file `--record` wrote, unedited (torch names the MI355X "AMD Radeon Graphics"). One input is not an existing
fixture as it stands: the [64, 64] net has no saturating fixture, so `fixture` derives one from mlp64_fixtures' policy and rollout
(hidden weights times MLP64_SCALE, old_logp moved by the log-probability's change; no random draw of its own).

A case whose INPUT hash differs fails with "fixture changed, not the kernel": the golden must then be recorded again from a commit
whose kernels are trusted (python tests/test_gpu_learner_bits.py --record PATH COMMIT on an MI355X), never from the commit under test."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import learner_edge_fixtures as lf  # noqa: E402
import mlp64_fixtures as mfx  # noqa: E402
import trpo_reference as tr  # noqa: E402
import tuned_reference as tref  # noqa: E402
from edge_fixtures import index_vector  # noqa: E402
from policy_reference import state_dict_arrays  # noqa: E402
from tennisbot_rl_amd.params import ENV_SWING, ENV_TENNIS, NET_DEFAULT, NET_MLP64, NET_TUNED  # noqa: E402
from test_ppo_reference import flat_shard, make_policy, rollout  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "learner_bits_parent.json")
DEV = "cuda:0"
PAIRS = {"swing-default": (ENV_SWING, NET_DEFAULT), "swing-mlp64": (ENV_SWING, NET_MLP64), "tennis-default": (ENV_TENNIS, NET_DEFAULT),
         "tennis-tuned": (ENV_TENNIS, NET_TUNED)}
TRPO_PAIRS = ("swing-default", "swing-mlp64", "tennis-default")
KNAME = {"swing-default": "swing", "tennis-default": "tennis"}
REGIMES = ("benign", "saturating")
N_ROWS = lf.N_ROWS
SEARCH_BATCHES = (17, 1025)
SEARCH_STEPS = np.array([0.0, 1e-3, 1e-2], np.float32)
DAMPINGS = (0.0, 0.1)
MLP64_SCALE = 8.0
_cache = {}


def f32(x):
    return np.ascontiguousarray(x, np.float32)


def fixture(pair, regime):
    """(flat float32 parameters, the parameters by name or None, (obs, act, old_logp, adv, returns) of N_ROWS rows, hyper-parameters).
    benign: the first rows of test_ppo_reference's rollouts with make_policy's weights (clipped rows and active ones), of
    mlp64_fixtures' rollout with its policy, the tuned net's `sb3` gradient fixture. saturating: the edge fixtures' own; for the [64, 64]
    net, which has none, its hidden weight matrices times MLP64_SCALE with old_logp moved by the change of the log-probability."""
    if (pair, regime) in _cache:
        return _cache[pair, regime]
    if pair in KNAME and regime == "saturating":
        f = lf.build(KNAME[pair], "saturating")
        out = (tr.join_flat(f.P, f.P, np.float32), f.P, tuple(x[:N_ROWS] for x in f.data), f.hp)
    elif pair != "tennis-tuned":
        ro = mfx.rollout() if pair == "swing-mlp64" else rollout(lf.CASE[KNAME[pair]])
        P = state_dict_arrays(mfx.policy() if pair == "swing-mlp64" else make_policy(ro.arch, ro.kind))
        obs, act, old_logp, adv, ret = (x[:N_ROWS] for x in flat_shard(ro, ro.gae.adv, ro.gae.returns))
        if regime == "saturating":
            S = {k: (f32(MLP64_SCALE * v).astype(np.float64) if k.endswith(".weight") and k.startswith(("policy_net.", "value_net_body.")) else v) for k, v in P.items()}
            old_logp = f32(old_logp + (lf.logp64(S, obs, act) - lf.logp64(P, obs, act)))
            P = S
        out = (tr.join_flat(P, P, np.float32), P, (obs, act, old_logp, adv, ret), ro.hp)
    elif regime == "benign":
        from test_tuned_reference import HP, gradient_fixture
        fx = gradient_fixture("sb3")
        P = state_dict_arrays(fx["policy"])
        out = (tref.flat(P).astype(np.float32), None, tuple(fx[k][:N_ROWS] for k in ("obs", "act", "old_logp", "adv", "returns")), HP)
    else:
        P, hp, data, _, _ = lf.tuned_fixture("saturating", "saturating")
        out = (tref.flat(P).astype(np.float32), None, tuple(x[:N_ROWS] for x in data), hp)
    _cache[pair, regime] = out
    return out


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def h(x):
    return x.detach().cpu().numpy().copy()


# ------------------------------------------------------------------------------------------------------------------ the cases
def grad_case(torch, lib, pair, regime, batch, value_only=False):
    kind, net = PAIRS[pair]
    flat, _, data, hp = fixture(pair, regime)
    idx, _ = index_vector(N_ROWS, batch, 300 + batch)
    scalars = np.array([hp["clip_range"], hp["vf_coef"], hp["ent_coef"], float(value_only)], np.float64)
    inputs = [flat, *data, idx, scalars]
    arrays = [dev(torch, f32(x)) for x in data]
    flat_d, idx_d = dev(torch, flat), dev(torch, idx)
    need = lib.tb_ppo_workspace_bytes_net(kind, net, batch)
    assert need > 0
    ws = torch.full(((need + 7) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    grad, stats = torch.full((len(flat),), 7.0, device=DEV), torch.full((3,), 7.0, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    rc = lib.tb_ppo_grad_net(kind, net, 0, s, *(a.data_ptr() for a in arrays), N_ROWS, idx_d.data_ptr(), batch, flat_d.data_ptr(), len(flat), float(hp["clip_range"]),
                             float(hp["vf_coef"]), ws.data_ptr(), ws.numel() * 8)
    assert rc == 0, lib.tb_last_error()
    rc = lib.tb_ppo_apply_net(kind, net, 0, s, 1 | (4 if value_only else 0), ws.data_ptr(), ws.numel() * 8, batch, flat_d.data_ptr(), grad.data_ptr(), None, None, len(flat),
                              stats.data_ptr(), float(hp["ent_coef"]), 0.5, 1, 3e-4, 0.9, 0.999, 1e-5, 1)
    assert rc == 0, lib.tb_last_error()
    torch.cuda.synchronize()
    g, st = h(grad), h(stats)
    assert np.isfinite(g).all() and np.isfinite(st).all() and np.abs(g).max() > 0
    if value_only:
        assert (g == 7.0).any() and (g != 7.0).any()
    return inputs, [g, st]


def members_case(torch, lib, pair, batch=129):
    import test_gpu_learner_members as tm
    kind, net = PAIRS[pair]
    P = lib.tb_ppo_param_floats_net(kind, net)
    rows, state = tm.device_rows(torch, kind), tm.member_state(torch, kind, net, P)
    g = torch.Generator().manual_seed(100 + batch)
    idx = torch.stack([torch.randperm(tm.N_ROWS, generator=g) for _ in range(tm.M)])[:, :batch + 5].contiguous()
    idx[:, 1], idx[:, batch // 2] = -5, tm.N_ROWS + 7
    inputs = [h(x) for x in rows] + [h(x) for x in state] + [h(idx), np.array(tm.HP, np.float64)]
    out = tm.run_members(torch, lib, kind, net, batch, rows, idx.to(DEV), state, tm.HP)
    assert all(np.isfinite(x).all() for x in out)
    return inputs, out


def fvp_case(torch, lib, pair, m, damping):
    kind, net = PAIRS[pair]
    flat, P, data, _ = fixture(pair, "benign")
    vec = lf.fvp_vector(P)[0]
    idx, _ = index_vector(N_ROWS, m, 100 + m)
    inputs = [flat, data[0], vec, idx, np.array([damping], np.float64)]
    obs_d, flat_d, vec_d, idx_d = dev(torch, f32(data[0])), dev(torch, flat), dev(torch, vec), dev(torch, idx)
    need = lib.tb_trpo_fvp_workspace_bytes_net(kind, net, m)
    assert need > 0
    ws = torch.full(((need + 7) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((len(flat),), 7.0, device=DEV)
    rc = lib.tb_trpo_fvp_net(kind, net, 0, torch.cuda.current_stream().cuda_stream, obs_d.data_ptr(), N_ROWS, idx_d.data_ptr(), m, flat_d.data_ptr(), vec_d.data_ptr(), len(flat),
                             damping, out.data_ptr(), ws.data_ptr(), ws.numel() * 8)
    assert rc == 0, lib.tb_last_error()
    torch.cuda.synchronize()
    got = h(out)
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    return inputs, [got]


def search_case(torch, lib, pair, batch):
    kind, net = PAIRS[pair]
    flat, P, data, _ = fixture(pair, "benign")
    direction = lf.fvp_vector(P, seed=9)[0]
    idx, _ = index_vector(N_ROWS, batch, 200 + batch)
    inputs = [flat, *data[:4], direction, idx, SEARCH_STEPS]
    arrays = [dev(torch, f32(x)) for x in data[:4]]
    flat_d, dir_d, idx_d, steps_d = dev(torch, flat), dev(torch, direction), dev(torch, idx), dev(torch, SEARCH_STEPS)
    K = len(SEARCH_STEPS)
    need = lib.tb_trpo_search_workspace_bytes_net(kind, net, batch, K)
    assert need > 0
    ws = torch.full(((need + 7) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((K, 2), 7.0, dtype=torch.float64, device=DEV)
    rc = lib.tb_trpo_search_net(kind, net, 0, torch.cuda.current_stream().cuda_stream, *(a.data_ptr() for a in arrays), N_ROWS, idx_d.data_ptr(), batch, flat_d.data_ptr(),
                                dir_d.data_ptr(), len(flat), steps_d.data_ptr(), K, out.data_ptr(), ws.data_ptr(), ws.numel() * 8)
    assert rc == 0, lib.tb_last_error()
    torch.cuda.synchronize()
    got = h(out)
    assert np.isfinite(got).all() and got[0, 1] == 0.0, "the zero step's KL is %r, not exactly 0" % got[0, 1]
    assert (got[1:, 1] > 0.0).all()
    return inputs, [got]


CASES = {}
for _pair in PAIRS:
    for _regime in REGIMES:
        for _b in lf.SIZES:
            CASES["grad %s %s b=%d" % (_pair, _regime, _b)] = (grad_case, (_pair, _regime, _b))
for _pair in KNAME:
    CASES["value %s b=129" % _pair] = (grad_case, (_pair, "benign", 129, True))
for _pair in ("swing-default", "tennis-tuned"):
    CASES["members %s b=129" % _pair] = (members_case, (_pair,))
for _pair in TRPO_PAIRS:
    for _m in lf.SIZES:
        for _d in DAMPINGS:
            CASES["fvp %s m=%d damping=%g" % (_pair, _m, _d)] = (fvp_case, (_pair, _m, _d))
    for _b in SEARCH_BATCHES:
        CASES["search %s b=%d" % (_pair, _b)] = (search_case, (_pair, _b))


def digest(arrays):
    """sha256 over the arrays' bytes in order, each in its own dtype (floats are never converted: a NaN's payload counts)"""
    s = hashlib.sha256()
    for a in arrays:
        s.update(np.ascontiguousarray(a).tobytes())
    return s.hexdigest()


def run_case(torch, lib, name):
    fn, args = CASES[name]
    inputs, outputs = fn(torch, lib, *args)
    return digest(inputs), digest(outputs)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def lib(torch):
    from tennisbot_rl_amd.stepper import load_library
    return load_library()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_the_golden_lists_exactly_these_cases(golden):
    assert sorted(golden["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_bits_are_the_recorded_ones(torch, lib, golden, name):
    want = golden["cases"][name]
    got_in, got_out = run_case(torch, lib, name)
    assert got_in == want["input"], "%s: fixture changed, not the kernel (the input bytes are not the recorded ones)" % name
    assert run_case(torch, lib, name)[1] == got_out, "%s: a second run gave other bits" % name
    assert got_out == want["output"], "%s: the output bits are not those of commit %s" % (name, golden["commit"])


def record(path, commit):
    import torch
    from tennisbot_rl_amd.stepper import load_library
    lib = load_library()
    cases = {}
    for name in CASES:
        i, o = run_case(torch, lib, name)
        assert run_case(torch, lib, name) == (i, o), name
        cases[name] = {"input": i, "output": o}
        print(name, o[:16], flush=True)
    out = {"what": "per case of tests/test_gpu_learner_bits.py: sha256 of the input arrays' bytes and sha256 of the output arrays' bytes, computed by the library of "
                   "`commit` on `card`",
           "commit": commit, "card": torch.cuda.get_device_name(0), "cases": cases}
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    if len(sys.argv) != 4 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_learner_bits.py --record PATH COMMIT   (COMMIT: the commit whose library is loaded)")
    record(sys.argv[2], sys.argv[3])
