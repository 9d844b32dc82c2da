"""The reference of tb_trpo_returns (tests/trpo_returns_reference.py) against agent.py's own loop, and what of form="agent_returns"
needs no GPU:

  * the float64 reference (returns, finished-row mask, index list) against agent.py's per-episode loop (agent.py:253-279, 264-268) run
    env by env over ragged synthetic episodes: the same rows, the same bits;
  * the restatement of the four launches (kernel_reference, compact_by_table) against that definition, past one scan pass too; the
    value fixtures hold what they are named for and agree with agent.py's loop where they are finite; each of the seven mutants
    (a kernel that is subtly wrong) is rejected by the fixture named for it in tests/test_gpu_trpo_returns_edges.py;
  * the host side of the C ABI: the symbols, the workspace query, every refusal (tb_ppo_gae's conventions);
  * AGENT_PY_DEFAULTS is the list of the issue, cited to agent.py; an explicit keyword and a command-line flag beat it;
  * the raw log_std direction and the skip rule on hand-made inputs;
  * main.py's and train_swing.py's options.
"""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest

import trpo_returns_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ragged(T, n, seed):
    rng = np.random.default_rng(seed)
    dones = (rng.random((T, n)) < 0.08).astype(np.uint8)
    dones[:, 0] = 0                      # an env that never finishes
    dones[:, 1] = 0; dones[T - 1, 1] = 1   # one episode over the whole rollout
    dones[:, 2] = 1                      # an episode per step
    dones[:, 3] = 0; dones[0, 3] = 1       # only the first row is finished
    return rr.rollout_rewards(T, n, seed), dones


@pytest.mark.parametrize("T,n,seed", [(1, 5, 0), (40, 9, 1), (133, 17, 2)])
def test_reference_is_agent_py_on_ragged_episodes(T, n, seed):
    rewards, dones = ragged(T, n, seed)
    R, mask, idx = rr.returns_reference(rewards, dones)
    theirs = rr.agent_py_returns(rewards, dones)
    assert sorted(theirs) == list(idx) and len(idx) == int(mask.sum()) and np.all(np.diff(idx) > 0)
    flat = R.reshape(-1)
    assert all(flat[i] == v and math.copysign(1.0, flat[i]) == math.copysign(1.0, v) for i, v in theirs.items())   # float64, bit for bit
    assert not flat[~mask.reshape(-1)].any()
    # the mask from its definition: t <= the env's last done
    for e in range(n):
        ends = np.flatnonzero(dones[:, e])
        last = ends[-1] if len(ends) else -1
        assert np.array_equal(mask[:, e], np.arange(T) <= last)
    assert not mask[:, 0].any() and mask[:, 1].all() and mask[:, 2].all() and mask[:, 3].sum() == 1
    assert np.array_equal(R[:, 2], rewards[:, 2].astype(np.float64))          # done at every step: R == r
    # the closed form of one whole-rollout episode, to float64 accuracy (the recurrence is not the sum, bit for bit)
    want = sum(float(rewards[t, 1]) * rr.DISCOUNT ** t for t in range(T))
    assert abs(R[0, 1] - want) <= 1e-12 * sum(abs(float(rewards[t, 1])) for t in range(T))


def test_the_discount_is_a_parameter_and_the_rounding_is_single():
    rewards, dones = ragged(60, 7, 5)
    a, _, _ = rr.returns_reference(rewards, dones, 0.98)
    b, _, _ = rr.returns_reference(rewards, dones, 0.5)
    one, _, _ = rr.returns_reference(rewards, dones, 1.0)
    assert not np.array_equal(a, b)
    # carrying the recurrence in float32 gives other bits somewhere: the float64 carry is observable
    R32 = np.zeros_like(rewards)
    for e in range(rewards.shape[1]):
        nxt = np.float32(0.0)
        for t in range(rewards.shape[0] - 1, -1, -1):
            nxt = rewards[t, e] if dones[t, e] else np.float32(rewards[t, e] + np.float32(np.float32(0.98) * nxt))
            R32[t, e] = nxt
    _, mask, _ = rr.returns_reference(rewards, dones)
    assert not np.array_equal(np.where(mask, R32, 0).astype(np.float32), a.astype(np.float32))
    assert np.allclose(one[0, 1], rewards[:, 1].astype(np.float64).sum(), rtol=1e-12)


# --------------------------------------------------------------------------------- the launches restated, the fixtures, the mutants
SCAN_SHAPES = [(1025, 1), (2048, 1), (33, 2000), (17, 4097)]     # tests/test_gpu_trpo_returns_edges.py: past one scan pass of 1024 entries
OLD_SHAPES = [(1, 1), (2, 63), (27, 64), (27, 65), (53, 130), (3, 4097)]   # tests/test_gpu_trpo_returns.py


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def definition(rewards, dones, discount=rr.DISCOUNT):
    """returns_reference in the shape of kernel_reference's result"""
    with np.errstate(all="ignore"):
        R, mask, idx = rr.returns_reference(rewards, dones, discount)
        return np.where(mask, R, 0.0).astype(np.float32), idx, len(idx)


def same(a, b):
    """bit for bit where the first is not NaN, NaN where it is; the same list and count"""
    nan = np.isnan(a[0])
    return np.array_equal(nan, np.isnan(b[0])) and np.array_equal(u32(a[0])[~nan], u32(b[0])[~nan]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("T,n", SCAN_SHAPES + [(78, 1100), (104, 4096)])
def test_compact_by_table_is_flatnonzero(T, n):
    entries = T * ((n + 63) // 64)
    assert entries > rr.SCAN_PASS
    for p, which in enumerate(rr.PATTERNS):
        if T * n > 10 ** 5 and which not in ("bernoulli", "last-step"):
            continue
        mask = np.zeros((T, n), bool)
        d = rr.patterns(T, n, which, seed=7 + p) != 0
        for e in range(n):
            ends = np.flatnonzero(d[:, e])
            if len(ends):
                mask[:ends[-1] + 1, e] = True
        want = np.flatnonzero(mask.reshape(-1))
        assert np.array_equal(rr.compact_by_table(mask), want), (T, n, which)
        if T * n <= 10 ** 5:
            for pass_entries in (1, 7, 64, entries - 1, entries, entries + 1):
                assert np.array_equal(rr.compact_by_table(mask, pass_entries), want), (T, n, which, pass_entries)
        # without the carry the list is another one as soon as a set row lies behind the first pass
        entry = np.arange(T)[:, None] * ((n + 63) // 64) + np.arange(n)[None, :] // 64
        if mask[entry >= rr.SCAN_PASS].any():
            assert not np.array_equal(rr.compact_by_table(mask, carry=False), want), (T, n, which)


@pytest.mark.parametrize("T,n", OLD_SHAPES[:5] + [(1025, 1), (33, 2000)])
def test_kernel_reference_is_the_definition(T, n):
    for p, which in enumerate(rr.PATTERNS):
        rewards, dones = rr.rollout_rewards(T, n, seed=p), rr.patterns(T, n, which, seed=7 + p)
        got, want = rr.kernel_reference(rewards, dones), definition(rewards, dones)
        assert not rr.differs(got, want), (T, n, which)
        assert not rr.differs(rr.kernel_reference(rewards, dones, 0.5), definition(rewards, dones, 0.5))


def test_value_fixtures_hold_what_they_are_named_for():
    fx = rr.value_fixtures()
    assert set(fx) == set(rr.VALUE_FIXTURES) and len(fx) == len(rr.VALUE_FIXTURES) == 8
    T, n = rr.VALUE_T, rr.VALUE_N
    clean = np.arange(n) % 3 == 2
    plain = definition(rr.rollout_rewards(T, n, 0), fx["overflow"][1])
    for name, (rewards, dones, discount) in fx.items():
        assert rewards.shape == dones.shape == (T, n) and rewards.dtype == np.float32 and dones.dtype == np.uint8
        want = definition(rewards, dones, discount)
        assert same(want, rr.kernel_reference(rewards, dones, discount)), name
        assert np.isfinite(want[0][:, clean]).all() and np.isfinite(want[0][:9]).all() and np.isfinite(want[0][18:]).all(), name   # what is special stays in its episode
        if name != "done_bytes" and name != "nonfinite":
            assert np.array_equal(want[1], plain[1]), name                  # values never move the mask
        if name in rr.FINITE_VALUE_FIXTURES:                                # agent.py's own loop, float64 bit for bit
            with np.errstate(all="ignore"):
                R, mask, idx = rr.returns_reference(rewards, dones, discount)
                theirs = rr.agent_py_returns(rewards, dones, discount)
            flat = R.reshape(-1)
            assert sorted(theirs) == list(idx)
            assert all(flat[i] == v and math.copysign(1.0, flat[i]) == math.copysign(1.0, v) for i, v in theirs.items()), name
    with np.errstate(all="ignore"):
        R = {k: rr.returns_reference(*v)[0] for k, v in fx.items()}
    stored = {k: definition(*v)[0] for k, v in fx.items()}
    for name in ("overflow", "overflow_and_back"):
        over = np.abs(R[name]) > rr.F32_MAX
        assert np.isfinite(R[name]).all() and over.any() and (stored[name][over] == np.inf).any() and (stored[name][over] == -np.inf).any()
    back = (np.abs(R["overflow_and_back"][1:]) > rr.F32_MAX) & (np.abs(R["overflow_and_back"][:-1]) < rr.F32_MAX) & (R["overflow_and_back"][:-1] != 0)
    assert back.sum() >= 40 and np.isfinite(stored["overflow_and_back"][:-1][back]).all() and (np.abs(stored["overflow_and_back"][:-1][back]) > 1e38).all()
    s, S = stored["subnormal"], R["subnormal"]
    sub = (s != 0) & (np.abs(s) < rr.F32_TINY)
    assert (sub & (s > 0)).sum() > 100 and (sub & (s < 0)).sum() > 100
    assert (np.abs(fx["subnormal"][0][9:18, ~clean]) < rr.F32_TINY).all() and fx["subnormal"][0][9:18, ~clean].all()
    tiny = (S != 0) & (np.abs(S) < 2.0 ** -150)
    assert (tiny & (S > 0)).any() and (tiny & (S < 0)).any() and not s[tiny].any()
    assert set(u32(s[tiny])) == {0, 0x80000000}                            # the zero keeps the sign
    z = stored["signed_zero"]
    assert (u32(z[16:18, ~clean]) == 0x80000000).all() and (u32(z[14:16, ~clean]) == 0).all() and (u32(z[8, ~clean]) == 0x80000000).all()
    assert (u32(fx["signed_zero"][0][20:, 0::2]) == 0x80000000).all() and (u32(z[18:, 0::2]) == 0).all()
    nf = stored["nonfinite"]
    e = np.arange(n)
    assert np.isnan(nf[9:14, e % 6 == 0]).all() and (nf[9:14, e % 6 == 1] == np.inf).all() and (nf[9:14, e % 6 == 3] == -np.inf).all()
    assert np.isnan(nf[9:14, e % 6 == 4]).all() and (nf[14, e % 6 == 4] == np.inf).all() and np.isfinite(nf[14:18, e % 6 != 4]).all()
    assert np.isnan(fx["nonfinite"][0][20, 2]) and not nf[18:, 2].any() and len(definition(*fx["nonfinite"])[1]) == T * n - 9
    assert set(np.unique(fx["done_bytes"][1])) == {0, 1, 2, 0x80, 0xFF}
    d0 = stored["discount_0"]
    assert np.isnan(d0[9:13, ~clean]).all() and np.isinf(d0[13, ~clean]).all() and np.array_equal(u32(d0[:18, clean]), u32(fx["discount_0"][0][:18, clean] + np.float32(0.0)))
    assert np.allclose(R["discount_1"][9], fx["discount_1"][0][9:18].astype(np.float64).sum(0), rtol=1e-9, atol=1e-9)


def test_tie_fixture_separates_the_two_roundings():
    assert rr.tie_discounts() >= 2
    seen = set()
    for i in range(rr.tie_discounts()):
        rewards, dones, discount = rr.tie_fixture(i)
        seen.add(discount)
        n = rewards.shape[1]
        assert rewards.shape == (2, n) and n >= 65 and dones[1].all() and not dones[0].any() and 0.0 < discount < 1.0
        sep, fused = rr.kernel_reference(rewards, dones, discount), rr.Mutant("fused")(rewards, dones, discount)
        assert not rr.differs(sep, definition(rewards, dones, discount))
        assert (u32(sep[0][0]) != u32(fused[0][0])).all(), "tie fixture %d: an env does not tell the fused form apart" % i
        assert np.array_equal(u32(sep[0][1]), u32(fused[0][1])) and np.array_equal(sep[1], fused[1])
        print("tie fixture %d: discount %r, r1 = %g, %d envs" % (i, discount, rewards[1, 0], n))
    assert len(seen) == rr.tie_discounts()
    # the issue's example
    r = np.array([[16777256.0], [5.0]], np.float32)
    d = np.array([[0], [1]], np.uint8)
    assert rr.kernel_reference(r, d, 0.20000000037252905)[0][0, 0] == 16777256.0 and rr.Mutant("fused")(r, d, 0.20000000037252905)[0][0, 0] == 16777258.0


def rejecting_inputs(name):
    """the table of the module docstring of tests/test_gpu_trpo_returns_edges.py: the fixture that rejects each mutant"""
    fx = rr.value_fixtures()
    if name == "no_carry":
        return rr.rollout_rewards(1025, 1, 0), rr.patterns(1025, 1, "last-step"), rr.DISCOUNT
    if name == "fused":
        return rr.tie_fixture(0)
    if name == "first_done":
        return rr.rollout_rewards(27, 65, 4), rr.patterns(27, 65, "bernoulli", seed=11), rr.DISCOUNT
    if name == "unfinished_keep":
        dones = rr.patterns(27, 65, "last-step")
        dones[26, 64] = 0                                   # last-step minus one env: its rows hold 0.0, whatever R the lane carries
        return rr.rollout_rewards(27, 65, 1), dones, rr.DISCOUNT
    return fx[{"float32_carry": "overflow_and_back", "done_is_one": "done_bytes", "flush_subnormal": "subnormal"}[name]]


@pytest.mark.parametrize("name", rr.MUTANTS)
def test_every_mutant_is_rejected_by_its_fixture(name):
    rewards, dones, discount = rejecting_inputs(name)
    want, got = rr.kernel_reference(rewards, dones, discount), rr.Mutant(name)(rewards, dones, discount)
    assert not rr.differs(want, definition(rewards, dones, discount))
    assert np.isfinite(got[0]).all() or name == "float32_carry"
    assert rr.differs(got, want), "the mutant %s passes the fixture named for it" % name
    if name == "no_carry":
        assert want[2] == 1025 and got[2] == 1 and np.array_equal(u32(got[0]), u32(want[0]))
    if name == "first_done":
        assert (rr.patterns(27, 65, "bernoulli", seed=11).sum(0) >= 2).any()


def test_the_older_fixtures_do_not_see_a_fused_recurrence():
    """printed, not asserted: fl(r + discount R') and r + fl(discount R') part after the float32 store only beside a float32 tie"""
    apart = 0
    for T, n in OLD_SHAPES:
        for p, which in enumerate(rr.PATTERNS):
            rewards, dones = rr.rollout_rewards(T, n, seed=p), rr.patterns(T, n, which, seed=7 + p)
            apart += int(rr.differs(rr.kernel_reference(rewards, dones), rr.Mutant("fused")(rewards, dones)))
    print("rollout_rewards fixtures that tell the fused recurrence apart: %d of %d" % (apart, len(OLD_SHAPES) * len(rr.PATTERNS)))


# ------------------------------------------------------------------------------------------------------ the host side of the ABI
@pytest.fixture(scope="module")
def lib():
    from tennisbot_rl_amd.build import build_library
    from tennisbot_rl_amd.stepper import load_library
    build_library()
    return load_library()


def test_returns_symbols_and_workspace_query(lib):
    assert hasattr(lib, "tb_trpo_returns") and hasattr(lib, "tb_trpo_returns_workspace_bytes")
    assert lib.tb_abi_version() == 4
    q = lib.tb_trpo_returns_workspace_bytes
    for T, n in ((1, 1), (2, 63), (27, 64), (27, 65), (53, 130), (3, 4097), (104, 4096)):
        b = q(T, n)
        assert b % 8 == 0 and b >= 8 * T * ((n + 63) // 64) + 4 * n, (T, n, b)     # a [T][chunks] int64 table and L_e [n] int32
        assert q(T + 1, n) - b == 8 * ((n + 63) // 64)
    assert q(27, 64) < q(27, 65) and q(1, 1) == 16
    for bad in (q(0, 4), q(4, 0), q(-1, 4)):
        assert bad == -1 and b"tb_trpo_returns_workspace_bytes" in lib.tb_last_error()


def test_returns_refusals_need_no_device(lib):
    buf = (ctypes.c_double * 8192)()
    a = ctypes.addressof(buf)
    assert a % 8 == 0
    T, n = 4, 6
    ws = lib.tb_trpo_returns_workspace_bytes(T, n)

    def refused(args, word):
        assert lib.tb_trpo_returns(*args) == -1 and word in lib.tb_last_error(), lib.tb_last_error()

    #       kind dev stream T  n  rewards stride dones  stride discount returns  idx      count     workspace  bytes
    good = [0, 0, None, T, n, a, 0, a + 512, 0, 0.98, a + 1024, a + 2048, a + 4096, a + 8192, ws]
    for k in (5, 7, 10, 11, 12, 13):
        bad = list(good); bad[k] = None
        refused(bad, b"null")
    for k in (5, 10):
        bad = list(good); bad[k] += 2
        refused(bad, b"4-byte aligned")
    for k in (11, 12, 13):
        bad = list(good); bad[k] += 4
        refused(bad, b"8-byte aligned")
    for stride in (4 * n - 4, 4 * n + 2):                       # tb_ppo_gae's convention: 0 = contiguous, else >= n floats and a multiple of 4
        bad = list(good); bad[6] = stride
        refused(bad, b"rewards' step stride")
    bad = list(good); bad[8] = n - 1
    refused(bad, b"dones' step stride")
    for k in (3, 4):
        bad = list(good); bad[k] = 0
        refused(bad, b"n_steps and n_envs")
    bad = list(good); bad[0] = 9
    refused(bad, b"env kind")
    bad = list(good); bad[14] = ws - 8
    refused(bad, b"workspace")
    # everything in order, strides larger than n included: the call gets as far as looking for a device
    import torch
    if not torch.cuda.is_available():
        for rs, ds in ((0, 0), (4 * n, n), (4 * n + 12, n + 5)):
            ok = list(good); ok[6], ok[8] = rs, ds
            assert lib.tb_trpo_returns(*ok) == -2 and b"no HIP device" in lib.tb_last_error(), lib.tb_last_error()


# ------------------------------------------------------------------------------------------------------------ preset and flags
def test_the_preset_is_the_issues_list():
    from tennisbot_rl_amd import trpo
    assert trpo.FORMS == ("agent", "sb3", "agent_returns")
    P = trpo.AGENT_PY_DEFAULTS
    assert {k: P[k] for k in trpo.TRPO_DEFAULTS} == trpo.TRPO_DEFAULTS
    extra = {k: v for k, v in P.items() if k not in trpo.TRPO_DEFAULTS}
    assert extra == dict(discount=0.98, log_std_step="raw", step_rows="all", log_std_init=math.exp(-1))
    # agent.py:39-42 divides a vector of ones by its exponential
    assert abs(P["log_std_init"] - 1.0 / math.e) <= 1e-16
    assert P["discount"] == rr.DISCOUNT
    # the other forms' presets do not name the new hyper-parameters: they keep "natural", "cg" and the module's log_std
    assert not set(extra) & (set(trpo.TRPO_DEFAULTS) | set(trpo.SB3_TRPO_DEFAULTS))


def test_keywords_beat_the_preset():
    from tennisbot_rl_amd import trpo
    kw = trpo.form_keywords("agent_returns", dict(discount=0.9, log_std_step="natural", cg_iterations=3, policy="default"))
    assert (kw["discount"], kw["log_std_step"], kw["cg_iterations"], kw["step_rows"], kw["policy"]) == (0.9, "natural", 3, "all", "default")
    assert kw["log_std_init"] == math.exp(-1) and kw["kl_delta"] == 0.01
    assert trpo.form_keywords("agent", dict(step_rows="all")) == dict(step_rows="all")
    assert trpo.form_keywords("sb3", {})["cg_iterations"] == 15
    with pytest.raises(ValueError, match="agent_returns"):
        trpo.TRPOTrainer("SwingRacket-v0", num_envs=64, n_steps=26, form="returns")
    for bad in (dict(log_std_step="rough"), dict(step_rows="some"), dict(form="agent_returns", step_rows="none")):
        with pytest.raises(ValueError, match="must be one of"):
            trpo.TRPOTrainer("SwingRacket-v0", num_envs=64, n_steps=26, **bad)
    # the learner fills its caller's dict before it looks for a device: what was given stays, the rest is the form's
    import torch
    from tennisbot_rl_amd.ppo import build_actor_critic
    from tennisbot_rl_amd.stepper import StepperError
    for form, given, want in (("agent_returns", dict(cg_damping=0.5, step_rows="cg"), dict(cg_damping=0.5, step_rows="cg", log_std_step="raw", discount=0.98)),
                              ("agent", dict(log_std_step="raw"), dict(log_std_step="raw", step_rows="cg", cg_damping=0.001)),
                              ("sb3", {}, dict(log_std_step="natural", step_rows="cg", cg_damping=0.1))):
        policy = build_actor_critic(6, 6, (32, 64, 32))
        hp = dict(given)
        with pytest.raises(StepperError, match="needs a GPU"):
            trpo.FusedTRPO(0, policy, torch.optim.Adam(policy.parameters()), hp, "cpu", form=form)
        assert {k: hp[k] for k in want} == want, (form, hp)
        assert ("discount" in hp) == (form == "agent_returns")


# ---------------------------------------------------------------------------------------------------- direction and skip rule
def test_raw_direction_assembly_and_the_skip_rule():
    import torch
    from tennisbot_rl_amd.trpo import raw_log_std_direction, skip_update
    # a flat vector of 2 log_std slots, 5 network slots, 3 value slots
    ls = torch.tensor([True, True] + [False] * 8)
    g = torch.tensor([0.25, -0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 0.0, 0.0, 0.0])          # the masked surrogate gradient: 0 on the value slots
    xf = torch.tensor([0.0, 0.0, -7.0, 8.0, -9.0, 10.0, -11.0, 0.0, 0.0, 0.0])      # the CG solve on the network's slots alone
    d = raw_log_std_direction(torch, xf, g, ls)
    assert d.is_contiguous() and d.dtype == torch.float32
    assert d.tolist() == [0.25, -0.5, -7.0, 8.0, -9.0, 10.0, -11.0, 0.0, 0.0, 0.0]
    # theta + step * direction, as policy_step forms it: log_std moves by fl(step * g_logstd), the network by fl(step * x)
    flat = torch.tensor([0.3, -0.1] + [1.0] * 8)
    step = torch.tensor(0.3)
    moved = flat + step * d
    assert torch.equal(moved[:2], flat[:2] + step * g[:2]) and torch.equal(moved[2:7], flat[2:7] + step * xf[2:7]) and torch.equal(moved[7:], flat[7:])
    assert [skip_update(c) for c in (0, 1, 2, 3, 10 ** 6)] == [True, True, False, False, False]


# -------------------------------------------------------------------------------------------------------------------- scripts
def load_script(name):
    spec = importlib.util.spec_from_file_location(name.replace(".", "_") + "_for_trpo_returns", os.path.join(ROOT, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_swing_options():
    mod = load_script("train_swing.py")
    kw = mod.trpo_keywords(mod.parse_args(["-s", "trpo", "--trpo-form", "agent_returns"]))
    assert kw == dict(form="agent_returns", policy="default")                                            # everything else: the preset's
    kw = mod.trpo_keywords(mod.parse_args(["-s", "trpo", "--trpo-form", "agent_returns", "--discount", "0.9", "--log-std-step", "natural", "--step-rows", "cg", "--kl-delta", "0.02"]))
    assert kw == dict(form="agent_returns", policy="default", discount=0.9, log_std_step="natural", step_rows="cg", kl_delta=0.02)
    kw = mod.trpo_keywords(mod.parse_args(["-s", "trpo", "--log-std-step", "raw", "--step-rows", "all"]))
    assert kw == dict(form="agent", policy="default", log_std_step="raw", step_rows="all")
    for argv, word in ((["--discount", "0.9"], "-s trpo"), (["--step-rows", "all"], "-s trpo"), (["-s", "trpo", "--discount", "0.9"], "agent_returns")):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(argv)
        assert word in str(e.value.code)


def test_main_options(monkeypatch):
    mod = load_script("main.py")
    a = mod.parse_args([])
    assert (a.strategy, a.iteration, a.load) == (0, 10, False)                       # main.py:94-97
    a = mod.parse_args(["-s", "1", "-i", "3", "--load"])
    assert (a.strategy, a.iteration, a.load) == (1, 3, True)
    with pytest.raises(SystemExit) as e:
        mod.parse_args(["-s", "2"])
    assert "Invalid strategy" in str(e.value.code)
    made = []
    import tennisbot_rl_amd.ppo as ppo
    import tennisbot_rl_amd.trpo as trpo
    monkeypatch.setattr(trpo, "TRPOTrainer", lambda env_id, **kw: made.append(("trpo", env_id, kw)))
    monkeypatch.setattr(ppo, "PPOTrainer", lambda env_id, **kw: made.append(("ppo", env_id, kw)))
    mod.make_trainer(mod.parse_args([]), "cuda:0")
    mod.make_trainer(mod.parse_args(["-s", "1"]), "cuda:0")
    assert made[0][:2] == ("trpo", "Tennisbot-v0") and made[0][2]["form"] == "agent_returns" and "net_arch" not in made[0][2]
    assert made[1][:2] == ("ppo", "Tennisbot-v0") and "form" not in made[1][2]
