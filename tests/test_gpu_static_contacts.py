"""The ball's court, net and goal contacts on forced states, kernel by kernel, on a real MI355X: every kernel that steps an env carries
the same static narrowphase (sphere_vs_box, sphere_vs_goal behind the near_ground / near_net / near_goal culls and the static_top
wave vote) and the same static contact rows (setup_static, normal_static, friction_static, Tennisbot's ground-only solo loop, rows in
registers or in the lane's LDS column). Here they start on tests/static_contact_fixtures.py's labelled states -- box edges, corners
and interiors, the goal's wall, rim, interior and axis, two and three static rows in one solve, a racket row on top -- and every
comparison is bit for bit (test_gpu_parity's same / compare_state, TOL = 0) against a float32 OracleBatch with 8 threads. What the
batch reaches is pinned on the oracle alone in tests/test_static_contact_states.py.

  a. the yardstick: unpipelined tb_step, both kinds, both lane orders, block 64 and 256: every output and the whole state after each
     of 8 steps, last_substeps, the counters (SwingRacket's step counts are random in 0 .. 23: the batch crosses 25 and flies to its end);
  b. tb_rollout, one call of 8 steps, against a);
  c. SwingRacket pipelined, step_count = 10 everywhere, step_waves 1 and 2 (the two-wave SHORT form: every wave holding a low ball
     takes its rare path, the blocked order's `high` wave the common one);
  d. SwingRacket pipelined at step_count = 25: the episode-end launch as a kernel per episode end, with stragglers deferred, and as
     the pool with ff_seal -- rewards after flush(), states, counters against the oracle's full flights;
  e. the loop kernels from the forced states: tb_policy_rollout_net and tb_sac_collect, their reported actions replayed through
     tb_step on a twin and through the oracle;
  f. tb_swing_trace at step_count = 25, stride 16, 8 frames;
  g. the extended contact set (F_RACKET_GROUND + rolling-friction rows: rolling rows on oblique normals, rows in the LDS column);
  h. not a no-op: in a) the final state differs from a twin with other restitution and friction, region by region.

Out of scope: the large-batch forms (RELOAD, the phased fast-forward above 131 072 envs: test_gpu_parity's 131 075- and 200 003-env
tests), and tb_es_evaluate, tb_policy_evaluate, tb_sac_evaluate, which reset before they run and cannot start from a forced state.

What the batch holds (float32 oracle, lanes that hit / lanes, row sets: R racket, G ground, N net, C goal; from
test_static_contact_states.py's printout):

  region      Tennisbot                                  SwingRacket
  high         0/66  -                                    0/66  -
  g_top       57/67  G                                   57/66  G
  g_edge_x    52/66  G                                   53/66  G
  g_edge_y    50/67  G                                   56/66  G
  g_corner    53/66  G                                   58/65  G
  g_side      51/66  G                                   53/65  G
  g_under     55/66  G                                   52/66  G
  n_face      52/66  N                                   55/66  N
  n_top       55/67  N                                   57/66  N
  n_tape      58/66  N                                   60/66  N
  n_end       57/67  N                                   54/66  N
  n_end_edge  55/66  N                                   55/65  N
  n_corner    55/66  N                                   49/65  N
  n_inside    66/66  N                                   66/66  N
  n_foot      66/66  GN 56, G 10                         66/66  GN 55, G 11
  c_top                                                  54/66  C
  c_wall                                                 62/66  GC 50, G 8, C 4
  c_rim                                                  60/66  C
  c_inside                                               65/65  C
  c_axis                                                 56/65  C
  c_net                                                  65/65  GNC 55, GC 10
  r_foot      67/67  RGN 29, GN 28, RG 3, G 7            66/66  RGN 29, GN 27, RG 6, G 4

Would it notice? Four deliberate mutants of csrc/tb_device.hpp, built one at a time outside the tree, case a) and test_gpu_parity's
test_forced_contacts_exercise_the_solver run once on each on an MI355X (lanes that left the oracle within the 8 steps, by region):

  1. near_net's x margin made negative (`contact_threshold - 1.0e-3f`: net contacts shallower than 0.33 mm are culled): all 8 cases
     of a) fail at step 0 -- n_face 28 / 31 lanes (Tennisbot / SwingRacket), n_tape 7 / 2, n_end_edge 1, n_foot 32 / 30, c_net 30,
     r_foot 31 / 33; today's forced batch fails too (its net third is on the x faces, -3 .. +0.6 mm).
  2. the interior tie order, `sz >= sx` made `sz > sx` in sphere_vs_box's nout == 0 branch: all 8 cases of a) fail at step 0, on ONE
     lane each -- n_inside's slot 0, where both separations are -1/32 exactly; today's forced batch PASSES.
  3. the goal's row set up with the court's restitution (both row placements): SwingRacket's 4 cases of a) fail -- c_top 58, c_wall
     57, c_rim 58, c_inside 58, c_axis 56, c_net 57 lanes, and one n_inside and one r_foot ball that reach a goal later; Tennisbot
     has no goal and passes; today's forced batch fails too (its goal third sits on the cap).
  4. the static friction rows visited in reverse order (goal, net, ground; both placements) -- a change that only a solve with
     two static rows can see: all 8 cases of a) fail at step 0 -- n_foot 48 / 46, r_foot 49 / 51, c_wall 43, c_net 48 lanes;
     today's forced batch PASSES (one static row per lane).
"""
import functools
import time

import numpy as np
import pytest

import test_gpu_policy_evaluate as pe
import test_gpu_sac_collect as sc
import test_gpu_sac_evaluate as ev
import test_static_contact_states as cs
from helpers import same_bits
from oracle import OracleBatch
from static_contact_fixtures import lane_order, static_contact_states
from test_gpu_parity import compare_state, same
from tennisbot_rl_amd.params import (COUNTER_NAMES, ENV_SWING, ENV_TENNIS, F_AUTO_RESET, F_DEFAULT, F_RACKET_GROUND, NET_DEFAULT, NET_TUNED, STATE_WORDS,
                                     default_params, reference_rolling_friction)

pytestmark = pytest.mark.gpu

DEV, NOISE_SEED, ENV_SEED, ID_BASE = ev.DEV, ev.NOISE_SEED, ev.ENV_SEED, ev.ID_BASE
T = cs.STEPS
KINDS = [ENV_TENNIS, ENV_SWING]
ORDERS = ["blocked", "interleaved"]
TWO_WAVE_SHORT = 2
NAME = {ENV_TENNIS: "Tennisbot", ENV_SWING: "SwingRacket"}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def params_of(variant):
    """"default", "altered" (h: other restitution and friction on court and goal), "extended" (g: racket<->court contact + rolling rows),
    or a TbParams of the caller's own (tests/test_gpu_racket_contacts.py: other outlines; for make_env, make_oracle and replay only --
    yardstick() caches by the variant's name and takes the three names alone)"""
    if not isinstance(variant, str):
        return variant.copy()
    if variant == "extended":
        return default_params(flags=F_DEFAULT | F_RACKET_GROUND, **reference_rolling_friction())
    return cs.altered(default_params()) if variant == "altered" else default_params()


def make_env(kind, n, variant="default", auto_reset=False, pipeline=False, **options):
    from tennisbot_rl_amd.stepper import BatchedEnv
    return BatchedEnv(kind, n, device=DEV, seed=ENV_SEED, env_id_base=ID_BASE, params=params_of(variant), auto_reset=auto_reset, pipeline=pipeline,
                      track_terminal_obs=False, options=options)


def make_oracle(kind, n, variant="default", auto_reset=False):
    p = params_of(variant)
    p.flags = (p.flags | F_AUTO_RESET) if auto_reset else (p.flags & ~F_AUTO_RESET)
    return OracleBatch(p, kind, n, seed=ENV_SEED, env_id_base=ID_BASE, precision="f32", threads=8)


def load(env, words, done):
    if isinstance(env, OracleBatch):
        env.set_state_words(words, done)
    else:
        env.set_state_words(words.view(np.int32), done)


def counters_of(ref):
    return dict(zip(COUNTER_NAMES, [int(x) for x in ref.counters()]))


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def yardstick(kind, order, step_count=None, auto_reset=False, variant="default", steps=T):
    """the float32 oracle from the forced states through cs.actions_of's actions, computed once and shared, read-only: dict of
    actions [S, n, A], obs / rew / done / sub [S, ...], words [S, W, n] and done bytes [S, n] after every step, counters"""
    words, done, _, _ = static_contact_states(kind, order, step_count=step_count)
    n = words.shape[1]
    acts = cs.actions_of(kind, n, steps)
    ref = make_oracle(kind, n, variant, auto_reset)
    ref.set_state_words(words, done)
    out = dict(actions=acts, obs=[], rew=[], done=[], sub=[], words=[], dbyte=[])
    for a in acts:
        o, r, d, s = ref.step(a)
        w, db = ref.get_state_words()
        for k, v in zip(("obs", "rew", "done", "sub", "words", "dbyte"), (o, r, d, s, w, db)):
            out[k].append(v.copy())
    out = {k: np.stack(v) if isinstance(v, list) else v for k, v in out.items()}
    frozen(*out.values())
    out["counters"] = counters_of(ref)
    ref.close()
    assert out["counters"]["nonfinite_states"] == 0
    return out


def state_is(env, want_words, want_done, what):
    """the handle's state against stored oracle words, as compare_state compares"""
    w, d = env.get_state_words()
    w = w.cpu().numpy().view(np.uint32)
    nw = STATE_WORDS[env.kind]
    same(w[nw - 2:], want_words[nw - 2:], what + " step_count/episode")
    same(d.cpu().numpy(), want_done, what + " done byte")
    same(w[: nw - 2].view(np.float32), want_words[: nw - 2].view(np.float32), what + " float state")


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)   # (a copy: the shared references are read-only)


def step_against(torch, env, y, what, substeps=True):
    """env through the yardstick's actions with tb_step: every output and the whole state after every step"""
    a_dev = dev(torch, y["actions"])
    for t in range(len(y["actions"])):
        o, r, d = env.step(a_dev[t].clone())
        tag = "%s step %d" % (what, t)
        same(d.cpu().numpy(), y["done"][t], tag + " done")
        if substeps:
            same(env.last_substeps().cpu().numpy(), y["sub"][t], tag + " substeps")
        same(o.cpu().numpy(), y["obs"][t], tag + " obs")
        same(r.cpu().numpy(), y["rew"][t], tag + " reward")
        state_is(env, y["words"][t], y["dbyte"][t], tag)


def differing_by_region(kind, order, wa, wb):
    """per region: (lanes that hit and approach, those whose state words differ between wa and wb) -- cs.acted's count, in this lane order"""
    _, _, region, names = static_contact_states(kind, order)
    app = cs.approaching(kind)[lane_order(kind, order)]
    differ = (wa != wb).any(0)
    return {name: (int(((region == k) & app).sum()), int(((region == k) & app & differ).sum())) for k, name in enumerate(names) if name != "high"}


# ------------------------------------------------------------------------------------------------------------------- a. and h.
@pytest.mark.parametrize("block", [64, 256])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", KINDS)
def test_tb_step_is_the_oracle(torch, kind, order, block):
    t0 = time.perf_counter()
    words, done, _, _ = static_contact_states(kind, order)
    n = words.shape[1]
    y = yardstick(kind, order)
    env = make_env(kind, n, block=block)
    load(env, words, done)
    what = "%s %s block %d" % (NAME[kind], order, block)
    step_against(torch, env, y, what)
    got = env.counters()
    assert got == y["counters"], (what, got, y["counters"])
    if kind == ENV_SWING:
        assert got["ball_court_terminations"] > 0 and got["goal_hits"] > 0 and got["timeouts"] > 0 and y["sub"].max() > 700
    if block == 64:   # h. the static rows ran on the device: a twin with other restitution and friction ends elsewhere
        twin = make_env(kind, n, "altered", block=block)
        load(twin, words, done)
        a_dev = dev(torch, y["actions"])
        for t in range(T):
            twin.step(a_dev[t].clone())
        by_region = differing_by_region(kind, order, env.get_state_words()[0].cpu().numpy(), twin.get_state_words()[0].cpu().numpy())
        twin.close()
        print("%s: (hit and approach, differ from the altered twin) %s" % (what, by_region))
        for name, (lanes, moved) in by_region.items():
            assert lanes >= 24 and 4 * moved >= 3 * lanes, (what, name, lanes, moved)
    env.close()
    print("%s: counters %s; %.2f s" % (what, got, time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------------------------- b.
@pytest.mark.parametrize("kind", KINDS)
def test_tb_rollout_is_the_oracle(torch, kind):
    """(tb_rollout needs auto-reset: its yardstick is the oracle with auto-reset, and a tb_step handle with it beside it)"""
    words, done, _, _ = static_contact_states(kind, "interleaved")
    n = words.shape[1]
    y = yardstick(kind, "interleaved", auto_reset=True)
    stepped = make_env(kind, n, auto_reset=True)
    load(stepped, words, done)
    step_against(torch, stepped, y, "%s tb_step with auto-reset" % NAME[kind])
    env = make_env(kind, n, auto_reset=True)
    load(env, words, done)
    obs, rew, dn = env.rollout(dev(torch, y["actions"]))
    torch.cuda.synchronize()
    same(dn.cpu().numpy(), y["done"], "rollout done")
    same(obs.cpu().numpy(), y["obs"], "rollout obs")
    same(rew.cpu().numpy(), y["rew"], "rollout reward")
    same(env.last_substeps().cpu().numpy(), y["sub"].sum(0).astype(np.int32), "rollout substeps")
    state_is(env, y["words"][-1], y["dbyte"][-1], "rollout final")
    assert env.counters() == y["counters"] and stepped.counters() == y["counters"]
    if kind == ENV_SWING:
        assert y["counters"]["episodes_finished"] > 100   # flights ended and envs restarted inside the launch
    env.close(); stepped.close()


# ------------------------------------------------------------------------------------------------------------------- c.
@pytest.mark.parametrize("waves", [1, 2])
@pytest.mark.parametrize("order", ORDERS)
def test_pipelined_short_steps(torch, order, waves):
    words, done, _, _ = static_contact_states(ENV_SWING, order, step_count=10)
    y = yardstick(ENV_SWING, order, step_count=10, auto_reset=True)
    env = make_env(ENV_SWING, words.shape[1], auto_reset=True, pipeline=True, step_waves=waves)
    assert env.step_waves() == waves
    load(env, words, done)
    assert env.phase() == 10
    a_dev = dev(torch, y["actions"])
    rews = []
    for t in range(T):
        if waves == 2:
            assert env.step_form() == TWO_WAVE_SHORT
        o, r, d = env.step(a_dev[t].clone())
        rews.append(r)
        tag = "pipelined %s waves %d step %d" % (order, waves, t)
        same(d.cpu().numpy(), y["done"][t], tag + " done")
        same(o.cpu().numpy(), y["obs"][t], tag + " obs")
        state_is(env, y["words"][t], y["dbyte"][t], tag)
    env.flush()
    same(torch.stack(rews).cpu().numpy(), y["rew"], "pipelined rewards")
    assert env.counters() == y["counters"] and env.phase() == 18 and not y["done"].any()
    env.close()


# ------------------------------------------------------------------------------------------------------------------- d.
@pytest.mark.parametrize("form,options", [("slots", dict(ff_defer=False)), ("slots+pool", dict(ff_defer=True)), ("pool", dict(ff_defer="all", ff_seal=True))])
@pytest.mark.parametrize("order", ORDERS)
def test_pipelined_episode_end_launch(torch, order, form, options):
    words, done, _, _ = static_contact_states(ENV_SWING, order, step_count=25)
    y = yardstick(ENV_SWING, order, step_count=25, auto_reset=True, steps=2)
    env = make_env(ENV_SWING, words.shape[1], auto_reset=True, pipeline=True, **options)
    assert env.pipeline_form() == form
    load(env, words, done)
    assert env.phase() == 25
    a_dev = dev(torch, y["actions"])
    outs = []
    for t in range(2):
        o, r, d = env.step(a_dev[t].clone())
        outs.append(r)
        same(d.cpu().numpy(), y["done"][t], "%s done %d" % (form, t))
        same(o.cpu().numpy(), y["obs"][t], "%s obs %d" % (form, t))
    env.flush()
    same(torch.stack(outs).cpu().numpy(), y["rew"], form + " rewards after flush")
    state_is(env, y["words"][-1], y["dbyte"][-1], form + " final")
    got, sealed = env.counters(), env.sealed_substeps()
    print("%s %s: counters %s, sealed substeps %d" % (form, order, got, sealed))
    assert got == y["counters"], (got, y["counters"])
    assert y["done"][0].all() and got["episodes_finished"] == words.shape[1] and got["timeouts"] > 0 and got["ball_court_terminations"] > 0 and got["goal_hits"] > 0
    assert 0 <= sealed < got["substeps"] and (form != "slots" or sealed == 0)
    env.close()


# ------------------------------------------------------------------------------------------------------------------- e.
def replay(torch, kind, words, done, variant, pipeline, actions, obs, rew, dn, env, what):
    """the loop kernel's reported actions through tb_step on a twin and through the oracle, from the same forced states: the twin
    and the oracle agree after every step, the kernel's rows are theirs, and the handle ends where the twin does, with its counters"""
    n = words.shape[1]
    twin, ref = make_env(kind, n, variant, auto_reset=True, pipeline=pipeline), make_oracle(kind, n, variant, auto_reset=True)
    load(twin, words, done); load(ref, words, done)
    a_dev = dev(torch, actions)
    rews = []
    for t in range(len(actions)):
        o, r, d = twin.step(a_dev[t].clone())
        o2, r2, d2, s2 = ref.step(actions[t])
        tag = "%s, tb_step against the oracle, step %d" % (what, t)
        same(d.cpu().numpy(), d2, tag + " done")
        same(o.cpu().numpy(), o2, tag + " obs")
        compare_state(twin, ref, tag)
        rews.append(r)
        same(obs[t], o2, "%s step %d obs" % (what, t))
        same(rew[t], r2, "%s step %d reward" % (what, t))
        same(dn[t] != 0, d2 != 0, "%s step %d done" % (what, t))
    if pipeline:
        twin.flush()
    same(torch.stack(rews).cpu().numpy(), rew, what + " rewards against tb_step")
    compare_state(env, ref, what + " final state")
    got, want = env.counters(), counters_of(ref)
    assert got == want and twin.counters() == want, (what, got, want)
    assert got["nonfinite_states"] == 0 and got["lockstep_violations"] == 0
    twin.close(); ref.close()
    return got


def loop_states(kind, variant="default"):
    """interleaved order; SwingRacket in lockstep at step_count = 10, pipelined"""
    swing = kind == ENV_SWING
    words, done, _, _ = static_contact_states(kind, "interleaved", step_count=10 if swing else None)
    return words, done, swing


def run_policy_rollout(torch, kind, net, slices, variant="default"):
    t0 = time.perf_counter()
    words, done, swing = loop_states(kind)
    w = pe.blob(torch, kind, net)
    env = make_env(kind, words.shape[1], variant, auto_reset=True, pipeline=swing, policy_slices=slices)
    load(env, words, done)
    (obs, rew, dn), (act, raw, logp, value) = env.policy_rollout(w, env.observe(), T, seed=NOISE_SEED, net=net)
    if swing:
        env.flush()
    torch.cuda.synchronize()
    assert torch.equal(act, raw.clamp(-1.0, 1.0)) and bool(torch.isfinite(logp).all()) and bool(torch.isfinite(value).all())
    what = "%s policy_rollout net=%d slices=%d %s" % (NAME[kind], net, slices, variant)
    got = replay(torch, kind, words, done, variant, swing, act.cpu().numpy(), obs.cpu().numpy(), rew.cpu().numpy(), dn.cpu().numpy(), env, what)
    env.close()
    print("%s: counters %s; %.2f s" % (what, got, time.perf_counter() - t0))


@pytest.mark.parametrize("kind,net,slices", [(ENV_TENNIS, NET_DEFAULT, 1), (ENV_TENNIS, NET_DEFAULT, 3), (ENV_TENNIS, NET_TUNED, 1), (ENV_TENNIS, NET_TUNED, 3),
                                             (ENV_SWING, NET_DEFAULT, 1)])
def test_policy_rollout_from_the_forced_states(torch, kind, net, slices):
    run_policy_rollout(torch, kind, net, slices)


@pytest.mark.parametrize("kind,uniform", [(ENV_TENNIS, False), (ENV_TENNIS, True), (ENV_SWING, False)])
def test_sac_collect_from_the_forced_states(torch, kind, uniform):
    t0 = time.perf_counter()
    words, done, swing = loop_states(kind)
    act = ev.actor(torch, kind, "plain")
    env = make_env(kind, words.shape[1], auto_reset=True, pipeline=swing)
    load(env, words, done)
    obs0 = env.observe().cpu().numpy()
    rec = sc.collect(torch, env, act.flat, (T,), uniform=uniform)
    if swing:
        env.flush()
    what = "%s sac_collect %s" % (NAME[kind], "uniform" if uniform else "actor")
    assert not any(np.isnan(rec[k]).any() for k in rec), what + ": a row was not written"
    assert same_bits(rec["obs"][0], obs0) and same_bits(rec["obs"][1:], rec["next_obs"][:-1])
    assert set(np.unique(rec["done"])) <= {0.0, 1.0} and np.abs(rec["action"]).max() <= 1.0
    got = replay(torch, kind, words, done, "default", swing, rec["action"], rec["next_obs"], rec["reward"], rec["done"], env, what)
    env.close()
    print("%s: counters %s; %.2f s" % (what, got, time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------------------------- f.
def test_swing_trace_from_the_forced_states(torch):
    stride, F = 16, 8
    words, done, _, _ = static_contact_states(ENV_SWING, "interleaved", step_count=25)
    n = words.shape[1]
    y = yardstick(ENV_SWING, "interleaved", step_count=25, steps=1)
    y24 = yardstick(ENV_SWING, "interleaved", step_count=24, steps=1)
    env = make_env(ENV_SWING, 7, auto_reset=True)
    env.reset()
    out = env.trace_step(dev(torch, y["actions"][0]), stride=stride, words=dev(torch, words.view(np.int32)), done=dev(torch, done), max_frames=F)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    env.close()
    same(got["substeps"], y["sub"][0], "trace substeps")
    same(got["done"], y["done"][0], "trace done")
    same(got["reward"], y["rew"][0], "trace reward")
    same(got["obs"], y["obs"][0], "trace obs")
    frames = got["frames"].view(np.uint32)
    assert frames.shape == (F, STATE_WORDS[ENV_SWING], n)
    same(frames[-1], y["words"][0], "the last frame against the oracle's final state")
    nw = STATE_WORDS[ENV_SWING]
    # frame 0: the state after the agent's substep -- what one step from step_count = 24 leaves (that step ends there: 25, not 26)
    same(frames[0][: nw - 2].view(np.float32), y24["words"][0][: nw - 2].view(np.float32), "frame 0 against the step from step_count 24")
    assert (y24["sub"][0] == 1).all() and (frames[0][nw - 2].view(np.int32) == 26).all() and (y24["words"][0][nw - 2].view(np.int32) == 25).all()
    ns = y["sub"][0]
    want_frames = 1 + (ns - 1) // stride + ((ns - 1) % stride != 0)
    same(got["n_frames"], want_frames.astype(np.int32), "n_frames")
    assert ns.min() == 2 and ns.max() == 776


# ------------------------------------------------------------------------------------------------------------------- g.
@pytest.mark.parametrize("kind", KINDS)
def test_extended_contact_set_tb_step(torch, kind):
    words, done, _, _ = static_contact_states(kind, "interleaved")
    y = yardstick(kind, "interleaved", variant="extended")
    env = make_env(kind, words.shape[1], "extended")
    load(env, words, done)
    step_against(torch, env, y, "%s extended" % NAME[kind])
    assert env.counters() == y["counters"]
    env.close()


@pytest.mark.parametrize("slices", [1, 3])
def test_extended_contact_set_policy_rollout(torch, slices):
    run_policy_rollout(torch, ENV_TENNIS, NET_DEFAULT, slices, variant="extended")
