"""What the forced Tennisbot contact states with low rackets (helpers.racket_contact_states(low_rackets=True)) reach, on the float32
oracle alone: conditions on the INPUTS of tests/test_gpu_tennis_extended_loops.py, not measurements of the code under test. That file
holds the kernels to the oracle bit for bit on this batch; this one makes sure the batch is worth it -- racket<->court contact
points cached and kept, caches that fill up, the racket<->court rows and the rolling rows both changing where envs end up, racket<->ball
contacts, a cached court point and a ball contact in one solve, and episodes that end and restart inside the 12 steps.

Every threshold is half of what the oracle shows with the committed builder (written next to it), so that a change of the
builder, of the seed or of the engine that thins the batch out fails here, on the CPU, and not silently on the GPU."""
import numpy as np

from helpers import LOW_RACKET_STEPS, low_racket_batch, low_racket_params
from oracle import OracleBatch
from tennisbot_rl_amd.params import COUNTER_NAMES, ENV_TENNIS, F_AUTO_RESET, F_RACKET_GROUND

# measured on the float32 oracle with the committed builder (2048 envs, 12 steps) / the threshold: half of it
MEASURED = dict(
    court_point_envs=460,                    # envs holding a cached racket<->court point before their first done        -> 230
    full_cache_envs=31,                      # ... whose cache reached all 4 points                                      -> 15
    differ_without_rg=335,                   # envs whose final state words differ from the run without F_RACKET_GROUND  -> 167
    differ_without_rolling=568,              # ... from the run without the rolling-friction rows                        -> 284
    racket_ball_contact_substeps=1489,       # the counter                                                               -> 744
    episodes_restarted=475,                  # episodes ended and restarted inside the 12 steps (all pass-racket)        -> 237
    court_point_and_ball_contact_envs=216)   # a cached court point and a racket<->ball contact in one step's solve      -> 108
AT_LEAST = {k: v // 2 for k, v in MEASURED.items()}
AT_LEAST["court_point_and_ball_contact_envs"] = max(16, AT_LEAST["court_point_and_ball_contact_envs"])  # the multi-row solve: never fewer than 16


def run(params, words, done, actions, watch=False):
    """the oracle from these words through these actions: (final words, done bytes, counters by name[, the per-env reach])"""
    n = words.shape[1]
    pf = params.copy()
    pf.flags |= F_AUTO_RESET
    ref = OracleBatch(pf, ENV_TENNIS, n, seed=11, precision="f32", threads=8)
    ref.set_state_words(words, done)
    running = np.ones(n, bool)                       # before the env's first done
    point, full, both = (np.zeros(n, bool) for _ in range(3))
    for a in actions:
        _, rew, d, _ = ref.step(a)
        if watch:
            running &= d == 0                        # (an env that restarts has an empty cache: only steps before that count)
            cached = np.array([len(ref.manifold(i)[0]) if running[i] else 0 for i in range(n)])
            point |= cached > 0
            full |= cached == 4
            both |= (cached > 0) & (rew >= 25.0)     # step_count >= 5: a reward of 25 or more is a racket<->ball contact in this substep
    w, db = ref.get_state_words()
    c = dict(zip(COUNTER_NAMES, [int(x) for x in ref.counters()]))
    ref.close()
    return (w, db, c, dict(point=point, full=full, both=both)) if watch else (w, db, c)


def measure(n=2048):
    words, done, actions = low_racket_batch(n)
    p = low_racket_params()
    w, _, c, reach = run(p, words, done, actions, watch=True)
    no_rg = p.copy()
    no_rg.flags &= ~F_RACKET_GROUND
    w_rg, _, _ = run(no_rg, words, done, actions)
    no_roll = p.copy()
    no_roll.roll_racket = no_roll.roll_court = no_roll.roll_goal = 0.0
    w_roll, _, _ = run(no_roll, words, done, actions)
    got = dict(court_point_envs=int(reach["point"].sum()), full_cache_envs=int(reach["full"].sum()),
               differ_without_rg=int((w != w_rg).any(0).sum()), differ_without_rolling=int((w != w_roll).any(0).sum()),
               racket_ball_contact_substeps=c["racket_ball_contact_substeps"], episodes_restarted=c["episodes_finished"],
               court_point_and_ball_contact_envs=int(reach["both"].sum()))
    return got, c


def test_low_racket_batch_reaches_what_the_gpu_tests_rely_on():
    got, c = measure()
    print("low-racket batch on the oracle: %s; counters %s" % (got, c))
    assert len(low_racket_batch(2048)[2]) == LOW_RACKET_STEPS
    assert c["nonfinite_states"] == 0
    assert c["episodes_finished"] == c["pass_racket_terminations"], "an episode ended on something else than the ball passing the racket"
    for k, least in AT_LEAST.items():
        assert got[k] >= least, "%s: %d, the batch should reach %d (half of the %d measured when it was built)" % (k, got[k], least, MEASURED[k])
    assert got["court_point_and_ball_contact_envs"] >= 16

