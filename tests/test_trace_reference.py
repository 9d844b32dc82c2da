"""tb_swing_trace's reference, without a GPU: the sampling rule (stepper.trace_frame_substeps) on hand-worked cases, the oracle helper
of tests/trace_reference.py against the oracle's own uninterrupted step, the four hand-built flights and their outcomes, and the
properties the GPU tests rely on in the mixed batches (a flight with a racket contact in it, every ending, a contact bonus)."""
import numpy as np
import pytest

import trace_reference as tr
from tennisbot_rl_amd.params import COUNTER_NAMES, default_params
from tennisbot_rl_amd.stepper import trace_frame_substeps

AMPLE = 2 + 775   # room for every substep of the longest step and a row to spare


def test_sampling_rule_on_hand_worked_cases():
    f = trace_frame_substeps
    assert f(1, 1, 1) == [1] and f(1, 8, 3) == [1, 1, 1] and f(1, 10000, 2) == [1, 1]
    assert f(2, 1, 2) == [1, 2] and f(2, 1, 1) == [2] and f(2, 7, 3) == [1, 2, 2] and f(2, 776, 2) == [1, 2]
    assert f(9, 8, 2) == [1, 9] and f(9, 7, 3) == [1, 8, 9] and f(9, 7, 2) == [1, 9] and f(9, 7, 1) == [9] and f(9, 7, 5) == [1, 8, 9, 9, 9]
    assert f(9, 1, 3) == [1, 2, 9] and f(9, 1, 9) == list(range(1, 10)) and f(9, 775, 3) == [1, 9, 9] and f(9, 10000, 1) == [9]
    long8 = f(776, 8, 98)
    assert long8 == list(range(1, 770, 8)) + [776] and len(long8) == 98 and tr.n_samples(776, 8) == 98
    assert f(776, 8, 3) == [1, 9, 776] and f(776, 8, 99)[-2:] == [776, 776] and f(776, 8, 97) == list(range(1, 762, 8)) + [776]
    assert f(776, 7, 2) == [1, 776] and tr.n_samples(776, 7) == 112   # 1 + 7 j <= 776: j <= 110, and 771 is not 776
    assert f(776, 775, 3) == [1, 776, 776] and f(776, 776, 3) == [1, 776, 776] and f(776, 10000, 1) == [776]
    assert f(776, 1, AMPLE) == list(range(1, 777)) + [776]
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(ValueError):
            f(*bad)


@pytest.mark.parametrize("ns", [1, 2, 9, 776])
def test_sampling_rule_against_its_statement(ns):
    """the rule as include/tb_stepper.h words it, built here from a set"""
    for stride in (1, 7, 8, 775, 776, 10000):
        want = sorted({1 + j * stride for j in range(ns) if 1 + j * stride <= ns} | {ns})
        m = 1 + (ns - 1) // stride + ((ns - 1) % stride != 0)
        assert len(want) == m == tr.n_samples(ns, stride)
        for F in (1, 2, 3, AMPLE):
            got = trace_frame_substeps(ns, stride, F)
            assert len(got) == F and got[-1] == ns
            assert got == (want + [ns] * (F - m) if m <= F else want[:F - 1] + [ns]), (ns, stride, F)


@pytest.fixture(scope="module")
def fixtures():
    words, done, actions, outcomes = tr.swing_fixtures()
    return tr.TraceOracle(default_params(), words, done, actions), outcomes


def test_the_hand_built_flights_end_as_stated(fixtures):
    o, outcomes = fixtures
    for i, (ns, reward, ending) in enumerate(outcomes):
        assert o.substeps[i] == ns and o.done[i] == 1, (i, o.substeps[i])
        if reward is not None:
            assert o.reward[i] == np.float32(reward)
        one = tr.TraceOracle(default_params(), o.words[:, i:i + 1], None, o.actions[i:i + 1])
        c = dict(zip(COUNTER_NAMES, one.counters))
        assert c[ending] == 1 and sum(c[k] for k in ("ball_court_terminations", "goal_hits", "timeouts")) == 1, (i, c)
        assert c["racket_ball_contact_substeps"] == 0   # (none of them meets the racket: it is out of reach or swings past)


def test_a_copy_cut_at_the_last_substep_is_the_uninterrupted_step(fixtures):
    """k = ns - 1 flight substeps: the copy reports ns substeps, and every row but the step count is the oracle's own final state"""
    o, _ = fixtures
    pairs = [(i, int(o.substeps[i])) for i in range(o.n)]
    idx, w = o._cut_words(pairs)
    _, _, done, sub, out, _ = o._step(w, np.zeros(o.n, np.uint8), o.actions[idx])
    assert np.array_equal(sub, o.substeps) and (done == 1).all()
    keep = np.arange(tr.W) != tr.ROW_STEP
    assert np.array_equal(out[keep], o.final[keep])
    assert np.array_equal(out[tr.ROW_STEP].view(np.int32), np.full(o.n, 801))   # the copies all ran into the 800-limit ...
    assert np.array_equal(o.final[tr.ROW_STEP].view(np.int32), 25 + o.substeps)  # ... the step itself counts from its own 25


def test_frames_follow_the_rule_and_meet_the_final_state(fixtures):
    o, _ = fixtures
    for stride, F in ((1, AMPLE), (8, 99), (8, 3), (775, 2), (7, 1)):
        fr, nf, steps = o.frames(stride, F)
        assert fr.shape == (F, tr.W, o.n) and np.array_equal(nf, [tr.n_samples(int(ns), stride) for ns in o.substeps])
        keep = np.arange(tr.W) != tr.ROW_STEP
        for i in range(o.n):
            assert list(steps[:, i]) == trace_frame_substeps(int(o.substeps[i]), stride, F)
            assert np.array_equal(fr[-1, :, i], o.final[:, i])   # the last stored row is the final state, step count included
            assert np.array_equal(fr[:, tr.ROW_STEP, i].view(np.int32), 25 + steps[:, i])
            assert np.array_equal(fr[:, tr.W - 1, i], np.full(F, o.words[tr.W - 1, i]))   # the episode word never changes
            for k in range(F):   # unstored rows are copies of the final row
                if steps[k, i] == o.substeps[i]:
                    assert np.array_equal(fr[k, :, i], o.final[:, i])
        # a ball in flight moves: consecutive distinct samples differ in the ball's position
        z = fr[:, 15, 1].view(np.float32)   # the falling ball of fixture 1
        assert (np.diff(z[:min(F, int(nf[1]))]) < 0).all()


@pytest.mark.parametrize("name", list(tr.param_sets()))
def test_the_mixed_batches_hold_what_the_gpu_tests_rely_on(name):
    params, seed = tr.param_sets()[name]
    words, done, actions = tr.mixed_batch(params, seed)
    o = tr.TraceOracle(params, words, done, actions)
    c = dict(zip(COUNTER_NAMES, o.counters))
    assert o.flight_contact_substeps() > 0, "no flight with a racket contact in it"
    assert c["ball_court_terminations"] > 0 and c["goal_hits"] > 0 and c["timeouts"] > 0 and c["nonfinite_states"] == 0
    step0 = words[tr.ROW_STEP].view(np.int32)
    flight = (step0 == 25) & (done == 0)
    assert (o.substeps[flight] > 1).all() and (o.substeps[~flight] == 1).all() and o.substeps.max() == 776
    assert set(step0[~flight & (done == 0)]) == {0, 10, 24}
    assert sorted(done[done != 0]) == [1, 2] and (o.done[done != 0] == 1).all() and (o.done[~flight & (done == 0)] == 0).all()
    bonus = o.reward[~flight] == 2.0
    assert bonus.sum() >= 2 and set(step0[~flight][bonus]) == {0, 10}   # step 24 becomes 25: the bonus window has closed
    for n in (1, 5, 64, 65):   # the prefixes the GPU tests take keep the mix
        f = flight[:n]
        assert f[0] and (n == 1 or (~f).any())
    assert flight[:64].any() and (~flight[:64]).any() and (~flight[64:]).any()
