"""The SAC edge fixtures (tests/edge_fixtures.py: `clamp`, `deep`, `band`) that tests/test_gpu_sac_edges.py runs on the device, proof on
the CPU that they can fail, and the replay ring against a Python-list model. Everything here runs without a GPU.

The existing fixtures (tests/test_sac_reference.py) keep a row only if log_std lies INSIDE its clamp and |g| <= 4, so the clamp's
bound branches and a saturated squash never ran. These three start from the same nets, pool, critic, target and log_ent_coef and
change only the actor's heads (see edge_fixtures' docstring). Asserted here, for both env kinds:

  * the margins: KINK >= 100 x the float32-twin error of the hidden pre-activations, KINK_Q of Q, KINK_RAW of the raw log_std,
    each MEASURED on the fixture's own pool of 4096 candidates. For `deep` the error of the pre-activations and of Q is taken over
    the candidates that pass the fixture's conditions on log_std and g, not over the whole pool: where an odd column is NOT
    saturated the x 1000 head carries a float32 error of 1e-3 in g, hence in a~ and in the critics' first layer (4e-5 pool-wide,
    which would ask a margin that no row of any pool survives), but such a row is rejected by |g| >= 18 in float64 with a margin
    of thousands of twin errors, and where the column IS saturated a~ is +-1 exactly in both precisions. The pool-wide figure is
    printed beside it;
  * at least 257 rows kept, ordered so that the first 17, 65 and 257 each hold every sort of entry the fixture is for, in the
    pass on s and in the pass on s', and so does every batch the GPU tests draw (rows 0 and 256 hold them between the two);
  * the float64 run and the float32 twin take the same side of every ReLU, of the critic minimum and of both clamp edges
    (three-valued) on EVERY kept row;
  * six mutants, each a float32 evaluation with one line changed, lie more than ref.MULTIPLE = 24 twin errors from the float64
    reference at 17, 65 and 257 rows, on the prefixes and on the GPU tests' own batches.

Measured (swing / tennis), with the constants below:
  rows kept of 4096     clamp 708 / 1073,  deep 897 / 1232,  band 288 / 400
  twin error, pool      clamp z 3.48e-6 / 2.62e-6, Q 5.87e-7 / 3.24e-7, raw log_std 3.94e-5 / 2.35e-5
                        band  z 6.30e-6 / 3.63e-6, Q 7.80e-7 / 4.23e-7, raw log_std 5.3e-7 / 4.4e-7
  twin error, deep      z 2.19e-6 / 2.62e-6, Q 2.84e-7 / 2.99e-7 over the candidates (pool-wide z 3.98e-5 / 4.39e-5, Q 5.97e-6 / 5.54e-6)
  twin error of what the GPU tests compare, 257 rows: clamp logp 4.3e-5 / 2.9e-5, gradients 2.1e-6 / 7.9e-7 (entries up to 3.4);
                        deep logp 6.7e-6 / 1.7e-6, gradients 8.9e-7 (entries up to 0.57); band logp 0.22 / 0.10, gradients 0.058 / 0.024
  entries bound below / above (clamp, pass on s)  18 % / 20 % (swing), 20 % / 21 % (tennis); beyond 45 / 89 (deep) 48 % / 44 %, 44 % / 37 %
  smallest mutant ratio over both kinds, 17 / 65 / 257 rows, the prefixes and the GPU batches (allowed to pass: 24):
      (i) not zeroed 1.35e6   (ii) zeroed below only 1.43e6   (iii) zeroed above only 1.92e5   (iv) no low clamp 1.19e6
      (v) softplus squash 6.2e8   (vi) no epsilon: infinite (0 / 0 = NaN in every saturated column)
  KINK for `band` (6.4e-4 against 6.30e-6 measured) leaves SwingRacket 288 rows: 257 are needed, the margin is not widened.
(the tests print all of these figures; the ones above are those of the day the module was written)
"""
import functools

import pytest

import edge_fixtures as ef
import sac_reference as sr
import test_sac_reference as base

KINDS = base.KINDS
ALGO = ef.Algo("sac", sr, base, qgap=True)
# >= 100 x the measured float32-twin errors (asserted below)
KINK = {"clamp": 3.5e-4, "deep": 3.0e-4, "band": 6.4e-4}
KINK_Q = {"clamp": 6.0e-5, "deep": 5.0e-5, "band": 8.0e-5}
KINK_RAW = {"clamp": 4.0e-3, "deep": 3.0e-4, "band": 3.0e-4}
CASES = [(w, k) for w in ef.FIXTURES for k in KINDS]


@functools.lru_cache(maxsize=None)
def fixture(which, kname):
    return ef.build(ALGO, kname, which, KINK[which], KINK_RAW[which], KINK_Q[which])


@pytest.mark.parametrize("which,kname", CASES)
def test_edge_fixture_margins_rows_and_sides(which, kname):
    ef.check_fixture(ALGO, fixture(which, kname), base.POOL)


@pytest.mark.parametrize("which,kname", [c for c in CASES if ef.MUTANTS[c[0]]])
def test_mutants_lie_beyond_the_tolerance(which, kname):
    ef.check_mutants(ALGO, fixture(which, kname))


# --------------------------------------------------------------------------------------------------------------- the replay ring
class RingModel:
    """the ring as a Python list: slot -> the number of the transition it holds (None: never written)"""

    def __init__(self, capacity):
        self.capacity, self.slots, self.pos, self.size = capacity, [None] * capacity, 0, 0

    def add(self, numbers):
        for k in numbers:
            self.slots[self.pos] = k
            self.pos = (self.pos + 1) % self.capacity
            self.size = min(self.capacity, self.size + 1)


def transitions(torch, first, n, O=3, A=2):
    """n transitions numbered first .. first + n - 1, the number written into EVERY field of its row (done: number % 2, as uint8)"""
    k = torch.arange(first, first + n, dtype=torch.float32)
    return k[:, None].repeat(1, O) + 0.25, k[:, None].repeat(1, O) + 0.5, k[:, None].repeat(1, A) + 0.75, k + 0.125, (k.long() % 2).to(torch.uint8)


def check_ring(R, model):
    assert R.pos == model.pos and R.size == model.size
    for slot, k in enumerate(model.slots):
        got = [float(R.obs[slot, 0]), float(R.obs[slot, -1]), float(R.next_obs[slot, 0]), float(R.next_obs[slot, -1]), float(R.action[slot, 0]), float(R.action[slot, -1]),
               float(R.reward[slot]), float(R.done[slot])]
        want = [0.0] * 8 if k is None else [k + 0.25, k + 0.25, k + 0.5, k + 0.5, k + 0.75, k + 0.75, k + 0.125, float(k % 2)]
        assert got == want, "slot %d holds %s, the model says transition %s" % (slot, got, k)


def filled(torch, capacity, adds):
    from tennisbot_rl_amd.sac import ReplayBuffer
    R, model, first = ReplayBuffer(3, 2, capacity, "cpu"), RingModel(capacity), 0
    for n in adds:
        R.add(*transitions(torch, first, n))
        model.add(range(first, first + n))
        first += n
        check_ring(R, model)
    return R, model


def test_ring_add_wraps_where_the_model_does():
    import torch
    from tennisbot_rl_amd.sac import ReplayBuffer
    R, model = filled(torch, 10, (4, 4, 4, 4))           # the third add crosses the end
    assert (R.pos, R.size) == (6, 10) and model.slots == [10, 11, 12, 13, 14, 15, 6, 7, 8, 9]
    R, model = filled(torch, 8, (8, 3))                  # n == capacity, then on top of it
    assert (R.pos, R.size) == (3, 8) and model.slots == [8, 9, 10, 3, 4, 5, 6, 7]
    R, model = filled(torch, 8, (8,))
    assert (R.pos, R.size) == (0, 8)
    R = ReplayBuffer(3, 2, 7, "cpu")
    with pytest.raises(ValueError, match="do not fit"):
        R.add(*transitions(torch, 0, 8))
    assert (R.pos, R.size) == (0, 0) and not bool(R.obs.any())
    with pytest.raises(ValueError, match="capacity"):
        ReplayBuffer(3, 2, 0, "cpu")


def test_ring_sample_stays_inside_the_filled_part():
    import torch
    from tennisbot_rl_amd.sac import ReplayBuffer
    with pytest.raises(ValueError, match="empty"):
        ReplayBuffer(3, 2, 10, "cpu").sample(4)
    torch.manual_seed(0)
    for adds, size in (((4,), 4), ((4, 4), 8), ((4, 4, 4), 10), ((4, 4, 4, 4), 10)):     # before and after the wrap
        R, _ = filled(torch, 10, adds)
        idx = R.sample(4000)
        assert idx.dtype == torch.int64 and tuple(idx.shape) == (4000,)
        assert int(idx.min()) == 0 and int(idx.max()) == size - 1, "4000 draws over %d slots reach 0 and size - 1 (the chance that they do not is below 1e-170)" % size


def test_ring_state_dict_round_trip_before_and_after_the_wrap():
    import torch
    from tennisbot_rl_amd.sac import ReplayBuffer
    for adds in ((4,), (4, 4), (4, 4, 4), (4, 4, 4, 4)):
        R, model = filled(torch, 10, adds)
        sd = R.state_dict()
        assert sd["pos"] == R.pos and sd["size"] == R.size and sd["capacity"] == 10 and all(len(a) == R.size for a in sd["arrays"])
        other = ReplayBuffer(3, 2, 10, "cpu")
        other.load_state_dict(sd)
        check_ring(other, model)
        assert all(torch.equal(a, b) for a, b in zip(R.arrays(), other.arrays()))
        with pytest.raises(ValueError, match="capacity"):
            ReplayBuffer(3, 2, 11, "cpu").load_state_dict(sd)
    R, model = filled(torch, 8, (8, 3))                  # a full ring whose cursor is not 0
    other = ReplayBuffer(3, 2, 8, "cpu")
    other.load_state_dict(R.state_dict())
    check_ring(other, model)
    other.add(*transitions(torch, 11, 2))                # ... and the loaded ring goes on where the saved one would
    model.add(range(11, 13))
    check_ring(other, model)
