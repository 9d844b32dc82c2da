"""The TQC edge fixtures (tests/edge_fixtures.py: `clamp`, `deep`, `band`) that tests/test_gpu_tqc_edges.py runs on the device, and
proof on the CPU that they can fail. Everything here runs without a GPU.

TQC runs SAC's sample and head-backward kernels through its own launch code and workspace offsets, and feeds logp' into 46 targets
per row; the existing fixtures (tests/test_tqc_reference.py) keep log_std inside its clamp and |g| <= 4. These three are built from
test_tqc_reference.fixture with tqc_reference's functions exactly as tests/test_sac_edges_reference.py builds SAC's (there is no
critic minimum, so no KINK_Q). Asserted here, for both env kinds:

  * the margins: KINK >= 100 x the float32-twin error of the hidden pre-activations and KINK_RAW of the raw log_std, MEASURED on
    the fixture's own pool of 4096 candidates; for `deep` the pre-activations' error over the candidates that pass the fixture's
    conditions on log_std and g (test_sac_edges_reference's docstring says why), the pool-wide figure printed beside it;
  * at least 257 rows kept, ordered so that the first 17, 65 and 257 each hold every sort of entry the fixture is for in both
    actor passes, and so does every batch the GPU tests draw;
  * the float64 run and the float32 twin take the same side of every ReLU and of both clamp edges on every kept row;
  * the six mutants lie more than ref.MULTIPLE = 24 twin errors from the float64 reference at 17, 65 and 257 rows.

Measured (swing / tennis), with the constants below:
  rows kept of 4096     clamp 831 / 1396,  deep 786 / 1273,  band 430 / 662
  twin error, pool      clamp z 2.89e-6 / 2.12e-6, raw log_std 3.74e-5 / 1.80e-5;  band z 5.12e-6 / 4.24e-6, raw log_std 5.2e-7 / 2.9e-7
  twin error, deep      z 2.59e-6 / 2.12e-6 over the candidates (pool-wide 5.85e-5 / 3.60e-5)
  twin error of what the GPU tests compare, 257 rows: clamp logp 4.9e-5 / 1.2e-5, gradients 2.4e-6 / 8.0e-7 (entries up to 4.2);
                        deep logp 8.1e-6 / 2.7e-6, gradients 8.9e-7 (entries up to 0.57); band logp 0.18 / 0.19, gradients 0.061 / 0.033
  smallest mutant ratio over both kinds, 17 / 65 / 257 rows, the prefixes and the GPU batches (allowed to pass: 24):
      (i) not zeroed 5.53e5   (ii) zeroed below only 6.79e4   (iii) zeroed above only 5.53e5   (iv) no low clamp 9.02e5
      (v) softplus squash 5.96e8   (vi) no epsilon: infinite (0 / 0 = NaN in every saturated column)
  Tennisbot's `clamp` binds above in 4 % of the entries only (113 of 1396 kept rows hold one in the pass on s): the ordering
  puts such rows into every prefix and every GPU batch, a blind draw of 17 would miss them half the time.
(the tests print all of these figures; the ones above are those of the day the module was written)
"""
import functools

import pytest

import edge_fixtures as ef
import test_tqc_reference as base
import tqc_reference as tr

KINDS = base.KINDS
ALGO = ef.Algo("tqc", tr, base, qgap=False)
# >= 100 x the measured float32-twin errors (asserted below)
KINK = {"clamp": 3.0e-4, "deep": 3.0e-4, "band": 5.2e-4}
KINK_RAW = {"clamp": 4.0e-3, "deep": 3.0e-4, "band": 3.0e-4}
CASES = [(w, k) for w in ef.FIXTURES for k in KINDS]


@functools.lru_cache(maxsize=None)
def fixture(which, kname):
    return ef.build(ALGO, kname, which, KINK[which], KINK_RAW[which])


@pytest.mark.parametrize("which,kname", CASES)
def test_edge_fixture_margins_rows_and_sides(which, kname):
    ef.check_fixture(ALGO, fixture(which, kname), base.POOL)


@pytest.mark.parametrize("which,kname", [c for c in CASES if ef.MUTANTS[c[0]]])
def test_mutants_lie_beyond_the_tolerance(which, kname):
    ef.check_mutants(ALGO, fixture(which, kname))
