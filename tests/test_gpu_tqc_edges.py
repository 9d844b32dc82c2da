"""The TQC kernels where log_std clamps and tanh saturates, on the device.

TQC runs SAC's sample and head-backward kernels through its own launch code and workspace offsets and feeds logp' into 46 targets
per row. tests/test_gpu_tqc.py holds every stage to the float64 reference at rows whose log_std lies inside its clamp and whose
|g| <= 4; here the same stages run at the three edge fixtures of tests/test_tqc_edges_reference.py (`clamp`, `deep`, `band`: the
last catches only gross failures), both env kinds, B = 17, 65 and 257, the sibling's index vector over the fixture's first 257
rows, y [B, 46] through a guarded buffer. The tolerance is the sibling's: ppo_reference.MULTIPLE float32-twin errors per tensor;
no row is left out of any comparison. The largest ratios and what was seen of exactness in `deep` are printed at the end."""
import pytest

import edge_fixtures as ef
import edge_gpu_checks as eg
import tqc_reference as tr
from test_gpu_tqc import index_vector, make_tqc, same_bits, snapshot
from test_tqc_edges_reference import KINDS, fixture

pytestmark = pytest.mark.gpu

G = eg.Learner(name="tqc", mod=tr, fixture=fixture, make=make_tqc, workspace_bytes="tb_tqc_workspace_bytes", y_shape=lambda B: (B, tr.N_TARGETS), index_vector=index_vector,
               snapshot=snapshot, same_bits=same_bits)
CASES = [(w, k) for w in ef.FIXTURES for k in KINDS]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    G.report()


@pytest.mark.parametrize("which,kname", CASES)
def test_actor_forward_and_targets_at_the_edges(torch, which, kname):
    eg.actor_forward_and_targets(torch, G, which, kname)


@pytest.mark.parametrize("which,kname", CASES)
def test_actor_gradient_at_the_edges(torch, which, kname):
    eg.actor_gradient(torch, G, which, kname)


@pytest.mark.parametrize("which,kname", [(w, k) for w in ("clamp", "deep") for k in KINDS])
def test_gradient_step_at_the_edges_is_finite_and_is_the_stages(torch, which, kname):
    eg.whole_step(torch, G, which, kname)
