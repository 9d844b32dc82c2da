"""The SAC kernels where log_std clamps and tanh saturates, and the replay ring where it wraps, on the device.

tests/test_gpu_sac.py holds every stage to the float64 reference at rows whose log_std lies inside its clamp and whose |g| <= 4.
Here the same stages run at the three edge fixtures of tests/test_sac_edges_reference.py (`clamp`: both sides of the clamp bind;
`deep`: the squash is saturated in the odd columns of every row, |g| up to about 1000; `band`: the transition zone, which
catches only gross failures), both env kinds, B = 17 (one past the 16-row tile), 65 (one past a workgroup's 64 rows) and 257 (one
past the 256-thread blocks of the row kernels, the first batch in the loss kernels' strided loop), the sibling's index vector over
the fixture's first 257 rows. The tolerance is the sibling's: ppo_reference.MULTIPLE float32-twin errors per tensor; no row is
left out of any comparison. The largest ratios and what was seen of exactness in `deep` are printed at the end of the module.

The ring: a SACTrainer whose capacity (1000) is no multiple of its 64 envs wraps in the middle of its 16th add."""
import numpy as np
import pytest

import edge_fixtures as ef
import edge_gpu_checks as eg
import sac_reference as sr
from test_gpu_sac import index_vector, make_sac, same_bits, snapshot
from test_sac_edges_reference import KINDS, fixture

pytestmark = pytest.mark.gpu

DEV = eg.DEV
G = eg.Learner(name="sac", mod=sr, fixture=fixture, make=make_sac, workspace_bytes="tb_sac_workspace_bytes", y_shape=lambda B: (B,), index_vector=index_vector,
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


# --------------------------------------------------------------------------------------------------------------- the replay ring
def test_trainer_ring_wraps_in_the_middle_of_an_add(torch, tmp_path):
    from tennisbot_rl_amd.sac import SACTrainer
    n, cap, steps = 64, 1000, 20
    kw = dict(num_envs=n, buffer_size=cap, batch_size=64, gradient_steps=1, learning_starts=64, device=DEV)
    t = SACTrainer("SwingRacket-v0", seed=3, **kw)
    R = t.replay
    model = [h.clone() for h in R.arrays()]                    # the ring as the adds below should leave it
    assert cap % n != 0 and all(not bool(x.any()) for x in model)
    split = []
    for k in range(steps):
        prev = t.obs.clone()
        a, obs, r, d = t.vector_step()
        slots = torch.arange(k * n, (k + 1) * n, device=DEV) % cap
        split.append(bool(slots[-1] < slots[0]))
        for dst, src in zip(model, (prev, obs, a, r, d.float())):
            dst[slots] = src
        # the 64 rows just written sit where the model says, and every other row is unchanged
        assert all(torch.equal(x[slots], src) for x, src in zip(R.arrays(), (prev, obs, a, r, d.float()))), "step %d: the rows just written are not where they belong" % (k + 1)
        assert all(torch.equal(x, y) for x, y in zip(R.arrays(), model)), "step %d: the ring is not the model's" % (k + 1)
        assert R.pos == ((k + 1) * n) % cap and R.size == min(cap, (k + 1) * n)
    assert split == [k == 15 for k in range(steps)], "the 16th add, and it alone, is split across the ring's end"
    assert R.size == 1000 and R.pos == 1280 % 1000 and t.num_timesteps == 1280
    L = t._learner
    assert L.step == steps - 1
    assert all(np.isfinite(x).all() for x in snapshot(L)), "the learner's state is not finite"
    path = str(tmp_path / "sac_ring.pt")
    t.save(path)
    other = SACTrainer("SwingRacket-v0", seed=91, **kw).load(path)
    assert other.replay.pos == R.pos and other.replay.size == R.size and other._learner.step == L.step
    assert all(torch.equal(x, y) for x, y in zip(R.arrays(), other.replay.arrays()))
    torch.manual_seed(5)
    idx = R.sample(64)
    assert int(idx.min()) >= 0 and int(idx.max()) < 1000
    idx[0], idx[1] = 0, cap - 1                                     # both ends of the full ring
    eps = torch.randn((2, 64, t.env.act_dim), device=DEV)
    for x in (t, other):
        x._learner.gradient_step(x.replay.arrays(), idx, eps[0], eps[1])
    assert same_bits(snapshot(L), snapshot(other._learner)), "the loaded trainer's next gradient step gave other bits"
    for x in (t, other):
        x.env.close()
