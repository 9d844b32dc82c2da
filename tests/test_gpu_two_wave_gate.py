"""The two-wave step kernel's common path is the one its launches take: tb_diag_two_wave_gate runs the kernel's own rare-path test
(tb_kernels.hpp, two_wave_rare) on the current state. In a random-action episode it passes every env in the 25 short steps, fails every
env at the 26th (the parking step), and fails exactly the envs whose ball was moved into the racket or onto the court."""
import numpy as np
import pytest

from tennisbot_rl_amd.params import ENV_SWING

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def test_two_wave_gate_passes_the_short_steps_and_stops_the_rest(torch):
    from tennisbot_rl_amd.stepper import BatchedEnv
    n = 4096
    env = BatchedEnv(ENV_SWING, n, device="cuda:0", seed=12, pipeline=True, track_terminal_obs=False)
    assert env.step_waves() == 2
    out = torch.empty(n, dtype=torch.uint8, device="cuda:0")

    def gate():
        assert env.L.tb_diag_two_wave_gate(env._h, out.data_ptr(), env._stream()) == 0
        torch.cuda.synchronize()
        return out.cpu().numpy().astype(bool)

    rng = np.random.default_rng(3)
    env.reset()
    for t in range(2 * 26):
        g = gate()
        if t % 26 < 25:
            assert not g.any(), (t, int(g.sum()))
        else:
            assert g.all(), (t, int((~g).sum()))
        env.step(torch.from_numpy(rng.uniform(-1, 1, (n, 6)).astype(np.float32)).cuda())
    for _ in range(10):
        env.step(torch.from_numpy(rng.uniform(-1, 1, (n, 6)).astype(np.float32)).cuda())
    assert not gate().any()
    w, d = env.get_state_words()
    f = w.cpu().numpy().copy().view(np.float32)
    face, low = np.arange(0, n, 7), np.arange(3, n, 29)
    f[13:16, face] = f[0:3, face]  # the ball's centre on the racket's: inside the slab
    f[15, low] = np.float32(0.05)
    env.set_state_words(f.view(np.int32), d.cpu().numpy())
    want = np.zeros(n, bool)
    want[face] = True
    want[low] = True
    assert np.array_equal(gate(), want)
    env.close()
