"""Data-parallel PPO with the fused learner over two ranks (the form of tests/test_gpu_ppo_dist.py: one process per rank, both on
cuda:0, gloo): each rank reduces its own partial gradients, ONE all-reduce of the flat gradient averages them, and the clip and
Adam kernels run on identical inputs -- so both ranks must finish with bit-identical weights while having stepped different envs."""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from tennisbot_rl_amd.ppo import PPOTrainer
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    tr = PPOTrainer("SwingRacket-v0", num_envs=512, n_steps=26, device="cuda:0", seed=5, batch_size=6656, learner="fused")
    assert tr.world == 2 and tr.rank == rank and tr.env.env_id_base == rank * 512 and tr._learner is not None
    start = torch.cat([p.detach().reshape(-1) for p in tr.policy.parameters()]).cpu().numpy()
    hist = tr.learn(2 * 512 * 26 * 3, log=None)  # three rollouts of the 1024-env global batch
    flat = torch.cat([p.detach().reshape(-1) for p in tr.policy.parameters()]).cpu().numpy()
    steps = {int(tr.opt.state[p]["step"]) for p in tr.policy.parameters()}
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), weights=flat, start=start, obs=tr.buf.obs.cpu().numpy(), timesteps=tr.num_timesteps,
             reward=np.float64(hist[-1]["mean_episode_reward"]), steps=np.array(sorted(steps)), grad=tr._learner.grad.cpu().numpy(),
             losses=np.array([[x["policy_loss"], x["value_loss"], x["entropy"]] for x in hist]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_fused_learner_keeps_replicas_in_sync(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(_free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert a["timesteps"] == b["timesteps"] == 2 * 512 * 26 * 3
    assert np.array_equal(a["weights"], b["weights"]), "replicas diverged: gradients were not averaged identically"
    assert np.array_equal(a["grad"], b["grad"])
    assert not np.array_equal(a["obs"], b["obs"]), "both ranks stepped the same envs"
    assert np.isfinite(a["weights"]).all() and np.isfinite(a["losses"]).all() and np.isfinite(b["losses"]).all()
    assert not np.array_equal(a["weights"], a["start"])
    assert list(a["steps"]) == list(b["steps"]) == [3 * 10 * 2]    # three rollouts x 10 epochs x 2 minibatches of 6656 rows
    assert not np.array_equal(a["losses"], b["losses"])            # each rank reports its own shard's statistics
