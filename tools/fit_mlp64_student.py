#!/usr/bin/env python3
"""How tests/golden/mlp64_swing_student.npz was made: a [64, 64] tanh actor-critic (SB3's default net on SwingRacket-v0, NET_MLP64)
fitted to the reference's shipped ppo_swing policy (tests/golden/ppo_swing_policy.npz, [32, 64, 32]). No GPU needed.

  data     the teacher acts stochastically on the float32 CPU oracle (oracle.OracleBatch, SwingRacket-v0, 1024 envs, env seed 3,
           torch seed 0) for 52 steps = two episodes; the 53 248 observations it met are the inputs
  targets  the teacher's action means and values on those observations
  loss     mean squared error of the means + 1e-3 x that of the values
  fit      Adam, lr 2e-3, 3000 steps on minibatches of 2048 rows drawn with torch.randint; SB3's orthogonal init
  log_std  copied from the teacher
  check    26-step episodes of 64 oracle envs (env seed 11): teacher, student and the student's deterministic actions each finish
           64 of 64 episodes with a non-zero return (printed) -- what the fixture is for: tests/test_gpu_mlp64_policy.py needs a
           [64, 64] policy whose rackets meet the ball, and a randomly initialised one's never do (every return 0)

    python tools/fit_mlp64_student.py [--out tests/golden/mlp64_swing_student.npz]

The keys of the file are the module's state_dict names. A rerun with the same torch build reproduced the committed file bit for bit (the
loss ends near 4e-4); another build's matrix products may round differently, and the tests do not depend on the exact weights, only on
the student striking balls, which they assert."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def episodes(policy, n, seed, deterministic):
    """returns of one 26-step episode per env on the CPU oracle"""
    import torch
    from oracle import OracleBatch
    from tennisbot_rl_amd.params import ENV_SWING, F_AUTO_RESET, F_DEFAULT, default_params
    env = OracleBatch(default_params(flags=F_DEFAULT | F_AUTO_RESET), ENV_SWING, n, seed=seed, precision="f32")
    obs, ret = env.reset(), np.zeros(n)
    with torch.no_grad():
        for _ in range(26):
            a, _, _ = policy.act(torch.from_numpy(obs), deterministic=deterministic)
            obs, r, _, _ = env.step(a.clamp(-1, 1).numpy().astype(np.float32))
            ret += r
    return ret


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mlp64_swing_student.npz"))
    ap.add_argument("--steps", type=int, default=3000)
    args = ap.parse_args()
    import torch
    from oracle import OracleBatch
    from tennisbot_rl_amd.params import ENV_SWING, F_AUTO_RESET, F_DEFAULT, default_params
    from tennisbot_rl_amd.ppo import SB3_SWING_DEFAULTS, SWING_DEFAULTS, build_actor_critic
    torch.manual_seed(0)
    teacher = build_actor_critic(6, 6, tuple(SWING_DEFAULTS["net_arch"])).load_sb3_arrays(dict(np.load(os.path.join(ROOT, "tests", "golden", "ppo_swing_policy.npz"))))
    env = OracleBatch(default_params(flags=F_DEFAULT | F_AUTO_RESET), ENV_SWING, 1024, seed=3, precision="f32")
    obs, seen = env.reset(), []
    with torch.no_grad():
        for _ in range(52):
            seen.append(obs.copy())
            a, _, _ = teacher.act(torch.from_numpy(obs))
            obs, _, _, _ = env.step(a.clamp(-1, 1).numpy().astype(np.float32))
        X = torch.from_numpy(np.concatenate(seen))
        M, V = teacher(X)
    student = build_actor_critic(6, 6, tuple(SB3_SWING_DEFAULTS["net_arch"]))
    opt = torch.optim.Adam(student.parameters(), lr=2e-3)
    for it in range(args.steps):
        idx = torch.randint(0, X.shape[0], (2048,))
        m, v = student(X[idx])
        loss = ((m - M[idx]) ** 2).mean() + 1e-3 * ((v - V[idx]) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        if it % 500 == 0 or it == args.steps - 1:
            print("step %4d  loss %.6f" % (it, float(loss.detach())))
    with torch.no_grad():
        student.log_std.copy_(teacher.log_std)
    for name, policy, det in (("teacher", teacher, False), ("student", student, False), ("student, deterministic", student, True)):
        ret = episodes(policy, 64, 11, det)
        print("%-24s non-zero returns %d of 64, mean %.2f" % (name, int((ret != 0).sum()), ret.mean()))
    np.savez(args.out, **{k: v.numpy() for k, v in student.state_dict().items()})
    print("wrote", args.out)


if __name__ == "__main__":
    main()
