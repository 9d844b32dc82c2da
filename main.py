#!/usr/bin/env python3
"""Counterpart of the reference's `main.py` on the batched MI355X envs.

  python main.py              # -s 0: agent.py's TRPOAgent on Tennisbot-v0 -- TRPOTrainer(form="agent_returns"), 10 iterations
  python main.py -s 1 -i 4    # -s 1: default PPO on Tennisbot-v0 (main.py:48-71: PPO("MlpPolicy", env), 25000 timesteps per iteration)
  python main.py --load       # go on from the checkpoint the last run left (agent.pt / ppo_agent.pt)

What is the reference's and what is not:
  * -s 0 is main.py:25-44: TRPOAgent with its defaults (trpo.AGENT_PY_DEFAULTS: discount 0.98, kl_delta 0.01, 10 CG iterations on 0.1
    of the rows, damping 0.001; log_std moved by the raw gradient, x^T F x over all rows, log_std starting at exp(-1)), the surrogate
    weighted by the discounted returns of finished episodes, no critic. An iteration is one rollout of --num-envs x --n-steps rows and
    one update, where the reference's is 5000 steps of one env (main.py:41).
  * The network: main.py:26-34 builds 9 -> 32 (tanh) -> 64 (ReLU) -> 2, which does not fit its own env -- Tennisbot-v0 observes 12
    numbers, not 9. The env's default network is used here: pi = [64, 64], tanh (ppo.TENNIS_DEFAULTS), the one the kernels are
    instantiated for.
  * max_episode_length = 2500 (main.py:43) is above the env's own limit of 1000 steps and never binds: it has no counterpart.
  * The endless rendering loop behind the training (main.py:75-84) has none either: this script ends when the training does.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TRPO, PPO = 0, 1                                          # main.py:12-14
CHECKPOINT = {TRPO: "agent.pt", PPO: "ppo_agent.pt"}      # main.py:39,44,54,71 (agent.pth, ppo_agent)
PPO_TIMESTEPS_PER_ITERATION = 25000                       # main.py:69


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--iteration", type=int, default=10)
    ap.add_argument("--load", action="store_true", help="load model")
    ap.add_argument("-s", "--strategy", type=int, default=0, help="0: for trpo, 1: for ppo")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--n-steps", type=int, default=128, help="agent steps per env per iteration; only episodes that end inside them are learned from under -s 0")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if args.strategy not in (TRPO, PPO):
        sys.exit("Invalid strategy: 0 for trpo, 1 for ppo")
    return args


def make_trainer(args, device):
    kw = dict(num_envs=args.num_envs, n_steps=args.n_steps, device=device, seed=args.seed)
    if args.strategy == TRPO:
        from tennisbot_rl_amd.trpo import TRPOTrainer
        return TRPOTrainer("Tennisbot-v0", form="agent_returns", **kw)
    from tennisbot_rl_amd.ppo import PPOTrainer
    return PPOTrainer("Tennisbot-v0", **kw)


def main(argv=None):
    args = parse_args(argv)
    import torch
    tr = make_trainer(args, torch.device("cuda", 0))
    path = CHECKPOINT[args.strategy]
    if args.load:
        print("loading previously trained %s model" % ("TRPO" if args.strategy == TRPO else "PPO"))
        tr.load(path)
    rollout = tr.n_steps * tr.num_envs
    for i in range(args.iteration):
        print("iteration: ", i)
        tr.learn(tr.num_timesteps + (rollout if args.strategy == TRPO else max(rollout, PPO_TIMESTEPS_PER_ITERATION)))
    tr.save(path)
    print("saved", path)
    tr.env.close()


if __name__ == "__main__":
    main()
