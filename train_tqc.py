#!/usr/bin/env python3
"""`-s tqc` of the reference's train_swing.py on the batched MI355X envs: sb3_contrib's TQC with MlpPolicy, its gradient step as
HIP kernels (tennisbot_rl_amd/tqc.py, csrc/tb_tqc.hpp on csrc/tb_sac.hpp).

  python train_tqc.py                                  # SwingRacket-v0, 256 envs, batch 256 (train_swing.py:98-99)
  python train_tqc.py --env Tennisbot-v0 --curri       # the racket-size curriculum

Hyper-parameters are sb3_contrib 1.8.0's TQC defaults as the reference leaves them (25 quantiles, 2 critics, 2 dropped per net,
lr 3e-4, gamma 0.99, tau 0.005, ent_coef "auto", batch_size 256, buffer_size 1e6, learning_starts 100). One vector step collects
--num-envs transitions and runs --gradient-steps gradient steps (default: one per transition, the reference's update-to-data
ratio). Checkpoints hold the learner, the replay ring AND the env batch state. One rank only.
"""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from train_sac import off_policy_main  # noqa: E402  (one body for both off-policy scripts)


def _trainer():
    from tennisbot_rl_amd.tqc import TQCTrainer
    return TQCTrainer


PARSER = ("TQC on SwingRacket-v0 or Tennisbot-v0 (the reference's train_swing.py -s tqc)", "TQC", "default: 256, sb3_contrib's, as the reference script leaves it", 2e6,
          "default: 2e6, as the reference")   # off_policy_parser's arguments


def main(argv=None):
    off_policy_main(argv, "train_tqc.py", "TQC", _trainer, PARSER[0], PARSER[2], PARSER[3], PARSER[4], {})


if __name__ == "__main__":
    main()
