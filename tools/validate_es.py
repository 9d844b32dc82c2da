#!/usr/bin/env python3
"""Mean return of the reference's shipped ES policy (tests/golden/es_swing_policy.npz, exported from backup_models/es_swing.dat)
over many SwingRacket-v0 episodes, each with a fresh normaliser (evaluate_es.py's protocol), in one tb_es_evaluate call:
    python tools/validate_es.py [--episodes 65536]
The file name's rew_30 is the generation-101 POPULATION mean fitness the reference logged when it saved the weights: printed
beside the figure as context, not as a target (a population mean is not the centre's return)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tennisbot_rl_amd.stepper import BatchedEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--episodes", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "es_swing_policy.npz"))
    w = torch.zeros((1, 768), device="cuda:0")
    w[0, :766] = torch.from_numpy(z["weights"]).cuda()
    env = BatchedEnv("SwingRacket-v0", args.episodes, device="cuda:0", seed=args.seed, pipeline=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ret, length = env.es_evaluate(w, args.episodes)
    r = ret.reshape(-1).cpu().numpy()
    dt = time.perf_counter() - t0
    c = env.counters()
    env.close()
    print("policy: %s (sha256 %s...)" % (z["member"], str(z["sha256"])[:16]))
    print("episodes: %d (seed %d), %.3f s" % (r.size, args.seed, dt))
    print("mean return: %.4f  (std %.4f, standard error %.4f; min %.3f, max %.3f)" % (r.mean(), r.std(), r.std() / np.sqrt(r.size), r.min(), r.max()))
    print("goal hits: %d of %d episodes" % (c["goal_hits"], r.size))
    print("context: the file name's rew_30 = generation-101 population mean fitness as the reference logged it (not a pin)")


if __name__ == "__main__":
    main()
