#!/usr/bin/env python3
"""Counterpart of the reference's train_es.py: evolution strategies with a GatedCNN policy, every generation's episodes on the GPU
(tennisbot_rl_amd/es.py, one tb_es_evaluate launch per generation). Same flags; --threads is accepted and ignored (the population
runs in one kernel launch, not in a process pool). Weights are saved as .npz (no pickle)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--environment", default="SwingRacket-v0", choices=("SwingRacket-v0", "Tennisbot-v0"))
    ap.add_argument("--popsize", type=int, default=200, help="antithetic pairs per generation")
    ap.add_argument("--print_every", type=int, default=1)
    ap.add_argument("--lr", type=float, default=0.2)
    ap.add_argument("--decay", type=float, default=0.995)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--generations", type=int, default=300)
    ap.add_argument("--folder", default="heb_coeffs", help="where the .npz weights are saved")
    ap.add_argument("--threads", type=int, default=-1, help="accepted and ignored: the population runs in one kernel launch")
    ap.add_argument("--repeats", type=int, default=10, help="episodes per member (the reference's repeat_j)")
    ap.add_argument("--elite", type=int, default=66, help="top pairs in the update")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--racket-ground", action="store_true", help="also simulate racket<->court contact (TB_F_RACKET_GROUND)")
    ap.add_argument("--rolling-friction", action="store_true", help="also solve the rolling-friction rows of every ball contact")
    args = ap.parse_args()
    if args.threads != -1:
        print("--threads %d ignored: every episode of a generation runs in one kernel launch" % args.threads)

    from tennisbot_rl_amd.es import ESTrainer
    params = None
    if args.racket_ground or args.rolling_friction:
        from tennisbot_rl_amd.params import F_DEFAULT, F_RACKET_GROUND, default_params, reference_rolling_friction
        params = default_params(flags=F_DEFAULT | (F_RACKET_GROUND if args.racket_ground else 0), **(reference_rolling_friction() if args.rolling_friction else {}))
    tr = ESTrainer(args.environment, popsize=args.popsize, repeats=args.repeats, elite=args.elite, sigma=args.sigma, lr=args.lr,
                   decay=args.decay, seed=args.seed, params=params)
    os.makedirs(args.folder, exist_ok=True)
    t0 = time.time()
    for g in range(args.generations):
        tr.step()
        if (g + 1) % args.print_every == 0 or g + 1 == args.generations:
            log = tr.log()
            print("generation %d  mean fitness %.3f  max %.3f  elite std %.3f%s  lr %.4f  sigma %.4f  %.1f s" % (
                log["generation"], log["mean"], log["max"], log["elite_std"], "  (update skipped: std 0)" if log["skipped"] else "",
                log["lr"], log["sigma"], time.time() - t0), flush=True)
            tr.save(os.path.join(args.folder, "%s__rew_%d__pop_%d__%d.npz" % (args.environment, int(log["mean"]), args.popsize, log["generation"])))
    tr.close()


if __name__ == "__main__":
    main()
