#!/usr/bin/env python3
"""Counterpart of the reference's train_es.py: evolution strategies with a GatedCNN policy, every generation's episodes on the GPU
(tennisbot_rl_amd/es.py, one tb_es_evaluate launch per generation). Same flags; --threads is accepted and ignored (the population
runs in one kernel launch, not in a process pool). Weights are saved as .npz (no pickle).

--policy mlp evolves the MlpPolicy ACTOR that PPO / TRPO train instead (tennisbot_rl_amd/policy_es.py, one
tb_policy_evaluate_members launch per generation: the members' networks on the matrix cores), optionally from a checkpoint
(--init); checkpoints are .pt files with the trainers' "policy" / "net" entries."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REPEATS = {"gatedcnn": 10, "mlp": 16}  # episodes per member: the reference's repeat_j; mlp: a multiple of the member granule (16)
REFERENCE_POLICY = os.path.join(ROOT, "tests", "golden", "ppo_swing_policy.npz")


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--environment", default="SwingRacket-v0", choices=("SwingRacket-v0", "Tennisbot-v0"))
    ap.add_argument("--policy", default="gatedcnn", choices=("gatedcnn", "mlp"), help="gatedcnn: the reference's ES policy; mlp: the MlpPolicy actor of PPO / TRPO")
    ap.add_argument("--popsize", type=int, default=200, help="antithetic pairs per generation")
    ap.add_argument("--print_every", type=int, default=1)
    ap.add_argument("--lr", type=float, default=0.2)
    ap.add_argument("--decay", type=float, default=0.995)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--generations", type=int, default=300)
    ap.add_argument("--folder", default="heb_coeffs", help="where the weights are saved (.npz; --policy mlp: .pt)")
    ap.add_argument("--threads", type=int, default=-1, help="accepted and ignored: the population runs in one kernel launch")
    ap.add_argument("--repeats", type=int, default=None, help="episodes per member (the reference's repeat_j): default 10; with --policy mlp 16, "
                    "and a multiple of 16 (a workgroup's 16 envs share one member's weights)")
    ap.add_argument("--elite", type=int, default=66, help="top pairs in the update")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--racket-ground", action="store_true", help="also simulate racket<->court contact (TB_F_RACKET_GROUND)")
    ap.add_argument("--rolling-friction", action="store_true", help="also solve the rolling-friction rows of every ball contact")
    ap.add_argument("--net", default="default", choices=("default", "tuned", "mlp64"), help="--policy mlp: the network (tuned: Tennisbot-v0, mlp64: SwingRacket-v0)")
    ap.add_argument("--init", default=None, metavar="PATH|reference", help="--policy mlp: start from a checkpoint of train_swing.py / train.py / this script; "
                    "`reference`: the reference's shipped ppo_swing policy (tests/golden/ppo_swing_policy.npz, SwingRacket-v0 with --net default only)")
    ap.add_argument("--stochastic", action="store_true", help="--policy mlp: members sample their actions (the policy's log_std) instead of acting on the mean")
    ap.add_argument("--curve", default=None, metavar="JSON", help="--policy mlp: also write every generation's log line to this file")
    return ap


def parse(argv=None):
    """the arguments with what depends on --policy resolved"""
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.repeats is None:
        args.repeats = REPEATS[args.policy]
    if args.policy != "mlp" and (args.net != "default" or args.init is not None or args.stochastic or args.curve):
        ap.error("--net / --init / --stochastic / --curve belong to --policy mlp")
    args.init_name = args.init   # (as given: what a --curve file records)
    if args.init == "reference":
        if args.environment != "SwingRacket-v0" or args.net != "default":
            ap.error("--init reference is SwingRacket-v0's default network")
        args.init = REFERENCE_POLICY
    return args


def engine_params(args):
    if not (args.racket_ground or args.rolling_friction):
        return None
    from tennisbot_rl_amd.params import F_DEFAULT, F_RACKET_GROUND, default_params, reference_rolling_friction
    return default_params(flags=F_DEFAULT | (F_RACKET_GROUND if args.racket_ground else 0), **(reference_rolling_friction() if args.rolling_friction else {}))


def main():
    args = parse()
    if args.threads != -1:
        print("--threads %d ignored: every episode of a generation runs in one kernel launch" % args.threads)

    mlp = args.policy == "mlp"
    if mlp:
        from tennisbot_rl_amd.policy_es import PolicyESTrainer
        tr = PolicyESTrainer(args.environment, net=args.net, popsize=args.popsize, repeats=args.repeats, elite=args.elite, sigma=args.sigma, lr=args.lr,
                             decay=args.decay, seed=args.seed, deterministic=not args.stochastic, init=args.init, params=engine_params(args))
    else:
        from tennisbot_rl_amd.es import ESTrainer
        tr = ESTrainer(args.environment, popsize=args.popsize, repeats=args.repeats, elite=args.elite, sigma=args.sigma, lr=args.lr,
                       decay=args.decay, seed=args.seed, params=engine_params(args))
    os.makedirs(args.folder, exist_ok=True)
    t0 = time.time()
    curve = []
    for g in range(args.generations):
        tr.step()
        if (g + 1) % args.print_every == 0 or g + 1 == args.generations:
            log = tr.log()
            print("generation %d  mean fitness %.3f  max %.3f  elite std %.3f%s  lr %.4f  sigma %.4f  %.1f s" % (
                log["generation"], log["mean"], log["max"], log["elite_std"], "  (update skipped: std 0)" if log["skipped"] else "",
                log["lr"], log["sigma"], time.time() - t0), flush=True)
            curve.append(dict(log, seconds=time.time() - t0))
            name = "%s__rew_%d__pop_%d__%d" % (args.environment, int(log["mean"]), args.popsize, log["generation"])
            tr.save(os.path.join(args.folder, name + (".pt" if mlp else ".npz")))
    if mlp and args.curve:
        import json
        with open(args.curve, "w") as f:
            json.dump({"policy": args.policy, "environment": args.environment, "net": args.net, "init": args.init_name, "popsize": args.popsize, "repeats": args.repeats,
                       "elite": args.elite, "sigma": args.sigma, "lr": args.lr, "decay": args.decay, "seed": args.seed, "deterministic": not args.stochastic,
                       "generations": curve}, f, indent=1)
    tr.close()


if __name__ == "__main__":
    main()
