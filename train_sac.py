#!/usr/bin/env python3
"""`-s sac` of the reference's train.py / train_swing.py on the batched MI355X envs: SB3's SAC with MlpPolicy, its gradient step
as HIP kernels (tennisbot_rl_amd/sac.py, csrc/tb_sac.hpp).

  python train_sac.py                                  # SwingRacket-v0, 256 envs, batch 1100 (train_swing.py:93-96)
  python train_sac.py --env Tennisbot-v0 --curri       # batch 256 (train.py:129-130), the racket-size curriculum

Hyper-parameters are SB3 1.8.0's SAC defaults as the reference leaves them (lr 3e-4, gamma 0.99, tau 0.005, ent_coef "auto",
buffer_size 1e6, learning_starts 100). One vector step collects --num-envs transitions and runs --gradient-steps gradient steps
(default: one per transition, the reference's update-to-data ratio); with --collect-form fused it is --collect-steps env steps in
one launch and --gradient-steps gradient steps per env step. Checkpoints hold the learner, the replay ring AND the env
batch state. One rank only. TQC (train_swing.py only) is train_tqc.py.

  python train_sac.py --population 16 --num-envs 256 --member-lr 1e-4,3e-4,...   # 16 learners side by side, one set of launches

--population M trains M learners on one GPU (tennisbot_rl_amd/sac_population.py): --num-envs stays the total, --total-timesteps
and --learning-starts count each member's own timesteps, --gradient-steps defaults to the envs per member; --member-lr /
--member-gamma / --member-tau give per-member values, --pbt-every K exploits and explores every K vector steps. It writes the
population checkpoint to --save and the best member, in the trainer's own format, to best_model.pt beside it, at the end and
every --save-freq of a member's timesteps (the same two files each time, not rl_model_<timesteps>_steps.pt).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tennisbot_rl_amd.evaluation import add_schedule_arguments, resolve_load, schedule_from_args  # noqa: E402
from train_swing import racket_scale_for  # noqa: E402  (train.py:164-176, one table for every script)


def off_policy_parser(description, algo, batch_help, total_default, total_help):
    """the arguments of train_sac.py and train_tqc.py"""
    ap = argparse.ArgumentParser(description=description)
    ap.add_argument("--env", default="SwingRacket-v0", choices=["SwingRacket-v0", "Tennisbot-v0"])
    ap.add_argument("--num-envs", type=int, default=256)
    ap.add_argument("--batch-size", type=int, default=None, help=batch_help)
    ap.add_argument("--gradient-steps", type=int, default=None, help="gradient steps per vector step (default: --num-envs, one per transition)")
    ap.add_argument("--buffer-size", type=int, default=1_000_000)
    ap.add_argument("--learning-starts", type=int, default=100, help="timesteps of uniform actions before the first gradient step")
    ap.add_argument("--total-timesteps", type=float, default=total_default, help=total_help)
    ap.add_argument("--curri", action="store_true", help="curriculum learning: size change of racket (Tennisbot-v0)")
    ap.add_argument("--load", type=str, default=None, help="checkpoint written by --save; `best`: best_model.pt beside --save (written under --eval-freq)")
    ap.add_argument("--save", type=str, default=None, help="default: ./model/%s_<env id>.pt" % algo.lower())
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log-json", type=str, default=None)
    ap.add_argument("--racket-ground", action="store_true", help="also simulate racket<->court contact (TB_F_RACKET_GROUND)")
    ap.add_argument("--rolling-friction", action="store_true", help="also solve the rolling-friction rows of every ball contact")
    add_schedule_arguments(ap)
    ap.add_argument("--eval-form", choices=["torch", "fused"], default="torch", help="how --eval-freq's whole episodes run: `torch` steps a separate batch with "
                    "the torch actor; `fused` runs every episode of a batch in one launch with the actor inside (tb_sac_evaluate)")
    ap.add_argument("--collect-form", choices=["torch", "fused"], default="torch", help="how transitions are collected: `torch` runs the torch actor between "
                    "single env steps; `fused` runs --collect-steps env steps in one launch with the actor inside, straight into the replay ring (tb_sac_collect)")
    ap.add_argument("--collect-steps", type=int, default=1, help="env steps per vector step with --collect-form fused (--gradient-steps stays per env step)")
    from tennisbot_rl_amd.sac_population import add_population_arguments
    add_population_arguments(ap)
    return ap


def trainer_arguments(args):
    """the trainer's keyword arguments that come straight from the parsed command line"""
    return dict(num_envs=args.num_envs, batch_size=args.batch_size, gradient_steps=args.gradient_steps, buffer_size=args.buffer_size,
                learning_starts=args.learning_starts, seed=args.seed, eval_form=args.eval_form, collect_form=args.collect_form, collect_steps=args.collect_steps)


def off_policy_main(argv, script, algo, trainer, description, batch_help, total_default, total_help, total_by_env):
    """the body of train_sac.py and train_tqc.py. trainer() returns the trainer class (called after the arguments are parsed, so
    that --help needs no torch); algo names it in messages and in the default --save path; total_by_env: the timesteps per env id
    where --total-timesteps is not given (its own default is total_default)."""
    args = off_policy_parser(description, algo, batch_help, total_default, total_help).parse_args(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("%s runs on one rank: multi-rank %s is not provided" % (script, algo))

    from tennisbot_rl_amd.sac_population import population_keywords
    try:
        population = population_keywords(args)
    except ValueError as e:
        sys.exit("%s: %s" % (script, e))
    if population is not None and (args.curri or args.eval_freq or args.collect_form != "torch" or args.collect_steps != 1 or args.load == "best"):
        sys.exit("%s: --population takes no --curri, --eval-freq, --collect-form fused, --collect-steps or --load best (not provided for a population)" % script)

    import torch

    total = args.total_timesteps or total_by_env.get(args.env, 0)
    params = None
    if args.racket_ground or args.rolling_friction:
        from tennisbot_rl_amd.params import F_DEFAULT, F_RACKET_GROUND, default_params, reference_rolling_friction
        params = default_params(flags=F_DEFAULT | (F_RACKET_GROUND if args.racket_ground else 0), **(reference_rolling_friction() if args.rolling_friction else {}))
    path = args.save or "./model/%s_%s.pt" % (algo.lower(), args.env)
    if population is not None:
        from tennisbot_rl_amd.sac_population import PopulationSAC, run_population
        pop = PopulationSAC(args.env, algo=algo.lower(), batch_size=args.batch_size, gradient_steps=args.gradient_steps, buffer_size=args.buffer_size,
                            learning_starts=args.learning_starts, seed=args.seed, params=params, device=torch.device("cuda", 0), **population)
        if args.load:
            pop.load(args.load)
        history = run_population(pop, total, path, save_freq=int(args.save_freq))   # --save-freq: in a member's own timesteps, like --total-timesteps
        if args.log_json:
            json.dump(history, open(args.log_json, "w"))
        return
    tr = trainer()(args.env, params=params, device=torch.device("cuda", 0), **trainer_arguments(args))
    if args.load:
        tr.load(resolve_load(args.load, path))
    schedule = schedule_from_args(args, path)
    if schedule is not None:
        schedule.reset(tr.num_timesteps)
    history = []
    chunk = 10 * tr.num_envs
    while tr.num_timesteps < total:
        if args.curri and args.env == "Tennisbot-v0":
            tr.env.set_racket_scale(racket_scale_for(100.0 * tr.num_timesteps / total))
        history += tr.learn(min(total, tr.num_timesteps + chunk), schedule=schedule)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tr.save(path)
    if args.eval_freq:
        print("saved", path, "eval (%d whole episodes, %s policy):" % (args.n_eval_episodes, "deterministic" if args.eval_deterministic else "stochastic"),
              tr.evaluate_episodes(args.n_eval_episodes, deterministic=args.eval_deterministic))
    else:
        print("saved", path, "eval (stochastic policy, as EvalCallback in the reference):", tr.evaluate())
    if args.log_json:
        json.dump(history, open(args.log_json, "w"))


def _trainer():
    from tennisbot_rl_amd.sac import SACTrainer
    return SACTrainer


PARSER = ("SAC on SwingRacket-v0 or Tennisbot-v0 (the reference's -s sac)", "SAC", "default: 1100 on SwingRacket-v0, 256 on Tennisbot-v0, as the reference scripts", None,
          "default: 2e6 SwingRacket-v0 / 1e6 Tennisbot-v0, as the reference")   # off_policy_parser's arguments


def main(argv=None):
    off_policy_main(argv, "train_sac.py", "SAC", _trainer, PARSER[0], PARSER[2], PARSER[3], PARSER[4], {"SwingRacket-v0": 2e6, "Tennisbot-v0": 1e6})


if __name__ == "__main__":
    main()
