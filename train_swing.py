#!/usr/bin/env python3
"""Counterpart of the reference's `train_swing.py` / `train.py` on the batched MI355X envs.

  python train_swing.py                      # PPO on SwingRacket-v0, 4096 envs on cuda:0
  python train_swing.py --env Tennisbot-v0 --curri
  torchrun --nproc-per-node 8 train_swing.py # one process per GPU, sharded envs
  python train_swing.py -s trpo --trpo-form sb3 --net mlp64   # the reference's `-s trpo`: sb3_contrib's TRPO on SB3's [64, 64] net
  python train_swing.py -s trpo --trpo-form agent_returns     # agent.py's own estimator: discounted returns of finished episodes, no critic
  python train_swing.py --population 4 --member-lr 1e-4,3e-4,1e-3,3e-3 --pbt-every 4   # 4 PPO learners side by side, 1024 envs each

Hyper-parameters follow train_swing.py:46-50,80-91 (net_arch pi=vf=[32,64,32], ent_coef 0.002,
total_timesteps 2e6) and train.py:76-80,104-110 (Tennisbot: 64-64, ent_coef 0.01, 1e6); the
rollout is n_steps per env x num_envs instead of 1100 x 1. `--curri` is the racket-size
curriculum of train.py:155-176 (progress thresholds -> racket scale, applied at each env's
next reset). Checkpoints hold the learner AND the env batch state.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CURRICULUM = ((3, 3.0), (5, 2.6), (10, 2.3), (15, 2.1), (25, 1.9), (45, 1.7), (70, 1.3), (101, 1.0))  # train.py:164-176 (% progress, scale)


def racket_scale_for(progress_percent):
    for limit, scale in CURRICULUM:
        if progress_percent < limit:
            return scale
    return 1.0


TRPO_FLAGS = ("kl_delta", "cg_iterations", "cg_damping", "cg_state_percent", "discount", "log_std_step", "step_rows")


def trpo_keywords(args):
    """TRPOTrainer's keywords from the command line: the form, the net, and of the trust-region flags only those given explicitly --
    the others are left to the form's preset (trpo.TRPO_DEFAULTS / trpo.SB3_TRPO_DEFAULTS / trpo.AGENT_PY_DEFAULTS), so a flag always wins over it"""
    kw = dict(form=args.trpo_form, policy=args.net)
    kw.update({k: getattr(args, k) for k in TRPO_FLAGS if getattr(args, k) is not None})
    return kw


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="SwingRacket-v0", choices=["SwingRacket-v0", "Tennisbot-v0"])
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--n-steps", type=int, default=104, help="agent steps per env per rollout (4 SwingRacket episodes)")
    ap.add_argument("--total-timesteps", type=float, default=None, help="default: 2e6 Swing / 1e6 Tennisbot, as the reference")
    ap.add_argument("--load", type=str, default=None, help="checkpoint written by --save; `best`: best_model.pt beside --save (written under --eval-freq)")
    ap.add_argument("--load-reference", action="store_true", help="warm start from the reference's shipped ppo_swing policy (tests/golden/ppo_swing_policy.npz)")
    ap.add_argument("--save", type=str, default=None, help="default: ./model/ppo_%%s.pt, or ./model/trpo_%%s.pt under -s trpo (%%s: the env id)")
    ap.add_argument("--curri", action="store_true", help="curriculum learning: size change of racket (Tennisbot-v0)")
    ap.add_argument("--gui", action="store_true", help="accepted for CLI compatibility; there is no GUI")
    ap.add_argument("-s", "--select", default="ppo", help="ppo or trpo (train_swing.py:102; tennisbot_rl_amd/trpo.py); sac and tqc have their own scripts, train_sac.py and train_tqc.py")
    ap.add_argument("--trpo-form", default="agent", choices=["agent", "sb3", "agent_returns"],
                    help="trpo: agent = the reference's agent.py (TRPOAgent) with GAE and a critic; sb3 = sb3_contrib's TRPO, what the reference's train_swing.py -s trpo runs; "
                         "agent_returns = agent.py's own estimator, discounted returns of finished episodes and no critic (tennisbot_rl_amd/trpo.py)")
    ap.add_argument("--net", default="default", choices=["default", "mlp64"],
                    help="mlp64: SB3's MlpPolicy default pi = vf = [64, 64] on SwingRacket-v0 (on Tennisbot-v0 the default net is that one)")
    ap.add_argument("--kl-delta", type=float, default=None, help="trpo: the trust region's KL bound (default 0.01, agent.py:17; sb3: 0.01)")
    ap.add_argument("--cg-iterations", type=int, default=None, help="trpo: conjugate-gradient iterations (default 10; sb3: 15)")
    ap.add_argument("--cg-damping", type=float, default=None, help="trpo: damping added to the Fisher-vector product (default 0.001; sb3: 0.1)")
    ap.add_argument("--cg-state-percent", type=float, default=None, help="trpo: share of the rollout's rows the Fisher-vector products run over (default 0.1; sb3: 1.0)")
    ap.add_argument("--discount", type=float, default=None, help="trpo, agent_returns: the returns' discount (default 0.98, agent.py:17)")
    ap.add_argument("--log-std-step", default=None, choices=["natural", "raw"],
                    help="trpo: natural = log_std inside the natural gradient; raw = moved by the surrogate's raw gradient, agent.py:120,136 (default natural; agent_returns: raw)")
    ap.add_argument("--step-rows", default=None, choices=["cg", "all"],
                    help="trpo: the rows of the x^T F x behind the step size: the CG rows, or all rows as agent.py:110-111 (default cg; agent_returns: all)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--racket-ground", action="store_true", help="also simulate racket<->court contact (court.urdf:19-24; TB_F_RACKET_GROUND, opt-in: DESIGN.md section 3)")
    ap.add_argument("--rolling-friction", action="store_true", help="also solve the rolling-friction rows of every ball contact (rollingFriction=.001 in racket.py:43-45, objects.py:29-31,48-50)")
    ap.add_argument("--no-fused", action="store_true", help="run the policy as torch modules between env steps instead of inside the step kernel")
    ap.add_argument("--learner", default=None, choices=["torch", "fused"], help="ppo (default torch): fused = GAE, minibatch gradient and Adam as HIP kernels (tennisbot_rl_amd/learner.py); trpo has the fused learner only")
    ap.add_argument("--log-json", type=str, default=None)
    from tennisbot_rl_amd.evaluation import add_schedule_arguments
    from tennisbot_rl_amd.population import add_population_arguments, population_keywords
    add_schedule_arguments(ap)
    add_population_arguments(ap)
    args = ap.parse_args(argv)
    try:
        args.population_keywords = population_keywords(args, args.select)
    except ValueError as exc:
        sys.exit(str(exc))
    if args.population_keywords is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("--population runs on one rank: multi-GPU populations are not provided")
    if args.select not in ("ppo", "trpo"):
        sys.exit("only -s ppo and -s trpo are implemented on the batched envs by this script. SAC: train_sac.py; TQC: train_tqc.py")
    if args.select == "trpo" and args.learner == "torch":
        sys.exit("-s trpo has no torch learner: its update runs as HIP kernels (leave --learner out, or --learner fused)")
    if args.select == "trpo" and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("-s trpo runs on one rank: multi-rank TRPO is not provided")
    if args.select != "trpo" and args.trpo_form != "agent":
        sys.exit("--trpo-form belongs to -s trpo")
    if args.select != "trpo" and (args.discount is not None or args.log_std_step or args.step_rows):
        sys.exit("--discount, --log-std-step and --step-rows belong to -s trpo")
    if args.discount is not None and args.trpo_form != "agent_returns":
        sys.exit("--discount belongs to --trpo-form agent_returns (the other forms discount with PPO's gamma)")
    if args.net == "mlp64" and args.env != "SwingRacket-v0":
        sys.exit("--net mlp64 is SwingRacket-v0's: on Tennisbot-v0 the default net already is SB3's [64, 64]")
    if args.save is None:
        args.save = "./model/%s_%%s.pt" % args.select
    return args


def main():
    from tennisbot_rl_amd.evaluation import resolve_load, schedule_from_args
    args = parse_args()

    import torch
    from tennisbot_rl_amd.ppo import PPOTrainer

    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.distributed.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    total = args.total_timesteps or (2e6 if args.env == "SwingRacket-v0" else 1e6)
    params = None
    if args.racket_ground or args.rolling_friction:
        from tennisbot_rl_amd.params import F_DEFAULT, F_RACKET_GROUND, default_params, reference_rolling_friction
        params = default_params(flags=F_DEFAULT | (F_RACKET_GROUND if args.racket_ground else 0), **(reference_rolling_friction() if args.rolling_friction else {}))
    if args.population_keywords is not None:
        from tennisbot_rl_amd.population import PopulationPPO, run_population
        pop = PopulationPPO(args.env, n_steps=args.n_steps, net=args.net, device=torch.device("cuda", local_rank), seed=args.seed, params=params,
                            **args.population_keywords)
        path = args.save % args.env if "%s" in args.save else args.save
        if args.load:
            pop.load(args.load)
        history = run_population(pop, total, path, save_freq=args.save_freq)
        if args.log_json:
            json.dump(history, open(args.log_json, "w"))
        return
    if args.select == "trpo":
        from tennisbot_rl_amd.trpo import TRPOTrainer
        tr = TRPOTrainer(args.env, num_envs=args.num_envs, n_steps=args.n_steps, device=torch.device("cuda", local_rank), seed=args.seed, fused=not args.no_fused,
                         params=params, **trpo_keywords(args))
    else:
        tr = PPOTrainer(args.env, num_envs=args.num_envs, n_steps=args.n_steps, device=torch.device("cuda", local_rank), seed=args.seed,
                        fused=not args.no_fused, params=params, learner=args.learner or "torch", policy=args.net)
    if args.load_reference:
        import numpy as np
        tr.policy.load_sb3_arrays(dict(np.load(os.path.join(ROOT, "tests", "golden", "ppo_swing_policy.npz"))))
    path = args.save % args.env if "%s" in args.save else args.save
    if args.load:
        tr.load(resolve_load(args.load, path))
    schedule = schedule_from_args(args, path)
    if schedule is not None:
        schedule.reset(tr.num_timesteps)
    history = []
    while tr.num_timesteps < total:
        if args.curri and args.env == "Tennisbot-v0":
            tr.env.set_racket_scale(racket_scale_for(100.0 * tr.num_timesteps / total))
        history += tr.learn(min(total, tr.num_timesteps + tr.n_steps * tr.num_envs * world), schedule=schedule)
    if tr.rank == 0:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tr.save(path)
        if args.eval_freq:
            print("saved", path, "eval (%d whole episodes, %s policy):" % (args.n_eval_episodes, "deterministic" if args.eval_deterministic else "stochastic"),
                  tr.evaluate_episodes(args.n_eval_episodes, deterministic=args.eval_deterministic))
        else:
            print("saved", path, "eval (stochastic policy, as EvalCallback in the reference):", tr.evaluate())
        if args.log_json:
            json.dump(history, open(args.log_json, "w"))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
