#!/usr/bin/env python3
"""Counterpart of the reference's `train.py` on the batched MI355X envs: PPO on Tennisbot-v0.

  python train.py                                   # -s ppo: SB3's default 64-64 tanh MlpPolicy (train.py:104-110)
  python train.py -s tuned_ppo --curri              # the ReLU net with the shared features extractor (train.py:54-67,112-127)
  torchrun --nproc-per-node 8 train.py -s tuned_ppo # one process per GPU, sharded envs
  python train.py -s tuned_ppo --population 4 --member-ent-coef 0,1e-3,3e-3,1e-2 --pbt-every 4   # 4 learners side by side, 1024 envs each

`-s tuned_ppo` selects `PPOTrainer(policy="tuned")`: the network runs inside the rollout kernels (tb_policy_rollout_net with
TB_NET_TUNED) and, with --learner fused, its update in the learner kernels (tb_ppo_grad_net / tb_ppo_apply_net). Hyper-parameters follow train.py (ppo.TENNIS_DEFAULTS / ppo.TUNED_TENNIS_DEFAULTS); the rollout is n_steps per
env x num_envs instead of 1100 x 1. One deviation: the reference passes n_epochs = int(1e6 / 500) = 2000 to the tuned model
(train.py:76-78,126; recorded as TUNED_TENNIS_DEFAULTS["reference_n_epochs"]); this script keeps PPOTrainer's 10 for both
selections unless --n-epochs is given, because 2000 epochs over a 4096-env rollout is not a usable default. `--curri` is the
racket-size curriculum of train.py:155-176. `-s sac` has its own script, train_sac.py (tennisbot_rl_amd/sac.py). `--gui` is
accepted and does nothing. train_swing.py stays the script for SwingRacket-v0 and for TRPO.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tennisbot_rl_amd.evaluation import add_schedule_arguments, resolve_load, schedule_from_args  # noqa: E402
from tennisbot_rl_amd.population import add_population_arguments, population_keywords  # noqa: E402
from train_swing import racket_scale_for  # noqa: E402  (train.py:164-176, one table for both scripts)

ENV_ID = "Tennisbot-v0"
SELECT = {"ppo": "default", "tuned_ppo": "tuned"}


def main(argv=None):
    ap = argparse.ArgumentParser(description="PPO on Tennisbot-v0 (the reference's train.py)")
    ap.add_argument("-s", "--select", default="ppo", help="ppo or tuned_ppo")
    ap.add_argument("--curri", action="store_true", help="curriculum learning: size change of racket")
    ap.add_argument("--load", type=str, default=None, help="checkpoint written by --save; `best`: best_model.pt beside --save (written under --eval-freq)")
    ap.add_argument("--save", type=str, default=None, help="default: ./model/<select>_Tennisbot-v0.pt")
    ap.add_argument("--gui", action="store_true", help="accepted for CLI compatibility; there is no GUI")
    ap.add_argument("--learner", default="torch", choices=["torch", "fused"], help="fused: GAE, minibatch gradient and Adam as HIP kernels (tennisbot_rl_amd/learner.py)")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--n-steps", type=int, default=104, help="agent steps per env per rollout")
    ap.add_argument("--n-epochs", type=int, default=None, help="default: PPOTrainer's 10 (the reference's tuned_ppo: 2000)")
    ap.add_argument("--total-timesteps", type=float, default=1e6)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log-json", type=str, default=None)
    add_schedule_arguments(ap)
    add_population_arguments(ap)
    args = ap.parse_args(argv)
    if args.select not in SELECT:
        sys.exit("-s %s: only ppo and tuned_ppo are implemented on the batched envs (trpo: train_swing.py). SAC: train_sac.py" % args.select)
    try:
        population = population_keywords(args, args.select)
    except ValueError as exc:
        sys.exit(str(exc))
    if population is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("--population runs on one rank: multi-GPU populations are not provided")

    import torch
    from tennisbot_rl_amd.ppo import PPOTrainer

    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.distributed.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    hp = {} if args.n_epochs is None else {"n_epochs": args.n_epochs}
    if population is not None:
        from tennisbot_rl_amd.population import PopulationPPO, run_population
        pop = PopulationPPO(ENV_ID, n_steps=args.n_steps, net=SELECT[args.select], device=torch.device("cuda", local_rank), seed=args.seed, **population, **hp)
        path = args.save or "./model/%s_%s.pt" % (args.select, ENV_ID)
        if args.load:
            pop.load(args.load)
        history = run_population(pop, args.total_timesteps, path, save_freq=args.save_freq)
        if args.log_json:
            json.dump(history, open(args.log_json, "w"))
        return
    tr = PPOTrainer(ENV_ID, num_envs=args.num_envs, n_steps=args.n_steps, device=torch.device("cuda", local_rank), seed=args.seed,
                    learner=args.learner, policy=SELECT[args.select], **hp)
    path = args.save or "./model/%s_%s.pt" % (args.select, ENV_ID)
    if args.load:
        tr.load(resolve_load(args.load, path))
    schedule = schedule_from_args(args, path)
    if schedule is not None:
        schedule.reset(tr.num_timesteps)
    total = args.total_timesteps
    history = []
    while tr.num_timesteps < total:
        if args.curri:
            tr.env.set_racket_scale(racket_scale_for(100.0 * tr.num_timesteps / total))
        history += tr.learn(min(total, tr.num_timesteps + tr.n_steps * tr.num_envs * world), schedule=schedule)
    if tr.rank == 0:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tr.save(path)
        if args.eval_freq:
            print("saved", path, "eval (%d whole episodes, %s policy):" % (args.n_eval_episodes, "deterministic" if args.eval_deterministic else "stochastic"),
                  tr.evaluate_episodes(args.n_eval_episodes, deterministic=args.eval_deterministic))
        else:
            print("saved", path, "eval (stochastic policy, as EvalCallback in the reference):", tr.evaluate(n_episodes_steps=200))
        if args.log_json:
            json.dump(history, open(args.log_json, "w"))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
