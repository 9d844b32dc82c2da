#!/usr/bin/env python3
"""Counterpart of the reference's `validate.py` (play a trained Tennisbot-v0 policy and report how it does) on the batched
MI355X envs -- headless only, whole episodes, many at once (tools/validate_swing.py is the SwingRacket-v0 one).

  python tools/validate.py -m model/ppo_Tennisbot-v0.pt                        # a checkpoint of train.py (-s ppo)
  python tools/validate.py -s tuned_ppo -m model/best_model.pt --racket-scale 3  # the tuned net, on the curriculum's big racket
  python tools/validate.py -s sac --env SwingRacket-v0 -m model/sac_SwingRacket-v0.pt   # a checkpoint of train_sac.py / train_tqc.py

Every episode runs from its reset to its first `done` inside one launch per --num-envs episodes (evaluation.PolicyEvaluator,
tb_policy_evaluate; SAC / TQC: evaluation.ActorEvaluator, tb_sac_evaluate, on the checkpoint's `actor` flattened in
named_parameters() order); the report is the mean, standard deviation, extremes and mean length over --episodes episodes. Like
`model.predict(ob)` in the reference the policy acts stochastically unless --deterministic.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ENV_ID = "Tennisbot-v0"


def main(argv=None):
    ap = argparse.ArgumentParser(description="whole-episode validation of a Tennisbot-v0 checkpoint")
    ap.add_argument("-m", "--model_file", type=str, required=True, help="checkpoint written by train.py (--save, best_model.pt or rl_model_<n>_steps.pt)")
    ap.add_argument("-s", "--select", default="ppo", choices=["ppo", "tuned_ppo", "sac", "tqc"], help="the network the checkpoint holds")
    ap.add_argument("--env", default=None, choices=["SwingRacket-v0", "Tennisbot-v0"], help="needed with -s sac / tqc, whose checkpoints exist for both env ids")
    ap.add_argument("--episodes", type=int, default=65536)
    ap.add_argument("--num-envs", type=int, default=4096, help="episodes per launch")
    ap.add_argument("--racket-scale", type=float, default=1.0, help="the racket size to validate on (train.py --curri ends at 1)")
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--headless", action="store_true", help="accepted for CLI compatibility; there is no GUI (tools/render_episode.py films a policy)")
    args = ap.parse_args(argv)
    if args.select in ("sac", "tqc") and args.env is None:
        ap.error("-s %s needs --env: its checkpoints exist for both env ids" % args.select)

    import torch
    from tennisbot_rl_amd.evaluation import PolicyEvaluator
    from tennisbot_rl_amd.params import ACT_DIM, ENV_TENNIS, NET_DEFAULT, NET_TUNED, OBS_DIM
    from tennisbot_rl_amd.ppo import TENNIS_DEFAULTS, TUNED_TENNIS_DEFAULTS, build_actor_critic, build_tuned_actor_critic, pack_policy

    dev = torch.device("cuda", 0)
    if args.select in ("sac", "tqc"):
        return validate_actor(args, torch, dev)
    if args.env not in (None, ENV_ID):
        ap.error("-s %s checkpoints are %s's" % (args.select, ENV_ID))
    tuned = args.select == "tuned_ppo"
    if tuned:
        policy = build_tuned_actor_critic(OBS_DIM[ENV_TENNIS], ACT_DIM[ENV_TENNIS], tuple(TUNED_TENNIS_DEFAULTS["net_arch"]), TUNED_TENNIS_DEFAULTS["extractor_hidden"])
    else:
        policy = build_actor_critic(OBS_DIM[ENV_TENNIS], ACT_DIM[ENV_TENNIS], tuple(TENNIS_DEFAULTS["net_arch"]))
    policy.load_state_dict(torch.load(args.model_file, map_location="cpu", weights_only=True)["policy"])
    policy = policy.to(dev)
    ev = PolicyEvaluator(ENV_TENNIS, n_envs=args.num_envs, seed=args.seed, device=dev, net=NET_TUNED if tuned else NET_DEFAULT)
    if args.racket_scale != 1.0:
        ev.set_racket_scale(args.racket_scale)
    print("------------- start running -------------")
    out = ev.evaluate(pack_policy(policy), args.episodes, deterministic=args.deterministic)
    return report(out, ENV_ID)


def report(out, env_id):
    print("%d episodes of %s: mean reward %.3f, std %.3f, min %.3f, max %.3f, mean length %.1f steps"
          % (out["episodes"], env_id, out["mean"], out["std"], out["min"], out["max"], out["mean_length"]))
    print(json.dumps(out))
    return out


def validate_actor(args, torch, dev):
    from tennisbot_rl_amd.evaluation import ActorEvaluator
    from tennisbot_rl_amd.sac import flatten_actor
    ck = torch.load(args.model_file, map_location="cpu", weights_only=True)
    flat = flatten_actor(ck["actor"]).to(dev)
    ev = ActorEvaluator(args.env, n_envs=args.num_envs, seed=args.seed, device=dev)
    if len(flat) != ev.env.sac_actor_floats():
        sys.exit("%s: the actor has %d parameters; %s's has %d (is --env right?)" % (args.model_file, len(flat), args.env, ev.env.sac_actor_floats()))
    if args.racket_scale != 1.0:
        ev.set_racket_scale(args.racket_scale)
    print("------------- start running -------------")
    return report(ev.evaluate(flat, args.episodes, deterministic=args.deterministic), args.env)


if __name__ == "__main__":
    main()
