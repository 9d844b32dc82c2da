#!/usr/bin/env python3
"""What training a population of PPO learners in one batch saves, measured in ONE process on one GPU (does not touch bench.py).

For SwingRacket-v0 (default net) and Tennisbot-v0 (tuned net), M in --members (default 4, 16), at the scripts' default shape
(--num-envs 4096 in total, so R = 4096 / M envs per member; n_steps 104; 10 epochs; one minibatch of min(T R, 65536) rows per
member and epoch), two legs:

  population  one PopulationPPO iteration: collect (pack + tb_policy_rollout_members + the bookkeeping), then advantages + update
              (tb_ppo_gae, and per minibatch tb_ppo_grad_members + tb_ppo_apply_members);
  trainers    M PPOTrainer(learner="fused", graph=False) iterations of R envs each, one after another on the same stream: what a
              sweep of M runs took before. All M collects are issued, then the device is joined; likewise the M updates.

The legs ALTERNATE: after a warm-up iteration of each, --reps (default 5) timed repetitions each, collect and update timed
separately with the host clock around a device join (the launches' host cost is part of what is compared). Medians are reported, and
`update_ratio` / `collect_ratio` = population / trainers: below 1 means the population is faster.

    python tools/population_rate.py [--reps 5] [--out profiles/r22_population_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", type=str, default="4,16")
    ap.add_argument("--num-envs", type=int, default=4096, help="in total, as the scripts' --num-envs")
    ap.add_argument("--n-steps", type=int, default=104)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)

    import torch
    from tennisbot_rl_amd.population import PopulationPPO
    from tennisbot_rl_amd.ppo import PPOTrainer

    dev = torch.device("cuda", 0)
    T = args.n_steps

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    result = {"num_envs": args.num_envs, "n_steps": T, "reps": args.reps, "device": torch.cuda.get_device_name(dev),
              "timing": "host clock around a device join; the two legs alternate", "cases": []}
    for env_id, net, policy in (("SwingRacket-v0", "default", "default"), ("Tennisbot-v0", "tuned", "tuned")):
        for M in [int(x) for x in args.members.split(",")]:
            R = args.num_envs // M
            pop = PopulationPPO(env_id, members=M, envs_per_member=R, n_steps=T, net=net, device=dev, seed=args.seed)
            trainers = [PPOTrainer(env_id, num_envs=R, n_steps=T, device=dev, seed=args.seed + m, graph=False, learner="fused", policy=policy) for m in range(M)]
            assert pop.batch_size == trainers[0].batch_size and pop.hp["n_epochs"] == trainers[0].hp["n_epochs"]

            def pop_collect():
                return pop.collect()

            def pop_update(last_value):
                return pop.update(*pop.advantages(last_value))

            def trainers_collect():
                return [tr.collect() for tr in trainers]

            def trainers_update(last_values):
                return [tr.update(*tr.advantages(lv)) for tr, lv in zip(trainers, last_values)]

            times = {"population_collect": [], "population_update": [], "trainers_collect": [], "trainers_update": []}
            for rep in range(args.reps + 1):   # (the first iteration of each leg is the warm-up)
                for leg, collect, update in (("population", pop_collect, pop_update), ("trainers", trainers_collect, trainers_update)):
                    tc, last = timed(collect)
                    tu, _ = timed(lambda: update(last))
                    if rep:
                        times[leg + "_collect"].append(tc)
                        times[leg + "_update"].append(tu)
            med = {k: statistics.median(v) for k, v in times.items()}
            steps = pop.step_count // (args.reps + 1)
            row = {"env": env_id, "net": net, "members": M, "envs_per_member": R, "batch": pop.batch_size, "minibatch_steps_per_update": steps,
                   "median_s": med, "spread": {k: (max(v) - min(v)) / med[k] for k, v in times.items()}, "all_s": times,
                   "collect_ratio": med["population_collect"] / med["trainers_collect"], "update_ratio": med["population_update"] / med["trainers_update"],
                   "iteration_ratio": (med["population_collect"] + med["population_update"]) / (med["trainers_collect"] + med["trainers_update"])}
            result["cases"].append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "all_s"}), flush=True)
            pop.close()
            for tr in trainers:
                tr.env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return result


if __name__ == "__main__":
    main()
