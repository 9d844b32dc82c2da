"""Time the PPO learner -- advantages + update -- at the training shape for both learners (learner="torch" / "fused") in ONE process
on ONE collected rollout, alternating, with a device synchronisation on both sides of every timed region: one warm-up each, then
the median of --runs runs each. Every run starts from the same policy and optimiser state. Prints one JSON line.

    python tools/update_rate.py [--env SwingRacket-v0] [--num-envs 4096] [--n-steps 1100] [--batch-size 65536] [--n-epochs 10] [--runs 5]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="SwingRacket-v0", choices=["SwingRacket-v0", "Tennisbot-v0"])
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--n-steps", type=int, default=1100)
    ap.add_argument("--batch-size", type=int, default=65536)
    ap.add_argument("--n-epochs", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5 (a median of fewer says little)")
    import torch
    from tennisbot_rl_amd.ppo import PPOTrainer
    tr = PPOTrainer(args.env, num_envs=args.num_envs, n_steps=args.n_steps, device="cuda:0", seed=0, batch_size=args.batch_size, n_epochs=args.n_epochs,
                    learner="fused")
    tr.collect()
    torch.cuda.synchronize()
    fused = tr._learner
    start = copy.deepcopy(tr.policy.state_dict()), copy.deepcopy(tr.opt.state_dict())

    def run(learner):
        tr.policy.load_state_dict(start[0]); tr.opt.load_state_dict(copy.deepcopy(start[1]))
        tr._learner = learner
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        adv, returns = tr.advantages(tr.last_value)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        stats = tr.update(adv, returns)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return t1 - t0, t2 - t1, stats

    times = {"torch": [], "fused": []}
    stats = {}
    for k in range(args.runs + 1):            # run 0 of each is the warm-up
        for name, learner in (("torch", None), ("fused", fused)):
            a, u, stats[name] = run(learner)
            if k:
                times[name].append((a, u))
    tr._learner = fused
    med = lambda xs: statistics.median(xs)  # noqa: E731
    out = {"tool": "update_rate", "env": args.env, "num_envs": args.num_envs, "n_steps": args.n_steps, "batch_size": tr.batch_size, "n_epochs": args.n_epochs,
           "minibatches_per_epoch": -(-args.num_envs * args.n_steps // tr.batch_size), "runs": args.runs, "device": torch.cuda.get_device_name(0)}
    for name in ("torch", "fused"):
        out[name + "_advantages_s"] = med([a for a, _ in times[name]])
        out[name + "_update_s"] = med([u for _, u in times[name]])
        out[name + "_s"] = med([a + u for a, u in times[name]])
        out[name + "_runs_s"] = [round(a + u, 6) for a, u in times[name]]
        out[name + "_last_stats"] = stats[name]
    out["fused_over_torch"] = out["fused_s"] / out["torch_s"]
    print(json.dumps(out))
    tr.env.close()


if __name__ == "__main__":
    main()
