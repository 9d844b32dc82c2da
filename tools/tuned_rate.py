"""Rates of the tuned network (PPOTrainer(policy="tuned"), Tennisbot-v0) on one GPU, in ONE process. Prints one JSON line and,
with --out, writes it to a file.

  (a) collect: env steps/s of PPOTrainer.collect with the tuned net inside the rollout kernel, against fused=False (the torch
      module between the env steps), and the default Tennisbot net inside the rollout kernel from the same run: trainers
      alternating, one warm-up collect each (the fused ones capture their graph in it), the median of --runs collects each, a
      device synchronisation on both sides of every timed region.
  (b) update: advantages + update on ONE collected rollout, the fused learner against the torch learner, alternating, one warm-up
      each and the median of --runs, every run from the same policy and optimiser state (the form of tools/update_rate.py).

Exits with status 1 if a fused form is slower than its torch counterpart; no other threshold.

    python tools/tuned_rate.py [--num-envs 4096] [--n-steps 104] [--batch-size 65536] [--n-epochs 10] [--runs 5] [--out FILE]
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
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--n-steps", type=int, default=104)
    ap.add_argument("--batch-size", type=int, default=65536)
    ap.add_argument("--n-epochs", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5 (a median of fewer says little)")
    import torch
    from tennisbot_rl_amd.ppo import PPOTrainer
    kw = dict(num_envs=args.num_envs, n_steps=args.n_steps, device="cuda:0", seed=0, batch_size=args.batch_size, n_epochs=args.n_epochs)
    trainers = {"tuned_fused": PPOTrainer("Tennisbot-v0", policy="tuned", learner="fused", **kw),
                "tuned_torch": PPOTrainer("Tennisbot-v0", policy="tuned", fused=False, **kw),
                "default_fused": PPOTrainer("Tennisbot-v0", **kw)}
    steps = args.num_envs * args.n_steps

    def collect(tr):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.collect()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    times = {k: [] for k in trainers}
    for k in range(args.runs + 1):            # run 0 of each is the warm-up (and the fused trainers' graph capture)
        for name, tr in trainers.items():
            t = collect(tr)
            if k:
                times[name].append(t)
    out = {"tool": "tuned_rate", "env": "Tennisbot-v0", "num_envs": args.num_envs, "n_steps": args.n_steps, "batch_size": trainers["tuned_fused"].batch_size,
           "n_epochs": args.n_epochs, "runs": args.runs, "device": torch.cuda.get_device_name(0)}
    for name in trainers:
        out["collect_%s_s" % name] = statistics.median(times[name])
        out["collect_%s_steps_per_s" % name] = steps / statistics.median(times[name])
        out["collect_%s_runs_s" % name] = [round(t, 6) for t in times[name]]
    out["collect_fused_over_torch"] = out["collect_tuned_fused_steps_per_s"] / out["collect_tuned_torch_steps_per_s"]

    tr = trainers["tuned_fused"]
    fused = tr._learner
    start = copy.deepcopy(tr.policy.state_dict()), copy.deepcopy(tr.opt.state_dict())

    def update(learner):
        tr.policy.load_state_dict(start[0]); tr.opt.load_state_dict(copy.deepcopy(start[1]))
        tr._learner = learner
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = tr.update(*tr.advantages(tr.last_value))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, stats

    utimes, ustats = {"torch": [], "fused": []}, {}
    for k in range(args.runs + 1):
        for name, learner in (("torch", None), ("fused", fused)):
            t, ustats[name] = update(learner)
            if k:
                utimes[name].append(t)
    tr._learner = fused
    for name in ("torch", "fused"):
        out["update_%s_s" % name] = statistics.median(utimes[name])
        out["update_%s_runs_s" % name] = [round(t, 6) for t in utimes[name]]
        out["update_%s_last_stats" % name] = ustats[name]
    out["update_fused_over_torch_time"] = out["update_fused_s"] / out["update_torch_s"]
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for t in trainers.values():
        t.env.close()
    slower = [k for k, bad in (("collect", out["collect_fused_over_torch"] < 1.0), ("update", out["update_fused_over_torch_time"] > 1.0)) if bad]
    if slower:
        sys.exit("tuned_rate: the fused form is slower than its torch counterpart: %s" % ", ".join(slower))


if __name__ == "__main__":
    main()
