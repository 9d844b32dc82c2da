#!/usr/bin/env python3
"""Rate of SAC / TQC collect, two forms of the same work in ONE process (does not touch bench.py): S steps of every env of a
batch under the same actor weights, every transition into a replay ring, the episode statistics kept.

  (a) SACTrainer(collect_form="fused").collect_fused(S): tb_sac_collect launches with the actor inside, rows written in place
      (as few launches as the ring's wrap and SwingRacket's episode end allow: one here), then the statistics of the S steps;
      (a_launch) is the launch alone, BatchedEnv.sac_collect into reserved rows, without the statistics;
  (b) S calls of SACTrainer.collect(): the torch actor, one BatchedEnv.step, the ring copies and the statistics per env step --
      the yardstick, and the trainers' default form.

Both env kinds, --num-envs batch sizes, S = 26 (SwingRacket-v0, one episode) / 64 (Tennisbot-v0), learning_starts = 0 (the actor
acts from the first step) and no gradient step: collect alone. The forms alternate, one warm-up each, then --runs timed runs
per form: the median and the spread (min, max), a device synchronisation on both sides of every timed region. A timed region is
--inner calls of the form back to back (successive steps of the same envs), so that a window of a 1 ms launch is not a window of
the host clock; the seconds reported are per call. The two trainers
are built from the same seed, so their actors hold the same weights; their noise differs (keyed in the kernel / torch's RNG), so
their episodes are not the same ones. Prints one JSON line and writes it to --out.

    python tools/sac_collect_rate.py [--num-envs 256 4096] [--runs 5] [--out profiles/r16_sac_collect_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"SwingRacket-v0": 26, "Tennisbot-v0": 64}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls of a form per timed region (the seconds reported are per call)")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)

    import torch
    from tennisbot_rl_amd.sac import SACTrainer

    dev = torch.device("cuda", 0)

    def sync():
        torch.cuda.synchronize(dev)

    def spread(xs, steps):
        med = statistics.median(xs)
        return {"seconds": med, "min_seconds": min(xs), "max_seconds": max(xs), "all_seconds": xs, "us_per_env_step_of_the_batch": 1e6 * med / steps}

    result = {"runs": args.runs, "inner": args.inner, "device": torch.cuda.get_device_name(dev), "cases": []}
    for name, S in STEPS.items():
        for n in args.num_envs:
            kw = dict(num_envs=n, batch_size=32, gradient_steps=1, buffer_size=4 * S * n, learning_starts=0, seed=args.seed, device=dev)
            fused = SACTrainer(name, collect_form="fused", collect_steps=S, **kw)
            stepped = SACTrainer(name, **kw)
            assert torch.equal(fused._learner.pi.flat, stepped._learner.pi.flat)
            with torch.no_grad():   # (torch's default init is near zero: the racket would not move; the parameters are views of the flat vector)
                for tr in (fused, stepped):
                    tr.actor.mu.weight.mul_(30.0)
            assert torch.equal(fused._learner.pi.flat, stepped._learner.pi.flat)

            def form_a():
                fused.collect_fused(S)

            def form_a_launch():
                views = fused.replay.reserve(S, n)
                fused.env.sac_collect(fused._learner.pi.flat, S, views, seed=fused._collect_seed)

            def form_b():
                for _ in range(S):
                    stepped.collect()

            forms = (("a", form_a), ("a_launch", form_a_launch), ("b", form_b))
            sync()
            for _, f in forms:   # warm-up
                f()
            sync()
            times = {k: [] for k, _ in forms}
            for _ in range(args.runs):
                for k, f in forms:
                    sync()
                    t0 = time.perf_counter()
                    for _ in range(args.inner):
                        f()
                    sync()
                    times[k].append((time.perf_counter() - t0) / args.inner)
            row = {"env": name, "num_envs": n, "steps": S}
            row.update({k: spread(times[k], S) for k, _ in forms})
            row["b_over_a"] = row["b"]["seconds"] / row["a"]["seconds"]
            row["a_is_faster_in_every_run"] = max(times["a"]) < min(times["b"])
            row["episodes_finished"] = {"fused": fused.env.counters()["episodes_finished"], "torch": stepped.env.counters()["episodes_finished"]}
            result["cases"].append(row)
            fused.env.close(); stepped.env.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return result


if __name__ == "__main__":
    main()
