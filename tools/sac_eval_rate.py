#!/usr/bin/env python3
"""Rate of whole-episode evaluation of a SAC / TQC actor, two forms of the same work in ONE process (does not touch bench.py):
every env of a batch runs one episode under the same actor weights, and a float64 return and a length per env come out.

  (a) BatchedEnv.sac_evaluate: one tb_sac_evaluate launch, the actor inside the episode loop (SACTrainer's eval_form="fused");
  (b) evaluation.evaluate_actor_episodes: a separate batch stepped by the torch actor between env steps, to the batch's last
      `done` (asked of the device every 8 steps on Tennisbot-v0) -- the yardstick, and the trainers' default form.

Both env kinds, --num-envs batch sizes, the forms alternating, one warm-up each, then --runs timed runs per form: the median and
the spread (min, max). A device synchronisation on both sides of every timed region. A timed region of form (a) is --inner calls
back to back (successive episodes), so that a window of a 64-env SwingRacket launch is not a window of the host clock; the
seconds reported are per call. The two forms draw different noise (keyed in the kernel / a torch.Generator), so their episodes
are not the same ones: the mean and the maximum episode length of each form's timed runs are recorded beside its time. Prints one
JSON line and writes it to --out.

    python tools/sac_eval_rate.py [--num-envs 64 4096] [--runs 5] [--out profiles/r15_sac_eval_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACTOR_SEED = {"SwingRacket-v0": 3, "Tennisbot-v0": 1235}   # tests/test_gpu_sac_evaluate.py's plain actors: balls are struck, episodes end early and late


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, nargs="+", default=[64, 4096])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="form (a) calls per timed region")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)

    import torch
    from tennisbot_rl_amd.evaluation import evaluate_actor_episodes
    from tennisbot_rl_amd.learner import flatten_parameters
    from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, OBS_DIM
    from tennisbot_rl_amd.sac import build_sac_modules
    from tennisbot_rl_amd.stepper import BatchedEnv

    dev = torch.device("cuda", 0)

    def sync():
        torch.cuda.synchronize(dev)

    def spread(xs):
        return {"seconds": statistics.median(xs), "min_seconds": min(xs), "max_seconds": max(xs), "all_seconds": xs}

    result = {"runs": args.runs, "inner": args.inner, "device": torch.cuda.get_device_name(dev), "cases": []}
    for kind, name in ((ENV_SWING, "SwingRacket-v0"), (ENV_TENNIS, "Tennisbot-v0")):
        swing = kind == ENV_SWING
        torch.manual_seed(ACTOR_SEED[name])
        actor = build_sac_modules(OBS_DIM[kind], ACT_DIM[kind])[0]
        with torch.no_grad():
            actor.mu.weight.mul_(30.0)   # (torch's default init is near zero: the racket would not move)
        actor = actor.to(dev)
        flat = flatten_parameters(actor)
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed)
        for n in args.num_envs:
            fused = BatchedEnv(kind, n, device=dev, seed=args.seed, pipeline=swing, track_terminal_obs=False)
            stepped = BatchedEnv(kind, n, device=dev, seed=args.seed, pipeline=False, track_terminal_obs=False)
            lengths = {"a": [], "b": []}

            def form_a():
                for _ in range(args.inner):
                    out = fused.sac_evaluate(flat, seed=args.seed)
                return out[1]

            def form_b():
                act = lambda obs: actor.sample(obs, torch.randn((n, ACT_DIM[kind]), device=dev, generator=gen))[0]  # noqa: E731
                return evaluate_actor_episodes(stepped, act, n)

            sync()
            form_a(); form_b()   # warm-up
            sync()
            times = {"a": [], "b": []}
            for _ in range(args.runs):
                sync()
                t0 = time.perf_counter()
                ln = form_a()
                sync()
                times["a"].append((time.perf_counter() - t0) / args.inner)
                lengths["a"].append((float(ln.double().mean()), int(ln.max())))   # (the region's last call)
                sync()
                t0 = time.perf_counter()
                out = form_b()   # (its summary is one host read inside the region: part of the form)
                sync()
                times["b"].append(time.perf_counter() - t0)
                lengths["b"].append((out["mean_length"], None))
            row = {"env": name, "num_envs": n, "steps_cap": 26 if swing else 1001, "a": spread(times["a"]), "b": spread(times["b"])}
            row["a"].update(mean_length=statistics.mean(m for m, _ in lengths["a"]), max_length=max(x for _, x in lengths["a"]))
            row["b"].update(mean_length=statistics.mean(m for m, _ in lengths["b"]))
            row["b_over_a"] = row["b"]["seconds"] / row["a"]["seconds"]
            row["a_is_faster_in_every_run"] = max(times["a"]) < min(times["b"])
            result["cases"].append(row)
            fused.close(); stepped.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return result


if __name__ == "__main__":
    main()
