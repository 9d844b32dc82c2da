#!/usr/bin/env python3
"""Rate of evaluating a POPULATION of SAC / TQC actors, three legs in ONE process on one GPU (does not touch bench.py), both env
kinds, at two shapes of 1024 envs -- M = 64 members x R = 16 envs and M = 16 x R = 64:

  (a) one BatchedEnv.sac_evaluate_members launch with M DIFFERENT actors (tb_sac_evaluate_members);
  (b) BatchedEnv.sac_evaluate on the SAME handle with ONE actor: the per-workgroup work is the same, but every workgroup streams the
      same 283 KB from its XCD's L2 where (a)'s stream M different vectors -- (a) / (b) is what that costs; reported, not gated;
  (c) M sac_evaluate launches on ONE R-env handle, one actor each: how M actors were compared before (a), and the yardstick of
      (a)'s claim. (a) must be faster than (c) by more than either leg's spread: the tool exits with status 1 where it is not.

Every leg is warmed up, then the legs ALTERNATE for --reps repetitions each (default 20); a repetition is timed with events on the
stream, so host work outside the enqueue is not in it. Every call of every leg runs the next episode of its envs, so on
Tennisbot-v0 the lengths differ from repetition to repetition: the medians and spreads, (max - min) / median, of the times and of
the env steps per second (the sum of the lengths that call returned over its time) are both recorded.

    python tools/sac_members_rate.py [--reps 20] [--out profiles/r23_sac_members_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((64, 16), (16, 64))   # (members, envs per member): one and four workgroups per member


def spread(xs):
    """(max - min) / median of a leg's repetitions"""
    return (max(xs) - min(xs)) / statistics.median(xs)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)

    import torch
    from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, OBS_DIM
    from tennisbot_rl_amd.sac import build_sac_modules, flatten_actor
    from tennisbot_rl_amd.stepper import BatchedEnv

    dev = torch.device("cuda", 0)

    def actors(kind, M):
        """M seeded default-init actors, the mu head scaled so that the racket moves (SB3's init is near zero)"""
        rows = []
        for m in range(M):
            torch.manual_seed(args.seed + m)
            actor = build_sac_modules(OBS_DIM[kind], ACT_DIM[kind])[0]
            with torch.no_grad():
                actor.mu.weight.mul_(30.0)
            rows.append(flatten_actor(actor.state_dict()))
        return torch.stack(rows).to(dev)

    result = {"shapes": [list(s) for s in SHAPES], "reps": args.reps, "device": torch.cuda.get_device_name(dev), "timing": "events on the stream",
              "envs_kinds": {}}
    ok = True
    for kind, name in ((ENV_SWING, "SwingRacket-v0"), (ENV_TENNIS, "Tennisbot-v0")):
        swing = kind == ENV_SWING
        result["envs_kinds"][name] = {}
        for M, R in SHAPES:
            n = M * R
            W = actors(kind, M)
            big = BatchedEnv(kind, n, device=dev, seed=args.seed, pipeline=swing, track_terminal_obs=False)       # legs a, b
            small = BatchedEnv(kind, R, device=dev, seed=args.seed, pipeline=swing, track_terminal_obs=False)     # leg c

            def leg_a():
                return big.sac_evaluate_members(W, R, seed=args.seed)[1].sum()

            def leg_b():
                return big.sac_evaluate(W[0], seed=args.seed)[1].sum()

            def leg_c():
                total = torch.zeros((), dtype=torch.int64, device=dev)
                for m in range(M):
                    total += small.sac_evaluate(W[m], seed=args.seed)[1].sum()
                return total

            legs = {"a": leg_a, "b": leg_b, "c": leg_c}
            for fn in legs.values():   # warm-up: code objects, allocations, the fast-forward's slots
                fn(); fn()
            torch.cuda.synchronize(dev)
            times, steps = {k: [] for k in legs}, {k: [] for k in legs}
            for _ in range(args.reps):
                for k, fn in legs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    s = fn()
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e-3)
                    steps[k].append(int(s))
            row = {"members": M, "envs_per_member": R, "envs": n}
            for k in legs:
                rates = [s / t for s, t in zip(steps[k], times[k])]
                row[k] = {"median_s": statistics.median(times[k]), "min_s": min(times[k]), "max_s": max(times[k]), "spread": spread(times[k]),
                          "median_env_steps": statistics.median(steps[k]), "median_env_steps_per_s": statistics.median(rates), "rate_spread": spread(rates),
                          "all_s": times[k]}
            row["a_over_b_time"] = row["a"]["median_s"] / row["b"]["median_s"]
            row["a_over_b_rate"] = row["a"]["median_env_steps_per_s"] / row["b"]["median_env_steps_per_s"]
            row["a_spread"], row["b_spread"], row["c_spread"] = row["a"]["spread"], row["b"]["spread"], row["c"]["spread"]
            row["c_over_a_time"] = row["c"]["median_s"] / row["a"]["median_s"]
            row["a_over_c_rate"] = row["a"]["median_env_steps_per_s"] / row["c"]["median_env_steps_per_s"]
            # the claim: (a)'s median, raised by the larger of the two spreads, is still below (c)'s
            row["a_faster_than_c_beyond_spreads"] = bool(row["a"]["median_s"] * (1.0 + max(row["a_spread"], row["c_spread"])) < row["c"]["median_s"])
            ok = ok and row["a_faster_than_c_beyond_spreads"]
            result["envs_kinds"][name]["%dx%d" % (M, R)] = row
            print(name, M, R, json.dumps({k: v for k, v in row.items() if not isinstance(v, dict)}), flush=True)
            big.close(); small.close()
    result["a_faster_than_c_beyond_spreads"] = ok
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    if not ok:
        sys.exit(1)
    return result


if __name__ == "__main__":
    main()
