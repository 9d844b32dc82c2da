#!/usr/bin/env python3
"""Rate of evaluating a POPULATION of MlpPolicy networks, four legs in ONE process on one GPU (does not touch bench.py), both env
kinds at --members x --envs-per-member (default 400 x 16 = 6400 envs):

  (a) one BatchedEnv.policy_evaluate_members launch with 400 DISTINCT blobs (tb_policy_evaluate_members);
  (b) BatchedEnv.policy_evaluate on the SAME handle with ONE blob: the per-workgroup work is the same, so this is (a)'s yardstick;
  (c) 400 policy_evaluate launches on ONE 16-env handle, one blob each: what comparing 400 policies took before (a);
  (d) tb_es_evaluate (the GatedCNN population kernel) at the same 400 x 16, for context only: another network, another kernel.

Every leg is warmed up, then the legs ALTERNATE for --reps repetitions each (default 20); a repetition is timed with events on the
stream, so host work outside the enqueue is not in it. Every call of every leg runs the next episode of its envs, so on
Tennisbot-v0 the lengths differ from repetition to repetition: the rate is env steps of the EPISODES (the sum of the lengths that
call returned) over its time, and the medians and spreads of both are recorded. The margin (a) gets over (b) is the spread (b)
shows against itself in this same run (`b_spread`: its repetitions' (max - min) / median).

    python tools/policy_members_rate.py [--reps 20] [--out profiles/r21_policy_members_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    """(max - min) / median of a leg's repetitions"""
    return (max(xs) - min(xs)) / statistics.median(xs)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", type=int, default=400)
    ap.add_argument("--envs-per-member", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    from tennisbot_rl_amd import es
    from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, NET_DEFAULT, OBS_DIM
    from tennisbot_rl_amd.policy_es import actor_flat, build_policy, pack_policy_members
    from tennisbot_rl_amd.ppo import pack_policy
    from tennisbot_rl_amd.stepper import BatchedEnv

    dev = torch.device("cuda", 0)
    M, R = args.members, args.envs_per_member
    n = M * R

    def template(kind):
        policy = build_policy(kind, NET_DEFAULT, args.seed)
        if kind == ENV_SWING:  # the reference's shipped policy: balls are struck
            policy.load_sb3_arrays(dict(np.load(os.path.join(ROOT, "tests", "golden", "ppo_swing_policy.npz"))))
        else:                  # an action head that moves the racket (SB3's init is near zero)
            with torch.no_grad():
                policy.action_net.weight.mul_(30.0)
        return policy.to(dev)

    result = {"members": M, "envs_per_member": R, "envs": n, "reps": args.reps, "device": torch.cuda.get_device_name(dev), "timing": "events on the stream", "envs_kinds": {}}
    for kind, name in ((ENV_SWING, "SwingRacket-v0"), (ENV_TENNIS, "Tennisbot-v0")):
        swing = kind == ENV_SWING
        policy = template(kind)
        g = torch.Generator(device=dev).manual_seed(args.seed)
        base = actor_flat(policy)
        flat = base + 0.1 * torch.randn((M, base.numel()), generator=g, device=dev)
        blobs = pack_policy_members(policy, flat)                  # 400 distinct networks
        one = pack_policy(policy)
        big = BatchedEnv(kind, n, device=dev, seed=args.seed, pipeline=swing, track_terminal_obs=False)       # legs a, b
        small = BatchedEnv(kind, R, device=dev, seed=args.seed, pipeline=swing, track_terminal_obs=False)     # leg c
        cnn = BatchedEnv(kind, n, device=dev, seed=args.seed, pipeline=swing, track_terminal_obs=False)       # leg d
        P = es.es_floats(OBS_DIM[kind], ACT_DIM[kind])
        W = es.pack_population(es.initial_weights(kind, 0).to(dev), torch.randn((M // 2, P), generator=g, device=dev), 0.1)

        def leg_a():
            return big.policy_evaluate_members(blobs, R, seed=args.seed)[1].sum()

        def leg_b():
            return big.policy_evaluate(one, seed=args.seed)[1].sum()

        def leg_c():
            total = torch.zeros((), dtype=torch.int64, device=dev)
            for m in range(M):
                total += small.policy_evaluate(blobs[m], seed=args.seed)[1].sum()
            return total

        def leg_d():
            return cnn.es_evaluate(W, R)[1].sum()

        legs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d}
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
        row = {}
        for k in legs:
            rates = [s / t for s, t in zip(steps[k], times[k])]
            row[k] = {"median_s": statistics.median(times[k]), "min_s": min(times[k]), "max_s": max(times[k]), "spread": spread(times[k]),
                      "median_env_steps": statistics.median(steps[k]), "median_env_steps_per_s": statistics.median(rates), "rate_spread": spread(rates),
                      "all_s": times[k]}
        row["a_over_b_time"] = row["a"]["median_s"] / row["b"]["median_s"]
        row["a_over_b_rate"] = row["a"]["median_env_steps_per_s"] / row["b"]["median_env_steps_per_s"]
        row["c_over_a_time"] = row["c"]["median_s"] / row["a"]["median_s"]
        row["b_spread"] = row["b"]["spread"]
        row["a_within_b_spread"] = bool(abs(row["a_over_b_time"] - 1.0) <= row["b_spread"])
        result["envs_kinds"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not isinstance(v, dict)}), flush=True)
        for e in (big, small, cnn):
            e.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return result


if __name__ == "__main__":
    main()
