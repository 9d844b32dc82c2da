#!/usr/bin/env python3
"""Rate of whole-episode evaluation, three forms of the same work in ONE process (does not touch bench.py): every env of a batch
runs one episode under the same policy, noise seed and episode index, and a float64 return and a length per env come out.

  (a) BatchedEnv.policy_evaluate: one tb_policy_evaluate launch, every workgroup leaves when its last env is done;
  (b) a policy_step loop, one launch per step, to the batch's last `done` (asked of the device every 8 steps on Tennisbot-v0;
      SwingRacket-v0: 26 steps and a flush), first-`done` masks and float64 sums in torch between the steps;
  (c) one policy_rollout of 26 / 1001 steps -- every env steps on past its episode's end -- and a torch first-`done` fold.

Both env kinds, the forms alternating, one warm-up each, then the median of --runs runs; a device synchronisation on both sides
of every timed region. The three forms must agree on every return and length (checked on the warm-up). Prints one JSON line and
writes it to --out.

    python tools/eval_rate.py [--num-envs 4096] [--runs 5] [--out profiles/r14_eval_rate.json]
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, OBS_DIM
    from tennisbot_rl_amd.ppo import SWING_DEFAULTS, TENNIS_DEFAULTS, build_actor_critic, pack_policy
    from tennisbot_rl_amd.stepper import BatchedEnv

    dev, n = torch.device("cuda", 0), args.num_envs

    def weights(kind):
        torch.manual_seed(args.seed)
        arch = (SWING_DEFAULTS if kind == ENV_SWING else TENNIS_DEFAULTS)["net_arch"]
        policy = build_actor_critic(OBS_DIM[kind], ACT_DIM[kind], tuple(arch))
        if kind == ENV_SWING:  # the reference's shipped policy: balls are struck
            policy.load_sb3_arrays(dict(np.load(os.path.join(ROOT, "tests", "golden", "ppo_swing_policy.npz"))))
        return pack_policy(policy.to(dev))

    def sync():
        torch.cuda.synchronize(dev)

    result = {"num_envs": n, "runs": args.runs, "device": torch.cuda.get_device_name(dev), "forms": {}}
    for kind, name in ((ENV_SWING, "SwingRacket-v0"), (ENV_TENNIS, "Tennisbot-v0")):
        swing = kind == ENV_SWING
        T = 26 if swing else 1001
        w = weights(kind)
        # one handle per form, same seed and env ids: run k of every form is episode k of every env
        envs = {f: BatchedEnv(kind, n, device=dev, seed=args.seed, pipeline=swing, track_terminal_obs=False) for f in "abc"}

        def form_a():
            return envs["a"].policy_evaluate(w, seed=args.seed)

        def form_b():
            env = envs["b"]
            obs = env.reset()
            ret = torch.zeros(n, dtype=torch.float64, device=dev)
            length = torch.zeros(n, dtype=torch.int32, device=dev)
            active = torch.ones(n, dtype=torch.bool, device=dev)
            if swing:  # exactly 26 steps; the terminal rewards are in place after the flush
                rews = []
                for _ in range(T):
                    (obs, r, d), _ = env.policy_step(w, obs, seed=args.seed)
                    rews.append(r)
                env.flush()
                return torch.stack(rews).double().sum(0), torch.full((n,), T, dtype=torch.int32, device=dev)
            for t in range(T):
                (obs, r, d), _ = env.policy_step(w, obs, seed=args.seed)
                ret += torch.where(active, r.double(), torch.zeros_like(ret))
                length += active.int()
                active &= d == 0
                if (t + 1) % 8 == 0 and not bool(active.any()):
                    break
            return ret, length

        def form_c():
            env = envs["c"]
            (obs, rew, done), _ = env.policy_rollout(w, env.reset(), T, seed=args.seed)
            env.flush() if swing else None
            before = done.long().cumsum(0) - done.long()          # dones strictly before step t
            first = before == 0
            return (rew.double() * first).sum(0), first.sum(0).int()

        forms = {"a": form_a, "b": form_b, "c": form_c}
        # warm-up, and the three forms' agreement (float64 sums in step order: bit for bit)
        sync()
        warm = {f: fn() for f, fn in forms.items()}
        sync()
        agree = all(torch.equal(warm["a"][0], warm[f][0]) and torch.equal(warm["a"][1], warm[f][1]) for f in "bc")
        times = {f: [] for f in forms}
        lengths = None
        for _ in range(args.runs):
            for f, fn in forms.items():
                sync()
                t0 = time.perf_counter()
                out = fn()
                sync()
                times[f].append(time.perf_counter() - t0)
                if f == "a":
                    lengths = out[1]
        ln = lengths.double()
        pad = (-n) % 16
        per_wg = torch.cat([ln, torch.zeros(pad, dtype=ln.dtype, device=dev)]).view(-1, 16).max(1).values   # the last run's episodes
        row = {"forms_agree": bool(agree), "mean_length": float(ln.mean()), "max_length": float(ln.max()),
               "mean_longest_per_workgroup": float(per_wg.mean()), "steps_cap": T}
        for f in forms:
            s = statistics.median(times[f])
            # env steps of the EPISODES (what an evaluation is for), not the steps a form ran past their ends
            row[f] = {"seconds": s, "episodes_per_s": n / s, "episode_env_steps_per_s": float(ln.sum()) / s, "all_seconds": times[f]}
        result["forms"][name] = row
        for e in envs.values():
            e.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return result


if __name__ == "__main__":
    main()
