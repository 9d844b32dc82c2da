#!/usr/bin/env python3
"""Time one gradient step of a POPULATION of SAC learners, two legs in ONE process on one GPU (does not touch bench.py), at
M = 4 and 16 members, B = 256 and 1100, both env ids, on synthetic replay rows:

  population  one FusedSACMembers.gradient_step (tb_sac_*_members): sac_population.MEMBERS_LAUNCHES_PER_STEP["sac"] = 40 launches
              whatever M is;
  learners    M FusedSAC.gradient_step calls back to back on M separate learners: M x 40 launches, how M learners were trained
              before the members entry points existed.

Both legs do the same arithmetic per member (the members stages are bit for bit the single-member stages). A timed run is --steps
steps issued back to back between two device synchronisations, the host clock around them, divided by --steps. The legs
ALTERNATE; run 0 of each is the warm-up; then the median of --runs runs with the spread (max - min) / median recorded, as
tools/sac_rate.py does. The tool exits 1 unless, at every point, the population's median raised by the larger of the two legs'
spreads is still below the learners' median (the rule of tools/sac_members_rate.py). --algo tqc times TQC's step (41 launches).

    python tools/sac_population_rate.py [--runs 5] [--steps 50] [--algo sac] [--out profiles/r24_sac_population_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEMBERS, BATCHES = (4, 16), (256, 1100)


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def measure(torch, algo, env_id, M, B, runs, steps, n_rows=100_000):
    from tennisbot_rl_amd import sac_population as sp
    from tennisbot_rl_amd.sac import SAC_DEFAULTS, FusedSAC
    from tennisbot_rl_amd.stepper import ACT_DIM, ENV_IDS, OBS_DIM
    from tennisbot_rl_amd.tqc import FusedTQC
    kind = ENV_IDS[env_id]
    O, A = OBS_DIM[kind], ACT_DIM[kind]
    dev = torch.device("cuda", 0)
    build = sp._algo(algo)[2]
    pop = (sp.FusedSACMembers if algo == "sac" else sp.FusedTQCMembers)(kind, M, dev, seed=0)
    lr, eps = SAC_DEFAULTS["learning_rate"], SAC_DEFAULTS["adam_eps"]
    learners = []
    for m in range(M):   # M separate learners on member m's initial nets
        torch.manual_seed(m)
        actor, critic, target = (x.to(dev) for x in build(O, A))
        lec = torch.zeros(1, device=dev, requires_grad=True)
        opts = (torch.optim.Adam(actor.parameters(), lr=lr, eps=eps), torch.optim.Adam(critic.parameters(), lr=lr, eps=eps), torch.optim.Adam([lec], lr=lr, eps=eps))
        learners.append((FusedSAC if algo == "sac" else FusedTQC)(kind, actor, critic, target, lec, opts, dict(SAC_DEFAULTS), dev))
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    arrays = (r(n_rows, O), r(n_rows, O), torch.rand(n_rows, A, device=dev, generator=g) * 2 - 1, r(n_rows), (torch.rand(n_rows, device=dev, generator=g) < 0.04).float())
    idx = torch.randint(0, n_rows, (steps, M, B), device=dev, generator=g)
    noise = r(steps, 2, M, B, A)

    def population():
        for k in range(steps):
            pop.gradient_step(arrays, idx[k], noise[k, 0], noise[k, 1])

    def separate():
        for k in range(steps):
            for m, L in enumerate(learners):
                L.gradient_step(arrays, idx[k, m], noise[k, 0, m], noise[k, 1, m])

    legs = {"population": population, "learners": separate}
    times = {name: [] for name in legs}
    for k in range(runs + 1):                 # run 0 of each is the warm-up
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k:
                times[name].append((time.perf_counter() - t0) / steps)
    launches = sp.MEMBERS_LAUNCHES_PER_STEP[algo]
    out = {"env": env_id, "members": M, "batch": B, "launches_per_population_step": launches, "launches_per_learners_step": M * launches}
    for name in legs:
        out[name + "_step_s"] = statistics.median(times[name])
        out[name + "_runs_s"] = [round(s, 8) for s in times[name]]
        out[name + "_spread"] = spread(times[name])
    out["learners_over_population"] = out["learners_step_s"] / out["population_step_s"]
    out["population_s_per_launch"] = out["population_step_s"] / launches
    out["learners_s_per_launch"] = out["learners_step_s"] / (M * launches)
    out["population_faster_beyond_spreads"] = bool(out["population_step_s"] * (1.0 + max(out["population_spread"], out["learners_spread"])) < out["learners_step_s"])
    finite = all(bool(torch.isfinite(x).all()) for x in (pop.pi.flat, pop.q.flat, pop.stats))
    out["finite"] = finite
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50, help="gradient steps per timed run")
    ap.add_argument("--algo", default="sac", choices=("sac", "tqc"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5 (a median of fewer says little)")
    import torch
    cases = []
    for env_id in ("SwingRacket-v0", "Tennisbot-v0"):
        for M in MEMBERS:
            for B in BATCHES:
                cases.append(measure(torch, args.algo, env_id, M, B, args.runs, args.steps))
                print(json.dumps({k: v for k, v in cases[-1].items() if not k.endswith("_runs_s")}), flush=True)
    ok = all(c["population_faster_beyond_spreads"] and c["finite"] for c in cases)
    out = {"tool": "sac_population_rate", "algo": args.algo, "runs": args.runs, "steps_per_run": args.steps, "device": torch.cuda.get_device_name(0),
           "timing": "host clock around a device synchronise", "launches_per_population_step": cases[0]["launches_per_population_step"],
           "population_faster_beyond_spreads": ok, "cases": cases}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
