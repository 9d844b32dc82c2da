#!/usr/bin/env python3
"""What tracing a SwingRacket-v0 flight costs: tb_swing_trace (BatchedEnv.trace_step) at stride 8 and at stride 1 beside the same
states' last step through tb_step on a pipeline-off handle with the substeps output -- the same flight without the frame stores.

  python tools/trace_rate.py                 # writes profiles/r20_trace_rate.json

Workload: 4096 states at step 25, once after 25 random steps from reset and once after 25 steps under the reference policy
(tests/golden/ppo_swing_policy.npz), each with the actions its 26th step takes. Every figure is the best of --repeats windows of
--launches calls, each call between two device events of its own (the tb_step handle gets its state back before every call, outside
the events); the time is the whole call's, launch overhead included. All in one process, one after the other. tb_step runs the
flight in the generic step kernel, not in the trace's: the difference of the two is two kernels' difference, so the cost of a stored
row is also taken from the two strides (the same kernel on the same flights) and the stores' share estimated from it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N = 4096


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_trace_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from tennisbot_rl_amd import stepper
    from tennisbot_rl_amd.ppo import PPOTrainer, pack_policy

    if not torch.cuda.is_available():
        sys.exit("no GPU: a trace rate can only be measured on one")

    def random_workload():
        env = stepper.BatchedEnv("SwingRacket-v0", N, device="cuda:0", seed=0)
        env.reset()
        gen = torch.Generator(device="cpu").manual_seed(0)
        for _ in range(25):
            env.step((torch.rand((N, env.act_dim), generator=gen) * 2 - 1).to(env.device))
        words, done = env.get_state_words()
        actions = (torch.rand((N, env.act_dim), generator=gen) * 2 - 1).to(env.device)
        env.close()
        return words, done, actions

    def policy_workload():
        tr = PPOTrainer("SwingRacket-v0", num_envs=N, n_steps=26, device="cuda:0", seed=0, graph=False)
        tr.policy.load_sb3_arrays(dict(np.load(os.path.join(ROOT, "tests", "golden", "ppo_swing_policy.npz"))))
        env, blob, obs = tr.env, pack_policy(tr.policy), tr.obs_in
        for _ in range(25):
            (obs, _, _), _ = env.policy_step(blob, obs, seed=1, net=tr.net)
        words, done = env.get_state_words()
        _, (actions, _, _, _) = env.policy_step(blob, obs, seed=1, net=tr.net)   # the clipped actions of the 26th step
        env.flush()
        actions = actions.clone()
        env.close()
        return words, done, actions

    def best_of(call, before=None):
        for _ in range(3):
            if before:
                before()
            call()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(args.repeats):
            total = 0.0
            for _ in range(args.launches):
                if before:
                    before()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call()
                t1.record()
                t1.synchronize()
                total += t0.elapsed_time(t1) * 1e-3
            best = min(best, total / args.launches)
        return best

    tracer = stepper.BatchedEnv("SwingRacket-v0", 64, device="cuda:0", seed=0)   # parameters, outline table and device: all the trace takes of it
    stepped = stepper.BatchedEnv("SwingRacket-v0", N, device="cuda:0", seed=0, auto_reset=False)   # pipeline off: the flight runs inside tb_step
    stepped.reset()
    rows = []
    for name, make in (("random actions", random_workload), ("reference policy", policy_workload)):
        words, done, actions = make()
        t_step = best_of(lambda: stepped.step(actions), before=lambda: stepped.set_state_words(words, done))
        ns = stepped.last_substeps().cpu().numpy()
        for stride in (8, 1):
            F = 2 + 775 // stride
            out = tracer.trace_step(actions, stride=stride, words=words, done=done)
            torch.cuda.synchronize()
            assert np.array_equal(out["substeps"].cpu().numpy(), ns), "the trace and the step disagree"
            t_trace = best_of(lambda: tracer.trace_step(actions, stride=stride, words=words, done=done))
            nbytes = F * tracer.words * N * 4
            row = dict(workload=name, states=N, stride=stride, max_frames=F, substeps_mean=float(ns.mean()), substeps_max=int(ns.max()),
                       seconds_per_trace=t_trace, seconds_per_step=t_step, frame_bytes=nbytes, frame_bytes_per_s=nbytes / t_trace,
                       trace_beyond_step_share=(t_trace - t_step) / t_trace)
            rows.append(row)
            print("%-16s stride %d (%3d rows, %6.1f MB): trace %8.1f us, tb_step %8.1f us, the trace's time beyond the step's %5.1f %%, %6.1f GB/s of "
                  "frames; substeps mean %.1f max %d" % (name, stride, F, nbytes * 1e-6, t_trace * 1e6, t_step * 1e6, 100 * row["trace_beyond_step_share"],
                                                         row["frame_bytes_per_s"] * 1e-9, row["substeps_mean"], row["substeps_max"]))
        # tb_step runs the flight in another kernel (the generic step kernel), so the difference above is two kernels', not the stores'
        # alone. The two strides are the same kernel on the same flights: what a stored row costs, and from it the stores' share at stride 8
        r8, r1 = rows[-2], rows[-1]
        per_row = (r1["seconds_per_trace"] - r8["seconds_per_trace"]) / (r1["max_frames"] - r8["max_frames"])
        for r in (r8, r1):
            r["seconds_per_stored_row"] = per_row
            r["stores_share_estimate"] = per_row * r["max_frames"] / r["seconds_per_trace"]
        print("%-16s a stored row costs %.3f us: an estimated %.1f %% of the trace at stride 8, %.1f %% at stride 1"
              % (name, per_row * 1e6, 100 * r8["stores_share_estimate"], 100 * r1["stores_share_estimate"]))
    out = dict(what="tb_swing_trace beside tb_step on the same states (tools/trace_rate.py): best of %d windows of %d calls, device events around each "
                    "call, whole call" % (args.repeats, args.launches), device=torch.cuda.get_device_name(0), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
