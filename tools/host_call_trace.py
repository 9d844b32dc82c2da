#!/usr/bin/env python3
"""A fixed host-side workload for comparing two builds of the library call by call (not kernel by kernel): 4096 pipelined
SwingRacket envs, 104 eager tb_step calls and a flush, a capture of the same 104 steps and two replays, then tb_set_params
switching racket<->court contact on.
  rocprofv3 --hip-trace --stats -d OUT -- python tools/host_call_trace.py [LIB]   -> per-API call counts (tracing only, no counters)
  python tools/host_call_trace.py --time [LIB]   -> one JSON line: microseconds per eager tb_step call (host path on the clock), median of 9 x 1040
LIB: another build of the same ABI (default: the in-tree library). Reads nothing outside the repository."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = [a for a in sys.argv[1:] if a != "--time"]
import torch
from tennisbot_rl_amd import stepper
if args:
    stepper.use_library(args[0])
from tennisbot_rl_amd.params import ENV_SWING, F_AUTO_RESET, F_DEFAULT, F_RACKET_GROUND, default_params
from tennisbot_rl_amd.rollout import RolloutBuffer
from tennisbot_rl_amd.stepper import BatchedEnv

N, T = 4096, 104
dev = torch.device("cuda", 0)
env = BatchedEnv(ENV_SWING, N, device=dev, seed=0, track_terminal_obs=False, pipeline=True)
buf = RolloutBuffer(ENV_SWING, T, N, dev)
torch.manual_seed(0)
buf.actions.uniform_(-1, 1)
buf.bind(env)
env.reset()
if "--time" in sys.argv[1:]:
    for t in range(T): buf.step_into(env, t)
    env.flush(); torch.cuda.synchronize()
    us = []
    for _ in range(9):
        t0 = time.perf_counter()
        for _r in range(10):
            for t in range(T): buf.step_into(env, t)
        dt = time.perf_counter() - t0  # enqueue time only: the device is joined after the clock stops
        env.flush(); torch.cuda.synchronize()
        us.append(dt / (10 * T) * 1e6)
    us.sort()
    print(json.dumps({"eager_step_us": round(us[len(us) // 2], 3), "min": round(us[0], 3), "max": round(us[-1], 3)}))
    sys.exit(0)
for t in range(T): buf.step_into(env, t)
env.flush(); torch.cuda.synchronize()
g = env.capture(lambda: buf.step_range(env, 0, T))
for _ in range(2): g.replay()
torch.cuda.synchronize()
env.set_params(default_params(flags=F_DEFAULT | F_AUTO_RESET | F_RACKET_GROUND))
torch.cuda.synchronize()
print(json.dumps({"phase": env.phase(), "reward_sum": float(buf.rewards.double().sum())}))
