#!/usr/bin/env python3
"""Same-process-per-run A/B of the pipelined SwingRacket step kernel's two forms (TbOptions.step_waves = 1 / 2) at the batch sizes the
automatic choice covers: the headline's replayed rollout graph (1040 agent steps, pool form), median of 15 timed replays after bench.py's
settle time, each (size, form) in a process of its own, alternated twice. Run on the GPU box:  python tools/diag/r05_step_waves_ab.py"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
T = 1040
if len(sys.argv) > 3 and sys.argv[1] == "--child":
    n, waves = int(sys.argv[2]), int(sys.argv[3])
    import torch
    from tennisbot_rl_amd.params import ENV_SWING
    from tennisbot_rl_amd.rollout import RolloutBuffer
    from tennisbot_rl_amd.stepper import BatchedEnv
    dev = torch.device("cuda", 0)
    env = BatchedEnv(ENV_SWING, n, device=dev, seed=0, track_terminal_obs=False, pipeline=True, options=dict(step_waves=waves))
    assert env.step_waves() == waves
    buf = RolloutBuffer(ENV_SWING, T, n, dev); torch.manual_seed(0); buf.actions.uniform_(-1, 1); buf.bind(env); env.reset()
    for t in range(T): buf.step_into(env, t)
    env.flush()
    g = env.capture(lambda: buf.step_range(env, 0, T))
    t_end = time.perf_counter() + 1.5
    while time.perf_counter() < t_end: g.replay(); torch.cuda.synchronize()
    ts = []
    for _ in range(15):
        torch.cuda.synchronize(); t0 = time.perf_counter(); g.replay(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    ts.sort()
    print(json.dumps({"envs": n, "step_waves": waves, "rate_M": round(n * T / ts[len(ts) // 2] / 1e6, 1)})); sys.exit(0)
for n in (4096, 8192, 16384):
    for rep in range(2):
        for waves in (1, 2):
            r = subprocess.run([sys.executable, __file__, "--child", str(n), str(waves)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                print(r.stderr[-600:]); sys.exit(1)
            print(r.stdout.strip().splitlines()[-1], flush=True)
