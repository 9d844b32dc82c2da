#!/usr/bin/env python3
"""Where a wave of the two-wave SwingRacket step kernel (tb_kernels.hpp, two_wave_step) spends its cycles in the 25 short steps of an
episode, at 4096 envs (diagnostic build, -DTB_DIAG_STAMPS; needs a GPU). For each wave, s_memtime cycles from the kernel's
entry stamp to: its loads landed (an explicit wait for every load: the build is not the product's), the common-path gate done,
barrier arrival, barrier passed, stores issued. Every mark fences the scheduler and costs ~40 cycles: read the differences, not the
absolute span. Prints a table (and writes it to --out FILE: profiles/r06_two_wave_stamps_*.txt).
On a handle in lockstep these are launches of the kernel's SHORT form (BatchedEnv.step_form() == 2), whose waves issue their own
loads: "loads landed" and "gate done" then coincide (that form has no gate).
    python tools/diag/r06_two_wave_stamps.py [--envs N] [--out FILE] [--lib BUILD.so]"""
import argparse
import ctypes
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tennisbot_rl_amd import stepper  # noqa: E402
from tennisbot_rl_amd.build import HIPCC_FLAGS, SOURCES, hipcc  # noqa: E402
from tennisbot_rl_amd.params import ENV_SWING  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--out", default=None)
ap.add_argument("--lib", default=None, help="a -DTB_DIAG_STAMPS build made beforehand (default: compile one now)")
args = ap.parse_args()
out = args.lib
if out is None:
    out = os.path.join(tempfile.mkdtemp(prefix="tb_r06_"), "libtb_stamps.so")
    subprocess.check_call([hipcc()] + HIPCC_FLAGS + ["-DTB_DIAG_STAMPS", "-o", out] + SOURCES)
stepper.use_library(out)
L = stepper.load_library()
L.tb_diag_read_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
n = args.envs
EPISODES = 4
env = stepper.BatchedEnv(ENV_SWING, n, seed=0, pipeline=True, track_terminal_obs=False)
assert env.step_waves() == 2
rng = np.random.Generator(np.random.PCG64(0))
acts = torch.from_numpy(rng.uniform(-1, 1, (26, n, 6)).astype(np.float32)).cuda()
env.reset()
buf = (ctypes.c_ulonglong * 16)()
tot = np.zeros(16)
for ep in range(EPISODES):
    env.flush()
    L.tb_diag_read_stamps(buf, 1)  # steps 1-25 only: the parking step and the pool's fast-forward are left out
    for t in range(25):
        env.step(acts[t])
    L.tb_diag_read_stamps(buf, 1)
    if ep > 0:  # the first episode warms up
        tot += np.array(list(buf), dtype=np.float64)
    env.step(acts[25])
env.close()
marks = ["loads landed", "gate done", "barrier arrival", "barrier passed", "stores issued"]
lines = ["two-wave step kernel, %d envs, steps 1-25 of %d episodes: cycles from the kernel's entry stamp, mean per wave per launch" % (n, EPISODES - 1)]
for name, base in (("racket wave (wave 0)", 0), ("ball wave (wave 1)", 8)):
    waves = tot[base + 5]
    lines.append("%s: %d wave-launches" % (name, waves))
    prev = 0.0
    for k, m in enumerate(marks):
        v = tot[base + k] / max(waves, 1)
        lines.append("    %-16s %7.0f   (+%.0f)" % (m, v, v - prev))
        prev = v
    span = tot[base + 4] / max(waves, 1) - tot[base] / max(waves, 1)
    gate = (tot[base + 1] - tot[base]) / max(waves, 1)
    lines.append("    gate share of the span from loads landed to stores issued: %.1f %%" % (100.0 * gate / max(span, 1.0)))
txt = "\n".join(lines)
print(txt)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(txt + "\n")
