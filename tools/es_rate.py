#!/usr/bin/env python3
"""Rate of the fused ES evaluation (tb_es_evaluate), one JSON line per config (does not touch bench.py):
    python tools/es_rate.py [--reps K] [--out FILE]
Per config: env steps/s (sum of episode lengths / time of the evaluation call), lane utilisation (mean over max episode length
per 64-env wave), the SwingRacket fast-forward form. At the reference shape (400 members x 10 episodes) also generations/s of
ESTrainer.step with its evaluation / update split, and -- as CONTEXT, not a product path -- an unfused composition: a torch
float64 normaliser, a batched-einsum GatedCNN and BatchedEnv.step per agent step."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tennisbot_rl_amd import es  # noqa: E402
from tennisbot_rl_amd.params import ACT_DIM, ENV_SWING, ENV_TENNIS, OBS_DIM  # noqa: E402
from tennisbot_rl_amd.stepper import BatchedEnv  # noqa: E402

NAMES = {ENV_SWING: "SwingRacket-v0", ENV_TENNIS: "Tennisbot-v0"}
CONFIGS = [(400, 10), (4000, 1), (64, 64), (6560, 10)]  # members x envs per member (the last: ~65 536 envs)


def population(kind, M, dev):
    P = es.es_floats(OBS_DIM[kind], ACT_DIM[kind])
    g = torch.Generator(device=dev).manual_seed(1)
    w = es.initial_weights(kind, 0).to(dev)
    return es.pack_population(w, torch.randn((M // 2 + 1, P), generator=g, device=dev), 0.1)[:M].contiguous()


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def unfused_rate(kind, n, W, R, steps, dev):
    """context: the same episode work as separate launches per agent step"""
    O, A = OBS_DIM[kind], ACT_DIM[kind]
    env = BatchedEnv(kind, n, device=dev, seed=3)
    Wm = W[:, :es.es_floats(O, A)].repeat_interleave(R, dim=0)  # per env
    k = 0
    parts = {}
    for name, cout, cin in (("w0", 8, O), ("g0", 8, O), ("w1", 12, 8), ("g1", 12, 8), ("w2", A, 12)):
        parts[name] = Wm[:, k:k + cout * cin * 2].reshape(n, cout, cin, 2)
        k += cout * cin * 2
        parts[name + "b"] = Wm[:, k:k + cout]
        k += cout

    def conv(name, x, d):  # x [n, cin, L] -> [n, cout, L - d]
        w = parts[name]
        return torch.einsum("noi,nil->nol", w[..., 0], x[..., :-d]) + torch.einsum("noi,nil->nol", w[..., 1], x[..., d:]) + parts[name + "b"][..., None]

    def run():
        obs = env.reset()
        cnt = torch.zeros((n, 1), dtype=torch.float64, device=dev)
        mean = torch.zeros((n, O), dtype=torch.float64, device=dev)
        md = torch.zeros_like(mean)
        hist = None
        for t in range(steps):
            x = obs.double()
            cnt += 1
            last = mean.clone()
            mean += (x - mean) / cnt
            md += (x - last) * (x - mean)
            row = ((x - mean) / torch.sqrt((md / cnt).clamp(min=1e-2))).float()
            hist = row[:, :, None].repeat(1, 1, 8) if hist is None else torch.cat([hist[:, :, 1:], row[:, :, None]], dim=2)
            h = torch.tanh(conv("w0", hist, 1)) * torch.sigmoid(conv("g0", hist, 1))
            h = torch.tanh(conv("w1", h, 2)) * torch.sigmoid(conv("g1", h, 2))
            a = conv("w2", h, 4)[..., 0].clamp(-1, 1)
            obs, rew, done = env.step(a.contiguous())
        return steps
    run()
    dt, _ = timed(run, 1)
    env.close()
    return n * steps / dt


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for kind in (ENV_SWING, ENV_TENNIS):
        for M, R in CONFIGS:
            n = M * R
            env = BatchedEnv(kind, n, device=dev, seed=2, pipeline=kind == ENV_SWING)
            W = population(kind, M, dev)
            env.es_evaluate(W, R)  # warm-up
            dt, (ret, length) = timed(lambda: env.es_evaluate(W, R), args.reps)
            L = length.reshape(-1).cpu().numpy().astype(np.float64)
            waves = [L[k:k + 64] for k in range(0, n, 64)]
            rec = dict(env=NAMES[kind], members=M, envs_per_member=R, envs=n, eval_s=dt, env_steps=int(L.sum()),
                       env_steps_per_s=L.sum() / dt, mean_length=float(L.mean()),
                       lane_utilisation=float(np.mean([w.mean() / w.max() for w in waves])),
                       ff_form=env.pipeline_form() if kind == ENV_SWING else "n/a")
            env.close()
            if (M, R) == (400, 10):
                tr = es.ESTrainer(NAMES[kind], popsize=200, repeats=10, seed=0, device=dev)
                tr.step()
                ev, up = [], []
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    eps = torch.randn((tr.popsize, tr.P), generator=tr.gen, device=dev)
                    pop = es.pack_population(tr.w, eps, tr.sigma, tr.stride)
                    r, _ = tr.env.es_evaluate(pop, tr.repeats)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    f = es.fitness(r)
                    tr.w, _ = es.es_update(tr.w, eps, f[:tr.popsize], f[tr.popsize:], tr.lr, tr.elite)
                    torch.cuda.synchronize()
                    ev.append(t1 - t0)
                    up.append(time.perf_counter() - t1)
                tr.close()
                rec.update(generation_s=float(np.mean(ev) + np.mean(up)), generations_per_s=1.0 / float(np.mean(ev) + np.mean(up)),
                           generation_eval_s=float(np.mean(ev)), generation_update_s=float(np.mean(up)))
                steps = 26 if kind == ENV_SWING else 100
                rec["unfused_context_env_steps_per_s"] = unfused_rate(kind, n, W, R, steps, dev)
                rec["unfused_context_steps"] = steps
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
