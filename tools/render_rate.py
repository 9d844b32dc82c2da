#!/usr/bin/env python3
"""How fast tb_render draws: images/s and bytes written/s at 4096 images of 64 x 48 and at 64 images of 256 x 192, rgb alone and with the
id and depth layers, as a fraction of the HBM write floor (the bytes written / 8 TB/s -- the least time the stores alone could take).

  python tools/render_rate.py                 # writes profiles/r19_render_rate.json

The states are Tennisbot-v0 / SwingRacket-v0 envs after 10 random steps from reset, the camera is default_camera(kind). Each figure
is the best of --repeats windows of --launches back-to-back launches on one stream, timed with device events after a warm-up; the
time is the whole call's (launch overhead included), so at the small shape it is an end-to-end rate, not the kernel's own.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
SHAPES = [(4096, 64, 48), (64, 256, 192)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_render_rate.json"))
    args = ap.parse_args()

    import torch
    from tennisbot_rl_amd import stepper

    if not torch.cuda.is_available():
        sys.exit("no GPU: a render rate can only be measured on one")
    rows = []
    for env_id in ("SwingRacket-v0", "Tennisbot-v0"):
        for n, W, H in SHAPES:
            env = stepper.BatchedEnv(env_id, n, device="cuda:0", seed=0)
            env.reset()
            gen = torch.Generator(device="cpu").manual_seed(0)
            for _ in range(10):
                env.step((torch.rand((n, env.act_dim), generator=gen) * 2 - 1).to(env.device))
            words, _ = env.get_state_words()
            for layers in (False, True):
                def draw():
                    return stepper.render_words(env.kind, env.params, words, width=W, height=H, layers=layers)
                for _ in range(10):
                    draw()
                torch.cuda.synchronize()
                best = float("inf")
                for _ in range(args.repeats):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(args.launches):
                        draw()
                    t1.record()
                    t1.synchronize()
                    best = min(best, t0.elapsed_time(t1) * 1e-3 / args.launches)
                nbytes = n * W * H * (3 + (5 if layers else 0))
                row = dict(env=env_id, images=n, width=W, height=H, layers=bool(layers), seconds_per_call=best, images_per_s=n / best,
                           pixels_per_s=n * W * H / best, bytes_written=nbytes, bytes_written_per_s=nbytes / best,
                           hbm_write_floor_s=nbytes / HBM_BYTES_PER_S, fraction_of_hbm_write_floor=nbytes / HBM_BYTES_PER_S / best)
                rows.append(row)
                print("%-15s %5d x %3d x %3d layers=%-5s %8.1f us/call  %10.0f images/s  %7.2f GB/s written  %.4f of the HBM write floor"
                      % (env_id, n, W, H, layers, best * 1e6, row["images_per_s"], row["bytes_written_per_s"] * 1e-9, row["fraction_of_hbm_write_floor"]))
            env.close()
    out = dict(what="tb_render rate (tools/render_rate.py): best of %d windows of %d launches, device events, whole call" % (args.repeats, args.launches),
               device=torch.cuda.get_device_name(0), hbm_bytes_per_s=HBM_BYTES_PER_S, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
