#!/usr/bin/env python3
"""Time of one cn_render_scenes launch on the MI355X -> profiles/render_throughput.json

    python tools/render_throughput.py --out profiles/render_throughput.json

Three shapes (envs x humans x image side): 4096 x 20 x 128, 8192 x 50 x 128, 500 x 20 x 256.  The scenes are synthetic (seeded): humans
spread uniformly over the arena with the default radius and random velocities, all slots present, a third of them out of sight, sensor ring
on, no dots.  Per shape: 5 warm-up launches, then 21 launches each bracketed by device events on the launch's stream; the record keeps every
sample and reports the median next to the store floor 4 n S^2 bytes / HBM rate (8.0 TB/s spec and 6.29 TB/s measured float4 copy).  There is
no parent-commit figure to compare with: the kernel is new.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(4096, 20, 128), (8192, 50, 128), (500, 20, 256)]
HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12     # bytes / s
WARMUP, LAUNCHES = 5, 21


def scenes(torch, n, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g, device="cuda", dtype=torch.float64) * 2.0 - 1.0
    humans = torch.zeros(n, H, 8, dtype=torch.float64, device="cuda")
    humans[:, :, 0:2] = u(n, H, 2) * 6.0
    humans[:, :, 2:4] = u(n, H, 2)
    humans[:, :, 4:6] = -humans[:, :, 0:2]
    humans[:, :, 6] = 0.3
    humans[:, :, 7] = 1.0
    robot = torch.zeros(n, 8, dtype=torch.float64, device="cuda")
    robot[:, 0:2] = u(n, 2) * 5.0
    robot[:, 2:4] = u(n, 2)
    robot[:, 4:6] = u(n, 2) * 6.0
    visible = (torch.rand(n, H, generator=g, device="cuda") < 2.0 / 3.0).to(torch.uint8)
    return humans, robot, visible


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_throughput.json"))
    args = ap.parse_args()
    import torch
    from crowdnav_prediction_attngraph_amd import hip
    if not torch.cuda.is_available():
        raise SystemExit("render_throughput: no GPU visible (nothing is measured without the MI355X)")
    rec = {"kernel": "cn_render_scenes (render_scenes_kernel: 32 x 32 pixel tile per workgroup, 4 pixels per lane)", "warmup": WARMUP,
           "launches": LAUNCHES, "timing": "device events around each launch", "device": torch.cuda.get_device_name(0),
           "hbm_bytes_per_s": {"spec": HBM_SPEC, "measured_float4_copy": HBM_MEASURED}, "shapes": []}
    for n, H, S in SHAPES:
        humans, robot, visible = scenes(torch, n, H, 1000 + H)
        out = torch.empty(n, S, S, 4, dtype=torch.uint8, device="cuda")
        heading = robot[:, 2:4].to(torch.float32).contiguous()
        run = lambda: hip.render_scenes(humans, robot, visible=visible, robot_heading=heading, robot_radius=0.3, ring_radius=5.6, size=S,
                                        half_width=7.0, out=out)
        for _ in range(WARMUP):
            run()
        torch.cuda.synchronize()
        us = []
        for _ in range(LAUNCHES):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
        nbytes = 4 * n * S * S
        med = statistics.median(us)
        rec["shapes"].append({"envs": n, "humans": H, "size": S, "bytes_stored": nbytes, "median_us": med, "min_us": min(us), "max_us": max(us),
                              "all_us": us, "store_floor_us": {"spec": nbytes / HBM_SPEC * 1e6, "measured_copy": nbytes / HBM_MEASURED * 1e6},
                              "stored_bytes_per_s_at_median": nbytes / (med * 1e-6), "images_per_s_at_median": n / (med * 1e-6)})
        print("%5d envs x %2d humans x %d^2: median %.1f us (min %.1f, max %.1f); store floor %.1f us at 8.0 TB/s, %.1f us at 6.29 TB/s"
              % (n, H, S, med, min(us), max(us), nbytes / HBM_SPEC * 1e6, nbytes / HBM_MEASURED * 1e6), flush=True)
        del out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
