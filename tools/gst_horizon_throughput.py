#!/usr/bin/env python3
"""What a prediction horizon costs on the GST device path, and what carrying the horizon costs the shipped five steps.

    python tools/gst_horizon_throughput.py --out profiles/gst_horizon_throughput.json [--parent DIR]

Per horizon P in {1, 3, 5, 8}: one cn_gst_wrapper_step (history push, the GST forward with P decode steps, penalty / edge write-back / sort) at
2048 envs x 20 humans over a stream of drifting humans with a fifth invisible and 2 % visibility flips per step (frames are taken over as they are
in a rollout).  Device events around each Python call -- a step as the caller sees it, launch gaps included, not summed kernel time --, 5 warm-ups, the median of 21 with [min .. max].  There is no earlier figure for P != 5: before the
horizon reached the kernels only P = 5 ran.

--parent DIR (a built checkout of the parent commit): the cost to the default.  P = 5 on DIR and on this tree as ALTERNATING CHILD PROCESSES (a
child imports one tree's package and library and measures one thing), --runs of each (at least 8), the side that goes first alternating; the same
for one cn_gst_train_step at B = 32 sequences of 20 pedestrians (dropout 0.1) and one cn_gst_eval_step at B = 32, S = 20.  A child reports its median
of 21; the record holds every child's median, each side's median of medians with [min .. max], and whether this tree's median lies inside the
parent's own [min .. max] -- if it does not, that is a regression to fix, not a number to re-baseline."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, H, WARMUP, ITERS = 2048, 20, 5, 21
HORIZONS = (1, 3, 5, 8)


def _timed(fn, torch):
    """fn(i) for i in range(WARMUP + ITERS), device events around each call -> the ITERS last times in microseconds."""
    out = []
    for i in range(WARMUP + ITERS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out[WARMUP:]


def _stats(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "n": len(v)}


def child(what, root, P):
    """Runs in a process of its own with `root`'s package: one measurement -> one JSON line."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from crowdnav_prediction_attngraph_amd.gst import GSTPredictor
    from crowdnav_prediction_attngraph_amd.gst_hip import HipGST, HipGstEvaluator, HipGstTrainer
    torch.manual_seed(0)
    if what == "wrapper":
        m = GSTPredictor().cuda()
        g = HipGST(H, E) if P == 5 else HipGST(H, E, pred_steps=P)          # (the parent's handle takes no horizon)
        g.set_weights(m.state_dict())
        g.wrapper_set_interval(1)
        g.wrapper_reset(E)
        rs = np.random.RandomState(1)
        pos, vel = rs.standard_normal((E, H, 2)).astype(np.float32) * 3, rs.standard_normal((E, H, 2)).astype(np.float32) * 0.2
        vis = rs.uniform(size=(E, H)) > 0.2
        D = 2 * (P + 1)
        obs = []
        for t in range(WARMUP + ITERS):
            pos = pos + vel
            vis = vis ^ (rs.uniform(size=(E, H)) < 0.02)
            se = np.full((E, H, D), 15.0, np.float32)
            se[:, :, :2] = np.where(vis[..., None], pos, 15.0)
            rn = np.zeros((E, 1, 7), np.float32)
            rn[:, 0, 2] = 0.3
            obs.append({"robot_node": torch.from_numpy(rn).cuda(), "spatial_edges": torch.from_numpy(se).cuda(), "visible_masks": torch.from_numpy(vis.copy()).cuda()})
        rews, out = torch.zeros(E, device="cuda"), torch.empty(E, H, D, device="cuda")
        times = _timed(lambda i: g.wrapper_step(obs[i], rews, 0.6, -20.0, out=out), torch)
    else:
        B, N, S = 32, 20, 20
        m = GSTPredictor(5, P).cuda()
        gen = torch.Generator().manual_seed(2)
        lm = (torch.rand(B, N, 5 + P, generator=gen) > 0.2).float()
        lm[:, 0] = 1.0
        v_obs, v_pred = (0.4 * torch.randn(B, 5, N, 2, generator=gen)).cuda(), (0.4 * torch.randn(B, P, N, 2, generator=gen)).cuda()
        lm = lm.cuda()
        if what == "train":
            tr = HipGstTrainer(m)
            times = _timed(lambda i: tr.loss_and_grads(v_obs, v_pred, lm, p_drop=0.1, seed=i), torch)
        else:
            ev = HipGstEvaluator(m.eval())
            noise = torch.randn(B, S, P, N, 2, generator=gen).cuda()
            times = _timed(lambda i: ev.evaluate_batch(v_obs, v_pred, lm, noise), torch)
    print(json.dumps(dict(_stats(times), what=what, P=P)))


def _run_child(what, root, P):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--root", root, "--horizon", str(P)], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError("child %s on %s failed (%d):\n%s" % (what, root, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: measure the cost to P = 5")
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--child", default=None, choices=("wrapper", "train", "eval"))
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--horizon", type=int, default=5)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.root, a.horizon)
    rec = {"envs": E, "humans": H, "warmup": WARMUP, "iterations": ITERS, "unit": "microseconds, device events",
           "note": "no earlier figure exists for P != 5: only P = 5 ran on the device before", "wrapper_step": {}}
    for P in HORIZONS:
        rec["wrapper_step"]["P=%d" % P] = _run_child("wrapper", ROOT, P)
        print("wrapper_step P=%d: %s" % (P, rec["wrapper_step"]["P=%d" % P]), flush=True)
    if a.parent:
        runs = max(8, a.runs)
        rec["default_cost"] = {"runs_each": runs}
        for what in ("wrapper", "train", "eval"):
            sides = {"parent": [], "tree": []}
            for k in range(runs):
                order = ("parent", "tree") if k % 2 == 0 else ("tree", "parent")
                for side in order:
                    sides[side].append(_run_child(what, a.parent if side == "parent" else ROOT, 5)["median_us"])
            p, t = sides["parent"], sides["tree"]
            rec["default_cost"][what] = {"parent": dict(_stats(p), medians=p), "tree": dict(_stats(t), medians=t),
                                         "tree_median_inside_parent_range": min(p) <= statistics.median(t) <= max(p)}
            print("P=5 %s: parent %.1f [%.1f .. %.1f]  tree %.1f [%.1f .. %.1f]  inside: %s"
                  % (what, statistics.median(p), min(p), max(p), statistics.median(t), min(t), max(t), rec["default_cost"][what]["tree_median_inside_parent_range"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
