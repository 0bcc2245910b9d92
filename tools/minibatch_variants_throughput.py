#!/usr/bin/env python3
"""One PPO.update with use_self_attn / sort_humans off, before and after cn_ppo_minibatch_step_variant -> profiles/minibatch_variants_throughput.json

    python tools/minibatch_variants_throughput.py --parent-dir DIR --out profiles/minibatch_variants_throughput.json [--rounds 2]

The protocol of tools/minibatch_sized_throughput.py: one PPO.update at 4096 envs x 20 humans, T = 30, 2 048 envs per minibatch, 5 epochs = 10
optimiser steps, as trainer.train runs it; the tree under --parent-dir (a checkout of the parent commit with its library built) and this tree as
alternating child processes in one box (the side that goes first alternates as well), `--rounds` children of three timed updates per side and
configuration (update 0 of a child is the warm-up): six updates each at the default.  Every child runs under its own `timeout`, and the chain
stops at the first child that fails.  Four configurations: the three variants and the default network.  Per configuration: update_s median
[min..max] of both sides, the child's peak device memory (torch.cuda.max_memory_allocated, which counts the step's cached workspace and the
autograd graph alike), and the producer PPO.update took.  In the parent a variant's update runs the autograd-joined producer; in this tree it
runs one cn_ppo_minibatch_step_variant per minibatch.

What the record may carry as a claim: "faster" for a variant only where this tree's [min..max] lies below the parent's without overlap
(this_below_parent_without_overlap); otherwise the intervals overlap and the variant stands on coverage.  The default network runs the same
launches in both trees, so its median must lie inside the parent's own range (this_median_inside_parent_range).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name: (use_self_attn, sort_humans)
CONFIGS = {"no_self_attn": (False, True), "unsorted": (True, False), "no_self_attn_unsorted": (False, False), "default": (True, True)}
CHILD = """
import json, sys
from types import SimpleNamespace
sys.path.insert(0, '.')
import torch
from crowdnav_prediction_attngraph_amd import config as C
from crowdnav_prediction_attngraph_amd import ppo
from crowdnav_prediction_attngraph_amd.trainer import train
attn, srt = json.loads(sys.argv[1])
took = []
plan = ppo.PPO._fast_plan
def seen(self, rollouts):
    p = plan(self, rollouts)
    took.append(type(p[0]).__name__ if p is not None else "autograd-joined (rows past the bound)")
    return p
ppo.PPO._fast_plan = seen
cfg = C.non_randomized(**{"sim.human_num": 20})
cfg.args = SimpleNamespace(**dict(vars(cfg.args), sort_humans=bool(srt)))
hist, _ = train("CrowdSimVarNum-v0", num_processes=int(sys.argv[2]), num_steps=30, num_updates=4, seed=425, config=cfg, log=None, use_self_attn=bool(attn))
print("RESULT " + json.dumps({"update_s": [r["update_s"] for r in hist[1:]], "peak_bytes": int(torch.cuda.max_memory_allocated()),
                              "producer": sorted(set(took)) or ["autograd-joined"]}))
"""


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": list(xs)}


def child(tree, switches, E, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", CHILD, json.dumps(list(switches)), str(E)], cwd=tree, capture_output=True, text=True)
    if p.returncode != 0:                                   # a fault, an abort or the time limit: nothing more is started
        raise RuntimeError("update child in %s failed (%d): %s" % (tree, p.returncode, p.stderr[-2000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parent-dir", required=True)
    ap.add_argument("--rounds", type=int, default=2, help="child processes per side and configuration, three timed updates each")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one child may take")
    ap.add_argument("--configs", default=",".join(CONFIGS), help="comma-separated subset of: " + ", ".join(CONFIGS))
    a = ap.parse_args()
    parent = os.path.abspath(a.parent_dir)
    res = {"cmd": " ".join(sys.argv), "envs": a.envs, "humans": 20, "steps": 30, "minibatches": 2, "ppo_epoch": 5, "rows": []}
    for name in a.configs.split(","):
        switches = CONFIGS[name]
        runs = {"parent": [], "this": []}
        for r in range(a.rounds):
            pair = (("parent", parent), ("this", ROOT))
            for side, tree in (pair if r % 2 == 0 else pair[::-1]):
                runs[side].append(child(tree, switches, a.envs, a.child_timeout))
                print(name, side, runs[side][-1], flush=True)
        row = {"config": name, "use_self_attn": switches[0], "sort_humans": switches[1]}
        for side, rs in runs.items():
            row[side + "_update_s"] = summary([x for r in rs for x in r["update_s"]])
            row[side + "_peak_bytes"] = max(r["peak_bytes"] for r in rs)
            row[side + "_producer"] = sorted({p for r in rs for p in r["producer"]})
        p, t = row["parent_update_s"], row["this_update_s"]
        row["this_below_parent_without_overlap"] = bool(t["max"] < p["min"])
        row["intervals_overlap"] = bool(t["max"] >= p["min"] and p["max"] >= t["min"])
        row["this_median_inside_parent_range"] = bool(p["min"] <= t["median"] <= p["max"])
        res["rows"].append(row)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res)[:4000])


if __name__ == "__main__":
    main()
