#!/usr/bin/env python3
"""What HipEnvBatch.set_scene costs on the MI355X, beside reset() of the same batch -> profiles/scene_throughput.json; and the default path's
A/B against a checkout of the parent commit -> profiles/scene_bench_ab.jsonl.

    python tools/scene_throughput.py [--out profiles/scene_throughput.json]
    python tools/scene_throughput.py --bench-ab PARENT_DIR [--ab-out profiles/scene_bench_ab.jsonl] [--runs 8]

  throughput: one set_scene(check=False) of every env at 4096 envs x 20 humans and at 8192 x 50 (CrowdSimVarNum-v0, fixed attributes): the
      scene is the batch's own state read once with get_state.  5 warm-ups, then 21 calls, each bracketed by device events on the caller's
      stream; median [min..max].  reset() of the same batch is measured the same way in the same run: reset() did not change, so it is the
      yardstick.  The events see what the call puts on the caller's stream (the scene / reset kernel and, up to 32 agents, the ORCA lane
      kernel); `to_idle_us` is the host clock from the call to an idle device, which also covers the side-stream ORCA tail and the episode
      pre-generation.  There is no bar: the call is new and is not on a training path.
  --bench-ab: `python bench.py --gpus 1 --steps 20 --warmup 5` in PARENT_DIR (a checkout of the parent commit with its library built) and in this
      tree as alternating child processes, `runs` each, the side that goes first alternating; every result line goes into the .jsonl, then a
      summary line.  Bar: this tree's median ms per step lies inside the parent's own [min..max].

Every child runs under its own `timeout -k 10`; the first one that fails ends the run (nothing is started after it)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, CALLS = 5, 21
SHAPES = ((4096, 20), (8192, 50))
CHILD_LIMIT_S = 180


def _spread(us):
    return dict(median_us=statistics.median(us), min_us=min(us), max_us=max(us), all_us=us)


def _measure(torch, run):
    for _ in range(WARMUP):
        run()
    torch.cuda.synchronize()
    ev, idle = [], []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        idle.append((time.perf_counter() - t0) * 1e6)
        ev.append(a.elapsed_time(b) * 1e3)
    return dict(_spread(ev), to_idle_us=_spread(idle))


def throughput(out):
    import torch
    sys.path.insert(0, ROOT)
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
    torch.cuda.set_device(0)
    rec = dict(workload="CrowdSimVarNum-v0, fixed attributes, every env selected, check=False; the scene is the batch's own state",
               warmup=WARMUP, calls=CALLS, timing="device events on the caller's stream around each call; to_idle_us: host clock to an idle device",
               earlier_figure=None, shapes=[])
    for E, H in SHAPES:
        env = HipEnvBatch(A.default_env_config(human_num=H, nenv=E), E, 425)
        env.reset()
        humans, robot = env.get_state()
        scene = _measure(torch, lambda: env.set_scene(humans, robot, check=False))
        reset = _measure(torch, env.reset)
        rec["shapes"].append(dict(envs=E, humans=H, set_scene=scene, reset=reset, bytes_read=int(humans.numel() + robot.numel()) * 8))
        env.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for s in rec["shapes"]:
        print("%d x %d: set_scene %.1f us [%.1f..%.1f] (to idle %.1f), reset %.1f us [%.1f..%.1f] (to idle %.1f)" % (
            s["envs"], s["humans"], s["set_scene"]["median_us"], s["set_scene"]["min_us"], s["set_scene"]["max_us"],
            s["set_scene"]["to_idle_us"]["median_us"], s["reset"]["median_us"], s["reset"]["min_us"], s["reset"]["max_us"],
            s["reset"]["to_idle_us"]["median_us"]))


def _bench(tree):
    env = dict(os.environ, PYTHONPATH=tree)
    env.pop("CN_HIP_LIB", None)
    p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"],
                       cwd=tree, env=env, capture_output=True, text=True)
    if p.returncode != 0:        # nothing more is started after a child that failed, faulted or ran into its limit
        raise SystemExit("bench.py in %s failed (%d):\n%s" % (tree, p.returncode, p.stderr[-3000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def bench_ab(parent, out, runs):
    trees = {"parent": os.path.abspath(parent), "this": ROOT}
    ms = {"parent": [], "this": []}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for k in range(runs):
            for side in (("parent", "this") if k % 2 == 0 else ("this", "parent")):
                r = _bench(trees[side])
                ms[side].append(r["ms_per_step"])
                f.write(json.dumps(dict(side=side, run=k + 1, result=r)) + "\n")
                f.flush()
        par, this = ms["parent"], ms["this"]
        summary = dict(summary=True, rule="this tree's median ms per step inside the parent's own [min..max]", runs_each=runs,
                       parent_ms=dict(median=statistics.median(par), min=min(par), max=max(par), all=par),
                       this_ms=dict(median=statistics.median(this), min=min(this), max=max(this), all=this),
                       met=min(par) <= statistics.median(this) <= max(par), faster_than_parent_range=statistics.median(this) < min(par))
        f.write(json.dumps(summary) + "\n")
    print(json.dumps(summary, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_throughput.json"))
    ap.add_argument("--bench-ab", default=None, metavar="PARENT_DIR")
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "scene_bench_ab.jsonl"))
    ap.add_argument("--runs", type=int, default=8)
    a = ap.parse_args()
    if a.bench_ab:
        return bench_ab(a.bench_ab, a.ab_out, a.runs)
    return throughput(a.out)


if __name__ == "__main__":
    main()
