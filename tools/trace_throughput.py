#!/usr/bin/env python3
"""What recording episodes costs and how long the trajectory figure takes on the MI355X -> profiles/trace_throughput.json

    python tools/trace_throughput.py --out profiles/trace_throughput.json [--parent-dir DIR] [--rounds 3] [--repeats 7]

  (a) evaluate_batched, 500 test cases of CrowdSimVarNum-v0, 20 humans, seeded policy: the tree under --parent-dir (a checkout of the parent
      commit with its library built; omitted when the option is), this tree with traces=False and this tree with traces=True.  The three run
      as child processes of this one, alternating, `rounds` times; each child warms up once and times `repeats` calls (host clock around a
      call that ends in its own read-back): rounds x repeats = 21 samples per side by default.  The condition on traces=False: its median is
      not above the parent's median by more than the parent's own run-to-run range (max - min of the parent's samples); the range is written
      next to the verdict.  The cost of traces=True is reported, nothing is required of it.
  (b) one cn_render_trajectories launch at 256 x 256, stride 8: test cases 0..499 of (a)'s workload recorded by record_episodes (500 episodes x
      21 agents x their own lengths), and a synthetic 500 x 65 agents x 201 records (seeded random walks, every slot present).  Median of 21 launches bracketed by device events after 5 warm-ups, next to the
      store floor 4 n S^2 bytes at the 8.0 TB/s spec rate and to the same episodes' states drawn frame by frame through cn_render_scenes:
      one launch per step over all 500 episodes, times that kernel's recorded median for 500 x 20 x 256^2 (profiles/render_throughput.json)
      and times its median measured here on record 0 of the same episodes.
      cn_trace_metrics is timed on the same traces.  There is no earlier figure for (b): the kernels are new.

Every child runs under its own `timeout -k 10`; the first one that fails ends the run (nothing is started after it).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_SPEC = 8.0e12     # bytes / s
WARMUP, LAUNCHES = 5, 21
CHILD_LIMIT_S = 240


def _policy(torch, env_name, cfg):
    from crowdnav_prediction_attngraph_amd.policy import Policy
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
    dev = torch.device("cuda", 0)
    envs = make_vec_envs(env_name, 425, 1, 0.99, None, dev, True, config=cfg)
    torch.manual_seed(3)
    pol = Policy(envs.observation_space.spaces, envs.action_space, base="selfAttn_merge_srnn",
                 base_kwargs=dict(env_name=env_name, num_processes=1, num_mini_batch=1, seq_length=30)).to(dev)
    with torch.no_grad():
        pol.dist.fc_mean.bias.copy_(torch.tensor([0.3, -0.2]))
    envs.close()
    return pol, dev


def _timed(torch, fn, repeats):
    out = fn()                       # warm-up: code objects, allocator
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times, out


def _launch_us(torch, run):
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
    return dict(median_us=statistics.median(us), min_us=min(us), max_us=max(us), all_us=us)


def worker(what, repeats):
    import torch
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd import evaluation as EV
    res = {"what": what}
    cfg = C.non_randomized(**{"sim.human_num": 20})
    if what in ("eval", "eval_traces"):
        pol, dev = _policy(torch, "CrowdSimVarNum-v0", cfg)
        kw = {"traces": True} if what == "eval_traces" else {}          # the parent's evaluate_batched has no such argument
        res["times_s"], out = _timed(torch, lambda: EV.evaluate_batched(pol, "CrowdSimVarNum-v0", cfg, 425, 500, device=dev, **kw), repeats)
        res["metrics"] = out[0] if kw else out
    elif what == "figure":
        from crowdnav_prediction_attngraph_amd import hip
        pol, dev = _policy(torch, "CrowdSimVarNum-v0", cfg)
        tr = EV.record_episodes(pol, "CrowdSimVarNum-v0", cfg, 425, list(range(500)), device=dev)     # 500 distinct cases = 500 envs
        S, stride = 256, 8
        g = torch.Generator(device="cuda").manual_seed(7)
        n, cap, A_ = 500, 201, 65
        vel = (torch.rand(n, 1, A_, 2, generator=g, device="cuda") - 0.5) * 0.12 + torch.randn(n, cap, A_, 2, generator=g, device="cuda") * 0.02
        agents = torch.zeros(n, cap, A_, 6, device="cuda")
        agents[..., 0:2] = (torch.rand(n, 1, A_, 2, generator=g, device="cuda") - 0.5) * 12.0 + torch.cumsum(vel, dim=1)
        agents[..., 2:4] = vel * 4.0
        agents[..., 4], agents[..., 5] = 0.3, 1.0
        flags = torch.where(torch.rand(n, cap, A_, generator=g, device="cuda") < 2.0 / 3.0, 3, 1).to(torch.uint8)
        flags[:, :, 0] = 1
        synthetic = (agents, flags, torch.full((n,), cap, dtype=torch.int32, device="cuda"), torch.zeros(n, 2, device="cuda"))
        res["shapes"] = []
        for name, (ag, fl, ln, goal) in (("recorded", (tr.agents, tr.flags, tr.length, tr.goal)), ("synthetic", synthetic)):
            n, cap, A_ = (int(x) for x in ag.shape[:3])
            out = torch.empty(n, S, S, 4, dtype=torch.uint8, device="cuda")
            fig = _launch_us(torch, lambda: hip.render_trajectories(ag, fl, ln, goal, stride=stride, size=S, half_width=7.0, out=out))
            met = _launch_us(torch, lambda: hip.trace_metrics(ag, fl, ln, 0.25, 0.25))
            lengths = ln.cpu().tolist()
            # the frame-by-frame alternative: one cn_render_scenes launch draws one record of every episode (here: record 0, rebuilt as
            # EpisodeTraces.frames rebuilds it)
            humans = torch.zeros(n, A_ - 1, 8, dtype=torch.float64, device="cuda")
            humans[:, :, 0:4], humans[:, :, 6:8] = ag[:, 0, 1:, 0:4].double(), ag[:, 0, 1:, 4:6].double()
            robot = torch.zeros(n, 8, dtype=torch.float64, device="cuda")
            robot[:, 0:4], robot[:, 4:6] = ag[:, 0, 0, 0:4].double(), goal.double()
            visible = ((fl[:, 0, 1:] >> 1) & 1).contiguous()
            heading = robot[:, 2:4].float().contiguous()
            sc = _launch_us(torch, lambda: hip.render_scenes(humans, robot, visible=visible, robot_heading=heading, robot_radius=0.3, ring_radius=5.6,
                                                             size=S, half_width=7.0, out=out))
            res["shapes"].append(dict(name=name, episodes=n, cap=cap, agents=A_, size=S, stride=stride, records=sum(lengths), longest=max(lengths),
                                      bytes_stored=4 * n * S * S, store_floor_us_at_spec=4 * n * S * S / HBM_SPEC * 1e6,
                                      render_trajectories=fig, trace_metrics=met, render_scenes_one_frame=sc))
            del out
    print("RESULT " + json.dumps(res))


def child(tree, what, repeats):
    env = dict(os.environ, PYTHONPATH=tree)
    env.pop("CN_HIP_LIB", None)
    p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--worker", what, "--repeats", str(repeats)],
                       cwd=tree, env=env, capture_output=True, text=True)
    if p.returncode != 0:        # nothing more is started after a child that failed, faulted or ran into its limit
        raise SystemExit("worker %s in %s failed (%d):\n%s" % (what, tree, p.returncode, p.stderr[-3000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def spread(times):
    return dict(median_s=statistics.median(times), min_s=min(times), max_s=max(times), n=len(times), all_s=times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_throughput.json"))
    ap.add_argument("--parent-dir", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--worker", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.repeats)
    rec = {"workload": "evaluate_batched, 500 test cases of CrowdSimVarNum-v0, 20 humans, seeded untrained policy, fused rollout kernels",
           "rounds": a.rounds, "repeats": a.repeats}
    sides = ([("parent", os.path.abspath(a.parent_dir), "eval")] if a.parent_dir else []) + [("traces_off", ROOT, "eval"), ("traces_on", ROOT, "eval_traces")]
    times, metrics = {name: [] for name, _, _ in sides}, {}
    for _ in range(a.rounds):
        for name, tree, what in sides:             # alternating: all sides see the same box in the same minutes
            r = child(tree, what, a.repeats)
            times[name] += r["times_s"]
            metrics[name] = r["metrics"]
    for name in times:
        rec["eval_" + name] = spread(times[name])
    same = lambda x, y: json.dumps(x, sort_keys=True) == json.dumps(y, sort_keys=True)
    rec["summaries_equal"] = {name: same(metrics[name], metrics["traces_off"]) for name in metrics}
    off, on = rec["eval_traces_off"], rec["eval_traces_on"]
    rec["traces_on_cost"] = dict(extra_s_at_median=on["median_s"] - off["median_s"], ratio_at_median=on["median_s"] / off["median_s"])
    if "parent" in times:
        par = rec["eval_parent"]
        rng = par["max_s"] - par["min_s"]
        rec["bar"] = dict(rule="median of traces_off <= median of parent + (max - min of the parent's own samples)", parent_median_s=par["median_s"],
                          parent_range_s=rng, traces_off_median_s=off["median_s"], met=off["median_s"] <= par["median_s"] + rng)
    fig = child(ROOT, "figure", 1)
    scenes = None
    try:
        with open(os.path.join(ROOT, "profiles", "render_throughput.json")) as f:
            scenes = [s for s in json.load(f)["shapes"] if (s["envs"], s["humans"], s["size"]) == (500, 20, 256)][0]["median_us"]
    except (OSError, KeyError, IndexError, ValueError):
        pass
    for s in fig["shapes"]:
        # one cn_render_scenes launch per step over all 500 episodes: at the median measured here for one frame, and (20 humans) at that
        # kernel's recorded median for 500 x 20 x 256^2
        here = s["render_scenes_one_frame"]["median_us"]
        s["frame_by_frame"] = dict(launches=s["longest"], render_scenes_median_us_here=here, total_us_here=s["longest"] * here,
                                   render_scenes_recorded_median_us=scenes if s["agents"] == 21 else None,
                                   total_us_recorded=s["longest"] * scenes if scenes is not None and s["agents"] == 21 else None)
    rec["figure"] = dict(warmup=WARMUP, launches=LAUNCHES, timing="device events around each launch", hbm_spec_bytes_per_s=HBM_SPEC,
                         earlier_figure=None, shapes=fig["shapes"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    brief = {k: {x: v[x] for x in ("median_s", "min_s", "max_s")} for k, v in rec.items() if k.startswith("eval_")}
    brief.update(bar=rec.get("bar"), traces_on_cost=rec["traces_on_cost"], summaries_equal=rec["summaries_equal"],
                 figure=[(s["name"], s["render_trajectories"]["median_us"], s["trace_metrics"]["median_us"], s["store_floor_us_at_spec"], s["frame_by_frame"])
                         for s in fig["shapes"]])
    print(json.dumps(brief, indent=1))


if __name__ == "__main__":
    main()
