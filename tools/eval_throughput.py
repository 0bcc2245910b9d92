#!/usr/bin/env python3
"""Wall time of the batched evaluation protocol on the MI355X -> profiles/eval_batched_throughput.json

    python tools/eval_throughput.py --out profiles/eval_batched_throughput.json [--parent-dir DIR] [--rounds 3] [--repeats 7]

  (a) / (b) evaluate_batched, 500 test cases of CrowdSimVarNum-v0, 20 humans, seeded policy: (a) the tree under --parent-dir (a checkout of the
            parent commit with its library built; omitted when the option is), (b) this tree.  Both sides run as child processes of this
            one, alternating, `rounds` times; each child warms up once and times `repeats` calls (host clock around a call that ends in its
            own read-back).  The record holds every repeat: the bar for (b) is (a)'s own spread, not a figure chosen beforehand.
  (c)       CrowdSimPredRealGST-v0 behind the GST wrapper (seeded predictor), this tree: evaluate_batched next to the sequential evaluate()
            for the same 500 episodes.
  (d)       the bookkeeping alone, this tree: the same call with cn_eval_accumulate and with the torch-op form.
  (e)       what eval_interval costs inside train() at 4096 envs: rec["eval_s"] next to rollout_s + update_s, with and without.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _policy(torch, env_name, cfg, pred=None):
    from crowdnav_prediction_attngraph_amd.policy import Policy
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
    dev = torch.device("cuda", 0)
    envs = make_vec_envs(env_name, 425, 1, 0.99, None, dev, True, config=cfg, **({"pretext_wrapper": True, "predictor": pred} if pred is not None else {}))
    torch.manual_seed(3)
    pol = Policy(envs.observation_space.spaces, envs.action_space, base="selfAttn_merge_srnn",
                 base_kwargs=dict(env_name=env_name, num_processes=1, num_mini_batch=1, seq_length=30)).to(dev)
    with torch.no_grad():
        pol.dist.fc_mean.bias.copy_(torch.tensor([0.3, -0.2]))
    return pol, envs, dev


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


def worker(what, repeats):
    import torch
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd import evaluation as EV
    res = {"what": what}
    if what == "varnum":
        cfg = C.non_randomized(**{"sim.human_num": 20})
        pol, envs, dev = _policy(torch, "CrowdSimVarNum-v0", cfg)
        envs.close()
        res["times_s"], m = _timed(torch, lambda: EV.evaluate_batched(pol, "CrowdSimVarNum-v0", cfg, 425, 500, device=dev), repeats)
        res["metrics"] = m
    elif what == "bookkeeping":
        cfg = C.non_randomized(**{"sim.human_num": 20})
        pol, envs, dev = _policy(torch, "CrowdSimVarNum-v0", cfg)
        envs.close()
        for name, kw in (("kernel", {}), ("torch_ops", {"use_kernel": False}), ("kernel_poll_1", {"poll_every": 1})):
            res[name + "_times_s"], _ = _timed(torch, lambda: EV._evaluate_batched(pol, "CrowdSimVarNum-v0", cfg, 425, 500, dev, None, **kw), repeats)
    elif what == "gst":
        from crowdnav_prediction_attngraph_amd.gst import GSTPredictor
        cfg = C.non_randomized(**{"sim.human_num": 20, "sim.predict_method": "inferred"})
        torch.manual_seed(0)
        pred = GSTPredictor().to("cuda")
        pol, envs, dev = _policy(torch, "CrowdSimPredRealGST-v0", cfg, pred)
        res["batched_times_s"], m = _timed(torch, lambda: EV.evaluate_batched(pol, "CrowdSimPredRealGST-v0", cfg, 425, 500, device=dev, predictor=pred), repeats)
        res["batched_metrics"] = m
        t0 = time.perf_counter()
        res["sequential_metrics"] = EV.evaluate(pol, envs, 1, dev, 500, None, cfg, None)
        res["sequential_time_s"] = time.perf_counter() - t0
    elif what == "train_share":
        from crowdnav_prediction_attngraph_amd.trainer import train
        cfg = C.non_randomized(**{"sim.human_num": 20})
        for name, kw in (("without", {}), ("with", {"eval_interval": 1})):
            hist, _ = train("CrowdSimVarNum-v0", num_processes=4096, num_steps=30, num_updates=4, config=cfg, log=None, **kw)
            res[name] = [dict(rollout_s=r["rollout_s"], update_s=r["update_s"], eval_s=r.get("eval_s")) for r in hist]
    print("RESULT " + json.dumps(res))


def child(tree, what, repeats):
    env = dict(os.environ, PYTHONPATH=tree)
    env.pop("CN_HIP_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", what, "--repeats", str(repeats)], cwd=tree, env=env, capture_output=True,
                       text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError("worker %s in %s failed (%d):\n%s" % (what, tree, p.returncode, p.stderr[-3000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def spread(times):
    return dict(median_s=statistics.median(times), min_s=min(times), max_s=max(times), n=len(times), all_s=times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_batched_throughput.json"))
    ap.add_argument("--parent-dir", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--skip", default="", help="comma-separated: gst, bookkeeping, train_share")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.repeats)
    skip = set(a.skip.split(","))
    rec = {"workload": "evaluate_batched, 500 test cases, 20 humans, seeded untrained policy, fused rollout kernels", "rounds": a.rounds, "repeats": a.repeats}
    sides = ([("parent", os.path.abspath(a.parent_dir))] if a.parent_dir else []) + [("branch", ROOT)]
    times = {name: [] for name, _ in sides}
    metrics = {}
    for _ in range(a.rounds):
        for name, tree in sides:             # alternating: both sides see the same box in the same minutes
            r = child(tree, "varnum", a.repeats)
            times[name] += r["times_s"]
            metrics[name] = r["metrics"]
    for name in times:
        rec["varnum_" + name] = spread(times[name])
    rec["varnum_metrics"] = metrics
    if "parent" in times:
        rec["bar"] = dict(rule="median of branch <= slowest repeat of parent", branch_median_s=rec["varnum_branch"]["median_s"],
                          parent_slowest_s=rec["varnum_parent"]["max_s"], met=rec["varnum_branch"]["median_s"] <= rec["varnum_parent"]["max_s"])
    if "bookkeeping" not in skip:
        r = child(ROOT, "bookkeeping", a.repeats)
        rec["bookkeeping"] = {k[:-8]: spread(v) for k, v in r.items() if k.endswith("_times_s")}
    if "gst" not in skip:
        r = child(ROOT, "gst", a.repeats)
        rec["gst"] = dict(batched=spread(r["batched_times_s"]), sequential_time_s=r["sequential_time_s"], batched_metrics=r["batched_metrics"],
                          sequential_metrics=r["sequential_metrics"])
    if "train_share" not in skip:
        rec["train_share_4096_envs"] = child(ROOT, "train_share", 1)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k in ("varnum_parent", "varnum_branch", "bar", "bookkeeping")}, indent=1))


if __name__ == "__main__":
    main()
