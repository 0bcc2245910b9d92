#!/usr/bin/env python3
"""Cost of the GST predictor's training stage with the data on the device against the file-based path, on the GPU.

    python tools/gst_train_throughput.py --out profiles/gst_train_epoch.json

Protocol of tools/gst_throughput.py: one process, the variants of a group alternate, a warm-up first, median / minimum / maximum over --repeats
timed windows; a window is wall clock around work that ends in torch.cuda.synchronize() or in a read-back.
  (a) build:  the dataset of --envs collect envs x --samples observations (20 humans).  'files': collect_lines + one text file per env +
              TrajectoriesDataset over the directory; 'device': collect_log + DeviceTrajectories.from_log.  The simulation is common to both and
              also timed alone ('simulate': collect_log), so is the part after it ('files_after_sim' from the lines, 'device_after_sim' from the log).
  (b) epoch:  gst_train.train(backend='hip'), the logged period of the epochs after the first, as training sequences per second (the period
              includes the epoch's validation pass).  'files_B1': today's per-item loop on the files; 'device_B<n>': train(dataset=...) at batch
              sizes 1, 8 and 32.  The per-item loop and B = 1 take ~7 ms per sequence, so they run on the first --slow-envs envs; B = 8 and 32
              on the first --fast-envs.  Rates are per sequence, the env counts are recorded.
  (c) for information: validation loss / aoe / foe after --epochs epochs at B = 1 and B = 32 on the same --slow-envs envs and seed.
"""
import argparse
import json
import os
import re
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--samples", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--slow-envs", type=int, default=2)
    ap.add_argument("--fast-envs", type=int, default=16)
    a = ap.parse_args()
    import torch

    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd import gst_train as T
    from crowdnav_prediction_attngraph_amd.collect import CollectVecEnv, collect_lines, collect_log

    assert torch.cuda.is_available(), "gst_train_throughput.py measures the GPU paths"
    dev = torch.device("cuda", 0)
    cfg = C.non_randomized(**{"sim.human_num": 20, "robot.policy": "orca"})
    tmp = tempfile.mkdtemp()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def with_envs(fn):
        envs = CollectVecEnv(425, a.envs, dev, config=cfg)
        try:
            return timed(lambda: fn(envs))
        finally:
            envs.close()

    def write_files(lines, d, n):
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
        for i in range(n):
            with open(os.path.join(d, "%d.txt" % i), "w") as f:
                f.write("\n".join(lines[i]) + "\n")
        return d

    def stats(v, key="s"):
        return {key + "_median": statistics.median(v), key + "_min": min(v), key + "_max": max(v), "windows": v}

    out = {"device": torch.cuda.get_device_name(0), "envs": a.envs, "samples": a.samples, "humans": 20, "repeats": a.repeats, "epochs": a.epochs}
    # (a) the dataset build
    build = {k: [] for k in ("files", "device", "simulate", "files_after_sim", "device_after_sim")}
    lines = log = None
    for rep in range(a.repeats + 1):                        # the first round is the warm-up
        t_lines, lines = with_envs(lambda e: collect_lines(e, a.samples))
        t_files, ds_files = timed(lambda: T.TrajectoriesDataset(write_files(lines, os.path.join(tmp, "all"), a.envs)))
        t_log, log = with_envs(lambda e: collect_log(e, a.samples))
        t_dev, ds_dev = timed(lambda: T.DeviceTrajectories.from_log(log))
        if rep:
            for k, v in (("files", t_lines + t_files), ("device", t_log + t_dev), ("simulate", t_log), ("files_after_sim", t_lines - t_log + t_files), ("device_after_sim", t_dev)):
                build[k].append(v)
    assert len(ds_files) == len(ds_dev)
    out["build"] = dict({k: stats(v) for k, v in build.items()}, sequences=len(ds_dev), pedestrian_rows=ds_dev.total_peds)
    out["build"]["files_over_device"] = statistics.median(build["files"]) / statistics.median(build["device"])
    out["build"]["files_over_device_after_sim"] = statistics.median(build["files_after_sim"]) / statistics.median(build["device_after_sim"])
    del ds_files, ds_dev

    # (b) the epoch
    def split(n):
        ids = list(range(n))
        return T.DeviceTrajectories.from_log(log, "train", ids), T.DeviceTrajectories.from_log(log, "val", ids)

    slow_dir = write_files(lines, os.path.join(tmp, "slow"), a.slow_envs)
    sets = {"slow": split(a.slow_envs), "fast": split(a.fast_envs)}
    kw = dict(num_epochs=a.epochs, temp_epochs=max(a.epochs, 4), save_epochs=1000, device=dev, backend="hip", random_seed=1000)
    variants = {"files_B1": ("slow", 1, dict(data_dir=slow_dir)), "device_B1": ("slow", 1, dict(dataset=sets["slow"])),
                "device_B8": ("fast", 8, dict(dataset=sets["fast"])), "device_B32": ("fast", 32, dict(dataset=sets["fast"]))}
    rates, hists = {k: [] for k in variants}, {}
    for rep in range(a.repeats):
        for name, (which, B, src) in variants.items():
            logged = []
            _, hist = T.train(out_dir=tempfile.mkdtemp(dir=tmp), log=logged.append, batch_size=B, **dict(kw, **src))
            periods = [float(re.search(r"period: ([0-9.]+) sec", ln).group(1)) for ln in logged[1:]]
            rates[name] += [len(sets[which][0]) / p for p in periods]
            hists[name] = hist
    out["epoch"] = {k: dict(stats(v, "train_seq_per_s"), envs=a.slow_envs if variants[k][0] == "slow" else a.fast_envs, batch_size=variants[k][1],
                            train_sequences=len(sets[variants[k][0]][0]), validation_sequences=len(sets[variants[k][0]][1])) for k, v in rates.items()}
    med = lambda k: out["epoch"][k]["train_seq_per_s_median"]   # noqa: E731
    out["ratios"] = {k + "_over_files_B1": med(k) / med("files_B1") for k in ("device_B1", "device_B8", "device_B32")}
    # (c) for information: where the validation ends after the same number of epochs, same envs, same seed
    _, hist32 = T.train(out_dir=tempfile.mkdtemp(dir=tmp), log=lambda s: None, batch_size=32, dataset=sets["slow"], **kw)
    out["validation_after_epochs"] = {name: {m: h["val_%s_task" % m][-1] for m in ("loss", "aoe", "foe")}
                                      for name, h in (("files_B1", hists["files_B1"]), ("device_B1", hists["device_B1"]), ("device_B32", hist32))}
    shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
