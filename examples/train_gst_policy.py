#!/usr/bin/env python3
"""The reference's whole pipeline for its GST-predictor policy on one MI355X: collect crowd trajectories -> train the trajectory predictor
on them (or load one from --model-dir) -> PPO on CrowdSimPredRealGST-v0 with that predictor in the loop (VecPretextNormalize processing),
evaluating on the seeded test cases every --eval-interval updates -> the final 500-case line.

    python examples/train_gst_policy.py [--model-dir DIR] [--envs 512] [--updates 400] [--lr 4e-5] [--eval-interval 100] [--out /tmp/gst_policy]
                                        [--device-data --batch-size 32]

--device-data keeps the collected observations on the GPU and trains the predictor on ALL collect envs in minibatches (no files).
"""
import argparse
import logging
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crowdnav_prediction_attngraph_amd import config as C  # noqa: E402
from crowdnav_prediction_attngraph_amd import gst_train  # noqa: E402
from crowdnav_prediction_attngraph_amd.collect import CollectVecEnv, collect_lines, collect_log  # noqa: E402
from crowdnav_prediction_attngraph_amd.gst import GSTPredictor, find_checkpoint  # noqa: E402
from crowdnav_prediction_attngraph_amd.trainer import train  # noqa: E402

ENV = "CrowdSimPredRealGST-v0"


def fresh_predictor(a, dev):
    """collect_data.py -> gst_updated train.py, as examples/collect_and_train_gst.py does it."""
    envs = CollectVecEnv(a.seed, a.collect_envs, dev, config=C.non_randomized(**{"sim.human_num": 20, "robot.policy": "orca"}))
    run = os.path.join(a.out, "predictor")
    if a.device_data:
        log = collect_log(envs, a.collect_steps)
        envs.close()
        sets = tuple(gst_train.DeviceTrajectories.from_log(log, mode, pred_seq_len=a.predict_steps) for mode in ("train", "val"))
        _, hist = gst_train.train(out_dir=run, dataset=sets, batch_size=a.batch_size, num_epochs=a.epochs, temp_epochs=max(a.epochs, 4), save_epochs=a.epochs, device=dev,
                                  pred_seq_len=a.predict_steps)
        print("predictor (%d + %d sequences of %d envs, batches of %d): val aoe %.4f -> %.4f, val foe %.4f -> %.4f" % (
            len(sets[0]), len(sets[1]), a.collect_envs, a.batch_size, hist["val_aoe_task"][0], hist["val_aoe_task"][-1], hist["val_foe_task"][0], hist["val_foe_task"][-1]), flush=True)
        return run
    lines = collect_lines(envs, a.collect_steps)
    envs.close()
    data_dir = os.path.join(a.out, "data")
    os.makedirs(data_dir, exist_ok=True)
    for i in range(min(a.train_files, a.collect_envs)):
        with open(os.path.join(data_dir, "%d.txt" % i), "w") as f:
            f.write("\n".join(lines[i]) + "\n")
    _, hist = gst_train.train(data_dir, run, num_epochs=a.epochs, temp_epochs=max(a.epochs, 4), save_epochs=a.epochs, device=dev, batch_size=a.batch_size,
                              pred_seq_len=a.predict_steps)
    print("predictor: val aoe %.4f -> %.4f, val foe %.4f -> %.4f" % (hist["val_aoe_task"][0], hist["val_aoe_task"][-1], hist["val_foe_task"][0],
                                                                   hist["val_foe_task"][-1]), flush=True)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=None, help="a gst_updated/results/.../sj style directory or the out_dir of gst_train.train; default: train one")
    ap.add_argument("--collect-envs", type=int, default=256)
    ap.add_argument("--collect-steps", type=int, default=400)
    ap.add_argument("--train-files", type=int, default=4)
    ap.add_argument("--device-data", action="store_true", help="cut the sequences out of the observations on the GPU and train on all collect envs (no files)")
    ap.add_argument("--batch-size", type=int, default=1, help="sequences per optimiser step (train.py's args.batch_size)")
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--updates", type=int, default=400)
    ap.add_argument("--lr", type=float, default=4e-5)
    ap.add_argument("--eval-interval", type=int, default=100)
    ap.add_argument("--eval-cases", type=int, default=500)
    ap.add_argument("--seed", type=int, default=425)
    ap.add_argument("--predict-steps", type=int, default=5, help="the prediction horizon P = sim.predict_steps = the predictor's pred_seq_len (1 .. 7 with this policy; "
                    "a --model-dir must hold a predictor of that horizon)")
    ap.add_argument("--out", default="/tmp/gst_policy")
    a = ap.parse_args()
    logging.basicConfig(level=logging.INFO, stream=sys.stdout)
    dev = torch.device("cuda", 0)
    t0 = time.time()
    model_dir = a.model_dir or fresh_predictor(a, dev)
    pred = GSTPredictor.from_checkpoint(find_checkpoint(model_dir), dev)
    t1 = time.time()
    cfg = C.non_randomized(**{"sim.human_num": 20, "sim.predict_method": "inferred", "sim.predict_steps": a.predict_steps, "env.use_wrapper": True, "pred.model_dir": model_dir})
    every = max(a.updates // 12, 1)
    acc = []

    def log(r):
        acc.append(r)
        if (r["update"] + 1) % every == 0:
            w = acc[-every:]
            ep = sum(x["episodes"] for x in w) or 1
            print("update %4d  steps %.1fM  eprewmean %7.2f  success %.2f collision %.2f timeout %.2f  entropy %.3f  (%.0f s)" % (
                r["update"] + 1, (r["update"] + 1) * 30 * a.envs / 1e6, sum(x["eprewmean"] * x["episodes"] for x in w) / ep,
                sum(x["success"] * x["episodes"] for x in w) / ep, sum(x["collision"] * x["episodes"] for x in w) / ep,
                sum(x["timeout"] * x["episodes"] for x in w) / ep, r["entropy"], time.time() - t1), flush=True)
        if "eval" in r:
            print("  test after update %d (%.2f s): %s" % (r["update"] + 1, r["eval_s"], {k: v for k, v in r["eval"].items() if "cases" not in k}), flush=True)
    # pretext_wrapper follows cfg.env.use_wrapper; the predictor object is handed over so that training and evaluation share one copy
    hist, pol = train(ENV, a.envs, 30, a.updates, a.seed, config=cfg, lr=a.lr, log=log, predictor=pred, eval_interval=a.eval_interval or a.updates, eval_cases=a.eval_cases)
    t2 = time.time()
    print("predictor %.1f s, policy training %.1f s for %.1f M env steps (of which %.1f s in %d evaluations)"
          % (t1 - t0, t2 - t1, a.updates * 30 * a.envs / 1e6, sum(r.get("eval_s", 0.0) for r in hist), sum("eval" in r for r in hist)))
    m = hist[-1]["eval"]
    print("final %d-case test: %s" % (a.eval_cases, {k: v for k, v in m.items() if "cases" not in k}))


if __name__ == "__main__":
    main()
