#!/usr/bin/env python3
"""End to end, the way the reference's pipeline goes (collect_data.py -> gst_updated train.py -> config.pred.model_dir):
simulate crowds on the GPU, write the GST dataset files, train the predictor on them, load the checkpoint back.

    python examples/collect_and_train_gst.py [--envs 256] [--steps 400] [--epochs 5] [--out /tmp/gst_run] [--device-data --batch-size 32] [--predict-steps 5]

--device-data skips the files: the observations stay on the GPU, the sequences are cut out of them there and ALL envs train, in minibatches.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crowdnav_prediction_attngraph_amd import config as C  # noqa: E402
from crowdnav_prediction_attngraph_amd import gst_train  # noqa: E402
from crowdnav_prediction_attngraph_amd.collect import CollectVecEnv, collect_lines, collect_log  # noqa: E402
from crowdnav_prediction_attngraph_amd.gst import GSTPredictor  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--train-files", type=int, default=4, help="how many of the env files the (per-sequence, host-driven) training loop reads")
    ap.add_argument("--device-data", action="store_true", help="cut the sequences out of the observations on the GPU and train on all envs (no files)")
    ap.add_argument("--batch-size", type=int, default=1, help="sequences per optimiser step (train.py's args.batch_size)")
    ap.add_argument("--predict-steps", type=int, default=5, help="the prediction horizon P = pred_seq_len: windows of 5 + P frames, a predictor of P steps (1 .. 8)")
    ap.add_argument("--out", default="/tmp/gst_run")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = C.non_randomized(**{"sim.human_num": 20, "robot.policy": "orca"})
    envs = CollectVecEnv(425, a.envs, dev, config=cfg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if a.device_data:
        log = collect_log(envs, a.steps)
        sets = tuple(gst_train.DeviceTrajectories.from_log(log, mode, pred_seq_len=a.predict_steps) for mode in ("train", "val"))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        envs.close()
        print("collected %d envs x %d steps = %d env-steps and cut %d + %d sequences out of them on the device in %.2f s (%.0f env-steps/s)"
              % (a.envs, a.steps, a.envs * a.steps, len(sets[0]), len(sets[1]), t1 - t0, a.envs * a.steps / (t1 - t0)))
        model, hist = gst_train.train(out_dir=os.path.join(a.out, "run"), dataset=sets, batch_size=a.batch_size, num_epochs=a.epochs, temp_epochs=max(a.epochs, 4),
                                      save_epochs=a.epochs, device=dev, pred_seq_len=a.predict_steps)
        return report(a, dev, hist)
    lines = collect_lines(envs, a.steps)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    envs.close()
    data_dir = os.path.join(a.out, "data")
    os.makedirs(data_dir, exist_ok=True)
    rows = 0
    for i in range(min(a.train_files, a.envs)):
        with open(os.path.join(data_dir, "%d.txt" % i), "w") as f:
            f.write("\n".join(lines[i]) + "\n")
    rows = sum(len(x) for x in lines)
    print("collected %d envs x %d steps = %d env-steps, %d (frame, id, x, y) rows in %.2f s (%.0f env-steps/s incl. the text formatting on the host)"
          % (a.envs, a.steps, a.envs * a.steps, rows, t1 - t0, a.envs * a.steps / (t1 - t0)))
    model, hist = gst_train.train(data_dir, os.path.join(a.out, "run"), num_epochs=a.epochs, temp_epochs=max(a.epochs, 4), save_epochs=a.epochs, device=dev,
                                  batch_size=a.batch_size, pred_seq_len=a.predict_steps)
    report(a, dev, hist)


def report(a, dev, hist):
    ck = os.path.join(a.out, "run", "checkpoint", "epoch_%d.pt" % a.epochs)
    GSTPredictor.from_checkpoint(ck, dev)
    print("val aoe %.4f -> %.4f, val foe %.4f -> %.4f; checkpoint %s" % (hist["val_aoe_task"][0], hist["val_aoe_task"][-1], hist["val_foe_task"][0],
                                                                      hist["val_foe_task"][-1], ck))


if __name__ == "__main__":
    main()
