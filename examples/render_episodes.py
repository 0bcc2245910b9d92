#!/usr/bin/env python3
"""Watch test cases: run them as evaluate_batched does, draw every state on the MI355X and write the frames to disk.

    python examples/render_episodes.py --checkpoint policy.pt --cases 0 3 137 --out /tmp/episodes      # a policy saved by train_ppo.py --save
    python examples/render_episodes.py --orca --cases 0 3 4 --out /tmp/episodes                        # the ORCA-driven robot, no policy

Writes <out>/case_<k>/<t>.png for every frame and <out>/case_<k>/sheet.png, a contact sheet of up to 16 frames spread over the episode --
as PNG through matplotlib.image.imsave when matplotlib is installed, as .npy arrays otherwise (the package itself never imports matplotlib).
Blue / red outlines: humans the robot sees / does not see; gold: the robot; red diamond: its goal; grey: sensor range; green dots
(CrowdSimPred-v0): predicted positions.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None, help="state_dict of the policy (examples/train_ppo.py --save)")
    ap.add_argument("--orca", action="store_true", help="no policy: robot.policy = 'orca'")
    ap.add_argument("--env-name", default="CrowdSimVarNum-v0")
    ap.add_argument("--humans", type=int, default=20)
    ap.add_argument("--randomized", action="store_true")
    ap.add_argument("--cases", type=int, nargs="+", default=[0])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--seed", type=int, default=425)
    ap.add_argument("--out", default="/tmp/episodes")
    a = ap.parse_args()
    if (a.checkpoint is None) == (not a.orca):
        ap.error("give either --checkpoint FILE or --orca")
    import numpy as np
    import torch
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.evaluation import render_episodes
    from crowdnav_prediction_attngraph_amd.hip import tile_images
    over = {"sim.human_num": a.humans}
    if a.orca:
        over["robot.policy"] = "orca"
    cfg = (C.Config if a.randomized else C.non_randomized)(**over)
    dev = torch.device("cuda", 0)
    pol = None
    if not a.orca:
        from crowdnav_prediction_attngraph_amd.policy import Policy
        from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
        envs = make_vec_envs(a.env_name, a.seed, 1, 0.99, None, dev, True, config=cfg)
        pol = Policy(envs.observation_space.spaces, envs.action_space, base="selfAttn_merge_srnn",
                     base_kwargs=dict(env_name=a.env_name, num_processes=1, num_mini_batch=1, seq_length=30)).to(dev)
        envs.close()
        pol.load_state_dict(torch.load(a.checkpoint, map_location=dev))
    try:
        from matplotlib.image import imsave
        save, ext = (lambda path, img: imsave(path, img)), ".png"
    except ImportError:
        save, ext = (lambda path, img: np.save(path, img)), ".npy"
    names = {1: "timeout", 2: "collision", 3: "reached the goal"}
    for case, ep in sorted(render_episodes(pol, a.env_name, cfg, a.seed, a.cases, size=a.size, device=dev).items()):
        d = os.path.join(a.out, "case_%d" % case)
        os.makedirs(d, exist_ok=True)
        for t, frame in enumerate(ep["frames"]):
            save(os.path.join(d, "%d%s" % (t, ext)), frame)
        pick = np.unique(np.linspace(0, len(ep["frames"]) - 1, 16).round().astype(int))
        save(os.path.join(d, "sheet" + ext), tile_images(ep["frames"][pick]))
        print("case %d: %s after %d steps -> %s (%d frames)" % (case, names[ep["outcome"]], ep["steps"], d, len(ep["frames"])))


if __name__ == "__main__":
    main()
