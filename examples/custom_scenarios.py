#!/usr/bin/env python3
"""Four hand-built situations instead of drawn test cases: a circle crossing of 8 humans with the robot through the centre, two rows walking
head-on across the robot's line, a stationary cluster on the straight line to the goal, and one human overtaking from behind
(crowdnav_prediction_attngraph_amd/scenes.py builds them from closed forms).  The four scenes are the four envs of one batch on the MI355X
(evaluation.evaluate_scenes: reset once, HipEnvBatch.set_scene, each env's first episode); a checkpoint or the scripted ORCA robot drives
them, and every scene gets its trajectory figure.

    python examples/custom_scenarios.py --orca --out /tmp/scenarios                                   # the ORCA-driven robot, no policy
    python examples/custom_scenarios.py --checkpoint policy.pt [--base srnn] --out /tmp/scenarios     # a policy saved by train_ppo.py --save

Writes <out>/<scene>.png (through matplotlib.image.imsave when matplotlib is installed, .npy arrays otherwise) and <out>/traces.npz.  Humans
end_goal_changing is off, so that the humans of the stationary cluster -- standing on their goals -- stay where they were put.  A scene
keeps the radii and speed limits the batch's reset drew (here: fixed attributes, 0.3 m and 1 m/s)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None, help="state_dict of the policy (examples/train_ppo.py --save)")
    ap.add_argument("--base", default="selfAttn_merge_srnn", choices=("selfAttn_merge_srnn", "srnn"))
    ap.add_argument("--orca", action="store_true", help="no policy: robot.policy = 'orca'")
    ap.add_argument("--env-name", default="CrowdSimVarNum-v0")
    ap.add_argument("--humans", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--seed", type=int, default=425)
    ap.add_argument("--out", default="/tmp/scenarios")
    a = ap.parse_args()
    if (a.checkpoint is None) == (not a.orca):
        ap.error("give either --checkpoint FILE or --orca")
    import numpy as np
    import torch
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd import scenes as SC
    from crowdnav_prediction_attngraph_amd.evaluation import evaluate_scenes
    over = {"sim.human_num": a.humans, "humans.end_goal_changing": False}
    if a.orca:
        over["robot.policy"] = "orca"
    cfg = C.non_randomized(**over)
    dev = torch.device("cuda", 0)
    pol = None
    if not a.orca:
        from crowdnav_prediction_attngraph_amd.policy import Policy
        from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
        envs = make_vec_envs(a.env_name, a.seed, 1, 0.99, None, dev, True, config=cfg)
        pol = Policy(envs.observation_space.spaces, envs.action_space, base=a.base,
                     base_kwargs=dict(env_name=a.env_name, num_processes=1, num_mini_batch=1, seq_length=30)).to(dev)
        envs.close()
        pol.load_state_dict(torch.load(a.checkpoint, map_location=dev))
    try:
        from matplotlib.image import imsave
        save, ext = (lambda path, img: imsave(path, img)), ".png"
    except ImportError:
        save, ext = (lambda path, img: np.save(path, img)), ".npy"
    names = list(SC.CATALOGUE)
    humans, robot = SC.stack([SC.CATALOGUE[k](a.humans) for k in names])
    res, tr = evaluate_scenes(pol, a.env_name, cfg, humans, robot, seed=a.seed, traces=True, device=dev)
    images = tr.figure(size=a.size, stride=a.stride)[..., :3].contiguous().cpu().numpy()
    os.makedirs(a.out, exist_ok=True)
    tr.save(os.path.join(a.out, "traces.npz"))
    outcome = {0: "still running", 1: "timeout", 2: "collision", 3: "reached the goal"}
    for e, name in enumerate(names):
        path = os.path.join(a.out, name + ext)
        save(path, images[e])
        print("%s: %s after %d steps, return %.2f, path %.2f m, minimum clearance %.3f m -> %s"
              % (name, outcome[res["outcome"][e]], res["steps"][e], res["ep_return"][e], res["path_length"][e], res["min_clearance"][e], path))


if __name__ == "__main__":
    main()
