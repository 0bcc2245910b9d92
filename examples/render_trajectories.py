#!/usr/bin/env python3
"""One picture per test case: run the cases as evaluate_batched does, record every state on the MI355X, draw each episode as a trajectory
figure and print what the record measures (the reference's test.py --render_traj, which it announces and never draws).

    python examples/render_trajectories.py --checkpoint policy.pt --cases 0 3 137 --out /tmp/trajectories      # a policy saved by train_ppo.py --save
    python examples/render_trajectories.py --orca --cases 0 3 4 --out /tmp/trajectories                        # the ORCA-driven robot, no policy

Writes <out>/case_<k>.png -- as PNG through matplotlib.image.imsave when matplotlib is installed, as .npy arrays otherwise (the package itself
never imports matplotlib) -- and <out>/traces.npz (EpisodeTraces.save: the record itself, to be measured or re-drawn later at another size).
Every record leaves a small disc per agent, light at the start of the episode and dark at its end: blue / red humans the robot sees / does
not see, orange the robot; every --stride-th record and the last one also show the agent's outline, the robot's last record its full disc;
red diamond: the goal.  A record is the state a step was taken FROM: the state after the final step (the collision or the arrival itself) is
not in it -- the simulator replaces it with the next episode's start inside the step.
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
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--seed", type=int, default=425)
    ap.add_argument("--out", default="/tmp/trajectories")
    a = ap.parse_args()
    if (a.checkpoint is None) == (not a.orca):
        ap.error("give either --checkpoint FILE or --orca")
    import numpy as np
    import torch
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.evaluation import record_episodes
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
    tr = record_episodes(pol, a.env_name, cfg, a.seed, a.cases, device=dev)
    images = tr.figure(size=a.size, stride=a.stride)[..., :3].contiguous().cpu().numpy()
    m = tr.metrics()
    os.makedirs(a.out, exist_ok=True)
    tr.save(os.path.join(a.out, "traces.npz"))
    for e, case in enumerate(tr.cases):
        path = os.path.join(a.out, "case_%d%s" % (case, ext))
        save(path, images[e])
        print("case %d: %s after %d steps -> %s" % (case, names[tr.outcome[e]], tr.steps[e], path))
        print("    path %.3f m, mean speed %.3f m/s, mean acceleration %.3f m/s^2, minimum clearance %.3f m, %d of %d records inside a comfort "
              "zone (%d by a human the robot saw), %.1f humans on average"
              % (m["path_length"][e], m["mean_speed"][e], m["mean_accel"][e], m["min_clearance"][e], m["intrusion_steps"][e], m["records"][e],
                 m["visible_intrusion_steps"][e], m["mean_crowd"][e]))


if __name__ == "__main__":
    main()
