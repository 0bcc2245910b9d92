#!/usr/bin/env python3
"""Golden episodes of the reference's own `rl.evaluation.evaluate` on CrowdSimPredRealGST-v0 behind VecPretextNormalize (build container
only; _ref_import.py has the import recipe and the rvo2 caveat):

    python tests/golden/make_golden_eval_gst.py       # rewrites tests/golden/ref_eval_predgst_h8.npz

The env, the wrapper (reset() and process_obs_rew) and the evaluation loop are the reference's; the wrapper object is assembled the way
make_golden_gst.py does it (no args.pickle is loaded) with the SHIPPED predictor weights.  This file's own: the one-env vec-env under the
wrapper (DummyVecEnv + bench.Monitor + VecPyTorch in one: auto-reset, info['episode'], tensors), which also notes what every episode did,
and the stub policy -- a fixed rule on robot_node (towards the goal at min(speed, dist / 0.25)) that records the action it returns and the
wrapped spatial_edges it was shown.  Two runs, speed 1.0 and speed 0.0 (the robot stands still), 8 episodes each with env.test_size = 10:
the case index wraps (cases 0 2 4 6 8 0 2 4).  The file holds data only: actions, observations, per-episode results, the logged metrics."""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import as R  # noqa: E402

R.install()
import torch  # noqa: E402
import make_golden as MG  # noqa: E402
import make_golden_gst as MGG  # noqa: E402

SEED, H, TEST_SIZE, EPISODES = 425, 8, 10, 8
OVER = dict(MG.NON_RAND, **{"sim.human_num": H, "sim.predict_method": "inferred", "env.use_wrapper": True, "env.test_size": TEST_SIZE})


class OneEnvVec(object):
    """What DummyVecEnv([Monitor(env)]) under VecPyTorch gives for one env, plus a log of every episode."""
    num_envs = 1

    def __init__(self, env):
        self.env = env
        self.envs = [self]                       # evaluate() reaches the base env as eval_envs.venv.envs[0].env
        self.observation_space, self.action_space = env.observation_space, env.action_space
        self.episodes, self._cur = [], None

    def _obs(self, ob):
        o = MG.cast_obs(ob, H)
        return {k: torch.from_numpy(np.asarray(v)[None].copy()) for k, v in o.items()}

    def reset(self):
        self._rets = []
        self._cur = dict(steps=0, danger=[], path=0.0)
        obs = self._obs(self.env.reset())
        self._cur["last"] = obs["robot_node"][0, 0, :2].numpy().copy()
        return obs

    def step_async(self, actions):
        self._a = np.asarray(actions.cpu().numpy() if torch.is_tensor(actions) else actions, dtype=np.float32)

    def step_wait(self):
        ob, reward, done, info = self.env.step(self._a[0].copy())
        self._rets.append(reward)
        c = self._cur
        if c is not None:
            c["steps"] += 1
            if MG.info_code(info["info"]) == 4:
                c["danger"].append(float(info["info"].min_dist))
        info = dict(info)
        if done:
            info["episode"] = {"r": round(sum(self._rets), 6), "l": len(self._rets)}
            self._rets = []
            ob = self.env.reset()                # DummyVecEnv's auto-reset: the start of the next case is what comes back
        obs = self._obs(ob)
        if c is not None:
            pos = obs["robot_node"][0, 0, :2].numpy()
            c["path"] += float(np.linalg.norm(pos - c["last"]))
            c["last"] = pos.copy()
            if done:
                c.update(outcome=MG.info_code(info["info"]), reward=info["episode"]["r"])
                self.episodes.append(c)
                self._cur = None
        return obs, torch.from_numpy(np.array([reward], dtype=np.float64)).unsqueeze(1).float(), np.array([done]), [info]

    def talk2Env_async(self, data):
        self._ack = [self.env.talk2Env(data[0])]

    def talk2Env_wait(self):
        return self._ack

    def close(self):
        pass


class RulePolicy(object):
    """`act` = full `speed` towards the goal, slower on the last step; notes (action, wrapped spatial_edges) of every call."""

    class base:
        human_num, human_node_rnn_size, human_human_edge_rnn_size = H, 128, 256

    def __init__(self, speed):
        self.speed, self.actions, self.edges = float(speed), [], []

    def act(self, obs, hxs, masks, deterministic=False):
        rn = obs["robot_node"][0, 0]
        g = rn[3:5] - rn[0:2]
        d = float(torch.linalg.norm(g))
        a = (g / max(d, 1e-9) * min(self.speed, d / 0.25)).to(torch.float32).view(1, 2)
        self.actions.append(a[0].numpy().copy())
        self.edges.append(obs["spatial_edges"][0].numpy().copy())
        return None, a, None, hxs


class Log(object):
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def build_wrapper(cfg, venv):
    from rl.vec_env.vec_pretext_normalize import VecPretextNormalize
    pred, _ = MGG.build_predictor(1, real=True)
    w = VecPretextNormalize.__new__(VecPretextNormalize)
    w.venv, w.config, w.device, w.num_envs, w.max_human_num, w.predictor = venv, cfg, torch.device("cpu"), 1, H, pred
    w.pred_interval = int(cfg.data.pred_timestep // cfg.env.time_step)              # what __init__ derives (:56-57)
    w.buffer_len = 4 * w.pred_interval + 1
    w.observation_space, w.action_space = venv.observation_space, venv.action_space
    # the prediction mask of every call, in the row order of the wrapped observation (the wrapper does not return it)
    w.masks = []
    inner = pred.forward

    def forward(input_traj, input_binary_mask):
        out_traj, out_mask = inner(input_traj=input_traj, input_binary_mask=input_binary_mask)
        w._last_mask = out_mask.bool().reshape(1, H).clone()
        return out_traj, out_mask
    pred.forward = forward
    process = w.process_obs_rew

    def process_obs_rew(O, done, rews=0.):
        order = torch.argsort(torch.linalg.norm(O["spatial_edges"][:, :, :2], dim=-1), dim=1)      # the wrapper's own sort key (:174-175)
        obs, rews = process(O, done, rews=rews)
        w.masks.append(torch.gather(w._last_mask, 1, order)[0].numpy().copy())
        return obs, rews
    w.process_obs_rew = process_obs_rew
    return w


def run(speed):
    from rl.evaluation import evaluate
    cfg = R.make_config(**OVER)
    cfg.args.env_name = "CrowdSimPredRealGST-v0"
    env = MG.make_env("CrowdSimPredRealGST-v0", cfg, SEED, 0, 1)
    assert env.phase == "test"
    venv = OneEnvVec(env)
    w = build_wrapper(cfg, venv)
    pol, log = RulePolicy(speed), Log()
    evaluate(pol, w, 1, torch.device("cpu"), EPISODES, log, cfg, cfg.args)
    eps = venv.episodes
    assert len(eps) == EPISODES and sum(e["steps"] for e in eps) == len(pol.actions)
    # a policy call sees the mask of the observation it is shown: reset() of episode k, then one per step (the last one of an episode, the
    # auto-reset observation, is shown to nobody)
    masks, i = [], 0
    for e in eps:
        masks.extend(w.masks[i:i + e["steps"]])
        i += e["steps"] + 1
    assert i == len(w.masks)
    m = re.match(r"Testing success rate: ([-\d.naninf]+), collision rate: ([-\d.naninf]+), timeout rate: ([-\d.naninf]+), nav time: ([-\d.naninf]+), "
                 r"path length: ([-\d.naninf]+), average intrusion ratio: ([-\d.naninf]+)%, average minimal distance during intrusions: ([-\d.naninf]+)", log.lines[0])
    logged = dict(zip(("success_rate", "collision_rate", "timeout_rate", "nav_time", "path_length", "intrusion_ratio", "min_intrusion_dist"), m.groups()))
    cases = lambda line, head: [int(x) for x in line[len(head):].split()]  # noqa: E731
    logged["collision_cases"] = cases(log.lines[1], "Collision cases: ")
    logged["timeout_cases"] = cases(log.lines[2], "Timeout cases: ")
    return dict(actions=np.array(pol.actions, dtype=np.float32), edges=np.array(pol.edges, dtype=np.float32), masks=np.array(masks, dtype=bool),
                outcome=np.array([e["outcome"] for e in eps]), steps=np.array([e["steps"] for e in eps]), path_length=np.array([e["path"] for e in eps]),
                danger_steps=np.array([len(e["danger"]) for e in eps]), danger_dists=np.array([d for e in eps for d in e["danger"]], dtype=np.float64),
                reward=np.array([e["reward"] for e in eps])), logged


def main():
    out, meta = {}, dict(seed=SEED, human_num=H, test_size=TEST_SIZE, episodes=EPISODES, over=OVER, cases=[(2 * k) % TEST_SIZE for k in range(EPISODES)], runs={})
    outcomes, danger = [], 0
    for tag, speed in (("fast", 1.0), ("still", 0.0)):
        rec, logged = run(speed)
        for k, v in rec.items():
            out["%s_%s" % (tag, k)] = v
        meta["runs"][tag] = dict(speed=speed, logged=logged)
        outcomes += rec["outcome"].tolist()
        danger += int(rec["danger_steps"].sum())
        # a repeated case is the same episode again (the wrapper starts every episode from its dummy history)
        for k in range(TEST_SIZE // 2, EPISODES):
            j = k - TEST_SIZE // 2
            assert rec["outcome"][k] == rec["outcome"][j] and rec["steps"][k] == rec["steps"][j] and rec["path_length"][k] == rec["path_length"][j]
        print(tag, "outcomes", rec["outcome"].tolist(), "steps", rec["steps"].tolist(), "danger", rec["danger_steps"].tolist(), logged)
    assert 3 in outcomes and 2 in outcomes and 1 in outcomes and danger > 0, "the fixture must hold a success, a collision, a timeout and a Danger step"
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "ref_eval_predgst_h8.npz")
    np.savez_compressed(path, **out)
    print("-> %s (%.0f KB)" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
