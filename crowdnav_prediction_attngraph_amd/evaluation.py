"""Deterministic evaluation (drop-in for rl/evaluation.py:7-160) on the batched device simulator.

`evaluate` keeps the reference's argument list and its sequential semantics (one env, `test_size` episodes, a
`reset()` per episode on top of the vec-env's own auto-reset -- so consecutive episodes use every SECOND test case and the
case index wraps at `test_size`; the robot-path length includes the jump to the auto-reset start position; nav time is the
env time before the final step).  `evaluate_batched` produces the same numbers by running every distinct test case as one
env of a single batch (first episode of each env), which is how the device simulator wants to be driven.
Both return the metrics as a dict (the reference only logs them).
"""
import numpy as np
import torch

from . import info as I
from .config import to_env_config


def _summarise(outcomes, steps, path_len, too_close, min_dists, ep_rewards, time_limit, time_step, logging, danger_sums=None):
    """min_dists: the Danger distances of all episodes as one flat list, or None with danger_sums = their sum per episode (too_close = count)."""
    test_size = len(outcomes)
    if min_dists is None:
        n_close = sum(too_close)
        min_intrusion = float(sum(danger_sums) / n_close) if n_close else float("nan")
    else:
        min_intrusion = float(np.mean(min_dists)) if len(min_dists) else float("nan")
    success = [k for k, o in enumerate(outcomes) if o == 3]
    collision = [k for k, o in enumerate(outcomes) if o == 2]
    timeout = [k for k, o in enumerate(outcomes) if o == 1]
    assert len(success) + len(collision) + len(timeout) == test_size
    success_times = [(steps[k] - 1) * time_step for k in success]      # env.global_time read before the final step (:75-76)
    m = dict(success_rate=len(success) / test_size, collision_rate=len(collision) / test_size, timeout_rate=len(timeout) / test_size,
             nav_time=sum(success_times) / len(success_times) if success_times else time_limit,
             path_length=float(np.mean(path_len)), intrusion_ratio=float(np.mean([100.0 * c / s for c, s in zip(too_close, steps)])),
             min_intrusion_dist=min_intrusion,
             collision_cases=collision, timeout_cases=timeout, mean_reward=float(np.mean(ep_rewards)), episodes=test_size)
    if logging is not None:
        logging.info('Testing success rate: {:.2f}, collision rate: {:.2f}, timeout rate: {:.2f}, '
                     'nav time: {:.2f}, path length: {:.2f}, average intrusion ratio: {:.2f}%, '
                     'average minimal distance during intrusions: {:.2f}'.format(m["success_rate"], m["collision_rate"], m["timeout_rate"],
                                                                                  m["nav_time"], m["path_length"], m["intrusion_ratio"],
                                                                                  m["min_intrusion_dist"]))
        logging.info('Collision cases: ' + ' '.join(str(x) for x in collision))
        logging.info('Timeout cases: ' + ' '.join(str(x) for x in timeout))
    return m


class _batch_invariant(object):
    """batch_invariant=True: run the policy with the launches whose per-env results do not depend on which other envs share the batch
    ('bf16x3': the same arithmetic as separate launches), so that one-env-at-a-time and all-cases-in-one-batch evaluation give
    bit-identical episodes.  Default (False): the policy's own rollout mode -- 'fused' unless the caller changed it, i.e. exactly the
    arithmetic training and bench.py run; its per-env results depend on the tile neighbours at the 1e-7 level (softmax summation order)."""

    def __init__(self, actor_critic, on):
        self.ac = actor_critic if on else None

    def __enter__(self):
        if self.ac is not None and hasattr(self.ac, "rollout_gemm_mode"):
            self.saved = self.ac.rollout_gemm_mode
            self.ac.rollout_gemm_mode = "bf16x3"
        return self

    def __exit__(self, *exc):
        if self.ac is not None and hasattr(self.ac, "rollout_gemm_mode"):
            self.ac.rollout_gemm_mode = self.saved
        return False


def evaluate(actor_critic, eval_envs, num_processes, device, test_size, logging, config, args, visualize=False, *, batch_invariant=False):
    """Same call as the reference's `evaluate`.  eval_envs = make_vec_envs(..., num_processes=1, ...) (phase 'test').  The policy runs in its
    own rollout mode (the benchmarked fused kernels) unless batch_invariant=True is passed (see _batch_invariant)."""
    with _batch_invariant(actor_critic, batch_invariant):
        return _evaluate(actor_critic, eval_envs, num_processes, device, test_size, logging, config, args, visualize)


def _evaluate(actor_critic, eval_envs, num_processes, device, test_size, logging, config, args, visualize=False):
    if num_processes != 1 or eval_envs.num_envs != 1:
        raise NotImplementedError("the reference evaluates with ONE env (test.py:136); use evaluate_batched for the parallel form")
    if visualize:
        # rl/evaluation.py:84-85 draws every step.  Rendering is out of scope here, but the reference's test.py cannot switch it off (its
        # --visualize flag is `default=True, action='store_true'`, test.py:25), so the request is acknowledged instead of refused: the
        # episodes run, nothing is drawn, the metrics are the same.
        import warnings
        warnings.warn("evaluate(visualize=True): rendering is not implemented on the accelerated path; running the episodes without drawing")
    scripted = actor_critic is None          # robot.policy in ('orca', ...): the env drives the robot itself (test.py:152-153)
    if scripted and int(eval_envs.cfg.robot_policy) == 0:
        raise ValueError("actor_critic is None but the env was not configured with robot.policy = 'orca'")
    if not scripted:
        base = actor_critic.base
        hxs = {"human_node_rnn": torch.zeros(1, 1, base.human_node_rnn_size, device=device),
               "human_human_edge_rnn": torch.zeros(1, base.human_num + 1, base.human_human_edge_rnn_size, device=device)}
    masks = torch.zeros(1, 1, device=device)
    time_limit, time_step = float(eval_envs.cfg.time_limit), float(eval_envs.cfg.time_step)
    outcomes, steps, path_lens, too_closes, min_dists, ep_rewards = [], [], [], [], [], []
    for _ in range(test_size):
        obs = eval_envs.reset()
        done, n, too_close, path_len = False, 0, 0, 0.0
        last_pos = obs["robot_node"][0, 0, :2].cpu().numpy()
        while not done:
            n += 1
            if scripted:
                action = torch.zeros(1, 2, device=device)                       # rl/evaluation.py:73-74
            else:
                with torch.no_grad():
                    _, action, _, hxs = actor_critic.act(obs, hxs, masks, deterministic=True)
            obs, rew, dones, infos = eval_envs.step(action)
            pos = obs["robot_node"][0, 0, :2].cpu().numpy()
            path_len += float(np.linalg.norm(pos - last_pos))
            last_pos = pos
            if isinstance(infos[0]["info"], I.Danger):
                too_close += 1
                min_dists.append(infos[0]["info"].min_dist)
            done = bool(dones[0])
            masks = torch.tensor([[0.0] if done else [1.0]], dtype=torch.float32, device=device)
            if "episode" in infos[0]:
                ep_rewards.append(infos[0]["episode"]["r"])
        code = {I.Timeout: 1, I.Collision: 2, I.ReachGoal: 3}.get(type(infos[0]["info"]))
        if code is None:
            raise ValueError("Invalid end signal from environment")
        outcomes.append(code); steps.append(n); path_lens.append(path_len); too_closes.append(too_close)
    eval_envs.close()
    return _summarise(outcomes, steps, path_lens, too_closes, min_dists, ep_rewards, time_limit, time_step, logging)


class EvalAccumulator(object):
    """The bookkeeping of the evaluation protocol for the first episode of each of E envs, fed with the step outputs of HipEnvBatch as they are.
    The state is ONE int64 buffer laid out as include/crowdnav_hip.h describes (CN_EVAL_*): on the GPU an update is one launch of
    cn_eval_accumulate and nothing is read back until `n_active()` / `results()`; the torch-op form below works on the same buffer -- it is
    what CPU tensors use and the cross-check of the kernel (use_kernel=False on the GPU)."""
    HEADER, FIELDS = 8, 8
    ACTIVE, STEPS, DANGER_STEPS, OUTCOME, DANGER_SUM, PATH_LENGTH, RETURN, LAST_POS = range(8)

    def __init__(self, num_envs, device, use_kernel=None):
        self.E, self.device = int(num_envs), torch.device(device)
        self.use_kernel = (self.device.type == "cuda") if use_kernel is None else bool(use_kernel)
        self.state = torch.zeros(self.HEADER + self.FIELDS * self.E, dtype=torch.int64, device=self.device)
        f = self.state[self.HEADER:].view(self.FIELDS, self.E)
        self.active, self.steps, self.danger_steps, self.outcome = f[self.ACTIVE], f[self.STEPS], f[self.DANGER_STEPS], f[self.OUTCOME]
        self.danger_sum, self.path_length, self.ep_return = (f[k].view(torch.float64) for k in (self.DANGER_SUM, self.PATH_LENGTH, self.RETURN))
        self.last_pos = f[self.LAST_POS].view(torch.float32).view(self.E, 2)
        self.masks = torch.zeros(self.E, 1, device=self.device)

    def start(self, robot_node):
        """robot_node: the [E,1,7] rows of the reset observation."""
        self.state.zero_()
        self.active.fill_(1)
        self.state[0] = self.E
        self.last_pos.copy_(robot_node.reshape(self.E, 7)[:, :2])
        self.masks.zero_()

    def update(self, done, info, ep_return, robot_node, danger_dist):
        """One vec-env step.  Returns the masks of the next forward (done == 0 as float32 [E,1])."""
        E = self.E
        if self.use_kernel:
            from . import _abi as A
            if (done.dtype != torch.uint8 or info.dtype != torch.uint8 or ep_return.dtype != torch.float64 or robot_node.dtype != torch.float32
                    or danger_dist.dtype != torch.float64 or done.numel() != E or info.numel() != E or ep_return.numel() != E
                    or robot_node.numel() != 7 * E or danger_dist.numel() != E):
                raise A.CnError("EvalAccumulator.update: done / info u8 [E], ep_return / danger_dist f64 [E], robot_node f32 [E,1,7] expected (E = %d)" % E)
            A.call("cn_eval_accumulate", E, A.ptr(done), A.ptr(info), A.ptr(ep_return), A.ptr(robot_node), A.ptr(danger_dist), A.ptr(self.state),
                   A.ptr(self.masks), A.stream_ptr(), device=self.device)
            return self.masks
        act = self.active != 0
        pos = robot_node.reshape(E, 7)[:, :2]
        # the reference measures the path on the float32 observation tensors, episode-end jump to the auto-reset start included
        self.path_length += torch.where(act, torch.linalg.norm((pos - self.last_pos).float(), dim=1).double(), torch.zeros_like(self.path_length))
        self.last_pos.copy_(torch.where(act.unsqueeze(1), pos, self.last_pos))
        self.steps += act.long()
        danger = act & (info == 4)
        self.danger_steps += danger.long()
        self.danger_sum += torch.where(danger, danger_dist, torch.zeros_like(danger_dist))
        fin = act & (done != 0)
        self.outcome.copy_(torch.where(fin, info.long(), self.outcome))
        self.ep_return.copy_(torch.where(fin, ep_return, self.ep_return))
        self.active.copy_((act & ~fin).long())
        self.state[0] = self.active.sum()
        self.masks.copy_((done == 0).float().view(E, 1))
        return self.masks

    def n_active(self):
        """Envs whose first episode is still running (one host synchronisation)."""
        return int(self.state[0].item())

    def results(self):
        """dict of per-env host lists: outcome, steps, danger_steps, danger_sum, path_length, ep_return."""
        h = self.state.cpu()[self.HEADER:].view(self.FIELDS, self.E)
        return dict(outcome=h[self.OUTCOME].tolist(), steps=h[self.STEPS].tolist(), danger_steps=h[self.DANGER_STEPS].tolist(),
                    danger_sum=h[self.DANGER_SUM].view(torch.float64).tolist(), path_length=h[self.PATH_LENGTH].view(torch.float64).tolist(),
                    ep_return=h[self.RETURN].view(torch.float64).tolist())


def evaluate_batched(actor_critic, env_name, config, seed, test_size, device=None, logging=None, *, batch_invariant=False, predictor=None,
                     traces=False):
    """The same protocol with every distinct test case as one env of one batch (all tensors stay on the GPU).  batch_invariant=True on both
    this and evaluate() makes the two report bit-identical episodes (tests/test_gpu_eval.py); by default both run the fused kernels and
    agree to the policy's 1e-7-level sensitivity to its tile neighbours (which can flip a chaotic episode's outcome).
    CrowdSimPredRealGST-v0 runs behind the VecPretextNormalize processing (gst.PretextProcessor over the batch): predictor = a
    gst.GSTPredictor, or None to load config.pred.model_dir.
    traces=True: every episode is also recorded on the device (one more launch per step, see record_episodes) and the call returns
    (summary, EpisodeTraces); the summary is the one traces=False gives, bit for bit."""
    with _batch_invariant(actor_critic, batch_invariant):
        if not traces:
            return _evaluate_batched(actor_critic, env_name, config, seed, test_size, device, logging, predictor=predictor)
        rec = _TraceRecorder(config, env_name)
        summary = _evaluate_batched(actor_critic, env_name, config, seed, test_size, device, logging, predictor=predictor, per_env=rec.per_env,
                                    pre_step_fn=rec)
        return summary, rec.finish()


def _evaluate_batched(actor_critic, env_name, config, seed, test_size, device=None, logging=None, predictor=None, poll_every=16, act_fn=None,
                      hip_policy=None, use_kernel=True, per_env=None, frame_fn=None, pre_step_fn=None, scenes=None, max_steps=None):
    """test_size: the episode count of the sequential protocol (episode k runs case 2 k mod the config's test_size), or a sequence of case
    numbers to run instead (render_episodes).  poll_every: the count of running episodes is read back (the loop's only host synchronisation)
    every that many steps; steps taken after the last episode ended change nothing.  act_fn(t, obs) -> actions [E,2] replaces the policy forward (tests replay recorded actions);
    hip_policy: a policy handle (base.make_hip_handle) to run instead of actor_critic's own (train() evaluates through a second handle so that the training
    rollout finds its handle as it left it); use_kernel=False: the torch-op bookkeeping; per_env: a dict that receives the per-env results;
    frame_fn(t, env, obs): called once after the reset (t = 0) and once after every step (t = steps taken) with the HipEnvBatch and the
    observation it returned, e.g. to draw the state (render_episodes); it must leave both as they are.  pre_step_fn(t, env, acc): called
    immediately BEFORE step t is taken with the HipEnvBatch and the accumulator, whose `active` / `steps` arrays then say which envs' first
    episode is still running and how many steps it has taken -- the moment to record the state a step is taken from (record_episodes;
    after the step the env of a finished episode already holds its next episode's start); it must leave both as they are.
    scenes=(humans [n,H,8], robot [n,8]) (evaluate_scenes): n envs, reset once and then started from these states (HipEnvBatch.set_scene)
    instead of n test cases; test_size is ignored, per_env["cases"] is range(n), an episode still running after max_steps steps is reported
    with outcome 0 instead of raising, and the return value is None.  max_steps: the step bound (default: round(time_limit / time_step) + 1)."""
    from .hip_env import HipEnvBatch
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    cfg = to_env_config(config, env_name, 1, "test")          # nenv = 1: case counters advance by one, as in the sequential run
    scripted = actor_critic is None and act_fn is None
    if scripted and int(cfg.robot_policy) == 0:
        raise ValueError("actor_critic is None but config.robot.policy is not 'orca'")
    if int(cfg.robot_policy) == 1 and int(cfg.randomize_attributes):
        raise NotImplementedError("an ORCA robot with randomised humans keeps ONE rvo2 simulator (radii / neighbour distance frozen in the "
                                  "first episode) across the whole sequential run; use evaluate() for that configuration"
                                  + ("" if scenes is None else " (scenes: not covered either -- run the ORCA robot on scenes with env.randomize_attributes off)"))
    case_size = int(cfg.test_size)
    if scenes is not None:
        case_of = list(range(int(scenes[0].shape[0])))
        test_size = len(case_of)
    elif isinstance(test_size, (list, tuple)):
        case_of, test_size = [int(c) for c in test_size], len(test_size)
    else:
        case_of = [(2 * k) % case_size for k in range(test_size)]  # reset() + the vec-env's auto-reset: two resets per episode
    cases = sorted(set(case_of))
    E = len(cases)
    env = HipEnvBatch(cfg, E, int(seed), device=device)
    # env e draws seed offset + counter[e] + (seed + e): counter[e] = case - e  (cases are distinct and sorted, so case >= e)
    if scenes is None:
        env.set_case_counters(torch.tensor([c - e for e, c in enumerate(cases)], dtype=torch.int64))
    pretext = None
    if env_name == "CrowdSimPredRealGST-v0":
        # VecPretextNormalize over the batch: GST predictions into spatial_edges[:, :, 2:], rows sorted by distance.  Every episode evaluated
        # here is the first one after the wrapper's reset(), i.e. starts from the dummy history, as every episode of the sequential run does
        from .gst import PretextProcessor, load_predictor
        pred = predictor if predictor is not None else load_predictor(config, device)
        data = getattr(config, "data", None)
        interval = int(float(getattr(data, "pred_timestep", cfg.time_step)) // float(cfg.time_step))   # as BatchedCrowdSim.__init__
        pretext = PretextProcessor(pred.to(device), E, env.H, int(cfg.predict_steps), float(cfg.robot_radius), float(cfg.human_radius),
                                   float(cfg.collision_penalty), device, pred_interval=interval)
        zero_reward = torch.zeros(E, device=device)
    obs = env.reset()
    if scenes is not None:
        obs = env.set_scene(*_scene_tensors(env, scenes[0], scenes[1]))
    if frame_fn is not None:
        frame_fn(0, env, obs)
    pol = None
    if act_fn is None and not scripted:
        pol = hip_policy if hip_policy is not None else actor_critic._hip_handle(E, device)
        # the state the handle carries ping-pongs between two buffers
        hxs = [{k: torch.zeros(shape, device=device) for k, shape in pol.state_shapes(E).items()} for _ in (0, 1)]
    zero_action = torch.zeros(E, 2, device=device)
    acc = EvalAccumulator(E, device, use_kernel=use_kernel)
    acc.start(obs["robot_node"])
    masks = acc.masks
    danger_dist = torch.zeros(E, dtype=torch.float64, device=device)
    if max_steps is None:
        max_steps = int(round(float(cfg.time_limit) / float(cfg.time_step))) + 1
    poll_every = max(1, int(poll_every))
    for t in range(max_steps):
        if scripted:
            action = zero_action
        else:
            pobs = {k: obs[k] for k in ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num")}
            if pretext is not None:
                # the social penalty lands in the env's own reward buffer, as in BatchedCrowdSim.step_device: no metric reads it (the episode
                # reward is the Monitor's sum of the raw reward)
                pobs["spatial_edges"], _ = pretext.process(obs, zero_reward if t == 0 else rew)
            if act_fn is not None:
                action = act_fn(t, pobs)
            else:
                # deterministic: dist.mode() (model.py:66-67); the masks zero the state at episode ends inside the kernels
                out, _ = pol.act_rnn(pobs, hxs[t & 1], masks, eps=None, rnn_hxs_out=hxs[(t + 1) & 1])
                action = out["action"]
        if pre_step_fn is not None:
            pre_step_fn(t, env, acc)
        obs, rew, done, info, ep_ret, _ = env.step(action)
        env.get_danger_min_dist(out=danger_dist)
        if frame_fn is not None:
            frame_fn(t + 1, env, obs)
        masks = acc.update(done, info, ep_ret, obs["robot_node"], danger_dist)
        if (t + 1) % poll_every == 0 and acc.n_active() == 0:
            break
    env.close()
    if pretext is not None and pretext.hip is not None:
        pretext.hip.close()
    r = acc.results()
    if per_env is not None:
        per_env.update(r, cases=cases)
    if scenes is not None:
        return None
    if any(o == 0 for o in r["outcome"]):
        raise ValueError("Invalid end signal from environment")
    rew_h = [round(x, 6) for x in r["ep_return"]]
    e_of = {c: e for e, c in enumerate(cases)}
    order = [e_of[case_of[k]] for k in range(test_size)]       # sequential episode k == first episode of the env of its case
    pick = lambda xs: [xs[e] for e in order]
    return _summarise(pick(r["outcome"]), pick(r["steps"]), pick(r["path_length"]), pick(r["danger_steps"]), None, pick(rew_h), float(cfg.time_limit),
                      float(cfg.time_step), logging, danger_sums=pick(r["danger_sum"]))


def _scene_tensors(env, humans, robot):
    """Scenes as the caller wrote them -> the float64 device tensors HipEnvBatch.set_scene takes.  humans [n,H,8], or [n,H,6] (px, py, vx, vy,
    gx, gy: the radius / v_pref columns are filled with the env's own, which a scene keeps anyway); robot [n,8], or [n,7] / [n,6] (the potential
    is recomputed by the call; a missing theta is pi / 2, the heading a holonomic robot's reset gives it)."""
    dev = env.device
    humans = torch.as_tensor(humans, dtype=torch.float64).to(dev)
    robot = torch.as_tensor(robot, dtype=torch.float64).to(dev)
    if humans.dim() == 3 and humans.shape[2] == 6 and tuple(humans.shape[:2]) == (env.E, env.H):
        own, _ = env.get_state()
        humans = torch.cat([humans, own[:, :, 6:8]], dim=2)
    if robot.dim() == 2 and robot.shape[1] in (6, 7):
        pad = torch.zeros(robot.shape[0], 8 - robot.shape[1], dtype=torch.float64, device=dev)
        if robot.shape[1] == 6:
            pad[:, 0] = float(np.pi / 2.0)
        robot = torch.cat([robot, pad], dim=1)
    return humans.contiguous(), robot.contiguous()


def evaluate_scenes(actor_critic, env_name, config, humans, robot, seed=0, act_fn=None, traces=False, max_steps=None, device=None,
                    predictor=None, batch_invariant=False):
    """Run a policy on n hand-built (or recorded) situations: the n scenes are the n envs of one batch, which is reset once (that draws each
    env's radii, speed limits and random stream from `seed`), started from the scenes (HipEnvBatch.set_scene) and then driven by the loop of
    evaluate_batched through each env's FIRST episode -- the one that starts at the scene: bookkeeping by cn_eval_accumulate, the count of running
    episodes read back every 16 steps, no synchronisation per step.  Phase 'test', as in evaluate_batched.
    humans [n,H,8] or [n,H,6], robot [n,8], [n,7] or [n,6] (numpy or torch; see _scene_tensors), H = human_num + human_num_range of the config.
    actor_critic: a Policy of either base ('selfAttn_merge_srnn', 'srnn'); None with config.robot.policy 'orca' / 'social_force' runs the
    scripted robot (the ORCA robot with env.randomize_attributes on is refused, as in evaluate_batched); act_fn(t, obs) -> actions [n,2] replaces the forward.  max_steps: step bound (default round(time_limit / time_step) + 1).
    Returns a dict of per-scene host lists: outcome (the info code: 1 timeout, 2 collision, 3 goal reached; 0: still running after max_steps),
    steps, ep_return, and from the recorded states (cn_trace_metrics) path_length -- over the states steps were taken FROM, so without the
    final step's move -- and min_clearance.  traces=True: (that dict, EpisodeTraces) -- .figure() / .frames(scene index) draw them; record 0
    of scene i is scene i itself."""
    if env_name == "CrowdSimVarNumCollect-v0":
        raise ValueError("evaluate_scenes: CrowdSimVarNumCollect-v0 takes no scenes")
    rec = _TraceRecorder(config, env_name)
    with _batch_invariant(actor_critic, batch_invariant):
        _evaluate_batched(actor_critic, env_name, config, seed, 0, device, None, predictor=predictor, act_fn=act_fn, per_env=rec.per_env,
                          pre_step_fn=rec, scenes=(humans, robot), max_steps=max_steps)
    tr = rec.finish()
    m = tr.metrics()
    r = rec.per_env
    out = dict(outcome=[int(o) for o in r["outcome"]], steps=[int(x) for x in r["steps"]], ep_return=list(r["ep_return"]),
               path_length=m["path_length"].tolist(), min_clearance=m["min_clearance"].tolist())
    return (out, tr) if traces else out


FRAME_BUFFER_LIMIT = 4 << 30     # bytes of device memory render_episodes may ask for


def render_episodes(actor_critic, env_name, config, seed, cases, size=256, device=None, predictor=None, batch_invariant=False):
    """Run the test cases `cases` exactly as evaluate_batched runs them (one env per case, its first episode; actor_critic=None: the ORCA
    robot) and draw every state on the device (HipEnvBatch.render; CrowdSimPred-v0 also gets its predictions as dots).
    Returns {case: dict(frames=uint8 [steps+1,size,size,3], outcome=1 timeout / 2 collision / 3 goal, steps=...)}: frame 0 is the reset
    state, frame t the state after step t -- the last one therefore shows what the vec-env's auto-reset left.  The frames go into ONE
    preallocated device buffer [T,n,size,size] RGBA and are read back once at the end; a request whose buffer would exceed 4 GiB is
    refused."""
    from .hip_env import prediction_dots
    cases = sorted(set(int(c) for c in cases))
    if not cases:
        raise ValueError("render_episodes: no cases given")
    size, n = int(size), len(cases)
    cfg = to_env_config(config, env_name, 1, "test")
    T = int(round(float(cfg.time_limit) / float(cfg.time_step))) + 2      # the reset frame + one per step of the longest episode
    nbytes = 4 * T * n * size * size
    if nbytes > FRAME_BUFFER_LIMIT:
        raise ValueError("render_episodes: %d cases x %d frames of %d x %d pixels need a %.1f GiB frame buffer (limit 4 GiB): fewer cases per "
                         "call, or a smaller size" % (n, T, size, size, nbytes / float(1 << 30)))
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    buf = torch.zeros(T, n, size, size, 4, dtype=torch.uint8, device=device)
    with_dots = env_name == "CrowdSimPred-v0"

    def draw(t, env, obs):
        dots, counts = prediction_dots(obs) if with_dots else (None, None)
        env.render(size=size, dots=dots, dot_counts=counts, out=buf[t])

    per_env = {}
    with _batch_invariant(actor_critic, batch_invariant):
        _evaluate_batched(actor_critic, env_name, config, seed, cases, device, None, predictor=predictor, per_env=per_env, frame_fn=draw)
    last = max(per_env["steps"])
    frames = buf[:last + 1, :, :, :, :3].contiguous().cpu().numpy()
    return {c: dict(frames=frames[:per_env["steps"][e] + 1, e].copy(), outcome=per_env["outcome"][e], steps=per_env["steps"][e])
            for e, c in enumerate(per_env["cases"])}


class EpisodeTraces(object):
    """n recorded episodes on the device, in the layout of cn_env_trace_append (include/crowdnav_hip.h): agents float32 [n,cap,A,6] (slot 0 the
    robot: px, py, vx, vy, radius, theta; slot 1 + h human slot h: px, py, vx, vy, radius, v_pref), flags uint8 [n,cap,A] (bit 0 present, bit 1
    visible to the robot), goal float32 [n,2], length int32 [n]; cases / outcome / steps as host lists, and the config values measuring and
    drawing need.  Record t is the state step t was taken FROM (record 0: the reset state; length == steps); the state after the final step
    is not in a trace -- the simulator replaces it with the next episode's start inside the step -- and nothing here pretends otherwise."""
    CONFIG_KEYS = ("time_step", "discomfort_dist", "robot_radius", "arena_size", "sensor_range", "human_radius", "kinematics")

    def __init__(self, agents, flags, goal, length, cases, outcome, steps, **config):
        missing = [k for k in self.CONFIG_KEYS if k not in config]
        if missing or len(config) != len(self.CONFIG_KEYS):
            raise ValueError("EpisodeTraces: config values %s expected" % (self.CONFIG_KEYS,))
        self.agents, self.flags, self.goal, self.length = agents, flags, goal, length
        self.cases, self.outcome, self.steps = [int(c) for c in cases], [int(o) for o in outcome], [int(x) for x in steps]
        for k in self.CONFIG_KEYS:
            setattr(self, k, int(config[k]) if k == "kinematics" else float(config[k]))

    @property
    def n(self):
        return int(self.agents.shape[0])

    def config(self):
        return {k: getattr(self, k) for k in self.CONFIG_KEYS}

    def metrics(self):
        """{column name: numpy [n]} of cn_trace_metrics (hip_env.TRACE_METRICS; the counts as int64, the rest float64): one launch, one
        read-back."""
        from .hip_env import TRACE_METRICS, trace_metrics
        m = trace_metrics(self.agents, self.flags, self.length, self.time_step, self.discomfort_dist).cpu().numpy()
        ints = ("records", "intrusion_steps", "visible_intrusion_steps")
        return {k: (m[:, j].astype(np.int64) if k in ints else m[:, j].copy()) for j, k in enumerate(TRACE_METRICS)}

    def figure(self, size=256, stride=8):
        """One picture per episode (cn_render_trajectories): uint8 [n,size,size,4] RGBA on the device, the view render() uses
        (half width arena_size + 1)."""
        from .hip_env import render_trajectories as draw
        return draw(self.agents, self.flags, self.length, self.goal, stride=stride, size=size, half_width=self.arena_size + 1.0)

    def frames(self, case, size=256):
        """The episode of `case` re-drawn record by record through render_scenes: uint8 [steps,size,size,3] (numpy).  The float64 inputs of
        render_scenes are rebuilt from the float32 records (float32 -> float64 -> float32 is the identity), so with a holonomic robot
        (CrowdSimVarNum-v0) these are the pixels render_episodes produced for frames 0..steps-1; a unicycle robot's heading mark is drawn
        from the recorded float32 theta."""
        from .hip_env import render_scenes
        e = self.cases.index(int(case))
        L = int(self.length[e].item())
        if L < 1:
            return np.zeros((0, int(size), int(size), 3), dtype=np.uint8)
        ag, fl = self.agents[e, :L].to(torch.float64), self.flags[e, :L, 1:]
        H = ag.shape[1] - 1
        humans = torch.zeros(L, H, 8, dtype=torch.float64, device=ag.device)
        humans[:, :, 0:4], humans[:, :, 6:8] = ag[:, 1:, 0:4], ag[:, 1:, 4:6]
        robot = torch.zeros(L, 8, dtype=torch.float64, device=ag.device)
        robot[:, 0:4], robot[:, 4:6], robot[:, 6] = ag[:, 0, 0:4], self.goal[e].to(torch.float64), ag[:, 0, 5]
        counts = (fl & 1).sum(dim=1).to(torch.int32)
        visible = ((fl >> 1) & 1).contiguous()
        if self.kinematics == 0:
            heading = robot[:, 2:4].to(torch.float32)
        else:
            heading = torch.stack((torch.cos(robot[:, 6]), torch.sin(robot[:, 6])), dim=1).to(torch.float32)
        img = render_scenes(humans, robot, counts=counts, visible=visible, robot_heading=heading.contiguous(), robot_radius=self.robot_radius,
                            ring_radius=self.sensor_range + self.robot_radius + self.human_radius, size=size, half_width=self.arena_size + 1.0)
        return img[..., :3].contiguous().cpu().numpy()

    def save(self, path):
        """Everything into one .npz."""
        np.savez_compressed(path, agents=self.agents.cpu().numpy(), flags=self.flags.cpu().numpy(), goal=self.goal.cpu().numpy(),
                            length=self.length.cpu().numpy(), cases=np.asarray(self.cases, dtype=np.int64),
                            outcome=np.asarray(self.outcome, dtype=np.int64), steps=np.asarray(self.steps, dtype=np.int64),
                            **{k: np.asarray(getattr(self, k)) for k in self.CONFIG_KEYS})

    @classmethod
    def load(cls, path, device=None):
        """device None: the tensors stay on the CPU (metrics / figure / frames need them on the GPU)."""
        with np.load(path) as z:
            dev = torch.device(device) if device is not None else torch.device("cpu")
            t = {k: torch.from_numpy(z[k]).to(dev) for k in ("agents", "flags", "goal", "length")}
            return cls(t["agents"], t["flags"], t["goal"], t["length"], z["cases"].tolist(), z["outcome"].tolist(), z["steps"].tolist(),
                       **{k: z[k].item() for k in cls.CONFIG_KEYS})


class _TraceRecorder(object):
    """The pre_step_fn of _evaluate_batched that records: buffers allocated once at the first call, then one cn_env_trace_append per step fed
    with the accumulator's ACTIVE and STEPS arrays as they are."""

    def __init__(self, config, env_name):
        self.cfg = to_env_config(config, env_name, 1, "test")
        self.cap = int(round(float(self.cfg.time_limit) / float(self.cfg.time_step))) + 1
        self.per_env, self.trace = {}, None

    def __call__(self, t, env, acc):
        if self.trace is None:
            E, A_, dev = env.E, env.H + 1, env.device
            self.trace = EpisodeTraces(torch.zeros(E, self.cap, A_, 6, device=dev), torch.zeros(E, self.cap, A_, dtype=torch.uint8, device=dev),
                                       torch.zeros(E, 2, device=dev), torch.zeros(E, dtype=torch.int32, device=dev), [], [], [],
                                       **{k: getattr(self.cfg, k) for k in EpisodeTraces.CONFIG_KEYS})
        env.trace_append(acc.active, acc.steps, self.trace)

    def finish(self):
        tr, r = self.trace, self.per_env
        tr.cases, tr.outcome, tr.steps = list(r["cases"]), list(r["outcome"]), list(r["steps"])
        return tr


def record_episodes(actor_critic, env_name, config, seed, cases, device=None, predictor=None, batch_invariant=False):
    """Run the test cases `cases` exactly as evaluate_batched runs them (one env per case, its first episode; actor_critic=None: the ORCA
    robot) and record every state a step was taken from on the device: one cn_env_trace_append launch per step in front of the step, no
    allocation inside the loop, no host synchronisation.  Returns EpisodeTraces with cap = round(time_limit / time_step) + 1 records per
    episode, in the order of sorted(set(cases)).  The state after an episode's final step is not recorded (see EpisodeTraces)."""
    cases = sorted(set(int(c) for c in cases))
    if not cases:
        raise ValueError("record_episodes: no cases given")
    rec = _TraceRecorder(config, env_name)
    with _batch_invariant(actor_critic, batch_invariant):
        _evaluate_batched(actor_critic, env_name, config, seed, cases, device, None, predictor=predictor, per_env=rec.per_env, pre_step_fn=rec)
    return rec.finish()


def render_trajectories(actor_critic, env_name, config, seed, cases, size=256, stride=8, device=None, predictor=None, batch_invariant=False):
    """The per-episode trajectory figure (the reference's test.py --render_traj, which it announces and never draws): record_episodes, then
    one cn_render_trajectories launch and one cn_trace_metrics launch.  Returns {case: dict(image=uint8 [size,size,3], outcome, steps,
    metrics={column: value})}."""
    tr = record_episodes(actor_critic, env_name, config, seed, cases, device=device, predictor=predictor, batch_invariant=batch_invariant)
    img = tr.figure(size=size, stride=stride)[..., :3].contiguous().cpu().numpy()
    m = tr.metrics()
    return {c: dict(image=img[e], outcome=tr.outcome[e], steps=tr.steps[e], metrics={k: v[e].item() for k, v in m.items()})
            for e, c in enumerate(tr.cases)}
