"""The simulator's handle (cn_env_batch: HipEnvBatch), drawing (render_scenes, prediction_dots, tile_images), recorded episodes (trace_metrics,
render_trajectories), the stand-alone ORCA solve and the device-side launch stamps of the step's kernels (StepStamps)."""
import ctypes as C

import torch

from . import _abi as A
from .hip_policy import HipHandle, _need_cuda


class HipEnvBatch(HipHandle):
    """E device-resident environments (cn_env_batch).  Mirrors VecEnv reset/step at tensor level; no host sync."""

    _sym = "cn_env"

    def __init__(self, cfg, num_envs, seed, first_env_index=0, device=None):
        self.cfg = cfg
        self.E = int(num_envs)
        self.H = int(cfg.human_num) + int(cfg.human_num_range)   # observation rows (the crowd holds <= H humans)
        self._open(device, C.byref(cfg), self.E, int(seed), int(first_env_index))
        self.D = A.lib().cn_env_obs_width(C.byref(cfg))
        E, H, D, dev = self.E, self.H, self.D, self.device
        self.obs = {
            "robot_node": torch.zeros(E, 1, 7, device=dev), "temporal_edges": torch.zeros(E, 1, 2, device=dev),
            "spatial_edges": torch.zeros(E, H, D, device=dev), "detected_human_num": torch.zeros(E, 1, device=dev),
            "visible_masks": torch.zeros(E, H, dtype=torch.uint8, device=dev),
        }
        # derived data of the newest observation, written by every reset() / step() beside it: row offsets + a packing of the envs into
        # equally filled tiles for the policy's fused human-human kernel (csrc/row_plan.h).  Pass it to HipPolicy.act(..., row_plan=) ONLY
        # together with the observation it was made for (the one the last reset() / step() of THIS batch returned or wrote).
        self.row_plan = torch.zeros(int(A.lib().cn_row_plan_words(E)), dtype=torch.int32, device=dev)
        # the per-step host-visible outputs live in ONE buffer (ep_return f64 | reward f32 | ep_len i32 | done u8 | info u8): a caller that
        # needs them on the host (the reference's VecPyTorch contract, vec_env.BatchedCrowdSim.step) fetches all five with one transfer
        self._packed = torch.zeros(18 * E, dtype=torch.uint8, device=dev)
        self.ep_return = self._packed[0:8 * E].view(torch.float64)
        self.reward = self._packed[8 * E:12 * E].view(torch.float32)
        self.ep_len = self._packed[12 * E:16 * E].view(torch.int32)
        self.done = self._packed[16 * E:17 * E]
        self.info = self._packed[17 * E:18 * E]
        self._packed_host = None
        self._reward_in_packed = False    # did the last step() write its reward into the packed buffer (fetch_step_outputs reads it there)?
        self._tail_policies = []          # weak references to the HipPolicy objects whose post-hh hook points at this batch (attach_env_tail)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            # a policy whose hook still holds this handle would call cn_env_launch_tail on freed memory at its next forward: detach first
            for ref in list(getattr(self, "_tail_policies", ())):
                pol = ref()
                if pol is not None and getattr(pol, "_tail_env", None) is self:
                    pol.attach_env_tail(None)
            self._tail_policies = []
        super().close()

    def reset(self, obs=None):
        obs = self.obs if obs is None else obs
        o = A.obs_struct(obs, self.row_plan)
        A.call("cn_env_reset", self._h, C.byref(o), A.stream_ptr(), device=self.device)
        return obs

    def step(self, actions, obs=None, not_done=None, reward=None):
        """actions [E,2] float32 on the device -> (obs, reward [E], done [E] u8, info [E] u8, ep_return, ep_len).
        not_done: optional float32 [E] / [E,1] tensor that receives 1 - done (the rollout `masks`);
        reward: optional float32 [E] / [E,1] tensor written instead of the internal reward buffer."""
        obs = self.obs if obs is None else obs
        reward = self.reward if reward is None else reward
        for name, t in (("not_done", not_done), ("reward", reward)):
            if t is not None and (t.dtype != torch.float32 or t.numel() != self.E or not t.is_contiguous()):
                raise A.CnError("%s must be a contiguous float32 tensor of %d elements" % (name, self.E))
        if actions.dtype != torch.float32 or actions.shape != (self.E, 2):
            raise A.CnError("actions must be float32 [%d,2]" % self.E)
        actions = actions.contiguous()
        o = A.obs_struct(obs, self.row_plan)
        A.call("cn_env_step", self._h, A.ptr(actions), C.byref(o), A.ptr(reward), A.ptr(self.done), A.ptr(self.info),
               A.ptr(self.ep_return), A.ptr(self.ep_len), A.ptr(not_done), A.stream_ptr(), device=self.device)
        self._reward_in_packed = reward.data_ptr() == self.reward.data_ptr()
        return obs, reward, self.done, self.info, self.ep_return, self.ep_len

    def fetch_step_outputs(self):
        """(reward f32 [E], done bool [E], info u8 [E], ep_return f64 [E], ep_len i32 [E]) of the last step() as numpy arrays: ONE
        device-to-host transfer into a pinned buffer and one stream synchronisation.  The arrays are views of that buffer: valid until the
        next call.  The reward is whatever the packed buffer holds at the time of the call: the raw env reward, or -- when a wrapper
        (gst.PretextProcessor / HipGST.wrapper_step) has added its prediction penalty to that buffer in place -- the reward after the penalty.
        After a step(reward=<caller's tensor>) the packed buffer does not hold that step's reward at all, and the call raises."""
        if not self._reward_in_packed:
            raise A.CnError("fetch_step_outputs: the last step() wrote its reward into a caller-supplied tensor (or no step ran yet), "
                            "the packed buffer holds an older one; read the tensor passed as step(reward=...)")
        E = self.E
        if self._packed_host is None:
            self._packed_host = torch.empty(18 * E, dtype=torch.uint8, pin_memory=True)
        self._packed_host.copy_(self._packed, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        h = self._packed_host.numpy()
        return (h[8 * E:12 * E].view("float32"), h[16 * E:17 * E].view("bool"), h[17 * E:18 * E], h[0:8 * E].view("float64"),
                h[12 * E:16 * E].view("int32"))

    def set_tail_deferral(self, enabled):
        """Hold the side-stream tail of every step (ORCA fallback programs + episode pre-generation) back until launch_tail() -- or until
        HipPolicy.attach_env_tail(env) makes the policy release it right behind its human-human kernel (cn_env_set_tail_deferral)."""
        A.call("cn_env_set_tail_deferral", self._h, int(bool(enabled)))

    def launch_tail(self):
        A.call("cn_env_launch_tail", self._h, A.stream_ptr(), device=self.device)

    def set_pregen_budget(self, ticks_10ns):
        """Time budget (x 10 ns) of one launch of the episode pre-generation kernel; the episodes do not depend on it (cn_env_set_pregen_budget)."""
        A.call("cn_env_set_pregen_budget", self._h, int(ticks_10ns))

    def join(self):
        """Order the library's side-stream work (ORCA of the current state, episode pre-generation) before what the caller enqueues next
        on the current stream: needed to close a graph capture of a block of steps."""
        A.call("cn_env_join", self._h, A.stream_ptr(), device=self.device)

    def get_state(self):
        humans = torch.zeros(self.E, self.H, 8, dtype=torch.float64, device=self.device)
        robot = torch.zeros(self.E, 8, dtype=torch.float64, device=self.device)
        A.call("cn_env_get_state", self._h, A.ptr(humans), A.ptr(robot), A.stream_ptr(), device=self.device)
        return humans, robot

    def set_scene(self, humans, robot, select=None, obs=None, check=True):
        """Start a new episode of the selected envs from a state of the caller's (cn_env_set_scene; include/crowdnav_hip.h is the definition):
        humans [E,H,8] / robot [E,8] float64 device tensors in the layout of get_state() -- `env.set_scene(*other.get_state())` transplants a
        state.  Taken: px, py, vx, vy, gx, gy of the humans present and px, py, vx, vy, gx, gy, theta of the robot; radius / v_pref and the crowd
        size stay the env's, the potential is recomputed.  select: bool / uint8 [E] device tensor, None = every env; the rows of `obs` that
        belong to other envs are left as they are, so with the default buffer (the one reset() / step() write) the result is a complete
        observation of the batch.  Returns the observation dict.  The batch must have been reset once.
        check=True (one host read-back; this is not a hot path) raises ValueError naming the env and slot for non-finite values and for
        radius / v_pref columns that differ from the env's own; check=False goes straight to the launch.  Shapes, dtypes and devices are
        checked either way (no read-back needed)."""
        E, H = self.E, self.H
        if torch.is_tensor(select) and select.dtype == torch.bool:
            select = select.to(torch.uint8)
        check_scene_tensors(humans, robot, select, E, H, self.device)
        humans, robot = humans.contiguous(), robot.contiguous()
        select = select.contiguous() if select is not None else None
        if check:
            own, _ = self.get_state()
            counts = self.get_human_counts().to(torch.float64)
            sel = torch.ones(E, dtype=torch.float64, device=self.device) if select is None else select.to(torch.float64)
            host = torch.cat([humans.reshape(-1), robot.reshape(-1), own[:, :, 6:8].reshape(-1), counts, sel]).cpu().numpy()   # the one read-back
            o = 0
            parts = []
            for n in (E * H * 8, E * 8, E * H * 2, E, E):
                parts.append(host[o:o + n])
                o += n
            check_scene_values(parts[0].reshape(E, H, 8), parts[1].reshape(E, 8), parts[2].reshape(E, H, 2), parts[3].astype("int64"),
                               parts[4] != 0)
        obs = self.obs if obs is None else obs
        o = A.obs_struct(obs, self.row_plan)
        A.call("cn_env_set_scene", self._h, A.ptr(select), A.ptr(humans), A.ptr(robot), C.byref(o), A.stream_ptr(), device=self.device)
        return obs

    def set_case_counters(self, counters):
        """counters: int64/uint64 [E] tensor; the next reset of env e generates test/train case `counters[e]` (+ its seed)."""
        c = torch.as_tensor(counters, dtype=torch.int64).to(self.device).contiguous()
        if c.numel() != self.E or bool((c < 0).any()):
            raise A.CnError("counters must be %d non-negative integers" % self.E)
        A.call("cn_env_set_case_counters", self._h, A.ptr(c), A.stream_ptr(), device=self.device)

    def state_dict(self):
        """Snapshot of the whole simulator state (cn_env_save) as one uint8 CPU tensor -- torch.save()-able next to the policy."""
        n = int(A.lib().cn_env_snapshot_bytes(self._h))
        buf = torch.empty(n, dtype=torch.uint8, device=self.device)
        A.call("cn_env_save", self._h, A.ptr(buf), A.stream_ptr(), device=self.device)
        return buf.cpu()

    def load_state_dict(self, snap):
        """Restore a snapshot taken from a batch of the same configuration / shape / seed / shard (cn_env_load)."""
        n = int(A.lib().cn_env_snapshot_bytes(self._h))
        snap = torch.as_tensor(snap, dtype=torch.uint8)
        if snap.numel() != n:
            raise A.CnError("snapshot has %d bytes, this batch needs %d (different env count / humans / config?)" % (snap.numel(), n))
        buf = snap.to(self.device).contiguous()
        A.call("cn_env_load", self._h, A.ptr(buf), A.stream_ptr(), device=self.device)
        self.row_plan[:8].zero_()   # the plan belongs to an observation of the state that was just replaced

    def get_danger_min_dist(self, out=None):
        """Danger.min_dist of the last step per env (float64 [E]); non-zero only in the test phase.  out: optional tensor to write into."""
        if out is None:
            out = torch.zeros(self.E, dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64 or out.numel() != self.E or not out.is_contiguous():
            raise A.CnError("out must be a contiguous float64 tensor of %d elements" % self.E)
        A.call("cn_env_get_danger_min_dist", self._h, A.ptr(out), A.stream_ptr(), device=self.device)
        return out

    def get_human_counts(self):
        """len(self.humans) per env (int32 [E]); constant unless sim.human_num_range > 0."""
        out = torch.zeros(self.E, dtype=torch.int32, device=self.device)
        A.call("cn_env_get_human_counts", self._h, A.ptr(out), A.stream_ptr(), device=self.device)
        return out

    def get_human_actions(self):
        out = torch.zeros(self.E, self.H, 2, device=self.device)
        A.call("cn_env_get_human_actions", self._h, A.ptr(out), A.stream_ptr(), device=self.device)
        return out

    def get_visibility(self):
        """The robot-side detect_visible decision on the current state (uint8 [E,H], 0 beyond the env's crowd size): what the next
        observation of this state would call visible (cn_env_get_visibility)."""
        out = torch.zeros(self.E, self.H, dtype=torch.uint8, device=self.device)
        A.call("cn_env_get_visibility", self._h, A.ptr(out), A.stream_ptr(), device=self.device)
        return out

    def trace_append(self, active, index, trace):
        """Append the CURRENT state of the envs `active` / `index` select to `trace` in one launch (cn_env_trace_append): every env e with
        active[e] != 0 (active None: all) and 0 <= index[e] < cap gets record index[e] written and length[e] = index[e] + 1, the others are
        left alone.  active / index: contiguous int64 [E] device tensors -- EvalAccumulator.active / .steps as they are.  trace: anything with
        agents float32 [E,cap,H+1,6], flags uint8 [E,cap,H+1], goal float32 [E,2] (or None) and length int32 [E] on the device
        (evaluation.EpisodeTraces).  Called before every step, record t is the state step t was taken from; the state after an episode's
        final step is never recorded (the step replaces it with the next episode's start).  No allocation, no host synchronisation."""
        E, A_ = self.E, self.H + 1
        agents, flags, goal, length = trace.agents, trace.flags, trace.goal, trace.length
        _check_tensors("trace_append", (("active", active, torch.int64), ("index", index, torch.int64), ("agents", agents, torch.float32),
                                        ("flags", flags, torch.uint8), ("goal", goal, torch.float32), ("length", length, torch.int32)))
        if index is None or agents is None or flags is None or length is None:
            raise A.CnError("trace_append: index, agents, flags and length are required")
        if agents.dim() != 4 or agents.shape[0] != E or tuple(agents.shape[2:]) != (A_, 6) or agents.shape[1] < 1:
            raise A.CnError("trace_append: agents must be [%d,cap,%d,6]" % (E, A_))
        cap = int(agents.shape[1])
        _check_shapes("trace_append", (("active", active, (E,)), ("index", index, (E,)), ("flags", flags, (E, cap, A_)), ("goal", goal, (E, 2)),
                                       ("length", length, (E,))))
        A.call("cn_env_trace_append", self._h, A.ptr(active), A.ptr(index), cap, A.ptr(agents), A.ptr(flags), A.ptr(goal), A.ptr(length),
               A.stream_ptr(), device=self.device)

    def render(self, size=128, env_ids=None, half_width=None, dots=None, dot_counts=None, out=None):
        """The current state of the envs (all, or those `env_ids` -- an int tensor or list -- selects) as uint8 [n,size,size,4] RGBA images
        on the device: get_state, get_human_counts, get_visibility and the robot's heading (its velocity when holonomic, (cos theta, sin theta)
        for a unicycle) go to render_scenes.  No host synchronisation.  dots [n,max_dots,2] float32 absolute positions with dot_counts [n]
        int32 (e.g. predicted human positions) are drawn as green discs; half_width defaults to arena_size + 1."""
        cfg = self.cfg
        humans, robot = self.get_state()
        counts, visible = self.get_human_counts(), self.get_visibility()
        if env_ids is not None:
            idx = torch.as_tensor(env_ids, dtype=torch.int64, device=self.device).reshape(-1)
            humans, robot = humans.index_select(0, idx), robot.index_select(0, idx)
            counts, visible = counts.index_select(0, idx), visible.index_select(0, idx)
        if cfg.kinematics == 0:
            heading = robot[:, 2:4].to(torch.float32)
        else:
            heading = torch.stack((torch.cos(robot[:, 6]), torch.sin(robot[:, 6])), dim=1).to(torch.float32)
        return render_scenes(humans, robot, counts=counts, visible=visible, robot_heading=heading.contiguous(), dots=dots, dot_counts=dot_counts,
                             robot_radius=cfg.robot_radius, ring_radius=cfg.sensor_range + cfg.robot_radius + cfg.human_radius, size=size,
                             half_width=cfg.arena_size + 1.0 if half_width is None else half_width, out=out)


def _scene_tensor(name, t, shape, dtype, device):
    """set_scene's refusal of a wrong type, dtype, shape or device, by name (no device needed to decide)."""
    if not torch.is_tensor(t):
        raise ValueError("set_scene: %s must be a torch tensor, got %s" % (name, type(t).__name__))
    if t.dtype != dtype:
        raise ValueError("set_scene: %s must be %s, got %s" % (name, dtype, t.dtype))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("set_scene: %s must have shape %s, got %s" % (name, list(shape), list(t.shape)))
    device = torch.device(device)
    if t.device.type != device.type or (device.index is not None and t.device.index != device.index):
        raise ValueError("set_scene: %s must live on %s (the batch's device), got %s" % (name, device, t.device))


def check_scene_tensors(humans, robot, select, E, H, device):
    """The shape / dtype / device half of HipEnvBatch.set_scene's checks for a batch of E envs x H slots on `device`: ValueError naming the
    argument.  select: uint8 [E] or None."""
    _scene_tensor("humans", humans, (E, H, 8), torch.float64, device)
    _scene_tensor("robot", robot, (E, 8), torch.float64, device)
    if select is not None:
        _scene_tensor("select", select, (E,), torch.uint8, device)


def check_scene_values(humans, robot, own_attrs, counts, selected=None):
    """The value half of set_scene(check=True), on host (numpy) arrays: humans [E,H,8], robot [E,8] as passed, own_attrs [E,H,2] the batch's
    own radius / v_pref columns, counts [E] its crowd sizes, selected [E] bool (None: all).  ValueError naming the env and slot for a
    non-finite value in a field the call takes (px .. gy of the humans present, px .. theta of the robot) and for a radius / v_pref that
    differs from the env's own (a scene does not change them: include/crowdnav_hip.h); unselected envs and slots beyond the crowd are not
    looked at."""
    import numpy as np
    names_h = ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref")
    names_r = ("px", "py", "vx", "vy", "gx", "gy", "theta")
    E, H = humans.shape[0], humans.shape[1]
    selected = np.ones(E, dtype=bool) if selected is None else np.asarray(selected, dtype=bool)
    present = (np.arange(H)[None, :] < np.asarray(counts).reshape(E, 1)) & selected[:, None]
    bad = np.argwhere(~np.isfinite(humans[:, :, 0:6]) & present[:, :, None])
    if len(bad):
        e, j, f = (int(x) for x in bad[0])
        raise ValueError("set_scene: env %d human slot %d: %s is %r (must be finite)" % (e, j, names_h[f], float(humans[e, j, f])))
    bad = np.argwhere(~np.isfinite(robot[:, 0:7]) & selected[:, None])
    if len(bad):
        e, f = (int(x) for x in bad[0])
        raise ValueError("set_scene: env %d robot: %s is %r (must be finite)" % (e, names_r[f], float(robot[e, f])))
    bad = np.argwhere((humans[:, :, 6:8] != own_attrs) & present[:, :, None])
    if len(bad):
        e, j, f = (int(x) for x in bad[0])
        raise ValueError("set_scene: env %d human slot %d: %s is %r, the env's own is %r -- a scene keeps the radii and speed limits the env's "
                         "last reset made (its private ORCA simulators froze them); take columns 6:8 from get_state()"
                         % (e, j, names_h[6 + f], float(humans[e, j, 6 + f]), float(own_attrs[e, j, f])))


def _check_tensors(who, items):
    for name, t, dt in items:
        if t is None:
            continue
        if not t.is_cuda:
            raise A.CnError("%s: %s must live on the GPU (no CPU fallback)" % (who, name))
        if t.dtype != dt or not t.is_contiguous():
            raise A.CnError("%s: %s must be a contiguous %s tensor" % (who, name, dt))
    _need_cuda()


def _check_shapes(who, items):
    for name, t, shape in items:
        if t is not None and tuple(t.shape) != tuple(shape):
            raise A.CnError("%s: %s must have shape %s" % (who, name, list(shape)))


def render_scenes(humans, robot, counts=None, visible=None, robot_heading=None, dots=None, dot_counts=None, robot_radius=0.3,
                  ring_radius=0.0, size=128, half_width=7.0, out=None):
    """cn_render_scenes: n scenes -> uint8 [n,size,size,4] RGBA images on the device, one launch, by the exact fp32 rule of
    include/crowdnav_hip.h.  humans float64 [n,H,8] / robot float64 [n,8] in the layout of HipEnvBatch.get_state(); counts int32 [n], visible
    uint8 [n,H], robot_heading float32 [n,2], dots float32 [n,max_dots,2] + dot_counts int32 [n] are optional (None: every slot holds a human,
    all visible, heading = robot velocity, no dots).  out: optional uint8 [n,size,size,4] tensor to draw into."""
    _check_tensors("render_scenes", (("humans", humans, torch.float64), ("robot", robot, torch.float64), ("counts", counts, torch.int32),
                                     ("visible", visible, torch.uint8), ("robot_heading", robot_heading, torch.float32),
                                     ("dots", dots, torch.float32), ("dot_counts", dot_counts, torch.int32), ("out", out, torch.uint8)))
    if humans.dim() != 3 or humans.shape[2] != 8 or robot.shape != (humans.shape[0], 8):
        raise A.CnError("render_scenes: humans must be [n,H,8] and robot [n,8]")
    n, H, size = int(humans.shape[0]), int(humans.shape[1]), int(size)
    max_dots = 0
    if dots is not None:
        if dots.dim() != 3 or dots.shape[0] != n or dots.shape[2] != 2:
            raise A.CnError("render_scenes: dots must be [n,max_dots,2]")
        max_dots = int(dots.shape[1])
        if max_dots == 0:
            dots = dot_counts = None
    elif dot_counts is not None:
        raise A.CnError("render_scenes: dot_counts given without dots")
    _check_shapes("render_scenes", (("counts", counts, (n,)), ("visible", visible, (n, H)), ("robot_heading", robot_heading, (n, 2)),
                                    ("dot_counts", dot_counts, (n,)), ("out", out, (n, size, size, 4))))
    if out is None:
        out = torch.empty(n, size, size, 4, dtype=torch.uint8, device=humans.device)
    A.call("cn_render_scenes", n, H, A.ptr(humans), A.ptr(robot), A.ptr(counts), A.ptr(visible), A.ptr(robot_heading), A.ptr(dots),
           A.ptr(dot_counts), max_dots, float(robot_radius), float(ring_radius), size, float(half_width),
           A.ptr(out), A.stream_ptr(), device=humans.device)
    return out


TRACE_METRICS = ("records", "path_length", "min_clearance", "intrusion_steps", "visible_intrusion_steps", "mean_speed", "mean_accel",
                 "mean_crowd")           # the CN_TRACE_* columns of include/crowdnav_hip.h, in order


def _trace_shape(who, agents, flags, length):
    _check_tensors(who, (("agents", agents, torch.float32), ("flags", flags, torch.uint8), ("length", length, torch.int32)))
    if agents.dim() != 4 or agents.shape[3] != 6 or min(agents.shape[:3]) < 1:
        raise A.CnError("%s: agents must be [n,cap,A,6]" % who)
    n, cap, A_ = (int(x) for x in agents.shape[:3])
    _check_shapes(who, (("flags", flags, (n, cap, A_)), ("length", length, (n,))))
    return n, cap, A_


def trace_metrics(agents, flags, length, time_step=0.25, discomfort_dist=0.25, out=None):
    """cn_trace_metrics: n recorded episodes (agents float32 [n,cap,A,6], flags uint8 [n,cap,A], length int32 [n], the layout of
    HipEnvBatch.trace_append) -> float64 [n,8] on the device, columns TRACE_METRICS as include/crowdnav_hip.h defines them (path length over
    the recorded segments only, minimum clearance, intrusion steps, ...).  One launch, no host synchronisation."""
    n, cap, A_ = _trace_shape("trace_metrics", agents, flags, length)
    _check_tensors("trace_metrics", (("out", out, torch.float64),))
    _check_shapes("trace_metrics", (("out", out, (n, len(TRACE_METRICS))),))
    if out is None:
        out = torch.empty(n, len(TRACE_METRICS), dtype=torch.float64, device=agents.device)
    A.call("cn_trace_metrics", n, cap, A_, A.ptr(agents), A.ptr(flags), A.ptr(length), float(time_step), float(discomfort_dist), A.ptr(out),
           A.stream_ptr(), device=agents.device)
    return out


def render_trajectories(agents, flags, length, goal, stride=8, size=256, half_width=7.0, out=None):
    """cn_render_trajectories: n recorded episodes -> uint8 [n,size,size,4] RGBA images on the device, one picture per episode, one launch, by
    the exact fp32 rule of include/crowdnav_hip.h: every record leaves a small trail disc per agent, shaded by the record index, every
    `stride`-th record and the last one also the agent's outline, the robot's last record its full disc.  goal float32 [n,2]; out: optional
    uint8 [n,size,size,4] tensor to draw into."""
    n, cap, A_ = _trace_shape("render_trajectories", agents, flags, length)
    size = int(size)
    _check_tensors("render_trajectories", (("goal", goal, torch.float32), ("out", out, torch.uint8)))
    if goal is None:
        raise A.CnError("render_trajectories: goal is required")
    _check_shapes("render_trajectories", (("goal", goal, (n, 2)), ("out", out, (n, size, size, 4))))
    if out is None:
        out = torch.empty(n, size, size, 4, dtype=torch.uint8, device=agents.device)
    A.call("cn_render_trajectories", n, cap, A_, A.ptr(agents), A.ptr(flags), A.ptr(length), A.ptr(goal), int(stride), size, float(half_width),
           A.ptr(out), A.stream_ptr(), device=agents.device)
    return out


def prediction_dots(obs, env_ids=None):
    """The predicted human positions an observation with predictions carries (spatial_edges wider than 2: CrowdSimPred-v0, or
    CrowdSimPredRealGST-v0 behind the prediction wrapper) as the (dots [n,H*P,2] float32, dot_counts [n] int32) pair of render_scenes: rows
    0..detected_human_num-1, columns 2.. as (P,2) robot-relative offsets, plus the robot position.  Device tensors in, device tensors out."""
    se, rn, det = obs["spatial_edges"], obs["robot_node"], obs["detected_human_num"]
    if env_ids is not None:
        idx = torch.as_tensor(env_ids, dtype=torch.int64, device=se.device).reshape(-1)
        se, rn, det = se.index_select(0, idx), rn.index_select(0, idx), det.index_select(0, idx)
    n, H, P = se.shape[0], se.shape[1], (se.shape[2] - 2) // 2
    dots = se[:, :, 2:].to(torch.float32).reshape(n, H * P, 2) + rn.reshape(n, 1, -1)[:, :, 0:2].to(torch.float32)
    counts = (det.reshape(n).to(torch.int32) * P).contiguous()
    return dots.contiguous(), counts


def tile_images(images):
    """[N,h,w,c] -> one [rows*h, cols*w, c] mosaic with rows = ceil(sqrt(N)), cols = ceil(N / rows), filled row by row; missing tiles are
    black (the layout of the vec-env API's tile_images)."""
    import numpy as np
    images = np.asarray(images)
    N, h, w, c = images.shape
    rows = int(np.ceil(np.sqrt(N)))
    cols = int(np.ceil(float(N) / rows))
    grid = np.zeros((rows * cols, h, w, c), dtype=images.dtype)
    grid[:N] = images
    return grid.reshape(rows, cols, h, w, c).transpose(0, 2, 1, 3, 4).reshape(rows * h, cols * w, c)


def orca_solve(self_state, others, neighbor_dist=10.0, max_neighbors=None, time_horizon=5.0, time_step=0.25):
    """Batched stand-alone ORCA (rvo2 replacement).  self_state [B,8], others [B,n,5] float32 device tensors -> [B,2]."""
    _need_cuda()
    B, n = others.shape[0], others.shape[1]
    out = torch.zeros(B, 2, device=self_state.device)
    A.call("cn_orca_solve", B, n, A.ptr(self_state.contiguous()), A.ptr(others.contiguous()), float(neighbor_dist),
           n if max_neighbors is None else int(max_neighbors), float(time_horizon), float(time_step),
           A.ptr(out), A.stream_ptr())
    return out


class StepStamps:
    """Device-side launch stamps of the rollout step's kernels (cn_prof_set_stamps / cn_prof_next_step): a ring of `steps` rows, one slot per
    kernel; a kernel stamps the 100 MHz device clock when it starts and when its last wavefront ends.  Process-wide, one at a time.

        st = StepStamps(steps, ("hh_fused", "rn_fused")); for ...: st.next(); <enqueue one step>; ...; torch.cuda.synchronize(); st.close()
        st.durations_us("hh_fused") -> per-step kernel durations;  st.table() -> start / end of every stamped kernel relative to row 0
    """

    def __init__(self, steps, kernels=tuple(A.PROF_KERNEL_IDS), device=None):
        _need_cuda()
        self.steps = int(steps)
        self.kernels = tuple(kernels)
        dev = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        ring = torch.zeros(self.steps, A.PROF_KERNELS, A.PROF_SLOT_WORDS, dtype=torch.int64, device=dev)
        ring[:, :, 0:1024:16] = -1      # start candidates (word 16 b of the first half): unsigned minimum counts
        self.ring = ring
        mask = 0
        for k in self.kernels:
            mask |= 1 << A.PROF_KERNEL_IDS[k]
        torch.cuda.synchronize(dev)
        A.call("cn_prof_set_stamps", A.ptr(ring), self.steps, mask)
        self._open = True

    def next(self):
        return A.lib().cn_prof_next_step()

    def close(self):
        if self._open:
            A.call("cn_prof_set_stamps", None, 0, 0)
            self._open = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _host(self):
        r = self.ring.cpu().numpy()
        import numpy as np
        t0 = r[:, :, 0:1024:16].astype(np.uint64).min(axis=2)          # all ones = never stamped
        t1 = r[:, :, 1024:2048:16].astype(np.uint64).max(axis=2)
        return t0, t1, r[:, :, 1]

    def durations_us(self, kernel):
        """Per stamped step: (last wavefront's end - first workgroup's start) of `kernel` in microseconds (10 ns resolution)."""
        import numpy as np
        t0, t1, _ = self._host()
        k = A.PROF_KERNEL_IDS[kernel]
        ok = (t1[:, k] > 0) & (t0[:, k] != np.uint64(0xFFFFFFFFFFFFFFFF))
        return ((t1[ok, k] - t0[ok, k]).astype(np.float64) * 0.01).tolist()

    def counts(self, kernel):
        import numpy as np
        t0, t1, c = self._host()
        k = A.PROF_KERNEL_IDS[kernel]
        ok = (t1[:, k] > 0) & (t0[:, k] != np.uint64(0xFFFFFFFFFFFFFFFF))
        return c[ok, k].tolist()

    def table(self):
        """[(step, kernel, start_us, end_us)] of every stamped launch, relative to the earliest stamp, sorted by start."""
        import numpy as np
        t0, t1, _ = self._host()
        rows = []
        valid = (t1 > 0) & (t0 != np.uint64(0xFFFFFFFFFFFFFFFF))
        if not valid.any():
            return rows
        base = t0[valid].min()
        names = {v: k for k, v in A.PROF_KERNEL_IDS.items()}
        for s_ in range(self.steps):
            for k in range(A.PROF_KERNELS):
                if valid[s_, k]:
                    rows.append((s_, names[k], float(t0[s_, k] - base) * 0.01, float(t1[s_, k] - base) * 0.01))
        rows.sort(key=lambda r: r[2])
        return rows
