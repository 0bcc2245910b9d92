"""The stream order of a simulator step against the CPU oracle, bit for bit.

A step releases its side-stream work through three events: ev_pre (the episode pre-generation, behind env_step_kernel), ev_state
(the ORCA tail, behind orca_lane_kernel) and ev_orca (what the next step or a reader waits for, behind the tail).  Where the event
follows a launch directly it is that launch's stop event; everywhere else it is recorded (csrc/env_sim.hip: launch_ev,
prefetch_orca, launch_tail).  Which of the two a call took is not observable through the C ABI; what is observable is the result:
an event bound to the wrong launch or stream, or a record left out where something else was enqueued in between, lets a kernel
read a state that is not there yet, and the trajectory leaves the oracle's.

The oracle's run is computed once per case on the CPU with test_gpu_env.py's scripted actions (the runs of
test_gpu_env_profile.py are shared where the case is the same); every output of every step is compared with assert_array_equal.
The cases are the smallest shapes on which each ordering edge can go wrong: the flagship's lane kernel <20, 32> and <8, 8> stepped
with the plan buffer, without one, with a plan buffer the step cannot fill (the 4-byte memset behind the lane launch) and with
readers between the steps; batches without a lane kernel, with the second side stream, with the truth roll-out behind the tail;
the held-back tail; two batches on two streams; a snapshot mid-run."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_env_profile import FLIP_E, FLIP_T, FLIPPED, KEYS, PINNED, SEED, _key, _oracle_run  # noqa: E402

# name -> (E, T, config)
LANE = {"h20": PINNED["h20"], "h5": PINNED["h5"]}
OTHER = {
    "sf_humans": (FLIP_E, FLIP_T, FLIPPED["sf_humans"]),                       # no lane kernel, no tail: ev_state / ev_orca with no launch in front
    "h40_coop": (3, 100, dict(human_num=40, random_goal_changing=1)),         # cooperative ORCA, deferred post-observation updates, second side stream
    "test_phase": (FLIP_E, FLIP_T, FLIPPED["test_phase"]),                     # truth roll-out behind the tail on the side stream
}
# how the batch is stepped
WAYS = ("plan", "no_plan", "unfilled_plan", "reader", "held_tail_reader")


@pytest.mark.parametrize("name", list(LANE))
def test_lane_cases_reach_a_reset_and_a_goal_change_in_the_oracle(name):
    E, T, kw = LANE[name]
    _, n_reset, n_goal = _oracle_run(E, T, _key(kw))
    assert n_reset >= 1 and n_goal >= 1


class _Replay:
    """One GPU batch driven with the oracle's actions; check(a, b) steps it through the oracle's steps a .. b - 1 and compares."""

    def __init__(self, E, T, kw, way="plan"):
        from crowdnav_prediction_attngraph_amd import _abi as A
        from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
        self.E, self.way = E, way
        self.steps, self.n_reset, self.n_goal = _oracle_run(E, T, _key(kw))
        self.env = env = HipEnvBatch(A.default_env_config(**dict(kw, nenv=E)), E, SEED)
        self.obs = None
        if way == "no_plan":
            env.row_plan = None           # cn_obs.row_plan = NULL: the lane kernel builds no plan, nothing follows it on the stream
        elif way == "unfilled_plan":
            # a count view at an odd offset gets no plan (prefetch_orca): the caller's buffer is cleared by a memset BEHIND the lane launch
            self.obs = dict(env.obs)
            self.obs["detected_human_num"] = torch.zeros(E + 1, device=env.device)[1:].view(E, 1)
            assert self.obs["detected_human_num"].data_ptr() % 16 != 0
        elif way == "held_tail_reader":
            env.set_tail_deferral(True)   # no hook: the tail goes out with the next call into the batch (sync_side)

    def _compare(self, obs, want, what):
        for k in KEYS:
            np.testing.assert_array_equal(obs[k].cpu().numpy().reshape(want[k].shape).astype(want[k].dtype), want[k], err_msg="%s %s (%s)" % (k, what, self.way))

    def reset(self):
        self._compare(self.env.reset(self.obs), self.steps[0]["obs"], "reset")

    def check(self, a, b):
        env = self.env
        for t in range(a, b):
            st = self.steps[t + 1]
            obs, rew, done, info, _, _ = env.step(torch.from_numpy(st["act"]).to(env.device), self.obs)
            if self.way in ("reader", "held_tail_reader") and t % 7 == 6:
                hact = env.get_human_actions()
                humans, robot = env.get_state()
                assert bool(torch.isfinite(hact).all()) and bool(torch.isfinite(humans).all())
                np.testing.assert_array_equal(robot[:, 0:2].cpu().numpy().astype(np.float32), st["obs"]["robot_node"][:, 0, 0:2], err_msg="get_state t=%d" % t)
            np.testing.assert_array_equal(done.cpu().numpy().astype(bool), st["done"], err_msg="done t=%d (%s)" % (t, self.way))
            np.testing.assert_array_equal(info.cpu().numpy().astype(np.int64), st["info"], err_msg="info t=%d (%s)" % (t, self.way))
            np.testing.assert_array_equal(rew.cpu().numpy(), st["rew"], err_msg="reward t=%d (%s)" % (t, self.way))
            np.testing.assert_array_equal(env.get_danger_min_dist().cpu().numpy(), st["md"], err_msg="min_dist t=%d (%s)" % (t, self.way))
            self._compare(obs, st["obs"], "t=%d" % t)


@pytest.mark.gpu
@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("name", list(LANE))
def test_lane_batches_follow_the_oracle_however_they_are_stepped(name, way):
    E, T, kw = LANE[name]
    r = _Replay(E, T, kw, way)
    assert r.n_reset >= 1 and r.n_goal >= 1   # the sequence length is a condition of the case
    r.reset()
    r.check(0, T)
    r.env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("way", ("plan", "reader"))
@pytest.mark.parametrize("name", list(OTHER))
def test_batches_without_a_lane_kernel_or_with_more_behind_the_tail_follow_the_oracle(name, way):
    E, T, kw = OTHER[name]
    r = _Replay(E, T, kw, way)
    r.reset()
    r.check(0, T)
    r.env.close()


@pytest.mark.gpu
def test_two_batches_on_two_streams_stepped_alternately_follow_their_oracles():
    """An event bound to the wrong launch or stream shows here: the second batch lives on a non-default stream."""
    (Ea, Ta, kwa), (Eb, Tb, kwb) = LANE["h20"], LANE["h5"]
    side = torch.cuda.Stream()
    ra = _Replay(Ea, Ta, kwa)
    with torch.cuda.stream(side):
        rb = _Replay(Eb, Tb, kwb)
        rb.reset()
    ra.reset()
    for t in range(0, min(Ta, Tb), 3):   # three steps of one, three of the other
        ra.check(t, t + 3)
        with torch.cuda.stream(side):
            rb.check(t, t + 3)
    with torch.cuda.stream(side):
        rb.env.close()
    ra.env.close()


@pytest.mark.gpu
def test_snapshot_mid_run_replays_the_same_steps():
    """cn_env_save between two steps, 30 more steps, cn_env_load, the same 30 steps again: both equal the oracle's."""
    E, T, kw = LANE["h20"]
    r = _Replay(E, T, kw)
    r.reset()
    r.check(0, 50)
    snap = r.env.state_dict()
    r.check(50, 80)
    r.env.load_state_dict(snap)
    r.check(50, 80)
    r.env.close()


@pytest.mark.gpu
def test_held_back_tail_released_by_the_policy_equals_the_inline_mode():
    """cn_env_set_tail_deferral + the policy's post-hh hook (cn_env_launch_tail): the tail's events are recorded, the inline mode's are
    bound to the launches; the same kernels on the same data, so 40 steps of the rollout loop agree bit for bit."""
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch, HipPolicy
    from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces
    E, H = 4, 20
    torch.manual_seed(425)
    ob_space, act_space = make_spaces(H, 2)
    net = Policy(ob_space.spaces, act_space, base_kwargs=dict(env_name="CrowdSimVarNum-v0", num_processes=E), base="selfAttn_merge_srnn").cuda()
    runs = []
    for deferred in (False, True):
        env = HipEnvBatch(A.default_env_config(human_num=H, nenv=E, random_goal_changing=1), E, SEED)
        pol = HipPolicy(H, 2, E)
        pol.set_weights(net.state_dict())
        if deferred:
            env.set_tail_deferral(True)
            pol.attach_env_tail(env)
        obs = env.reset()
        h, m = torch.zeros(E, 1, 128, device="cuda"), torch.ones(E, 1, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(9)
        trace = []
        for t in range(40):
            eps = torch.randn(E, 2, device="cuda", generator=g)
            a = pol.act(obs, h, m, eps=eps, row_plan=env.row_plan)
            h = a["hxs"].clone()
            obs, rew, done, info, _, _ = env.step(a["action"])
            m = (done == 0).float().view(E, 1)
            trace.append([a["action"].clone(), a["value"].clone(), rew.clone(), done.clone(), info.clone()] + [obs[k].clone() for k in sorted(obs)])
        trace.append([env.get_human_actions()])
        pol.attach_env_tail(None)
        env.close()
        pol.close()
        runs.append(trace)
    for t, (ra, rb) in enumerate(zip(*runs)):
        for i, (x, y) in enumerate(zip(ra, rb)):
            assert torch.equal(x, y), (t, i)
