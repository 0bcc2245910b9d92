"""-m gpu: cn_env_set_scene / HipEnvBatch.set_scene / BatchedCrowdSim.set_scene / evaluation.evaluate_scenes.

A scene is the start of an episode from the caller's records.  Everything here is bit for bit: against the snapshot route the older suites use
(tests/orca_scene_util.inject), against the scalar ORCA reference, against the batch the records were read from (round trip, mid-episode
transplant), against twins that never saw the call (select) and across a snapshot.  The premises -- a transplanted state continues like its
source, the outcomes of the three evaluate_scenes cases -- are validated on the CPU oracle in tests/test_scene_cases.py, whose constants the
outcome test imports."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import orca_scene_util as S  # noqa: E402
from tests import scene_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
OBS_KEYS = ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num", "visible_masks")


def _env(E, seed=U.SEED, **cfg):
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
    return HipEnvBatch(A.default_env_config(**dict(cfg, nenv=E)), E, seed)


def _np(x):
    return x.cpu().numpy().copy()


def _obs(obs):
    return {k: _np(obs[k]) for k in OBS_KEYS}


def _step(env, action):
    """One step -> dict of host copies: humans, robot, reward, done, info and every observation tensor."""
    obs, rew, done, info, _, _ = env.step(action)
    h, r = env.get_state()
    return dict(_obs(obs), humans=_np(h), robot=_np(r), reward=_np(rew), done=_np(done), info=_np(info))


def _assert_same(a, b, what, rows=None, keys=None):
    for k in (keys if keys is not None else a):
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        np.testing.assert_array_equal(x, y, err_msg="%s: %s" % (what, k))


def _cuda(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrays)


def _records(env, humans6, robot6):
    """humans [E,H,6] / robot [E,6] -> the get_state layout on the device: columns 6, 7 the env's own, theta the env's own."""
    h, r = env.get_state()
    h, r = h.clone(), r.clone()
    h[:, :, 0:6] = torch.from_numpy(np.asarray(humans6, dtype=np.float64)).cuda()
    r[:, 0:6] = torch.from_numpy(np.asarray(robot6, dtype=np.float64)).cuda()
    return h, r


# ---- 1. the snapshot route, bit for bit ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("h8_rv0", "h20_rv0", "h32_rv1", "h40_rv0"))
def test_set_scene_equals_the_snapshot_route(name):
    c = S.CASES[name]
    E, H = c["E"], c["H"]
    assert (E * H) % 64 != 0
    _, humans, robot = S.case_scene(name)
    a, b = _env(E, **S.case_config(name)), _env(E, **S.case_config(name))
    a.reset()
    b.reset()
    h1, r1 = S.inject(a, humans, robot)
    b.set_scene(*_cuda(h1, r1))
    hb, rb = S.read(b)
    np.testing.assert_array_equal(hb, h1)
    np.testing.assert_array_equal(rb, r1)                      # the potential included: -||p - g||, as inject() patches it
    zero = torch.zeros(E, 2, device="cuda")
    for t in range(8):
        _assert_same(_step(a, zero), _step(b, zero), "%s step %d" % (name, t))
    a.close()
    b.close()


# ---- 2. the scalar ORCA reference -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("h20_rv0", "h32_rv1"))
def test_first_step_after_set_scene_matches_the_scalar_reference(name):
    c = S.CASES[name]
    E = c["E"]
    _, humans, robot = S.case_scene(name)
    env = _env(E, **S.case_config(name))
    env.reset()
    _, nds = S.oracle_reset_attrs(name)
    env.set_scene(*_records(env, humans, robot))
    h, r = S.read(env)
    np.testing.assert_array_equal(h[:, :, 0:6], humans)
    _, _, done, _, _, _ = env.step(torch.zeros(E, 2, device="cuda"))
    assert not _np(done).any()
    h1, _ = S.read(env)
    ref = np.stack([S.env_reference(env.cfg, h[e], r[e], nds[e]) for e in range(E)])
    kept = (h1[:, :, 4:6] == h[:, :, 4:6]).all(axis=2)          # a human the step respawned (it stood on its goal) is exempt
    assert kept.sum() > kept.size // 2
    np.testing.assert_array_equal(h1[:, :, 2:4].astype(np.float32)[kept], ref[kept])
    env.close()


# ---- 3. round trip -----------------------------------------------------------------------------------------------------------------

ROUND_TRIP = {
    "varnum": {}, "pred_const_vel": dict(env_kind=1), "pred_truth": dict(env_kind=1, predict_truth=1), "sf_humans": dict(humans_policy=1),
    "unicycle": dict(kinematics=1), "random_attrs": dict(randomize_attributes=1),
}


@pytest.mark.parametrize("H", (5, 20))
@pytest.mark.parametrize("kind", sorted(ROUND_TRIP))
def test_round_trip_is_the_identity(kind, H):
    """B.set_scene(*A.get_state()) right after both were reset: the same first observation, then 30 common steps (goal changes at step 20,
    arrivals, auto-resets: everything that draws from the stream or reads the reset bookkeeping) leave the two batches equal."""
    E = 7
    cfg = dict(ROUND_TRIP[kind], human_num=H, random_goal_changing=1)
    a, b = _env(E, **cfg), _env(E, **cfg)
    first = _obs(a.reset())
    b.reset()
    got = _obs(b.set_scene(*a.get_state()))
    _assert_same(first, got, "%s H=%d reset observation" % (kind, H))
    actions = torch.from_numpy(np.random.RandomState(H).uniform(-1.0, 1.0, (30, E, 2)).astype(np.float32)).cuda()
    for t in range(30):
        _assert_same(_step(a, actions[t]), _step(b, actions[t]), "%s H=%d step %d" % (kind, H, t))
    a.close()
    b.close()


# ---- 4. mid-episode transplant -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", (8, 20))
def test_mid_episode_transplant(H):
    """Premise (a) of tests/test_scene_cases.py on the device: 12 steps, the state into a batch that was only reset (goal changing off), the
    observation set_scene returns is the one the 12th step returned, and one more common step leaves the same agent records -- and, where
    the source's potential already was that of its position, the same potential and reward."""
    E = 7
    cfg = dict(human_num=H, random_goal_changing=0, end_goal_changing=0)
    a, b = _env(E, **cfg), _env(E, **cfg)
    a.reset()
    b.reset()
    actions = np.random.RandomState(H).uniform(-0.4, 0.4, (13, E, 2)).astype(np.float32)
    actions[11, 0::2] = 0.0              # these robots stand still in the 12th step: see `fresh` below
    actions = torch.from_numpy(actions).cuda()
    for t in range(12):
        last = _step(a, actions[t])          # (an env whose episode ended meanwhile carries the first steps of its next one: as good a state)
    assert np.abs(last["humans"][:, :, 2:4]).max() > 0.1
    got = _obs(b.set_scene(*a.get_state()))
    _assert_same(last, got, "observation of the transplanted state", keys=OBS_KEYS)
    sa, sb = _step(a, actions[12]), _step(b, actions[12])
    # Column 7, the potential, is not taken: set_scene recomputes it as -||p - g|| of the state it is given, as a reset does.  The source's
    # is the one calc_reward left, -||p - g|| of the position its last step STARTED from (crowd_sim_var_num.py:536-542: evaluated before the
    # move, and not at all in a step that ended in the discomfort zone).  The two are the same number where the robot stood still in a 12th
    # step without a Danger, or where that step ended the episode (the auto-reset's potential is a reset's): there the whole record and the
    # reward must agree; elsewhere the seven fields the call takes (what tests/test_scene_cases.py compares on the oracle).
    r12 = last["robot"]
    fresh = r12[:, 7] == -np.sqrt((r12[:, 4] - r12[:, 0]) ** 2 + (r12[:, 5] - r12[:, 1]) ** 2)
    print("H=%d: source potential is that of its position in envs %s" % (H, np.flatnonzero(fresh).tolist()))
    assert fresh.sum() >= 2 and not fresh.all()
    _assert_same(sa, sb, "the step after, potential in step", rows=fresh, keys=("humans", "robot", "reward", "done", "info") + OBS_KEYS)
    sa["robot"], sb["robot"] = sa["robot"][:, 0:7], sb["robot"][:, 0:7]
    _assert_same(sa, sb, "the step after", keys=("humans", "robot", "done", "info") + OBS_KEYS)
    a.close()
    b.close()


# ---- 5. select ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("varnum", "pred_truth"))
def test_select_leaves_the_other_envs_alone(kind):
    """pred_truth: the 'truth' roll-out kernels run over the whole batch again and env_obs_kernel only finishes the selected envs; the others
    must come out as if nothing had been called."""
    name = "h20_rv0"
    E = S.CASES[name]["E"]
    assert E == 13
    _, humans, robot = S.case_scene(name)
    cfg = dict(S.case_config(name), **ROUND_TRIP[kind])
    never, some, every = (_env(E, **cfg) for _ in range(3))
    odd = np.arange(E) % 2 == 1
    first = _obs(never.reset())
    some.reset()
    every.reset()
    got = _obs(some.set_scene(*_records(some, humans, robot), select=torch.from_numpy(odd).cuda()))
    full = _obs(every.set_scene(*_records(every, humans, robot)))
    _assert_same(got, first, "rows of the envs that were not selected", rows=~odd)
    _assert_same(got, full, "rows of the selected envs", rows=odd)
    zero = torch.zeros(E, 2, device="cuda")
    for t in range(10):
        n, s, f = _step(never, zero), _step(some, zero), _step(every, zero)
        _assert_same(s, n, "step %d, not selected" % t, rows=~odd)
        _assert_same(s, f, "step %d, selected" % t, rows=odd)
    for env in (never, some, every):
        env.close()


# ---- 6. snapshot ---------------------------------------------------------------------------------------------------------------------

def test_a_snapshot_taken_after_set_scene_continues_bit_for_bit():
    name = "h20_rv0"
    E = S.CASES[name]["E"]
    _, humans, robot = S.case_scene(name)
    env, twin = _env(E, **S.case_config(name)), _env(E, **S.case_config(name))
    env.reset()
    env.set_scene(*_records(env, humans, robot))
    actions = torch.from_numpy(np.random.RandomState(6).uniform(-0.3, 0.3, (8, E, 2)).astype(np.float32)).cuda()
    for t in range(3):
        env.step(actions[t])
    twin.load_state_dict(env.state_dict())
    for t in range(3, 8):
        _assert_same(_step(env, actions[t]), _step(twin, actions[t]), "step %d" % t)
    env.close()
    twin.close()


# ---- 7. evaluate_scenes ---------------------------------------------------------------------------------------------------------------

def _outcome_config(time_limit):
    from crowdnav_prediction_attngraph_amd import config as C
    return C.non_randomized(**{"sim.human_num": U.OUTCOME_H, "humans.end_goal_changing": False, "robot.visible": False, "env.time_limit": time_limit})


@pytest.mark.parametrize("time_limit", (50.0, 2.0))
def test_evaluate_scenes_outcomes_and_traces(time_limit):
    """The three outcome scenes as ONE batch, one action per scene, at most 40 steps.  One batch has one time limit, and the reach scene needs 16
    steps where time_limit = 2.0 ends every episode at step 5: so the batch runs twice -- with the default limit (goal reached at step 16,
    collision at step 7, the idle robot still running after 40 steps: outcome 0) and with time_limit = 2.0 (the idle robot times out at step 5,
    as do the other two).  Expected values: the constants of tests/test_scene_cases.py, produced by the CPU oracle.
    Traces: record t of scene e is the state step t was taken from -- read here with get_state from a batch driven by hand through the same
    scenes and actions -- rounded once to float32; record 0 is the scene itself."""
    from crowdnav_prediction_attngraph_amd.config import to_env_config
    from crowdnav_prediction_attngraph_amd.evaluation import evaluate_scenes
    from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
    from tests.test_scene_cases import EXPECTED_DEFAULT_LIMIT, EXPECTED_LIMIT_2S
    expected = EXPECTED_DEFAULT_LIMIT if time_limit == 50.0 else EXPECTED_LIMIT_2S
    humans, robot = U.outcome_scenes()
    actions = torch.from_numpy(U.OUTCOME_ACTIONS).cuda()
    config = _outcome_config(time_limit)
    res, tr = evaluate_scenes(None, "CrowdSimVarNum-v0", config, humans, robot, seed=U.SEED, act_fn=lambda t, obs: actions, traces=True,
                              max_steps=U.OUTCOME_MAX_STEPS)
    print("time_limit %.1f: %s" % (time_limit, res))
    assert list(zip(res["outcome"], res["steps"])) == expected
    assert tr.outcome == res["outcome"] and tr.steps == res["steps"] and _np(tr.length).tolist() == res["steps"]
    if time_limit == 50.0:
        # the reach scene: 15 recorded moves of 0.25 m; the collision scene: the robot ends 0.5 m from a human of radius 0.3
        assert res["path_length"][0] == pytest.approx(15 * 0.25, abs=1e-6) and res["min_clearance"][1] == pytest.approx(-0.1, abs=1e-6)
        assert res["ep_return"][0] > 0.0 > res["ep_return"][1]
    # the same scenes and actions by hand
    env = HipEnvBatch(to_env_config(config, "CrowdSimVarNum-v0", 1, "test"), 3, U.SEED)
    env.reset()
    own, _ = env.get_state()
    h = torch.cat([torch.from_numpy(humans).cuda(), own[:, :, 6:8]], dim=2)
    r = torch.cat([torch.from_numpy(robot).cuda(), torch.zeros(3, 1, dtype=torch.float64, device="cuda")], dim=1)
    env.set_scene(h, r)
    agents, flags = _np(tr.agents), _np(tr.flags)
    f32 = np.float32
    for t in range(max(res["steps"])):
        hs, rs = S.read(env)
        for e in range(3):
            if t < res["steps"][e]:
                want_r = np.array([rs[e, 0], rs[e, 1], rs[e, 2], rs[e, 3], env.cfg.robot_radius, rs[e, 6]]).astype(f32)
                np.testing.assert_array_equal(agents[e, t, 0], want_r, err_msg="scene %d record %d robot" % (e, t))
                np.testing.assert_array_equal(agents[e, t, 1:], hs[e][:, [0, 1, 2, 3, 6, 7]].astype(f32), err_msg="scene %d record %d" % (e, t))
                assert (flags[e, t] & 1).all()
        env.step(actions)
    np.testing.assert_array_equal(agents[:, 0, 1:, 0:4], humans[:, :, 0:4].astype(f32))       # record 0 is the scene, rounded once
    np.testing.assert_array_equal(agents[:, 0, 0, 0:4], robot[:, 0:4].astype(f32))
    np.testing.assert_array_equal(_np(tr.goal), robot[:, 4:6].astype(f32))
    assert tuple(tr.figure(size=64).shape) == (3, 64, 64, 4)
    env.close()


# ---- 8. the vec-env form, with and without the GST wrapper ----------------------------------------------------------------------------

def _spiral(E, H):
    """Every human within sensor range of a robot at the origin, no two at the same distance (the wrapper and the simulator both sort rows by
    distance), at least 2 m away."""
    k = np.arange(H)
    p = ((2.0 + 0.25 * k) * np.stack([np.cos(1.1 * k), np.sin(1.1 * k)])).T
    humans = np.concatenate([p, np.tile([0.125, -0.25], (H, 1)), -p], axis=1)
    robot = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 4.0])
    return np.tile(humans, (E, 1, 1)), np.tile(robot, (E, 1))


def test_vec_env_set_scene_with_the_gst_wrapper():
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
    from tests import gst_horizon_util as HU
    E, H, P = 4, 8, 5
    GST = "CrowdSimPredRealGST-v0"
    cfg = C.non_randomized(**{"sim.human_num": H, "sim.predict_method": "inferred"})
    dev = torch.device("cuda", 0)
    humans6, robot6 = _spiral(E, H)
    S.check_scene(humans6, robot6)
    pred = HU.model(5, P).cuda()
    fresh = make_vec_envs(GST, U.SEED, E, 0.99, None, dev, False, config=cfg, pretext_wrapper=True, predictor=pred)
    used = make_vec_envs(GST, U.SEED, E, 0.99, None, dev, False, config=cfg, pretext_wrapper=True, predictor=pred)
    plain = make_vec_envs("CrowdSimVarNum-v0", U.SEED, E, 0.99, None, dev, False, config=cfg)
    # a wrapper that was just reset, and one that has a history: set to the state the first one was reset to
    first = fresh.reset()
    used.reset()
    for t in range(7):
        used.step(torch.full((E, 2), 0.3, device="cuda"))
    got = used.set_scene(*fresh.get_state())
    assert tuple(got["spatial_edges"].shape) == (E, H, 2 * (P + 1))
    for k in first:
        assert torch.equal(first[k], got[k]), k
    sd_fresh, sd_used = fresh.state_dict()["pretext"], used.state_dict()["pretext"]
    assert sorted(sd_fresh) == sorted(sd_used)
    for k in sd_fresh:
        if torch.is_tensor(sd_fresh[k]):
            assert torch.equal(sd_fresh[k], sd_used[k]), k
        else:
            assert sd_fresh[k] == sd_used[k], k
    # a hand-built scene: the current positions are the plain env's observation of the same scene
    plain.reset()
    h, r = _records(used._env, humans6, robot6)
    wide = used.set_scene(h, r)
    narrow = plain.set_scene(*_records(plain._env, humans6, robot6))
    assert tuple(wide["spatial_edges"].shape) == (E, H, 2 * (P + 1)) and tuple(narrow["spatial_edges"].shape) == (E, H, 2)
    assert torch.equal(wide["spatial_edges"][:, :, 0:2], narrow["spatial_edges"])
    assert bool((narrow["spatial_edges"].norm(dim=2) < 5.0).all()) and bool(torch.isfinite(wide["spatial_edges"]).all())
    with pytest.raises(ValueError, match="whole batch"):
        used.set_scene(h, r, select=np.arange(E) % 2 == 1)
    for v in (fresh, used, plain):
        v.close()


# ---- refusals on a live batch ---------------------------------------------------------------------------------------------------------

def test_refusals_on_a_live_batch():
    from crowdnav_prediction_attngraph_amd import _abi as A
    env = _env(3, human_num=5, randomize_attributes=1)
    h = torch.zeros(3, 5, 8, dtype=torch.float64, device="cuda")
    r = torch.zeros(3, 8, dtype=torch.float64, device="cuda")
    with pytest.raises(A.CnError, match="cn_env_set_scene: the batch was never reset"):
        env.set_scene(h, r, check=False)
    env.reset()
    h, r = env.get_state()
    bad = h.clone()
    bad[1, 3, 1] = float("nan")
    with pytest.raises(ValueError, match="env 1 human slot 3: py is nan"):
        env.set_scene(bad, r)
    bad = h.clone()
    bad[2, 0, 6] += 0.01
    with pytest.raises(ValueError, match="env 2 human slot 0: radius"):
        env.set_scene(bad, r)
    with pytest.raises(ValueError, match="humans must be torch.float64"):
        env.set_scene(h.float(), r)
    with pytest.raises(ValueError, match="robot must live on"):
        env.set_scene(h, r.cpu())
    env.set_scene(h, r)
    env.close()


# ---- evaluate_scenes drivers: both network bases, the scripted robots -------------------------------------------------------------------

@pytest.mark.parametrize("driver", ("selfAttn_merge_srnn", "srnn", "orca", "social_force"))
def test_evaluate_scenes_runs_every_driver_on_the_catalogue(driver):
    """The four catalogue scenes of 8 humans as one batch, 40 steps at the most: every driver runs them, twice with the same result, and
    record 0 of every trace is the scene."""
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd import scenes as SC
    from crowdnav_prediction_attngraph_amd.evaluation import evaluate_scenes
    H, name = 8, "CrowdSimVarNum-v0"
    over = {"sim.human_num": H, "humans.end_goal_changing": False}
    if driver in ("orca", "social_force"):
        over["robot.policy"] = driver
    cfg = C.non_randomized(**over)
    dev = torch.device("cuda", 0)
    pol = None
    if driver not in ("orca", "social_force"):
        from crowdnav_prediction_attngraph_amd.policy import Policy
        from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
        envs = make_vec_envs(name, U.SEED, 1, 0.99, None, dev, True, config=cfg)
        torch.manual_seed(3)
        pol = Policy(envs.observation_space.spaces, envs.action_space, base=driver,
                     base_kwargs=dict(env_name=name, num_processes=1, num_mini_batch=1, seq_length=30)).to(dev)
        with torch.no_grad():
            pol.dist.fc_mean.bias.copy_(torch.tensor([0.0, 0.8]))          # an untrained policy that heads up the arena, towards the goals
        envs.close()
    humans, robot = SC.stack([fn(H) for fn in SC.CATALOGUE.values()])
    runs = [evaluate_scenes(pol, name, cfg, humans, robot, seed=U.SEED, traces=True, max_steps=40, device=dev, batch_invariant=True) for _ in (0, 1)]
    (res, tr), (res2, tr2) = runs
    print(driver, res)
    assert res == res2 and torch.equal(tr.agents, tr2.agents)
    assert all(o in (0, 1, 2, 3) for o in res["outcome"]) and all(1 <= s <= 40 for s in res["steps"])
    assert all(s == 40 for o, s in zip(res["outcome"], res["steps"]) if o == 0)
    agents = _np(tr.agents)
    np.testing.assert_array_equal(agents[:, 0, 1:, 0:4], humans[:, :, 0:4].astype(np.float32))
    np.testing.assert_array_equal(agents[:, 0, 0, 0:4], robot[:, 0:4].astype(np.float32))
    assert float(np.abs(agents[:, 1, 0, 0:2] - agents[:, 0, 0, 0:2]).max()) > 0.0           # the robot moved
