"""The simulator's config profiles (csrc/env_profile.h) against the CPU oracle, bit for bit.

A batch of the default training class (CrowdSimVarNum-v0, ORCA humans with fixed attributes, a network-driven holonomic robot the
humans do not see, phase train, a fixed crowd size, no narrowed field of view) takes the step kernel compiled for
ProfileTrain; a batch that misses any one predicate takes the generic instantiation.  Which instantiation a launch took is not
observable through the C ABI (and gets no entry point); what is observable is the result: the pinned kernel has no code for a
visible robot, a test phase, a unicycle, social forces, a varying crowd, predictions or per-human radii, so a batch with one of
them that was routed to the pinned kernel could not follow the oracle.

The oracle's run is computed once per case, on the CPU, with the scripted actions of test_gpu_env.py taken from the oracle's own
observations; the GPU batch is then driven with the same actions and must reproduce every output of every step.  For the pinned
cases the run itself is checked: it must contain an auto-reset and a human goal change (read from the oracle's human records),
or the case would not reach the paths it is there for."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_env import _actions, _unicycle_actions  # noqa: E402

KEYS = ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num", "visible_masks")
SEED = 425

# name -> (E, T, config).  T: the shortest run (rounded up to 10) in which the oracle shows what the case is for.
PINNED = {
    # the flagship's shape: the pinned step kernel in front of lane kernel <20, 32>
    "h20": (3, 120, dict(human_num=20, random_goal_changing=1)),
    # ... in front of lane kernel <8, 8>
    "h5": (5, 120, dict(human_num=5, random_goal_changing=1)),
    # a short time limit: time-outs, resets from the staged episode and goal changes (periodic ones and humans at their goal) in one run
    "h20_short_limit": (4, 160, dict(human_num=20, random_goal_changing=1, time_limit=9.0)),
}
# one predicate of ProfileTrain flipped, alone (train_profile_of, env_profile.h)
FLIPPED = {
    "robot_visible": dict(human_num=20, robot_visible=1),
    "human_fov": dict(human_num=20, human_fov=1.2),
    "robot_fov": dict(human_num=20, robot_fov=1.0),
    "test_phase": dict(human_num=20, phase=2),
    "unicycle": dict(human_num=20, kinematics=1),
    "sf_humans": dict(human_num=20, humans_policy=1),
    "human_num_range": dict(human_num=17, human_num_range=3),   # 20 observation rows
    "pred_constvel": dict(human_num=20, env_kind=1),
    "randomize_attributes": dict(human_num=20, randomize_attributes=1),   # brings sim_seen
}
FLIP_E, FLIP_T = 3, 100


def _oracle_env_head():
    """The leading members of OrcEnv (oracle/crowdsim_oracle.h) up to the human records."""
    from oracle import oracle as O

    class OrcMT(C.Structure):
        _fields_ = [("key", C.c_uint32 * 624), ("pos", C.c_int32)]

    class OrcHuman(C.Structure):
        _fields_ = [(k, C.c_double) for k in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref")]

    class OrcEnvHead(C.Structure):
        _fields_ = [("cfg", O.OrcConfig), ("this_seed", C.c_int64), ("case_counter", C.c_uint64 * 3), ("rng", OrcMT), ("rng_draws", C.c_uint64),
                    ("robot", C.c_double * 7), ("humans", OrcHuman * O.MAX_HUMANS)]
    return OrcEnvHead


def _goals(oe, head, n):
    st = C.cast(oe._h, C.POINTER(head)).contents
    return np.array([[st.humans[j].gx, st.humans[j].gy] for j in range(n)]), np.array(list(st.robot))


@functools.lru_cache(maxsize=None)
def _oracle_run(E, T, kw_items):
    """Reset + T scripted steps of E oracle envs: the actions, every output, and what happened (resets, human goal changes)."""
    from oracle import oracle as O
    kw = dict(kw_items, nenv=E)
    head = _oracle_env_head()
    oenvs = [O.OracleEnv(O.default_config(**kw), SEED + i) for i in range(E)]
    H = kw["human_num"] + kw.get("human_num_range", 0)

    def stack(obs_list):
        return {k: np.stack([ob[k] for ob in obs_list]) for k in KEYS}
    host = stack([oe.reset() for oe in oenvs])
    # the private layout the goal check relies on: the robot record of the head is the one the observation shows
    for i, oe in enumerate(oenvs):
        rob = _goals(oe, head, H)[1]
        assert np.float32(rob[0]) == host["robot_node"][i, 0, 0] and np.float32(rob[1]) == host["robot_node"][i, 0, 1]
        assert np.float32(rob[4]) == host["robot_node"][i, 0, 3] and np.float32(rob[5]) == host["robot_node"][i, 0, 4]
    steps = [dict(obs=host)]
    n_reset = n_goal = 0
    goals = [_goals(oe, head, H)[0] for oe in oenvs]
    for t in range(T):
        act = _unicycle_actions(t, E) if kw.get("kinematics", 0) else _actions(host, t, E)
        out, rew, done, info, md, cnt = [], [], [], [], [], []
        for i, oe in enumerate(oenvs):
            ob, r, d, inf = oe.step(act[i], autoreset=True)
            out.append(ob); rew.append(np.float32(r)); done.append(d); info.append(inf["info"]); md.append(inf["min_dist"]); cnt.append(oe.human_count)
            g = _goals(oe, head, H)[0]
            n_reset += int(d)
            n_goal += int(not d and not np.array_equal(g[:cnt[-1]], goals[i][:cnt[-1]]))   # (a reset replaces every goal: not counted)
            goals[i] = g
        host = stack(out)
        steps.append(dict(act=act, obs=host, rew=np.array(rew), done=np.array(done), info=np.array(info), md=np.array(md), cnt=np.array(cnt)))
    return steps, n_reset, n_goal


def _key(kw):
    return tuple(sorted(kw.items()))


@pytest.mark.parametrize("name", list(PINNED))
def test_pinned_cases_reach_a_reset_and_a_goal_change_in_the_oracle(name):
    E, T, kw = PINNED[name]
    _, n_reset, n_goal = _oracle_run(E, T, _key(kw))
    print("%s: %d auto-resets, %d steps with a human goal change" % (name, n_reset, n_goal))
    assert n_reset >= 1 and n_goal >= 1


def _replay(E, T, kw):
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
    steps, n_reset, n_goal = _oracle_run(E, T, _key(kw))
    env = HipEnvBatch(A.default_env_config(**dict(kw, nenv=E)), E, SEED)

    def check(obs, want, what):
        for k in KEYS:
            np.testing.assert_array_equal(obs[k].cpu().numpy().reshape(want[k].shape).astype(want[k].dtype), want[k], err_msg="%s %s" % (k, what))
    check(env.reset(), steps[0]["obs"], "reset")
    for t, st in enumerate(steps[1:]):
        obs, rew, done, info, _, _ = env.step(torch.from_numpy(st["act"]).to(env.device))
        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), st["done"], err_msg="done t=%d" % t)
        np.testing.assert_array_equal(info.cpu().numpy().astype(np.int64), st["info"], err_msg="info t=%d" % t)
        np.testing.assert_array_equal(rew.cpu().numpy(), st["rew"], err_msg="reward t=%d" % t)
        np.testing.assert_array_equal(env.get_danger_min_dist().cpu().numpy(), st["md"], err_msg="min_dist t=%d" % t)
        np.testing.assert_array_equal(env.get_human_counts().cpu().numpy(), st["cnt"], err_msg="len(humans) t=%d" % t)
        check(obs, st["obs"], "t=%d" % t)
    env.close()
    return n_reset, n_goal


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PINNED))
def test_pinned_profile_matches_oracle_bit_exact(name):
    E, T, kw = PINNED[name]
    n_reset, n_goal = _replay(E, T, kw)
    assert n_reset >= 1 and n_goal >= 1   # the sequence length is a condition of the case


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FLIPPED))
def test_one_flipped_predicate_takes_the_generic_kernel_bit_exact(name):
    _replay(FLIP_E, FLIP_T, FLIPPED[name])
