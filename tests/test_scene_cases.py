"""The premises of tests/test_gpu_scenes.py, validated on the CPU oracle (no GPU): (a) records written into a fresh env continue like the
env they were read from, (b) the outcomes the evaluate_scenes case expects -- the constants below are what THIS run produces, the device test
imports them -- and (c) every scene the device tests set keeps the conditions an injected state must keep."""
import numpy as np
import pytest

from crowdnav_prediction_attngraph_amd import scenes as SC
from oracle import oracle as O
from tests import orca_scene_util as S
from tests import scene_util as U

# (info code, steps) of the three outcome scenes, with the default time limit (50 s; 40 steps at the most: the idle robot is still running)
# and with time_limit = 2.0, where the idle robot -- like the other two -- runs into the limit first.  1 timeout, 2 collision, 3 goal reached.
EXPECTED_DEFAULT_LIMIT = [(3, 16), (2, 7), (0, 40)]
EXPECTED_LIMIT_2S = [(1, 5), (1, 5), (1, 5)]


@pytest.mark.parametrize("H", (8, 20))
def test_transplanted_records_continue_bit_for_bit(H):
    """(a) CrowdSimVarNum-v0, full field of view: 12 steps, the records into a fresh twin of the same seed with goal changing off, one more
    step with the same action on both."""
    kw = dict(human_num=H, nenv=1)
    src = O.OracleEnv(O.default_config(**kw), U.SEED)
    twin = O.OracleEnv(O.default_config(random_goal_changing=0, end_goal_changing=0, **kw), U.SEED)
    src.reset()
    twin.reset()
    rs = np.random.RandomState(H)
    for t in range(12):
        _, _, done, _ = src.step(rs.uniform(-0.4, 0.4, 2).astype(np.float32))
        assert not done, t
    h, r = U.oracle_records(src)
    assert np.abs(h[:, 2:4]).max() > 0.1                      # mid-episode: the humans are moving
    U.oracle_poke(twin, h, r)
    h2, r2 = U.oracle_records(twin)
    np.testing.assert_array_equal(h2, h)                      # radius / v_pref were the same to begin with (fixed attributes)
    np.testing.assert_array_equal(r2, r)
    a = np.array([0.3, -0.2], dtype=np.float32)
    src.step(a)
    twin.step(a)
    for got, want in zip(U.oracle_records(twin), U.oracle_records(src)):
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("time_limit,expected", ((50.0, EXPECTED_DEFAULT_LIMIT), (2.0, EXPECTED_LIMIT_2S)))
def test_outcome_scenes_end_as_the_device_test_expects(time_limit, expected):
    """(b) phase test and nenv = 1, as evaluate_scenes creates its batch; env e of the batch has seed SEED + e."""
    humans, robot = U.outcome_scenes()
    got = []
    for e in range(3):
        cfg = O.default_config(phase=2, nenv=1, time_limit=time_limit, **U.OUTCOME_CFG)
        got.append(U.oracle_outcome(cfg, U.SEED + e, humans[e], robot[e], U.OUTCOME_ACTIONS[e], U.OUTCOME_MAX_STEPS))
    print("time_limit %.1f: (info, steps) = %s" % (time_limit, got))
    assert got == expected


def test_every_scene_keeps_the_conditions_of_an_injected_state():
    """(c) finite, inside the arena, the robot clear of every human and of its goal (orca_scene_util.check_scene)."""
    humans, robot = U.outcome_scenes()
    S.check_scene(humans, robot)
    humans, robot = SC.stack([fn(8) for fn in SC.CATALOGUE.values()])      # the four scenes of examples/custom_scenarios.py
    S.check_scene(humans, robot)
    for name in ("h8_rv0", "h20_rv0", "h32_rv1", "h40_rv0"):
        _, humans, robot = S.case_scene(name)
        S.check_scene(humans, robot)
