"""orca_lane_kernel<8|20|32>, orca_lp3_kernel and the cooperative orca_kernel (csrc/orca.h) on injected degenerate crowds, bit for bit
against the CPU oracle's ORCA.

The other ORCA tests follow trajectories the simulator produces, and those never hold a distance tie, an agent on its goal or a full
hand-over list, and hardly ever two parallel lines.  Here every env of a batch is loaded with a hand-built scene
(tests/orca_scene_util.py; tests/test_orca_scenes.py asserts on the CPU what each holds) and stepped with a zero action and a parked
robot: the velocities of the state after a step are the ORCA pass's output for the state before it.  The reference is O.orca_velocity
once per agent on the state READ FROM THE DEVICE before the step, so a case follows its degenerate start for 8 steps as rounding
breaks the symmetry, without an oracle env in lockstep.  Compared with assert_array_equal as float32; the positions must have moved by
v * time_step in the oracle's own float64 expression.  A human the step replaced or sent elsewhere (its goal changed) is exempt."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import orca_scene_util as S  # noqa: E402


def _batch(name):
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
    c = S.CASES[name]
    old = os.environ.get("CN_LP3_BLOCKS")
    if "lp3_blocks" in c:
        os.environ["CN_LP3_BLOCKS"] = str(c["lp3_blocks"])      # read when the batch is created
    try:
        env = HipEnvBatch(A.default_env_config(**S.case_config(name)), c["E"], S.SEED)
    finally:
        if "lp3_blocks" in c:
            if old is None:
                del os.environ["CN_LP3_BLOCKS"]
            else:
                os.environ["CN_LP3_BLOCKS"] = old
    return env


def _run(name):
    c = S.CASES[name]
    E, H = c["E"], c["H"]
    env = _batch(name)
    cfg = env.cfg
    env.reset()
    attrs, nds = S.oracle_reset_attrs(name)
    h, r = S.read(env)
    # the reference takes radius / v_pref from the state: they are what the oracle's reset of the same seeds made them
    np.testing.assert_array_equal(h[:, :, 6:8], attrs)
    _, humans, robot = S.case_scene(name)
    h, r = S.inject(env, humans, robot)
    zero = torch.zeros(E, 2, device="cuda")
    dt = float(cfg.time_step)
    exempt = 0
    for t in range(c["steps"]):
        _, _, done, _, _, _ = env.step(zero)
        h1, r1 = S.read(env)
        assert not done.cpu().numpy().any(), (name, t)          # a finished episode would have replaced the state
        np.testing.assert_array_equal(r1[:, 0:2], r[:, 0:2])    # the robot stays parked
        ref = np.stack([S.env_reference(cfg, h[e], r[e], nds[e]) for e in range(E)])
        kept = (h1[:, :, 4:6] == h[:, :, 4:6]).all(axis=2)
        exempt += int((~kept).sum())
        got = h1[:, :, 2:4].astype(np.float32)
        assert np.array_equal(got.astype(np.float64), h1[:, :, 2:4])      # the state's velocities are widened float32
        bad = np.argwhere(kept & (got != ref).any(axis=2))
        print("%s step %d: %d of %d velocities differ%s" % (name, t, len(bad), int(kept.sum()), "".join(" (env %d human %d)" % tuple(b) for b in bad[:8])))
        np.testing.assert_array_equal(got[kept], ref[kept], err_msg="%s step %d" % (name, t))
        moved = h[:, :, 0:2] + h1[:, :, 2:4] * dt                # agent.py:143-183 on float64 records
        np.testing.assert_array_equal(h1[:, :, 0:2][kept], moved[kept], err_msg="%s step %d" % (name, t))
        np.testing.assert_array_equal(h1[:, :, 6:8][kept], h[:, :, 6:8][kept])     # (a respawn with randomised attributes draws new ones)
        h, r = h1, r1
    env.close()
    return exempt, E * H * c["steps"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, c in S.CASES.items() if c["kind"] == "scenes" and not c["cfg"]])
def test_every_dispatch_shape_matches_the_oracle_on_the_scenes(name):
    exempt, total = _run(name)
    assert exempt < total // 2, (exempt, total)     # respawns on arrival (end_goal_changing) stay the exception


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, c in S.CASES.items() if c["cfg"].get("end_goal_changing") == 0])
def test_agents_on_their_goal_keep_the_oracles_velocity(name):
    """end_goal_changing off: nobody is respawned on arrival, so every agent of every step is compared -- the ones with a zero preferred
    velocity included."""
    exempt, _ = _run(name)
    assert exempt == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["full_odd", "full_one_block"])
def test_a_full_hand_over_list_is_solved(name):
    """Every agent of every env infeasible in the injected state (tests/test_orca_scenes.py): E * H list entries, an odd number, or walked
    by one workgroup."""
    _run(name)


@pytest.mark.gpu
def test_randomised_attributes_use_the_frozen_radii_and_speed_limits():
    _run("random_attrs")
