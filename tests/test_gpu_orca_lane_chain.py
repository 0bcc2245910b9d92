"""-m gpu: orca_lane_kernel<8|20|32> (csrc/orca.h) on the scenes its staged floats and its float filter stand on, bit for bit against the
CPU oracle's ORCA.

The kernel converts every agent's record to float32 once, compares the floats in front of the exact (float64) coincidence test, orders
the neighbours by (key bits, slot) as one integer and fetches the divisor of its pair walk from a lane-computed table.  The scenes of
tests/orca_lane_scene_util.py (tests/test_orca_lane_scenes.py asserts on the CPU what each holds) put neighbours there that are equal as
floats and not as doubles, exactly coincident, or at equal distances; the existing degenerate scenes run at the same shapes.  As in
tests/test_gpu_orca_scenes.py, every env of a batch is loaded with a scene and stepped with a zero action and a parked robot, and the
reference is O.orca_velocity once per agent on the state read from the device before the step.

Shapes: E = 4, H = 5 (network 8); E = 4, H = 20 (network 20; 80 agents: a second, partly filled wavefront that spans env boundaries);
E = 2, H = 31 with a visible robot (network 32, the robot slot); E = 4, H = 20 with randomised attributes (radii from sim_seen).
One natural run, E = 8, H = 20, 40 steps in lock-step with the oracle: collisions (1 / time step) and hand-overs on the way."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import orca_lane_scene_util as L  # noqa: E402
from tests import orca_scene_util as S  # noqa: E402


def _run(name):
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
    c = L.CASES[name]
    E, H = c["E"], c["H"]
    env = HipEnvBatch(A.default_env_config(**L.case_config(name)), E, L.SEED)
    cfg = env.cfg
    env.reset()
    attrs, nds = L.reset_attrs(name)
    h, r = S.read(env)
    np.testing.assert_array_equal(h[:, :, 6:8], attrs)      # radius / v_pref are what the oracle's reset of the same seeds made them
    _, humans, robot = L.case_scene(name)
    h, r = S.inject(env, humans, robot)
    zero = torch.zeros(E, 2, device="cuda")
    dt = float(cfg.time_step)
    compared = 0
    for t in range(c["steps"]):
        _, _, done, _, _, _ = env.step(zero)
        h1, r1 = S.read(env)
        assert not done.cpu().numpy().any(), (name, t)
        np.testing.assert_array_equal(r1[:, 0:2], r[:, 0:2])    # the robot stays parked
        ref = np.stack([S.env_reference(cfg, h[e], r[e], nds[e]) for e in range(E)])
        kept = (h1[:, :, 4:6] == h[:, :, 4:6]).all(axis=2)      # (a human the step sent elsewhere is exempt)
        got = h1[:, :, 2:4].astype(np.float32)
        assert np.array_equal(got.astype(np.float64), h1[:, :, 2:4])
        bad = np.argwhere(kept & (got != ref).any(axis=2))
        print("%s step %d: %d of %d velocities differ%s" % (name, t, len(bad), int(kept.sum()), "".join(" (env %d human %d)" % tuple(b) for b in bad[:8])))
        np.testing.assert_array_equal(got[kept], ref[kept], err_msg="%s step %d" % (name, t))
        moved = h[:, :, 0:2] + h1[:, :, 2:4] * dt
        np.testing.assert_array_equal(h1[:, :, 0:2][kept], moved[kept], err_msg="%s step %d" % (name, t))
        compared += int(kept.sum())
        h, r = h1, r1
    env.close()
    assert compared > E * H * c["steps"] // 2, (compared, E * H * c["steps"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(L.CASES))
def test_the_lane_kernel_matches_the_oracle_on_the_scenes(name):
    _run(name)


@pytest.mark.gpu
def test_a_natural_run_follows_the_oracle_step_by_step():
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
    from tests.test_gpu_env_stream_order import _Replay
    n = L.NATURAL
    steps, hand, coll = L.natural_run()
    assert sum(hand) > 0 and sum(coll) > 0

    class Replay(_Replay):
        def __init__(self):
            self.E, self.way, self.obs, self.steps = n["E"], "plan", None, steps
            self.env = HipEnvBatch(A.default_env_config(**dict(n["kw"], nenv=n["E"])), n["E"], n["seed"])
    r = Replay()
    r.reset()
    r.check(0, n["T"])
    r.env.close()
