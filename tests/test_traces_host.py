"""CPU: the numpy restatements of the trajectory figure and the trace metrics (tests/trace_ref.py) on hand-checked cases, the .npz round trip
of EpisodeTraces, and the binding surface (symbols, no CPU fallback).  The kernels are compared with the restatements in
tests/test_gpu_traces.py."""
import numpy as np
import pytest

from crowdnav_prediction_attngraph_amd import _abi as A
from tests import trace_ref as T

FAR = 100.0     # off-screen


def _block(i0, j0):
    """The 12 pixel centres within 1 of a point midway between four centres whose top-left neighbour is pixel (i0 + 1, j0 + 1): a 4 x 4 block
    without its corners (centre offsets +-0.25 / +-0.75: d2 = 0.125, 0.625, 0.625 <= 1 < 1.125)."""
    return {(i0 + a, j0 + b) for a in range(4) for b in range(4)} - {(i0, j0), (i0, j0 + 3), (i0 + 3, j0), (i0 + 3, j0 + 3)}


def _pixels(img, colour):
    return {tuple(p) for p in np.argwhere((img == np.array(colour, dtype=np.uint8)).all(axis=-1))}


def _hand_made():
    """S = 16, L_w = 4: pitch 0.5, centres at -3.75 + 0.5 j (columns) and 3.75 - 0.5 i (rows), t = 0.75.  One episode of 3 records, A = 3.
    Robot, r = 1 (trail radius 0.4: the 4 centres at d2 = 0.125; outline 0.25 .. 1: the 12 centres of _block), at (-2,2), (0,0), (2,-2).
    Human 1, r = 0.6 (r - t <= 0: a filled outline, d2 <= 0.36: 4 centres; trail radius 0.24: none), resting at (2,2), visible in records 0 and
    1 only.  Human 2: absent, large, on the origin.  Goal on the centre of pixel (row 12, col 3)."""
    agents = np.zeros((1, 4, 3, 6), dtype=np.float32)
    flags = np.zeros((1, 4, 3), dtype=np.uint8)
    for k, (x, y) in enumerate([(-2.0, 2.0), (0.0, 0.0), (2.0, -2.0)]):
        agents[0, k, 0] = [x, y, 1.0, 0.0, 1.0, 0.0]
        agents[0, k, 1] = [2.0, 2.0, 0.0, 0.0, 0.6, 1.0]
        agents[0, k, 2] = [0.0, 0.0, 0.0, 0.0, 3.0, 1.0]
        flags[0, k] = [1, 3 if k < 2 else 1, 0]
    agents[0, 3, 0] = [3.0, 3.0, 0.0, 0.0, 2.0, 0.0]     # beyond the length: never drawn
    flags[0, 3] = [1, 3, 3]
    return agents, flags, np.array([3], dtype=np.int32), np.array([[-2.25, -2.25]], dtype=np.float32)


def test_figure_on_a_16_pixel_image():
    agents, flags, length, goal = _hand_made()
    kw = dict(size=16, half_width=4.0)
    img = T.render_trajectories(agents, flags, length, goal, stride=5, **kw)
    assert img.dtype == np.uint8 and img.shape == (1, 16, 16, 4) and (img[..., 3] == 255).all()
    img = img[0, :, :, :3]
    # shades: D = 2, s = 0, 80, 160.  stride 5 > L: records 0 and 2 (the last) are stamps, record 1 leaves its trail only
    first, mid, last = _block(2, 2), {(7, 7), (7, 8), (8, 7), (8, 8)}, _block(10, 10)
    human = {(3, 11), (3, 12), (4, 11), (4, 12)}
    assert _pixels(img, (255, 215, 0)) == first
    assert _pixels(img, (255, 135, 0)) == mid
    assert _pixels(img, (255, 55, 0)) == last
    assert _pixels(img, (255, 40, 40)) == human           # record 2 (not visible, s = 160) over record 0 (visible, (200,200,255))
    assert _pixels(img, (220, 0, 0)) == {(12, 3)}
    assert len(_pixels(img, (255, 255, 255))) == 256 - 12 - 4 - 12 - 4 - 1
    # stride 1: record 1 is a stamp too -- the robot's outline around the origin; the human's filled outline of record 1 stays under record 2's
    every = T.render_trajectories(agents, flags, length, goal, stride=1, **kw)[0, :, :, :3]
    assert _pixels(every, (255, 135, 0)) == _block(6, 6)
    assert _pixels(every, (255, 40, 40)) == human and _pixels(every, (255, 215, 0)) == first
    # two records: D = 1, the human's last record is a visible one at s = 160
    two = T.render_trajectories(agents, flags, np.array([2], dtype=np.int32), goal, stride=5, **kw)[0, :, :, :3]
    assert _pixels(two, (40, 40, 255)) == human
    assert _pixels(two, (255, 55, 0)) == _block(6, 6) and _pixels(two, (255, 215, 0)) == first
    # no record: white and the goal; a length beyond cap is clamped to cap (record 3: the robot's r = 2 disc shows up)
    none = T.render_trajectories(agents, flags, np.array([0], dtype=np.int32), goal, **kw)[0, :, :, :3]
    assert _pixels(none, (220, 0, 0)) == {(12, 3)} and len(_pixels(none, (255, 255, 255))) == 255
    clamped = T.render_trajectories(agents, flags, np.array([9], dtype=np.int32), goal, **kw)
    assert np.array_equal(clamped, T.render_trajectories(agents, flags, np.array([4], dtype=np.int32), goal, **kw))
    assert tuple(clamped[0, 1, 14, :3]) == (255, 55, 0)     # centre (3.25, 3.25)


def test_metrics_of_a_straight_walk():
    """The robot walks along x at 1 m/s (0.25 m per record) for L = 9 records; human 1 stands 2 m above record 4's position with radius 0.5
    (robot radius 0.25: clearance there 2 - 0.25 - 0.5 = 1.25, all exact in binary), human 2 is present in records 0..2 only, far away."""
    L, cap = 9, 12
    agents = np.zeros((2, cap, 3, 6), dtype=np.float32)
    flags = np.zeros((2, cap, 3), dtype=np.uint8)
    for k in range(cap):
        agents[0, k, 0] = [0.25 * k - 1.0, 0.5, 1.0, 0.0, 0.25, 0.0]
        agents[0, k, 1] = [0.0, 2.5, 0.0, 0.0, 0.5, 1.0]
        agents[0, k, 2] = [50.0, 50.0, 0.0, 0.0, 0.5, 1.0]
        flags[0, k] = [1, 3, 1 if k < 3 else 0]
    m = T.trace_metrics(agents, flags, np.array([L, 0], dtype=np.int32), time_step=0.25, discomfort_dist=0.25)
    got = dict(zip(T.METRICS, m[0]))
    assert got["records"] == L and got["path_length"] == 0.25 * (L - 1) and got["mean_accel"] == 0.0 and got["mean_speed"] == 1.0
    assert got["min_clearance"] == 1.25 and got["intrusion_steps"] == 0 and got["visible_intrusion_steps"] == 0
    assert got["mean_crowd"] == (L + 3) / L
    # episode 1 has no record
    assert m[1].tolist() == [0.0, 0.0, np.inf, 0.0, 0.0, 0.0, 0.0, 0.0]
    # a wider comfort zone: clearance = sqrt(dx^2 + 4) - 0.75 < 1.5 iff |dx| < 1.03..: records 0..8 have dx = -1 .. 1: all nine; the human
    # is visible (bit 1) in all of them.  At 1.3: |dx| < 0.4: records 3, 4, 5
    wide = T.trace_metrics(agents, flags, np.array([L, 0], dtype=np.int32), time_step=0.25, discomfort_dist=1.5)
    assert wide[0, 3] == 9 and wide[0, 4] == 9
    flags[0, 4, 1] = 1       # not visible in record 4
    near = T.trace_metrics(agents, flags, np.array([L, 0], dtype=np.int32), time_step=0.25, discomfort_dist=1.3)
    assert near[0, 3] == 3 and near[0, 4] == 2
    # a turn: the velocity flips from +x to +y between records 8 and 9: |dv| = sqrt(2) once, over 9 intervals of 0.25 s
    agents[0, 9, 0, 2:4] = [0.0, 1.0]
    turn = T.trace_metrics(agents, flags, np.array([10, 0], dtype=np.int32), time_step=0.25, discomfort_dist=0.25)
    assert turn[0, 6] == np.sqrt(np.float64(2.0)) / (9 * 0.25) and turn[0, 1] == 0.25 * 9


def test_episode_traces_round_trip(tmp_path):
    torch = pytest.importorskip("torch")
    from crowdnav_prediction_attngraph_amd.evaluation import EpisodeTraces
    rng = np.random.RandomState(3)
    n, cap, A_ = 2, 5, 4
    cfg = dict(time_step=0.25, discomfort_dist=0.2, robot_radius=0.3, arena_size=6.0, sensor_range=5.0, human_radius=0.35, kinematics=1)
    tr = EpisodeTraces(torch.from_numpy(rng.normal(size=(n, cap, A_, 6)).astype(np.float32)),
                       torch.from_numpy(rng.randint(0, 4, (n, cap, A_)).astype(np.uint8)),
                       torch.from_numpy(rng.normal(size=(n, 2)).astype(np.float32)), torch.tensor([5, 2], dtype=torch.int32),
                       cases=[3, 8], outcome=[3, 1], steps=[5, 2], **cfg)
    path = str(tmp_path / "traces.npz")
    tr.save(path)
    back = EpisodeTraces.load(path)
    for k in ("agents", "flags", "goal", "length"):
        a, b = getattr(tr, k), getattr(back, k)
        assert b.device.type == "cpu" and a.dtype == b.dtype and torch.equal(a, b), k
    assert (back.cases, back.outcome, back.steps) == ([3, 8], [3, 1], [5, 2])
    assert back.config() == cfg and isinstance(back.kinematics, int) and back.n == 2
    with pytest.raises(ValueError):
        EpisodeTraces(tr.agents, tr.flags, tr.goal, tr.length, [3, 8], [3, 1], [5, 2], time_step=0.25)


def test_trace_entry_points_are_bound():
    for name in ("cn_env_trace_append", "cn_trace_metrics", "cn_render_trajectories"):
        assert name in A.ABI_SYMBOLS and hasattr(A.lib(), name)
    from crowdnav_prediction_attngraph_amd import hip_env
    assert hip_env.TRACE_METRICS == T.METRICS


def test_trace_wrappers_have_no_cpu_fallback():
    torch = pytest.importorskip("torch")
    from crowdnav_prediction_attngraph_amd import hip
    ag, fl = torch.zeros(1, 2, 3, 6), torch.zeros(1, 2, 3, dtype=torch.uint8)
    ln, goal = torch.ones(1, dtype=torch.int32), torch.zeros(1, 2)
    with pytest.raises(A.CnError, match="no CPU fallback"):
        hip.trace_metrics(ag, fl, ln)
    with pytest.raises(A.CnError, match="no CPU fallback"):
        hip.render_trajectories(ag, fl, ln, goal, size=16)
    with pytest.raises(A.CnError, match="no CPU fallback"):
        hip.HipEnvBatch.trace_append(type("E", (), dict(E=1, H=2))(), None, torch.zeros(1, dtype=torch.int64),
                                     type("Tr", (), dict(agents=ag, flags=fl, goal=goal, length=ln))())
