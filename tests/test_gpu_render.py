"""-m gpu: the rasteriser kernel (cn_render_scenes) and everything built on it against the float32 restatement of the drawing rule
(tests/render_ref.py).  Every image comparison is ALL PIXELS EQUAL: the rule has no rounding freedom."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import render_ref as R  # noqa: E402


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu(size, half_width, humans, robot, **kw):
    from crowdnav_prediction_attngraph_amd import hip
    rest = {k: kw.pop(k) for k in ("robot_radius", "ring_radius") if k in kw}
    return hip.render_scenes(_dev(humans), _dev(robot), size=size, half_width=half_width, **rest, **{k: _dev(v) for k, v in kw.items()}).cpu().numpy()


def _same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    bad = (got != want).any(axis=-1)
    assert not bad.any(), "%d of %d pixels differ, first at (image, row, col) %s: %s instead of %s" % (
        bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


def _synthetic():
    """n = 3, H = 5, counts (5, 3, 0), L = 7.  Env 0: a human overlapping the robot, one straddling the right edge, one fully outside, one of
    radius 0.05, one at rest; goal on-screen; heading given.  Env 1: robot in the top-left corner (ring partly outside), zero heading, 7
    dots; its slots 3, 4 hold large humans that must not appear.  Env 2: no human, 1 dot."""
    humans = np.zeros((3, 5, 8))
    humans[0] = [[1.2, -0.4, 0.5, -0.5, 0, 0, 0.3, 1.0], [6.9, 2.0, 1.0, 0.0, 0, 0, 0.45, 1.0], [9.5, 0.0, -1.0, 0.2, 0, 0, 0.3, 1.0],
                 [-3.0, -3.0, 0.0, 0.2, 0, 0, 0.05, 1.0], [-2.0, 4.0, 0.0, 0.0, 0, 0, 0.35, 1.0]]
    humans[1] = [[-4.9, 4.1, -0.3, 0.8, 0, 0, 0.3, 1.0], [0.13, 0.27, 0.7, 0.7, 0, 0, 0.5, 1.0], [3.3, -6.95, 0.0, -1.0, 0, 0, 0.4, 1.0],
                 [0.0, 0.0, 1.0, 1.0, 0, 0, 3.0, 1.0], [-1.0, -2.0, -1.0, 0.5, 0, 0, 2.5, 1.0]]
    humans[2] = [[1.0, 1.0, 0.5, 0.5, 0, 0, 2.0, 1.0]] * 5
    robot = np.array([[1.0, -0.5, 0.3, 0.1, 3.0, 4.0, 0.4, 0.0], [-5.5, 5.0, -0.2, 0.6, 5.0, -5.0, 2.0, 0.0], [0.0, 0.0, 0.0, 0.0, -6.9, 6.9, 0.0, 0.0]])
    counts = np.array([5, 3, 0], dtype=np.int32)
    visible = np.array([[1, 0, 1, 1, 0], [0, 1, 1, 1, 1], [1, 1, 1, 1, 1]], dtype=np.uint8)
    heading = np.array([[0.0, 1.5], [0.0, 0.0], [-1.0, -1.0]], dtype=np.float32)
    rng = np.random.RandomState(5)
    dots = rng.uniform(-7.2, 7.2, (3, 8, 2)).astype(np.float32)
    dots[1, 0] = [-5.5, 5.0]          # under the robot
    dots[1, 1] = [0.13, 0.9]          # on a human's outline
    dot_counts = np.array([0, 7, 1], dtype=np.int32)
    return humans, robot, dict(counts=counts, visible=visible, robot_heading=heading, dots=dots, dot_counts=dot_counts)


@pytest.mark.parametrize("size", [16, 48, 64])
def test_synthetic_scenes_equal_the_restatement(size):
    humans, robot, opt = _synthetic()
    kw = dict(robot_radius=0.3, ring_radius=5.6)
    full = _gpu(size, 7.0, humans, robot, **opt, **kw)
    _same(full, R.render_scenes(humans, robot, size=size, half_width=7.0, **opt, **kw))
    assert (full[..., 3] == 255).all()
    for drop in (("counts",), ("visible",), ("dots", "dot_counts"), ("robot_heading",)):
        o = {k: v for k, v in opt.items() if k not in drop}
        _same(_gpu(size, 7.0, humans, robot, **o, **kw), R.render_scenes(humans, robot, size=size, half_width=7.0, **o, **kw))
    # and without the ring
    _same(_gpu(size, 7.0, humans, robot, **opt, robot_radius=0.3, ring_radius=0.0),
          R.render_scenes(humans, robot, size=size, half_width=7.0, robot_radius=0.3, ring_radius=0.0, **opt))


def _random_scenes(n, H, seed):
    rng = np.random.RandomState(seed)
    humans = np.zeros((n, H, 8))
    humans[:, :, 0:2] = rng.uniform(-7.5, 7.5, (n, H, 2))
    humans[:, :, 2:4] = rng.uniform(-1, 1, (n, H, 2))
    humans[:, :, 6] = rng.uniform(0.05, 0.7, (n, H))
    robot = np.zeros((n, 8))
    robot[:, 0:2] = rng.uniform(-6, 6, (n, 2))
    robot[:, 2:4] = rng.uniform(-1, 1, (n, 2))
    robot[:, 4:6] = rng.uniform(-7, 7, (n, 2))
    return humans, robot


@pytest.mark.parametrize("n,H", [(1, 5), (70, 64), (70, 1)])
def test_indexing_and_guard_words(n, H):
    from crowdnav_prediction_attngraph_amd import hip
    S = 16
    humans, robot = _random_scenes(n, H, 100 + H)
    guard = 64 * 4                                   # 64 words before and after the images
    buf = torch.full((guard + n * S * S * 4 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[guard:guard + n * S * S * 4].view(n, S, S, 4)
    ret = hip.render_scenes(_dev(humans), _dev(robot), robot_radius=0.3, ring_radius=5.6, size=S, half_width=7.0, out=out)
    assert ret.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:guard] == 0xA5).all() and (host[-guard:] == 0xA5).all()
    _same(host[guard:-guard].reshape(n, S, S, 4), R.render_scenes(humans, robot, robot_radius=0.3, ring_radius=5.6, size=S, half_width=7.0))


def test_seventy_thousand_scenes_index_correctly():
    """70 000 images of 16 x 16 (one workgroup each, 72 MB): 70 distinct scenes repeated 1000 times, compared on the device."""
    from crowdnav_prediction_attngraph_amd import hip
    S, n0, rep = 16, 70, 1000
    humans, robot = _random_scenes(n0, 1, 7)
    want = torch.from_numpy(R.render_scenes(humans, robot, robot_radius=0.3, ring_radius=5.6, size=S, half_width=7.0)).cuda().repeat(rep, 1, 1, 1)
    got = hip.render_scenes(_dev(np.tile(humans, (rep, 1, 1))), _dev(np.tile(robot, (rep, 1))), robot_radius=0.3, ring_radius=5.6, size=S, half_width=7.0)
    assert got.shape == (n0 * rep, S, S, 4) and torch.equal(got, want)


def test_culling_never_drops_a_shape():
    """64 humans and 1024 dots: half of the dots on a jittered grid, half in a cluster, so most 32 x 32 tiles see few shapes and a few see
    hundreds (several staging rounds)."""
    rng = np.random.RandomState(21)
    g = (np.stack(np.meshgrid(np.arange(8), np.arange(8)), -1).reshape(64, 2) + 0.5) * (13.0 / 8) - 6.5
    humans = np.zeros((1, 64, 8))
    humans[0, :, 0:2] = g + rng.uniform(-0.6, 0.6, (64, 2))
    humans[0, :, 2:4] = rng.uniform(-1, 1, (64, 2))
    humans[0, :, 6] = rng.uniform(0.05, 0.8, 64)
    robot = np.array([[0.4, -0.7, 0.5, 0.2, -3.0, 2.0, 0.0, 0.0]])
    d = (np.stack(np.meshgrid(np.arange(32), np.arange(16)), -1).reshape(512, 2) + 0.5) * [14.0 / 32, 14.0 / 16] - 7.0
    dots = np.concatenate([d + rng.uniform(-0.2, 0.2, (512, 2)), rng.normal([2.0, 2.0], 0.5, (512, 2))])[None].astype(np.float32)
    visible = (rng.uniform(size=(1, 64)) < 0.5).astype(np.uint8)
    kw = dict(robot_radius=0.3, ring_radius=5.6)
    opt = dict(visible=visible, dots=dots, dot_counts=np.array([1024], dtype=np.int32))
    _same(_gpu(128, 7.0, humans, robot, **opt, **kw), R.render_scenes(humans, robot, size=128, half_width=7.0, **opt, **kw))


def _env_batch(seed, E, **kw):
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
    return HipEnvBatch(A.default_env_config(nenv=E, **kw), E, seed)


def _restated_frame(env, size, dots=None, dot_counts=None):
    cfg = env.cfg
    humans, robot = (t.cpu().numpy() for t in env.get_state())
    counts, visible = env.get_human_counts().cpu().numpy(), env.get_visibility().cpu().numpy()
    if cfg.kinematics == 0:
        heading = robot[:, 2:4].astype(np.float32)
    else:     # as HipEnvBatch.render: cos / sin of theta by torch, in fp64, rounded to fp32
        th = torch.from_numpy(robot[:, 6]).cuda()
        heading = torch.stack((torch.cos(th), torch.sin(th)), dim=1).to(torch.float32).cpu().numpy()
    assert (visible[np.arange(env.H)[None, :] >= counts[:, None]] == 0).all()
    return R.render_scenes(humans, robot, counts=counts, visible=visible, robot_heading=heading, dots=dots, dot_counts=dot_counts,
                           robot_radius=cfg.robot_radius, ring_radius=cfg.sensor_range + cfg.robot_radius + cfg.human_radius, size=size,
                           half_width=cfg.arena_size + 1.0), counts


@pytest.mark.parametrize("name,kw", [("varnum", dict(human_num=5)), ("varnum_range2", dict(human_num=5, human_num_range=2)),
                                     ("pred_unicycle", dict(human_num=5, env_kind=1, kinematics=1))])
def test_env_render_equals_the_restatement_and_leaves_the_env_alone(name, kw):
    """After every step env.render(size=64) equals the restatement applied to get_state / get_human_counts / get_visibility, and a second
    batch with the same seed that never renders produces bit-identical observations, rewards and dones."""
    from crowdnav_prediction_attngraph_amd import hip
    E, T, seed = 6, 12, 31
    env, twin = _env_batch(seed, E, **kw), _env_batch(seed, E, **kw)
    with_dots = kw.get("env_kind") == 1
    acts = torch.from_numpy(np.random.RandomState(seed).uniform(-1, 1, (T, E, 2)).astype(np.float32)).cuda()
    if kw.get("kinematics"):
        acts = acts * 0.1
    obs, tobs = env.reset(), twin.reset()
    seen_counts = set()
    for t in range(T + 1):
        dots = counts_d = None
        if with_dots:
            dots, counts_d = hip.prediction_dots(obs)
            se, rn = obs["spatial_edges"].cpu().numpy(), obs["robot_node"].cpu().numpy()
            want_dots = (se[:, :, 2:].reshape(E, -1, 2) + rn[:, :, 0:2]).astype(np.float32)
            assert np.array_equal(dots.cpu().numpy(), want_dots)
            assert np.array_equal(counts_d.cpu().numpy(), (obs["detected_human_num"].cpu().numpy().reshape(E) * 5).astype(np.int32))
        img = env.render(size=64, dots=dots, dot_counts=counts_d)
        assert img.shape == (E, 64, 64, 4) and img.dtype == torch.uint8 and img.is_cuda
        want, counts = _restated_frame(env, 64, None if dots is None else dots.cpu().numpy(), None if dots is None else counts_d.cpu().numpy())
        _same(img.cpu().numpy(), want)
        seen_counts.update(counts.tolist())
        for k in ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num"):
            assert torch.equal(obs[k], tobs[k]), (k, t)
        if t == T:
            break
        obs, rew, done, info, _, _ = env.step(acts[t])
        tobs, trew, tdone, tinfo, _, _ = twin.step(acts[t])
        assert torch.equal(rew, trew) and torch.equal(done, tdone) and torch.equal(info, tinfo), t
    if kw.get("human_num_range"):
        assert min(seen_counts) < env.H, "no env with a free slot: the count path was not exercised"
    # a subset, in the caller's order
    sub = env.render(size=64, env_ids=[4, 1], dots=None if dots is None else dots[[4, 1]].contiguous(),
                     dot_counts=None if dots is None else counts_d[[4, 1]].contiguous())
    assert torch.equal(sub, img[[4, 1]])
    env.close()
    twin.close()


def test_get_visibility_is_the_reference_decision():
    """E = 8, H = 20, 20 steps of seeded random actions: get_visibility equals the fp64 form of detect_visible(robot, human, robot1=True) on
    get_state(): norm - r1 - r2 <= sensor_range (FOV = 2 pi: no cone test).  No pair is excluded.  Seed 13 was picked with the C oracle on the
    CPU (same seeds and actions, sensor range widened so that the observation shows every human, which does not change the trajectories):
    the smallest |norm - r1 - r2 - sensor_range| over all 8 x 20 x 21 pairs is 6.05e-4 (seeds 11, 12, 14: 3.9e-4, 3.1e-4, 2.5e-4), so no
    pair comes anywhere near 1e-9 of the threshold -- asserted again here on the fp64 state."""
    E, H, T, seed = 8, 20, 20, 13
    env = _env_batch(seed, E, human_num=H, sort_humans=0)
    acts = torch.from_numpy(np.random.RandomState(seed).uniform(-1, 1, (T, E, 2)).astype(np.float32)).cuda()
    env.reset()
    margin, n_vis, n_inv = np.inf, 0, 0
    for t in range(T + 1):
        humans, robot = (x.cpu().numpy() for x in env.get_state())
        dx, dy = robot[:, None, 0] - humans[:, :, 0], robot[:, None, 1] - humans[:, :, 1]
        gap = np.sqrt(dx * dx + dy * dy) - env.cfg.robot_radius - humans[:, :, 6]
        want = ~((dx == 0) & (dy == 0)) & (gap <= env.cfg.sensor_range)
        margin = min(margin, np.abs(gap - env.cfg.sensor_range).min())
        got = env.get_visibility().cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8)), t
        n_vis, n_inv = n_vis + int(want.sum()), n_inv + int((~want).sum())
        if t < T:
            env.step(acts[t])
    print("smallest |norm - r1 - r2 - sensor_range| = %.3e; %d visible, %d invisible pairs" % (margin, n_vis, n_inv))
    assert margin > 1e-9 and n_vis > 0 and n_inv > 0
    env.close()


def test_vec_env_surface():
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
    dev = torch.device("cuda", 0)
    envs = make_vec_envs("CrowdSimVarNum-v0", 3, 5, 0.99, None, dev, True, config=C.non_randomized(**{"sim.human_num": 5}))
    envs.reset()
    envs.step(torch.zeros(5, 2, device=dev))
    imgs = envs.get_images(size=32)
    assert isinstance(imgs, np.ndarray) and imgs.shape == (5, 32, 32, 3) and imgs.dtype == np.uint8
    assert np.array_equal(imgs, envs._env.render(size=32)[..., :3].cpu().numpy())
    assert np.array_equal(envs.get_images(size=32, env_ids=[3, 0]), imgs[[3, 0]])
    mosaic = envs.render(mode="rgb_array", size=32)
    assert mosaic.shape == (3 * 32, 2 * 32, 3) and mosaic.dtype == np.uint8           # ceil(sqrt(5)) = 3 rows x ceil(5 / 3) = 2 columns
    for k in range(6):
        tile = mosaic[(k // 2) * 32:(k // 2 + 1) * 32, (k % 2) * 32:(k % 2 + 1) * 32]
        assert np.array_equal(tile, imgs[k]) if k < 5 else (tile == 0).all()
    assert envs.render(mode="rgb_array", size=32, max_envs=2).shape == (2 * 32, 1 * 32, 3)
    for call in (lambda: envs.render(), lambda: envs.render("human"), lambda: envs.render(mode="human")):
        with pytest.raises(NotImplementedError, match="rendering is out of scope of the accelerated path"):
            call()
    envs.close()


def test_vec_env_draws_the_predictions_of_its_last_observation():
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd import hip
    from crowdnav_prediction_attngraph_amd.vec_env import make_vec_envs
    dev = torch.device("cuda", 0)
    envs = make_vec_envs("CrowdSimPred-v0", 3, 4, 0.99, None, dev, True, config=C.non_randomized(**{"sim.human_num": 5, "sim.predict_method": "const_vel"}))
    envs.reset()
    for _ in range(24):          # 6 s: the humans start on a circle outside the view and the sensor range and walk across it
        obs, _, _, _ = envs.step(torch.zeros(4, 2, device=dev))
    dots, counts = hip.prediction_dots({k: obs[k] for k in ("spatial_edges", "robot_node", "detected_human_num")})
    with_dots = envs.get_images(size=64)
    assert np.array_equal(with_dots, envs._env.render(size=64, dots=dots, dot_counts=counts)[..., :3].cpu().numpy())
    without = envs.get_images(size=64, predictions=False)
    assert np.array_equal(without, envs._env.render(size=64)[..., :3].cpu().numpy())
    green = (with_dots == np.array(R.GREEN, dtype=np.uint8)).all(axis=-1)
    assert green.any() and not (without == np.array(R.GREEN, dtype=np.uint8)).all(axis=-1).any()
    envs.close()


def test_gym_env_renders_an_rgb_array():
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd import gym_env
    env = gym_env.CrowdSimVarNum()
    env.configure(C.non_randomized(**{"sim.human_num": 5}))
    env.reset()
    env.step(np.array([0.5, 0.1], dtype=np.float32))
    img = env.render(mode="rgb_array", size=48)
    assert isinstance(img, np.ndarray) and img.shape == (48, 48, 3) and img.dtype == np.uint8
    assert np.array_equal(img, env._env.render(size=48)[0, :, :, :3].cpu().numpy())
    assert (img == np.array(R.GOLD, dtype=np.uint8)).all(axis=-1).any()
    with pytest.raises(NotImplementedError):
        env.render()
    env.close()


def test_render_episodes():
    """ORCA robot, 5 non-randomised humans, cases 0, 3 and 4 at 64 x 64."""
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.evaluation import _evaluate_batched, render_episodes
    from crowdnav_prediction_attngraph_amd.config import to_env_config
    from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
    cfg = C.non_randomized(**{"sim.human_num": 5, "robot.policy": "orca"})
    cases, seed, S = [0, 3, 4], 7, 64
    ep = render_episodes(None, "CrowdSimVarNum-v0", cfg, seed, cases, size=S)
    per_env = {}
    _evaluate_batched(None, "CrowdSimVarNum-v0", cfg, seed, cases, per_env=per_env)
    assert per_env["cases"] == cases and sorted(ep) == cases
    # a fresh batch's reset frames of the same cases
    env = HipEnvBatch(to_env_config(cfg, "CrowdSimVarNum-v0", 1, "test"), len(cases), seed)
    env.set_case_counters(torch.tensor([c - e for e, c in enumerate(cases)], dtype=torch.int64))
    env.reset()
    first = env.render(size=S)[..., :3].cpu().numpy()
    env.close()
    for e, c in enumerate(cases):
        r = ep[c]
        assert r["outcome"] == per_env["outcome"][e] and r["steps"] == per_env["steps"][e] and r["outcome"] in (1, 2, 3)
        assert r["frames"].shape == (r["steps"] + 1, S, S, 3) and r["frames"].dtype == np.uint8
        assert np.array_equal(r["frames"][0], first[e])
        assert (r["frames"][1] != r["frames"][0]).any()
    with pytest.raises(ValueError, match="1024"):
        render_episodes(None, "CrowdSimVarNum-v0", cfg, seed, list(range(501)), size=1024)
