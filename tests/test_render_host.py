"""CPU: the float32 restatement of the drawing rule (tests/render_ref.py) on hand-checked scenes, and the binding surface of the
rasteriser (symbols, ABI version, no CPU fallback).  The kernel itself is compared with the restatement in tests/test_gpu_render.py."""
import numpy as np
import pytest

from crowdnav_prediction_attngraph_amd import _abi as A
from tests import render_ref as R

FAR = 100.0     # off-screen


def _robot(px=0.0, py=0.0, vx=0.0, vy=0.0, gx=FAR, gy=FAR):
    return np.array([[px, py, vx, vy, gx, gy, 0.0, 0.0]], dtype=np.float64)


def _human(px, py, vx=0.0, vy=0.0, r=0.3):
    return np.array([[[px, py, vx, vy, 0.0, 0.0, r, 1.0]]], dtype=np.float64)


def _rgb(img):
    assert img.dtype == np.uint8 and (img[..., 3] == 255).all()
    return img[0, :, :, :3]


def _is(img, colour):
    return (img == np.array(colour, dtype=np.uint8)).all(axis=-1)


def test_robot_disc_on_a_16_pixel_image():
    """S = 16, L = 4: pitch 0.5, pixel centres at -3.75 + 0.5 j (columns) and 3.75 - 0.5 i (rows).  A disc of radius 1 at the origin holds
    the centres (+-0.25, +-0.25) [d2 = 0.125] and (+-0.25, +-0.75), (+-0.75, +-0.25) [d2 = 0.625]; (+-0.75, +-0.75) has d2 = 1.125 > 1."""
    img = _rgb(R.render_scenes(_human(FAR, FAR), _robot(), counts=np.array([0]), robot_radius=1.0, ring_radius=0.0, size=16, half_width=4.0))
    gold = {(i, j) for i in (6, 7, 8, 9) for j in (6, 7, 8, 9)} - {(6, 6), (6, 9), (9, 6), (9, 9)}
    assert len(gold) == 12
    assert {tuple(p) for p in np.argwhere(_is(img, R.GOLD))} == gold
    assert _is(img, R.WHITE).sum() == 256 - 12


def test_layers_are_painted_in_order():
    """Pixel (row 7, col 9) has its centre at (0.75, 0.25), 0.79 from the origin: on a ring of radius 0.9 (w = 0.25: 0.65 .. 1.15) around a
    robot at the origin, and inside a goal diamond, a dot and a small (filled) human all centred on it."""
    P = (7, 9)
    kw = dict(size=16, half_width=4.0, ring_radius=0.9)
    none = dict(counts=np.array([0]))
    dots = np.array([[[0.75, 0.25]]], dtype=np.float32)
    tiny = 0.01     # a robot that covers no pixel centre
    img = _rgb(R.render_scenes(_human(0.75, 0.25), _robot(), robot_radius=tiny, **none, **kw))
    assert tuple(img[P]) == R.GREY
    img = _rgb(R.render_scenes(_human(0.75, 0.25), _robot(gx=0.75, gy=0.25), robot_radius=tiny, **none, **kw))
    assert tuple(img[P]) == R.GOAL
    img = _rgb(R.render_scenes(_human(0.75, 0.25), _robot(gx=0.75, gy=0.25), robot_radius=tiny, dots=dots, dot_counts=np.array([1]), **none, **kw))
    assert tuple(img[P]) == R.GREEN
    img = _rgb(R.render_scenes(_human(0.75, 0.25), _robot(gx=0.75, gy=0.25), robot_radius=tiny, dots=dots, dot_counts=np.array([1]), **kw))
    assert tuple(img[P]) == R.BLUE
    img = _rgb(R.render_scenes(_human(0.75, 0.25), _robot(gx=0.75, gy=0.25), robot_radius=tiny, dots=dots, dot_counts=np.array([1]),
                               visible=np.array([[0]], dtype=np.uint8), **kw))
    assert tuple(img[P]) == R.RED
    img = _rgb(R.render_scenes(_human(0.75, 0.25), _robot(gx=0.75, gy=0.25), robot_radius=1.0, dots=dots, dot_counts=np.array([1]), **kw))
    assert tuple(img[P]) == R.GOLD
    # the robot's heading mark goes over its disc: heading +x from the origin covers the centres (0.25, +-0.25) and (0.75, +-0.25)
    # (|cr| = 0.25 <= hw = 0.375, 0 <= dot <= 1)
    img = _rgb(R.render_scenes(_human(0.75, 0.25), _robot(gx=0.75, gy=0.25), robot_radius=1.0, robot_heading=np.array([[2.0, 0.0]], dtype=np.float32), **kw))
    assert {tuple(p) for p in np.argwhere(_is(img, R.DARK))} == {(7, 8), (8, 8), (7, 9), (8, 9)}


def test_a_slot_beyond_the_count_is_not_drawn():
    kw = dict(robot_radius=0.01, size=16, half_width=4.0)
    assert _is(_rgb(R.render_scenes(_human(0.25, 0.25, r=0.6), _robot(), counts=np.array([1]), **kw)), R.BLUE).any()
    assert _is(_rgb(R.render_scenes(_human(0.25, 0.25, r=0.6), _robot(), counts=np.array([0]), **kw)), R.WHITE).all()


def test_a_thin_human_is_filled_and_a_large_one_is_an_outline():
    """t = 1.5 q = 0.75: r = 0.6 gives r - t <= 0, a filled disc; r = 2 leaves a hole of radius 1.25."""
    kw = dict(robot_radius=0.01, size=16, half_width=4.0)
    small = _rgb(R.render_scenes(_human(0.25, 0.25, r=0.6), _robot(), **kw))
    assert tuple(small[7, 8]) == R.BLUE
    large = _rgb(R.render_scenes(_human(0.25, 0.25, r=2.0), _robot(), **kw))
    assert tuple(large[7, 8]) == R.WHITE and tuple(large[7, 11]) == R.BLUE       # centre (1.75, 0.25): 1.5 from the human's centre


def test_a_human_at_rest_has_no_heading_mark():
    kw = dict(robot_radius=0.01, size=16, half_width=4.0)
    assert not _is(_rgb(R.render_scenes(_human(0.25, 0.25, r=1.0), _robot(), **kw)), R.DARK).any()
    assert not _is(_rgb(R.render_scenes(_human(0.25, 0.25, vx=1e-7, vy=0.0, r=1.0), _robot(), **kw)), R.DARK).any()     # s2 = 1e-14 <= 1e-12
    moving = _rgb(R.render_scenes(_human(0.25, 0.25, vx=0.0, vy=-1.0, r=1.0), _robot(), **kw))
    assert {tuple(p) for p in np.argwhere(_is(moving, R.DARK))} == {(7, 8), (8, 8), (9, 8)}      # downwards: dot = 0, 0.5, 1.0 <= r


def test_render_entry_points_are_bound():
    assert "cn_render_scenes" in A.ABI_SYMBOLS and "cn_env_get_visibility" in A.ABI_SYMBOLS
    assert A.ABI_VERSION == 407
    lib = A.lib()
    assert lib.cn_version() == 407 and hasattr(lib, "cn_render_scenes") and hasattr(lib, "cn_env_get_visibility")


def test_render_scenes_has_no_cpu_fallback():
    torch = pytest.importorskip("torch")
    from crowdnav_prediction_attngraph_amd import hip
    with pytest.raises(A.CnError, match="no CPU fallback"):
        hip.render_scenes(torch.zeros(1, 1, 8, dtype=torch.float64), torch.zeros(1, 8, dtype=torch.float64), size=16)
