"""Host side of cn_env_set_scene / HipEnvBatch.set_scene: no GPU needed.  The call is in header, library and binding; it refuses NULL
arguments by name before it looks at the handle (so the refusals are the same on a box with or without a GPU); and the refusals of
set_scene(check=True) -- shapes, dtypes, devices, non-finite values, foreign radius / v_pref columns -- are decided by functions that take
host arrays."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402
from crowdnav_prediction_attngraph_amd import hip_env as HE  # noqa: E402
from crowdnav_prediction_attngraph_amd import scenes as SC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_call_is_declared_exported_and_bound():
    lib = A.lib()
    hdr = open(os.path.join(ROOT, "include", "crowdnav_hip.h")).read()
    assert "cn_env_set_scene" in A.ABI_SYMBOLS and hasattr(lib, "cn_env_set_scene") and "int cn_env_set_scene(" in hdr
    assert lib.cn_version() == A.ABI_VERSION == 407          # an addition: the version stays


def test_null_arguments_are_refused_by_name_before_the_handle_is_read():
    """CN_ERR_INVALID (-1) naming the call.  The handle is a dummy that is never dereferenced: a NULL humans / robot / obs is found first."""
    lib = A.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    null = C.c_void_p(0)
    obs = A.Obs()
    for name in ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num"):
        setattr(obs, name, p)
    empty = A.Obs()                                           # every member NULL
    for args in ((null, null, p, p, C.byref(obs), null),      # handle
                 (p, null, null, p, C.byref(obs), null),      # humans
                 (p, null, p, null, C.byref(obs), null),      # robot
                 (p, null, p, p, None, null),                 # obs
                 (p, null, p, p, C.byref(empty), null)):      # obs without its required members
        assert lib.cn_env_set_scene(*args) == -1
        assert b"cn_env_set_scene" in lib.cn_last_error(), lib.cn_last_error()


def _good(E=3, H=4):
    humans = torch.zeros(E, H, 8, dtype=torch.float64)
    humans[:, :, 6], humans[:, :, 7] = 0.3, 1.0
    return humans, torch.zeros(E, 8, dtype=torch.float64)


def test_wrong_shapes_dtypes_and_devices_are_refused_by_argument():
    E, H = 3, 4
    humans, robot = _good(E, H)
    HE.check_scene_tensors(humans, robot, None, E, H, "cpu")
    HE.check_scene_tensors(humans, robot, torch.ones(E, dtype=torch.uint8), E, H, "cpu")
    for bad, match in (((humans[:, :, :6], robot, None), "humans must have shape"), ((humans, robot[:, :7], None), "robot must have shape"),
                       ((humans.float(), robot, None), "humans must be torch.float64"), ((humans.numpy(), robot, None), "humans must be a torch tensor"),
                       ((humans, robot, torch.ones(E + 1, dtype=torch.uint8)), "select must have shape"),
                       ((humans, robot, torch.ones(E, dtype=torch.int64)), "select must be torch.uint8")):
        with pytest.raises(ValueError, match=match):
            HE.check_scene_tensors(*bad, E, H, "cpu")
    with pytest.raises(ValueError, match="humans must live on cuda:0"):      # CPU tensors offered to a batch on a GPU
        HE.check_scene_tensors(humans, robot, None, E, H, "cuda:0")


def test_values_are_refused_naming_env_and_slot():
    E, H = 3, 4
    humans, robot = (t.numpy() for t in _good(E, H))
    own = humans[:, :, 6:8].copy()
    counts = np.array([4, 2, 4])
    HE.check_scene_values(humans, robot, own, counts)
    h = humans.copy(); h[2, 1, 4] = np.nan
    with pytest.raises(ValueError, match=r"env 2 human slot 1: gx is nan"):
        HE.check_scene_values(h, robot, own, counts)
    HE.check_scene_values(h, robot, own, counts, selected=np.array([True, True, False]))      # an env that is not selected is not looked at
    h = humans.copy(); h[1, 3, 0] = np.inf                                                    # slot 3 of env 1 holds no human (crowd of 2)
    HE.check_scene_values(h, robot, own, counts)
    r = robot.copy(); r[0, 6] = -np.inf
    with pytest.raises(ValueError, match=r"env 0 robot: theta is -inf"):
        HE.check_scene_values(humans, r, own, counts)
    r = robot.copy(); r[0, 7] = np.nan                                                        # the potential is not taken
    HE.check_scene_values(humans, r, own, counts)
    h = humans.copy(); h[0, 2, 6] = 0.35
    with pytest.raises(ValueError, match=r"env 0 human slot 2: radius is 0.35, the env's own is 0.3"):
        HE.check_scene_values(h, robot, own, counts)
    h = humans.copy(); h[2, 0, 7] = 1.5
    with pytest.raises(ValueError, match=r"env 2 human slot 0: v_pref is 1.5, the env's own is 1.0"):
        HE.check_scene_values(h, robot, own, counts)


def test_the_catalogue_builds_scenes_of_the_documented_shapes():
    for name, fn in SC.CATALOGUE.items():
        for H in (5, 8, 20):
            humans, robot = fn(H)
            assert humans.shape == (H, 6) and robot.shape == (7,) and humans.dtype == robot.dtype == np.float64, name
            d = np.sqrt(((humans[:, None, 0:2] - humans[None, :, 0:2]) ** 2).sum(-1)) + 10.0 * np.eye(H)
            assert d.min() > 0.6, (name, H, d.min())          # no two humans overlap
    hs, rs = SC.stack([fn(8) for fn in SC.CATALOGUE.values()])
    assert hs.shape == (4, 8, 6) and rs.shape == (4, 7)
