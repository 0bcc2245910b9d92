"""Hand-built situations in closed form, as inputs of HipEnvBatch.set_scene / evaluation.evaluate_scenes: each builder returns
(humans [H,6] px, py, vx, vy, gx, gy; robot [7] px, py, vx, vy, gx, gy, theta) as float64 numpy arrays for a crowd of H humans of radius 0.3
in the default 6 m arena.  numpy only: no device needed to build or inspect a scene.  Humans meant to stand still are placed ON their goal
with zero velocity, which only lasts with humans.end_goal_changing (and random_goal_changing) off: with it on, the simulator respawns a human
that has arrived."""
import numpy as np

THETA_UP = float(np.pi / 2.0)      # the heading a holonomic robot's reset gives it


def _robot(px, py, gx, gy, theta=THETA_UP):
    return np.array([px, py, 0.0, 0.0, gx, gy, theta], dtype=np.float64)


def parked(H, x=5.5, spacing=1.0):
    """H humans at rest on their goals in two columns at x = -+x, out of the robot's sensor range along the y axis."""
    k = np.arange(H)
    side = np.where(k % 2 == 0, -1.0, 1.0)
    rows = (H + 1) // 2
    y = spacing * ((k // 2) - (rows - 1) / 2.0)
    p = np.stack([side * x, y], axis=1)
    return np.concatenate([p, np.zeros((H, 2)), p], axis=1)


def straight_run(H, start=-2.0, goal=2.0):
    """Nobody in the way: the robot at (0, start) with its goal at (0, goal), every human parked."""
    return parked(H), _robot(0.0, start, 0.0, goal)


def blocked_run(H, start=-2.0, goal=2.0):
    """straight_run with human 0 at rest on its goal at the origin, on the robot's straight line."""
    humans, robot = straight_run(H, start, goal)
    humans[0] = 0.0
    return humans, robot


def circle_crossing(H, radius=5.0):
    """H humans evenly on a circle, each heading for the antipode, the robot crossing through the centre from just outside the circle."""
    a = 2.0 * np.pi * (np.arange(H) + 0.5) / H
    p = radius * np.stack([np.cos(a), np.sin(a)], axis=1)
    return np.concatenate([p, np.zeros((H, 2)), -p], axis=1), _robot(0.0, -(radius + 0.5), 0.0, radius + 0.5)


def head_on_rows(H, half_gap=4.0, spacing=1.0):
    """Two rows facing each other across the robot's line, each human heading straight for the other side, the rows offset by half a spacing
    so that they interleave where they meet; the robot runs between them along the y axis."""
    k = np.arange(H)
    left = k % 2 == 0
    rows = (H + 1) // 2
    y = spacing * ((k // 2) - (rows - 1) / 2.0) + np.where(left, 0.0, spacing / 2.0)
    x = np.where(left, -half_gap, half_gap)
    p = np.stack([x, y], axis=1)
    g = np.stack([-x, y], axis=1)
    return np.concatenate([p, np.zeros((H, 2)), g], axis=1), _robot(0.0, -5.0, 0.0, 5.0)


def stationary_cluster(H, spacing=0.8):
    """A cluster at rest around the origin, on the straight line from the robot to its goal."""
    w = int(np.ceil(np.sqrt(H)))
    k = np.arange(H)
    p = spacing * np.stack([(k % w) - (w - 1) / 2.0, (k // w) - ((H - 1) // w) / 2.0], axis=1)
    return np.concatenate([p, np.zeros((H, 2)), p], axis=1), _robot(0.0, -4.5, 0.0, 4.5)


def overtaking(H):
    """Human 0 comes up from behind at full speed on a line 0.6 m beside the robot's, both heading up the arena; the others are parked."""
    humans = parked(H)
    humans[0] = (0.6, -6.0, 0.0, 1.0, 0.6, 6.0)
    return humans, _robot(0.0, -4.0, 0.0, 5.0)


CATALOGUE = {"circle_crossing": circle_crossing, "head_on_rows": head_on_rows, "stationary_cluster": stationary_cluster, "overtaking": overtaking}


def stack(scenes):
    """[(humans [H,6], robot [7]), ...] -> (humans [n,H,6], robot [n,7]): the batch form evaluate_scenes takes."""
    return np.stack([h for h, _ in scenes]), np.stack([r for _, r in scenes])
