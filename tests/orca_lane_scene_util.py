"""Scenes for the staged floats of orca_lane_kernel (csrc/orca.h), on the machinery of tests/orca_scene_util.py.

The lane kernel keeps every agent's position twice: as doubles, and converted once to the floats its loops work on.  The reference
replaces a neighbour whose DOUBLE position equals the agent's by the dummy human at (7, 7); the kernel compares the floats first and
reads the doubles only where the floats are equal.  The scenes here stand on that filter:

  twins_*      pairs (2k, 2k + 1) whose positions are equal as float32 and differ as float64 by 1e-12 in x only, in y only, in both --
               neighbours at float distance zero that are NOT the dummy -- and pairs that are exactly coincident, which are;
  centre_ring  one agent in the middle of points (+-a, +-b), (+-b, +-a): neighbours at exactly equal float distances, ordered by index.

tests/test_orca_lane_scenes.py counts these properties with the oracle's own neighbour lists; tests/test_gpu_orca_lane_chain.py steps
device batches loaded with the scenes."""
import ctypes as C
import functools

import numpy as np

from tests import orca_scene_util as S

TWIN_EPS = 1e-12
_TWIN_OFFSET = {"x": (TWIN_EPS, 0.0), "y": (0.0, TWIN_EPS), "xy": (TWIN_EPS, -TWIN_EPS), "same": (0.0, 0.0)}


def twins(n, kinds):
    """Pair k = agents (2k, 2k + 1): the second stands kinds[k % len(kinds)] away from the first -- 1e-12 in "x", in "y", in both ("xy"), or
    nowhere ("same": coincident).  The pairs stand on a lattice whose coordinates are multiples of 1/8 and never zero, so 1e-12 is far
    below half a float32 step of every coordinate.  One of a pair is at rest, the other moves: the relative velocity is never zero (a
    neighbour at distance zero takes the collision branch, which divides by its length)."""
    m = (n + 1) // 2
    q = S.lattice(m, 0.75)[:, 0:2] + np.array([0.25, -0.125])
    k = np.arange(n)
    p = q[k // 2].copy()
    for a in range(1, n, 2):
        p[a] += np.array(_TWIN_OFFSET[kinds[(a // 2) % len(kinds)]])
    f = np.float32
    assert (q != 0.0).all() and np.array_equal(p.astype(f), q[k // 2].astype(f)), "the twins must be equal as float32"
    even = (k % 2 == 0)[:, None]
    g = np.where(even, -3.0 * q[k // 2], np.tile(np.array([-3.0, 1.0]), (n, 1)))
    v = np.where(even, 0.0, 0.25) * np.stack([np.ones(n), -np.ones(n)], axis=1)
    return np.concatenate([p, v, g], axis=1)


_RING_FAMILIES = ((1.0, 0.5), (1.5, 0.25), (0.75, 1.25), (2.0, 0.125))
_RING_CENTRE = np.array([0.5, -0.25])


def centre_ring(n):
    """Agent 0 in the middle, the others on the points centre + (+-a, +-b), centre + (+-b, +-a) of up to four (a, b): all coordinates are
    dyadic, so the eight points of a family are at EXACTLY one float32 distance from agent 0 (a * a + b * b, in either order of the two
    squares).  At rest; the ring agents cross the centre, agent 0 leaves it."""
    pts = []
    for a, b in _RING_FAMILIES:
        pts += [(a, b), (-a, b), (a, -b), (-a, -b), (b, a), (-b, a), (b, -a), (-b, -a)]
    assert n - 1 <= len(pts)
    off = np.array(pts[:max(n - 1, 0)], dtype=np.float64).reshape(-1, 2)
    p = np.concatenate([_RING_CENTRE[None, :], _RING_CENTRE[None, :] + off])[:n]
    g = np.concatenate([np.array([[3.0, 2.0]]), _RING_CENTRE[None, :] - off])[:n]
    return np.concatenate([p, np.zeros((n, 2)), g], axis=1)


# name -> (builder, the properties (property_counts) that must be >= 1 from 5 humans on)
SCENES = {
    "twins_x": (lambda n: twins(n, ("x",)), ("float_equal_x",)),
    "twins_y": (lambda n: twins(n, ("y",)), ("float_equal_y",)),
    "twins_xy": (lambda n: twins(n, ("xy", "same")), ("float_equal_xy", "coincident")),
    "twins_all": (lambda n: twins(n, ("x", "y", "xy", "same")), ("float_equal_x", "float_equal_y", "float_equal_xy", "coincident")),
    "centre_ring": (centre_ring, ("ties", "ties_of_agent_0")),
}

SEED = S.SEED
# name -> dict(H, rv, E, scenes (one per env: a name of SCENES here, or of orca_scene_util.SCENES), cfg, steps)
CASES = {
    # network 8
    "h5_new": dict(H=5, rv=0, E=4, scenes=("twins_x", "twins_y", "twins_xy", "centre_ring"), cfg={}, steps=3),
    "h5_old": dict(H=5, rv=0, E=4, scenes=("pairs", "ring_collide", "boundaries", "control"), cfg={}, steps=3),
    # network 20; 80 agents: a second, partly filled wavefront whose lanes span env boundaries
    "h20_new": dict(H=20, rv=0, E=4, scenes=("twins_x", "twins_y", "twins_xy", "centre_ring"), cfg={}, steps=3),
    "h20_old": dict(H=20, rv=0, E=4, scenes=("pairs", "lattice", "stacks", "ring_tight"), cfg={}, steps=3),
    # network 32 with the robot in the last slot
    "h31_robot_new": dict(H=31, rv=1, E=2, scenes=("twins_all", "centre_ring"), cfg={}, steps=3),
    "h31_robot_old": dict(H=31, rv=1, E=2, scenes=("pairs", "stacks_drift"), cfg={}, steps=3),
    # per-human radii, read from sim_seen in global memory: one step on the frozen values
    "h20_random_attrs": dict(H=20, rv=0, E=4, scenes=("twins_all", "centre_ring", "pairs", "ring_collide"), cfg=dict(randomize_attributes=1), steps=1),
}


def case_config(name):
    c = CASES[name]
    return dict(c["cfg"], human_num=c["H"], robot_visible=c["rv"], nenv=c["E"])


def case_scene(name):
    """-> (scene names [E], humans [E][H][6], robot [E][6]) of the state the case injects."""
    c = CASES[name]
    humans = np.stack([(SCENES[nm][0] if nm in SCENES else S.SCENES[nm][0])(c["H"]) for nm in c["scenes"]])
    return list(c["scenes"]), humans, S.parked_robot(c["E"])


@functools.lru_cache(maxsize=None)
def reset_attrs(name):
    """orca_scene_util.oracle_reset_attrs for the cases of this file."""
    from oracle import oracle as O
    from tests.lp3_util import oracle_env_head
    c = CASES[name]
    head = oracle_env_head()
    attrs, nds = [], []
    for e in range(c["E"]):
        oe = O.OracleEnv(O.default_config(**case_config(name)), SEED + e)
        oe.reset()
        st = C.cast(oe._h, C.POINTER(head)).contents
        attrs.append([(st.humans[j].radius, st.humans[j].v_pref) for j in range(c["H"])])
        nds.append(S.oracle_neighbor_dist(oe))
    return np.array(attrs), np.array(nds)


def property_counts(hum, robot, neighbor_dist, cfg):
    """What the filter meets in one env, from the neighbour lists the oracle's ORCA is given (orca_scene_util.orca_inputs): neighbours
    whose float32 position equals the agent's while the float64 one differs in x only / y only / both, neighbours replaced by the
    dummy, and -- from the oracle's own run on those lists -- distance ties (of the env, and of agent 0)."""
    f = np.float32
    out = dict(float_equal_x=0, float_equal_y=0, float_equal_xy=0, coincident=0, ties=0, ties_of_agent_0=0)
    rob = robot if cfg.robot_visible else None
    for i in range(len(hum)):
        me, others = S.orca_inputs(hum, i, rob, cfg.robot_radius, cfg.orca_safety_space)
        raw = [o for j, o in enumerate(hum) if j != i] + ([rob] if rob is not None else [])
        for seen, o in zip(others, raw):
            if f(o[0]) == f(me[0]) and f(o[1]) == f(me[1]):
                dx, dy = o[0] != me[0], o[1] != me[1]
                if dx or dy:
                    assert seen[0] == o[0] and seen[1] == o[1], "equal as floats only: the oracle sees the neighbour where it stands"
                    out["float_equal_xy" if dx and dy else ("float_equal_x" if dx else "float_equal_y")] += 1
                else:
                    assert seen[0] == 7.0 and seen[1] == 7.0
    _, tot = S.reference(hum, rob, neighbor_dist=neighbor_dist, time_horizon=cfg.orca_time_horizon, time_step=cfg.time_step,
                         robot_radius=cfg.robot_radius, safety=cfg.orca_safety_space, counts=True)
    out["coincident"], out["ties"] = tot["coincident"], tot["ties"]
    # agent 0's own ties: its sorted float32 keys, as Agent::computeNeighbors has them
    me, others = S.orca_inputs(hum, 0, rob, cfg.robot_radius, cfg.orca_safety_space)
    if others:
        o = np.asarray(others, dtype=f)
        dq = (f(me[0]) - o[:, 0]) ** 2 + (f(me[1]) - o[:, 1]) ** 2
        key = np.sort(dq[dq < f(neighbor_dist) * f(neighbor_dist)])
        out["ties_of_agent_0"] = int((key[1:] == key[:-1]).sum())
    return out


# ---- the natural run: E = 8, H = 20, 40 scripted steps of the oracle, with what the agents meet on the way ----

NATURAL = dict(E=8, T=40, seed=425, kw=dict(human_num=20))


@functools.lru_cache(maxsize=None)
def natural_run():
    """-> (steps in tests.test_gpu_env_profile._oracle_run's layout, hand-overs per step, colliding ordered pairs per step): the oracle's
    humans in the states they act on.  A pair collides when its float32 distance is not above the float32 sum of the radii each agent's
    simulator holds -- the `collide` of pass 2, the branch that uses 1 / time step."""
    from oracle import oracle as O
    from tests.lp3_util import handovers, oracle_env_head
    from tests.test_gpu_env import _actions
    from tests.test_gpu_env_profile import KEYS
    E, T, seed, kw = NATURAL["E"], NATURAL["T"], NATURAL["seed"], dict(NATURAL["kw"], nenv=NATURAL["E"])
    H = kw["human_num"]
    head = oracle_env_head()
    oenvs = [O.OracleEnv(O.default_config(**kw), seed + i) for i in range(E)]
    f = np.float32

    def stack(obs_list):
        return {k: np.stack([ob[k] for ob in obs_list]) for k in KEYS}

    def collisions(oe):
        st = C.cast(oe._h, C.POINTER(head)).contents
        h = np.array([(st.humans[j].px, st.humans[j].py, st.humans[j].radius) for j in range(H)])
        p, r = h[:, 0:2].astype(f), (h[:, 2] + 0.01 + 0.15).astype(f)
        d = p[:, None, :] - p[None, :, :]
        dq = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        cr = r[:, None] + r[None, :]
        return int((~(dq > cr * cr) & ~np.eye(H, dtype=bool)).sum())
    host = stack([oe.reset() for oe in oenvs])
    steps, hand, coll = [dict(obs=host)], [], []
    for t in range(T):
        hand.append(sum(len(handovers(oe, head)) for oe in oenvs))
        coll.append(sum(collisions(oe) for oe in oenvs))
        act = _actions(host, t, E)
        out, rew, done, info, md = [], [], [], [], []
        for i, oe in enumerate(oenvs):
            ob, r, d, inf = oe.step(act[i], autoreset=True)
            out.append(ob); rew.append(np.float32(r)); done.append(d); info.append(inf["info"]); md.append(inf["min_dist"])
        host = stack(out)
        steps.append(dict(act=act, obs=host, rew=np.array(rew), done=np.array(done), info=np.array(info), md=np.array(md)))
    return steps, hand, coll
