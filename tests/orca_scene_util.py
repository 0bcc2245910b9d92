"""Hand-built crowds for the ORCA pass (tests/test_orca_scenes.py, tests/test_gpu_orca_scenes.py): the scenes, the way a chosen state gets
into a device batch, and the per-agent reference.

The trajectories the simulator produces never hold two neighbours at one distance, hardly ever two parallel ORCA lines, never an agent
standing on its goal.  The scenes here are built of exactly that: rings, lattices, rows, coincident pairs, agents on and around the
thresholds of the neighbour search and of the collision branch.  A scene is a function of the crowd size n alone and returns the
[n][6] float64 records (px, py, vx, vy, gx, gy) of valid simulator states; radius and v_pref stay what the batch's reset made them.

inject() writes such records over the human and robot blocks of a snapshot (HipEnvBatch.state_dict) and loads it; the load drops the
prefetched velocities, so the next step recomputes the ORCA pass from the loaded records and applies it: the velocities of the state
after that step ARE the ORCA output for the injected state.  reference() is O.orca_velocity once per agent on the neighbour list
get_human_actions builds (orca_inputs, which tests/lp3_util.handovers shares)."""
import ctypes as C

import numpy as np

PX, PY, VX, VY, GX, GY, RADIUS, V_PREF = range(8)
RVO_EPS = np.float32(0.00001)
# the robot's parking place: a corner of the arena no scene comes near, its goal in the opposite corner, at rest
ROBOT_PARK = np.array([5.0, -5.0, 0.0, 0.0, -5.0, 5.0])
ROBOT_CLEARANCE = 2.0


# ---- the neighbour list of one human (get_human_actions, crowd_sim.py:680-703, as oracle/crowdsim_oracle.c human_orca_action restates it) ----

def orca_inputs(hum, i, robot=None, robot_radius=0.3, safety=0.15):
    """hum: [n] records indexable as (px, py, vx, vy, gx, gy, radius, v_pref); robot: (px, py, vx, vy, ...) when the humans see it, else None.
    -> (self_state, others) as O.orca_velocity takes them: the others in index order, then the robot; a neighbour at the agent's own
    position becomes (7, 7, 0, 0); radii get + 0.01 + safety; the preferred velocity is the goal vector, capped at norm 1."""
    me = hum[i]
    others = []
    for j, o in enumerate(hum):
        if j == i:
            continue
        seen = not (o[PX] == me[PX] and o[PY] == me[PY])
        others.append((o[PX], o[PY], o[VX], o[VY], o[RADIUS] + 0.01 + safety) if seen else (7.0, 7.0, 0.0, 0.0, o[RADIUS] + 0.01 + safety))
    if robot is not None:
        seen = not (robot[0] == me[PX] and robot[1] == me[PY])
        others.append((robot[0], robot[1], robot[2], robot[3], robot_radius + 0.01 + safety) if seen else (7.0, 7.0, 0.0, 0.0, robot_radius + 0.01 + safety))
    vx, vy = me[GX] - me[PX], me[GY] - me[PY]
    speed = np.sqrt(vx * vx + vy * vy)
    if speed > 1.0:
        vx, vy = vx / speed, vy / speed
    return (me[PX], me[PY], me[VX], me[VY], me[RADIUS] + 0.01 + safety, me[V_PREF], vx, vy), others


COUNTS = ("ties", "parallel", "collisions", "coincident", "zero_pref", "short_list", "handovers")


def _agent_counts(self_state, others, lines, fail, neighbor_dist):
    """What one agent's program holds of the properties the scenes are built for, in the float32 arithmetic of Agent::computeNeighbors
    and computeNewVelocity."""
    f = np.float32
    c = dict.fromkeys(COUNTS, 0)
    c["zero_pref"] = int(self_state[6] == 0.0 and self_state[7] == 0.0)
    if others:
        o = np.asarray(others, dtype=np.float32)
        dx, dy = f(self_state[0]) - o[:, 0], f(self_state[1]) - o[:, 1]
        dq = dx * dx + dy * dy
        nd = f(neighbor_dist)
        near = dq < nd * nd
        assert int(near.sum()) == len(lines), (int(near.sum()), len(lines))
        key = np.sort(dq[near])
        c["ties"] = int((key[1:] == key[:-1]).sum())
        cr = f(self_state[4]) + o[:, 4]
        c["collisions"] = int((near & ~(dq > cr * cr)).sum())
        c["coincident"] = int(((o[:, 0] == f(7.0)) & (o[:, 1] == f(7.0))).sum())
        c["short_list"] = int(len(lines) < len(others))
        d = np.asarray(lines, dtype=np.float32).reshape(-1, 4)[:, 2:4]
        det = d[:, None, 0] * d[None, :, 1] - d[:, None, 1] * d[None, :, 0]
        c["parallel"] = int(np.triu(np.abs(det) <= RVO_EPS, 1).sum())
        c["handovers"] = int(fail < len(lines))
    return c


# ---- which branches of the linear programs an agent's program takes: RVO2's linearProgram1/2/3 in numpy float32, operation by operation as
# oracle/crowdsim_oracle.c states them, with a counter at every branch a degenerate crowd is there to reach.  The oracle stays the
# reference: lp_events() asserts that this restatement ends on the oracle's velocity, bit for bit, and is used for counting only. ----

EVENTS = ("lp_parallel", "lp_pfail", "lp3_par", "lp3_skip", "lp3_inner_parallel", "lp3_inner_pfail", "lp3_restore")
_F = np.float32
_Z = np.float32(0.0)


def _det(ax, ay, bx, by):
    return ax * by - ay * bx


def _dot(ax, ay, bx, by):
    return ax * bx + ay * by


def _unit(x, y):
    inv = _F(1.0) / np.sqrt(_dot(x, y, x, y))
    return x * inv, y * inv


def _lp1(L, no, rad, ox, oy, dir_opt, ev, inner, drop_pfail):
    px, py, dx, dy = L[no]
    dp = _dot(px, py, dx, dy)
    disc = dp * dp + rad * rad - _dot(px, py, px, py)
    if disc < _Z:
        return None
    sq = np.sqrt(disc)
    t_left, t_right = -dp - sq, -dp + sq
    for i in range(no):
        qx, qy, ex, ey = L[i]
        den = _det(dx, dy, ex, ey)
        num = _det(ex, ey, px - qx, py - qy)
        if abs(den) <= RVO_EPS:
            ev["lp3_inner_parallel" if inner else "lp_parallel"] += 1
            if num < _Z:
                ev["lp3_inner_pfail" if inner else "lp_pfail"] += 1
                if not (inner and drop_pfail):
                    return None
            continue
        t = num / den
        if den >= _Z:
            t_right = min(t_right, t)
        else:
            t_left = max(t_left, t)
        if t_left > t_right:
            return None
    if dir_opt:
        t = t_right if _dot(ox, oy, dx, dy) > _Z else t_left
    else:
        t = _dot(dx, dy, ox - px, oy - py)
        t = t_left if t < t_left else (t_right if t > t_right else t)
    return px + t * dx, py + t * dy


def _lp2(L, rad, ox, oy, dir_opt, ev, inner=False, drop_pfail=False):
    if dir_opt:
        res = (rad * ox, rad * oy)
    elif _dot(ox, oy, ox, oy) > rad * rad:
        ux, uy = _unit(ox, oy)
        res = (rad * ux, rad * uy)
    else:
        res = (ox, oy)
    for i, (px, py, dx, dy) in enumerate(L):
        if _det(dx, dy, px - res[0], py - res[1]) > _Z:
            new = _lp1(L, i, rad, ox, oy, dir_opt, ev, inner, drop_pfail)
            if new is None:
                return i, res
            res = new
    return len(L), res


def _lp3(L, begin, rad, res, ev, drop_pfail):
    distance = _Z
    for i in range(begin, len(L)):
        px, py, dx, dy = L[i]
        if _det(dx, dy, px - res[0], py - res[1]) > distance:
            proj = []
            for j in range(i):
                qx, qy, ex, ey = L[j]
                d = _det(dx, dy, ex, ey)
                if abs(d) <= RVO_EPS:
                    ev["lp3_par"] += 1
                    if _dot(dx, dy, ex, ey) > _Z:
                        ev["lp3_skip"] += 1
                        continue
                    ppx, ppy = _F(0.5) * (px + qx), _F(0.5) * (py + qy)
                else:
                    s = _det(ex, ey, px - qx, py - qy) / d
                    ppx, ppy = px + s * dx, py + s * dy
                proj.append((ppx, ppy) + _unit(ex - dx, ey - dy))
            fail, new = _lp2(proj, rad, -dy, dx, True, ev, True, drop_pfail)
            if fail < len(proj):
                ev["lp3_restore"] += 1
            else:
                res = new
            distance = _det(dx, dy, px - res[0], py - res[1])
    return res


def lp_events(self_state, lines, fail, vel, drop_inner_pfail=False):
    """The EVENTS of one agent's program (its ORCA lines, the line linearProgram2 failed on and the velocity, all from O.orca_velocity).
    drop_inner_pfail: also return whether the velocity would change if linearProgram3's inner linearProgram1 ignored `parallel and
    numerator < 0` -- the slip `pfail` in lp1_pair guards against."""
    ev = dict.fromkeys(EVENTS, 0)
    L = [tuple(_F(x) for x in ln) for ln in lines]
    rad, ox, oy = _F(self_state[5]), _F(self_state[6]), _F(self_state[7])
    f, res = _lp2(L, rad, ox, oy, False, ev)
    assert f == fail, (f, fail)
    out = _lp3(L, f, rad, res, ev, False) if f < len(L) else res
    assert (_F(vel[0]), _F(vel[1])) == out, (vel, out)
    if drop_inner_pfail:
        mutant = _lp3(L, f, rad, res, dict.fromkeys(EVENTS, 0), True) if f < len(L) else res
        return ev, mutant != out
    return ev


def reference(hum, robot=None, neighbor_dist=10.0, time_horizon=5.0, time_step=0.25, robot_radius=0.3, safety=0.15, counts=False):
    """The ORCA velocity of every human of one env: hum [n][8] float64, robot [>= 4] (or None: the humans do not see it) -> vel [n][2]
    float32 (, with counts=True, the env's sums of COUNTS, of EVENTS and of the agents whose velocity `pfail` in lp1_pair decides)."""
    from oracle import oracle as O
    n = len(hum)
    vel = np.zeros((n, 2), dtype=np.float32)
    total = dict.fromkeys(COUNTS + EVENTS + ("pfail_decides",), 0)
    for i in range(n):
        me, others = orca_inputs(hum, i, robot, robot_radius, safety)
        if counts:
            v, lines, fail = O.orca_velocity(me, others, neighbor_dist=neighbor_dist, time_horizon=time_horizon, time_step=time_step, want_lines=True)
            if not others:
                lines = lines[:0]
            for k, x in _agent_counts(me, others, lines, fail, neighbor_dist).items():
                total[k] += x
            ev, decisive = lp_events(me, lines, fail, v, drop_inner_pfail=True)
            for k, x in ev.items():
                total[k] += x
            total["pfail_decides"] += int(decisive)
        else:
            v = O.orca_velocity(me, others, neighbor_dist=neighbor_dist, time_horizon=time_horizon, time_step=time_step)
        vel[i] = v
    return (vel, total) if counts else vel


def oracle_neighbor_dist(oe):
    """config.orca.neighbor_dist as oracle env `oe` holds it right now: with randomize_attributes every new human redraws this class
    attribute (agent.py:21-22), and a private simulator built afterwards freezes the value."""
    from tests.lp3_util import oracle_env_head
    from oracle import oracle as O
    M = O.MAX_HUMANS

    class OrcEnvSims(C.Structure):   # OrcEnv (oracle/crowdsim_oracle.h) up to shared_neighbor_dist
        _fields_ = [("head", oracle_env_head()), ("n_humans", C.c_int32), ("observed_count", C.c_int32), ("observed_max", C.c_int32),
                    ("desired_v", C.c_double), ("last_left", C.c_double), ("last_right", C.c_double), ("has_gauss", C.c_int32), ("gauss", C.c_double),
                    ("sim_valid", C.c_int32 * M), ("sim_n", C.c_int32 * M), ("sim_nd", C.c_float * M), ("sim_self_radius", C.c_float * M),
                    ("sim_self_maxspeed", C.c_float * M), ("sim_seen_radius", C.c_float * M * M), ("shared_neighbor_dist", C.c_double)]
    st = C.cast(oe._h, C.POINTER(OrcEnvSims)).contents
    assert st.n_humans == oe.human_count and 5.0 <= st.shared_neighbor_dist <= 10.0, (st.n_humans, st.shared_neighbor_dist)
    return st.shared_neighbor_dist


# ---- scenes: n -> [n][6] float64 (px, py, vx, vy, gx, gy) ----

def _nf(x, towards):
    return float(np.nextafter(np.float32(x), np.float32(towards)))


def ring(n, radius, phase=0.0):
    """n agents evenly spaced on a circle, at rest, each with the antipodal point as its goal (the simulator's circle crossing without
    its placement noise)."""
    a = phase + 2.0 * np.pi * np.arange(n) / max(n, 1)
    p = radius * np.stack([np.cos(a), np.sin(a)], axis=1)
    return np.concatenate([p, np.zeros((n, 2)), -p], axis=1)


def ring_chord(n, chord, phase=0.0):
    """A ring whose neighbours stand `chord` apart (n = 1: the agent stands on its goal, n = 2: the two of them)."""
    return ring(n, chord / (2.0 * np.sin(np.pi / n)) if n > 1 else 0.0, phase)


def lattice(n, spacing=0.6, goal=(3.0, 2.5)):
    """A square lattice around the origin, at rest, everybody heading for one goal."""
    w = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    p = spacing * np.stack([k % w - (w - 1) / 2.0, k // w - (w - 1) / 2.0], axis=1)
    return np.concatenate([p, np.zeros((n, 2)), np.tile(np.asarray(goal, dtype=np.float64), (n, 1))], axis=1)


def marching_row(n, y=3.0, half_length=5.5, v=(0.0, -0.75)):
    """A row 11 m long (its ends do not see each other: neighbour distance 10) that marches with one velocity towards goals 1.5 m ahead."""
    x = np.linspace(-half_length, half_length, n) if n > 1 else np.zeros(1)
    p = np.stack([x, np.full(n, y)], axis=1)
    v = np.tile(np.asarray(v, dtype=np.float64), (n, 1))
    return np.concatenate([p, v, p + 2.0 * v], axis=1)


def head_on_rows(n, gap=2.0, spacing=1.0):
    """Two rows that walk into each other, every agent exactly facing its partner (relative position and relative velocity parallel)."""
    k = np.arange(n)
    top = (k % 2 == 0)
    spacing = min(spacing, 9.5 / max((n + 1) // 2 - 1, 1))      # large crowds close ranks: the rows stay inside the arena
    x = spacing * (k // 2 - ((n + 1) // 2 - 1) / 2.0)
    y = np.where(top, gap / 2.0, -gap / 2.0)
    vy = np.where(top, -0.75, 0.75)
    return np.stack([x, y, np.zeros(n), vy, x, -2.0 * y], axis=1)


def coincident_pairs(n, spacing=0.75):
    """Agents 2k and 2k + 1 stand on one point (each sees the other as the dummy at (7, 7)); the points form a lattice, one of a pair walks
    to the far side, the other to a common goal."""
    m = (n + 1) // 2
    q = lattice(m, spacing)[:, 0:2] + np.array([0.25, -0.125])
    k = np.arange(n)
    p = q[k // 2]
    g = np.where((k % 2 == 0)[:, None], -3.0 * p, np.tile(np.array([-3.0, 1.0]), (n, 1)))
    v = np.where((k % 2 == 0)[:, None], 0.0, 0.25) * np.stack([np.ones(n), -np.ones(n)], axis=1)
    return np.concatenate([p, v, g], axis=1)


def mixed(n):
    """A loose ring of agents with every kind of goal and speed: 0 stands on its goal (zero preferred velocity), 1 has 0.5 m to go, 2
    exactly 1 m (the cap `speed > 1` just does not apply), 3 runs faster than its v_pref allows, 4 stands on its goal while moving; the
    rest cross the ring at various speeds."""
    s = ring(n, 2.5, 0.3)
    k = np.arange(n)
    s[:, 0:2] = np.round(s[:, 0:2] * (1.0 + 0.07 * (k % 3))[:, None] * 64.0) / 64.0     # dyadic positions: goal offsets below are exact
    s[:, 4:6] = -s[:, 0:2]
    s[:, 2] = 0.125 * ((k % 5) - 2)
    s[:, 3] = 0.0625 * ((k % 7) - 3)
    kinds = min(n, 5)
    for i in range(kinds):
        if i == 0:
            s[i, 2:4] = 0.0; s[i, 4:6] = s[i, 0:2]
        elif i == 1:
            s[i, 4:6] = s[i, 0:2] + np.array([-0.5, 0.0])
        elif i == 2:
            s[i, 4:6] = s[i, 0:2] + np.array([0.0, 1.0])
        elif i == 3:
            s[i, 2:4] = np.array([-1.25, 1.0])
        else:
            s[i, 4:6] = s[i, 0:2]
    return s


def boundaries(n, combined_radius=None, neighbor_dist=10.0):
    """Pairs on the thresholds.  0-1, 2-3, 4-5: centres at exactly the combined radius (float32: self radius + seen radius), one float
    below and one above (`!(distSq > combinedRadiusSq)`).  6-7: exactly the neighbour distance apart (`distSq < rangeSq` is false: no
    neighbour); 8-9: the largest float32 distance below it.  Further agents stand in rows below them."""
    f = np.float32
    cr = f(0.3 + 0.01 + 0.15) + f(0.3 + 0.01 + 0.15) if combined_radius is None else f(combined_radius)
    pts = []
    for y, d in ((0.0, float(cr)), (1.5, _nf(cr, 0.0)), (-1.5, _nf(cr, 1.0))):
        pts += [(0.0, y), (d, y)]
    nd = f(neighbor_dist)
    x = f(nd / f(2.0))
    pts += [(-float(x), 3.5), (float(x), 3.5)]
    below = x
    while not ((f(-x) - below) * (f(-x) - below) < nd * nd):
        below = np.nextafter(below, f(0.0))
    pts += [(-float(x), 5.0), (float(below), 5.0)]
    pts += [(-3.0 + 0.5 * (k % 12), -3.0 - 0.5 * (k // 12)) for k in range(max(0, n - len(pts)))]
    p = np.array(pts[:n], dtype=np.float64)
    g = np.stack([p[:, 0], -p[:, 1] - 1.0], axis=1)
    return np.concatenate([p, np.zeros((n, 2)), g], axis=1)


def control(n, seed=7, spread=1.2):
    """A seeded uniform dense scene: nothing special about it except that most agents need linearProgram3."""
    r = np.random.RandomState(seed)
    p = r.uniform(-spread, spread, (n, 2))
    v = r.uniform(-0.5, 0.5, (n, 2))
    g = r.uniform(-4.0, 4.0, (n, 2))
    return np.concatenate([p, v, g], axis=1)


def stacks(n, gap=2.0 ** -20, vel=0.0, spacing=1.0):
    """Clusters of three agents a few float32 steps apart (not coincident: no dummy), the clusters on a lattice.  An observer's ORCA lines for
    the members of a cluster are parallel within RVO_EPSILON without being equal: linearProgram3 projects them into lines that are parallel
    again, and its inner linearProgram2 fails on them (`parallel and numerator < 0`, crossing bounds, a chord that misses the disc) and
    restores the result -- branches no other scene reaches.  vel: the members of a cluster drift apart at that speed."""
    k = np.arange(n)
    c, r = k // 3, k % 3
    w = int(np.ceil(np.sqrt((n + 2) // 3)))
    px = spacing * (c % w - (w - 1) / 2.0) + gap * r
    py = spacing * (c // w - (w - 1) / 2.0) + gap * (r * r)
    return np.stack([px, py, vel * (r - 1.0), np.zeros(n), -3.0 * px - 1.0, -3.0 * py + 0.5], axis=1)


# name -> (builder, the counts that must be >= 1 once the crowd is large enough for the scene to show them, that crowd size)
SCENES = {
    "ring4": (lambda n: ring(n, 4.0), ("ties",), 3),
    "ring_tight": (lambda n: ring_chord(n, 0.47), ("ties", "handovers", "collisions"), 5),
    "ring_collide": (lambda n: ring(n, 0.4375, 0.1), ("ties", "collisions"), 3),
    "lattice": (lattice, ("ties", "parallel", "collisions"), 7),
    "row": (marching_row, ("ties", "parallel", "short_list"), 7),
    "head_on": (head_on_rows, ("ties", "parallel"), 7),
    "pairs": (coincident_pairs, ("coincident", "ties", "parallel", "collisions"), 7),
    "mixed": (mixed, ("zero_pref",), 1),
    "boundaries": (boundaries, ("collisions", "short_list"), 8),
    "control": (control, ("handovers",), 7),
    "stacks": (stacks, ("collisions", "lp3_par", "lp3_skip"), 19),
    "stacks_drift": (lambda n: stacks(n, 2.0 ** -18, 0.125), ("collisions", "lp3_restore"), 19),
}
SCENE_ORDER = tuple(SCENES)


def batch_scenes(E, H, shift=0):
    """Env e of a batch gets scene (e + shift) mod 12: neighbouring envs -- the agents of one wavefront -- hold unrelated geometry.
    -> (names [E], humans [E][H][6])."""
    names = [SCENE_ORDER[(e + shift) % len(SCENE_ORDER)] for e in range(E)]
    return names, np.stack([SCENES[nm][0](H) for nm in names])


def infeasible_rings(E, H):
    """A batch in which (the CPU half checks it with the oracle) every agent of every env needs linearProgram3: tight rings, no two envs
    with the same radius or phase."""
    return np.stack([ring_chord(H, 0.44 + 0.01 * (e % 6), 0.37 * e) for e in range(E)])


def parked_robot(E):
    return np.tile(ROBOT_PARK, (E, 1))


def check_scene(humans, robot, arena=6.0):
    """The conditions an injected state must keep: finite, inside the arena, the robot parked clear of every human and of its goal."""
    humans, robot = np.asarray(humans), np.asarray(robot)
    assert np.isfinite(humans).all() and np.isfinite(robot).all()
    assert (np.abs(humans[..., 0:2]) <= arena).all() and (np.abs(robot[..., 0:2]) <= arena).all(), "positions outside the arena"
    assert (np.abs(humans[..., 4:6]) <= arena * np.sqrt(2.0) + 0.75).all(), "goals beyond the circle the simulator draws them from"
    d = np.sqrt(((humans[..., 0:2] - robot[:, None, 0:2]) ** 2).sum(-1))
    assert d.min() >= ROBOT_CLEARANCE, "robot parked %.3f m from a human" % d.min()
    assert np.sqrt(((robot[:, 0:2] - robot[:, 4:6]) ** 2).sum(-1)).min() >= ROBOT_CLEARANCE, "robot parked on its goal"
    return float(d.min())


# ---- a chosen state into a device batch ----

def read(env):
    """(humans [E][H][8], robot [E][8]) float64 numpy copies of the batch's state (get_state)."""
    h, r = env.get_state()
    return h.cpu().numpy().copy(), r.cpu().numpy().copy()


def inject(env, humans, robot):
    """Overwrite px, py, vx, vy, gx, gy of every human (humans [E][H][6]) and of the robot (robot [E][6]) of a batch that was JUST reset,
    through its snapshot: SnapHeader | blob, the blob starting with the human records [E][8][H] float64 and, at the next 256-byte
    boundary, the robot records [E][8] (cn_env_create's carve).  radius / v_pref stay what the reset made them: the private simulators
    that reset's ORCA pass built froze them.  Loading the snapshot clears the prefetched velocities; the next step recomputes them."""
    E, H = env.E, env.H
    humans, robot = np.asarray(humans, dtype=np.float64), np.asarray(robot, dtype=np.float64)
    assert humans.shape == (E, H, 6) and robot.shape == (E, 6), (humans.shape, robot.shape)
    check_scene(humans, robot, float(env.cfg.arena_size))
    h0, r0 = read(env)
    # right after reset(): everybody at rest, every goal the antipode of its owner (generate_circle_crossing_human)
    assert not h0[:, :, 2:4].any() and np.array_equal(h0[:, :, 4:6], -h0[:, :, 0:2]) and not r0[:, 2:4].any(), "inject() wants a batch right after reset()"
    snap = env.state_dict()
    raw = snap.numpy()
    blob_bytes = int(raw[8:16].view(np.uint64)[0])
    head = raw.size - blob_bytes
    assert 16 < head < 1024 and head % 8 == 0, (raw.size, blob_bytes)
    blob = raw[head:]
    hum_bytes = E * 8 * H * 8
    o_rob = (hum_bytes + 255) & ~255
    hum = blob[:hum_bytes].view(np.float64).reshape(E, 8, H)
    rob = blob[o_rob:o_rob + E * 64].view(np.float64).reshape(E, 8)
    # the two blocks about to be overwritten ARE the records get_state reports: a layout change fails here, not somewhere in the blob
    assert hum.transpose(0, 2, 1).tobytes() == h0.tobytes() and rob.tobytes() == r0.tobytes(), "the snapshot does not start with the agent records"
    hum[:, 0:6, :] = humans.transpose(0, 2, 1)
    rob[:, 0:6] = robot
    rob[:, 7] = -np.sqrt(((robot[:, 0:2] - robot[:, 4:6]) ** 2).sum(-1))     # R_POT: the potential of the robot's new place
    env.load_state_dict(snap)
    h1, r1 = read(env)
    assert np.array_equal(h1[:, :, 0:6], humans) and np.array_equal(h1[:, :, 6:8], h0[:, :, 6:8]) and np.array_equal(r1[:, 0:6], robot)
    return h1, r1


# ---- the cases both halves run: name -> dict(H, rv (robot_visible), E, kind, cfg (further config), steps[, lp3_blocks]) ----

SEED = 425
SHAPES = ((1, 0), (2, 0), (7, 1), (8, 0), (9, 0), (19, 1), (20, 0), (21, 0), (31, 1), (32, 0), (32, 1), (40, 0))


def _envs_for(H):
    """13 envs (every scene at least once), or as many as it takes for E * H to exceed 64; never a multiple of the wavefront."""
    E = max(13, -(-65 // H))
    while (E * H) % 64 == 0:
        E += 1
    return E


def _cases():
    cases = {}
    for H, rv in SHAPES:
        cases["h%d_rv%d" % (H, rv)] = dict(H=H, rv=rv, E=_envs_for(H), kind="scenes", cfg={}, steps=8)
    # with end_goal_changing off nobody is respawned on arrival: the agents that stand on their goal keep the velocity ORCA gave them
    for H, rv in ((8, 0), (20, 0), (32, 0), (32, 1)):
        cases["h%d_rv%d_stay" % (H, rv)] = dict(H=H, rv=rv, E=_envs_for(H), kind="scenes", cfg=dict(end_goal_changing=0), steps=8)
    # every agent of every env infeasible: the hand-over list holds E * H entries, all it has room for
    cases["full_odd"] = dict(H=19, rv=0, E=7, kind="rings", cfg={}, steps=8)
    cases["full_one_block"] = dict(H=20, rv=0, E=4, kind="rings", cfg={}, steps=8, lp3_blocks=1)
    # per-human radii and speed limits (sim_seen, sim_self_maxspeed), a neighbour distance drawn at reset: one step on the frozen values
    cases["random_attrs"] = dict(H=20, rv=0, E=13, kind="scenes", cfg=dict(randomize_attributes=1), steps=1)
    return cases


CASES = _cases()


def case_config(name):
    c = CASES[name]
    return dict(c["cfg"], human_num=c["H"], robot_visible=c["rv"], nenv=c["E"])


def case_scene(name):
    """-> (scene names [E], humans [E][H][6], robot [E][6]) of the state the case injects."""
    c = CASES[name]
    E, H = c["E"], c["H"]
    if c["kind"] == "rings":
        return ["ring_tight"] * E, infeasible_rings(E, H), parked_robot(E)
    names, humans = batch_scenes(E, H, shift=H)
    return names, humans, parked_robot(E)


def oracle_reset_attrs(name):
    """radius / v_pref [E][H][2] and the neighbour distance [E] of the case's envs right after reset, from oracle envs of the same seeds
    (fixed attributes: the config's values; randomised: what the reset drew)."""
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
        nds.append(oracle_neighbor_dist(oe))
    return np.array(attrs), np.array(nds)


def env_reference(cfg, hum, rob, neighbor_dist, counts=False):
    """reference() with an env config's parameters (an _abi / oracle config object: the same member names)."""
    return reference(hum, rob if cfg.robot_visible else None, neighbor_dist=neighbor_dist, time_horizon=cfg.orca_time_horizon,
                     time_step=cfg.time_step, robot_radius=cfg.robot_radius, safety=cfg.orca_safety_space, counts=counts)
