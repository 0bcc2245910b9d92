"""linearProgram3 hand-overs read from the CPU oracle's own records (tests/test_gpu_lp3_pairs.py, tools/lp3_pairing_study.py).

The device's orca_lane_kernel hands every agent whose linearProgram2 is infeasible to orca_lp3_kernel: a header (number of lines, the
line linearProgram2 failed on, the result it had reached, the speed limit) and the agent's ORCA lines in neighbour order.  The same
records are rebuilt here from the oracle's human states, for batches with fixed human attributes and a full field of view (what the
simulator's private rvo2 instances were built from is then what the records show)."""
import ctypes as C

import numpy as np

from tests.orca_scene_util import orca_inputs


def oracle_env_head():
    """The leading members of OrcEnv (oracle/crowdsim_oracle.h) up to the human records."""
    from oracle import oracle as O

    class OrcMT(C.Structure):
        _fields_ = [("key", C.c_uint32 * 624), ("pos", C.c_int32)]

    class OrcHuman(C.Structure):
        _fields_ = [(k, C.c_double) for k in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref")]

    class OrcEnvHead(C.Structure):
        _fields_ = [("cfg", O.OrcConfig), ("this_seed", C.c_int64), ("case_counter", C.c_uint64 * 3), ("rng", OrcMT), ("rng_draws", C.c_uint64),
                    ("robot", C.c_double * 7), ("humans", OrcHuman * O.MAX_HUMANS)]
    return OrcEnvHead


def handovers(oe, head, want_lines=False):
    """The humans of oracle env `oe` whose next ORCA action needs linearProgram3, from the state the env is in right now:
    a list of dict(agent, nn, line_fail, radius, pref, out (the oracle's new velocity)[, lines [nn][4] float32]).  Humans: ORCA.predict (crowd_nav/policy/orca.py:64-117) as
    oracle/crowdsim_oracle.c human_orca_action restates it; the neighbour list is tests/orca_scene_util.orca_inputs."""
    from oracle import oracle as O
    cfg = oe.cfg
    assert not cfg.randomize_attributes and cfg.human_fov >= 2.0 and cfg.humans_policy == 0
    st = C.cast(oe._h, C.POINTER(head)).contents
    n = oe.human_count
    hs = [tuple(getattr(st.humans[j], k) for k in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref")) for j in range(n)]
    rob = list(st.robot) if cfg.robot_visible else None   # px, py, vx, vy, gx, gy, theta
    saf = cfg.orca_safety_space
    out = []
    for i in range(n):
        state, others = orca_inputs(hs, i, rob, cfg.robot_radius, saf)
        if not others:
            continue
        v_pref, (vx, vy) = state[5], state[6:8]
        vel, lines, fail = O.orca_velocity(state, others, neighbor_dist=cfg.orca_neighbor_dist, time_horizon=cfg.orca_time_horizon,
                                         time_step=cfg.time_step, want_lines=True)
        if fail < len(lines):
            rec = dict(agent=i, nn=len(lines), line_fail=fail, radius=np.float32(v_pref), pref=(np.float32(vx), np.float32(vy)), out=(np.float32(vel[0]), np.float32(vel[1])))
            if want_lines:
                rec["lines"] = lines
            out.append(rec)
    return out
