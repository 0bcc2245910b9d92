"""The hand-built ORCA scenes (tests/orca_scene_util.py) are what they are built to be -- asserted from the CPU oracle alone.

tests/test_gpu_orca_scenes.py injects these states into device batches and holds orca_lane_kernel / orca_lp3_kernel / orca_kernel to the
oracle on them.  That says something only if the states really hold what the simulator's own trajectories never do: neighbours at
equal distances (the tie rule of the sorting networks), parallel ORCA lines (`parallel` / `pfail`, `par` / `skip`), agents on their
goal (the zero optimisation direction), neighbour lists with +inf keys, coincident neighbours, collisions on and beside the
threshold, and hand-over lists that are full.  Per case this file counts them in the injected state and prints the table DESIGN.md
shows (pytest -s)."""
import functools

import numpy as np
import pytest

from tests import orca_scene_util as S


@functools.lru_cache(maxsize=None)
def _counts(name):
    """-> (per-env scene names, per-env counts, velocities [E][H][2]) of the state the case injects."""
    from oracle import oracle as O
    cfg = O.default_config(**S.case_config(name))
    names, humans, robot = S.case_scene(name)
    attrs, nds = S.oracle_reset_attrs(name)
    per_env, vels = [], []
    for e in range(len(names)):
        vel, c = S.env_reference(cfg, np.concatenate([humans[e], attrs[e]], axis=1), robot[e], nds[e], counts=True)
        per_env.append(c)
        vels.append(vel)
    return names, per_env, np.stack(vels)


def _total(per_env):
    return {k: sum(c[k] for c in per_env) for k in per_env[0]}


@pytest.mark.parametrize("name", list(S.CASES))
def test_the_injected_state_is_a_valid_parked_scene(name):
    names, humans, robot = S.case_scene(name)
    c = S.CASES[name]
    assert humans.shape == (c["E"], c["H"], 6) and robot.shape == (c["E"], 6)
    assert c["E"] * c["H"] > 64 and (c["E"] * c["H"]) % 64 != 0 or "lp3_blocks" in c
    clearance = S.check_scene(humans, robot)     # finite, inside the arena, the robot >= 2 m from everybody and from its goal
    # ... and out of every collision test of the steps that follow: ORCA keeps a human below its v_pref (1, or up to 1.5 when drawn), a
    # step takes 0.25 s, and the robot (radius 0.3) touches a human (0.3, or up to 0.5) at the sum of the radii
    rand = bool(c["cfg"].get("randomize_attributes"))
    assert clearance - c["steps"] * 0.25 * (1.5 if rand else 1.0) > 0.3 + (0.5 if rand else 0.3)
    assert np.isfinite(_counts(name)[2]).all()
    if c["kind"] == "scenes" and c["E"] >= len(S.SCENE_ORDER):
        assert set(names) == set(S.SCENE_ORDER)


@pytest.mark.parametrize("name", list(S.CASES))
def test_every_scene_holds_what_it_is_built_for(name):
    names, per_env, _ = _counts(name)
    c = S.CASES[name]
    n_others = c["H"] - 1 + c["rv"]
    tot = _total(per_env)
    print("%-16s E=%-3d H=%-2d robot_visible=%d  " % (name, c["E"], c["H"], c["rv"]) + "  ".join("%s %d" % (k, tot[k]) for k in S.COUNTS + S.EVENTS + ("pfail_decides",)))
    if c["cfg"].get("randomize_attributes"):
        return      # the radii are the reset's: only the totals below are asked of this case
    for nm, cnt in zip(names, per_env):
        _, wanted, min_n = S.SCENES[nm]
        if c["H"] >= min_n and n_others >= 2:
            for k in wanted:
                assert cnt[k] >= 1, (name, nm, k, cnt)
        if c["H"] >= 7 and nm == "ring_tight":
            assert cnt["handovers"] == c["H"], (name, cnt)                       # a ring on which every agent is infeasible
        if c["H"] >= 7 and nm == "ring_collide":
            assert cnt["collisions"] == c["H"] * (c["H"] - 1), (name, cnt)       # ... and one on which every neighbour collides
        if c["H"] >= 7 and nm == "row":
            assert cnt["short_list"] >= 2, (name, cnt)                           # both ends of the row lose neighbours: +inf keys are sorted


def test_the_scenes_one_by_one_at_20_humans():
    """The scene table of DESIGN.md: 20 agents, radius 0.3, v_pref 1, neighbour distance 10, the robot not visible."""
    names, per_env, _ = _counts("h20_rv0")
    for nm, cnt in list(zip(names, per_env))[:len(S.SCENE_ORDER)]:
        print("%-13s " % nm + "  ".join("%s %d" % (k, cnt[k]) for k in S.COUNTS + S.EVENTS + ("pfail_decides",)))
    d = dict(zip(names, per_env))
    assert d["ring4"]["handovers"] == 0 and d["ring4"]["collisions"] == 0 and d["ring4"]["ties"] >= 20      # feasible, and full of ties
    assert d["control"]["ties"] == 0 and d["control"]["parallel"] == 0 and d["control"]["handovers"] >= 10   # generic, and mostly linearProgram3


@pytest.mark.parametrize("name", ["h8_rv0", "h19_rv1", "h20_rv0", "h31_rv1", "h32_rv0", "h32_rv1", "h40_rv0", "random_attrs"])
def test_a_batch_holds_every_property_at_once(name):
    """One batch per kernel (<8,8>, <20,32>, <32,32>, the cooperative one) and the randomised one: every count and every branch event at
    least once.  From 19 humans on the clusters of the `stacks` scene are complete, and with them the programs in which `pfail` of
    linearProgram3's inner linearProgram1 decides the velocity (lp_events reruns them without it: the velocity changes)."""
    tot = _total(_counts(name)[1])
    small = S.CASES[name]["H"] < 19 or name == "random_attrs"
    for k in S.COUNTS + (("lp_parallel", "lp_pfail", "lp3_par", "lp3_restore") if small else S.EVENTS + ("pfail_decides",)):
        assert tot[k] >= 1, (name, k, tot)


@pytest.mark.parametrize("name", ["full_odd", "full_one_block"])
def test_the_full_list_cases_hand_over_every_agent(name):
    """A condition on the input: the oracle needs linearProgram3 for every agent of every env, so the device's list holds E * H entries."""
    names, per_env, _ = _counts(name)
    c = S.CASES[name]
    assert [cnt["handovers"] for cnt in per_env] == [c["H"]] * c["E"]
    if name == "full_odd":
        assert (c["E"] * c["H"]) % 2 == 1


def test_the_threshold_pairs_sit_on_their_thresholds():
    f = np.float32
    s = S.boundaries(10)
    cr = f(0.3 + 0.01 + 0.15) + f(0.3 + 0.01 + 0.15)
    d = [f(s[2 * k + 1, 0]) - f(s[2 * k, 0]) for k in range(5)]
    assert d[0] * d[0] == cr * cr and d[1] == np.nextafter(cr, f(0)) and d[2] == np.nextafter(cr, f(1))
    assert not (d[1] * d[1] > cr * cr) and d[2] * d[2] > cr * cr           # collision, collision, none
    nd = f(10.0)
    assert d[3] * d[3] == nd * nd                                           # `distSq < rangeSq` fails: not a neighbour
    assert d[4] * d[4] < nd * nd and not (np.nextafter(d[4], f(11)) ** 2 < nd * nd)   # the last float32 distance that is one


def test_the_goal_kinds_of_the_mixed_scene():
    s = S.mixed(8)
    g = s[:, 4:6] - s[:, 0:2]
    d = np.sqrt((g * g).sum(1))
    assert d[0] == 0.0 and not s[0, 2:4].any() and d[1] == 0.5 and d[2] == 1.0 and d[4] == 0.0 and s[4, 2:4].any()
    assert np.sqrt((s[3, 2:4] ** 2).sum()) > 1.0 and (d[5:] > 1.0).all()


def test_handovers_still_reads_the_list_the_oracle_steps_with():
    """lp3_util.handovers builds its lists with orca_scene_util.orca_inputs now.  Its `out` is the velocity of a program rebuilt from the
    human records; the oracle's own step must give the same human the same velocity (unless the step replaced that human)."""
    import ctypes as C
    from oracle import oracle as O
    from tests.lp3_util import handovers, oracle_env_head
    oe = O.OracleEnv(O.default_config(human_num=20, nenv=3, robot_visible=1, random_goal_changing=1), 1)
    oe.reset()
    head = oracle_env_head()
    st = C.cast(oe._h, C.POINTER(head)).contents
    checked = 0
    for t in range(60):
        recs = handovers(oe, head, want_lines=True)
        goals = [(st.humans[j].gx, st.humans[j].gy) for j in range(20)]
        _, _, done, _ = oe.step(np.zeros(2, dtype=np.float32), autoreset=True)
        if done:
            continue
        for r in recs:
            h = st.humans[r["agent"]]
            assert r["lines"].shape == (r["nn"], 4) and 0 <= r["line_fail"] < r["nn"] and r["radius"] == np.float32(1.0)
            if (h.gx, h.gy) == goals[r["agent"]]:
                assert (np.float32(h.vx), np.float32(h.vy)) == r["out"], (t, r["agent"])
                checked += 1
    assert checked >= 20, checked
