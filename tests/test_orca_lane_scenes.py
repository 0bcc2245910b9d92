"""The scenes of tests/orca_lane_scene_util.py are what they are named for -- asserted from the CPU oracle alone.

tests/test_gpu_orca_lane_chain.py holds orca_lane_kernel to the oracle on these states.  That pins the kernel's float filter in front of
the exact coincidence test only if the states really hold neighbours that are equal as float32 and different as float64 (in x only, in
y only, in both), neighbours that are exactly coincident, and neighbours at equal distances.  A scene in which a property it is named
for counts zero fails here."""
import numpy as np
import pytest

from tests import orca_lane_scene_util as L
from tests import orca_scene_util as S


def _env_counts(name):
    from oracle import oracle as O
    cfg = O.default_config(**L.case_config(name))
    names, humans, robot = L.case_scene(name)
    attrs, nds = L.reset_attrs(name)
    return names, [L.property_counts(np.concatenate([humans[e], attrs[e]], axis=1), robot[e], nds[e], cfg) for e in range(len(names))]


@pytest.mark.parametrize("name", list(L.CASES))
def test_the_injected_state_is_a_valid_parked_scene(name):
    names, humans, robot = L.case_scene(name)
    c = L.CASES[name]
    assert humans.shape == (c["E"], c["H"], 6) and robot.shape == (c["E"], 6)
    clearance = S.check_scene(humans, robot)
    rand = bool(c["cfg"].get("randomize_attributes"))
    assert clearance - c["steps"] * 0.25 * (1.5 if rand else 1.0) > 0.3 + (0.5 if rand else 0.3)     # the robot stays out of every collision test


@pytest.mark.parametrize("name", [n for n in L.CASES if any(s in L.SCENES for s in L.CASES[n]["scenes"])])
def test_every_new_scene_holds_what_it_is_named_for(name):
    names, per_env = _env_counts(name)
    seen = 0
    for nm, cnt in zip(names, per_env):
        print("%-18s %-12s " % (name, nm) + "  ".join("%s %d" % kv for kv in cnt.items()))
        if nm in L.SCENES:
            for k in L.SCENES[nm][1]:
                assert cnt[k] >= 1, (name, nm, k, cnt)
            seen += 1
    assert seen >= 1


def test_twins_differ_where_their_kind_says_and_nowhere_as_floats():
    f = np.float32
    for kinds, (dx, dy) in ((("x",), (True, False)), (("y",), (False, True)), (("xy",), (True, True)), (("same",), (False, False))):
        s = L.twins(6, kinds)
        for a in range(0, 6, 2):
            assert (s[a, 0] != s[a + 1, 0]) == dx and (s[a, 1] != s[a + 1, 1]) == dy
            assert f(s[a, 0]) == f(s[a + 1, 0]) and f(s[a, 1]) == f(s[a + 1, 1])
            assert (s[a, 2:4] != s[a + 1, 2:4]).any()       # the relative velocity is not zero


def test_the_centre_ring_is_a_ring_of_exact_ties():
    f = np.float32
    s = L.centre_ring(32)
    d = s[1:, 0:2].astype(f) - s[0, 0:2].astype(f)
    dq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    assert len(set(dq[0:8])) == 1 and len(set(dq[8:16])) == 1 and len(set(dq[16:24])) == 1 and len(set(dq)) == 4
    assert len({tuple(p) for p in s[:, 0:2]}) == 32


def test_the_natural_run_reaches_collisions_and_hand_overs():
    """40 steps of 8 envs x 20 humans: pairs inside their combined radius (pass 2's collision branch, 1 / time step) and infeasible
    programs (the hand-over to orca_lp3_kernel) both occur, in more than one step."""
    _, hand, coll = L.natural_run()
    print("hand-overs per step", hand)
    print("colliding ordered pairs per step", coll)
    assert sum(1 for x in hand if x) >= 2 and sum(1 for x in coll if x) >= 2
