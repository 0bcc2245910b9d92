"""orca_lp3_kernel (two linearProgram3 programs per wavefront, csrc/orca.h) against the CPU oracle, bit for bit.

The lane kernel hands every agent whose linearProgram2 is infeasible to orca_lp3_kernel through a list whose order is whatever
atomicAdd made of it; the kernel takes the list two entries at a time.  What can go wrong there shows in the trajectory: an odd
list (the last wavefront's upper half idles), a list of one, an empty list, programs of a single line, programs that fill a
half, a list longer than the grid (the stride walk), a counter that is state of the batch (two batches, a snapshot).  Every case
steps a small batch with test_gpu_env.py's scripted actions taken from the oracle's own observations and compares every output of
every step with assert_array_equal.  The oracle runs once per case, on the CPU; how many programs each step hands over is read
from the oracle's own human records (tests/lp3_util.py) and, for the two lane shapes, asserted: the runs contain steps with 0, 1,
an odd and an even (>= 4) number of hand-overs."""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.lp3_util import handovers, oracle_env_head  # noqa: E402
from tests.test_gpu_env import _actions  # noqa: E402
from tests.test_gpu_env_profile import KEYS, _goals, _oracle_env_head  # noqa: E402
from tests.test_gpu_env_stream_order import _Replay  # noqa: E402

# name -> (E, T, seed, config).  The seeds of the first two were picked on the CPU (the oracle's counts below).
CASES = {
    "h20": (3, 120, 1, dict(human_num=20, random_goal_changing=1)),        # lane kernel <20, 32>
    "h5": (5, 120, 425, dict(human_num=5, random_goal_changing=1)),        # lane kernel <8, 8>
    # one neighbour, one line.  No seed of 200 tried makes such a program infeasible (the line would have to miss the speed disc): the list
    # stays empty for 120 steps, which is what this case then pins; with the robot visible there are two lines and lists of one
    "h2": (2, 120, 425, dict(human_num=2, random_goal_changing=1)),
    "h2_robot": (2, 120, 4, dict(human_num=2, robot_visible=1, random_goal_changing=1)),
    # 31 neighbours + self fill the lane kernel's 32 slots: programs of up to 31 lines, the most a half ever holds
    "h31_robot": (2, 80, 425, dict(human_num=31, robot_visible=1, random_goal_changing=1)),
    # 32 humans and a visible robot: 32 lines per agent -- one slot more than the lane kernel has, so this batch takes the cooperative
    # orca_kernel (lp3_wave, one program per wavefront, the n >= 32 masks of ITS routines)
    "h32_robot": (2, 80, 425, dict(human_num=32, robot_visible=1, random_goal_changing=1)),
    "h20_e4": (4, 120, 425, dict(human_num=20, random_goal_changing=1)),   # stepped with a grid of one workgroup
}
COUNTED = ("h20", "h5")


@functools.lru_cache(maxsize=None)
def _run(name):
    """Reset + T scripted steps of the case's oracle envs: the steps in test_gpu_env_profile._oracle_run's layout, and the number of
    linearProgram3 hand-overs of the batch in every state the humans act on."""
    from oracle import oracle as O
    E, T, seed, kw = CASES[name]
    kw = dict(kw, nenv=E)
    head, ghead = oracle_env_head(), _oracle_env_head()
    oenvs = [O.OracleEnv(O.default_config(**kw), seed + i) for i in range(E)]
    H = kw["human_num"]

    def stack(obs_list):
        return {k: np.stack([ob[k] for ob in obs_list]) for k in KEYS}
    host = stack([oe.reset() for oe in oenvs])
    steps, counts = [dict(obs=host)], []
    n_reset = n_goal = 0
    goals = [_goals(oe, ghead, H)[0] for oe in oenvs]
    for t in range(T):
        counts.append(sum(len(handovers(oe, head)) for oe in oenvs))
        act = _actions(host, t, E)
        out, rew, done, info, md, cnt = [], [], [], [], [], []
        for i, oe in enumerate(oenvs):
            ob, r, d, inf = oe.step(act[i], autoreset=True)
            out.append(ob); rew.append(np.float32(r)); done.append(d); info.append(inf["info"]); md.append(inf["min_dist"]); cnt.append(oe.human_count)
            g = _goals(oe, ghead, H)[0]
            n_reset += int(d)
            n_goal += int(not d and not np.array_equal(g, goals[i]))
            goals[i] = g
        host = stack(out)
        steps.append(dict(act=act, obs=host, rew=np.array(rew), done=np.array(done), info=np.array(info), md=np.array(md), cnt=np.array(cnt)))
    return steps, counts, n_reset, n_goal


def _kinds(counts):
    c = np.array(counts)
    return dict(none=int((c == 0).sum()), one=int((c == 1).sum()), odd=int(((c % 2 == 1) & (c > 1)).sum()), even=int(((c % 2 == 0) & (c >= 4)).sum()))


@pytest.mark.parametrize("name", list(CASES))
def test_the_oracle_runs_hand_over_what_the_cases_are_for(name):
    _, counts, n_reset, n_goal = _run(name)
    k = _kinds(counts)
    print("%s: steps with 0 / 1 / an odd / an even (>= 4) number of hand-overs: %s; %d hand-overs in all, at most %d per step; %d resets, %d goal-change steps"
          % (name, k, sum(counts), max(counts), n_reset, n_goal))
    assert sum(counts) > 0 or name == "h2"
    if name in COUNTED:
        assert k["none"] >= 1 and k["one"] >= 1 and k["odd"] >= 1 and k["even"] >= 1, k


class _Lp3Replay(_Replay):
    """_Replay on this file's oracle runs (its own seeds and the hand-over counts)."""

    def __init__(self, name):
        from crowdnav_prediction_attngraph_amd import _abi as A
        from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
        E, T, seed, kw = CASES[name]
        self.E, self.T, self.way, self.obs = E, T, "plan", None
        self.steps, self.counts, self.n_reset, self.n_goal = _run(name)
        self.env = HipEnvBatch(A.default_env_config(**dict(kw, nenv=E)), E, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["h20", "h5", "h2", "h2_robot", "h31_robot", "h32_robot"])
def test_batches_follow_the_oracle_through_every_list_length(name):
    r = _Lp3Replay(name)
    r.reset()
    r.check(0, r.T)
    r.env.close()


@pytest.mark.gpu
def test_a_list_longer_than_the_grid_is_walked_with_a_stride():
    """CN_LP3_BLOCKS=1 (read when the batch is created): four wavefronts for lists of up to 80 programs."""
    assert max(_run("h20_e4")[1]) > 8   # more pairs than one workgroup has wavefronts
    old = os.environ.get("CN_LP3_BLOCKS")
    os.environ["CN_LP3_BLOCKS"] = "1"
    try:
        r = _Lp3Replay("h20_e4")
    finally:
        if old is None:
            del os.environ["CN_LP3_BLOCKS"]
        else:
            os.environ["CN_LP3_BLOCKS"] = old
    r.reset()
    r.check(0, r.T)
    r.env.close()


@pytest.mark.gpu
def test_two_batches_on_two_streams_keep_their_own_lists():
    side = torch.cuda.Stream()
    ra = _Lp3Replay("h20")
    with torch.cuda.stream(side):
        rb = _Lp3Replay("h5")
        rb.reset()
    ra.reset()
    for t in range(0, min(ra.T, rb.T), 3):   # three steps of one, three of the other
        ra.check(t, t + 3)
        with torch.cuda.stream(side):
            rb.check(t, t + 3)
    with torch.cuda.stream(side):
        rb.env.close()
    ra.env.close()


@pytest.mark.gpu
def test_a_snapshot_mid_run_replays_the_same_steps():
    """The list counter is scratch of the ORCA pass, not part of the snapshot: save, 30 more steps, load, the same 30 again."""
    r = _Lp3Replay("h20")
    r.reset()
    r.check(0, 50)
    snap = r.env.state_dict()
    r.check(50, 80)
    r.env.load_state_dict(snap)
    r.check(50, 80)
    r.env.close()
