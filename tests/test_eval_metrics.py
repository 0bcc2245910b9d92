"""The bookkeeping of the evaluation protocol (evaluation.EvalAccumulator, torch-op form on CPU tensors) against a plain Python loop over a
synthetic stream of step outputs: envs finish at different steps, some never see Danger, and steps keep arriving after everybody finished."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def _stream(E, T, seed):
    rng = np.random.RandomState(seed)
    end = rng.randint(1, T - 8, size=E)                     # the step (0-based) at which env e's first episode ends
    end[0], end[1] = 0, T - 9                               # one env finishes at once, one last
    steps = []
    for t in range(T):
        done = np.zeros(E, np.uint8)
        info = np.where(rng.rand(E) < 0.3, 4, 0).astype(np.uint8)            # Danger or Nothing
        for e in range(E):
            # the first episode ends at end[e]; afterwards the env runs further episodes that end every few steps (must not count)
            if t == end[e] or (t > end[e] and (t - end[e]) % 5 == 0):
                done[e], info[e] = 1, 1 + (e + t) % 3
        steps.append(dict(done=done, info=info, ep_ret=rng.randn(E), pos=rng.randn(E, 2).astype(np.float32) * 3,
                          dd=np.where(info == 4, rng.rand(E), 0.0)))
    return end, steps


def _python_loop(E, start, steps):
    out = []
    for e in range(E):
        last, n, close, dsum, path, outcome, ret = start[e], 0, 0, 0.0, 0.0, 0, 0.0
        for s in steps:
            n += 1
            path += float(np.linalg.norm(s["pos"][e] - last))
            last = s["pos"][e]
            if s["info"][e] == 4:
                close += 1
                dsum += float(s["dd"][e])
            if s["done"][e]:
                outcome, ret = int(s["info"][e]), float(s["ep_ret"][e])
                break
        out.append((outcome, n, close, dsum, path, ret))
    return out


def test_torch_accumulator_equals_a_python_loop():
    from crowdnav_prediction_attngraph_amd.evaluation import EvalAccumulator
    E, T = 37, 40
    end, steps = _stream(E, T, 5)
    start = np.random.RandomState(9).randn(E, 2).astype(np.float32)
    acc = EvalAccumulator(E, "cpu")
    assert not acc.use_kernel and acc.state.numel() == 8 + 8 * E
    rn = torch.zeros(E, 1, 7)
    rn[:, 0, :2] = torch.from_numpy(start)
    acc.start(rn)
    assert acc.n_active() == E
    left = []
    for s in steps:
        rn = torch.randn(E, 1, 7)
        rn[:, 0, :2] = torch.from_numpy(s["pos"])
        m = acc.update(torch.from_numpy(s["done"]), torch.from_numpy(s["info"]), torch.from_numpy(s["ep_ret"]), rn, torch.from_numpy(s["dd"]))
        assert m.dtype == torch.float32 and m.shape == (E, 1) and m.view(-1).tolist() == [0.0 if d else 1.0 for d in s["done"]]
        left.append(acc.n_active())
    assert left == [int((end > t).sum()) for t in range(T)] and left[-9:] == [0] * 9       # the last 8 steps came after everybody finished
    r = acc.results()
    ref = _python_loop(E, start, steps)
    assert r["outcome"] == [x[0] for x in ref] and all(o in (1, 2, 3) for o in r["outcome"])
    assert r["steps"] == [x[1] for x in ref] == (end + 1).tolist()
    assert r["danger_steps"] == [x[2] for x in ref] and 0 in r["danger_steps"] and max(r["danger_steps"]) > 1
    for key, col in (("danger_sum", 3), ("ep_return", 5)):
        for a, b in zip(r[key], ref):
            assert a == pytest.approx(b[col], rel=1e-12, abs=0.0)
    for a, b in zip(r["path_length"], ref):                # float32 norm summed in float64: numpy and torch round the norm alike to 1 ulp
        assert a == pytest.approx(b[4], rel=1e-6)


def test_steps_after_the_end_change_nothing_and_start_resets():
    from crowdnav_prediction_attngraph_amd.evaluation import EvalAccumulator
    E, T = 5, 30
    _, steps = _stream(E, T, 2)
    acc = EvalAccumulator(E, "cpu")

    def feed(upto):
        acc.start(torch.zeros(E, 1, 7))
        for s in steps[:upto]:
            rn = torch.zeros(E, 1, 7)
            rn[:, 0, :2] = torch.from_numpy(s["pos"])
            acc.update(torch.from_numpy(s["done"]), torch.from_numpy(s["info"]), torch.from_numpy(s["ep_ret"]), rn, torch.from_numpy(s["dd"]))
        return acc.state[8:8 + 7 * E].clone()              # every field but the last position
    a, b = feed(T - 8), feed(T)
    assert acc.n_active() == 0 and torch.equal(a, b)


def test_summary_from_per_episode_danger_sums():
    from crowdnav_prediction_attngraph_amd.evaluation import _summarise
    flat = _summarise([3, 2, 1], [10, 4, 8], [1.0, 2.0, 3.0], [2, 0, 1], [0.1, 0.3, 0.2], [1.0, -1.0, 0.0], 50.0, 0.25, None)
    sums = _summarise([3, 2, 1], [10, 4, 8], [1.0, 2.0, 3.0], [2, 0, 1], None, [1.0, -1.0, 0.0], 50.0, 0.25, None, danger_sums=[0.4, 0.0, 0.2])
    assert flat.keys() == sums.keys()
    for k in flat:
        assert flat[k] == pytest.approx(sums[k], rel=1e-12), k
    none = _summarise([3], [10], [1.0], [0], None, [1.0], 50.0, 0.25, None, danger_sums=[0.0])
    assert math.isnan(none["min_intrusion_dist"])
