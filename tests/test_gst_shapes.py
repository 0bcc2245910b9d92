"""What tests/test_gpu_gst_shapes.py relies on, checked without a GPU: every case of its two tables reaches the launch geometry it is in the
table for (csrc/gst.hip's arithmetic restated in tests/gst_shape_util.py), and the wrapper streams are well conditioned -- no near-tie of the
sort key, no predicted distance at the collision radius, both branches of the frame take-over -- so that the GPU test can hold every env to
the row order and the penalty of the references, with none left out."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd.gst import PretextProcessor  # noqa: E402
from tests import gst_shape_util as U  # noqa: E402

WCASES = list(U.WRAPPER_CASES)


def _ids(cases):
    return ["x".join(str(v) for v in c) for c in cases]


def test_the_case_tables_reach_what_they_claim():
    fmt = ("%-14s TG %2d  tile rows %2d (+%2d padding)  obs tiles %4d turns %2d last %2d groups  decode tiles %4d turns %d last %2d  "
           "lstm<%d> tiles %4d turns %d tail %2d  copy trips %d")
    for table in (U.PREDICT_CASES, U.WRAPPER_CASES):
        for case, claim in table.items():
            p = U.launch_plan(case[0], case[1])
            print(fmt % (case, p["TG"], p["tile_rows"], p["pad_rows"], p["obs_tiles"], p["obs_turns"], p["obs_last_groups"], p["dec_tiles"], p["dec_turns"],
                         p["dec_last_groups"], p["lstm_rows"], p["lstm_tiles"], p["lstm_turns"], p["lstm_tail"], p["copy_trips"]))
            assert claim(p), (case, p)
            # any shape: the tiles cover the groups / nodes, the last one is not empty
            assert 1 <= p["obs_last_groups"] <= p["TG"] and (p["obs_tiles"] - 1) * p["TG"] + p["obs_last_groups"] == 5 * case[0]
            assert 1 <= p["lstm_tail"] <= p["lstm_rows"] and (p["lstm_tiles"] - 1) * p["lstm_rows"] + p["lstm_tail"] == p["N"]
            assert p["tile_rows"] + p["pad_rows"] <= U.GL_ROWS
            if len(case) == 3:
                assert case[0] <= case[2]
    plans = [U.launch_plan(E, H) for E, H in U.PREDICT_CASES]
    # the tables as a whole: both LSTM templates past one turn, every case with a ragged last LSTM tile, both sides of the register-score
    # branch, padded tiles past one turn with a short last tile, every number of copy trips, a handle larger than its batch
    assert {(p["lstm_rows"], p["lstm_turns"]) for p in plans} >= {(32, 2), (80, 1), (80, 2)}
    assert all(p["lstm_tail"] < p["lstm_rows"] for p in plans)
    assert {p["scores_in_registers"] for p in plans} == {True, False}
    assert any(p["pad_rows"] and p["obs_turns"] > 1 and p["obs_last_groups"] < p["TG"] for p in plans)
    assert {U.launch_plan(E, H)["copy_trips"] for E, H, _ in U.WRAPPER_CASES} == {1, 2, 3, 4}
    assert any(E < M for E, _, M in U.WRAPPER_CASES)


def test_predict_inputs_have_their_special_envs_and_both_take_over_branches():
    for (E, H) in U.PREDICT_CASES:
        traj, mask = U.inputs(E, H, H)
        s = U.special_envs(E)
        assert mask[s["present"]].all() and not mask[s["absent"]].any() and mask[s["newest"], :, :4].all() and not mask[s["newest"], :, 4].any()
        assert (traj[mask[..., 0] == 0] == U.INVALID).all() and 0.25 < 1 - mask.mean() < 0.35
        t6, m6 = U.inputs(E, H, H, frames=6)
        took = U.taken_over(U.prep(t6[:, :, :5], m6[:, :, :5]), U.prep(t6[:, :, 1:], m6[:, :, 1:]))
        share = took.mean()
        print("predict %-10s shifted window: %.3f of the groups (e, 1..3) taken over" % ((E, H), share))
        assert 0.1 <= share <= 0.9
        # a human seen in frames t and 4 but not in frame 5 (or the other way round) changes m_rel of the group: it is encoded again
        m = m6[..., 0]
        changed = np.stack([((m[:, :, t] > 0) & (m[:, :, 4] != m[:, :, 5])).any(axis=1) for t in (1, 2, 3)], axis=1)
        assert changed.any() and not took[changed].any()


@functools.lru_cache(maxsize=None)
def _oracle(case):
    E, H, _ = case
    return U.oracle_run(E, H, U.WRAPPER_SEEDS[case], U.sliced_envs(E, H))


@pytest.mark.parametrize("case", WCASES, ids=_ids(WCASES))
def test_wrapper_stream_row_order_is_well_conditioned(case):
    """No two sort keys of an env within 8 float32 ulp unless they are the same bits, and the torch path and the numpy oracle order every env's
    rows alike at every step (on the CPU; events included).  The order does not depend on the predictor, so gst_oracle.PretextWrapper itself runs
    on the envs the GPU test follows with it, and its ordering expression (stable argsort of numpy's float32 norm) on all of them."""
    E, H, _ = case
    stream = U.wrapper_stream(E, H, U.WRAPPER_STEPS, U.WRAPPER_SEEDS[case])
    bad, gap = U.key_condition(stream)
    print("wrapper %-14s near-ties %d, smallest relative gap of unequal keys %.3g" % (case, bad, gap))
    assert bad == 0
    s = U.stream_envs(E, H)
    if H >= 3:
        k32, _ = U.sort_keys(np.stack([o["spatial_edges"][s["mirror"]] for o in stream]))
        assert (k32[:, 0] == k32[:, 1]).all() and (k32[:, 0] == k32[:, 2]).all(), "the mirrored humans tie exactly"
    assert all(o["visible_masks"][s["visible"]].all() and not o["visible_masks"][s["hidden"]].any() for o in stream)
    m1, m2 = U.wrapper_models(H)
    w = PretextProcessor(m1, E, H, 5, 0.3, 0.3, U.PENALTY, torch.device("cpu"), use_hip=False)
    differing, idx = 0, U.sliced_envs(E, H)
    for t, (o, want) in enumerate(zip(stream, _oracle(case))):
        se, rews = w.process({k: torch.from_numpy(o[k].copy()) for k in ("robot_node", "spatial_edges", "visible_masks")}, torch.from_numpy(o["rews_in"].copy()))
        order = np.argsort(np.linalg.norm(o["spatial_edges"][:, :, :2], axis=-1), axis=1, kind="stable")
        differing += int((se.numpy()[:, :, :2] != np.take_along_axis(o["spatial_edges"][:, :, :2], order[:, :, None], axis=1)).any(axis=(1, 2)).sum())
        differing += int((se.numpy()[idx][:, :, :2] != want["se"][:, :, :2]).any(axis=(1, 2)).sum())
        assert np.array_equal(order[idx], want["order"])

        def on_history():
            sd = w.state_dict()
            sd["traj"] = sd["traj"] + 0.125
            w.load_state_dict(sd)

        def on_weights():
            w.pred = m2
        U.apply_event(t, on_history, on_weights, w.reset_buffers)
    assert differing == 0


def test_wrapper_streams_keep_predictions_off_the_collision_radius_and_penalise_some():
    """On the envs the GPU test follows with the oracle: no predicted distance of the float64 oracle within 1e-3 of robot_radius + human_radius
    (a float32 path then takes the same side), and some env-steps are penalised."""
    penalised = total = 0
    for case in WCASES:
        E, H, _ = case
        idx = U.sliced_envs(E, H)
        assert len(idx) <= 8
        n = 0
        for want in _oracle(case):
            d = want["dist"][want["valid"]]
            assert d.size == 0 or float(np.abs(d - U.DIST).min()) >= 1e-3, (case, float(np.abs(d - U.DIST).min()))
            n += int((((want["dist"] < U.DIST) & want["valid"][..., None]).any(axis=(1, 2))).sum())
        print("wrapper %-14s penalised env-steps %d of %d" % (case, n, len(idx) * U.WRAPPER_STEPS))
        penalised += n
        total += len(idx) * U.WRAPPER_STEPS
    assert penalised > 0


@pytest.mark.parametrize("case", WCASES, ids=_ids(WCASES))
def test_wrapper_streams_take_over_some_groups_and_encode_others(case):
    E, H, _ = case
    share, listed = U.reuse_share(E, H, U.WRAPPER_SEEDS[case])
    p = U.launch_plan(E, H)
    tiles, last = [p["listed_tiles"](n) for n in listed], [p["listed_last_groups"](n) for n in listed]
    print("wrapper %-14s taken over %.3f; listed tiles per step %s, groups in the last tile %s" % (case, share, tiles, last))
    assert 0.1 <= share <= 0.9
    # what the listed-tile pass of the case reaches, over its own stream
    if case == (5, 1, 64):
        assert max(tiles) == 1 and max(last) < p["TG"]
    if case == (97, 21, 97):
        assert any(n < p["TG"] for n in last) and max(tiles) <= U.WGS
    if case == (60, 50, 64):
        assert max(tiles) > U.WGS > min(tiles)
    if case == (129, 64, 129):
        assert min(tiles) > U.WGS


@pytest.mark.parametrize("H", U.CV_SIZES)
def test_constant_velocity_scenes_hold_every_first_colliding_horizon(H):
    stream = U.cv_stream(H)
    hist = U.History(7, H)
    seen = set()
    for t, o in enumerate(stream):
        hist.push(o)
        se, rews, first = U.cv_expected(hist, o)
        if t == 0:
            assert (first == -1).all() and np.array_equal(rews, o["rews_in"]), "nobody is predicted from a single frame"
            continue
        assert list(first[:6]) == [0, 1, 2, 3, 4, -1] and first[6] == (1 if H >= 3 else 2)
        seen |= set(first.tolist())
        want = np.where(first >= 0, U.PENALTY / 2.0 ** (first + 2), 0).astype(np.float32)
        assert np.array_equal(rews, o["rews_in"] + want)
        key, _ = U.sort_keys(se)
        assert (np.diff(key, axis=1) >= 0).all()
        if H >= 3:
            assert (np.diff(key, axis=1) == 0).any(), "tied keys"
    assert seen == {-1, 0, 1, 2, 3, 4}
