"""Shared by tests/test_gst_horizon.py (CPU) and the tests/test_gpu_gst_horizon*.py files: what the prediction-horizon tests need on top of
tests/gst_shape_util.py -- the horizons and shapes of the cases, predictors of a horizon, the observation streams of the wrapper cases at an
edge width of 2 (P + 1), the constant-velocity stream and its closed form restated for a horizon, ragged training batches of 5 + P steps and a
hand-made observation log."""
import functools

import numpy as np

from tests import gst_shape_util as U

HORIZONS = (1, 3, 8)
INVALID, DIST, PENALTY = U.INVALID, U.DIST, U.PENALTY
# (E, H) of the predict cases -> the property of U.launch_plan(E, H) the case is in the table for
PREDICT_CASES = {
    (155, 21): lambda p: ((p["lstm_rows"], p["lstm_tail"]) == (32, 23) and p["lstm_tail"] < p["lstm_rows"] and p["obs_turns"] == 2 and p["pad_rows"] == 1
                          and not p["scores_in_registers"]),
    (5, 64): lambda p: (p["TG"], p["copy_trips"], p["lstm_tail"]) == (1, 4, 32) and p["lstm_tiles"] == 10,
}
WRAPPER_CASE, WRAPPER_SEED = (97, 21, 97), U.WRAPPER_SEEDS[(97, 21, 97)]
CV_SIZES, CV_V = U.CV_SIZES, U.CV_V


def model(seed, P):
    """U.model(seed) decoding P steps: the parameters do not depend on the horizon."""
    m = U.model(seed)
    m.pred_len = P
    return m


def marker(H, P):
    """What a visible row carries in columns 2 .. 2P+1 before the wrapper writes them: 15 + a multiple of 2^-10, different in every row and column."""
    return (15 + (np.arange(H)[:, None] * 2 * P + np.arange(2 * P)[None, :] + 1) / 1024.0).astype(np.float32)


def widen(o, P):
    """An observation of U.wrapper_stream / U.cv_stream (edge width 12) at edge width 2 (P + 1): the same positions, visibility and rewards."""
    se12 = o["spatial_edges"]
    E, H, _ = se12.shape
    se = np.empty((E, H, 2 * (P + 1)), np.float32)
    se[:, :, :2] = se12[:, :, :2]
    se[:, :, 2:] = marker(H, P)
    se[~o["visible_masks"]] = 15.0                         # the stream's invisible rows are 15.0 throughout
    out = dict(o, spatial_edges=se)
    se.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def wrapper_stream(E, H, steps, seed, P):
    """U.wrapper_stream at edge width 2 (P + 1)."""
    return tuple(widen(o, P) for o in U.wrapper_stream(E, H, steps, seed))


@functools.lru_cache(maxsize=None)
def cv_stream(H, P, steps=6):
    """U.cv_stream restated for a horizon: P + 2 envs for the constant-velocity predictor with v = CV_V, robot at (0.5, -0.25), nobody moves.
    Human 0 of env k (k < P) stands where its prediction first comes within DIST of the robot at horizon k (0.5 m after k + 1 steps, 0.78 m the
    step before); env P has nobody near; env P + 1 has two humans arriving at horizons min(3, P - 1) and min(1, P - 1) (H >= 3).  The other
    humans stand far away in mirrored pairs (tied keys).  Human H - 1 of every env is invisible in odd steps (H >= 3), so it is never predicted
    and keeps its input columns."""
    f32 = np.float32
    E = P + 2
    vx, vy = CV_V
    rob = np.tile(f32([0.5, -0.25]), (E, 1))
    rel = np.empty((E, H, 2), f32)
    for h in range(H):
        j = (h + 1) // 2
        rel[:, h] = f32([(4 + 0.5 * j) * (1 if h % 2 else -1), 3 + 0.25 * j])

    def arriving(k):
        return f32([0.5 - (k + 1) * vx, 0 - (k + 1) * vy])
    for k in range(P):
        rel[k, 0] = arriving(k)
    if H >= 3:
        rel[P + 1, 0], rel[P + 1, 2] = arriving(min(3, P - 1)), arriving(min(1, P - 1))
    else:
        rel[P + 1, 0] = arriving(min(2, P - 1))
    rs = np.random.RandomState(5)
    out = []
    for t in range(steps):
        vis = np.ones((E, H), bool)
        if H >= 3:
            vis[:, H - 1] = t % 2 == 0
        se = np.empty((E, H, 2 * (P + 1)), f32)
        se[:, :, :2] = rel
        se[:, :, 2:] = marker(H, P)
        o = dict(robot_node=U.robot_node(rob), spatial_edges=se, visible_masks=vis, rews_in=rs.uniform(-1, 1, E).astype(f32))
        for a in o.values():
            a.setflags(write=False)
        out.append(o)
    return tuple(out)


def cv_expected(hist, o, P, v=CV_V):
    """U.cv_expected over P horizons: (spatial_edges sorted, rewards, first colliding horizon per env or -1), float32 in the kernels' order."""
    f32 = np.float32
    E, H = hist.E, hist.H
    rxy = o["robot_node"][:, 0, :2]
    last = hist.traj[4]
    om = hist.out_mask()
    se = o["spatial_edges"].copy()
    pen = np.zeros((E, H), f32)
    first = np.full((E, H), 99)
    acc = np.zeros(2, f32)
    for k in range(P):
        acc = (acc + f32(v)).astype(f32)
        d = ((acc[None, None, :] + last).astype(f32) - rxy[:, None, :]).astype(f32)
        coll = om & (np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) < f32(DIST))
        pen = np.where(coll, np.minimum(pen, f32(PENALTY / 2 ** (k + 2))), pen)
        first = np.where(coll, np.minimum(first, k), first)
        se[:, :, 2 + 2 * k:4 + 2 * k] = np.where(om[..., None], d, se[:, :, 2 + 2 * k:4 + 2 * k])
    key, _ = U.sort_keys(se)
    order = np.argsort(key, axis=1, kind="stable")
    first = first.min(1)
    return np.take_along_axis(se, order[:, :, None], axis=1), (o["rews_in"] + pen.min(1)).astype(f32), np.where(first == 99, -1, first)


def cv_plan(H, P):
    """What the constant-velocity case of (H, P) reaches, on the host alone: the set of first colliding horizons over the stream, the key
    violations of U.key_condition, and how many rows keep their input columns."""
    hist, seen, kept = U.History(P + 2, H), set(), 0
    stream = cv_stream(H, P)
    for o in stream:
        hist.push(o)
        seen |= set(cv_expected(hist, o, P)[2].tolist())
        kept += int((~hist.out_mask()).sum())
    return seen, U.key_condition(stream)[0], kept


def ragged_case(B, N, seed, P):
    """tests/gst_dropout_ref.ragged_case for a horizon: B sequences of N pedestrians over 5 + P steps, one present throughout, one without a last
    observed step, one never present, -999 where missing; weights drawn on the CPU.  -> (model of pred_len P on the CPU, lm [B,N,5+P],
    v_obs [B,5,N,2], v_pred [B,P,N,2])."""
    import torch
    from crowdnav_prediction_attngraph_amd.gst import GSTPredictor
    gw = torch.Generator().manual_seed(100 + seed)
    torch.manual_seed(100 + seed)
    m = GSTPredictor(5, P)
    with torch.no_grad():
        for q in m.parameters():
            q.add_(0.05 * torch.randn(q.shape, generator=gw))
    g = torch.Generator().manual_seed(seed)
    lm = (torch.rand(B, N, 5 + P, generator=g) > 0.25).float()
    lm[:, 0] = 1.0
    lm[:, 1, 4] = 0.0
    if N > 2:
        lm[:, 2, :] = 0.0
    v_obs = torch.where(lm[:, :, :5].permute(0, 2, 1).unsqueeze(-1) > 0, 0.4 * torch.randn(B, 5, N, 2, generator=g), torch.full((B, 5, N, 2), -999.0))
    v_pred = torch.where(lm[:, :, 5:].permute(0, 2, 1).unsqueeze(-1) > 0, 0.4 * torch.randn(B, P, N, 2, generator=g), torch.full((B, P, N, 2), -999.0))
    return m, lm, v_obs, v_pred


def ragged_crowds(sizes, seed, P):
    """ragged_case with a crowd size per sequence: padded to the largest with absent pedestrians (zeros, values and mask), as the wrappers pad."""
    m, lm, v_obs, v_pred = ragged_case(len(sizes), max(sizes), seed, P)
    for b, n in enumerate(sizes):
        lm[b, n:] = 0.0
        v_obs[b, :, n:] = 0.0
        v_pred[b, :, n:] = 0.0
    return m, lm, v_obs, v_pred


def hand_made_log():
    """F = 30 observations, E = 3 envs, H = 5 humans ([F,E,H,4] float32: frame id, prediction id, px, py; +inf where not visible).
    env 0: human 0 throughout; human 1 leaves at samples 9, 10 and returns under a new id; human 2 on and off; nobody visible at samples 0 and 17;
           human 3 appears from sample 20.
    env 1: frame ids from 100; one human throughout, one seen in samples 3 .. 14 only.
    env 2: seven frames -- too short for any window of 5 + 3."""
    from tests import gst_data_util as D
    rng = np.random.default_rng(31)
    F, E, H = 30, 3, 5
    log = D.empty_log(F, E, H)
    for f in range(F):
        if f in (0, 17):
            continue
        D.show(log, rng, f, 0, 0, 0)
        if f not in (9, 10):
            D.show(log, rng, f, 0, 1, 7 if f > 10 else 1)
        if f % 4 != 2:
            D.show(log, rng, f, 0, 2, 2)
        if f >= 20:
            D.show(log, rng, f, 0, 3, 3)
    log[:, 1, :, 0] += 100.0
    for f in range(F):
        D.show(log, rng, f, 1, 4, 4)
        if 3 <= f <= 14:
            D.show(log, rng, f, 1, 1, 1)
    for f in (2, 3, 4, 5, 6, 20, 21):
        D.show(log, rng, f, 2, 1, 1)
    return log


def walking_log():
    """F = 14 observations of one env, H = 5: pedestrians walking at 0.1 .. 0.3 m per frame with 0.02 m of noise (displacements of the size of the
    simulator's), human 0 throughout, human 1 absent in frames 5 and 6, human 3 from frame 4 on, human 4 never.  At 5 + 3 frames: seven windows,
    six of them training sequences and one for validation."""
    from tests import gst_data_util as D
    rng = np.random.default_rng(14)
    F, H = 14, 5
    log = D.empty_log(F, 1, H)
    pos, vel = rng.uniform(-4, 4, (H, 2)), rng.uniform(0.1, 0.3, (H, 2)) * rng.choice([-1.0, 1.0], (H, 2))
    for f in range(F):
        pos = pos + vel + 0.02 * rng.standard_normal((H, 2))
        for h in range(4):
            if (h == 1 and f in (5, 6)) or (h == 3 and f < 4):
                continue
            log[f, 0, h, 1] = h
            log[f, 0, h, 2:] = pos[h].astype(np.float32)
    return log


def host_dataset(dirs, mode, P):
    """tests/gst_data_util.host_dataset with TrajectoriesDataset(obs_seq_len=5, pred_seq_len=P)."""
    from crowdnav_prediction_attngraph_amd.gst_train import TrajectoriesDataset
    from tests import gst_data_util as D
    parts = []
    for d in dirs:
        try:
            parts.append(TrajectoriesDataset(d, obs_seq_len=5, pred_seq_len=P, mode=mode))
        except RuntimeError as err:
            if "no sequence" not in str(err):
                raise
            parts.append(None)
    if all(p is None for p in parts):
        return None, parts
    out = {k: np.concatenate([getattr(p, k).numpy() for p in parts if p is not None], 0) for k in D.FIELDS}
    sse, off = [], 0
    for p in parts:
        if p is not None:
            sse += [(s + off, e + off) for s, e in p.seq_start_end]
            off += p.seq_start_end[-1][1]
    out["seq_start_end"] = np.asarray(sse, np.int64)
    out["frame_id_seq"] = np.asarray([v for p in parts if p is not None for v in p.frame_id_seq], np.float64)
    out["seq_env"] = np.asarray([e for e, p in enumerate(parts) if p is not None for _ in range(len(p))], np.int64)
    return out, parts


GOLDEN_HORIZONS = (3, 8)


def golden(P):
    """(tests/golden/gst_horizon_p<P>_h8.npz, GSTPredictor(5, P) on the CPU with the fixture's formula weights)."""
    import json
    import os
    import sys
    import torch
    from crowdnav_prediction_attngraph_amd.gst import GSTPredictor
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if here not in sys.path:
        sys.path.insert(0, here)
    from make_golden_gst import gst_formula_state_dict
    z = np.load(os.path.join(here, "gst_horizon_p%d_h8.npz" % P))
    meta = json.loads(str(z["meta"]))
    assert meta["pred_seq_len"] == P
    m = GSTPredictor(5, P)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v)) for k, v in meta["shapes"].items()]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in gst_formula_state_dict({k: tuple(v) for k, v in meta["shapes"].items()}).items()})
    return z, m
