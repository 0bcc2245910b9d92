"""Helpers of the device-dataset tests: hand-made observation logs ([F,E,H,4] float32: frame id, prediction id, px, py; +inf where the human
is not visible) and the host side they are held against -- the log written as collect.format_rows lines, one file per env, and
TrajectoriesDataset built per file, files in env order."""
import os

import numpy as np

FIELDS = ("obs_traj", "pred_traj", "obs_traj_rel", "pred_traj_rel", "loss_mask", "loss_mask_rel")


def empty_log(F, E, H, first_frame=0.0):
    """Nobody visible anywhere; frame ids first_frame, first_frame + 1, ...; prediction ids = slot."""
    log = np.empty((F, E, H, 4), np.float32)
    log[..., 0] = (first_frame + np.arange(F, dtype=np.float32))[:, None, None]
    log[..., 1] = np.arange(H, dtype=np.float32)[None, None, :]
    log[..., 2:] = np.inf
    return log


def show(log, rng, f, e, slot, pid):
    """Human `slot` of env e is visible at sample f under prediction id pid, at a position of several float32 digits."""
    log[f, e, slot, 1] = pid
    log[f, e, slot, 2:] = (rng.standard_normal(2) * 7.3).astype(np.float32)


def synthetic_log():
    """F = 40, E = 3, H = 8.
    env 0: samples with nobody visible at the start (0), in the middle (15) and three in a row (27..29); human 2 leaves after sample 8 and
           returns at 11 under a new id; human 5 is seen on and off under one id; at sample 21 everybody comes back under a new id, so the
           windows of samples 16..26 hold nobody throughout; samples 30..39 are the env's one validation window.
    env 1: crowds of 1 to 3, frame ids from 100; one human stays throughout, two come and go, one of them under a new id.
    env 2: fewer than 10 frames."""
    rng = np.random.default_rng(20)
    F, E, H = 40, 3, 8
    log = empty_log(F, E, H)
    for f in range(F):
        if f in (0, 15, 27, 28, 29):
            continue
        for slot in range(6):
            if (slot == 2 and f in (9, 10)) or (slot == 5 and f % 7 == 3):
                continue
            pid = 9 if slot == 2 and 11 <= f < 16 else slot
            show(log, rng, f, 0, slot, pid + 20 if 21 <= f < 27 else pid)
    log[:, 1, :, 0] += 100.0
    for f in range(F):
        show(log, rng, f, 1, 7, 3)
        if f in (1, 2, 30):
            show(log, rng, f, 1, 4, 1)
        if f in (14, 15, 17):
            show(log, rng, f, 1, 0, 11 if f < 17 else 12)
    for f in (2, 3, 4, 5, 6, 30, 31):
        show(log, rng, f, 2, 1, 1)
    return log


def crowded_log(extra_id=False):
    """F = 14, E = 2, H = 64: env 0 shows all 64 humans in every sample (windows of 64 pedestrians), env 1 every other human.  extra_id: human 5
    of env 0 comes back under a new id at sample 6 -- 65 pedestrians in the windows across it."""
    rng = np.random.default_rng(64)
    F, E, H = 14, 2, 64
    log = empty_log(F, E, H)
    for f in range(F):
        for slot in range(H):
            show(log, rng, f, 0, slot, 200 if extra_id and slot == 5 and f >= 6 else 63 - slot)   # ids descend along the slots
            if slot % 2 == 0:
                show(log, rng, f, 1, slot, slot)
    return log


def write_files(log, root):
    """One directory per env holding its one file, as collect_lines + collectData write it."""
    from crowdnav_prediction_attngraph_amd.collect import format_rows
    dirs = []
    for e in range(log.shape[1]):
        d = os.path.join(str(root), "env%d" % e)
        os.makedirs(d)
        with open(os.path.join(d, "%d.txt" % e), "w") as f:
            for k in range(log.shape[0]):
                for line in format_rows(log[k, e]):
                    f.write("%s\n" % line)
        dirs.append(d)
    return dirs


def host_dataset(dirs, mode):
    """TrajectoriesDataset per file, concatenated in env order -> dict of numpy arrays (the six fields, seq_start_end [S,2], frame_id_seq [S],
    seq_env [S]) and the per-env datasets (None where a file yields no sequence)."""
    from crowdnav_prediction_attngraph_amd.gst_train import TrajectoriesDataset
    parts = []
    for d in dirs:
        try:
            parts.append(TrajectoriesDataset(d, mode=mode))
        except RuntimeError as err:
            if "no sequence" not in str(err):
                raise
            parts.append(None)
    if all(p is None for p in parts):
        return None, parts
    out = {k: np.concatenate([getattr(p, k).numpy() for p in parts if p is not None], 0) for k in FIELDS}
    sse, off = [], 0
    for p in parts:
        if p is not None:
            sse += [(s + off, e + off) for s, e in p.seq_start_end]
            off += p.seq_start_end[-1][1]
    out["seq_start_end"] = np.asarray(sse, np.int64)
    out["frame_id_seq"] = np.asarray([v for p in parts if p is not None for v in p.frame_id_seq], np.float64)
    out["seq_env"] = np.asarray([e for e, p in enumerate(parts) if p is not None for _ in range(len(p))], np.int64)
    return out, parts


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_same_dataset(dev_ds, host):
    """Every array bit for bit (no tolerance: both sides are defined by the same rule)."""
    for k in FIELDS:
        got = getattr(dev_ds, k).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == host[k].shape, (k, got.shape, host[k].shape)
        assert np.array_equal(bits(got), bits(host[k])), k
    assert np.array_equal(np.asarray(dev_ds.seq_start_end, np.int64), host["seq_start_end"])
    assert np.array_equal(np.asarray(dev_ds.frame_id_seq, np.float64), host["frame_id_seq"])
    assert np.array_equal(dev_ds.seq_env, host["seq_env"])
    assert len(dev_ds) == len(host["seq_env"])


def window_census(log):
    """What a log contains, counted on the host from the log alone: samples with nobody visible, candidate windows whose ten frames are not
    consecutive, candidates of consecutive frames in which nobody stays throughout, and the crowd sizes of the windows that are sequences."""
    F, E, H, _ = log.shape
    vis = ~np.isinf(log[..., 3])
    empty = off_grid = nobody = 0
    crowds = []
    for e in range(E):
        listed = [f for f in range(F) if vis[f, e].any()]
        empty += F - len(listed)
        for i in range(len(listed) - 9):
            fr = listed[i:i + 10]
            ids = [set(log[f, e, vis[f, e], 1].tolist()) for f in fr]
            if log[fr[-1], e, 0, 0] - log[fr[0], e, 0, 0] != 9:
                off_grid += 1
            elif not set.intersection(*ids):
                nobody += 1
            else:
                crowds.append(len(set.union(*ids)))
    return dict(empty=empty, off_grid=off_grid, nobody=nobody, crowds=crowds)
