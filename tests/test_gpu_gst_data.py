"""-m gpu: the GST predictor's training data on the device (csrc/gst_data.hip) and the device-resident epoch of gst_train.train.

The sequences cn_gst_data_frames / _count / _fill cut out of an observation log are held, bit for bit, against TrajectoriesDataset built from
the text files collect.format_rows writes from the same log (hand-made logs with every corner of the rule, and logs of the simulator); the
minibatch of cn_gst_gather_batch against the host assembly (rotate_graph on the CPU, HipGstEvaluator._stack's padding); the epoch of
train(dataset=...) against today's per-item loop (batch size 1: equal weights and history) and against explicit HipGstTrainer calls on
host-assembled batches (batch size 8).  No tolerance anywhere: both sides are defined by the same rule."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import gst_data_util as U  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = (None, "train", "val")


def _compare_all_modes(log, tmp):
    """from_log against the files of the same log in the three modes ('test' is 'val'); -> the host dict of mode None."""
    from crowdnav_prediction_attngraph_amd.gst_train import DeviceTrajectories
    dirs = U.write_files(log, tmp)
    dev_log = torch.from_numpy(log).cuda()
    first = None
    for mode in MODES:
        host, _ = U.host_dataset(dirs, mode)
        assert host is not None, mode
        U.assert_same_dataset(DeviceTrajectories.from_log(dev_log, mode=mode), host)
        first = host if first is None else first
    U.assert_same_dataset(DeviceTrajectories.from_log(dev_log, mode="test"), U.host_dataset(dirs, "test")[0])
    return first


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """The hand-made log, its files and the host dataset of every mode: built once, shared, left unchanged."""
    log = U.synthetic_log()
    dirs = U.write_files(log, tmp_path_factory.mktemp("gstdata_syn"))
    return log, dirs, {mode: U.host_dataset(dirs, mode) for mode in MODES}


def test_hand_made_log_gives_the_host_dataset_bit_for_bit(synthetic):
    from crowdnav_prediction_attngraph_amd.gst_train import DeviceTrajectories
    log, dirs, hosts = synthetic
    census = U.window_census(log)
    assert census["empty"] >= 5 and census["off_grid"] >= 1 and census["nobody"] >= 2 and min(census["crowds"]) == 1 and max(census["crowds"]) >= 7
    assert hosts[None][1][2] is None                       # the env with fewer than 10 frames has no sequence
    dev_log = torch.from_numpy(log).cuda()
    for mode in MODES:
        ds = DeviceTrajectories.from_log(dev_log, mode=mode)
        U.assert_same_dataset(ds, hosts[mode][0])
    U.assert_same_dataset(DeviceTrajectories.from_log(dev_log, mode="test"), hosts["val"][0])
    with pytest.raises(RuntimeError):
        DeviceTrajectories.from_log(dev_log, mode="validation")
    # a subset of the envs, in the caller's order; the items are the host class's 12 entries
    sub = DeviceTrajectories.from_log(dev_log, env_ids=[1, 0])
    parts = hosts[None][1]
    assert sub.seq_env.tolist() == [1] * len(parts[1]) + [0] * len(parts[0])
    for i in (0, len(parts[1]) - 1, len(parts[1]), len(sub) - 1):
        ref = parts[1][i] if i < len(parts[1]) else parts[0][i - len(parts[1])]
        got = sub[i]
        assert len(got) == len(ref) == 12
        for a, b in zip(got, ref):
            assert a.is_cuda and np.array_equal(U.bits(a.cpu().numpy()), U.bits(b.numpy()))


def test_windows_of_64_pedestrians(tmp_path):
    host = _compare_all_modes(U.crowded_log(), tmp_path)
    assert np.diff(host["seq_start_end"], axis=1).max() == 64


def test_frame_ids_that_step_by_two_hold_no_sequence(tmp_path):
    from crowdnav_prediction_attngraph_amd.gst_train import DeviceTrajectories
    log = U.synthetic_log()
    log[..., 0] *= 2.0
    assert U.host_dataset(U.write_files(log, tmp_path), None)[0] is None
    with pytest.raises(RuntimeError, match="no sequence"):
        DeviceTrajectories.from_log(torch.from_numpy(log).cuda())


def test_the_three_refusals_raise():
    from crowdnav_prediction_attngraph_amd.gst_train import DeviceTrajectories
    build = lambda log: DeviceTrajectories.from_log(torch.from_numpy(log).cuda())   # noqa: E731
    boundary = U.synthetic_log()
    boundary[25:, 1, :, 0] -= 125.0                        # env 1 starts a new episode at sample 25: its frame ids fall back to 0
    with pytest.raises(RuntimeError, match="strictly increase"):
        build(boundary)
    short = U.synthetic_log()
    short[31, 2, :, 0] = short[30, 2, :, 0]                # also in an env too short for any window
    with pytest.raises(RuntimeError, match="strictly increase"):
        build(short)
    twice = U.synthetic_log()
    twice[5, 0, 4, 1] = twice[5, 0, 1, 1]                  # two visible rows of one sample under one id
    with pytest.raises(RuntimeError, match="multiple locations"):
        build(twice)
    hidden = U.synthetic_log()
    hidden[5, 0, 7, 1] = hidden[5, 0, 1, 1]                # a row that is not visible may carry any id
    build(hidden)
    with pytest.raises(RuntimeError, match="more than 64"):
        build(U.crowded_log(extra_id=True))


def _simulator_log(human_num, samples):
    from crowdnav_prediction_attngraph_amd import _abi as A
    from crowdnav_prediction_attngraph_amd.hip import HipEnvBatch
    env = HipEnvBatch(A.default_env_config(human_num=human_num, env_kind=3, robot_policy=1, nenv=4), 4, 425)
    log = torch.empty(samples, 4, human_num, 4, device=env.device)
    act = torch.zeros(4, 2, device=env.device)
    pred = env.reset()["spatial_edges"]
    for k in range(samples):
        log[k].copy_(pred)
        pred = env.step(act)[0]["spatial_edges"]
    env.close()
    return log.cpu().numpy()


def test_simulator_log_of_small_crowds(tmp_path):
    log = _simulator_log(5, 200)
    census = U.window_census(log)
    # the log must keep its corners, or this test checks less than it says
    assert census["empty"] >= 1 and census["off_grid"] >= 1 and census["nobody"] >= 1 and min(census["crowds"]) < 4, {k: v for k, v in census.items() if k != "crowds"}
    _compare_all_modes(log, tmp_path)


def test_simulator_log_of_twenty_humans(tmp_path):
    host = _compare_all_modes(_simulator_log(20, 150), tmp_path)
    assert len(host["seq_env"]) == 4 * 141 and np.diff(host["seq_start_end"], axis=1).max() > 20


def test_collect_log_is_what_collect_lines_formats():
    from crowdnav_prediction_attngraph_amd import config as C
    from crowdnav_prediction_attngraph_amd.collect import CollectVecEnv, collect_lines, collect_log, format_rows
    cfg = C.Config(**{"sim.human_num": 7, "robot.policy": "orca"})
    for interval, steps in ((1, 40), (2, 41)):
        envs = CollectVecEnv(425, 3, torch.device("cuda", 0), config=cfg)
        lines = collect_lines(envs, steps, interval, block=16)
        envs.close()
        envs = CollectVecEnv(425, 3, torch.device("cuda", 0), config=cfg)
        log = collect_log(envs, steps, interval)
        envs.close()
        assert log.is_cuda and tuple(log.shape) == ((steps + interval - 1) // interval, 3, 7, 4)
        host = log.cpu().numpy()
        for e in range(3):
            assert [ln for k in range(host.shape[0]) for ln in format_rows(host[k, e])] == lines[e]


# ---- the minibatch ----
def _host_batch(parts, picks, thetas):
    """seq_to_graph's vertices of the picked (env, item) sequences, rotated on the CPU by rotate_graph, padded as HipGstEvaluator._stack and
    the trainers pad: zeros up to the largest crowd, at least four."""
    from crowdnav_prediction_attngraph_amd import gst_train as T
    rot = (lambda v, th: v) if thetas is None else T.rotate_graph
    items = [parts[e][i] for e, i in picks]
    th = [None] * len(items) if thetas is None else thetas
    out = [T.HipGstEvaluator._stack([rot(it[k], t) for it, t in zip(items, th)], 3, 1) for k in (6, 8)] + [T.HipGstEvaluator._stack([it[4] for it in items], 2, 0)]
    n = out[0].shape[2]
    if n < 4:
        out = [torch.nn.functional.pad(t, (0, 0, 0, 4 - n)) for t in out]
    return out


@pytest.mark.parametrize("picks", [[(1, 3)], [(0, 0)], [(0, 1), (1, 3), (1, 8), (0, 5), (1, 0)], [(1, 3), (1, 0), (1, 8)]], ids=["B1_crowd1", "B1_crowd6", "B5_ragged", "B3_below4"])
@pytest.mark.parametrize("rotated", [True, False], ids=["rotated", "copied"])
def test_gather_equals_the_host_assembly(synthetic, picks, rotated):
    from crowdnav_prediction_attngraph_amd.gst_train import DeviceTrajectories
    log, _, hosts = synthetic
    parts = hosts[None][1]
    ds = DeviceTrajectories.from_log(torch.from_numpy(log).cuda())
    crowds = [parts[e][i][0].shape[0] for e, i in picks]
    assert len(picks) == 1 or (min(crowds) < 4 and len(set(crowds)) >= 3)     # ragged, one crowd below the kernels' four
    thetas = [float(t) for t in np.random.default_rng(3).uniform(0, 2 * np.pi, len(picks))] if rotated else None
    index = [i + (len(parts[0]) if e == 1 else 0) for e, i in picks]
    cs = None if thetas is None else torch.tensor(np.stack((np.cos(thetas), np.sin(thetas)), 1).astype(np.float32)).cuda()
    got = ds.gather(torch.tensor(index, dtype=torch.int32).cuda(), ds.num_peds(np.asarray(index)), cs)
    for g, h in zip(got, _host_batch(parts, picks, thetas)):
        assert tuple(g.shape) == tuple(h.shape) and g.shape[-2 if g.dim() == 4 else 1] == max(4, max(crowds))
        assert np.array_equal(U.bits(g.cpu().numpy()), U.bits(h.numpy()))


# ---- the epoch ----
@pytest.fixture(scope="module")
def gold_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("gstdata_gold")
    with open(str(d / "0.txt"), "w") as f:
        f.write(str(np.load(os.path.join(GOLDEN, "gst_train_h20.npz"))["file_lines"]) + "\n")
    return str(d)


def _device_split(gold_dir):
    from crowdnav_prediction_attngraph_amd.gst_train import DeviceTrajectories, TrajectoriesDataset
    return tuple(DeviceTrajectories.from_dataset(TrajectoriesDataset(gold_dir, mode=m), "cuda:0") for m in ("train", "val"))


def test_device_epoch_at_batch_size_one_is_the_per_item_loop(gold_dir, tmp_path):
    from crowdnav_prediction_attngraph_amd import gst_train as T
    from crowdnav_prediction_attngraph_amd.gst_train import TrajectoriesDataset
    assert len(TrajectoriesDataset(gold_dir)) == 111
    kw = dict(num_epochs=2, temp_epochs=4, save_epochs=2, random_seed=77, device="cuda:0", log=lambda s: None)
    m0, h0 = T.train(gold_dir, str(tmp_path / "files"), **kw)
    m1, h1 = T.train(out_dir=str(tmp_path / "device"), dataset=_device_split(gold_dir), **kw)
    assert h0 == h1
    for (k, a), (_, b) in zip(m0.state_dict().items(), m1.state_dict().items()):
        assert np.array_equal(U.bits(a.cpu().numpy()), U.bits(b.cpu().numpy())), k
    ck0, ck1 = (torch.load(str(tmp_path / d / "checkpoint" / "epoch_2.pt"), map_location="cpu", weights_only=False) for d in ("files", "device"))
    assert ck0["val_loss_epoch"] == ck1["val_loss_epoch"] and ck0["train_aoe_epoch"] == ck1["train_aoe_epoch"]
    for a, b in zip(ck0["optimizer_state_dict"]["state"].values(), ck1["optimizer_state_dict"]["state"].values()):
        assert torch.equal(a["exp_avg_sq"], b["exp_avg_sq"]) and float(a["step"]) == float(b["step"])


def test_device_epoch_at_batch_size_eight_is_explicit_trainer_calls(gold_dir, tmp_path):
    import json
    from crowdnav_prediction_attngraph_amd import gst_train as T
    from crowdnav_prediction_attngraph_amd.gst import GSTPredictor
    seed, B = 31, 8
    model, hist = T.train(out_dir=str(tmp_path / "run"), dataset=_device_split(gold_dir), batch_size=B, num_epochs=1, temp_epochs=4, random_seed=seed,
                          device="cuda:0", log=lambda s: None)
    assert json.load(open(str(tmp_path / "run" / "checkpoint" / "args.json")))["batch_size"] == B and np.isfinite(hist["train_loss_task"] + hist["val_loss_task"]).all()
    ds = T.TrajectoriesDataset(gold_dir, mode="train")
    torch.manual_seed(seed)
    np.random.seed(seed)
    ref = GSTPredictor().to("cuda:0")
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    tr = T.HipGstTrainer(ref, lr=1e-3, clip_grad=10.0, seed=seed, optimizer=opt)
    order, thetas = T.epoch_plan(len(ds), "random")
    stack = T.HipGstEvaluator._stack
    for lo in range(0, len(ds), B):
        items = [(ds[int(i)], float(t)) for i, t in zip(order[lo:lo + B], thetas[lo:lo + B])]
        tr.loss_and_grads(stack([T.rotate_graph(it[6], t) for it, t in items], 3, 1), stack([T.rotate_graph(it[8], t) for it, t in items], 3, 1),
                          stack([it[4] for it, _ in items], 2, 0), p_drop=0.1)
        tr.optimizer_step(grad_scale=1.0 / B)
    assert tr.step_no == (len(ds) + B - 1) // B and len(ds) % B != 0          # the last minibatch is short
    for (k, a), (_, b) in zip(model.state_dict().items(), ref.state_dict().items()):
        assert np.array_equal(U.bits(a.cpu().numpy()), U.bits(b.cpu().numpy())), k
