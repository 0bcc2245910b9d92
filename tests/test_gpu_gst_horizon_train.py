"""-m gpu: the GST predictor's training step, evaluation step and device-built dataset at prediction horizons P = pred_seq_len other than 5
(cn_gst_train_step_horizon, cn_gst_eval_step_horizon, cn_gst_data_*_horizon, cn_gst_gather_batch_horizon) and, at P = 5, the entry points
with a horizon against those without in bits.

Bars.  Training step: those of tests/test_gpu_gst_train.py (tests/gst_dropout_ref.bars: 2e-5 x max(1, |ref|) on the loss and the Gaussian
parameters, 1e-4 x a gradient tensor's largest entry + 1e-7), each taken as max(bar, 4 d), d = float32 against float64 of the same graph on the CPU
(printed) -- the reverse pass at P = 8 is twelve encoder passes deep.  Evaluation step: tests/test_gpu_gst_eval.py's 2e-5 on the loss and the
Gaussian parameters; its 1.5e-4 on the offset errors is 5 x sqrt(2) x 2e-5 for a five-step cumulative sum: here min(1.5e-4, P x sqrt(2) x 2e-5),
tighter below five steps and that file's bar above.  Dataset and gather: bits."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402
from tests import gst_data_util as D  # noqa: E402
from tests import gst_dropout_ref as R  # noqa: E402
from tests import gst_horizon_util as HU  # noqa: E402
from tests import gst_shape_util as U  # noqa: E402

BAR, BAR_OE = 2e-5, 1.5e-4
# three sequences of ragged crowd sizes, and one of the kernels' 64
TRAIN_CASES = [((1, 7, 20), 11), ((64,), 12)]


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_step(P, sizes, seed, p_drop):
    """cn_gst_train_step_horizon against the float64 graph of tests/gst_dropout_ref.py, which restates the counter rule of the header for the
    4 + P passes of model.pred_len = P (p_drop = 0: every mask is one, the graph is autograd on the host mirror)."""
    from crowdnav_prediction_attngraph_amd import gst_train as T
    cpu_model, lm, v_obs, v_pred = HU.ragged_crowds(sizes, seed, P)
    assert cpu_model.pred_len == P
    ref = R.masked_loss_and_grads(cpu_model, v_obs, v_pred, lm, seed, p_drop, torch.float64)
    d = R.errors(R.masked_loss_and_grads(cpu_model, v_obs, v_pred, lm, seed, p_drop, torch.float32), ref)
    bar = {k: max(v, 4 * d[k]) for k, v in R.bars(ref).items()}
    model = copy.deepcopy(cpu_model).cuda()
    tr = T.HipGstTrainer(model)
    out, gauss = tr.loss_and_grads(v_obs, v_pred, lm, p_drop=p_drop, seed=seed)
    assert tuple(gauss.shape) == (len(sizes), P, max(sizes), 5) and torch.isfinite(out).all() and torch.isfinite(gauss).all()
    res = (float(out[0]), float(out[1]), gauss.cpu(), {k: q.grad.detach().cpu() for k, q in model.named_parameters()})
    err = R.errors(res, ref)
    worst = max((err[k] / bar[k], k) for k in bar if k not in ("loss", "gauss"))
    print("train step P=%d crowds %s p=%.1f: loss err %.2e bar %.2e (d %.1e) | Gaussians err %.2e bar %.2e (d %.1e) | worst gradient %.3f bar (%s: err %.2e bar %.2e d %.1e)"
          % (P, sizes, p_drop, err["loss"], bar["loss"], d["loss"], err["gauss"], bar["gauss"], d["gauss"], worst[0], worst[1], err[worst[1]], bar[worst[1]], d[worst[1]]))
    assert res[1] == float(ref[1]) > 0, (res[1], float(ref[1]))
    for k in bar:
        assert np.isfinite(err[k]) and err[k] <= bar[k], (k, err[k], bar[k], d[k])


@pytest.mark.parametrize("sizes,seed", TRAIN_CASES, ids=["ragged_1_7_20", "crowd_64"])
@pytest.mark.parametrize("P", HU.HORIZONS)
def test_training_step_at_a_horizon_equals_autograd_on_the_fp64_host_graph(P, sizes, seed):
    _check_step(P, sizes, seed, 0.0)


def test_training_step_with_dropout_at_three_steps_equals_the_masked_fp64_graph():
    """The documented counter rule over 4 + P = 7 passes: observed slice t is pass t, decode step tt = 1, 2 is pass 4 + tt."""
    _check_step(3, (1, 7, 20), 13, 0.1)
    # the passes the masked graph visits for a three-step predictor: 0 .. 6 of every sequence, no more
    cpu_model, lm, v_obs, v_pred = HU.ragged_crowds((1, 7, 20), 13, 3)
    record = {}
    R.masked_loss_and_grads(cpu_model, v_obs, v_pred, lm, 13, 0.1, torch.float64, record=record)
    assert sorted(record) == [(b, call) for b in range(3) for call in range(4 + 3)]


def _raw_train_step(entry, P, vo, vp, lm, model, p_drop, seed):
    """One C call of `entry` on its own workspace and gradient buffers -> (loss_and_count, gauss, flat gradients)."""
    from crowdnav_prediction_attngraph_amd.gst_hip import gst_weights, predictor_params
    dev, L = vo.device, A.lib()
    B, Np = vo.shape[0], vo.shape[2]
    params = [p for _, p in predictor_params(model)]
    grads = [torch.full_like(p, float("nan")) for p in params]
    w, g = gst_weights(params, "test"), gst_weights(grads, "test")
    horizon = entry.endswith("_horizon")
    need = int(L.cn_gst_train_workspace_bytes_horizon(B, Np, P) if horizon else L.cn_gst_train_workspace_bytes(B, Np))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out, gauss = torch.empty(2, device=dev), torch.empty(B, P, Np, 5, device=dev)
    args = (B, Np) + ((P,) if horizon else ()) + (A.ptr(vo), A.ptr(vp), A.ptr(lm), C.byref(w), C.byref(g), float(p_drop), C.c_uint64(seed), C.c_void_p(ws.data_ptr()),
                                                  need, A.ptr(out), A.ptr(gauss), A.stream_ptr())
    A.call(entry, *args, device=dev)
    return out, gauss, torch.cat([x.reshape(-1) for x in grads])


def test_five_step_entry_points_with_a_horizon_are_those_without_in_bits():
    """Training step (ragged batch, dropout on), evaluation step (S = 0: validation, and S = 20), dataset build and gathered batch."""
    from crowdnav_prediction_attngraph_amd import gst_train as T
    from crowdnav_prediction_attngraph_amd.gst_hip import gst_weights, predictor_params
    L = A.lib()
    cpu_model, lm, v_obs, v_pred = HU.ragged_crowds((3, 20, 37), 21, 5)
    model = cpu_model.cuda()
    vo, vp, lmd = (t.cuda().contiguous() for t in (v_obs, v_pred, lm))
    a = _raw_train_step("cn_gst_train_step", 5, vo, vp, lmd, model, 0.1, 77)
    b = _raw_train_step("cn_gst_train_step_horizon", 5, vo, vp, lmd, model, 0.1, 77)
    assert L.cn_gst_train_workspace_bytes(3, 37) == L.cn_gst_train_workspace_bytes_horizon(3, 37, 5) > 0
    assert all(_bits(x, y) for x, y in zip(a, b)) and bool(torch.isfinite(a[2]).all()) and float(a[0][1]) > 0
    # evaluation
    B, Np = 3, 37
    w = gst_weights([p for _, p in predictor_params(model)], "test")
    for S in (0, 20):
        nz = torch.randn(B, S, 5, Np, 2, generator=torch.Generator().manual_seed(5)).cuda() if S else None
        R_ = max(S, 1)
        res = []
        for entry in ("cn_gst_eval_step", "cn_gst_eval_step_horizon"):
            horizon = entry.endswith("_horizon")
            need = int(L.cn_gst_eval_workspace_bytes_horizon(B, Np, S, 5) if horizon else L.cn_gst_eval_workspace_bytes(B, Np, S))
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            seq, ped, gauss = torch.empty(B, R_, 4, device="cuda"), torch.empty(B, R_, Np, 3, device="cuda"), torch.empty(B, R_, 5, Np, 5, device="cuda")
            args = (B, Np, S) + ((5,) if horizon else ()) + (A.ptr(vo), A.ptr(vp), A.ptr(lmd), C.byref(w), A.ptr(nz), C.c_void_p(ws.data_ptr()), need, A.ptr(seq),
                                                             A.ptr(ped), A.ptr(gauss), A.stream_ptr())
            A.call(entry, *args, device=torch.device("cuda"))
            res.append((seq, ped, gauss))
        assert all(_bits(x, y) for x, y in zip(*res)) and bool(torch.isfinite(res[0][0]).all()), S
    # the wrappers go through the entry points with a horizon: the same bits again
    ev = T.HipGstEvaluator(model)
    seq, ped, gauss = ev.evaluate_batch(v_obs, v_pred, lm, nz.cpu())
    assert _bits(seq, res[0][0]) and _bits(gauss, res[0][2])
    # dataset and gather: the calls without a horizon by hand against DeviceTrajectories (which uses the ones with)
    log = torch.from_numpy(D.synthetic_log()).cuda()
    ds = T.DeviceTrajectories.from_log(log)
    F_, E, H, _ = log.shape
    W = F_ - 9
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device="cuda")   # noqa: E731
    visible, frame_id, status = i32(F_, E), torch.empty(F_, E, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    frame_list, ped_count, first_frame = i32(E, F_), i32(E * W), torch.empty(E * W, device="cuda")
    A.call("cn_gst_data_frames", F_, E, H, A.ptr(log), A.ptr(visible), A.ptr(frame_id), A.ptr(status), A.stream_ptr())
    listed_before = (torch.cumsum(visible, 0).to(torch.int32) - visible).contiguous()
    A.call("cn_gst_data_count", F_, E, H, 0, A.ptr(log), A.ptr(visible), A.ptr(listed_before), A.ptr(frame_id), A.ptr(frame_list), A.ptr(ped_count), A.ptr(first_frame),
           A.ptr(status), A.stream_ptr())
    ped_offset = (torch.cumsum(ped_count, 0).to(torch.int32) - ped_count).contiguous()
    total = int(ped_count.sum())
    assert int(status) == 0 and total == ds.total_peds
    arrays = [torch.empty(total, 2, 5, device="cuda") for _ in range(4)] + [torch.empty(total, 10, device="cuda") for _ in range(2)]
    A.call("cn_gst_data_fill", F_, E, H, 0, A.ptr(log), A.ptr(visible), A.ptr(listed_before), A.ptr(frame_id), A.ptr(frame_list), A.ptr(ped_count), A.ptr(ped_offset),
           total, *([A.ptr(t) for t in arrays] + [A.stream_ptr()]))
    for k, t in zip(ds.FIELDS, arrays):
        assert _bits(getattr(ds, k), t), k
    index = torch.tensor([0, 5, len(ds) - 1], dtype=torch.int32).cuda()
    n = ds.num_peds(index.cpu().numpy())
    cs = torch.tensor([[0.6, 0.8], [1.0, 0.0], [-0.8, 0.6]]).cuda()
    got = ds.gather(index, n, cs)
    old = [torch.empty(3, 5, n, 2, device="cuda"), torch.empty(3, 5, n, 2, device="cuda"), torch.empty(3, n, 10, device="cuda")]
    A.call("cn_gst_gather_batch", 3, n, ds.num_seq, ds.total_peds, A.ptr(index), A.ptr(cs), A.ptr(ds._seq_start), A.ptr(ds._seq_count), A.ptr(ds.obs_traj_rel),
           A.ptr(ds.pred_traj_rel), A.ptr(ds.loss_mask_rel), A.ptr(old[0]), A.ptr(old[1]), A.ptr(old[2]), A.stream_ptr())
    assert all(_bits(x, y) for x, y in zip(got, old))


def test_six_optimiser_steps_at_three_predicted_steps_match_the_torch_backend(tmp_path):
    """gst_train.train(backend='hip', pred_seq_len=3) against backend='torch': one epoch of six sequences = six optimiser steps, then the
    validation pass, rotation off and p_drop = 0 (the two backends draw their dropout masks from different streams; without dropout both are
    deterministic, the loaders shuffle alike under the run's seed, and the histories follow each other).  Bars of the existing six-step test
    (tests/test_gpu_gst_train.py): 5e-5 on the losses, 1e-4 on every weight; the offset errors at the evaluation bar of three steps.  The KEY
    bias (entries 64 .. 127 of in_proj_bias) has a gradient of exactly zero in exact arithmetic -- the softmax is invariant to a shift of all
    scores of a row -- so Adam normalises rounding noise there and the entries carry no information: they are left out of the weight comparison,
    and, since they do not enter the function either, the two trained predictors must give the same forward within 1e-4.  The run records
    pred_seq_len = 3 and its checkpoint loads as a three-step predictor into the wrapper's handle."""
    from crowdnav_prediction_attngraph_amd import gst_train as T
    from crowdnav_prediction_attngraph_amd.gst import GSTPredictor, PretextProcessor
    dirs = D.write_files(HU.walking_log(), tmp_path / "data")
    assert (len(T.TrajectoriesDataset(dirs[0], pred_seq_len=3, mode="train")), len(T.TrajectoriesDataset(dirs[0], pred_seq_len=3, mode="val"))) == (6, 1)
    runs = {}
    for backend in ("hip", "torch"):
        runs[backend] = T.train(dirs[0], str(tmp_path / backend), num_epochs=1, temp_epochs=4, save_epochs=1, device="cuda", log=lambda s: None, backend=backend,
                                rotation_pattern=None, pred_seq_len=3, p_drop=0.0)
    (m_hip, h_hip), (m_ref, h_ref) = runs["hip"], runs["torch"]
    bar_oe = min(BAR_OE, 3 * 2 ** 0.5 * BAR)
    for k in sorted(h_ref):
        if k == "epoch":
            assert h_hip[k] == h_ref[k] == 1
            continue
        bar = 5e-5 if "loss" in k else bar_oe
        print("six steps P=3 history %-16s hip %s torch %s (bar %.1e)" % (k, h_hip[k], h_ref[k], bar))
        assert len(h_hip[k]) == len(h_ref[k]) == 1 and np.isfinite(h_ref[k]).all()
        assert abs(h_hip[k][0] - h_ref[k][0]) <= bar, (k, h_hip[k], h_ref[k])
    assert m_hip.pred_len == m_ref.pred_len == 3
    for (k, a), (_, b) in zip(m_hip.state_dict().items(), m_ref.state_dict().items()):
        diff = (a - b).abs()
        if k.endswith("in_proj_bias"):
            print("six steps P=3: key bias differs by %.3g (not compared), the rest of in_proj_bias by %.3g" % (float(diff[64:128].max()), float(torch.cat((diff[:64], diff[128:])).max())))
            diff = torch.cat((diff[:64], diff[128:]))
        assert float(diff.max()) <= 1e-4, (k, float(diff.max()))
    traj, mask = (torch.from_numpy(x).cuda() for x in U.inputs(6, 9, 9))
    with torch.no_grad():
        (oa, ma), (ob, mb) = m_hip(traj, mask), m_ref(traj, mask)
    valid = ma[..., 0] > 0
    fwd = float((oa - ob)[valid].abs().max())
    print("six steps P=3: forward of the two trained predictors differs by %.3g (bar 1e-4)" % fwd)
    assert torch.equal(ma, mb) and int(valid.sum()) > 0 and fwd <= 1e-4
    m3 = GSTPredictor.from_checkpoint(str(tmp_path / "hip" / "checkpoint" / "epoch_1.pt"), "cuda")
    assert m3.pred_len == 3
    w = PretextProcessor(m3, 4, 5, 3, 0.3, 0.3, -20.0, torch.device("cuda"))
    assert w.hip is not None and w.hip.P == 3


# ---- evaluation ----
def _torch_rows(T, model, lm, v_obs, v_pred, P, noise=None):
    """The op graph per sequence (and per sample) on the device -> seq [B,R,4], ped [B,R,N,3], gauss [B,R,P,N,5] like evaluate_batch
    (tests/test_gpu_gst_eval.py's helper for a horizon; gst_train.test_sequence is this loop's body)."""
    B, N = lm.shape[:2]
    R_ = 1 if noise is None else noise.shape[1]
    seq, ped, gauss = torch.zeros(B, R_, 4), torch.zeros(B, R_, N, 3), torch.zeros(B, R_, P, N, 5)
    with torch.no_grad():
        for b in range(B):
            l1 = lm[b:b + 1].cuda()
            am = (l1[0].t().unsqueeze(2) * l1[0].t().unsqueeze(1))[:5].unsqueeze(0)
            for s in range(R_):
                nz = None if noise is None else noise[b, s:s + 1].cuda()
                gp, xs, info = T.forward_train(model, v_obs[b:b + 1].cuda(), am, l1, 0.0, nz)
                vp = v_pred[b:b + 1].cuda()
                pl, elm = T.negative_log_likelihood_full_partial(gp, vp, info["loss_mask_rel_full_partial"], l1[:, :, 5:])
                lpp = info["loss_mask_per_pedestrian"]
                aoe, foe = T.average_offset_error(xs, vp, lpp), T.final_offset_error(xs, vp, lpp)
                seq[b, s] = torch.stack((pl.sum(), elm.sum(), aoe.sum(), foe.sum())).cpu()
                ped[b, s] = torch.stack((aoe, foe, lpp[0]), -1).cpu()
                gauss[b, s] = torch.cat(gp, -1)[0].cpu()
    return seq, ped, gauss


def _close(a, b, bar, what, tensor_scale=False):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert torch.isfinite(a).all(), what
    scale = b.abs().max().clamp(min=1.0) if tensor_scale else b.abs().clamp(min=1.0)
    err = float(((a - b).abs() / scale).max())
    print("%-70s err = %.3e  bar = %.1e" % (what, err, bar))
    assert err <= bar, (what, err, bar)


@pytest.mark.parametrize("S", [0, 20], ids=["validation", "S20"])
@pytest.mark.parametrize("P", HU.HORIZONS)
def test_evaluation_step_at_a_horizon_equals_the_host_graph(P, S):
    """B = 3 ragged crowds (3 -> padded to 4 inside the batch, 20, 64): validation (the mean fed back) and S = 20 decodes on the caller's draws."""
    from crowdnav_prediction_attngraph_amd import gst_train as T
    sizes = (3, 20, 64)
    cpu_model, lm, v_obs, v_pred = HU.ragged_crowds(sizes, 30 + P, P)
    model = cpu_model.cuda().eval()
    B, N = len(sizes), max(sizes)
    noise = torch.randn(B, S, P, N, 2, generator=torch.Generator().manual_seed(P)) if S else None
    ev = T.HipGstEvaluator(model)
    seq, ped, gauss = ev.evaluate_batch(v_obs, v_pred, lm, noise)
    R_ = max(S, 1)
    assert tuple(seq.shape) == (B, R_, 4) and tuple(ped.shape) == (B, R_, N, 3) and tuple(gauss.shape) == (B, R_, P, N, 5)
    rseq, rped, rgauss = _torch_rows(T, model, lm, v_obs, v_pred, P, noise)
    what, bar_oe = "evaluation P=%d S=%d" % (P, S), min(BAR_OE, P * 2 ** 0.5 * BAR)
    assert torch.equal(seq[..., 1].cpu(), rseq[..., 1]) and float(rseq[..., 1].min()) > 0, what + ": valid (step, pedestrian) pairs"
    assert torch.equal(ped[..., 2].cpu(), rped[..., 2]) and float(rped[..., 2].sum()) > 0, what + ": loss_mask_per_pedestrian"
    _close(seq[..., 0] / seq[..., 1], rseq[..., 0] / rseq[..., 1], BAR, what + ": loss")
    _close(gauss, rgauss, BAR, what + ": Gaussian parameters", tensor_scale=True)
    _close(ped[..., :2], rped[..., :2], bar_oe, what + ": aoe / foe per pedestrian")
    absent = rped[..., 2] == 0
    assert float(ped[..., :2].cpu()[absent].abs().max()) == 0.0, what + ": aoe / foe of a pedestrian not present throughout"
    _close(seq[..., 2:], ped[..., :2].sum(2), BAR, what + ": sums of aoe / foe")
    # one sequence through gst_train.test_sequence, the body of the host pass
    item_lm = lm[1:2, :sizes[1]]
    item = [None] * 12
    item[4], item[6], item[8] = item_lm, v_obs[1:2, :, :sizes[1]], v_pred[1:2, :, :sizes[1]]
    item[10] = (item_lm[0].t().unsqueeze(2) * item_lm[0].t().unsqueeze(1))[:5].unsqueeze(0)
    loss, aoe, foe, m = T.test_sequence(model, item, None if noise is None else noise[1, :, :, :sizes[1]], "cuda")
    _close(seq[1, :, 0] / seq[1, :, 1], loss, BAR, what + ": test_sequence loss")
    _close(seq[1, :, 2], aoe, bar_oe, what + ": test_sequence aoe sum")
    _close(seq[1, :, 3], foe, bar_oe, what + ": test_sequence foe sum")
    assert float(m) == float(ped[1, 0, :, 2].sum())


def test_the_largest_evaluation_case_is_inside_the_lds_and_the_next_is_refused():
    """N = 64 at P = 8: 133 KB of the CU's 160 KiB by the kernel's own formula (run above); N = 65 and P = 9 are refused before any launch."""
    from crowdnav_prediction_attngraph_amd import gst_train as T
    L = A.lib()
    lds = lambda N, P: 4 * (7 * N * 64 + ((N * 2 + 3) & ~3) + 128 + N * (5 + P) + P * N * 2 + P * N * 5 + 8)   # noqa: E731  csrc/gst_eval.hip
    assert 130 * 1024 < lds(64, 8) <= 160 * 1024
    assert L.cn_gst_eval_workspace_bytes_horizon(2, 64, 20, 8) > 0
    assert L.cn_gst_eval_workspace_bytes_horizon(2, 64, 20, 9) == L.cn_gst_eval_workspace_bytes_horizon(2, 65, 20, 8) == 0
    assert L.cn_gst_train_workspace_bytes_horizon(2, 64, 9) == L.cn_gst_train_workspace_bytes_horizon(2, 64, 0) == 0
    model, lm, v_obs, v_pred = HU.ragged_case(1, 8, 3, 8)
    ev = T.HipGstEvaluator(model.cuda())
    with pytest.raises(A.CnError, match=r"in \[1, 8\]"):
        ev.evaluate_batch(v_obs, torch.zeros(1, 9, 8, 2), torch.ones(1, 8, 14))
    with pytest.raises(A.CnError, match=r"loss_mask_rel \[B,N,5\+P\]"):
        ev.evaluate_batch(v_obs, v_pred, lm[:, :, :10])
    seq, _, _ = ev.evaluate_batch(v_obs, v_pred, lm)          # the evaluator is as usable as before
    assert bool(torch.isfinite(seq).all())


# ---- dataset ----
def _simulator_log(human_num, samples):
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


@pytest.fixture(scope="module")
def logs(tmp_path_factory):
    """The hand-made log and a short simulator log with their files: built once, shared, left unchanged."""
    out = {}
    for name, log in (("hand_made", HU.hand_made_log()), ("simulator", _simulator_log(5, 60))):
        out[name] = (log, D.write_files(log, tmp_path_factory.mktemp("gsth_" + name)))
    return out


@pytest.mark.parametrize("name", ["hand_made", "simulator"])
@pytest.mark.parametrize("P", [3, 8])
def test_device_dataset_at_a_horizon_is_the_host_dataset_bit_for_bit(logs, name, P):
    from crowdnav_prediction_attngraph_amd import gst_train as T
    log, dirs = logs[name]
    dev_log = torch.from_numpy(log).cuda()
    hosts = {}
    for mode in (None, "train", "val"):
        host, parts = HU.host_dataset(dirs, mode, P)
        assert host is not None, mode
        ds = T.DeviceTrajectories.from_log(dev_log, mode, pred_seq_len=P)
        assert (ds.obs_seq_len, ds.pred_seq_len, ds.seq_len) == (5, P, 5 + P)
        assert tuple(ds.pred_traj.shape[1:]) == (2, P) and tuple(ds.loss_mask.shape[1:]) == (5 + P,)
        D.assert_same_dataset(ds, host)
        hosts[mode] = (host, parts, ds)
    host, parts, ds = hosts[None]
    crowds = np.diff(host["seq_start_end"], axis=1).ravel()
    assert len(set(crowds.tolist())) >= 2                      # ragged
    if name == "hand_made":
        assert parts[2] is None and min(crowds) < 4            # the env of seven frames has no window; a crowd below the kernels' four
        five = HU.host_dataset(dirs, None, 5)[0]
        assert len(five["seq_env"]) != len(host["seq_env"])     # another horizon cuts other windows
    # the items are the host class's 12 entries
    flat = [it for p in parts if p is not None for it in (p[i] for i in range(len(p)))]
    for i in (0, len(ds) // 2, len(ds) - 1):
        for a, b in zip(ds[i], flat[i]):
            assert a.is_cuda and np.array_equal(D.bits(a.cpu().numpy()), D.bits(b.numpy()))
    # the gathered batch against the host assembly: rotated and copied, ragged, one crowd below four where the log has one
    order = np.argsort(crowds, kind="stable")
    picks = sorted({int(order[0]), int(order[len(order) // 2]), int(order[-1]), 0})
    for thetas in (None, [float(t) for t in np.random.default_rng(3).uniform(0, 2 * np.pi, len(picks))]):
        rot = (lambda v, th: v) if thetas is None else T.rotate_graph
        th = [None] * len(picks) if thetas is None else thetas
        want = [T.HipGstEvaluator._stack([rot(flat[i][k], t) for i, t in zip(picks, th)], 3, 1) for k in (6, 8)] + [T.HipGstEvaluator._stack([flat[i][4] for i in picks], 2, 0)]
        n = want[0].shape[2]
        if n < 4:
            want = [torch.nn.functional.pad(t, (0, 0, 0, 4 - n)) for t in want]
        cs = None if thetas is None else torch.tensor(np.stack((np.cos(thetas), np.sin(thetas)), 1).astype(np.float32)).cuda()
        got = ds.gather(torch.tensor(picks, dtype=torch.int32).cuda(), ds.num_peds(np.asarray(picks)), cs)
        assert tuple(got[1].shape[:2]) == (len(picks), P) and got[2].shape[2] == 5 + P
        for g, h in zip(got, want):
            assert tuple(g.shape) == tuple(h.shape) and np.array_equal(D.bits(g.cpu().numpy()), D.bits(h.numpy()))


def test_a_log_shorter_than_the_window_is_refused_by_the_c_call_and_launches_nothing():
    """F = 12 samples hold windows of 5 + 3 but none of 5 + 8: the C calls refuse (nothing is written), the Python class says what is missing."""
    from crowdnav_prediction_attngraph_amd import gst_train as T
    log = torch.from_numpy(HU.hand_made_log()[:12].copy()).cuda()
    F_, E, H, _ = log.shape
    sentinel = torch.full((F_, E), -7, dtype=torch.int32, device="cuda")
    fid, status = torch.full((F_, E), -7.0, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(A.CnError, match=r"at least 5 \+ P = 13"):
        A.call("cn_gst_data_frames_horizon", F_, E, H, 8, A.ptr(log), A.ptr(sentinel), A.ptr(fid), A.ptr(status), A.stream_ptr())
    with pytest.raises(A.CnError, match=r"at least 5 \+ P = 13"):
        A.call("cn_gst_data_count_horizon", F_, E, H, 0, 8, A.ptr(log), A.ptr(sentinel), A.ptr(sentinel), A.ptr(fid), A.ptr(sentinel), A.ptr(sentinel), A.ptr(fid),
               A.ptr(status), A.stream_ptr())
    torch.cuda.synchronize()
    assert bool((sentinel == -7).all()) and bool((fid == -7.0).all()) and int(status) == 0
    with pytest.raises(RuntimeError, match="no sequence of 13 frames"):
        T.DeviceTrajectories.from_log(log, pred_seq_len=8)
    assert len(T.DeviceTrajectories.from_log(log, pred_seq_len=3)) > 0


# ---- the reference's own numbers ----
@pytest.mark.parametrize("P", HU.GOLDEN_HORIZONS)
def test_device_path_reproduces_the_reference_at_a_horizon(P):
    """tests/golden/gst_horizon_p<P>_h8.npz (the reference's st_model with pred_seq_len = P): cn_gst_predict within 1e-4, cn_gst_train_step_horizon
    within 2e-5 on the loss and the Gaussian parameters and 2e-5 x max(1, largest entry) on every gradient, cn_gst_eval_step_horizon within 2e-5
    on the loss -- the bars the P = 5 goldens are held at (tests/test_gst_host.py, tests/test_gpu_gst_train.py, tests/test_gpu_gst_eval.py)."""
    from crowdnav_prediction_attngraph_amd import gst_train as T
    from crowdnav_prediction_attngraph_amd.hip import HipGST
    z, m = HU.golden(P)
    m = m.cuda()
    g = HipGST(8, 4, pred_steps=P)
    g.set_weights(m.state_dict())
    out, om = g.predict(torch.from_numpy(z["in_traj"]).cuda(), torch.from_numpy(z["in_mask"]).cuda())
    np.testing.assert_array_equal(om.cpu().numpy(), z["out_mask"])
    valid = z["out_mask"][..., 0] > 0
    err = float(np.abs(out.cpu().numpy()[valid] - z["out_traj"][valid]).max())
    assert err <= 1e-4 and np.all(out.cpu().numpy()[~valid][..., :2] == -999.0)
    lm, v_obs, v_pred = (torch.from_numpy(z[k]) for k in ("loss_mask_rel", "v_obs", "v_pred"))
    seq, _, gauss_e = T.HipGstEvaluator(m).evaluate_batch(v_obs, v_pred, lm)
    e_loss = abs(float(seq[:, 0, 0].sum() / seq[:, 0, 1].sum()) - float(z["loss"]))
    tr = T.HipGstTrainer(m)
    o, gauss = tr.loss_and_grads(v_obs, v_pred, lm, p_drop=0.0)
    t_loss, t_gauss = abs(float(o[0]) - float(z["loss"])), float(np.abs(gauss.cpu().numpy() - z["gauss"]).max())
    worst = max((float(np.abs(p.grad.cpu().numpy() - z["grad_" + k]).max()) / max(1.0, float(np.abs(z["grad_" + k]).max())), k) for k, p in m.named_parameters())
    print("golden P=%d: predict %.3g (bar 1e-4) | train loss %.3g Gaussians %.3g worst gradient %.3g (%s) | eval loss %.3g (bars 2e-5)"
          % (P, err, t_loss, t_gauss, worst[0], worst[1], e_loss))
    assert float(o[1]) == float(z["count"]) == float(seq[:, 0, 1].sum())
    assert t_loss <= BAR and t_gauss <= BAR and worst[0] <= BAR and e_loss <= BAR
    assert float(np.abs(gauss_e[:, 0].cpu().numpy() - z["gauss"]).max()) <= BAR
