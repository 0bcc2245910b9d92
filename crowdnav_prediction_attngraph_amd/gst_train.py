"""Training of the GST trajectory predictor on the data-collection env's files -- the counterpart of the reference's
gst_updated/src/gumbel_social_transformer/st_model.py (the loss, :62-112), gst_updated/scripts/experiments/train.py (the loop) and eval.py
(`inference`: the per-epoch validation pass and the sampled test protocol), for the shipped hyper-parameters (embedding 64,
8 heads, 1 layer, spatial_num_heads_edges = 0, no ghost, faster_lstm, obs 5 / pred 5, recursive decoding).  Here: the loss and the offset
errors, the three epoch functions, evaluate / test, train / eval_run (the run directory format) and the CLI.  Its neighbours hold the rest:
  * gst.py       the predictor's one op graph (GSTPredictor.recursion: inference, training with the reference's four dropout sites, the sampled
                 test decode); forward_train below is its adapter from the dataset's layout;
  * gst_data.py  TrajectoriesDataset over the text files, for the per-item loop (train(data_dir, ...)), and DeviceTrajectories -- the sequences
                 cut out of collect_log's observations on the device (csrc/gst_data.hip), minibatches assembled and rotated there
                 (cn_gst_gather_batch), one read-back per epoch (train(dataset=..., batch_size=...));
  * gst_hip.py   the boundary calls: HipGstTrainer (cn_gst_train_step, csrc/gst_train.hip: forward + loss + hand-derived reverse pass, + the
                 flat_adam.FlatAdam bucket) and HipGstEvaluator (cn_gst_eval_step, csrc/gst_eval.hip).

Two execution paths of the training step (train.py:121-146: forward, negative log-likelihood, backward, clip, Adam) and of evaluation:
  * on a GPU (backend 'hip', the default there): the kernels through the C ABI -- one boundary call per optimiser step plus the fused clip + Adam
    step; batches of sequences per evaluation call and one read-back per pass (_eval_pass);
  * the op graph (backend 'torch'; under autograd when training): what CPU tensors use (unit tests, pinned to the reference's numbers) and the
    independent cross-check of the kernels (tests/test_gpu_gst_train.py and tests/test_gpu_gst_eval.py hold the two against each other).
The learning-rate schedule and the checkpoint format are host code either way, and the producer of the data is the batched simulator
(collect.py: thousands of simulated crowds per GPU).

Scope note: the reference trains on `<dataset>_dset_<split>_batch_trajectories.pt` files produced by scripts/data/create_*datasets*.py,
which are NOT part of the reference checkout (only the shell wrappers that call them are).  This module therefore feeds the loop with
TrajectoriesDataset items directly -- one sequence (all pedestrians of a 10-frame window) per optimiser step, which is what a
BatchTrajectoriesDataset item of one sequence is.
"""
import argparse
import json
import os
import pickle
import time

import numpy as np
import torch
from torch.utils.data import DataLoader

from .gst import GSTPredictor, find_checkpoint, load_checkpoint
from .gst_data import DeviceTrajectories, TrajectoriesDataset, read_file, rotate_graph, seq_to_graph  # noqa: F401
from .gst_hip import HipGstEvaluator, HipGstTrainer


def forward_train(model, v_obs, attn_mask_obs, loss_mask_rel, p_drop=0.1, noise=None):
    """GSTPredictor.recursion (st_model.py:271-455) on the dataset's layout.
    v_obs [1,T,N,2], attn_mask_obs [1,T,N,N] (neighbour, target), loss_mask_rel [1,N,T+P] ->
    (mu [1,P,N,2], sx, sy, corr [1,P,N,1]), x_sample_pred [1,P,N,2], info{'loss_mask_rel_full_partial', 'loss_mask_per_pedestrian'}.
    noise None: sampling = False, the mean is fed back.  noise [1,P,N,2] (standard-normal draws): sampling = True on the caller's draws."""
    gp, samples = model.recursion(v_obs, attn_mask_obs.permute(0, 1, 3, 2), loss_mask_rel, p_drop, noise)
    lm_pp = (loss_mask_rel.sum(2) == loss_mask_rel.shape[2]).float()
    return gp, samples, {"loss_mask_rel_full_partial": loss_mask_rel[:, :, v_obs.shape[1] - 1], "loss_mask_per_pedestrian": lm_pp}


def negative_log_likelihood_full_partial(gaussian_params, x_target, loss_mask_ped, loss_mask_pred_seq):
    """st_model.py:62-112 -> (prob_loss [P,N] already masked, eventual_loss_mask [P,N])."""
    mu, sx, sy, corr = gaussian_params
    m_t = loss_mask_pred_seq.permute(0, 2, 1).unsqueeze(-1)
    m_p = loss_mask_ped.unsqueeze(1).unsqueeze(-1)
    mu = mu * m_t * m_p
    corr = corr * m_t * m_p
    x_target = x_target * m_t * m_p
    sx = (sx * m_t + (1. - m_t)) * m_p + (1. - m_p)
    sy = (sy * m_t + (1. - m_t)) * m_p + (1. - m_p)
    sigma = torch.cat((sx, sy), dim=3)
    xn = (x_target - mu) / sigma
    nx, ny = xn[..., 0:1], xn[..., 1:2]
    t1 = torch.log(1. - corr ** 2.) / 2. + torch.log(sx) + torch.log(sy)
    t2 = (nx ** 2. - 2. * corr * nx * ny + ny ** 2.) / (2. * (1. - corr ** 2.))
    prob_loss = (t1 + t2).squeeze(3).squeeze(0)
    elm = m_t[0, :, :, 0] * loss_mask_ped[0]
    return prob_loss * elm, elm


def average_offset_error(x_pred, x_target, loss_mask=None):
    """mgnn/utils.py:8-17."""
    err = torch.sqrt(((torch.cumsum(x_pred, 1) - torch.cumsum(x_target, 1)) ** 2.).sum(3))[0]
    aoe = err.mean(0)
    return aoe * loss_mask[0] if loss_mask is not None else aoe


def final_offset_error(x_pred, x_target, loss_mask=None):
    """mgnn/utils.py:19-28."""
    err = torch.sqrt(((torch.cumsum(x_pred, 1) - torch.cumsum(x_target, 1)) ** 2.).sum(3))[0]
    foe = err[-1]
    return foe * loss_mask[0] if loss_mask is not None else foe


def sequence_loss(model, item, device, p_drop=0.1, noise=None):
    """One step's loss exactly as train.py:113-137 computes it (non-deterministic branch: NLL / number of valid (step, pedestrian)).
    noise: see forward_train (the test protocol's sampled decode)."""
    obs_traj, pred_gt, obs_rel, pred_rel_gt, lm_rel, lm, v_obs, A_obs, v_pred_gt, A_pred_gt, am_obs, am_pred = item
    v_obs, v_pred_gt, am_obs, lm_rel = v_obs.to(device), v_pred_gt.to(device), am_obs.to(device), lm_rel.to(device)
    gp, xs, info = forward_train(model, v_obs, am_obs, lm_rel, p_drop, noise)
    prob_loss, elm = negative_log_likelihood_full_partial(gp, v_pred_gt, info["loss_mask_rel_full_partial"], lm_rel[:, :, -model.pred_len:])
    return prob_loss.sum() / elm.sum(), gp, xs, info, v_pred_gt


def temperature(epoch, total_epochs, base_temp, temp_min=0.03):
    """temperature_scheduler.py (kept for the checkpoint / log; without edge heads the Gumbel temperature is never read)."""
    return max((1 - epoch / total_epochs) * (base_temp - temp_min) + temp_min, temp_min)


def _draw_theta(rotation_pattern):
    """train.py:115-117: the rotation angle of one training item, drawn from torch's global generator."""
    return (torch.randint(0, 4, ()).float() / 2. * np.pi).item() if rotation_pattern == "right_angle" else (torch.rand(()) * 2. * np.pi).item()


def epoch_plan(n, rotation_pattern):
    """The order and the rotation angles of one training epoch over n sequences, drawn up front by the calls the per-item loop makes, in its
    sequence: iterating DataLoader(dataset, batch_size=1, shuffle=True) and drawing theta after every item.  -> (order [n] int64,
    thetas [n] float64 or None); torch's global generator is left where that loop leaves it."""
    order, thetas = [], []
    for idx in DataLoader(range(int(n)), batch_size=1, shuffle=True):
        order.append(int(idx))
        if rotation_pattern is not None:
            thetas.append(_draw_theta(rotation_pattern))
    return np.asarray(order, dtype=np.int64), (np.asarray(thetas, dtype=np.float64) if rotation_pattern is not None else None)


def _offset_errors_batched(x_pred, x_target, loss_mask):
    """average_offset_error / final_offset_error (mgnn/utils.py:8-28) of every sequence of a batch: [B,P,N,2], [B,P,N,2], [B,N] -> [B,N] each."""
    err = torch.sqrt(((torch.cumsum(x_pred, 1) - torch.cumsum(x_target, 1)) ** 2.).sum(3))
    return err.mean(1) * loss_mask, err[:, -1] * loss_mask


def _step_sample_and_mask(gauss, lm_rel, obs_len):
    """forward_train's x_sample_pred [B,P,N,2] and loss_mask_per_pedestrian [B,N] from cn_gst_train_step's gauss [B,P,N,5] and loss_mask_rel [B,N,T+P]."""
    xs = gauss[..., :2] * lm_rel[:, :, obs_len - 1].unsqueeze(1).unsqueeze(-1)
    return xs, (lm_rel.sum(2) == lm_rel.shape[2]).float()


def _train_epoch_device(hip_tr, ds, order, thetas, batch_size, optimizer, obs_len, p_drop=0.1):
    """One training epoch with the data on the device: per step a gather, the training step, the fused clip + Adam step; the step's loss and
    its aoe / foe terms go into per-epoch device buffers and come back in ONE read-back.  -> (losses [steps] float64, [aoe], [foe], [m]: float32
    arrays of the per-pedestrian terms in step order)."""
    dev, n, B = ds.device, len(order), int(batch_size)
    index = torch.as_tensor(order.astype(np.int32)).to(dev)
    cos_sin = None if thetas is None else torch.as_tensor(np.stack((np.cos(thetas), np.sin(thetas)), 1).astype(np.float32)).to(dev)
    chunks = [(lo, min(lo + B, n)) for lo in range(0, n, B)]
    widths = [int(ds.counts[order[lo]]) if B == 1 else (hi - lo) * ds.num_peds(order[lo:hi]) for lo, hi in chunks]
    off = np.concatenate(([0], np.cumsum(widths))).astype(np.int64)
    loss_buf, terms = torch.empty(len(chunks), device=dev), torch.empty(3, int(off[-1]), device=dev)
    for k, (lo, hi) in enumerate(chunks):
        vo, vp, lm_rel = ds.gather(index[lo:hi], ds.num_peds(order[lo:hi]), None if cos_sin is None else cos_sin[lo:hi])
        hip_tr.lr = optimizer.param_groups[0]["lr"]                           # the StepLR schedule drives the fused step too
        out, gauss = hip_tr.loss_and_grads(vo, vp, lm_rel, p_drop=p_drop)
        hip_tr.optimizer_step(grad_scale=1.0 / B)
        loss_buf[k].copy_(out[0])
        seg = terms[:, off[k]:off[k + 1]]
        if B == 1:                                                            # the per-item loop's own expressions on its own shapes
            c = widths[k]
            gauss, lm_rel, vp = gauss[:, :, :c], lm_rel[:, :c], vp[:, :, :c].contiguous()
        xs, lm = _step_sample_and_mask(gauss, lm_rel, obs_len)
        aoe, foe = (average_offset_error(xs, vp, lm), final_offset_error(xs, vp, lm)) if B == 1 else _offset_errors_batched(xs, vp, lm)
        seg[0].copy_(aoe.reshape(-1)); seg[1].copy_(foe.reshape(-1)); seg[2].copy_(lm.reshape(-1))
    host = torch.cat((loss_buf, terms.reshape(-1))).cpu().numpy()              # the epoch's one read-back
    t = host[len(chunks):].reshape(3, -1)
    return host[:len(chunks)].astype(np.float64), [t[0]], [t[1]], [t[2]]


def _train_items(loader, rotation_pattern):
    """The per-item epochs' items (train.py:115-119): those of more than 128 pedestrians skipped, every kept one rotated by an angle drawn after it."""
    for item in loader:
        if item[6].shape[2] > 128:
            continue
        if rotation_pattern is not None:
            theta = _draw_theta(rotation_pattern)
            item = list(item)
            item[6], item[8] = rotate_graph(item[6], theta), rotate_graph(item[8], theta)
        yield item


def _item_terms(loss, xs, lm, v_pred_gt):
    """One per-item step's entries of (losses, aoes, foes, ms), read back."""
    return loss.item(), average_offset_error(xs, v_pred_gt, lm).cpu().numpy(), final_offset_error(xs, v_pred_gt, lm).cpu().numpy(), lm[0].cpu().numpy()


def _train_epoch_items_hip(hip_tr, loader, rotation_pattern, optimizer, device, obs_len, p_drop=0.1):
    """One epoch of one loader item per optimiser step through the kernels: forward, loss, backward (dropout p_drop: 0.1 like model.train()) as one boundary
    call, then the fused clip + Adam step.  -> (losses, aoes, foes, ms), one entry per step."""
    rows = []
    for item in _train_items(loader, rotation_pattern):
        lm_rel = item[4].to(device)
        hip_tr.lr = optimizer.param_groups[0]["lr"]                           # the StepLR schedule drives the fused step too
        out, gauss = hip_tr.loss_and_grads(item[6], item[8], lm_rel, p_drop=p_drop)
        hip_tr.optimizer_step()
        rows.append(_item_terms(out[0], *_step_sample_and_mask(gauss, lm_rel, obs_len), item[8].to(device)))
    return tuple(zip(*rows))


def _train_epoch_items_torch(model, loader, rotation_pattern, optimizer, clip_grad, device, p_drop=0.1):
    """The same epoch on the op graph under autograd (train.py:121-146)."""
    rows = []
    for item in _train_items(loader, rotation_pattern):
        loss, gp, xs, info, v_pred_gt = sequence_loss(model, item, device, p_drop)
        loss.backward()
        rows.append(_item_terms(loss.detach(), xs.detach(), info["loss_mask_per_pedestrian"], v_pred_gt))
        if clip_grad is not None:
            torch.nn.utils.clip_grad_norm_(model.parameters(), clip_grad)
        optimizer.step()
        optimizer.zero_grad()
    return tuple(zip(*rows))


def _eval_backend(model, backend):
    if backend is None:
        return "torch"
    if backend not in ("torch", "hip"):
        raise ValueError("backend must be None, 'torch' or 'hip' (got %r)" % (backend,))
    return backend


def test_sequence(model, item, noise, device):
    """eval.py:89-107 for one sequence on the op graph: noise [S,P,N,2] -> per-sample (loss [S], sum of masked aoe [S], sum of masked foe [S]) and
    the number of fully present pedestrians.  noise None: one decode with the mean fed back (the validation pass, eval.py:63-83)."""
    losses, aoes, foes = [], [], []
    with torch.no_grad():
        for s in range(1 if noise is None else noise.shape[0]):
            loss, gp, xs, info, v_pred_gt = sequence_loss(model, item, device, 0.0, None if noise is None else noise[s:s + 1].to(device))
            lm = info["loss_mask_per_pedestrian"]
            losses.append(loss); aoes.append(average_offset_error(xs, v_pred_gt, lm).sum()); foes.append(final_offset_error(xs, v_pred_gt, lm).sum())
    return torch.stack(losses), torch.stack(aoes), torch.stack(foes), lm.sum()


def _val_row(loss, aoe, foe, m):
    """The validation pass's row for sequences stacked on axis 0, one decode each: loss, aoe, foe [n,1], m [n] -> [n,4]."""
    return torch.stack((loss[:, 0], aoe[:, 0], foe[:, 0], m), 1)


def _test_row(loss, aoe, foe, m):
    """eval.py:108-117 for sequences stacked on axis 0: loss, aoe, foe [n,S], m [n] -> [n,8]: mean loss, aoe mean / std / min, foe mean / std / min, m."""
    return torch.stack((loss.mean(1), aoe.mean(1), aoe.std(1), aoe.min(1).values, foe.mean(1), foe.std(1), foe.min(1).values, m), 1)


def _item_batch(pend):
    """evaluate_batch's first three arguments from loader items."""
    return [it[6] for it in pend], [it[8] for it in pend], [it[4] for it in pend]


def _eval_pass(model, seqs, device, row, ev=None, batch_size=32, draw=None, batch=_item_batch, item=lambda s: s):
    """One pass over sequences in order: up to batch_size of them per cn_gst_eval_step call, the per-sequence rows kept on the device, ONE
    read-back -> rows [sequences, columns] float64.  seqs: (pedestrians, sequence) pairs; sequences of more than 128 pedestrians are skipped
    (eval.py:66), those of more than 64 -- the kernels' bound -- and all of them without an evaluator (ev None) go to the op graph and enter the
    rows ahead of the batch still pending.  row: _val_row or _test_row; draw(pedestrians) -> the sequence's [S,P,N,2] draws (None: validation).
    A sequence is a loader item unless batch(sequences) -> evaluate_batch's first three arguments and item(sequence) -> its loader item say otherwise."""
    rows, pend = [], []

    def flush():
        if pend:
            seq, ped, _ = ev.evaluate_batch(*batch([s for s, _ in pend]), None if draw is None else [nz for _, nz in pend])
            rows.append(row(seq[:, :, 0] / seq[:, :, 1], seq[:, :, 2], seq[:, :, 3], ped[:, 0, :, 2].sum(1)))
            del pend[:]

    with torch.no_grad():
        for n, s in seqs:
            if n > 128:
                continue
            noise = None if draw is None else draw(n)
            if ev is None or n > HipGstEvaluator.MAX_PEDS:
                loss, aoe, foe, m = test_sequence(model, item(s), noise, device)
                rows.append(row(loss.view(1, -1), aoe.view(1, -1), foe.view(1, -1), m.view(1)))
                continue
            pend.append((s, noise))
            if len(pend) == batch_size:
                flush()
        flush()
    return torch.cat(rows, 0).double().cpu().numpy()


def evaluate(model, loader, device, backend=None, batch_size=32):
    """eval.py's `inference` in 'val' mode: mean loss over the sequences, aoe / foe over the fully observed pedestrians.
    backend None / 'torch': the op graph, one sequence at a time.  'hip': cn_gst_eval_step on up to batch_size sequences per call; there `loader`
    may be a DeviceTrajectories, whose gather in its no-rotation form then assembles the batches of consecutive sequences on the device."""
    model.eval()
    if _eval_backend(model, backend) == "hip":
        ev = HipGstEvaluator(model)
        if isinstance(loader, DeviceTrajectories):
            ds = loader
            index = torch.arange(len(ds), dtype=torch.int32, device=ds.device)

            def gather(pend):      # consecutive sequence numbers, unless one between them went to the op graph
                idx = index[pend[0]:pend[-1] + 1] if pend[-1] - pend[0] + 1 == len(pend) else index[torch.as_tensor(pend, device=ds.device)]
                return ds.gather(idx, ds.num_peds(pend))

            r = _eval_pass(model, zip(ds.counts, range(len(ds))), ds.device, _val_row, ev, batch_size, batch=gather, item=lambda i: [t.unsqueeze(0) for t in ds[i]])
        else:
            r = _eval_pass(model, ((item[6].shape[2], item) for item in loader), device, _val_row, ev, batch_size)
        m = max(float(r[:, 3].sum()), 1.0)
        return float(r[:, 0].mean()), float(r[:, 1].sum() / m), float(r[:, 2].sum() / m)
    losses, aoes, foes, ms = [], [], [], []
    with torch.no_grad():
        for item in loader:
            if item[6].shape[2] > 128:
                continue
            loss, gp, xs, info, v_pred_gt = sequence_loss(model, item, device, 0.0)
            lm = info["loss_mask_per_pedestrian"]
            losses.append(loss.item())
            aoes.append(average_offset_error(xs, v_pred_gt, lm).cpu().numpy()); foes.append(final_offset_error(xs, v_pred_gt, lm).cpu().numpy())
            ms.append(lm[0].cpu().numpy())
    m = max(float(np.concatenate(ms).sum()), 1.0)
    return float(np.mean(losses)), float(np.concatenate(aoes).sum() / m), float(np.concatenate(foes).sum() / m)


def test(model, loader, device, num_samples=20, seed=1000, backend=None, batch_size=32, draws=None):
    """eval.py's `inference` in 'test' mode (:84-117, :148-157): num_samples decodes per sequence with the Gaussian sampled and fed back;
    per sequence the mean / unbiased std / min over the samples of the summed masked aoe and foe and the mean of the losses; over the pass those
    sums divided by the number of fully present pedestrians.  -> (loss, aoe, foe, aoe_std, foe_std, aoe_min, foe_min).
    The draws come from a CPU torch.Generator seeded with `seed`: torch.randn [num_samples,P,N,2] per sequence in loader order (P = the model's
    pred_len), the same for both backends; `draws` (an iterable of one [S,P,N,2] tensor per sequence) replaces them with recorded ones.  backend None: 'hip' for a model
    on the GPU, 'torch' otherwise."""
    model.eval()
    if backend is None:
        backend = "hip" if next(model.parameters()).is_cuda else "torch"
    backend = _eval_backend(model, backend)
    gen = torch.Generator().manual_seed(int(seed))
    draws = iter(draws) if draws is not None else None
    draw = lambda n: torch.randn(num_samples, model.pred_len, n, 2, generator=gen) if draws is None else next(draws)   # noqa: E731
    r = _eval_pass(model, ((item[6].shape[2], item) for item in loader), device, _test_row, HipGstEvaluator(model) if backend == "hip" else None, batch_size, draw)
    m = max(float(r[:, 7].sum()), 1.0)
    return (float(r[:, 0].mean()), float(r[:, 1].sum() / m), float(r[:, 4].sum() / m), float(r[:, 2].sum() / m), float(r[:, 5].sum() / m),
            float(r[:, 3].sum() / m), float(r[:, 6].sum() / m))


def train(data_dir=None, out_dir=None, num_epochs=100, temp_epochs=100, lr=1e-3, clip_grad=10.0, rotation_pattern="random", save_epochs=10, init_temp=0.5,
          random_seed=1000, device=None, num_workers=0, log=print, backend=None, val_backend=None, dataset=None, batch_size=1, pred_seq_len=5, p_drop=0.1):
    """gst_updated/scripts/experiments/train.py:49-195 for the shipped configuration.  data_dir holds the text files of collect.py /
    collect_data.py; the first 80 % of every file's windows train, the rest validate (TrajectoriesDataset modes).  Writes
    <out_dir>/checkpoint/{epoch_<n>.pt, args.pickle, train_hist.pickle} in the reference's format (+ args.json / train_hist.json): the
    directory is a valid config.pred.model_dir for load_predictor here and for the reference's CrowdNavPredInterfaceMultiEnv.
    dataset = (train, val) of DeviceTrajectories replaces data_dir.  With backend 'hip' the epoch then runs with the data on the device: the
    order and the angles are drawn up front (epoch_plan: the draws of the per-item loop), minibatches are consecutive chunks of batch_size of that
    order (train.py's args.batch_size; the last may be short), each assembled by cn_gst_gather_batch, and the losses come back once per epoch.
    batch_size > 1 needs that path (a data_dir is uploaded for it).
    pred_seq_len: the prediction horizon P -- windows of 5 + P frames, a predictor that decodes P steps, recorded in args.json / args.pickle for
    load_predictor; 1 .. 8 on the 'hip' backend (_abi.gst_horizon), any on 'torch'.  A dataset=(train, val) must have been cut for the same P.
    p_drop: the dropout of the training steps (the reference's 0.1).  The two backends draw their masks from different streams, so their runs
    differ at the level of the dropout noise; with p_drop = 0 both are deterministic and follow each other step for step."""
    if out_dir is None or (data_dir is None) == (dataset is None):
        raise ValueError("train() needs an out_dir and either a data_dir or dataset=(train, val)")
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1 (got %d)" % batch_size)
    torch.manual_seed(random_seed)
    np.random.seed(random_seed)
    device = torch.device(device if device is not None else ("cuda:0" if torch.cuda.is_available() else "cpu"))
    if backend is None:
        backend = "hip" if device.type == "cuda" else "torch"
    if batch_size > 1 and backend != "hip":
        raise ValueError("batch_size > 1 needs backend='hip': the op graph trains one sequence per step")
    pred_seq_len, p_drop = int(pred_seq_len), float(p_drop)
    if not 0.0 <= p_drop < 1.0:
        raise ValueError("p_drop must be in [0, 1) (got %s)" % p_drop)
    if backend == "hip" or val_backend == "hip":
        from ._abi import gst_horizon
        gst_horizon(pred_seq_len)                  # outside the device box: refused here, before anything is allocated
    elif pred_seq_len < 1:
        raise ValueError("pred_seq_len must be at least 1 (got %d)" % pred_seq_len)
    if dataset is not None:
        ds_train, ds_val = dataset
        for ds in dataset:
            if int(getattr(ds, "pred_seq_len", pred_seq_len)) != pred_seq_len:
                raise ValueError("the dataset holds windows of pred_seq_len = %d, train() was asked for %d" % (ds.pred_seq_len, pred_seq_len))
    else:
        ds_train = TrajectoriesDataset(data_dir, pred_seq_len=pred_seq_len, mode="train")
        ds_val = TrajectoriesDataset(data_dir, pred_seq_len=pred_seq_len, mode="val")
        if batch_size > 1:
            ds_train, ds_val = DeviceTrajectories.from_dataset(ds_train, device), DeviceTrajectories.from_dataset(ds_val, device)
    on_device = backend == "hip" and isinstance(ds_train, DeviceTrajectories)
    loader_train = DataLoader(ds_train, batch_size=1, shuffle=True, num_workers=num_workers)
    loader_val = DataLoader(ds_val, batch_size=1, shuffle=False, num_workers=num_workers)
    model = GSTPredictor(pred_len=pred_seq_len).to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=max(int(temp_epochs / 4), 1), gamma=0.3)
    # backend: 'hip' = the training step as hand-written kernels through the C ABI (HipGstTrainer; the default on a GPU), 'torch' = the op graph
    # above under autograd (CPU tests, and the cross-check of the kernels)
    if backend == "hip" and clip_grad is None:
        raise ValueError("backend='hip' clips the gradient norm in its fused Adam step: pass a clip_grad (the reference's default is 10)")
    # the per-epoch validation follows the training step's backend (cn_gst_eval_step with 'hip'); val_backend forces one ('torch': the op graph)
    if val_backend is None:
        val_backend = backend
    hip_tr = HipGstTrainer(model, lr=lr, clip_grad=clip_grad, seed=random_seed, optimizer=optimizer) if backend == "hip" else None
    ckpt_dir = os.path.join(out_dir, "checkpoint")
    os.makedirs(ckpt_dir, exist_ok=True)
    run_args = dict(spatial="gumbel_social_transformer", temporal="faster_lstm", output_dim=5, embedding_size=64, spatial_num_heads=8,
                    spatial_num_heads_edges=0, spatial_num_layers=1, ghost=False, lstm_hidden_size=64, lstm_num_layers=1, decode_style="recursive",
                    detach_sample=False, motion_dim=2, only_observe_full_period=False, dataset="sj", obs_seq_len=5, pred_seq_len=pred_seq_len, batch_size=batch_size,
                    lr=lr, clip_grad=clip_grad, rotation_pattern=rotation_pattern, num_epochs=num_epochs, temp_epochs=temp_epochs,
                    save_epochs=save_epochs, init_temp=init_temp, random_seed=random_seed, deterministic=False, resume_training=False,
                    resume_epoch=None)
    with open(os.path.join(ckpt_dir, "args.json"), "w") as f:
        json.dump(run_args, f)
    # the reference's loaders (crowd_nav_interface_multi_env_parallel.py:21-28, scripts/experiments/eval.py:30) unpickle an
    # argparse.Namespace from args.pickle and open 'epoch_<args.num_epochs>.pt': write that too (train.py:88-89)
    with open(os.path.join(ckpt_dir, "args.pickle"), "wb") as f:
        pickle.dump(argparse.Namespace(**run_args), f)
    hist = {"epoch": 0, "train_loss_task": [], "val_loss_task": [], "train_aoe_task": [], "val_aoe_task": [], "train_foe_task": [], "val_foe_task": []}
    if on_device:            # the order and the angles drawn up front by the per-item loop's own calls
        run_epoch = lambda: _train_epoch_device(hip_tr, ds_train, *epoch_plan(len(ds_train), rotation_pattern), batch_size, optimizer, model.obs_len, p_drop)   # noqa: E731
    elif hip_tr is not None:
        run_epoch = lambda: _train_epoch_items_hip(hip_tr, loader_train, rotation_pattern, optimizer, device, model.obs_len, p_drop)   # noqa: E731
    else:
        run_epoch = lambda: _train_epoch_items_torch(model, loader_train, rotation_pattern, optimizer, clip_grad, device, p_drop)   # noqa: E731
    for epoch in range(1, num_epochs + 1):
        model.train()
        t0 = time.time()
        tau = temperature(epoch, temp_epochs, init_temp)
        losses, aoes, foes, ms = run_epoch()
        scheduler.step()
        m = max(float(np.concatenate(ms).sum()), 1.0)
        tr = (float(np.mean(losses)), float(np.concatenate(aoes).sum() / m), float(np.concatenate(foes).sum() / m))
        if on_device and val_backend == "hip" and isinstance(ds_val, DeviceTrajectories):
            iter(DataLoader(range(len(ds_val)), batch_size=1, shuffle=False))   # every DataLoader iterator draws its base seed from the global generator
            va = evaluate(model, ds_val, device, backend="hip")
        else:
            va = evaluate(model, loader_val, device, backend=val_backend)
        for k, a, b in (("loss", tr[0], va[0]), ("aoe", tr[1], va[1]), ("foe", tr[2], va[2])):
            hist["train_%s_task" % k].append(a); hist["val_%s_task" % k].append(b)
        hist["epoch"] = epoch
        log("Epoch: %d | train loss: %.4f | val loss: %.4f | train aoe: %.4f | val aoe: %.4f | train foe: %.4f | val foe: %.4f | tau %.3f | period: %.2f sec"
            % (epoch, tr[0], va[0], tr[1], va[1], tr[2], va[2], tau, time.time() - t0))
        if epoch % save_epochs == 0 or epoch == num_epochs:
            torch.save({"epoch": epoch, "model_state_dict": model.state_dict(), "optimizer_state_dict": optimizer.state_dict(),
                        "lr_scheduler_state_dict": scheduler.state_dict(), "train_loss_epoch": tr[0], "val_loss_epoch": va[0], "train_aoe_epoch": tr[1],
                        "val_aoe_epoch": va[1], "train_foe_epoch": tr[2], "val_foe_epoch": va[2]}, os.path.join(ckpt_dir, "epoch_%d.pt" % epoch))
            with open(os.path.join(ckpt_dir, "train_hist.json"), "w") as f:
                json.dump(hist, f)
            with open(os.path.join(ckpt_dir, "train_hist.pickle"), "wb") as f:      # train.py:189-190 (resume reads it back)
                pickle.dump(hist, f)
    model.eval()
    return model, hist


def eval_run(run_dir, data_dir, num_samples=20, seed=1000, device=None, backend=None, log=print):
    """gst_updated/scripts/experiments/eval.py:12-43 for a run directory of train(): the checkpoint's stored validation loss, the validation
    loss recomputed from the loaded model, and the test protocol's line, on the last 20 % of every file's windows of data_dir."""
    device = torch.device(device if device is not None else ("cuda:0" if torch.cuda.is_available() else "cpu"))
    if backend is None:
        backend = "hip" if device.type == "cuda" else "torch"
    path = find_checkpoint(run_dir)
    model = GSTPredictor.from_checkpoint(path, device)
    stored = load_checkpoint(path, "cpu").get("val_loss_epoch")
    loader_val = DataLoader(TrajectoriesDataset(data_dir, pred_seq_len=model.pred_len, mode="val"), batch_size=1, shuffle=False)
    loader_test = DataLoader(TrajectoriesDataset(data_dir, pred_seq_len=model.pred_len, mode="test"), batch_size=1, shuffle=False)
    log("The best validation losses printed below should be the same.")
    log("Validation loss in the checkpoint:  %s" % (stored,))
    val = evaluate(model, loader_val, device, backend=backend)
    log("Validation loss from loaded model:  %s" % (val[0],))
    t = test(model, loader_test, device, num_samples=num_samples, seed=seed, backend=backend)
    log("Test loss from loaded model:  %s" % (t[0],))
    log("dataset: %s | test aoe: %.4f | test aoe std: %.4f | test foe: %.4f | test foe std: %.4f | min aoe: %.4f, min foe: %.4f"
        % (os.path.basename(os.path.normpath(data_dir)), t[1], t[3], t[2], t[4], t[5], t[6]))
    return val, t


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m crowdnav_prediction_attngraph_amd.gst_train")
    sub = ap.add_subparsers(dest="cmd", required=True)
    ev = sub.add_parser("eval", help="validation loss and the sampled test protocol of a trained run (the reference's scripts/experiments/eval.py)")
    ev.add_argument("run_dir"); ev.add_argument("data_dir")
    ev.add_argument("--samples", type=int, default=20); ev.add_argument("--seed", type=int, default=1000)
    ev.add_argument("--device", default=None); ev.add_argument("--backend", default=None, choices=("torch", "hip"))
    a = ap.parse_args(argv)
    eval_run(a.run_dir, a.data_dir, num_samples=a.samples, seed=a.seed, device=a.device, backend=a.backend)


if __name__ == "__main__":
    main()
