"""Training of the GST trajectory predictor on the data-collection env's files -- the counterpart of the reference's
gst_updated/src/mgnn/trajectories.py (dataset), gst_updated/src/gumbel_social_transformer/st_model.py (training-time forward and
loss, :62-112, :271-455) and gst_updated/scripts/experiments/train.py (loop), for the shipped hyper-parameters (SURVEY.md 8a-G3:
embedding 64, 8 heads, 1 layer, spatial_num_heads_edges = 0, no ghost, faster_lstm, obs 5 / pred 5, recursive decoding).

Two execution paths of the training step (train.py:121-146: forward, negative log-likelihood, backward, clip, Adam):
  * on a GPU (backend 'hip', the default there): HipGstTrainer -- cn_gst_train_step (csrc/gst_train.hip: forward + loss + hand-derived
    reverse pass, one workgroup per sequence, the reference's four dropout sites) and flat_adam.FlatAdam (cn_adam_clip_step), through the C ABI;
  * the torch-op graph below under autograd (backend 'torch'): what CPU tensors use (unit tests, pinned to the reference's numbers) and the
    independent cross-check of the kernels (tests/test_gpu_gst_train.py holds the two against each other).
Evaluation (eval.py's `inference`: the per-epoch validation pass and the sampled test protocol) has the same two paths: HipGstEvaluator --
cn_gst_eval_step (csrc/gst_eval.hip), batches of sequences per boundary call, one read-back per pass -- behind evaluate(backend='hip') / test(), and
the torch-op graph (evaluate's default, the CPU tests' path and the cross-check of the kernel).
The learning-rate schedule and the checkpoint format are host code either way, and the producer of the data is the batched simulator
(collect.py: thousands of simulated crowds per GPU).  The dataset and the rotation augmentation have the same two paths: TrajectoriesDataset over the
text files with the per-item loop (train(data_dir, ...)), or DeviceTrajectories -- the sequences cut out of collect_log's observations on the device
(csrc/gst_data.hip), minibatches assembled and rotated there (cn_gst_gather_batch), one read-back per epoch (train(dataset=..., batch_size=...)).

Scope note: the reference trains on `<dataset>_dset_<split>_batch_trajectories.pt` files produced by scripts/data/create_*datasets*.py,
which are NOT part of the reference checkout (only the shell wrappers that call them are).  This module therefore feeds the loop with
TrajectoriesDataset items directly -- one sequence (all pedestrians of a 10-frame window) per optimiser step, which is what a
BatchTrajectoriesDataset item of one sequence is.
"""
import argparse
import json
import math
import os
import pickle
import time

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, Dataset

from .gst import GSTPredictor

INVALID = -999.0


def read_file(path, delim="\t"):
    """trajectories.py:163-174: rows of (frame id, pedestrian id, x, y)."""
    delim = {"tab": "\t", "space": " "}.get(delim, delim)
    rows = []
    with open(path, "r") as f:
        for line in f:
            line = line.strip()
            if line:
                rows.append([float(v) for v in line.split(delim)])
    return np.asarray(rows, dtype=np.float64).reshape(-1, 4)


def seq_to_graph(seq, seq_rel):
    """mgnn/utils.py:44-77 with attn_mech 'rel_conv': V[t, h] = displacement of pedestrian h at step t; A[t, i, j] = pos_i - pos_j."""
    V = seq_rel.permute(2, 0, 1).contiguous().float()                  # [T, N, 2]
    x = seq.permute(2, 0, 1).float()                                  # [T, N, 2]
    A = x.unsqueeze(2) - x.unsqueeze(1)                               # [T, N, N, 2]
    return V, A


class TrajectoriesDataset(Dataset):
    """gst_updated/src/mgnn/trajectories.py:9-160.  Every window of obs + pred consecutive frames of a file in which at least one
    pedestrian is present throughout becomes a sequence: positions / displacements [N, 2, T] (-999 where missing), loss masks [N, T],
    the graph tensors of seq_to_graph and the per-step attention masks (outer product of the displacement mask)."""

    def __init__(self, data_dir, obs_seq_len=5, pred_seq_len=5, skip=1, delim="\t", invalid_value=INVALID, mode=None, frame_diff=1.0, verbose=False):
        super().__init__()
        self.data_dir, self.obs_seq_len, self.pred_seq_len, self.skip = data_dir, obs_seq_len, pred_seq_len, skip
        self.seq_len = T = obs_seq_len + pred_seq_len
        files = [os.path.join(data_dir, p) for p in os.listdir(data_dir)]
        num_peds, seqs, seqs_rel, masks, masks_rel, self.frame_id_seq = [], [], [], [], [], []
        for path in files:
            if verbose:
                print(path)
            data = read_file(path, delim)
            frames = np.unique(data[:, 0]).tolist()
            frame_data = [data[data[:, 0] == fr, :] for fr in frames]
            num_sequences = math.floor((len(frames) - T) / skip) + 1
            stop = num_sequences * skip + 1
            if mode is None:
                idx_range = range(0, stop, skip)
            elif mode == "train":
                idx_range = range(0, int(stop * 0.8), skip)
            elif mode in ("val", "test"):
                idx_range = range(int(stop * 0.8), stop, skip)
            else:
                raise RuntimeError("Wrong mode for TrajectoriesDataset.")
            for idx in idx_range:
                chunk = frame_data[idx:idx + T]
                if not chunk:
                    continue
                cur = np.concatenate(chunk, axis=0)
                start = cur[0, 0]
                peds = np.unique(cur[:, 1])
                # slot of every row inside the window (frame id -> step), rows on other frame ids are ignored like in the reference
                step_f = (cur[:, 0] - start) / frame_diff
                step = np.rint(step_f).astype(np.int64)
                on_grid = (step_f == step) & (step >= 0) & (step < T)
                col = np.searchsorted(peds, cur[:, 1])
                present = np.zeros((len(peds), T), dtype=np.int64)
                np.add.at(present, (col[on_grid], step[on_grid]), 1)
                if present.max() > 1:
                    raise RuntimeError("The same pedestrian has multiple locations in the same frame.")
                # :60-68 a pedestrian with a row in EVERY one of the window's frames, those frames spaced by frame_diff
                survive = False
                for k in range(len(peds)):
                    fr_k = np.unique(cur[col == k, 0])
                    if len(fr_k) == T and np.all(fr_k[1:] - fr_k[:-1] == frame_diff):
                        survive = True
                        break
                if not survive:
                    continue
                seq = np.ones((len(peds), 2, T)) * invalid_value
                seq_rel = np.ones((len(peds), 2, T)) * invalid_value
                seq[col[on_grid], :, step[on_grid]] = cur[on_grid, 2:]
                m = present.astype(np.float64)
                m_rel = np.zeros_like(m)
                m_rel[:, 0] = m[:, 0]
                m_rel[:, 1:] = m[:, 1:] * m[:, :-1]
                rel = np.zeros_like(seq)
                rel[:, :, 1:] = seq[:, :, 1:] - seq[:, :, :-1]
                sel = m_rel.astype(bool)[:, None, :].repeat(2, axis=1)
                seq_rel[sel] = rel[sel]
                num_peds.append(len(peds)); seqs.append(seq); seqs_rel.append(seq_rel); masks.append(m); masks_rel.append(m_rel)
                self.frame_id_seq.append(start)
        self.num_seq = len(seqs)
        if self.num_seq == 0:
            raise RuntimeError("no sequence of %d frames with a pedestrian present throughout in %s" % (T, data_dir))
        seq_all, rel_all = np.concatenate(seqs, axis=0), np.concatenate(seqs_rel, axis=0)
        self.obs_traj = torch.from_numpy(seq_all[:, :, :obs_seq_len]).type(torch.float)
        self.pred_traj = torch.from_numpy(seq_all[:, :, obs_seq_len:]).type(torch.float)
        self.obs_traj_rel = torch.from_numpy(rel_all[:, :, :obs_seq_len]).type(torch.float)
        self.pred_traj_rel = torch.from_numpy(rel_all[:, :, obs_seq_len:]).type(torch.float)
        self.loss_mask = torch.from_numpy(np.concatenate(masks, axis=0)).type(torch.float)
        self.loss_mask_rel = torch.from_numpy(np.concatenate(masks_rel, axis=0)).type(torch.float)
        cum = [0] + np.cumsum(num_peds).tolist()
        self.seq_start_end = list(zip(cum[:-1], cum[1:]))
        self.v_obs, self.A_obs, self.v_pred, self.A_pred, self.attn_mask_obs, self.attn_mask_pred = [], [], [], [], [], []
        for s, e in self.seq_start_end:
            v, a = seq_to_graph(self.obs_traj[s:e], self.obs_traj_rel[s:e])
            self.v_obs.append(v); self.A_obs.append(a)
            v, a = seq_to_graph(self.pred_traj[s:e], self.pred_traj_rel[s:e])
            self.v_pred.append(v); self.A_pred.append(a)
            lm = self.loss_mask_rel[s:e]                                              # [N, T]
            am = (lm.t().unsqueeze(2) * lm.t().unsqueeze(1)).float()                  # [T, N, N]
            self.attn_mask_obs.append(am[:obs_seq_len]); self.attn_mask_pred.append(am[obs_seq_len:])

    def __len__(self):
        return self.num_seq

    def __getitem__(self, index):
        s, e = self.seq_start_end[index]
        return [self.obs_traj[s:e], self.pred_traj[s:e], self.obs_traj_rel[s:e], self.pred_traj_rel[s:e], self.loss_mask_rel[s:e],
                self.loss_mask[s:e], self.v_obs[index], self.A_obs[index], self.v_pred[index], self.A_pred[index],
                self.attn_mask_obs[index], self.attn_mask_pred[index]]


# ---- training-time forward (st_model.forward with sampling = False) on the checkpoint-compatible GSTPredictor ----
def _transformer_train(model, x, attn_mask, p_drop):
    """GSTPredictor._transformer with the reference's four dropout sites (mha.py:243, node_encoder_layer_no_ghost.py:57,61,62)."""
    g = model.gumbel_social_transformer
    L = g.node_encoder_layers[0]
    B, H, _ = x.shape
    tr = model.training and p_drop > 0
    x = g.node_embedding(x)
    ped = (attn_mask.sum(-1) > 0).to(x.dtype).unsqueeze(-1)
    x = L.norm_node(x) * ped
    q, k, v = [t.view(B, H, 8, 8).transpose(1, 2) for t in F.linear(x, L.self_attn.in_proj_weight, L.self_attn.in_proj_bias).chunk(3, dim=-1)]
    p = torch.softmax((q * 8 ** -0.5) @ k.transpose(-1, -2), dim=-1)
    p = p * attn_mask.unsqueeze(1)
    p = p / (p.sum(-1, keepdim=True) + 1e-10)
    p = F.dropout(p, p_drop, tr)
    o = (p @ v).transpose(1, 2).reshape(B, H, 64)
    x = x + F.dropout(L.self_attn.out_proj(o), p_drop, tr)
    x2 = F.dropout(F.relu(L.linear1(L.norm1_node(x))), p_drop, tr)
    return x + F.dropout(L.linear2(x2), p_drop, tr)


def forward_train(model, v_obs, attn_mask_obs, loss_mask_rel, p_drop=0.1, noise=None):
    """st_model.py:271-455 (faster_lstm, recursive, only_observe_full_period = False).
    v_obs [1,T,N,2], attn_mask_obs [1,T,N,N] (neighbour, target), loss_mask_rel [1,N,T+P] ->
    (mu [1,P,N,2], sx, sy, corr [1,P,N,1]), x_sample_pred [1,P,N,2], info{'loss_mask_rel_full_partial', 'loss_mask_per_pedestrian'}.
    noise None: sampling = False, the mean is fed back.  noise [1,P,N,2] (standard-normal draws): sampling = True with sample_gaussian's
    arithmetic (st_model.py:235-240) on the caller's draws instead of torch.empty(...).normal_()."""
    B, T, N, _ = v_obs.shape
    P = model.pred_len
    dev = v_obs.device
    lm_pp = (loss_mask_rel.sum(2) == loss_mask_rel.shape[2]).float()
    am = attn_mask_obs.permute(0, 1, 3, 2).reshape(B * T, N, N)                       # (target, neighbour)
    xs = _transformer_train(model, v_obs.reshape(B * T, N, 2), am, p_drop).view(B, T, N, 64)
    xs = xs * loss_mask_rel[:, :, :T].permute(0, 2, 1).unsqueeze(-1)
    h = torch.zeros(B * N, 64, device=dev, dtype=xs.dtype)
    c = torch.zeros_like(h)
    for t in range(T):
        h, c = model._lstm_cell(xs[:, t].reshape(B * N, 64), h, c)
    lm_fp = loss_mask_rel[:, :, T - 1]                                                # [B, N]
    mk = lm_fp.reshape(B * N, 1)
    h, c = h * mk, c * mk
    attn_pred = (lm_fp.unsqueeze(2) * lm_fp.unsqueeze(1)).permute(0, 2, 1)
    mus, sxs, sys_, cors, samples = [], [], [], [], []
    x_sample = None
    for tt in range(P):
        if tt > 0:
            xt = _transformer_train(model, x_sample.reshape(B, N, 2), attn_pred, p_drop).reshape(B * N, 64) * mk
            hp, cp = model._lstm_cell(xt, h, c)
            h = hp * mk + h * (1 - mk)
            c = cp * mk + c * (1 - mk)
        raw = model.hidden2pos(h).view(B, N, 5).unsqueeze(1)
        mu = raw[..., :2]
        mus.append(mu); sxs.append(raw[..., 2:3].exp()); sys_.append(raw[..., 3:4].exp()); cors.append(raw[..., 4:5].tanh())
        if noise is not None:
            sx, sy, corr, ex, ey = sxs[-1], sys_[-1], cors[-1], noise[:, tt:tt + 1, :, 0:1], noise[:, tt:tt + 1, :, 1:2]
            mu = torch.cat((sx * ex, corr * sy * ex + ((1. - corr ** 2.) ** 0.5) * sy * ey), dim=3) + mu
        x_sample = mu * lm_fp.unsqueeze(1).unsqueeze(-1)
        samples.append(x_sample)
    gp = (torch.cat(mus, 1), torch.cat(sxs, 1), torch.cat(sys_, 1), torch.cat(cors, 1))
    return gp, torch.cat(samples, 1), {"loss_mask_rel_full_partial": lm_fp, "loss_mask_per_pedestrian": lm_pp}


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


def rotate_graph(vtx, theta):
    """mgnn/utils.py:80-90 (vertices only: the edge tensor is unused with spatial_num_heads_edges = 0)."""
    c, s = np.cos(theta), np.sin(theta)
    return torch.cat((vtx[..., 0:1] * c - vtx[..., 1:2] * s, vtx[..., 0:1] * s + vtx[..., 1:2] * c), dim=-1)


def sequence_loss(model, item, device, p_drop=0.1, noise=None):
    """One step's loss exactly as train.py:113-137 computes it (non-deterministic branch: NLL / number of valid (step, pedestrian)).
    noise: see forward_train (the test protocol's sampled decode)."""
    obs_traj, pred_gt, obs_rel, pred_rel_gt, lm_rel, lm, v_obs, A_obs, v_pred_gt, A_pred_gt, am_obs, am_pred = item
    v_obs, v_pred_gt, am_obs, lm_rel = v_obs.to(device), v_pred_gt.to(device), am_obs.to(device), lm_rel.to(device)
    gp, xs, info = forward_train(model, v_obs, am_obs, lm_rel, p_drop, noise)
    prob_loss, elm = negative_log_likelihood_full_partial(gp, v_pred_gt, info["loss_mask_rel_full_partial"], lm_rel[:, :, -model.pred_len:])
    return prob_loss.sum() / elm.sum(), gp, xs, info, v_pred_gt


class HipGstTrainer:
    """The training step of the predictor on the MI355X through the C ABI: forward + negative log-likelihood + backward as ONE boundary call
    (cn_gst_train_step, csrc/gst_train.hip: one workgroup per sequence, hand-derived reverse pass, the reference's four dropout sites with the
    library's own counter-based masks) and gradient-norm clip + Adam as another (flat_adam.FlatAdam: cn_adam_clip_step over one flat bucket).  Replaces, per
    optimiser step, train.py:121-146: model(...) -> negative_log_likelihood_full_partial -> loss.backward() -> clip_grad_norm_ -> optimizer.step().
    The model's parameters become views of the flat bucket, so state_dict() / checkpoints are those of the torch path."""

    def __init__(self, model, lr=1e-3, clip_grad=10.0, betas=(0.9, 0.999), eps=1e-8, seed=1000, optimizer=None):
        from . import _abi as A
        from .flat_adam import FlatAdam
        self.A, self.model = A, model
        named = dict(model.named_parameters())
        named = [(k, named[k]) for _, k in A.GST_WEIGHT_KEYS]
        if not all(p.is_cuda and p.dtype == torch.float32 for _, p in named):
            raise A.CnError("HipGstTrainer: the predictor must live on the GPU in float32 (there is no CPU fallback of the HIP path)")
        self.flat = FlatAdam(named, optimizer)   # the torch optimiser object stays the owner of the moments (its state_dict() goes into the checkpoints)
        self.w, self.g = A.GstWeights(), A.GstWeights()
        for (field, _), (pv, gv, _, _) in zip(A.GST_WEIGHT_KEYS, self.flat.views):
            setattr(self.w, field, pv.data_ptr())
            setattr(self.g, field, gv.data_ptr())
        self.lr, self.clip_grad, self.betas, self.eps, self.seed = float(lr), clip_grad, betas, float(eps), int(seed)
        self.ws, self.dev = None, self.flat.p.device

    @property
    def step_no(self):
        return self.flat.step_no

    def loss_and_grads(self, v_obs, v_pred, loss_mask_rel, p_drop=0.1, seed=None):
        """v_obs [B,5,N,2], v_pred [B,5,N,2], loss_mask_rel [B,N,10] (any device) -> (loss_and_count [2] on the device, gauss [B,5,N,5]: mu_x, mu_y,
        sigma_x, sigma_y, corr); the gradients land in the flat bucket (every parameter's .grad).  Crowds of fewer than 4 pedestrians are padded
        with absent ones."""
        A = self.A
        C = A.C
        B, T, N, _ = v_obs.shape
        if T != 5 or v_pred.shape[1] != 5 or N > 64:
            raise A.CnError("HipGstTrainer: 5 observed + 5 predicted steps and at most 64 pedestrians per sequence (got %d + %d steps, %d pedestrians)" % (T, v_pred.shape[1], N))
        Np = max(N, 4)
        f = lambda t: t.to(self.dev, torch.float32)   # noqa: E731
        vo, vp, lm = f(v_obs), f(v_pred), f(loss_mask_rel)
        if Np != N:
            vo = torch.nn.functional.pad(vo, (0, 0, 0, Np - N)); vp = torch.nn.functional.pad(vp, (0, 0, 0, Np - N)); lm = torch.nn.functional.pad(lm, (0, 0, 0, Np - N))
        vo, vp, lm = vo.contiguous(), vp.contiguous(), lm.contiguous()
        need = int(A.lib().cn_gst_train_workspace_bytes(B, Np))
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        out = torch.empty(2, device=self.dev)
        gauss = torch.empty(B, 5, Np, 5, device=self.dev)
        sd = self.seed + 7919 * self.step_no if seed is None else int(seed)
        with torch.cuda.device(self.dev):
            A.check(A.lib().cn_gst_train_step(B, Np, A.ptr(vo), A.ptr(vp), A.ptr(lm), C.byref(self.w), C.byref(self.g), float(p_drop), C.c_uint64(sd & (2 ** 64 - 1)),
                                              C.c_void_p(self.ws.data_ptr()), int(self.ws.numel()), A.ptr(out), A.ptr(gauss), A.stream_ptr()), "cn_gst_train_step")
        return out, gauss[:, :, :N]

    def optimizer_step(self, grad_scale=1.0):
        """clip_grad_norm_(parameters, clip_grad) + Adam.step() (train.py:143-146) over the flat bucket.  grad_scale multiplies the gradient before
        the norm is taken (train.py:134: loss / args.batch_size ahead of backward and clip_grad_norm_)."""
        self.flat.step(self.lr, self.betas, self.eps, self.clip_grad, grad_scale=grad_scale)
        self.flat.sync_optimizer_state()


def temperature(epoch, total_epochs, base_temp, temp_min=0.03):
    """temperature_scheduler.py (kept for the checkpoint / log; without edge heads the Gumbel temperature is never read)."""
    return max((1 - epoch / total_epochs) * (base_temp - temp_min) + temp_min, temp_min)


class HipGstEvaluator:
    """Evaluation of the predictor on the MI355X through the C ABI: cn_gst_eval_step (csrc/gst_eval.hip) runs, for a batch of sequences in one
    boundary call, what eval.py:63-117 does per sequence -- the forward with dropout off, the masked negative log-likelihood and the
    average / final offset errors; validation (the mean fed back) or the test protocol (S sampled decodes per sequence on the caller's draws).
    The kernels read the model's parameters where they are (also when they are views of a HipGstTrainer's flat bucket): nothing is copied."""

    MAX_PEDS, MAX_SAMPLES = 64, 64

    def __init__(self, model):
        from . import _abi as A
        self.A = A
        self.model = model
        params = self._params()
        if not all(p.is_cuda and p.dtype == torch.float32 for p in params):
            raise A.CnError("HipGstEvaluator: the predictor must live on the GPU in float32 (there is no CPU fallback of the HIP path)")
        self.dev = params[0].device
        self.ws = None

    def _params(self):
        named = dict(self.model.named_parameters())
        return [named[k] for _, k in self.A.GST_WEIGHT_KEYS]

    def evaluate_batch(self, v_obs, v_pred, loss_mask_rel, noise=None):
        """v_obs, v_pred [B,5,N,2], loss_mask_rel [B,N,10] (any device), or lists of B per-sequence tensors ([5,N_b,2] / [N_b,10], a leading
        axis of one allowed) of different crowd sizes; noise None (validation) or [B,S,5,N,2] / a list of [S,5,N_b,2] (test: S decodes per
        sequence on these standard-normal draws).  Crowds are padded to the batch's largest (at least four) with absent pedestrians.
        -> seq [B,R,4] (NLL sum, valid pairs, sum of masked aoe, sum of masked foe), ped [B,R,N,3] (aoe, foe, loss_mask_per_pedestrian),
        gauss [B,R,5,N,5] (mu_x, mu_y, sigma_x, sigma_y, corr), R = max(S, 1), all on the device (nothing is read back here)."""
        A = self.A
        C = A.C
        vo, vp, lm, nz = self._stack(v_obs, 3, 1), self._stack(v_pred, 3, 1), self._stack(loss_mask_rel, 2, 0), None if noise is None else self._stack(noise, 4, 2)
        B, T, N, _ = vo.shape
        if T != 5 or vp.shape[1] != 5 or N > self.MAX_PEDS:
            raise A.CnError("HipGstEvaluator: 5 observed + 5 predicted steps and at most 64 pedestrians per sequence (got %d + %d steps, %d pedestrians)" % (T, vp.shape[1], N))
        S = 0 if nz is None else int(nz.shape[1])
        if nz is not None and (S < 1 or S > self.MAX_SAMPLES or tuple(nz.shape) != (B, S, 5, N, 2)):
            raise A.CnError("HipGstEvaluator: noise must be [B,S,5,N,2] with 1 <= S <= 64 (got %s for B=%d, N=%d)" % (tuple(nz.shape), B, N))
        Np = max(N, 4)
        if Np != N:
            pad = torch.nn.functional.pad
            vo, vp, lm = pad(vo, (0, 0, 0, Np - N)), pad(vp, (0, 0, 0, Np - N)), pad(lm, (0, 0, 0, Np - N))
            nz = None if nz is None else pad(nz, (0, 0, 0, Np - N))
        f = lambda t: None if t is None else t.to(self.dev, torch.float32, non_blocking=True).contiguous()   # noqa: E731
        vo, vp, lm, nz = f(vo), f(vp), f(lm), f(nz)
        w = A.GstWeights()
        for (field, _), p in zip(A.GST_WEIGHT_KEYS, self._params()):
            setattr(w, field, p.data_ptr())
        need = int(A.lib().cn_gst_eval_workspace_bytes(B, Np, S))
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        R = max(S, 1)
        seq, ped, gauss = torch.empty(B, R, 4, device=self.dev), torch.empty(B, R, Np, 3, device=self.dev), torch.empty(B, R, 5, Np, 5, device=self.dev)
        with torch.cuda.device(self.dev):
            A.check(A.lib().cn_gst_eval_step(B, Np, S, A.ptr(vo), A.ptr(vp), A.ptr(lm), C.byref(w), A.ptr(nz), C.c_void_p(self.ws.data_ptr()), int(self.ws.numel()),
                                             A.ptr(seq), A.ptr(ped), A.ptr(gauss), A.stream_ptr()), "cn_gst_eval_step")
        return seq, ped[:, :, :N], gauss[:, :, :, :N]

    @staticmethod
    def _stack(x, rank, ax):
        """A tensor as it is; a list of per-sequence tensors of `rank` axes (a leading axis of one allowed) padded along the pedestrian axis `ax`
        with zeros (absent pedestrians) and stacked."""
        if torch.is_tensor(x):
            return x
        xs = [t[0] if t.dim() == rank + 1 else t for t in x]
        n = max(t.shape[ax] for t in xs)
        out = []
        for t in xs:
            if t.shape[ax] != n:
                shape = list(t.shape)
                shape[ax] = n - t.shape[ax]
                t = torch.cat((t, torch.zeros(shape, dtype=t.dtype, device=t.device)), dim=ax)
            out.append(t)
        return torch.stack(out, 0)


class DeviceTrajectories(Dataset):
    """TrajectoriesDataset's content as device tensors: the six ragged arrays (obs_traj, pred_traj, obs_traj_rel, pred_traj_rel [P,2,5],
    loss_mask, loss_mask_rel [P,10]), seq_start_end, frame_id_seq and the env of every sequence (seq_env).  from_log builds it on the device
    from collect.collect_log's observations (csrc/gst_data.hip: cn_gst_data_frames / _count / _fill, no files, one read-back); from_dataset
    uploads a TrajectoriesDataset.  __getitem__ returns the host class's 12 entries as device tensors (the graph tensors are made on demand),
    so evaluate / test / the torch backend take it through a DataLoader unchanged; gather() assembles a minibatch for cn_gst_train_step /
    cn_gst_eval_step on the device (cn_gst_gather_batch)."""

    FIELDS = ("obs_traj", "pred_traj", "obs_traj_rel", "pred_traj_rel", "loss_mask", "loss_mask_rel")

    def __init__(self, arrays, counts, frame_id_seq, seq_env, obs_seq_len=5, pred_seq_len=5):
        super().__init__()
        from . import _abi as A
        self.A = A
        self.obs_seq_len, self.pred_seq_len, self.skip, self.seq_len = obs_seq_len, pred_seq_len, 1, obs_seq_len + pred_seq_len
        for k, t in zip(self.FIELDS, arrays):
            setattr(self, k, t)
        self.device = self.obs_traj.device
        self.counts = np.asarray(counts, dtype=np.int64)
        self.num_seq = len(self.counts)
        if self.num_seq == 0:
            raise RuntimeError("no sequence of %d frames with a pedestrian present throughout" % self.seq_len)
        cum = [0] + np.cumsum(self.counts).tolist()
        self.seq_start_end = list(zip(cum[:-1], cum[1:]))
        self.total_peds = int(cum[-1])
        self.frame_id_seq = [np.float64(v) for v in frame_id_seq]
        self.seq_env = np.asarray(seq_env, dtype=np.int64)
        self._seq_start = torch.as_tensor(np.asarray(cum[:-1], dtype=np.int32)).to(self.device)
        self._seq_count = torch.as_tensor(self.counts.astype(np.int32)).to(self.device)

    @classmethod
    def from_dataset(cls, ds, device):
        """Upload of a TrajectoriesDataset (the sequences' envs are not known to it: seq_env is -1)."""
        dev = torch.device(device)
        arrays = [getattr(ds, k).to(dev, torch.float32).contiguous() for k in cls.FIELDS]
        return cls(arrays, [e - s for s, e in ds.seq_start_end], ds.frame_id_seq, [-1] * len(ds.seq_start_end), ds.obs_seq_len, ds.pred_seq_len)

    @classmethod
    def from_log(cls, log, mode=None, env_ids=None):
        """log [F,E,H,4] float32 on the device (collect.collect_log) -> what TrajectoriesDataset(dir, mode=mode) holds for the files
        collect_lines writes from it, files in env order.  env_ids: only these envs, in this order.  Raises on a log the rule does not cover:
        frame ids that do not strictly increase within an env (an episode boundary), a sample with the same prediction id twice, a sequence
        of more than 64 pedestrians."""
        from . import _abi as A
        if mode not in A.GSTD_MODES:
            raise RuntimeError("Wrong mode for TrajectoriesDataset.")
        if not (torch.is_tensor(log) and log.is_cuda and log.dtype == torch.float32 and log.dim() == 4 and log.shape[3] == 4):
            raise A.CnError("DeviceTrajectories.from_log: log must be a float32 [F,E,H,4] tensor on the GPU (there is no CPU fallback of the HIP path)")
        envs = None if env_ids is None else [int(e) for e in env_ids]
        if envs is not None:
            log = log[:, torch.as_tensor(envs, dtype=torch.int64, device=log.device)]
        log = log.contiguous()
        F_, E, H, _ = log.shape
        if H > A.CN_MAX_HUMANS:
            raise A.CnError("DeviceTrajectories.from_log: %d rows per observation, the kernels stop at %d" % (H, A.CN_MAX_HUMANS))
        if F_ < 10 or E < 1:
            raise RuntimeError("no sequence of 10 frames with a pedestrian present throughout in a log of %d samples of %d envs" % (F_, E))
        dev, L, md, W = log.device, A.lib(), A.GSTD_MODES[mode], F_ - 9
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)   # noqa: E731
        visible, frame_id, status = i32(F_, E), torch.empty(F_, E, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        frame_list, ped_count, first_frame = i32(E, F_), i32(E * W), torch.empty(E * W, device=dev)
        with torch.cuda.device(dev):
            A.check(L.cn_gst_data_frames(F_, E, H, A.ptr(log), A.ptr(visible), A.ptr(frame_id), A.ptr(status), A.stream_ptr()), "cn_gst_data_frames")
            listed_before = (torch.cumsum(visible, 0).to(torch.int32) - visible).contiguous()
            A.check(L.cn_gst_data_count(F_, E, H, md, A.ptr(log), A.ptr(visible), A.ptr(listed_before), A.ptr(frame_id), A.ptr(frame_list), A.ptr(ped_count),
                                        A.ptr(first_frame), A.ptr(status), A.stream_ptr()), "cn_gst_data_count")
            ped_offset = (torch.cumsum(ped_count, 0).to(torch.int32) - ped_count).contiguous()
            host = torch.cat((status, ped_count, first_frame.view(torch.int32))).cpu().numpy()       # the one read-back of the build
            st, counts, first = int(host[0]), host[1:1 + E * W].astype(np.int64), host[1 + E * W:].view(np.float32)
            if st & A.GSTD_FRAME_ORDER:
                raise RuntimeError("DeviceTrajectories.from_log: the frame ids of an env do not strictly increase (the log spans an episode boundary)")
            if st & A.GSTD_DUPLICATE_ID:
                raise RuntimeError("The same pedestrian has multiple locations in the same frame.")
            if st & A.GSTD_TOO_MANY_PEDS:
                raise RuntimeError("DeviceTrajectories.from_log: a window holds more than %d pedestrians, the training kernels' bound" % A.CN_MAX_HUMANS)
            is_seq = counts > 0
            total = int(counts.sum())
            if total == 0:
                raise RuntimeError("no sequence of 10 frames with a pedestrian present throughout in the log (mode %r)" % (mode,))
            if total >= 2 ** 31 // 10:
                raise A.CnError("DeviceTrajectories.from_log: %d pedestrian rows exceed the 32-bit offsets of the build" % total)
            arrays = [torch.empty(total, 2, 5, device=dev) for _ in range(4)] + [torch.empty(total, 10, device=dev) for _ in range(2)]
            A.check(L.cn_gst_data_fill(F_, E, H, md, A.ptr(log), A.ptr(visible), A.ptr(listed_before), A.ptr(frame_id), A.ptr(frame_list), A.ptr(ped_count),
                                       A.ptr(ped_offset), total, *([A.ptr(t) for t in arrays] + [A.stream_ptr()])), "cn_gst_data_fill")
        env_of = np.nonzero(is_seq)[0] // W
        return cls(arrays, counts[is_seq], first[is_seq], env_of if envs is None else np.asarray(envs, dtype=np.int64)[env_of])

    def __len__(self):
        return self.num_seq

    def __getitem__(self, index):
        s, e = self.seq_start_end[index]
        T = self.obs_seq_len
        v_obs, A_obs = seq_to_graph(self.obs_traj[s:e], self.obs_traj_rel[s:e])
        v_pred, A_pred = seq_to_graph(self.pred_traj[s:e], self.pred_traj_rel[s:e])
        lm = self.loss_mask_rel[s:e]
        am = (lm.t().unsqueeze(2) * lm.t().unsqueeze(1)).float()
        return [self.obs_traj[s:e], self.pred_traj[s:e], self.obs_traj_rel[s:e], self.pred_traj_rel[s:e], lm, self.loss_mask[s:e],
                v_obs, A_obs, v_pred, A_pred, am[:T], am[T:]]

    def gather(self, index, num_peds, cos_sin=None):
        """index [B] int32 on the device, num_peds = max(4, the largest crowd among them), cos_sin None or [B,2] float32 on the device ->
        v_obs, v_pred [B,5,num_peds,2] (seq_to_graph's vertices, rotated as rotate_graph does), loss_mask_rel [B,num_peds,10]; rows at or beyond a
        sequence's crowd are zeros."""
        A = self.A
        B = int(index.shape[0])
        if index.dtype != torch.int32 or (cos_sin is not None and (cos_sin.dtype != torch.float32 or tuple(cos_sin.shape) != (B, 2))):
            raise A.CnError("DeviceTrajectories.gather: index must be int32 [B] and cos_sin float32 [B,2]")
        v_obs, v_pred = torch.empty(B, 5, num_peds, 2, device=self.device), torch.empty(B, 5, num_peds, 2, device=self.device)
        lm = torch.empty(B, num_peds, 10, device=self.device)
        with torch.cuda.device(self.device):
            A.check(A.lib().cn_gst_gather_batch(B, int(num_peds), self.num_seq, self.total_peds, A.ptr(index), A.ptr(cos_sin), A.ptr(self._seq_start),
                                                A.ptr(self._seq_count), A.ptr(self.obs_traj_rel), A.ptr(self.pred_traj_rel), A.ptr(self.loss_mask_rel),
                                                A.ptr(v_obs), A.ptr(v_pred), A.ptr(lm), A.stream_ptr()), "cn_gst_gather_batch")
        return v_obs, v_pred, lm

    def num_peds(self, order):
        """The gather's pedestrian axis for the sequences `order` (host indices): max(4, the largest crowd among them)."""
        return max(4, int(self.counts[order].max()))


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


def _train_epoch_device(hip_tr, ds, order, thetas, batch_size, optimizer, obs_len):
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
        out, gauss = hip_tr.loss_and_grads(vo, vp, lm_rel, p_drop=0.1)
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


def _train_epoch_items_hip(hip_tr, loader, rotation_pattern, optimizer, device, obs_len):
    """One epoch of one loader item per optimiser step through the kernels: forward, loss, backward (dropout 0.1 like model.train()) as one boundary
    call, then the fused clip + Adam step.  -> (losses, aoes, foes, ms), one entry per step."""
    rows = []
    for item in _train_items(loader, rotation_pattern):
        lm_rel = item[4].to(device)
        hip_tr.lr = optimizer.param_groups[0]["lr"]                           # the StepLR schedule drives the fused step too
        out, gauss = hip_tr.loss_and_grads(item[6], item[8], lm_rel, p_drop=0.1)
        hip_tr.optimizer_step()
        rows.append(_item_terms(out[0], *_step_sample_and_mask(gauss, lm_rel, obs_len), item[8].to(device)))
    return tuple(zip(*rows))


def _train_epoch_items_torch(model, loader, rotation_pattern, optimizer, clip_grad, device):
    """The same epoch on the op graph under autograd (train.py:121-146)."""
    rows = []
    for item in _train_items(loader, rotation_pattern):
        loss, gp, xs, info, v_pred_gt = sequence_loss(model, item, device)
        loss.backward()
        rows.append(_item_terms(loss.detach(), xs.detach(), info["loss_mask_per_pedestrian"], v_pred_gt))
        if clip_grad is not None:
            torch.nn.utils.clip_grad_norm_(model.parameters(), clip_grad)
        optimizer.step()
        optimizer.zero_grad()
    return tuple(zip(*rows))


def _evaluate_device(model, ds, batch_size=32):
    """evaluate(backend='hip') with the data on the device: the gather in its no-rotation form feeds cn_gst_eval_step, batches of consecutive
    sequences, one read-back per pass."""
    model.eval()
    ev = HipGstEvaluator(model)
    index = torch.arange(len(ds), dtype=torch.int32, device=ds.device)
    rows = []
    with torch.no_grad():
        for lo in range(0, len(ds), batch_size):
            hi = min(lo + batch_size, len(ds))
            seq, ped, _ = ev.evaluate_batch(*ds.gather(index[lo:hi], ds.num_peds(np.arange(lo, hi))))
            rows.append(torch.stack((seq[:, 0, 0] / seq[:, 0, 1], seq[:, 0, 2], seq[:, 0, 3], ped[:, 0, :, 2].sum(1)), 1))
    r = torch.cat(rows, 0).double().cpu().numpy()
    m = max(float(r[:, 3].sum()), 1.0)
    return float(r[:, 0].mean()), float(r[:, 1].sum() / m), float(r[:, 2].sum() / m)


def _eval_backend(model, backend):
    if backend is None:
        return "torch"
    if backend not in ("torch", "hip"):
        raise ValueError("backend must be None, 'torch' or 'hip' (got %r)" % (backend,))
    return backend


def _evaluate_hip(model, loader, device, batch_size):
    """The validation pass in batches of sequences through cn_gst_eval_step: per-sequence results stay on the device, one read-back per pass."""
    ev = HipGstEvaluator(model)
    rows, pend = [], []

    def flush():
        if pend:
            seq, ped, _ = ev.evaluate_batch([it[6] for it in pend], [it[8] for it in pend], [it[4] for it in pend])
            rows.append(torch.stack((seq[:, 0, 0] / seq[:, 0, 1], seq[:, 0, 2], seq[:, 0, 3], ped[:, 0, :, 2].sum(1)), 1))
            del pend[:]

    with torch.no_grad():
        for item in loader:
            n = item[6].shape[2]
            if n > 128:
                continue
            if n > HipGstEvaluator.MAX_PEDS:      # the kernels stop at 64 pedestrians: the op graph takes the sequence
                loss, gp, xs, info, v_pred_gt = sequence_loss(model, item, device, 0.0)
                lm = info["loss_mask_per_pedestrian"]
                rows.append(torch.stack((loss, average_offset_error(xs, v_pred_gt, lm).sum(), final_offset_error(xs, v_pred_gt, lm).sum(), lm.sum())).view(1, 4))
                continue
            pend.append(item)
            if len(pend) == batch_size:
                flush()
        flush()
    r = torch.cat(rows, 0).double().cpu().numpy()
    m = max(float(r[:, 3].sum()), 1.0)
    return float(r[:, 0].mean()), float(r[:, 1].sum() / m), float(r[:, 2].sum() / m)


def evaluate(model, loader, device, backend=None, batch_size=32):
    """eval.py's `inference` in 'val' mode: mean loss over the sequences, aoe / foe over the fully observed pedestrians.
    backend None / 'torch': the op graph, one sequence at a time.  'hip': cn_gst_eval_step on up to batch_size sequences per call."""
    model.eval()
    if _eval_backend(model, backend) == "hip":
        return _evaluate_hip(model, loader, device, batch_size)
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


def test_sequence(model, item, noise, device):
    """eval.py:89-107 for one sequence on the op graph: noise [S,5,N,2] -> per-sample (loss [S], sum of masked aoe [S], sum of masked foe [S]) and
    the number of fully present pedestrians."""
    losses, aoes, foes = [], [], []
    with torch.no_grad():
        for s in range(noise.shape[0]):
            loss, gp, xs, info, v_pred_gt = sequence_loss(model, item, device, 0.0, noise[s:s + 1].to(device))
            lm = info["loss_mask_per_pedestrian"]
            losses.append(loss); aoes.append(average_offset_error(xs, v_pred_gt, lm).sum()); foes.append(final_offset_error(xs, v_pred_gt, lm).sum())
    return torch.stack(losses), torch.stack(aoes), torch.stack(foes), lm.sum()


def _test_row(loss, aoe, foe, m):
    """eval.py:108-117 for sequences stacked on axis 0: loss, aoe, foe [n,S], m [n] -> [n,8]: mean loss, aoe mean / std / min, foe mean / std / min, m."""
    return torch.stack((loss.mean(1), aoe.mean(1), aoe.std(1), aoe.min(1).values, foe.mean(1), foe.std(1), foe.min(1).values, m), 1)


def test(model, loader, device, num_samples=20, seed=1000, backend=None, batch_size=32, draws=None):
    """eval.py's `inference` in 'test' mode (:84-117, :148-157): num_samples decodes per sequence with the Gaussian sampled and fed back;
    per sequence the mean / unbiased std / min over the samples of the summed masked aoe and foe and the mean of the losses; over the pass those
    sums divided by the number of fully present pedestrians.  -> (loss, aoe, foe, aoe_std, foe_std, aoe_min, foe_min).
    The draws come from a CPU torch.Generator seeded with `seed`: torch.randn [num_samples,5,N,2] per sequence in loader order, the same for
    both backends; `draws` (an iterable of one [S,5,N,2] tensor per sequence) replaces them with recorded ones.  backend None: 'hip' for a model
    on the GPU, 'torch' otherwise."""
    model.eval()
    if backend is None:
        backend = "hip" if next(model.parameters()).is_cuda else "torch"
    backend = _eval_backend(model, backend)
    gen = torch.Generator().manual_seed(int(seed))
    draws = iter(draws) if draws is not None else None
    ev = HipGstEvaluator(model) if backend == "hip" else None
    rows, pend = [], []

    def flush():
        if pend:
            seq, ped, _ = ev.evaluate_batch([it[6] for it, _ in pend], [it[8] for it, _ in pend], [it[4] for it, _ in pend], [nz for _, nz in pend])
            rows.append(_test_row(seq[:, :, 0] / seq[:, :, 1], seq[:, :, 2], seq[:, :, 3], ped[:, 0, :, 2].sum(1)))
            del pend[:]

    with torch.no_grad():
        for item in loader:
            n = item[6].shape[2]
            if n > 128:
                continue
            noise = torch.randn(num_samples, 5, n, 2, generator=gen) if draws is None else next(draws)
            if ev is None or n > HipGstEvaluator.MAX_PEDS:
                loss, aoe, foe, m = test_sequence(model, item, noise, device)
                rows.append(_test_row(loss.view(1, -1), aoe.view(1, -1), foe.view(1, -1), m.view(1)))
                continue
            pend.append((item, noise))
            if len(pend) == batch_size:
                flush()
        flush()
    r = torch.cat(rows, 0).double().cpu().numpy()
    m = max(float(r[:, 7].sum()), 1.0)
    return (float(r[:, 0].mean()), float(r[:, 1].sum() / m), float(r[:, 4].sum() / m), float(r[:, 2].sum() / m), float(r[:, 5].sum() / m),
            float(r[:, 3].sum() / m), float(r[:, 6].sum() / m))


def train(data_dir=None, out_dir=None, num_epochs=100, temp_epochs=100, lr=1e-3, clip_grad=10.0, rotation_pattern="random", save_epochs=10, init_temp=0.5,
          random_seed=1000, device=None, num_workers=0, log=print, backend=None, val_backend=None, dataset=None, batch_size=1):
    """gst_updated/scripts/experiments/train.py:49-195 for the shipped configuration.  data_dir holds the text files of collect.py /
    collect_data.py; the first 80 % of every file's windows train, the rest validate (TrajectoriesDataset modes).  Writes
    <out_dir>/checkpoint/{epoch_<n>.pt, args.pickle, train_hist.pickle} in the reference's format (+ args.json / train_hist.json): the
    directory is a valid config.pred.model_dir for load_predictor here and for the reference's CrowdNavPredInterfaceMultiEnv.
    dataset = (train, val) of DeviceTrajectories replaces data_dir.  With backend 'hip' the epoch then runs with the data on the device: the
    order and the angles are drawn up front (epoch_plan: the draws of the per-item loop), minibatches are consecutive chunks of batch_size of that
    order (train.py's args.batch_size; the last may be short), each assembled by cn_gst_gather_batch, and the losses come back once per epoch.
    batch_size > 1 needs that path (a data_dir is uploaded for it)."""
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
    if dataset is not None:
        ds_train, ds_val = dataset
    else:
        ds_train = TrajectoriesDataset(data_dir, mode="train")
        ds_val = TrajectoriesDataset(data_dir, mode="val")
        if batch_size > 1:
            ds_train, ds_val = DeviceTrajectories.from_dataset(ds_train, device), DeviceTrajectories.from_dataset(ds_val, device)
    on_device = backend == "hip" and isinstance(ds_train, DeviceTrajectories)
    loader_train = DataLoader(ds_train, batch_size=1, shuffle=True, num_workers=num_workers)
    loader_val = DataLoader(ds_val, batch_size=1, shuffle=False, num_workers=num_workers)
    model = GSTPredictor().to(device)
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
                    detach_sample=False, motion_dim=2, only_observe_full_period=False, dataset="sj", obs_seq_len=5, pred_seq_len=5, batch_size=batch_size,
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
        run_epoch = lambda: _train_epoch_device(hip_tr, ds_train, *epoch_plan(len(ds_train), rotation_pattern), batch_size, optimizer, model.obs_len)   # noqa: E731
    elif hip_tr is not None:
        run_epoch = lambda: _train_epoch_items_hip(hip_tr, loader_train, rotation_pattern, optimizer, device, model.obs_len)   # noqa: E731
    else:
        run_epoch = lambda: _train_epoch_items_torch(model, loader_train, rotation_pattern, optimizer, clip_grad, device)   # noqa: E731
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
            va = _evaluate_device(model, ds_val)
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
    from .gst import GSTPredictor, find_checkpoint, load_checkpoint
    device = torch.device(device if device is not None else ("cuda:0" if torch.cuda.is_available() else "cpu"))
    if backend is None:
        backend = "hip" if device.type == "cuda" else "torch"
    path = find_checkpoint(run_dir)
    model = GSTPredictor.from_checkpoint(path, device)
    stored = load_checkpoint(path, "cpu").get("val_loss_epoch")
    loader_val = DataLoader(TrajectoriesDataset(data_dir, mode="val"), batch_size=1, shuffle=False)
    loader_test = DataLoader(TrajectoriesDataset(data_dir, mode="test"), batch_size=1, shuffle=False)
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
