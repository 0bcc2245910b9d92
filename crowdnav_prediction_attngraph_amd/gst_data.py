"""The GST predictor's training data -- the counterpart of the reference's gst_updated/src/mgnn/trajectories.py (dataset) and the graph helpers of
mgnn/utils.py.  Two forms of the same content: TrajectoriesDataset over the text files of collect.py / collect_data.py, per-item, on the host;
DeviceTrajectories -- the sequences cut out of collect_log's observations on the device (csrc/gst_data.hip), minibatches assembled and rotated
there (cn_gst_gather_batch)."""
import math
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from . import _abi as A
from .gst import INVALID


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


def rotate_graph(vtx, theta):
    """mgnn/utils.py:80-90 (vertices only: the edge tensor is unused with spatial_num_heads_edges = 0)."""
    c, s = np.cos(theta), np.sin(theta)
    return torch.cat((vtx[..., 0:1] * c - vtx[..., 1:2] * s, vtx[..., 0:1] * s + vtx[..., 1:2] * c), dim=-1)


class DeviceTrajectories(Dataset):
    """TrajectoriesDataset's content as device tensors: the six ragged arrays (obs_traj, obs_traj_rel [peds,2,5], pred_traj, pred_traj_rel
    [peds,2,P], loss_mask, loss_mask_rel [peds,5 + P]; P = pred_seq_len in 1 .. 8), seq_start_end, frame_id_seq and the env of every sequence (seq_env).  from_log builds it on the device
    from collect.collect_log's observations (csrc/gst_data.hip: cn_gst_data_frames_horizon / _count_horizon / _fill_horizon, no files, one read-back); from_dataset
    uploads a TrajectoriesDataset.  __getitem__ returns the host class's 12 entries as device tensors (the graph tensors are made on demand),
    so evaluate / test / the torch backend take it through a DataLoader unchanged; gather() assembles a minibatch for cn_gst_train_step /
    cn_gst_eval_step on the device (cn_gst_gather_batch_horizon)."""

    FIELDS = ("obs_traj", "pred_traj", "obs_traj_rel", "pred_traj_rel", "loss_mask", "loss_mask_rel")

    def __init__(self, arrays, counts, frame_id_seq, seq_env, obs_seq_len=5, pred_seq_len=5):
        super().__init__()
        self.pred_seq_len = A.gst_horizon(pred_seq_len, obs_seq_len)
        self.obs_seq_len, self.skip, self.seq_len = obs_seq_len, 1, obs_seq_len + pred_seq_len
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
    def from_log(cls, log, mode=None, env_ids=None, pred_seq_len=5):
        """log [F,E,H,4] float32 on the device (collect.collect_log) -> what TrajectoriesDataset(dir, pred_seq_len=pred_seq_len, mode=mode)
        holds for the files collect_lines writes from it, files in env order; windows of T = 5 + pred_seq_len frames.  env_ids: only these envs, in this order.  Raises on a log the rule does not cover:
        frame ids that do not strictly increase within an env (an episode boundary), a sample with the same prediction id twice, a sequence
        of more than 64 pedestrians."""
        P = A.gst_horizon(pred_seq_len)
        T = 5 + P
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
        if F_ < T or E < 1:
            raise RuntimeError("no sequence of %d frames with a pedestrian present throughout in a log of %d samples of %d envs" % (T, F_, E))
        dev, L, md, W = log.device, A.lib(), A.GSTD_MODES[mode], F_ - (T - 1)
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)   # noqa: E731
        visible, frame_id, status = i32(F_, E), torch.empty(F_, E, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        frame_list, ped_count, first_frame = i32(E, F_), i32(E * W), torch.empty(E * W, device=dev)
        with torch.cuda.device(dev):
            A.call("cn_gst_data_frames_horizon", F_, E, H, P, A.ptr(log), A.ptr(visible), A.ptr(frame_id), A.ptr(status), A.stream_ptr())
            listed_before = (torch.cumsum(visible, 0).to(torch.int32) - visible).contiguous()
            A.call("cn_gst_data_count_horizon", F_, E, H, md, P, A.ptr(log), A.ptr(visible), A.ptr(listed_before), A.ptr(frame_id), A.ptr(frame_list), A.ptr(ped_count),
                   A.ptr(first_frame), A.ptr(status), A.stream_ptr())
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
                raise RuntimeError("no sequence of %d frames with a pedestrian present throughout in the log (mode %r)" % (T, mode))
            if total >= 2 ** 31 // T:
                raise A.CnError("DeviceTrajectories.from_log: %d pedestrian rows exceed the 32-bit offsets of the build" % total)
            arrays = [torch.empty(total, 2, n, device=dev) for n in (5, P, 5, P)] + [torch.empty(total, T, device=dev) for _ in range(2)]
            A.call("cn_gst_data_fill_horizon", F_, E, H, md, P, A.ptr(log), A.ptr(visible), A.ptr(listed_before), A.ptr(frame_id), A.ptr(frame_list), A.ptr(ped_count),
                   A.ptr(ped_offset), total, *([A.ptr(t) for t in arrays] + [A.stream_ptr()]))
        env_of = np.nonzero(is_seq)[0] // W
        return cls(arrays, counts[is_seq], first[is_seq], env_of if envs is None else np.asarray(envs, dtype=np.int64)[env_of], 5, P)

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
        v_obs [B,5,num_peds,2], v_pred [B,P,num_peds,2] (seq_to_graph's vertices, rotated as rotate_graph does), loss_mask_rel [B,num_peds,5 + P]; rows at or beyond a
        sequence's crowd are zeros."""
        B = int(index.shape[0])
        if index.dtype != torch.int32 or (cos_sin is not None and (cos_sin.dtype != torch.float32 or tuple(cos_sin.shape) != (B, 2))):
            raise A.CnError("DeviceTrajectories.gather: index must be int32 [B] and cos_sin float32 [B,2]")
        P = self.pred_seq_len
        v_obs, v_pred = torch.empty(B, 5, num_peds, 2, device=self.device), torch.empty(B, P, num_peds, 2, device=self.device)
        lm = torch.empty(B, num_peds, 5 + P, device=self.device)
        A.call("cn_gst_gather_batch_horizon", B, int(num_peds), P, self.num_seq, self.total_peds, A.ptr(index), A.ptr(cos_sin), A.ptr(self._seq_start),
               A.ptr(self._seq_count), A.ptr(self.obs_traj_rel), A.ptr(self.pred_traj_rel), A.ptr(self.loss_mask_rel),
               A.ptr(v_obs), A.ptr(v_pred), A.ptr(lm), A.stream_ptr(), device=self.device)
        return v_obs, v_pred, lm

    def num_peds(self, order):
        """The gather's pedestrian axis for the sequences `order` (host indices): max(4, the largest crowd among them)."""
        return max(4, int(self.counts[order].max()))
