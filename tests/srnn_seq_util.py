"""Shared helpers of the DS-RNN edge-sequence tests (test_srnn_train_host.py, test_gpu_srnn_train.py, test_gpu_srnn_shapes.py): formula-weight
policies of any (H, D), seeded synthetic [T, N] sequences in the simulator's ranges, the fp64 definitions (op loop, its gradients, the loss through
evaluate_actions), the gradient bar and the launch arithmetic of the kernels restated."""
import os
import re

import numpy as np
import torch

from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces
from tests import policy_util as PU

# (T, N, H, D): the smallest shapes that reach every tile case of the sequence kernels (64 rows per tile, per weight set)
SHAPES = [(1, 1, 1, 2),      # less than one tile of either kind
          (3, 3, 20, 2),     # 60 spatial rows, under one tile
          (4, 4, 20, 12),    # 80 rows: one tile plus a tail; a temporal tile of 4
          (2, 2, 64, 2),     # exactly two full spatial tiles
          (30, 2, 5, 2)]     # the real sequence length
OBS_KEYS = ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num")


def shape_id(s):
    return "t%d_n%d_h%d_d%d" % tuple(s)


def policy(H, D, N, T):
    ob_space, act_space = make_spaces(H, D)
    pol = Policy(ob_space.spaces, act_space, base="srnn", base_kwargs=dict(num_processes=N, num_mini_batch=1, seq_length=T))
    sd = PU.formula_state_dict({k: tuple(v.shape) for k, v in pol.state_dict().items()})
    pol.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return pol


def sequence(T, N, H, D, seed=11):
    """dict(obs = {key: [T*N, ...]}, node_h0 [N,128], edge_h0 [N,H+1,256], masks [T*N,1], actions [T*N,2]) as float32 CPU tensors.  Unseen
    humans are padded with 15 m (PU.synth_obs).  Masks: env 0 is reset at t = 0, env 1 at the interior steps 1 and T - 2 and env 2 at T // 2,
    where those exist (two envs: env 0 again at T // 2); the last env is never reset."""
    steps = [PU.synth_obs(N, H, D, seed + 31 * t) for t in range(T)]
    obs = {k: torch.from_numpy(np.concatenate([s[k] for s in steps], 0)) for k in OBS_KEYS}
    rs = np.random.RandomState(seed)
    masks = np.ones((T, N, 1), np.float32)
    masks[0, 0] = 0.0
    if N > 2:
        for t in (1, T - 2):
            if 0 < t < T:
                masks[t, 1] = 0.0
    if N > 3 and T > 2:
        masks[T // 2, 2] = 0.0
    if N == 2 and T > 2:
        masks[T // 2, 0] = 0.0          # two envs: env 0 is also the one with an interior reset
    if N > 1:
        masks[:, N - 1] = 1.0
    return dict(obs=obs, node_h0=torch.from_numpy(rs.uniform(-0.5, 0.5, (N, 128)).astype(np.float32)),
                edge_h0=torch.from_numpy(rs.uniform(-0.9, 0.9, (N, H + 1, 256)).astype(np.float32)),
                masks=torch.from_numpy(masks.reshape(T * N, 1)), actions=torch.from_numpy(rs.uniform(-1, 1, (T * N, 2)).astype(np.float32)))


def op_loop(pol, seq, T, N, dtype, device="cpu"):
    """h_all [T,N,H+1,256] of the torch-op loop (the definition), from SRNNBase's own cells."""
    from crowdnav_prediction_attngraph_amd.policy import _gru_cell
    b = pol.base
    H = b.human_num
    to = lambda t: t.to(device=device, dtype=dtype)  # noqa: E731
    et, es = b.humanhumanEdgeRNN_temporal, b.humanhumanEdgeRNN_spatial
    gi_t = b._edge_gi(et, to(seq["obs"]["temporal_edges"]).reshape(T * N, 2)).view(T, N, -1)
    gi_s = b._edge_gi(es, to(seq["obs"]["spatial_edges"]).reshape(T * N, H, -1)).view(T, N, H, -1)
    m = to(seq["masks"]).reshape(T, N, 1)
    e0 = to(seq["edge_h0"])
    h_t, h_s = e0[:, 0], e0[:, 1:]
    out = []
    for t in range(T):
        h_t = _gru_cell(gi_t[t], h_t * m[t], et.gru.weight_hh_l0, et.gru.bias_hh_l0)
        h_s = _gru_cell(gi_s[t], h_s * m[t].unsqueeze(1), es.gru.weight_hh_l0, es.gru.bias_hh_l0)
        out.append(torch.cat((h_t.unsqueeze(1), h_s), 1))
    return torch.stack(out, 0)


def d_h_all(T, N, H, seed=5):
    """A seeded gradient of h_all in [-1, 1], float32 [T,N,H+1,256]."""
    return torch.from_numpy(np.random.RandomState(seed).uniform(-1, 1, (T, N, H + 1, 256)).astype(np.float32))


def op_grads(pol64, seq, T, N, d_h):
    """The gradients of sum(op_loop * d_h) in fp64 on the CPU (torch.autograd.grad): the twelve of pol64.base._edge_parameters(), in that order
    (_abi.SRNN_EDGE_KEYS), then the one of edge_h0.  pol64 is a .double() copy; neither it nor seq is written."""
    e0 = seq["edge_h0"].double().requires_grad_(True)
    h = op_loop(pol64, dict(seq, edge_h0=e0), T, N, torch.float64)
    return [g.detach() for g in torch.autograd.grad((h * d_h.double()).sum(), pol64.base._edge_parameters() + [e0])]


def evaluate(p, seq, dev, dt):
    """The loss of tests/test_gpu_srnn.py through evaluate_actions; returns value, log-prob, {name: grad or None} and the gradient of edge_h0."""
    to = lambda t: t.to(device=dev, dtype=dt)  # noqa: E731
    e0 = to(seq["edge_h0"]).requires_grad_(True)
    p.zero_grad(set_to_none=True)
    v, lp, ent, _ = p.evaluate_actions({k: to(t) for k, t in seq["obs"].items()}, {"human_node_rnn": to(seq["node_h0"]), "human_human_edge_rnn": e0},
                                       to(seq["masks"]), to(seq["actions"]))
    w = torch.linspace(-1, 1, v.numel(), dtype=dt, device=dev).view_as(v)
    ((v * w).sum() + (lp * w.flip(0)).sum() + ent).backward()
    grads = {n: (None if q.grad is None else q.grad.detach().cpu().double().clone()) for n, q in p.named_parameters()}
    return v.detach().cpu().double(), lp.detach().cpu().double(), grads, e0.grad.detach().cpu().double()


def check_grads(got, want, mode, label, cancelling=(), dead=()):
    """Every tensor of `want` ({name: fp64 gradient or None}) at 5e-4 of its largest entry + 1e-7 (the bar of tests/test_gpu_minibatch_step.py); the
    names in `cancelling`, in mode 'bf16x3' only, at 1e-2 of the largest entry and 1 - cos <= 2e-6 instead; names starting with `dead` are None on
    both sides.  Prints the eight worst ratios."""
    rows, bad = [], []
    for name, g64 in want.items():
        if dead and name.startswith(dead):
            assert got[name] is None and g64 is None, name
            continue
        scale = float(g64.abs().max())
        err = float((got[name] - g64).abs().max())
        cos = float((g64 * got[name]).sum() / (g64.norm() * got[name].norm()).clamp(min=1e-30))
        rows.append((err / max(scale, 1e-30), name, err, scale, 1 - cos))
        if mode == "bf16x3" and name in cancelling:
            ok = err <= 1e-2 * scale and 1 - cos <= 2e-6
        else:
            ok = err <= 5e-4 * scale + 1e-7
        if not ok:
            bad.append((name, err, scale, 1 - cos))
    for r in sorted(rows, reverse=True)[:8]:
        print("%s %s  %.2e  %-58s err %.3e  max %.3e  1-cos %.2e" % (label, mode, r[0], r[1], r[2], r[3], r[4]))
    assert not bad, bad


# ---- the launch arithmetic of csrc/srnn.hip (srnn_forward) and csrc/srnn_train.hip (cn_srnn_seq_fwd / _bwd, set_wgrads), restated ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constants():
    """SR_TILE, SR_G, SW_ROWS from the kernel headers and CN_SRNN_SEQ_CHUNKS from the public one."""
    csrc = os.path.join(ROOT, "crowdnav_prediction_attngraph_amd", "csrc")
    text = open(os.path.join(csrc, "srnn_kernels.h")).read() + open(os.path.join(csrc, "srnn_train_kernels.h")).read()
    c = {k: int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1)) for k in ("SR_TILE", "SR_G", "SW_ROWS")}
    hdr = open(os.path.join(ROOT, "include", "crowdnav_hip.h")).read()
    c["CHUNKS"] = int(re.search(r"#define CN_SRNN_SEQ_CHUNKS (\d+)", hdr).group(1))
    return c


def launch_plan(T, N, H, D, c=None):
    """What the host code launches for a [T, N] sequence (T = 1: one rollout forward of N envs) of H humans and edge width D:
    tiles_t / tiles_s  workgroups of the edge kernels per weight set (temporal ones first), last_t / last_s the live rows of the last one;
    groups / last_group  workgroups of srnn_node_kernel and the envs of the last one;
    kb  the 16-column blocks of the spatial encoder gradient's operand [x | 1];
    s / t  the weight-gradient ranges of the spatial / temporal set: M rows, rpc rows per range, chunks ranges, last = rows of the last one."""
    c = c or kernel_constants()
    up = lambda a, b: -(-a // b)  # noqa: E731

    def tiles(rows):
        n = up(rows, c["SR_TILE"])
        return n, rows - (n - 1) * c["SR_TILE"]

    def ranges(M):
        rpc = max(256, up(up(M, c["CHUNKS"]), c["SW_ROWS"]) * c["SW_ROWS"])
        chunks = up(M, rpc)
        return dict(M=M, rpc=rpc, chunks=chunks, last=M - (chunks - 1) * rpc)

    (tiles_t, last_t), (tiles_s, last_s) = tiles(N), tiles(N * H)
    groups = up(N, c["SR_G"])
    return dict(tiles_t=tiles_t, last_t=last_t, tiles_s=tiles_s, last_s=last_s, groups=groups, last_group=N - (groups - 1) * c["SR_G"],
                kb=1 if D + 1 <= 16 else 5, s=ranges(T * N * H), t=ranges(T * N))
