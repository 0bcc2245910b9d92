"""Shared helpers of the strided-grid tests (test_strided_refs.py, test_gpu_strided_grids.py): the grid caps of the PPO update's capped launchers
restated from their host code, seeded inputs that put one size class of the human-human attention past its cap, the fp64 CPU references
(vectorised human-human attention with autograd, PPO losses on planted ties, advantage normalisation, embed0) and the per-sample error helpers."""
import numpy as np
import torch

# ---- the caps, restated from the launchers ----
# csrc/srnn_node_train.hip: SA_MAX_BLOCKS workgroups of SA_WAVES wavefronts, one sample per wavefront and trip
SA_CAP = 256 * 16
# csrc/ppo.hip: PPO_BLOCKS blocks of 256 threads (cn_ppo_loss_fwd), 2048 blocks of 256 (cn_ppo_loss_bwd); csrc/rollout.hip: 2048 x 256 (cn_adv_normalize)
PPO_FWD_CAP = 256 * 256
PPO_BWD_CAP = ADV_CAP = 2048 * 256
# csrc/linear.hip: 8192 blocks, one row per block and trip (cn_embed0_fwd); hip_train.Embed0: min(R, 4096) blocks of eight rows per trip
EMBED0_FWD_CAP = 8192
EMBED0_BWD_CAP = 8 * 4096
HH_CLASSES = (8, 16, 32, 64)


def hh_caps():
    """{class: (forward cap, backward cap)} in samples of that class per trip of its launch, from the arithmetic of launch_hh_attention and
    launch_hh_attention_bwd (csrc/attention.h): blocks capped at 256 CUs x resident blocks per CU, wpb (sample, head) units per block, 8 heads."""
    out = {}
    for cap in HH_CLASSES:
        per_wave = (2 * cap * 68 + cap * cap) * 4
        wpb = min(max(65536 // per_wave, 1), 4)
        per_cu = min(160 * 1024 // (per_wave * wpb), 8)
        fwd = 256 * per_cu * wpb // 8
        if cap in (16, 32):                                  # the MFMA backward: 4 / 2 wavefronts per block, two blocks per CU
            wpb, per_cu = (4 if cap == 16 else 2), 2
        else:
            per_wave = (4 * cap * 68 + (4 if cap <= 32 else 2) * cap * cap) * 4
            wpb = min(max(65536 // per_wave, 1), 4)
            per_cu = min(max(160 * 1024 // (per_wave * wpb), 1), 8)
        out[cap] = (fwd, 256 * per_cu * wpb // 8)
    return out


def hh_class(nd):
    return 8 if nd <= 8 else (16 if nd <= 16 else (32 if nd <= 32 else 64))


# ---- human-human attention ----
def hh_counts(groups, seed):
    """groups = [(lo, hi, n)]: n counts uniform in lo .. hi with lo and hi planted, per group; more than one group: the samples of all groups in one
    seeded random order.  int64 [B]."""
    rs = np.random.RandomState(seed)
    parts = []
    for lo, hi, n in groups:
        nd = rs.randint(lo, hi + 1, n)
        nd[0], nd[1] = lo, hi
        parts.append(nd)
    nd = np.concatenate(parts)
    if len(groups) > 1:
        nd = nd[rs.permutation(nd.size)]
    return torch.from_numpy(nd.astype(np.int64))


def hh_inputs(nd, seed):
    """(row_off int32 [B+1], qkv [R,1536], d_out [R,512]) for the counts nd: standard normal float32, as tests/test_gpu_train.py draws them."""
    g = torch.Generator().manual_seed(seed)
    row_off = torch.zeros(nd.numel() + 1, dtype=torch.int32)
    row_off[1:] = torch.cumsum(nd, 0)
    R = int(row_off[-1])
    return row_off, torch.randn(R, 1536, generator=g), torch.randn(R, 512, generator=g)


def hh_reference(qkv, d_out, row_off, scale=0.125):
    """softmax(scale q k^T) v per (sample, head) on the compacted rows and the gradient of sum(out * d_out), in fp64 on the CPU: the samples
    grouped by their count, one batched product with autograd per group.  Returns (out [R,512], d_qkv [R,1536]), float64."""
    qr = qkv.double().requires_grad_()
    g = d_out.double()
    off = row_off.long()
    nd = off[1:] - off[:-1]
    out = torch.zeros(qr.shape[0], 512, dtype=torch.float64)
    loss = qr.new_zeros(())
    for n in torch.unique(nd).tolist():
        rows = (off[:-1][nd == n].unsqueeze(1) + torch.arange(n).unsqueeze(0))          # [G, n]
        blk = qr[rows.reshape(-1)].view(-1, n, 3, 8, 64)
        q, k, v = (blk[:, :, i].transpose(1, 2) for i in range(3))                      # [G, 8, n, 64]
        p = torch.softmax(scale * q @ k.transpose(2, 3), dim=-1)
        o = (p @ v).transpose(1, 2).reshape(-1, 512)                                    # [G * n, 512]
        out[rows.reshape(-1)] = o.detach()
        loss = loss + (o * g[rows.reshape(-1)]).sum()
    return out, torch.autograd.grad(loss, qr)[0]


def hh_reference_loop(qkv, d_out, row_off, scale=0.125):
    """The same as a Python loop over the samples, the formulation of tests/test_gpu_train.py::_check_hh_attention."""
    qr = qkv.double().requires_grad_()
    outs = []
    for b in range(row_off.numel() - 1):
        r0, r1 = int(row_off[b]), int(row_off[b + 1])
        blk = qr[r0:r1].view(r1 - r0, 3, 8, 64)
        q, k, v = blk[:, 0].transpose(0, 1), blk[:, 1].transpose(0, 1), blk[:, 2].transpose(0, 1)     # [8, nd, 64]
        p = torch.softmax(scale * q @ k.transpose(1, 2), dim=-1)
        outs.append((p @ v).transpose(0, 1).reshape(r1 - r0, 512))
    ref = torch.cat(outs)
    ref.backward(d_out.double())
    return ref.detach(), qr.grad


def per_sample_max(x, row_off):
    """x [R, ...] -> float64 numpy [B]: the largest |entry| among the rows row_off[b] .. row_off[b + 1] of every sample b (every count >= 1)."""
    rows = x.reshape(x.shape[0], -1).abs().amax(1).double().numpy()
    return np.maximum.reduceat(rows, row_off[:-1].long().numpy())


def worst(err, cap, label, bar, extra=None):
    """The line every strided test prints and the message of its assertion: the worst sample (or row, element) of err [B], the trip index // cap
    it belongs to (cap = None: left to `extra`) and the bar.  bar may be an array (a bar per sample): the worst is then the largest err / bar.
    Returns (message, whether every sample is within its bar); a NaN is outside."""
    err = np.asarray(err, np.float64)
    bars = np.broadcast_to(np.asarray(bar, np.float64), err.shape)
    ratio = err / bars
    i = int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)))
    msg = "%s: worst %.3g (bar %.3g) at index %d of %d" % (label, err[i], bars[i], i, err.size)
    if cap is not None:
        msg += ", trip %d of cap %d" % (i // cap, cap)
    if extra is not None:
        msg += ", " + extra(i)
    print(msg)
    return msg, bool(np.all(ratio <= 1.0))


# ---- PPO losses on planted ties ----
PPO_CLIP = 0.25
# (name, values, logp, old_logp, adv, value_preds, returns, dv, dlp): every number a multiple of 0.25 (but one old_logp beside adv = 0), so fp32 and
# fp64 see the same tie.  dv = d(0.5 max((v - ret)^2, (vpc - ret)^2)) / dv and dlp = d(-min(surr1, surr2)) / dlogp of that sample by torch's rules,
# worked out by hand: min / max of equal operands send half of the gradient to each, clamp passes it on the closed interval.
PPO_TIES = [
    # adv == 0: both surrogates are zero whatever the ratio (exp(0.25), outside no range), the gradient is zero.  The value side is plain:
    # d = 0.5 is clipped to 0.25, (v - ret)^2 = 1 > (0.75 - 0)^2, dv = v - ret
    ("adv == 0", 1.0, -2.0, -2.25, 0.0, 0.5, 0.0, 1.0, 0.0),
    # logp == old_logp: ratio = 1 exactly, surr1 == surr2; half of the gradient through each, the clamp passes its half: dlp = -adv
    ("ratio == 1, adv > 0", 1.0, -2.0, -2.0, 0.75, 0.5, 0.0, 1.0, -0.75),
    ("ratio == 1, adv < 0", 1.0, -2.0, -2.0, -0.5, 0.5, 0.0, 1.0, 0.5),
    ("ratio == 1, adv == 0", 1.0, -2.0, -2.0, 0.0, 0.5, 0.0, 1.0, 0.0),
    # values == value_preds: vpc = values, both squares equal, the clamp passes at 0: dv = v - ret
    ("values == value_preds", 0.5, -2.0, -2.0, 0.5, 0.5, -0.25, 0.75, -0.5),
    # values - value_preds == +-clip: the clamp still passes (closed interval), vpc = values, tie: dv = v - ret
    ("values - value_preds == +clip", 1.0, -2.0, -2.0, 0.5, 0.75, 0.25, 0.75, -0.5),
    ("values - value_preds == -clip", 0.5, -2.0, -2.0, 0.5, 0.75, 1.5, -1.0, -0.5),
    # ... and values == returns on top: both squares are zero, dv = 0
    ("values - value_preds == +clip, values == returns", 1.0, -2.0, -2.0, 0.5, 0.75, 1.0, 0.0, -0.5),
    ("values - value_preds == -clip, values == returns", 0.5, -2.0, -2.0, 0.5, 0.75, 0.5, 0.0, -0.5),
    # values == returns past the clip range: (v - ret)^2 = 0 < (0.25 - 1)^2, the maximum is the clipped branch, whose clamp blocks: dv = 0
    ("values == returns, past the clip", 1.0, -2.0, -2.0, 0.5, 0.0, 1.0, 0.0, -0.5),
    # equal squares of opposite sign past the clip range: v - ret = 1, vpc - ret = -1.25 + 0.25 - 0 = -1; half of the gradient goes to the
    # unclipped branch, the clamp blocks the other half: dv = 0.5 (v - ret)
    ("equal squares past the clip", 1.0, -2.0, -2.0, 0.5, -1.25, 0.0, 0.5, -0.5),
]
PPO_KINK_MARGIN = 1e-4


def ppo_inputs(n, seed, n_tail=77):
    """Six float32 [n, 1] tensors (values, logp, old_logp, adv, value_preds, returns) drawn as tests/test_gpu_ppo.py draws them, moved off the
    kinks, with PPO_TIES planted; and the planted positions with the index into PPO_TIES of each.

    Off the kinks: at ratio = 1 +- clip, at values - value_preds = +-clip and, past the clip, at returns = (values + clipped values) / 2 (the two
    squares equal) the gradient jumps, and an fp32 and an fp64 graph may take different sides of a sample that lies within rounding of one -- among
    a million samples that is likely.  Random samples closer than PPO_KINK_MARGIN to a kink are moved 0.01 away from it; the exact ties, which both
    precisions see alike, are planted afterwards.
    Planted: n <= len(PPO_TIES) + 1: positions 0 .. n - 2 in order; else every tie at two seeded positions of the whole range and at one of the
    last n_tail elements (the ragged last trip of every capped grid here)."""
    g = torch.Generator().manual_seed(seed)
    values = torch.randn(n, 1, generator=g)
    vp = values + 0.3 * torch.randn(n, 1, generator=g)
    ret = values + torch.randn(n, 1, generator=g)
    old = -2.0 + 0.5 * torch.randn(n, 1, generator=g)
    logp = old + 0.25 * torch.randn(n, 1, generator=g)
    adv = torch.randn(n, 1, generator=g)
    ratio = torch.exp(logp.double() - old.double())
    near = ((ratio - (1 - PPO_CLIP)).abs() < PPO_KINK_MARGIN) | ((ratio - (1 + PPO_CLIP)).abs() < PPO_KINK_MARGIN)
    logp = torch.where(near, logp + 0.01, logp)
    d = values.double() - vp.double()
    near = (d.abs() - PPO_CLIP).abs() < PPO_KINK_MARGIN
    vp = torch.where(near, vp + 0.01, vp)
    d = values.double() - vp.double()
    mid = 0.5 * (values.double() + vp.double() + d.clamp(-PPO_CLIP, PPO_CLIP))      # past the clip, returns == mid makes the two squares equal
    near = (d.abs() > PPO_CLIP) & ((ret.double() - mid).abs() < PPO_KINK_MARGIN)
    ret = torch.where(near, ret + 0.01, ret)
    K = len(PPO_TIES)
    if n <= K + 1:
        pos, kind = np.arange(n - 1), np.arange(n - 1)
    else:
        rs = np.random.RandomState(seed)
        pos = np.concatenate([rs.choice(n - n_tail, 2 * K, replace=False), n - n_tail + rs.choice(n_tail, K, replace=False)])
        kind = np.concatenate([np.arange(K), np.arange(K), np.arange(K)])
    table = torch.tensor([t[1:7] for t in PPO_TIES], dtype=torch.float32)[torch.from_numpy(kind)]
    p = torch.from_numpy(pos)
    for col, t in enumerate((values, logp, old, adv, vp, ret)):
        t[p, 0] = table[:, col]
    return (values, logp, old, adv, vp, ret), pos, kind


def ppo_reference(inputs, clipped=True, clip=PPO_CLIP, w_value=0.5, w_action=1.0):
    """fp64 autograd over tests/test_gpu_ppo.py::_ref_losses on the float32 inputs: (value_loss, action_loss, d_values [n,1], d_logp [n,1]) of
    w_value * value_loss + w_action * action_loss."""
    from tests.test_gpu_ppo import _ref_losses
    values, logp, old, adv, vp, ret = (t.double() for t in inputs)
    vd, ld = values.requires_grad_(), logp.requires_grad_()
    vl, al = _ref_losses(vd, ld, old, adv, vp, ret, clip, clipped)
    (w_value * vl + w_action * al).backward()
    return float(vl.detach()), float(al.detach()), vd.grad, ld.grad


def ppo_tie_gradients(kind, n, w_value=0.5, w_action=1.0):
    """The closed form at the planted positions: (d_values, d_logp) = (w_value dv / n, w_action dlp / n) from PPO_TIES, float64 numpy."""
    dv = np.array([PPO_TIES[k][7] for k in kind], np.float64)
    dlp = np.array([PPO_TIES[k][8] for k in kind], np.float64)
    return w_value * dv / n, w_action * dlp / n


def adv_reference(returns, values):
    """(a - mean) / (std(ddof = 1) + 1e-5) in fp64 numpy on a = the float32 difference returns - values, which is what the kernels take."""
    a = (returns - values).reshape(-1).numpy().astype(np.float64)
    return (a - a.mean()) / (a.std(ddof=1) + 1e-5)


# ---- embed0 ----
def embed0_inputs(R, D):
    """(x [R,D], w [128,D], b [128], dy [R,128]) as tests/test_gpu_train.py::test_embed0_forward_and_gradients_match_fp64 draws them: a fifth of the
    rows, and row R // 2, carry the simulator's padding value 15.0 in every column."""
    g = torch.Generator().manual_seed(100 * R + D)
    x = 3.0 * torch.randn(R, D, generator=g)
    x[torch.rand(R, generator=g) < 0.2] = 15.0
    x[R // 2] = 15.0
    w = torch.randn(128, D, generator=g) / D ** 0.5
    b = torch.randn(128, generator=g) * 0.5
    dy = torch.randn(R, 128, generator=g)
    return x, w, b, dy


def embed0_reference(x, w, b, dy, act):
    """fp64: the pre-activation x w^T + b [R,128] and (dW [128,D], db [128]) of sum(pre * act * dy), act [R,128] the active set to use."""
    ga = (dy.double() * act.double())
    return x.double() @ w.double().t() + b.double(), ga.t() @ x.double(), ga.sum(0)
