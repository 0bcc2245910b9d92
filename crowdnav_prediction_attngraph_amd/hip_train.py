"""The training path's boundary calls: the torch.autograd.Functions over the update-time kernels, the linear / weight-gradient helpers, the
rollout math (gae, adv_*), clip + Adam over a flat bucket (adam_clip_step) and the one-call PPO minibatch (MinibatchStepper)."""
import ctypes as C

import torch

from . import _abi as A


class SrnnEdgeSequence(torch.autograd.Function):
    """Both edge GRUs of the DS-RNN baseline over a [T,N] rollout slice: h_t = GRU(ReLU(enc x_t), mask_t * h_{t-1}) for the temporal edge and
    the H spatial edges, on the kernel and with the arithmetic of the rollout (cn_srnn_seq_fwd), and BPTT plus the weight gradients as
    cn_srnn_seq_bwd.  (hip, temporal_edges [T*N,2], spatial_edges [T*N,H,D], edge_h0 [N,H+1,256], masks [T*N,1], *the twelve parameters in
    A.SRNN_EDGE_KEYS order) -> h_all [T,N,H+1,256].  `hip` is a HipSrnn whose weight snapshot holds these parameters (Policy._hip_handle sees
    to that); the parameter arguments only give autograd somewhere to put the gradients."""

    @staticmethod
    def forward(ctx, hip, temporal_edges, spatial_edges, edge_h0, masks, *params):
        N = edge_h0.shape[0]
        T = masks.numel() // N
        te, se, h0, m = (t.detach().contiguous() for t in (temporal_edges, spatial_edges, edge_h0, masks))
        h_all, ws = hip.seq_fwd(te, se, h0, m, T, N)
        ctx.hip, ctx.ws, ctx.TN = hip, ws, (T, N)
        ctx.shapes = [p.shape for p in params]
        ctx.save_for_backward(te, se, h0, m, h_all)
        return h_all

    @staticmethod
    def backward(ctx, d_h_all):
        te, se, h0, m, h_all = ctx.saved_tensors
        T, N = ctx.TN
        if ctx.ws is None:
            raise RuntimeError("SrnnEdgeSequence: the backward consumes the saved gates; it cannot run twice")
        grads = [torch.empty(s, device=h_all.device) for s in ctx.shapes]
        d_h0 = torch.empty_like(h0) if ctx.needs_input_grad[3] else None
        ctx.hip.seq_bwd(te, se, h0, m, h_all, d_h_all.contiguous(), ctx.ws, T, N, grads, d_h0)
        ctx.ws = None
        return (None, None, None, d_h0, None) + tuple(grads)


class SrnnAttention(torch.autograd.Function):
    """The DS-RNN baseline's edge attention (SRNNBase.attention) over the saved edge states, read in place: (h_all [..., H+1, 256] -- slot 0 the
    temporal edge, slots 1 .. H the spatial edges --, Wt [64,256], bt [64], Ws [64,256], bs [64]) -> (weighted [..., 256], attn [..., H]) as
    cn_srnn_attn_fwd / cn_srnn_attn_bwd (plain fp32).  te . (Ws s_j + bs) = (Ws^T te) . s_j + te . bs and the softmax does not see the second
    term: the kernels never read bs, and its gradient is an exact zero (not None).  The backward writes every element of d_h_all once, as
    SrnnEdgeSequence.backward takes it; the three weight gradients are sums over all rows on the split-K kernel (cn_linear_wgrad, N = 64,
    K = 256).  attn is not differentiable (a tap).  with_t = True adds a third output, the temporal rows h_all[..., 0, :] as a tensor of their own:
    a consumer that uses it instead of a view of h_all hands its gradient to the kernel (d_t_direct) rather than to a zero-filled d_h_all."""

    @staticmethod
    def forward(ctx, h_all, Wt, bt, Ws, bs, with_t=False):
        if not (h_all.is_cuda and h_all.dtype == torch.float32):
            raise A.CnError("SrnnAttention: h_all must be a float32 tensor on the GPU (CPU tensors take SRNNBase.attention), got %s on %s"
                            % (h_all.dtype, h_all.device))
        if h_all.dim() < 2 or h_all.shape[-1] != 256 or tuple(Wt.shape) != (64, 256) or tuple(Ws.shape) != (64, 256) or bt.numel() != 64 or bs.numel() != 64:
            raise A.CnError("SrnnAttention: h_all [..., H+1, 256], Wt / Ws [64,256], bt / bs [64] expected, got %s, %s, %s, %s, %s"
                            % tuple(list(t.shape) for t in (h_all, Wt, bt, Ws, bs)))
        h_all = h_all.detach().contiguous()
        lead, H = h_all.shape[:-2], h_all.shape[-2] - 1
        B = h_all.numel() // ((H + 1) * 256)
        wt, b_t, ws = (p.detach().contiguous() for p in (Wt, bt, Ws))
        dev = h_all.device
        weighted, attn = torch.empty(B, 256, device=dev), torch.empty(B, H, device=dev)
        te, u = torch.empty(B, 64, device=dev), torch.empty(B, 256, device=dev)
        A.call("cn_srnn_attn_fwd", B, H, A.ptr(h_all), A.ptr(wt), A.ptr(b_t), A.ptr(ws), A.ptr(weighted), A.ptr(attn), A.ptr(te), A.ptr(u), A.stream_ptr(),
               device=dev)
        ctx.save_for_backward(h_all, wt, ws, attn, te, u)
        ctx.BH = (B, H)
        attn = attn.view(*lead, H)
        ctx.mark_non_differentiable(attn)
        if with_t:
            return weighted.view(*lead, 256), attn, h_all[..., 0, :].contiguous()
        return weighted.view(*lead, 256), attn

    @staticmethod
    def backward(ctx, d_weighted, _d_attn, d_t=None):
        h_all, wt, ws, attn, te, u = ctx.saved_tensors
        B, H = ctx.BH
        dev = h_all.device
        d_weighted = d_weighted.contiguous() if d_weighted is not None else torch.zeros(B, 256, device=dev)
        d_h_all = torch.empty_like(h_all)
        d_u, d_te = torch.empty(B, 256, device=dev), torch.empty(B, 64, device=dev)
        d_t = None if d_t is None else d_t.contiguous()
        A.call("cn_srnn_attn_bwd", B, H, A.ptr(h_all), A.ptr(wt), A.ptr(ws), A.ptr(attn), A.ptr(u), A.ptr(d_weighted), A.ptr(d_t), A.ptr(d_h_all), A.ptr(d_u),
               A.ptr(d_te), A.stream_ptr(), device=dev)
        d_ws = _wgrad_ld(te, 64, d_u, 256, B, 64, 256, bias=False)[0]            # dWs = te^T d_u
        d_wt, d_bt = _wgrad_ld(d_te, 64, h_all, (H + 1) * 256, B, 64, 256)        # dWt = d_te^T t (t in place: row stride (H+1) * 256), dbt
        return d_h_all, d_wt, d_bt, d_ws, torch.zeros(64, device=dev), None


def _wgrad_ld(dy, ldy, x, ldx, M, N, K, bias=True):
    """(dy^T x [N,K], column sums of dy [N] or None) over M rows of two row-major buffers with the given row strides (cn_linear_wgrad)."""
    splits = A.lib().cn_linear_wgrad_splits(M, N, K)
    if splits <= 0:
        raise A.CnError("cn_linear_wgrad: no split-K plan for a %d x %d weight gradient over %d rows" % (N, K, M))
    part = torch.empty(splits, N, K, device=x.device)
    dw = torch.empty(N, K, device=x.device)
    dbp, db = (torch.empty(splits, N, device=x.device), torch.empty(N, device=x.device)) if bias else (None, None)
    A.call("cn_linear_wgrad", M, N, K, A.ptr(dy), ldy, None, A.ptr(x), ldx, splits, A.ptr(part), A.ptr(dbp), A.ptr(dw), A.ptr(db), A.stream_ptr(),
           device=x.device)
    return dw, db


class HHAttention(torch.autograd.Function):
    """softmax(scale * q k^T) v per (sample, head) on compacted rows, forward and backward as HIP kernels
    (cn_hh_attention_fwd / cn_hh_attention_bwd).  qkv [R,1536] float32 cuda, row_off [B+1] int32 cuda."""

    @staticmethod
    def forward(ctx, qkv, row_off, B, H, scale):
        qkv = qkv.contiguous()
        out = torch.empty(qkv.shape[0], 512, device=qkv.device)
        cls = torch.empty(int(A.lib().cn_hh_attention_workspace_ints(int(B))), dtype=torch.int32, device=qkv.device)   # size-class lists
        A.call("cn_hh_attention_fwd", int(B), int(H), A.ptr(qkv), A.ptr(row_off), float(scale), A.ptr(out), A.ptr(cls), A.stream_ptr())
        ctx.save_for_backward(qkv, row_off, cls)
        ctx.meta = (int(B), int(H), float(scale))
        return out

    @staticmethod
    def backward(ctx, d_out):
        qkv, row_off, cls = ctx.saved_tensors
        B, H, scale = ctx.meta
        d_qkv = torch.empty_like(qkv)
        A.call("cn_hh_attention_bwd", B, H, A.ptr(qkv), A.ptr(row_off), A.ptr(d_out.contiguous()), scale, A.ptr(d_qkv), A.ptr(cls), 1,
               A.stream_ptr())
        return d_qkv, None, None, None, None


class HRAttention(torch.autograd.Function):
    """Robot-human attention on compacted rows (cn_hr_attention_fwd / cn_hr_attention_bwd): u [B,256] = Ws^T t (the
    spatial_edge_layer projection moved to the robot side, see include/crowdnav_hip.h), o [R,256], row_off [B+1] int32
    -> hr [B,256]."""

    @staticmethod
    def forward(ctx, u, o, row_off, H):
        u, o = u.contiguous(), o.contiguous()
        B = u.shape[0]
        hr = torch.empty(B, 256, device=u.device)
        attn = torch.empty(B, H, device=u.device)
        A.call("cn_hr_attention_fwd", B, int(H), A.ptr(u), A.ptr(o), A.ptr(row_off), A.ptr(hr), A.ptr(attn), A.stream_ptr())
        ctx.save_for_backward(u, o, row_off, attn)
        ctx.H = int(H)
        return hr

    @staticmethod
    def backward(ctx, d_hr):
        u, o, row_off, attn = ctx.saved_tensors
        d_u, d_o = torch.empty_like(u), torch.empty_like(o)
        A.call("cn_hr_attention_bwd", u.shape[0], ctx.H, A.ptr(u), A.ptr(o), A.ptr(row_off), A.ptr(attn), A.ptr(d_hr.contiguous()), A.ptr(d_u), A.ptr(d_o),
               A.stream_ptr())
        return d_u, d_o, None, None


class GRUSequence(torch.autograd.Function):
    """The human-node GRU over a [T,N] rollout slice with the done mask applied to h before every step (the reference's
    split-at-done trick, rl/networks/srnn_model.py:52-104, is arithmetically this).  gi [T,N,384] = x W_ih^T + b_ih,
    h0 [N,128], m [T,N,1] -> hs [T,N,128].  ONE launch for the whole forward sequence and one for the backward
    (cn_gru_seq_fwd / cn_gru_seq_bwd: W_hh resident in registers as bf16 hi / lo fragments, bf16x3 MFMA); the weight gradient of W_hh is one
    product over all T*N rows at the end."""

    @staticmethod
    def forward(ctx, gi, h0, m, w_hh, b_hh):
        T, N = gi.shape[0], gi.shape[1]
        gi, h0, m = gi.contiguous(), h0.contiguous(), m.contiguous()
        w, b = w_hh.detach().contiguous(), b_hh.detach().contiguous()
        hs = torch.empty(T, N, 128, device=gi.device)
        hms = torch.empty(T, N, 128, device=gi.device)
        gates = torch.empty(T, N, 512, device=gi.device)
        A.call("cn_gru_seq_fwd", T, N, A.ptr(gi), A.ptr(h0), A.ptr(m), A.ptr(w), A.ptr(b), A.ptr(hs), A.ptr(hms), A.ptr(gates), A.stream_ptr())
        ctx.save_for_backward(hms, gates, m, w)
        return hs

    @staticmethod
    def backward(ctx, d_hs):
        hms, gates, m, w = ctx.saved_tensors
        T, N = hms.shape[0], hms.shape[1]
        d_hs = d_hs.contiguous()
        dgi = torch.empty(T, N, 384, device=hms.device)
        dgh = torch.empty(T, N, 384, device=hms.device)
        dh0 = torch.empty(N, 128, device=hms.device)
        A.call("cn_gru_seq_bwd", T, N, A.ptr(gates), A.ptr(hms), A.ptr(m), A.ptr(w), A.ptr(d_hs), A.ptr(dgi), A.ptr(dgh), A.ptr(dh0), A.stream_ptr())
        # d(W_hh) = d(gh)^T hms and d(b_hh) = column sums of d(gh): a reduction over all T*N rows into a 384 x 128 matrix, which the
        # library product leaves on a dozen workgroups (287 us) -- the split-K weight-gradient kernel does both in one pass
        dw, db = wgrad(dgh.view(T * N, 384), hms.view(T * N, 128))
        return dgi, dh0, None, dw, db


def split_bf16(w, transpose=False):
    """fp32 matrix -> (hi, lo) bf16 planes (int16 storage) of w, or of w^T when transpose is set."""
    w = w.contiguous()
    rows, cols = w.shape
    shape = (cols, rows) if transpose else (rows, cols)
    hi = torch.empty(shape, dtype=torch.int16, device=w.device)
    lo = torch.empty(shape, dtype=torch.int16, device=w.device)
    A.call("cn_split_bf16", A.ptr(w), rows, cols, int(bool(transpose)), A.ptr(hi), A.ptr(lo), A.stream_ptr())
    return hi, lo


def linear_act(x, w, b, act, aux=None, relu_from=None, pad_to=0):
    """act(x w^T + b) on the split-precision kernel with the robot-node sequence's epilogues (cn_linear_fwd_act): act 0 none, 1 ReLU, 2 tanh,
    3 = times [aux > 0], 4 = times (1 - aux^2); columns >= relu_from also get a ReLU; pad_to = the weight's row count padded with zero rows
    to a multiple of 128 (the result then has pad_to columns).  x [M,K] (row stride may exceed K), w [N,K]."""
    M, K = x.shape
    N = w.shape[0]
    Np = pad_to or N

    def rows_ptr(t):   # a column slice of a wider row-major buffer: unit column stride, any row stride
        if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or t.dtype != torch.float32:
            raise A.CnError("linear_act: operands must be fp32 GPU matrices with unit column stride")
        return C.c_void_p(t.data_ptr())
    w = w.detach().contiguous()
    hi = torch.empty(Np, K, dtype=torch.int16, device=x.device)
    lo = torch.empty(Np, K, dtype=torch.int16, device=x.device)
    A.call("cn_split_bf16_padded", A.ptr(w), N, K, 0, Np if pad_to else 0, A.ptr(hi), A.ptr(lo), A.stream_ptr())
    bias = None
    if b is not None:
        bias = torch.zeros(Np, device=x.device)
        bias[:N] = b.detach()
    y = torch.empty(M, Np, device=x.device)
    A.call("cn_linear_fwd_act", M, Np, K, rows_ptr(x), x.stride(0), A.ptr(hi), A.ptr(lo), A.ptr(bias) if bias is not None else None, int(act),
           rows_ptr(aux) if aux is not None else None, aux.stride(0) if aux is not None else 0,
           int(relu_from) if relu_from is not None else 1 << 30, A.ptr(y), Np, A.stream_ptr())
    return y


def linear_supported(x, w):
    """Shapes the split-precision training kernels cover (the three large human-human Linear layers)."""
    N, K = w.shape
    return x.is_cuda and x.dtype == torch.float32 and N % 128 == 0 and K % 128 == 0


class Embed0(torch.autograd.Function):
    """relu(x w^T + b) for the D -> 128 input embedding of the human-human block (cn_embed0_fwd / cn_embed0_bwd)."""

    @staticmethod
    def forward(ctx, x, w, b):
        x = x.contiguous()
        R, D = x.shape
        y = torch.empty(R, 128, device=x.device)
        if R:
            A.call("cn_embed0_fwd", R, D, A.ptr(x), A.ptr(w.detach().contiguous()), A.ptr(b.detach().contiguous()), A.ptr(y), A.stream_ptr())
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        R, D = x.shape
        if R == 0:
            return None, x.new_zeros(128, D), x.new_zeros(128)
        # 16 resident blocks of 128 threads per CU: each walks its rows 8 at a time (one round trip per trip)
        blocks = min(R, 4096)   # (a new cap: move tests/test_gpu_strided_grids.py, which runs past twice 8 x this one)
        part = torch.empty(blocks, 128, D + 1, device=x.device)
        dwb = torch.empty(128, D + 1, device=x.device)
        A.call("cn_embed0_bwd", R, D, A.ptr(x), A.ptr(y), A.ptr(dy.contiguous()), blocks, A.ptr(part), A.ptr(dwb), A.stream_ptr())
        return None, dwb[:, :D].contiguous(), dwb[:, D].contiguous()


def wgrad(dy, x, gate=None, required=False):
    """((dy * [gate > 0])^T x [N,K], column sums of dy * [gate > 0] [N]) over all M rows on the split-K TN kernel (cn_linear_wgrad); N % 64 == 0,
    K % 64 == 0.  `gate` = the ReLU output whose backward is applied while dy is loaded (None: no gate).  A shape the kernel has no plan for goes to
    torch, unless the caller has checked the shape beforehand (`required`): then it is an error."""
    dy, x = dy.contiguous(), x.contiguous()
    M, N = dy.shape
    K = x.shape[1]
    splits = A.lib().cn_linear_wgrad_splits(M, N, K)
    if splits <= 0:
        if required:
            raise A.CnError("cn_linear_wgrad: no split-K plan for a %d x %d weight gradient over %d rows" % (N, K, M))
        if gate is not None:
            dy = dy * (gate > 0)
        return dy.t() @ x, dy.sum(0)
    part = torch.empty(splits, N, K, device=x.device)
    dbp = torch.empty(splits, N, device=x.device)
    dw = torch.empty(N, K, device=x.device)
    db = torch.empty(N, device=x.device)
    A.call("cn_linear_wgrad", M, N, K, A.ptr(dy), N, None if gate is None else A.ptr(gate), A.ptr(x), K, splits, A.ptr(part), A.ptr(dbp), A.ptr(dw), A.ptr(db),
           A.stream_ptr())
    return dw, db


def _small_mm(a, b):
    """a [M,K] @ b [K,N] (any strides, fp32, on the GPU) through cn_small_mm -> contiguous [M,N]."""
    M, K = a.shape
    K2, N = b.shape
    assert K == K2
    if not (a.is_cuda and b.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32):
        raise A.CnError("cn_small_mm: float32 tensors on the GPU expected")
    out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    # (raw pointers + element strides: the operands are views -- transposes, row slices of in_proj_weight -- by design)
    A.call("cn_small_mm", M, N, K, C.c_void_p(a.data_ptr()), a.stride(0), a.stride(1), C.c_void_p(b.data_ptr()), b.stride(0), b.stride(1),
           A.ptr(out), A.stream_ptr(), device=a.device)
    return out


class SmallMM(torch.autograd.Function):
    """a @ b for WEIGHT-sized operands (the affine folds of the update and their backward): forward and both gradients are cn_small_mm
    launches -- transposes are strides, a vector operand is an [n, 1] matrix.  Replaces the library's GEMM / GEMV kernels on the training path."""

    @staticmethod
    def forward(ctx, a, b):
        vec = b.dim() == 1
        b2 = b.unsqueeze(1) if vec else b
        a32, b32 = a.detach().float(), b2.detach().float()
        ctx.save_for_backward(a32, b32)
        ctx.vec = vec
        out = _small_mm(a32, b32)
        return out.squeeze(1) if vec else out

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        dc = (dc.unsqueeze(1) if ctx.vec else dc).float()
        da = _small_mm(dc, b.t()) if ctx.needs_input_grad[0] else None
        db = _small_mm(a.t(), dc) if ctx.needs_input_grad[1] else None
        if db is not None and ctx.vec:
            db = db.squeeze(1)
        return da, db


def weight_mm(a, b):
    """a @ b between parameters / their slices: cn_small_mm on the GPU (fp32), torch on the CPU."""
    if a.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32:
        return SmallMM.apply(a, b)
    return a @ b


class RightMatmul(torch.autograd.Function):
    """t @ w for a tall t [M,N] and a small w [N,K]: the weight gradient t^T d(out) (a reduction over all M rows) on the split-K
    TN kernel; forward and d(t) are ordinary library products."""

    @staticmethod
    def forward(ctx, t, w):
        ctx.save_for_backward(t, w)
        return t @ w

    @staticmethod
    def backward(ctx, du):
        t, w = ctx.saved_tensors
        dt = du @ w.t() if ctx.needs_input_grad[0] else None
        dw = wgrad(t, du)[0] if ctx.needs_input_grad[1] else None
        return dt, dw


def wgrad_supported(x, w):
    N, K = w.shape
    return x.is_cuda and x.dtype == torch.float32 and N % 64 == 0 and K % 128 == 0


class WgradLinear(torch.autograd.Function):
    """y = x w^T + b for the per-sample layers (a few hundred output columns, tens of thousands of rows): forward and input
    gradient are ordinary library products; the weight/bias gradient, a reduction over all rows into a tiny matrix that the
    BLAS heuristics leave on a handful of workgroups, runs on the split-K TN kernel (cn_linear_wgrad)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return torch.addmm(b, x, w.t())

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dy @ w if ctx.needs_input_grad[0] else None
        dw, db = wgrad(dy, x, required=True)
        return dx, dw, db


class HipLinear(torch.autograd.Function):
    """y = [relu](x w^T + b) with forward, input gradient and weight/bias gradient on the bf16x3 MFMA kernels
    (cn_linear_fwd / cn_linear_wgrad).  x [M,K], w [N,K], b [N]; N, K multiples of 128."""

    @staticmethod
    def forward(ctx, x, w, b, relu):
        x = x.contiguous()
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(M, N, device=x.device)
        if M:
            hi, lo = split_bf16(w.detach())
            A.call("cn_linear_fwd", M, N, K, A.ptr(x), K, None, A.ptr(hi), A.ptr(lo), A.ptr(b.detach().contiguous()), int(bool(relu)), A.ptr(y), N,
                   A.stream_ptr())
        ctx.save_for_backward(x, w, y if relu else None)
        ctx.relu = bool(relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        M, K = x.shape
        N = w.shape[0]
        dy = dy.contiguous()
        gate = y if ctx.relu else None                 # ReLU backward is applied while dY is loaded (no masking pass)
        dx = dw = db = None
        if M == 0:
            return torch.zeros_like(x), torch.zeros_like(w), x.new_zeros(N), None
        if ctx.needs_input_grad[0]:
            hi_t, lo_t = split_bf16(w.detach(), transpose=True)              # [K,N]: dX = dY W as an NT product with W^T
            dx = torch.empty(M, K, device=x.device)
            A.call("cn_linear_fwd", M, K, N, A.ptr(dy), N, None if gate is None else A.ptr(gate), A.ptr(hi_t), A.ptr(lo_t), None, 0, A.ptr(dx), K,
                   A.stream_ptr())
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = wgrad(dy, x, gate, required=True)
        return dx, dw, db, None


class HHBlockFused(torch.autograd.Function):
    """The whole human-human block of evaluate_actions (embedding_layer -> folded q|k|v -> 8-head attention -> folded
    out_proj∘spatial_linear) on the compacted live rows: forward = ONE launch of the rollout's fused kernel on the training weights
    (cn_hh_block_fwd), which writes every activation the backward needs exactly once; backward = the per-layer kernels of HipLinear /
    HHAttention / Embed0 on those activations, in reverse order.  spatial_edges [B,H,D], x_live [R,D] (its live rows, for the input
    layer's weight gradient), row_off [B+1] int32; weights as the mirror composes them (qkv / os folded, q unscaled)."""

    @staticmethod
    def forward(ctx, spatial_edges, x_live, row_off, emb0_w, emb0_b, emb2_w, emb2_b, qkv_w, qkv_b, os_w, os_b):
        B, H, D = spatial_edges.shape
        R = x_live.shape[0]
        dev = spatial_edges.device
        se = spatial_edges.contiguous()
        ws = torch.empty(int(A.lib().cn_hh_block_workspace_bytes()), dtype=torch.uint8, device=dev)
        e0, x, qkv = torch.empty(R, 128, device=dev), torch.empty(R, 512, device=dev), torch.empty(R, 1536, device=dev)
        attn, out = torch.empty(R, 512, device=dev), torch.empty(R, 256, device=dev)
        ws_w = [t.detach().contiguous() for t in (emb0_w, emb0_b, emb2_w, emb2_b, qkv_w, qkv_b, os_w, os_b)]
        A.call("cn_hh_block_fwd", B, H, D, A.ptr(se), A.ptr(row_off), *[A.ptr(t) for t in ws_w], 0.125, A.ptr(ws), A.ptr(e0), A.ptr(x), A.ptr(qkv),
               A.ptr(attn), A.ptr(out), A.stream_ptr())
        ctx.save_for_backward(x_live, row_off, e0, x, qkv, attn, out, emb2_w, qkv_w, os_w)
        ctx.meta = (B, H, D)
        return out

    @staticmethod
    def backward(ctx, d_out):
        x_live, row_off, e0, x, qkv, attn, out, emb2_w, qkv_w, os_w = ctx.saved_tensors
        B, H, D = ctx.meta
        R = x_live.shape[0]
        L = A.lib()
        dev = d_out.device

        def layer_bwd(dy, gate, w, inp):
            """Linear (+ReLU when `gate` = its output) backward: dX = (dY * [gate > 0]) W, dW = (dY * [gate > 0])^T X, db = column sums."""
            M, N = dy.shape
            K = w.shape[1]
            g = A.ptr(gate) if gate is not None else None
            hi_t, lo_t = split_bf16(w.detach(), transpose=True)
            dx = torch.empty(M, K, device=dev)
            A.call("cn_linear_fwd", M, K, N, A.ptr(dy), N, g, A.ptr(hi_t), A.ptr(lo_t), None, 0, A.ptr(dx), K, A.stream_ptr())
            dw, db = wgrad(dy, inp, gate, required=True)
            return dx, dw, db

        d_out = d_out.contiguous()
        if R == 0:
            z = lambda t: torch.zeros_like(t)   # noqa: E731
            return (None, None, None, x_live.new_zeros(128, D), x_live.new_zeros(128), z(emb2_w), x_live.new_zeros(512), z(qkv_w), x_live.new_zeros(1536),
                    z(os_w), x_live.new_zeros(256))
        d_attn, d_os_w, d_os_b = layer_bwd(d_out, out, os_w, attn)                       # out = relu(attn Wos^T + b)
        d_qkv = torch.empty_like(qkv)
        cls = torch.empty(int(L.cn_hh_attention_workspace_ints(int(B))), dtype=torch.int32, device=dev)
        A.call("cn_hh_attention_bwd", B, H, A.ptr(qkv), A.ptr(row_off), A.ptr(d_attn), 0.125, A.ptr(d_qkv), A.ptr(cls), 0, A.stream_ptr())
        d_x, d_qkv_w, d_qkv_b = layer_bwd(d_qkv, None, qkv_w, x)                         # qkv = x Wc^T + bc
        d_e0, d_emb2_w, d_emb2_b = layer_bwd(d_x, x, emb2_w, e0)                         # x = relu(e0 W2^T + b2)
        blocks = min(R, 4096)   # (as in Embed0.backward; a new cap: move tests/test_gpu_strided_grids.py)
        part = torch.empty(blocks, 128, D + 1, device=dev)
        dwb = torch.empty(128, D + 1, device=dev)
        A.call("cn_embed0_bwd", R, D, A.ptr(x_live), A.ptr(e0), A.ptr(d_e0), blocks, A.ptr(part), A.ptr(dwb), A.stream_ptr())
        return (None, None, None, dwb[:, :D].contiguous(), dwb[:, D].contiguous(), d_emb2_w, d_emb2_b, d_qkv_w, d_qkv_b, d_os_w, d_os_b)


class RnSequence(torch.autograd.Function):
    """Everything behind the human-human block in evaluate_actions for a [T, N] rollout slice -- robot_linear, [u | encoder_linear], robot-human
    attention, edge_attention_embed, the GRU over the T steps with the done mask, the actor / critic trunks, critic_linear and the log-probability
    of the given actions -- as ONE call forward (cn_rn_seq_fwd_sized) and ONE backward (cn_rn_seq_bwd_sized).  robot_node [B,7], temporal [B,2],
    out_sp [rows,256] (compacted rows of the human-human block), row_off [B+1] int32, h0 [N,R], masks [B], actions [B,2]; weights in the order of
    _abi.RN_WEIGHT_FIELDS as the mirror composes them (te = [Ws^T Wt ; encoder_linear], ac0 = (actor.0 ; critic.0) o output_linear).
    The network sizes (R, M, O) are read off the weight shapes (whh [3R,R], edge_w [M,256], a2_w [O,O]) and must lie in the device box
    (_abi.DIMS_BOX); the attention size A, which no shape carries, comes with H: pass H = (human_num, attention_size), or a plain int for the
    reference's 64.  Returns value [B,1], logp [B,1] and the final hidden state [N,R] (not differentiable)."""

    @staticmethod
    def dims_of(weights, attention_size=64):
        """cn_policy_dims of a weight list in _abi.RN_WEIGHT_FIELDS order, checked against the box and against every other shape."""
        idx = {n: i for i, n in enumerate(A.RN_WEIGHT_FIELDS)}
        try:
            dims = A.policy_dims((int(weights[idx["whh"]].shape[1]), int(weights[idx["edge_w"]].shape[0]), int(attention_size), int(weights[idx["a2_w"]].shape[0])))
        except NotImplementedError as e:
            raise A.CnError("RnSequence: %s" % e)
        for w, shp, name in zip(weights, A.rn_weight_shapes(dims), A.RN_WEIGHT_FIELDS):
            if tuple(w.shape) != shp:
                raise A.CnError("RnSequence: weight %s has shape %s, expected %s at sizes %s" % (name, tuple(w.shape), shp, dims.astuple()))
        return dims

    @staticmethod
    def forward(ctx, robot_node, temporal, out_sp, row_off, h0, masks, actions, T, N, H, *weights):
        B, dev = T * N, out_sp.device
        H, attention_size = H if isinstance(H, (tuple, list)) else (H, 64)
        f = lambda t: t.detach().to(torch.float32).contiguous()   # noqa: E731
        ws = [f(w) for w in weights]
        dims = RnSequence.dims_of(ws, attention_size)
        rn, te, osp, h0c, m, act = f(robot_node).view(B, 7), f(temporal).view(B, 2), f(out_sp), f(h0).view(N, dims.rnn_size), f(masks).view(B), f(actions).view(B, 2)
        wst = A.RnWeights(*[w.data_ptr() for w in ws])
        widths = A.rn_saved_widths(dims, H)
        saved = {k: torch.empty(B, widths[k], device=dev) for k in A.RN_SAVED_FIELDS}
        sst = A.RnSaved(*[saved[k].data_ptr() for k in A.RN_SAVED_FIELDS])
        value, logp = torch.empty(B, 1, device=dev), torch.empty(B, 1, device=dev)
        work = torch.empty(int(A.lib().cn_rn_seq_fwd_workspace_floats_sized(C.byref(dims))), device=dev)
        A.call("cn_rn_seq_fwd_sized", T, N, H, A.ptr(rn), A.ptr(te), A.ptr(osp), A.ptr(row_off), A.ptr(h0c), A.ptr(m), A.ptr(act), C.byref(wst), C.byref(sst),
               A.ptr(work), A.ptr(value), A.ptr(logp), C.byref(dims), A.stream_ptr())
        ctx.save_for_backward(rn, te, osp, row_off, m, act, *ws, *[saved[k] for k in A.RN_SAVED_FIELDS])
        ctx.meta = (T, N, H, len(ws), dims.astuple())
        h_last = saved["hs"][(T - 1) * N:].clone()
        ctx.mark_non_differentiable(h_last)
        return value, logp, h_last

    @staticmethod
    def backward(ctx, d_value, d_logp, _d_h):
        T, N, H, nw, dims = ctx.meta
        dims = A.PolicyDims(*dims)
        t = ctx.saved_tensors
        rn, te, osp, row_off, m, act = t[:6]
        ws, sv = t[6:6 + nw], t[6 + nw:]
        B, dev = T * N, osp.device
        wst = A.RnWeights(*[w.data_ptr() for w in ws])
        sst = A.RnSaved(*[x.data_ptr() for x in sv])
        grads = [torch.empty_like(w) for w in ws]
        gst = A.RnWeights(*[g.data_ptr() for g in grads])
        work = torch.empty(int(A.lib().cn_rn_seq_workspace_floats_sized(T, N, C.byref(dims))), device=dev)
        d_osp, d_h0 = torch.empty_like(osp), torch.empty(N, dims.rnn_size, device=dev)
        dv = d_value.reshape(B).to(torch.float32).contiguous()
        dl = d_logp.reshape(B).to(torch.float32).contiguous()
        A.call("cn_rn_seq_bwd_sized", T, N, H, A.ptr(rn), A.ptr(te), A.ptr(osp), A.ptr(row_off), A.ptr(m), A.ptr(act), C.byref(wst), C.byref(sst), A.ptr(dv), A.ptr(dl),
               A.ptr(work), A.ptr(d_osp), A.ptr(d_h0), C.byref(gst), C.byref(dims), A.stream_ptr())
        return (None, None, d_osp, None, None, None, None, None, None, None, *grads)


class PPOLoss(torch.autograd.Function):
    """(value_loss, action_loss) of rl/ppo/ppo.py:66-84 as one tensor [2]: forward = cn_ppo_loss_fwd, backward =
    cn_ppo_loss_bwd (gradients w.r.t. `values` and `logp` only -- everything else is rollout data)."""

    @staticmethod
    def forward(ctx, values, logp, old_logp, adv, value_preds, returns, clip_param, use_clipped_value_loss):
        ts = [t.reshape(-1).contiguous() for t in (values, logp, old_logp, adv, value_preds, returns)]
        n = ts[0].numel()
        if any(t.numel() != n or t.dtype != torch.float32 for t in ts):
            raise A.CnError("PPOLoss: all inputs must be float32 tensors of the same number of elements")
        ws = torch.empty(A.lib().cn_ppo_loss_workspace_doubles(), dtype=torch.float64, device=ts[0].device)
        losses = torch.empty(2, device=ts[0].device)
        A.call("cn_ppo_loss_fwd", n, *[A.ptr(t) for t in ts], float(clip_param), int(bool(use_clipped_value_loss)), A.ptr(ws), A.ptr(losses),
               A.stream_ptr())
        ctx.save_for_backward(*ts)
        ctx.meta = (n, float(clip_param), int(bool(use_clipped_value_loss)), values.shape, logp.shape)
        return losses

    @staticmethod
    def backward(ctx, g):
        ts = ctx.saved_tensors
        n, clip, ucv, vshape, lshape = ctx.meta
        dv, dlp = torch.empty(n, device=g.device), torch.empty(n, device=g.device)
        A.call("cn_ppo_loss_bwd", n, *[A.ptr(t) for t in ts], clip, ucv, A.ptr(g.contiguous()), A.ptr(dv), A.ptr(dlp), A.stream_ptr())
        return dv.view(vshape), dlp.view(lshape), None, None, None, None, None, None


def adam_clip_step(param, grad, exp_avg, exp_avg_sq, step, lr, betas, eps, max_grad_norm, grad_scale=1.0, workspace=None, norm_out=None):
    """nn.utils.clip_grad_norm_ + torch.optim.Adam.step over one flat fp32 bucket (cn_adam_clip_step), in place."""
    n = param.numel()
    if workspace is None:
        workspace = torch.empty(A.lib().cn_adam_workspace_doubles(), dtype=torch.float64, device=param.device)
    A.call("cn_adam_clip_step", n, A.ptr(param), A.ptr(grad), A.ptr(exp_avg), A.ptr(exp_avg_sq), float(grad_scale),
           float(max_grad_norm if max_grad_norm is not None else 0.0), float(lr), float(betas[0]), float(betas[1]),
           float(eps), int(step), A.ptr(workspace), A.ptr(norm_out), A.stream_ptr())


def gae(rewards, values, masks, gamma, lam, returns):
    """rewards [T,N,1], values/masks/returns [T+1,N,1] contiguous float32 device tensors; fills returns[:T]."""
    T, N = rewards.shape[0], rewards.shape[1]
    A.call("cn_gae", T, N, A.ptr(rewards), A.ptr(values), A.ptr(masks), float(gamma), float(lam), A.ptr(returns), A.stream_ptr())
    return returns


def adv_stats(returns, values, n):
    stats = torch.zeros(3, dtype=torch.float64, device=returns.device)
    A.call("cn_adv_stats", int(n), A.ptr(returns), A.ptr(values), A.ptr(stats), A.stream_ptr())
    return stats


def adv_normalize(returns, values, stats, n, out):
    A.call("cn_adv_normalize", int(n), A.ptr(returns), A.ptr(values), A.ptr(stats), A.ptr(out), A.stream_ptr())
    return out


class MinibatchStepper:
    """One PPO minibatch -- gather from the rollout storage, train-mode forward, losses, backward, every parameter gradient written into the
    caller's flat bucket -- as ONE boundary call (cn_ppo_minibatch_step; rl/networks/storage.py:184-253 + rl/networks/model.py:82-90 +
    rl/ppo/ppo.py:66-88).  Built by ppo.PPO for the default network sizes (SizedMinibatchStepper below: every sizes tuple of the device box); the
    workspace is one cached byte tensor that grows with the row count.  The two switches of the network, base.use_self_attn and
    base.sort_humans, travel as cn_ppo_variant (cn_ppo_minibatch_step_variant); with both on, the calls are the ones without a variant."""

    def __init__(self, policy):
        self.policy = policy
        self._ws = None
        self._ptrs = None
        base = policy.base
        self.self_attn, self.sort_humans = bool(getattr(base, "use_self_attn", True)), bool(getattr(base, "sort_humans", True))
        # (field of cn_policy_weights, parameter name): the table the rollout handle sets its weights by (use_self_attn off: the remap)
        self.weight_keys = A.policy_weight_keys(self.self_attn)
        # Parameters the call does not write: only the ones the loss never reaches (the reference leaves their .grad None).  Their slices of
        # the flat bucket still enter the all-reduce, the clip norm and Adam, so the caller keeps them zero (ppo.PPO._minibatch_step_producer); any
        # OTHER parameter outside cn_policy_weights would silently train on a stale gradient, hence the refusal here.
        covered = {k for _, k in self.weight_keys}
        self.uncovered = [name for name, p in policy.named_parameters() if p.requires_grad and name not in covered]
        stray = [name for name in self.uncovered if not name.startswith("base.human_node_final_linear.")]
        if stray:
            raise A.CnError("MinibatchStepper: cn_ppo_minibatch_step writes no gradient for %s" % ", ".join(stray))

    @staticmethod
    def max_rows():
        """The most compacted rows one call takes (cn_ppo_minibatch_max_rows: host-only, the bound the C call itself enforces)."""
        return int(A.lib().cn_ppo_minibatch_max_rows())

    @staticmethod
    def supported(policy, rollouts):
        """The default sizes only (base.fused_rn_shapes_ok()); SizedMinibatchStepper.supported covers the device box."""
        return MinibatchStepper._supported(policy, rollouts, lambda base: base.fused_rn_shapes_ok())

    @staticmethod
    def _supported(policy, rollouts, shapes_ok):
        base = policy.base
        if getattr(policy, "is_srnn_baseline", False):      # DS-RNN: cn_ppo_minibatch_step knows the attention-graph network only
            return False
        if not (base.train_gemm_mode == "bf16x3" and base.train_fused_hh and base.train_fused_rn
                and shapes_ok(base) and base.human_num <= 48 and base.edge_width <= 16):
            return False
        if base.use_self_attn:
            if tuple(base.spatial_attn.embedding_layer[0].weight.shape) != (128, base.edge_width):
                return False
        elif (tuple(base.spatial_linear[0].weight.shape) != (128, base.edge_width) or tuple(base.spatial_linear[2].weight.shape) != (256, 128)):
            return False                                    # use_self_attn off: spatial_linear is the two-layer MLP the step runs
        if not base.sort_humans:                            # the gather compacts by the storage's visibility bytes
            vm = rollouts.obs.get("visible_masks")
            if vm is None or not (vm.is_cuda and vm.dtype == torch.bool and vm.is_contiguous()):
                return False
        need = ("robot_node", "temporal_edges", "spatial_edges", "detected_human_num")
        ts = [rollouts.obs.get(k) for k in need] + [rollouts.recurrent_hidden_states["human_node_rnn"], rollouts.masks, rollouts.actions,
                                                    rollouts.value_preds, rollouts.returns, rollouts.action_log_probs]
        return all(t is not None and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in ts)

    def _structs(self):
        """Parameter / gradient pointer structs (views of the flat buckets ppo.PPO binds; re-read whenever a pointer moved)."""
        named = dict(self.policy.named_parameters())
        key = tuple((named[k].data_ptr(), named[k].grad.data_ptr()) for _, k in self.weight_keys)
        if self._ptrs is None or self._ptrs[0] != key:
            w, g = A.PolicyWeights(), A.PolicyWeights()     # use_self_attn off: the fields of the layers that do not exist stay NULL
            for field, k in self.weight_keys:
                p = named[k]
                if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() or p.grad is None:
                    raise A.CnError("MinibatchStepper: parameter %s must be a contiguous float32 GPU tensor with a bound gradient" % k)
                setattr(w, field, p.data_ptr())
                setattr(g, field, p.grad.data_ptr())
            self._ptrs = (key, w, g)
        return self._ptrs[1], self._ptrs[2]

    def row_totals(self, rollouts):
        """[E] int64 on the HOST: the compacted rows every env contributes to a minibatch (one readback per update())."""
        det = rollouts.obs["detected_human_num"]
        T, E = rollouts.rewards.shape[0], rollouts.rewards.shape[1]
        tot = torch.empty(E, dtype=torch.int32, device=det.device)
        if self.sort_humans:
            A.call("cn_ppo_row_totals", T, E, self.policy.base.human_num, A.ptr(det), A.ptr(tot), A.stream_ptr(), device=det.device)
        else:                                               # sort_humans off: max(1, visible) per sample, from the visibility bytes
            A.call("cn_ppo_row_totals_visible", T, E, self.policy.base.human_num, A.ptr(self._visible(rollouts)), A.ptr(tot), A.stream_ptr(), device=det.device)
        return tot.cpu().to(torch.int64)

    def _visible(self, rollouts):
        vm = rollouts.obs.get("visible_masks")
        if vm is None or not (vm.is_cuda and vm.dtype == torch.bool and vm.is_contiguous()):
            raise A.CnError("MinibatchStepper: sort_humans = False needs rollouts.obs['visible_masks'] as a contiguous bool GPU tensor")
        return vm

    def _variant(self, rollouts):
        """cn_ppo_variant of this policy on this storage, or None for the network without a variant (both switches on)."""
        if self.self_attn and self.sort_humans:
            return None
        return A.PpoVariant(int(self.self_attn), int(self.sort_humans), None if self.sort_humans else self._visible(rollouts).data_ptr())

    def step(self, rollouts, advantages, env_idx, rows, hyper, losses_out, value_logp_out=None):
        """env_idx [N] int32 on the device, rows = their row total, hyper = (clip, value_loss_coef, entropy_coef, use_clipped_value_loss),
        losses_out [3] float32 on the device; value_logp_out (optional, tests): [2, T * N] float32 on the device."""
        base = self.policy.base
        T, E = rollouts.rewards.shape[0], rollouts.rewards.shape[1]
        N, H, D = int(env_idx.numel()), base.human_num, base.edge_width
        dev = rollouts.rewards.device
        v = self._variant(rollouts)
        need = self._workspace_bytes(T, N, H, D, int(rows), v)
        if need <= 0:
            raise A.CnError("cn_ppo_minibatch_workspace_bytes: unsupported shape T=%d N=%d H=%d D=%d rows=%d" % (T, N, H, D, rows))
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = None                       # free the old block first: the two do not need to coexist
            self._ws = torch.empty(int(need * 1.1) + 4096, dtype=torch.uint8, device=dev)
        w, g = self._structs()
        b = A.PpoBatch(T, N, E, H, D)
        ts = dict(env_idx=env_idx, robot_node=rollouts.obs["robot_node"], temporal_edges=rollouts.obs["temporal_edges"],
                  spatial_edges=rollouts.obs["spatial_edges"], detected_human_num=rollouts.obs["detected_human_num"],
                  h0=rollouts.recurrent_hidden_states["human_node_rnn"], masks=rollouts.masks, actions=rollouts.actions,
                  value_preds=rollouts.value_preds, returns=rollouts.returns, old_logp=rollouts.action_log_probs, adv=advantages)
        for k in A.PPO_BATCH_TENSORS:
            setattr(b, k, ts[k].data_ptr())
        hy = A.PpoHyper(float(hyper[0]), float(hyper[1]), float(hyper[2]), int(bool(hyper[3])))
        self._call(C.byref(b), int(rows), C.byref(w), C.byref(g), C.byref(hy), C.c_void_p(self._ws.data_ptr()), int(self._ws.numel()),
                   A.ptr(losses_out), A.ptr(value_logp_out), A.stream_ptr(), dev, v)

    # the two boundary calls of step(): what SizedMinibatchStepper replaces.  v: the A.PpoVariant of _variant(), or None
    _dims = None                                            # cn_policy_dims of the variant calls: NULL = the default tuple

    def _workspace_bytes(self, T, N, H, D, rows, v=None):
        if v is not None:
            return int(A.lib().cn_ppo_minibatch_workspace_bytes_variant(T, N, H, D, rows, self._dims, C.byref(v)))
        return int(A.lib().cn_ppo_minibatch_workspace_bytes(T, N, H, D, rows))

    def _call(self, b, rows, w, g, hy, ws, ws_bytes, losses_out, value_logp_out, stream, dev, v=None):
        if v is not None:
            return A.call("cn_ppo_minibatch_step_variant", b, rows, w, g, hy, self._dims, C.byref(v), ws, ws_bytes, losses_out, value_logp_out, stream, device=dev)
        A.call("cn_ppo_minibatch_step", b, rows, w, g, hy, ws, ws_bytes, losses_out, value_logp_out, stream, device=dev)


class SizedMinibatchStepper(MinibatchStepper):
    """MinibatchStepper at the network sizes of policy.base.dims = (R, M, A, O), any tuple inside the device box (_abi.DIMS_BOX):
    cn_ppo_minibatch_workspace_bytes_sized / cn_ppo_minibatch_step_sized.  At the default tuple the C call is cn_ppo_minibatch_step itself."""

    def __init__(self, policy):
        super().__init__(policy)
        try:
            self.dims = A.policy_dims(policy.base.dims)
        except NotImplementedError as e:
            raise A.CnError("SizedMinibatchStepper: %s" % e)
        self._dims = C.byref(self.dims)

    @staticmethod
    def supported(policy, rollouts):
        """An attention-graph policy on GPU tensors whose sizes lie in the device box (base.sized_rn_ok()); otherwise the conditions of
        MinibatchStepper.supported.  False for the DS-RNN baseline."""
        return MinibatchStepper._supported(policy, rollouts, lambda base: base.sized_rn_ok())

    def _workspace_bytes(self, T, N, H, D, rows, v=None):
        if v is not None:
            return super()._workspace_bytes(T, N, H, D, rows, v)
        return int(A.lib().cn_ppo_minibatch_workspace_bytes_sized(T, N, H, D, rows, C.byref(self.dims)))

    def _call(self, b, rows, w, g, hy, ws, ws_bytes, losses_out, value_logp_out, stream, dev, v=None):
        if v is not None:
            return super()._call(b, rows, w, g, hy, ws, ws_bytes, losses_out, value_logp_out, stream, dev, v)
        A.call("cn_ppo_minibatch_step_sized", b, rows, w, g, hy, C.byref(self.dims), ws, ws_bytes, losses_out, value_logp_out, stream, device=dev)
