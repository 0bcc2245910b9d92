"""Host side of the DS-RNN baseline's node-half training path (SRNNBase.train_node_kernels, hip_train.SrnnAttention = cn_srnn_attn_fwd /
cn_srnn_attn_bwd): no GPU needed.  The flag leaves the CPU graph alone bit for bit, the Function refuses CPU tensors by name, the two calls are
in header, library and binding and refuse arguments outside their box before they look for a device, and the backward formulas the kernel
implements -- restated here in fp64 -- are the gradients autograd finds through SRNNBase.attention."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from crowdnav_prediction_attngraph_amd import _abi as A  # noqa: E402
from crowdnav_prediction_attngraph_amd.policy import SRNNBase  # noqa: E402
from tests import srnn_seq_util as Q  # noqa: E402

NEW = ("cn_srnn_attn_fwd", "cn_srnn_attn_bwd")


def test_the_two_calls_are_declared_exported_and_bound():
    lib = A.lib()
    hdr = open(Q.ROOT + "/include/crowdnav_hip.h").read()
    for name in NEW:
        assert name in A.ABI_SYMBOLS and hasattr(lib, name) and ("int %s(" % name) in hdr, name


def test_flag_on_and_off_give_the_same_bits_on_cpu_tensors():
    """value, actor features, both states, log-prob and every gradient: on CPU tensors the flag selects nothing."""
    assert SRNNBase.train_node_kernels is True
    T, N, H, D = shape = (3, 3, 5, 2)
    pol, seq = Q.policy(H, D, N, T), Q.sequence(*shape)
    res = []
    for flag in (True, False):
        p = copy.deepcopy(pol)
        p.base.train_node_kernels = flag
        taps = {}
        with torch.no_grad():
            out = p.base.forward_sequence(seq["obs"], seq["node_h0"], seq["edge_h0"], seq["masks"], T, N, taps=taps)
        # (a copy of edge_h0: on the CPU in fp32 Q.evaluate makes the tensor it is given the leaf, and a second call would add to its .grad)
        v, lp, grads, d_h0 = Q.evaluate(p, dict(seq, edge_h0=seq["edge_h0"].clone()), "cpu", torch.float32)
        assert sorted(taps) == ["actor_feat", "attn", "edge_out", "node_out", "weighted"]
        res.append(list(out) + [taps[k] for k in sorted(taps)] + [v, lp, d_h0] + [g for _, g in sorted(grads.items()) if g is not None])
    assert len(res[0]) == len(res[1]) > 20
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_srnn_attention_refuses_cpu_tensors_by_name():
    from crowdnav_prediction_attngraph_amd.hip_train import SrnnAttention
    h = torch.zeros(2, 4, 256)
    w, b = torch.zeros(64, 256), torch.zeros(64)
    with pytest.raises(A.CnError, match="SrnnAttention: h_all must be a float32 tensor on the GPU"):
        SrnnAttention.apply(h, w, b, w, b)


def test_refusals_come_before_the_device_and_name_the_call():
    """H = 0, H = 65, B = 0 and a NULL operand: CN_ERR_INVALID (-1) naming the call, on a box with or without a GPU (dummy non-null pointers are
    never dereferenced: nothing is launched)."""
    lib = A.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    null = C.c_void_p(0)
    for B, H, first in ((4, 0, p), (4, 65, p), (0, 5, p), (4, 5, null)):
        assert lib.cn_srnn_attn_fwd(B, H, first, p, p, p, p, p, p, p, null) == -1
        assert b"cn_srnn_attn_fwd" in lib.cn_last_error()
        assert lib.cn_srnn_attn_bwd(B, H, first, p, p, p, p, p, null, p, p, p, null) == -1
        assert b"cn_srnn_attn_bwd" in lib.cn_last_error()


def attention_formulas(t, s, Wt, bt, Ws, d_weighted, d_t_direct):
    """The forward and backward of csrc/srnn_node_train.hip in the order the kernels compute them (any float dtype): dict of weighted, attn, te, u,
    d_t (slot 0), d_s (slots 1 .. H), d_u, d_te, dWt, dbt, dWs."""
    H = s.shape[1]
    scale = H / math.sqrt(64.0)
    te = t @ Wt.t() + bt
    u = te @ Ws
    score = (u.unsqueeze(1) * s).sum(-1) * scale
    a = torch.softmax(score, -1)
    weighted = (a.unsqueeze(-1) * s).sum(1)
    dp = (d_weighted.unsqueeze(1) * s).sum(-1)
    dot = (a * dp).sum(-1, keepdim=True)
    d_score = a * (dp - dot)
    d_s = a.unsqueeze(-1) * d_weighted.unsqueeze(1) + scale * d_score.unsqueeze(-1) * u.unsqueeze(1)
    d_u = scale * ((a * dp).unsqueeze(-1) * s).sum(1) - scale * dot * weighted           # = scale * sum_j d_score_j s_j
    d_te = d_u @ Ws.t()
    d_t = d_te @ Wt + (0 if d_t_direct is None else d_t_direct)
    return dict(weighted=weighted, attn=a, te=te, u=u, d_t=d_t, d_s=d_s, d_u=d_u, d_te=d_te, dWt=d_te.t() @ t, dbt=d_te.sum(0), dWs=te.t() @ d_u)


@pytest.mark.parametrize("direct", (False, True))
def test_backward_formulas_are_autograd_through_srnn_attention(direct):
    torch.manual_seed(3)
    base = Q.policy(5, 2, 2, 2).base.double()
    tl, sl = base.attn.temporal_edge_layer[0], base.attn.spatial_edge_layer[0]
    with torch.no_grad():
        sl.bias.uniform_(-0.5, 0.5)                                  # a bias the softmax must not see
    rs = np.random.RandomState(7)
    B, H = 6, 5
    t = torch.from_numpy(rs.uniform(-1, 1, (B, 256))).requires_grad_(True)
    s = torch.from_numpy(rs.uniform(-1, 1, (B, H, 256))).requires_grad_(True)
    dW = torch.from_numpy(rs.uniform(-1, 1, (B, 256)))
    dT = torch.from_numpy(rs.uniform(-1, 1, (B, 256))) if direct else None
    weighted, a = base.attention(t, s)
    loss = (weighted * dW).sum() + ((t * dT).sum() if direct else 0.0)
    params = [tl.weight, tl.bias, sl.weight, sl.bias]
    g_t, g_s, g_wt, g_bt, g_ws, g_bs = torch.autograd.grad(loss, [t, s] + params)
    with torch.no_grad():
        f = attention_formulas(t, s, tl.weight, tl.bias, sl.weight, dW, dT)
    for name, got, want in (("weighted", f["weighted"], weighted), ("attn", f["attn"], a), ("d_t", f["d_t"], g_t), ("d_s", f["d_s"], g_s),
                            ("dWt", f["dWt"], g_wt), ("dbt", f["dbt"], g_bt), ("dWs", f["dWs"], g_ws)):
        err = float((got - want.detach()).abs().max())
        print("%-8s |formula - autograd| = %.3e of %.3e" % (name, err, float(want.detach().abs().max())))
        assert err <= 1e-12 * max(1.0, float(want.detach().abs().max())), name
    # the bias of spatial_edge_layer: zero to fp64 rounding against gradients of order one
    assert float(g_bs.abs().max()) <= 1e-12 * float(g_bt.abs().max())
