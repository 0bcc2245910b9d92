"""Shared by tests/test_rn_seq_sizes.py (CPU) and tests/test_gpu_rn_seq_sizes.py (-m gpu): the size / shape tables of the robot-node sequence at
off-default network sizes, formula-weighted policies, synthetic inputs, and the sequence's graph in torch ops written on the FOLDED weights of
cn_rn_weights (te = [Ws^T Wt ; encoder_linear], ac0 = (actor.0 ; critic.0) o output_linear) so that every gradient the C ABI returns has a
reference.  test_rn_seq_sizes.py ties that graph to the definition: Policy(...).double() with forward_sequence in torch ops."""
import math

import numpy as np
import torch

from crowdnav_prediction_attngraph_amd import _abi as A
from crowdnav_prediction_attngraph_amd.policy import Policy, make_spaces
from tests import policy_util as PU
from tests.test_policy_sizes import size_kwargs

# (R, M, A, O).  The last one: the resident sized GRU, M = 128, the largest A, and every padded-N and K = 64 (2 a + 1) product at once.
DIMS = [(64, 64, 32, 64), (256, 128, 128, 512), (192, 64, 48, 320), (128, 128, 64, 256), (128, 64, 16, 256), (64, 128, 256, 448)]

# What each tuple reaches (A.rn_seq_plan): padded-N products, K % 128 != 0 weight gradients, GRU kernel, head strides.  DESIGN.md section 4 mirrors it.
PLAN = {
    (64, 64, 32, 64): dict(padded_n={"te": 320, "gi": 192, "a2": 64, "c2": 64, "d1_a": 64, "d1_c": 64, "dhs": 64},
                           ragged_k={"a2_w": 64, "c2_w": 64, "ac0_w": 64, "whh": 64}, gru="resident", head_strides=1),
    (256, 128, 128, 512): dict(padded_n={}, ragged_k={}, gru="streamed", head_strides=8),
    (192, 64, 48, 320): dict(padded_n={"te": 320, "gi": 576, "a2": 320, "c2": 320, "d1_a": 320, "d1_c": 320, "dhs": 192},
                             ragged_k={"a2_w": 320, "c2_w": 320, "ac0_w": 192, "whh": 192}, gru="streamed", head_strides=5),
    (128, 128, 64, 256): dict(padded_n={}, ragged_k={}, gru="resident128", head_strides=4),
    (128, 64, 16, 256): dict(padded_n={"te": 320}, ragged_k={}, gru="resident128", head_strides=4),
    (64, 128, 256, 448): dict(padded_n={"gi": 192, "a2": 448, "c2": 448, "d1_a": 448, "d1_c": 448, "dhs": 64},
                              ragged_k={"a2_w": 448, "c2_w": 448, "ac0_w": 64, "whh": 64}, gru="resident", head_strides=7),
}

# (T, N, H): interior done masks at T = 3; N past one and past two 16-row GRU workgroups with a ragged last one; B = 51 and 99 are not multiples
# of 32 (the weight gradients' row tail); H = 1 and 5 with ragged detected counts; one case at T = 1.
SHAPES = [(3, 17, 5), (3, 33, 1), (1, 17, 5)]
CASES = [(d, SHAPES[0]) for d in DIMS] + [(d, SHAPES[1]) for d in (DIMS[1], DIMS[2], DIMS[5])] + [(DIMS[2], SHAPES[2])]
# Crowds of 49 to 64 humans: the temperature H / sqrt(A) and the two-pass (> 32 rows) robot-human attention inside the sequence.  Default dims at
# the box edge H = 64 and at H = 49 past one 16-row GRU workgroup with a row tail (B = 51); A = 128 (the temperature reaches the kernel through
# the host's scale) with the streamed GRU at H = 64.
CASES += [(DIMS[3], (2, 5, 64)), (DIMS[3], (3, 17, 49)), (DIMS[1], (2, 5, 64))]

VALUE_BAR = 1e-4              # value, logp, h_T: the project bar, absolute
GRAD_REL, GRAD_ABS = 3e-4, 1e-7   # gradients: of the tensor's largest fp64 entry (tests/test_gpu_policy_sizes.py:279-282)


def case_id(c):
    return "R%d_M%d_A%d_O%d-T%d_N%d_H%d" % (c[0] + c[1])


def sized_policy(dims, H, D=2):
    ob_space, act_space = make_spaces(H, D)
    torch.manual_seed(0)
    pol = Policy(ob_space.spaces, act_space, base="selfAttn_merge_srnn", base_kwargs=size_kwargs(dims))
    shapes = {k: tuple(v.shape) for k, v in pol.state_dict().items()}
    pol.load_state_dict({k: torch.from_numpy(v) for k, v in PU.formula_state_dict(shapes).items()})
    return pol


def folded_weights(pol):
    """The tensors of cn_rn_weights, in field order, composed from the modules of `pol` in its own dtype (what AttnGraphBase.rn_sequence does)."""
    b, d = pol.base, pol.dist
    sl, tl, rnn, g = b.attn.spatial_edge_layer[0], b.attn.temporal_edge_layer[0], b.humanNodeRNN, b.humanNodeRNN.gru
    with torch.no_grad():
        te_w = torch.cat([sl.weight.t() @ tl.weight, rnn.encoder_linear.weight], 0)
        te_b = torch.cat([sl.weight.t() @ tl.bias, rnn.encoder_linear.bias], 0)
        w0 = torch.cat([b.actor[0].weight, b.critic[0].weight], 0)
        ac0_w = w0 @ rnn.output_linear.weight
        ac0_b = w0 @ rnn.output_linear.bias + torch.cat([b.actor[0].bias, b.critic[0].bias], 0)
        ws = [b.robot_linear[0].weight, b.robot_linear[0].bias, te_w, te_b, rnn.edge_attention_embed.weight, rnn.edge_attention_embed.bias,
              g.weight_ih_l0, g.bias_ih_l0, g.weight_hh_l0, g.bias_hh_l0, ac0_w, ac0_b, b.actor[2].weight, b.actor[2].bias, b.critic[2].weight,
              b.critic[2].bias, b.critic_linear.weight, b.critic_linear.bias, d.fc_mean.weight, d.fc_mean.bias, d.logstd._bias]
        return [w.detach().clone().contiguous() for w in ws]


def make_inputs(dims, T, N, H, seed=0):
    """float64 numpy inputs of one [T, N] slice: ragged detected counts 1..H (sample 0 has a single row, the last one H), non-negative out_sp rows
    (post-ReLU, like the human-human block's), done masks with env 1 masked at t = 1 and env 2 at t = 2 (and env 0 at t = 0: h0 is dropped)."""
    rs = np.random.RandomState(1000 * seed + 7 * T + N + H)
    B, R = T * N, dims[0]
    det = rs.randint(1, H + 1, size=B)
    det[0], det[-1] = 1, H
    masks = np.ones((T, N))
    masks[0, 0] = 0.0
    if T > 1:
        masks[1, 1] = 0.0
    if T > 2:
        masks[2, 2] = 0.0
    dense = rs.uniform(0.0, 1.0, (B, H, 256)) * (rs.uniform(0, 1, (B, H, 256)) < 0.6)
    valid = np.arange(H)[None, :] < det[:, None]
    dense = dense * valid[:, :, None]
    return dict(robot_node=rs.uniform(-2, 2, (B, 7)), temporal=rs.uniform(-1, 1, (B, 2)), det=det, valid=valid, out_sp=dense, h0=rs.uniform(-1, 1, (N, R)),
                masks=masks.reshape(B), actions=rs.uniform(-1, 1, (B, 2)), d_value=rs.uniform(-1, 1, B) / B, d_logp=rs.uniform(-1, 1, B) / B)


def graph(ws, inp, dims, T, N, H):
    """The sequence in torch ops on the folded weights (any dtype): returns value [B], logp [B], h_T [N,R] and the GRU's saved tensors."""
    R, M, A_, O = dims
    w = dict(zip(A.RN_WEIGHT_FIELDS, ws))
    B = T * N
    rs = torch.relu(torch.cat([inp["temporal"], inp["robot_node"]], 1) @ w["rl_w"].t() + w["rl_b"])
    zz = rs @ w["te_w"].t() + w["te_b"]
    u, enc = zz[:, :256], torch.relu(zz[:, 256:])
    osp = inp["out_sp"]
    a = (u.unsqueeze(1) * osp).sum(-1) * (H / math.sqrt(float(A_)))
    a = torch.softmax(a.masked_fill(~inp["valid"], -1e9), -1)
    hr = torch.bmm(a.unsqueeze(1), osp).squeeze(1)
    x = torch.cat([enc, torch.relu(hr @ w["edge_w"].t() + w["edge_b"])], 1)
    gi = (x @ w["wih"].t() + w["bih"]).view(T, N, 3 * R)
    m = inp["masks"].view(T, N, 1)
    h, hs = inp["h0"], []
    for t in range(T):
        hm = h * m[t]
        gh = hm @ w["whh"].t() + w["bhh"]
        r = torch.sigmoid(gi[t][:, :R] + gh[:, :R])
        z = torch.sigmoid(gi[t][:, R:2 * R] + gh[:, R:2 * R])
        n = torch.tanh(gi[t][:, 2 * R:] + r * gh[:, 2 * R:])
        h = (1.0 - z) * n + z * hm
        hs.append(h)
    a1 = torch.tanh(torch.stack(hs, 0).view(B, R) @ w["ac0_w"].t() + w["ac0_b"])
    actor = torch.tanh(a1[:, :O] @ w["a2_w"].t() + w["a2_b"])
    critic = torch.tanh(a1[:, O:] @ w["c2_w"].t() + w["c2_b"])
    value = (critic @ w["cl_w"].t() + w["cl_b"]).view(B)
    mean = actor @ w["fm_w"].t() + w["fm_b"]
    logstd = w["logstd"].view(1, 2)
    logp = (-((inp["actions"] - mean) ** 2) / (2 * torch.exp(2 * logstd)) - logstd - math.log(math.sqrt(2 * math.pi))).sum(-1)
    return value, logp, h


def run_graph(ws, inp_np, dims, T, N, H, dtype):
    """Forward and backward of graph() in `dtype`: dict of numpy float64 results (value, logp, h_T, d_out_sp [B,H,256], d_h0, g_<field>...)."""
    t = lambda x: torch.from_numpy(np.asarray(x)).to(dtype)   # noqa: E731
    ws = [w.detach().to(dtype).clone().requires_grad_(True) for w in ws]
    inp = {k: t(v) for k, v in inp_np.items() if k not in ("det", "valid")}
    inp["valid"] = torch.from_numpy(inp_np["valid"])
    inp["out_sp"].requires_grad_(True)
    inp["h0"].requires_grad_(True)
    value, logp, h = graph(ws, inp, dims, T, N, H)
    ((value * inp["d_value"]).sum() + (logp * inp["d_logp"]).sum()).backward()
    n = lambda x: x.detach().double().numpy()   # noqa: E731
    res = dict(value=n(value), logp=n(logp), h_T=n(h), d_out_sp=n(inp["out_sp"].grad), d_h0=n(inp["h0"].grad))
    for name, w in zip(A.RN_WEIGHT_FIELDS, ws):
        res["g_" + name] = n(w.grad) if w.grad is not None else np.zeros(tuple(w.shape))
    return res


def compact(inp_np):
    """Dense out_sp [B,H,256] -> the compacted rows [rows,256] and row_off [B+1] the kernels take; and the index of the live rows."""
    valid = inp_np["valid"]
    rows = inp_np["out_sp"][valid]
    row_off = np.concatenate([[0], np.cumsum(inp_np["det"])]).astype(np.int32)
    return rows, row_off


def grad_bar(ref):
    return GRAD_REL * max(float(np.abs(ref).max()), 0.0) + GRAD_ABS
