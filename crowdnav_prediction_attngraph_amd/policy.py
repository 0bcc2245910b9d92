"""Policy -- host-side mirror of the reference's `rl.networks.model.Policy` (selfAttn_merge_srnn base, or the DS-RNN baseline 'srnn', +
DiagGaussian).

Same constructor signature, `act` / `get_value` / `evaluate_actions` contracts and state-dict keys as
/root/reference/rl/networks/model.py:14-90 and rl/networks/selfAttn_srnn_temp_node.py:287-449, so reference
checkpoints load and `train.py` runs unchanged.  Two execution paths:

  * rollout (`act`, `get_value`, no autograd) on a GPU -> hand-written HIP kernels through the C ABI
    (cn_policy_act / cn_policy_get_value).  There is no fallback: on CUDA tensors a missing extension raises.
  * training (`evaluate_actions`, needs gradients) -> on a GPU the forward and the backward of every heavy stage are hand-written HIP
    kernels behind torch.autograd.Functions (hip_train: HHBlockFused, RnSequence, SrnnEdgeSequence, ...); autograd only joins them and
    carries the folded weights' gradients back to their factors.  CPU tensors take the same graph in torch ops: it is the definition, and
    it exists for the CPU unit tests and the reference's `--no-cuda` plumbing mode, never silently on a GPU box.

Parameter construction order follows the reference so that `torch.manual_seed(s); Policy(...)` yields bit-identical
initial weights (tests/test_host_policy.py checks this against checksums captured from the reference).
"""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class Box:
    """Minimal gym.spaces.Box stand-in (gym is not a dependency of the hot path)."""

    def __init__(self, low=-np.inf, high=np.inf, shape=None, dtype=np.float32):
        self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), dtype

    def __repr__(self):
        return "Box%s" % (self.shape,)


class Dict:
    def __init__(self, spaces):
        self.spaces = OrderedDict(sorted(spaces.items()))


def make_spaces(human_num, edge_width, with_masks=True):
    """Observation / action spaces of CrowdSimVarNum-v0 (crowd_sim_var_num.py:37-58) and the Pred variants."""
    d = {"robot_node": Box(shape=(1, 7)), "temporal_edges": Box(shape=(1, 2)), "spatial_edges": Box(shape=(human_num, edge_width)),
         "detected_human_num": Box(shape=(1,))}
    if with_masks:
        d["visible_masks"] = Box(shape=(human_num,), dtype=np.bool_)
    return Dict(d), Box(shape=(2,))


def _arg(args, name, default):
    if args is None:
        return default
    if isinstance(args, dict):
        return args.get(name, default)
    return getattr(args, name, default)


def _skinny_linear(x, w, b):
    """nn.Linear with one or two output columns over tens of thousands of rows (critic_linear, dist.fc_mean in the update).  On the GPU
    the library runs these skinny products, and above all their weight gradients, on a handful of workgroups (0.1-0.2 ms each); as
    row-wise multiply + reduce they are memory-bound passes over x, and autograd's backward of them is too."""
    if x.is_cuda and x.dim() == 2 and w.shape[0] <= 4 and x.shape[0] >= 4096:
        return torch.stack([(x * w[n]).sum(-1) for n in range(w.shape[0])], -1) + b
    return F.linear(x, w, b)


def _ortho(module, gain=1.0):
    nn.init.orthogonal_(module.weight.data, gain=gain)
    nn.init.constant_(module.bias.data, 0)
    return module


class _AddBias(nn.Module):
    """rl/networks/network_utils.py:31-42 -- keeps the checkpoint key `dist.logstd._bias` ([2,1])."""

    def __init__(self, bias):
        super().__init__()
        self._bias = nn.Parameter(bias.unsqueeze(1))

    def forward(self, x):
        return x + self._bias.t().view(1, -1)


class _DiagGaussian(nn.Module):
    def __init__(self, num_inputs, num_outputs):
        super().__init__()
        self.fc_mean = _ortho(nn.Linear(num_inputs, num_outputs))
        self.logstd = _AddBias(torch.zeros(num_outputs))


class _EndRNN(nn.Module):
    def __init__(self, rnn_size, embedding_size, edge_rnn_size, output_size):
        super().__init__()
        self.gru = nn.GRU(embedding_size * 2, rnn_size)
        for name, param in self.gru.named_parameters():
            if "bias" in name:
                nn.init.constant_(param, 0)
            elif "weight" in name:
                nn.init.orthogonal_(param)
        self.encoder_linear = nn.Linear(256, embedding_size)
        self.edge_attention_embed = nn.Linear(edge_rnn_size, embedding_size)
        self.output_linear = nn.Linear(rnn_size, output_size)


class _EdgeAttention(nn.Module):
    def __init__(self, edge_rnn_size, attention_size):
        super().__init__()
        self.temporal_edge_layer = nn.ModuleList()
        self.spatial_edge_layer = nn.ModuleList()
        self.temporal_edge_layer.append(nn.Linear(edge_rnn_size, attention_size))
        self.spatial_edge_layer.append(nn.Linear(edge_rnn_size, attention_size))


class _SpatialSelfAttn(nn.Module):
    def __init__(self, input_size):
        super().__init__()
        self.embedding_layer = nn.Sequential(nn.Linear(input_size, 128), nn.ReLU(), nn.Linear(128, 512), nn.ReLU())
        self.q_linear = nn.Linear(512, 512)
        self.v_linear = nn.Linear(512, 512)
        self.k_linear = nn.Linear(512, 512)
        self.multihead_attn = nn.MultiheadAttention(512, 8)


class AttnGraphBase(nn.Module):
    """The network body (`base`).  Hyper-parameters as in arguments.py:155-206."""

    def __init__(self, obs_space_dict, args):
        super().__init__()
        self.is_recurrent = True
        self.args = args
        self.human_num = obs_space_dict["spatial_edges"].shape[0]
        self.edge_width = obs_space_dict["spatial_edges"].shape[1]
        self.seq_length = _arg(args, "seq_length", 30)
        self.nenv = _arg(args, "num_processes", 16)
        self.nminibatch = _arg(args, "num_mini_batch", 2)
        self.human_node_rnn_size = _arg(args, "human_node_rnn_size", 128)
        self.human_human_edge_rnn_size = _arg(args, "human_human_edge_rnn_size", 256)
        self.output_size = _arg(args, "human_node_output_size", 256)
        emb = self.embedding_size = _arg(args, "human_node_embedding_size", 64)
        attention_size = self.attention_size = _arg(args, "attention_size", 64)
        if self.human_human_edge_rnn_size != 256:
            # selfAttn_srnn_temp_node.py:330-345: robot_linear and spatial_linear are hard-wired to 256 columns, so the reference's own first forward
            # fails on the shapes ("mat1 and mat2 shapes cannot be multiplied") for any other value of this flag
            raise NotImplementedError("human_human_edge_rnn_size = %d: the reference itself cannot run an edge size other than 256 (its robot_linear "
                                      "and spatial_linear are hard-wired to 256)" % self.human_human_edge_rnn_size)
        if min(self.human_node_rnn_size, self.output_size, emb, attention_size) < 1:
            raise ValueError("network sizes must be positive")
        # arguments.py:189, :206.  use_self_attn = False: no human-human attention, spatial_linear embeds the raw edges
        # (selfAttn_srnn_temp_node.py:340-345); sort_humans = False: attention masks from `visible_masks` instead of the detected count (:378-383)
        self.use_self_attn = bool(_arg(args, "use_self_attn", True))
        self.sort_humans = bool(_arg(args, "sort_humans", True))
        env_name = _arg(args, "env_name", None)
        expect = {"CrowdSimVarNum-v0": 2, "CrowdSimPred-v0": 12, "CrowdSimPredRealGST-v0": 12}.get(env_name)
        if expect is not None and _arg(args, "predict_steps", 5) == 5 and expect != self.edge_width:
            raise ValueError("env_name %s expects spatial edge width %d, observation space has %d" % (env_name, expect, self.edge_width))
        gain = math.sqrt(2)
        # construction order == reference (selfAttn_srnn_temp_node.py:309-343) so seeded inits are bit-identical
        self.humanNodeRNN = _EndRNN(self.human_node_rnn_size, emb, self.human_human_edge_rnn_size, self.output_size)
        self.attn = _EdgeAttention(self.human_human_edge_rnn_size, attention_size)
        h = self.output_size
        self.actor = nn.Sequential(_ortho(nn.Linear(h, h), gain), nn.Tanh(), _ortho(nn.Linear(h, h), gain), nn.Tanh())
        self.critic = nn.Sequential(_ortho(nn.Linear(h, h), gain), nn.Tanh(), _ortho(nn.Linear(h, h), gain), nn.Tanh())
        self.critic_linear = _ortho(nn.Linear(h, 1), gain)
        self.robot_linear = nn.Sequential(_ortho(nn.Linear(9, 256), gain), nn.ReLU())
        self.human_node_final_linear = _ortho(nn.Linear(self.output_size, 2), gain)
        if self.use_self_attn:
            self.spatial_attn = _SpatialSelfAttn(self.edge_width)
            self.spatial_linear = nn.Sequential(_ortho(nn.Linear(512, 256), gain), nn.ReLU())
        else:
            self.spatial_linear = nn.Sequential(_ortho(nn.Linear(self.edge_width, 128), gain), nn.ReLU(), _ortho(nn.Linear(128, 256), gain), nn.ReLU())

    # ---- training-time forward in torch ops (autograd) ----
    # arithmetic of the three large human-human Linear layers in the PPO update on the GPU: 'bf16x3' = split-precision MFMA
    # kernels (forward, dX, dW; same arithmetic as the rollout forward), 'fp32' = torch / rocBLAS fp32
    train_gemm_mode = "bf16x3"
    # the human-human block of the update's forward as one fused launch (hip_train.HHBlockFused; crowds of <= 48 humans) instead of five
    train_fused_hh = True
    # everything behind the human-human block (robot node, robot-human attention, GRU sequence, trunks, heads, log-prob) as ONE call forward and
    # ONE backward (hip_train.RnSequence: cn_rn_seq_fwd / cn_rn_seq_bwd) instead of torch modules with HIP Functions spliced in
    train_fused_rn = True

    gemm_mode_attr = "rollout_gemm_mode"      # the Policy attribute that holds the gemm mode of this base's rollout handle

    def make_hip_handle(self, E, device):
        """The rollout handle of this network for up to E envs, configured but without weights."""
        from .hip_policy import HipPolicy
        hip = HipPolicy(self.human_num, self.edge_width, E, device=device, dims=self.dims)     # sizes outside the device box: refused here
        hip.set_self_attention(self.use_self_attn)
        hip.set_taps(False)          # rollout path: nobody reads the test taps
        return hip

    @property
    def dims(self):
        """(R, M, A, O) = (human_node_rnn_size, human_node_embedding_size, attention_size, human_node_output_size): cn_policy_dims."""
        return (self.human_node_rnn_size, self.embedding_size, self.attention_size, self.output_size)

    @property
    def default_sizes(self):
        """The reference's default widths: the ones the per-op training Functions of the torch-op route (train_fused_rn = False, 'fp32') are
        specialised to.  The robot-node sequence (rn_sequence) and the one-call minibatch step (cn_ppo_minibatch_step_sized) run any sizes in
        the device box."""
        from ._abi import DEFAULT_DIMS
        return self.dims == DEFAULT_DIMS

    def forward_rnn(self, inputs, rnn_hxs, masks, T, N):
        """forward_sequence under the contract both bases share: (value, actor features, rnn_hxs after step T of the state this base carries)."""
        value, feat, h = self.forward_sequence(inputs, rnn_hxs["human_node_rnn"], masks, T, N)
        return value, feat, {"human_node_rnn": h.view(N, 1, -1)}

    def counted_inputs(self, inputs):
        """sort_humans = True: the inputs as they are.  sort_humans = False (selfAttn_srnn_temp_node.py:378-383, :410-414): both attention modules
        mask by `visible_masks` (an all-invisible sample keeps human 0).  They are permutation-equivariant over the humans, and masked humans
        contribute exactly nothing (their keys are excluded, their rows meet an exactly-zero robot-human weight), so the masked form equals
        the counted form on the observation with the visible humans moved to the front -- stable, so that equal inputs give equal outputs."""
        if self.sort_humans:
            return inputs
        se = inputs["spatial_edges"]
        B = se.shape[0]
        se = se.reshape(B, self.human_num, self.edge_width)
        vm = inputs["visible_masks"].reshape(B, self.human_num)
        out = dict(inputs)
        if se.is_cuda:
            from .hip_policy import compact_visible
            out["spatial_edges"], out["detected_human_num"] = compact_visible(se, vm)
        else:
            m = vm.to(torch.bool).clone()
            m[~m.any(1), 0] = True
            order = torch.argsort((~m).to(torch.int8), dim=1, stable=True)
            out["spatial_edges"] = torch.gather(se, 1, order.unsqueeze(-1).expand(-1, -1, self.edge_width))
            out["detected_human_num"] = m.sum(1, keepdim=True).to(se.dtype)
        return out

    def fused_rn_shapes_ok(self):
        """The modules have exactly the DEFAULT layer shapes of the robot-node sequence (_abi.RN_WEIGHT_SHAPES): what the unsized
        cn_ppo_minibatch_step takes (hip_train.MinibatchStepper.supported).  evaluate_actions and hip_train.SizedMinibatchStepper.supported ask
        sized_rn_ok(): hip_train.RnSequence and cn_ppo_minibatch_step_sized run every sizes tuple inside the device box."""
        rnn, g = self.humanNodeRNN, self.humanNodeRNN.gru
        return (tuple(self.robot_linear[0].weight.shape) == (256, 9) and tuple(rnn.edge_attention_embed.weight.shape) == (64, 256)
                and tuple(rnn.encoder_linear.weight.shape) == (64, 256) and tuple(self.attn.temporal_edge_layer[0].weight.shape) == (64, 256)
                and tuple(self.attn.spatial_edge_layer[0].weight.shape) == (64, 256)
                and tuple(g.weight_ih_l0.shape) == (384, 128) and tuple(g.weight_hh_l0.shape) == (384, 128)
                and tuple(rnn.output_linear.weight.shape) == (256, 128) and tuple(self.actor[2].weight.shape) == (256, 256)
                and tuple(self.critic_linear.weight.shape) == (1, 256))

    def sized_rn_ok(self):
        """The robot-node sequence (hip_train.RnSequence: cn_rn_seq_fwd_sized / cn_rn_seq_bwd_sized) and the one-call minibatch step
        (hip_train.SizedMinibatchStepper: cn_ppo_minibatch_step_sized) run at these sizes: every dims tuple inside the device box with the
        reference's 256-wide edge features.  Wider than fused_rn_shapes_ok(), which keeps meaning "the default shapes" (what
        hip_train.MinibatchStepper.supported answers for)."""
        from ._abi import policy_dims
        try:
            policy_dims(self.dims)
        except NotImplementedError:
            return False
        rnn = self.humanNodeRNN
        return (tuple(self.robot_linear[0].weight.shape) == (256, 9) and rnn.edge_attention_embed.weight.shape[1] == 256
                and rnn.encoder_linear.weight.shape[1] == 256 and self.attn.spatial_edge_layer[0].weight.shape[1] == 256)

    def rn_sequence(self, inputs, out_sp, row_off, h0, masks, actions, T, N, dist):
        """(value [B,1], logp [B,1], h_T [N,R]) through hip_train.RnSequence.  The two affine pairs without a nonlinearity in between are composed
        here in torch ops (tiny products, autograd carries the folded gradients back to both factors): u = Ws^T (Wt r + bt) -- the
        spatial_edge_layer projection moved to the robot side, its bias keeps an exactly-zero gradient -- and (actor.0 ; critic.0) o output_linear."""
        from .hip_train import RnSequence
        B = T * N
        sl, tl, rnn = self.attn.spatial_edge_layer[0], self.attn.temporal_edge_layer[0], self.humanNodeRNN
        from .hip_train import weight_mm as mm     # weight-by-weight products: cn_small_mm forward and backward (no library GEMM / GEMV)
        te_w = torch.cat([mm(sl.weight.t(), tl.weight), rnn.encoder_linear.weight], 0)
        te_b = torch.cat([mm(sl.weight.t(), tl.bias) + 0.0 * sl.bias.sum(), rnn.encoder_linear.bias], 0)
        w0 = torch.cat([self.actor[0].weight, self.critic[0].weight], 0)
        ac0_w = mm(w0, rnn.output_linear.weight)
        ac0_b = mm(w0, rnn.output_linear.bias) + torch.cat([self.actor[0].bias, self.critic[0].bias], 0)
        g = rnn.gru
        return RnSequence.apply(inputs["robot_node"].reshape(B, 7), inputs["temporal_edges"].reshape(B, 2), out_sp, row_off, h0.reshape(N, -1), masks.reshape(B),
                                actions.reshape(B, 2), T, N, (self.human_num, self.attention_size),
                                self.robot_linear[0].weight, self.robot_linear[0].bias, te_w, te_b, rnn.edge_attention_embed.weight, rnn.edge_attention_embed.bias,
                                g.weight_ih_l0, g.bias_ih_l0, g.weight_hh_l0, g.bias_hh_l0, ac0_w, ac0_b, self.actor[2].weight, self.actor[2].bias,
                                self.critic[2].weight, self.critic[2].bias, self.critic_linear.weight, self.critic_linear.bias, dist.fc_mean.weight, dist.fc_mean.bias,
                                dist.logstd._bias)

    def _big_linear(self, x, w, b, relu=False):
        if x.is_cuda and self.train_gemm_mode == "bf16x3":
            from . import hip_train as hip
            if hip.linear_supported(x, w):
                return hip.HipLinear.apply(x, w, b, relu)
        y = F.linear(x, w, b)
        return F.relu(y) if relu else y

    def _lin(self, x, w, b):
        """Per-sample Linear layer of the update: on the GPU the weight gradient (a reduction over all T*N rows into a small
        matrix) goes to the split-K TN kernel, everything else stays a library product."""
        if x.is_cuda and self.train_gemm_mode == "bf16x3" and self.default_sizes:    # other widths: the torch-op definition (library products)
            from . import hip_train as hip
            if hip.linear_supported(x, w) and x.shape[0] >= 16384:
                return hip.HipLinear.apply(x, w, b, False)   # [128 a, 128 b] weights: forward, dX and dW on the pipelined bf16x3 kernels
            if hip.wgrad_supported(x, w):
                return hip.WgradLinear.apply(x, w, b)
        return F.linear(x, w, b)

    def _mlp2(self, seq, x):
        """Sequential(Linear, Tanh, Linear, Tanh) (actor / critic trunks)."""
        return torch.tanh(self._lin(torch.tanh(self._lin(x, seq[0].weight, seq[0].bias)), seq[2].weight, seq[2].bias))

    def _hh_block(self, spatial_edges, det):
        """[B,H,D] -> [B,H,256].  SpatialEdgeSelfAttn.forward + spatial_linear (selfAttn_srnn_temp_node.py:63-91,:408).

        Only the detected humans (index < det) are pushed through the linear layers: padded humans are masked as keys
        and their own outputs only ever meet an exactly-zero robot-human attention weight, so values and gradients are
        identical to the dense computation while the dominant GEMMs shrink by H / mean(det) (~3.4x at 20 humans).
        The tiny per-env attention itself runs on zero-padded [B,8,H,64] tensors."""
        B, H, D = spatial_edges.shape
        sa = self.spatial_attn if self.use_self_attn else None
        det = det.clamp(1, H)   # every sample has 1..H rows, as the env guarantees (crowd_sim_var_num.py:290-292) and the kernels assume
        valid = torch.arange(H, device=spatial_edges.device).view(1, H) < det.view(B, 1)     # key padding mask
        idx = valid.reshape(-1).nonzero(as_tuple=False).squeeze(1)                            # live (sample, human) rows
        x_live = spatial_edges.reshape(B * H, D).index_select(0, idx)
        if not self.use_self_attn:
            # selfAttn_srnn_temp_node.py:404-408 with use_self_attn = False: output_spatial = spatial_linear(spatial_edges), a two-layer MLP per
            # human; only the live rows are computed (the others only ever meet an exactly-zero robot-human weight)
            l0, l2 = self.spatial_linear[0], self.spatial_linear[2]
            if x_live.is_cuda and D <= 16:
                from .hip_train import Embed0
                e0 = Embed0.apply(x_live, l0.weight, l0.bias)
            else:
                e0 = F.relu(l0(x_live))
            o = self._big_linear(e0, l2.weight, l2.bias, relu=True)
            if o.is_cuda:
                nd = det.to(torch.int32)
                return o, torch.cat([nd.new_zeros(1), nd.cumsum(0, dtype=torch.int32)])
            return o.new_zeros(B * H, o.shape[1]).index_copy(0, idx, o).view(B, H, -1), valid
        emb0, emb2 = sa.embedding_layer[0], sa.embedding_layer[2]
        if x_live.is_cuda and self.train_gemm_mode == "bf16x3" and self.train_fused_hh and H <= 48 and D <= 16 and emb0.weight.shape[0] == 128:
            # ONE launch for the whole block (the rollout's fused kernel on the training weights, writing the activations the backward
            # needs); the affine pairs are composed exactly as below, so both factors still receive their exact gradients
            from .hip_train import HHBlockFused
            W, b = sa.multihead_attn.in_proj_weight, sa.multihead_attn.in_proj_bias
            lins = (sa.q_linear, sa.k_linear, sa.v_linear)
            from .hip_train import weight_mm as mm     # the folds and their backward as cn_small_mm launches
            Wc = torch.cat([mm(W[i * 512:(i + 1) * 512], lins[i].weight) for i in range(3)], 0)
            bc = torch.cat([mm(W[i * 512:(i + 1) * 512], lins[i].bias) + b[i * 512:(i + 1) * 512] for i in range(3)], 0)
            op, sl = sa.multihead_attn.out_proj, self.spatial_linear[0]
            nd = det.clamp(1, H).to(torch.int32)   # 1..H rows per sample, like the rollout kernels (crowd_sim_var_num.py:290-292)
            row_off = torch.cat([nd.new_zeros(1), nd.cumsum(0, dtype=torch.int32)])
            o = HHBlockFused.apply(spatial_edges, x_live, row_off, emb0.weight, emb0.bias, emb2.weight, emb2.bias, Wc, bc,
                                   mm(sl.weight, op.weight), mm(sl.weight, op.bias) + sl.bias)
            return o, row_off
        if x_live.is_cuda and D <= 16 and emb0.weight.shape[0] == 128:
            from .hip_train import Embed0
            e0 = Embed0.apply(x_live, emb0.weight, emb0.bias)
        else:
            e0 = F.relu(emb0(x_live))
        e = self._big_linear(e0, emb2.weight, emb2.bias, relu=True)
        # (q|k|v)_linear followed by in_proj is an affine pair with no nonlinearity in between: compose the two weight
        # matrices first (a 512^3 product, differentiable, so both factors still receive their exact gradients) and run ONE
        # [rows,512]x[512,1536] GEMM instead of six [rows,512]x[512,512] ones, in the forward and in the backward pass.
        W, b = sa.multihead_attn.in_proj_weight, sa.multihead_attn.in_proj_bias
        lins = (sa.q_linear, sa.k_linear, sa.v_linear)
        Wc = torch.cat([W[i * 512:(i + 1) * 512] @ lins[i].weight for i in range(3)], 0)
        bc = torch.cat([W[i * 512:(i + 1) * 512] @ lins[i].bias + b[i * 512:(i + 1) * 512] for i in range(3)], 0)
        qkv = self._big_linear(e, Wc, bc)                                                   # [rows, 1536] = [q | k | v]
        if qkv.is_cuda:
            # attention core on the compacted rows, forward AND backward as hand-written HIP kernels
            from .hip_train import HHAttention
            nd = det.clamp(1, H).to(torch.int32)   # 1..H rows per sample, like the rollout kernels (crowd_sim_var_num.py:290-292)
            row_off = torch.cat([nd.new_zeros(1), nd.cumsum(0, dtype=torch.int32)])
            o_live = HHAttention.apply(qkv, row_off, B, H, 0.125)
        else:
            # CPU tensors (unit tests): the same math on zero-padded [B,8,H,64] tensors in torch ops
            q, k, v = qkv.split(512, dim=-1)

            def pad(x):
                return x.new_zeros(B * H, 512).index_copy(0, idx, x).view(B, H, 8, 64).transpose(1, 2)

            scores = torch.matmul(pad(q), pad(k).transpose(-1, -2)) * 0.125
            scores = scores.masked_fill(~valid.view(B, 1, 1, H), float("-inf"))
            o = torch.matmul(torch.softmax(scores, dim=-1), pad(v)).transpose(1, 2).reshape(B * H, 512)
            o_live = o.index_select(0, idx)
        # same composition for out_proj followed by spatial_linear (Linear -> Linear -> ReLU)
        op, sl = sa.multihead_attn.out_proj, self.spatial_linear[0]
        o = self._big_linear(o_live, sl.weight @ op.weight, sl.weight @ op.bias + sl.bias, relu=True)
        if o.is_cuda:
            return o, row_off                     # stays compacted: the robot-human attention kernels index rows through row_off
        out_sp = o.new_zeros(B * H, o.shape[1]).index_copy(0, idx, o).view(B, H, -1)
        return out_sp, valid

    def _hr_attention(self, robot_states, out_sp, valid):
        """EdgeAttention_M (selfAttn_srnn_temp_node.py:145-223): [B,256],[B,H,256] -> [B,256]."""
        H = out_sp.shape[1]
        t = self.attn.temporal_edge_layer[0](robot_states)
        s = self.attn.spatial_edge_layer[0](out_sp)
        a = (t.unsqueeze(1) * s).sum(-1) * (H / math.sqrt(float(self.attention_size)))     # :151-152: a double scalar times a float32 tensor
        a = torch.softmax(a.masked_fill(~valid, -1e9), dim=-1)
        return torch.bmm(a.unsqueeze(1), out_sp).squeeze(1), a

    def _gru_cell(self, gi, h):
        g = self.humanNodeRNN.gru
        gh = F.linear(h, g.weight_hh_l0, g.bias_hh_l0)
        i_r, i_z, i_n = gi.chunk(3, -1)
        h_r, h_z, h_n = gh.chunk(3, -1)
        r = torch.sigmoid(i_r + h_r)
        z = torch.sigmoid(i_z + h_z)
        n = torch.tanh(i_n + r * h_n)
        return (1.0 - z) * n + z * h

    def forward_sequence(self, inputs, h0, masks, T, N):
        """inputs: dict of [T*N, ...] (T-major), h0 [N,1,R] or [N,R], masks [T*N,1] (R = human_node_rnn_size, 128 by default).
        Returns value [T*N,1], actor features [T*N,O], h_T [N,R] (O = human_node_output_size, 256 by default).  Masking h at every step is arithmetically the
        reference's split-at-done trick (rl/networks/srnn_model.py:52-104)."""
        B = T * N
        inputs = self.counted_inputs(inputs)
        robot_in = torch.cat((inputs["temporal_edges"].reshape(B, 2), inputs["robot_node"].reshape(B, 7)), dim=-1)
        robot_states = self.robot_linear(robot_in)
        det = inputs["detected_human_num"].reshape(B).to(torch.int64).clamp(min=1)
        out_sp, valid = self._hh_block(inputs["spatial_edges"].reshape(B, self.human_num, self.edge_width), det)
        if out_sp.is_cuda:
            # compacted rows [R,256] + row offsets: HIP robot-human attention forward/backward (no dense [B,H,256] tensors)
            # t . (Ws o_j + bs) = (Ws^T t) . o_j + const: the spatial_edge_layer projection moves to the robot side (B rows
            # instead of ~6B) and its bias, which the softmax cannot see, keeps an exactly-zero gradient
            from .hip_train import HRAttention
            sl = self.attn.spatial_edge_layer[0]
            tl = self.attn.temporal_edge_layer[0]
            from .hip_train import RightMatmul
            t_emb = self._lin(robot_states, tl.weight, tl.bias)
            u = (RightMatmul.apply(t_emb, sl.weight) if t_emb.shape[0] >= 4096 and self.default_sizes else t_emb @ sl.weight) + 0.0 * sl.bias.sum()
            if self.attention_size != 64:
                # cn_hr_attention_fwd / _bwd scale the scores by H / 8 = H / sqrt(64); H / sqrt(A) is that times 8 / sqrt(A), carried by u
                u = u * (8.0 / math.sqrt(float(self.attention_size)))
            hr = HRAttention.apply(u, out_sp, valid, self.human_num)
        else:
            hr, _ = self._hr_attention(robot_states, out_sp, valid)
        rnn = self.humanNodeRNN
        x = torch.cat((F.relu(self._lin(robot_states, rnn.encoder_linear.weight, rnn.encoder_linear.bias)),
                       F.relu(self._lin(hr, rnn.edge_attention_embed.weight, rnn.edge_attention_embed.bias))), dim=-1)
        gi = self._lin(x, rnn.gru.weight_ih_l0, rnn.gru.bias_ih_l0).view(T, N, -1)
        m = masks.reshape(T, N, 1)
        h = h0.reshape(N, -1)
        if gi.is_cuda and tuple(rnn.gru.weight_hh_l0.shape) == (384, 128):      # hip_train.GRUSequence (this per-op route) takes R = 128 only
            from .hip_train import GRUSequence
            hs_all = GRUSequence.apply(gi, h, m, rnn.gru.weight_hh_l0, rnn.gru.bias_hh_l0)
            h = hs_all[-1]
        else:
            hs = []
            for gi_t, m_t in zip(gi.unbind(0), m.unbind(0)):
                h = self._gru_cell(gi_t, h * m_t)
                hs.append(h)
            hs_all = torch.stack(hs, 0)
        out = self._lin(hs_all.view(B, -1), rnn.output_linear.weight, rnn.output_linear.bias)
        value = _skinny_linear(self._mlp2(self.critic, out), self.critic_linear.weight, self.critic_linear.bias)
        return value, self._mlp2(self.actor, out), h


class _SrnnRNN(nn.Module):
    """RNNBase of rl/networks/srnn_model.py:10-30: the GRU is created, and orthogonally initialised, before the Linear layers of the subclass.
    The parameters live in nn.GRU for checkpoint-key parity; the forward below never calls the module (explicit cells: no vendor RNN library)."""

    def __init__(self, input_size, rnn_size):
        super().__init__()
        self.gru = nn.GRU(input_size, rnn_size)
        for name, param in self.gru.named_parameters():
            if "bias" in name:
                nn.init.constant_(param, 0)
            elif "weight" in name:
                nn.init.orthogonal_(param)


class _SrnnNodeRNN(_SrnnRNN):
    """HumanNodeRNN (srnn_model.py:108-146).  edge_embed is constructed and never used (a dead module: no gradient, in the state dict)."""

    def __init__(self, rnn_size, embedding_size, input_size, edge_rnn_size, output_size):
        super().__init__(embedding_size * 2, rnn_size)
        self.encoder_linear = nn.Linear(input_size, embedding_size)
        self.edge_embed = nn.Linear(edge_rnn_size, embedding_size)
        self.edge_attention_embed = nn.Linear(edge_rnn_size * 2, embedding_size)
        self.output_linear = nn.Linear(rnn_size, output_size)


class _SrnnEdgeRNN(_SrnnRNN):
    """HumanHumanEdgeRNN (srnn_model.py:177-199)."""

    def __init__(self, input_size, embedding_size, rnn_size):
        super().__init__(embedding_size, rnn_size)
        self.encoder_linear = nn.Linear(input_size, embedding_size)


def _gru_cell(gi, h, w_hh, b_hh):
    """torch's GRU cell (gate order r, z, n) on a precomputed input side gi = W_i x + b_i."""
    gh = F.linear(h, w_hh, b_hh)
    i_r, i_z, i_n = gi.chunk(3, -1)
    h_r, h_z, h_n = gh.chunk(3, -1)
    r = torch.sigmoid(i_r + h_r)
    z = torch.sigmoid(i_z + h_z)
    n = torch.tanh(i_n + r * h_n)
    return (1.0 - z) * n + z * h


class SRNNBase(nn.Module):
    """The DS-RNN baseline body (`base='srnn'`: rl/networks/srnn_model.py:326-468, the `args.env_type == 'crowd_sim'` branch, i.e. a 7-wide robot
    node).  Two edge GRUs (one temporal edge, H spatial edges, hidden 256) whose state is LIVE -- `human_human_edge_rnn` [N,H+1,256], slot 0 the
    temporal edge --, dot-product attention over ALL H slots (no mask: detected_human_num / visible_masks are not read), a node GRU (128) and the
    actor / critic trunks.  Module names and construction order are the reference's: seeded inits are bit-identical and reference checkpoints load.
    Three modules never reach the output and never get a gradient (humanNodeRNN.edge_embed, human_node_final_linear, spatial_linear)."""

    DEAD_MODULES = ("humanNodeRNN.edge_embed", "human_node_final_linear", "spatial_linear")
    # forward_sequence on GPU tensors: both edge GRUs over all T steps as hip_train.SrnnEdgeSequence (cn_srnn_seq_fwd / cn_srnn_seq_bwd) instead of
    # the torch-op loop, which stays the definition (False, CPU tensors, or a shape cn_srnn_seq_workspace_bytes refuses)
    train_edge_kernels = True
    # ... and everything behind h_all: the attention as hip_train.SrnnAttention (cn_srnn_attn_fwd / cn_srnn_attn_bwd) on h_all itself, the node GRU
    # as hip_train.GRUSequence, the products over the T*N rows through HipLinear / WgradLinear (_node_kernels).  False, CPU or non-fp32 tensors,
    # or no provider: the torch ops below, which stay the definition
    train_node_kernels = True

    def __init__(self, obs_space_dict, args):
        super().__init__()
        self.is_recurrent = True
        self.hip_provider = None            # Policy sets it (_hip_handle): (N, device) -> the HipSrnn handle with the current weights
        self.gemm_mode_provider = None      # ... and this (_base_gemm_mode): () -> the gemm mode that handle runs in
        self.args = args
        self.human_num = obs_space_dict["spatial_edges"].shape[0]
        self.edge_width = obs_space_dict["spatial_edges"].shape[1]
        self.seq_length = _arg(args, "seq_length", 30)
        self.nenv = _arg(args, "num_processes", 16)
        self.nminibatch = _arg(args, "num_mini_batch", 2)
        self.human_node_rnn_size = _arg(args, "human_node_rnn_size", 128)
        self.human_human_edge_rnn_size = _arg(args, "human_human_edge_rnn_size", 256)
        self.output_size = _arg(args, "human_node_output_size", 256)
        emb = _arg(args, "human_node_embedding_size", 64)
        edge_emb = _arg(args, "human_human_edge_embedding_size", 64)
        attention_size = _arg(args, "attention_size", 64)
        node_in = _arg(args, "human_node_input_size", 3)
        temporal_in = _arg(args, "human_human_edge_input_size", 2)
        if (self.human_node_rnn_size, self.human_human_edge_rnn_size, self.output_size, emb, attention_size) != (128, 256, 256, 64, 64) \
                or (edge_emb, node_in, temporal_in) != (64, 3, 2):
            raise NotImplementedError("the HIP kernels are specialised to the reference's network sizes (128/256/256/64/64)")
        if _arg(args, "env_type", "crowd_sim") != "crowd_sim":
            raise NotImplementedError("only the env_type == 'crowd_sim' branch of srnn_model.py:378 (robot node width 7) is implemented")
        if not 1 <= self.human_num <= 64:
            raise NotImplementedError("crowds of 1..64 humans (CN_MAX_HUMANS)")
        # the flags of the attention-graph network that the rest of the package reads off a base; DS-RNN reads neither the count nor the masks
        self.use_self_attn, self.sort_humans = False, True
        gain = math.sqrt(2)
        # construction order == srnn_model.py:354-386
        self.humanNodeRNN = _SrnnNodeRNN(self.human_node_rnn_size, emb, node_in, self.human_human_edge_rnn_size, self.output_size)
        self.humanhumanEdgeRNN_spatial = _SrnnEdgeRNN(self.edge_width, edge_emb, self.human_human_edge_rnn_size)
        self.humanhumanEdgeRNN_temporal = _SrnnEdgeRNN(temporal_in, edge_emb, self.human_human_edge_rnn_size)
        self.attn = _EdgeAttention(self.human_human_edge_rnn_size, attention_size)
        h = self.output_size
        self.actor = nn.Sequential(_ortho(nn.Linear(h, h), gain), nn.Tanh(), _ortho(nn.Linear(h, h), gain), nn.Tanh())
        self.critic = nn.Sequential(_ortho(nn.Linear(h, h), gain), nn.Tanh(), _ortho(nn.Linear(h, h), gain), nn.Tanh())
        self.critic_linear = _ortho(nn.Linear(h, 1), gain)
        self.robot_linear = _ortho(nn.Linear(7, 3), gain)
        self.human_node_final_linear = _ortho(nn.Linear(self.output_size, 2), gain)
        self.spatial_linear = _ortho(nn.Linear(self.edge_width, 2), gain)

    gemm_mode_attr = "srnn_gemm_mode"

    def make_hip_handle(self, E, device):
        from .hip_policy import HipSrnn
        return HipSrnn(self.human_num, self.edge_width, E, device=device)

    def forward_rnn(self, inputs, rnn_hxs, masks, T, N):
        value, feat, h, e = self.forward_sequence(inputs, rnn_hxs["human_node_rnn"], rnn_hxs["human_human_edge_rnn"], masks, T, N)
        return value, feat, {"human_node_rnn": h.view(N, 1, -1), "human_human_edge_rnn": e}

    def counted_inputs(self, inputs):
        return inputs

    @staticmethod
    def _edge_gi(rnn, x):
        """ReLU(encoder_linear(x)) and the input side of the GRU for all time steps at once."""
        e = F.relu(F.linear(x, rnn.encoder_linear.weight, rnn.encoder_linear.bias))
        return F.linear(e, rnn.gru.weight_ih_l0, rnn.gru.bias_ih_l0)

    def attention(self, h_t, h_s):
        """EdgeAttention (srnn_model.py:256-323) on [..., 256] and [..., H, 256]: the temperature H / sqrt(64) MULTIPLIES, softmax over all H
        slots without a mask.  Returns (weighted [..., 256], attention weights [..., H])."""
        H = h_s.shape[-2]
        te = F.linear(h_t, self.attn.temporal_edge_layer[0].weight, self.attn.temporal_edge_layer[0].bias)
        se = F.linear(h_s, self.attn.spatial_edge_layer[0].weight, self.attn.spatial_edge_layer[0].bias)
        a = torch.softmax((te.unsqueeze(-2) * se).sum(-1) * (H / math.sqrt(64.0)), dim=-1)
        return (a.unsqueeze(-1) * h_s).sum(-2), a

    def _edge_parameters(self):
        """The twelve parameters of the two edge RNNs in cn_srnn_weights field order (_abi.SRNN_EDGE_KEYS)."""
        out = []
        for rnn in (self.humanhumanEdgeRNN_spatial, self.humanhumanEdgeRNN_temporal):
            out += [rnn.encoder_linear.weight, rnn.encoder_linear.bias, rnn.gru.weight_ih_l0, rnn.gru.weight_hh_l0, rnn.gru.bias_ih_l0, rnn.gru.bias_hh_l0]
        return out

    def _edge_sequence_handle(self, inputs, edge_h0, masks, T, N):
        """The HipSrnn handle for the kernel path of the edge-GRU sequence, or None where the torch-op loop runs: train_edge_kernels off, CPU or
        non-fp32 tensors, no provider (a base outside a Policy), or a shape the kernels refuse."""
        if not (self.train_edge_kernels and self.hip_provider is not None and edge_h0.is_cuda):
            return None
        if any(t.dtype != torch.float32 for t in (inputs["temporal_edges"], inputs["spatial_edges"], edge_h0, masks)):
            return None
        from . import _abi as A
        if A.lib().cn_srnn_seq_workspace_bytes(T, N, self.human_num, self.edge_width) <= 0:
            return None
        return self.hip_provider(N, edge_h0.device)

    def _node_kernel_mode(self, inputs, node_h0, edge_h0, masks):
        """The gemm mode the kernel path behind h_all follows (_node_kernels: the Policy's, which its handle has too), or None where the torch ops
        run: train_node_kernels off, CPU or non-fp32 tensors, or no provider (a base outside a Policy).  H is inside the kernels' box by
        construction.  No handle is asked for: these kernels read the parameters themselves."""
        if not (self.train_node_kernels and self.hip_provider is not None and edge_h0.is_cuda):
            return None
        if any(t.dtype != torch.float32 for t in (inputs["robot_node"], inputs["temporal_edges"], inputs["spatial_edges"], node_h0, edge_h0, masks)):
            return None
        return self.gemm_mode_provider()

    def _node_kernels(self, mode, h_all, rn, node_h0, m, T, N):
        """Everything behind the edge GRUs on h_all [T,N,H+1,256]: (value, actor features, node h_T, node output, weighted, attention weights).
        The attention kernels are plain fp32 and run in both gemm modes.  In 'bf16x3' the node GRU is hip_train.GRUSequence (one launch each
        way), the products over the T*N rows go through HipLinear (forward, dX and dW on the split-precision kernels) or, where only the weight
        gradient has a kernel (edge_attention_embed: 64 columns), WgradLinear, and robot_linear -> encoder_linear, two affine maps with nothing
        in between, is one 7 -> 64 map composed weight by weight (autograd carries the gradient back to both factors).  In 'fp32' those pieces
        are the torch ops of the definition."""
        from . import hip_train as K
        B, node, split = T * N, self.humanNodeRNN, mode == "bf16x3"

        def lin(x, layer):
            w, b = (layer.weight, layer.bias) if isinstance(layer, nn.Linear) else layer
            if split and K.linear_supported(x, w):
                return K.HipLinear.apply(x, w, b, False)
            if split and K.wgrad_supported(x, w):
                return K.WgradLinear.apply(x, w, b)
            return F.linear(x, w, b)

        tl, sl = self.attn.temporal_edge_layer[0], self.attn.spatial_edge_layer[0]
        weighted, a, ht = K.SrnnAttention.apply(h_all, tl.weight, tl.bias, sl.weight, sl.bias, True)
        rl, enc = self.robot_linear, node.encoder_linear
        if split:
            enc_in = F.linear(rn, K.weight_mm(enc.weight, rl.weight), K.weight_mm(enc.weight, rl.bias) + enc.bias)
        else:
            enc_in = F.linear(F.linear(rn, rl.weight, rl.bias), enc.weight, enc.bias)
        ee = F.relu(lin(torch.cat((ht, weighted), -1).view(B, -1), node.edge_attention_embed))
        gi_n = lin(torch.cat((F.relu(enc_in), ee), -1), (node.gru.weight_ih_l0, node.gru.bias_ih_l0)).view(T, N, -1)
        h_n = node_h0.reshape(N, -1)
        if split:
            hns = K.GRUSequence.apply(gi_n, h_n, m, node.gru.weight_hh_l0, node.gru.bias_hh_l0)
            h_n = hns[-1]
        else:
            hs = []
            for t in range(T):
                h_n = _gru_cell(gi_n[t], h_n * m[t], node.gru.weight_hh_l0, node.gru.bias_hh_l0)
                hs.append(h_n)
            hns = torch.stack(hs, 0)
        out = lin(hns.view(B, -1), node.output_linear)
        feat = torch.tanh(lin(torch.tanh(lin(out, self.actor[0])), self.actor[2]))
        crit = torch.tanh(lin(torch.tanh(lin(out, self.critic[0])), self.critic[2]))
        return _skinny_linear(crit, self.critic_linear.weight, self.critic_linear.bias), feat, h_n, out, weighted, a

    def forward_sequence(self, inputs, node_h0, edge_h0, masks, T, N, taps=None):
        """inputs: dict of [T*N, ...] (T-major), node_h0 [N,1,128] or [N,128], edge_h0 [N,H+1,256], masks [T*N,1].
        Returns value [T*N,1], actor features [T*N,256], node h_T [N,128], edge h_T [N,H+1,256].  The state is multiplied by masks[t] at EVERY
        step, which equals the reference's split of the sequence at the steps where any env has a zero mask (srnn_model.py:52-104)."""
        B, H = T * N, self.human_num
        rn = inputs["robot_node"].reshape(B, 7)
        m = masks.reshape(T, N, 1)
        et, es, node = self.humanhumanEdgeRNN_temporal, self.humanhumanEdgeRNN_spatial, self.humanNodeRNN
        edge_h0 = edge_h0.reshape(N, H + 1, -1)
        hip = self._edge_sequence_handle(inputs, edge_h0, masks, T, N)
        if hip is not None:
            from .hip_train import SrnnEdgeSequence
            h_all = SrnnEdgeSequence.apply(hip, inputs["temporal_edges"].reshape(B, 2), inputs["spatial_edges"].reshape(B, H, self.edge_width), edge_h0,
                                           masks.reshape(B, 1), *self._edge_parameters())
            ht_all, hs_all = h_all[:, :, 0], h_all[:, :, 1:]                            # views of [T,N,H+1,256]
            h_t, h_s = ht_all[-1].detach(), hs_all[-1].detach()
        else:
            gi_t = self._edge_gi(et, inputs["temporal_edges"].reshape(B, 2)).view(T, N, -1)
            gi_s = self._edge_gi(es, inputs["spatial_edges"].reshape(B, H, self.edge_width)).view(T, N, H, -1)
            h_t, h_s = edge_h0[:, 0], edge_h0[:, 1:]
            hts, hss = [], []
            for t in range(T):
                h_t = _gru_cell(gi_t[t], h_t * m[t], et.gru.weight_hh_l0, et.gru.bias_hh_l0)
                h_s = _gru_cell(gi_s[t], h_s * m[t].unsqueeze(1), es.gru.weight_hh_l0, es.gru.bias_hh_l0)
                hts.append(h_t)
                hss.append(h_s)
            ht_all, hs_all = torch.stack(hts, 0), torch.stack(hss, 0)                   # [T,N,256], [T,N,H,256]
        node_mode = self._node_kernel_mode(inputs, node_h0, edge_h0, masks)
        if node_mode is not None:
            if hip is None:
                h_all = torch.cat((ht_all.unsqueeze(2), hs_all), 2)                     # the torch-op edge loop: [T,N,H+1,256] as the kernels read it
            value, feat, h_n, out, weighted, a = self._node_kernels(node_mode, h_all, rn, node_h0, m, T, N)
            if taps is not None:
                taps.update(edge_out=torch.cat((h_t.unsqueeze(1), h_s), 1), attn=a.reshape(B, H), weighted=weighted.reshape(B, -1), node_out=out, actor_feat=feat)
            return value, feat, h_n, torch.cat((h_t.unsqueeze(1), h_s), 1)
        weighted, a = self.attention(ht_all, hs_all)
        enc = F.relu(F.linear(F.linear(rn, self.robot_linear.weight, self.robot_linear.bias), node.encoder_linear.weight, node.encoder_linear.bias))
        ee = F.relu(F.linear(torch.cat((ht_all, weighted), -1).view(B, -1), node.edge_attention_embed.weight, node.edge_attention_embed.bias))
        gi_n = F.linear(torch.cat((enc, ee), -1), node.gru.weight_ih_l0, node.gru.bias_ih_l0).view(T, N, -1)
        h_n = node_h0.reshape(N, -1)
        hns = []
        for t in range(T):
            h_n = _gru_cell(gi_n[t], h_n * m[t], node.gru.weight_hh_l0, node.gru.bias_hh_l0)
            hns.append(h_n)
        out = F.linear(torch.stack(hns, 0).view(B, -1), node.output_linear.weight, node.output_linear.bias)
        feat = self.actor(out)
        value = _skinny_linear(self.critic(out), self.critic_linear.weight, self.critic_linear.bias)
        if taps is not None:
            taps.update(edge_out=torch.cat((h_t.unsqueeze(1), h_s), 1), attn=a.reshape(B, H), weighted=weighted.reshape(B, -1), node_out=out, actor_feat=feat)
        return value, feat, h_n, torch.cat((h_t.unsqueeze(1), h_s), 1)


class Policy(nn.Module):
    """Drop-in for rl.networks.model.Policy."""

    def __init__(self, obs_shape, action_space, base=None, base_kwargs=None):
        super().__init__()
        if base not in ("selfAttn_merge_srnn", "srnn", None):
            raise NotImplementedError("only base='selfAttn_merge_srnn' and base='srnn' are implemented")
        if action_space.__class__.__name__ != "Box":
            raise NotImplementedError("only Box(2) action spaces (holonomic robot) are implemented")
        self.base = (SRNNBase if base == "srnn" else AttnGraphBase)(obs_shape, base_kwargs)
        if base == "srnn":
            self.base.hip_provider = self._hip_handle
            self.base.gemm_mode_provider = self._base_gemm_mode
        self.srnn = True
        self.dist = _DiagGaussian(self.base.output_size, action_space.shape[0])
        self._hip = None
        self._hip_version = self._hip_mode = None
        self._zero_edge = {}

    @property
    def is_recurrent(self):
        return self.base.is_recurrent

    # ---- HIP rollout path ----
    def _weights_version(self):
        return tuple(p._version for p in self.parameters()) + tuple(p.data_ptr() for p in self.parameters())

    # rollout arithmetic / launch structure (cn_policy_set_gemm_mode): 'fused' = two persistent kernels (default, fastest; an env's
    # result depends on its tile neighbours at the 1e-7 level through the softmax summation order), 'bf16x3' = the same arithmetic as
    # separate launches whose per-env results are independent of the batch composition, 'fp32' = exact fp32 MFMA
    rollout_gemm_mode = "fused"

    def _hip_handle(self, E, device):
        """The base's rollout handle (HipPolicy / HipSrnn) for E envs on `device`, in the gemm mode and with the weights of this moment."""
        if self._hip is None or self._hip.maxE < E or self._hip.device != device:
            self._hip = self.base.make_hip_handle(E, device)
            self._hip_version = self._hip_mode = None
        mode = getattr(self, self.base.gemm_mode_attr)
        if self._hip_mode != mode:
            self._hip.set_gemm_mode(mode)
            self._hip_mode = mode
        ver = self._weights_version()
        if ver != self._hip_version:
            self._hip.set_weights(self.state_dict())
            self._hip_version = ver
        return self._hip

    def _base_gemm_mode(self):
        return getattr(self, self.base.gemm_mode_attr)

    _hip_policy = _hip_srnn = _hip_handle     # the per-base names the handle had before: the existing tests reach it through them

    def weights_changed(self):
        """Tell the rollout path that parameter storage was written through raw pointers (the fused Adam kernel): the next
        act / get_value re-snapshots the weights (cn_policy_set_weights / cn_srnn_set_weights)."""
        self._hip_version = None

    # arithmetic of the two edge-GRU products (cn_srnn_set_gemm_mode): 'bf16x3' = split-precision MFMA (default), 'fp32' = exact fp32 MFMA
    srnn_gemm_mode = "bf16x3"

    @property
    def is_srnn_baseline(self):
        return isinstance(self.base, SRNNBase)

    def _edge_zeros(self, E, device):
        key = (E, str(device))
        if key not in self._zero_edge:
            self._zero_edge = {key: torch.zeros(1, 1, 1, device=device).expand(E, self.base.human_num + 1, self.base.human_human_edge_rnn_size)}
        return self._zero_edge[key]

    def _obs32(self, inputs):
        inputs = self.base.counted_inputs(inputs)      # sort_humans = False: visible humans first + their count (cn_obs_compact_visible)
        return {k: (v if v.dtype == torch.float32 else v.float()).contiguous() for k, v in inputs.items() if k != "visible_masks"}

    def _all_states(self, hxs, N, device):
        """rnn_hxs as the reference returns it: the state the base carries plus, where the edge state is not live, its zeros."""
        if "human_human_edge_rnn" not in hxs:
            hxs["human_human_edge_rnn"] = self._edge_zeros(N, device)
        return hxs

    def _hip_args(self, pol, E, inputs, rnn_hxs, masks):
        return self._obs32(inputs), {k: rnn_hxs[k].reshape(shape).float() for k, shape in pol.state_shapes(E).items()}, masks.reshape(E, 1).float()

    def act(self, inputs, rnn_hxs, masks, deterministic=False):
        E = inputs["robot_node"].shape[0]
        dev = rnn_hxs["human_node_rnn"].device
        if dev.type == "cuda":
            pol = self._hip_handle(E, dev)
            eps = None if deterministic else torch.randn(E, 2, device=dev)
            out, h = pol.act_rnn(*self._hip_args(pol, E, inputs, rnn_hxs, masks), eps=eps)
            value, action, logp = out["value"], out["action"], out["logp"]
        else:
            with torch.no_grad():
                value, feat, h = self.base.forward_rnn(inputs, rnn_hxs, masks, 1, E)
                mean = self.dist.fc_mean(feat)
                std = self.dist.logstd(torch.zeros_like(mean)).exp()
                action = mean if deterministic else mean + std * torch.randn_like(mean)
                logp = self._log_prob(mean, std, action)
        return value, action, logp, self._all_states(h, E, dev)

    def get_value(self, inputs, rnn_hxs, masks):
        E = inputs["robot_node"].shape[0]
        dev = rnn_hxs["human_node_rnn"].device
        if dev.type == "cuda":
            pol = self._hip_handle(E, dev)
            return pol.get_value_rnn(*self._hip_args(pol, E, inputs, rnn_hxs, masks))
        with torch.no_grad():
            value, _, _ = self.base.forward_rnn(inputs, rnn_hxs, masks, 1, E)
        return value

    @staticmethod
    def _log_prob(mean, std, action):
        var = std * std
        return (-((action - mean) ** 2) / (2 * var) - std.log() - math.log(math.sqrt(2 * math.pi))).sum(-1, keepdim=True)

    def evaluate_actions(self, inputs, rnn_hxs, masks, action):
        """inputs [T*N,...] (T = seq_length, N = num_processes / num_mini_batch), rnn_hxs at t=0 ([N,...]).  The T-step sequence under
        autograd: on the GPU its heavy stages are HIP kernels behind autograd.Functions (the attention-graph base: the whole of it, below;
        DS-RNN: the two edge GRUs, SRNNBase.train_edge_kernels, and the attention and node half behind them, SRNNBase.train_node_kernels), on the
        CPU everything is torch ops: that graph is the definition."""
        B = inputs["robot_node"].shape[0]
        N = rnn_hxs["human_node_rnn"].shape[0]
        T = B // N
        base = self.base
        if getattr(base, "train_fused_rn", False) and inputs["robot_node"].is_cuda and base.train_gemm_mode == "bf16x3" and base.sized_rn_ok():
            # the attention-graph base's train-mode forward as two boundary calls: the human-human block (cn_hh_block_fwd behind _hh_block)
            # and the robot-node sequence (cn_rn_seq_fwd_sized: any sizes inside the device box), each with ONE backward entry
            inputs = base.counted_inputs(inputs)
            det = inputs["detected_human_num"].reshape(B).to(torch.int64).clamp(min=1)
            out_sp, row_off = base._hh_block(inputs["spatial_edges"].reshape(B, base.human_num, base.edge_width), det)
            value, logp, h = base.rn_sequence(inputs, out_sp, row_off, rnn_hxs["human_node_rnn"], masks, action, T, N, self.dist)
            logstd = self.dist.logstd._bias.t().view(1, -1)
            entropy = (0.5 + 0.5 * math.log(2 * math.pi) + logstd).mean()   # FixedNormal.entropy().mean(): the same for every sample
            return value, logp, entropy, self._all_states({"human_node_rnn": h.view(N, 1, -1)}, N, h.device)
        value, feat, h = base.forward_rnn(inputs, rnn_hxs, masks, T, N)
        mean = _skinny_linear(feat, self.dist.fc_mean.weight, self.dist.fc_mean.bias)
        logstd = self.dist.logstd(torch.zeros_like(mean))
        logp = self._log_prob(mean, logstd.exp(), action)
        entropy = (0.5 + 0.5 * math.log(2 * math.pi) + logstd).mean()   # FixedNormal.entropy().mean(): over batch and dims
        return value, logp, entropy, self._all_states(h, N, value.device)
