"""The handles of the rollout-time policy forward (cn_policy: HipPolicy, cn_srnn: HipSrnn), the base class every handle wrapper of the package
shares (HipHandle), and the observation compaction of sort_humans = False (compact_visible)."""
import ctypes as C
import math

import torch

from . import _abi as A


def _need_cuda():
    if not torch.cuda.is_available():
        raise A.CnError("no GPU visible: the crowd-sim / policy / GST hot path only runs on MI355X (no CPU fallback)")


class HipHandle:
    """What the wrappers of the library's handles (cn_env_batch, cn_policy, cn_srnn, cn_gst) share: <_sym>_create on the handle's device,
    <_sym>_destroy in close() / __del__, and set_weights over _weights = (pointer struct, [(field, state-dict key)])."""
    _sym, _weights = None, None

    def _open(self, device, *create_args, create=None):
        _need_cuda()
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        h = C.c_void_p()
        A.call(create or self._sym + "_create", *create_args, C.byref(h), device=self.device)
        self._h = h
        self._keep = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            getattr(A.lib(), self._sym + "_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _weight_keys(self):
        """[(field, state-dict key)] of the weights to set: the table, unless a setting of the handle changes it."""
        return self._weights[1]

    def _weights_struct(self, fields, tensors):
        w = self._weights[0]()
        for field, t in zip(fields, tensors):
            setattr(w, field, t.data_ptr())
        return w

    def set_weights(self, state_dict):
        """state_dict: reference key -> tensor; brought to float32 on the handle's device where it is not.  The library snapshots them."""
        keys = self._weight_keys()
        keep = [state_dict[key].detach().to(device=self.device, dtype=torch.float32).contiguous() for _, key in keys]
        w = self._weights_struct([f for f, _ in keys], keep)
        A.call(self._sym + "_set_weights", self._h, C.byref(w), A.stream_ptr(), device=self.device)
        self._keep = keep  # keep sources alive until the async copies are ordered behind later work on the stream


class HipPolicy(HipHandle):
    """cn_policy handle: rollout-time forward (act / get_value) of the attention-graph policy."""

    _sym, _weights = "cn_policy", (A.PolicyWeights, A.POLICY_WEIGHT_KEYS)
    uses_row_plan = True      # act takes the row plan the simulator wrote beside the observation

    def __init__(self, human_num, edge_width, max_envs, device=None, dims=None):
        """dims: the network sizes (R, M, A, O) -- None, a tuple, a dict of the reference's flag names or an A.PolicyDims (A.policy_dims).  None and
        the default tuple take cn_policy_create; any other tuple inside the device box cn_policy_create_sized; outside the box NotImplementedError."""
        self.H, self.D, self.maxE = int(human_num), int(edge_width), int(max_envs)
        self.dims = A.policy_dims(dims)                 # refuses sizes outside the box before anything is allocated
        self.R, self.O = self.dims.rnn_size, self.dims.output_size
        if self.dims.astuple() == A.DEFAULT_DIMS:
            self._open(device, self.H, self.D, self.maxE)
        else:
            self._open(device, self.H, self.D, self.maxE, C.byref(self.dims), create="cn_policy_create_sized")

    def set_self_attention(self, enabled):
        """args.use_self_attn (cn_policy_set_self_attention): False = no human-human attention, spatial_linear is the two-layer MLP
        Linear(D, 128) - ReLU - Linear(128, 256) - ReLU on the spatial edges.  Call before set_weights."""
        A.call("cn_policy_set_self_attention", self._h, int(bool(enabled)))
        self._self_attn = bool(enabled)

    def _weight_keys(self):
        return A.policy_weight_keys(getattr(self, "_self_attn", True))     # use_self_attn = False: the remap, no spatial_attn.* entry

    def act(self, obs, hxs, masks, eps=None, out=None, row_plan=None):
        """row_plan: HipEnvBatch.row_plan of the batch that produced `obs` with its last reset() / step() (optional; see there)."""
        E = obs["robot_node"].shape[0]
        dev = self.device
        if out is None:
            out = dict(value=torch.empty(E, 1, device=dev), action=torch.empty(E, 2, device=dev),
                       logp=torch.empty(E, 1, device=dev), hxs=torch.empty(E, 1, self.R, device=dev))
        if hxs.numel() != E * self.R or out["hxs"].numel() != E * self.R:
            raise A.CnError("HipPolicy.act: the hidden state must be [E,%d] (human_node_rnn_size)" % self.R)
        o = A.obs_struct(obs, row_plan)
        A.call("cn_policy_act", self._h, E, C.byref(o), A.ptr(hxs.contiguous()), A.ptr(masks.contiguous()),
               A.ptr(None if eps is None else eps.contiguous()), A.ptr(out["value"]), A.ptr(out["action"]),
               A.ptr(out["logp"]), A.ptr(out["hxs"]), A.stream_ptr(), device=dev)
        return out

    def get_value(self, obs, hxs, masks, out=None):
        E = obs["robot_node"].shape[0]
        if out is None:
            out = torch.empty(E, 1, device=self.device)
        if hxs.numel() != E * self.R:
            raise A.CnError("HipPolicy.get_value: the hidden state must be [E,%d] (human_node_rnn_size)" % self.R)
        o = A.obs_struct(obs)
        A.call("cn_policy_get_value", self._h, E, C.byref(o), A.ptr(hxs.contiguous()), A.ptr(masks.contiguous()), A.ptr(out),
               A.stream_ptr(), device=self.device)
        return out

    def state_shapes(self, E):
        """The recurrent state this handle carries, under the reference's rnn_hxs names."""
        return {"human_node_rnn": (E, 1, self.R)}

    def act_rnn(self, obs, rnn_hxs, masks, eps=None, out=None, rnn_hxs_out=None, row_plan=None):
        """act under the rollout contract both policy handles share: out = dict(value, action, logp), rnn_hxs / rnn_hxs_out = dicts of the
        tensors state_shapes names (others are ignored), both written in place when given.  Returns (out, rnn_hxs_out)."""
        E, dev = obs["robot_node"].shape[0], self.device
        if out is None:
            out = dict(value=torch.empty(E, 1, device=dev), action=torch.empty(E, 2, device=dev), logp=torch.empty(E, 1, device=dev))
        if rnn_hxs_out is None:
            rnn_hxs_out = {"human_node_rnn": torch.empty(E, 1, self.R, device=dev)}
        self.act(obs, rnn_hxs["human_node_rnn"], masks, eps=eps, out=dict(out, hxs=rnn_hxs_out["human_node_rnn"]), row_plan=row_plan)
        return out, rnn_hxs_out

    def get_value_rnn(self, obs, rnn_hxs, masks, out=None):
        return self.get_value(obs, rnn_hxs["human_node_rnn"], masks, out=out)

    def taps(self, E):
        dev, H = self.device, self.H
        t = dict(spatial_lin=torch.empty(E, H, 256, device=dev), hr_attn=torch.empty(E, H, device=dev),
                 hr_out=torch.empty(E, 256, device=dev), robot_emb=torch.empty(E, 256, device=dev), actor_feat=torch.empty(E, self.O, device=dev))
        A.call("cn_policy_get_taps", self._h, E, A.ptr(t["spatial_lin"]), A.ptr(t["hr_attn"]), A.ptr(t["hr_out"]),
               A.ptr(t["robot_emb"]), A.ptr(t["actor_feat"]), A.stream_ptr(), device=dev)
        return t

    def set_gemm_mode(self, mode):
        """'fused' (default: the whole human-human block as one persistent kernel, bf16x3 split-precision MFMA, ~2e-5 of fp32),
        'bf16x3' (the same arithmetic as separate launches: embedding / q|k|v GEMMs, attention, out_proj) or 'fp32' (exact fp32 MFMA)."""
        A.call("cn_policy_set_gemm_mode", self._h, {"fp32": 0, "bf16x3": 1, "fused": 2}[mode])

    def set_taps(self, enabled):
        """Fused mode: keep / drop the test taps (robot_emb, hr_attn, hr_out, actor_feat) the robot-node kernel writes per forward."""
        A.call("cn_policy_set_taps", self._h, int(bool(enabled)))

    def set_profiling(self, every):
        """0 / False: off; n >= 1 (True = 1): every n-th forward's dominant kernel is timed with a pair of events on its stream."""
        A.call("cn_policy_set_profiling", self._h, int(every))

    def attach_env_tail(self, env):
        """env: a HipEnvBatch in tail-deferral mode (or None to detach): every forward releases that batch's held-back side work right after
        its human-human kernel is enqueued (cn_policy_set_post_hh_hook with cn_env_launch_tail).  Detach before closing the env."""
        if env is None:
            if getattr(self, "_h", None) is not None and self._h:
                A.call("cn_policy_set_post_hh_hook", self._h, None, None)
            old = getattr(self, "_tail_env", None)
            if old is not None:      # forget this policy in the batch's list (repeated attach / detach must not grow it)
                old._tail_policies[:] = [r for r in old._tail_policies if r() is not None and r() is not self]
            self._tail_env = None
            return
        if getattr(env, "_h", None) is None or not env._h:
            raise A.CnError("attach_env_tail: the env batch is closed")
        fn = C.cast(A.lib().cn_env_launch_tail, C.c_void_p)
        A.call("cn_policy_set_post_hh_hook", self._h, fn, env._h)
        self._tail_env = env          # keeps the batch alive as long as the hook points at it
        import weakref
        env._tail_policies[:] = [r for r in env._tail_policies if r() is not None and r() is not self]
        env._tail_policies.append(weakref.ref(self))   # ... and env.close() detaches the hook before the handle is freed

    def get_profile(self):
        ms = (C.c_double * 8)()
        n = (C.c_int64 * 8)()
        A.call("cn_policy_get_profile", self._h, ms, n)
        return list(ms), list(n)

    def get_profile_samples(self):
        """The event brackets of the dominant kernel one by one [ms], in launch order (cn_policy_get_profile_samples)."""
        n = A.lib().cn_policy_get_profile_samples(self._h, None, 0)
        if n < 0:
            A.check(n, "cn_policy_get_profile_samples")
        buf = (C.c_float * max(n, 1))()
        n = A.lib().cn_policy_get_profile_samples(self._h, buf, n)
        return [float(buf[i]) for i in range(n)]

    def reset_profile(self):
        """Drop the samples and sums collected so far, keep the stride (the events stay warm)."""
        A.call("cn_policy_reset_profile", self._h)


class HipSrnn(HipHandle):
    """cn_srnn handle of the DS-RNN baseline (Policy(base='srnn')): the rollout-time forward (act / get_value), two launches per forward, and the
    edge-GRU sequence of the update (seq_fwd / seq_bwd)."""

    _sym, _weights = "cn_srnn", (A.SrnnWeights, A.SRNN_WEIGHT_KEYS)
    uses_row_plan = False

    def __init__(self, human_num, edge_width, max_envs, device=None):
        self.H, self.D, self.maxE = int(human_num), int(edge_width), int(max_envs)
        self._open(device, self.H, self.D, self.maxE)

    @staticmethod
    def _obs(obs):
        o = A.Obs()
        o.robot_node, o.temporal_edges, o.spatial_edges = A.ptr(obs["robot_node"]), A.ptr(obs["temporal_edges"]), A.ptr(obs["spatial_edges"])
        return o

    def act(self, obs, hxs, edge_hxs, masks, eps=None, out=None):
        """hxs [E,128] (or [E,1,128]), edge_hxs [E,H+1,256], masks [E,1].  out: dict(value, action, logp, hxs, edge_hxs) written in place (the
        rollout passes storage rows); out["edge_hxs"] may be edge_hxs itself."""
        E = obs["robot_node"].shape[0]
        dev = self.device
        if out is None:
            out = dict(value=torch.empty(E, 1, device=dev), action=torch.empty(E, 2, device=dev), logp=torch.empty(E, 1, device=dev),
                       hxs=torch.empty(E, 1, 128, device=dev), edge_hxs=torch.empty(E, self.H + 1, 256, device=dev))
        if tuple(out["edge_hxs"].shape) != (E, self.H + 1, 256) or tuple(edge_hxs.shape) != (E, self.H + 1, 256) or hxs.numel() != E * 128:
            raise A.CnError("HipSrnn.act: hidden state shapes must be [E,128] and [E,H+1,256]")
        o = self._obs(obs)
        A.call("cn_srnn_act", self._h, E, C.byref(o), A.ptr(hxs.contiguous()), A.ptr(edge_hxs.contiguous()), A.ptr(masks.contiguous()),
               A.ptr(None if eps is None else eps.contiguous()), A.ptr(out["value"]), A.ptr(out["action"]),
               A.ptr(out["logp"]), A.ptr(out["hxs"]), A.ptr(out["edge_hxs"]), A.stream_ptr(), device=dev)
        return out

    def get_value(self, obs, hxs, edge_hxs, masks, out=None):
        E = obs["robot_node"].shape[0]
        if out is None:
            out = torch.empty(E, 1, device=self.device)
        if tuple(edge_hxs.shape) != (E, self.H + 1, 256) or hxs.numel() != E * 128:
            raise A.CnError("HipSrnn.get_value: hidden state shapes must be [E,128] and [E,H+1,256]")
        o = self._obs(obs)
        A.call("cn_srnn_get_value", self._h, E, C.byref(o), A.ptr(hxs.contiguous()), A.ptr(edge_hxs.contiguous()), A.ptr(masks.contiguous()),
               A.ptr(out), A.stream_ptr(), device=self.device)
        return out

    def state_shapes(self, E):
        """The recurrent state this handle carries, under the reference's rnn_hxs names: the edge state is live."""
        return {"human_node_rnn": (E, 1, 128), "human_human_edge_rnn": (E, self.H + 1, 256)}

    def act_rnn(self, obs, rnn_hxs, masks, eps=None, out=None, rnn_hxs_out=None, row_plan=None):
        """act under the rollout contract of HipPolicy.act_rnn.  row_plan is ignored: DS-RNN runs every slot of every env, so there is no
        packing of live rows to plan."""
        E, dev = obs["robot_node"].shape[0], self.device
        if out is None:
            out = dict(value=torch.empty(E, 1, device=dev), action=torch.empty(E, 2, device=dev), logp=torch.empty(E, 1, device=dev))
        if rnn_hxs_out is None:
            rnn_hxs_out = {k: torch.empty(shape, device=dev) for k, shape in self.state_shapes(E).items()}
        self.act(obs, rnn_hxs["human_node_rnn"], rnn_hxs["human_human_edge_rnn"], masks, eps=eps,
                 out=dict(out, hxs=rnn_hxs_out["human_node_rnn"], edge_hxs=rnn_hxs_out["human_human_edge_rnn"]))
        return out, rnn_hxs_out

    def get_value_rnn(self, obs, rnn_hxs, masks, out=None):
        return self.get_value(obs, rnn_hxs["human_node_rnn"], rnn_hxs["human_human_edge_rnn"], masks, out=out)

    def taps(self, E):
        dev, H = self.device, self.H
        t = dict(edge_out=torch.empty(E, H + 1, 256, device=dev), attn=torch.empty(E, H, device=dev), weighted=torch.empty(E, 256, device=dev),
                 node_out=torch.empty(E, 256, device=dev), actor_feat=torch.empty(E, 256, device=dev))
        A.call("cn_srnn_get_taps", self._h, E, A.ptr(t["edge_out"]), A.ptr(t["attn"]), A.ptr(t["weighted"]), A.ptr(t["node_out"]),
               A.ptr(t["actor_feat"]), A.stream_ptr(), device=dev)
        return t

    def set_gemm_mode(self, mode):
        """'bf16x3' (default: the two edge-GRU products as split-precision MFMA) or 'fp32' (exact fp32 MFMA)."""
        A.call("cn_srnn_set_gemm_mode", self._h, {"fp32": 0, "bf16x3": 1}[mode])

    # ---- the edge-GRU sequence of the update (cn_srnn_seq_fwd / cn_srnn_seq_bwd); SrnnEdgeSequence below is the autograd face ----
    def seq_workspace_bytes(self, T, N):
        """0 = a shape the sequence kernels refuse (the caller then runs the torch-op loop)."""
        return int(A.lib().cn_srnn_seq_workspace_bytes(int(T), int(N), self.H, self.D))

    def _seq_args(self, who, T, N, tensors):
        for name, t, shape in tensors:
            if t is None:
                continue
            if not t.is_cuda or t.device != self.device:
                raise A.CnError("%s: %s must live on %s" % (who, name, self.device))
            if t.dtype != torch.float32:
                raise A.CnError("%s: %s must be float32, not %s" % (who, name, t.dtype))
            if t.numel() != math.prod(shape) or not t.is_contiguous():
                raise A.CnError("%s: %s must be a contiguous tensor of shape %s" % (who, name, list(shape)))

    def seq_fwd(self, temporal_edges, spatial_edges, edge_h0, masks, T, N, workspace=None):
        """temporal_edges [T*N,2], spatial_edges [T*N,H,D], edge_h0 [N,H+1,256], masks [T*N,1] -> (h_all [T,N,H+1,256], workspace)."""
        H, D, dev = self.H, self.D, self.device
        self._seq_args("cn_srnn_seq_fwd", T, N, (("temporal_edges", temporal_edges, (T, N, 2)), ("spatial_edges", spatial_edges, (T, N, H, D)),
                                                  ("edge_h0", edge_h0, (N, H + 1, 256)), ("masks", masks, (T, N))))
        if workspace is None:
            workspace = torch.empty(self.seq_workspace_bytes(T, N) // 4, device=dev)
        h_all = torch.empty(T, N, H + 1, 256, device=dev)
        A.call("cn_srnn_seq_fwd", self._h, T, N, A.ptr(temporal_edges), A.ptr(spatial_edges), A.ptr(edge_h0), A.ptr(masks), A.ptr(h_all),
               A.ptr(workspace), workspace.numel() * workspace.element_size(), A.stream_ptr(), device=dev)
        return h_all, workspace

    def seq_bwd(self, temporal_edges, spatial_edges, edge_h0, masks, h_all, d_h_all, workspace, T, N, grads, d_edge_h0=None):
        """grads: the twelve gradient tensors in A.SRNN_EDGE_KEYS order (overwritten); d_edge_h0 [N,H+1,256] or None.  The workspace is the one
        seq_fwd filled for the same arguments; the call consumes it."""
        H, D, dev = self.H, self.D, self.device
        who = "cn_srnn_seq_bwd"
        self._seq_args(who, T, N, (("temporal_edges", temporal_edges, (T, N, 2)), ("spatial_edges", spatial_edges, (T, N, H, D)),
                                   ("edge_h0", edge_h0, (N, H + 1, 256)), ("masks", masks, (T, N)), ("h_all", h_all, (T, N, H + 1, 256)),
                                   ("d_h_all", d_h_all, (T, N, H + 1, 256)), ("d_edge_h0", d_edge_h0, (N, H + 1, 256))))
        g = A.SrnnEdgeGrads()
        for (field, _), t in zip(A.SRNN_EDGE_KEYS, grads):
            if t is not None:
                self._seq_args(who, T, N, ((field, t, t.shape),))
            setattr(g, field, None if t is None else t.data_ptr())
        if getattr(self, "_seq_partials", None) is None:
            self._seq_partials = torch.empty(A.SRNN_SEQ_PARTIALS_BYTES // 4, device=dev)
        A.call("cn_srnn_seq_bwd", self._h, T, N, A.ptr(temporal_edges), A.ptr(spatial_edges), A.ptr(edge_h0), A.ptr(masks), A.ptr(h_all),
               A.ptr(d_h_all), A.ptr(workspace), workspace.numel() * workspace.element_size(), C.byref(g),
               A.ptr(d_edge_h0), A.ptr(self._seq_partials), A.stream_ptr(), device=dev)


def compact_visible(spatial_edges, visible_masks):
    """args.sort_humans = False: (spatial_edges [B,H,D] with the visible humans moved to the front, detected [B,1] = max(1, visible)) --
    cn_obs_compact_visible; see include/crowdnav_hip.h for why this equals the reference's mask-based attention."""
    B, H, D = spatial_edges.shape
    se = spatial_edges.detach().to(torch.float32).contiguous()
    vm = visible_masks.detach().reshape(B, H).to(torch.uint8).contiguous()
    out = torch.empty_like(se)
    det = torch.empty(B, 1, device=se.device)
    A.call("cn_obs_compact_visible", B, H, D, A.ptr(se), A.ptr(vm), A.ptr(out), A.ptr(det), A.stream_ptr(), device=se.device)
    return out, det
