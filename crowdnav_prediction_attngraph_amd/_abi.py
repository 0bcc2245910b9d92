"""ctypes binding of libcrowdnav_hip.so -- the C ABI declared in include/crowdnav_hip.h.

PyTorch is plumbing here (device memory, streams): tensors cross the boundary as raw device pointers
(`tensor.data_ptr()`) plus the current HIP stream.  There is no CPU fallback: if the extension is missing,
or a call fails, this module raises.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CN_HIP_LIB") or os.path.join(_PKG, "libcrowdnav_hip.so")   # CN_HIP_LIB: another build of the same ABI (A/B measurements)

CN_MAX_HUMANS = 64
ABI_VERSION = 407          # CN_ABI_VERSION of include/crowdnav_hip.h this binding was written against
PROF_KERNELS, PROF_SLOT_WORDS = 8, 2048
PROF_KERNEL_IDS = {"env_step": 0, "orca_lane": 1, "hh_fused": 2, "rn_fused": 3, "orca_lp3": 4, "env_pregen": 5, "row_plan": 6, "other": 7}
ENV_KINDS = {"CrowdSimVarNum-v0": 0, "CrowdSimPred-v0": 1, "CrowdSimPredRealGST-v0": 2, "CrowdSimVarNumCollect-v0": 3}
GSTD_MODES = {None: 0, "train": 1, "val": 2, "test": 2}        # CN_GSTD_ALL / TRAIN / VAL
GSTD_FRAME_ORDER, GSTD_DUPLICATE_ID, GSTD_TOO_MANY_PEDS = 1, 2, 4
INFO_NOTHING, INFO_TIMEOUT, INFO_COLLISION, INFO_REACHGOAL, INFO_DANGER = range(5)


class CnError(RuntimeError):
    pass


class EnvConfig(C.Structure):
    """cn_env_config (mirrors the crowd_nav/configs/config.py fields the path reads)."""
    _fields_ = [
        ("human_num", C.c_int32), ("predict_steps", C.c_int32), ("env_kind", C.c_int32),
        ("randomize_attributes", C.c_int32), ("random_goal_changing", C.c_int32),
        ("end_goal_changing", C.c_int32), ("sort_humans", C.c_int32), ("phase", C.c_int32),
        ("nenv", C.c_int32), ("val_size", C.c_uint32), ("test_size", C.c_uint32), ("robot_policy", C.c_int32),
        ("robot_visible", C.c_int32), ("auto_reset", C.c_int32), ("predict_truth", C.c_int32), ("max_placement_attempts", C.c_int32),
        ("human_num_range", C.c_int32), ("kinematics", C.c_int32), ("humans_policy", C.c_int32), ("pred_interval", C.c_int32),
        ("time_step", C.c_double), ("time_limit", C.c_double),
        ("success_reward", C.c_double), ("collision_penalty", C.c_double),
        ("discomfort_dist", C.c_double), ("discomfort_penalty_factor", C.c_double),
        ("circle_radius", C.c_double), ("arena_size", C.c_double),
        ("human_radius", C.c_double), ("human_v_pref", C.c_double),
        ("robot_radius", C.c_double), ("robot_v_pref", C.c_double), ("sensor_range", C.c_double),
        ("goal_change_chance", C.c_double), ("end_goal_change_chance", C.c_double),
        ("orca_neighbor_dist", C.c_double), ("orca_safety_space", C.c_double),
        ("orca_time_horizon", C.c_double), ("orca_time_horizon_obst", C.c_double),
        ("sf_A", C.c_double), ("sf_B", C.c_double), ("sf_KI", C.c_double),
        ("robot_fov", C.c_double), ("human_fov", C.c_double),
    ]


class PolicyDims(C.Structure):
    """cn_policy_dims: the reference's four network-size flags (arguments.py:155-181) as cn_policy_create_sized takes them."""
    _fields_ = [("rnn_size", C.c_int), ("embedding_size", C.c_int), ("attention_size", C.c_int), ("output_size", C.c_int)]

    def astuple(self):
        return (self.rnn_size, self.embedding_size, self.attention_size, self.output_size)

    def __eq__(self, other):
        return isinstance(other, PolicyDims) and self.astuple() == other.astuple()

    __hash__ = None


DEFAULT_DIMS = (128, 64, 64, 256)      # (R, M, A, O) = human_node_rnn_size, human_node_embedding_size, attention_size, human_node_output_size
DIMS_BOX = "human_node_rnn_size in {64, 128, 192, 256}, human_node_embedding_size in {64, 128}, human_node_output_size a multiple of 64 in [64, 512], " \
           "attention_size in [1, 256]"


def policy_dims(dims=None):
    """dims: None (the default), an (R, M, A, O) tuple, a dict of the four flag names or a PolicyDims -> a PolicyDims inside the device box.
    Outside the box: NotImplementedError naming the box -- raised here, in Python, before anything is allocated (and without needing a GPU)."""
    if dims is None:
        dims = DEFAULT_DIMS
    elif isinstance(dims, PolicyDims):
        dims = dims.astuple()
    elif isinstance(dims, dict):
        names = ("human_node_rnn_size", "human_node_embedding_size", "attention_size", "human_node_output_size")
        stray = sorted(set(dims) - set(names))
        if stray:
            raise KeyError("unknown network size flag(s) %s: the flags are %s" % (", ".join(stray), ", ".join(names)))
        dims = tuple(dims.get(n, d) for n, d in zip(names, DEFAULT_DIMS))
    R, M, A_, O = (int(v) for v in dims)
    if not (R in (64, 128, 192, 256) and M in (64, 128) and 64 <= O <= 512 and O % 64 == 0 and 1 <= A_ <= 256):
        raise NotImplementedError("network sizes (human_node_rnn_size %d, human_node_embedding_size %d, attention_size %d, human_node_output_size %d) are "
                                  "outside the device box: %s (CPU tensors run any sizes the reference accepts)" % (R, M, A_, O, DIMS_BOX))
    return PolicyDims(R, M, A_, O)


CN_MAX_PRED = 8                      # include/crowdnav_hip.h
GST_OBS_LEN = 5
HORIZON_BOX = "observed length %d, prediction horizon (pred_seq_len = sim.predict_steps) in [1, %d]" % (GST_OBS_LEN, CN_MAX_PRED)


def gst_horizon(pred_steps=5, obs_len=GST_OBS_LEN):
    """The prediction horizon P of the GST device path as an int inside the box -- 5 observed frames (the wrapper's history ring and the frame
    take-over are built around them), 1 <= P <= CN_MAX_PRED.  Outside it: NotImplementedError naming the box, raised here, in Python, before
    anything is allocated (and without needing a GPU)."""
    if int(obs_len) != GST_OBS_LEN or int(obs_len) != obs_len:
        raise NotImplementedError("an observed length of %s is outside the device box of the GST kernels: %s (CPU tensors run any lengths)" % (obs_len, HORIZON_BOX))
    if int(pred_steps) != pred_steps or not 1 <= int(pred_steps) <= CN_MAX_PRED:
        raise NotImplementedError("a prediction horizon of %s steps is outside the device box of the GST kernels: %s (CPU tensors run any horizon)"
                                  % (pred_steps, HORIZON_BOX))
    return int(pred_steps)


class Obs(C.Structure):
    _fields_ = [("robot_node", C.c_void_p), ("temporal_edges", C.c_void_p), ("spatial_edges", C.c_void_p),
                ("detected_human_num", C.c_void_p), ("visible_masks", C.c_void_p), ("row_plan", C.c_void_p)]


# order == field order of cn_policy_weights; values == reference state_dict keys
POLICY_WEIGHT_KEYS = [
    ("robot_linear_w", "base.robot_linear.0.weight"), ("robot_linear_b", "base.robot_linear.0.bias"),
    ("emb0_w", "base.spatial_attn.embedding_layer.0.weight"), ("emb0_b", "base.spatial_attn.embedding_layer.0.bias"),
    ("emb2_w", "base.spatial_attn.embedding_layer.2.weight"), ("emb2_b", "base.spatial_attn.embedding_layer.2.bias"),
    ("q_w", "base.spatial_attn.q_linear.weight"), ("q_b", "base.spatial_attn.q_linear.bias"),
    ("k_w", "base.spatial_attn.k_linear.weight"), ("k_b", "base.spatial_attn.k_linear.bias"),
    ("v_w", "base.spatial_attn.v_linear.weight"), ("v_b", "base.spatial_attn.v_linear.bias"),
    ("in_proj_w", "base.spatial_attn.multihead_attn.in_proj_weight"), ("in_proj_b", "base.spatial_attn.multihead_attn.in_proj_bias"),
    ("out_proj_w", "base.spatial_attn.multihead_attn.out_proj.weight"), ("out_proj_b", "base.spatial_attn.multihead_attn.out_proj.bias"),
    ("spatial_linear_w", "base.spatial_linear.0.weight"), ("spatial_linear_b", "base.spatial_linear.0.bias"),
    ("attn_temporal_w", "base.attn.temporal_edge_layer.0.weight"), ("attn_temporal_b", "base.attn.temporal_edge_layer.0.bias"),
    ("attn_spatial_w", "base.attn.spatial_edge_layer.0.weight"), ("attn_spatial_b", "base.attn.spatial_edge_layer.0.bias"),
    ("enc_w", "base.humanNodeRNN.encoder_linear.weight"), ("enc_b", "base.humanNodeRNN.encoder_linear.bias"),
    ("edge_embed_w", "base.humanNodeRNN.edge_attention_embed.weight"), ("edge_embed_b", "base.humanNodeRNN.edge_attention_embed.bias"),
    ("gru_w_ih", "base.humanNodeRNN.gru.weight_ih_l0"), ("gru_w_hh", "base.humanNodeRNN.gru.weight_hh_l0"),
    ("gru_b_ih", "base.humanNodeRNN.gru.bias_ih_l0"), ("gru_b_hh", "base.humanNodeRNN.gru.bias_hh_l0"),
    ("out_w", "base.humanNodeRNN.output_linear.weight"), ("out_b", "base.humanNodeRNN.output_linear.bias"),
    ("actor0_w", "base.actor.0.weight"), ("actor0_b", "base.actor.0.bias"),
    ("actor2_w", "base.actor.2.weight"), ("actor2_b", "base.actor.2.bias"),
    ("critic0_w", "base.critic.0.weight"), ("critic0_b", "base.critic.0.bias"),
    ("critic2_w", "base.critic.2.weight"), ("critic2_b", "base.critic.2.bias"),
    ("critic_linear_w", "base.critic_linear.weight"), ("critic_linear_b", "base.critic_linear.bias"),
    ("fc_mean_w", "dist.fc_mean.weight"), ("fc_mean_b", "dist.fc_mean.bias"),
    ("logstd", "dist.logstd._bias"),
]


def policy_weight_keys(use_self_attn=True):
    """[(field of cn_policy_weights, state-dict key)] of the attention-graph network: POLICY_WEIGHT_KEYS, or, with use_self_attn off
    (cn_policy_set_self_attention(p, 0), cn_ppo_variant.self_attn = 0), the remap the library reads in that mode -- the state dict has no
    spatial_attn.* tensors (those fields stay NULL) and spatial_linear is [.0: 128 x D, .2: 256 x 128].  The one copy of that remap: the rollout
    handle (hip_policy.HipPolicy._weight_keys) and the minibatch steppers (hip_train.MinibatchStepper) both ask here."""
    if use_self_attn:
        return POLICY_WEIGHT_KEYS
    remap = {"emb0_w": "base.spatial_linear.0.weight", "emb0_b": "base.spatial_linear.0.bias",
             "spatial_linear_w": "base.spatial_linear.2.weight", "spatial_linear_b": "base.spatial_linear.2.bias"}
    return [(f, remap.get(f, k)) for f, k in POLICY_WEIGHT_KEYS if f in remap or not k.startswith("base.spatial_attn.")]


# order == field order of cn_srnn_weights (DS-RNN baseline, base='srnn'); values == reference state_dict keys.  The three modules no gradient
# reaches (base.humanNodeRNN.edge_embed, base.human_node_final_linear, base.spatial_linear) are not part of the forward
SRNN_WEIGHT_KEYS = [
    ("enc_s_w", "base.humanhumanEdgeRNN_spatial.encoder_linear.weight"), ("enc_s_b", "base.humanhumanEdgeRNN_spatial.encoder_linear.bias"),
    ("gru_s_w_ih", "base.humanhumanEdgeRNN_spatial.gru.weight_ih_l0"), ("gru_s_w_hh", "base.humanhumanEdgeRNN_spatial.gru.weight_hh_l0"),
    ("gru_s_b_ih", "base.humanhumanEdgeRNN_spatial.gru.bias_ih_l0"), ("gru_s_b_hh", "base.humanhumanEdgeRNN_spatial.gru.bias_hh_l0"),
    ("enc_t_w", "base.humanhumanEdgeRNN_temporal.encoder_linear.weight"), ("enc_t_b", "base.humanhumanEdgeRNN_temporal.encoder_linear.bias"),
    ("gru_t_w_ih", "base.humanhumanEdgeRNN_temporal.gru.weight_ih_l0"), ("gru_t_w_hh", "base.humanhumanEdgeRNN_temporal.gru.weight_hh_l0"),
    ("gru_t_b_ih", "base.humanhumanEdgeRNN_temporal.gru.bias_ih_l0"), ("gru_t_b_hh", "base.humanhumanEdgeRNN_temporal.gru.bias_hh_l0"),
    ("attn_temporal_w", "base.attn.temporal_edge_layer.0.weight"), ("attn_temporal_b", "base.attn.temporal_edge_layer.0.bias"),
    ("attn_spatial_w", "base.attn.spatial_edge_layer.0.weight"), ("attn_spatial_b", "base.attn.spatial_edge_layer.0.bias"),
    ("node_enc_w", "base.humanNodeRNN.encoder_linear.weight"), ("node_enc_b", "base.humanNodeRNN.encoder_linear.bias"),
    ("edge_embed_w", "base.humanNodeRNN.edge_attention_embed.weight"), ("edge_embed_b", "base.humanNodeRNN.edge_attention_embed.bias"),
    ("node_gru_w_ih", "base.humanNodeRNN.gru.weight_ih_l0"), ("node_gru_w_hh", "base.humanNodeRNN.gru.weight_hh_l0"),
    ("node_gru_b_ih", "base.humanNodeRNN.gru.bias_ih_l0"), ("node_gru_b_hh", "base.humanNodeRNN.gru.bias_hh_l0"),
    ("out_w", "base.humanNodeRNN.output_linear.weight"), ("out_b", "base.humanNodeRNN.output_linear.bias"),
    ("actor0_w", "base.actor.0.weight"), ("actor0_b", "base.actor.0.bias"), ("actor2_w", "base.actor.2.weight"), ("actor2_b", "base.actor.2.bias"),
    ("critic0_w", "base.critic.0.weight"), ("critic0_b", "base.critic.0.bias"), ("critic2_w", "base.critic.2.weight"), ("critic2_b", "base.critic.2.bias"),
    ("critic_linear_w", "base.critic_linear.weight"), ("critic_linear_b", "base.critic_linear.bias"),
    ("robot_linear_w", "base.robot_linear.weight"), ("robot_linear_b", "base.robot_linear.bias"),
    ("fc_mean_w", "dist.fc_mean.weight"), ("fc_mean_b", "dist.fc_mean.bias"),
    ("logstd", "dist.logstd._bias"),
]


# order == field order of cn_gst_weights; values == keys of the reference's GST checkpoint
GST_WEIGHT_KEYS = [
    ("node_embedding_w", "gumbel_social_transformer.node_embedding.weight"), ("node_embedding_b", "gumbel_social_transformer.node_embedding.bias"),
    ("in_proj_w", "gumbel_social_transformer.node_encoder_layers.0.self_attn.in_proj_weight"),
    ("in_proj_b", "gumbel_social_transformer.node_encoder_layers.0.self_attn.in_proj_bias"),
    ("out_proj_w", "gumbel_social_transformer.node_encoder_layers.0.self_attn.out_proj.weight"),
    ("out_proj_b", "gumbel_social_transformer.node_encoder_layers.0.self_attn.out_proj.bias"),
    ("norm_node_w", "gumbel_social_transformer.node_encoder_layers.0.norm_node.weight"),
    ("norm_node_b", "gumbel_social_transformer.node_encoder_layers.0.norm_node.bias"),
    ("norm1_node_w", "gumbel_social_transformer.node_encoder_layers.0.norm1_node.weight"),
    ("norm1_node_b", "gumbel_social_transformer.node_encoder_layers.0.norm1_node.bias"),
    ("linear1_w", "gumbel_social_transformer.node_encoder_layers.0.linear1.weight"), ("linear1_b", "gumbel_social_transformer.node_encoder_layers.0.linear1.bias"),
    ("linear2_w", "gumbel_social_transformer.node_encoder_layers.0.linear2.weight"), ("linear2_b", "gumbel_social_transformer.node_encoder_layers.0.linear2.bias"),
    ("lstm_w_ih", "lstm.weight_ih_l0"), ("lstm_w_hh", "lstm.weight_hh_l0"), ("lstm_b_ih", "lstm.bias_ih_l0"), ("lstm_b_hh", "lstm.bias_hh_l0"),
    ("hidden2pos_w", "hidden2pos.weight"), ("hidden2pos_b", "hidden2pos.bias"),
]


RN_WEIGHT_FIELDS = ["rl_w", "rl_b", "te_w", "te_b", "edge_w", "edge_b", "wih", "bih", "whh", "bhh", "ac0_w", "ac0_b", "a2_w", "a2_b", "c2_w", "c2_b",
                    "cl_w", "cl_b", "fm_w", "fm_b", "logstd"]                  # cn_rn_weights / cn_rn_grads, in field order
RN_WEIGHT_SHAPES = [(256, 9), (256,), (320, 256), (320,), (64, 256), (64,), (384, 128), (384,), (384, 128), (384,), (512, 128), (512,),
                    (256, 256), (256,), (256, 256), (256,), (1, 256), (1,), (2, 256), (2,), (2, 1)]
RN_SAVED_FIELDS = ["rs", "z", "hr", "attn", "gi", "hs", "hms", "gates", "a1", "a2"]   # cn_rn_saved


def rn_weight_shapes(dims=None):
    """Shapes of cn_rn_weights / cn_rn_grads, in field order, under cn_policy_dims (R, M, A, O); RN_WEIGHT_SHAPES at the default.  The edge
    width stays 256 and A is not a dimension (it disappears in the fold u = Ws^T (Wt r + bt) and survives as the score temperature)."""
    R, M, _, O = policy_dims(dims).astuple()
    return [(256, 9), (256,), (256 + M, 256), (256 + M,), (M, 256), (M,), (3 * R, 2 * M), (3 * R,), (3 * R, R), (3 * R,), (2 * O, R), (2 * O,),
            (O, O), (O,), (O, O), (O,), (1, O), (1,), (2, O), (2,), (2, 1)]


def rn_saved_widths(dims=None, H=1):
    """Row widths of the cn_rn_saved buffers (each [B, width], dense) under cn_policy_dims."""
    R, M, _, O = policy_dims(dims).astuple()
    return dict(rs=256, z=256 + 2 * M, hr=256, attn=H, gi=3 * R, hs=R, hms=R, gates=4 * R, a1=2 * O, a2=2 * O)


def rn_seq_plan(dims=None):
    """Which of its size-dependent code paths the robot-node sequence takes under cn_policy_dims -- the host-side dispatch of csrc/policy.hip
    and csrc/linear.hip written out (tests/test_rn_seq_sizes.py pins the table; DESIGN.md section 4 mirrors it):
      padded_n     the forward / dX products whose output width is not a multiple of 128 (planes zero-padded, guarded store), as (name, N)
      ragged_k     the weight gradients whose K is 64 (2 a + 1) (half-empty last X tile of the two-barrier split-K kernel), as (name, K)
      gru          the instantiation of csrc/gru_seq.h: 'resident128' / 'resident' (R = 128 / 64: W_hh split once, kept in registers) or 'streamed'
                   (R = 192 / 256: W_hh re-read every step from its fragment image)
      gru_rows     rows (envs) per GRU workgroup: a [T, N] slice runs ceil(N / gru_rows) workgroups
      head_strides O / 64: the strides of the 64 lanes of the head kernels over the trunk features"""
    R, M, _, O = policy_dims(dims).astuple()
    fwd = [("te", 256 + M), ("gi", 3 * R), ("a2", O), ("c2", O), ("d1_a", O), ("d1_c", O), ("dhs", R)]
    wg = [("a2_w", O), ("c2_w", O), ("ac0_w", R), ("whh", R)]
    return dict(padded_n=[(n, w) for n, w in fwd if w % 128], ragged_k=[(n, k) for n, k in wg if k % 128],
                gru="resident128" if R == 128 else ("resident" if R == 64 else "streamed"), gru_rows=16, head_strides=O // 64)


class RnWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in RN_WEIGHT_FIELDS]


class RnSaved(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in RN_SAVED_FIELDS]


class GstWeights(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _ in GST_WEIGHT_KEYS]


class PolicyWeights(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _ in POLICY_WEIGHT_KEYS]


class SrnnWeights(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _ in SRNN_WEIGHT_KEYS]


PPO_BATCH_TENSORS = ["env_idx", "robot_node", "temporal_edges", "spatial_edges", "detected_human_num", "h0", "masks", "actions", "value_preds", "returns",
                     "old_logp", "adv"]     # pointer fields of cn_ppo_batch, in field order


# the twelve parameters of the two edge RNNs: the first twelve fields of cn_srnn_weights == the fields of cn_srnn_edge_grads (cn_srnn_seq_bwd)
SRNN_EDGE_KEYS = SRNN_WEIGHT_KEYS[:12]
SRNN_SEQ_PARTIALS_BYTES = 64 * (768 * 256 + 1024 * 80 + 64 * 80) * 4      # CN_SRNN_SEQ_PARTIALS_BYTES


class SrnnEdgeGrads(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _ in SRNN_EDGE_KEYS]


class PpoBatch(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("T", "N", "E", "H", "D")] + [(n, C.c_void_p) for n in PPO_BATCH_TENSORS]


class PpoHyper(C.Structure):
    _fields_ = [("clip_param", C.c_float), ("value_loss_coef", C.c_float), ("entropy_coef", C.c_float), ("use_clipped_value_loss", C.c_int)]


class PpoVariant(C.Structure):
    """cn_ppo_variant: the two switches of the attention-graph network in the one-call minibatch step; visible_masks = the storage's [T+1,E,H]
    bool tensor, required exactly when sort_humans == 0."""
    _fields_ = [("self_attn", C.c_int32), ("sort_humans", C.c_int32), ("visible_masks", C.c_void_p)]


# every symbol include/crowdnav_hip.h declares (checked by tests/test_abi_symbols.py)
ABI_SYMBOLS = [
    "cn_last_error", "cn_version", "cn_device_count", "cn_env_config_default", "cn_env_create", "cn_env_destroy",
    "cn_env_obs_width", "cn_row_plan_words", "cn_row_plan_build", "cn_env_set_pregen_budget", "cn_env_set_tail_deferral", "cn_env_launch_tail", "cn_policy_set_post_hh_hook", "cn_env_reset", "cn_env_step", "cn_env_join", "cn_env_get_state", "cn_env_get_human_actions", "cn_env_get_danger_min_dist", "cn_env_get_human_counts", "cn_env_set_case_counters", "cn_env_snapshot_bytes", "cn_env_save", "cn_env_load", "cn_orca_solve",
    "cn_policy_create", "cn_policy_create_sized", "cn_policy_destroy", "cn_policy_set_weights", "cn_policy_act", "cn_policy_get_value",
    "cn_policy_get_taps", "cn_policy_set_gemm_mode", "cn_policy_set_self_attention", "cn_obs_compact_visible", "cn_policy_set_taps", "cn_policy_set_profiling", "cn_policy_get_profile",
    "cn_policy_get_profile_samples", "cn_policy_reset_profile", "cn_prof_set_stamps", "cn_prof_next_step", "cn_hh_block_workspace_bytes", "cn_hh_block_fwd", "cn_rn_seq_workspace_floats", "cn_rn_seq_fwd_workspace_floats", "cn_rn_seq_fwd", "cn_rn_seq_bwd", "cn_rn_seq_workspace_floats_sized", "cn_rn_seq_fwd_workspace_floats_sized", "cn_rn_seq_fwd_sized", "cn_rn_seq_bwd_sized", "cn_gru_seq_fwd_sized", "cn_gru_seq_bwd_sized", "cn_hh_attention_workspace_ints", "cn_hh_attention_fwd", "cn_hh_attention_bwd", "cn_hr_attention_fwd", "cn_hr_attention_bwd", "cn_gru_seq_fwd", "cn_gru_seq_bwd", "cn_embed0_fwd", "cn_embed0_bwd",
    "cn_split_bf16", "cn_split_bf16_padded", "cn_linear_fwd", "cn_linear_fwd_act", "cn_linear_wgrad_splits", "cn_linear_wgrad", "cn_small_mm", "cn_gst_create", "cn_gst_create_horizon", "cn_gst_pred_steps", "cn_gst_destroy", "cn_gst_set_weights", "cn_gst_predict",
    "cn_gst_wrapper_reset", "cn_gst_wrapper_step", "cn_gst_wrapper_set_interval", "cn_gst_wrapper_history_len", "cn_gst_wrapper_save", "cn_gst_wrapper_load", "cn_gae", "cn_adv_stats", "cn_adv_normalize", "cn_episode_stats_update", "cn_eval_state_words", "cn_eval_accumulate",
    "cn_ppo_loss_workspace_doubles", "cn_ppo_loss_fwd", "cn_ppo_loss_bwd", "cn_adam_workspace_doubles", "cn_adam_clip_step",
    "cn_ppo_minibatch_max_rows", "cn_ppo_minibatch_workspace_bytes", "cn_ppo_row_totals", "cn_ppo_minibatch_step",
    "cn_ppo_minibatch_workspace_bytes_sized", "cn_ppo_minibatch_step_sized",
    "cn_ppo_minibatch_workspace_bytes_variant", "cn_ppo_minibatch_step_variant", "cn_ppo_row_totals_visible",
    "cn_gst_train_workspace_bytes", "cn_gst_train_step", "cn_gst_eval_workspace_bytes", "cn_gst_eval_step",
    "cn_gst_train_workspace_bytes_horizon", "cn_gst_train_step_horizon", "cn_gst_eval_workspace_bytes_horizon", "cn_gst_eval_step_horizon",
    "cn_gst_data_frames_horizon", "cn_gst_data_count_horizon", "cn_gst_data_fill_horizon", "cn_gst_gather_batch_horizon",
    "cn_env_get_visibility", "cn_render_scenes",
    "cn_env_trace_append", "cn_trace_metrics", "cn_render_trajectories",
    "cn_gst_data_frames", "cn_gst_data_count", "cn_gst_data_fill", "cn_gst_gather_batch",
    "cn_srnn_create", "cn_srnn_destroy", "cn_srnn_set_weights", "cn_srnn_act", "cn_srnn_get_value", "cn_srnn_get_taps", "cn_srnn_set_gemm_mode",
    "cn_srnn_seq_workspace_bytes", "cn_srnn_seq_fwd", "cn_srnn_seq_bwd", "cn_srnn_attn_fwd", "cn_srnn_attn_bwd",
    "cn_env_set_scene",
]

_lib = None


def lib():
    """Load the HIP extension (fails loudly if it was not built: there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CnError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(make -C crowdnav_prediction_attngraph_amd/csrc)" % LIB_PATH)
        # ONE HIP runtime per process: PyTorch-ROCm ships its own libamdhip64; loaded first (import torch), the library's HIP symbols bind to
        # that copy.  Loaded the other way round -- this library before torch, e.g. build() followed by smoke() in one interpreter -- the
        # process ends up with /opt/rocm's runtime AND torch's, and the one behind this library sees no device (measured: cn_env_create
        # "no HIP device visible" while torch.cuda.is_available() is True).
        try:
            import torch  # noqa: F401
        except ImportError:      # the symbol / ABI checks of the CPU-only tests do not need it
            pass
        L = C.CDLL(LIB_PATH)
        vp, i32, i64, f32, f64 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double
        L.cn_last_error.restype = C.c_char_p
        if L.cn_version() != ABI_VERSION:
            raise CnError("%s reports ABI version %d, this binding needs %d: rebuild the library (struct layouts / signatures differ)"
                          % (LIB_PATH, L.cn_version(), ABI_VERSION))
        L.cn_env_config_default.argtypes = [C.POINTER(EnvConfig)]
        L.cn_env_config_default.restype = None
        L.cn_env_create.argtypes = [C.POINTER(EnvConfig), i32, i64, i64, C.POINTER(vp)]
        L.cn_env_destroy.argtypes = [vp]
        L.cn_env_obs_width.argtypes = [C.POINTER(EnvConfig)]
        L.cn_env_reset.argtypes = [vp, C.POINTER(Obs), vp]
        L.cn_env_step.argtypes = [vp, vp, C.POINTER(Obs), vp, vp, vp, vp, vp, vp, vp]
        L.cn_env_join.argtypes = [vp, vp]
        L.cn_env_set_pregen_budget.argtypes = [vp, C.c_int64]
        L.cn_env_set_tail_deferral.argtypes = [vp, i32]
        L.cn_env_launch_tail.argtypes = [vp, vp]
        L.cn_policy_set_post_hh_hook.argtypes = [vp, vp, vp]
        L.cn_row_plan_words.restype = C.c_int64
        L.cn_row_plan_words.argtypes = [C.c_int]
        L.cn_row_plan_build.argtypes = [i32, i32, vp, vp, vp]
        L.cn_env_get_state.argtypes = [vp, vp, vp, vp]
        L.cn_env_set_scene.argtypes = [vp, vp, vp, vp, C.POINTER(Obs), vp]
        L.cn_env_get_danger_min_dist.argtypes = [vp, vp, vp]
        L.cn_env_set_case_counters.argtypes = [vp, vp, vp]
        L.cn_env_get_human_counts.argtypes = [vp, vp, vp]
        L.cn_env_get_human_actions.argtypes = [vp, vp, vp]
        L.cn_env_get_visibility.argtypes = [vp, vp, vp]
        L.cn_render_scenes.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, f32, f32, i32, f32, vp, vp]
        L.cn_env_trace_append.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp]
        L.cn_trace_metrics.argtypes = [i32, i32, i32, vp, vp, vp, f64, f64, vp, vp]
        L.cn_render_trajectories.argtypes = [i32, i32, i32, vp, vp, vp, vp, i32, i32, f32, vp, vp]
        L.cn_env_snapshot_bytes.argtypes = [vp]
        L.cn_env_snapshot_bytes.restype = i64
        L.cn_env_save.argtypes = [vp, vp, vp]
        L.cn_env_load.argtypes = [vp, vp, vp]
        L.cn_orca_solve.argtypes = [i32, i32, vp, vp, f32, i32, f32, f32, vp, vp]
        L.cn_policy_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
        L.cn_policy_create_sized.argtypes = [i32, i32, i32, C.POINTER(PolicyDims), C.POINTER(vp)]
        L.cn_policy_destroy.argtypes = [vp]
        L.cn_policy_set_weights.argtypes = [vp, C.POINTER(PolicyWeights), vp]
        L.cn_policy_act.argtypes = [vp, i32, C.POINTER(Obs), vp, vp, vp, vp, vp, vp, vp, vp]
        L.cn_policy_get_value.argtypes = [vp, i32, C.POINTER(Obs), vp, vp, vp, vp]
        L.cn_policy_get_taps.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
        L.cn_srnn_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
        L.cn_srnn_destroy.argtypes = [vp]
        L.cn_srnn_set_weights.argtypes = [vp, C.POINTER(SrnnWeights), vp]
        L.cn_srnn_act.argtypes = [vp, i32, C.POINTER(Obs), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cn_srnn_get_value.argtypes = [vp, i32, C.POINTER(Obs), vp, vp, vp, vp, vp]
        L.cn_srnn_get_taps.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
        L.cn_srnn_set_gemm_mode.argtypes = [vp, i32]
        L.cn_srnn_seq_workspace_bytes.argtypes = [i32, i32, i32, i32]
        L.cn_srnn_seq_workspace_bytes.restype = i64
        L.cn_srnn_seq_fwd.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp]
        L.cn_srnn_seq_bwd.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64, C.POINTER(SrnnEdgeGrads), vp, vp, vp]
        L.cn_srnn_attn_fwd.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cn_srnn_attn_bwd.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cn_policy_set_profiling.argtypes = [vp, i32]
        L.cn_policy_set_gemm_mode.argtypes = [vp, i32]
        L.cn_policy_set_self_attention.argtypes = [vp, i32]
        L.cn_obs_compact_visible.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp]
        L.cn_policy_set_taps.argtypes = [vp, i32]
        L.cn_policy_get_profile.argtypes = [vp, C.POINTER(f64), C.POINTER(i64)]
        L.cn_policy_get_profile_samples.argtypes = [vp, C.POINTER(f32), i32]
        L.cn_policy_reset_profile.argtypes = [vp]
        L.cn_prof_set_stamps.argtypes = [vp, i32, C.c_uint]
        L.cn_prof_next_step.argtypes = []
        L.cn_hh_block_workspace_bytes.restype = C.c_int64
        L.cn_hh_block_workspace_bytes.argtypes = []
        L.cn_hh_block_fwd.argtypes = [i32, i32, i32] + [vp] * 10 + [f32] + [vp] * 7
        L.cn_rn_seq_workspace_floats.restype = C.c_int64
        L.cn_rn_seq_workspace_floats.argtypes = [i32, i32]
        L.cn_rn_seq_fwd_workspace_floats.restype = C.c_int64
        L.cn_rn_seq_fwd_workspace_floats.argtypes = []
        L.cn_rn_seq_fwd.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(RnWeights), C.POINTER(RnSaved), vp, vp, vp, vp]
        L.cn_rn_seq_bwd.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(RnWeights), C.POINTER(RnSaved), vp, vp, vp, vp, vp, C.POINTER(RnWeights), vp]
        L.cn_hh_attention_workspace_ints.restype = C.c_int64
        L.cn_hh_attention_workspace_ints.argtypes = [i32]
        L.cn_hh_attention_fwd.argtypes = [i32, i32, vp, vp, f32, vp, vp, vp]
        L.cn_hh_attention_bwd.argtypes = [i32, i32, vp, vp, vp, f32, vp, vp, i32, vp]
        L.cn_hr_attention_fwd.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp]
        L.cn_hr_attention_bwd.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cn_rn_seq_workspace_floats_sized.restype = C.c_int64
        L.cn_rn_seq_workspace_floats_sized.argtypes = [i32, i32, C.POINTER(PolicyDims)]
        L.cn_rn_seq_fwd_workspace_floats_sized.restype = C.c_int64
        L.cn_rn_seq_fwd_workspace_floats_sized.argtypes = [C.POINTER(PolicyDims)]
        L.cn_rn_seq_fwd_sized.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(RnWeights), C.POINTER(RnSaved), vp, vp, vp, C.POINTER(PolicyDims), vp]
        L.cn_rn_seq_bwd_sized.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(RnWeights), C.POINTER(RnSaved), vp, vp, vp, vp, vp, C.POINTER(RnWeights),
                                          C.POINTER(PolicyDims), vp]
        L.cn_gru_seq_fwd_sized.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cn_gru_seq_bwd_sized.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cn_gru_seq_fwd.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cn_gru_seq_bwd.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cn_embed0_fwd.argtypes = [i32, i32, vp, vp, vp, vp, vp]
        L.cn_embed0_bwd.argtypes = [i32, i32, vp, vp, vp, i32, vp, vp, vp]
        L.cn_split_bf16.argtypes = [vp, i32, i32, i32, vp, vp, vp]
        L.cn_linear_fwd.argtypes = [i32, i32, i32, vp, i32, vp, vp, vp, vp, i32, vp, i32, vp]
        L.cn_split_bf16_padded.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp]
        L.cn_linear_fwd_act.argtypes = [i32, i32, i32, vp, i32, vp, vp, vp, i32, vp, i32, i32, vp, i32, vp]
        L.cn_linear_wgrad_splits.argtypes = [i32, i32, i32]
        L.cn_small_mm.argtypes = [i32, i32, i32, vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int64, vp, vp]
        L.cn_linear_wgrad.argtypes = [i32, i32, i32, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp]
        L.cn_gst_create.argtypes = [i32, i32, C.POINTER(vp)]
        L.cn_gst_create_horizon.argtypes = [i32, i32, i32, C.POINTER(vp)]
        L.cn_gst_pred_steps.argtypes = [vp]
        L.cn_gst_destroy.argtypes = [vp]
        L.cn_gst_set_weights.argtypes = [vp, C.POINTER(GstWeights), vp]
        L.cn_gst_predict.argtypes = [vp, i32, vp, vp, vp, vp, vp]
        L.cn_gst_wrapper_reset.argtypes = [vp, i32, vp]
        L.cn_gst_wrapper_set_interval.argtypes = [vp, i32]
        L.cn_gst_wrapper_history_len.argtypes = [vp]
        L.cn_gst_wrapper_save.argtypes = [vp, vp, vp, vp]
        L.cn_gst_wrapper_load.argtypes = [vp, i32, vp, vp, vp]
        L.cn_gst_wrapper_step.argtypes = [vp, i32, C.POINTER(Obs), f32, f32, vp, vp, vp]
        L.cn_gae.argtypes = [i32, i32, vp, vp, vp, f64, f64, vp, vp]
        L.cn_episode_stats_update.argtypes = [i32, vp, vp, vp, vp, vp, vp]
        L.cn_eval_state_words.restype = C.c_int64
        L.cn_eval_state_words.argtypes = [i32]
        L.cn_eval_accumulate.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cn_adv_stats.argtypes = [i64, vp, vp, vp, vp]
        L.cn_adv_normalize.argtypes = [i64, vp, vp, vp, vp, vp]
        L.cn_ppo_loss_workspace_doubles.argtypes = []
        L.cn_adam_workspace_doubles.argtypes = []
        L.cn_ppo_loss_fwd.argtypes = [i64, vp, vp, vp, vp, vp, vp, f32, i32, vp, vp, vp]
        L.cn_ppo_loss_bwd.argtypes = [i64, vp, vp, vp, vp, vp, vp, f32, i32, vp, vp, vp, vp]
        L.cn_adam_clip_step.argtypes = [i64, vp, vp, vp, vp, f64, f64, f64, f64, f64, f64, i64, vp, vp, vp]
        L.cn_gst_train_workspace_bytes.restype = C.c_int64
        L.cn_gst_train_workspace_bytes.argtypes = [i32, i32]
        L.cn_gst_train_step.argtypes = [i32, i32, vp, vp, vp, C.POINTER(GstWeights), C.POINTER(GstWeights), f32, C.c_uint64, vp, i64, vp, vp, vp]
        L.cn_gst_eval_workspace_bytes.restype = C.c_int64
        L.cn_gst_eval_workspace_bytes.argtypes = [i32, i32, i32]
        L.cn_gst_eval_step.argtypes = [i32, i32, i32, vp, vp, vp, C.POINTER(GstWeights), vp, vp, i64, vp, vp, vp, vp]
        L.cn_gst_data_frames.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp]
        L.cn_gst_data_count.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cn_gst_data_fill.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
        L.cn_gst_gather_batch.argtypes = [i32, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        # the same calls with the prediction horizon P (the ones above: P = 5)
        L.cn_gst_train_workspace_bytes_horizon.restype = C.c_int64
        L.cn_gst_train_workspace_bytes_horizon.argtypes = [i32, i32, i32]
        L.cn_gst_train_step_horizon.argtypes = [i32, i32, i32, vp, vp, vp, C.POINTER(GstWeights), C.POINTER(GstWeights), f32, C.c_uint64, vp, i64, vp, vp, vp]
        L.cn_gst_eval_workspace_bytes_horizon.restype = C.c_int64
        L.cn_gst_eval_workspace_bytes_horizon.argtypes = [i32, i32, i32, i32]
        L.cn_gst_eval_step_horizon.argtypes = [i32, i32, i32, i32, vp, vp, vp, C.POINTER(GstWeights), vp, vp, i64, vp, vp, vp, vp]
        L.cn_gst_data_frames_horizon.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp]
        L.cn_gst_data_count_horizon.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cn_gst_data_fill_horizon.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
        L.cn_gst_gather_batch_horizon.argtypes = [i32, i32, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cn_ppo_minibatch_max_rows.restype = C.c_int64
        L.cn_ppo_minibatch_max_rows.argtypes = []
        L.cn_ppo_minibatch_workspace_bytes.restype = C.c_int64
        L.cn_ppo_minibatch_workspace_bytes.argtypes = [i32, i32, i32, i32, i64]
        L.cn_ppo_row_totals.argtypes = [i32, i32, i32, vp, vp, vp]
        L.cn_ppo_minibatch_step.argtypes = [C.POINTER(PpoBatch), i64, C.POINTER(PolicyWeights), C.POINTER(PolicyWeights), C.POINTER(PpoHyper), vp, i64, vp, vp, vp]
        L.cn_ppo_minibatch_workspace_bytes_sized.restype = C.c_int64
        L.cn_ppo_minibatch_workspace_bytes_sized.argtypes = [i32, i32, i32, i32, i64, C.POINTER(PolicyDims)]
        L.cn_ppo_minibatch_step_sized.argtypes = [C.POINTER(PpoBatch), i64, C.POINTER(PolicyWeights), C.POINTER(PolicyWeights), C.POINTER(PpoHyper),
                                                  C.POINTER(PolicyDims), vp, i64, vp, vp, vp]
        L.cn_ppo_minibatch_workspace_bytes_variant.restype = C.c_int64
        L.cn_ppo_minibatch_workspace_bytes_variant.argtypes = [i32, i32, i32, i32, i64, C.POINTER(PolicyDims), C.POINTER(PpoVariant)]
        L.cn_ppo_minibatch_step_variant.argtypes = [C.POINTER(PpoBatch), i64, C.POINTER(PolicyWeights), C.POINTER(PolicyWeights), C.POINTER(PpoHyper),
                                                    C.POINTER(PolicyDims), C.POINTER(PpoVariant), vp, i64, vp, vp, vp]
        L.cn_ppo_row_totals_visible.argtypes = [i32, i32, i32, vp, vp, vp]
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().cn_last_error()
        raise CnError("%s failed (status %d): %s" % (what or "libcrowdnav_hip call", rc, msg.decode() if msg else ""))


def call(name, *args, device=None):
    """Run the library function `name`, which returns a status, and raise CnError with the library's message when it is not 0.  device: run it
    under torch.cuda.device(device), for the calls that launch on (or allocate for) the current device; None: no guard."""
    fn = getattr(lib(), name)
    if device is None:
        return check(fn(*args), name)
    import torch
    with torch.cuda.device(device):
        return check(fn(*args), name)


def default_env_config(**over):
    cfg = EnvConfig()
    lib().cn_env_config_default(C.byref(cfg))
    for k, v in over.items():
        if not hasattr(cfg, k):
            raise AttributeError("cn_env_config has no field %r" % k)
        setattr(cfg, k, v)
    return cfg


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Raw device pointer of a contiguous CUDA(HIP) tensor (None -> NULL)."""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise CnError("tensor must live on the GPU (no CPU fallback)")
    if not t.is_contiguous():
        raise CnError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def torch_int32():
    import torch
    return torch.int32


def obs_struct(obs, row_plan=None):
    """cn_obs over the tensors of an observation dict.  row_plan: optional int32 tensor of cn_row_plan_words(E) elements -- an OUTPUT of
    cn_env_reset / cn_env_step beside the observation and an INPUT of cn_policy_act with that same observation (csrc/row_plan.h)."""
    o = Obs()
    if row_plan is not None and (row_plan.dtype != torch_int32() or not row_plan.is_cuda or not row_plan.is_contiguous()):
        raise CnError("row_plan must be a contiguous int32 tensor on the GPU")
    o.row_plan = ptr(row_plan)
    o.robot_node = ptr(obs["robot_node"])
    o.temporal_edges = ptr(obs["temporal_edges"])
    o.spatial_edges = ptr(obs["spatial_edges"])
    o.detected_human_num = ptr(obs["detected_human_num"])
    o.visible_masks = ptr(obs.get("visible_masks"))
    return o
