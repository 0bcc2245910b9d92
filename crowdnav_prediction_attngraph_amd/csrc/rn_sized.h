// rn_sized.h -- internal interface of the robot-node kernel with run-time network sizes (rn_sized.hip), used by policy.hip.
#pragma once
#include "rn_fused.h"

// (R, M, O) = human_node_rnn_size, human_node_embedding_size, human_node_output_size (cn_policy_dims; attention_size only sets the score scale).
// The weight images are rn_fused_bake's: f_te [256 + M, 256], f_whh [3R, R], f_edge [M, 256], f_wih [3R, 2M], f_ac0 [2O, R], f_a2 / f_c2 [O, O];
// the biases and head weights have the matching lengths, hxs_in / hxs_out are [E, R], tap_actor [E, O].
struct RnSizedDims {
    int R, M, O;
    int te;       // envs per workgroup: rn_sized_envs_per_group(R, M, O)
    float scale;  // robot-human score scale (float)((double)H / sqrt((double)attention_size))
};

// 16 when sixteen envs' activation images and the table fit into the 160 KB of LDS, else 8; 0 = sizes outside the kernel's box
int rn_sized_envs_per_group(int R, int M, int O);
size_t rn_sized_lds_bytes(int R, int M, int O, int te);
int rn_sized_forward(int E, int H, const RnFusedArgs &args, const RnSizedDims &dims, hipStream_t st);
