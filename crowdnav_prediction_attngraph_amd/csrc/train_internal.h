// train_internal.h -- pieces of the training path shared between linear.hip, policy.hip (its part 2, the training entry points) and
// train_step.hip (not part of the C ABI).
#pragma once
#include "common.h"

// One weight-preparation job of a grouped launch: the bf16 hi / lo planes of w (or of w^T), zero-padded to Nw rows, in the fragment order
// cn_linear_fwd loads (cn_split_bf16_padded) -- or, with Kw == 0, a bias vector copied into an Nw-float buffer behind `hi`, zero-padded.
struct CnSplitJob {
    const float *w;
    void *hi, *lo;
    int Nw, Kw, transpose, Nreal; // the weight as the product sees it: [Nreal rows (padded to Nw), Kw]
    int block0;                   // filled by the launcher
};
constexpr int CN_SPLIT_MAX_JOBS = 20;
int cn_split_group_launch(CnSplitJob *jobs, int n, hipStream_t st);                                            // linear.hip
// job for cn_split_bf16_padded(w, rows, cols, transpose, n_padded, planes) with hi = planes, lo = planes + n elements (rn_split in policy.hip, part 2)
CnSplitJob cn_split_job(const float *w, int rows, int cols, int transpose, int n_padded, float *planes);

// cn_linear_fwd_act with weight planes zero-padded to N rows of which only the first n_store columns are stored (linear.hip)
int cn_linear_fwd_act_cols(int M, int N, int n_store, int K, const float *X, int ldx, const void *Whi, const void *Wlo, const float *bias, int act,
                           const float *aux, int ldaux, int relu_from, float *Y, int ldy, void *stream);

// the split jobs of one optimiser step's robot-node sequence: five for cn_rn_seq_fwd (+ the padded te bias), six for cn_rn_seq_bwd
// dims == NULL in the three functions below: the default sizes (128, 64, 64, 256)
int rn_seq_prep_jobs(const cn_rn_weights *w, float *fwd_ws, float *bwd_ws, int T, int N, CnSplitJob *out, const cn_policy_dims *dims = nullptr); // policy.hip, part 2: returns the count (12)
int rn_seq_fwd_impl(int T, int N, int H, const float *robot_node, const float *temporal, const float *out_sp, const int *row_off, const float *h0,
                    const float *masks, const float *actions, const cn_rn_weights *w, const cn_rn_saved *sv, float *ws, float *value, float *logp,
                    void *stream, bool prepared, const cn_policy_dims *dims = nullptr);
// packed_heads != NULL: the heads' gradients stay packed there ([fc_mean.w 512 | critic_linear.w 256 | fc_mean.b 2 | critic_linear.b 1 | logstd 2])
// instead of five device-to-device copies; prepared: the transposed split planes are already in the workspace (rn_seq_prep_jobs)
int rn_seq_bwd_impl(int T, int N, int H, const float *robot_node, const float *temporal, const float *out_sp, const int *row_off, const float *masks,
                    const float *actions, const cn_rn_weights *w, const cn_rn_saved *sv, const float *d_value, const float *d_logp, float *ws,
                    float *d_out_sp, float *d_h0, const cn_rn_grads *g, void *stream, bool prepared, float **packed_heads, const cn_policy_dims *dims = nullptr);
