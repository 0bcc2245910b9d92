// gst_model.h -- the GST predictor's shape constants and parameter table, shared by the training step (gst_train.hip) and the evaluation
// step (gst_eval.hip).  Shipped hyper-parameters: embedding 64, 8 heads, one NodeEncoderLayer without ghost / edge heads, LSTM 64,
// 5 observed steps and GP = pred_seq_len predicted ones, 1 .. GP_MAX = CN_MAX_PRED: a template parameter of the kernels (the parameters do not depend
// on it -- the decode is a recurrence -- and GP = 5 is the shipped predictor).  The order of the table is the field order of cn_gst_weights (include/crowdnav_hip.h).
#pragma once
#include "crowdnav_hip.h" // CN_MAX_PRED

#include <type_traits>

namespace gst_model {

constexpr int GT = 5;                         // observed steps
constexpr int GP_DEFAULT = 5, GP_MAX = CN_MAX_PRED; // predicted steps of the entry points without a horizon; the most
constexpr int seq_steps(int GP) { return GT + GP; }   // TT: steps of a sequence = columns of loss_mask_rel
constexpr int ncall(int GP) { return GT + GP - 1; }   // encoder-layer passes: 5 observed slices + GP - 1 decode steps
constexpr int nstep(int GP) { return GT + GP - 1; }   // LSTM steps
constexpr int NT = 256;                       // threads per workgroup
constexpr int NPARAM = 20;
constexpr int PSIZE[NPARAM] = {128, 64, 192 * 64, 192, 64 * 64, 64, 64, 64, 64, 64, 128 * 64, 128, 64 * 128, 64, 256 * 64, 256 * 64, 256, 256, 320, 5};
enum { P_EW = 0, P_EB, P_INW, P_INB, P_OW, P_OB, P_NW, P_NB, P_N1W, P_N1B, P_L1W, P_L1B, P_L2W, P_L2B, P_WIH, P_WHH, P_BIH, P_BHH, P_HW, P_HB };
constexpr int param_total()
{
    int s = 0;
    for (int i = 0; i < NPARAM; ++i) s += PSIZE[i];
    return s;
}
constexpr int NPARAMS = param_total(); // 67 269

struct Wts { const float *p[NPARAM]; };

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// fn(std::integral_constant<int, GP>) for the run-time horizon P in 1 .. GP_MAX (checked by the caller): picks the kernels' instantiation
template <int GP = GP_MAX, class F>
inline int for_horizon(int P, F &&fn)
{
    if constexpr (GP > 1) {
        if (P != GP) return for_horizon<GP - 1>(P, fn);
    }
    return fn(std::integral_constant<int, GP>{});
}

} // namespace gst_model
