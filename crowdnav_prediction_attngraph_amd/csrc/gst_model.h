// gst_model.h -- the GST predictor's shape constants and parameter table, shared by the training step (gst_train.hip) and the evaluation
// step (gst_eval.hip).  Shipped hyper-parameters: embedding 64, 8 heads, one NodeEncoderLayer without ghost / edge heads, LSTM 64,
// 5 observed + 5 predicted steps.  The order of the table is the field order of cn_gst_weights (include/crowdnav_hip.h).
#pragma once

namespace gst_model {

constexpr int GT = 5, GP = 5, TT = GT + GP;   // observed / predicted steps
constexpr int NCALL = GT + GP - 1;            // encoder-layer passes: 5 observed slices + 4 decode steps
constexpr int NSTEP = GT + GP - 1;            // LSTM steps
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

} // namespace gst_model
